"""Forward-only consumers of the path, on the MI355X kernels.

The reference runs three kinds of inference through the same heads:
  * embedding export for stage 2 -- `model(..., return_features=True)` per subject under `torch.no_grad()`
    (pre_trained_feature.py:116-162);
  * per-patient inference -- hazards, risk = -sum(S), raw attention scores (utils/heatmap_utils.py:249-275);
  * attention scoring of patch batches for heat-maps -- `_, _, _, A = model(path_features=features)` per batch of 512
    patch embeddings (utils/heatmap_utils.py:111-150).
Everything below is host plumbing around the drop-in heads; under `torch.no_grad()` in eval mode the heads take the
forward-only C-ABI entry points (include/mmf_amil.h: mmf_amil[_bf16]_infer), which save nothing for a backward.
File I/O (.pt / .h5), WSI handling and the image feature extractor stay with the caller: they are outside the path.
"""
from __future__ import annotations

import numpy as np
import torch

from .models import (MaxNet, MIL_Attention_fc_surv_path, MIL_Attention_fc_surv_radio, MM_MIL_Attention_fc_surv)


def _dev(model):
    return next(model.parameters()).device


def extract_features(model, **inputs) -> torch.Tensor:
    """One subject's pooled embedding, as pre_trained_feature.py:128,144,160 computes it:
    `model(**inputs, return_features=True)` in eval mode without autograd.  Returns a CPU tensor ([1 x 256] for the
    path / radio heads, [B x 256] for the omic head)."""
    dev = _dev(model)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inputs.items()}
            if isinstance(model, MaxNet) and "genomic_features" in kw:
                kw["genomic_features"] = kw["genomic_features"].float()          # pre_trained_feature.py:158
            feat = model(**kw, return_features=True)
        return feat.detach().cpu()
    finally:
        model.train(was_training)


class _ExportGroup:
    """extract_features_for_subjects(group=True): one head's bags held on the device for one grouped forward-only call
    (model.forward_group(..., return_features=True)); `entries` are the output slots the call fills."""

    def __init__(self, model):
        self.model, self.bags, self.entries, self.rows, self.limit = model, [], [], 0, None

    def takes(self, xs):
        """xs: the bag's tensors (one per modality), or None when the grouped pass does not take the bag.  Leaves the
        bag's row limit in self.limit, for full()."""
        from .utils.core_utils import _HeldBags
        if xs is None:
            return False
        self.limit = _HeldBags.row_limit(self.model, len(xs), int(xs[0].shape[1]), xs[0].dtype)
        return int(xs[0].shape[0]) <= self.limit and (not self.bags or self.bags[0][0].dtype == xs[0].dtype)

    def full(self, xs):
        """Whether what is held must run before the bag takes() just passed joins it."""
        from . import ops
        return bool(self.bags) and (len(self.bags) >= ops.GROUP_MAX or self.rows + int(xs[0].shape[0]) > self.limit
                                    or self.bags[0][0].dtype != xs[0].dtype)

    def add(self, xs, entry):
        dev = _dev(self.model)
        self.bags.append([x.to(dev) for x in xs])
        self.entries.append(entry)
        self.rows += int(xs[0].shape[0])

    def run(self):
        if not self.bags:
            return
        model = self.model
        was_training = model.training
        model.eval()
        try:
            if hasattr(model, "attention_net_radio"):
                bags = [dict(zip(model.modalities, b)) for b in self.bags]
            else:
                bags = [b[0] for b in self.bags]
            M = model.forward_group(bags, return_features=True).cpu()
        finally:
            model.train(was_training)
        for g, entry in enumerate(self.entries):
            entry[2] = M[g:g + 1]
        self.bags, self.entries, self.rows = [], [], 0


def extract_features_for_subjects(models: dict, subjects, skip=lambda subject_id, modality: False, group=False):
    """The export loop of pre_trained_feature.py:116-162 over an iterable of
    (subject_id, radio_features: dict, path_features, genomic_features) tuples.  `models` maps
    'path' / 'radio' / 'omic' to loaded heads (any subset).  A modality whose tensor is the reference's
    "missing" sentinel (`torch.zeros((1, 1))`, pre_trained_feature.py:122,135,153) is skipped.
    Yields (subject_id, modality, features_cpu).
    group=True: the path / radio bags of consecutive subjects are embedded by grouped forward-only calls
    (model.forward_group, up to ops.GROUP_MAX bags or the row limit each); the same items in the same order, each
    embedding what the per-subject call gives to fp32 rounding.  A bag the grouped pass does not take runs alone."""
    from .utils.core_utils import _eval_group_bags
    sentinel = torch.zeros((1, 1))

    def missing(t):
        return tuple(t.shape) == (1, 1) and torch.equal(t.detach().float().cpu(), sentinel)

    groups = {m: _ExportGroup(models[m]) for m in ("path", "radio") if group and m in models}
    pending = []                 # [subject_id, modality, features or None] in output order

    def drain():
        for g in groups.values():
            g.run()
        out = [tuple(e) for e in pending]
        pending.clear()
        return out

    def item(subject_id, modality, xs, compute):
        g = groups.get(modality)
        if g is None or not g.takes(xs):
            if not pending:
                return [(subject_id, modality, compute())]
            pending.append([subject_id, modality, compute()])
            return []
        out = drain() if g.full(xs) else []
        entry = [subject_id, modality, None]
        pending.append(entry)
        g.add(xs, entry)
        return out

    for subject_id, radio_features, path_features, genomic_features in subjects:
        if "path" in models and path_features is not None and not missing(path_features) and not skip(subject_id, "path"):
            xs = _eval_group_bags(models["path"], {}, path_features) if "path" in groups else None
            yield from item(subject_id, "path", xs, lambda: extract_features(models["path"], path_features=path_features))
        if ("radio" in models and radio_features and not all(missing(r) for r in radio_features.values())
                and not skip(subject_id, "radio")):
            xs = _eval_group_bags(models["radio"], radio_features, None) if "radio" in groups else None
            yield from item(subject_id, "radio", xs, lambda: extract_features(models["radio"], **radio_features))
        if "omic" in models and genomic_features is not None and not missing(genomic_features) and not skip(subject_id, "omic"):
            yield from item(subject_id, "omic", None,
                            lambda: extract_features(models["omic"], genomic_features=genomic_features))
    yield from drain()


def _no_grad_iter(it):
    """Items of a generator, each produced under torch.no_grad()."""
    it = iter(it)
    while True:
        with torch.no_grad():
            try:
                A = next(it)
            except StopIteration:
                return
        yield A


def infer_patient(model, features, bins=None, label=None, verbose=False):
    """utils/heatmap_utils.py:249-275: returns (Y_hat_model, risk, A_final) with risk = -sum(S) and A_final the raw
    (pre-softmax) attention scores as an [N x 1] numpy array.  `features` is the bag tensor for a path head and the
    dict of modality bags for a radio head, exactly as the reference passes them."""
    dev = _dev(model)
    with torch.no_grad():
        if isinstance(model, MIL_Attention_fc_surv_path):
            hazards, survival, Y_hat_model, A = model(path_features=features.to(dev))
        elif isinstance(model, MIL_Attention_fc_surv_radio):
            hazards, survival, Y_hat_model, A = model(**{k: v.to(dev) for k, v in features.items()})
        else:
            raise NotImplementedError            # as the reference (heatmap_utils.py:268-269)
        risk = -torch.sum(survival, dim=1).cpu().numpy()
        Y_hat = int(np.digitize(risk, np.array(bins))[0] - 1) if bins is not None else None
        A_final = A.view(-1, 1).cpu().numpy()
    Y_hat_model = Y_hat_model.cpu().numpy()[0][0]
    if verbose:
        print("Y_hat: {}, Y: {}, risk: {}, hazards: {}".format(
            Y_hat, label, risk, ["{:.4f}".format(p) for p in hazards.cpu().flatten()]))
    return Y_hat_model, risk, A_final


def _ig_autograd(model, inputs, alphas, weights, call):
    """The loop of both autograd routes over the tensors `inputs`; call(list of tensors) runs the model on them.  Returns
    ([attr per input], risk, risk_baseline, step_risk [n_steps]) on the device."""
    if model.training:
        raise RuntimeError("integrated gradients are an eval-mode pass: call model.eval() first")
    dev = _dev(model)
    xs = [x.to(dev).float() for x in inputs]
    acc = [torch.zeros_like(x) for x in xs]
    step_risk = []
    for a, w in zip(alphas, weights):
        xi = [(x * float(a)).requires_grad_() for x in xs]
        _, S, _, _ = call(xi)
        risk = -S.sum()
        gs = torch.autograd.grad(risk, xi)
        for t, g in zip(acc, gs):
            t.add_(g, alpha=float(w))
        step_risk.append(risk.detach())
    with torch.no_grad():
        risk_x = -call(xs)[1].sum()
        risk_base = -call([torch.zeros_like(x) for x in xs])[1].sum()
    return [t * x for t, x in zip(acc, xs)], risk_x, risk_base, torch.stack(step_risk)


def _attribute_in_eval(model, call, score, top_k):
    """call() -- the model's integrated_gradients -- with the model in eval mode for the call and restored; with top_k the
    pair (its result, indices of the top_k entries of score(result), largest first)."""
    was_training = model.training
    model.eval()
    try:
        out = call()
    finally:
        model.train(was_training)
    if top_k is None:
        return out
    s = score(out)
    return out, torch.topk(s, min(int(top_k), int(s.numel()))).indices


def integrated_gradients_autograd(model, bag, alphas, weights):
    """Integrated gradients of risk = -sum(S) from a zero baseline by the definition, one autograd pass per node: for each
    (alpha_k, w_k) `model(path_features=(alpha_k * bag).requires_grad_())`, the gradient of the risk with respect to that
    input, and attr = bag * sum_k w_k grad_k -- what captum's IntegratedGradients does around the reference's models
    (create_attributions.py:94-102), and the route to attributions without model.integrated_gradients: n_steps training-
    sized backward passes, weight gradients included.  The yardstick of the fused call (tools/ig_bench.py, the tests).
    Returns (patch_attr [N], patch_abs [N], attr [N x L], risk, risk_baseline, step_risk [n_steps]) on the device."""
    (attr,), *risks = _ig_autograd(model, [bag], alphas, weights, lambda xs: model(path_features=xs[0]))
    return (attr.sum(1), attr.abs().sum(1), attr, *risks)


def attribute_patches(model, bag, n_steps=20, method="gausslegendre", return_full=False, window_steps=0, top_k=None):
    """Patch attribution of one slide, create_attributions.py:94-102 for the pathology head: integrated gradients of the
    risk from a zero baseline in one fused call (model.integrated_gradients; `patch_abs` is the reference's per-patch
    sum |attr|).  The model is put in eval mode for the call and restored.  Returns the PatchAttribution, or with top_k the
    pair (PatchAttribution, indices of the top_k patches by patch_abs, largest first)."""
    if not isinstance(model, MIL_Attention_fc_surv_path):
        raise NotImplementedError("attribute_patches serves the pathology head")
    return _attribute_in_eval(model, lambda: model.integrated_gradients(
        bag.to(_dev(model)), n_steps=n_steps, method=method, return_full=return_full, window_steps=window_steps),
        lambda out: out.patch_abs, top_k)


def radio_integrated_gradients_autograd(model, bags, alphas, weights):
    """integrated_gradients_autograd for the radiology head: for each (alpha_k, w_k) one
    `model(**{m: (alpha_k * x_m).requires_grad_()})` pass, the gradient of risk = -sum(S) with respect to every modality,
    and attr_m = x_m * sum_k w_k grad_km -- what captum does around the reference's radiology branch
    (create_attributions.py:94-147), reduce_dim's and the stack's weight gradients included.  The yardstick of the fused
    call (tools/ig_bench.py --head radio, the tests).  Returns (inst_attr [n_mod x N], inst_abs [n_mod x N],
    attr [n_mod x N x k], risk, risk_baseline, step_risk [n_steps]) on the device, the modalities in model.modalities order."""
    mods = list(model.modalities)
    attrs, *risks = _ig_autograd(model, [bags[m] for m in mods], alphas, weights, lambda xs: model(**dict(zip(mods, xs))))
    attr = torch.stack(attrs)
    return (attr.sum(2), attr.abs().sum(2), attr, *risks)


def attribute_radiology(model, bags, n_steps=20, method="gausslegendre", return_full=False, top_k=None):
    """Attribution of one patient's MRI sequences, create_attributions.py:94-147 for the radiology head: integrated
    gradients of the risk from a zero baseline in one fused call (model.integrated_gradients; `modality_abs` is the
    reference's radio_attr per sequence, `inst_abs` per slice of each).  bags: {modality: [N x k]}.  The model is put in
    eval mode for the call and restored.  Returns the RadioAttribution, or with top_k the pair (RadioAttribution, indices
    of the top_k instances by sum_m inst_abs, largest first)."""
    if not isinstance(model, MIL_Attention_fc_surv_radio):
        raise NotImplementedError("attribute_radiology serves the radiology head")
    dev = _dev(model)
    return _attribute_in_eval(model, lambda: model.integrated_gradients(
        n_steps=n_steps, method=method, return_full=return_full, **{m: bags[m].to(dev) for m in model.modalities}),
        lambda out: out.inst_abs.sum(0), top_k)


def mm_integrated_gradients_autograd(model, features, alphas, weights):
    """integrated_gradients_autograd for the multimodal head: for each (alpha_k, w_k) one `model(**(alpha_k * every input))`
    pass, the gradient of risk = -sum(S) with respect to every input, and attr = input * sum_k w_k grad_k -- what captum
    does around the reference's multimodal model (create_attributions.py:93-164), every weight gradient included.  The
    yardstick of the fused call (tools/ig_bench.py --head mm, the tests).  features: what forward takes for model.mode.
    Returns ({"radio": [n_mod x N_r x k], "path": [N_p x L], "omic": [G]} for the branches of the mode, risk,
    risk_baseline, step_risk [n_steps]) on the device."""
    order = model._concat_order()
    names = ((list(model.modalities) if "radio" in order else []) + (["path_features"] if "path" in order else [])
             + (["genomic_features"] if "omic" in order else []))
    attrs, *risks = _ig_autograd(model, [features[k] for k in names], alphas, weights,
                                 lambda xs: model(**dict(zip(names, xs))))
    by_name = dict(zip(names, attrs))
    out = {}
    if "radio" in order:
        out["radio"] = torch.stack([by_name[m] for m in model.modalities])
    if "path" in order:
        out["path"] = by_name["path_features"]
    if "omic" in order:
        out["omic"] = by_name["genomic_features"].reshape(-1)
    return (out, *risks)


def attribute_modalities(model, features, n_steps=20, method="gausslegendre", return_full=False, top_k=None):
    """How much of one patient's predicted risk comes from radiology, pathology and omics, create_attributions.py:93-164:
    integrated gradients of the risk from a joint zero baseline in one fused call (model.integrated_gradients, or
    model.integrated_gradients_tensor for fusion='tensor'; `modality_abs` holds the reference's radio_attr, path_attr and
    omic_attr, `share` their fractions).  features: what forward takes for model.mode.  The model is put in eval mode for
    the call and restored.  Returns the
    ModalityAttribution, or with top_k the triple (ModalityAttribution, indices of the top_k patches by patch_abs, indices
    of the top_k slices by sum_m inst_abs), largest first, None for an absent branch."""
    from .models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    if not isinstance(model, MM_MIL_Attention_fc_surv):
        raise NotImplementedError("attribute_modalities serves the multimodal head")
    dev = _dev(model)
    feats = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in features.items()}
    call = model.integrated_gradients_tensor if model.fusion == "tensor" else model.integrated_gradients
    out = _attribute_in_eval(model, lambda: call(n_steps=n_steps, method=method, return_full=return_full, **feats), None, None)
    if top_k is None:
        return out
    top = lambda s: None if s is None else torch.topk(s, min(int(top_k), int(s.numel()))).indices
    return out, top(out.patch_abs), top(None if out.inst_abs is None else out.inst_abs.sum(0))


def _stage2_names(model):
    from .models.nll_models_pretrained import _names
    return _names(model.mode)


def stage2_integrated_gradients_autograd(model, h_radio, h_path, h_omic, alphas, weights):
    """Integrated gradients of a stage-2 multimodal_pretrained's risk by the definition: for each (alpha_k, w_k) one autograd
    pass of the captum method of the model's mode over alpha_k * the [P x 256] embeddings (in eval mode a row's risk
    depends on that row alone, so the gradient of sum_p risk_p is every patient's own), attr = embedding * sum_k w_k grad_k
    -- what captum does around the reference's models, one patient at a time (create_attributions.py:93-164), every
    weight gradient included.  The yardstick of the fused call (tools/ig_bench.py --head stage2, the tests).
    Returns ({name: attr [P x 256]} for the modalities the mode keeps, risk [P], risk_baseline [P], step_risk [P x n_steps])
    on the device."""
    if model.training:
        raise RuntimeError("integrated gradients are an eval-mode pass: call model.eval() first")
    names = _stage2_names(model)
    dev = _dev(model)
    given = dict(radio=h_radio, path=h_path, omic=h_omic)
    xs = [given[n].to(dev).float() for n in names]
    risk_of = lambda ts: model._risk(**{"h_" + n: t for n, t in zip(names, ts)}).reshape(-1)
    acc = [torch.zeros_like(x) for x in xs]
    step_risk = []
    for a, w in zip(alphas, weights):
        xi = [(x * float(a)).requires_grad_() for x in xs]
        risk = risk_of(xi)
        gs = torch.autograd.grad(risk.sum(), xi)
        for t, g in zip(acc, gs):
            t.add_(g, alpha=float(w))
        step_risk.append(risk.detach())
    with torch.no_grad():
        risk_x = risk_of(xs)
        risk_base = risk_of([torch.zeros_like(x) for x in xs])
    return {n: t * x for n, t, x in zip(names, acc, xs)}, risk_x, risk_base, torch.stack(step_risk, 1)


def attribute_embeddings(model, h_radio=None, h_path=None, h_omic=None, subject_ids=None, n_steps=20,
                         method="gausslegendre"):
    """The columns of the reference's attr.csv and attr_orig.csv for a cohort (create_attributions.py:93-175): integrated
    gradients of a stage-2 multimodal_pretrained's risk with respect to the [P x 256] embeddings of the modalities its mode
    keeps, from a zero baseline, in one fused call (model.integrated_gradients), reduced per modality to sum |attr| and
    sum attr.  subject_ids (a sequence of P ids): rows of one id are averaged, as the script's groupby('subject_id').mean()
    does over the splits, and the ids come back sorted.  The model is put in eval mode for the call and restored.
    Returns dict(attr={"radio_attr": array, ...}, attr_orig={...}, subject_id=array or None): float64 numpy arrays, one
    value per patient (or per distinct id), the present modalities only."""
    if not hasattr(model, "integrated_gradients") or not hasattr(model, "captum"):
        raise NotImplementedError("attribute_embeddings serves the stage-2 multimodal_pretrained models")
    dev = _dev(model)
    to = lambda h: None if h is None else h.to(dev)
    out = _attribute_in_eval(model, lambda: model.integrated_gradients(to(h_radio), to(h_path), to(h_omic), n_steps=n_steps,
                                                                       method=method), None, None)
    cols = {n + "_attr": out.modality_abs[n].double().cpu().numpy() for n in out.modality_abs}
    orig = {n + "_attr": out.modality_attr[n].double().cpu().numpy() for n in out.modality_attr}
    if subject_ids is None:
        return dict(attr=cols, attr_orig=orig, subject_id=None)
    ids = np.asarray(subject_ids)
    if ids.shape != next(iter(cols.values())).shape:
        raise ValueError(f"subject_ids: one id per patient expected, got {ids.shape}")
    uniq, inv = np.unique(ids, return_inverse=True)
    cnt = np.bincount(inv, minlength=len(uniq))
    mean = lambda v: np.bincount(inv, weights=v, minlength=len(uniq)) / cnt
    return dict(attr={k: mean(v) for k, v in cols.items()}, attr_orig={k: mean(v) for k, v in orig.items()}, subject_id=uniq)


# score_patch_batches(group=True): rows of one grouped scoring call per 256 hidden units.  Up to 128 projection tiles of 64 x
# 64 (2,048 rows of the `small` head, 1,024 of `big`) a window of fp32 batches keeps the projection plan of a 512-patch
# batch -- the same four-way K split, the same order of additions -- and with it every score bit for bit.
SCORE_GROUP_ROWS_PER_256 = 2048


def _scores_grouped(model, feature_batches, dev):
    """The per-batch scores of score_patch_batches, batch after batch, from grouped forward-only calls
    (ops.amil_infer_group) over consecutive batches.  The caller advances it under torch.no_grad() (_no_grad_iter)."""
    from . import ops
    from .models.model_modules import stack_args
    from .utils.core_utils import _eval_group_bags, _eval_group_head
    gated, stack, _, _ = stack_args(model.attention_net_WSI, False)
    cap = SCORE_GROUP_ROWS_PER_256 * 256 // model.attention_net_WSI[0].out_features
    held, rows = [], 0

    def run():
        x = torch.cat(held, 0) if len(held) > 1 else held[0]
        A = ops.amil_infer_group(x, [int(b.shape[0]) for b in held], stack, gated, want_M=True)[4]
        held.clear()
        return A

    kind = _eval_group_head(model)
    for features in feature_batches:
        # fp32 batches only: a bf16 batch's scores depend on which bf16 kernels run (fused or not), so it keeps its own call
        xs = _eval_group_bags(model, {}, features, kind) if kind and features.dtype == torch.float32 else None
        n = int(features.shape[0]) if torch.is_tensor(features) else 0
        if xs is None or n > cap:
            if held:
                yield from run()
            rows = 0
            yield model(path_features=features.to(dev), attention_only=True)
            continue
        if held and (len(held) >= ops.GROUP_MAX or rows + n > cap or held[0].dtype != features.dtype):
            yield from run()
            rows = 0
        held.append(features.to(dev))
        rows += n
    if held:
        yield from run()


def score_patch_batches(model, feature_batches, ref_scores=None, group=False):
    """Attention scoring of utils/heatmap_utils.py:129-141: for every batch of patch embeddings ([n x 1024], n <= 512
    in the reference) the raw attention scores of `model(path_features=features)`; optionally mapped to percentiles
    of `ref_scores` (score2percentile, heatmap_utils.py:32-34).  Batches are independent bags of the SAME head, so
    they are simply run back to back on the forward-only kernels; yields one [n x 1] float32 numpy array per batch.
    group=True: consecutive fp32 batches of the pathology head are scored by grouped forward-only calls of at most
    SCORE_GROUP_ROWS_PER_256 x 256 / H rows, which give the per-batch scores bit for bit; bf16 batches keep one call each."""
    dev = _dev(model)
    was_training = model.training
    model.eval()
    try:
        ref_sorted = np.sort(np.asarray(ref_scores).reshape(-1)) if ref_scores is not None else None
        if group and isinstance(model, MIL_Attention_fc_surv_path):
            scores = _scores_grouped(model, feature_batches, dev)
        else:
            scores = (model(path_features=features.to(dev), attention_only=True) for features in feature_batches)
        for A in _no_grad_iter(scores):
            A = A.view(-1, 1).cpu().numpy()
            if ref_sorted is not None:
                # scipy.stats.percentileofscore(ref, score) with the default kind='rank', vectorised
                lo = np.searchsorted(ref_sorted, A[:, 0], side="left")
                hi = np.searchsorted(ref_sorted, A[:, 0], side="right")
                A = ((lo + hi + (hi > lo)) * 50.0 / len(ref_sorted)).reshape(-1, 1).astype(A.dtype)
            yield A
    finally:
        model.train(was_training)
