"""Stage-2 models on the exported 256-d embeddings, discrete-hazard (nll) heads: drop-in for
models/nll_models_pretrained.py:13-197 of the reference (same class names -- including the reference's spelling
`unimonal_pretrained` --, constructor signatures, submodule trees and therefore state_dict keys).
All arithmetic runs in the HIP kernels behind include/mmf_amil.h (dense, batchnorm, highway mix, Kronecker fusion,
hazards)."""
from __future__ import annotations

import collections

import torch
import torch.nn as nn

from .. import ops
from ..utils.utils_pretrained import initialize_weights
from .model_modules import Highway, XlinearFusion, fcnn_block, step_grad_buffers, times_to_device


def _seed(training):
    return ops.next_dropout_seed() if training else 0


class unimonal_pretrained(nn.Module):
    """models/nll_models_pretrained.py:13-62."""

    def __init__(self, dropout=True, n_classes=4, mode=None, train_type=None, bag_loss=None, n_layers=1):
        super().__init__()
        self.n_classes = n_classes
        self.train_type = train_type
        self.bag_loss = bag_loss
        self.mode = mode
        if self.train_type == "fcnn":
            self.classifier = nn.Sequential(*[nn.Linear(256, n_classes), nn.Dropout(0.7)])
        elif self.train_type == "highway":
            self.highway = Highway(256, n_layers)
            self.classifier = nn.Linear(256, n_classes)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def forward(self, **kwargs):
        h = kwargs[{"path": "h_path", "radio": "h_radio", "omic": "h_omic"}[self.mode]]
        if self.train_type == "fcnn":
            lin, drop = self.classifier[0], self.classifier[1]
            p = drop.p if self.training else 0.0
            logits = ops.dense(h, lin.weight, lin.bias, drop_kind="dropout" if p > 0 else "none", drop_p=p,
                               seed=_seed(self.training), site=0)
        elif self.train_type == "highway":
            logits = ops.dense(self.highway(h), self.classifier.weight, self.classifier.bias)
        else:
            raise NotImplementedError(f"train_type {self.train_type!r}")     # 'residual' is commented out in the reference (:27-29)
        risk, hazards, S, _ = ops.hazards_from_logits(logits)
        return risk, hazards, S


def _pick(mode, h_radio, h_path, h_omic):
    """The modality order of the reference's cat / v_list (nll_models_pretrained.py:153-160, 164-171, 180-187):
    [radio, path] | [radio, omic] | [omic, path] | [radio, path, omic]."""
    r, p, o = "radio" in mode, "path" in mode, "omic" in mode
    if r and p and not o:
        return [h_radio, h_path]
    if r and o and not p:
        return [h_radio, h_omic]
    if o and p and not r:
        return [h_omic, h_path]
    if r and p and o:
        return [h_radio, h_path, h_omic]
    raise NotImplementedError(f"mode {mode!r}")


# what integrated_gradients returns: dicts by modality name ("radio", "path", "omic": the ones the mode keeps) of
# per-patient tensors [P]; attr: dict of [P x 256] or None; the risks [P]; step_risk [P x n_steps]; hazards, S [P x K] or None
Stage2Attribution = collections.namedtuple("Stage2Attribution", [
    "modality_attr", "modality_abs", "share", "attr", "risk", "risk_baseline", "delta", "step_risk", "hazards", "S"])


def _names(mode):
    """The present modalities in _pick's order."""
    return _pick(mode, "radio", "path", "omic")


def _bn_args(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def _highway_args(hw):
    pairs = lambda layers: [(l.weight, l.bias) for l in layers]
    return dict(bn1=_bn_args(hw.bn1), bn2=_bn_args(hw.bn2), gate=pairs(hw.gate), nonlinear=pairs(hw.nonlinear),
                linear=pairs(hw.linear))


def _fcnn_args(seq):
    d = dict(W0=seq[0].weight, b0=seq[0].bias, bn=_bn_args(seq[1]))
    if len(seq) > 4:
        d.update(W4=seq[4].weight, b4=seq[4].bias)
    return d


def stage2_ig_operands(model, family):
    """(blocks, Wk, bk, n_layers, xfusion weights or None) of a multimodal_pretrained for
    ops.stage2_integrated_gradients."""
    tt, names = model.train_type, _names(model.mode)
    late = {"radio": "MRI", "path": "WSI", "omic": "omic"}
    if tt == "early-fcnn":
        seq = model.classifier
        return [dict(W0=seq[0].weight, b0=seq[0].bias, bn=_bn_args(seq[1]))], seq[4].weight, seq[4].bias, 1, None
    if tt == "late-fcnn":
        cls = model.classifier[0]
        return [_fcnn_args(getattr(model, "layer_" + late[n])) for n in names], cls.weight, cls.bias, 1, None
    if tt == "early-highway":
        return [_highway_args(model.highway)], model.classifier.weight, model.classifier.bias, model.highway.num_layers, None
    if tt == "late-highway":
        hws = [getattr(model, "highway_" + n) for n in names]
        return [_highway_args(h) for h in hws], model.classifier.weight, model.classifier.bias, hws[0].num_layers, None
    if tt == "kronecker":
        xw = []
        for i in range(len(names)):
            for lin in (model.xfusion.reduce[i][0][0], model.xfusion.reduce[i][1][0], model.xfusion.reduce[i][2][0]):
                xw += [lin.weight, lin.bias]
        e1, e2 = model.xfusion.encoder1[0], model.xfusion.encoder2[0]
        return [], model.classifier.weight, model.classifier.bias, 1, xw + [e1.weight, e1.bias, e2.weight, e2.bias]
    raise NotImplementedError(f"integrated_gradients: train_type {tt!r}")


def stage2_integrated_gradients(model, family, h_radio, h_path, h_omic, n_steps, method, return_full):
    """integrated_gradients of both multimodal_pretrained classes: the refusals (train mode, non-fp32 or CPU-side shapes),
    the rule's nodes, the one fused call and the per-patient sums."""
    if model.training:
        raise RuntimeError("integrated_gradients is an eval-mode pass (dropout and batch statistics would make the "
                           "integrand depend on the cohort): call model.eval() first")
    names = _names(model.mode)
    given = dict(radio=h_radio, path=h_path, omic=h_omic)
    vs = [given[n] for n in names]
    if any(v is None for v in vs):
        raise ops._lib.MmfError(f"mode {model.mode!r} needs the embeddings {names}")
    if any(v.dtype != torch.float32 for v in vs):
        raise NotImplementedError("integrated_gradients takes fp32 embeddings")
    alphas, weights = ops.ig_quadrature(method, n_steps)
    blocks, Wk, bk, n_layers, xfusion = stage2_ig_operands(model, family)
    present = tuple(n in names for n in ("radio", "path", "omic"))
    with torch.no_grad():
        r = ops.stage2_integrated_gradients(family, model.train_type, present, vs, blocks, Wk, bk, alphas, weights,
                                            n_layers=n_layers, want_attr=return_full, xfusion=xfusion)
        m_attr = {n: r["mod_sum"][:, i] for i, n in enumerate(names)}
        m_abs = {n: r["mod_abs"][:, i] for i, n in enumerate(names)}
        tot_abs = r["mod_abs"].sum(1)
        share = {n: m_abs[n] / tot_abs for n in names}
        delta = r["mod_sum"].sum(1) - (r["risk"] - r["risk_base"])
    attr = dict(zip(names, r["attr"])) if return_full else None
    return Stage2Attribution(m_attr, m_abs, share, attr, r["risk"], r["risk_base"], delta, r["step_risk"], r["hazards"],
                             r["S"])


STEP_TYPES = ("early-fcnn", "late-fcnn", "early-highway", "late-highway")
STEP_MAX_ROWS = 256
# Where the one-call step did NOT beat the existing route on an MI355X (tools/stage2_step_bench.py, radio_path_omic,
# profiles/r18/stage2_step_bench.txt), step_ok says no -- early-highway only, whose 768-wide contractions run one thread
# per row:
#   forward only (eval mode: validation): 1.14 to 2.40 x the validation route at 32 to 128 rows, 0.80 to 1.02 x at 256;
#   training with n_layers >= 2 below 128 rows: 1.00 to 1.28 x the autograd route at 32 and 64 rows (nll B=32: 1.00,
#   nll B=64: 1.07, cox B=32: 1.28, cox B=64: 1.15), 0.48 to 0.84 x from 128 rows on.
STEP_EARLY_HIGHWAY_DEEP_MIN_ROWS = 128


def _step_loss(loss_fn, family):
    """The loss of a one-call step as ops.stage2_step takes it, or None: a class the loop does not dispatch, or one the
    family's head cannot feed (hazards are an nll-family output)."""
    from ..utils.loss_utils import CoxSurvLoss, NLLSurvLoss, RankingNLLSurvLoss, RankingSurvLoss
    if type(loss_fn) is CoxSurvLoss:
        return dict(kind="cox")
    if type(loss_fn) is RankingSurvLoss:
        spec = dict(kind="rank", phi=loss_fn.phi, reduction=loss_fn.reduction)
    elif family == "nll" and type(loss_fn) is NLLSurvLoss:
        return dict(kind="nll", alpha=loss_fn.alpha)
    elif family == "nll" and type(loss_fn) is RankingNLLSurvLoss:
        spec = dict(kind="rank_nll", phi=loss_fn.phi, reduction=loss_fn.reduction, alpha=loss_fn.alpha, nll_ratio=loss_fn.nll_ratio)
    else:
        return None
    return spec if spec["phi"] in ("sigmoid", "relu") and spec["reduction"] in ("mean", "sum") else None


def _step_blocks(model):
    """(modules, classifier) of a step: per block the dict of ops.stage2_step with nn.Parameters / buffers in it -- one
    block for the early types, the radio / path / omic blocks for the late ones -- and the BatchNorm modules it evaluates."""
    tt = model.train_type
    bn = lambda b: (b.weight, b.bias, b.running_mean, b.running_var, b.eps, 0.0 if b.momentum is None else b.momentum)
    pairs = lambda layers: [(l.weight, l.bias) for l in layers]

    def fcnn(seq):
        d = dict(W0=seq[0].weight, b0=seq[0].bias, bn=bn(seq[1]))
        if len(seq) > 4 and tt == "late-fcnn":
            d.update(W4=seq[4].weight, b4=seq[4].bias)
        return d, [seq[1]]

    def highway(hw):
        return dict(bn1=bn(hw.bn1), bn2=bn(hw.bn2), gate=pairs(hw.gate), nonlinear=pairs(hw.nonlinear),
                    linear=pairs(hw.linear)), [hw.bn1, hw.bn2]

    if tt == "early-fcnn":
        seq = model.classifier
        return [fcnn(seq)], seq[4]
    if tt == "late-fcnn":
        return [fcnn(getattr(model, "layer_" + n)) for n in ("MRI", "WSI", "omic")], model.classifier[0]
    if tt == "early-highway":
        return [highway(model.highway)], model.classifier
    return [highway(getattr(model, "highway_" + n)) for n in ("radio", "path", "omic")], model.classifier


def _block_params(b):
    """(parameter, path into the block's dict) of one block, in a fixed order."""
    out = []
    for k in ("W0", "b0", "W4", "b4"):
        if b.get(k) is not None:
            out.append((b[k], (k,)))
    for k in ("bn", "bn1", "bn2"):
        if k in b:
            out += [(b[k][0], (k, 0)), (b[k][1], (k, 1))]
    for k in ("gate", "nonlinear", "linear"):
        for l, (W, bias) in enumerate(b.get(k, ())):
            out += [(W, (k, l, 0)), (bias, (k, l, 1))]
    return out


def stage2_step_ok(model, family, h_radio, h_path, h_omic, loss_fn):
    """True when stage2_step can take this batch -- both multimodal_pretrained classes."""
    spec = _step_loss(loss_fn, family) if model.train_type in STEP_TYPES else None
    if spec is None:
        return False
    hs = (h_radio, h_path, h_omic)
    late = "late" in model.train_type
    read = [h for h, n in zip(hs, ("radio", "path", "omic")) if late or n in model.mode]
    if len(read) < 2 or any(not torch.is_tensor(h) or not h.is_cuda or h.dtype != torch.float32 or h.dim() != 2
                            or h.shape[1] != 256 for h in read):
        return False
    B = read[0].shape[0]
    if any(h.shape[0] != B for h in read) or not (2 if model.training else 1) <= B <= STEP_MAX_ROWS:
        return False
    if spec["kind"] in ("rank", "rank_nll") and B < 2:             # the reference raises: leave that to the existing route
        return False
    if model.train_type == "early-highway":                        # the measured exceptions, see STEP_EARLY_HIGHWAY_DEEP_MIN_ROWS
        if not model.training or (model.highway.num_layers >= 2 and B < STEP_EARLY_HIGHWAY_DEEP_MIN_ROWS):
            return False
    return all(p.requires_grad for p in model.parameters())


def stage2_step(model, family, h_radio, h_path, h_omic, loss_fn, label, event_time, c, loss_scale, grad_out, accumulate,
                backward):
    """step of both multimodal_pretrained classes: the operands, the gradient destinations, the one dropout draw, the one
    fused call, num_batches_tracked."""
    import numpy as np
    spec = _step_loss(loss_fn, family)
    if model.train_type not in STEP_TYPES or spec is None:
        raise NotImplementedError(f"step: train_type {model.train_type!r} with {type(loss_fn).__name__} (see step_ok)")
    blocks_bns, cls = _step_blocks(model)
    blocks = [b for b, _ in blocks_bns]
    late = "late" in model.train_type
    present = tuple(n in model.mode for n in ("radio", "path", "omic"))
    dev = h_path.device if h_path is not None else h_radio.device
    times = None
    if spec["kind"] in ("cox", "rank"):
        times = event_time
        if not (torch.is_tensor(times) and times.is_cuda and times.dtype == torch.float64):
            times = times_to_device(model, np.asarray(times.cpu() if torch.is_tensor(times) else times, dtype=np.float64), dev)
    grads = None
    if backward:
        # the parameters that take part, in a fixed order: the blocks the mode keeps, then the classifier
        live = []
        for i, b in enumerate(blocks):
            if not late or present[i]:
                live += [(p, (i,) + path) for p, path in _block_params(b)]
        live += [(cls.weight, ("dWk",)), (cls.bias, ("dbk",))]
        params = [p for p, _ in live]
        if grad_out is not None:
            where = {id(p): t for p, t in zip(model.parameters(), grad_out)}
            taken = {id(p) for p in params}
            if not accumulate:
                idle = [t for p, t in zip(model.parameters(), grad_out) if id(p) not in taken]
                if idle:
                    torch._foreach_zero_(idle)
            grad_out = [where[id(p)] for p in params]
        dst, accumulate = step_grad_buffers(params, dev, grad_out, accumulate)
        gblocks = [None if (late and not present[i]) else {} for i in range(len(blocks))]
        grads = dict(blocks=gblocks)
        for (p, path), t in zip(live, dst):
            if len(path) == 1:
                grads[path[0]] = t
                continue
            g, key = gblocks[path[0]], path[1]
            if len(path) == 2:
                g[key] = t
            elif len(path) == 3:
                g.setdefault(key, [None, None])[path[2]] = t
            else:
                lst = g.setdefault(key, [[None, None] for _ in blocks[path[0]][key]])
                lst[path[2]][path[3]] = t
    tr = model.training
    seed = ops.next_dropout_seed() if tr else 0
    n_layers = len(blocks[0]["gate"]) if "gate" in blocks[0] else 1
    drop = model.highway.dropout1 if model.train_type == "early-highway" else model.highway_radio.dropout1 \
        if model.train_type == "late-highway" else (model.classifier if model.train_type == "early-fcnn" else model.layer_MRI)[3]
    with torch.no_grad():
        out = ops.stage2_step(family, model.train_type, present, (h_radio, h_path, h_omic), blocks, cls.weight, cls.bias, spec,
                              Y=label, c=c, times=times, grads=grads, accumulate=bool(accumulate), loss_scale=loss_scale,
                              training=tr, n_layers=n_layers, p_drop=drop.p, seed=seed)
        if tr:
            tracked = [bn.num_batches_tracked for _, bns in blocks_bns for bn in bns if bn.num_batches_tracked is not None]
            if tracked:
                torch._foreach_add_(tracked, 1)
    return out


def late_branches(model, h_radio, h_path, h_omic, seed):
    """The late types' per-modality blocks (layer_MRI / layer_WSI / layer_omic, or the three Highways) on every embedding
    that is given, dropout sites 0, 1, 2: forward hands in all three, as the reference does (:144-151), even if the mode
    drops one; the captum_* methods leave that one out (None).  Shared by both families' multimodal_pretrained."""
    late = {"radio": "MRI", "path": "WSI", "omic": "omic"}
    out = []
    for site, (n, h) in enumerate((("radio", h_radio), ("path", h_path), ("omic", h_omic))):
        if h is None:
            out.append(None)
        elif model.train_type == "late-fcnn":
            out.append(fcnn_block(getattr(model, "layer_" + late[n]), h, seed or 0, site))
        else:
            out.append(getattr(model, "highway_" + n)(h, seed=None if seed is None else seed + site))
    return out


class multimodal_pretrained(nn.Module):
    """models/nll_models_pretrained.py:66-197."""

    def __init__(self, input_dim: int = 37, dropout=True, n_classes=4, mode="radio_path_omic", train_type=None,
                 bag_loss=None, n_layers=1):
        super().__init__()
        self.n_classes = n_classes
        self.mode = mode
        self.train_type = train_type
        self.bag_loss = bag_loss
        num_modalities = sum(k in mode for k in ("radio", "path", "omic"))
        if train_type == "early-fcnn":
            self.classifier = nn.Sequential(*[nn.Linear(num_modalities * 256, 128), nn.BatchNorm1d(128), nn.ReLU(),
                                              nn.Dropout(0.7), nn.Linear(128, n_classes)])
        elif train_type == "late-fcnn":
            self.layer_WSI = nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7)])
            self.layer_MRI = nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7)])
            self.layer_omic = nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7)])
            self.classifier = nn.Sequential(*[nn.Linear(num_modalities * 128, n_classes)])
        elif train_type == "early-highway":
            self.highway = Highway(num_modalities * 256, n_layers)
            self.classifier = nn.Linear(num_modalities * 256, n_classes)
        elif train_type == "late-highway":
            self.highway_radio = Highway(256, n_layers)
            self.highway_path = Highway(256, n_layers)
            self.highway_omic = Highway(256, n_layers)
            self.classifier = nn.Linear(num_modalities * 256, n_classes)
        elif train_type == "kronecker":
            self.xfusion = XlinearFusion(num_modalities=num_modalities, dropout_rate=0.7)
            self.classifier = nn.Linear(256, n_classes)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def _logits(self, h_radio, h_path, h_omic):
        seed = _seed(self.training) if self.training else None
        if "late" in self.train_type:
            r, p, o = late_branches(self, h_radio, h_path, h_omic, seed)
            mm = torch.cat(_pick(self.mode, r, p, o), dim=1)
            cls = self.classifier[0] if isinstance(self.classifier, nn.Sequential) else self.classifier
            return ops.dense(mm, cls.weight, cls.bias)
        if "early" in self.train_type:
            mm = torch.cat(_pick(self.mode, h_radio, h_path, h_omic), dim=1)
            if self.train_type == "early-fcnn":
                return fcnn_block(self.classifier, mm, seed or 0, 0)
            return ops.dense(self.highway(mm, seed=seed), self.classifier.weight, self.classifier.bias)
        if self.train_type == "kronecker":
            mm = self.xfusion(v_list=_pick(self.mode, h_radio, h_path, h_omic), seed=seed)
            return ops.dense(mm, self.classifier.weight, self.classifier.bias)
        raise NotImplementedError(f"train_type {self.train_type!r}")

    def forward(self, h_radio, h_path, h_omic):
        logits = self._logits(h_radio, h_path, h_omic)
        risk, hazards, S, _ = ops.hazards_from_logits(logits)
        return risk, hazards, S

    def step_ok(self, h_radio, h_path, h_omic, loss_fn):
        """True when step can take this batch: an fcnn or highway type, a loss class the loop dispatches, fp32 CUDA
        embeddings [B x 256] with B <= 256 (train mode: B >= 2), every parameter trainable -- and not one of the measured
        exceptions (early-highway in eval mode, or with two or more layers below 128 rows: STEP_EARLY_HIGHWAY_DEEP_MIN_ROWS).
        Otherwise callers keep to forward, the loss and .backward()."""
        return stage2_step_ok(self, "nll", h_radio, h_path, h_omic, loss_fn)

    def step(self, h_radio, h_path, h_omic, loss_fn, label=None, event_time=None, c=None, loss_scale=1.0, grad_out=None,
             accumulate=None, backward=True):
        """Extension of the reference surface (the training-loop mirror uses it with fused=True): `risk, hazards, S =
        model(h_radio, h_path, h_omic)`, the loss the loop would dispatch for loss_fn and `(loss * loss_scale).backward()` as
        ONE C-ABI call (ops.stage2_step), with the same dropout draw, the same running-statistics update and the same
        num_batches_tracked.  Gradients land in the parameters' .grad (accumulated; a late type's dropped modality keeps
        None) -- or in `grad_out` (tensors in self.parameters() order; overwritten unless `accumulate`).  backward=False:
        forward and loss only (validation).  Returns (risk [B], hazards, S, loss), detached; the loss is unscaled."""
        return stage2_step(self, "nll", h_radio, h_path, h_omic, loss_fn, label, event_time, c, loss_scale, grad_out,
                           accumulate, backward)

    # the methods captum is pointed at (models/nll_models_pretrained.py:200-320): the risk alone, as a function of the
    # embeddings the mode keeps, through the same autograd ops as forward
    def _risk(self, h_radio=None, h_path=None, h_omic=None):
        return ops.hazards_from_logits(self._logits(h_radio, h_path, h_omic))[0]

    def captum_radio_path(self, h_radio, h_path):
        return self._risk(h_radio=h_radio, h_path=h_path)

    def captum_path_omic(self, h_omic, h_path):
        return self._risk(h_path=h_path, h_omic=h_omic)

    def captum_radio_omic(self, h_radio, h_omic):
        return self._risk(h_radio=h_radio, h_omic=h_omic)

    def captum(self, h_radio, h_path, h_omic):
        return self._risk(h_radio, h_path, h_omic)

    def integrated_gradients(self, h_radio=None, h_path=None, h_omic=None, n_steps=20, method="gausslegendre",
                             return_full=False):
        """Integrated gradients of risk = -sum(S) with respect to the embeddings the mode keeps, from a zero baseline, for
        a cohort [P x 256] in ONE fused call (ops.stage2_integrated_gradients): create_attributions.py:93-164 for every
        patient at once.  Eval mode, fp32.  Returns a Stage2Attribution; modality_abs holds the columns of attr.csv,
        modality_attr those of attr_orig.csv."""
        return stage2_integrated_gradients(self, "nll", h_radio, h_path, h_omic, n_steps, method, return_full)
