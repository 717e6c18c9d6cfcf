"""Training / validation loops with the reference's call surface (utils/core_utils.py:173-264 and :267-355):
same signature, same per-bag order of operations (forward, loss, l1 regulariser added AFTER the /gc division,
backward, optimizer step every `gc` bags), same logged quantities.  The forward, loss and backward run in the
HIP kernels through the drop-in modules; this file is host control flow only.

Differences, all outside the arithmetic:
  * the c-index is computed with a small numpy restatement of sksurv's concordance_index_censored (sksurv is
    not a dependency of this package);
  * optional one-bag-per-GPU data parallelism (`dp=True` under torch.distributed): the loader is sharded by rank
    (feed.RankShard) and the flat gradient bucket is all-reduced once per optimizer step (see dp.py);
  * host synchronisation (`loss.item()`) is deferred to the end of the epoch instead of every bag.
"""
from __future__ import annotations

import numpy as np
import torch

from ..dp import FlatGradBuffer
from ..optim import FlatAdam
from .loss_utils import CoxSurvLoss, NLLSurvLoss


def concordance_index_censored(event_indicator, event_time, estimate, tied_tol=1e-8):
    """Harrell's c for right-censored data (sksurv.metrics.concordance_index_censored semantics):
    a pair (i, j) is comparable when the shorter time is an observed event; risk ties count 1/2."""
    e = np.asarray(event_indicator, dtype=bool)
    t = np.asarray(event_time, dtype=np.float64)
    r = np.asarray(estimate, dtype=np.float64)
    n = len(t)
    conc = disc = tied = 0.0
    for i in range(n):
        if not e[i]:
            continue
        later = (t > t[i]) | ((t == t[i]) & ~e)     # j outlived i (or was censored at the same time)
        later[i] = False
        d = r[i] - r[later]
        conc += float((d > tied_tol).sum())
        disc += float((d < -tied_tol).sum())
        tied += float((np.abs(d) <= tied_tol).sum())
    comparable = conc + disc + tied
    cindex = (conc + 0.5 * tied) / comparable if comparable > 0 else float("nan")
    return cindex, conc, disc, tied, 0


def _to_device(radio_features, path_features, genomic_features, label, c, device):
    feats = {i: r.to(device, non_blocking=True) for i, r in radio_features.items()}
    feats["path_features"] = path_features.to(device, non_blocking=True)
    feats["genomic_features"] = genomic_features.to(device, non_blocking=True).float()
    return feats, label.to(device), c.to(device)


def _is_sentinel(t):
    """The dataset marks a missing modality with zeros((1, 1)) (utils/core_utils.py:185-192 of the reference).
    Shape is checked first so that real bags (possibly already on the GPU via feed.DevicePrefetcher) cost no sync."""
    return tuple(t.shape) == (1, 1) and not bool(t.any())


def _skip(mode, radio_features, path_features, genomic_features):
    if "omic" in mode and _is_sentinel(genomic_features):
        return True
    if "path" in mode and _is_sentinel(path_features):
        return True
    if "radio" in mode and all(_is_sentinel(r) for r in radio_features.values()):
        return True
    return False


def _fused_step_ok(model, loss_fn, feats):
    """One bag = one C-ABI call (model.nll_step).  Only where that is exactly what `model(**feats)` + the stock loss would
    compute: the pathology head ITSELF (a subclass that overrides forward(), or any module / global hook, would be bypassed
    by a graph-free step -- those take the autograd path), the stock NLLSurvLoss, one 2-D fp32 / bf16 bag on the GPU, a
    classifier the kernel's single-workgroup tail holds (<= 32 classes), every parameter trainable."""
    from ..models.model_attention_mil_path import MIL_Attention_fc_surv_path
    import torch.nn.modules.module as tm
    x = feats.get("path_features")
    if not (type(loss_fn) is NLLSurvLoss and torch.is_tensor(x) and x.dim() == 2 and x.is_cuda
            and x.dtype in (torch.float32, torch.bfloat16)):
        return False
    if type(model).forward is not MIL_Attention_fc_surv_path.forward or not hasattr(model, "nll_step"):
        return False
    if getattr(getattr(model, "classifier", None), "out_features", 1 << 30) > 32:
        return False
    hooked = lambda m: bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None))
    if any(hooked(m) for m in model.modules()):
        return False
    if tm._global_forward_hooks or tm._global_forward_pre_hooks or tm._global_backward_hooks or getattr(tm, "_global_backward_pre_hooks", None):
        return False
    return all(p.requires_grad for p in model.parameters())


class _Window:
    """Gradient accumulation window of `train_loop_survival`, kept on the optimizer object between calls because the
    reference's accumulated gradients survive the end of an epoch (a trailing partial window is NOT stepped and NOT
    cleared, utils/core_utils.py:245-247: its gradients join the first window of the next epoch).

    Three ways to hold the window's gradient, one interface:
      fused   FlatAdam: p.grad are views of its flat bucket [n grads | 2 control words];
      buffer  any torch optimizer + dp.FlatGradBuffer (made here when world > 1): same bucket layout;
      plain   any torch optimizer, world == 1: p.grad as autograd leaves them.
    With `inflight` > 1 (fused only) the bags run on side streams into per-stream slots (pipeline.BagsInFlight) that
    are folded into the bucket at every boundary and at the end of the epoch."""

    def __init__(self, model, optimizer, world, grad_buffer, inflight, device):
        self.opt, self.world = optimizer, world
        self.fused = isinstance(optimizer, FlatAdam)
        self.buf = None if self.fused else grad_buffer
        if world > 1 and not self.fused and self.buf is None:
            self.buf = FlatGradBuffer(model)
        self.pipe = None
        if inflight > 1:
            if not self.fused:
                raise ValueError("inflight > 1 needs the FlatAdam optimizer (flat gradient buffer)")
            from ..pipeline import BagsInFlight
            self.pipe = BagsInFlight(model, inflight, device)
        self.kept = 0            # bags that contributed since the last optimizer step (this rank)

    @property
    def bucket(self):
        return self.opt.bucket if self.fused else (self.buf.bucket if self.buf is not None else None)

    def fold(self):
        """Side-stream slots -> the flat bucket (also called at the end of an epoch so that nothing is left in flight)."""
        if self.pipe is not None and any(self.pipe._used):
            self.opt.flat_g.add_(self.pipe.reduce(all_reduce=False))

    def boundary(self, last_bag_ran):
        """A window's last loader position has been passed.  The reference steps there only when that bag was not
        skipped (its `continue` jumps over the step, so the gradients stay and the window merges with the next one).
        world > 1: ONE all-reduce of [grads | ran-flag | kept-count]; every rank takes the same decision from the
        reduced control words (`last_bag_ran` is known to the rank that owns the window's last position only)."""
        self.fold()
        ran, kept = bool(last_bag_ran), self.kept
        if self.world > 1:
            tail = self.bucket[-2:]
            tail[0] += 1.0 if last_bag_ran else 0.0
            tail[1] += float(self.kept)
            (self.opt if self.fused else self.buf).all_reduce()
            flag, total = self.bucket[-2:].tolist()         # host sync, once per optimizer step
            ran, kept = flag > 0.5, int(round(total))
            if not ran:
                # no step: the window stays open.  The reduced sum now sits on every rank; keep it on rank 0 only so
                # that the next all-reduce counts it once.
                if torch.distributed.get_rank() != 0:
                    self.bucket.zero_()
                self.kept = 0
                if self.pipe is not None:
                    self.pipe.release()
                return False
        if not ran:
            return False
        if self.fused:
            self.opt.step(l1_micro_batches=kept)
            self.opt.zero_grad()
        else:
            self.opt.step()
            if self.buf is not None:
                self.buf.zero()
            else:
                self.opt.zero_grad()
        self.kept = 0
        if self.pipe is not None:
            self.pipe.release()
        return True


class _HeldBags:
    """The bags a grouped call will take, held on the device until it runs (_BagGroup: a training window's; _EvalGroup: an
    evaluation pass's).  Each bag is copied straight into its rows of one reusable device buffer [n_mod x rows x L] (no
    concatenation pass; fp32, or bf16 pathology bags in an evaluation pass): the pathology head's bag is one [n x L]
    tensor, the radiology head's one per modality.  A bag that would take the group past ops.GROUP_MAX bags or the row
    limit, or one of the other storage type, flushes what is held first (the window then runs as several grouped calls).
    A bag that feed.ResidentBagCache keeps in HBM (it carries `_mmf_resident`) is held BY REFERENCE instead -- its arena view,
    no copy -- and reaches its rows when the grouped call is about to run: ONE ops.bag_gather for all planes of a window of
    resident bags (one per run of consecutive resident bags when a window mixes both kinds), which also widens the bags of a
    bf16-stored cache."""

    def __init__(self):
        self.buf = None
        self.reset()

    def reset(self):
        self.rows, self.sizes, self.labels, self.cs, self.seeds, self.slots = 0, [], [], [], [], []
        self.refs = []       # (first row, rows, [arena view per modality]) of the bags held by reference

    @staticmethod
    def resident_source(x, device):
        """The arena view behind a bag feed.ResidentBagCache delivered (the bag itself, or what it was widened from), or
        None: any other tensor, which is copied as it arrives."""
        r = getattr(x, "_mmf_resident", None)
        if r is None:
            return None
        src = x if r is True else r
        return src if src.device == device and src.dim() == 2 and src.shape[1] % 8 == 0 and src.is_contiguous() else None

    def materialise(self):
        """The bags held by reference, into their rows of the buffer."""
        from .. import ops
        refs, self.refs = self.refs, []
        i = 0
        while i < len(refs):
            j = i + 1
            while j < len(refs) and refs[j][0] == refs[j - 1][0] + refs[j - 1][1] and refs[j][2][0].dtype == refs[i][2][0].dtype:
                j += 1
            r0 = refs[i][0]
            ops.bag_gather([[ref[2][m] for ref in refs[i:j]] for m in range(self.buf.shape[0])],
                           [self.buf[m, r0:] for m in range(self.buf.shape[0])])
            i = j

    @staticmethod
    def row_limit(model, nmod, L, dtype=torch.float32):
        """Most rows of one grouped call (an fp32 window's are the same forward-only and in training)."""
        from .. import ops
        seq = model.attention_net_radio if hasattr(model, "attention_net_radio") else model.attention_net_WSI
        H, D = seq[0].out_features, seq[3].stack_params()[0].shape[0]
        if nmod > 1:
            return ops.radio_infer_group_row_limit(nmod, L, H, D)
        return ops.infer_group_row_limit(L, H, D, bf16=dtype == torch.bfloat16)

    @staticmethod
    def limit_of(model, xs, cache):
        """row_limit for the bag xs, memoised in `cache` (a dict the pass keeps) by modality count, width and dtype."""
        key = (len(xs), int(xs[0].shape[1]), xs[0].dtype)
        if key not in cache:
            cache[key] = _HeldBags.row_limit(model, *key)
        return cache[key]

    def add(self, xs, label, c, slot, limit, device, flush, seed=0):
        """xs: the bag's [n x L] tensors, one per modality (the pathology head: one); label, c: device tensors; seed: its
        dropout seed in a training window."""
        from .. import ops
        nmod, n, L, dtype = len(xs), int(xs[0].shape[0]), int(xs[0].shape[1]), xs[0].dtype
        if device.type == "cuda" and device.index is None:        # compare with the buffer's device, which has its index
            device = torch.device("cuda", torch.cuda.current_device())
        if self.sizes and (len(self.sizes) >= ops.GROUP_MAX or self.rows + n > limit or self.buf.dtype != dtype):
            flush()
        need = self.rows + n
        if (self.buf is None or self.buf.shape[0] != nmod or self.buf.shape[2] != L or self.buf.shape[1] < need
                or self.buf.dtype != dtype or self.buf.device != device):
            grown = torch.empty((nmod, max(need, 2 * self.buf.shape[1] if self.buf is not None else need), L),
                                dtype=dtype, device=device)
            if self.rows and len(self.refs) < len(self.sizes):       # some held bag is in the buffer already
                grown[:, :self.rows].copy_(self.buf[:, :self.rows])
            self.buf = grown
        srcs = [self.resident_source(x, device) for x in xs]
        if all(src is not None for src in srcs):
            self.refs.append((self.rows, n, srcs))
        else:
            for m, x in enumerate(xs):
                self.buf[m, self.rows:need].copy_(x, non_blocking=True)
        self.rows = need
        self.sizes.append(n); self.labels.append(label.reshape(1)); self.cs.append(c.reshape(1))
        self.seeds.append(seed); self.slots.append(slot)

    def held(self, model):
        """The held rows as the model's grouped calls take them: (x or [n_mod x rows x L], sizes)."""
        self.materialise()
        x = self.buf[:, :self.rows] if hasattr(model, "attention_net_radio") else self.buf[0, :self.rows]
        return x, list(self.sizes)


class _BagGroup(_HeldBags):
    """train_loop_survival(group=True): the eligible bags of the current window, until one grouped call
    (model.nll_step_group) runs them.  A bag's dropout seed is drawn when it arrives, so bag g of the loader gets the
    masks the per-bag route gives it.  fp32 only, by what the loop feeds it."""

    def run(self, model, alpha, loss_scale):
        """One grouped call over the held bags -> [(loader slot, loss [1], risk [1])]; the group is empty afterwards."""
        if not self.sizes:
            return []
        seeds = self.seeds if model.training else None
        _, _, _, _, loss, risk = model.nll_step_group(self.held(model), torch.cat(self.labels), torch.cat(self.cs),
                                                      alpha=alpha, loss_scale=loss_scale, seeds=seeds)
        out = [(slot, loss[g:g + 1], risk[g:g + 1]) for g, slot in enumerate(self.slots)]
        self.reset()
        return out


def _group_tensor(model):
    """The tensor fusion on the grouped route: a per-instance opt-in (model.mmf_group_tensor = True; absent means off),
    like mmf_one_call_step / mmf_side_stream / mmf_fork_min_one_call."""
    return (getattr(model, "fusion", None) == "tensor" and bool(getattr(model, "mmf_group_tensor", False))
            and hasattr(model, "nll_step_group_tensor"))


class _MMGroup:
    """train_loop_survival(group=True) with the multimodal head: the eligible patients of the current window, until
    one grouped call (MM_MIL_Attention_fc_surv.nll_step_group; nll_step_group_tensor for a tensor-fusion model that opted
    in) runs them.  A patient's bags are copied straight into their
    rows of three reusable device buffers -- the pathology plane [1 x rows x L], the radio planes [n_mod x rows x L] and the
    omic rows [GROUP_MAX x input_dim] -- and its up to three dropout seeds are drawn when it arrives, in nll_step's order
    (radio, path, omic; then the fusion seed of the tensor fusion), so patient g of the loader gets the masks the per-patient
    route gives it.  A patient that would
    take the group past ops.GROUP_MAX or past either branch's row limit flushes what is held first."""

    def __init__(self):
        self.path, self.radio, self.omic = _HeldBags(), _HeldBags(), None
        self.limits = {}
        self.reset()

    def reset(self):
        self.path.reset()
        self.radio.reset()
        self.labels, self.cs, self.slots = [], [], []
        self.seeds = {"radio": [], "path": [], "omic": []}

    def row_limits(self, model, L_path, L_radio):
        """(pathology, radio) row limits of one grouped call (ops.mm_group_row_limits), memoised by the bags' widths."""
        from .. import ops
        key = (L_path, L_radio)
        if key not in self.limits:
            dims = lambda seq: (seq[0].out_features, seq[3].stack_params()[0].shape[0])
            self.limits[key] = ops.mm_group_row_limits(
                path=None if L_path is None else (L_path, *dims(model.attention_net_WSI)),
                radio=None if L_radio is None else (len(model.modalities), L_radio, *dims(model.attention_net_radio)))
        return self.limits[key]

    def add(self, model, radio_features, path_features, genomic_features, label, c, slot, device, flush):
        """One patient (host or device tensors; label, c: device tensors) of loader slot `slot`."""
        from .. import ops
        has = lambda k: k in model.mode
        xs_r = [radio_features[m] for m in model.modalities] if has("radio") else None
        n_p = int(path_features.shape[0]) if has("path") else 0
        n_r = int(xs_r[0].shape[0]) if has("radio") else 0
        lim_p, lim_r = self.row_limits(model, int(path_features.shape[1]) if has("path") else None,
                                       int(xs_r[0].shape[1]) if has("radio") else None)
        if self.slots and (len(self.slots) >= ops.GROUP_MAX or has("path") and self.path.rows + n_p > lim_p
                           or has("radio") and self.radio.rows + n_r > lim_r):
            flush()
        for k in ("radio", "path", "omic"):
            if has(k):
                self.seeds[k].append(ops.next_dropout_seed() if model.training else 0)
        if _group_tensor(model):               # nll_step draws the fusion seed after the branches'
            self.seeds.setdefault("fusion", []).append(ops.next_dropout_seed() if model.training else 0)
        never = lambda: None                   # the flush above has made room in both planes
        if has("radio"):
            self.radio.add(xs_r, label, c, slot, lim_r, device, never)
        if has("path"):
            self.path.add([path_features], label, c, slot, lim_p, device, never)
        if has("omic"):
            x = genomic_features.reshape(-1)
            if self.omic is None or self.omic.shape[1] != x.numel() or self.omic.device != label.device:
                self.omic = torch.empty((ops.GROUP_MAX, x.numel()), dtype=torch.float32, device=label.device)
            self.omic[len(self.slots)].copy_(x, non_blocking=True)
        self.labels.append(label.reshape(1)); self.cs.append(c.reshape(1)); self.slots.append(slot)

    def window(self, model):
        """The held patients as the model's grouped calls take them: the pre-stacked (path, radio, omic) triple."""
        has = lambda k: k in model.mode
        self.path.materialise()
        self.radio.materialise()
        return ((self.path.buf[0, :self.path.rows], list(self.path.sizes)) if has("path") else None,
                (self.radio.buf[:, :self.radio.rows], list(self.radio.sizes)) if has("radio") else None,
                self.omic[:len(self.slots)] if has("omic") else None)

    def run(self, model, alpha, loss_scale):
        """One grouped call over the held patients -> [(loader slot, loss [1], risk [1])]; the group is empty afterwards."""
        if not self.slots:
            return []
        has = lambda k: k in model.mode
        seeds = {k: v for k, v in self.seeds.items() if has(k)} if model.training else None
        step = model.nll_step_group
        if _group_tensor(model):
            step = model.nll_step_group_tensor
            if seeds is not None:
                seeds["fusion"] = self.seeds["fusion"]
        _, _, _, _, loss, risk = step(self.window(model), torch.cat(self.labels), torch.cat(self.cs), alpha=alpha,
                                      loss_scale=loss_scale, seeds=seeds)
        out = [(slot, loss[g:g + 1], risk[g:g + 1]) for g, slot in enumerate(self.slots)]
        self.reset()
        return out


def _window_of(model, optimizer, world, grad_buffer, inflight, device):
    key = (world, inflight, id(model))
    w = getattr(optimizer, "_mmf_window", None)
    if w is None or getattr(w, "key", None) != key:
        w = _Window(model, optimizer, world, grad_buffer, inflight, device)
        w.key = key
        try:
            optimizer._mmf_window = w
        except AttributeError:
            pass
    return w


def _fused_cox_ok(model, loss_fn, feats):
    """One omic batch = one launch (model.cox_step: MaxNet forward + CoxSurvLoss + backward).  Only where that is exactly what
    `model(**feats)` + the stock loss would compute: MaxNet ITSELF with a Cox head, the stock CoxSurvLoss, no hooks."""
    from ..models.model_genomic import MaxNet
    import torch.nn.modules.module as tm
    x = feats.get("genomic_features")
    if type(loss_fn) is not CoxSurvLoss or type(model).forward is not MaxNet.forward or not hasattr(model, "cox_step"):
        return False
    hooked = lambda m: bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None))
    if any(hooked(m) for m in model.modules()):
        return False
    if tm._global_forward_hooks or tm._global_forward_pre_hooks or tm._global_backward_hooks or getattr(tm, "_global_backward_pre_hooks", None):
        return False
    return x is not None and x.dtype == torch.float32 and model.cox_step_ok(x)


def _fused_radio_ok(model, loss_fn, feats, on_host=False):
    """The radiology head's step without an autograd graph (model.nll_step: reduce_dim, then stack + head + loss + backward
    in one call, then reduce_dim's backward).  Only where that is exactly what `model(**feats)` + the stock loss would
    compute: MIL_Attention_fc_surv_radio ITSELF, the stock NLLSurvLoss, fp32 2-D modality bags of one shape on the GPU, no
    hooks, every parameter trainable.  on_host: the bags may still be on the host (group=True asks before the copy)."""
    from ..models.model_attention_mil_radio import MIL_Attention_fc_surv_radio
    import torch.nn.modules.module as tm
    if type(loss_fn) is not NLLSurvLoss or type(model).forward is not MIL_Attention_fc_surv_radio.forward:
        return False
    if not getattr(model, "mmf_one_call_step", True) or getattr(model.classifier, "out_features", 1 << 30) > 32:
        return False
    bags = [feats.get(m) for m in model.modalities]
    if any(not (torch.is_tensor(b) and (b.is_cuda or on_host) and b.dim() == 2 and b.dtype == torch.float32) for b in bags):
        return False
    if any(b.shape != bags[0].shape for b in bags):
        return False
    hooked = lambda m: bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None))
    if any(hooked(m) for m in model.modules()):
        return False
    if tm._global_forward_hooks or tm._global_forward_pre_hooks or tm._global_backward_hooks or getattr(tm, "_global_backward_pre_hooks", None):
        return False
    return all(p.requires_grad for p in model.parameters())


def _fused_mm_ok(model, loss_fn, feats, on_host=False):
    """One patient = one fixed sequence of C-ABI calls without an autograd graph (model.nll_step of the multimodal concat
    head).  Only where that is exactly what `model(**feats)` + the stock loss would compute: MM_MIL_Attention_fc_surv ITSELF
    (concat fusion, or the tensor fusion as the heads configure it), the stock NLLSurvLoss, no hooks, every parameter trainable, inputs on the GPU.
    on_host: the inputs may still be on the host (group=True asks before the copy)."""
    from ..models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    import torch.nn.modules.module as tm
    if type(loss_fn) is not NLLSurvLoss or type(model).forward is not MM_MIL_Attention_fc_surv.forward:
        return False
    if not getattr(model, "mmf_one_call_step", True):
        return False
    fusion = getattr(model, "fusion", None)
    if fusion == "concat":
        head = model.classifier
    elif fusion == "tensor":
        head = model.classifier[3]
        if not (model.mm.skip and len(model._concat_order()) * model.mm.reduce[0][0][0].weight.shape[0] <= 384):
            return False
    else:
        return False
    if head.out_features > 32:
        return False
    for v in feats.values():
        if not (torch.is_tensor(v) and (v.is_cuda or on_host)):
            return False
    hooked = lambda m: bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None))
    if any(hooked(m) for m in model.modules()):
        return False
    if tm._global_forward_hooks or tm._global_forward_pre_hooks or tm._global_backward_hooks or getattr(tm, "_global_backward_pre_hooks", None):
        return False
    return all(p.requires_grad for p in model.parameters())


def _mm_group_ok(model, loss_fn, radio_features, path_features, genomic_features):
    """A multimodal patient the window's grouped call takes (model.nll_step_group): what _fused_mm_ok allows (asked on the
    tensors as the loader delivers them, host or device), the concat fusion -- or the tensor fusion with scale width 16 on a
    model that opted in (model.mmf_group_tensor = True: nll_step_group_tensor) --, and for every branch in model.mode a
    2-D fp32 bag (the modalities of one shape) or an omic vector of the model's input width."""
    if _group_tensor(model):
        if model.mm.reduce[0][0][0].weight.shape[0] != 16:
            return False
    elif getattr(model, "fusion", None) != "concat" or not hasattr(model, "nll_step_group"):
        return False
    feats = dict(radio_features, path_features=path_features, genomic_features=genomic_features)
    if not _fused_mm_ok(model, loss_fn, feats, on_host=True):
        return False
    bag = lambda t: t.dim() == 2 and t.dtype == torch.float32 and t.shape[0] >= 1
    if "path" in model.mode and not bag(path_features):
        return False
    if "radio" in model.mode:
        xs = [radio_features.get(m) for m in model.modalities]
        if any(x is None or not bag(x) or x.shape != xs[0].shape for x in xs):
            return False
    if "omic" in model.mode and genomic_features.numel() != model.fc_omic[0][0].in_features:
        return False
    return True


def train_loop_survival(epoch, model, loader, optimizer, n_classes, mode, writer=None, loss_fn=None, reg_fn=None,
                        lambda_reg=0., gc=16, t_bin=None, dp=False, grad_buffer=None, inflight=1, group=False):
    """utils/core_utils.py:173-264: same per-bag order (forward, loss, regulariser added AFTER the /gc division,
    backward), and the same window rule -- the optimizer steps after loader position b when (b + 1) % gc == 0 and bag b
    was not skipped; skipped bags (missing modality) contribute nothing but still occupy their position.

    Extras, all off by default:
      dp        one bag per rank (torch.distributed initialised): rank r takes loader positions r, r + world, ...
                (feed.RankShard: only those bags are loaded); the window is gc x world positions and ends with ONE
                all-reduce (SUM) of the flat gradient bucket -- the reference's `--gc gc*world`, see dp.py.  Every rank
                issues exactly one collective per window boundary, whatever it skipped;
      FlatAdam  fused L1 + Adam tail (optim.py); reg_fn must then be l1_reg_all, or l1_reg_modules with a FlatAdam
                built with the matching `l1_modules`;
      inflight  > 1 (needs FlatAdam): the window's bags run round-robin on that many HIP streams (pipeline.py);
      group     the pathology and radiology heads' fp32 bags (those their one-call steps take, exact-fp32 GEMMs) are held
                on the device as they arrive and run as ONE grouped call per window (model.nll_step_group: one launch chain over their
                concatenated rows), issued before the window's boundary and, for a trailing partial window, at the end
                of the epoch; more than ops.GROUP_MAX bags or the row limit split it into several calls.  Each bag's
                dropout seed is drawn when it arrives; a bag the grouped call does not take flushes the group and runs
                alone.  Losses and risks are logged in loader order as before.  Not with inflight > 1 or dp on several
                ranks.  The multimodal concat head's patients (those its one-call step takes, fp32 bags) are held in the same
                way -- a pathology plane, the radio planes and the omic rows -- and run as ONE nll_step_group per window;
                the tensor fusion keeps the per-patient route."""
    from ..feed import RankShard
    from .utils import l1_reg_all, l1_reg_modules
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.train()
    world, rank = 1, 0
    if dp and torch.distributed.is_available() and torch.distributed.is_initialized():
        world, rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
    if group and inflight > 1:
        raise ValueError("group=True runs a window as one grouped call: not together with inflight > 1")
    if group and world > 1:
        raise ValueError("group=True is single-GPU for now: not together with dp on several ranks")
    win = _window_of(model, optimizer, world, grad_buffer, inflight, device)
    fused_tail, pipe = win.fused, win.pipe
    if fused_tail:
        if reg_fn is not None and lambda_reg:
            want_mask = reg_fn is l1_reg_modules
            if reg_fn not in (l1_reg_all, l1_reg_modules) or want_mask != (optimizer.l1_mask is not None):
                raise ValueError("FlatAdam applies the L1 term inside its kernel: reg_fn must be l1_reg_all, or "
                                 "l1_reg_modules with FlatAdam(l1_modules=[model.fc_omic, model.mm])")
        optimizer.lambda_l1 = lambda_reg if reg_fn is not None else 0.0      # before the first l1_value() / step
    G = gc * world
    shard = RankShard(loader, rank, world) if world > 1 else None
    n_total = shard.n_total if shard is not None else None
    losses, regs, all_risk, all_c, all_t = [], [], [], [], []
    n_pos = 0
    held = None
    if group:
        from .. import ops
        held = getattr(win, "group", None)
        if held is None:
            held = win.group = _MMGroup() if hasattr(model, "attention_net_radio") and hasattr(model, "attention_net_WSI") \
                else _BagGroup()
        alpha_g = getattr(loss_fn, "alpha", 0.0)

        def flush():      # the held bags' losses / risks land in their loader slots
            for slot, loss_g, risk_g in held.run(model, alpha_g, 1.0 / G):
                losses[slot] = loss_g.reshape(())
                all_risk[slot] = risk_g.reshape(-1)
    for i, batch in enumerate(shard if shard is not None else loader):
        radio_features, path_features, genomic_features, label, event_time, c = batch
        pos = shard.position(i) if shard is not None else i
        n_pos += 1
        skipped = _skip(mode, radio_features, path_features, genomic_features)
        if not skipped:
            if isinstance(loss_fn, NLLSurvLoss) and torch.is_tensor(label) and not label.is_cuda and label.numel() \
                    and (int(label.min()) < 0 or int(label.max()) >= n_classes):
                # the reference's gather (utils/loss_utils.py:30-33) raises on such a label; on the device the kernels
                # would write a NaN loss instead, which only shows in the epoch mean -- so check while it is on the host
                raise IndexError(f"survival bin label {label.tolist()} outside [0, {n_classes})")
            # group: a host bag goes straight from the loader into its rows of the group buffer (an empty slice of it
            # stands in while the route is decided).  A radiology bag is judged on its host tensors, before any copy.
            direct = group and torch.is_tensor(path_features) and not path_features.is_cuda
            grouped_radio = group and ops._gemm == 0 and _fused_radio_ok(model, loss_fn, radio_features, on_host=True)
            grouped_mm = group and ops._gemm == 0 and isinstance(held, _MMGroup) \
                and _mm_group_ok(model, loss_fn, radio_features, path_features, genomic_features)
            feats, label, c = _to_device({k: r[:0] for k, r in radio_features.items()} if grouped_radio or grouped_mm
                                         else radio_features,
                                         path_features[:0] if direct else path_features, genomic_features, label, c,
                                         device)

            def forward_loss():
                hazards, S, Y_hat, _ = model(**feats)
                if isinstance(loss_fn, CoxSurvLoss):
                    return hazards, loss_fn(risks=hazards, times=torch.as_tensor(np.asarray(event_time)), c=c)
                if isinstance(loss_fn, NLLSurvLoss):
                    return -torch.sum(S, dim=1), loss_fn(hazards=hazards, S=S, Y=label, c=c)
                raise NotImplementedError(type(loss_fn))

            fused_step = _fused_step_ok(model, loss_fn, feats)
            grouped = grouped_radio or grouped_mm or (group and fused_step and feats["path_features"].dtype == torch.float32
                                                      and ops._gemm == 0)
            if group and not grouped:
                flush()                  # the bags held so far run first: the window keeps loader order
                if direct:
                    feats["path_features"] = path_features.to(device, non_blocking=True)
            fused_cox = (not fused_step) and pipe is None and _fused_cox_ok(model, loss_fn, feats)
            fused_mm = (not fused_step) and (not fused_cox) and pipe is None and _fused_mm_ok(model, loss_fn, feats)
            fused_radio = (not grouped) and (not fused_step) and (not fused_cox) and (not fused_mm) and pipe is None \
                and _fused_radio_ok(model, loss_fn, feats)
            if grouped_mm:
                # the multimodal patient, held for the window's grouped call: host tensors go straight into their rows
                held.add(model, radio_features, path_features, genomic_features, label, c, len(losses), device, flush)
                loss = risk = None
            elif grouped:
                # held for the window's grouped call; its loss and risk fill these slots when the group runs
                if grouped_radio:
                    xs = [radio_features[m] for m in model.modalities]
                else:
                    xs = [path_features if direct else feats["path_features"]]
                held.add(xs, label, c, len(losses), held.row_limit(model, len(xs), int(xs[0].shape[1])), device, flush,
                         seed=ops.next_dropout_seed() if model.training else 0)
                loss = risk = None
            elif fused_radio:
                _, _, _, _, loss, risk = model.nll_step(label, c, alpha=loss_fn.alpha, loss_scale=1.0 / G, **feats)
                fused_step = True
            elif fused_mm:
                # the multimodal concat head: branches, one head + loss launch, branch backwards -- no autograd graph; the
                # gradient of loss / G is already in .grad
                _, _, _, _, loss, risk = model.nll_step(label, c, alpha=loss_fn.alpha, loss_scale=1.0 / G, **feats)
                fused_step = True
            elif fused_cox:
                # the omic batch: MaxNet forward + Cox + backward in one launch; the gradient of loss / G is already in .grad
                risk, loss = model.cox_step(feats["genomic_features"], event_time, c, loss_scale=1.0 / G)
                fused_step = True
            elif pipe is not None and fused_step:
                _, _, _, _, loss, risk = pipe.run_fused(model, feats["path_features"], label, c, loss_fn.alpha,
                                                        loss_scale=1.0 / G)
            elif pipe is not None:
                box = {}

                def bag():
                    box["risk"], box["loss"] = forward_loss()
                    return box["loss"] / G

                pipe.run(bag, inputs=list(feats.values()) + [label, c])
                risk, loss = box["risk"], box["loss"]
            elif fused_step:
                # forward + nll_surv + backward of the bag in one call; the gradient of loss / G is already in .grad
                _, _, _, _, loss, risk = model.nll_step(feats["path_features"], label, c, alpha=loss_fn.alpha,
                                                        loss_scale=1.0 / G)
            else:
                risk, loss = forward_loss()
            if fused_tail:
                # the L1 term never enters autograd: its gradient (lambda * sign(W) per kept bag) is added inside the
                # Adam kernel, its value is a device scalar for logging only
                loss_reg = optimizer.l1_value() if (reg_fn is not None and lambda_reg) else 0
            else:
                loss_reg = 0 if reg_fn is None else reg_fn(model) * lambda_reg
            losses.append(None if grouped else loss.detach())
            regs.append(loss_reg.detach() if torch.is_tensor(loss_reg) else torch.tensor(float(loss_reg), device=device))
            all_risk.append(None if grouped else risk.detach().reshape(-1))
            all_c.append(c.detach().reshape(-1))
            all_t.append(np.asarray(event_time).reshape(-1))
            # the reference: loss = loss / gc + loss_reg ; backward (core_utils.py:242-243)
            if fused_step or grouped:
                if not fused_tail and torch.is_tensor(loss_reg) and loss_reg.requires_grad:
                    loss_reg.backward()          # the autograd L1 term touches parameters only
            elif pipe is None:
                (loss / G if fused_tail else loss / G + loss_reg).backward()
            win.kept += 1
        # window boundary: the last position of this rank's window is `last`; (last + 1) % G == 0 as the reference's
        # (batch_idx + 1) % gc == 0.  With world > 1 `last` belongs to rank world - 1 and must exist in the loader.
        last = pos + (world - 1 - rank)
        if (last + 1) % G == 0 and (n_total is None or last < n_total):
            if group:
                flush()
            win.boundary(last_bag_ran=(not skipped) if rank == world - 1 else False)
    if group:
        flush()                      # a trailing partial window: run, accumulated and not stepped, as in the reference
    if pipe is not None:
        pipe.join()                  # the epoch's statistics below read tensors produced on the side streams
        win.fold()                   # a trailing partial window stays accumulated in the bucket, as in the reference
    n = max(n_pos, 1)                # the reference divides by len(loader), skipped positions included (:250-251)
    loss_vals = torch.stack(losses).float().cpu().numpy() if losses else np.zeros(0)
    reg_vals = torch.stack(regs).float().cpu().numpy() if regs else np.zeros(0)
    train_loss_surv = float(loss_vals.sum()) / n
    train_loss = float((loss_vals + reg_vals).sum()) / n
    risks = torch.cat(all_risk).cpu().numpy() if all_risk else np.zeros(0)
    cens = torch.cat(all_c).cpu().numpy() if all_c else np.zeros(0)
    times = np.concatenate(all_t) if all_t else np.zeros(0)
    c_index = concordance_index_censored((1 - cens).astype(bool), times, risks, tied_tol=1e-08)[0]
    print('Epoch: {}, train_loss_surv: {:.4f}, train_loss: {:.4f}, train_c_index: {:.4f}'.format(
        epoch, train_loss_surv, train_loss, c_index))
    if writer:
        writer.add_scalar('train/loss_surv', train_loss_surv, epoch)
        writer.add_scalar('train/loss', train_loss, epoch)
        writer.add_scalar('train/c_index', c_index, epoch)
    return dict(loss_surv=train_loss_surv, loss=train_loss, c_index=c_index, losses=loss_vals, risks=risks)


def _eval_group_head(model):
    """'path' / 'path_fp32' / 'radio' / 'mm' when the grouped forward-only pass (model.forward_group) computes what
    `model(**feats)` does under no_grad -- the pathology, radiology or multimodal head ITSELF (an overridden forward or any hook would
    be bypassed), a classifier of <= 32 classes, the exact-fp32 GEMM mode -- else None.  'path_fp32': a pathology head
    whose bf16 bags the grouped pass does not take (ops.infer_group_takes_bf16).  Asked once per pass: none of it changes
    between bags."""
    from .. import ops
    from ..models.model_attention_mil_path import MIL_Attention_fc_surv_path
    from ..models.model_attention_mil_radio import MIL_Attention_fc_surv_radio
    import torch.nn.modules.module as tm
    from ..models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    kind = {MIL_Attention_fc_surv_path.forward: "path", MIL_Attention_fc_surv_radio.forward: "radio",
            MM_MIL_Attention_fc_surv.forward: "mm"}.get(type(model).forward)
    head = getattr(model, "classifier", None)
    if kind == "mm":             # both fusions; the tensor fusion in the configuration its kernels take (as nll_step)
        if getattr(model, "fusion", None) == "tensor":
            head = head[3]
            if not (model.mm.skip and len(model._concat_order()) * model.mm.reduce[0][0][0].weight.shape[0] <= 384):
                return None
        elif getattr(model, "fusion", None) != "concat" or not hasattr(model, "forward_group"):
            return None
    if ops._gemm != 0 or getattr(head, "out_features", 1 << 30) > 32:
        return None
    hooked = lambda m: bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None))
    if kind is None or any(hooked(m) for m in model.modules()):
        return None
    if tm._global_forward_hooks or tm._global_forward_pre_hooks or tm._global_backward_hooks or getattr(tm, "_global_backward_pre_hooks", None):
        return None
    if kind == "path":           # bf16 bags too, unless the head's one-bag bf16 route is a fused form
        from ..models.model_modules import stack_args
        gated, stack, _, _ = stack_args(model.attention_net_WSI, False)
        if not ops.infer_group_takes_bf16(gated, stack[0].shape[0], stack[2].shape[0]):
            kind = "path_fp32"
    return kind


def _eval_group_bags(model, radio_features, path_features, kind=0):
    """The bag tensors (one per modality) of a subject the grouped forward-only pass takes, or None: a head it takes
    (_eval_group_head; `kind`: its answer, when the caller asked already), 2-D bags -- fp32 (or bf16 where the head's kind
    allows it) for the pathology head, fp32 modalities of one shape for the radiology head.  The bags may still be on the
    host."""
    kind = _eval_group_head(model) if kind == 0 else kind
    if kind in ("path", "path_fp32"):
        xs = [path_features]
        dtypes = (torch.float32, torch.bfloat16) if kind == "path" else (torch.float32,)
        if not (torch.is_tensor(path_features) and path_features.dtype in dtypes):
            return None
    elif kind == "radio":
        xs = [radio_features.get(m) if isinstance(radio_features, dict) else None for m in model.modalities]
        if any(not (torch.is_tensor(x) and x.dtype == torch.float32) for x in xs):
            return None
    else:
        return None
    if any(x.dim() != 2 or x.shape != xs[0].shape or x.shape[0] < 1 for x in xs):
        return None
    return xs


class _EvalGroup(_HeldBags):
    """validate_survival / summary_survival(group=True): the eligible bags of an evaluation pass, until one grouped
    forward-only call (model.forward_group) runs them.  One per pass: nothing outlives the pass (an exception leaves no
    held bags behind, and the buffer is freed with it)."""

    def run(self, model, loss_alpha=None):
        """One grouped call over the held bags -> [(slot, hazards [1 x K], S [1 x K], loss (0-dim) or None, risk [1])];
        loss_alpha: each bag's NLLSurvLoss value with that alpha, or None for no loss.  The group is empty afterwards."""
        if not self.sizes:
            return []
        want = loss_alpha is not None
        hz, S, _, _, loss, risk = model.forward_group(self.held(model), torch.cat(self.labels) if want else None,
                                                      torch.cat(self.cs) if want else None,
                                                      alpha=loss_alpha if want else 0.0)
        out = [(slot, hz[g:g + 1], S[g:g + 1], loss[g] if want else None, risk[g:g + 1])
               for g, slot in enumerate(self.slots)]
        self.reset()
        return out


def _mm_eval_ok(model, radio_features, path_features, genomic_features):
    """A multimodal subject the grouped forward-only pass takes (MM_MIL_Attention_fc_surv.forward_group): for every
    branch in model.mode a 2-D fp32 bag (the modalities of one shape) or an omic vector of the model's input width.  The
    tensors may still be on the host."""
    bag = lambda t: torch.is_tensor(t) and t.dim() == 2 and t.dtype == torch.float32 and t.shape[0] >= 1
    if "path" in model.mode and not bag(path_features):
        return False
    if "radio" in model.mode:
        xs = [radio_features.get(m) if isinstance(radio_features, dict) else None for m in model.modalities]
        if any(not bag(x) or x.shape != xs[0].shape for x in xs):
            return False
    if "omic" in model.mode and not (torch.is_tensor(genomic_features) and genomic_features.is_floating_point()
                                     and genomic_features.numel() == model.fc_omic[0][0].in_features):
        return False
    return True


class _MMEvalGroup(_MMGroup):
    """validate_survival / summary_survival(group=True) with the multimodal head: the forward-only sibling of _MMGroup --
    the eligible patients of an evaluation pass in the same three buffers (pathology plane, radio planes, omic rows),
    until one grouped forward-only call (model.forward_group) runs them.  One per pass, as _EvalGroup."""

    def takes(self, model, radio_features, path_features, genomic_features):
        """Whether the subject can be held: _mm_eval_ok, and each of its bags within that branch's row limit."""
        if not _mm_eval_ok(model, radio_features, path_features, genomic_features):
            return False
        has = lambda k: k in model.mode
        x_r = radio_features[model.modalities[0]] if has("radio") else None
        lim_p, lim_r = self.row_limits(model, int(path_features.shape[1]) if has("path") else None,
                                       int(x_r.shape[1]) if has("radio") else None)
        return not (has("path") and int(path_features.shape[0]) > lim_p or has("radio") and int(x_r.shape[0]) > lim_r)

    def run(self, model, loss_alpha=None):
        """As _EvalGroup.run, over the held patients."""
        if not self.slots:
            return []
        want = loss_alpha is not None
        hz, S, _, _, loss, risk = model.forward_group(self.window(model), torch.cat(self.labels) if want else None,
                                                      torch.cat(self.cs) if want else None,
                                                      alpha=loss_alpha if want else 0.0)
        out = [(slot, hz[g:g + 1], S[g:g + 1], loss[g] if want else None, risk[g:g + 1])
               for g, slot in enumerate(self.slots)]
        self.reset()
        return out


def _eval_hold(model, kind, held, limits, batch, slot, device, flush):
    """Holds the subject `batch` (the loader's tuple) for the pass's grouped call when that call takes it (`kind`:
    _eval_group_head's answer) and returns its (label, c) on the device; None: the subject runs alone."""
    radio_features, path_features, genomic_features, label, _, c = batch
    if kind == "mm":
        if not held.takes(model, radio_features, path_features, genomic_features):
            return None
        label, c = label.to(device), c.to(device)
        held.add(model, radio_features, path_features, genomic_features.float(), label, c, slot, device, flush)
        return label, c
    xs = _eval_group_bags(model, radio_features, path_features, kind)
    limit = _EvalGroup.limit_of(model, xs, limits) if xs is not None else 0
    if xs is None or int(xs[0].shape[0]) > limit:
        return None
    label, c = label.to(device), c.to(device)
    held.add(xs, label, c, slot, limit, device, flush)
    return label, c


def validate_survival(cur, epoch, model, loader, n_classes, mode, early_stopping=None, writer=None, loss_fn=None,
                      reg_fn=None, lambda_reg=0., results_dir=None, t_bin=None, group=False):
    """utils/core_utils.py:267-355: eval-mode forward + loss + c-index (early stopping hook kept).

    group=True: the bags the grouped forward-only pass takes (_eval_group_bags) are held on the device and run as one
    model.forward_group call per ops.GROUP_MAX bags or row limit, flushed at the end; each bag's loss and risk land in its
    loader slot, so every logged quantity is in the order of the per-bag loop.  A bag it does not take flushes the group
    and runs alone.  The stock NLLSurvLoss value comes from the grouped call, with the alpha the per-bag branch passes;
    other losses are called on the bag's slice.  reg_fn(model) is evaluated once per pass (the weights are fixed).
    A multimodal model's patients (both fusions; _mm_eval_ok) are held the same way in _MMEvalGroup -- a pathology plane,
    the radio planes and the omic rows -- and run as one MM_MIL_Attention_fc_surv.forward_group call per flush."""
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.eval()
    losses, regs, all_risk, all_c, all_t = [], [], [], [], []
    if group:
        reg_once, meta, kind, limits = [], {}, _eval_group_head(model), {}
        held = _MMEvalGroup() if kind == "mm" else _EvalGroup()
        kernel_loss = type(loss_fn) is NLLSurvLoss

        def flush():      # the held bags' losses / risks land in their loader slots
            for slot, hz_g, S_g, loss_g, _ in held.run(model, 0.0 if kernel_loss else None):
                label_g, c_g, t_g = meta.pop(slot)
                if isinstance(loss_fn, CoxSurvLoss):
                    risk_g = hz_g
                    loss_g = loss_fn(risks=risk_g, times=torch.as_tensor(np.asarray(t_g)), c=c_g)
                else:
                    risk_g = -torch.sum(S_g, dim=1)          # the per-bag branch's expression, on the bag's S
                    if not kernel_loss:
                        loss_g = loss_fn(hazards=hz_g, S=S_g, Y=label_g, c=c_g, alpha=0)
                losses[slot] = loss_g
                all_risk[slot] = risk_g.reshape(-1)
    with torch.no_grad():
        for batch in loader:
            radio_features, path_features, genomic_features, label, event_time, c = batch
            if _skip(mode, radio_features, path_features, genomic_features):
                continue
            took = _eval_hold(model, kind, held, limits, batch, len(losses), device, flush) if group and kind else None
            if took is not None:
                label, c = took
                meta[len(losses)] = (label, c, event_time)
                if not reg_once:         # the weights are fixed: one value (one device tensor) for the pass
                    loss_reg = 0 if reg_fn is None else reg_fn(model) * lambda_reg
                    reg_once.append(loss_reg if torch.is_tensor(loss_reg) else torch.tensor(float(loss_reg), device=device))
                losses.append(None)
                regs.append(reg_once[0])
                all_risk.append(None)
                all_c.append(c.reshape(-1))
                all_t.append(np.asarray(event_time).reshape(-1))
                continue
            if group:
                flush()                  # the bags held so far run first
            feats, label, c = _to_device(radio_features, path_features, genomic_features, label, c, device)
            hazards, S, Y_hat, _ = model(**feats)
            if isinstance(loss_fn, CoxSurvLoss):
                risk = hazards
                loss = loss_fn(risks=risk, times=torch.as_tensor(np.asarray(event_time)), c=c)
            else:
                risk = -torch.sum(S, dim=1)
                loss = loss_fn(hazards=hazards, S=S, Y=label, c=c, alpha=0)
            loss_reg = 0 if reg_fn is None else reg_fn(model) * lambda_reg
            losses.append(loss)
            regs.append(loss_reg if torch.is_tensor(loss_reg) else torch.tensor(float(loss_reg), device=device))
            all_risk.append(risk.reshape(-1))
            all_c.append(c.reshape(-1))
            all_t.append(np.asarray(event_time).reshape(-1))
        if group:
            flush()
    n = max(len(losses), 1)
    loss_vals = torch.stack(losses).float().cpu().numpy()
    reg_vals = torch.stack(regs).float().cpu().numpy()
    val_loss_surv = float(loss_vals.sum()) / n
    val_loss = float((loss_vals + reg_vals).sum()) / n
    risks = torch.cat(all_risk).cpu().numpy()
    cens = torch.cat(all_c).cpu().numpy()
    times = np.concatenate(all_t)
    c_index = concordance_index_censored((1 - cens).astype(bool), times, risks, tied_tol=1e-08)[0]
    if writer:
        writer.add_scalar('val/loss_surv', val_loss_surv, epoch)
        writer.add_scalar('val/loss', val_loss, epoch)
        writer.add_scalar('val/c-index', c_index, epoch)
    if early_stopping is not None:
        early_stopping(epoch, val_loss_surv, model)
        if getattr(early_stopping, "early_stop", False):
            print("Early stopping")
            return True
    return False


def summary_survival(model, loader, n_classes, mode, t_bin=None, loss_fn=None, group=False):
    """utils/core_utils.py:358-430: eval-mode pass over a loader -> (patient_results, c_index).
    risk = the head's scalar output for Cox / ranking losses, -sum(S) for the discrete-hazard losses; subjects whose
    required modality is the "missing" sentinel are skipped exactly as in the reference (:379-386).  Subject ids are
    read from `loader.dataset.slides_radio_data['subject_id']` when the loader has one (the reference requires it),
    else the running index is used.  One device -> host copy at the end instead of one per subject.
    group=True: as validate_survival(group=True) -- the bags the grouped forward-only pass takes run as grouped calls,
    each risk lands in its subject's slot (same ids, same order)."""
    from .loss_utils import RankingSurvLoss
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.eval()
    ids = None
    ds = getattr(loader, "dataset", None)
    if ds is not None and hasattr(ds, "slides_radio_data"):
        ids = list(ds.slides_radio_data["subject_id"])
    all_ids, all_risk, all_c, all_t, all_y = [], [], [], [], []
    count = 0
    head_risk = isinstance(loss_fn, (CoxSurvLoss, RankingSurvLoss))
    if group:
        kind, limits = _eval_group_head(model), {}
        held = _MMEvalGroup() if kind == "mm" else _EvalGroup()

        def flush():      # the held bags' risks land in their subjects' slots (the per-bag expressions, on the bag's slice)
            for slot, hz_g, S_g, _, _ in held.run(model):
                all_risk[slot] = (hz_g if head_risk else -torch.sum(S_g, dim=1)).reshape(-1)
    with torch.no_grad():
        for batch in loader:
            radio_features, path_features, genomic_features, label, event_time, c = batch
            n = len(label)
            sid = ids[count:count + n] if ids is not None else list(range(count, count + n))
            count += n
            if _skip(mode, radio_features, path_features, genomic_features):
                continue
            took = _eval_hold(model, kind, held, limits, batch, len(all_risk), device, flush) if group and kind else None
            if took is not None:
                label, c = took
                all_ids.extend(sid)
                all_risk.append(None)
                all_c.append(c.reshape(-1))
                all_t.append(np.asarray(event_time).reshape(-1))
                all_y.append(label.reshape(-1))
                continue
            if group:
                flush()                  # the bags held so far run first
            feats, label, c = _to_device(radio_features, path_features, genomic_features, label, c, device)
            hazards, S, Y_hat, _ = model(**feats)
            risk = hazards if head_risk else -torch.sum(S, dim=1)
            all_ids.extend(sid)
            all_risk.append(risk.reshape(-1))
            all_c.append(c.reshape(-1))
            all_t.append(np.asarray(event_time).reshape(-1))
            all_y.append(label.reshape(-1))
        if group:
            flush()
    risks = torch.cat(all_risk).cpu().numpy()
    cens = torch.cat(all_c).cpu().numpy()
    labels = torch.cat(all_y).cpu().numpy()
    times = np.concatenate(all_t)
    patient_results = {"subject_id": np.asarray(all_ids), "risk": risks, "disc_label": labels, "survival": times,
                       "censorship": cens}
    c_index = concordance_index_censored((1 - cens).astype(bool), times, risks, tied_tol=1e-08)[0]
    return patient_results, c_index
