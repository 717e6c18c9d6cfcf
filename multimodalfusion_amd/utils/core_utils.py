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


def _unhooked(model):
    """Nothing that a call which goes round `model(...)` would bypass: no hook on any module of `model`, no global hook."""
    import torch.nn.modules.module as tm
    if tm._global_forward_hooks or tm._global_forward_pre_hooks or tm._global_backward_hooks or getattr(tm, "_global_backward_pre_hooks", None):
        return False
    return not any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None)
                   for m in model.modules())


def _stock_head(model, step):
    """(kind, hazard-head Linear) when a graph-free call computes what `model(**feats)` does, else (None, None).  kind:
    'path' / 'radio' / 'mm' / 'omic' -- type(model).forward IS that head's (a subclass that overrides forward() would be
    bypassed), the multimodal head with the concat fusion or the tensor fusion as the heads configure it
    (xfusion_step_ok), a hazard head of <= 32 classes (the kernels' single-workgroup tail), nothing hooked (_unhooked: the
    one walk over the modules).  step: asked for the one-call training steps -- every parameter trainable (the omic head:
    cox_step_ok asks that itself) and, for the radiology and multimodal heads, the per-instance switch mmf_one_call_step (the
    pathology step ignores it) -- or, False, for the grouped forward-only pass, which has no omic form.  DESIGN.md 7m."""
    from ..models.model_attention_mil_path import MIL_Attention_fc_surv_path
    from ..models.model_attention_mil_radio import MIL_Attention_fc_surv_radio
    from ..models.model_genomic import MaxNet
    from ..models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    kind = {MIL_Attention_fc_surv_path.forward: "path", MIL_Attention_fc_surv_radio.forward: "radio",
            MM_MIL_Attention_fc_surv.forward: "mm", MaxNet.forward: "omic"}.get(type(model).forward)
    entry = ("cox_step" if kind == "omic" else "nll_step") if step else "forward_group"
    if kind is None or (kind == "omic" and not step) or not hasattr(model, entry):
        return None, None
    head = getattr(model, "classifier", None)
    if kind == "mm":
        fusion = getattr(model, "fusion", None)
        if fusion == "tensor" and model.xfusion_step_ok():
            head = head[3]
        elif fusion != "concat":
            return None, None
    if getattr(head, "out_features", 1 << 30) > 32:
        return None, None
    if step and kind in ("radio", "mm") and not getattr(model, "mmf_one_call_step", True):
        return None, None
    if not _unhooked(model) or (step and kind != "omic" and not all(p.requires_grad for p in model.parameters())):
        return None, None
    return kind, head


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


class _Group:
    """What the two holders share.  Each exposes `held(model)`, what the model's grouped calls take, and `slots`, the
    loader slots of what it holds (with `labels`, `cs`, `seeds` beside them); the training and the evaluation call are here."""

    def run_step(self, model, alpha, loss_scale):
        """One grouped training call (model.nll_step_group; nll_step_group_tensor for the tensor fusion) over what is held
        -> [(loader slot, loss [1], risk [1])]; the holder is empty afterwards."""
        if not self.slots:
            return []
        step = model.nll_step_group_tensor if getattr(model, "fusion", None) == "tensor" else model.nll_step_group
        _, _, _, _, loss, risk = step(self.held(model), torch.cat(self.labels), torch.cat(self.cs), alpha=alpha,
                                      loss_scale=loss_scale, seeds=self.seeds if model.training else None)
        out = [(slot, loss[g:g + 1], risk[g:g + 1]) for g, slot in enumerate(self.slots)]
        self.reset()
        return out

    def run_eval(self, model, loss_alpha=None):
        """One grouped forward-only call (model.forward_group) over what is held -> [(slot, hazards [1 x K], S [1 x K], loss
        (0-dim) or None)]; loss_alpha: each subject's NLLSurvLoss value with that alpha, or None for no loss.  The holder
        is empty afterwards."""
        if not self.slots:
            return []
        want = loss_alpha is not None
        hz, S, _, _, loss, _ = model.forward_group(self.held(model), torch.cat(self.labels) if want else None,
                                                   torch.cat(self.cs) if want else None, alpha=loss_alpha if want else 0.0)
        out = [(slot, hz[g:g + 1], S[g:g + 1], loss[g] if want else None) for g, slot in enumerate(self.slots)]
        self.reset()
        return out


class _HeldBags(_Group):
    """The pathology and radiology heads' holder: the bags a grouped call will take, held on the device until it runs (a
    training window's -- each with the dropout seed drawn when it arrived, so bag g of the loader gets the masks the per-bag
    route gives it -- or an evaluation pass's).  Each bag is copied straight into its rows of one reusable device buffer [n_mod x rows x L] (no
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

    def planes(self, stacked):
        """The held rows, (x [rows x L] or, stacked, [n_mod x rows x L], sizes); the bags held by reference reach them here."""
        self.materialise()
        return (self.buf[:, :self.rows] if stacked else self.buf[0, :self.rows]), list(self.sizes)

    def held(self, model):
        """The held rows as the model's grouped calls take them: the radiology head's stacked, the pathology head's not."""
        return self.planes(hasattr(model, "attention_net_radio"))


class _MMGroup(_Group):
    """The multimodal head's holder: the eligible patients of a training window or of an evaluation pass, until one grouped
    call (MM_MIL_Attention_fc_surv.nll_step_group, nll_step_group_tensor for a tensor-fusion model that opted in, or
    forward_group) runs them.  A patient's bags are copied straight into their rows of three reusable device buffers -- the
    pathology plane [1 x rows x L], the radio planes [n_mod x rows x L] and the omic rows [GROUP_MAX x input_dim] -- and its
    dropout seeds are drawn when it arrives, in nll_step's order (radio, path, omic; then the fusion seed of the tensor
    fusion), so patient g of the loader gets the masks the per-patient route gives it.  A patient that would take the group
    past ops.GROUP_MAX or past either branch's row limit flushes what is held first."""

    def __init__(self):
        self.path, self.radio, self.omic = _HeldBags(), _HeldBags(), None
        self.limits = {}
        self.reset()

    def reset(self):
        self.path.reset()
        self.radio.reset()
        self.labels, self.cs, self.slots, self.seeds = [], [], [], {}

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

    def takes(self, model, radio_features, path_features):
        """Whether each bag of a patient _mm_bags_ok passed is within its branch's row limit (an evaluation pass asks; a
        training window splits instead)."""
        has = lambda k: k in model.mode
        x_r = radio_features[model.modalities[0]] if has("radio") else None
        lim_p, lim_r = self.row_limits(model, int(path_features.shape[1]) if has("path") else None,
                                       int(x_r.shape[1]) if has("radio") else None)
        return not (has("path") and int(path_features.shape[0]) > lim_p or has("radio") and int(x_r.shape[0]) > lim_r)

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
        # nll_step's order; a held tensor-fusion patient is one of a model that opted in (_bag_route)
        for k in [k for k in ("radio", "path", "omic") if has(k)] + (["fusion"] if model.fusion == "tensor" else []):
            self.seeds.setdefault(k, []).append(ops.next_dropout_seed() if model.training else 0)
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

    def held(self, model):
        """The held patients as the model's grouped calls take them: the pre-stacked (path, radio, omic) triple."""
        has = lambda k: k in model.mode
        return (self.path.planes(False) if has("path") else None,
                self.radio.planes(True) if has("radio") else None,
                self.omic[:len(self.slots)] if has("omic") else None)


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


def _mm_bags_ok(model, radio_features, path_features, genomic_features):
    """A multimodal patient's tensors as the grouped calls take them (nll_step_group[_tensor], forward_group): for every
    branch in model.mode a 2-D fp32 bag of >= 1 rows (the modalities of one shape) or an omic vector of the model's input
    width -- its dtype is the caller's question.  The tensors may still be on the host."""
    bag = lambda t: torch.is_tensor(t) and t.dim() == 2 and t.dtype == torch.float32 and t.shape[0] >= 1
    if "path" in model.mode and not bag(path_features):
        return False
    if "radio" in model.mode:
        xs = [radio_features.get(m) if isinstance(radio_features, dict) else None for m in model.modalities]
        if any(not bag(x) or x.shape != xs[0].shape for x in xs):
            return False
    if "omic" in model.mode and not (torch.is_tensor(genomic_features)
                                     and genomic_features.numel() == model.fc_omic[0][0].in_features):
        return False
    return True


def _bag_route(model, loss_fn, radio_features, path_features, genomic_features, group=False, inflight=1, gemm=0):
    """The one route a bag takes through train_loop_survival (the table of DESIGN.md 7m), from the tensors as the loader
    delivers them -- nothing is copied to decide it -- and with one walk over the model's modules (_stock_head):
      held-path / held-radio / held-mm   held for the window's grouped call (group, exact-fp32 GEMMs, fp32 bags);
      step-path / step-radio / step-mm   the head's nll_step, no autograd graph;   step-cox   MaxNet.cox_step;
      pipe-fused / pipe-autograd         inflight > 1: only the pathology head has a fused form there;
      autograd                           model(**feats), the loss, backward().
    A graph-free route only where it is exactly what `model(**feats)` + the stock loss would compute: a stock head
    (_stock_head) and the stock loss class.  The one-call steps need their inputs on the GPU, where the loop's copy leaves
    them whenever there is one; a held bag may stay where it is."""
    kind, _ = _stock_head(model, step=True)
    piped, hold, fp32 = inflight > 1, group and gemm == 0, torch.float32
    on_gpu = lambda t: t.is_cuda or torch.cuda.is_available()
    nll = type(loss_fn) is NLLSurvLoss
    if kind == "path" and nll:
        x = path_features
        if torch.is_tensor(x) and x.dim() == 2 and on_gpu(x) and x.dtype in (fp32, torch.bfloat16):
            if piped:
                return "pipe-fused"
            return "held-path" if hold and x.dtype == fp32 else "step-path"       # a bf16 bag runs alone
    elif kind == "radio" and nll:
        xs = [radio_features.get(m) for m in model.modalities]
        if all(torch.is_tensor(x) and x.dim() == 2 and x.dtype == fp32 and x.shape == xs[0].shape for x in xs):
            if hold:
                return "held-radio"
            if not piped and all(on_gpu(x) for x in xs):
                return "step-radio"
    elif kind == "mm" and nll:
        every = [*radio_features.values(), path_features, genomic_features]
        if all(torch.is_tensor(t) for t in every):
            opted = model.fusion == "tensor" and bool(getattr(model, "mmf_group_tensor", False))   # per instance; absent: off
            if hold and (model.xfusion_group_ok() if opted else model.fusion == "concat") \
                    and _mm_bags_ok(model, radio_features, path_features, genomic_features):
                return "held-mm"
            if not piped and all(on_gpu(t) for t in every):
                return "step-mm"
    elif kind == "omic" and type(loss_fn) is CoxSurvLoss and not piped:
        # cox_step_ok: the batch's shape, a Cox head, every parameter trainable; the loop's copy makes the batch fp32
        x = genomic_features
        if torch.is_tensor(x) and on_gpu(x) and model.cox_step_ok(x, on_host=True):
            return "step-cox"
    return "pipe-autograd" if piped else "autograd"


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
                ranks.  The multimodal head's patients (those its one-call step takes, fp32 bags) are held in the same
                way -- a pathology plane, the radio planes and the omic rows -- and run as ONE nll_step_group per window;
                a tensor-fusion model's when it opted in (model.mmf_group_tensor = True, scale width 16:
                nll_step_group_tensor), else they keep the per-patient route.  _bag_route picks each bag's route."""
    from .. import ops
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
    if group:
        held = getattr(win, "group", None)
        if held is None:
            held = win.group = _MMGroup() if hasattr(model, "attention_net_radio") and hasattr(model, "attention_net_WSI") \
                else _HeldBags()
        alpha_g = getattr(loss_fn, "alpha", 0.0)

        def flush():      # the held bags' losses / risks land in their loader slots
            for slot, loss_g, risk_g in held.run_step(model, alpha_g, 1.0 / G):
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
            # one route per bag, asked per bag (a hook registered mid-epoch takes effect at the next one) on the tensors as
            # they arrive: a held bag goes straight from where it is into its rows of the group buffer
            route = _bag_route(model, loss_fn, radio_features, path_features, genomic_features, group, inflight, ops._gemm)
            holds = route.startswith("held-")
            if group and not holds:
                flush()                  # the bags held so far run first: the window keeps loader order
            if holds:
                label, c = label.to(device), c.to(device)
            else:
                feats, label, c = _to_device(radio_features, path_features, genomic_features, label, c, device)

            def forward_loss():
                hazards, S, Y_hat, _ = model(**feats)
                if isinstance(loss_fn, CoxSurvLoss):
                    return hazards, loss_fn(risks=hazards, times=torch.as_tensor(np.asarray(event_time)), c=c)
                if isinstance(loss_fn, NLLSurvLoss):
                    return -torch.sum(S, dim=1), loss_fn(hazards=hazards, S=S, Y=label, c=c)
                raise NotImplementedError(type(loss_fn))

            loss = risk = None           # a held bag's fill these slots when its group runs
            if route == "held-mm":
                held.add(model, radio_features, path_features, genomic_features, label, c, len(losses), device, flush)
            elif holds:
                xs = [radio_features[m] for m in model.modalities] if route == "held-radio" else [path_features]
                held.add(xs, label, c, len(losses), held.row_limit(model, len(xs), int(xs[0].shape[1])), device, flush,
                         seed=ops.next_dropout_seed() if model.training else 0)
            elif route in ("step-radio", "step-mm"):
                # reduce_dim / the branches, one head + loss launch, their backwards -- no autograd graph
                _, _, _, _, loss, risk = model.nll_step(label, c, alpha=loss_fn.alpha, loss_scale=1.0 / G, **feats)
            elif route == "step-path":
                # forward + nll_surv + backward of the bag in one call
                _, _, _, _, loss, risk = model.nll_step(feats["path_features"], label, c, alpha=loss_fn.alpha,
                                                        loss_scale=1.0 / G)
            elif route == "step-cox":
                # the omic batch: MaxNet forward + Cox + backward in one launch
                risk, loss = model.cox_step(feats["genomic_features"], event_time, c, loss_scale=1.0 / G)
            elif route == "pipe-fused":
                _, _, _, _, loss, risk = pipe.run_fused(model, feats["path_features"], label, c, loss_fn.alpha,
                                                        loss_scale=1.0 / G)
            elif route == "pipe-autograd":
                box = {}

                def bag():
                    box["risk"], box["loss"] = forward_loss()
                    return box["loss"] / G

                pipe.run(bag, inputs=list(feats.values()) + [label, c])
                risk, loss = box["risk"], box["loss"]
            else:
                risk, loss = forward_loss()
            if fused_tail:
                # the L1 term never enters autograd: its gradient (lambda * sign(W) per kept bag) is added inside the
                # Adam kernel, its value is a device scalar for logging only
                loss_reg = optimizer.l1_value() if (reg_fn is not None and lambda_reg) else 0
            else:
                loss_reg = 0 if reg_fn is None else reg_fn(model) * lambda_reg
            losses.append(None if holds else loss.detach())
            regs.append(loss_reg.detach() if torch.is_tensor(loss_reg) else torch.tensor(float(loss_reg), device=device))
            all_risk.append(None if holds else risk.detach().reshape(-1))
            all_c.append(c.detach().reshape(-1))
            all_t.append(np.asarray(event_time).reshape(-1))
            # the reference: loss = loss / gc + loss_reg ; backward (core_utils.py:242-243)
            if route == "autograd":
                (loss / G if fused_tail else loss / G + loss_reg).backward()
            elif not route.startswith("pipe-"):
                # held or a one-call step: the gradient of loss / G is (or will be) in .grad already
                if not fused_tail and torch.is_tensor(loss_reg) and loss_reg.requires_grad:
                    loss_reg.backward()          # the autograd L1 term touches parameters only
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
    `model(**feats)` does under no_grad -- a stock pathology, radiology or multimodal head (_stock_head) in the exact-fp32
    GEMM mode -- else None.  'path_fp32': a pathology head whose bf16 bags the grouped pass does not take
    (ops.infer_group_takes_bf16).  Asked once per pass: none of it changes between bags."""
    from .. import ops
    kind, _ = _stock_head(model, step=False)
    if kind is None or ops._gemm != 0:
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


def _eval_hold(model, kind, held, limits, batch, slot, device, flush):
    """Holds the subject `batch` (the loader's tuple) for the pass's grouped call when that call takes it (`kind`:
    _eval_group_head's answer) and returns its (label, c) on the device; None: the subject runs alone.  A multimodal
    patient: _mm_bags_ok, a floating-point omic vector, each bag within its branch's row limit."""
    radio_features, path_features, genomic_features, label, _, c = batch
    if kind == "mm":
        if not (_mm_bags_ok(model, radio_features, path_features, genomic_features)
                and ("omic" not in model.mode or genomic_features.is_floating_point())
                and held.takes(model, radio_features, path_features)):
            return None
        label, c = label.to(device), c.to(device)
        held.add(model, radio_features, path_features, genomic_features.float(), label, c, slot, device, flush)
        return label, c
    xs = _eval_group_bags(model, radio_features, path_features, kind)
    limit = _HeldBags.limit_of(model, xs, limits) if xs is not None else 0
    if xs is None or int(xs[0].shape[0]) > limit:
        return None
    label, c = label.to(device), c.to(device)
    held.add(xs, label, c, slot, limit, device, flush)
    return label, c


def _eval_pass(model, loader, mode, group, device, land, loss_alpha=None):
    """The one skeleton of validate_survival and summary_survival, to be advanced under torch.no_grad(): yields (batch,
    label, c on the device, held) for every subject the reference does not skip, in loader order, one batch at a time.
    Slot s belongs to the s-th subject yielded; `land(slot, event_time, label, c, hazards, S, loss)` receives its outputs:
    before the yield for a subject that ran alone (loss None), and for a held one (group=True, a head the grouped pass
    takes: _eval_hold) when its grouped call runs -- before any subject that runs alone, and at the end of the pass --
    with its NLLSurvLoss(loss_alpha) value when loss_alpha is given.  One holder per pass: nothing outlives it (an
    exception leaves no held bags behind, and the buffer is freed with it)."""
    kind = _eval_group_head(model) if group else None
    held, limits, meta = _MMGroup() if kind == "mm" else _HeldBags(), {}, {}

    def flush():
        for slot, hz, S, loss in held.run_eval(model, loss_alpha):
            land(slot, *meta.pop(slot), hz, S, loss)

    slot = 0
    for batch in loader:
        radio_features, path_features, genomic_features, label, event_time, c = batch
        if _skip(mode, radio_features, path_features, genomic_features):
            continue
        took = _eval_hold(model, kind, held, limits, batch, slot, device, flush) if kind else None
        if took is not None:
            meta[slot] = (event_time, *took)
            yield batch, *took, True
        else:
            flush()                      # the bags held so far run first
            feats, label, c = _to_device(radio_features, path_features, genomic_features, label, c, device)
            hazards, S, _, _ = model(**feats)
            land(slot, event_time, label, c, hazards, S, None)
            yield batch, label, c, False
        slot += 1
    flush()


def validate_survival(cur, epoch, model, loader, n_classes, mode, early_stopping=None, writer=None, loss_fn=None,
                      reg_fn=None, lambda_reg=0., results_dir=None, t_bin=None, group=False):
    """utils/core_utils.py:267-355: eval-mode forward + loss + c-index (early stopping hook kept).

    group=True: the bags the grouped forward-only pass takes (_eval_group_bags) are held on the device and run as one
    model.forward_group call per ops.GROUP_MAX bags or row limit, flushed at the end; each bag's loss and risk land in its
    loader slot, so every logged quantity is in the order of the per-bag loop.  A bag it does not take flushes the group
    and runs alone.  The stock NLLSurvLoss value comes from the grouped call, with the alpha the per-bag branch passes;
    other losses are called on the bag's slice.  reg_fn(model) is evaluated once per pass for the held bags (the weights
    are fixed).  A multimodal model's patients (both fusions; _mm_bags_ok) are held the same way in _MMGroup -- a pathology
    plane, the radio planes and the omic rows -- and run as one MM_MIL_Attention_fc_surv.forward_group call per flush."""
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.eval()
    losses, all_risk = {}, {}            # by slot: a held bag's land after later bags were logged
    regs, all_c, all_t, reg_once = [], [], [], []

    def land(slot, event_time, label, c, hazards, S, loss):     # the per-bag expressions, on the bag's slice when held
        if isinstance(loss_fn, CoxSurvLoss):
            risk = hazards
            loss = loss_fn(risks=risk, times=torch.as_tensor(np.asarray(event_time)), c=c)
        else:
            risk = -torch.sum(S, dim=1)
            if loss is None:
                loss = loss_fn(hazards=hazards, S=S, Y=label, c=c, alpha=0)
        losses[slot] = loss
        all_risk[slot] = risk.reshape(-1)

    with torch.no_grad():
        for batch, label, c, was_held in _eval_pass(model, loader, mode, group, device, land,
                                                    0.0 if type(loss_fn) is NLLSurvLoss else None):
            if not (was_held and reg_once):
                loss_reg = 0 if reg_fn is None else reg_fn(model) * lambda_reg
                reg = loss_reg if torch.is_tensor(loss_reg) else torch.tensor(float(loss_reg), device=device)
                if was_held:             # the weights are fixed: one value (one device tensor) for the pass's held bags
                    reg_once.append(reg)
            regs.append(reg_once[0] if was_held else reg)
            all_c.append(c.reshape(-1))
            all_t.append(np.asarray(batch[4]).reshape(-1))
    n = max(len(regs), 1)
    loss_vals = torch.stack([losses[s] for s in range(len(regs))]).float().cpu().numpy()
    reg_vals = torch.stack(regs).float().cpu().numpy()
    val_loss_surv = float(loss_vals.sum()) / n
    val_loss = float((loss_vals + reg_vals).sum()) / n
    risks = torch.cat([all_risk[s] for s in range(len(regs))]).cpu().numpy()
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
    all_ids, all_risk, all_c, all_t, all_y = [], {}, [], [], []          # all_risk by slot
    head_risk = isinstance(loss_fn, (CoxSurvLoss, RankingSurvLoss))
    sid = []

    def counted():               # the ids go by loader position, skipped subjects included; `sid`: the current batch's
        count = 0
        for batch in loader:
            n = len(batch[3])
            sid[:] = ids[count:count + n] if ids is not None else range(count, count + n)
            count += n
            yield batch

    def land(slot, event_time, label, c, hazards, S, loss):
        all_risk[slot] = (hazards if head_risk else -torch.sum(S, dim=1)).reshape(-1)

    with torch.no_grad():
        for batch, label, c, _ in _eval_pass(model, counted(), mode, group, device, land):
            all_ids.extend(sid)
            all_c.append(c.reshape(-1))
            all_t.append(np.asarray(batch[4]).reshape(-1))
            all_y.append(label.reshape(-1))
    risks = torch.cat([all_risk[s] for s in range(len(all_c))]).cpu().numpy()
    cens = torch.cat(all_c).cpu().numpy()
    labels = torch.cat(all_y).cpu().numpy()
    times = np.concatenate(all_t)
    patient_results = {"subject_id": np.asarray(all_ids), "risk": risks, "disc_label": labels, "survival": times,
                       "censorship": cens}
    c_index = concordance_index_censored((1 - cens).astype(bool), times, risks, tied_tol=1e-08)[0]
    return patient_results, c_index
