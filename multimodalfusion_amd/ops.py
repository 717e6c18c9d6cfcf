"""torch.autograd Functions over the C ABI (include/mmf_amil.h).

PyTorch is used for device memory, streams and the autograd graph only; every arithmetic
step of the path runs in the HIP kernels of libmmf_amil.so.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._lib import AmilDesc, AmilGrads, NllTarget, SurvHead, check, lib, ptr, stream_ptr

ACT = {"none": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "selu": 4}

_drop_calls = 0

# Host-side plumbing state for two optional per-call ABI arguments (the library itself keeps no state):
#   _seed_word  a device int32 word added to every dropout seed (graph.DeviceSeed sets it while it captures / replays a
#               hipGraph); each autograd node remembers the word its forward used, so its backward uses the same one;
#   _trace      an mmf_trace handle (bench.py's roofline leg: per-kernel HIP-event timing on the launch stream).
#   _concurrent scheduling hint (mmf_amil_desc::concurrent): pipeline.BagsInFlight raises it while it issues a bag.
#   _gemm       mmf_amil_desc::gemm: 0 = exact-fp32 MFMA, 1 = split-operand bf16x3 (fp32-equivalent error, faster on large
#               bags); starts from the MMF_GEMM environment variable (0 / 1, default 0).
_seed_word = None
_trace = None
_concurrent = 0
_gemm = int(os.environ.get("MMF_GEMM", "0"))


def set_gemm(mode):
    """mode: 0 (exact fp32 MFMA) or 1 (bf16x3 split operands).  Returns the previous one."""
    global _gemm
    prev, _gemm = _gemm, int(mode)
    return prev


def set_concurrent(flag):
    global _concurrent
    prev, _concurrent = _concurrent, 1 if flag else 0
    return prev


def set_device_seed(word):
    """word: int32 CUDA tensor [1] or None.  Returns the previous one."""
    global _seed_word
    prev, _seed_word = _seed_word, word
    return prev


def set_trace(handle):
    global _trace
    prev, _trace = _trace, handle
    return prev


SYNC_WORDS = 1024
_sync = {}
_sync_override = None
_have_gpu = None          # torch.cuda.is_available(), asked once (it reads the environment on every call)


def set_sync_override(words):
    """words: zeroed int32 CUDA tensor [SYNC_WORDS] that every call made from now on uses, or None.  Returns the previous one.
    graph.GraphedStep gives each captured graph its own (replays of two graphs may overlap on different streams)."""
    global _sync_override
    prev, _sync_override = _sync_override, words
    return prev


def sync_words(device=None):
    """The tick words of mmf_amil_desc::sync for calls issued on the CURRENT stream of `device`: one zeroed int32 tensor per
    (device, stream), made once and kept -- every call leaves the words zero, and calls that may overlap (other streams: bags in
    flight) get their own.  None while a stream is being captured without an override (the calls then run unsplit)."""
    if _sync_override is not None:
        return _sync_override
    global _have_gpu
    if device is not None and not isinstance(device, torch.device):
        device = torch.device(device)
    if device is not None and device.type != "cuda":
        return None                      # CPU tensors: the call itself raises MmfError (there is no CPU path)
    if _have_gpu is None:
        _have_gpu = torch.cuda.is_available()
    if not _have_gpu:
        return None
    if torch.cuda.is_current_stream_capturing():
        return None
    index = torch._C._cuda_getDevice() if device is None or device.index is None else device.index
    key = (index, torch._C._cuda_getCurrentRawStream(index))
    t = _sync.get(key)
    if t is None:
        t = _sync[key] = torch.zeros(SYNC_WORDS, dtype=torch.int32, device=torch.device("cuda", index))
    return t


def _amil_desc(stack, N, L, H, D, gated, p_h, p_att, seed, seed_word, concurrent=None):
    """The mmf_amil_desc of one call on stack = (W1, b1, Wa, ba, Wb, bb, Wc, bc).  concurrent: the hint a backward takes
    from its forward (default: the current one).  The scorer alone (W1 = None: mmf_attn_net_*) gets no tick words, and
    concurrent / gemm stay 0: those entry points read none of them."""
    W1, b1, Wa, ba, Wb, bb, Wc, bc = stack
    full = W1 is not None
    sw = sync_words(W1.device) if full else None
    return AmilDesc(sync=ptr(sw), sync_words=SYNC_WORDS if sw is not None else 0,
                    N=N, L=L, H=H, D=D, gated=1 if gated else 0,
                    W1=ptr(W1), b1=ptr(b1), Wa=ptr(Wa), ba=ptr(ba),
                    Wb=ptr(Wb) if gated else None, bb=ptr(bb) if gated else None,
                    Wc=ptr(Wc), bc=ptr(bc), p_h=float(p_h), p_att=float(p_att), seed=int(seed) & 0xFFFFFFFF,
                    seed_dev=ptr(seed_word), trace=_trace,
                    concurrent=(_concurrent if concurrent is None else concurrent) if full else 0, gemm=_gemm if full else 0)


def next_dropout_seed() -> int:
    """Per-call dropout seed: deterministic given torch.manual_seed(), no device sync."""
    global _drop_calls
    _drop_calls += 1
    return (torch.initial_seed() * 0x9E3779B1 + _drop_calls * 0x85EBCA6B) & 0xFFFFFFFF


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise _lib.MmfError(f"expected float32 tensor, got {t.dtype}")
    return t.contiguous()


def _stack_operands(stack, L, head=None, what="bag", fused_head=False):
    """stack (W1, b1, Wa, ba, Wb, bb, Wc, bc) and the classifier head (Wk, bk) behind it, if any, as contiguous fp32
    (model.half() / .double() must not reach the fp32 kernels), checked against the bag width L; fused_head: the head
    runs in the tail of the pooling merge kernel (K <= 32).  Returns (stack, head, H, D)."""
    stack = tuple(map(_f32c, stack))
    head = None if head is None else tuple(map(_f32c, head))
    W1, Wa, Wc = stack[0], stack[2], stack[6]
    H, D = W1.shape[0], Wa.shape[0]
    if (W1.shape[1] != L or Wa.shape[1] != H or Wc.numel() != D
            or head is not None and (head[0].shape[1] != H or fused_head and head[0].shape[0] > 32)):
        raise _lib.MmfError(f"attention stack {'' if head is None else '/ classifier '}shapes do not match the {what}")
    return stack, head, H, D


def _bag_operands(x, stack, gated, p_h, p_att, seed, seed_word, head=None, fused_head=False):
    """One bag x [N x L] and its stack for a call: a bf16 bag selects the bf16-storage kernels (include/mmf_amil.h:
    mmf_amil_bf16_*), the parameters stay fp32.  Returns (bf16, x, stack, head, the call's mmf_amil_desc)."""
    bf16 = x.dtype == torch.bfloat16
    x = x.contiguous() if bf16 else _f32c(x)
    if x.dim() != 2:
        raise _lib.MmfError(f"bag must be [N x L], got {tuple(x.shape)}")
    N, L = x.shape
    stack, head, H, D = _stack_operands(stack, L, head, "bag", fused_head)
    return bf16, x, stack, head, _amil_desc(stack, N, L, H, D, gated, p_h, p_att, seed, seed_word)


def _stack_workspace(d, bf16, dev, infer=False):
    """(bytes, uint8 tensor) of a one-bag call's workspace: the forward's size, or the no-save kernels' (infer)."""
    l = lib()
    if infer:
        query = l.mmf_amil_bf16_infer_workspace_bytes if bf16 else l.mmf_amil_infer_workspace_bytes
    else:
        query = l.mmf_amil_bf16_workspace_bytes if bf16 else l.mmf_amil_workspace_bytes
    nbytes = query(d.N, d.L, d.H, d.D, d.gated)
    return nbytes, torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _stack_grads(x, stack, gated, need_dx):
    """Fresh gradient buffers of a stack's backward -- None where the stack has no tensor (the scorer alone: W1, b1; an
    ungated stack: Wb, bb) -- and of the bag when need_dx.  Returns (the eight gradients, dx, their mmf_amil_grads)."""
    ds = tuple(None if t is None or not gated and i in (4, 5) else torch.empty_like(t) for i, t in enumerate(stack))
    dx = torch.empty_like(x) if need_dx else None
    return ds, dx, AmilGrads(*map(ptr, ds), ptr(dx))


def _check_dx(bf16, need_dx):
    if bf16 and need_dx:
        raise _lib.MmfError("a bf16 bag is a leaf: no input gradient on the bf16 path")


def _stack_fwd_raw(x, stack, gated, p_h=0.0, p_att=0.0, seed=0, head=None, infer=False, M_out=None):
    """`A, h = attention_net(x); A_raw = A.T; M = softmax(A_raw) @ h` (models/model_attention_mil_path.py:52-56) on one
    bag x [N x L] (fp32; bf16: the bf16-storage kernels) in one call: mmf_amil[_bf16]_infer (infer: nothing is kept for a
    backward), mmf_amil[_bf16]_forward, or with head = (Wk, bk) mmf_amil_head_forward, the classifier / hazard head (:58-61)
    in the tail of the pooling merge kernel (K > 32: the forward + mmf_surv_head_forward).  M_out: the [1 x H] tensor M goes
    to.  Returns (saved, hd, state) for _stack_bwd_raw: saved = (x, *stack, M, A_raw) as the kernels took them; hd = (Wk,
    bk, logits / hazards / S [3 x 1 x K], Y_hat) or None; state = (bf16, desc arguments, workspace, seed word, concurrent)
    as of this forward -- the backward runs later, on the autograd thread after the caller has lowered the hint."""
    word = None if infer else _seed_word
    bf16, x, stack, head, d = _bag_operands(x, stack, gated, p_h, p_att, seed, word, head)
    N, H = d.N, d.H
    dev = x.device
    nbytes, ws = _stack_workspace(d, bf16, dev, infer)
    M = torch.empty((1, H), dtype=torch.float32, device=dev) if M_out is None else M_out
    A_raw = torch.empty((1, N), dtype=torch.float32, device=dev)
    hd = None
    if head is not None:
        Wk, bk = head
        K = Wk.shape[0]
        out = torch.empty((3, 1, K), dtype=torch.float32, device=dev)        # logits, hazards, S
        Y_hat = torch.empty((1, 1), dtype=torch.int64, device=dev)
        hd = (Wk, bk, out, Y_hat)
    l = lib()
    if hd is not None and K <= 32:
        sh = SurvHead(Wk=ptr(Wk), bk=ptr(bk), K=K, logits=ptr(out[0]), hazards=ptr(out[1]), S=ptr(out[2]),
                      Y_hat=ptr(Y_hat), risk=None)
        check(l.mmf_amil_head_forward(C.byref(d), ptr(x), 1 if bf16 else 0, ptr(ws), nbytes, C.byref(sh), ptr(M),
                                      ptr(A_raw), stream_ptr()), "mmf_amil_head_forward")
    else:
        if infer:
            fwd_fn, name = ((l.mmf_amil_bf16_infer, "mmf_amil_bf16_infer") if bf16 else (l.mmf_amil_infer, "mmf_amil_infer"))
        else:
            fwd_fn, name = ((l.mmf_amil_bf16_forward, "mmf_amil_bf16_forward") if bf16
                            else (l.mmf_amil_forward, "mmf_amil_forward"))
        check(fwd_fn(C.byref(d), ptr(x), ptr(ws), nbytes, ptr(M), ptr(A_raw), stream_ptr()), name)
        if hd is not None:
            _surv_head_fwd_raw(M, Wk, bk, (out[0], out[1], out[2], Y_hat))
    return (x, *stack, M, A_raw), hd, (bf16, (N, d.L, H, d.D, gated, p_h, p_att, seed), ws, word, _concurrent)


def _stack_bwd_raw(saved, state, gM, gA, need_dx):
    """mmf_amil[_bf16]_backward of a _stack_fwd_raw call (saved, state: what it returned); gM, gA: the gradients of M and
    A_raw, None where none reaches it.  Returns (dx or None, the eight stack gradients: None for an ungated Wb, bb)."""
    x, *stack, M, A_raw = saved
    bf16, cfg, ws, word, concurrent = state
    _check_dx(bf16, need_dx)
    gM = torch.zeros((1, cfg[2]), dtype=torch.float32, device=x.device) if gM is None else _f32c(gM)
    gA = _f32c(gA)
    d = _amil_desc(stack, *cfg, word, concurrent)
    ds, dx, g = _stack_grads(x, stack, cfg[4], need_dx)
    bwd_fn, name = ((lib().mmf_amil_bf16_backward, "mmf_amil_bf16_backward") if bf16
                    else (lib().mmf_amil_backward, "mmf_amil_backward"))
    check(bwd_fn(C.byref(d), ptr(x), ptr(ws), ws.numel(), ptr(M), ptr(A_raw), ptr(gM), ptr(gA), C.byref(g), stream_ptr()),
          name)
    return dx, ds


class AmilPoolFn(torch.autograd.Function):
    """(x, attention-stack params) -> (M [1 x H], A_raw [1 x N]): _stack_fwd_raw / _stack_bwd_raw."""

    @staticmethod
    def forward(ctx, x, W1, b1, Wa, ba, Wb, bb, Wc, bc, gated, p_h, p_att, seed):
        saved, _, ctx.state = _stack_fwd_raw(x, (W1, b1, Wa, ba, Wb, bb, Wc, bc), gated, p_h, p_att, seed)
        ctx.save_for_backward(*saved)
        ctx.set_materialize_grads(False)      # an unused output (A_raw, mostly) must not cost a zero-fill launch
        return saved[-2], saved[-1]

    @staticmethod
    def backward(ctx, gM, gA):
        dx, ds = _stack_bwd_raw(ctx.saved_tensors, ctx.state, gM, gA, ctx.needs_input_grad[0])
        return (dx, *ds, None, None, None, None)


def amil_infer(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, gated):
    """Forward-only attention stack (include/mmf_amil.h: mmf_amil[_bf16]_infer): nothing is saved for a backward."""
    saved = _stack_fwd_raw(x, (W1, b1, Wa, ba, Wb, bb, Wc, bc), gated, infer=True)[0]
    return saved[-2], saved[-1]


def amil_pool(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, gated, p_h=0.0, p_att=0.0, seed=0):
    if not torch.is_grad_enabled() and p_h == 0.0 and p_att == 0.0:
        return amil_infer(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, gated)     # torch.no_grad() + eval: the inference consumers
    return AmilPoolFn.apply(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, gated, p_h, p_att, seed)


class AmilHeadFn(torch.autograd.Function):
    """Attention stack + classifier/hazard head as ONE autograd node (models/model_attention_mil_path.py:52-61):
    (x, stack params, Wk, bk) -> (hazards, S, Y_hat, A_raw).  Same kernels as AmilPoolFn + SurvHeadFn; one node less
    on a path where a 1k-10k bag step is bound by host dispatch."""

    @staticmethod
    def forward(ctx, x, W1, b1, Wa, ba, Wb, bb, Wc, bc, Wk, bk, gated, p_h, p_att, seed):
        saved, (Wk, _, out, Y_hat), ctx.state = _stack_fwd_raw(x, (W1, b1, Wa, ba, Wb, bb, Wc, bc), gated, p_h, p_att,
                                                               seed, head=(Wk, bk))
        ctx.save_for_backward(Wk, out, *saved)
        ctx.mark_non_differentiable(Y_hat)
        ctx.set_materialize_grads(False)      # no zero-fill launches for the outputs the loss does not use (A_raw, Y_hat)
        return out[1], out[2], Y_hat, saved[-1]

    @staticmethod
    def backward(ctx, gH, gS, _gY, gA):
        Wk, out, *saved = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        _check_dx(ctx.state[0], need_dx)
        dM, dWk, dbk = _surv_head_bwd_raw(gH, gS, out[1], saved[-2], Wk)
        dx, ds = _stack_bwd_raw(saved, ctx.state, dM, gA, need_dx)
        return (dx, *ds, dWk, dbk, None, None, None, None)


def _check_grad_buffers(pairs):
    for g_, w_ in pairs:
        if g_ is None or g_.dtype != torch.float32 or g_.shape != w_.shape or not g_.is_contiguous():
            raise _lib.MmfError("gradient buffers must be contiguous float32 tensors shaped like their parameters")


def _step_grads(stack, Wk, bk, gated, grads):
    """The gradient buffers grads (dW1, ..., dbc, dWk, dbk) of a one-call step, checked against the stack and classifier
    (_stack_operands).  Returns their AmilGrads, with no dx."""
    W1, b1, Wa, ba, Wb, bb, Wc, bc = stack
    dW1, db1, dWa, dba, dWb, dbb, dWc, dbc, dWk, dbk = grads
    _check_grad_buffers(((dW1, W1), (db1, b1), (dWa, Wa), (dba, ba), (dWc, Wc), (dbc, bc), (dWk, Wk), (dbk, bk)) +
                        (((dWb, Wb), (dbb, bb)) if gated else ()))
    return AmilGrads(dW1=ptr(dW1), db1=ptr(db1), dWa=ptr(dWa), dba=ptr(dba), dWb=ptr(dWb) if gated else None,
                     dbb=ptr(dbb) if gated else None, dWc=ptr(dWc), dbc=ptr(dbc), dx=None)


def _nll_head(Wk, bk, Y, c, alpha, eps, loss_scale, dWk, dbk, accumulate, dev, G=0):
    """The classifier + hazards + nll_surv part of a one-call step: labels / censorships on the device, the outputs and
    the SurvHead / NllTarget structs.  G = 0: one bag (Y, c: one value each; the outputs share one buffer); G > 0: G bags
    (Y, c: [G] each).  A forward-only call passes no gradient buffers (dWk = dbk = None) and may pass no labels (Y = None:
    no NllTarget, no loss); on purpose its out-of-range host labels go through to a NaN loss, as mmf_nll_surv's, where
    a training step raises.  Returns (hd, tg, (hazards, S, Y_hat, loss, risk), keep); keep holds the other tensors the
    structs point to (the device Y, c and the logits), which must stay alive until the launch."""
    K = Wk.shape[0]
    if dWk is not None and not Y.is_cuda and bool(((Y < 0) | (Y >= K)).any()):
        raise IndexError(f"nll_surv: label out of range [0, {K})")
    if G:
        logits, hz, S = (torch.empty((G, K), dtype=torch.float32, device=dev) for _ in range(3))
        risk = torch.empty((G,), dtype=torch.float32, device=dev)
        if Y is not None:
            Y = Y.to(device=dev, dtype=torch.int64).contiguous()
            c = c.to(device=dev, dtype=torch.float32).contiguous()
            loss = torch.empty((G,), dtype=torch.float32, device=dev)
    else:
        Y = Y.reshape(1).to(device=dev, dtype=torch.int64)
        c = c.reshape(1).to(device=dev, dtype=torch.float32)
        out = torch.empty((3 * K + 2,), dtype=torch.float32, device=dev)       # logits, hazards, S, loss, risk
        logits, hz, S = out[0:K], out[K:2 * K].view(1, K), out[2 * K:3 * K].view(1, K)
        loss, risk = out[3 * K].view(()), out[3 * K + 1:].view(1)
    Y_hat = torch.empty((G or 1, 1), dtype=torch.int64, device=dev)
    hd = SurvHead(Wk=ptr(Wk), bk=ptr(bk), K=K, logits=ptr(logits), hazards=ptr(hz), S=ptr(S), Y_hat=ptr(Y_hat),
                  risk=ptr(risk))
    if Y is None:
        return hd, None, (hz, S, Y_hat, None, risk), (logits,)
    tg = NllTarget(Y=ptr(Y), c=ptr(c), alpha=float(alpha), eps=float(eps), loss_scale=float(loss_scale),
                   loss=ptr(loss), dWk=ptr(dWk), dbk=ptr(dbk), accumulate=1 if accumulate else 0)
    return hd, tg, (hz, S, Y_hat, loss, risk), (Y, c, logits)


def amil_nll_step(x, stack, Wk, bk, gated, Y, c, alpha, grads, loss_scale=1.0, accumulate=False, p_h=0.0, p_att=0.0,
                  seed=0, eps=1e-7, dx=None):
    """(dx: optional [N x L] fp32 tensor that receives d(loss * loss_scale)/dx -- the radio head, whose bag is
    reduce_dim's output.)
    One bag's whole training step in ONE C-ABI call (include/mmf_amil.h: mmf_amil_nll_step): attention stack +
    classifier / hazard head + nll_surv + backward.  No autograd graph is built.

    stack = (W1, b1, Wa, ba, Wb, bb, Wc, bc); grads = the matching gradient tensors (dW1, db1, dWa, dba, dWb, dbb, dWc,
    dbc, dWk, dbk), written with d(loss * loss_scale) -- added to when `accumulate`.  Y, c: device tensors [1].
    Returns (hazards [1 x K], S [1 x K], Y_hat [1 x 1], A_raw [1 x N], loss (0-dim, unscaled), risk [1])."""
    bf16, x, stack, (Wk, bk), d = _bag_operands(x, stack, gated, p_h, p_att, seed, _seed_word, (Wk, bk), fused_head=True)
    g = _step_grads(stack, Wk, bk, gated, grads)
    dev = x.device
    hd, tg, (hz, S, Y_hat, loss, risk), _keep = _nll_head(Wk, bk, Y, c, alpha, eps, loss_scale, grads[8], grads[9],
                                                          accumulate, dev)
    nbytes, ws = _stack_workspace(d, bf16, dev)
    A_raw = torch.empty((1, d.N), dtype=torch.float32, device=dev)
    if dx is not None and (bf16 or dx.dtype != torch.float32 or dx.shape != x.shape or not dx.is_contiguous()):
        raise _lib.MmfError("dx must be a contiguous float32 tensor shaped like an fp32 bag")
    g.dx = ptr(dx)
    check(lib().mmf_amil_nll_step(C.byref(d), ptr(x), 1 if bf16 else 0, ptr(ws), nbytes, C.byref(hd), C.byref(tg),
                                  ptr(A_raw), C.byref(g), stream_ptr()), "mmf_amil_nll_step")
    return hz, S, Y_hat, A_raw, loss, risk


GROUP_MAX = 64       # include/mmf_amil.h: MMF_GROUP_MAX


def group_row_limit(L, H, D):
    """Most rows one grouped call takes (the single-bag limits of include/mmf_amil.h applied to sum N: 32-bit mask
    indices, every [sum N x *] operand < 2 GiB, pooling groups of <= 8192 rows)."""
    return min(((1 << 32) - 1) // max(H, D), ((1 << 31) - 1) // (4 * max(L, H, 2 * D)), 256 * 8192)


def radio_group_row_limit(nseg, L, H, D):
    """Most rows one grouped radio call takes: group_row_limit of the stack, and the [sum N x nseg * L] input of
    reduce_dim < 2 GiB (131,071 rows at four 1024-wide modalities)."""
    return min(group_row_limit(L, H, D), ((1 << 31) - 1) // (4 * nseg * L))


def _group_table(sizes, rows, Y, c, seeds=None, train=True, labels=True):
    """The bag table of a grouped call: sizes checked against the rows given, G labels / censorships (None: a forward-only
    call without a loss; labels=False: a stack half of the multimodal step, whose labels go to the head) and, for a
    training call, G dropout seeds (a forward-only table carries none).
    Returns (sizes, Y, c, offsets (host int64 [G + 1]), BagGroup); the BagGroup points into the offsets and seeds arrays,
    which it keeps alive as attributes."""
    sizes = [int(n) for n in sizes]
    G = len(sizes)
    if G < 1 or G > GROUP_MAX:
        raise _lib.MmfError(f"a group holds 1 .. {GROUP_MAX} bags, got {G}")
    if min(sizes) < 1:
        raise _lib.MmfError("empty bag in the group")
    if rows is not None and rows != sum(sizes):
        raise _lib.MmfError(f"the bags hold {rows} rows, their sizes add up to {sum(sizes)}")
    if Y is not None or train and labels:
        Y = torch.as_tensor(Y).reshape(-1)
        c = torch.as_tensor(c).reshape(-1)
        if Y.numel() != G or c.numel() != G:
            raise _lib.MmfError(f"{G} bags need {G} labels and censorships, got {Y.numel()} / {c.numel()}")
    sd = None
    if train:
        seeds = [0] * G if seeds is None else [int(v) & 0xFFFFFFFF for v in seeds]
        if len(seeds) != G:
            raise _lib.MmfError(f"{G} bags need {G} dropout seeds")
        sd = (C.c_uint32 * G)(*seeds)
    offs = (C.c_int64 * (G + 1))()
    for i, n in enumerate(sizes):
        offs[i + 1] = offs[i] + n
    grp = _lib.BagGroup(G=G, offsets=offs, seeds=sd)
    grp._keep = (offs, sd)
    return sizes, Y, c, offs, grp


def bag_gather(planes, dst):
    """mmf_bag_gather: the bags of a grouped window, each contiguous somewhere in HBM, into the leading rows of one
    matrix per plane, in ONE launch on the current stream.  planes: n_plane (1 .. 4) lists of the same G bags' tensors
    ([n_g x L], fp32 or bf16, one type for all); dst: n_plane tensors [rows >= sum n_g x L] of row pitch L (or one
    [n_plane x rows x L] tensor), fp32 or bf16: the storage type is converted on the way (narrowing rounds to nearest
    even, as tensor.to(torch.bfloat16)).  Rows of dst beyond sum n_g are left alone.  Returns the bags' sizes."""
    planes = [list(p) for p in planes]
    dst = list(dst)
    nplane, G = len(planes), len(planes[0]) if planes else 0
    if nplane < 1 or nplane > 4 or len(dst) != nplane or any(len(p) != G for p in planes):
        raise _lib.MmfError(f"bag_gather takes 1 .. 4 planes of the same bags and one destination each, got {nplane} / {len(dst)}")
    if G < 1 or G > GROUP_MAX:
        raise _lib.MmfError(f"a group holds 1 .. {GROUP_MAX} bags, got {G}")
    store = {torch.float32: 0, torch.bfloat16: 1}
    sdt, ddt, L = planes[0][0].dtype, dst[0].dtype, int(dst[0].shape[-1])
    if sdt not in store or ddt not in store:
        raise _lib.MmfError(f"bag_gather moves fp32 and bf16 bags, got {sdt} -> {ddt}")
    sizes = [int(x.shape[0]) for x in planes[0]]
    for p in planes:
        if any(x.dim() != 2 or x.dtype != sdt or int(x.shape[1]) != L for x in p) or [int(x.shape[0]) for x in p] != sizes:
            raise _lib.MmfError(f"every plane holds the same [n_g x {L}] bags of one storage type")
    rows = sum(sizes)
    if any(d.dim() != 2 or d.dtype != ddt or int(d.shape[1]) != L or int(d.shape[0]) < rows for d in dst):
        raise _lib.MmfError(f"every destination is [>= {rows} x {L}] of one storage type")
    offs = (C.c_int64 * (G + 1))()
    for i, n in enumerate(sizes):
        offs[i + 1] = offs[i] + n
    src = (C.c_void_p * (nplane * G))(*[ptr(x) for p in planes for x in p])
    out = (C.c_void_p * nplane)(*[ptr(d) for d in dst])
    check(lib().mmf_bag_gather(offs, G, nplane, src, out, L, store[sdt], store[ddt], stream_ptr()), "mmf_bag_gather")
    return sizes


def _radio_operands(xs, Wr, br, kind, dWr=None, dbr=None):
    """The modality tensors xs (2 .. 4, each [sum N x k] fp32) and reduce_dim (Wr [k x nseg k], br [k]; dWr, dbr: its
    gradient buffers, None for a forward-only call) of a grouped radio `kind` ("step" / "pass"), checked.
    Returns (xs, R, nseg, k, RadioReduce)."""
    xs = list(xs)
    nseg = len(xs)
    if nseg < 2 or nseg > 4:
        raise _lib.MmfError(f"the grouped radio {kind} takes 2 .. 4 modalities, got {nseg}")
    if any(x.dtype != torch.float32 for x in xs):
        raise _lib.MmfError(f"the grouped {'step' if kind == 'step' else 'radio pass'} takes fp32 bags only")
    xs = [_f32c(x) for x in xs]
    if any(x.dim() != 2 or tuple(x.shape) != tuple(xs[0].shape) for x in xs):
        raise _lib.MmfError("every modality must be one [sum N x k] tensor of the same shape")
    R, kseg = xs[0].shape
    Wr, br = _f32c(Wr), _f32c(br)
    if tuple(Wr.shape) != (kseg, nseg * kseg) or tuple(br.shape) != (kseg,):
        raise _lib.MmfError(f"reduce_dim must be [{kseg} x {nseg * kseg}] with a [{kseg}] bias for {nseg} modalities of {kseg}")
    if kind == "step":
        _check_grad_buffers(((dWr, Wr), (dbr, br)))
    segs = (C.c_void_p * nseg)(*[ptr(x) for x in xs])
    return xs, R, nseg, kseg, _lib.RadioReduce(x=segs, nseg=nseg, kseg=kseg, W=ptr(Wr), bias=ptr(br), dW=ptr(dWr),
                                               db=ptr(dbr))


def _run_group(query, qargs, name, d, grp, lead, hd, tg, tail, A_raw, sizes):
    """One grouped C-ABI call: the workspace of `query`(*qargs), then `name`(desc, group, *lead, workspace, bytes, head,
    target, *tail, stream).  Returns A_raw split per bag: [1 x N_g] views."""
    l = lib()
    nbytes = getattr(l, query)(*qargs)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=A_raw.device)
    check(getattr(l, name)(C.byref(d), C.byref(grp), *lead, ptr(ws), nbytes, hd and C.byref(hd), tg and C.byref(tg), *tail,
                           stream_ptr()), name)
    return [v.view(1, -1) for v in torch.split(A_raw, sizes)]


def amil_nll_step_group(x_cat, sizes, stack, Wk, bk, gated, Y, c, alpha, grads, loss_scale=1.0, accumulate=False, p_h=0.0,
                        p_att=0.0, seeds=None, eps=1e-7):
    """The G bags of one accumulation window in ONE C-ABI call (include/mmf_amil.h: mmf_amil_nll_step_group): the stack's
    GEMMs run once over the concatenated rows, pooling / head / loss per bag.  x_cat: [sum N x L] fp32, the bags' rows in
    order; sizes: the G bag sizes (host ints); Y, c: G labels / censorships; seeds: G dropout seeds (train mode).
    grads as amil_nll_step: those of sum_g loss_g * loss_scale, added to when `accumulate`.
    Returns (hazards [G x K], S [G x K], Y_hat [G x 1], [A_raw of bag g: [1 x N_g] views of one buffer], loss [G]
    (unscaled), risk [G])."""
    if x_cat.dtype != torch.float32:
        raise _lib.MmfError("the grouped step takes fp32 bags only (bf16 bags: one amil_nll_step per bag)")
    x_cat = _f32c(x_cat)
    sizes, Y, c, offs, grp = _group_table(sizes, None, Y, c, seeds)
    G = len(sizes)
    if x_cat.dim() != 2 or x_cat.shape[0] != sum(sizes):
        raise _lib.MmfError(f"x_cat must be [sum N x L] = [{sum(sizes)} x L], got {tuple(x_cat.shape)}")
    R, L = x_cat.shape
    stack, (Wk, bk), H, D = _stack_operands(stack, L, (Wk, bk), "bags", fused_head=True)
    g = _step_grads(stack, Wk, bk, gated, grads)
    dev = x_cat.device
    hd, tg, (hz, S, Y_hat, loss, risk), _keep = _nll_head(Wk, bk, Y, c, alpha, eps, loss_scale, grads[8], grads[9],
                                                          accumulate, dev, G)
    d = _amil_desc(stack, R, L, H, D, gated, p_h, p_att, 0, _seed_word)
    A_raw = torch.empty((R,), dtype=torch.float32, device=dev)
    A_list = _run_group("mmf_amil_group_workspace_bytes", (offs, G, L, H, D, d.gated), "mmf_amil_nll_step_group", d, grp,
                        (ptr(x_cat),), hd, tg, (ptr(A_raw), C.byref(g)), A_raw, sizes)
    return hz, S, Y_hat, A_list, loss, risk


def radio_nll_step_group(xs, sizes, Wr, br, stack, Wk, bk, gated, Y, c, alpha, grads, loss_scale=1.0, accumulate=False,
                         p_h=0.0, p_att=0.0, seeds=None, eps=1e-7):
    """The radiology head's G bags of one accumulation window in ONE C-ABI call (include/mmf_amil.h:
    mmf_radio_nll_step_group): reduce_dim over the modality segments and the stack's GEMMs run once over all rows,
    pooling / head / loss per bag, reduce_dim's backward on the stack's TN and reduce launches.
    xs: 2 .. 4 modality tensors, each [sum N x k] fp32 (the bags' rows in order); sizes: the G bag sizes; Wr, br:
    reduce_dim's weight [L x nseg k] and bias [L]; grads = (dWr, dbr, dW1, ..., dbk), those of sum_g loss_g * loss_scale,
    added to when `accumulate`.  Other arguments as amil_nll_step_group.
    Returns (hazards [G x K], S [G x K], Y_hat [G x 1], [A_raw [1 x N_g]], loss [G] (unscaled), risk [G])."""
    xs, R, nseg, kseg, rd = _radio_operands(xs, Wr, br, "step", *grads[:2])
    sizes, Y, c, offs, grp = _group_table(sizes, R, Y, c, seeds)
    G = len(sizes)
    stack, (Wk, bk), H, D = _stack_operands(stack, kseg, (Wk, bk), "bags", fused_head=True)
    g = _step_grads(stack, Wk, bk, gated, grads[2:])
    dev = xs[0].device
    hd, tg, (hz, S, Y_hat, loss, risk), _keep = _nll_head(Wk, bk, Y, c, alpha, eps, loss_scale, grads[10], grads[11],
                                                          accumulate, dev, G)
    d = _amil_desc(stack, R, kseg, H, D, gated, p_h, p_att, 0, _seed_word)
    A_raw = torch.empty((R,), dtype=torch.float32, device=dev)
    A_list = _run_group("mmf_radio_group_workspace_bytes", (offs, G, nseg, kseg, H, D, d.gated), "mmf_radio_nll_step_group",
                        d, grp, (C.byref(rd),), hd, tg, (ptr(A_raw), C.byref(g)), A_raw, sizes)
    return hz, S, Y_hat, A_list, loss, risk


def mm_group_row_limits(path=None, radio=None):
    """The row limits of one grouped multimodal window (MM_MIL_Attention_fc_surv.nll_step_group): (pathology rows, radio
    rows) one call takes, None for a branch that is not given.  path: (L, H, D) of the pathology stack; radio: (nseg, L, H,
    D) of the radio stack behind reduce_dim (nseg = 1: no reduce_dim, the pathology limit of that stack)."""
    lim_p = None if path is None else group_row_limit(*path)
    lim_r = None
    if radio is not None:
        nseg, L, H, D = radio
        lim_r = group_row_limit(L, H, D) if nseg == 1 else radio_group_row_limit(nseg, L, H, D)
    return lim_p, lim_r


def _rows_ptr(t, what):
    """(device pointer, leading dimension in floats) of a [B x N] fp32 device tensor whose rows are contiguous: a plain
    matrix, or some columns of a wider one (a branch's slot of the fused feature matrix)."""
    if t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise _lib.MmfError(f"{what} must be a [B x N] float32 tensor with contiguous rows")
    return ptr(t[0]), max(int(t.stride(0)), int(t.shape[1]))


def _group_half_fwd_raw(xs, sizes, stack, gated, p_h, p_att, seeds, M_out, Wr=None, br=None):
    """The forward half of a grouped stack chain (mmf_amil_group_forward; with reduce_dim Wr, br over several modality
    tensors xs: mmf_radio_group_forward): the window's rows through the stack, bag g's pooled embedding into row g of
    M_out (a [G x H] tensor or H columns of a wider one).  xs: [x_cat [sum N x L]] or 2 .. 4 modality tensors.
    Returns ([A_raw [1 x N_g]], state); state is what _group_half_bwd_raw takes."""
    radio = len(xs) > 1
    if any(x.dtype != torch.float32 for x in xs):
        raise _lib.MmfError("the grouped step takes fp32 bags only")
    if radio:
        xs, R, nseg, L, rd = _radio_operands(xs, Wr, br, "pass")
        Wr, br = _f32c(Wr), _f32c(br)
    else:
        xs = [_f32c(xs[0])]
        if xs[0].dim() != 2:
            raise _lib.MmfError(f"x_cat must be [sum N x L], got {tuple(xs[0].shape)}")
        R, L = xs[0].shape
        nseg = 1
    sizes, _, _, offs, grp = _group_table(sizes, R, None, None, seeds, train=True, labels=False)
    G = len(sizes)
    stack, _, H, D = _stack_operands(stack, L, None, "bags")
    mp, ldm = _rows_ptr(M_out, "M_out")
    if M_out.shape[0] != G or M_out.shape[1] != H:
        raise _lib.MmfError(f"M_out must be [{G} x {H}], got {tuple(M_out.shape)}")
    word = _seed_word
    d = _amil_desc(stack, R, L, H, D, gated, p_h, p_att, 0, word)
    dev = xs[0].device
    A_raw = torch.empty((R,), dtype=torch.float32, device=dev)
    l = lib()
    if radio:
        nbytes = l.mmf_radio_group_workspace_bytes(offs, G, nseg, L, H, D, d.gated)
    else:
        nbytes = l.mmf_amil_group_workspace_bytes(offs, G, L, H, D, d.gated)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if radio:
        check(l.mmf_radio_group_forward(C.byref(d), C.byref(grp), C.byref(rd), ptr(ws), nbytes, mp, ldm, ptr(A_raw),
                                        stream_ptr()), "mmf_radio_group_forward")
    else:
        check(l.mmf_amil_group_forward(C.byref(d), C.byref(grp), ptr(xs[0]), ptr(ws), nbytes, mp, ldm, ptr(A_raw),
                                       stream_ptr()), "mmf_amil_group_forward")
    state = (xs, sizes, stack, gated, (R, L, H, D, gated, p_h, p_att, 0), ws, word, grp, A_raw, Wr, br)
    return [v.view(1, -1) for v in torch.split(A_raw, sizes)], state


def _group_half_bwd_raw(state, dM):
    """The backward half of a _group_half_fwd_raw call (mmf_amil_group_backward / mmf_radio_group_backward) from dM: a
    [G x H] tensor or H columns of a wider one (the stack's slot of the head's dfeat).  Returns the stack's eight fresh
    gradients (None for an ungated Wb, bb) of sum_g loss_g, and (dWr, dbr) or None."""
    xs, sizes, stack, gated, cfg, ws, word, grp, A_raw, Wr, br = state
    dp, ldm = _rows_ptr(dM, "dM")
    if dM.shape[0] != len(sizes) or dM.shape[1] != cfg[2]:
        raise _lib.MmfError(f"dM must be [{len(sizes)} x {cfg[2]}], got {tuple(dM.shape)}")
    d = _amil_desc(stack, *cfg, word)
    ds, _, g = _stack_grads(xs[0], stack, gated, False)
    l = lib()
    if len(xs) > 1:
        dWr, dbr = torch.empty_like(Wr), torch.empty_like(br)
        rd = _radio_operands(xs, Wr, br, "step", dWr, dbr)[4]
        check(l.mmf_radio_group_backward(C.byref(d), C.byref(grp), C.byref(rd), ptr(ws), ws.numel(), dp, ldm, ptr(A_raw),
                                         C.byref(g), 0, stream_ptr()), "mmf_radio_group_backward")
        return ds, (dWr, dbr)
    check(l.mmf_amil_group_backward(C.byref(d), C.byref(grp), ptr(xs[0]), ptr(ws), ws.numel(), dp, ldm, ptr(A_raw),
                                    C.byref(g), 0, stream_ptr()), "mmf_amil_group_backward")
    return ds, None


def surv_head_nll_step_group(feat, Wk, bk, Y, c, alpha, dWk, dbk, loss_scale=1.0, accumulate=False, eps=1e-7):
    """surv_head_nll_step for the G patients of one accumulation window (mmf_surv_head_nll_step_group): feat [G x F]
    (F <= 1024, G <= GROUP_MAX), one workgroup per patient and one reduce launch; Y, c: G labels / censorships.  dWk / dbk
    get the gradient of sum_g loss_g * loss_scale (added when `accumulate`).
    Returns (hazards [G x K], S [G x K], Y_hat [G x 1], loss [G] (unscaled), risk [G], dfeat [G x F]), detached."""
    Wk, bk = _f32c(Wk), _f32c(bk)
    fp, ldf = _rows_ptr(feat, "feat")
    G, F = feat.shape
    K = Wk.shape[0]
    if G < 1 or G > GROUP_MAX:
        raise _lib.MmfError(f"a group holds 1 .. {GROUP_MAX} patients, got {G}")
    if Wk.shape[1] != F or F > 1024 or K > 32:
        raise _lib.MmfError("surv_head_nll_step_group: classifier does not match the feature matrix (F <= 1024, K <= 32)")
    _check_grad_buffers(((dWk, Wk), (dbk, bk)))
    Y = torch.as_tensor(Y).reshape(-1)
    c = torch.as_tensor(c).reshape(-1)
    if Y.numel() != G or c.numel() != G:
        raise _lib.MmfError(f"{G} patients need {G} labels and censorships, got {Y.numel()} / {c.numel()}")
    dev = feat.device
    hd, tg, (hz, S, Y_hat, loss, risk), _keep = _nll_head(Wk, bk, Y, c, alpha, eps, loss_scale, dWk, dbk, accumulate, dev, G)
    dfeat = torch.empty((G, F), dtype=torch.float32, device=dev)
    l = lib()
    nbytes = l.mmf_surv_head_group_workspace_bytes(F, K, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(l.mmf_surv_head_nll_step_group(fp, ldf, F, G, C.byref(hd), C.byref(tg), ptr(dfeat), ptr(ws), nbytes, stream_ptr()),
          "mmf_surv_head_nll_step_group")
    return hz, S, Y_hat, loss, risk, dfeat


_HASH_MUL_INV = pow(0x9E3779B1, -1, 1 << 32)       # mmf_dropout_row_base: the inverse of the keep-hash's index multiplier


def dropout_row_base(seeds, device):
    """The per-row mask index bases of a dense batch whose row b draws with seeds[b] (mmf_dense_forward_rows): an int32
    device tensor [B] holding seed_b * inverse(0x9E3779B1) mod 2^32."""
    vals = [((int(v) & 0xFFFFFFFF) * _HASH_MUL_INV) & 0xFFFFFFFF for v in seeds]
    return torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in vals], dtype=torch.int32).to(device)


def _dense_rows_fwd_raw(x, W, b, act, kind, p, site, row_base, word=None, out=None):
    """_dense_fwd_raw on a batch whose row b draws the mask of its own seed (mmf_dense_forward_rows; row_base:
    dropout_row_base of the seeds).  out: a [B x N] tensor or N columns of a wider one."""
    B, K = x.shape
    N = W.shape[0]
    y = torch.empty((B, N), dtype=torch.float32, device=x.device) if out is None else out
    yp, ldy = _rows_ptr(y, "out")
    if tuple(y.shape) != (B, N) or row_base.numel() != B:
        raise _lib.MmfError(f"dense rows: out must be [{B} x {N}] and row_base [{B}]")
    check(lib().mmf_dense_forward_rows(ptr(x), ptr(W), ptr(b), B, K, N, ACT[act], DROP_KIND[kind], float(p), int(site),
                                       ptr(word), ptr(row_base), yp, ldy, stream_ptr()), "mmf_dense_forward_rows")
    return y


def _dense_rows_bwd_raw(gy, y, x, W, has_bias, act, kind, p, site, row_base, need_dx=True, word=None):
    """(dx, dW, db) of a _dense_rows_fwd_raw call (mmf_dense_backward_rows); gy and y may be columns of wider matrices."""
    B, K = x.shape
    N = W.shape[0]
    gp, ldg = _rows_ptr(gy, "gy")
    yp, ldy = _rows_ptr(y, "y")
    dpre = torch.empty((B, N), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if need_dx else None
    dW = torch.empty_like(W)
    db = torch.empty((N,), dtype=torch.float32, device=x.device) if has_bias else None
    check(lib().mmf_dense_backward_rows(gp, ldg, yp, ldy, ptr(x), ptr(W), B, K, N, ACT[act], DROP_KIND[kind], float(p),
                                        int(site), ptr(word), ptr(row_base), ptr(dpre), ptr(dx), ptr(dW), ptr(db),
                                        stream_ptr()), "mmf_dense_backward_rows")
    return dx, dW, db


def infer_group_row_limit(L, H, D, bf16=False):
    """Most rows one forward-only grouped call takes (ops.amil_infer_group): group_row_limit, with the [sum N x *]
    operands of a bf16 window two bytes wide."""
    if not bf16:
        return group_row_limit(L, H, D)
    return min(((1 << 32) - 1) // max(H, D), ((1 << 31) - 1) // (2 * max(L, H, 2 * D)), 256 * 8192)


def infer_group_takes_bf16(gated, H, D):
    """Whether ops.amil_infer_group takes bf16 bags on this stack.  It runs the unfused bf16 kernels; a gated stack with
    H = D = 256 (the `small` head) takes the fused forward forms one bag at a time, which round differently, so the C ABI
    refuses its bf16 windows (MMF_ERR_SHAPE) and such bags are evaluated one at a time."""
    return not (gated and H == 256 and D == 256)


def radio_infer_group_row_limit(nseg, L, H, D):
    """Most rows one forward-only grouped radio call takes (ops.radio_infer_group): radio_group_row_limit."""
    return radio_group_row_limit(nseg, L, H, D)


def _infer_operands(stack, L, Wk, bk, Y, c, alpha, eps, want_M, G, dev):
    """The stack, the optional classifier (Wk = None: M only) and the per-bag outputs of a forward-only grouped call.
    Returns (stack, H, D, hd, tg, (hazards, S, Y_hat, loss, risk), M, keep); hd, tg and the outputs are None where not
    asked for."""
    stack, head, H, D = _stack_operands(stack, L, None if Wk is None else (Wk, bk), "bags", fused_head=True)
    if head is None and not want_M:
        raise _lib.MmfError("nothing to compute: give the classifier or ask for M")
    if head is None and Y is not None:
        raise _lib.MmfError("a loss needs the classifier head")
    M = torch.empty((G, H), dtype=torch.float32, device=dev) if want_M else None
    if head is None:
        return stack, H, D, None, None, (None,) * 5, M, ()
    hd, tg, outs, keep = _nll_head(*head, Y, c, alpha, eps, 1.0, None, None, False, dev, G)
    return stack, H, D, hd, tg, outs, M, keep


def amil_infer_group(x_cat, sizes, stack, gated, Wk=None, bk=None, Y=None, c=None, alpha=0.0, want_M=False, eps=1e-7):
    """G bags evaluated with fixed weights in ONE C-ABI call (include/mmf_amil.h: mmf_amil_infer_group): the stack's
    GEMMs run once over the concatenated rows, pooling and the head per bag; nothing is saved for a backward, no dropout.
    x_cat: [sum N x L], fp32 or bf16 (the bf16-storage kernels), the bags' rows in order; sizes: the G bag sizes (host
    ints; bf16 only where infer_group_takes_bf16); Wk, bk: the classifier (K <= 32), or None for M only; Y, c: G labels /
    censorships for each bag's
    NLLSurvLoss(alpha) value, or None.  Returns (hazards [G x K], S [G x K], Y_hat [G x 1], risk [G], [A_raw of bag g:
    [1 x N_g] views of one buffer], M [G x H] or None, loss [G] or None); the head outputs are None without a head."""
    bf16 = x_cat.dtype == torch.bfloat16
    x_cat = x_cat.contiguous() if bf16 else _f32c(x_cat)
    if x_cat.dim() != 2:
        raise _lib.MmfError(f"x_cat must be [sum N x L], got {tuple(x_cat.shape)}")
    R, L = x_cat.shape
    sizes, Y, c, offs, grp = _group_table(sizes, R, Y, c, train=False)
    G, dev = len(sizes), x_cat.device
    stack, H, D, hd, tg, (hz, S, Y_hat, loss, risk), M, _keep = _infer_operands(stack, L, Wk, bk, Y, c, alpha, eps, want_M,
                                                                                G, dev)
    d = _amil_desc(stack, R, L, H, D, gated, 0.0, 0.0, 0, None)
    A_raw = torch.empty((R,), dtype=torch.float32, device=dev)
    A_list = _run_group("mmf_amil_group_infer_workspace_bytes", (offs, G, L, H, D, d.gated, 1 if bf16 else 0),
                        "mmf_amil_infer_group", d, grp, (ptr(x_cat), 1 if bf16 else 0), hd, tg, (ptr(M), ptr(A_raw)), A_raw,
                        sizes)
    return hz, S, Y_hat, risk, A_list, M, loss


IG_METHODS = ("gausslegendre", "riemann_trapezoid", "riemann_middle")


def ig_quadrature(method, n_steps):
    """(nodes, weights) of an n_steps-point rule on [0, 1], float64 numpy arrays: `gausslegendre` (captum's default, what
    the reference's create_attributions.py gets), `riemann_trapezoid` (nodes linspace(0, 1, n), the end weights halved;
    n >= 2) or `riemann_middle` (midpoints, equal weights).  The weights sum to 1."""
    import numpy as np
    n = int(n_steps)
    if n < 1 or n > GROUP_MAX:
        raise ValueError(f"n_steps must be in 1..{GROUP_MAX}, got {n_steps}")
    if method == "gausslegendre":
        t, w = np.polynomial.legendre.leggauss(n)
        return 0.5 * (1.0 + t), 0.5 * w
    if method == "riemann_trapezoid":
        if n < 2:
            raise ValueError("riemann_trapezoid needs n_steps >= 2")
        w = np.full(n, 1.0 / (n - 1))
        w[0] *= 0.5
        w[-1] *= 0.5
        return np.linspace(0.0, 1.0, n), w
    if method == "riemann_middle":
        return (np.arange(n) + 0.5) / n, np.full(n, 1.0 / n)
    raise ValueError(f"method must be one of {IG_METHODS}, got {method!r}")


def _integrated_gradients(name, dims, lead, ranged, stack, H, D, gated, Wk, bk, alphas, weights, want_attr, window_steps,
                          dev):
    """What both integrated-gradients calls do once their operands are prepared.  name: the entry point; dims: the leading
    arguments of its workspace query, (N, L) or (N, nseg, kseg), whose middle ones are the leading extents of the row sums
    and of attr; lead: the call's arguments between the descriptor and the workspace; ranged: what the query's refusal
    names as out of range."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).astype(np.float32))
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).astype(np.float32))
    if a.ndim != 1 or a.shape != w.shape or not 1 <= a.size <= GROUP_MAX:
        raise _lib.MmfError(f"alphas / weights: two sequences of 1..{GROUP_MAX} values each")
    n = int(a.size)
    N, ext, L = dims[0], tuple(dims[1:-1]), dims[-1]
    d = _amil_desc(stack, N, L, H, D, gated, 0.0, 0.0, 0, None)
    l = lib()
    nbytes = getattr(l, name + "_workspace_bytes")(*dims, H, D, d.gated, n, int(window_steps))
    if nbytes == 0:
        raise _lib.MmfError(f"{name}: n_steps, window_steps{ranged} or the bag's size out of range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rows = torch.empty((2,) + ext + (N,), dtype=torch.float32, device=dev)
    attr = torch.empty(ext + (N, L), dtype=torch.float32, device=dev) if want_attr else None
    risks = torch.empty(2 + n, dtype=torch.float32, device=dev)
    sh = SurvHead(Wk=ptr(Wk), bk=ptr(bk), K=Wk.shape[0], logits=None, hazards=None, S=None, Y_hat=None, risk=None)
    fp = C.POINTER(C.c_float)
    ig = _lib.IgDesc(n_steps=n, alpha=a.ctypes.data_as(fp), weight=w.ctypes.data_as(fp), window_steps=int(window_steps),
                     row_sum=ptr(rows[0]), row_abs=ptr(rows[1]), attr=ptr(attr), risk_x=ptr(risks[0:1]),
                     risk_base=ptr(risks[1:2]), step_risk=ptr(risks[2:]))
    check(getattr(l, name)(C.byref(d), lead, ptr(ws), nbytes, C.byref(sh), C.byref(ig), stream_ptr()), name)
    return rows[0], rows[1], attr, risks[0:1], risks[1:2], risks[2:]


def amil_integrated_gradients(x, stack, Wk, bk, gated, alphas, weights, want_attr=False, window_steps=0):
    """Integrated gradients of risk = -sum(S) with respect to the bag x [N x L] (fp32), from a zero baseline, in ONE C-ABI
    call (include/mmf_amil.h: mmf_amil_ig): the L-wide contractions run once, the H-wide part once per quadrature node.
    alphas, weights: the rule's nodes and weights (host sequences, rounded once to fp32); window_steps: nodes per grouped
    window (0: the library chooses).  Eval mode: no dropout.  Returns (row_sum [N], row_abs [N], attr [N x L] or None,
    risk_x [1], risk_base [1], step_risk [n_steps])."""
    if x.dtype == torch.bfloat16:
        raise NotImplementedError("integrated gradients take fp32 bags: the bf16 path has no input gradient")
    x = _f32c(x)
    if x.dim() != 2:
        raise _lib.MmfError(f"bag must be [N x L], got {tuple(x.shape)}")
    N, L = x.shape
    stack, (Wk, bk), H, D = _stack_operands(stack, L, (Wk, bk), "bag", fused_head=True)
    return _integrated_gradients("mmf_amil_ig", (N, L), ptr(x), "", stack, H, D, gated, Wk, bk, alphas, weights, want_attr,
                                 window_steps, x.device)


def radio_integrated_gradients(xs, Wr, br, stack, Wk, bk, gated, alphas, weights, want_attr=False, window_steps=0):
    """Integrated gradients of the radiology head's risk = -sum(S) with respect to every modality, from a zero baseline, in
    ONE C-ABI call (include/mmf_amil.h: mmf_radio_ig): reduce_dim and its transpose, the projection and its transpose run
    once, the H-wide part once per quadrature node.  xs: 2 .. 4 modality tensors, each [N x k] fp32; Wr, br: reduce_dim
    [k x nseg k], [k]; the other arguments as amil_integrated_gradients.  Returns (row_sum [nseg x N], row_abs [nseg x N],
    attr [nseg x N x k] or None, risk_x [1], risk_base [1], step_risk [n_steps])."""
    if any(x.dtype == torch.bfloat16 for x in xs):
        raise NotImplementedError("integrated gradients take fp32 bags: the bf16 path has no input gradient")
    xs, N, nseg, kseg, rd = _radio_operands(xs, Wr, br, "pass")
    stack, (Wk, bk), H, D = _stack_operands(stack, kseg, (Wk, bk), "bags", fused_head=True)
    return _integrated_gradients("mmf_radio_ig", (N, nseg, kseg), C.byref(rd), ", the modalities", stack, H, D, gated, Wk,
                                 bk, alphas, weights, want_attr, window_steps, xs[0].device)


def mm_integrated_gradients(branches, Wk, bk, alphas, weights, want_attr=False, window_steps=0, xfusion=None):
    """Integrated gradients of the multimodal concat head's risk = -sum(S) with respect to every input of every branch, from
    a joint zero baseline, in ONE C-ABI call (include/mmf_amil.h: mmf_mm_ig): the L-wide contractions, reduce_dim and
    W_o0 x_o run once, the H-wide part of each stack, the omic hidden layers and one head launch once per node.
    branches: two or three of ("path", x [N x L], stack, gated), ("radio", xs (2 .. 4 of [N x k]), Wr, br, stack, gated) and
    ("omic", x_o [Gin], W0, b0, W1, b1) in the order of their columns in the fused row; Wk [K x F], bk the hazard head over
    it; alphas, weights, want_attr, window_steps as amil_integrated_gradients.  Returns ({"path": (row_sum [N], row_abs
    [N], attr [N x L] or None), "radio": (row_sum [nseg x N], row_abs [nseg x N], attr [nseg x N x k] or None), "omic":
    attr [Gin]} for the branches given, risk_x [1], risk_base [1], step_risk [n_steps], (hazards [1 x K], S [1 x K],
    Y_hat [1 x 1]) at alpha = 1).
    xfusion = (weights, Wc0, bc0): the tensor-fusion head instead (mmf_mm_ig_tensor) -- the XlinearFusion weights as xfusion
    takes them and classifier[0]; every branch's embedding is dim wide, the branches stand in the order of the fusion's
    v_list, Wk [K x nhid], bk are classifier[3], and the tail (seven launches) runs once per window between the branches'
    halves, without a weight gradient."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).astype(np.float32))
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).astype(np.float32))
    if a.ndim != 1 or a.shape != w.shape or not 1 <= a.size <= GROUP_MAX:
        raise _lib.MmfError(f"alphas / weights: two sequences of 1..{GROUP_MAX} values each")
    n = int(a.size)
    kinds = [b[0] for b in branches]
    if len(set(kinds)) != len(kinds) or len(kinds) < 2 or any(k not in ("path", "radio", "omic") for k in kinds):
        raise _lib.MmfError(f"branches: two or three of path, radio and omic, each once, got {kinds}")
    for b in branches:
        xs = b[1] if b[0] == "radio" else [b[1]]
        if any(x.dtype == torch.bfloat16 for x in xs):
            raise NotImplementedError("integrated gradients take fp32 inputs: the bf16 path has no input gradient")
    fp = C.POINTER(C.c_float)
    mm = _lib.MmIgDesc(n_steps=n, window_steps=int(window_steps), alpha=a.ctypes.data_as(fp), weight=w.ctypes.data_as(fp))
    q = dict(Np=0, Lp=0, Hp=0, Dp=0, gp=0, Nr=0, nseg=0, kseg=0, Hr=0, Dr=0, gr=0, Gin=0, W0=0, We=0)
    keep, out, F, dev = [], {}, 0, None

    def outputs(ext, N, L):
        rows = torch.empty((2,) + ext + (N,), dtype=torch.float32, device=dev)
        attr = torch.empty(ext + (N, L), dtype=torch.float32, device=dev) if want_attr else None
        return rows, attr

    for b in branches:
        if b[0] == "path":
            _, x, stack, gated = b
            x = _f32c(x)
            if x.dim() != 2:
                raise _lib.MmfError(f"bag must be [N x L], got {tuple(x.shape)}")
            dev = x.device
            N, L = x.shape
            stack, _, H, D = _stack_operands(stack, L, None, "bag")
            d = _amil_desc(stack, N, L, H, D, gated, 0.0, 0.0, 0, None)
            rows, attr = outputs((), N, L)
            mm.path, mm.path_x, mm.path_col = C.pointer(d), ptr(x), F
            mm.path_row_sum, mm.path_row_abs, mm.path_attr = ptr(rows[0]), ptr(rows[1]), ptr(attr)
            q.update(Np=N, Lp=L, Hp=H, Dp=D, gp=d.gated)
            out["path"] = (rows[0], rows[1], attr)
            keep += [x, stack, d]
            F += H
        elif b[0] == "radio":
            _, xs, Wr, br, stack, gated = b
            xs, N, nseg, kseg, rd = _radio_operands(xs, Wr, br, "pass")
            dev = xs[0].device
            stack, _, H, D = _stack_operands(stack, kseg, None, "bags")
            d = _amil_desc(stack, N, kseg, H, D, gated, 0.0, 0.0, 0, None)
            rows, attr = outputs((nseg,), N, kseg)
            mm.radio, mm.rd, mm.radio_col = C.pointer(d), C.pointer(rd), F
            mm.radio_row_sum, mm.radio_row_abs, mm.radio_attr = ptr(rows[0]), ptr(rows[1]), ptr(attr)
            q.update(Nr=N, nseg=nseg, kseg=kseg, Hr=H, Dr=D, gr=d.gated)
            out["radio"] = (rows[0], rows[1], attr)
            keep += [xs, stack, d, rd]
            F += H
        else:
            _, x, W0, b0, W1, b1 = b
            x, W0, b0, W1, b1 = (_f32c(t) for t in (x, W0, b0, W1, b1))
            Gin = x.numel()
            if (x.dim() != 1 or W0.dim() != 2 or W0.shape[1] != Gin or W1.dim() != 2 or W1.shape[1] != W0.shape[0]
                    or tuple(b0.shape) != (W0.shape[0],) or tuple(b1.shape) != (W1.shape[0],)):
                raise _lib.MmfError(f"omic: x [Gin], W0 [W0 x Gin], b0 [W0], W1 [We x W0], b1 [We]; got {tuple(x.shape)}, "
                                    f"{tuple(W0.shape)}, {tuple(b0.shape)}, {tuple(W1.shape)}, {tuple(b1.shape)}")
            dev = x.device if dev is None else dev
            attr_o = torch.empty((Gin,), dtype=torch.float32, device=x.device)
            mm.omic_x, mm.omic_W0, mm.omic_b0, mm.omic_W1, mm.omic_b1 = ptr(x), ptr(W0), ptr(b0), ptr(W1), ptr(b1)
            mm.omic_attr, mm.omic_Gin, mm.omic_W0n, mm.omic_We, mm.omic_col = ptr(attr_o), Gin, W0.shape[0], W1.shape[0], F
            q.update(Gin=Gin, W0=W0.shape[0], We=W1.shape[0])
            out["omic"] = attr_o
            keep += [x, W0, b0, W1, b1]
            F += W1.shape[0]
    Wk, bk = _f32c(Wk), _f32c(bk)
    K = Wk.shape[0]
    name, xw, tail = "mmf_mm_ig", None, ()
    if xfusion is not None:
        name = "mmf_mm_ig_tensor"
        xweights, Wc0, bc0 = xfusion
        m = len(branches)
        if F % m != 0:
            raise _lib.MmfError(f"{name}: the {m} embeddings must be equally wide, the fused row has {F} columns")
        xw, xkeep, (sdim, mmhid1, mmhid2, nhid) = _xfusion_operands(m, 1, F // m, xweights, Wc0, bc0, name)
        keep += xkeep
        tail, F = (F // m, sdim, mmhid1, mmhid2, nhid), nhid
    if Wk.dim() != 2 or Wk.shape[1] != F or tuple(bk.shape) != (K,) or K > 32:
        raise _lib.MmfError(f"the hazard head must be [K <= 32 x {F}] over the {'fused row' if xw is None else 'hidden layer'}, "
                            f"got {tuple(Wk.shape)}")
    l = lib()
    nbytes = getattr(l, name + "_workspace_bytes")(q["Np"], q["Lp"], q["Hp"], q["Dp"], q["gp"], q["Nr"], q["nseg"], q["kseg"],
                                                   q["Hr"], q["Dr"], q["gr"], q["Gin"], q["W0"], q["We"], n,
                                                   int(window_steps), *tail)
    if nbytes == 0:
        raise _lib.MmfError(f"{name}: n_steps, window_steps, a branch's widths, the fused width{'' if xw is None else ', the tail'} "
                            "or a bag's size out of range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    risks = torch.empty(2 + n, dtype=torch.float32, device=dev)
    hz = torch.empty((2, 1, K), dtype=torch.float32, device=dev)
    Y_hat = torch.empty((1, 1), dtype=torch.int64, device=dev)
    mm.risk_x, mm.risk_base, mm.step_risk = ptr(risks[0:1]), ptr(risks[1:2]), ptr(risks[2:])
    sh = SurvHead(Wk=ptr(Wk), bk=ptr(bk), K=K, logits=None, hazards=ptr(hz[0]), S=ptr(hz[1]), Y_hat=ptr(Y_hat), risk=None)
    lead = (C.byref(mm),) if xw is None else (C.byref(mm), C.byref(xw))
    check(getattr(l, name)(*lead, ptr(ws), nbytes, C.byref(sh), stream_ptr()), name)
    return out, risks[0:1], risks[1:2], risks[2:], (hz[0], hz[1], Y_hat)


STAGE2_FAMILIES = {"nll": 0, "cox": 1}
STAGE2_TYPES = {"early-fcnn": 0, "late-fcnn": 1, "early-highway": 2, "late-highway": 3, "kronecker": 4}


def _bn1d(bn, keep):
    """mmf_bn1d of (weight, bias, running_mean, running_var, eps)."""
    w, b, mean, var, eps = bn
    w, b, mean, var = (_f32c(t) for t in (w, b, mean, var))
    keep += [w, b, mean, var]
    return _lib.Bn1d(weight=ptr(w), bias=ptr(b), mean=ptr(mean), var=ptr(var), eps=float(eps))


def stage2_integrated_gradients(family, train_type, present, vs, blocks, Wk, bk, alphas, weights, n_layers=1,
                                want_attr=False, xfusion=None):
    """Integrated gradients of a stage-2 fusion model's risk with respect to the embeddings of a cohort, from a zero
    baseline, in ONE C-ABI call (include/mmf_amil.h: mmf_stage2_ig): the first layer runs once per patient, everything
    behind it once per patient and node inside one launch.
    family: "nll" (risk = -sum S) or "cox" (the scalar output); train_type: a key of STAGE2_TYPES; present: (radio, path,
    omic) booleans; vs: the present embeddings, [P x 256] fp32 each, in the reference's cat order; blocks: one dict (early
    types) or one per embedding (late types) -- fcnn: W0, b0, bn = (weight, bias, running_mean, running_var, eps) and, for
    the cox late blocks, W4, b4; highway: bn1, bn2 and gate, nonlinear, linear = lists of n_layers (W, b) pairs; Wk, bk: the
    classifier behind them; alphas, weights: the rule's nodes (host sequences, rounded once to fp32).  kronecker: blocks
    is empty and xfusion holds the XlinearFusion weights as ops.xfusion takes them; its (patient, node) rows pass in
    windows of up to GROUP_MAX through the tensor fusion's grouped tail, nothing folds.
    Returns dict(mod_sum [P x m], mod_abs [P x m], attr (list of m [P x 256]) or None, risk [P], risk_base [P],
    step_risk [P x n_steps], hazards, S ([P x K], or None for cox))."""
    import numpy as np
    if family not in STAGE2_FAMILIES or train_type not in STAGE2_TYPES:
        raise ValueError(f"family in {sorted(STAGE2_FAMILIES)}, train_type in {sorted(STAGE2_TYPES)}; got {family!r}, {train_type!r}")
    a = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).astype(np.float32))
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).astype(np.float32))
    if a.ndim != 1 or a.shape != w.shape or not 1 <= a.size <= GROUP_MAX:
        raise _lib.MmfError(f"alphas / weights: two sequences of 1..{GROUP_MAX} values each")
    if any(v.dtype != torch.float32 for v in vs):
        raise NotImplementedError("integrated gradients take fp32 embeddings")
    n, m = int(a.size), len(vs)
    if m != sum(1 for f in present if f) or m not in (2, 3):
        raise _lib.MmfError(f"two or three embeddings, one per present modality; got {m} for {tuple(present)}")
    vs = [_f32c(v) for v in vs]
    P = vs[0].shape[0]
    if any(v.dim() != 2 or tuple(v.shape) != (P, 256) for v in vs):
        raise _lib.MmfError(f"every embedding must be [P x 256], got {[tuple(v.shape) for v in vs]}")
    hw, late = "highway" in train_type, "late" in train_type
    kron = train_type == "kronecker"
    if len(blocks) != (0 if kron else m if late else 1):
        raise _lib.MmfError(f"{train_type}: {0 if kron else m if late else 1} block(s) expected, got {len(blocks)}")
    Wk, bk = _f32c(Wk), _f32c(bk)
    K = bk.numel()
    dev, keep = vs[0].device, []
    fp = C.POINTER(C.c_float)
    d = _lib.Stage2IgDesc(family=STAGE2_FAMILIES[family], train_type=STAGE2_TYPES[train_type], radio=int(bool(present[0])),
                          path=int(bool(present[1])), omic=int(bool(present[2])), n_layers=int(n_layers), P=P, K=K, n_steps=n,
                          alpha=a.ctypes.data_as(fp), weight=w.ctypes.data_as(fp), Wk=ptr(Wk), bk=ptr(bk), trace=_trace)
    kin = 256 if late else 256 * m
    width = 256 if kron else (kin if hw else 128) * len(blocks)
    want_k = (1, m) if (family == "cox" and train_type == "late-fcnn") else (K, width)
    if Wk.dim() != 2 or tuple(Wk.shape) != want_k:
        raise _lib.MmfError(f"{train_type}: the classifier must be {want_k}, got {tuple(Wk.shape)}")
    for i, b in enumerate(blocks):
        blk = d.blk[i]
        if hw:
            blk.bn1, blk.bn2 = _bn1d(b["bn1"], keep), _bn1d(b["bn2"], keep)
            for name, key in (("gate", "gate"), ("nl", "nonlinear"), ("lin", "linear")):
                pairs = [(_f32c(W_), _f32c(b_)) for W_, b_ in b[key]]
                if len(pairs) != n_layers or any(tuple(W_.shape) != (kin, kin) or b_.numel() != kin for W_, b_ in pairs):
                    raise _lib.MmfError(f"{train_type}: {n_layers} {key} layer(s) of [{kin} x {kin}] expected")
                Ws = (C.c_void_p * n_layers)(*[ptr(W_) for W_, _ in pairs])
                bs = (C.c_void_p * n_layers)(*[ptr(b_) for _, b_ in pairs])
                setattr(blk, "W" + name, Ws)
                setattr(blk, "b" + name, bs)
                keep += [pairs, Ws, bs]
        else:
            W0, b0 = _f32c(b["W0"]), _f32c(b["b0"])
            if tuple(W0.shape) != (128, kin) or b0.numel() != 128:
                raise _lib.MmfError(f"{train_type}: W0 must be [128 x {kin}], got {tuple(W0.shape)}")
            blk.W0, blk.b0, blk.bn = ptr(W0), ptr(b0), _bn1d(b["bn"], keep)
            keep += [W0, b0]
            if b.get("W4") is not None:
                W4, b4 = _f32c(b["W4"]), _f32c(b["b4"])
                if W4.numel() != 128 or b4.numel() != 1:
                    raise _lib.MmfError(f"{train_type}: W4 must be [1 x 128], b4 [1]")
                blk.W4, blk.b4 = ptr(W4), ptr(b4)
                keep += [W4, b4]
    if kron:
        xw, xkeep, dims = _xfusion_operands(m, 1, 256, xfusion, Wk, bk, "mmf_stage2_ig")     # Wc0, bc0 are not read
        if dims[:3] != (16, 256, 256):
            raise _lib.MmfError(f"mmf_stage2_ig: the stage-2 fusion is 16 / 256 / 256 wide, got {dims[:3]}")
        d.xf = C.pointer(xw)
        keep += [xw, xkeep]
    l = lib()
    nbytes = l.mmf_stage2_ig_workspace_bytes(d.family, d.train_type, m, d.n_layers, P, K, n)
    if nbytes == 0:
        raise _lib.MmfError("mmf_stage2_ig: P, n_steps, K or n_layers out of range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sums = torch.empty((2, P, m), dtype=torch.float32, device=dev)
    risks = torch.empty((2, P), dtype=torch.float32, device=dev)
    step_risk = torch.empty((P, n), dtype=torch.float32, device=dev)
    hz = torch.empty((2, P, K), dtype=torch.float32, device=dev) if family == "nll" else None
    attr = [torch.empty((P, 256), dtype=torch.float32, device=dev) for _ in range(m)] if want_attr else None
    for i in range(m):
        d.v[i] = ptr(vs[i])
        d.attr[i] = ptr(attr[i]) if attr else None
    d.mod_sum, d.mod_abs, d.risk, d.risk_base, d.step_risk = ptr(sums[0]), ptr(sums[1]), ptr(risks[0]), ptr(risks[1]), ptr(step_risk)
    if hz is not None:
        d.hazards, d.S = ptr(hz[0]), ptr(hz[1])
    check(l.mmf_stage2_ig(C.byref(d), ptr(ws), nbytes, stream_ptr()), "mmf_stage2_ig")
    return dict(mod_sum=sums[0], mod_abs=sums[1], attr=attr, risk=risks[0], risk_base=risks[1], step_risk=step_risk,
                hazards=None if hz is None else hz[0], S=None if hz is None else hz[1])


STAGE2_LOSSES = {"nll": 0, "cox": 1, "rank": 2, "rank_nll": 3}
_S2_LAYERS = (("gate", "gate"), ("nl", "nonlinear"), ("lin", "linear"))


def _bn_train(bn, keep):
    """mmf_stage2_bn_train of (weight, bias, running_mean, running_var, eps, momentum)."""
    w, b, mean, var, eps, mom = bn
    keep += [w, b, mean, var]
    return _lib.Stage2BnTrain(weight=ptr(w), bias=ptr(b), running_mean=ptr(mean), running_var=ptr(var), eps=float(eps),
                              momentum=float(mom))


def stage2_step(family, train_type, present, hs, blocks, Wk, bk, loss, Y=None, c=None, times=None, grads=None,
                accumulate=False, loss_scale=1.0, training=True, n_layers=1, p_drop=0.7, seed=0):
    """One training step of a stage-2 fcnn or highway model -- forward, loss, every parameter gradient, the BatchNorm
    running statistics -- in ONE C-ABI call (include/mmf_amil.h: mmf_stage2_step), three launches for the fcnn types and
    2 n_layers + 3 for the highway types.
    family: "nll" or "cox"; train_type: early-fcnn, late-fcnn, early-highway or late-highway; present: (radio, path, omic)
    booleans; hs: (h_radio, h_path, h_omic), [B x 256] fp32 each (the late types read all three, the early types the present
    ones).  blocks: one dict (early types) or three, radio / path / omic (late types: the forward runs the block of the
    modality the mode drops too) -- fcnn: W0, b0, bn = (weight, bias, running_mean, running_var, eps, momentum) and, for the cox
    late blocks, W4, b4; highway: bn1, bn2 and gate, nonlinear, linear = lists of n_layers (W, b) pairs.  Wk, bk: the
    classifier.  loss: dict(kind = a key of STAGE2_LOSSES, alpha, nll_ratio, phi = "sigmoid" | "relu", reduction = "mean" |
    "sum"); Y int64 [B], c [B], times float64 CUDA [B] as the loss needs them.
    grads: None (forward and loss only: validation) or dict(blocks = a list like `blocks` of the gradient tensors under the
    same keys -- bn, bn1, bn2 = (dweight, dbias); None for the block without a gradient --, dWk, dbk): the gradients of
    loss * loss_scale are written there, or added when `accumulate`.
    Returns (risk [B], hazards, S ([B x K], or None for cox), loss), detached; the loss is unscaled."""
    if family not in STAGE2_FAMILIES or train_type not in STAGE2_TYPES or train_type == "kronecker":
        raise ValueError(f"stage2_step: family in {sorted(STAGE2_FAMILIES)}, train_type fcnn or highway; got {family!r}, {train_type!r}")
    hw, late = "highway" in train_type, "late" in train_type
    m = sum(1 for f in present if f)
    read = [late or bool(f) for f in present]
    hs = [_f32c(h) if r else None for h, r in zip(hs, read)]
    first = next(h for h in hs if h is not None)
    B, dev = first.shape[0], first.device
    if any(h is not None and tuple(h.shape) != (B, 256) for h in hs):
        raise _lib.MmfError(f"stage2_step: every embedding must be [B x 256], got {[None if h is None else tuple(h.shape) for h in hs]}")
    nb = 3 if late else 1
    if len(blocks) != nb:
        raise _lib.MmfError(f"{train_type}: {nb} block(s) expected, got {len(blocks)}")
    K = bk.numel()
    kin = 256 if late else 256 * m
    want_k = (1, m) if (family == "cox" and train_type == "late-fcnn") else (K, (kin if hw else 128) * (m if late else 1))
    if tuple(Wk.shape) != want_k:
        raise _lib.MmfError(f"{train_type}: the classifier must be {want_k}, got {tuple(Wk.shape)}")
    for b in blocks:                                   # the kernels index by these widths
        if hw:
            if any(len(b[key]) != n_layers or any(tuple(W_.shape) != (kin, kin) or b_.numel() != kin for W_, b_ in b[key])
                   for _, key in _S2_LAYERS) or any(t.numel() != kin for bn in (b["bn1"], b["bn2"]) for t in bn[:4]):
                raise _lib.MmfError(f"{train_type}: {n_layers} layer(s) of [{kin} x {kin}] and BatchNorm1d({kin}) expected")
        elif tuple(b["W0"].shape) != (128, kin) or b["b0"].numel() != 128 or any(t.numel() != 128 for t in b["bn"][:4]) or (
                b.get("W4") is not None and (b["W4"].numel() != 128 or b["b4"].numel() != 1)):
            raise _lib.MmfError(f"{train_type}: W0 must be [128 x {kin}] with BatchNorm1d(128), W4 [1 x 128]")
    keep = []
    d = _lib.Stage2StepDesc(family=STAGE2_FAMILIES[family], train_type=STAGE2_TYPES[train_type], radio=int(bool(present[0])),
                            path=int(bool(present[1])), omic=int(bool(present[2])), n_layers=int(n_layers), B=B, K=K,
                            training=1 if training else 0, Wk=ptr(Wk), bk=ptr(bk), p_drop=float(p_drop),
                            seed=int(seed) & 0xFFFFFFFF, seed_dev=ptr(_seed_word), trace=_trace)
    for i, h in enumerate(hs):
        d.h[i] = ptr(h)
    g = _lib.Stage2StepGrads(dWk=ptr(grads["dWk"]), dbk=ptr(grads["dbk"])) if grads is not None else None
    for i, b in enumerate(blocks):
        blk = d.blk[i]
        gb = grads["blocks"][i] if grads is not None else None
        gblk = g.blk[i] if gb is not None else None
        if hw:
            blk.bn1, blk.bn2 = _bn_train(b["bn1"], keep), _bn_train(b["bn2"], keep)
            if gb is not None:
                gblk.dbn1_weight, gblk.dbn1_bias = ptr(gb["bn1"][0]), ptr(gb["bn1"][1])
                gblk.dbn2_weight, gblk.dbn2_bias = ptr(gb["bn2"][0]), ptr(gb["bn2"][1])
            for name, key in _S2_LAYERS:
                Ws = (C.c_void_p * n_layers)(*[ptr(W_) for W_, _ in b[key]])
                bs = (C.c_void_p * n_layers)(*[ptr(b_) for _, b_ in b[key]])
                setattr(blk, "W" + name, Ws)
                setattr(blk, "b" + name, bs)
                keep += [Ws, bs]
                if gb is not None:
                    dWs = (C.c_void_p * n_layers)(*[ptr(W_) for W_, _ in gb[key]])
                    dbs = (C.c_void_p * n_layers)(*[ptr(b_) for _, b_ in gb[key]])
                    setattr(gblk, "dW" + name, dWs)
                    setattr(gblk, "db" + name, dbs)
                    keep += [dWs, dbs]
        else:
            blk.W0, blk.b0, blk.bn = ptr(b["W0"]), ptr(b["b0"]), _bn_train(b["bn"], keep)
            if b.get("W4") is not None:
                blk.W4, blk.b4 = ptr(b["W4"]), ptr(b["b4"])
            if gb is not None:
                gblk.dW0, gblk.db0 = ptr(gb["W0"]), ptr(gb["b0"])
                gblk.dbn_weight, gblk.dbn_bias = ptr(gb["bn"][0]), ptr(gb["bn"][1])
                if gb.get("W4") is not None:
                    gblk.dW4, gblk.db4 = ptr(gb["W4"]), ptr(gb["b4"])
    kind = loss["kind"]
    if Y is not None:
        Y = Y.reshape(B).to(device=dev, dtype=torch.int64).contiguous()
    if times is not None and (times.dtype != torch.float64 or not times.is_cuda):
        raise _lib.MmfError("stage2_step: event times must be a float64 CUDA tensor")
    cc = c.reshape(B).to(device=dev, dtype=torch.float32).contiguous()
    t = _lib.Stage2Target(loss=STAGE2_LOSSES[kind], Y=ptr(Y), c=ptr(cc), times=ptr(times),
                          alpha=float(loss.get("alpha", 0.0)), nll_ratio=float(loss.get("nll_ratio", 0.0)),
                          phi={"sigmoid": 0, "relu": 1}[loss.get("phi", "sigmoid")],
                          reduction={"mean": 0, "sum": 1}[loss.get("reduction", "mean")], loss_scale=float(loss_scale))
    l = lib()
    nbytes = l.mmf_stage2_step_workspace_bytes(d.family, d.train_type, m, d.n_layers, B, K, d.training)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    risk = torch.empty((B,), dtype=torch.float32, device=dev)
    hz = torch.empty((2, B, K), dtype=torch.float32, device=dev) if family == "nll" else None
    out = torch.empty((), dtype=torch.float32, device=dev)
    check(l.mmf_stage2_step(C.byref(d), C.byref(t), ptr(ws), nbytes, ptr(risk), None if hz is None else ptr(hz[0]),
                            None if hz is None else ptr(hz[1]), ptr(out), None if g is None else C.byref(g),
                            1 if accumulate else 0, stream_ptr()), "mmf_stage2_step")
    return risk, (None if hz is None else hz[0]), (None if hz is None else hz[1]), out


def radio_infer_group(xs, sizes, Wr, br, stack, gated, Wk=None, bk=None, Y=None, c=None, alpha=0.0, want_M=False,
                      eps=1e-7):
    """The radiology head's G bags evaluated in ONE C-ABI call (include/mmf_amil.h: mmf_radio_infer_group): reduce_dim
    over the modality segments and the stack's GEMMs once over all rows, pooling and the head per bag.  xs: 2 .. 4
    modality tensors, each [sum N x k] fp32 (the bags' rows in order); Wr, br: reduce_dim [k x nseg k], [k].  Other
    arguments and the result as amil_infer_group."""
    xs, R, nseg, kseg, rd = _radio_operands(xs, Wr, br, "pass")
    sizes, Y, c, offs, grp = _group_table(sizes, R, Y, c, train=False)
    G, dev = len(sizes), xs[0].device
    stack, H, D, hd, tg, (hz, S, Y_hat, loss, risk), M, _keep = _infer_operands(stack, kseg, Wk, bk, Y, c, alpha, eps,
                                                                                want_M, G, dev)
    d = _amil_desc(stack, R, kseg, H, D, gated, 0.0, 0.0, 0, None)
    A_raw = torch.empty((R,), dtype=torch.float32, device=dev)
    A_list = _run_group("mmf_radio_group_infer_workspace_bytes", (offs, G, nseg, kseg, H, D, d.gated),
                        "mmf_radio_infer_group", d, grp, (C.byref(rd),), hd, tg, (ptr(M), ptr(A_raw)), A_raw, sizes)
    return hz, S, Y_hat, risk, A_list, M, loss


def _group_rows(ts, what):
    """ts: 1 .. 3 dense fp32 matrices with the same number G of rows, 1 <= G <= GROUP_MAX.  Returns (ts contiguous, G)."""
    ts = list(ts)
    if any(not torch.is_tensor(t) or t.dim() != 2 for t in ts):
        raise _lib.MmfError(f"{what}: [G x width] matrices expected")
    ts = [_f32c(t) for t in ts]
    G = int(ts[0].shape[0]) if ts else 0
    if any(t.shape[0] != G for t in ts):
        raise _lib.MmfError(f"{what}: the matrices hold different numbers of patients: {[int(t.shape[0]) for t in ts]}")
    if G < 1 or G > GROUP_MAX:
        raise _lib.MmfError(f"a group holds 1 .. {GROUP_MAX} patients, got {G}")
    return ts, G


def _xfusion_operands(m, G, dim, weights, Wc0, bc0, what):
    """The XlinearFusion weights (xfusion's order) and classifier[0] of a grouped fusion call, checked against m
    embeddings [G x dim].  Returns (mmf_xfusion_weights, the contiguous tensors it points to, (sdim, mmhid1, mmhid2, nhid))."""
    if m < 2 or m > 3 or len(weights) != 6 * m + 4:
        raise _lib.MmfError(f"{what} takes 2 or 3 modalities with 6 m + 4 weights, got {m} / {len(weights)}")
    w = [_f32c(t) for t in weights]
    Wc0, bc0 = _f32c(Wc0), _f32c(bc0)
    sdim = int(w[0].shape[0])
    We1, be1, We2, be2 = w[6 * m:]
    mmhid1, mmhid2, nhid = int(We1.shape[0]), int(We2.shape[0]), int(Wc0.shape[0])
    ok = (tuple(We1.shape) == (mmhid1, (sdim + 1) ** m)
          and tuple(We2.shape) == (mmhid2, mmhid1 + m * dim) and tuple(Wc0.shape) == (nhid, mmhid2)
          and be1.numel() == mmhid1 and be2.numel() == mmhid2 and bc0.numel() == nhid)
    for i in range(m):
        Wh, bh, Wz, bz, Wo, bo = w[6 * i:6 * i + 6]
        ok = ok and (tuple(Wh.shape) == (sdim, dim) and tuple(Wz.shape) == (sdim, m * dim) and tuple(Wo.shape) == (sdim, sdim)
                     and bh.numel() == bz.numel() == bo.numel() == sdim)
    if not ok or dim % 4 != 0 or sdim != 16:
        raise _lib.MmfError(f"{what}: the weights do not match the embeddings (dim % 4 == 0, scale width 16)")
    xw = _lib.XFusionWeights(m=m, dim=dim, sdim=sdim, mmhid1=mmhid1, mmhid2=mmhid2, nhid=nhid, We1=ptr(We1), be1=ptr(be1),
                             We2=ptr(We2), be2=ptr(be2), Wc0=ptr(Wc0), bc0=ptr(bc0))
    for i in range(m):
        for name, t in zip(("Wh", "bh", "Wz", "bz", "Wo", "bo"), w[6 * i:6 * i + 6]):
            getattr(xw, name)[i] = ptr(t)
    return xw, w + [Wc0, bc0], (sdim, mmhid1, mmhid2, nhid)


def xfusion_infer_group(vs, weights, Wc0, bc0):
    """The XlinearFusion block (gate, skip) and classifier[0] + ReLU for the G patients of an evaluation window, forward
    only, in ONE C-ABI call of four launches (include/mmf_amil.h: mmf_xfusion_infer_group): the gating stage per
    patient, the Kronecker product fused into encoder1 (never written; encoder1's weight is read once per window),
    encoder2 on [e1 | v_0 | ...] read in place, classifier[0].  vs: 2 or 3 embedding matrices [G x dim]; weights as
    xfusion takes them ([Wh_0, bh_0, Wz_0, bz_0, Wo_0, bo_0, ..., We1, be1, We2, be2]); Wc0, bc0: classifier[0].  Eval
    mode: no dropout.  Returns (MM [G x mmhid2], hid [G x nhid]); row g is what the call gives patient g alone, bit for
    bit."""
    m = len(vs)
    if m < 2 or m > 3 or len(weights) != 6 * m + 4:
        raise _lib.MmfError(f"xfusion_infer_group takes 2 or 3 modalities with 6 m + 4 weights, got {m} / {len(weights)}")
    vs, G = _group_rows(vs, "xfusion_infer_group")
    dim = int(vs[0].shape[1])
    if any(tuple(v.shape) != (G, dim) for v in vs):
        raise _lib.MmfError("xfusion_infer_group: the weights do not match the embeddings (dim % 4 == 0, scale width 16)")
    xw, _keep, (sdim, mmhid1, mmhid2, nhid) = _xfusion_operands(m, G, dim, weights, Wc0, bc0, "xfusion_infer_group")
    dev = vs[0].device
    MM = torch.empty((G, mmhid2), dtype=torch.float32, device=dev)
    hid = torch.empty((G, nhid), dtype=torch.float32, device=dev)
    vp = (C.c_void_p * m)(*[ptr(v) for v in vs])
    l = lib()
    nbytes = l.mmf_xfusion_group_infer_workspace_bytes(m, sdim, mmhid1, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(l.mmf_xfusion_infer_group(C.byref(xw), vp, G, ptr(ws), nbytes, ptr(MM), ptr(hid), stream_ptr()),
          "mmf_xfusion_infer_group")
    return MM, hid


def xfusion_group_input(G, m, dim, mmhid1, device):
    """encoder2's input matrix x2 [G x mmhid1 + m dim] of a grouped tensor-fusion step and the m views [G x dim] where the
    branches write v_i (columns mmhid1 + i dim ..): _xfusion_group_fwd_raw reads the embeddings there and fills the first
    mmhid1 columns, so no concatenation is ever a launch."""
    x2 = torch.empty((G, mmhid1 + m * dim), dtype=torch.float32, device=device)
    return x2, [x2[:, mmhid1 + i * dim: mmhid1 + (i + 1) * dim] for i in range(m)]


def _xfusion_group_fwd_raw(x2, m, weights, Wc0, bc0, p, p_c, seeds, word=None):
    """The XlinearFusion block and classifier[0] + ReLU + Dropout for the G patients of one accumulation window, training
    form, in ONE C-ABI call of four launches (include/mmf_amil.h: mmf_xfusion_group_forward).  x2: xfusion_group_input's
    matrix with the embeddings in place; weights as xfusion takes them; p: XlinearFusion's dropout rate (sites 0 .. 10),
    p_c: classifier[2]'s (site 11), both 0 in eval mode; seeds: the G fusion seeds -- patient g gets the masks a one-patient
    call draws under seeds[g].  Returns (MM [G x mmhid2], hid [G x nhid], state for _xfusion_group_bwd_raw)."""
    if not torch.is_tensor(x2) or x2.dim() != 2 or x2.dtype != torch.float32 or not x2.is_contiguous():
        raise _lib.MmfError("xfusion group step: x2 must be a contiguous fp32 [G x mmhid1 + m dim] matrix")
    G = int(x2.shape[0])
    if G < 1 or G > GROUP_MAX:
        raise _lib.MmfError(f"a group holds 1 .. {GROUP_MAX} patients, got {G}")
    if len(seeds) != G:
        raise _lib.MmfError(f"{G} patients need {G} fusion seeds, got {len(seeds)}")
    mmhid1 = int(weights[6 * m].shape[0]) if 2 <= m <= 3 and len(weights) == 6 * m + 4 else 0
    dim = (int(x2.shape[1]) - mmhid1) // max(m, 1)
    xw, keep, (sdim, mmhid1, mmhid2, nhid) = _xfusion_operands(m, G, dim, weights, Wc0, bc0, "xfusion group step")
    if x2.shape[1] != mmhid1 + m * dim:
        raise _lib.MmfError(f"xfusion group step: x2 must be [G x {mmhid1} + {m} dim], got {tuple(x2.shape)}")
    dev = x2.device
    base = dropout_row_base(seeds, dev)
    MM = torch.empty((G, mmhid2), dtype=torch.float32, device=dev)
    hid = torch.empty((G, nhid), dtype=torch.float32, device=dev)
    l = lib()
    nbytes = l.mmf_xfusion_group_workspace_bytes(m, dim, sdim, mmhid1, mmhid2, nhid, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(l.mmf_xfusion_group_forward(C.byref(xw), ptr(x2), G, float(p), float(p_c), ptr(base), ptr(word), ptr(ws), nbytes,
                                      ptr(MM), ptr(hid), stream_ptr()), "mmf_xfusion_group_forward")
    return MM, hid, (xw, keep, x2, m, G, float(p), float(p_c), base, word, MM, hid, ws, mmhid1, dim)


def _xfusion_group_bwd_raw(dhid, state, grads=None, accumulate=False):
    """The backward of a _xfusion_group_fwd_raw call from dhid ([G x nhid] or columns of a wider matrix: the hazard
    head's dfeat) (mmf_xfusion_group_backward).  grads: gradient tensors in the order of (weights, Wc0, bc0), overwritten
    or, with `accumulate`, added to; None: fresh ones.  Returns ([dv_i: views of one [G x K2] matrix, skip connection
    included], grads): sums over the patients in patient order."""
    xw, keep, x2, m, G, p, p_c, base, word, MM, hid, ws, mmhid1, dim = state
    dp, ldd = _rows_ptr(dhid, "dhid")
    if tuple(dhid.shape) != tuple(hid.shape):
        raise _lib.MmfError(f"dhid must be {tuple(hid.shape)}, got {tuple(dhid.shape)}")
    if grads is None:
        if accumulate:
            raise _lib.MmfError("accumulate needs the gradient tensors to add to")
        grads = [torch.empty_like(t) for t in keep]
    else:
        grads = list(grads)
        if len(grads) != len(keep):
            raise _lib.MmfError(f"xfusion group step: {len(keep)} gradient tensors expected, got {len(grads)}")
        _check_grad_buffers(tuple(zip(grads, keep)))
    xg = _lib.XFusionGrads()
    for i in range(m):
        for name, t in zip(("dWh", "dbh", "dWz", "dbz", "dWo", "dbo"), grads[6 * i:6 * i + 6]):
            getattr(xg, name)[i] = ptr(t)
    for name, t in zip(("dWe1", "dbe1", "dWe2", "dbe2", "dWc0", "dbc0"), grads[6 * m:]):
        setattr(xg, name, ptr(t))
    dx2 = torch.empty_like(x2)
    check(lib().mmf_xfusion_group_backward(C.byref(xw), ptr(x2), G, p, p_c, ptr(base), ptr(word), ptr(MM), ptr(hid), dp, ldd,
                                           ptr(ws), ws.numel(), ptr(dx2), C.byref(xg), 1 if accumulate else 0,
                                           stream_ptr()), "mmf_xfusion_group_backward")
    return [dx2[:, mmhid1 + i * dim: mmhid1 + (i + 1) * dim] for i in range(m)], grads


def surv_head_infer_group(segs, Wk, bk, Y=None, c=None, alpha=0.0, eps=1e-7):
    """The hazard head for the G patients of an evaluation window, forward only, in ONE launch (include/mmf_amil.h:
    mmf_surv_head_infer_group).  segs: 1 .. 3 dense matrices [G x width_s]; patient g's feature row is the concatenation of
    their rows g (the branch embeddings in the model's order -- no torch.cat -- or the tensor fusion's hid alone), sum
    width <= 1024; Wk [K x sum width], K <= 32; Y, c: G labels / censorships for each patient's NLLSurvLoss(alpha) value,
    or None.  Returns (hazards [G x K], S [G x K], Y_hat [G x 1], loss [G] or None, risk [G]): the forward outputs of
    surv_head_nll_step_group on the concatenated matrix, bit for bit."""
    Wk, bk = _f32c(Wk), _f32c(bk)
    segs = list(segs)
    if len(segs) < 1 or len(segs) > 3:
        raise _lib.MmfError(f"surv_head_infer_group takes 1 .. 3 feature segments, got {len(segs)}")
    segs, G = _group_rows(segs, "surv_head_infer_group")
    widths = [int(t.shape[1]) for t in segs]
    F, K = sum(widths), int(Wk.shape[0])
    if min(widths) < 1 or Wk.dim() != 2 or Wk.shape[1] != F or F > 1024 or K > 32 or bk.numel() != K:
        raise _lib.MmfError("surv_head_infer_group: classifier does not match the feature segments (sum width <= 1024, K <= 32)")
    if Y is not None:
        Y = torch.as_tensor(Y).reshape(-1)
        c = torch.as_tensor(c).reshape(-1)
        if Y.numel() != G or c.numel() != G:
            raise _lib.MmfError(f"{G} patients need {G} labels and censorships, got {Y.numel()} / {c.numel()}")
    dev = segs[0].device
    hd, tg, (hz, S, Y_hat, loss, risk), _keep = _nll_head(Wk, bk, Y, c, alpha, eps, 1.0, None, None, False, dev, G)
    sp = (C.c_void_p * len(segs))(*[ptr(t) for t in segs])
    wd = (C.c_int32 * len(segs))(*widths)
    check(lib().mmf_surv_head_infer_group(sp, wd, len(segs), G, C.byref(hd), tg and C.byref(tg), stream_ptr()),
          "mmf_surv_head_infer_group")
    return hz, S, Y_hat, loss, risk


def amil_head(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, Wk, bk, gated, p_h=0.0, p_att=0.0, seed=0):
    if not torch.is_grad_enabled() and p_h == 0.0 and p_att == 0.0:       # inference consumers: no-save kernels
        M, A_raw = amil_infer(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, gated)
        hz, S, Y_hat = surv_head(M, Wk, bk)
        return hz, S, Y_hat, A_raw
    return AmilHeadFn.apply(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, Wk, bk, gated, p_h, p_att, seed)


class AttnNetFn(torch.autograd.Function):
    """The attention scorer alone: x [N x L] -> A [N x 1] (models/model_modules.py:84-85 / :105-110)."""

    @staticmethod
    def forward(ctx, x, Wa, ba, Wb, bb, Wc, bc, gated, p_att, seed):
        x, Wa, ba, Wb, bb, Wc, bc = map(_f32c, (x, Wa, ba, Wb, bb, Wc, bc))
        if x.dim() != 2 or Wa.shape[1] != x.shape[1] or Wc.shape[0] != 1 or Wc.shape[1] != Wa.shape[0]:
            raise _lib.MmfError("Attn_Net: x must be [N x L] and the scorer must have n_classes = 1")
        N, H = x.shape
        D = Wa.shape[0]
        cfg, word = (N, H, H, D, gated, 0.0, p_att, seed), _seed_word
        d = _amil_desc((None, None, Wa, ba, Wb, bb, Wc, bc), *cfg, word)
        l = lib()
        nbytes = l.mmf_attn_net_workspace_bytes(N, H, D, d.gated)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        A = torch.empty((N, 1), dtype=torch.float32, device=x.device)
        check(l.mmf_attn_net_forward(C.byref(d), ptr(x), ptr(ws), nbytes, ptr(A), stream_ptr()), "mmf_attn_net_forward")
        ctx.state = (cfg, ws, word)
        ctx.save_for_backward(x, Wa, ba, Wb, bb, Wc, bc)
        return A

    @staticmethod
    def backward(ctx, gA):
        x, *scorer = ctx.saved_tensors
        stack, (cfg, ws, word) = (None, None, *scorer), ctx.state
        gA = _f32c(gA).reshape(cfg[0])
        d = _amil_desc(stack, *cfg, word)
        ds, dx, g = _stack_grads(x, stack, cfg[4], ctx.needs_input_grad[0])
        check(lib().mmf_attn_net_backward(C.byref(d), ptr(x), ptr(ws), ws.numel(), ptr(gA), C.byref(g), stream_ptr()),
              "mmf_attn_net_backward")
        return (dx, *ds[2:], None, None, None)


def attn_net(x, Wa, ba, Wb, bb, Wc, bc, gated, p_att=0.0, seed=0):
    return AttnNetFn.apply(x, Wa, ba, Wb, bb, Wc, bc, gated, p_att, seed)


def _linear_cat_fwd_raw(xs, W, b):
    """y = cat(xs, dim=1) @ W.T + b without materialising the concatenation (mmf_linear_forward).
    Returns (y, saved): saved = (W, *xs) as the kernel took them, for _linear_cat_bwd_raw."""
    xs = [_f32c(x) for x in xs]
    W, b = _f32c(W), _f32c(b)
    M, kseg = xs[0].shape
    for x in xs:
        if tuple(x.shape) != (M, kseg):
            raise _lib.MmfError("all concatenated segments must have the same [M x k] shape")
    nseg = len(xs)
    N = W.shape[0]
    if W.shape[1] != nseg * kseg:
        raise _lib.MmfError("weight does not match the concatenated width")
    y = torch.empty((M, N), dtype=torch.float32, device=W.device)
    segs = (C.c_void_p * nseg)(*[ptr(x) for x in xs])
    wsb = lib().mmf_linear_forward_workspace_bytes(M, N, nseg, kseg)
    sw = sync_words(W.device) if wsb else None
    ws = torch.empty(wsb, dtype=torch.uint8, device=W.device) if sw is not None else None
    check(lib().mmf_linear_forward(segs, nseg, kseg, M, ptr(W), ptr(b), N, ACT["none"], 0.0, 0, 0, None,
                                   ptr(y), ptr(ws), wsb if ws is not None else 0, ptr(sw), SYNC_WORDS if sw is not None else 0,
                                   stream_ptr()), "mmf_linear_forward")
    return y, (W, *xs)


def _linear_cat_bwd_raw(gy, saved, has_bias, need_dx):
    """(dW, db, dx) of a _linear_cat_fwd_raw call (mmf_linear_backward); db only with a bias, dx only when need_dx."""
    W, *xs = saved
    gy = _f32c(gy)
    M, kseg = xs[0].shape
    nseg = len(xs)
    N, K = W.shape
    l = lib()
    dW = torch.empty_like(W)
    db = torch.empty((N,), dtype=torch.float32, device=W.device) if has_bias else None
    if need_dx and nseg != 1:
        raise _lib.MmfError("input gradient of a concatenated linear is not provided (bags are leaves)")
    dx = torch.empty_like(xs[0]) if need_dx else None
    nbytes = l.mmf_linear_backward_workspace_bytes(M, N, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=W.device)
    segs = (C.c_void_p * nseg)(*[ptr(x) for x in xs])
    check(l.mmf_linear_backward(ptr(gy), segs, nseg, kseg, M, ptr(W), N, ptr(dW), ptr(db), ptr(dx),
                                ptr(ws), nbytes, stream_ptr()), "mmf_linear_backward")
    return dW, db, dx


def _linear_cat_dx_raw(gy, saved):
    """The input gradients of a _linear_cat_fwd_raw call over several segments, one [M x k] tensor per segment
    (mmf_linear_input_grad) -- the training steps never ask for them (bags are leaves); attribution by autograd does."""
    W, *xs = saved
    gy = _f32c(gy)
    M, kseg = xs[0].shape
    nseg = len(xs)
    dxs = tuple(torch.empty_like(x) for x in xs)
    segs = (C.c_void_p * nseg)(*[ptr(t) for t in dxs])
    check(lib().mmf_linear_input_grad(ptr(gy), ptr(W), nseg, kseg, M, W.shape[0], segs, stream_ptr()),
          "mmf_linear_input_grad")
    return dxs


class LinearCatFn(torch.autograd.Function):
    """y = cat(xs, dim=1) @ W.T + b without materialising the concatenation
    (models/model_attention_mil_radio.py:80-82)."""

    @staticmethod
    def forward(ctx, W, b, *xs):
        y, saved = _linear_cat_fwd_raw(xs, W, b)
        ctx.save_for_backward(*saved)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        nseg = len(ctx.needs_input_grad) - 2
        need_dx = any(ctx.needs_input_grad[2:])
        dW, db, dx = _linear_cat_bwd_raw(gy, ctx.saved_tensors, ctx.has_bias, need_dx and nseg == 1)
        if nseg == 1:
            return dW, db, dx
        return (dW, db) + (_linear_cat_dx_raw(gy, ctx.saved_tensors) if need_dx else (None,) * nseg)


def linear_cat(xs, W, b):
    return LinearCatFn.apply(W, b, *xs)


def _surv_head_fwd_raw(feat, Wk, bk, out=None):
    """Classifier + hazards on feat [B x F] (mmf_surv_head_forward).  Returns out = (logits, hazards, S [B x K],
    Y_hat [B x 1]): the tensors given, or fresh ones."""
    B, F = feat.shape
    K = Wk.shape[0]
    if out is None:
        logits = torch.empty((B, K), dtype=torch.float32, device=feat.device)
        out = (logits, torch.empty_like(logits), torch.empty_like(logits),
               torch.empty((B, 1), dtype=torch.int64, device=feat.device))
    logits, hazards, S, Y_hat = out
    check(lib().mmf_surv_head_forward(ptr(feat), ptr(Wk), ptr(bk), B, F, K, ptr(logits), ptr(hazards),
                                      ptr(S), ptr(Y_hat), stream_ptr()), "mmf_surv_head_forward")
    return out


def _surv_head_bwd_raw(gH, gS, hazards, feat, Wk):
    """(dfeat, dWk, dbk) of a _surv_head_fwd_raw call (mmf_surv_head_backward); gH, gS: None where no gradient reaches."""
    B, F = feat.shape
    K = Wk.shape[0]
    gH, gS = _f32c(gH), _f32c(gS)
    dfeat = torch.empty_like(feat)
    dWk = torch.empty_like(Wk)
    dbk = torch.empty((K,), dtype=torch.float32, device=feat.device)
    check(lib().mmf_surv_head_backward(ptr(gH), ptr(gS), ptr(hazards), ptr(feat), ptr(Wk), B, F, K,
                                       ptr(dfeat), ptr(dWk), ptr(dbk), stream_ptr()), "mmf_surv_head_backward")
    return dfeat, dWk, dbk


class SurvHeadFn(torch.autograd.Function):
    """feat [B x F] -> hazards, S [B x K], Y_hat [B x 1] (models/model_attention_mil_path.py:58-61)."""

    @staticmethod
    def forward(ctx, feat, Wk, bk):
        feat, Wk, bk = _f32c(feat), _f32c(Wk), _f32c(bk)
        _, hazards, S, Y_hat = _surv_head_fwd_raw(feat, Wk, bk)
        ctx.save_for_backward(feat, Wk, hazards)
        ctx.mark_non_differentiable(Y_hat)
        ctx.set_materialize_grads(False)
        return hazards, S, Y_hat

    @staticmethod
    def backward(ctx, gH, gS, _gY):
        feat, Wk, hazards = ctx.saved_tensors
        return _surv_head_bwd_raw(gH, gS, hazards, feat, Wk)


def surv_head(feat, Wk, bk):
    return SurvHeadFn.apply(feat, Wk, bk)


class NllSurvFn(torch.autograd.Function):
    """utils/loss_utils.py:22-39; loss and both input gradients come out of one launch."""

    @staticmethod
    def forward(ctx, hazards, S, Y, c, alpha, eps):
        hazards, S = _f32c(hazards), _f32c(S)
        B, K = hazards.shape
        if not Y.is_cuda:       # labels still on the host: validate for free (the reference's gather raises IndexError);
            if bool(((Y < 0) | (Y >= K)).any()):       # device labels are checked by the kernel (NaN loss, no stray access)
                raise IndexError(f"nll_surv: label out of range [0, {K})")
        Y = Y.reshape(B).to(device=hazards.device, dtype=torch.int64).contiguous()
        c = c.reshape(B).to(device=hazards.device, dtype=torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=hazards.device)
        g = torch.empty((2, B, K), dtype=torch.float32, device=hazards.device)     # [d/d hazards ; d/d S]
        check(lib().mmf_nll_surv(ptr(hazards), ptr(S), ptr(Y), ptr(c), B, K, float(alpha), float(eps),
                                 ptr(loss), ptr(g[0]), ptr(g[1]), stream_ptr()), "mmf_nll_surv")
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (g,) = ctx.saved_tensors
        out = g * gl                      # one launch for both
        return out[0], out[1], None, None, None, None


def nll_surv(hazards, S, Y, c, alpha=0.4, eps=1e-7):
    return NllSurvFn.apply(hazards, S, Y, c, alpha, eps)


def surv_head_nll_step(feat, Wk, bk, Y, c, alpha, dWk, dbk, loss_scale=1.0, accumulate=False, eps=1e-7):
    """Classifier + hazard head + NLLSurvLoss(alpha) + their backward on a feature vector feat [1 x F] (F <= 1024) in ONE
    launch (mmf_surv_head_nll_step; models/model_mm_attention_mil.py:190-191 + utils/loss_utils.py:22-39): dWk / dbk get
    the gradient of loss * loss_scale (added when `accumulate`).
    Returns (hazards [1 x K], S [1 x K], Y_hat [1 x 1], loss (0-dim, unscaled), risk [1], dfeat [1 x F]), detached."""
    feat, Wk, bk = _f32c(feat), _f32c(Wk), _f32c(bk)
    F = feat.numel()
    K = Wk.shape[0]
    if Wk.shape[1] != F or F > 1024 or K > 32:
        raise _lib.MmfError("surv_head_nll_step: classifier does not match the feature vector (F <= 1024, K <= 32)")
    _check_grad_buffers(((dWk, Wk), (dbk, bk)))
    dev = feat.device
    hd, tg, (hz, S, Y_hat, loss, risk), _keep = _nll_head(Wk, bk, Y, c, alpha, eps, loss_scale, dWk, dbk, accumulate, dev)
    dfeat = torch.empty((1, F), dtype=torch.float32, device=dev)
    check(lib().mmf_surv_head_nll_step(ptr(feat), F, C.byref(hd), C.byref(tg), ptr(dfeat), stream_ptr()),
          "mmf_surv_head_nll_step")
    return hz, S, Y_hat, loss, risk, dfeat


class CoxSurvFn(torch.autograd.Function):
    """utils/loss_utils.py:124-139."""

    @staticmethod
    def forward(ctx, risks, times, c):
        shape = risks.shape
        r = _f32c(risks.reshape(-1))
        B = r.numel()
        t = times.reshape(B).to(device=r.device, dtype=torch.float64).contiguous()
        cc = c.reshape(B).to(device=r.device, dtype=torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=r.device)
        dr = torch.empty_like(r)
        check(lib().mmf_cox_surv(ptr(r), ptr(t), ptr(cc), B, ptr(loss), ptr(dr), stream_ptr()), "mmf_cox_surv")
        ctx.save_for_backward(dr)
        ctx.shape = shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (dr,) = ctx.saved_tensors
        return (dr * g).reshape(ctx.shape), None, None


def cox_surv(risks, times, c):
    return CoxSurvFn.apply(risks, times, c)


def maxnet_cox_step(x, W0, b0, W1, b1, Wc, bc, times, c, grads, loss_scale=1.0, accumulate=False, p_drop=0.0, seed=0):
    """MaxNet forward + CoxSurvLoss + backward of one batch in ONE launch (mmf_maxnet_cox_step; models/model_genomic.py:
    53-72 + utils/loss_utils.py:124-139).  times: float64 CUDA tensor [B]; grads: (dW0, db0, dW1, db1, dWc, dbc) tensors the
    gradients of loss * loss_scale are written to (or added to, `accumulate`).  Returns (risk [B], loss), detached."""
    x = _f32c(x)
    B, G = x.shape
    dev = x.device
    if times.dtype != torch.float64 or not times.is_cuda:
        raise _lib.MmfError("maxnet_cox_step: event times must be a float64 CUDA tensor")
    sw = sync_words(dev)
    if sw is None:
        raise _lib.MmfError("maxnet_cox_step needs tick words (ops.set_sync_override inside a stream capture)")
    cc = c.reshape(B).to(device=dev, dtype=torch.float32).contiguous()
    tt = times.reshape(B).contiguous()
    d = _lib.MaxnetDesc(B=B, G=G, H0=W0.shape[0], H1=W1.shape[0], x=ptr(x), W0=ptr(W0), b0=ptr(b0), W1=ptr(W1), b1=ptr(b1),
                        Wc=ptr(Wc), bc=ptr(bc), p_drop=float(p_drop), seed=int(seed) & 0xFFFFFFFF, seed_dev=ptr(_seed_word),
                        sync=ptr(sw), sync_words=SYNC_WORDS, trace=_trace)
    l = lib()
    nbytes = l.mmf_maxnet_cox_step_workspace_bytes(B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    risk = torch.empty((B,), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    g = _lib.MaxnetGrads(*[ptr(t) for t in grads])
    check(l.mmf_maxnet_cox_step(C.byref(d), ptr(tt), ptr(cc), float(loss_scale), ptr(ws), nbytes, ptr(risk), ptr(loss),
                                C.byref(g), 1 if accumulate else 0, stream_ptr()), "mmf_maxnet_cox_step")
    return risk, loss


DROP_KIND = {"none": 0, "dropout": 1, "alpha": 2}


def _dense_fwd_raw(x, W, b, act, kind, p, seed, site, word=None, out=None):
    """y = drop(act(x @ W.T + b)) (mmf_dense_forward) into out, or a fresh [B x N] tensor."""
    B, K = x.shape
    N = W.shape[0]
    y = torch.empty((B, N), dtype=torch.float32, device=x.device) if out is None else out
    check(lib().mmf_dense_forward(ptr(x), ptr(W), ptr(b), B, K, N, ACT[act], DROP_KIND[kind], float(p),
                                  int(seed) & 0xFFFFFFFF, int(site), ptr(word), ptr(y), stream_ptr()), "mmf_dense_forward")
    return y


def _dense_bwd_raw(gy, y, x, W, has_bias, act, kind, p, seed, site, need_dx=True, word=None):
    """(dx, dW, db) of a _dense_fwd_raw call (mmf_dense_backward); dx only when need_dx, db only with a bias."""
    B, K = x.shape
    N = W.shape[0]
    dpre = torch.empty_like(y)
    dx = torch.empty_like(x) if need_dx else None
    dW = torch.empty_like(W)
    db = torch.empty((N,), dtype=torch.float32, device=x.device) if has_bias else None
    check(lib().mmf_dense_backward(ptr(gy), ptr(y), ptr(x), ptr(W), B, K, N, ACT[act], DROP_KIND[kind], float(p),
                                   int(seed) & 0xFFFFFFFF, int(site), ptr(word), ptr(dpre), ptr(dx), ptr(dW), ptr(db),
                                   stream_ptr()), "mmf_dense_backward")
    return dx, dW, db


class DenseFn(torch.autograd.Function):
    """y = drop(act(x @ W.T + b)) for small / odd-shaped layers (SNN blocks, fusion MLPs, classifiers)."""

    @staticmethod
    def forward(ctx, x, W, b, act, drop_kind, drop_p, seed, site):
        x, W, b = _f32c(x), _f32c(W), _f32c(b)
        _, K = x.shape
        if W.shape[1] != K:
            raise _lib.MmfError(f"dense: weight {tuple(W.shape)} does not match input {tuple(x.shape)}")
        ctx.cfg = (act, drop_kind, drop_p, seed, site)
        ctx.seed_word = _seed_word
        ctx.has_bias = b is not None
        y = _dense_fwd_raw(x, W, b, *ctx.cfg, ctx.seed_word)
        ctx.save_for_backward(x, W, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, W, y = ctx.saved_tensors
        dx, dW, db = _dense_bwd_raw(_f32c(gy), y, x, W, ctx.has_bias, *ctx.cfg, ctx.needs_input_grad[0], ctx.seed_word)
        return dx, dW, db, None, None, None, None, None


def dense(x, W, b, act="none", drop_kind="none", drop_p=0.0, seed=0, site=0):
    return DenseFn.apply(x, W, b, act, drop_kind, drop_p, seed, site)


class GateMulFn(torch.autograd.Function):
    """sigmoid(z) * h (models/model_modules.py:163)."""

    @staticmethod
    def forward(ctx, z, h):
        z, h = _f32c(z), _f32c(h)
        o = torch.empty_like(h)
        check(lib().mmf_gate_mul_forward(ptr(z), ptr(h), ptr(o), h.numel(), stream_ptr()), "mmf_gate_mul_forward")
        ctx.save_for_backward(z, h)
        return o

    @staticmethod
    def backward(ctx, g):
        z, h = ctx.saved_tensors
        g = _f32c(g)
        dz, dh = torch.empty_like(z), torch.empty_like(h)
        check(lib().mmf_gate_mul_backward(ptr(g), ptr(z), ptr(h), ptr(dz), ptr(dh), h.numel(), stream_ptr()),
              "mmf_gate_mul_backward")
        return dz, dh


def gate_mul(z, h):
    return GateMulFn.apply(z, h)


def _kron_fwd_raw(os_, p, seed, site, word):
    """[o0,1] (x) [o1,1] ((x) [o2,1]) + dropout of the contiguous fp32 os_ ([B x dim] each) (mmf_kron_forward)."""
    m = len(os_)
    B, dim = os_[0].shape
    out = torch.empty((B, (dim + 1) ** m), dtype=torch.float32, device=os_[0].device)
    arr = (C.c_void_p * m)(*[ptr(o) for o in os_])
    check(lib().mmf_kron_forward(arr, m, dim, B, float(p), int(seed) & 0xFFFFFFFF, int(site), ptr(word), ptr(out),
                                 stream_ptr()), "mmf_kron_forward")
    return out


def _kron_bwd_raw(g, os_, p, seed, site, word):
    """The gradients of the os_ of a _kron_fwd_raw call (mmf_kron_backward)."""
    m = len(os_)
    B, dim = os_[0].shape
    ds = [torch.empty_like(o) for o in os_]
    arr = (C.c_void_p * m)(*[ptr(o) for o in os_])
    darr = (C.c_void_p * m)(*[ptr(d) for d in ds])
    check(lib().mmf_kron_backward(ptr(g), arr, m, dim, B, float(p), int(seed) & 0xFFFFFFFF, int(site), ptr(word), darr,
                                  stream_ptr()), "mmf_kron_backward")
    return ds


class KronFn(torch.autograd.Function):
    """[o0,1] (x) [o1,1] ((x) [o2,1]) + post-fusion Dropout (models/model_modules.py:164-171)."""

    @staticmethod
    def forward(ctx, drop_p, seed, site, *os_):
        os_ = [_f32c(o) for o in os_]
        ctx.cfg = (drop_p, seed, site, _seed_word)
        ctx.save_for_backward(*os_)
        return _kron_fwd_raw(os_, *ctx.cfg)

    @staticmethod
    def backward(ctx, g):
        return (None, None, None, *_kron_bwd_raw(_f32c(g), ctx.saved_tensors, *ctx.cfg))


def kron_ones(os_, drop_p=0.0, seed=0, site=0):
    return KronFn.apply(drop_p, seed, site, *os_)


class MlpFn(torch.autograd.Function):
    """A chain of dense layers as ONE autograd node (the omic head: SNN blocks + classifier,
    models/model_genomic.py:56-72): same dense kernels, one Python forward / backward instead of one per layer.
    spec: tuple of (act, drop_kind, drop_p, site) per layer; tensors: x, then (W, b) per layer."""

    @staticmethod
    def forward(ctx, spec, seed, x, *wb):
        x = _f32c(x)
        seed = int(seed) & 0xFFFFFFFF
        acts = [x]
        word = _seed_word
        for i, (act, kind, p, site) in enumerate(spec):
            acts.append(_dense_fwd_raw(acts[-1], wb[2 * i], wb[2 * i + 1], act, kind, p, seed, site, word))
        ctx.cfg = (spec, seed)
        ctx.seed_word = word
        ctx.save_for_backward(*acts, *wb)
        return acts[-1]

    @staticmethod
    def backward(ctx, g):
        spec, seed = ctx.cfg
        n = len(spec)
        t = ctx.saved_tensors
        acts, wb = t[:n + 1], t[n + 1:]
        g = _f32c(g)
        grads = [None] * (2 * n)
        for i in range(n - 1, -1, -1):
            act, kind, p, site = spec[i]
            need_dx = i > 0 or ctx.needs_input_grad[2]
            g, dW, db = _dense_bwd_raw(g, acts[i + 1], acts[i], wb[2 * i], wb[2 * i + 1] is not None, act, kind, p, seed,
                                       site, need_dx=need_dx, word=ctx.seed_word)
            grads[2 * i], grads[2 * i + 1] = dW, db
        return (None, None, g) + tuple(grads)


def mlp(x, layers, seed=0):
    """layers: list of (W, b, act, drop_kind, drop_p, site)."""
    spec = tuple((a, k, float(p), int(s)) for (_, _, a, k, p, s) in layers)
    wb = []
    for (W, b, *_r) in layers:
        wb += [W, b]
    return MlpFn.apply(spec, seed, x, *wb)


def _xreduce_io(m, vs, w, hs, zs, gms, os_):
    io = _lib.XReduceIO(m=m, B=vs[0].shape[0], dim=vs[0].shape[1], sdim=w[0].shape[0])
    for i in range(m):
        Wh, bh, Wz, bz, Wo, bo = w[6 * i:6 * i + 6]
        io.v[i] = ptr(vs[i]); io.Wh[i] = ptr(Wh); io.bh[i] = ptr(bh); io.Wz[i] = ptr(Wz); io.bz[i] = ptr(bz)
        io.Wo[i] = ptr(Wo); io.bo[i] = ptr(bo)
        io.h[i] = ptr(hs[i]); io.z[i] = ptr(zs[i]); io.gm[i] = ptr(gms[i]); io.o[i] = ptr(os_[i])
    return io


def _xfusion_fwd_raw(vs, w, p, seed):
    """The XlinearFusion block (XFusionFn) on vs (m tensors [B x dim]) with weights w: mmf_xreduce_forward, the Kronecker
    product, encoder1, encoder2.  Returns (e2, saved, state) for _xfusion_bwd_raw."""
    m = len(vs)
    vs = [_f32c(t) for t in vs]
    w = [_f32c(t) for t in w]
    kind = "dropout" if p > 0 else "none"
    seed = int(seed) & 0xFFFFFFFF
    B = vs[0].shape[0]
    sdim = w[0].shape[0]
    new = lambda: [torch.empty((B, sdim), dtype=torch.float32, device=vs[0].device) for _ in range(m)]
    hs, zs, gms, os_ = new(), new(), new(), new()
    io = _xreduce_io(m, vs, w, hs, zs, gms, os_)
    word = _seed_word
    check(lib().mmf_xreduce_forward(C.byref(io), float(p), seed, ptr(word), stream_ptr()), "mmf_xreduce_forward")
    We1, be1, We2, be2 = w[6 * m:6 * m + 4]
    kr = _kron_fwd_raw(os_, p, seed, 8, word)
    e1 = _dense_fwd_raw(kr, We1, be1, "relu", kind, p, seed, 9, word)
    cat2 = torch.cat([e1] + vs, dim=1)
    e2 = _dense_fwd_raw(cat2, We2, be2, "relu", kind, p, seed, 10, word)
    return e2, (*vs, *w, *hs, *zs, *gms, *os_, kr, e1, cat2, e2), (m, float(p), seed, kind, word)


def _xfusion_bwd_raw(g, saved, state):
    """The gradients of a _xfusion_fwd_raw call: (those of the vs, those of the weights in w's order)."""
    m, p, seed, kind, word = state
    t = list(saved)
    vs, t = t[:m], t[m:]
    w, t = t[:6 * m + 4], t[6 * m + 4:]
    hs, zs, gms, os_ = t[:m], t[m:2 * m], t[2 * m:3 * m], t[3 * m:4 * m]
    kr, e1, cat2, e2 = t[4 * m:4 * m + 4]
    We1, be1, We2, be2 = w[6 * m:6 * m + 4]
    g = _f32c(g)
    d_cat2, dWe2, dbe2 = _dense_bwd_raw(g, e2, cat2, We2, True, "relu", kind, p, seed, 10, word=word)
    H1 = e1.shape[1]
    d_e1 = d_cat2[:, :H1].contiguous()
    dim_v = vs[0].shape[1]
    d_kr, dWe1, dbe1 = _dense_bwd_raw(d_e1, e1, kr, We1, True, "relu", kind, p, seed, 9, word=word)
    d_os = _kron_bwd_raw(d_kr, os_, p, seed, 8, word)
    io = _xreduce_io(m, vs, w, hs, zs, gms, os_)
    dvs = [torch.empty_like(v) for v in vs]
    grads_w = []
    for i in range(m):
        Wh, bh, Wz, bz, Wo, bo = w[6 * i:6 * i + 6]
        gw = [torch.empty_like(x) for x in (Wh, bh, Wz, bz, Wo, bo)]
        io.d_o[i] = ptr(d_os[i]); io.dv[i] = ptr(dvs[i])
        io.dWh[i], io.dbh[i], io.dWz[i], io.dbz[i], io.dWo[i], io.dbo[i] = [ptr(x) for x in gw]
        grads_w += gw
    check(lib().mmf_xreduce_backward(C.byref(io), p, seed, ptr(word), stream_ptr()), "mmf_xreduce_backward")
    for i in range(m):      # skip connection: encoder2 saw the v_i directly
        dvs[i] += d_cat2[:, H1 + dim_v * i: H1 + dim_v * (i + 1)]
    return dvs, grads_w + [dWe1, dbe1, dWe2, dbe2]


class XFusionFn(torch.autograd.Function):
    """The whole XlinearFusion block (models/model_modules.py:156-178, gate=1, skip=1) as ONE autograd node: the same
    HIP kernels as the composable ops above, but one Python forward and one Python backward instead of ~25 nodes
    (the block is latency-bound; at B = 1 the autograd/ctypes dispatch dominated it).

    params: per modality (Wh, bh, Wz, bz, Wo, bo), then We1, be1, We2, be2.  Dropout sites: o_i -> i, post-fusion -> 8,
    encoder1 -> 9, encoder2 -> 10 (same as the composable path)."""

    @staticmethod
    def forward(ctx, m, p, seed, *tensors):
        e2, saved, ctx.state = _xfusion_fwd_raw(tensors[:m], tensors[m:], p, seed)
        ctx.save_for_backward(*saved)
        return e2

    @staticmethod
    def backward(ctx, g):
        dvs, dw = _xfusion_bwd_raw(g, ctx.saved_tensors, ctx.state)
        return (None, None, None, *dvs, *dw)


def xfusion(v_list, weights, p=0.0, seed=0):
    """weights: [Wh_0, bh_0, Wz_0, bz_0, Wo_0, bo_0, ..., We1, be1, We2, be2]."""
    return XFusionFn.apply(len(v_list), p, seed, *v_list, *weights)


# ---- stage-2 building blocks (include/mmf_amil.h "Stage-2 building blocks") -------------------------
class BatchNormFn(torch.autograd.Function):
    """y = dropout(act(BatchNorm1d(x) [+ res])) in one launch; running statistics are updated in place (training)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var, training, eps, momentum, act, drop_p, seed, site):
        x = _f32c(x)
        res = _f32c(res) if res is not None else None
        B, F = x.shape
        y = torch.empty_like(x)
        mean = torch.empty((F,), dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        word = _seed_word
        check(lib().mmf_batchnorm_forward(ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                                          B, F, 1 if training else 0, float(eps), float(momentum), ACT[act],
                                          float(drop_p), int(seed) & 0xFFFFFFFF, int(site), ptr(word), ptr(y), ptr(mean),
                                          ptr(invstd), stream_ptr()), "mmf_batchnorm_forward")
        ctx.cfg = (bool(training), act, float(drop_p), int(seed) & 0xFFFFFFFF, int(site), res is not None)
        ctx.seed_word = word
        ctx.save_for_backward(x, y, gamma, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, gamma, mean, invstd = ctx.saved_tensors
        training, act, drop_p, seed, site, has_res = ctx.cfg
        gy = _f32c(gy)
        B, F = x.shape
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if has_res else None
        dgamma = torch.empty_like(mean)
        dbeta = torch.empty_like(mean)
        check(lib().mmf_batchnorm_backward(ptr(gy), ptr(y), ptr(x), ptr(gamma), ptr(mean), ptr(invstd), B, F,
                                           1 if training else 0, ACT[act], drop_p, seed, site, ptr(ctx.seed_word),
                                           ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), stream_ptr()),
              "mmf_batchnorm_backward")
        return dx, dres, (dgamma if gamma is not None else None), (dbeta if gamma is not None else None), \
            None, None, None, None, None, None, None, None, None


def batchnorm(x, bn, res=None, act="none", drop_p=0.0, seed=0, site=0):
    """Apply an nn.BatchNorm1d module's parameters / buffers on the GPU (train or eval as bn.training says)."""
    training = bn.training or bn.running_mean is None
    if bn.training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    mom = 0.0 if bn.momentum is None else bn.momentum
    return BatchNormFn.apply(x, res, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.eps, mom, act,
                             drop_p, seed, site)


class HighwayMixFn(torch.autograd.Function):
    """models/model_modules.py:21-25: sigmoid(zg) * relu(zn) + (1 - sigmoid(zg)) * zl."""

    @staticmethod
    def forward(ctx, zg, zn, zl):
        zg, zn, zl = _f32c(zg), _f32c(zn), _f32c(zl)
        y = torch.empty_like(zg)
        check(lib().mmf_highway_mix_forward(ptr(zg), ptr(zn), ptr(zl), zg.numel(), ptr(y), stream_ptr()),
              "mmf_highway_mix_forward")
        ctx.save_for_backward(zg, zn, zl)
        return y

    @staticmethod
    def backward(ctx, gy):
        zg, zn, zl = ctx.saved_tensors
        gy = _f32c(gy)
        dzg, dzn, dzl = torch.empty_like(zg), torch.empty_like(zg), torch.empty_like(zg)
        check(lib().mmf_highway_mix_backward(ptr(gy), ptr(zg), ptr(zn), ptr(zl), zg.numel(), ptr(dzg), ptr(dzn), ptr(dzl),
                                             stream_ptr()), "mmf_highway_mix_backward")
        return dzg, dzn, dzl


def highway_mix(zg, zn, zl):
    return HighwayMixFn.apply(zg, zn, zl)


class RankLossFn(torch.autograd.Function):
    """utils/loss_utils.py:58-101; loss and d(risks) in one launch."""

    @staticmethod
    def forward(ctx, risks, times, c, phi, reduction):
        shape = risks.shape
        r = _f32c(risks.reshape(-1))
        B = r.numel()
        if B == 1:
            raise NotImplementedError("Batch size must be at least 2")          # as the reference (loss_utils.py:60-61)
        t = torch.as_tensor(times).reshape(B).to(device=r.device, dtype=torch.float64).contiguous()
        cc = c.reshape(B).to(device=r.device, dtype=torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=r.device)
        dr = torch.empty_like(r)
        check(lib().mmf_ranking_loss(ptr(r), ptr(t), ptr(cc), B, {"sigmoid": 0, "relu": 1}[phi],
                                     {"mean": 0, "sum": 1}[reduction], ptr(loss), ptr(dr), stream_ptr()), "mmf_ranking_loss")
        ctx.save_for_backward(dr)
        ctx.shape = shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (dr,) = ctx.saved_tensors
        return (dr * g).reshape(ctx.shape), None, None, None, None


def ranking_loss(risks, times, c, phi="sigmoid", reduction="mean"):
    return RankLossFn.apply(risks, times, c, phi, reduction)


class HazardFn(torch.autograd.Function):
    """logits -> (risk, hazards, S, Y_hat): models/nll_models_pretrained.py:58-62."""

    @staticmethod
    def forward(ctx, logits):
        logits = _f32c(logits)
        B, K = logits.shape
        hz, S = torch.empty_like(logits), torch.empty_like(logits)
        risk = torch.empty((B,), dtype=torch.float32, device=logits.device)
        Y_hat = torch.empty((B, 1), dtype=torch.int64, device=logits.device)
        check(lib().mmf_hazards_forward(ptr(logits), B, K, ptr(hz), ptr(S), ptr(Y_hat), ptr(risk), stream_ptr()),
              "mmf_hazards_forward")
        ctx.save_for_backward(hz)
        ctx.mark_non_differentiable(Y_hat)
        return risk, hz, S, Y_hat

    @staticmethod
    def backward(ctx, g_risk, g_hz, g_S, _gY):
        (hz,) = ctx.saved_tensors
        B, K = hz.shape
        f = lambda t: _f32c(t) if t is not None else None
        dl = torch.empty_like(hz)
        check(lib().mmf_hazards_backward(ptr(f(g_hz)), ptr(f(g_S)), ptr(f(g_risk)), ptr(hz), B, K, ptr(dl), stream_ptr()),
              "mmf_hazards_backward")
        return dl


def hazards_from_logits(logits):
    return HazardFn.apply(logits)
