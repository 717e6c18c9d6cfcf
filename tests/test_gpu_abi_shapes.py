"""GPU: the scorer, the dense layer and the stack over the shapes the C ABI admits (tests/abi_shapes.py), not only the
dimensions of the three shipped models -- one-chunk, odd-count and four-chunk K loops, ragged attention-dim and output
column tiles, segmented inputs that leave the deep loop, two-way K splits, D = 128 / 640 and H = 1024 stacks -- each
against a float64 reference of the same operation at the bars the suite already holds for the shipped dimensions.

Every output is a view inside a larger buffer filled with a canary word (Guard): after the call every word of the output
has been written and the 256-byte bands in front of and behind it still hold the canary, which is how a store outside a
buffer shows itself without a fault.  Calls that go through ops / the modules allocate with torch.empty, which
Guard.patch() turns into guarded views: their workspaces, outputs and gradient buffers are all checked the same way.
Refused shapes return their code before any launch and leave the output untouched."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import abi_shapes as ab
from oracle import cases
from oracle import inputs as gen
from oracle import torch_port as tp
from test_gpu_attn_net import _case as scorer_case
from test_gpu_bf16 import _oracle as bf16_oracle
from test_gpu_bf16 import _xq, compare_bf16, run_path_hip_bf16
from test_gpu_group_step import _bag_meta, check_group, group_oracle, run_group
from test_gpu_path import DEV, _grads, _load, _t, compare, relu_kink_units, run_path_hip

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5          # a quiet NaN with a payload: no kernel computes it
BAND = 64                    # guard band, in 32-bit words, on each side: 256 bytes, so views stay 16-byte aligned


class Guard:
    """Canary-filled buffers with a view in the middle."""

    def __init__(self):
        self.bufs = []

    def alloc(self, shape, dtype=torch.float32, skew=0, name="buffer"):
        """A `shape` view of `dtype`, `skew` words past a 16-byte boundary, inside a canary-filled buffer."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        words = (nbytes + 3) // 4
        buf = torch.full((BAND + skew + words + BAND,), CANARY, dtype=torch.int32, device=DEV)
        self.bufs.append((buf, BAND + skew, words, name))
        return buf[BAND + skew:BAND + skew + words].view(torch.uint8)[:nbytes].view(dtype).view(shape)

    @staticmethod
    def words(t):
        return t.detach().contiguous().reshape(-1).view(torch.int32)

    def owns(self, t):
        """t lies wholly inside the view of one guarded buffer."""
        a, b = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        return any(buf.data_ptr() + 4 * lead <= a and b <= buf.data_ptr() + 4 * (lead + words)
                   for buf, lead, words, _ in self.bufs)

    def written(self, t, name, owned=True):
        """No word of t still holds the canary.  owned: t itself must be memory this Guard handed out -- on any other
        tensor the check would pass whatever the kernels did.  owned=False is for a parameter's .grad only, which
        autograd may have copied out of the (guarded) buffer the kernels wrote: a copy carries unwritten canaries along."""
        assert not owned or self.owns(t), f"{name} is not in a guarded buffer: its bands and canaries check nothing"
        left = int((self.words(t) == CANARY).sum())
        assert left == 0, f"{name}: {left} of {t.numel()} elements were never written"

    def untouched(self, t, name):
        assert bool((self.words(t) == CANARY).all()), f"{name} was written by a refused call"

    def check(self):
        """Every guard band still holds the canary, bit for bit."""
        torch.cuda.synchronize()
        for buf, lead, words, name in self.bufs:
            assert bool((buf[:lead] == CANARY).all()), f"{name}: the band in FRONT of the buffer was written"
            assert bool((buf[lead + words:] == CANARY).all()), f"{name}: the band BEHIND the buffer was written"

    @contextlib.contextmanager
    def patch(self, monkeypatch):
        """torch.empty / torch.empty_like (the only forms ops.py and models/ allocate device memory with) hand out
        guarded views while the block runs; CPU tensors (the oracle's) are left alone."""
        empty, empty_like = torch.empty, torch.empty_like

        def wrap(t):
            if torch.is_tensor(t) and t.is_cuda and t.numel():
                return self.alloc(t.shape, t.dtype, name=f"torch.empty{tuple(t.shape)} {t.dtype}")
            return t
        with monkeypatch.context() as mp:
            mp.setattr(torch, "empty", lambda *a, **kw: wrap(empty(*a, **kw)))
            mp.setattr(torch, "empty_like", lambda *a, **kw: wrap(empty_like(*a, **kw)))
            n0 = len(self.bufs)
            yield self
            torch.cuda.synchronize()
        assert len(self.bufs) > n0, "the call allocated nothing through torch.empty"


def _lib():
    from multimodalfusion_amd import _lib as m
    return m.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _id(c):
    return c.why


# =======================================================================================================================
# mmf_linear_forward
# =======================================================================================================================
SEED, SITE = 321, 1
ACT_REF = {0: lambda v: v, 1: lambda v: np.maximum(v, 0), 2: np.tanh, 3: lambda v: 1 / (1 + np.exp(-v)),
           4: lambda v: 1.0507009873554805 * np.where(v > 0, v, 1.6732632423543772 * (np.exp(v) - 1))}


def _lin_inputs(M, N, nseg, kseg):
    xs = [gen.normal(31 + i, (M, kseg), stream=i) for i in range(nseg)]
    W = gen.normal(41, (N, nseg * kseg), stream=5, std=1.0 / np.sqrt(nseg * kseg))       # pre-activations of unit scale
    b = gen.normal(42, (N,), stream=6, std=0.3)
    return xs, W, b


def _lin_forward(c, txs, tW, tb, y, g, ws):
    from multimodalfusion_amd import ops
    l = _lib()
    segs = (C.c_void_p * len(txs))(*[x.data_ptr() for x in txs])
    wsb = l.mmf_linear_forward_workspace_bytes(c.M, c.N, c.nseg, c.kseg) if ws else 0
    wst = g.alloc(wsb, torch.uint8, name="K-split workspace") if wsb else None
    sw = ops.sync_words(DEV) if wsb else None
    rc = l.mmf_linear_forward(segs, c.nseg, c.kseg, c.M, _p(tW), _p(tb), c.N, c.act, C.c_float(c.drop_p), SEED, SITE, None,
                              _p(y), _p(wst), wsb, _p(sw), ops.SYNC_WORDS if wsb else 0, _stream())
    torch.cuda.synchronize()
    if sw is not None:
        assert int(sw.abs().sum()) == 0, "the tick words are not zero after the call"
    return rc, wsb


def _lin_reference(c, xs, W, b):
    pre = np.concatenate(xs, axis=1).astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    ref = ACT_REF[c.act](pre)
    if c.drop_p > 0:
        ref = np.where(gen.keep_mask(SEED, SITE, c.M, c.N, c.drop_p), ref / (1 - c.drop_p), 0.0)
    return ref


@pytest.mark.parametrize("c", ab.accepted(ab.LINEAR_FORWARD, ab.linear_forward_rule), ids=_id)
def test_linear_forward(c):
    """Bars: test_linear_forward_abi_all_activations_large's (rtol 1e-4, atol 2e-5); a K-split call also against the
    same call without workspace, to fp32 rounding (test_gpu_ksplit.py's rtol 1e-5, atol 2e-5)."""
    xs, W, b = _lin_inputs(c.M, c.N, c.nseg, c.kseg)
    txs, tW, tb = [_t(x) for x in xs], _t(W), _t(b)
    g = Guard()
    y = g.alloc((c.M, c.N), name="y")
    rc, wsb = _lin_forward(c, txs, tW, tb, y, g, c.ws)
    assert rc == ab.OK
    if c.ws:
        assert wsb == ab.linear_ksplit(c.M, c.N, c.K, c.nseg, c.kseg) * ((c.M + 63) // 64) * ((c.N + 63) // 64) * 64 * 64 * 4 > 0
    g.written(y, "y")
    g.check()
    np.testing.assert_allclose(y.cpu().numpy(), _lin_reference(c, xs, W, b), rtol=1e-4, atol=2e-5)
    if c.ws:
        y0 = g.alloc((c.M, c.N), name="y (unsplit)")
        assert _lin_forward(c, txs, tW, tb, y0, g, False) == (ab.OK, 0)
        g.written(y0, "y (unsplit)")
        g.check()
        np.testing.assert_allclose(y.cpu().numpy(), y0.cpu().numpy(), rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("c", ab.refused(ab.LINEAR_FORWARD, ab.linear_forward_rule), ids=_id)
def test_linear_forward_refusals_leave_y_untouched(c):
    """y is M x (N rounded up to 4) and the bias N rounded up to 4, so that the float4 accesses of a call that was NOT
    refused would still stay inside the allocations."""
    n4 = (c.N + 3) // 4 * 4
    nseg = max(c.nseg, 1)
    xs, W, b = _lin_inputs(c.M, n4, nseg, c.kseg)
    txs, tW = [_t(x) for x in xs], _t(W)
    bias = _t(np.concatenate([b, b[:4]]))
    g = Guard()
    y = g.alloc(c.M * n4, skew=1 if c.misalign == "y" else 0, name="y")
    tb = bias[1:1 + n4] if c.misalign == "bias" else bias[:n4]
    assert (y.data_ptr() % 16 != 0) == (c.misalign == "y") and (tb.data_ptr() % 16 != 0) == (c.misalign == "bias")
    rc, _ = _lin_forward(c, txs, tW, tb, y, g, False)
    assert rc == ab.linear_forward_rule(c) != ab.OK
    g.untouched(y, "y")
    g.check()


def test_linear_cat_autograd_on_a_ragged_segmented_shape(monkeypatch):
    """ops.linear_cat forward + backward at (M, N, nseg, kseg) = (65, 36, 3, 96), every allocation guarded; bars of
    test_linear_cat_matches_torch."""
    from multimodalfusion_amd import ops
    M, N, nseg, kseg = 65, 36, 3, 96
    xs, W, b = _lin_inputs(M, N, nseg, kseg)
    gy = gen.normal(6, (M, N), stream=1)
    tW, tb = _t(W).requires_grad_(True), _t(b).requires_grad_(True)
    g = Guard()
    with g.patch(monkeypatch):
        y = ops.linear_cat([_t(x) for x in xs], tW, tb)
        y.backward(_t(gy))
    g.check()
    g.written(y, "y")
    for name, t in (("dW", tW.grad), ("db", tb.grad)):
        g.written(t, name, owned=False)
    rW, rb = torch.as_tensor(W).double().requires_grad_(True), torch.as_tensor(b).double().requires_grad_(True)
    ry = torch.nn.functional.linear(torch.cat([torch.as_tensor(x).double() for x in xs], 1), rW, rb)
    ry.backward(torch.as_tensor(gy).double())
    np.testing.assert_allclose(y.detach().cpu().numpy(), ry.detach().numpy(), atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(tW.grad.cpu().numpy(), rW.grad.numpy(), atol=1e-5 * max(float(rW.grad.abs().max()), 1), rtol=1e-4)
    np.testing.assert_allclose(tb.grad.cpu().numpy(), rb.grad.numpy(), atol=1e-4, rtol=1e-4)


# =======================================================================================================================
# mmf_linear_backward
# =======================================================================================================================
def _lin_backward(c, g):
    l = _lib()
    xs, W, _ = _lin_inputs(c.M, c.N, c.nseg, c.kseg)
    dy = gen.normal(6, (c.M, c.N), stream=1)
    txs, tW, tdy = [_t(x) for x in xs], _t(W), _t(dy)
    dW = g.alloc((c.N, c.K), name="dW")
    db = g.alloc((c.N,), name="db") if c.db else None
    dx = g.alloc((c.M, c.K), name="dx") if c.dx else None
    nbytes = l.mmf_linear_backward_workspace_bytes(c.M, c.N, c.K)
    ws = g.alloc(nbytes, torch.uint8, name="workspace")
    segs = (C.c_void_p * len(txs))(*[x.data_ptr() for x in txs])
    rc = l.mmf_linear_backward(_p(tdy), segs, c.nseg, c.kseg, c.M, _p(tW), c.N, _p(dW), _p(db), _p(dx), _p(ws), nbytes, _stream())
    torch.cuda.synchronize()
    return rc, nbytes, (xs, W, dy), (dW, db, dx)


@pytest.mark.parametrize("c", ab.accepted(ab.LINEAR_BACKWARD, ab.linear_backward_rule), ids=_id)
def test_linear_backward(c):
    """Against fp64 torch autograd; bars of test_linear_cat_matches_torch (dW: rtol 1e-4, atol 1e-5 max(|dW|max, 1);
    db: rtol 1e-4, atol 1e-4).  The project has no bar for dx of this entry point yet: the one used here is dW's, chosen
    by reasoning, not taken from an existing test -- dx = dy . W is an fp32 MFMA GEMM of the same kind over a K of at
    most 256 terms of unit scale, where dW sums up to 1000."""
    g = Guard()
    rc, nbytes, (xs, W, dy), (dW, db, dx) = _lin_backward(c, g)
    assert rc == ab.OK
    assert (nbytes > 256) == (ab.linear_bwd_splits(c.M, c.N, c.K) > 1)
    g.check()
    rx = torch.cat([torch.as_tensor(x).double() for x in xs], 1).requires_grad_(True)
    rW, rb = torch.as_tensor(W).double().requires_grad_(True), torch.zeros(c.N, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.linear(rx, rW, rb).backward(torch.as_tensor(dy).double())
    for name, got, ref in (("dW", dW, rW.grad), ("db", db, rb.grad), ("dx", dx, rx.grad)):
        if got is None:
            continue
        g.written(got, name)
        atol = 1e-4 if name == "db" else 1e-5 * max(float(ref.abs().max()), 1.0)
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=atol, err_msg=name)


@pytest.mark.parametrize("c", ab.refused(ab.LINEAR_BACKWARD, ab.linear_backward_rule), ids=_id)
def test_linear_backward_refusals_write_nothing(c):
    g = Guard()
    rc, _, _, outs = _lin_backward(c, g)
    assert rc == ab.linear_backward_rule(c) != ab.OK
    for name, t in zip(("dW", "db", "dx"), outs):
        if t is not None:
            g.untouched(t, name)
    g.check()


# =======================================================================================================================
# mmf_attn_net_forward / _backward
# =======================================================================================================================
MASK_SEED = 5151


@pytest.mark.parametrize("c", ab.accepted(ab.ATTN, ab.attn_rule), ids=_id)
def test_attn_net(c, monkeypatch):
    """The scorer modules on bare tensors against oracle.torch_port.attn_net in fp64; bars of tests/test_gpu_attn_net.py
    (scores 1e-4, gradients 1e-5 + 1e-4 max|g|)."""
    from multimodalfusion_amd import ops
    net, sd, x, gA = scorer_case(c.N, c.H, c.D, c.gated, c.dropout, c.dropout, seed=100 + c.N + c.H)
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: MASK_SEED)
    xt = _t(x).requires_grad_(c.dx)
    g = Guard()
    with g.patch(monkeypatch):
        A, x_out = net(xt)
        A.backward(_t(gA))
    g.check()
    assert x_out is xt and tuple(A.shape) == (c.N, 1) and (xt.grad is not None) == c.dx
    masks = None
    if c.dropout:
        masks = {"a": torch.as_tensor(gen.drop_scale_mask(MASK_SEED, 1, c.N, c.D, 0.25, np.float64))}
        if c.gated:
            masks["b"] = torch.as_tensor(gen.drop_scale_mask(MASK_SEED, 2, c.N, c.D, 0.25, np.float64))
    tsd = tp.to_torch({"s." + k: v for k, v in sd.items()}, torch.float64)
    xr = torch.as_tensor(x).double().requires_grad_(True)
    A_r, _ = tp.attn_net(tsd, "s", xr, c.gated, c.dropout, masks)
    A_r.backward(torch.as_tensor(gA).double())
    g.written(A, "A")
    np.testing.assert_allclose(A.detach().cpu().numpy(), A_r.detach().numpy(), rtol=0, atol=1e-4)
    got = {k: p.grad for k, p in net.named_parameters()}
    ref = {k[2:]: v.grad.numpy() for k, v in tsd.items()}
    if c.dx:
        got["x"], ref["x"] = xt.grad, xr.grad.numpy()
    for k, r in ref.items():
        g.written(got[k], k, owned=False)
        tol = 1e-5 + 1e-4 * float(np.abs(r).max())
        err = float(np.abs(got[k].cpu().numpy() - r).max())
        assert err <= tol, (k, err, tol)


# =======================================================================================================================
# the stack, fp32: mmf_amil_head_forward + mmf_amil_backward (autograd), mmf_amil_infer, mmf_amil_nll_step
# =======================================================================================================================
def _admit(monkeypatch, size):
    """The model classes look their widths up by name: give the explicit (L, H, D) a name of its own."""
    from multimodalfusion_amd.models import model_modules
    monkeypatch.setitem(model_modules.AMIL_SIZES, tuple(size), tuple(size))


def _stack_meta(c, N, train):
    return dict(N=N, gated=c.gated, size=c.size, K=4, dropout=train, y=N % 4, c=N % 2, alpha=0.15, bias_std=0.05, train=train,
                seed=4300 + c.L + c.D, x_seed=5300 + N, mask_seed=977)


@functools.lru_cache(maxsize=None)
def _stack_reference(c, N, train):
    """The fp64 oracle of one (shape, bag, mode), computed once for both gemm modes and left unchanged."""
    m = _stack_meta(c, N, train)
    sd, x, _ = cases.path_inputs(m)
    return cases.run_path(m), relu_kink_units(sd, x)


def _nll_step_hip(m, monkeypatch):
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    sd, x, _ = cases.path_inputs(m)
    model = _load(MIL_Attention_fc_surv_path(gate_path=m["gated"], model_size_wsi=m["size"], dropout=m["dropout"],
                                             n_classes=m["K"]), sd)
    model.train() if m["train"] else model.eval()
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: m["mask_seed"])
    hz, S, Yh, A, loss, risk = model.nll_step(_t(x), torch.tensor([m["y"]]), torch.tensor([float(m["c"])]), alpha=m["alpha"])
    torch.cuda.synchronize()
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), A_raw=A.cpu().numpy(), loss=float(loss), M=None,
                grads=_grads(model)), (hz, S, Yh, A, loss, risk)


@pytest.mark.parametrize("gemm", [0, 1], ids=["f32", "bf16x3"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("N", ab.STACK_BAGS)
@pytest.mark.parametrize("c", ab.accepted(ab.STACK_F32, ab.stack_rule), ids=_id)
def test_stack_f32(c, N, train, gemm, monkeypatch):
    """Both routes of one bag -- the autograd surface (and, in eval mode, the forward-only embedding) and the one-call
    step -- in both gemm modes against the fp64 oracle with the same hash masks; compare() of tests/test_gpu_path.py.
    Where L % 64 != 0 the bf16x3 projection is the exact-fp32 tiles (abi_shapes.split_core): same bars."""
    from multimodalfusion_amd import ops
    _admit(monkeypatch, c.size)
    m = _stack_meta(c, N, train)
    ref, kinks = _stack_reference(c, N, train)
    prev = ops.set_gemm(gemm)
    try:
        g = Guard()
        with g.patch(monkeypatch):
            res = run_path_hip(m, monkeypatch)
        g.check()
        compare(res, ref, f"autograd {c.size} N={N}", kink_units=kinks)
        g = Guard()
        with g.patch(monkeypatch):
            step, outs = _nll_step_hip(m, monkeypatch)
        g.check()
        for name, t in zip(("hazards", "S", "Y_hat", "A_raw", "loss", "risk"), outs):
            g.written(t, name)
        compare(step, ref, f"nll_step {c.size} N={N}", kink_units=kinks)
    finally:
        ops.set_gemm(prev)
    for k, v in res["grads"].items():
        assert np.isfinite(v).all() and np.isfinite(step["grads"][k]).all(), k


# =======================================================================================================================
# the grouped entry points
# =======================================================================================================================
@pytest.mark.parametrize("entry,sizes,size,gated", ab.GROUPED, ids=[f"{e} {s} {'gated' if g else 'ungated'}" for e, _, s, g in ab.GROUPED])
def test_grouped_entry_points(entry, sizes, size, gated, monkeypatch):
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    _admit(monkeypatch, size)
    train = entry == "mmf_amil_nll_step_group"
    base = dict(gated=gated, size=size, K=4, dropout=train, alpha=0.3, bias_std=0.05, train=train, seed=4242, x_seed=500,
                mask_seed=900)
    metas = [_bag_meta(base, i, n) for i, n in enumerate(sizes)]
    refs, kinks = group_oracle(metas)
    g = Guard()
    if train:
        scale = 1.0 / len(sizes)
        with g.patch(monkeypatch):
            res, _, _ = run_group(metas, monkeypatch, scale)
        g.check()
        check_group(res, scale, refs, kinks)
        return
    from test_gpu_group_step import _model
    model, _ = _model(metas[0])
    bags = [_t(cases.path_inputs(mm)[1]) for mm in metas]
    Y, cc = torch.tensor([mm["y"] for mm in metas]), torch.tensor([float(mm["c"]) for mm in metas])
    with g.patch(monkeypatch):
        hz, S, Yh, A, loss, risk = model.forward_group(bags, Y, cc, alpha=0.3)
        M = model.forward_group(bags, return_features=True)
    g.check()
    for name, t in (("hazards", hz), ("S", S), ("Y_hat", Yh), ("loss", loss), ("risk", risk), ("M", M)):
        g.written(t, name)
    for i, ref in enumerate(refs):
        one = dict(hazards=hz[i:i + 1].cpu().numpy(), S=S[i:i + 1].cpu().numpy(), A_raw=A[i].cpu().numpy(), loss=float(loss[i]),
                   M=M[i:i + 1].cpu().numpy(), grads={})
        compare(one, dict(ref, grads={}), f"bag {i}")
        assert abs(float(risk[i]) + float(S[i].sum())) < 1e-5


# =======================================================================================================================
# the stack, bf16 storage
# =======================================================================================================================
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("N", ab.BF16_BAGS)
@pytest.mark.parametrize("c", ab.accepted(ab.STACK_BF16, ab.stack_rule), ids=_id)
def test_stack_bf16(c, N, train, monkeypatch):
    """Against oracle/bf16_port.path_step_bf16 (the kernels' rounding points) at compare_bf16's bars against that oracle
    (tests/test_gpu_bf16.py: scores 5e-3, hazards 2e-3, loss 1e-3, gradients 1 % in norm)."""
    _admit(monkeypatch, c.size)
    m = _stack_meta(c, N, train)
    xq = _xq(m)
    g = Guard()
    with g.patch(monkeypatch):
        res = run_path_hip_bf16(m, monkeypatch, xq)
    g.check()
    compare_bf16(res, bf16_oracle(m, xq), f"bf16 {c.size} N={N}", a_tol=5e-3, h_tol=2e-3, l_tol=1e-3, g_rel=1e-2)


# =======================================================================================================================
# refused stack and scorer widths: the code, through the ops layer's error
# =======================================================================================================================
@pytest.mark.parametrize("c", ab.refused(ab.STACK_F32, ab.stack_rule) + ab.refused(ab.STACK_BF16, ab.stack_rule), ids=_id)
def test_stack_refusals(c, monkeypatch):
    from multimodalfusion_amd import _lib
    _admit(monkeypatch, c.size)
    m = _stack_meta(c, 65, False)
    with pytest.raises(_lib.MmfError, match=r"code -2"):
        if c.bf16:
            run_path_hip_bf16(m, monkeypatch, _xq(m))
        else:
            run_path_hip(m, monkeypatch)
