"""GPU: the entry points the suite reached only through the models, over the shapes the header admits (tests/abi_shapes.py,
the tables below DENSE_BWD): mmf_dense_forward / _rows across the 64-lane tail and the 4 x 64 unrolled round of its K loop
and past the cap of its grid, mmf_gate_mul_*, mmf_kron_* around the forward's 256-thread blocks and the backward's 64
lanes, mmf_xreduce_* around wave_dot's 256-float round, a sweep of its 16 waves, the unroll of 16 and the 1024-thread
stride, and the omic head's one-launch step (mmf_maxnet_cox_step) over its three layer-0 routes, the rows a workgroup owns,
the Cox loop tiers, the risk-set stride and the censoring patterns.

Each entry point is called through ctypes on the inputs of tests/small_cases.py and judged against that module's float64
reference at the bar it derives there (the summation bound; for the omic step cut at the bar tests/test_gpu_maxnet_step.py
holds).  Forward and backward are separate tests where the ABI separates them: a backward kernel is given the reference's
forward outputs rounded to fp32, so no element is excused.  The omic step fuses both; its inputs keep every SELU unit far
from the kink instead (tests/test_abi_shapes_cpu.py asserts the margin), so no unit is excused there either.

Every output is a Guard view: after a call every output word has been written and every band is intact; a refused call
leaves everything canary.  Each accepted case runs twice and must give identical bits.  The omic step's workspace is a
Guard view too, filled with the canary (a NaN) before each call: a read of anything the call did not write itself would
poison the result.  Each comparison prints its worst error / bar ratio (SMALL-ERR lines; DESIGN.md holds the table)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import abi_shapes as ab
import small_cases as sc
from test_gpu_abi_shapes import Guard, _id, _lib, _p, _stream
from test_gpu_path import DEV, _t
from test_gpu_small_shapes import _Dev, _held, _judge, _refused, _twice

pytestmark = pytest.mark.gpu
f = C.c_float


def _acc(table, rule):
    return ab.accepted(table, rule)


def _ref(table, rule):
    return ab.refused(table, rule)


# ---- dense forward -------------------------------------------------------------------------------------------------------------
def _dense_fwd(c, g):
    from multimodalfusion_amd import ops
    d = _Dev()
    ok = ab.dense_fwd_rule(c) == ab.OK
    B, K, N = max(c.B, 1), max(c.K, 1), max(c.N, 1)
    i = sc.dense_fwd_inputs(c if ok else ab.DenseFwd(B, K, N))
    bias = d(i["b"]) if c.bias else None
    if not c.rows:
        out = dict(y=g.alloc((B, N), name="y"))
        rc = _lib().mmf_dense_forward(d(i["x"]), d(i["W"]), bias, c.B, c.K, c.N, c.act, c.drop_kind, f(c.drop_p), sc.SEED, sc.SITE,
                                      None, _p(out["y"]), _stream())
        return rc, out
    ld = N + c.rows if c.rows > 1 else N
    wide = g.alloc((B, ld), name="y (rows of a wider matrix)")
    base = ops.dropout_row_base(sc.dense_fwd_row_seeds(ab.DenseFwd(B, K, N)), DEV)
    rc = _lib().mmf_dense_forward_rows(d(i["x"]), d(i["W"]), bias, c.B, c.K, c.N, c.act, c.drop_kind, f(c.drop_p), sc.SITE, None,
                                       _p(base) if c.base else None, _p(wide), N - 1 if c.rows < 0 else ld, _stream())
    torch.cuda.synchronize()
    if ld > N:
        g.untouched(wide[:, N:], "the columns between the rows of y")
    return rc, dict(y=wide[:, :N])


@pytest.mark.parametrize("c", _acc(ab.DENSE_FWD, ab.dense_fwd_rule), ids=_id)
def test_dense_forward(c):
    ref, bar = sc.dense_fwd_ref(c)
    _judge("dense_forward", c, _twice(lambda g: _dense_fwd(c, g)), ref, bar, ("y",))


@pytest.mark.parametrize("c", _ref(ab.DENSE_FWD, ab.dense_fwd_rule), ids=_id)
def test_dense_forward_refusals_write_nothing(c):
    _refused(lambda g: _dense_fwd(c, g), ab.dense_fwd_rule(c))


# ---- gate_mul ----------------------------------------------------------------------------------------------------------------------
def _gate_fwd(c, g):
    d = _Dev()
    i = sc.gate_mul_inputs(ab.GateMul(max(c.n, 1)))
    out = dict(o=g.alloc((max(c.n, 1),), name="o"))
    return _lib().mmf_gate_mul_forward(d(i["z"]), d(i["h"]), _p(out["o"]), c.n, _stream()), out


def _gate_bwd(c, g):
    d = _Dev()
    i = sc.gate_mul_inputs(ab.GateMul(max(c.n, 1)))
    out = dict(dz=g.alloc((max(c.n, 1),), name="dz"), dh=g.alloc((max(c.n, 1),), name="dh"))
    return _lib().mmf_gate_mul_backward(d(i["g"]), d(i["z"]), d(i["h"]), _p(out["dz"]), _p(out["dh"]), c.n, _stream()), out


@pytest.mark.parametrize("c", _acc(ab.GATE_MUL, ab.gate_mul_rule), ids=_id)
def test_gate_mul_forward(c):
    ref, bar = sc.gate_mul_ref(c)
    _judge("gate_mul_forward", c, _twice(lambda g: _gate_fwd(c, g)), ref, bar, ("o",))


@pytest.mark.parametrize("c", _acc(ab.GATE_MUL, ab.gate_mul_rule), ids=_id)
def test_gate_mul_backward(c):
    ref, bar = sc.gate_mul_ref(c)
    _judge("gate_mul_backward", c, _twice(lambda g: _gate_bwd(c, g)), ref, bar, ("dz", "dh"))


@pytest.mark.parametrize("c", _ref(ab.GATE_MUL, ab.gate_mul_rule), ids=_id)
def test_gate_mul_refusals_write_nothing(c):
    _refused(lambda g: _gate_fwd(c, g), ab.gate_mul_rule(c))
    _refused(lambda g: _gate_bwd(c, g), ab.gate_mul_rule(c))


# ---- kron ------------------------------------------------------------------------------------------------------------------------
def _kron_data(c):
    """The case's inputs, or for a refused one those of a stand-in that has real buffers of a small size."""
    ok = ab.kron_rule(c) == ab.OK
    s = c if ok else ab.Kron(3, 4, B=1)
    return s, sc.kron_inputs(s)


def _kron_fwd(c, g):
    d = _Dev()
    s, i = _kron_data(c)
    n = max(c.m, 3)
    ptrs = [d(i["o"][t % s.m]).value for t in range(n)]
    if c.null:
        ptrs[c.m - 1] = None
    out = dict(out=g.alloc((s.B, (s.dim + 1) ** s.m), name="out"))
    rc = _lib().mmf_kron_forward((C.c_void_p * n)(*ptrs), c.m, c.dim, c.B, f(c.drop_p), sc.SEED, sc.SITE, None, _p(out["out"]), _stream())
    return rc, out


def _kron_bwd(c, g):
    d = _Dev()
    s, i = _kron_data(c)
    n = max(c.m, 3)
    ptrs = [d(i["o"][t % s.m]).value for t in range(n)]
    if c.null:
        ptrs[c.m - 1] = None
    out = {f"d{t}": g.alloc((s.B, s.dim), name=f"d_o[{t}]") for t in range(s.m)}
    dptr = [out[f"d{t % s.m}"].data_ptr() for t in range(n)]
    rc = _lib().mmf_kron_backward(d(i["g"]), (C.c_void_p * n)(*ptrs), c.m, c.dim, c.B, f(c.drop_p), sc.SEED, sc.SITE, None,
                                  (C.c_void_p * n)(*dptr), _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.KRON, ab.kron_rule), ids=_id)
def test_kron_forward(c):
    ref, bar = sc.kron_ref(c)
    got = _twice(lambda g: _kron_fwd(c, g))
    _judge("kron_forward", c, got, ref, bar, ("out",))
    assert not got["out"][~sc.kron_inputs(c)["keep"]].any()              # dropped elements are exact zeros


@pytest.mark.parametrize("c", _acc(ab.KRON, ab.kron_rule), ids=_id)
def test_kron_backward(c):
    ref, bar = sc.kron_ref(c)
    _judge("kron_backward", c, _twice(lambda g: _kron_bwd(c, g)), ref, bar, tuple(f"d{t}" for t in range(c.m)))


@pytest.mark.parametrize("c", [c for c in _ref(ab.KRON, ab.kron_rule) if (c.m, c.dim, c.B) not in ab.KRON_CAPS], ids=_id)
def test_kron_refusals_write_nothing(c):
    """The shapes the caps refuse are pinned on the CPU with pointers that are never read (tests/test_abi_shapes_cpu.py): a
    shape of that size is never given to a launch here."""
    _refused(lambda g: _kron_fwd(c, g), ab.kron_rule(c))
    _refused(lambda g: _kron_bwd(c, g), ab.kron_rule(c))


# ---- xreduce -----------------------------------------------------------------------------------------------------------------------
def _xr_data(c):
    s = c if 1 <= c.m <= 3 else dataclasses.replace(c, m=2)
    return s, sc.xreduce_inputs(s)


def _xr_io(c, g, d, bwd, fwd32=None):
    """(io, outputs): inputs on the device, every array the call writes a guarded view."""
    from multimodalfusion_amd import _lib as m_
    s, i = _xr_data(c)
    io = m_.XReduceIO(m=c.m, B=c.B, dim=c.dim, sdim=c.sdim)
    out = {}
    shapes = dict(dv=(s.B, s.dim), dWh=(s.sdim, s.dim), dbh=(s.sdim,), dWz=(s.sdim, s.m * s.dim), dbz=(s.sdim,), dWo=(s.sdim, s.sdim), dbo=(s.sdim,))
    for t in range(s.m):
        for k in ("v", "Wh", "bh", "Wz", "bz", "Wo", "bo"):
            if k == "v" and t == 0 and c.misalign:
                getattr(io, k)[t] = _held(g, i[k][t], "v[0], 4 bytes off", skew=1).data_ptr()
            else:
                getattr(io, k)[t] = d(i[k][t]).value
        for k in sc.XR_FWD_KEYS:
            if bwd:
                getattr(io, k)[t] = d(fwd32[k + "32"][t] if fwd32 else np.zeros((s.B, s.sdim), np.float32)).value
            else:
                out[f"{k}{t}"] = g.alloc((s.B, s.sdim), name=f"{k}[{t}]")
                getattr(io, k)[t] = out[f"{k}{t}"].data_ptr()
        if bwd:
            io.d_o[t] = d(i["d_o"][t]).value
            for k in sc.XR_BWD_KEYS:
                out[f"{k}{t}"] = g.alloc(shapes[k], name=f"{k}[{t}]")
                getattr(io, k)[t] = out[f"{k}{t}"].data_ptr()
    if c.null:
        getattr(io, c.null)[c.m - 1] = None
    return io, out


def _xr_fwd(c, g):
    d = _Dev()
    io, out = _xr_io(c, g, d, False)
    return _lib().mmf_xreduce_forward(C.byref(io), f(c.drop_p), sc.SEED, None, _stream()), out


def _xr_bwd(c, g, fwd32=None):
    d = _Dev()
    io, out = _xr_io(c, g, d, True, fwd32)
    return _lib().mmf_xreduce_backward(C.byref(io), f(c.drop_p), sc.SEED, None, _stream()), out


@pytest.mark.parametrize("c", _acc(ab.XREDUCE, ab.xreduce_fwd_rule), ids=_id)
def test_xreduce_forward(c):
    ref, bar = sc.xreduce_ref(c)
    got = _twice(lambda g: _xr_fwd(c, g))
    _judge("xreduce_forward", c, got, ref, bar, tuple(f"{k}{t}" for k in sc.XR_FWD_KEYS for t in range(c.m)))
    for t in range(c.m):
        assert not got[f"o{t}"][~sc.xreduce_inputs(c)["keep"][t]].any()


@pytest.mark.parametrize("c", _acc(ab.XREDUCE, ab.xreduce_bwd_rule), ids=_id)
def test_xreduce_backward(c):
    ref, bar = sc.xreduce_ref(c)
    got = _twice(lambda g: _xr_bwd(c, g, ref))
    _judge("xreduce_backward", c, got, ref, bar, tuple(f"{k}{t}" for k in sc.XR_BWD_KEYS for t in range(c.m)))


@pytest.mark.parametrize("c", _ref(ab.XREDUCE, ab.xreduce_fwd_rule), ids=_id)
def test_xreduce_refusals_write_nothing(c):
    _refused(lambda g: _xr_fwd(c, g), ab.xreduce_fwd_rule(c))
    if ab.xreduce_bwd_rule(c) != ab.OK:
        _refused(lambda g: _xr_bwd(c, g), ab.xreduce_bwd_rule(c))


# ---- the omic step -------------------------------------------------------------------------------------------------------------------
MX_SHAPES = dict(dW0=None, db0=(256,), dW1=(256, 256), db1=(256,), dWc=(1, 256), dbc=(1,))


def _maxstep(c, g, ws=None):
    """One call -> (rc, outputs, (tick words, workspace)).  ws: a workspace to reuse (else a guarded, canary-filled one of
    exactly the queried size)."""
    from multimodalfusion_amd import _lib as m_
    d = _Dev()
    ok = ab.maxstep_rule(c) == ab.OK
    s = c if ok else ab.MaxStep(8, 36)
    i = sc.maxstep_inputs(s)
    ptr = {k: d(i[k]) for k in ("x", "b0", "W1", "b1", "Wc", "bc", "c")}
    ptr["W0"] = _p(_held(g, i["W0"], "W0", skew=1 if c.misalign else 0))
    ptr["times"] = d(i["times"], torch.float64)
    sync = g.alloc((3,), torch.int32, name="tick words")
    sync.zero_()
    ptr["sync"] = _p(sync)
    wsb = _lib().mmf_maxnet_cox_step_workspace_bytes(s.B)
    assert wsb == ab.maxstep_workspace_bytes(s.B)
    if ws is None:
        ws = g.alloc((wsb,), torch.uint8, name="workspace")
    ptr["workspace"] = _p(ws)
    out = dict(risk=g.alloc((s.B,), name="risk"), loss=g.alloc((1,), name="loss"))
    for k, shape in MX_SHAPES.items():
        shape = shape or (256, s.G)
        out[k] = _held(g, i["prior"][k], k) if s.accumulate else g.alloc(shape, name=k)
    for k in ("risk", "loss") + sc.MX_GRADS:
        ptr[k] = _p(out[k])
    word = d(np.array([s.word], np.int32), torch.int32) if s.word else None
    if c.null:
        ptr[c.null] = None
    if c.off:                              # refused before anything is read: the pointer itself, 4 bytes on
        ptr[c.off] = C.c_void_p(ptr[c.off].value + 4)
    desc = m_.MaxnetDesc(B=c.B, G=c.G, H0=c.H0, H1=256, p_drop=c.p_drop, seed=sc.MX_SEED, seed_dev=word, sync_words=c.sync_words, trace=None,
                         **{k: ptr[k] for k in ("x", "W0", "b0", "W1", "b1", "Wc", "bc", "sync")})
    grads = m_.MaxnetGrads(**{k: ptr[k] for k in sc.MX_GRADS})
    rc = _lib().mmf_maxnet_cox_step(C.byref(desc), ptr["times"], ptr["c"], f(c.loss_scale), ptr["workspace"], wsb - (1 if c.ws_short else 0),
                                    ptr["risk"], ptr["loss"], C.byref(grads), c.accumulate, _stream())
    torch.cuda.synchronize()
    assert int(sync.abs().sum()) == 0, "the tick words are not zero after the call"
    return rc, out, ws


def _maxstep_checked(c):
    ref, bar, _ = sc.maxstep_ref(c)
    got = _twice(lambda g: _maxstep(c, g)[:2])
    got["loss"] = got["loss"][0]
    _judge("maxnet_cox_step", c, got, ref, bar, ("risk", "loss") + sc.MX_GRADS)
    return got


@pytest.mark.parametrize("c", _acc(ab.MAXSTEP, ab.maxstep_rule), ids=_id)
def test_maxnet_cox_step(c):
    got = _maxstep_checked(c)
    if c.censor == "all":                  # F3: 1 / D_i with every 1 - c = 0 gives exact zeros, not NaN
        assert got["loss"] == 0 and all(not got[k].any() for k in sc.MX_GRADS)
    if c.misalign:                         # the same shape with W0 aligned takes the narrow route: the same numbers to the bar
        twin = dataclasses.replace(c, misalign=False)
        assert ab.maxstep_route(twin) == "narrow" != ab.maxstep_route(c)
        _maxstep_checked(twin)


def test_maxnet_cox_step_reads_nothing_an_earlier_larger_call_left():
    """F4: B = 256, then B = 5 in the same workspace -- bit-identical to B = 5 in a workspace that holds only canaries."""
    big = [c for c in _acc(ab.MAXSTEP, ab.maxstep_rule) if c.B == 256][0]
    small = dataclasses.replace([c for c in _acc(ab.MAXSTEP, ab.maxstep_rule) if c.B == 5][0], misalign=False)
    g = Guard()
    rc, _, ws = _maxstep(big, g)
    assert rc == ab.OK
    rc, used, _ = _maxstep(small, g, ws=ws)
    assert rc == ab.OK
    rc, fresh, _ = _maxstep(small, g)
    assert rc == ab.OK
    g.check()
    for k in used:
        g.written(used[k], k)
        assert torch.equal(Guard.words(used[k]), Guard.words(fresh[k])), f"{k} depends on what the workspace held"


@pytest.mark.parametrize("c", _ref(ab.MAXSTEP, ab.maxstep_rule), ids=_id)
def test_maxnet_cox_step_refusals_write_nothing(c):
    g = Guard()
    rc, out, ws = _maxstep(c, g)
    assert rc == ab.maxstep_rule(c) != ab.OK, (rc, c)
    for k, t in out.items():
        g.untouched(t, k)
    g.untouched(ws, "workspace")
    g.check()
