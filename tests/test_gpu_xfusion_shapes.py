"""GPU: the tensor-fusion tail over the shapes the C ABI admits (tests/abi_shapes.py XFUSION), not only the shipped
dim = 256, mmhid1 = mmhid2 = 512, nhid = 256 -- the forward-only pass (ops.xfusion_infer_group) and the training pair
(ops._xfusion_group_fwd_raw / _bwd_raw) against torch fp64 autograd of oracle.torch_port.xfusion + classifier[0], patient
by patient with that patient's masks (tests/xfusion_cases.py), in train (p = 0.25) and eval mode, overwritten and
accumulated, at the bars the suite holds for the shipped shape: MM, hid 1e-4; dv and every weight gradient
1e-5 + 1e-4 max|ref|; accumulate rtol 1e-6, atol 1e-7.  No ReLU unit is excused: every pre-activation of the fp64 oracle
is farther than KINK from zero under the seed the case records (tests/test_abi_shapes_cpu.py checks that without a GPU).

The classes the table covers: dim 4 / below one wave_dot round / 256 / 260; mmhid1 below one dW row block, ragged row
blocks with m = 2 and 3, 512, 516 (a second dkr pass of 4 rows, m = 3), 1528 (three passes, m = 2), % 4 != 0
(forward-only); K2 one chunk / % 64 != 0 / 1536; mmhid2 1 / % 4 != 0 / 1536; nhid 1 / % 4 != 0 under a wider lddhid / 1536 /
1537 (forward-only) / larger than mmhid2 and than K2 (classifier[0] sizes dpre, tmpb, tmpW); G 1 / 3 / 17 / 64.

Every call runs inside Guard.patch (tests/test_gpu_abi_shapes.py): MM, hid, dx2, the workspace and fresh gradient tensors
are views inside canary-filled buffers, x2 and held gradient buffers come from Guard.alloc; after each call the bands are
intact and every output and gradient word has been written.  Bit-level: eval-mode MM and hid of the training forward
equal the forward-only pass; a patient's MM, hid and dv rows equal a G = 1 call on that patient alone.  Refused shapes
return MMF_ERR_SHAPE through ctypes and write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_shapes as ab
import xfusion_cases as xc
from test_gpu_abi_shapes import Guard, _id, _lib, _p, _stream
from test_gpu_path import DEV, _t

pytestmark = pytest.mark.gpu

TRAIN = ab.accepted(ab.XFUSION, ab.xfusion_train_rule)
INFER = ab.accepted(ab.XFUSION, ab.xfusion_infer_rule)
HELD = 0.5                                   # what the held gradient buffers hold before an accumulating call


def _alone(G):
    """Patients compared with a G = 1 call: the first, the last, and the last one of the first XB_PG group (G = 17: 15 and
    16 stand on either side of the edge) or, in a smaller window, the middle one."""
    return sorted({0, G - 1, ab.XB_PG - 1 if G > ab.XB_PG else G // 2}) if G > 1 else []


def _weights(c):
    w, Wc0, bc0 = xc.weight_list(xc.inputs(c)[0], c.m)
    return [_t(a) for a in w], _t(Wc0), _t(bc0)


def _infer(c, g, monkeypatch, rows=None):
    from multimodalfusion_amd import ops
    _, vs, _, _ = xc.inputs(c)
    rows = slice(None) if rows is None else rows
    w, Wc0, bc0 = _weights(c)
    with g.patch(monkeypatch):
        MM, hid = ops.xfusion_infer_group([_t(v[rows]) for v in vs], w, Wc0, bc0)
    g.check()
    g.written(MM, "MM")
    g.written(hid, "hid")
    return MM, hid


def _pair(c, train, g, monkeypatch, rows=None, grads=None, accumulate=False):
    """One forward + backward of the training pair on the case's inputs (rows: that slice of the patients alone).
    Returns (MM, hid, [dv_i], gradients)."""
    from multimodalfusion_amd import ops
    _, vs, dhid, seeds = xc.inputs(c)
    rows = slice(None) if rows is None else rows
    vs, dhid, seeds = [v[rows] for v in vs], dhid[rows], seeds[rows]
    G = len(seeds)
    w, Wc0, bc0 = _weights(c)
    x2 = g.alloc((G, c.K2), name="x2")
    cols = [x2[:, c.mmhid1 + i * c.dim: c.mmhid1 + (i + 1) * c.dim] for i in range(c.m)]
    for col, v in zip(cols, vs):
        col.copy_(_t(v))
    put = [col.clone() for col in cols]
    wide = torch.full((G, c.lddhid), float("nan"), device=DEV)           # dhid as columns of a wider matrix
    off = c.lddhid_pad // 2
    wide[:, off:off + c.nhid] = _t(dhid)
    p = xc.P_FUS if train else 0.0
    with g.patch(monkeypatch):
        MM, hid, state = ops._xfusion_group_fwd_raw(x2, c.m, w, Wc0, bc0, p, p, seeds)
    g.check()
    g.written(MM, "MM")
    g.written(hid, "hid")
    g.written(x2[:, :c.mmhid1], "the e1 columns of x2")
    for i, (col, was) in enumerate(zip(cols, put)):
        assert torch.equal(col, was), f"the forward changed v_{i} in x2"
    with g.patch(monkeypatch):
        dvs, gw = ops._xfusion_group_bwd_raw(wide[:, off:off + c.nhid], state, grads=grads, accumulate=accumulate)
    g.check()
    for i, dv in enumerate(dvs):
        g.written(dv, f"dv{i}")
    for k, t in zip(xc._raw_names(c.m), gw):
        g.written(t, "d " + k)
    for i, (col, was) in enumerate(zip(cols, put)):
        assert torch.equal(col, was), f"the backward changed v_{i} in x2"
    return MM, hid, dvs, gw


def _report(c, mode, rows):
    print(f"XF-ERR | {c.why.split(':')[0][:48]} | m={c.m} dim={c.dim} mmhid1={c.mmhid1} mmhid2={c.mmhid2} nhid={c.nhid} G={c.G} | "
          f"{mode} | " + " | ".join(f"{k} {v:.2e}" for k, v in rows))


@pytest.mark.parametrize("c", INFER, ids=_id)
def test_forward_only_pass(c, monkeypatch):
    rMM, rhid, _, _, margin = xc.oracle(c, False)
    assert margin > xc.KINK, margin
    g = Guard()
    MM, hid = _infer(c, g, monkeypatch)
    e_MM, e_hid = float(np.abs(MM.cpu().numpy() - rMM).max()), float(np.abs(hid.cpu().numpy() - rhid).max())
    _report(c, "forward-only", [("MM", e_MM), ("hid", e_hid)])
    assert tuple(MM.shape) == (c.G, c.mmhid2) and tuple(hid.shape) == (c.G, c.nhid)
    np.testing.assert_allclose(MM.cpu().numpy(), rMM, rtol=0, atol=1e-4)
    np.testing.assert_allclose(hid.cpu().numpy(), rhid, rtol=0, atol=1e-4)
    for r in _alone(c.G):
        MM1, hid1 = _infer(c, g, monkeypatch, rows=slice(r, r + 1))
        assert torch.equal(MM1[0], MM[r]) and torch.equal(hid1[0], hid[r]), f"patient {r} alone"


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("c", TRAIN, ids=_id)
def test_training_pair(c, train, monkeypatch):
    rMM, rhid, rdv, rgw, margin = xc.oracle(c, train)
    assert margin > xc.KINK, margin
    names = xc._raw_names(c.m)
    g = Guard()
    MM, hid, dvs, gw = _pair(c, train, g, monkeypatch)
    checks = [(f"dv{i}", dvs[i].cpu().numpy(), rdv[i]) for i in range(c.m)]
    checks += [(k, t.cpu().numpy(), rgw[k]) for k, t in zip(names, gw)]
    errs = [(k, float(np.abs(got - ref).max()), 1e-5 + 1e-4 * float(np.abs(ref).max())) for k, got, ref in checks]
    e_MM, e_hid = float(np.abs(MM.cpu().numpy() - rMM).max()), float(np.abs(hid.cpu().numpy() - rhid).max())
    worst = max(errs, key=lambda e: e[1] / e[2])
    _report(c, "train" if train else "eval", [("MM", e_MM), ("hid", e_hid), ("dv", max(e[1] for e in errs[:c.m])),
                                               ("dv bar", min(e[2] for e in errs[:c.m])),
                                               (f"worst gradient {worst[0]}", worst[1]), ("its bar", worst[2])])
    np.testing.assert_allclose(MM.cpu().numpy(), rMM, rtol=0, atol=1e-4)
    np.testing.assert_allclose(hid.cpu().numpy(), rhid, rtol=0, atol=1e-4)
    for k, err, bar in errs:
        assert err <= bar, (k, err, bar)
    # accumulate: added to what the buffers hold (one fp32 rounding of the sum)
    held = [g.alloc(t.shape, name="held d " + k).fill_(HELD) for k, t in zip(names, gw)]
    _, _, dvs2, gw2 = _pair(c, train, g, monkeypatch, grads=held, accumulate=True)
    for k, a, b, h in zip(names, gw2, gw, held):
        assert a is h and a is not b
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy() + np.float32(HELD), rtol=1e-6, atol=1e-7, err_msg=k)
    for a, b in zip(dvs2, dvs):
        assert torch.equal(a, b)
    # overwrite: whatever the buffers held is gone
    junk = [g.alloc(t.shape, name="junk d " + k).fill_(float("nan")) for k, t in zip(names, gw)]
    _, _, _, gw3 = _pair(c, train, g, monkeypatch, grads=junk, accumulate=False)
    for k, a, b in zip(names, gw3, gw):
        assert torch.equal(a, b), k
    if not train:                            # eval mode: the forward-only pass, bit for bit
        MM0, hid0 = _infer(c, g, monkeypatch)
        assert torch.equal(MM, MM0) and torch.equal(hid, hid0)
    for r in _alone(c.G):                    # a patient's rows do not depend on the window
        MM1, hid1, dv1, _ = _pair(c, train, g, monkeypatch, rows=slice(r, r + 1))
        assert torch.equal(MM1[0], MM[r]) and torch.equal(hid1[0], hid[r]), f"patient {r} alone"
        for i, (a, b) in enumerate(zip(dv1, dvs)):
            assert torch.equal(a[0], b[r]), f"dv{i} of patient {r} alone"


# ---- refused shapes: the code, through ctypes, and nothing written ---------------------------------------------------------
def _refused_call(c, g, which=("infer", "forward", "backward")):
    """The three entry points on real buffers at least as large as the shape asks for (dimensions the rules refuse are
    rounded into range for the allocations only).  Returns (codes, every buffer a call could write)."""
    from multimodalfusion_amd import _lib as m_
    from multimodalfusion_amd import ops
    l = _lib()
    ms, G, dim = min(max(c.m, 2), 3), min(max(c.G, 1), ab.GROUP_MAX + 1), (c.dim + 3) // 4 * 4
    E, K2 = 17 ** ms, c.mmhid1 + 4 * dim
    z = lambda *shape: torch.zeros(shape, device=DEV)
    shapes = [s for _ in range(ms) for s in ((16, dim), (16,), (16, 4 * dim), (16,), (16, 16), (16,))]
    shapes += [(c.mmhid1, E), (c.mmhid1,), (c.mmhid2, K2), (c.mmhid2,), (c.nhid, c.mmhid2), (c.nhid,)]
    w = [z(*s) for s in shapes]
    gr = [g.alloc(s, name=f"gradient {i}") for i, s in enumerate(shapes)]

    def fill(struct, ts, prefix):
        for i in range(ms):
            for name, t in zip(("Wh", "bh", "Wz", "bz", "Wo", "bo"), ts[6 * i:6 * i + 6]):
                getattr(struct, prefix + name)[i] = t.data_ptr()
        for name, t in zip(("We1", "be1", "We2", "be2", "Wc0", "bc0"), ts[6 * ms:]):
            setattr(struct, prefix + name, t.data_ptr())
        return struct

    xw = fill(m_.XFusionWeights(m=c.m, dim=c.dim, sdim=c.sdim, mmhid1=c.mmhid1, mmhid2=c.mmhid2, nhid=c.nhid), w, "")
    xg = fill(m_.XFusionGrads(), gr, "d")
    vs = [z(G, dim) for _ in range(3)]
    vp = (C.c_void_p * 3)(*[v.data_ptr() for v in vs])
    x2, dx2 = g.alloc((G, K2), name="x2"), g.alloc((G, K2), name="dx2")
    MM, hid = g.alloc((G, c.mmhid2), name="MM"), g.alloc((G, c.nhid), name="hid")
    dhid = z(G, max(c.lddhid, c.nhid))
    nbytes = 1 << 24
    ws = g.alloc(nbytes, torch.uint8, name="workspace")
    base = ops.dropout_row_base(list(range(1, G + 1)), DEV)
    calls = dict(
        infer=lambda: l.mmf_xfusion_infer_group(C.byref(xw), vp, c.G, _p(ws), nbytes, _p(MM), _p(hid), _stream()),
        forward=lambda: l.mmf_xfusion_group_forward(C.byref(xw), _p(x2), c.G, C.c_float(0.25), C.c_float(0.25), _p(base), None,
                                                    _p(ws), nbytes, _p(MM), _p(hid), _stream()),
        backward=lambda: l.mmf_xfusion_group_backward(C.byref(xw), _p(x2), c.G, C.c_float(0.25), C.c_float(0.25), _p(base), None,
                                                      _p(MM), _p(hid), _p(dhid), c.lddhid, _p(ws), nbytes, _p(dx2), C.byref(xg),
                                                      0, _stream()))
    codes = {k: calls[k]() for k in which}
    torch.cuda.synchronize()
    return codes, [("MM", MM), ("hid", hid), ("x2", x2), ("dx2", dx2), ("workspace", ws)] + [(f"gradient {i}", t) for i, t in enumerate(gr)]


@pytest.mark.parametrize("c", ab.refused(ab.XFUSION, ab.xfusion_infer_rule), ids=_id)
def test_shapes_both_refuse_write_nothing(c):
    g = Guard()
    codes, bufs = _refused_call(c, g)
    assert codes == dict(infer=ab.ERR_SHAPE, forward=ab.ERR_SHAPE, backward=ab.ERR_SHAPE), codes
    for name, t in bufs:
        g.untouched(t, name)
    g.check()


@pytest.mark.parametrize("c", [c for c in INFER if c not in TRAIN], ids=_id)
def test_shapes_the_training_pair_refuses_write_nothing(c):
    """mmhid1 % 4, nhid = 1537, lddhid < nhid: the forward-only pass admits the widths (test_forward_only_pass runs them);
    the training forward refuses the first two and the backward all three, through ctypes with every pointer valid --
    through ops the calls carry the empty workspace the refusing query sized, and MMF_ERR_ARG for it comes first."""
    which = ("forward", "backward") if c.lddhid >= c.nhid else ("backward",)     # the forward has no dhid
    g = Guard()
    codes, bufs = _refused_call(c, g, which)
    assert codes == {k: ab.ERR_SHAPE for k in which}, codes
    for name, t in bufs:
        g.untouched(t, name)
    g.check()
