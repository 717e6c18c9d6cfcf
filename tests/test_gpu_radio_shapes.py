"""GPU: the radiology window (mmf_radio_nll_step_group, mmf_radio_infer_group) and the grouped half chains
(mmf_amil_group_forward / _backward, mmf_radio_group_forward / _backward) over the RADIO and HALF tables of
tests/abi_shapes.py -- reduce_dim widths of one, three, four and five chunks under the H = 256 / 512 / 1024 stacks, two to
four modalities, windows of one bag, (1, 65, 300) and 64 bags, a feature matrix wider than the stack -- against the float64
references of tests/radio_cases.py at the project's own bars: compare() of tests/test_gpu_path.py for the outputs, 1e-5 +
1e-4 max|ref| for every gradient (no case has a unit on the ReLU kink: tests/test_radio_shapes_cpu.py).

Every output, gradient buffer and workspace is a Guard view (tests/test_gpu_abi_shapes.py): fully written over NaN
canaries, the bands around it intact; the buffers the test hands in carry a canary of their own (OwnGuard), so that an
unwritten workspace word summed into a store past a gradient's end cannot pass for an intact band.  Every accepted case
runs twice, to identical bits.  Refused cases are those the CPU
file has shown to return before the workspace check; here they get device pointers and must leave every buffer untouched.
The dW_r problems run as a TN launch of their own, the only route there is."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_shapes as ab
import radio_cases as rc
from test_gpu_abi_shapes import CANARY, Guard
from test_gpu_path import DEV, compare

pytestmark = pytest.mark.gpu

RADIO_OK, RADIO_NO = ab.accepted(ab.RADIO, ab.radio_rule), ab.refused(ab.RADIO, ab.radio_rule)
HALF_OK, HALF_NO = ab.accepted(ab.HALF, ab.half_rule), ab.refused(ab.HALF, ab.half_rule)
_id = lambda c: c.why


OWN = 0x7FD1B2B2             # a second quiet NaN: the canary of the buffers the test itself hands in


class OwnGuard(Guard):
    """Guard with a canary of its own, for the gradient buffers and feature matrices the test hands in.  The workspace and
    the outputs ops.py allocates carry Guard's canary (Guard.patch); a kernel that sums unwritten workspace words into a
    store past the end of a gradient hands that NaN's payload on, and under one shared canary the band would still look
    intact (the db-length mutation of DESIGN.md 7q did exactly that)."""
    canary = OWN

    def alloc(self, shape, dtype=torch.float32, skew=0, name="buffer"):
        t = super().alloc(shape, dtype, skew, name)
        self.bufs[-1][0].fill_(OWN)
        return t

    def written(self, t, name, owned=True):
        assert not owned or self.owns(t), f"{name} is not in a guarded buffer"
        left = int((self.words(t) == OWN).sum())
        assert left == 0, f"{name}: {left} of {t.numel()} elements were never written"

    def check(self):
        torch.cuda.synchronize()
        for buf, lead, words, name in self.bufs:
            assert bool((buf[:lead] == OWN).all()), f"{name}: the band in FRONT of the buffer was written"
            assert bool((buf[lead + words:] == OWN).all()), f"{name}: the band BEHIND the buffer was written"


def _T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _world(c):
    """(xs, Wr, br, stack, Wk, bk) of a case on the device."""
    sd = rc.state(c)
    stack = tuple(None if n is None else _T(sd[n]) for n in rc.stack_names(c))
    Wr, br = (_T(sd["reduce_dim.weight"]), _T(sd["reduce_dim.bias"])) if c.nseg else (None, None)
    return [_T(x) for x in rc.window(c)], Wr, br, stack, _T(sd["classifier.weight"]), _T(sd["classifier.bias"])


def _grad_buffers(c, g, names, params, accumulate):
    out = []
    for n, p in zip(names, params):
        if p is None:
            out.append(None)
            continue
        t = g.alloc(p.shape, name="d " + n)
        if accumulate:
            t.copy_(torch.as_tensor(rc.before(c, n, tuple(p.shape))))
        out.append(t)
    return out


def _labels(c):
    metas = rc.bag_metas(c)
    return [m["y"] for m in metas], [float(m["c"]) for m in metas], [m["mask_seed"] for m in metas]


def _check_grads(c, tag, names, got, ref, accumulate):
    """Every gradient within 1e-5 + 1e-4 max|ref| of the float64 sum; an accumulate case holds `before + sum`."""
    worst = 0.0
    for n, t in zip(names, got):
        if n is None:
            continue
        v = t.detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(v).all(), (tag, n)
        if accumulate:
            v = v - rc.before(c, n, v.shape)
        r = ref[n].reshape(v.shape)
        err, bar = float(np.abs(v - r).max()), rc.grad_bar(r)
        worst = max(worst, err / bar)
        assert err <= bar, f"{tag} grad {n}: max abs err {err:.3e} > {bar:.3e}"
    print(f"FIGURE {tag}: worst gradient error / bar = {worst:.3f}")


def _step(c, world, monkeypatch, accumulate=None):
    from multimodalfusion_amd import ops
    xs, Wr, br, stack, Wk, bk = world
    accumulate = c.accumulate if accumulate is None else accumulate
    g, own = Guard(), OwnGuard()
    grads = _grad_buffers(c, own, rc.grad_names(c), [Wr, br, *stack, Wk, bk], accumulate)
    Y, cen, seeds = _labels(c)
    p = rc.P_DROP if c.train else 0.0
    with g.patch(monkeypatch):
        out = ops.radio_nll_step_group(xs, c.sizes, Wr, br, stack, Wk, bk, c.gated, Y, cen, rc.ALPHA, grads,
                                       loss_scale=rc.loss_scale(c), accumulate=bool(accumulate), p_h=p, p_att=p, seeds=seeds)
    g.check()
    own.check()
    hz, S, Yh, A, loss, risk = out
    for name, t in (("hazards", hz), ("S", S), ("Y_hat", Yh), ("loss", loss), ("risk", risk)) + tuple((f"A_raw[{i}]", a) for i, a in enumerate(A)):
        g.written(t, name)
    for n, t in zip(rc.grad_names(c), grads):
        if t is not None:
            own.written(t, "d " + n)
    return out, grads


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_outputs(tag, refs, hz, S, Yh, A, loss, risk, M=None, worst=None):
    for i, ref in enumerate(refs):
        one = dict(hazards=hz[i:i + 1].cpu().numpy(), S=S[i:i + 1].cpu().numpy(), A_raw=A[i].cpu().numpy(), loss=float(loss[i]),
                   M=None if M is None else M[i:i + 1].cpu().numpy(), grads={})
        compare(one, dict(ref, grads={}), f"{tag} bag {i}")
        assert np.array_equal(Yh[i].cpu().numpy().reshape(-1), np.asarray(ref["Y_hat"]).reshape(-1)), (tag, i)
        assert abs(float(risk[i]) + float(S[i].sum())) < 1e-5, (tag, i)
    e = max(float(np.abs(A[i].cpu().numpy() - r["A_raw"]).max()) for i, r in enumerate(refs)) / 1e-4
    l = max(abs(float(loss[i]) - float(r["loss"])) for i, r in enumerate(refs)) / 1e-5
    print(f"FIGURE {tag}: worst score error / bar = {e:.3f}, worst loss error / bar = {l:.3f}")


# =======================================================================================================================
# the two full chains
# =======================================================================================================================
@pytest.mark.parametrize("c", RADIO_OK, ids=_id)
def test_radio_window(c, monkeypatch):
    from multimodalfusion_amd import ops
    world = _world(c)
    xs, Wr, br, stack, Wk, bk = world
    refs, gsum = rc.full_reference(c)
    tag = f"radio nseg={c.nseg} {c.size}"
    out, grads = _step(c, world, monkeypatch)
    hz, S, Yh, A, loss, risk = out
    _check_outputs(tag, refs, hz, S, Yh, A, loss, risk)
    assert set(n for n in rc.grad_names(c) if n) == set(gsum)
    _check_grads(c, tag, rc.grad_names(c), grads, gsum, c.accumulate)
    # a second run: identical bits
    out2, grads2 = _step(c, world, monkeypatch)
    for a, b in zip((out[0], out[1], out[2], out[4], out[5], *out[3]), (out2[0], out2[1], out2[2], out2[4], out2[5], *out2[3])):
        assert _bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)
    for n, a, b in zip(rc.grad_names(c), grads, grads2):
        assert a is None or _bits(a, b), n
    torch.cuda.synchronize()
    assert int(ops.sync_words(torch.device(DEV)).abs().sum()) == 0
    if c.train:
        return
    # eval: the forward-only pass and the radio forward half give the same bags to fp32 rounding
    Y, cen, seeds = _labels(c)
    g, own = Guard(), OwnGuard()
    Mh = own.alloc((len(c.sizes), c.H), name="M of the forward half")
    with g.patch(monkeypatch):
        hz2, S2, Yh2, risk2, A2, M2, loss2 = ops.radio_infer_group(xs, c.sizes, Wr, br, stack, c.gated, Wk, bk, Y, cen, rc.ALPHA,
                                                                    want_M=True)
        A3, _ = ops._group_half_fwd_raw(xs, c.sizes, stack, c.gated, 0.0, 0.0, seeds, Mh, Wr, br)
    g.check()
    own.check()
    own.written(Mh, "M of the forward half")
    for name, t in (("hazards", hz2), ("S", S2), ("Y_hat", Yh2), ("loss", loss2), ("risk", risk2), ("M", M2)):
        g.written(t, name)
    _check_outputs(tag + " infer", refs, hz2, S2, Yh2, A2, loss2, risk2, M=M2)
    bar = rc.OUT_BAR
    for name, a, b in (("hazards", hz2, hz), ("S", S2, S), ("loss", loss2, loss), ("risk", risk2, risk), ("M", Mh, M2)):
        assert float((a - b).abs().max()) <= bar, (name, float((a - b).abs().max()))
    assert torch.equal(Yh2, Yh)
    for i in range(len(c.sizes)):
        g.written(A2[i], f"A_raw[{i}] infer")
        g.written(A3[i], f"A_raw[{i}] half")
        assert float((A2[i] - A[i]).abs().max()) <= bar and float((A3[i] - A[i]).abs().max()) <= bar, i
    # and a second forward-only run: identical bits
    again = ops.radio_infer_group(xs, c.sizes, Wr, br, stack, c.gated, Wk, bk, Y, cen, rc.ALPHA, want_M=True)
    assert _bits(again[0], hz2) and _bits(again[5], M2) and _bits(again[6], loss2) and all(_bits(a, b) for a, b in zip(again[4], A2))


class _ShortQueries:
    """The library with both radio workspace queries (and the plain group query) answering one byte less."""
    NAMES = ("mmf_radio_group_workspace_bytes", "mmf_radio_group_infer_workspace_bytes", "mmf_amil_group_workspace_bytes")

    def __init__(self, l):
        self._l = l
        self.asked = []

    def __getattr__(self, name):
        f = getattr(self._l, name)
        if name not in self.NAMES:
            return f

        def short(*a):
            n = f(*a)
            self.asked.append((name, n))
            return n - 1
        return short


def _all_untouched(what, *guards):
    torch.cuda.synchronize()
    for g in guards:
        for buf, lead, words, name in g.bufs:
            assert bool((buf == getattr(g, "canary", CANARY)).all()), f"{name} was written by {what}"


@pytest.mark.parametrize("c", [RADIO_OK[0], RADIO_OK[2], RADIO_OK[3]], ids=_id)
def test_radio_workspace_one_byte_short(c, monkeypatch):
    """The call with exactly the queried size is test_radio_window (ops allocates just that, inside guard bands); with one
    byte fewer both entry points return MMF_ERR_WORKSPACE and write nothing -- not an output, not a gradient, not the
    workspace itself."""
    from multimodalfusion_amd import _lib, ops
    xs, Wr, br, stack, Wk, bk = _world(c)
    Y, cen, seeds = _labels(c)
    proxy = _ShortQueries(_lib.lib())
    monkeypatch.setattr(ops, "lib", lambda: proxy)
    g, own = Guard(), OwnGuard()
    grads = _grad_buffers(c, own, rc.grad_names(c), [Wr, br, *stack, Wk, bk], 0)
    with g.patch(monkeypatch):
        with pytest.raises(_lib.MmfError, match=r"code -4"):
            ops.radio_nll_step_group(xs, c.sizes, Wr, br, stack, Wk, bk, c.gated, Y, cen, rc.ALPHA, grads, p_h=0.25, p_att=0.25,
                                     seeds=seeds)
        with pytest.raises(_lib.MmfError, match=r"code -4"):
            ops.radio_infer_group(xs, c.sizes, Wr, br, stack, c.gated, Wk, bk, Y, cen, rc.ALPHA, want_M=True)
        with pytest.raises(_lib.MmfError, match=r"code -4"):
            ops._group_half_fwd_raw(xs, c.sizes, stack, c.gated, 0.25, 0.25, seeds, own.alloc((len(c.sizes), c.H)), Wr, br)
    assert [n for n, _ in proxy.asked] == ["mmf_radio_group_workspace_bytes", "mmf_radio_group_infer_workspace_bytes",
                                           "mmf_radio_group_workspace_bytes"] and all(b > 1 for _, b in proxy.asked)
    _all_untouched("a call whose workspace is one byte short", g, own)


# =======================================================================================================================
# refusals, on device pointers
# =======================================================================================================================
def _device_pointers(g):
    """Every pointer of rc.PTRS as a guarded 1 MiB buffer (more than any refused case's operand), the workspace 64 MiB."""
    p = {n: g.alloc(1 << 18, name=n).data_ptr() for n in rc.PTRS if n != "ws"}
    ws = g.alloc(1 << 24, name="ws")
    p["ws"] = ws.data_ptr()
    return p, ws.numel() * 4


@pytest.mark.parametrize("c", RADIO_NO, ids=_id)
def test_radio_refusals_write_nothing(c):
    from multimodalfusion_amd import _lib
    g = Guard()
    p, ws_bytes = _device_pointers(g)
    refused = [n for n in rc.RADIO_ENTRIES if ab.radio_rule(c, grads=rc.WRITES_GRADS[n]) != ab.OK]
    assert refused
    got = rc.entry_calls(_lib, _lib.lib(), c, p, ws_bytes=ws_bytes, entries=refused,
                         stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert got == {n: ab.radio_rule(c, grads=rc.WRITES_GRADS[n]) for n in refused}
    _all_untouched("a refused call", g)


@pytest.mark.parametrize("c", HALF_NO, ids=_id)
def test_half_refusals_write_nothing(c):
    import dataclasses
    from multimodalfusion_amd import _lib
    g = Guard()
    p, ws_bytes = _device_pointers(g)
    for cc in (c, dataclasses.replace(c, radio=2)):
        names = rc.RADIO_ENTRIES[2:] if cc.radio else rc.PLAIN_ENTRIES
        refused = [n for n in names if ab.half_rule(cc, bwd=n.endswith("backward")) != ab.OK]
        assert refused
        got = rc.entry_calls(_lib, _lib.lib(), cc, p, ws_bytes=ws_bytes, ldm=cc.ldm, entries=refused,
                             stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert got == {n: ab.half_rule(cc, bwd=n.endswith("backward")) for n in refused}
    _all_untouched("a refused call", g)


# =======================================================================================================================
# the half chains
# =======================================================================================================================
def _half_run(c, world, monkeypatch):
    """Forward through ops._group_half_fwd_raw into the stack's slot of a [G x ldm] matrix; backward from the same slot of
    a dM matrix whose other columns hold 1e3 -- through ops._group_half_bwd_raw, or (accumulate) the entry point itself
    on buffers that start from radio_cases.before."""
    from multimodalfusion_amd import _lib, ops
    xs, Wr, br, stack, _, _ = world
    G, H = len(c.sizes), c.H
    _, _, seeds = _labels(c)
    p = rc.P_DROP if c.train else 0.0
    g, own = Guard(), OwnGuard()
    wide = own.alloc((G, c.ldm), name="feature matrix")
    slot = wide[:, c.m_offset:c.m_offset + H]
    with g.patch(monkeypatch):
        A, state = ops._group_half_fwd_raw(xs, c.sizes, stack, c.gated, p, p, seeds, slot, Wr, br)
    g.check()
    own.check()
    words = Guard.words(wide).view(G, c.ldm)
    assert not bool((words[:, c.m_offset:c.m_offset + H] == OWN).any()), "M: elements of the slot were never written"
    outside = torch.ones(c.ldm, dtype=torch.bool, device=DEV)
    outside[c.m_offset:c.m_offset + H] = False
    assert bool((words[:, outside] == OWN).all()), "columns of the feature matrix outside the stack's slot were written"
    for i, a in enumerate(A):
        g.written(a, f"A_raw[{i}]")
    dwide = torch.full((G, c.ldm), 1e3, dtype=torch.float32, device=DEV)
    dwide[:, c.m_offset:c.m_offset + H] = _T(rc.half_dm(c))
    dslot = dwide[:, c.m_offset:c.m_offset + H]
    names = (["reduce_dim.weight", "reduce_dim.bias"] if c.radio else []) + rc.stack_names(c)
    g2 = Guard() if not c.accumulate else OwnGuard()
    if not c.accumulate:
        with g2.patch(monkeypatch):
            ds, rd = ops._group_half_bwd_raw(state, dslot)
        grads = list(rd or ()) + list(ds)
    else:
        params = ([Wr, br] if c.radio else []) + list(stack)
        grads = _grad_buffers(c, g2, names, params, 1)
        ws = state[5]
        ptrs = dict(zip(("W1", "b1", "Wa", "ba", "Wb", "bb", "Wc", "bc"), (None if t is None else t.data_ptr() for t in stack)))
        ptrs.update(zip(("dW1", "db1", "dWa", "dba", "dWb", "dbb", "dWc", "dbc"),
                        (None if t is None else t.data_ptr() for t in grads[-8:])))
        ptrs.update({f"x{i}": x.data_ptr() for i, x in enumerate(state[0])}, ws=ws.data_ptr(), A_raw=state[8].data_ptr(),
                    dM=dslot[0].data_ptr(), M=None)
        if c.radio:
            ptrs.update(W=Wr.data_ptr(), bias=br.data_ptr(), dW=grads[0].data_ptr(), db=grads[1].data_ptr())
        for n in rc.PTRS:
            ptrs.setdefault(n, None)
        name = "mmf_radio_group_backward" if c.radio else "mmf_amil_group_backward"
        kw = dict(ws_bytes=ws.numel(), ldm=c.ldm, train=c.train, accumulate=1, seeds=seeds, entries=(name,),
                  stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), sync=ops.sync_words(torch.device(DEV)).data_ptr())
        before = [None if t is None else t.clone() for t in grads]
        short = rc.entry_calls(_lib, _lib.lib(), c, ptrs, **dict(kw, ws_bytes=ws.numel() - 1))
        assert short == {name: ab.ERR_WORKSPACE}
        torch.cuda.synchronize()
        assert all(a is None or _bits(a, b) for a, b in zip(grads, before)), "a backward one byte short wrote a gradient"
        assert rc.entry_calls(_lib, _lib.lib(), c, ptrs, **kw) == {name: ab.OK}
    g2.check()
    for n, t in zip(names, grads):
        if n is not None:
            g2.written(t, "d " + n)
    return slot, A, names, grads


@pytest.mark.parametrize("c", HALF_OK, ids=_id)
def test_half_chain(c, monkeypatch):
    world = _world(c)
    Mref, Aref, gref = rc.half_reference(c)
    tag = f"half {'radio' if c.radio else 'plain'} {c.size} ldm={c.ldm}"
    M, A, names, grads = _half_run(c, world, monkeypatch)
    np.testing.assert_allclose(M.cpu().numpy(), Mref, rtol=0, atol=1e-4, err_msg=tag)
    for i, a in enumerate(A):
        np.testing.assert_allclose(a.cpu().numpy(), Aref[i], rtol=0, atol=1e-4, err_msg=f"{tag} bag {i}")
    print(f"FIGURE {tag}: worst M error / bar = {float(np.abs(M.cpu().numpy() - Mref).max()) / 1e-4:.3f}")
    assert set(n for n in names if n) == set(gref)
    _check_grads(c, tag, names, grads, gref, c.accumulate)
    M2, A2, _, grads2 = _half_run(c, world, monkeypatch)
    assert _bits(M, M2) and all(_bits(a, b) for a, b in zip(A, A2))
    for n, a, b in zip(names, grads, grads2):
        assert a is None or _bits(a, b), n


@pytest.mark.parametrize("c", [HALF_OK[0], HALF_OK[3]], ids=_id)
def test_plain_half_workspace_one_byte_short(c, monkeypatch):
    from multimodalfusion_amd import _lib, ops
    xs, Wr, br, stack, _, _ = _world(c)
    proxy = _ShortQueries(_lib.lib())
    monkeypatch.setattr(ops, "lib", lambda: proxy)
    g, own = Guard(), OwnGuard()
    wide = own.alloc((len(c.sizes), c.ldm))
    with g.patch(monkeypatch):
        with pytest.raises(_lib.MmfError, match=r"code -4"):
            ops._group_half_fwd_raw(xs, c.sizes, stack, c.gated, 0.0, 0.0, _labels(c)[2], wide[:, c.m_offset:c.m_offset + c.H])
    assert [n for n, _ in proxy.asked] == ["mmf_amil_group_workspace_bytes"]
    _all_untouched("a forward half whose workspace is one byte short", g, own)
