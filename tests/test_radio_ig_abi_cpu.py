"""CPU checks of the radiology head's integrated-gradients entry points in the C ABI (include/mmf_amil.h:
mmf_radio_ig_workspace_bytes, mmf_radio_ig): both symbols are bound with the header's arity, the ABI version is unchanged
(the entry points are additive), every refusal comes back in the header's order before any HIP call -- the fake pointers are
never read -- and the workspace query is 0 exactly where the header says, non-zero for every case of tests/radio_ig_cases.py
and does not shrink as window_steps grows.  Needs the built library, not a GPU."""
import ctypes as C
import re

import pytest

import radio_ig_cases as rc
from test_abi_layout_cpu import HEADER
from test_ig_abi_cpu import ALIGN, ARG, FAKE, SHAPE, WORKSPACE, _desc as _ig_desc, _head, _ig

NEW = ["mmf_radio_ig_workspace_bytes", "mmf_radio_ig"]


def test_new_symbols_are_bound_with_the_headers_arity_and_the_abi_version_is_unchanged():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    assert _lib.ABI_VERSION == 12 and l.mmf_abi_version() == 12
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(l, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
    rt, args = _lib.SYMBOLS["mmf_radio_ig_workspace_bytes"]
    assert rt is C.c_size_t and args == [C.c_int64] + [C.c_int32] * 7
    rt, args = _lib.SYMBOLS["mmf_radio_ig"]
    assert rt is C.c_int and args == [C.POINTER(_lib.AmilDesc), C.POINTER(_lib.RadioReduce), C.c_void_p, C.c_size_t,
                                      C.POINTER(_lib.SurvHead), C.POINTER(_lib.IgDesc), C.c_void_p]


def _desc(**kw):
    return _ig_desc(**kw)           # N 300, L 1024, the small gated head


def _rd(keep, nseg=4, kseg=1024, x=None, null_x=False, W=FAKE, bias=FAKE):
    from multimodalfusion_amd import _lib
    segs = (C.c_void_p * 4)(*([FAKE] * 4 if x is None else x))
    keep.append(segs)
    return _lib.RadioReduce(x=None if null_x else segs, nseg=nseg, kseg=kseg, W=W, bias=bias, dW=None, db=None)


def _call(desc=None, rd=None, ig=None, head=None, ws=FAKE, nbytes=1 << 40):
    from multimodalfusion_amd import _lib
    keep = []
    desc = _desc() if desc is None else desc
    rd = _rd(keep) if rd is None else rd
    ig = _ig(keep=keep) if ig is None else ig
    head = _head() if head is None else head
    return _lib.lib().mmf_radio_ig(C.byref(desc), C.byref(rd), ws, nbytes, C.byref(head), C.byref(ig), None)


def test_refusals_that_need_no_device():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    keep = []
    assert _call(nbytes=16) == WORKSPACE                            # everything else in order
    # what mmf_amil_ig refuses with MMF_ERR_ARG
    rd = _rd(keep)
    assert l.mmf_radio_ig(None, C.byref(rd), FAKE, 1 << 40, C.byref(_head()), C.byref(_ig(keep=keep)), None) == ARG
    assert l.mmf_radio_ig(C.byref(_desc()), C.byref(rd), FAKE, 1 << 40, None, C.byref(_ig(keep=keep)), None) == ARG
    assert l.mmf_radio_ig(C.byref(_desc()), C.byref(rd), FAKE, 1 << 40, C.byref(_head()), None, None) == ARG
    assert _call(desc=_desc(p_h=0.25)) == ARG and _call(desc=_desc(p_att=0.25)) == ARG and _call(desc=_desc(gemm=1)) == ARG
    for n in (0, -1, 65):
        assert _call(ig=_ig(n, keep=keep)) == ARG, n
    assert _call(ig=_ig(keep=keep, alpha=None)) == ARG and _call(ig=_ig(keep=keep, weight=None)) == ARG
    assert _call(ig=_ig(keep=keep, window_steps=-1)) == ARG
    for name in ("row_sum", "row_abs", "risk_x", "risk_base", "step_risk"):
        assert _call(ig=_ig(keep=keep, **{name: None})) == ARG, name
    assert _call(head=_head(Wk=None)) == ARG and _call(head=_head(bk=None)) == ARG
    # reduce_dim's pointers
    assert l.mmf_radio_ig(C.byref(_desc()), None, FAKE, 1 << 40, C.byref(_head()), C.byref(_ig(keep=keep)), None) == ARG
    assert _call(rd=_rd(keep, null_x=True)) == ARG
    for m in range(4):
        x = [FAKE] * 4
        x[m] = None
        assert _call(rd=_rd(keep, x=x)) == ARG, m
    assert _call(rd=_rd(keep, nseg=3, x=[FAKE, FAKE, FAKE, None]), desc=_desc(N=300), nbytes=16) == WORKSPACE
    assert _call(rd=_rd(keep, W=None)) == ARG and _call(rd=_rd(keep, bias=None)) == ARG
    # MMF_ERR_ARG comes before every MMF_ERR_SHAPE: a bad shape next to a null pointer
    assert _call(rd=_rd(keep, kseg=512, W=None)) == ARG and _call(desc=_desc(H=128), rd=_rd(keep, bias=None)) == ARG
    assert _call(head=_head(K=33, Wk=None)) == ARG
    # MMF_ERR_SHAPE, in the header's order
    for nseg in (0, 1, 5, -2):
        assert _call(rd=_rd(keep, nseg=nseg)) == SHAPE, nseg
    for nseg in (2, 3, 4):
        assert _call(rd=_rd(keep, nseg=nseg), nbytes=16) == WORKSPACE, nseg
    assert _call(desc=_desc(N=0)) == SHAPE and _call(desc=_desc(L=1000)) == SHAPE
    assert _call(desc=_desc(H=128)) == SHAPE and _call(desc=_desc(D=100)) == SHAPE
    assert _call(desc=_desc(W1=None)) == ARG and _call(desc=_desc(Wb=None)) == ARG       # check_desc's own
    assert _call(desc=_desc(Wb=None, bb=None, gated=0), nbytes=16) == WORKSPACE
    assert _call(rd=_rd(keep, kseg=512)) == SHAPE and _call(desc=_desc(L=512), rd=_rd(keep, kseg=512), nbytes=16) == WORKSPACE
    # N nseg kseg 4 >= 2^31: 131072 rows of four 1024-wide modalities, while three fit
    assert _call(desc=_desc(N=131072)) == SHAPE and _call(desc=_desc(N=131071), nbytes=16) == WORKSPACE
    assert _call(desc=_desc(N=131072), rd=_rd(keep, nseg=3), nbytes=16) == WORKSPACE
    assert _call(head=_head(K=0)) == SHAPE and _call(head=_head(K=33)) == SHAPE
    assert _call(head=_head(K=32), nbytes=16) == WORKSPACE
    # a shape refusal comes before an alignment refusal
    assert _call(rd=_rd(keep, kseg=512, W=FAKE + 4)) == SHAPE and _call(head=_head(K=33), rd=_rd(keep, W=FAKE + 4)) == SHAPE
    # MMF_ERR_ALIGN
    for m in range(4):
        x = [FAKE] * 4
        x[m] = FAKE + 4
        assert _call(rd=_rd(keep, x=x)) == ALIGN, m
    assert _call(rd=_rd(keep, W=FAKE + 4)) == ALIGN and _call(rd=_rd(keep, bias=FAKE + 4), nbytes=16) == WORKSPACE
    assert _call(ig=_ig(keep=keep, attr=FAKE + 4)) == ALIGN and _call(ig=_ig(keep=keep, attr=FAKE), nbytes=16) == WORKSPACE
    assert _call(ws=FAKE + 8) == ALIGN and _call(desc=_desc(W1=FAKE + 4)) == ALIGN and _call(ws=None) == ARG
    # an alignment refusal comes before the workspace's
    assert _call(rd=_rd(keep, W=FAKE + 4), nbytes=16) == ALIGN
    need = l.mmf_radio_ig_workspace_bytes(300, 4, 1024, 256, 256, 1, 20, 0)
    assert need > 0 and _call(nbytes=need - 1) == WORKSPACE


def test_workspace_query_is_zero_exactly_where_the_header_says():
    from multimodalfusion_amd import _lib
    q = _lib.lib().mmf_radio_ig_workspace_bytes
    ok = dict(N=300, nseg=4, kseg=1024, H=256, D=256, gated=1, n_steps=20, window_steps=0)
    call = lambda **kw: q(*{**ok, **kw}.values())
    assert call() > 0
    for kw in (dict(n_steps=0), dict(n_steps=65), dict(window_steps=-1), dict(N=0), dict(N=-5), dict(nseg=1), dict(nseg=5),
               dict(kseg=31), dict(kseg=0), dict(H=31), dict(N=1 << 22, kseg=32, nseg=2),      # above the window's row limit
               dict(N=131072), dict(N=1 << 20, kseg=256, nseg=2)):                              # the 2 GiB input rule
        assert call(**kw) == 0, kw
    for kw in (dict(n_steps=1), dict(n_steps=64), dict(window_steps=64), dict(N=1), dict(nseg=2), dict(nseg=3), dict(kseg=32),
               dict(H=32), dict(N=131071), dict(N=131072, nseg=3), dict(gated=0), dict(N=(1 << 20) - 1, kseg=256, nseg=2)):
        assert call(**kw) > 0, kw
    # the window's row limit is mmf_amil_ig_workspace_bytes': the two queries turn 0 at the same N
    qa = _lib.lib().mmf_amil_ig_workspace_bytes
    for H, D in ((256, 256), (512, 640), (1024, 128)):
        lo, hi = 1, 1 << 23
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if qa(mid, 32, H, D, 1, 20, 0) else (lo, mid)
        assert q(lo, 2, 32, H, D, 1, 20, 0) > 0 and q(hi, 2, 32, H, D, 1, 20, 0) == 0, (H, D, lo)


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_workspace_of_every_case(name):
    from multimodalfusion_amd import _lib
    c = rc.BY_NAME[name]
    q = _lib.lib().mmf_radio_ig_workspace_bytes
    b = q(c.N, c.nseg, c.kseg, c.H, c.D, 1 if c.gated else 0, c.n_steps, c.window_steps)
    # at least Y, U, the folded gradient, and one step's h, a and du
    assert b >= 4 * c.N * (c.kseg + 4 * c.H + c.D)
    prev = 0
    for ws in range(1, c.n_steps + 3):                              # does not decrease in window_steps, up to the clamp
        cur = q(c.N, c.nseg, c.kseg, c.H, c.D, 1 if c.gated else 0, c.n_steps, ws)
        assert cur >= prev and cur > 0, ws
        prev = cur
    assert q(c.N, c.nseg, c.kseg, c.H, c.D, 1 if c.gated else 0, c.n_steps, 64) >= prev
    assert 0 < q(c.N, c.nseg, c.kseg, c.H, c.D, 1 if c.gated else 0, c.n_steps, 0) <= q(c.N, c.nseg, c.kseg, c.H, c.D,
                                                                                          1 if c.gated else 0, c.n_steps, 64)


def test_linear_input_grad_refusals():
    """mmf_linear_input_grad (the concatenated linear's input gradient, which the autograd yardstick needs): bound with the
    header's arity, every refusal before any launch."""
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bmmf_linear_input_grad\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SYMBOLS["mmf_linear_input_grad"][1])
    segs = lambda *v: (C.c_void_p * 4)(*v)
    ok = segs(FAKE, FAKE, FAKE, FAKE)
    f = l.mmf_linear_input_grad
    assert f(None, FAKE, 4, 1024, 8, 1024, ok, None) == ARG and f(FAKE, None, 4, 1024, 8, 1024, ok, None) == ARG
    assert f(FAKE, FAKE, 4, 1024, 8, 1024, None, None) == ARG
    assert f(FAKE, FAKE, 0, 1024, 8, 1024, ok, None) == ARG and f(FAKE, FAKE, 5, 1024, 8, 1024, ok, None) == ARG
    assert f(FAKE, FAKE, 4, 1024, 8, 1024, segs(FAKE, FAKE, None, FAKE), None) == ARG
    assert f(FAKE, FAKE, 2, 1022, 8, 1024, segs(FAKE, FAKE, None, None), None) == SHAPE     # segments past nseg are not read
    assert f(FAKE, FAKE, 4, 1024, 0, 1024, ok, None) == SHAPE and f(FAKE, FAKE, 4, 1024, 8, 1000, ok, None) == SHAPE
    assert f(FAKE, FAKE, 4, 1022, 8, 1024, ok, None) == SHAPE and f(FAKE, FAKE, 4, 1024, 1 << 19, 1024, ok, None) == SHAPE
    assert f(FAKE + 4, FAKE, 4, 1024, 8, 1024, ok, None) == ALIGN and f(FAKE, FAKE + 4, 4, 1024, 8, 1024, ok, None) == ALIGN
    assert f(FAKE, FAKE, 4, 1024, 8, 1024, segs(FAKE, FAKE + 8, FAKE, FAKE), None) == ALIGN


def test_python_surface_refuses_before_the_library_is_called():
    import torch
    from multimodalfusion_amd import _lib, ops
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio
    mods = ["T1", "T2"]
    model = MIL_Attention_fc_surv_radio(gate_radio=True, dropout=False, n_classes=4, modalities=mods)
    bags = {m: torch.zeros(4, 1024) for m in mods}
    model.train()
    with pytest.raises(RuntimeError):
        model.integrated_gradients(**bags)
    model.eval()
    with pytest.raises(NotImplementedError):
        model.integrated_gradients(**{m: x.to(torch.bfloat16) for m, x in bags.items()})
    with pytest.raises(NotImplementedError):
        ops.radio_integrated_gradients([x.to(torch.bfloat16) for x in bags.values()], None, None, (None,) * 8, None, None, True,
                                       [0.5], [1.0])
    with pytest.raises(_lib.MmfError):
        model.integrated_gradients(T1=bags["T1"], T2=torch.zeros(5, 1024))
    h = model.reduce_dim.register_forward_hook(lambda *a: None)
    try:
        with pytest.raises(NotImplementedError):
            model.integrated_gradients(**bags)
    finally:
        h.remove()
    wide = MIL_Attention_fc_surv_radio(gate_radio=True, dropout=False, n_classes=33, modalities=mods).eval()
    with pytest.raises(NotImplementedError):
        wide.integrated_gradients(**bags)
