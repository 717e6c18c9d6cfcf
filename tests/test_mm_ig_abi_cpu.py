"""CPU checks of the multimodal concat head's integrated-gradients entry points in the C ABI (include/mmf_amil.h:
mmf_mm_ig_workspace_bytes, mmf_mm_ig): the descriptor is laid out in ctypes as the header compiled as C lays it out, both
symbols are bound with the header's arity, the ABI version is unchanged (the entry points are additive), every refusal comes
back in the header's order before any HIP call -- the fake pointers are never read -- and the workspace query is 0 exactly
where the header says, non-zero for every case of tests/mm_ig_cases.py and does not shrink as window_steps grows; the Python
surface refuses before the library is called.  Needs the built library, not a GPU."""
import ctypes as C
import re

import pytest

import mm_ig_cases as mc
from test_abi_layout_cpu import HEADER, _c_layout
from test_ig_abi_cpu import ALIGN, ARG, FAKE, SHAPE, WORKSPACE, _desc, _head
from test_radio_ig_abi_cpu import _rd

NEW = ["mmf_mm_ig_workspace_bytes", "mmf_mm_ig"]


def test_mm_ig_desc_matches_the_c_header(tmp_path):
    from multimodalfusion_amd import _lib
    m = _lib.MmIgDesc
    got = _c_layout(tmp_path, {"mmf_mm_ig_desc": [n for n, _ in m._fields_]})
    assert got[("mmf_mm_ig_desc", "sizeof")] == C.sizeof(m)
    for n, _ in m._fields_:
        assert got[("mmf_mm_ig_desc", n)] == getattr(m, n).offset, n


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
    rt, args = _lib.SYMBOLS["mmf_mm_ig_workspace_bytes"]
    assert rt is C.c_size_t and args == [C.c_int64] + [C.c_int32] * 4 + [C.c_int64] + [C.c_int32] * 10
    rt, args = _lib.SYMBOLS["mmf_mm_ig"]
    assert rt is C.c_int and args == [C.POINTER(_lib.MmIgDesc), C.c_void_p, C.c_size_t, C.POINTER(_lib.SurvHead), C.c_void_p]


def _mm(keep, path=True, radio=True, omic=True, pdesc=None, rdesc=None, rd=None, **kw):
    """radio_path_omic over the small gated stacks (N_p 300, N_r 300, four sequences) and omic 80 -> [256, 256], F = 768."""
    from multimodalfusion_amd import _lib
    a = (C.c_float * 64)(*([0.5] * 64))
    w = (C.c_float * 64)(*([1.0 / 64] * 64))
    d = dict(n_steps=20, window_steps=0, alpha=a, weight=w, risk_x=FAKE, risk_base=FAKE, step_risk=FAKE)
    keep += [a, w]
    col = 0
    if radio:
        rdesc = _desc() if rdesc is None else rdesc
        rd = _rd(keep) if rd is None else rd
        keep += [rdesc, rd]
        d.update(radio=C.pointer(rdesc), rd=C.pointer(rd), radio_row_sum=FAKE, radio_row_abs=FAKE, radio_col=col)
        col += rdesc.H
    if path:
        pdesc = _desc() if pdesc is None else pdesc
        keep.append(pdesc)
        d.update(path=C.pointer(pdesc), path_x=FAKE, path_row_sum=FAKE, path_row_abs=FAKE, path_col=col)
        col += pdesc.H
    if omic:
        d.update(omic_x=FAKE, omic_W0=FAKE, omic_b0=FAKE, omic_W1=FAKE, omic_b1=FAKE, omic_attr=FAKE, omic_Gin=80,
                 omic_W0n=256, omic_We=256, omic_col=col)
    d.update(kw)
    return _lib.MmIgDesc(**d)


def _call(mm=None, head=None, ws=FAKE, nbytes=1 << 40, **kw):
    from multimodalfusion_amd import _lib
    keep = []
    mm = _mm(keep, **kw) if mm is None else mm
    head = _head() if head is None else head
    return _lib.lib().mmf_mm_ig(C.byref(mm), ws, nbytes, C.byref(head), None)


def test_refusals_that_need_no_device():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    keep = []
    assert _call(nbytes=16) == WORKSPACE                            # everything else in order
    for kw in (dict(path=False), dict(radio=False), dict(omic=False)):
        assert _call(nbytes=16, **kw) == WORKSPACE, kw              # every pair of branches is a call
    # MMF_ERR_ARG: the call's own pointers and the quadrature
    assert l.mmf_mm_ig(None, FAKE, 1 << 40, C.byref(_head()), None) == ARG
    assert l.mmf_mm_ig(C.byref(_mm(keep)), FAKE, 1 << 40, None, None) == ARG
    assert _call(head=_head(Wk=None)) == ARG and _call(head=_head(bk=None)) == ARG
    for n in (0, -1, 65):
        assert _call(n_steps=n) == ARG, n
    assert _call(alpha=None) == ARG and _call(weight=None) == ARG and _call(window_steps=-1) == ARG
    for name in ("risk_x", "risk_base", "step_risk"):
        assert _call(**{name: None}) == ARG, name
    # fewer than two branches
    assert _call(path=False, radio=False) == ARG and _call(path=False, omic=False) == ARG
    assert _call(radio=False, omic=False) == ARG and _call(path=False, radio=False, omic=False) == ARG
    # per branch: inputs, outputs, dropout, the bf16x3 GEMMs
    for name in ("path_x", "path_row_sum", "path_row_abs", "radio_row_sum", "radio_row_abs", "omic_W0", "omic_b0", "omic_W1",
                 "omic_b1", "omic_attr"):
        assert _call(**{name: None}) == ARG, name
    for bad in (dict(p_h=0.25), dict(p_att=0.25), dict(gemm=1)):
        assert _call(pdesc=_desc(**bad)) == ARG and _call(rdesc=_desc(**bad)) == ARG, bad
    assert _call(pdesc=_desc(W1=None)) == ARG and _call(rdesc=_desc(Wb=None)) == ARG
    assert _call(rd=_rd(keep, null_x=True)) == ARG and _call(rd=_rd(keep, W=None)) == ARG and _call(rd=_rd(keep, bias=None)) == ARG
    for m in range(4):
        x = [FAKE] * 4
        x[m] = None
        assert _call(rd=_rd(keep, x=x)) == ARG, m
    assert _call(rd=_rd(keep, nseg=3, x=[FAKE, FAKE, FAKE, None]), nbytes=16) == WORKSPACE
    # an absent branch's pointers are not looked at
    assert _call(path=False, path_x=None, path_row_sum=None, nbytes=16) == WORKSPACE
    assert _call(radio=False, radio_row_sum=None, rd=None, nbytes=16) == WORKSPACE
    # MMF_ERR_ARG comes before every MMF_ERR_SHAPE: a bad shape next to a null pointer
    assert _call(rd=_rd(keep, nseg=5), omic_attr=None) == ARG and _call(pdesc=_desc(H=128), omic_W0=None) == ARG
    assert _call(head=_head(K=33), path_x=None) == ARG and _call(omic_W0n=2000, rd=_rd(keep, W=None)) == ARG
    # MMF_ERR_SHAPE
    for nseg in (0, 1, 5, -2):
        assert _call(rd=_rd(keep, nseg=nseg)) == SHAPE, nseg
    for bad in (dict(N=0), dict(L=1000), dict(H=128), dict(D=100)):
        assert _call(pdesc=_desc(**bad)) == SHAPE and _call(rdesc=_desc(**bad)) == SHAPE, bad
    assert _call(rd=_rd(keep, kseg=512)) == SHAPE
    assert _call(rdesc=_desc(N=131072)) == SHAPE and _call(rdesc=_desc(N=131071), nbytes=16) == WORKSPACE
    for bad in (dict(omic_Gin=0), dict(omic_W0n=0), dict(omic_W0n=1025), dict(omic_We=0), dict(omic_We=-3)):
        assert _call(**bad) == SHAPE, bad
    assert _call(omic_W0n=1024, omic_Gin=1, nbytes=16) == WORKSPACE
    # F <= 1024: 512 + 512 is the widest row, so no call admits a stack with H = 1024
    assert _call(omic=False, pdesc=_desc(H=512), rdesc=_desc(H=512), nbytes=16) == WORKSPACE
    assert _call(pdesc=_desc(H=512), rdesc=_desc(H=512)) == SHAPE and _call(omic_We=513) == SHAPE
    assert _call(radio=False, pdesc=_desc(H=1024), omic_We=1, omic_col=1024) == SHAPE
    assert _call(omic=False, pdesc=_desc(H=1024)) == SHAPE
    # the columns tile 0 .. F - 1
    assert _call(path_col=0) == SHAPE and _call(omic_col=500) == SHAPE and _call(radio_col=-256) == SHAPE
    assert _call(radio_col=512, path_col=0, omic_col=256, nbytes=16) == WORKSPACE          # any order is the caller's
    assert _call(radio=False, omic_col=0, path_col=256, nbytes=16) == WORKSPACE            # omic first
    assert _call(head=_head(K=0)) == SHAPE and _call(head=_head(K=33)) == SHAPE and _call(head=_head(K=32), nbytes=16) == WORKSPACE
    # a bag too long for one step to be a window lies beyond the descriptor's row cap as well (the header of mmf_amil_ig)
    assert _call(pdesc=_desc(N=1 << 20, L=32)) == SHAPE and _call(pdesc=_desc(N=(1 << 20) - 1, L=32), nbytes=16) == WORKSPACE
    # a shape refusal comes before an alignment refusal
    assert _call(head=_head(K=33), path_x=FAKE + 4) == SHAPE and _call(omic_We=0, rd=_rd(keep, W=FAKE + 4)) == SHAPE
    # MMF_ERR_ALIGN
    assert _call(path_x=FAKE + 4) == ALIGN and _call(path_attr=FAKE + 4) == ALIGN and _call(radio_attr=FAKE + 4) == ALIGN
    assert _call(pdesc=_desc(W1=FAKE + 4)) == ALIGN and _call(rdesc=_desc(Wa=FAKE + 4)) == ALIGN
    assert _call(rd=_rd(keep, W=FAKE + 4)) == ALIGN and _call(rd=_rd(keep, x=[FAKE, FAKE + 8, FAKE, FAKE])) == ALIGN
    assert _call(ws=FAKE + 8) == ALIGN and _call(ws=None) == ARG
    assert _call(path=False, ws=FAKE + 8) == ALIGN and _call(radio=False, ws=FAKE + 8) == ALIGN
    # the omic operands are read element by element: any alignment
    assert _call(omic_x=FAKE + 4, omic_W0=FAKE + 4, omic_W1=FAKE + 4, omic_attr=FAKE + 4, nbytes=16) == WORKSPACE
    assert _call(path_attr=FAKE, radio_attr=FAKE, nbytes=16) == WORKSPACE
    # an alignment refusal comes before the workspace's
    assert _call(path_x=FAKE + 4, nbytes=16) == ALIGN
    need = l.mmf_mm_ig_workspace_bytes(300, 1024, 256, 256, 1, 300, 4, 1024, 256, 256, 1, 80, 256, 256, 20, 0)
    assert need > 0 and _call(nbytes=need - 1) == WORKSPACE


OK = dict(Np=300, Lp=1024, Hp=256, Dp=256, gp=1, Nr=33, nseg=4, kseg=1024, Hr=256, Dr=256, gr=1, Gin=80, W0=256, We=256,
          n_steps=20, window_steps=0)


def _q(**kw):
    from multimodalfusion_amd import _lib
    return _lib.lib().mmf_mm_ig_workspace_bytes(*{**OK, **kw}.values())


def test_workspace_query_is_zero_exactly_where_the_header_says():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    assert _q() > 0
    for kw in (dict(n_steps=0), dict(n_steps=65), dict(window_steps=-1), dict(Np=-1), dict(Nr=-1), dict(Gin=-1),
               dict(Np=0, Nr=0), dict(Np=0, Gin=0), dict(Nr=0, Gin=0), dict(Np=0, Nr=0, Gin=0),          # fewer than two branches
               dict(Lp=31), dict(Hp=31), dict(Np=1 << 22, Lp=32),                                        # mmf_amil_ig's zeros
               dict(nseg=1), dict(nseg=5), dict(kseg=31), dict(Hr=31), dict(Nr=131072),                  # mmf_radio_ig's
               dict(W0=0), dict(W0=1025), dict(We=0), dict(We=513), dict(Hp=512, Hr=512), dict(Hp=1024, Nr=0, We=1)):
        assert _q(**kw) == 0, kw
    for kw in (dict(n_steps=1), dict(n_steps=64), dict(window_steps=64), dict(Np=0), dict(Nr=0), dict(Gin=0), dict(Np=1, Nr=1),
               dict(Gin=1), dict(W0=1), dict(W0=1024), dict(We=1), dict(We=512), dict(Hp=512, Hr=512, Gin=0), dict(gp=0, gr=0),
               dict(nseg=2), dict(Nr=131071)):
        assert _q(**kw) > 0, kw
    # an absent branch's extents are not looked at
    assert _q(Np=0, Lp=0, Hp=0, Dp=0) == _q(Np=0, Lp=7, Hp=9, Dp=11) > 0
    assert _q(Nr=0, nseg=0, kseg=0, Hr=0, Dr=0) > 0 and _q(Gin=0, W0=0, We=0) > 0
    # it holds both single-head workspaces: the stacks run in the same windows
    both = l.mmf_amil_ig_workspace_bytes(300, 1024, 256, 256, 1, 20, 0) + l.mmf_radio_ig_workspace_bytes(33, 4, 1024, 256, 256, 1, 20, 0)
    assert _q() >= both and _q(Gin=0) >= both


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_workspace_of_every_case(name):
    c = mc.BY_NAME[name]
    p, r, o = c.path, c.radio, c.omic
    args = dict(Np=p.N if p else 0, Lp=p.L if p else 0, Hp=p.H if p else 0, Dp=p.D if p else 0, gp=int(p.gated) if p else 0,
                Nr=r.N if r else 0, nseg=r.nseg if r else 0, kseg=r.kseg if r else 0, Hr=r.H if r else 0, Dr=r.D if r else 0,
                gr=int(r.gated) if r else 0, Gin=o.Gin if o else 0, W0=o.W0 if o else 0, We=o.We if o else 0, n_steps=c.n_steps)
    prev = 0
    for ws in range(1, c.n_steps + 3):                              # does not decrease in window_steps, up to the clamp
        cur = _q(**args, window_steps=ws)
        assert cur >= prev and cur > 0, ws
        prev = cur
    assert _q(**args, window_steps=64) >= prev
    assert 0 < _q(**args, window_steps=0) <= _q(**args, window_steps=64)


def test_python_surface_refuses_before_the_library_is_called():
    import torch
    from multimodalfusion_amd import _lib, infer, ops
    from multimodalfusion_amd.models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    mods = ["T1", "T2", "T1Gd", "FLAIR"]
    model = MM_MIL_Attention_fc_surv(input_dim=80, fusion="concat", dropout=False, n_classes=4, mode="radio_path_omic")
    feats = {m: torch.zeros(4, 1024) for m in mods}
    feats.update(path_features=torch.zeros(6, 1024), genomic_features=torch.zeros(80))
    model.train()
    with pytest.raises(RuntimeError):
        model.integrated_gradients(**feats)
    with pytest.raises(RuntimeError):
        infer.mm_integrated_gradients_autograd(model, feats, [0.5], [1.0])
    model.eval()
    tensor = MM_MIL_Attention_fc_surv(input_dim=80, fusion="tensor", dropout=False, n_classes=4, mode="radio_path_omic").eval()
    with pytest.raises(NotImplementedError):
        tensor.integrated_gradients(**feats)
    for k in ("T2", "path_features", "genomic_features"):
        with pytest.raises(NotImplementedError):
            model.integrated_gradients(**{**feats, k: feats[k].to(torch.bfloat16)})
    with pytest.raises(NotImplementedError):
        ops.mm_integrated_gradients([("path", feats["path_features"].to(torch.bfloat16), (None,) * 8, True),
                                     ("omic", feats["genomic_features"], None, None, None, None)], None, None, [0.5], [1.0])
    for k in ("T1Gd", "path_features", "genomic_features"):
        with pytest.raises(_lib.MmfError):
            model.integrated_gradients(**{n: v for n, v in feats.items() if n != k})
    with pytest.raises(_lib.MmfError):
        model.integrated_gradients(**{**feats, "T2": torch.zeros(5, 1024)})
    with pytest.raises(_lib.MmfError):
        model.integrated_gradients(**{**feats, "genomic_features": torch.zeros(79)})
    with pytest.raises(_lib.MmfError):
        ops.mm_integrated_gradients([("path", feats["path_features"], (None,) * 8, True)], None, None, [0.5], [1.0])
    h = model.fc_omic.register_forward_hook(lambda *a: None)
    try:
        with pytest.raises(NotImplementedError):
            model.integrated_gradients(**feats)
    finally:
        h.remove()
    wide = MM_MIL_Attention_fc_surv(input_dim=80, fusion="concat", dropout=False, n_classes=33, mode="radio_path_omic").eval()
    with pytest.raises(NotImplementedError):
        wide.integrated_gradients(**feats)
    with pytest.raises(ValueError):
        model.integrated_gradients(method="riemann_left", **feats)
    with pytest.raises(NotImplementedError):
        infer.attribute_modalities(torch.nn.Linear(4, 4), feats)
    # a mode without a branch does not ask for its input
    po = MM_MIL_Attention_fc_surv(input_dim=80, fusion="concat", dropout=False, n_classes=4, mode="path_omic").eval()
    with pytest.raises(_lib.MmfError):
        po.integrated_gradients(path_features=feats["path_features"])
