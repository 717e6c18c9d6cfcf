"""CPU checks of the multimodal tensor-fusion head's integrated-gradients entry points in the C ABI (include/mmf_amil.h:
mmf_mm_ig_tensor_workspace_bytes, mmf_mm_ig_tensor): both symbols are bound with the header's arity, the ABI version and
mmf_mm_ig_desc are unchanged (the entry points are additive), every refusal comes back in the header's order before any HIP
call -- the fake pointers are never read -- and the workspace query is 0 where the header says, follows the header's
formula, grows with S and does not shrink as window_steps grows; the Python surface refuses before the library is called.
Needs the built library, not a GPU."""
import ctypes as C
import re

import pytest

import mm_tensor_ig_cases as tc
from test_abi_layout_cpu import HEADER
from test_ig_abi_cpu import ALIGN, ARG, FAKE, SHAPE, WORKSPACE, _desc, _head
from test_mm_ig_abi_cpu import OK, _mm
from test_radio_ig_abi_cpu import _rd

NEW = ["mmf_mm_ig_tensor_workspace_bytes", "mmf_mm_ig_tensor"]


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
    rt, args = _lib.SYMBOLS["mmf_mm_ig_tensor"]
    assert rt is C.c_int and args == [C.POINTER(_lib.MmIgDesc), C.POINTER(_lib.XFusionWeights), C.c_void_p, C.c_size_t,
                                      C.POINTER(_lib.SurvHead), C.c_void_p]


def _xf(m=3, dim=256, sdim=16, mmhid1=512, mmhid2=256, nhid=256, **kw):
    from multimodalfusion_amd import _lib
    x = _lib.XFusionWeights(m=m, dim=dim, sdim=sdim, mmhid1=mmhid1, mmhid2=mmhid2, nhid=nhid,
                            **{n: kw.get(n, FAKE) for n in ("We1", "be1", "We2", "be2", "Wc0", "bc0")})
    for n in ("Wh", "bh", "Wz", "bz", "Wo", "bo"):
        for i in range(3):
            getattr(x, n)[i] = kw.get(f"{n}{i}", FAKE)
    return x


def _call(mm=None, xf=None, head=None, ws=FAKE, nbytes=1 << 40, **kw):
    from multimodalfusion_amd import _lib
    keep = []
    m = 3 - sum(1 for b in ("path", "radio", "omic") if kw.get(b) is False)
    mm = _mm(keep, **kw) if mm is None else mm
    xf = _xf(m=m) if xf is None else xf
    head = _head() if head is None else head
    return _lib.lib().mmf_mm_ig_tensor(C.byref(mm), C.byref(xf) if xf is not False else None, ws, nbytes, C.byref(head), None)


def test_refusals_that_need_no_device():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    keep = []
    assert _call(nbytes=16) == WORKSPACE                            # everything else in order
    for kw in (dict(path=False), dict(radio=False), dict(omic=False)):
        assert _call(nbytes=16, **kw) == WORKSPACE, kw              # every pair of branches is a call
    # MMF_ERR_ARG: everything mmf_mm_ig refuses with it ...
    assert l.mmf_mm_ig_tensor(None, C.byref(_xf()), FAKE, 1 << 40, C.byref(_head()), None) == ARG
    assert l.mmf_mm_ig_tensor(C.byref(_mm(keep)), C.byref(_xf()), FAKE, 1 << 40, None, None) == ARG
    assert _call(head=_head(Wk=None)) == ARG and _call(head=_head(bk=None)) == ARG
    for n in (0, -1, 65):
        assert _call(n_steps=n) == ARG, n
    assert _call(alpha=None) == ARG and _call(weight=None) == ARG and _call(window_steps=-1) == ARG
    for name in ("risk_x", "risk_base", "step_risk", "path_x", "path_row_sum", "radio_row_abs", "omic_W1", "omic_attr"):
        assert _call(**{name: None}) == ARG, name
    assert _call(path=False, radio=False) == ARG and _call(radio=False, omic=False) == ARG
    for bad in (dict(p_h=0.25), dict(p_att=0.25), dict(gemm=1)):
        assert _call(pdesc=_desc(**bad)) == ARG and _call(rdesc=_desc(**bad)) == ARG, bad
    assert _call(pdesc=_desc(W1=None)) == ARG and _call(rd=_rd(keep, W=None)) == ARG
    # ... a null xf, and a null weight or bias of xf
    assert _call(xf=False) == ARG
    for n in ("We1", "be1", "We2", "be2", "Wc0", "bc0", "Wh0", "bh1", "Wz2", "bz0", "Wo1", "bo2"):
        assert _call(xf=_xf(**{n: None})) == ARG, n
    assert _call(omic=False, xf=_xf(m=2, Wh2=None, bo2=None), nbytes=16) == WORKSPACE     # a third modality's are not read
    # MMF_ERR_ARG comes before every MMF_ERR_SHAPE, a wild m included
    assert _call(xf=_xf(m=7, We1=None)) == ARG and _call(xf=_xf(dim=255), omic_attr=None) == ARG
    assert _call(xf=_xf(m=-4), path_x=None) == ARG and _call(head=_head(K=33), xf=_xf(Wz1=None)) == ARG
    # MMF_ERR_SHAPE: the stacks and the omic widths as mmf_mm_ig
    for nseg in (0, 1, 5):
        assert _call(rd=_rd(keep, nseg=nseg)) == SHAPE, nseg
    for bad in (dict(N=0), dict(L=1000), dict(H=128), dict(D=100)):
        assert _call(pdesc=_desc(**bad)) == SHAPE and _call(rdesc=_desc(**bad)) == SHAPE, bad
    for bad in (dict(omic_Gin=0), dict(omic_W0n=0), dict(omic_W0n=1025), dict(omic_We=0)):
        assert _call(**bad) == SHAPE, bad
    # the tail's own rules at G = S
    for bad in (dict(m=1), dict(m=4), dict(m=7), dict(sdim=8), dict(dim=0), dict(dim=258), dict(mmhid1=0), dict(mmhid1=510),
                dict(mmhid1=772), dict(mmhid2=0), dict(mmhid2=1537), dict(nhid=0)):
        assert _call(xf=_xf(**bad)) == SHAPE, bad
    assert _call(xf=_xf(mmhid1=768, mmhid2=1536), nbytes=16) == WORKSPACE                  # K2 = 1536, the widest row
    # xf->m against the number of branches, the widths against xf->dim
    assert _call(xf=_xf(m=2)) == SHAPE and _call(omic=False, xf=_xf(m=3)) == SHAPE
    assert _call(xf=_xf(dim=128)) == SHAPE and _call(omic_We=128) == SHAPE
    assert _call(omic=False, pdesc=_desc(H=512), rdesc=_desc(H=512), xf=_xf(m=2, dim=512), nbytes=16) == WORKSPACE
    assert _call(omic=False, pdesc=_desc(H=512), xf=_xf(m=2, dim=512)) == SHAPE
    assert _call(pdesc=_desc(H=512), rdesc=_desc(H=512), omic_We=512, xf=_xf(dim=512, mmhid1=4)) == SHAPE   # K2 > 1536
    # the columns tile 0 .. m dim - 1 in steps of dim
    assert _call(path_col=0) == SHAPE and _call(omic_col=500) == SHAPE and _call(radio_col=-256) == SHAPE
    assert _call(radio_col=512, path_col=0, omic_col=256, nbytes=16) == WORKSPACE
    assert _call(radio=False, omic_col=0, path_col=256, nbytes=16) == WORKSPACE            # omic first
    # nhid: hid is kept in LDS; K
    assert _call(xf=_xf(nhid=1025)) == SHAPE and _call(xf=_xf(nhid=1024), nbytes=16) == WORKSPACE
    assert _call(head=_head(K=0)) == SHAPE and _call(head=_head(K=33)) == SHAPE and _call(head=_head(K=32), nbytes=16) == WORKSPACE
    assert _call(pdesc=_desc(N=1 << 20, L=32)) == SHAPE
    # a shape refusal comes before an alignment refusal
    assert _call(xf=_xf(nhid=1025, Wh0=FAKE + 4)) == SHAPE and _call(head=_head(K=33), path_x=FAKE + 4) == SHAPE
    # MMF_ERR_ALIGN: everything mmf_mm_ig refuses with it, then Wh_i and Wz_i
    assert _call(path_x=FAKE + 4) == ALIGN and _call(path_attr=FAKE + 4) == ALIGN and _call(rd=_rd(keep, W=FAKE + 4)) == ALIGN
    assert _call(ws=FAKE + 8) == ALIGN and _call(ws=None) == ARG
    for n in ("Wh0", "Wh2", "Wz1"):
        assert _call(xf=_xf(**{n: FAKE + 4})) == ALIGN, n
    assert _call(xf=_xf(bh0=FAKE + 4, Wo1=FAKE + 4, We1=FAKE + 4, Wc0=FAKE + 4), nbytes=16) == WORKSPACE
    # an alignment refusal comes before the workspace's
    assert _call(xf=_xf(Wz0=FAKE + 8), nbytes=16) == ALIGN
    need = _q(Np=300, Nr=300)
    assert need > 0 and _call(nbytes=need - 1) == WORKSPACE


TAIL = dict(dim=256, sdim=16, mmhid1=512, mmhid2=256, nhid=256)


def _q(**kw):
    from multimodalfusion_amd import _lib
    return _lib.lib().mmf_mm_ig_tensor_workspace_bytes(*{**OK, **TAIL, **kw}.values())


def _concat(**kw):
    from multimodalfusion_amd import _lib
    return _lib.lib().mmf_mm_ig_workspace_bytes(*{**OK, **kw}.values())


def test_workspace_query_is_zero_for_refused_shapes_and_follows_the_headers_formula():
    assert _q() > 0
    for kw in (dict(n_steps=0), dict(n_steps=65), dict(window_steps=-1), dict(Np=-1), dict(Np=0, Nr=0), dict(Nr=0, Gin=0),
               dict(Lp=31), dict(Hp=31), dict(nseg=5), dict(kseg=31), dict(Nr=131072), dict(W0=0), dict(W0=1025), dict(We=0),
               dict(sdim=8), dict(dim=128), dict(dim=258), dict(We=128), dict(Hp=512), dict(mmhid1=510), dict(mmhid1=772),
               dict(mmhid2=0), dict(mmhid2=1537), dict(nhid=0), dict(nhid=1025)):
        assert _q(**kw) == 0, kw
    for kw in (dict(n_steps=1), dict(n_steps=64), dict(window_steps=64), dict(Np=0), dict(Nr=0), dict(Gin=0), dict(nhid=1024),
               dict(Hp=512, Hr=512, Gin=0, dim=512), dict(mmhid1=768, mmhid2=1536)):
        assert _q(**kw) > 0, kw
    # the concat query's stack and omic parts (its feat / dfeat [S x F] are not carved) plus the tail's buffers at S rows
    r256 = lambda n: (n + 255) // 256 * 256
    for S, m, kw in ((1, 3, {}), (3, 3, {}), (22, 3, {}), (5, 2, dict(Gin=0)), (7, 2, dict(Np=0, mmhid1=100, mmhid2=7, nhid=6))):
        kw = dict(kw, n_steps=20, window_steps=S)
        t = {**TAIL, **kw}
        F, K2, E = m * 256, t["mmhid1"] + m * 256, 17 ** m
        words = (E + 63) // 64 * 2
        tail = (2 * r256(4 * S * K2) + 3 * r256(4 * S * t["mmhid2"]) + 7 * r256(4 * S * m * 16) + r256(4 * S * E) + r256(4 * S)
                + r256(4 * S * words))
        assert _q(**kw) == _concat(**kw) - 2 * r256(4 * S * F) + tail, (S, m)


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_workspace_of_every_case(name):
    c = tc.BY_NAME[name]
    p, r, o = c.path, c.radio, c.omic
    args = dict(Np=p.N if p else 0, Lp=p.L if p else 0, Hp=p.H if p else 0, Dp=p.D if p else 0, gp=int(p.gated) if p else 0,
                Nr=r.N if r else 0, nseg=r.nseg if r else 0, kseg=r.kseg if r else 0, Hr=r.H if r else 0, Dr=r.D if r else 0,
                gr=int(r.gated) if r else 0, Gin=o.Gin if o else 0, W0=o.W0 if o else 0, We=o.We if o else 0, n_steps=c.n_steps,
                dim=tc.dim(c), mmhid1=c.tail.mmhid1, mmhid2=c.tail.mmhid2, nhid=c.tail.nhid)
    prev = 0
    for ws in range(1, c.n_steps + 3):                              # monotone in S = window_steps, up to the clamp
        cur = _q(**args, window_steps=ws)
        assert cur >= prev and cur > 0, ws
        prev = cur
    assert _q(**args, window_steps=64) >= prev
    assert 0 < _q(**args, window_steps=0) <= _q(**args, window_steps=64)


def test_python_surface_refuses_before_the_library_is_called():
    import torch
    from multimodalfusion_amd import _lib
    from multimodalfusion_amd.models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    mods = ["T1", "T2", "T1Gd", "FLAIR"]
    feats = {m: torch.zeros(4, 1024) for m in mods}
    feats.update(path_features=torch.zeros(6, 1024), genomic_features=torch.zeros(80))
    make = lambda **kw: MM_MIL_Attention_fc_surv(input_dim=80, dropout=False, n_classes=4, mode="radio_path_omic", **kw)
    concat = make(fusion="concat").eval()
    with pytest.raises(NotImplementedError, match="integrated_gradients"):
        concat.integrated_gradients_tensor(**feats)
    model = make()                                                   # fusion = 'tensor' is the default
    assert model.fusion == "tensor"
    model.train()
    with pytest.raises(RuntimeError):
        model.integrated_gradients_tensor(**feats)
    model.eval()
    with pytest.raises(NotImplementedError, match="integrated_gradients_tensor"):     # the concat method points at the new one
        model.integrated_gradients(**feats)
    for k in ("T2", "path_features", "genomic_features"):
        with pytest.raises(NotImplementedError):
            model.integrated_gradients_tensor(**{**feats, k: feats[k].to(torch.bfloat16)})
    for k in ("T1Gd", "path_features", "genomic_features"):
        with pytest.raises(_lib.MmfError):
            model.integrated_gradients_tensor(**{k2: v for k2, v in feats.items() if k2 != k})
    with pytest.raises(_lib.MmfError):
        model.integrated_gradients_tensor(**{**feats, "genomic_features": torch.zeros(79)})
    with pytest.raises(ValueError):
        model.integrated_gradients_tensor(method="riemann_left", **feats)
    # a scale width the grouped fusion kernels do not take
    wide = make()
    for i in range(3):
        wide.mm.reduce[i][0][0] = torch.nn.Linear(256, 8)
    assert not wide.eval().xfusion_group_ok()
    with pytest.raises(NotImplementedError):
        wide.integrated_gradients_tensor(**feats)
    h = model.fc_omic.register_forward_hook(lambda *a: None)
    try:
        with pytest.raises(NotImplementedError):
            model.integrated_gradients_tensor(**feats)
    finally:
        h.remove()
