"""CPU checks of the stage-2 integrated-gradients entry points in the C ABI (include/mmf_amil.h: mmf_stage2_ig_workspace_bytes,
mmf_stage2_ig): the descriptor's ctypes mirrors against the header compiled as C, both symbols bound with the header's arity,
every refusal in the header's order before any HIP call -- the fake pointers are never read -- and the workspace query's
zeros and monotonicity.  Needs the built library, not a GPU."""
import ctypes as C
import re

from test_abi_layout_cpu import HEADER, _c_layout

FAKE = 0x7F0000001000
OK, ARG, SHAPE, ALIGN, WORKSPACE = 0, -1, -2, -3, -4
NLL, COX = 0, 1
EF, LF, EH, LH, KR = range(5)
NEW = ["mmf_stage2_ig_workspace_bytes", "mmf_stage2_ig"]


def test_mirrors_match_the_header_compiled_as_c(tmp_path):
    from multimodalfusion_amd import _lib
    mirrors = {"mmf_bn1d": _lib.Bn1d, "mmf_stage2_block": _lib.Stage2Block, "mmf_stage2_ig_desc": _lib.Stage2IgDesc}
    got = _c_layout(tmp_path, {c: [n for n, _ in m._fields_] for c, m in mirrors.items()})
    for cname, m in mirrors.items():
        assert got[(cname, "sizeof")] == C.sizeof(m), cname
        for n, _ in m._fields_:
            assert got[(cname, n)] == getattr(m, n).offset, (cname, n)


def test_new_symbols_are_bound_with_the_headers_arity():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(l, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
    for macro in ("MMF_STAGE2_NLL 0", "MMF_STAGE2_COX 1", "MMF_STAGE2_EARLY_FCNN 0", "MMF_STAGE2_LATE_FCNN 1",
                  "MMF_STAGE2_EARLY_HIGHWAY 2", "MMF_STAGE2_LATE_HIGHWAY 3", "MMF_STAGE2_KRONECKER 4"):
        assert "#define " + macro in text
    assert l.mmf_abi_version() == _lib.ABI_VERSION          # additive: the version stays


def _bn(**kw):
    from multimodalfusion_amd import _lib
    return _lib.Bn1d(**{n: kw.get(n, FAKE) for n in ("weight", "bias", "mean", "var")}, eps=1e-5)


def _desc(keep, family=NLL, tt=EF, present=(1, 1, 1), n_layers=1, P=5, K=4, n_steps=20, blk=None, xf=None, **kw):
    """A descriptor of fake pointers; kw overrides a member (None: a null pointer); blk: {index: {member: value}}."""
    from multimodalfusion_amd import _lib
    a = (C.c_float * 64)(*([0.5] * 64))
    keep.append(a)
    d = _lib.Stage2IgDesc(family=family, train_type=tt, radio=present[0], path=present[1], omic=present[2], n_layers=n_layers,
                          P=P, K=K, n_steps=n_steps, alpha=a, weight=a)
    for n in ("Wk", "bk", "mod_sum", "mod_abs", "risk", "risk_base", "step_risk", "hazards", "S"):
        setattr(d, n, FAKE)
    for i in range(3):
        d.v[i] = FAKE
        b = d.blk[i]
        b.W0, b.b0, b.W4, b.b4, b.bn, b.bn1, b.bn2 = FAKE, FAKE, FAKE, FAKE, _bn(), _bn(), _bn()
        for n in ("Wgate", "bgate", "Wnl", "bnl", "Wlin", "blin"):
            arr = (C.c_void_p * max(1, n_layers))(*([FAKE] * max(1, n_layers)))
            keep.append(arr)
            setattr(b, n, arr)
        for n, v in (blk or {}).get(i, {}).items():
            if isinstance(v, list):
                v = (C.c_void_p * len(v))(*v)
                keep.append(v)
            setattr(b, n, v if v is not None else (C.POINTER(C.c_void_p)() if n[0] in "Wb" and n[1:] in ("gate", "nl", "lin") else None))
    if tt == KR and xf is not False:
        m = sum(1 for f in present if f)
        x = _lib.XFusionWeights(m=m, dim=256, sdim=16, mmhid1=256, mmhid2=256, nhid=4, We1=FAKE, be1=FAKE, We2=FAKE, be2=FAKE)
        for n in ("Wh", "bh", "Wz", "bz", "Wo", "bo"):
            for i in range(3):
                getattr(x, n)[i] = FAKE
        for n, v in (xf or {}).items():
            if n[-1].isdigit() and n[:-1] in ("Wh", "bh", "Wz", "bz", "Wo", "bo"):
                getattr(x, n[:-1])[int(n[-1])] = v
            else:
                setattr(x, n, v)
        keep.append(x)
        d.xf = C.pointer(x)
    for n, v in kw.items():
        if n.startswith("v") and n[1:].isdigit():
            d.v[int(n[1:])] = v
        elif n.startswith("attr"):
            d.attr[int(n[4:])] = v
        elif n in ("alpha", "weight"):
            setattr(d, n, v if v is not None else C.POINTER(C.c_float)())
        else:
            setattr(d, n, v)
    return d


def _call(ws=FAKE, nbytes=1 << 40, **kw):
    from multimodalfusion_amd import _lib
    keep = []
    return _lib.lib().mmf_stage2_ig(C.byref(_desc(keep, **kw)), ws, nbytes, None)


def test_refusals_in_the_headers_order_before_any_launch():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    types = [(f, t) for f in (NLL, COX) for t in (EF, LF, EH, LH, KR)]
    for f, t in types:                                   # everything else in order: only the workspace is wrong
        K = 1 if f == COX else 4
        assert _call(family=f, tt=t, K=K, nbytes=16) == WORKSPACE, (f, t)
        for present in ((1, 1, 0), (1, 0, 1), (0, 1, 1)):
            assert _call(family=f, tt=t, K=K, present=present, nbytes=16) == WORKSPACE, (f, t, present)
    # MMF_ERR_ARG
    assert l.mmf_stage2_ig(None, FAKE, 1 << 40, None) == ARG
    for n in ("alpha", "weight", "Wk", "bk", "mod_sum", "mod_abs", "risk", "risk_base", "step_risk", "v0", "v2"):
        assert _call(**{n: None}) == ARG, n
    assert _call(present=(1, 1, 0), v2=None, nbytes=16) == WORKSPACE          # a third embedding is not read
    assert _call(hazards=None, S=None, nbytes=16) == WORKSPACE                # optional outputs
    for bad in (dict(family=-1), dict(family=2), dict(tt=-1), dict(tt=5)):
        assert _call(**bad) == ARG, bad
    assert _call(tt=EF, blk={0: dict(W0=None)}) == ARG and _call(tt=EF, blk={0: dict(bn=_bn(var=None))}) == ARG
    assert _call(tt=EF, blk={1: dict(W0=None)}, nbytes=16) == WORKSPACE       # the early types read blk[0] alone
    assert _call(tt=LF, blk={2: dict(b0=None)}) == ARG and _call(tt=LF, blk={1: dict(W4=None)}, nbytes=16) == WORKSPACE
    assert _call(family=COX, K=1, tt=LF, blk={1: dict(W4=None)}) == ARG
    assert _call(tt=EH, blk={0: dict(bn2=_bn(mean=None))}) == ARG and _call(tt=LH, blk={2: dict(Wnl=None)}) == ARG
    assert _call(tt=LH, blk={1: dict(blin=[None])}) == ARG and _call(tt=EH, blk={0: dict(W0=None)}, nbytes=16) == WORKSPACE
    assert _call(tt=KR, xf=False) == ARG
    for n in ("We1", "be2", "Wh0", "bz1", "Wo2"):
        assert _call(tt=KR, xf={n: None}) == ARG, n
    assert _call(tt=KR, present=(1, 1, 0), xf=dict(Wh2=None), nbytes=16) == WORKSPACE
    # MMF_ERR_ARG comes before every MMF_ERR_SHAPE
    assert _call(P=0, Wk=None) == ARG and _call(n_steps=65, family=7) == ARG and _call(K=33, v1=None) == ARG
    # MMF_ERR_SHAPE
    for bad in (dict(P=0), dict(P=-3), dict(P=(1 << 20) + 1), dict(n_steps=0), dict(n_steps=65), dict(K=0), dict(K=33),
                dict(n_layers=0), dict(present=(1, 0, 0)), dict(present=(0, 0, 0)), dict(family=COX, K=4)):
        assert _call(**bad) == SHAPE, bad
    assert _call(K=32, n_steps=64, nbytes=16) == WORKSPACE and _call(n_steps=1, K=1, P=1, nbytes=16) == WORKSPACE
    for n, v in (("m", 2), ("dim", 128), ("sdim", 8), ("mmhid1", 512), ("mmhid2", 128)):
        assert _call(tt=KR, xf={n: v}) == SHAPE, n
    for t in (EH, LH):                                                         # a Highway's depth: 1 .. 8
        assert _call(tt=t, n_layers=9) == SHAPE
        assert _call(tt=t, n_layers=2, nbytes=16) == WORKSPACE and _call(tt=t, n_layers=8, nbytes=16) == WORKSPACE
        assert _call(tt=t, n_layers=2, blk={0: dict(Wlin=[FAKE, None])}) == ARG      # a null entry of a per-layer array
    assert _call(tt=EF, n_layers=9, nbytes=16) == WORKSPACE                    # the fcnn types have no layers to count
    # a shape refusal comes before an alignment refusal
    assert _call(P=0, v0=FAKE + 4) == SHAPE
    # MMF_ERR_ALIGN
    assert _call(v1=FAKE + 4) == ALIGN and _call(attr0=FAKE + 8) == ALIGN and _call(ws=FAKE + 4) == ALIGN
    assert _call(ws=None) == ARG and _call(attr2=FAKE, nbytes=16) == WORKSPACE
    assert _call(tt=KR, xf=dict(Wh1=FAKE + 4)) == ALIGN and _call(tt=KR, xf=dict(Wz0=FAKE + 8)) == ALIGN
    assert _call(tt=KR, xf=dict(bh0=FAKE + 4, Wo1=FAKE + 4), nbytes=16) == WORKSPACE
    assert _call(Wk=FAKE + 4, blk={0: dict(W0=FAKE + 4)}, nbytes=16) == WORKSPACE   # read one float at a time
    # an alignment refusal comes before the workspace's
    assert _call(v0=FAKE + 4, nbytes=16) == ALIGN
    for f, t in types:
        K = 1 if f == COX else 4
        need = l.mmf_stage2_ig_workspace_bytes(f, t, 3, 1, 5, K, 20)
        assert need > 0 and _call(family=f, tt=t, K=K, nbytes=need - 1) == WORKSPACE


def test_workspace_query_zeros_formula_and_monotonicity():
    from multimodalfusion_amd import _lib
    q = _lib.lib().mmf_stage2_ig_workspace_bytes
    ok = dict(family=NLL, tt=EF, m=3, n_layers=1, P=5, K=4, n_steps=20)
    ask = lambda **kw: q(*{**ok, **kw}.values())
    assert ask() > 0
    for kw in (dict(family=2), dict(family=-1), dict(tt=5), dict(tt=-1), dict(m=1), dict(m=4), dict(n_layers=0), dict(P=0),
               dict(P=(1 << 20) + 1), dict(K=0), dict(K=33), dict(n_steps=0), dict(n_steps=65), dict(family=COX),
               dict(tt=EH, n_layers=9), dict(tt=LH, n_layers=100)):
        assert ask(**kw) == 0, kw
    r256 = lambda n: (n + 255) // 256 * 256
    for tt, m, ld in ((EF, 3, 128), (EF, 2, 128), (LF, 3, 384), (LF, 2, 256), (EH, 3, 2304), (LH, 2, 1536)):
        for P in (1, 5, 33):
            assert ask(tt=tt, m=m, P=P) == r256(4 * (P + 1) * ld) + r256(4 * P * ld), (tt, m, P)
    # highway with n_layers >= 2: 4 n_layers + 5 more buffers of S x 256 m floats, S = min(256, P (n_steps + 2))
    for tt, m, L, P, n in ((EH, 3, 2, 5, 20), (LH, 2, 2, 33, 4), (LH, 3, 8, 1, 1), (EH, 2, 3, 100, 20)):
        S, ld = min(256, P * (n + 2)), 768 * m
        want = r256(4 * (P + 1) * ld) + r256(4 * P * ld) + (4 * L + 5) * r256(4 * S * 256 * m)
        assert ask(tt=tt, m=m, n_layers=L, P=P, n_steps=n) == want, (tt, m, L, P, n)
    for f in (NLL, COX):
        for tt, L in ((EF, 1), (LF, 1), (EH, 1), (LH, 1), (KR, 1), (EH, 2), (LH, 3)):
            for m in (2, 3):
                K = 1 if f == COX else 32
                prev = 0
                for P in (1, 2, 3, 5, 33, 34, 1000):
                    cur = ask(family=f, tt=tt, m=m, K=K, P=P, n_layers=L)
                    assert cur > prev, (f, tt, m, P)
                    prev = cur
                prev = 0
                for n in (1, 2, 4, 20, 30, 62, 64):
                    cur = ask(family=f, tt=tt, m=m, K=K, P=1, n_steps=n, n_layers=L)
                    assert cur >= prev > -1 and cur > 0, (f, tt, m, n)
                    prev = cur
    # kronecker: the accumulator and the tail's buffers for S = min(64, P (n_steps + 2)) rows
    for m, P, n in ((3, 1, 4), (2, 3, 20), (3, 5, 20)):
        S, K2, E = min(64, P * (n + 2)), 256 + 256 * m, 17 ** m
        words = (E + 63) // 64 * 2
        tail = (2 * r256(4 * S * K2) + 3 * r256(4 * S * 256) + 7 * r256(4 * S * m * 16) + r256(4 * S * E) + r256(4 * S)
                + r256(4 * S * words))
        assert ask(tt=KR, m=m, P=P, n_steps=n) == r256(4 * P * 256 * m) + tail, (m, P, n)


def test_python_surface_refuses_before_the_library_is_called():
    import pytest
    import torch
    from multimodalfusion_amd import _lib
    from multimodalfusion_amd.models import coxranking_models_pretrained as cm
    from multimodalfusion_amd.models import nll_models_pretrained as nm
    h = torch.zeros(3, 256)
    for mod in (nm, cm):
        model = mod.multimodal_pretrained(train_type="early-fcnn", mode="radio_path")
        with pytest.raises(RuntimeError):
            model.integrated_gradients(h, h, h)                                  # train mode
        model.eval()
        with pytest.raises(NotImplementedError):
            model.integrated_gradients(h.double(), h, None)
        with pytest.raises(_lib.MmfError):
            model.integrated_gradients(h, None, h)                               # the mode keeps pathology
        with pytest.raises(ValueError):
            model.integrated_gradients(h, h, None, method="riemann_left")
        with pytest.raises(_lib.MmfError):
            model.integrated_gradients(h, h, None)                               # CPU tensors: there is no CPU path
        for name in ("captum", "captum_radio_path", "captum_path_omic", "captum_radio_omic"):
            assert callable(getattr(model, name))
