"""CPU checks of the tensor fusion's grouped training step in the C ABI (include/mmf_amil.h: mmf_xfusion_grads,
mmf_xfusion_group_workspace_bytes, mmf_xfusion_group_forward, mmf_xfusion_group_backward): the new struct is laid out in
ctypes as the header compiled as C lays it out, every new prototype has the arity its binding declares, the workspace
query answers 0 outside every limit, refusals that need no device come back as error codes before any HIP call, and the
ABI version is unchanged (the entry points are additive).  Needs the built library, not a GPU."""
import ctypes as C
import re

from test_abi_layout_cpu import HEADER, _c_layout
from test_mm_infer_group_abi_cpu import _weights

NEW = ["mmf_xfusion_group_workspace_bytes", "mmf_xfusion_group_forward", "mmf_xfusion_group_backward"]


def test_xfusion_grads_match_the_c_header(tmp_path):
    from multimodalfusion_amd import _lib
    m = _lib.XFusionGrads
    got = _c_layout(tmp_path, {"mmf_xfusion_grads": [n for n, _ in m._fields_]})
    assert got[("mmf_xfusion_grads", "sizeof")] == C.sizeof(m)
    for n, _ in m._fields_:
        assert got[("mmf_xfusion_grads", n)] == getattr(m, n).offset, n
    # mmf_xfusion_weights' order: the gradient of a weight sits where the weight sits among the pointers
    wnames = [n for n, t in _lib.XFusionWeights._fields_ if t is not C.c_int32]
    assert [n for n, _ in m._fields_] == ["d" + n for n in wnames]


def test_new_symbols_are_bound_with_the_headers_arity_and_the_abi_version_is_unchanged():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    assert _lib.ABI_VERSION == 12 and l.mmf_abi_version() == 12
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(l, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name


def test_header_cites_the_reference_lines_replaced():
    text = open(HEADER).read()
    at = text.index("Grouped training step of the tensor fusion")
    block = text[at:text.index("typedef struct mmf_xfusion_grads")]
    assert "models/model_modules.py:156-178" in block and "models/model_mm_attention_mil.py:182-188" in block


def test_workspace_query():
    from multimodalfusion_amd import _lib
    q = _lib.lib().mmf_xfusion_group_workspace_bytes          # (m, dim, sdim, mmhid1, mmhid2, nhid, G)
    for m in (2, 3):
        for G in (1, 2, 9, 64):
            gate, bits, E = G * m * 16, G * ((17 ** m + 63) // 64 * 2), 17 ** m
            # o, h, z, gm, dpo, dz, dph; the keep bits; d of the product; dMM
            assert q(m, 256, 16, 512, 512, 256, G) >= 4 * (7 * gate + bits + G * E + G * 512), (m, G)
    assert q(3, 256, 16, 512, 512, 256, 1) < q(3, 256, 16, 512, 512, 256, 64)
    ok = dict(m=3, dim=256, sdim=16, mmhid1=512, mmhid2=512, nhid=256, G=8)
    call = lambda **kw: q(*[dict(ok, **kw)[k] for k in ("m", "dim", "sdim", "mmhid1", "mmhid2", "nhid", "G")])
    assert call() > 0
    assert call(m=1) == 0 and call(m=4) == 0                                   # m outside 2..3
    assert call(G=0) == 0 and call(G=65) == 0 and call(G=-1) == 0
    assert call(sdim=8) == 0 and call(sdim=17) == 0                            # the scale width the kernels take is 16
    assert call(dim=0) == 0 and call(dim=254) == 0                             # dim % 4
    assert call(mmhid1=0) == 0 and call(mmhid1=510) == 0 and call(mmhid1=1024) == 0     # % 4; 1024 + 3 * 256 > 1536
    assert call(mmhid2=0) == 0 and call(mmhid2=1537) == 0 and call(nhid=0) == 0 and call(nhid=1537) == 0


def _grads(fake, **kw):
    from multimodalfusion_amd import _lib
    g = _lib.XFusionGrads(**{n: fake for n in ("dWe1", "dbe1", "dWe2", "dbe2", "dWc0", "dbc0")})
    for n in ("dWh", "dbh", "dWz", "dbz", "dWo", "dbo"):
        for i in range(3):
            getattr(g, n)[i] = fake
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_refusals_that_need_no_device():
    """Null pointers, shapes, probabilities, alignment and the workspace size come back as error codes before any HIP call
    (the fake pointers are never dereferenced)."""
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    ARG, SHAPE, ALIGN, WORKSPACE = -1, -2, -3, -4
    fake = 4096
    big = 1 << 26

    def fwd(w=None, x2=fake, G=4, p=0.25, pc=0.25, base=fake, ws=fake, nb=big, MM=fake, hid=fake):
        w = _weights(fake) if w is None else w
        return l.mmf_xfusion_group_forward(C.byref(w), x2, G, p, pc, base, None, ws, nb, MM, hid, None)

    def bwd(w=None, x2=fake, G=4, p=0.25, pc=0.25, base=fake, MM=fake, hid=fake, dhid=fake, ldd=256, ws=fake, nb=big,
            dx2=fake, g=None, acc=0):
        w = _weights(fake) if w is None else w
        g = _grads(fake) if g is None else g
        return l.mmf_xfusion_group_backward(C.byref(w), x2, G, p, pc, base, None, MM, hid, dhid, ldd, ws, nb, dx2,
                                            C.byref(g), acc, None)

    assert l.mmf_xfusion_group_forward(None, fake, 4, 0.0, 0.0, fake, None, fake, big, fake, fake, None) == ARG
    for call in (fwd, bwd):
        assert call(x2=None) == ARG and call(base=None) == ARG and call(ws=None) == ARG
        assert call(MM=None) == ARG and call(hid=None) == ARG
        assert call(p=-0.1) == ARG and call(p=1.0) == ARG and call(pc=1.5) == ARG and call(p=float("nan")) == ARG
        assert call(w=_weights(fake, m=1)) == SHAPE and call(w=_weights(fake, m=4)) == SHAPE
        assert call(w=_weights(fake, dim=254)) == SHAPE and call(w=_weights(fake, sdim=8)) == SHAPE
        assert call(w=_weights(fake, mmhid1=510)) == SHAPE and call(w=_weights(fake, mmhid1=1024)) == SHAPE
        assert call(w=_weights(fake, mmhid2=1537)) == SHAPE and call(w=_weights(fake, nhid=0)) == SHAPE
        assert call(G=0) == SHAPE and call(G=65) == SHAPE
        assert call(w=_weights(fake, We1=None)) == ARG and call(w=_weights(fake, bc0=None)) == ARG
        w = _weights(fake)
        w.Wz[1] = None
        assert call(w=w) == ARG
        w = _weights(fake)
        w.Wh[2] = fake + 4
        assert call(w=w) == ALIGN
        assert call(x2=fake + 8) == ALIGN and call(ws=fake + 4) == ALIGN
        assert call(nb=4096) == WORKSPACE
    assert bwd(dhid=None) == ARG and bwd(dx2=None) == ARG and bwd(ldd=255) == SHAPE
    assert bwd(g=_grads(fake, dWe1=None)) == ARG and bwd(g=_grads(fake, dbc0=None)) == ARG
    g = _grads(fake)
    g.dWo[0] = None
    assert bwd(g=g) == ARG
    # the third modality's pointers are not read at m = 2
    w2 = _weights(fake, m=2)
    for n in ("Wh", "bh", "Wz", "bz", "Wo", "bo"):
        getattr(w2, n)[2] = None
    assert fwd(w=w2, nb=16) == WORKSPACE
