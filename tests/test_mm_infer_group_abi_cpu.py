"""CPU checks of the multimodal head's grouped forward-only pass in the C ABI (include/mmf_amil.h: mmf_xfusion_weights,
mmf_xfusion_group_infer_workspace_bytes, mmf_xfusion_infer_group, mmf_surv_head_infer_group): the new struct is laid out
in ctypes as the header compiled as C lays it out, every new prototype has the arity its binding declares, the workspace
query answers 0 outside its limits, refusals that need no device come back as error codes before any HIP call, and the
ABI version is unchanged (the entry points are additive).  Needs the built library, not a GPU."""
import ctypes as C
import re

from test_abi_layout_cpu import HEADER, _c_layout

NEW = ["mmf_xfusion_group_infer_workspace_bytes", "mmf_xfusion_infer_group", "mmf_surv_head_infer_group"]


def test_xfusion_weights_match_the_c_header(tmp_path):
    from multimodalfusion_amd import _lib
    m = _lib.XFusionWeights
    got = _c_layout(tmp_path, {"mmf_xfusion_weights": [n for n, _ in m._fields_]})
    assert got[("mmf_xfusion_weights", "sizeof")] == C.sizeof(m)
    for n, _ in m._fields_:
        assert got[("mmf_xfusion_weights", n)] == getattr(m, n).offset, n


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


def test_xfusion_workspace_query():
    from multimodalfusion_amd import _lib
    q = _lib.lib().mmf_xfusion_group_infer_workspace_bytes
    for m in (2, 3):
        for G in (1, 2, 9, 64):
            assert q(m, 16, 512, G) >= 4 * (G * m * 16 + G * 512), (m, G)      # o and encoder1's output
    assert q(3, 16, 512, 1) < q(3, 16, 512, 64)
    assert q(1, 16, 512, 8) == 0 and q(4, 16, 512, 8) == 0                     # m outside 2..3
    assert q(3, 16, 512, 0) == 0 and q(3, 16, 512, 65) == 0 and q(3, 16, 512, -1) == 0
    assert q(3, 8, 512, 8) == 0 and q(3, 17, 512, 8) == 0                      # the scale width the kernels take is 16
    assert q(3, 16, 0, 8) == 0 and q(3, 16, 1537, 8) == 0


def _weights(fake, **kw):
    from multimodalfusion_amd import _lib
    w = _lib.XFusionWeights(m=3, dim=256, sdim=16, mmhid1=512, mmhid2=512, nhid=256, We1=fake, be1=fake, We2=fake,
                            be2=fake, Wc0=fake, bc0=fake)
    for n in ("Wh", "bh", "Wz", "bz", "Wo", "bo"):
        for i in range(3):
            getattr(w, n)[i] = fake
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def test_refusals_that_need_no_device():
    """Null pointers and out-of-range shapes come back as error codes before any HIP call (the fake pointers are never
    dereferenced)."""
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    ARG, SHAPE, ALIGN, WORKSPACE = -1, -2, -3, -4
    fake = 4096
    v = (C.c_void_p * 3)(fake, fake, fake)
    xf = lambda w, G=4, v=v, ws=fake, nb=1 << 20, MM=fake, hid=fake: l.mmf_xfusion_infer_group(
        C.byref(w), v, G, ws, nb, MM, hid, None)
    assert l.mmf_xfusion_infer_group(None, v, 4, fake, 1 << 20, fake, fake, None) == ARG
    assert xf(_weights(fake), v=None) == ARG and xf(_weights(fake), MM=None) == ARG and xf(_weights(fake), hid=None) == ARG
    assert xf(_weights(fake), ws=None) == ARG
    assert xf(_weights(fake, m=1)) == SHAPE and xf(_weights(fake, m=4)) == SHAPE
    assert xf(_weights(fake, dim=254)) == SHAPE                    # dim % 4 != 0
    assert xf(_weights(fake, sdim=8)) == SHAPE
    assert xf(_weights(fake), G=0) == SHAPE and xf(_weights(fake), G=65) == SHAPE
    assert xf(_weights(fake, mmhid1=1024)) == SHAPE                # encoder2's input row 1024 + 3 * 256 > 1536
    assert xf(_weights(fake, We1=None)) == ARG and xf(_weights(fake, Wc0=None)) == ARG
    assert xf(_weights(fake), v=(C.c_void_p * 3)(fake, None, fake)) == ARG
    assert xf(_weights(fake), v=(C.c_void_p * 3)(fake, fake + 4, fake)) == ALIGN
    assert xf(_weights(fake), ws=fake + 8) == ALIGN
    assert xf(_weights(fake), nb=16) == WORKSPACE
    # the head: segments, widths, G, the head struct
    hd, tg = _lib.SurvHead(), _lib.NllTarget()
    segs = (C.c_void_p * 3)(fake, fake, fake)
    wd = lambda *a: (C.c_int32 * len(a))(*a)
    head = lambda segs=segs, widths=wd(256, 256, 256), n=3, G=4, hd=hd, tg=None: l.mmf_surv_head_infer_group(
        segs, widths, n, G, C.byref(hd), tg and C.byref(tg), None)
    assert head(segs=None) == ARG and head(widths=None) == ARG
    assert head(n=0) == SHAPE and head(n=4) == SHAPE and head(G=0) == SHAPE and head(G=65) == SHAPE
    assert head(widths=wd(256, 0, 256)) == SHAPE and head(widths=wd(512, 512, 1)) == SHAPE       # sum width 1025
    assert head(segs=(C.c_void_p * 3)(fake, None, fake)) == ARG
    assert head() == ARG                                           # an empty head struct
    full = _lib.SurvHead(Wk=fake, bk=fake, K=33, logits=fake, hazards=fake, S=fake, Y_hat=fake, risk=fake)
    assert head(hd=full) == SHAPE                                  # K = 33
    full.K = 4
    assert head(hd=full, tg=tg) == ARG                             # a target without labels
