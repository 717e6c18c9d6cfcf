"""CPU checks of the integrated-gradients entry points in the C ABI (include/mmf_amil.h: mmf_ig_desc,
mmf_amil_ig_workspace_bytes, mmf_amil_ig): the new struct is laid out in ctypes as the header compiled as C lays it out,
the prototypes have the arity their bindings declare, every refusal that needs no device comes back as an error code before
any HIP call, the workspace does not shrink as window_steps grows, the ABI version is unchanged (the entry points are
additive), and the host quadrature tables are the rules they are named after.  Needs the built library, not a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

from test_abi_layout_cpu import HEADER, _c_layout

NEW = ["mmf_amil_ig_workspace_bytes", "mmf_amil_ig"]
ARG, SHAPE, ALIGN, WORKSPACE = -1, -2, -3, -4
FAKE = 4096          # a 16-byte aligned address that is never read


def test_ig_desc_matches_the_c_header(tmp_path):
    from multimodalfusion_amd import _lib
    m = _lib.IgDesc
    got = _c_layout(tmp_path, {"mmf_ig_desc": [n for n, _ in m._fields_]})
    assert got[("mmf_ig_desc", "sizeof")] == C.sizeof(m)
    for n, _ in m._fields_:
        assert got[("mmf_ig_desc", n)] == getattr(m, n).offset, n


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


def _desc(**kw):
    from multimodalfusion_amd import _lib
    d = dict(N=300, L=1024, H=256, D=256, gated=1, W1=FAKE, b1=FAKE, Wa=FAKE, ba=FAKE, Wb=FAKE, bb=FAKE, Wc=FAKE, bc=FAKE,
             p_h=0.0, p_att=0.0, seed=0, gemm=0)
    d.update(kw)
    return _lib.AmilDesc(**d)


def _ig(n=20, keep=None, **kw):
    from multimodalfusion_amd import _lib
    a = (C.c_float * 64)(*([0.5] * 64))
    w = (C.c_float * 64)(*([1.0 / 64] * 64))
    if keep is not None:
        keep.extend([a, w])
    d = dict(n_steps=n, alpha=a, weight=w, window_steps=0, row_sum=FAKE, row_abs=FAKE, attr=None, risk_x=FAKE,
             risk_base=FAKE, step_risk=FAKE)
    d.update(kw)
    return _lib.IgDesc(**d)


def _head(**kw):
    from multimodalfusion_amd import _lib
    d = dict(Wk=FAKE, bk=FAKE, K=4)
    d.update(kw)
    return _lib.SurvHead(**d)


def _call(desc=None, ig=None, head=None, x=FAKE, ws=FAKE, nbytes=1 << 40):
    from multimodalfusion_amd import _lib
    keep = []
    desc = _desc() if desc is None else desc
    ig = _ig(keep=keep) if ig is None else ig
    head = _head() if head is None else head
    return _lib.lib().mmf_amil_ig(C.byref(desc), x, ws, nbytes, C.byref(head), C.byref(ig), None)


def test_refusals_that_need_no_device():
    """Every refusal of the header comes back before any launch: the fake pointers are never dereferenced, and the one
    call that passes every check but the workspace size (the last) shows that the others were refused for their reason."""
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    keep = []
    assert _call(nbytes=16) == WORKSPACE                            # everything else in order
    assert l.mmf_amil_ig(None, FAKE, FAKE, 1 << 40, C.byref(_head()), C.byref(_ig(keep=keep)), None) == ARG
    assert l.mmf_amil_ig(C.byref(_desc()), FAKE, FAKE, 1 << 40, None, C.byref(_ig(keep=keep)), None) == ARG
    assert l.mmf_amil_ig(C.byref(_desc()), FAKE, FAKE, 1 << 40, C.byref(_head()), None, None) == ARG
    # eval mode only, exact-fp32 GEMMs only
    assert _call(desc=_desc(p_h=0.25)) == ARG and _call(desc=_desc(p_att=0.25)) == ARG
    assert _call(desc=_desc(gemm=1)) == ARG
    # the step count and the quadrature tables
    for n in (0, -1, 65):
        assert _call(ig=_ig(n, keep=keep)) == ARG, n
    assert _call(ig=_ig(1, keep=keep), nbytes=16) == WORKSPACE and _call(ig=_ig(64, keep=keep), nbytes=16) == WORKSPACE
    assert _call(ig=_ig(keep=keep, alpha=None)) == ARG and _call(ig=_ig(keep=keep, weight=None)) == ARG
    assert _call(ig=_ig(keep=keep, window_steps=-1)) == ARG
    # outputs: attr alone is optional
    for name in ("row_sum", "row_abs", "risk_x", "risk_base", "step_risk"):
        assert _call(ig=_ig(keep=keep, **{name: None})) == ARG, name
    assert _call(ig=_ig(keep=keep, attr=FAKE), nbytes=16) == WORKSPACE
    assert _call(ig=_ig(keep=keep, attr=FAKE + 4)) == ALIGN
    # the head: the stock hazard head, K <= 32; its outputs are optional
    assert _call(head=_head(Wk=None)) == ARG and _call(head=_head(bk=None)) == ARG
    assert _call(head=_head(K=0)) == SHAPE and _call(head=_head(K=33)) == SHAPE
    assert _call(head=_head(K=32), nbytes=16) == WORKSPACE
    # shape, alignment and workspace as the one-bag entry points
    assert _call(desc=_desc(N=0)) == SHAPE and _call(desc=_desc(L=1000)) == SHAPE
    assert _call(desc=_desc(H=128)) == SHAPE and _call(desc=_desc(D=100)) == SHAPE
    assert _call(desc=_desc(W1=None)) == ARG and _call(desc=_desc(Wb=None)) == ARG
    assert _call(desc=_desc(Wb=None, bb=None, gated=0), nbytes=16) == WORKSPACE
    assert _call(desc=_desc(N=1 << 20)) == SHAPE                    # a [N x L] bag of 4 GiB
    assert _call(x=None) == ARG and _call(ws=None) == ARG
    assert _call(x=FAKE + 4) == ALIGN and _call(ws=FAKE + 8) == ALIGN and _call(desc=_desc(W1=FAKE + 4)) == ALIGN
    need = l.mmf_amil_ig_workspace_bytes(300, 1024, 256, 256, 1, 20, 0)
    assert need > 0 and _call(nbytes=need - 1) == WORKSPACE


def test_workspace_query():
    from multimodalfusion_amd import _lib
    q = _lib.lib().mmf_amil_ig_workspace_bytes
    for gated, H, D in ((1, 256, 256), (0, 512, 384)):
        for N in (1, 300, 4096, 50000):
            prev = 0
            for ws in range(1, 23):                                 # monotone in window_steps, up to the clamp
                b = q(N, 1024, H, D, gated, 20, ws)
                assert b >= prev > 0 or prev == 0 and b > 0, (N, ws)
                prev = b
            assert q(N, 1024, H, D, gated, 20, 64) == prev          # clamped: no more than the call's 22 steps
            assert 0 < q(N, 1024, H, D, gated, 20, 0) <= prev
            # at least U, the folded gradient and one step's h, a, du
            assert q(N, 1024, H, D, gated, 20, 1) >= 4 * N * (4 * H + D)
    assert q(300, 1024, 256, 256, 1, 0, 0) == 0 and q(300, 1024, 256, 256, 1, 65, 0) == 0
    assert q(300, 1024, 256, 256, 1, 20, -1) == 0 and q(0, 1024, 256, 256, 1, 20, 0) == 0
    assert q(1 << 22, 1024, 256, 256, 1, 20, 0) == 0                # one step is more rows than a window takes
    # a 50k bag: the row limit (2^31 bytes of a [rows x 2 D] operand) admits 20 steps of the small head in one window
    assert q(50000, 1024, 256, 256, 1, 20, 20) == q(50000, 1024, 256, 256, 1, 20, 22)
    assert q(50000, 1024, 256, 256, 1, 20, 19) < q(50000, 1024, 256, 256, 1, 20, 20)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 20, 50, 64])
def test_quadrature_tables(n):
    from multimodalfusion_amd import ops
    t, w = np.polynomial.legendre.leggauss(n)
    a, b = ops.ig_quadrature("gausslegendre", n)
    assert a.dtype == np.float64 and b.dtype == np.float64
    np.testing.assert_array_equal(a, 0.5 * (t + 1.0))
    np.testing.assert_array_equal(b, 0.5 * w)
    a, b = ops.ig_quadrature("riemann_middle", n)
    np.testing.assert_allclose(a, (2.0 * np.arange(n) + 1.0) / (2.0 * n), rtol=0, atol=1e-15)
    np.testing.assert_allclose(b, np.full(n, 1.0 / n), rtol=0, atol=1e-15)
    if n >= 2:
        a, b = ops.ig_quadrature("riemann_trapezoid", n)
        np.testing.assert_allclose(a, np.linspace(0.0, 1.0, n), rtol=0, atol=1e-15)
        h = 1.0 / (n - 1)
        np.testing.assert_allclose(b, [h / 2] + [h] * (n - 2) + [h / 2], rtol=0, atol=1e-15)
    for method in ops.IG_METHODS:
        if method == "riemann_trapezoid" and n < 2:
            continue
        a, b = ops.ig_quadrature(method, n)
        assert abs(b.sum() - 1.0) <= 1e-14 and (a >= 0).all() and (a <= 1).all() and (np.diff(a) > 0).all(), method
        # the rule integrates a line exactly, the Gauss rule every polynomial up to degree 2 n - 1
        assert abs((b * a).sum() - 0.5) <= 1e-14, method
    a, b = ops.ig_quadrature("gausslegendre", n)
    assert abs((b * a ** (2 * n - 1)).sum() - 1.0 / (2 * n)) <= 1e-13


def test_python_surface_refuses_before_the_library_is_called():
    """Train mode, a bf16 bag and a hooked module are refused on the host: no device is needed to see it."""
    import torch
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    model = MIL_Attention_fc_surv_path(gate_path=True, model_size_wsi="small", dropout=False, n_classes=4)
    x = torch.zeros(4, 1024)
    model.train()
    with pytest.raises(RuntimeError):
        model.integrated_gradients(x)
    model.eval()
    with pytest.raises(NotImplementedError):
        model.integrated_gradients(x.to(torch.bfloat16))
    with pytest.raises(NotImplementedError):
        ops.amil_integrated_gradients(x.to(torch.bfloat16), (None,) * 8, None, None, True, [0.5], [1.0])
    h = model.attention_net_WSI[0].register_forward_hook(lambda *a: None)
    try:
        with pytest.raises(NotImplementedError):
            model.integrated_gradients(x)
    finally:
        h.remove()
    wide = MIL_Attention_fc_surv_path(gate_path=True, model_size_wsi="small", dropout=False, n_classes=33).eval()
    with pytest.raises(NotImplementedError):
        wide.integrated_gradients(x)                 # a hazard head of more than 32 classes is not the stock head


def test_quadrature_refusals():
    from multimodalfusion_amd import ops
    for bad in (0, 65, -3):
        with pytest.raises(ValueError):
            ops.ig_quadrature("gausslegendre", bad)
    with pytest.raises(ValueError):
        ops.ig_quadrature("riemann_trapezoid", 1)
    with pytest.raises(ValueError):
        ops.ig_quadrature("riemann_left", 20)
