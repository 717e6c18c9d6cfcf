"""GPU: integrated-gradients patch attribution of the pathology head in one call (include/mmf_amil.h: mmf_amil_ig;
ops.amil_integrated_gradients, model.integrated_gradients, infer.attribute_patches) against the float64 oracle of
tests/ig_cases.py -- integrated gradients by the definition, one autograd pass per node over oracle.torch_port.path_forward --
with that module's bars and kink allowance; the L = 1024 heads, loose against float64 by construction, also against the
autograd route on the GPU (infer.integrated_gradients_autograd) at the tight bar; and the structure of the call:
determinism, windows, the launch list, poisoned memory, the optional N x L output."""
import ctypes as C

import numpy as np
import pytest
import torch

import ig_cases as ic
from test_gpu_path import DEV, _load

pytestmark = pytest.mark.gpu

PRE = "attention_net_WSI"


def _operands(name):
    c = ic.BY_NAME[name]
    sd, x = ic.inputs(name)
    t = lambda k: torch.as_tensor(sd[k]).to(DEV)
    if c.gated:
        names = [".0", ".3.attention_a.0", ".3.attention_b.0", ".3.attention_c"]
    else:
        names = [".0", ".3.module.0", None, ".3.module.2"]
    stack = []
    for n in names:
        stack += [None, None] if n is None else [t(PRE + n + ".weight"), t(PRE + n + ".bias")]
    return c, torch.as_tensor(x).to(DEV), tuple(stack), t("classifier.weight"), t("classifier.bias")


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def _run(name, want_attr=False, window_steps=0, n_steps=None):
    from multimodalfusion_amd import ops
    c, x, stack, Wk, bk = _operands(name)
    a, w = ops.ig_quadrature(c.method, c.n_steps if n_steps is None else n_steps)
    out = ops.amil_integrated_gradients(x, stack, Wk, bk, c.gated, a, w, want_attr=want_attr, window_steps=window_steps)
    torch.cuda.synchronize()
    rs, ra, attr, risk, base, steps = map(_np, out)
    return dict(row_sum=rs, row_abs=ra, attr=attr, risk=float(risk[0]), risk_base=float(base[0]), step_risk=steps)


def _worst(got, ref, bar):
    """(the largest error over its bar, where) -- printed before it is asserted on"""
    r = np.abs(got - ref) / bar
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), k, float(np.abs(got - ref).max())


def _check(res, o, tag):
    for key, ref, bar in (("row_sum", o.row_sum, o.bar_rows["row_sum"]), ("row_abs", o.row_abs, o.bar_rows["row_abs"])):
        ratio, k, err = _worst(res[key], ref, bar)
        print(f"{tag} {key}: max err {err:.3e}, worst err / bar {ratio:.3f} at row {k}")
        assert ratio <= 1.0, (tag, key, k)
    if res["attr"] is not None:
        ratio, k, err = _worst(res["attr"], o.attr, o.bar_attr)
        print(f"{tag} attr: max err {err:.3e} (max |attr| {np.abs(o.attr).max():.3e}), worst err / bar {ratio:.3f}")
        assert ratio <= 1.0, (tag, "attr", divmod(k, o.attr.shape[1]))
    total = float(res["row_sum"].sum())
    print(f"{tag} total {total:.6e} oracle {o.total:.6e} bar {o.bar_total:.3e}; risk {res['risk']:.6f} / {o.risk:.6f}")
    assert abs(total - o.total) <= o.bar_total, tag
    assert abs(res["risk"] - o.risk) <= 1e-4 and abs(res["risk_base"] - o.risk_base) <= 1e-4, tag
    np.testing.assert_allclose(res["step_risk"], o.step_risk, rtol=0, atol=1e-4, err_msg=tag)
    delta = total - (res["risk"] - res["risk_base"])
    assert abs(delta - o.delta) <= o.bar_total, (tag, delta, o.delta)


@pytest.mark.parametrize("name", [c.name for c in ic.CASES])
def test_case_matches_the_oracle_with_and_without_the_full_attribution(name):
    o = ic.oracle(name)
    full, rows = _run(name, want_attr=True), _run(name, want_attr=False)
    _check(full, o, name)
    # attr == NULL only drops the store: the sums are the same additions
    for key in ("row_sum", "row_abs", "step_risk"):
        np.testing.assert_array_equal(full[key], rows[key], err_msg=key)
    assert rows["attr"] is None and full["risk"] == rows["risk"] and full["risk_base"] == rows["risk_base"]
    np.testing.assert_allclose(full["attr"].sum(1), full["row_sum"], rtol=0, atol=32 * 2.0 ** -24 * np.abs(full["attr"]).sum(1).max())
    assert (full["row_abs"] >= np.abs(full["row_sum"]) * (1 - 1e-6)).all()


def _model(name):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    c = ic.BY_NAME[name]
    sd, x = ic.inputs(name)
    m = MIL_Attention_fc_surv_path(gate_path=c.gated, model_size_wsi=c.size, dropout=False, n_classes=c.K)
    return c, _load(m, sd).eval(), torch.as_tensor(x).to(DEV)


@pytest.mark.parametrize("name", [c.name for c in ic.WIDE_CASES])
def test_shipped_heads_match_the_oracle_and_the_autograd_route(name):
    from multimodalfusion_amd import infer, ops
    c, model, x = _model(name)
    o = ic.oracle(name)
    out = model.integrated_gradients(x, n_steps=c.n_steps, method=c.method, return_full=True)
    torch.cuda.synchronize()
    res = dict(row_sum=_np(out.patch_attr), row_abs=_np(out.patch_abs), attr=_np(out.attr), risk=float(out.risk),
               risk_base=float(out.risk_baseline), step_risk=_np(out.step_risk))
    _check(res, o, name)
    assert abs(float(out.total) - res["row_sum"].sum()) <= 1e-5 * o.total_abs
    assert abs(float(out.delta) - (float(out.total) - (res["risk"] - res["risk_base"]))) <= 1e-6
    # the same fp32 inputs through n_steps autograd passes on the GPU: the two differ by a few ulp in the pre-activation,
    # so the tight bar holds with no allowance -- but where the oracle shows a unit on the kink, by that one unit's term
    a, w = ops.ig_quadrature(c.method, c.n_steps)
    ps, pa, attr, risk, base, steps = infer.integrated_gradients_autograd(model, x, a.astype(np.float32), w.astype(np.float32))
    torch.cuda.synchronize()
    ps, pa, attr, steps = map(_np, (ps, pa, attr, steps))
    for key, got, ref, bar in (("attr", res["attr"], attr, 1e-4 * np.abs(attr).max() + o.allow_max),
                               ("row_sum", res["row_sum"], ps, 1e-4 * np.abs(ps).max() + o.allow_rowmax),
                               ("row_abs", res["row_abs"], pa, 1e-4 * np.abs(pa).max() + o.allow_rowmax)):
        ratio, k, err = _worst(got, ref, bar)
        plain = np.abs(got - ref).max() / (1e-4 * np.abs(ref).max())
        print(f"{name} vs autograd {key}: max err {err:.3e}, err / bar {ratio:.3f}, err / tight bar {plain:.3f}")
        assert ratio <= 1.0, (name, key, k)
    assert abs(res["risk"] - float(risk)) <= 1e-5 and abs(res["risk_base"] - float(base)) <= 1e-5
    np.testing.assert_allclose(res["step_risk"], steps, rtol=0, atol=1e-5)


def test_two_calls_agree_bit_for_bit():
    for name, ws in (("n300", 0), ("n33", 3), ("small_gated_n300", 0)):
        a, b = _run(name, True, ws), _run(name, True, ws)
        for key in ("row_sum", "row_abs", "attr", "step_risk"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{name} {key}")
        assert a["risk"] == b["risk"] and a["risk_base"] == b["risk_base"]


def test_windows_of_one_three_and_all_steps_agree():
    """20 nodes + the two riders in windows of 1 (22 windows), 3 (seven and a ragged one of 1) and the library's choice (one
    window): each within the oracle's bar, and step_risk the same array -- node k's risk at place k, whatever window ran it
    (to fp32 rounding: the pooling groups of a window depend on its rows)."""
    name = "n33"
    o = ic.oracle(name)
    runs = {ws: _run(name, True, ws) for ws in (1, 3, 0)}
    for ws, r in runs.items():
        _check(r, o, f"{name} window_steps={ws}")
    for ws in (1, 3):
        np.testing.assert_allclose(runs[ws]["step_risk"], runs[0]["step_risk"], rtol=0, atol=1e-5)
        assert abs(runs[ws]["risk"] - runs[0]["risk"]) <= 1e-5 and abs(runs[ws]["risk_base"] - runs[0]["risk_base"]) <= 1e-5
        d = np.abs(runs[ws]["attr"] - runs[0]["attr"]).max()
        print(f"window_steps {ws} vs 0: max |d attr| {d:.3e} of max {np.abs(o.attr).max():.3e}")
        assert (np.abs(runs[ws]["attr"] - runs[0]["attr"]) <= 2 * o.bar_attr).all()


def _traced(name, n_steps):
    from multimodalfusion_amd import _lib
    t = _lib.KernelTrace()
    try:
        with t:
            _run(name, False, 0, n_steps)
        return t.dump()
    finally:
        t.close()


def test_launch_list():
    """The projection and the attribution GEMM once per call, no weight-gradient launch; one window's launch count does not
    depend on the number of nodes in it."""
    k = _traced("n300", None)
    print(sorted((n, c) for n, (c, _) in k.items()))
    assert k["linear_nt_kernel"][0] == 1 and k["gemm_nn_attr_kernel"][0] == 1 and k["ig_rows_kernel"][0] == 1
    assert not any("tn_kernel" in n or "reduce" in n or n == "gemm_nn_kernel" for n in k), sorted(k)
    for n in ("ig_expand_kernel", "gate_fwd_kernel", "group_pool_partial_kernel", "group_merge_kernel", "ig_head_kernel",
              "group_bwd_prep_kernel", "bwd_dh_kernel", "ig_fold_kernel"):
        assert k[n][0] == 1, (n, k.get(n))                 # 22 steps of 300 rows: one window
    from multimodalfusion_amd import ops
    c, x, stack, Wk, bk = _operands("n300")
    x64 = x[:64].contiguous()
    counts = []
    for n_steps in (4, 20):
        from multimodalfusion_amd import _lib
        t = _lib.KernelTrace()
        try:
            with t:
                ops.amil_integrated_gradients(x64, stack, Wk, bk, c.gated, *ops.ig_quadrature("gausslegendre", n_steps))
                torch.cuda.synchronize()
            counts.append(sum(v[0] for v in t.dump().values()))
        finally:
            t.close()
    assert counts[0] == counts[1] > 0, counts


def _raw(name, fill, want_attr):
    """The raw call on a workspace and outputs filled with `fill` first."""
    from multimodalfusion_amd import _lib, ops
    c, x, stack, Wk, bk = _operands(name)
    N, L = x.shape
    stack, (Wk, bk), H, D = ops._stack_operands(stack, L, (Wk, bk), "bag", fused_head=True)
    a, w = (v.astype(np.float32) for v in ops.ig_quadrature(c.method, c.n_steps))
    d = ops._amil_desc(stack, N, L, H, D, c.gated, 0.0, 0.0, 0, None)
    l = _lib.lib()
    nbytes = l.mmf_amil_ig_workspace_bytes(N, L, H, D, d.gated, c.n_steps, 0)
    ws = torch.full((nbytes // 4,), fill, dtype=torch.float32, device=DEV)
    outs = torch.full((2 * N + 2 + c.n_steps + 2,), fill, dtype=torch.float32, device=DEV)
    attr = torch.full((N, L), fill, dtype=torch.float32, device=DEV)
    rs, ra, risks = outs[:N], outs[N:2 * N], outs[2 * N:]
    sh = _lib.SurvHead(Wk=_lib.ptr(Wk), bk=_lib.ptr(bk), K=Wk.shape[0])
    fp = C.POINTER(C.c_float)
    ig = _lib.IgDesc(n_steps=c.n_steps, alpha=a.ctypes.data_as(fp), weight=w.ctypes.data_as(fp), window_steps=0,
                     row_sum=rs.data_ptr(), row_abs=ra.data_ptr(), attr=attr.data_ptr() if want_attr else None,
                     risk_x=risks[0:1].data_ptr(), risk_base=risks[1:2].data_ptr(), step_risk=risks[2:].data_ptr())
    _lib.check(l.mmf_amil_ig(C.byref(d), _lib.ptr(x), ws.data_ptr(), nbytes, C.byref(sh), C.byref(ig), _lib.stream_ptr()),
               "mmf_amil_ig")
    torch.cuda.synchronize()
    return _np(rs), _np(ra), _np(attr), _np(risks[:2 + c.n_steps]), _np(risks[2 + c.n_steps:])


@pytest.mark.parametrize("name", ["n33", "n300", "n33_big_ungated_k1"])
def test_poisoned_workspace_and_outputs_are_overwritten(name):
    """NaN canaries in the workspace and in every output: the outputs come back finite, whole, and bit for bit what a
    zero-filled workspace gives -- nothing is read before the call writes it -- and the words behind step_risk stay."""
    nan = _raw(name, float("nan"), True)
    zero = _raw(name, 0.0, True)
    for a, b, what in zip(nan[:4], zero[:4], ("row_sum", "row_abs", "attr", "risks")):
        assert np.isfinite(a).all(), what
        np.testing.assert_array_equal(a, b, err_msg=what)
    assert np.isnan(nan[4]).all() and (zero[4] == 0).all()
    o = ic.oracle(name)
    assert (np.abs(nan[2] - o.attr) <= o.bar_attr).all()


def test_without_the_full_attribution_no_n_by_l_buffer_is_touched():
    rs, ra, canary, risks, _ = _raw("n300", float("nan"), False)
    assert np.isnan(canary).all() and np.isfinite(rs).all() and np.isfinite(ra).all() and np.isfinite(risks).all()


def test_fifty_nodes_leave_a_smaller_completeness_gap_than_the_oracle_at_twenty():
    name = "small_gated_n300"
    c, model, x = _model(name)
    out = model.integrated_gradients(x, n_steps=50)
    torch.cuda.synchronize()
    o20 = ic.oracle(name)
    print(f"|delta| at 50 nodes {abs(float(out.delta)):.3e}; the oracle's at 20 nodes {abs(o20.delta):.3e}")
    assert out.step_risk.numel() == 50 and out.attr is None
    assert abs(float(out.delta)) < abs(o20.delta)


def test_surface_refusals():
    from multimodalfusion_amd import infer
    c, model, x = _model("big_ungated_n33_k1")
    model.train()
    with pytest.raises(RuntimeError):
        model.integrated_gradients(x)
    model.eval()
    with pytest.raises(NotImplementedError):
        model.integrated_gradients(x.to(torch.bfloat16))
    h = model.classifier.register_forward_hook(lambda *a: None)
    try:
        with pytest.raises(NotImplementedError):
            model.integrated_gradients(x)
    finally:
        h.remove()
    with pytest.raises(ValueError):
        model.integrated_gradients(x, method="riemann_left")
    with pytest.raises(NotImplementedError):
        infer.attribute_patches(torch.nn.Linear(4, 4), x)
    model.train()
    out = infer.attribute_patches(model, x.cpu(), n_steps=4)      # eval mode for the call, restored behind it
    assert model.training and out.patch_abs.shape == (33,)


def test_attribute_patches_returns_the_oracles_top_five():
    from multimodalfusion_amd import infer
    name = "small_gated_n300"
    c, model, x = _model(name)
    o = ic.oracle(name)
    out, top = infer.attribute_patches(model, x, n_steps=c.n_steps, top_k=5)
    torch.cuda.synchronize()
    top = top.cpu().numpy().tolist()
    order = np.argsort(-o.row_abs)
    bar = o.bar_rows["row_abs"]
    assert len(top) == 5 and len(set(top)) == 5
    # a patch belongs to the top five for certain when it beats the sixth by more than both bars, and stays out when the
    # fifth beats it so; ranks are compared where neighbours are that far apart
    fifth, sixth = order[4], order[5]
    for i in order[:5]:
        if o.row_abs[i] - o.row_abs[sixth] > bar[i] + bar[sixth]:
            assert i in top, i
    for i in top:
        assert o.row_abs[i] + bar[i] >= o.row_abs[fifth] - bar[fifth], i
    for r in range(4):
        i, j = order[r], order[r + 1]
        if o.row_abs[i] - o.row_abs[j] > bar[i] + bar[j] and i in top and j in top:
            assert top.index(i) < top.index(j), (i, j)
    got = _np(out.patch_abs)
    assert (np.abs(got - o.row_abs) <= bar).all()
