"""GPU: integrated-gradients attribution of the radiology head in one call (include/mmf_amil.h: mmf_radio_ig;
ops.radio_integrated_gradients, MIL_Attention_fc_surv_radio.integrated_gradients, infer.attribute_radiology) against the
float64 oracle of tests/radio_ig_cases.py -- integrated gradients by the definition, one autograd pass per node over
oracle.torch_port.radio_forward -- with that module's bars: tier A with no allowance at all, tier B with the kink allowance,
tier C (the shipped width, loose against float64 by construction) also against the autograd route on the GPU
(infer.radio_integrated_gradients_autograd) at the tight bar; and the structure of the call: determinism, windows, the
launch list, poisoned memory, the optional full attribution, the segment pointers."""
import ctypes as C

import numpy as np
import pytest
import torch

import radio_ig_cases as rc
from test_gpu_path import DEV, _load

pytestmark = pytest.mark.gpu

PRE = rc.PRE
MODS = ["T1", "T2", "T1Gd", "FLAIR"]


def _operands(name):
    c = rc.BY_NAME[name]
    sd, xs, _ = rc.inputs(name)
    t = lambda k: torch.as_tensor(sd[k]).to(DEV)
    if c.gated:
        names = [".0", ".3.attention_a.0", ".3.attention_b.0", ".3.attention_c"]
    else:
        names = [".0", ".3.module.0", None, ".3.module.2"]
    stack = []
    for n in names:
        stack += [None, None] if n is None else [t(PRE + n + ".weight"), t(PRE + n + ".bias")]
    xs = [torch.as_tensor(np.array(x)).to(DEV) for x in xs]
    return c, xs, t("reduce_dim.weight"), t("reduce_dim.bias"), tuple(stack), t("classifier.weight"), t("classifier.bias")


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def _pack(out):
    rs, ra, attr, risk, base, steps = map(_np, out)
    return dict(row_sum=rs, row_abs=ra, attr=attr, risk=float(risk.reshape(-1)[0]), risk_base=float(base.reshape(-1)[0]),
                step_risk=steps)


def _run(name, want_attr=False, window_steps=None, n_steps=None, rows=None):
    from multimodalfusion_amd import ops
    c, xs, Wr, br, stack, Wk, bk = _operands(name)
    if rows is not None:
        xs = [x[:rows].contiguous() for x in xs]
    a, w = ops.ig_quadrature(c.method, c.n_steps if n_steps is None else n_steps)
    out = ops.radio_integrated_gradients(xs, Wr, br, stack, Wk, bk, c.gated, a, w, want_attr=want_attr,
                                         window_steps=c.window_steps if window_steps is None else window_steps)
    torch.cuda.synchronize()
    return _pack(out)


def _worst(got, ref, bar):
    """(the largest error over its bar, where, the largest error) -- printed before it is asserted on"""
    r = np.abs(got - ref) / bar
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), k, float(np.abs(got - ref).max())


def _check(res, o, tag):
    for key, ref, bar in (("row_sum", o.row_sum, o.bar_row_sum), ("row_abs", o.row_abs, o.bar_row_abs)):
        ratio, k, err = _worst(res[key], ref, bar)
        print(f"{tag} {key}: max err {err:.3e}, worst err / bar {ratio:.3f} at {divmod(k, ref.shape[1])}")
        assert ratio <= 1.0, (tag, key, k)
    if res["attr"] is not None:
        ratio, k, err = _worst(res["attr"], o.attr, o.bar_attr)
        print(f"{tag} attr: max err {err:.3e} (max |attr| {np.abs(o.attr).max():.3e}), worst err / bar {ratio:.3f}")
        assert ratio <= 1.0, (tag, "attr", np.unravel_index(k, o.attr.shape))
    mod_abs = res["row_abs"].sum(1)
    ratio, k, err = _worst(mod_abs, o.mod_abs, o.bar_mod_abs)
    print(f"{tag} modality_abs {mod_abs} oracle {o.mod_abs}: worst err / bar {ratio:.3f}")
    assert ratio <= 1.0, (tag, "modality_abs", k)
    total = float(res["row_sum"].sum())
    print(f"{tag} total {total:.6e} oracle {o.total:.6e} bar {o.bar_total:.3e}; risk {res['risk']:.6f} / {o.risk:.6f}")
    assert abs(total - o.total) <= o.bar_total, tag
    assert abs(res["risk"] - o.risk) <= 1e-4 and abs(res["risk_base"] - o.risk_base) <= 1e-4, tag
    np.testing.assert_allclose(res["step_risk"], o.step_risk, rtol=0, atol=1e-4, err_msg=tag)
    delta = total - (res["risk"] - res["risk_base"])
    assert abs(delta - o.delta) <= o.bar_total + 2e-4, (tag, delta, o.delta)      # the total's bar and the two risks'


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_case_matches_the_oracle_with_and_without_the_full_attribution(name):
    c = rc.BY_NAME[name]
    o = rc.oracle(name)
    full, rows = _run(name, want_attr=True), _run(name, want_attr=False)
    assert full["row_sum"].shape == (c.nseg, c.N) and full["attr"].shape == (c.nseg, c.N, c.kseg)
    _check(full, o, name)
    # attr == NULL only drops the store: the sums are the same additions
    for key in ("row_sum", "row_abs", "step_risk"):
        np.testing.assert_array_equal(full[key], rows[key], err_msg=key)
    assert rows["attr"] is None and full["risk"] == rows["risk"] and full["risk_base"] == rows["risk_base"]
    np.testing.assert_allclose(full["attr"].sum(2), full["row_sum"], rtol=0,
                               atol=(c.kseg + 8) * 2.0 ** -24 * np.abs(full["attr"]).sum(2).max())
    assert (full["row_abs"] >= np.abs(full["row_sum"]) * (1 - 1e-6)).all()


def _model(name):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio
    c = rc.BY_NAME[name]
    assert (c.kseg, c.H, c.D) == (1024, 256, 256)            # the radiology head is the small one
    sd, xs, _ = rc.inputs(name)
    m = MIL_Attention_fc_surv_radio(gate_radio=c.gated, dropout=False, n_classes=c.K, modalities=MODS[:c.nseg])
    return c, _load(m, sd).eval(), {k: torch.as_tensor(np.array(x)).to(DEV) for k, x in zip(MODS, xs)}


@pytest.mark.parametrize("name", [c.name for c in rc.TIER_C])
def test_shipped_width_matches_the_oracle_and_the_autograd_route(name):
    from multimodalfusion_amd import infer, ops
    c, model, bags = _model(name)
    o = rc.oracle(name)
    out = model.integrated_gradients(n_steps=c.n_steps, method=c.method, return_full=True, **bags)
    torch.cuda.synchronize()
    res = dict(row_sum=_np(out.inst_attr), row_abs=_np(out.inst_abs), attr=_np(out.attr), risk=float(out.risk),
               risk_base=float(out.risk_baseline), step_risk=_np(out.step_risk))
    _check(res, o, name)
    np.testing.assert_allclose(_np(out.modality_abs), res["row_abs"].sum(1), rtol=1e-5)
    np.testing.assert_allclose(_np(out.modality_attr), res["row_sum"].sum(1), rtol=0, atol=1e-5 * o.total_abs)
    assert abs(float(out.total) - res["row_sum"].sum()) <= 1e-5 * o.total_abs
    assert abs(float(out.total_abs) - res["row_abs"].sum()) <= 1e-5 * o.total_abs
    assert abs(float(out.delta) - (float(out.total) - (res["risk"] - res["risk_base"]))) <= 1e-6
    # the same fp32 inputs through n_steps autograd passes on the GPU: the two differ by a few ulp in the pre-activation,
    # so the tight bar holds with no allowance -- but where the oracle shows a unit on the kink, by that one unit's term
    a, w = ops.ig_quadrature(c.method, c.n_steps)
    ps, pa, attr, risk, base, steps = infer.radio_integrated_gradients_autograd(model, bags, a.astype(np.float32),
                                                                                w.astype(np.float32))
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


@pytest.mark.parametrize("nseg,kseg,N,M", [(2, 32, 32, 17), (3, 96, 96, 65), (4, 1024, 1024, 150), (4, 160, 64, 130)])
def test_concatenated_linear_input_gradient(nseg, kseg, N, M):
    """The autograd yardstick needs d loss / d x_m through reduce_dim (mmf_linear_input_grad): dx_m = gy W[:, m kseg ..]
    against float64, at (N / 2 + 8) 2^-24 sum |gy| |W| -- the chain of one two-product MFMA per k step -- and the weight
    gradients next to it unchanged by asking for it."""
    from multimodalfusion_amd import ops
    from oracle import inputs as gen
    W = torch.as_tensor(gen.normal(3, (N, nseg * kseg), std=0.05)).to(DEV).requires_grad_()
    b = torch.as_tensor(gen.normal(4, (N,), std=0.1)).to(DEV).requires_grad_()
    xs = [torch.as_tensor(gen.bag(5, M, dim=kseg, stream=m)).to(DEV).requires_grad_() for m in range(nseg)]
    gy = torch.as_tensor(gen.normal(6, (M, N))).to(DEV)
    ops.linear_cat(xs, W, b).backward(gy)
    dW = W.grad.clone()
    W.grad = None
    ops.linear_cat([x.detach() for x in xs], W, b).backward(gy)
    torch.cuda.synchronize()
    assert torch.equal(dW, W.grad)
    g64, W64 = _np(gy), _np(W)
    ref = g64 @ W64
    bar = (N // 2 + 8) * 2.0 ** -24 * (np.abs(g64) @ np.abs(W64))
    for m, x in enumerate(xs):
        err = np.abs(_np(x.grad) - ref[:, m * kseg:(m + 1) * kseg])
        print(f"nseg {nseg} kseg {kseg} segment {m}: worst err / bar {(err / bar[:, m * kseg:(m + 1) * kseg]).max():.3f}")
        assert (err <= bar[:, m * kseg:(m + 1) * kseg]).all(), m


def test_two_calls_agree_bit_for_bit():
    for name, ws in (("a_4seg_small_n300", 0), ("a_3seg_two_tiles_n65", 3), ("c_2seg_small_ungated_n33", 0)):
        a, b = _run(name, True, ws), _run(name, True, ws)
        for key in ("row_sum", "row_abs", "attr", "step_risk"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{name} {key}")
        assert a["risk"] == b["risk"] and a["risk_base"] == b["risk_base"]


def test_windows_of_one_three_and_all_steps_agree():
    """20 nodes + the two riders in windows of 1, 3 and the library's choice (one window): each within the oracle's bar, and
    step_risk the same array -- node k's risk at place k, whatever window ran it (to fp32 rounding: the pooling groups of a
    window depend on its rows)."""
    name = "a_3seg_two_tiles_n65"
    o = rc.oracle(name)
    runs = {ws: _run(name, True, ws) for ws in (1, 3, 0)}
    for ws, r in runs.items():
        _check(r, o, f"{name} window_steps={ws}")
    for ws in (1, 3):
        np.testing.assert_allclose(runs[ws]["step_risk"], runs[0]["step_risk"], rtol=0, atol=1e-5)
        assert abs(runs[ws]["risk"] - runs[0]["risk"]) <= 1e-5 and abs(runs[ws]["risk_base"] - runs[0]["risk_base"]) <= 1e-5
        d = np.abs(runs[ws]["attr"] - runs[0]["attr"]).max()
        print(f"window_steps {ws} vs 0: max |d attr| {d:.3e} of max {np.abs(o.attr).max():.3e}")
        assert (np.abs(runs[ws]["attr"] - runs[0]["attr"]) <= 2 * o.bar_attr).all()


def _traced(name, n_steps=None, rows=None, window_steps=0):
    from multimodalfusion_amd import _lib
    t = _lib.KernelTrace()
    try:
        with t:
            _run(name, False, window_steps, n_steps, rows)
        return t.dump()
    finally:
        t.close()


ONCE = {"linear_nt_kernel": 2,                     # reduce_dim and the projection
        "ig_bias_kernel": 1, "gemm_nn_kernel": 1, "gemm_nn_attr_seg_kernel": 1, "ig_rows_seg_kernel": 1}
PER_WINDOW = ("ig_expand_kernel", "group_rows_kernel", "gate_fwd_kernel", "group_pool_partial_kernel", "group_merge_kernel",
              "ig_head_kernel", "group_bwd_prep_kernel", "bwd_dh_kernel", "ig_fold_kernel")


def test_launch_list():
    """reduce_dim, the projection, the bias kernel, the two back-products and the row sums once per call, no weight-gradient
    launch; a window's launch count does not depend on the number of nodes in it."""
    k = _traced("a_4seg_small_n300")
    print(sorted((n, c) for n, (c, _) in k.items()))
    for n, cnt in ONCE.items():
        assert k[n][0] == cnt, (n, k.get(n))
    assert not any("tn_kernel" in n or "reduce" in n or n in ("gemm_nn_attr_kernel", "ig_rows_kernel") for n in k), sorted(k)
    for n in PER_WINDOW:
        assert k[n][0] == 1, (n, k.get(n))                 # 22 steps of 300 rows: one window
    assert sum(c for c, _ in k.values()) == sum(ONCE.values()) + len(PER_WINDOW)
    counts = [sum(v[0] for v in _traced("a_4seg_small_n300", n_steps, 64).values()) for n_steps in (4, 20)]
    assert counts[0] == counts[1] == sum(ONCE.values()) + len(PER_WINDOW), counts
    # three windows: the once-per-call launches stay, the window's repeat
    k = _traced("a_2seg_one_step_windows", window_steps=1)
    for n, cnt in ONCE.items():
        assert k[n][0] == cnt, (n, k.get(n))
    assert k["ig_expand_kernel"][0] == 3 and k["ig_head_kernel"][0] == 3 and k["ig_fold_kernel"][0] == 1


def _raw(name, fill, want_attr, swap=None):
    """The raw call on a workspace and outputs filled with `fill` first, with the head's optional outputs.  swap: two
    modalities exchanged, in the bags and in reduce_dim's column blocks."""
    from multimodalfusion_amd import _lib, ops
    c, xs, Wr, br, stack, Wk, bk = _operands(name)
    if swap:
        i, j = swap
        xs[i], xs[j] = xs[j], xs[i]
        blocks = list(Wr.split(c.kseg, dim=1))
        blocks[i], blocks[j] = blocks[j], blocks[i]
        Wr = torch.cat(blocks, dim=1).contiguous()
    xs, N, nseg, kseg, rd = ops._radio_operands(xs, Wr, br, "pass")
    stack, (Wk, bk), H, D = ops._stack_operands(stack, kseg, (Wk, bk), "bags", fused_head=True)
    a, w = (v.astype(np.float32) for v in ops.ig_quadrature(c.method, c.n_steps))
    d = ops._amil_desc(stack, N, kseg, H, D, c.gated, 0.0, 0.0, 0, None)
    l = _lib.lib()
    nbytes = l.mmf_radio_ig_workspace_bytes(N, nseg, kseg, H, D, d.gated, c.n_steps, c.window_steps)
    ws = torch.full((nbytes // 4,), fill, dtype=torch.float32, device=DEV)
    K, n = c.K, c.n_steps
    outs = torch.full((2 * nseg * N + 2 + n + 3 * K + 1 + 4,), fill, dtype=torch.float32, device=DEV)
    attr = torch.full((nseg, N, kseg), fill, dtype=torch.float32, device=DEV)
    yhat = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    o0 = 2 * nseg * N
    rs, ra, risks = outs[:nseg * N], outs[nseg * N:o0], outs[o0:o0 + 2 + n]
    head = outs[o0 + 2 + n:o0 + 2 + n + 3 * K + 1]
    guard = outs[o0 + 2 + n + 3 * K + 1:]
    sh = _lib.SurvHead(Wk=_lib.ptr(Wk), bk=_lib.ptr(bk), K=K, logits=head[:K].data_ptr(), hazards=head[K:2 * K].data_ptr(),
                       S=head[2 * K:3 * K].data_ptr(), Y_hat=yhat.data_ptr(), risk=head[3 * K:].data_ptr())
    fp = C.POINTER(C.c_float)
    ig = _lib.IgDesc(n_steps=n, alpha=a.ctypes.data_as(fp), weight=w.ctypes.data_as(fp), window_steps=c.window_steps,
                     row_sum=rs.data_ptr(), row_abs=ra.data_ptr(), attr=attr.data_ptr() if want_attr else None,
                     risk_x=risks[0:1].data_ptr(), risk_base=risks[1:2].data_ptr(), step_risk=risks[2:].data_ptr())
    _lib.check(l.mmf_radio_ig(C.byref(d), C.byref(rd), ws.data_ptr(), nbytes, C.byref(sh), C.byref(ig), _lib.stream_ptr()),
               "mmf_radio_ig")
    torch.cuda.synchronize()
    return dict(row_sum=_np(rs).reshape(nseg, N), row_abs=_np(ra).reshape(nseg, N), attr=_np(attr), risks=_np(risks),
                head=_np(head), Y_hat=int(yhat[0]), guard=_np(guard))


@pytest.mark.parametrize("name", ["a_3seg_two_tiles_n65", "a_4seg_small_n300", "a_2seg_h1024_k5_n65", "b_4seg_k128_h1024_n65",
                                  "a_2seg_one_step_windows"])
def test_poisoned_workspace_and_outputs_are_overwritten(name):
    """NaN canaries in the workspace and in every output: the outputs come back finite, whole, and bit for bit what a
    zero-filled workspace gives -- nothing is read before the call writes it -- and the words behind the outputs stay.  The
    head's optional outputs are the oracle's values at alpha = 1."""
    c = rc.BY_NAME[name]
    nan, zero = _raw(name, float("nan"), True), _raw(name, 0.0, True)
    for what in ("row_sum", "row_abs", "attr", "risks", "head"):
        assert np.isfinite(nan[what]).all(), what
        np.testing.assert_array_equal(nan[what], zero[what], err_msg=what)
    assert np.isnan(nan["guard"]).all() and (zero["guard"] == 0).all() and nan["Y_hat"] == zero["Y_hat"]
    o = rc.oracle(name)
    assert (np.abs(nan["attr"] - o.attr) <= o.bar_attr).all()
    K = c.K
    logits, hz, S, risk = nan["head"][:K], nan["head"][K:2 * K], nan["head"][2 * K:3 * K], nan["head"][3 * K]
    np.testing.assert_allclose(logits, o.logits, rtol=0, atol=1e-4)
    np.testing.assert_allclose(hz, o.hazards, rtol=0, atol=1e-4)
    np.testing.assert_allclose(S, o.S, rtol=0, atol=1e-4)
    assert risk == nan["risks"][0] and abs(risk - o.risk) <= 1e-4
    order = np.sort(o.logits)
    if K == 1 or order[-1] - order[-2] > 2e-4:
        assert nan["Y_hat"] == o.Y_hat


def test_head_outputs_at_alpha_one_are_the_models():
    name = "c_4seg_small_gated_n150"
    c, model, bags = _model(name)
    got = _raw(name, float("nan"), False)
    with torch.no_grad():
        hz, S, Y_hat, _ = model(**bags)
    torch.cuda.synchronize()
    K = c.K
    np.testing.assert_allclose(got["head"][K:2 * K], _np(hz).reshape(-1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(got["head"][2 * K:3 * K], _np(S).reshape(-1), rtol=0, atol=1e-5)
    assert abs(got["head"][3 * K] + float(S.sum())) <= 1e-5 and got["Y_hat"] == int(Y_hat.reshape(-1)[0])


def test_without_the_full_attribution_no_full_width_buffer_is_touched():
    r = _raw("a_4seg_small_n300", float("nan"), False)
    assert np.isnan(r["attr"]).all() and np.isnan(r["guard"]).all()
    assert np.isfinite(r["row_sum"]).all() and np.isfinite(r["row_abs"]).all() and np.isfinite(r["risks"]).all()


@pytest.mark.parametrize("name,swap", [("a_3seg_two_tiles_n65", (0, 2)), ("a_4seg_small_n300", (1, 3)),
                                       ("b_3seg_k96_n65", (0, 1))])
def test_swapped_modalities_return_the_swapped_rows(name, swap):
    """Two modalities exchanged in the bags and in reduce_dim's column blocks: the same function of the same numbers, so
    each modality's rows come back at its new place (to the bars: the K order of reduce_dim's sums changes).  A wrong
    segment pointer in the epilogue or the row sums fails here."""
    o = rc.oracle(name)
    plain, swapped = _raw(name, 0.0, True), _raw(name, 0.0, True, swap=swap)
    perm = list(range(rc.BY_NAME[name].nseg))
    perm[swap[0]], perm[swap[1]] = perm[swap[1]], perm[swap[0]]
    for what, bar in (("row_sum", o.bar_row_sum), ("row_abs", o.bar_row_abs), ("attr", o.bar_attr)):
        d = np.abs(swapped[what][perm] - plain[what])
        print(f"{name} swap {swap} {what}: max diff {d.max():.3e}")
        assert (d <= 2 * bar).all(), what
        assert (np.abs(swapped[what][perm] - getattr(o, what)) <= bar).all(), what
    # the modalities differ by more than the bars, so an unswapped result would not pass
    assert np.abs(o.row_abs[swap[0]] - o.row_abs[swap[1]]).max() > 4 * np.max(o.bar_row_abs)


def test_one_modality_is_the_pathology_call():
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio
    from multimodalfusion_amd.models.model_modules import stack_args
    from oracle import inputs as gen
    sd = gen.radio_state_dict(seed=5, gated=True, n_classes=4, dropout=False, n_mod=1, bias_std=0.1)
    model = _load(MIL_Attention_fc_surv_radio(gate_radio=True, dropout=False, n_classes=4, modalities=["T1"]), sd).eval()
    x = torch.as_tensor(gen.bag(6, 33)).to(DEV)
    out = model.integrated_gradients(n_steps=4, method="riemann_middle", return_full=True, T1=x)
    gated, stack, _, _ = stack_args(model.attention_net_radio, False)
    a, w = ops.ig_quadrature("riemann_middle", 4)
    with torch.no_grad():
        rs, ra, attr, risk, base, steps = ops.amil_integrated_gradients(x, stack, model.classifier.weight,
                                                                        model.classifier.bias, gated, a, w, want_attr=True)
    torch.cuda.synchronize()
    assert out.inst_attr.shape == (1, 33) and out.attr.shape == (1, 33, 1024) and out.modality_abs.shape == (1,)
    assert torch.equal(out.inst_attr[0], rs) and torch.equal(out.inst_abs[0], ra) and torch.equal(out.attr[0], attr)
    assert torch.equal(out.step_risk, steps) and float(out.risk) == float(risk) and float(out.risk_baseline) == float(base)


def test_surface_refusals():
    from multimodalfusion_amd import _lib, infer
    c, model, bags = _model("c_2seg_small_ungated_n33")
    model.train()
    with pytest.raises(RuntimeError):
        model.integrated_gradients(**bags)
    with pytest.raises(RuntimeError):
        infer.radio_integrated_gradients_autograd(model, bags, [0.5], [1.0])
    model.eval()
    with pytest.raises(NotImplementedError):
        model.integrated_gradients(**{m: x.to(torch.bfloat16) for m, x in bags.items()})
    with pytest.raises(_lib.MmfError):
        model.integrated_gradients(T1=bags["T1"], T2=bags["T2"][:5])
    h = model.classifier.register_forward_hook(lambda *a: None)
    try:
        with pytest.raises(NotImplementedError):
            model.integrated_gradients(**bags)
    finally:
        h.remove()
    with pytest.raises(ValueError):
        model.integrated_gradients(method="riemann_left", **bags)
    with pytest.raises(NotImplementedError):
        infer.attribute_radiology(torch.nn.Linear(4, 4), bags)
    model.train()
    out = infer.attribute_radiology(model, {m: x.cpu() for m, x in bags.items()}, n_steps=4)   # eval for the call, then restored
    assert model.training and out.inst_abs.shape == (2, 33) and out.modality_abs.shape == (2,) and out.attr is None


def test_attribute_radiology_returns_the_oracles_top_five():
    from multimodalfusion_amd import infer
    name = "c_4seg_small_gated_n150"
    c, model, bags = _model(name)
    o = rc.oracle(name)
    out, top = infer.attribute_radiology(model, bags, n_steps=c.n_steps, top_k=5)
    torch.cuda.synchronize()
    top = top.cpu().numpy().tolist()
    score, bar = o.row_abs.sum(0), o.bar_row_abs.sum(0)
    order = np.argsort(-score)
    assert len(top) == 5 and len(set(top)) == 5
    # an instance belongs to the top five for certain when it beats the sixth by more than both bars, and stays out when the
    # fifth beats it so; ranks are compared where neighbours are that far apart
    fifth, sixth = order[4], order[5]
    for i in order[:5]:
        if score[i] - score[sixth] > bar[i] + bar[sixth]:
            assert i in top, i
    for i in top:
        assert score[i] + bar[i] >= score[fifth] - bar[fifth], i
    for r in range(4):
        i, j = order[r], order[r + 1]
        if score[i] - score[j] > bar[i] + bar[j] and i in top and j in top:
            assert top.index(i) < top.index(j), (i, j)
    assert (np.abs(_np(out.inst_abs) - o.row_abs) <= o.bar_row_abs).all()
