"""CPU: the input conditions of the multimodal concat head's integrated-gradients tests, on the very arrays
tests/test_gpu_mm_ig.py runs the kernels on (tests/mm_ig_cases.py): the folded form the library runs -- U_p, U_r with the
composed bias, Z = W_o0 x_o, one head over the fused row, the back-products -- is the definition in float64 in every mode;
tier A is kink-free within its redraw cap, ReLU and SELU units alike; the allowance of tiers B and C stays below a tenth of
the signal; the biases are non-zero; completeness holds to quadrature error."""
import numpy as np
import pytest

import mm_ig_cases as mc

NAMES = [c.name for c in mc.CASES]


def _count(flags):
    """Flagged rows of a stack, or the flagged units of the two omic layers."""
    return [int(np.sum(v)) for v in (flags if isinstance(flags, list) else [flags])]


def test_the_case_table_is_the_one_the_tests_name():
    a = {c.name: c for c in mc.TIER_A}
    assert len(a) == 8 and all((c.path is None or c.path.L == 32) and (c.radio is None or c.radio.kseg == 32) for c in mc.TIER_A)
    c = a["a_rpo_shipped_hidden"]
    assert (c.path, c.radio, c.omic, c.K) == ((32, 256, 256, True, 65), (4, 32, 256, 256, True, 17), (80, 256, 256), 4)
    c = a["a_rp_mixed_gates_n300"]
    assert c.mode == "radio_path" and not c.path.gated and c.path.N == 300 and c.radio.gated and (c.radio.nseg, c.radio.N) == (2, 33)
    c = a["a_ro_odd_omic_k1"]
    assert c.mode == "radio_omic" and (c.radio.nseg, c.radio.N) == (3, 65) and c.omic == (7, 33, 64) and c.K == 1 and mc.columns(c)[1] == 320
    c = a["a_po_omic_first_big"]
    assert mc.order(c.mode) == ["omic", "path"] and c.path == (32, 512, 384, True, 17) and c.omic == (36, 256, 256)
    assert mc.columns(c) == ({"omic": (0, 256), "path": (256, 512)}, 768)
    c = a["a_rpo_one_row_k32"]
    assert c.path.N == c.radio.N == 1 and c.omic.Gin == 1 and c.K == 32
    c = a["a_rpo_far_apart_n4096"]
    assert (c.path.N, c.radio.N, c.n_steps, c.method, c.window_steps) == (4096, 150, 4, "riemann_middle", 0)
    assert (a["a_rp_riders_alone"].n_steps, a["a_rp_riders_alone"].window_steps) == (64, 64)
    assert (a["a_po_one_step_windows"].n_steps, a["a_po_one_step_windows"].window_steps) == (1, 1)
    assert sorted(c.path.L for c in mc.TIER_B) == [96, 160] and [c.omic for c in mc.TIER_B if c.omic] == [(80, 1024, 256)]
    assert max(mc.columns(c)[1] for c in mc.TIER_B) == 1024           # the widest fused row there is (module docstring)
    c = mc.TIER_C[0]
    assert (c.path, c.radio, c.omic, c.n_steps) == ((1024, 256, 256, True, 150), (4, 1024, 256, 256, True, 33), (80, 256, 256), 20)
    assert {c.mode for c in mc.CASES} == {"radio_path_omic", "radio_path", "radio_omic", "path_omic"}
    assert len(mc.BY_NAME) == len(mc.CASES) and mc.MAX_ROUNDS == 16 and mc.ALLOW_CAP == 0.1
    assert abs(mc.JUMP - 1.0507009873554805 * 0.6732632423543772) <= 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_the_folded_form_is_the_definition(name):
    o = mc.oracle(name)
    got = mc.folded_attr(name)
    top = max(np.abs(v).max() for v in o.attr.values())
    assert set(got) == set(o.attr) == set(mc.order(mc.BY_NAME[name].mode))
    for b, v in got.items():
        assert v.shape == o.attr[b].shape, b
        err = np.abs(v - o.attr[b]).max() / top
        print(f"{name} {b}: folded vs definition {err:.2e} of max|attr|")
        assert err <= 1e-12, b
    # every bias the identity moves is there: without them a dropped b1', b_o0 or b_o1 would go unseen
    sd = mc.inputs(name)[0]
    c = mc.BY_NAME[name]
    keys = ([mc.PRE_P + ".0.bias"] if c.path else []) + ([mc.PRE_R + ".0.bias", "reduce_dim.bias"] if c.radio else []) + (
        ["fc_omic.0.0.bias", "fc_omic.1.0.bias"] if c.omic else []) + ["classifier.bias"]
    for k in keys:
        assert np.abs(sd[k]).min() > 0, k


@pytest.mark.parametrize("name", [c.name for c in mc.TIER_A])
def test_tier_a_is_kink_free_within_its_rounds(name):
    c = mc.BY_NAME[name]
    sd, xs, rounds = mc.inputs(name)
    print(f"{name}: {rounds} redraw rounds")
    assert rounds <= mc.MAX_ROUNDS and all(not v.flags.writeable for v in xs.values())
    if c.path:
        assert xs["path"].shape == (c.path.N, c.path.L)
    if c.radio:
        assert xs["radio"].shape == (c.radio.nseg, c.radio.N, c.radio.kseg)
    if c.omic:
        assert xs["omic"].shape == (c.omic.Gin,)
    f = mc.flagged(c, sd, xs, mc.quadrature(c)[0])
    assert not any(np.any(v) for b, v in f.items() if b != "omic")
    assert not c.omic or not (f["omic"][0].any() or f["omic"][1].any())
    o = mc.oracle(name)
    for b in o.attr:
        assert not o.allow[b].any() and not any(_count(o.flagged[b]))
        assert (o.bar_attr[b] == 1e-4 * np.abs(o.attr[b]).max()).all()
    assert o.bar_total == 1e-4 * o.total_abs


@pytest.mark.parametrize("name", [c.name for c in mc.TIER_B])
def test_tier_b_allowance_stays_below_a_tenth_of_the_signal(name):
    o = mc.oracle(name)
    top = max(np.abs(v).max() for v in o.attr.values())
    for b in o.attr:
        ratio = o.allow[b].max() / top
        print(f"{name} {b}: largest allowance {ratio:.4f} of max|attr|, flagged {_count(o.flagged[b])}")
        assert ratio <= mc.ALLOW_CAP, b
        assert (o.allow[b] >= o.allow_max[b]).all()
    assert all(np.isfinite(v) for v in o.bar_share.values())


def test_the_omic_bound_counts_the_kernels_chains():
    assert mc.omic_chain(1) == 7 and mc.omic_chain(80) == 8 and mc.omic_chain(256) == 10 and mc.omic_chain(1024) == 22
    assert all(mc.omic_chain(n) <= n + 6 for n in (1, 7, 33, 64, 80, 256, 1024))


@pytest.mark.parametrize("name", NAMES)
def test_the_quadrature_is_what_the_library_is_given(name):
    from multimodalfusion_amd import ops
    c = mc.BY_NAME[name]
    a, w = mc.quadrature(c)
    a0, w0 = ops.ig_quadrature(c.method, c.n_steps)
    assert a.dtype == np.float64 and len(a) == c.n_steps
    np.testing.assert_array_equal(a, a0.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(w, w0.astype(np.float32).astype(np.float64))
    assert abs(w.sum() - 1.0) <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_oracle_sums_are_consistent(name):
    o = mc.oracle(name)
    for b, v in o.attr.items():
        assert abs(o.mod_abs[b] - np.abs(v).sum()) <= 1e-12 * o.total_abs and abs(o.mod_sum[b] - o.row_sum[b].sum()) <= 1e-12 * o.total_abs
    assert abs(sum(o.share.values()) - 1.0) <= 1e-12
    assert abs(o.risk + o.S.sum()) <= 1e-12 and abs(o.delta - (o.total - (o.risk - o.risk_base))) <= 1e-15


@pytest.mark.parametrize("name", [c.name for c in mc.CASES if c.n_steps == 20])
def test_completeness_holds_to_quadrature_error(name):
    """20 Gauss-Legendre nodes: delta = total - (risk - risk_base) is quadrature error (the integrand has a kink wherever a
    ReLU unit changes sign, so the rule is not exact to order 40).  The error of a sum of attributions scales with their
    magnitudes, not with what is left of them after cancellation -- radio_path's risk difference is 8e-3 of attributions
    that add up to 1.5 in magnitude -- so the gap is held to 5 % of the risk difference where that is the larger part of
    sum |attr|, and to 0.5 % of sum |attr| everywhere."""
    o = mc.oracle(name)
    diff = abs(o.risk - o.risk_base)
    print(f"{name}: delta {o.delta:.3e}, risk - base {o.risk - o.risk_base:.3e}, sum |attr| {o.total_abs:.3e}")
    assert abs(o.delta) <= 5e-3 * o.total_abs
    if diff >= 0.1 * o.total_abs:
        assert abs(o.delta) <= 0.05 * diff
