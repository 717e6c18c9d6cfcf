"""CPU: the input conditions of the radiology head's integrated-gradients tests, on the very arrays tests/test_gpu_radio_ig.py
runs the kernels on (tests/radio_ig_cases.py): the folded form the library runs -- composed bias, U, Gacc, the two
back-products -- is the definition in float64; tier A is kink-free within its redraw cap; tier B's allowance stays below a
tenth of the signal; the quadrature is what the library is given."""
import numpy as np
import pytest

import radio_ig_cases as rc

NAMES = [c.name for c in rc.CASES]


def test_the_case_table_is_the_one_the_tests_name():
    assert [(c.nseg, c.H, c.D, c.gated, c.N, c.K, c.n_steps, c.window_steps) for c in rc.TIER_A] == [
        (2, 256, 128, False, 17, 4, 20, 0), (3, 256, 128, True, 65, 4, 20, 0), (4, 256, 256, True, 300, 4, 20, 0),
        (4, 512, 384, True, 65, 4, 20, 0), (2, 1024, 384, False, 65, 5, 4, 0), (3, 256, 256, True, 1, 1, 20, 0),
        (4, 256, 256, True, 4096, 4, 4, 0), (2, 256, 128, False, 17, 4, 64, 64), (2, 256, 128, False, 17, 4, 1, 1)]
    assert all(c.kseg == 32 for c in rc.TIER_A)
    assert [(c.nseg, c.kseg, c.H, c.D, c.gated, c.N, c.K, c.n_steps) for c in rc.TIER_B] == [
        (3, 96, 256, 128, True, 65, 4, 20), (4, 160, 512, 640, True, 33, 32, 20), (4, 128, 1024, 128, True, 65, 1, 4)]
    assert [(c.nseg, c.kseg, c.H, c.D, c.gated, c.N, c.n_steps) for c in rc.TIER_C] == [
        (4, 1024, 256, 256, True, 150, 20), (2, 1024, 256, 256, False, 33, 4)]
    assert len(rc.BY_NAME) == len(rc.CASES) and rc.MAX_ROUNDS == 16 and rc.ALLOW_CAP == 0.1


@pytest.mark.parametrize("name", NAMES)
def test_the_folded_form_is_the_definition(name):
    o = rc.oracle(name)
    got = rc.folded_attr(name)
    err = np.abs(got - o.attr).max() / np.abs(o.attr).max()
    print(f"{name}: folded vs definition {err:.2e} of max|attr|")
    assert err <= 1e-12
    # the weights carry both biases: without them a dropped b1' would go unseen
    sd = rc.inputs(name)[0]
    assert np.abs(sd["reduce_dim.bias"]).min() > 0 and np.abs(sd[rc.PRE + ".0.bias"]).min() > 0


@pytest.mark.parametrize("name", [c.name for c in rc.TIER_A])
def test_tier_a_is_kink_free_within_its_rounds(name):
    c = rc.BY_NAME[name]
    sd, xs, rounds = rc.inputs(name)
    print(f"{name}: {rounds} redraw rounds")
    assert rounds <= rc.MAX_ROUNDS and xs.shape == (c.nseg, c.N, c.kseg) and not xs.flags.writeable
    assert not rc.flagged_units(sd, xs, rc.quadrature(c)[0]).any()
    o = rc.oracle(name)
    assert not o.allow.any() and not o.flagged_rows.any()
    assert (o.bar_attr == 1e-4 * np.abs(o.attr).max()).all() and o.bar_total == 1e-4 * o.total_abs


@pytest.mark.parametrize("name", [c.name for c in rc.TIER_B])
def test_tier_b_allowance_stays_below_a_tenth_of_the_signal(name):
    o = rc.oracle(name)
    ratio = o.allow.max() / np.abs(o.attr).max()
    print(f"{name}: largest allowance {ratio:.3f} of max|attr|, {int(o.flagged_rows.sum())} rows flagged")
    assert ratio <= rc.ALLOW_CAP
    assert (o.allow >= o.allow_max).all() and (o.allow.sum(2) >= o.allow_rowmax * (1 - 1e-12)).all()


def test_the_kink_bound_counts_the_bias_kernels_chain():
    assert rc.bias_chain(32) == 8 and rc.bias_chain(96) == 9 and rc.bias_chain(1024) == 23
    assert all(rc.bias_chain(L) <= L for L in (32, 96, 128, 160, 1024))       # c = L is safe for any order


@pytest.mark.parametrize("name", NAMES)
def test_the_quadrature_is_what_the_library_is_given(name):
    from multimodalfusion_amd import ops
    c = rc.BY_NAME[name]
    a, w = rc.quadrature(c)
    a0, w0 = ops.ig_quadrature(c.method, c.n_steps)
    assert a.dtype == np.float64 and len(a) == c.n_steps
    np.testing.assert_array_equal(a, a0.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(w, w0.astype(np.float32).astype(np.float64))
    assert abs(w.sum() - 1.0) <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_oracle_sums_are_consistent(name):
    o = rc.oracle(name)
    np.testing.assert_allclose(o.mod_abs, np.abs(o.attr).sum((1, 2)), rtol=1e-12)
    np.testing.assert_allclose(o.mod_sum.sum(), o.total, rtol=0, atol=1e-12 * o.total_abs)
    assert abs(o.risk + o.S.sum()) <= 1e-12 and abs(o.delta - (o.total - (o.risk - o.risk_base))) <= 1e-15
