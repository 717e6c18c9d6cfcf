"""CPU: the input conditions of the integrated-gradients cases (tests/ig_cases.py), on the oracle alone.

  * the cap: at L = 32, H = 256 and N in {300, 4096} at most 10 % of the rows carry any kink allowance, so the others are
    held to the tight bar (at L = 1024 every row carries one: those cases are also compared with the autograd route on the
    GPU, tests/test_gpu_ig.py);
  * the first-layer bias is not zero and the ReLU pattern changes from node to node -- a wrong alpha in the expand kernel
    would otherwise go unseen;
  * the identity the library rests on: the folded form (one projection, sum_k w_k du_k, one product with W1) is the
    pass-by-pass definition, in float64;
  * an allowance is what its definition says: a flagged unit's term, summed per element."""
import numpy as np
import pytest
import torch

import ig_cases as ic
from oracle import torch_port as tp


@pytest.mark.parametrize("name", ic.CAPPED)
def test_at_most_a_tenth_of_the_rows_carry_an_allowance(name):
    c = ic.BY_NAME[name]
    assert ic.gen.stack_dims(c.size)[:2] == [32, 256] and c.n_steps == 20 and c.method == "gausslegendre"
    o = ic.oracle(name)
    frac = o.flagged_rows.mean()
    print(f"{name}: {int(o.flagged_rows.sum())} of {c.N} rows carry an allowance ({100 * frac:.1f} %)")
    assert frac <= 0.10
    clean = ~o.flagged_rows
    assert (o.allow[clean] == 0).all() and (o.bar_attr[clean] == 1e-4 * np.abs(o.attr).max()).all()
    assert (o.allow[o.flagged_rows].sum(1) > 0).all()


def test_every_row_of_the_wide_cases_carries_an_allowance_or_nearly():
    """Why the L = 1024 cases are also held to the autograd route on the GPU: against float64 they are loose by construction."""
    o = ic.oracle("small_gated_n300")
    assert o.flagged_rows.mean() > 0.5


@pytest.mark.parametrize("name", ["n300", "n33_big_ungated_k1"])
def test_bias_moves_the_relu_pattern_between_nodes(name):
    c = ic.BY_NAME[name]
    sd, x = ic.inputs(name)
    W1, b1 = (np.asarray(sd["attention_net_WSI.0." + k], np.float64) for k in ("weight", "bias"))
    assert np.abs(b1).min() > 0 and abs(b1.std() - ic.BIAS_STD) < 0.03
    a, _ = ic.quadrature(c)
    u = np.asarray(x, np.float64) @ W1.T
    first, last = a[0] * u + b1 > 0, a[-1] * u + b1 > 0
    assert (first != last).mean() > 0.05


@pytest.mark.parametrize("name", ["n33", "n300", "n33_big_ungated_k1", "n33_four_steps_trapezoid"])
def test_the_folded_form_is_the_definition_in_float64(name):
    c = ic.BY_NAME[name]
    sd, x32 = ic.inputs(name)
    sdt = tp.to_torch(sd, torch.float64, False)
    x = torch.as_tensor(x32).double()
    W1, b1 = sdt["attention_net_WSI.0.weight"], sdt["attention_net_WSI.0.bias"]
    Uproj = x @ W1.T
    G = torch.zeros_like(Uproj)
    for a, w in zip(*ic.quadrature(c)):
        u = a * Uproj + b1
        h = torch.relu(u).requires_grad_()
        A, _ = tp.attn_net(sdt, "attention_net_WSI.3", h, c.gated, False, None)
        S = tp.surv_head(tp._lin(sdt, "classifier", torch.softmax(A.T, dim=1) @ h))[1]
        (dh,) = torch.autograd.grad(-S.sum(), h)
        G += w * dh * (u > 0)
    folded = (x * (G @ W1)).numpy()
    o = ic.oracle(name)
    assert np.abs(folded - o.attr).max() <= 1e-12 * max(np.abs(o.attr).max(), 1e-30)


def test_allowance_terms():
    o = ic.oracle("n300")
    assert (o.allow >= o.allow_max).all() and (o.allow_max >= 0).all()
    assert o.bar_total >= 1e-4 * o.total_abs and o.bar_rows["row_sum"].shape == (300,)


def test_fifty_nodes_close_the_completeness_gap_further_than_twenty():
    """The small gated head at N = 300 (the GPU test holds the library's 50-node delta to the oracle's at 20 nodes there).
    The integrand is piecewise smooth, so the gap does not shrink monotonically for every bag: at L = 32 it does not."""
    name = "small_gated_n300"
    o, o50 = ic.oracle(name), ic.oracle(name, 50, False)
    print(f"{name}: |delta| {abs(o.delta):.2e} at 20 nodes, {abs(o50.delta):.2e} at 50")
    assert abs(o50.delta) < 0.75 * abs(o.delta) < 1e-3
