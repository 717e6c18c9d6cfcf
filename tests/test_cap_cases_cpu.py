"""CPU: the inputs and the oracle of tests/test_gpu_row_caps.py (tests/cap_cases.py) -- on the very arrays the GPU tests use:
no hidden unit of a base bag within the summation bound of the ReLU kink, after a fixed, small number of redraw rounds;
multiplicities that sum to N; every case at the cap the rule gives its stack; the periodic oracle equal to
oracle.cases.run_path where the multiplicities are uniform, and equal to the plain oracle on the bag written out where
they are not."""
import numpy as np
import pytest
import torch

import abi_shapes as ab
import cap_cases as cc
from oracle import cases
from oracle import torch_port as tp

# redraw rounds of each base bag: fixed here, so that a change of the generator, the bound or a seed shows
ROUNDS = {"f32_32_256_128_ungated": 0, "f32_128_1024_128_gated": 1, "f32_small_gated": 2,
          "f32_small_gated_bf16x3": 4, "f32_160_512_640_gated": 2, "bf16_small_gated": 3,
          "bf16_64_512_384_ungated": 1, "bf16_64_1024_128_gated": 1, "group_96_256_128_ungated": 1,
          "scorer_256_128_gated": 0, "train_32_256_128_ungated": 0}


def test_every_case_has_its_rounds_pinned():
    assert set(ROUNDS) == set(cc.BY_NAME)


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c.name)
def test_base_bags_hold_no_unit_near_the_relu_kink(c):
    sd, x, rounds = cc.base_bag(c.name)
    assert x.shape == (c.n0, c.size[1] if c.chain == "scorer" else c.size[0]) and x.dtype == np.float32
    assert rounds == ROUNDS[c.name] <= cc.MAX_ROUNDS, (c.name, rounds)
    if c.chain != "scorer":
        assert int(cc.flagged_units(sd, x).sum()) == 0
        raw = cases.path_inputs(cc.meta(c))[1]
        assert (rounds == 0) == (int(cc.flagged_units(sd, raw).sum()) == 0)      # the redraw was needed, or it did nothing
    assert c.n0 > 256 and c.n0 % 16 != 0


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c.name)
def test_cases_sit_at_the_cap_and_multiplicities_sum_to_N(c):
    m = cc.multiplicities(c.N, c.n0)
    assert int(m.sum()) == c.N and m.shape == (c.n0,)
    assert np.array_equal(m, np.bincount(np.arange(c.N) % c.n0, minlength=c.n0))
    if c.N == cc.WEIGHTED:
        assert sorted(set(m.tolist())) == [1555, 1556] and int((m == 1556).sum()) == 252
    else:
        assert c.N % c.n0 == 0 and set(m.tolist()) == {c.N // c.n0}
    if c.chain == "scorer":
        a = ab.Attn(c.N, c.size[1], c.size[2], c.gated)
        assert ab.attn_rule(a) == ab.OK and ab.attn_rule(ab.Attn(c.N + 1, a.H, a.D, a.gated)) == ab.ERR_SHAPE
        return
    s = ab.Stack(*c.size, c.gated, bf16=c.chain == "bf16")
    cap = ab.group_row_cap(s) if c.chain == "group" else ab.stack_row_cap(s)
    assert c.N == cap and ab.stack_rule(s, c.N) == ab.OK and ab.stack_rule(s, c.N + 1) == ab.ERR_SHAPE
    if c.chain == "group":
        sizes = [p * c.n0 for p in c.periods]
        assert sum(sizes) == c.N and min(c.periods) == 1 and max(sizes) > c.N // 2 and len(set(sizes)) == len(sizes)
        assert ab.group_rule(s, sizes) == ab.OK and len(sizes) <= ab.GROUP_MAX
        assert max((n + ab.POOL_MAX_ROWS - 1) // ab.POOL_MAX_ROWS for n in sizes) <= ab.GROUP_BAG_MAX_PARTIALS


def test_the_issue_cases_are_all_here():
    have = {(c.chain, c.size, c.gated, c.N, c.n0, c.gemm) for c in cc.CASES}
    S = cc.SMALL
    assert have == {("f32", (32, 256, 128), False, 2097151, 337, 0), ("f32", (128, 1024, 128), True, 524287, 337, 0),
                    ("f32", S, True, 524287, 337, 0), ("f32", S, True, 524287, 337, 1),
                    ("f32", (160, 512, 640), True, 419430, 341, 0),
                    ("bf16", S, True, 1048575, 341, 0), ("bf16", (64, 512, 384), False, 1398101, 683, 0),
                    ("bf16", (64, 1024, 128), True, 1048575, 341, 0),
                    ("group", (96, 256, 128), False, 2097151, 337, 0), ("scorer", (256, 256, 128), True, 2097151, 337, 0),
                    ("train", (32, 256, 128), False, 2097151, 337, 0)}


def _close(a, b, tol=1e-12):
    assert float(a["loss"]) == pytest.approx(float(b["loss"]), abs=tol)
    for k in ("hazards", "S", "A_raw", "M"):
        assert float(np.abs(a[k] - b[k]).max()) <= tol, k
    assert set(a["grads"]) == set(b["grads"])
    for k, g in b["grads"].items():
        assert float(np.abs(a["grads"][k] - g).max()) <= tol, k


@pytest.mark.parametrize("c", [cc.F32[0], cc.F32[2], cc.F32[4]], ids=lambda c: c.name)
def test_periodic_oracle_is_run_path_under_uniform_multiplicities(c):
    """The pin: on the raw draw of the base bag, with every multiplicity N / n0 (here 6223, 1555 and 1230), the periodic
    oracle is oracle.cases.run_path to 1e-12."""
    m = cc.meta(c)
    sd, x, _ = cases.path_inputs(m)
    got = cc.periodic_oracle(sd, x, np.full(c.n0, c.N // c.n0), m["y"], m["c"], m["alpha"], c.gated)
    _close(got, cases.run_path(m))


def test_periodic_oracle_is_the_plain_oracle_on_the_bag_written_out():
    """Non-uniform multiplicities: 23 base rows, 60 rows (14 of them three times, 9 twice), against
    oracle.torch_port.path_step on the 60 rows."""
    c = cc.F32[0]
    m = cc.meta(c, 23)
    sd, x, _ = cases.path_inputs(m)
    mult = cc.multiplicities(60, 23)
    assert sorted(set(mult.tolist())) == [2, 3]
    got = cc.periodic_oracle(sd, x, mult, m["y"], m["c"], m["alpha"], c.gated)
    ref = tp.path_step(sd, x[np.arange(60) % 23], m["y"], m["c"], m["alpha"], gated=c.gated)
    ref["A_raw"] = ref["A_raw"][:, :23]
    _close(got, ref)


def test_scorer_oracle_is_autograd_on_the_bag_written_out():
    """The scorer's parameter gradients under multiplicities against plain autograd over 60 rows of 23."""
    c = cc.SCORER
    sd, x, _ = cc.base_bag(c.name)
    x, n0, n = x[:23], 23, 60
    gA = np.linspace(-1, 1, n0)[:, None]
    sdt = tp.to_torch({k: v for k, v in sd.items() if k.startswith(cc.PRE + ".3")}, torch.float64)
    idx = np.arange(n) % n0
    A, _ = tp.attn_net(sdt, cc.PRE + ".3", torch.as_tensor(x[idx]).double(), c.gated, False, None)
    ref = torch.autograd.grad(A, list(sdt.values()), torch.as_tensor(gA[idx]))
    A0, _ = tp.attn_net(sdt, cc.PRE + ".3", torch.as_tensor(x).double(), c.gated, False, None)
    got = torch.autograd.grad(A0, list(sdt.values()), torch.as_tensor(gA * cc.multiplicities(n, n0)[:, None]))
    for a, b in zip(got, ref):
        assert float((a - b).abs().max()) <= 1e-12


def test_bf16_cases_take_the_unchanged_bf16_oracle():
    for c in cc.BF16:
        assert c.N % c.n0 == 0
        xq = cc.xq(c.name)
        assert np.array_equal(xq, xq.astype(np.float32).astype(np.float64))
        assert np.array_equal(torch.as_tensor(xq).to(torch.bfloat16).double().numpy(), xq)
