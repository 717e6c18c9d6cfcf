"""CPU checks of the stage-2 integrated-gradients cases and their float64 oracle (tests/stage2_ig_cases.py): the kink caps
hold on the committed seeds, BOUND holds against a float32 evaluation of the same forward, the oracle's sums equal the
quadrature of step_risk's derivative, and the completeness gap shrinks with the nodes.  No GPU, no library."""
import numpy as np
import pytest
import torch

import stage2_ig_cases as sc

NAMES = [c.name for c in sc.CASES]


def test_the_cases_cover_what_the_kernels_branch_on():
    fams = {(c.family, c.train_type) for c in sc.CASES}
    assert fams == {(f, t) for f in ("nll", "cox") for t in ("early-fcnn", "late-fcnn", "early-highway", "late-highway",
                                                             "kronecker")}
    for mode in ("radio_path", "radio_omic", "path_omic", "radio_path_omic"):
        assert sum(c.mode == mode for c in sc.CASES) >= 2, mode
    for tt in {t for _, t in fams}:
        assert any(c.train_type == tt and c.mode == "radio_path_omic" for c in sc.CASES), tt
    assert {c.P for c in sc.CASES} >= {1, 2, 5, 33} and {c.n_steps for c in sc.CASES} == {1, 4, 20, 64}
    assert {c.K for c in sc.CASES if c.family == "nll"} == {1, 4, 32}
    assert any(c.method == "riemann_middle" for c in sc.CASES)
    assert {c.train_type for c in sc.CASES if c.n_layers == 2} == {"early-highway", "late-highway"}
    rows = {c.P * c.n_steps for c in sc.CASES if c.train_type == "kronecker"}
    assert {60, 100} <= rows                       # windows of 64 rows straddle patients, the last one is partial


@pytest.mark.parametrize("name", NAMES)
def test_caps_hold_on_the_committed_seeds(name):
    o = sc.oracle(name)
    per_node = max((len(v) for v in o.flagged.values()), default=0)
    total = sum(len(v) for v in o.flagged.values())
    print(f"{name}: {total} flagged units, at most {per_node} per (patient, node)")
    assert per_node <= sc.NODE_CAP and total <= sc.CASE_CAP


@pytest.mark.parametrize("name", NAMES)
def test_bound_holds_against_a_float32_evaluation(name):
    gap = sc.float32_gap(name)
    print(f"{name}: largest |pre32 - pre64| / BOUND = {gap:.3f}")
    assert gap <= 1.0


@pytest.mark.parametrize("name", NAMES)
def test_sums_equal_the_quadrature_of_the_risk_derivative(name):
    """sum attr = sum_k w_k d risk(alpha x) / d alpha at alpha_k: the derivative by central differences of the float64
    forward along the path.  A patient with a flagged unit is left out: the difference straddles that kink."""
    c, o = sc.BY_NAME[name], sc.oracle(name)
    _, sd = sc.make_model(c)
    sd64 = {k: torch.as_tensor(v).double() if v.dtype != np.int64 else torch.as_tensor(v) for k, v in sd.items()}
    x64 = {n: torch.as_tensor(v).double() for n, v in sc.inputs(c).items()}
    ns = sc.names(c.mode)
    al, wt = sc.quadrature(c)
    h, total = 1e-6, np.zeros(c.P)
    for a, w in zip(al, wt):
        r = []
        for t in (float(a) + h, float(a) - h):
            with torch.no_grad():
                r.append(sc._risk(c, sd64, {n: v * t if n in ns else v for n, v in x64.items()})[0].numpy())
        total += float(w) * (r[0] - r[1]) / (2 * h)
    clean = np.array([not any(q == p for q, _ in o.flagged) for p in range(c.P)])
    assert clean.sum() >= (c.P + 1) // 2
    assert np.abs(o.mod_sum.sum(1) - total)[clean].max() <= 1e-6 * max(1.0, np.abs(total).max())


def test_delta_shrinks_between_4_and_20_nodes():
    base = sc.BY_NAME["nll_early_fcnn_rpo"]
    gaps = []
    for n in (4, 20):
        c = base._replace(name=f"_delta_{n}", n_steps=n)
        sc.BY_NAME[c.name] = c
        try:
            o = sc.oracle(c.name)
        finally:
            del sc.BY_NAME[c.name]
        gaps.append(np.abs(o.mod_sum.sum(1) - (o.risk - o.risk_base)).max())
    print("delta at 4 and 20 nodes:", gaps)
    assert gaps[1] < gaps[0]
