"""CPU checks of tests/mm_tensor_ig_cases.py, the cases and the float64 oracle of the tensor-fusion head's integrated
gradients: the input conditions and the caps on the committed arrays, the folded form the library runs against the
definition in float64, the float32 check of the tail's kink bound, and the combination rule itself."""
import numpy as np
import pytest

import mm_ig_cases as mc
import mm_tensor_ig_cases as tc

NAMES = [c.name for c in tc.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_input_conditions_and_caps(name):
    c = tc.BY_NAME[name]
    sd, xs, rounds = tc.inputs(name)
    assert all(v.dtype == np.float32 and not v.flags.writeable for v in xs.values())
    assert rounds <= mc.MAX_ROUNDS
    m = len(tc.order(c.mode))
    assert sd["mm.encoder1.0.weight"].shape == (c.tail.mmhid1, 17 ** m)
    assert sd["mm.encoder2.0.weight"].shape == (c.tail.mmhid2, c.tail.mmhid1 + m * tc.dim(c))
    assert sd["classifier.3.weight"].shape == (c.K, c.tail.nhid)
    assert all(np.abs(np.asarray(sd[k])).max() > 0 for k in sd if k.endswith(".bias"))
    if c.tier == "A":                                               # no stack or omic unit on a kink: nothing excused there
        f = mc.flagged(c, sd, xs, tc.quadrature(c)[0])
        assert not any(np.any(x) for v in f.values() for x in (v if isinstance(v, tuple) else (v,)))
    o = tc.oracle(name)
    per_node = {k: len(v) for k, v in o.flagged.items()}
    print(f"{name}: flagged tail units per node {per_node}, combinations {int(np.prod([len(x[1]) + 1 for x in o.alt]))}")
    assert all(n <= tc.NODE_CAP for n in per_node.values()) and sum(per_node.values()) <= tc.CASE_CAP
    assert (tc.NODE_CAP, tc.CASE_CAP) == (3, 10)
    if c.tier == "A":
        assert all(np.all(v == 0) for v in o.allow.values())
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in o.attr.values())
    assert len(o.step_risk) == c.n_steps and abs(o.risk - o.risk_base) > 1e-3


def test_the_cases_meet_the_boundaries_they_are_there_for():
    by = tc.BY_NAME
    assert {len(tc.order(c.mode)) for c in tc.CASES} == {2, 3}
    assert {c.mode for c in tc.TIER_A} == {"radio_path_omic", "radio_path", "path_omic", "radio_omic"}
    c = by["t_rp_remainders_k1"]
    assert c.tail.mmhid1 % 64 and c.tail.mmhid2 % 4 and c.tail.nhid % 4 and c.K == 1 and c.path.gated != c.radio.gated
    c = by["t_po_omic_first_k32"]
    assert tc.order(c.mode)[0] == "omic" and c.tail.mmhid1 == 512 + 4 and c.K == 32
    assert by["t_ro_one_row"].radio.N == 1 and by["t_ro_one_row"].radio.nseg == 3
    c = by["t_rp_widest_row"]
    assert c.tail.mmhid1 + 2 * tc.dim(c) == 1536
    c = by["t_rp_riders_alone"]
    assert c.n_steps == 64 and c.window_steps == 64
    assert by["t_po_window_17"].window_steps == 17 and by["t_po_one_step_windows"].n_steps == 1
    assert all(c.path.L == 1024 for c in tc.TIER_C)
    # the rule is exercised: some node of some case has a flagged unit, in tier A and in tier C
    assert any(tc.oracle(c.name).alt for c in tc.TIER_A) and any(tc.oracle(c.name).alt for c in tc.TIER_C)


@pytest.mark.parametrize("name", NAMES)
def test_folded_form_is_the_definition_in_float64(name):
    o = tc.oracle(name)
    got = tc.folded_attr(name)
    for b, ref in o.attr.items():
        err = np.abs(got[b] - ref).max()
        print(f"{name} {b}: folded against the definition, max err {err:.3e} of max {np.abs(ref).max():.3e}")
        assert err <= 1e-9 * np.abs(ref).max(), b


@pytest.mark.parametrize("name", NAMES)
def test_float32_forward_stays_within_the_bound_at_every_unit(name):
    worst = {}
    for k, lay, gap, bound in tc.float32_gap(name):
        assert (bound > 0).all(), (k, lay)
        worst[lay] = max(worst.get(lay, 0.0), float((gap / bound).max()))
        assert (gap < bound).all(), (name, k, lay, int(np.argmax(gap / bound)))
    print(f"{name}: float32 against float64, worst gap / BOUND per layer {({k: round(v, 4) for k, v in worst.items()})}")


def test_the_combination_rule_accepts_one_combination_for_all_arrays():
    name = "t_rpo_shipped_tail"
    o = tc.oracle(name)
    assert o.alt
    rows = lambda attr: ({b: (v.sum(-1) if b != "omic" else v) for b, v in attr.items()},
                         {b: (np.abs(v).sum(-1) if b != "omic" else np.abs(v)) for b, v in attr.items()})
    combos = list(tc.combinations(o))
    assert len(combos) == int(np.prod([len(x[1]) + 1 for x in o.alt])) and all(v is None for v in combos[0][0].values())
    # every combination is accepted as itself ...
    moved = 0
    for pick, attr in combos:
        got, worst = tc.match(o, attr, *rows(attr))
        assert got is not None and worst <= 1.0
        rs, ra = rows(attr)
        moved += any(np.abs(attr[b] - o.attr[b]).max() > o.bar_attr[b].max() for b in attr)
    # ... a flipped unit moves some array past the plain bar (else the rule would be idle here) ...
    assert moved > 0
    # ... and arrays taken from two different combinations are refused: the first branch's arrays from the combination that
    # moves both it and another branch furthest, the rest from float64's own
    b0 = tc.order(tc.BY_NAME[name].mode)[0]
    shift = lambda attr, bs: min(np.abs(attr[b] - o.attr[b]).max() / o.bar_attr[b].max() for b in bs)
    both = lambda attr: min(shift(attr, [b0]), max(shift(attr, [b]) for b in o.attr if b != b0))
    far = max((attr for _, attr in combos[1:]), key=both)
    assert both(far) > 2.0, both(far)                 # the committed seed has such a combination: the check below is not idle
    mixed = {b: (far[b] if b == b0 else o.attr[b]) for b in o.attr}
    assert tc.match(o, mixed, *rows(mixed))[0] is None
