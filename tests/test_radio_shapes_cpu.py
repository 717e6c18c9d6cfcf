"""CPU: the admitted envelope of the radiology window (mmf_radio_nll_step_group, mmf_radio_infer_group) and of the grouped
half chains (mmf_amil_group_forward / _backward, mmf_radio_group_forward / _backward) -- the RADIO and HALF tables of
tests/abi_shapes.py against their required classes, the restated rules against the library on fake pointers with a
zero-byte workspace (an admitted shape stops at MMF_ERR_WORKSPACE, before any launch and any pointer read), both workspace
queries, the radio row cap with its operand census, the row limits ops.py restates against the caps restated here, and the
conditions the inputs of tests/radio_cases.py must meet for the bars tests/test_gpu_radio_shapes.py holds.  Needs the
built library, not a GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import abi_shapes as ab
import radio_cases as rc

RADIO_OK, RADIO_NO = ab.accepted(ab.RADIO, ab.radio_rule), ab.refused(ab.RADIO, ab.radio_rule)
HALF_OK, HALF_NO = ab.accepted(ab.HALF, ab.half_rule), ab.refused(ab.HALF, ab.half_rule)
_id = lambda c: c.why


def _lib():
    from multimodalfusion_amd import _lib as m
    return m, m.lib()


# ---- the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["RADIO", "HALF"])
def test_tables_are_pinned_to_their_required_classes_both_ways(name):
    table, tags, required = ab.TABLES[name]
    assert not ab.uncovered(name), sorted(ab.uncovered(name), key=str)
    for i, c in enumerate(table):
        assert c.why
        lost = ab.uncovered(name, table[:i] + table[i + 1:])
        assert lost and lost <= tags(c), f"{name}: {c} covers no required class of its own"
    assert len(set(table)) == len(table)


def test_the_tables_hold_what_the_issue_lists():
    """Read off the cases, not off REQUIRED."""
    from test_gpu_radio_group_step import SIXTY_FOUR
    assert ab.SIXTY_FOUR == tuple(SIXTY_FOUR) and len(SIXTY_FOUR) == 64 and (min(SIXTY_FOUR), max(SIXTY_FOUR)) == (1, 90)
    r = RADIO_OK
    assert {c.nseg for c in r} == {2, 3, 4} and {c.kseg for c in r} == {32, 96, 128, 160} and {c.H for c in r} == {256, 512, 1024}
    assert {ab.chunks(c.kseg) for c in r} == {"one", "odd", "four"} and ab.chunks(160) == "odd" and 160 // ab.KC == 5
    assert {c.gated for c in r} == {True, False} and {c.train for c in r} == {True, False} and {c.accumulate for c in r} == {0, 1}
    assert {(c.kseg, c.H, c.D, c.gated) for c in r} == {(s.L, s.H, s.D, s.gated) for s in ab.accepted(ab.STACK_F32, ab.stack_rule)}
    assert {tuple(c.sizes) for c in r} >= {(1, 65, 300), ab.SIXTY_FOUR} and any(len(c.sizes) == 1 for c in r)
    assert {ab.linear_ksplit(c.R, c.L, c.nseg * c.kseg, c.nseg, c.kseg) > 1 for c in r} == {True, False}
    assert {ab.radio_tn_splits(c) > 1 for c in r} == {True, False}
    assert all(c.R <= 4000 for c in ab.RADIO + ab.HALF), "no case needs more than a few thousand rows"
    assert {(c.nseg, c.kseg == c.L, ab.stack_rule(c.stack)) for c in RADIO_NO if not c.misalign} == {
        (1, True, ab.OK), (5, True, ab.OK), (2, False, ab.OK), (2, True, ab.ERR_SHAPE)}
    h = HALF_OK
    assert {c.ldm_extra for c in h} == {0, 1} | {2 * c.H for c in h if c.ldm == 3 * c.H} and any(c.ldm == 3 * c.H for c in h)
    assert all(c.m_offset > 0 and c.m_offset + c.H <= c.ldm for c in h if c.ldm != c.H)
    assert {c.H for c in h} == {256, 512, 1024} and {bool(c.radio) for c in h} == {True, False}
    assert {c.train for c in h} == {True, False} and {c.accumulate for c in h} == {0, 1}
    assert {(ab.half_rule(c), c.ldm < c.H, c.misalign) for c in HALF_NO} == {(ab.ERR_SHAPE, True, ""), (ab.ERR_ALIGN, False, "dM")}


# ---- the rules against the library ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RADIO_NO + RADIO_OK, ids=_id)
def test_radio_cases_get_the_rules_code_from_all_four_radio_entry_points(c):
    m, l = _lib()
    got = rc.entry_calls(m, l, c, rc.fake_pointers())
    assert set(got) == set(rc.RADIO_ENTRIES)
    for name, code in got.items():
        want = ab.radio_rule(c, grads=rc.WRITES_GRADS[name])
        assert code == (want if want != ab.OK else ab.ERR_WORKSPACE), (name, code, want)
    if c in RADIO_NO:
        assert any(code != ab.ERR_WORKSPACE for code in got.values())


@pytest.mark.parametrize("c", HALF_NO + HALF_OK, ids=_id)
def test_half_cases_get_the_rules_code_from_their_entry_points(c):
    """A plain case on the pathology pair; every case also as a radio pair (nseg 2 where the case has none), so that each
    refusal of the HALF table is seen by all four half entry points."""
    m, l = _lib()
    for cc in {c, dataclasses.replace(c, radio=c.radio or 2)}:
        got = rc.entry_calls(m, l, cc, rc.fake_pointers(), ldm=cc.ldm, entries=rc.PLAIN_ENTRIES + rc.RADIO_ENTRIES[2:])
        assert set(got) == set(rc.RADIO_ENTRIES[2:] if cc.radio else rc.PLAIN_ENTRIES)
        for name, code in got.items():
            want = ab.half_rule(cc, bwd=name.endswith("backward"))
            assert code == (want if want != ab.OK else ab.ERR_WORKSPACE), (name, code, want)


def test_half_refusals_come_in_the_rules_order():
    """ldm < H is MMF_ERR_SHAPE even with a misaligned dM; a refused stack width comes before ldm."""
    m, l = _lib()
    c = dataclasses.replace(HALF_NO[0], misalign="dM")
    assert set(rc.entry_calls(m, l, c, rc.fake_pointers(), ldm=c.ldm).values()) == {ab.ERR_SHAPE}
    c = dataclasses.replace(HALF_OK[0], H=768)
    assert ab.half_rule(c) == ab.ERR_SHAPE and set(rc.entry_calls(m, l, c, rc.fake_pointers(), ldm=768).values()) == {ab.ERR_SHAPE}
    wide = dataclasses.replace(HALF_NO[1], ldm_extra=4)      # a gathered dM may sit anywhere
    assert ab.half_rule(wide) == ab.OK
    assert set(rc.entry_calls(m, l, wide, rc.fake_pointers(), ldm=wide.ldm).values()) == {ab.ERR_WORKSPACE}


def _query(l, name, offsets, G, nseg, kseg, H=256, D=128, gated=1):
    arr = None if offsets is None else (C.c_int64 * len(offsets))(*offsets)
    return getattr(l, name)(arr, G, nseg, kseg, H, D, gated)


@pytest.mark.parametrize("name", ["mmf_radio_group_workspace_bytes", "mmf_radio_group_infer_workspace_bytes"])
def test_workspace_queries_answer_zero_exactly_where_the_header_says(name):
    """include/mmf_amil.h: 0 for an invalid offset table, nseg outside 2..4 or kseg < 1 -- and for nothing else: widths
    check_desc refuses still get a size (the query does not see the descriptor)."""
    m, l = _lib()
    ok = [0, 1, 66, 366]
    for nseg in range(0, 7):
        for kseg in (-32, 0, 1, 32, 96, 160):
            want_zero = not 2 <= nseg <= 4 or kseg < 1
            assert (_query(l, name, ok, 3, nseg, kseg) == 0) == want_zero, (nseg, kseg)
    for offsets, G in ((None, 1), ([0, 10], 0), ([0] + [1] * 64, 64), (list(range(66)), 65), ([0, 10, 5], 2), ([3, 10, 20], 2),
                       ([0, 2**21 + 1], 1)):
        assert _query(l, name, offsets, G, 2, 32) == 0, offsets and offsets[:4]
    assert _query(l, name, list(range(65)), 64, 2, 32) > 0 and _query(l, name, [0, 2**21], 1, 2, 32) > 0
    assert _query(l, name, ok, 3, 2, 32, H=768) > 0 and _query(l, name, ok, 3, 2, 48) > 0
    hdr = " ".join(_header().replace(" * ", " ").split())
    assert "mmf_radio_group_workspace_bytes: the workspace of that window (L = kseg), or 0 when the offset table is invalid, " \
           "nseg is outside 2..4 or kseg < 1" in hdr
    assert "mmf_radio_group_infer_workspace_bytes: its workspace, or 0 (invalid table, nseg outside 2..4 or kseg < 1)" in hdr


def _header():
    import os
    from conftest import ROOT
    return open(os.path.join(ROOT, "include", "mmf_amil.h")).read()


# ---- the radio row cap ---------------------------------------------------------------------------------------------------
CAPS = ab.radio_cap_stacks()
_cap_id = lambda c: f"nseg={c.nseg} {c.size} {'gated' if c.gated else 'ungated'}"


def _at(c, N):
    return dataclasses.replace(c, sizes=(337, N - 337))


def test_radio_row_cap_figures():
    R = lambda n, L, H, D: ab.Radio(n, L, H, D, True, (1,), True)
    assert ab.radio_row_cap(R(4, 1024, 256, 256)) == 131071 and ab.radio_row_cap(R(2, 1024, 256, 256)) == 262143
    assert ab.radio_row_cap(R(3, 1024, 256, 256)) == 174762
    assert ab.radio_row_cap(R(2, 32, 256, 128)) == ab.group_row_cap(ab.Stack(32, 256, 128, True)) == 2**21 - 1
    assert ab.radio_row_cap(R(4, 128, 1024, 128)) == 2**19 - 1            # H binds, not 4 * 128
    assert ab.radio_row_cap(R(4, 160, 512, 640)) == 419430                 # 2 D binds
    assert {c.size for c in CAPS} >= {(1024, 256, 256), (128, 1024, 128), (32, 1024, 384)} and {c.nseg for c in CAPS} == {2, 3, 4}


@pytest.mark.parametrize("c", CAPS, ids=_cap_id)
def test_every_operand_is_below_2_gib_at_the_radio_row_cap(c):
    cap = ab.radio_row_cap(c)
    for chain in ("radio", "radio infer"):
        over = {k: v for k, v in ab.census_bytes(chain, c, cap).items() if v >= 2**31}
        assert not over, (chain, c.size, cap, over)
        names = [n for n, *_ in ab.census(chain, c)]
        assert "xr" in names and ("dxr" in names) == (chain == "radio") and "x concatenated" in names
        assert sum(n.startswith("x[") for n in names) == c.nseg
    # tight: at cap + 1 the cap's own operand (or the window's pooling-group limit) is reached
    top = max(ab.census_bytes("radio", c, cap + 1).values())
    assert top >= 2**31 or ab.census_slack("group", c.stack) > 1 or cap + 1 > ab.GROUP_POOL_GROUPS * ab.POOL_MAX_ROWS - 1


@pytest.mark.parametrize("c", CAPS, ids=_cap_id)
def test_every_radio_entry_point_refuses_cap_plus_one_and_admits_the_cap(c):
    m, l = _lib()
    cap = ab.radio_row_cap(c)
    assert ab.radio_rule(_at(c, cap)) == ab.OK and ab.radio_rule(_at(c, cap + 1)) == ab.ERR_SHAPE
    for name, code in rc.entry_calls(m, l, _at(c, cap), rc.fake_pointers()).items():
        assert code == ab.ERR_WORKSPACE, (name, code, "at the cap: admitted, stopped by the zero-byte workspace")
    for name, code in rc.entry_calls(m, l, _at(c, cap + 1), rc.fake_pointers()).items():
        assert code == ab.ERR_SHAPE, (name, code, "at cap + 1")


@pytest.mark.parametrize("c", CAPS, ids=_cap_id)
def test_radio_workspace_queries_do_not_wrap_at_the_cap(c):
    m, l = _lib()
    cap = ab.radio_row_cap(c)
    for name, chain in (("mmf_radio_group_workspace_bytes", "radio"), ("mmf_radio_group_infer_workspace_bytes", "radio infer")):
        q = lambda N: _query(l, name, [0, 337, N], 2, c.nseg, c.kseg, c.H, c.D, 1 if c.gated else 0)
        at, below = q(cap), q(cap - 1)
        assert at >= ab.census_workspace(chain, c, cap), (name, c.size, at, ab.census_workspace(chain, c, cap))
        assert at >= below > 0


# ---- the row limits ops.py restates ----------------------------------------------------------------------------------------
LIMIT_STACKS = ([c for c in ab.STACK_F32 + ab.STACK_BF16 if ab.stack_rule(c) == ab.OK]
                + [ab.Stack(*s, True) for s in ab.SHIPPED_HEADS.values()])


@pytest.mark.parametrize("c", LIMIT_STACKS, ids=lambda c: f"{c.size}{' bf16' if c.bf16 else ''}")
def test_ops_row_limits_equal_the_restated_caps(c):
    """Python closes a window where the library would refuse it.  With max(L, 2 D) in ops.group_row_limit (the formula
    check_desc had before H went into its row cap) this fails for every H = 1024 stack of the tables: 2,097,152 rows
    promised for (128, 1024, 128) where the library admits 524,287."""
    from multimodalfusion_amd import ops
    f32, b16 = dataclasses.replace(c, bf16=False), dataclasses.replace(c, bf16=True)
    assert ops.group_row_limit(*c.size) == ab.group_row_cap(f32)
    assert ops.infer_group_row_limit(*c.size) == ab.group_row_cap(f32)
    assert ops.infer_group_row_limit(*c.size, bf16=True) == ab.group_row_cap(b16)
    for nseg in (2, 3, 4):
        r = ab.Radio(nseg, c.L, c.H, c.D, c.gated, (1,), True)
        assert ops.radio_group_row_limit(nseg, *c.size) == ops.radio_infer_group_row_limit(nseg, *c.size) == ab.radio_row_cap(r)
        assert ops.mm_group_row_limits(path=c.size, radio=(nseg, *c.size)) == (ab.group_row_cap(f32), ab.radio_row_cap(r))
    assert ops.mm_group_row_limits(radio=(1, *c.size)) == (None, ab.group_row_cap(f32))
    assert ops.mm_group_row_limits(path=c.size) == (ab.group_row_cap(f32), None)


def test_ops_row_limits_at_the_shipped_heads_keep_their_figures():
    from multimodalfusion_amd import ops
    for size in ((1024, 256, 256), (1024, 512, 384)):
        assert ops.group_row_limit(*size) == ops.infer_group_row_limit(*size) == 524287
        assert ops.infer_group_row_limit(*size, bf16=True) == 1048575
        assert ops.radio_group_row_limit(4, *size) == ops.radio_infer_group_row_limit(4, *size) == 131071
        assert ops.radio_group_row_limit(2, *size) == 262143 and ops.radio_group_row_limit(3, *size) == 174762
        assert ops.mm_group_row_limits(path=size, radio=(4, *size)) == (524287, 131071)
    assert "131,071 rows at four 1024-wide modalities" in ops.radio_group_row_limit.__doc__
    assert ops.group_row_limit(128, 1024, 128) == 524287 and ops.group_row_limit(32, 1024, 384) == 524287


# ---- the inputs the GPU file runs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RADIO_OK + HALF_OK, ids=_id)
def test_inputs_meet_the_conditions_the_gpu_file_relies_on(c):
    """The ReLU kink cap of the issue (at most 1 % of H excused, none at kseg = 32) -- met with room: the recorded seeds
    leave NO case with an excused unit, so every gradient is held to the tight bar.  The float64 reduce_dim output is of
    unit scale, every bag has rows of its own, and the state dict has the widths of the case."""
    kinks = rc.kink_units(c)
    assert len(kinks) <= 0.01 * c.H and not (c.kseg == 32 and kinks)
    assert not kinks, sorted(kinks)
    sd, xs = rc.state(c), rc.window(c)
    assert len(xs) == rc.n_mod(c) and all(x.shape == (c.R, c.L) and x.dtype == np.float32 for x in xs)
    assert sd[rc.PREFIX + ".0.weight"].shape == (c.H, c.L)
    names = [n for n in rc.stack_names(c) if n]
    assert all(n in sd for n in names) and len(names) == (8 if c.gated else 6)
    assert sd[names[2]].shape == (c.D, c.H)
    if c.nseg:
        assert sd["reduce_dim.weight"].shape == (c.L, c.nseg * c.L)
    else:
        assert "reduce_dim.weight" not in sd
    xr = rc.reduce_dim_output(c)
    assert 0.5 < float(xr.std()) < 2.0
    offs = np.concatenate([[0], np.cumsum(c.sizes)])
    if len(c.sizes) > 1:
        assert not np.array_equal(xs[0][offs[0]:offs[0] + 1], xs[0][offs[1]:offs[1] + 1])
    metas = rc.bag_metas(c)
    assert len({m["mask_seed"] for m in metas}) == len(metas) and {m["train"] for m in metas} == {c.train}


def test_the_majority_of_cases_has_no_excused_unit():
    cases_ = RADIO_OK + HALF_OK
    assert sum(not rc.kink_units(c) for c in cases_) == len(cases_)


def test_accumulate_cases_start_from_non_zero_buffers():
    for c in RADIO_OK + HALF_OK:
        if c.accumulate:
            b = rc.before(c, rc.PREFIX + ".0.weight", (c.H, c.L))
            assert b.dtype == np.float32 and float(np.abs(b).min()) > 0 and float(b.std()) > 0.1


def test_default_radio_inputs_are_unchanged():
    """oracle/inputs.py radio_state_dict and oracle/cases.py radio_inputs with no size are the shipped head's, bit for bit."""
    from oracle import cases
    from oracle import inputs as gen
    a = gen.radio_state_dict(seed=3, n_mod=2, bias_std=0.05)
    b = gen.radio_state_dict(seed=3, n_mod=2, bias_std=0.05, size="small")
    e = gen.radio_state_dict(seed=3, n_mod=2, bias_std=0.05, size=(1024, 256, 256))
    assert list(a) == list(b) == list(e) and all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], e[k]) for k in a)
    assert a["reduce_dim.weight"].shape == (1024, 2048) and a["attention_net_radio.0.weight"].shape == (256, 1024)
    m = dict(gated=True, n_mod=2, K=4, dropout=True, alpha=0.3, bias_std=0.05, train=True, seed=3, x_seed=4, mask_seed=5, n=3)
    sd, xs, masks = cases.radio_inputs(m)
    sd2, xs2, masks2 = cases.radio_inputs(dict(m, size="small"))
    assert all(np.array_equal(x, y) for x, y in zip(xs, xs2)) and xs[0].shape == (3, 1024)
    assert all(np.array_equal(masks[k], masks2[k]) for k in masks) and masks["h"].shape == (3, 256) and masks["a"].shape == (3, 256)
    s, x3, m3 = cases.radio_inputs(dict(m, size=(96, 512, 128)))
    assert x3[0].shape == (3, 96) and m3["h"].shape == (3, 512) and m3["a"].shape == (3, 128)
    assert s["reduce_dim.weight"].shape == (96, 192) and s["classifier.weight"].shape == (4, 512)
