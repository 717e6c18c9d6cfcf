"""CPU: mmf_amil_ig over the shapes and row counts it admits (tests/abi_shapes.py IG, tests/ig_cases.py shape_*).

  * the restated window planner (ig_row_limit, ig_window_steps) against the library through mmf_amil_ig_workspace_bytes: the
    query steps exactly where the restated steps-per-window change and returns 0 exactly where the rule returns 0;
  * the pooling groups of every admitted window stay within the slots carve_ig gives them, so ig_window's refusal behind
    the projection launch cannot be reached;
  * the refusal order (ig_rule) against the library on fake pointers, table case by table case;
  * the row cap from both sides, with the census of every operand that grows with N or with steps x N;
  * the workspace query: at least the census, no wrap, monotone in window_steps; where it returns 0, as the header says;
  * the table against REQUIRED_IG, and every case's tags against what its `why` claims;
  * the inputs of tests/test_gpu_ig_shapes.py: no flagged unit, pinned redraw rounds, the periodic oracle against the direct.
Needs the built library, not a GPU."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import abi_shapes as ab
import ig_cases as ic
from test_ig_abi_cpu import ALIGN, ARG, FAKE, SHAPE, WORKSPACE, _call, _desc, _head, _ig

HD = sorted({(c.H, c.D) for c in ab.ig_cap_stacks()} | {(c.H, c.D) for c in ab.accepted(ab.IG, ab.ig_rule)})
N_SWEEP = 2**22
WINDOW_STEPS = (0, 1, 3, 22, 64)


def _q():
    from multimodalfusion_amd import _lib
    return _lib.lib().mmf_amil_ig_workspace_bytes


# ---- the planner -------------------------------------------------------------------------------------------------------------
def _steps_vec(N, H, D, total, ws):
    """ab.ig_window_steps over an array of N (written again for arrays: the two are compared below)."""
    N = np.asarray(N, np.int64)
    smax = np.minimum(np.minimum(ab.ig_row_limit(H, D) // N, ab.GROUP_MAX), total)
    if ws > 0:
        return np.where(smax < 1, 0, np.minimum(ws, smax))
    s = np.minimum(np.maximum(ab.IG_LIB_WINDOW_ROWS // N, 1), np.maximum(smax, 1))
    nwin = (total + s - 1) // s
    return np.where(smax < 1, 0, (total + nwin - 1) // nwin)


def _library_steps(q, N, L, H, D, gated, n_steps, ws):
    """The steps per window the library plans, read off the query: its size grows strictly with the window's steps (h and du
    are [steps * N x H]), so the explicit window_steps that gives the same size names them."""
    got = q(N, L, H, D, gated, n_steps, ws)
    if got == 0:
        return 0
    sizes = [q(N, L, H, D, gated, n_steps, k) for k in range(1, n_steps + 3)]
    smax = 1 + max(k for k in range(len(sizes)) if k == 0 or sizes[k] > sizes[k - 1])
    assert all(sizes[k] > sizes[k - 1] for k in range(1, smax)) and all(s == sizes[smax - 1] for s in sizes[smax - 1:])
    assert q(N, L, H, D, gated, n_steps, ab.GROUP_MAX) == sizes[smax - 1]
    hits = [k + 1 for k in range(smax) if sizes[k] == got]
    assert len(hits) == 1, (N, H, D, ws, hits)
    return hits[0]


@pytest.mark.parametrize("H,D", HD)
def test_the_query_steps_where_the_restated_window_count_changes(H, D):
    """N over 1 .. 2^22 at window_steps 0, 1, 3, 22 and 64, for 20 and 64 nodes: the restated rule is evaluated at every N;
    the library at both sides of every N where the restated steps change, at the ends, and at 64 N drawn between them."""
    q = _q()
    N = np.arange(1, N_SWEEP + 1, dtype=np.int64)
    rng = np.random.default_rng(H + D)
    for n_steps in (20, 64):
        total = n_steps + 2
        for ws in WINDOW_STEPS:
            steps = _steps_vec(N, H, D, total, ws)
            edges = np.nonzero(np.diff(steps))[0]                     # steps[e] != steps[e + 1]: N = e + 1 and e + 2
            probe = np.unique(np.concatenate([[1, 2, N_SWEEP - 1, N_SWEEP], edges + 1, edges + 2, rng.integers(1, N_SWEEP, 64)]))
            probe = probe[(probe >= 1) & (probe <= N_SWEEP)]
            for n in probe.tolist():
                want = int(steps[n - 1])
                assert want == ab.ig_window_steps(n, H, D, total, ws), (n, H, D, ws)
                for gated in (0, 1):
                    assert _library_steps(q, n, 32, H, D, gated, n_steps, ws) == want, (n, H, D, gated, n_steps, ws, want)
            zero = N[steps == 0]
            if zero.size:                                               # 0 exactly above the row limit
                assert zero[0] == ab.ig_row_limit(H, D) + 1 and (np.diff(zero) == 1).all()
                assert q(int(zero[0]), 32, H, D, 1, n_steps, ws) == 0 and q(int(zero[0]) - 1, 32, H, D, 1, n_steps, ws) > 0


def test_the_issue_window_tables():
    c = lambda N, **kw: ab.Ig(32, 256, 256, True, N, **kw)
    assert ab.ig_windows(c(11915)) == [(0, 22, 20)] and len(ab.ig_windows(c(11916))) == 2
    assert ab._ig_sizes(ab.ig_windows(c(16384))) == (11, 11)
    assert ab.ig_windows(c(32768)) == [(0, 8, 8), (8, 8, 8), (16, 6, 4)]
    w = ab.ig_windows(c(131072))
    assert ab._ig_sizes(w) == (2,) * 11 and w[-1] == (20, 2, 0) and w[-2] == (18, 2, 2)
    assert ab.ig_windows(ab.Ig(32, 256, 128, False, 17, n_steps=64, window_steps=64)) == [(0, 64, 64), (64, 2, 0)]
    assert ab.ig_windows(ab.Ig(32, 256, 128, False, 17, n_steps=1, window_steps=1)) == [(0, 1, 1), (1, 1, 0), (2, 1, 0)]
    assert ab.ig_row_limit(1024, 128) == 2**19 - 1 and ab.ig_windows(ab.Ig(128, 1024, 128, True, 30000, window_steps=22))[0][1] == 17
    assert 17 * 30000 * 1024 * 4 == 2088960000
    assert ab.ig_row_limit(256, 128) == 2**21 - 1 and ab.ig_row_limit(256, 256) == 2**20 - 1 and ab.ig_row_limit(512, 640) == 419430


def test_the_pooling_groups_of_every_admitted_window_fit():
    """ig_window refuses seg.gbeg[S] > GROUP_POOL_GROUPS + 2 * GROUP_MAX = 384 behind the projection launch.  group_plan
    gives S equal bags of N rows S * ceil(N / rpg) groups with rpg = max(64, ceil(S N / 256)): at most S N / rpg + S <= 256
    + 64 = 320.  Swept over every (N, S) with S * N within the largest row limit of any (H, D) (2^21, the pooling limit
    itself), a superset of what each stack admits: the refusal cannot be reached, every refusal comes before any launch."""
    worst = 0
    lim = ab.GROUP_POOL_GROUPS * ab.POOL_MAX_ROWS
    assert max(ab.ig_row_limit(H, D) for H, D in HD) <= lim
    for S in range(1, ab.GROUP_MAX + 1):
        N = np.arange(1, lim // S + 1, dtype=np.int64)
        rpg = np.maximum(64, (S * N + ab.GROUP_POOL_GROUPS - 1) // ab.GROUP_POOL_GROUPS)
        assert rpg.max() <= ab.POOL_MAX_ROWS
        groups = S * ((N + rpg - 1) // rpg)
        k = int(np.argmax(groups))
        assert int(groups[k]) == ab.ig_pool_groups(int(N[k]), S)
        worst = max(worst, int(groups[k]))
    print(f"the most pooling groups of any admitted window: {worst} of {ab.GROUP_POOL_GROUPS + 2 * ab.GROUP_MAX} slots")
    assert worst <= ab.GROUP_POOL_GROUPS + ab.GROUP_MAX < ab.GROUP_POOL_GROUPS + 2 * ab.GROUP_MAX


# ---- the refusal order --------------------------------------------------------------------------------------------------------
def _table_call(c, nbytes=0):
    keep = []
    kw = dict(N=c.N, L=c.L, H=c.H, D=c.D, gated=1 if c.gated else 0)
    if not c.gated:
        kw.update(Wb=None, bb=None)
    if c.bad in ("p_h", "p_att"):
        kw[c.bad] = 0.25
    if c.bad == "gemm":
        kw["gemm"] = 1
    ikw = dict(window_steps=c.window_steps, attr=(FAKE + 4 if c.bad == "attr misaligned" else FAKE) if c.attr else None)
    if c.bad == "null row_sum":
        ikw["row_sum"] = None
    return _call(desc=_desc(**kw), ig=_ig(c.n_steps, keep=keep, **ikw), head=_head(K=c.K), nbytes=nbytes)


@pytest.mark.parametrize("c", ab.IG, ids=lambda c: (c.name + " " + c.bad).strip())
def test_the_rule_is_the_librarys(c):
    """Fake pointers: an admitted case passes every check but the size of its workspace, a refused one gets its code."""
    want = ab.ig_rule(c)
    if want == ab.OK:
        need = _q()(c.N, c.L, c.H, c.D, 1 if c.gated else 0, c.n_steps, c.window_steps)
        assert need > 0 and _table_call(c, need - 1) == WORKSPACE
        return
    if c.bad == "workspace short":
        good = dataclasses.replace(c, bad="")
        assert ab.ig_rule(good) == ab.OK
        need = _q()(c.N, c.L, c.H, c.D, 1 if c.gated else 0, c.n_steps, c.window_steps)
        assert _table_call(good, need - 1) == WORKSPACE == want
        return
    assert (ARG, SHAPE, ALIGN, WORKSPACE) == (ab.ERR_ARG, ab.ERR_SHAPE, ab.ERR_ALIGN, ab.ERR_WORKSPACE)
    assert _table_call(c, 1 << 62) == want


def test_an_earlier_refusal_wins():
    """The order of ig_rule: mode before the step count before the descriptor before K before alignment."""
    base = ab.Ig(32, 256, 128, False, 17)
    for c in (dataclasses.replace(base, bad="p_h", n_steps=65, K=33), dataclasses.replace(base, n_steps=65, N=2**21, K=33),
              dataclasses.replace(base, N=2**21, K=33, bad="attr misaligned"), dataclasses.replace(base, K=33, bad="attr misaligned"),
              dataclasses.replace(base, bad="null row_sum", N=2**21)):
        assert _table_call(c, 1 << 62) == ab.ig_rule(c), c


# ---- the row cap ----------------------------------------------------------------------------------------------------------------
CAP = ab.ig_cap_stacks()
_cap_id = lambda c: f"{c.size} {'gated' if c.gated else 'ungated'} {c.n_steps} nodes"


def _library_cap(c):
    at = lambda n: _table_call(dataclasses.replace(c, N=n), 0)
    lo, hi = 338, 2**33
    assert at(lo) == WORKSPACE and at(hi) == SHAPE
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid) == WORKSPACE else (lo, mid)
    return lo


@pytest.mark.parametrize("c", CAP, ids=map(_cap_id, CAP))
def test_every_operand_is_below_2_gib_at_the_cap_the_library_enforces(c):
    cap = _library_cap(c)
    assert cap == ab.stack_row_cap(c.stack) <= ab.ig_row_limit(c.H, c.D)       # one step always fits: the `steps < 1` refusal is dead
    at = dataclasses.replace(c, N=cap)
    assert ab.ig_rule(at) == ab.OK and ab.ig_rule(dataclasses.replace(c, N=cap + 1)) == ab.ERR_SHAPE
    for ws in WINDOW_STEPS:
        w = dataclasses.replace(at, window_steps=ws)
        sizes = ab.census_bytes("ig", w, cap)
        over = {k: v for k, v in sizes.items() if v >= 2**31}
        assert not over, (c.size, cap, ws, over)
        assert _table_call(w, 0) == WORKSPACE and _table_call(dataclasses.replace(w, N=cap + 1), 0) == SHAPE
    top = max(ab.census_bytes("ig", at, cap + 1).values())
    assert top >= 2**31 or 2 * c.D > max(c.L, c.H)                                  # tight, but for check_desc's 2 D term (7p)


@pytest.mark.parametrize("c", CAP, ids=map(_cap_id, CAP))
def test_below_the_cap_no_window_operand_reaches_2_gib(c):
    """The R-wide operands at every N where the restated steps change (R = steps * N peaks just below each)."""
    cap = ab.stack_row_cap(c.stack)
    N = np.arange(1, cap + 1, dtype=np.int64)
    widest = 4 * max(c.H, c.D)
    for ws in WINDOW_STEPS:
        steps = _steps_vec(N, c.H, c.D, c.total, ws)
        assert (steps >= 1).all() and int((steps * N).max()) * widest < 2**31
        assert int((steps * N).max()) <= ab.GROUP_POOL_GROUPS * ab.POOL_MAX_ROWS


# ---- the workspace query ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CAP, ids=map(_cap_id, CAP))
def test_the_query_holds_the_census_does_not_wrap_and_grows_with_window_steps(c):
    q = _q()
    cap = ab.stack_row_cap(c.stack)
    g = 1 if c.gated else 0
    for n in (1, 17, 300, 11915, 11916, 16384, 131072, cap - 1, cap):
        if n > cap:
            continue
        prev = 0
        for ws in list(range(1, c.total + 1)) + [ab.GROUP_MAX]:
            w = dataclasses.replace(c, N=n, window_steps=ws)
            got = q(n, c.L, c.H, c.D, g, c.n_steps, ws)
            assert got >= ab.census_workspace("ig", w, n) > 0, (c.size, n, ws)
            assert got >= prev, (c.size, n, ws)
            prev = got
        lib = q(n, c.L, c.H, c.D, g, c.n_steps, 0)
        assert ab.census_workspace("ig", dataclasses.replace(c, N=n), n) <= lib <= prev
        if n > 1:
            assert lib > 0 and q(n, c.L, c.H, c.D, g, c.n_steps, 1) >= q(n - 1, c.L, c.H, c.D, g, c.n_steps, 1)


def test_where_the_query_returns_zero_is_what_the_header_says():
    """The query has no descriptor: it answers 0 for the step counts, for N < 1 and for N above the window's row limit, and
    applies neither mmf_amil_desc::N's cap nor the rules for L, H and D.  At the shipped small head the L-wide bag holds N to
    524,287 while a window takes 1,048,575 rows: between the two the query is non-zero and the call refuses."""
    from conftest import ROOT
    q = _q()
    lim = ab.ig_row_limit(256, 256)
    assert q(lim, 1024, 256, 256, 1, 20, 0) > 0 and q(lim + 1, 1024, 256, 256, 1, 20, 0) == 0
    for bad in (dict(n_steps=0), dict(n_steps=65), dict(ws=-1), dict(N=0), dict(N=-5)):
        a = dict(N=300, n_steps=20, ws=0)
        a.update(bad)
        assert q(a["N"], 1024, 256, 256, 1, a["n_steps"], a["ws"]) == 0, bad
    cap = ab.stack_row_cap(ab.Stack(1024, 256, 256, True))
    assert cap < lim and q(cap + 1, 1024, 256, 256, 1, 20, 0) > 0
    assert _table_call(ab.Ig(1024, 256, 256, True, cap + 1), 1 << 62) == SHAPE
    hdr = open(os.path.join(ROOT, "include", "mmf_amil.h")).read()
    s = hdr[hdr.index("mmf_amil_ig_workspace_bytes: the workspace of that call"):hdr.index("typedef struct mmf_ig_desc")]
    for phrase in ("N < 1", "2,097,152", "has no descriptor", "does not shrink as window_steps grows"):
        assert phrase in s, phrase


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_the_required_classes():
    assert not ab.uncovered("mmf_amil_ig")
    assert {c.size + (c.gated,) for c in ab.accepted(ab.IG, ab.ig_rule)} >= {c.size + (c.gated,) for c in ab.accepted(ab.STACK_F32, ab.stack_rule)}


W = "windows"
CLAIMS = {      # what each accepted case's `why` says it reaches: attribution tile, projection, window sizes, window classes
    "96_256_128_gated_n65_k4_s20_w0": (64, True, "64 x 64", (22,), {"one window"}),
    "160_512_640_gated_n300_k32_s20_w0": (64, True, "64 x 64", (22,), {"one window"}),
    "32_1024_384_ungated_n300_k5_s20_w0": (64, True, "64 x 64", (22,), {"one window"}),
    "32_1024_384_ungated_n1_k4_s20_w0": (64, True, "64 x 64", (22,), {"one window"}),
    "128_1024_128_gated_n65_k1_s4_w0": (64, False, "64 x 64", (6,), {"one window"}),
    "32_256_128_ungated_n17_k4_s64_w0": (64, True, "64 x 64", (33, 33), {"a library cut into even windows"}),
    "32_256_128_ungated_n17_k4_s64_w64": (64, True, "64 x 64", (64, 2), {"S = GROUP_MAX", "a window of riders alone"}),
    "32_256_128_ungated_n17_k4_s1_w1": (64, True, "64 x 64", (1, 1, 1), {"a window of riders alone", "the two riders in different windows"}),
    "256_256_128_ungated_n16384_k4_s20_w0": (128, False, "wide", (11, 11), {"a library cut into even windows"}),
    "32_256_256_gated_n32768_k4_s20_w0": (128, True, "wide", (8, 8, 6), {"a library cut with a ragged last window"}),
    "32_256_256_gated_n131072_k4_s20_w0": (128, True, "wide", (2,) * 11, {"a library cut into even windows", "a window of riders alone"}),
    "128_1024_128_gated_n30000_k4_s20_w22": (64, False, "wide", (17, 5), {"window_steps clamped by the row limit"}),
    "32_256_128_ungated_n2097151_k4_s4_w0": (128, True, "wide", (1,) * 6, {"a library cut into even windows", "a window of riders alone",
                                                                          "the two riders in different windows"}),
    "128_1024_128_gated_n524287_k4_s4_w0": (128, False, "wide", (1,) * 6, {"a library cut into even windows", "a window of riders alone",
                                                                         "the two riders in different windows"}),
    "1024_256_256_gated_n524287_k4_s2_w0": (128, False, "wide", (1,) * 4, {"a library cut into even windows", "a window of riders alone",
                                                                         "the two riders in different windows"}),
    "1024_512_384_gated_n33_k4_s2_w0": (64, False, "64 x 64, K split", (4,), {"one window"}),
}


def test_every_case_reaches_what_its_why_claims():
    cases = ab.accepted(ab.IG, ab.ig_rule)
    assert sorted(c.name for c in cases) == sorted(CLAIMS) and len({c.name for c in cases}) == len(cases)
    for c in cases:
        tile, ragged, proj, sizes, classes = CLAIMS[c.name]
        t = ab.ig_tags(c)
        assert ("attr tile", tile) in t and (("a column tile partly outside L", tile) in t) == ragged, c.name
        assert ("projection", proj) in t and ("window sizes", sizes) in t, (c.name, sorted(t, key=str))
        assert {v for k, v, *_ in t if k == W} == classes, (c.name, sorted(t, key=str))
        assert sum(S for _, S, _ in ab.ig_windows(c)) == c.total and sum(f for _, _, f in ab.ig_windows(c)) == c.n_steps
    for c in ab.refused(ab.IG, ab.ig_rule):
        assert len(ab.ig_tags(c)) == 1


# ---- the inputs of the GPU file ----------------------------------------------------------------------------------------------------
ROUNDS = {
    "96_256_128_gated_n65_k4_s20_w0": 2, "160_512_640_gated_n300_k32_s20_w0": 4, "32_1024_384_ungated_n300_k5_s20_w0": 1,
    "32_1024_384_ungated_n1_k4_s20_w0": 0, "128_1024_128_gated_n65_k1_s4_w0": 1, "32_256_128_ungated_n17_k4_s64_w0": 1,
    "32_256_128_ungated_n17_k4_s64_w64": 1, "32_256_128_ungated_n17_k4_s1_w1": 0, "256_256_128_ungated_n16384_k4_s20_w0": 7,
    "32_256_256_gated_n32768_k4_s20_w0": 1, "32_256_256_gated_n131072_k4_s20_w0": 1, "128_1024_128_gated_n30000_k4_s20_w22": 4,
    "32_256_128_ungated_n2097151_k4_s4_w0": 0, "128_1024_128_gated_n524287_k4_s4_w0": 2, "1024_256_256_gated_n524287_k4_s2_w0": 5,
    "1024_512_384_gated_n33_k4_s2_w0": 5,
}


@pytest.mark.parametrize("name", sorted(ROUNDS))
def test_no_unit_is_flagged_at_any_node_and_the_redraw_rounds_are_pinned(name):
    c = ic.shape_by_name(name)
    sd, x, rounds = ic.shape_inputs(name)
    assert rounds == ROUNDS[name] <= ic.MAX_ROUNDS == 8
    assert x.shape == (c.n0 or c.N, c.L) and x.dtype == np.float32 and not x.flags.writeable
    a, w = ic.shape_quadrature(c)
    assert a.dtype == np.float32 and a.size == c.n_steps and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    assert not ic.flagged_units(sd, x, a).any()
    if c.n0:
        assert c.n0 > 256 and c.n0 % 16 != 0 and c.N > c.n0
        m = ic.multiplicities(c.N, c.n0)
        assert int(m.sum()) == c.N and set(m.tolist()) <= {c.N // c.n0, c.N // c.n0 + 1}
    b1 = np.asarray(sd["attention_net_WSI.0.bias"], np.float64)
    assert np.abs(b1).min() > 0                          # the ReLU pattern moves from node to node (tests/test_ig_cases_cpu.py)


def test_the_existing_cases_are_untouched():
    assert [c.name for c in ic.CASES + ic.WIDE_CASES] == [
        "n1", "n5", "n17", "n33", "n300", "n4096", "n33_big_ungated_k1", "n17_k1_one_step", "n33_four_steps_trapezoid",
        "n5_big_ungated_middle", "small_gated_n300", "big_ungated_n33_k1"]
    assert not set(ROUNDS) & set(ic.BY_NAME)


@pytest.mark.parametrize("name,m", [("32_256_256_gated_n32768_k4_s20_w0", 3), ("128_1024_128_gated_n524287_k4_s4_w0", 2)])
def test_with_uniform_multiplicities_the_periodic_oracle_is_the_direct_one(name, m):
    """The base bag repeated m times through oracle.torch_port.path_forward against the base bag with log m in the softmax."""
    c = ic.shape_by_name(name)
    sd, x, _ = ic.shape_inputs(name)
    a, w = ic.shape_quadrature(c)
    per = ic.ig_oracle(sd, x, np.full(c.n0, m), a, w, c.gated)
    direct = ic.ig_oracle(sd, np.tile(x, (m, 1)), None, a, w, c.gated)
    scale = np.abs(direct.attr).max()
    assert np.abs(direct.attr - np.tile(per.attr, (m, 1))).max() <= 1e-12 * scale
    assert np.abs(direct.row_abs - np.tile(per.row_abs, m)).max() <= 1e-12 * np.abs(direct.row_abs).max()
    assert abs(direct.total - per.total) <= 1e-12 and abs(direct.total_abs - per.total_abs) <= 1e-12
    assert abs(direct.risk - per.risk) <= 1e-12 and abs(direct.risk_base - per.risk_base) <= 1e-12
    assert np.abs(direct.step_risk - per.step_risk).max() <= 1e-12 and np.abs(direct.logits - per.logits).max() <= 1e-12
    two = ic.ig_oracle(sd, x, ic.multiplicities(c.n0 + 5, c.n0), a, w, c.gated)      # and with two multiplicities
    d2 = ic.ig_oracle(sd, np.concatenate([x, x[:5]]), None, a, w, c.gated)
    assert np.abs(d2.attr[:c.n0] - two.attr).max() <= 1e-12 * np.abs(d2.attr).max()
    assert np.abs(d2.attr[c.n0:] - two.attr[:5]).max() <= 1e-12 * np.abs(d2.attr).max() and abs(d2.total - two.total) <= 1e-12
