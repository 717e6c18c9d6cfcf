"""CPU checks of the large-bag launch planner (tests/launch_plans.py) and of the GPU size tables that run its plans.

The Python restatement of the planner is pinned to the library's own exported functions, bag size by bag size; every
plan any bag size reaches (both heads, gated or not, attention dropout, eval / train, the concurrent hint, one bag,
grouped pathology and radio windows, fp32 and bf16 storage) must be reached by a case of the GPU tables
(tests/test_gpu_tile_plans.py); and the wide-tile kernels compiled into the library are exactly the reachable ones.
Needs the built library, not a GPU."""
import re
import shutil
import subprocess

import numpy as np
import pytest

import launch_plans as lp


def test_planner_symbols_bind():
    """Every planner function the restatement is checked against is exported under the mangled name of its signature."""
    missing = []
    from multimodalfusion_amd import _lib
    lib = _lib.lib()
    for name, (sym, _, _) in lp.SYMBOLS.items():
        if not hasattr(lib, sym):
            missing.append(f"{sym} (mmf::{name})")
    assert not missing, "libmmf_amil.so no longer exports: " + ", ".join(missing)
    assert set(lp.bound()) == set(lp.SYMBOLS)


def _sizes():
    """Every N up to 100,000, then a stride of 97 up to the largest fp32 bag the ABI accepts (and that bag itself)."""
    return np.unique(np.concatenate([np.arange(1, 100_001), np.arange(100_001, lp.N_MAX["fp32"], 97),
                                     [lp.N_MAX["fp32"]]])).astype(np.int64)


def _lib_vec(f, N, *args):
    return np.array([f(int(n), *args) for n in N])


@pytest.mark.parametrize("head", ["small", "big"])
def test_restatement_matches_library(head):
    b = lp.bound()
    L, H, D = lp.HEADS[head]
    N = _sizes()
    for split in (0, 1):
        np.testing.assert_array_equal(lp.use_wide_tiles(N, H, split), _lib_vec(b["use_wide_tiles"], N, H, split),
                                      err_msg=f"use_wide_tiles {head} split={split}")
    np.testing.assert_array_equal(lp.use_wide_tiles(N, L), _lib_vec(b["use_wide_tiles"], N, L, 0),
                                  err_msg="use_wide_tiles (radio reduce_dim, N = L)")
    np.testing.assert_array_equal(lp.tn_tile_dim(N), _lib_vec(b["tn_tile_dim"], N, D), err_msg=f"tn_tile_dim {head}")
    for conc in (0, 1):
        for allow_half, max_rows in ((True, 240), (True, 224), (False, 224), (False, 240)):
            np.testing.assert_array_equal(
                lp.pick_wide_rows(N, H // 256, allow_half, conc, max_rows),
                _lib_vec(b["pick_wide_rows"], N, H // 256, allow_half, bool(conc), max_rows),
                err_msg=f"pick_wide_rows {head} allow_half={allow_half} concurrent={conc} max_rows={max_rows}")
        for gated in (1, 0):
            np.testing.assert_array_equal(lp.bwd_dh_fused_groups(N, H, conc),
                                          _lib_vec(b["bwd_dh_fused_groups"], N, H, 1, D, gated, 0, conc),
                                          err_msg=f"bwd_dh_fused_groups {head} gated={gated} concurrent={conc}")
            # K-dh's whole plan: one bag (the caller can fuse K-prep) and the grouped form (it cannot), fp32 (split 0)
            for p_att in (0, 1):
                for can_fuse in (1, 0):
                    want = lp.dh_plan(N, H, D, gated, p_att, conc, can_fuse)
                    got = [b["plan_bwd_dh"](int(n), H, D, gated, p_att, 0, conc, can_fuse, lp.PREP_GROUPS) for n in N]
                    for field, w in want.items():
                        np.testing.assert_array_equal(
                            w, np.array([getattr(g, field) for g in got]),
                            err_msg=f"plan_bwd_dh.{field} {head} gated={gated} dropout={p_att} concurrent={conc} "
                                    f"can_fuse={can_fuse}")
    # reduce_dim of the radio window: four 256-column tiles, whole blocks, not concurrent
    R = N[N <= lp.RADIO_R_MAX[2]]
    np.testing.assert_array_equal(lp.pick_wide_rows(R, L // 256, False, False, 240),
                                  _lib_vec(b["pick_wide_rows"], R, L // 256, False, False, 240), err_msg="reduce_dim")


def test_bf16_route_and_wide_ksplit_match_library():
    b = lp.bound()
    N = np.concatenate([np.arange(1, 2001, 7), np.arange(2001, lp.N_MAX["bf16"], 1009), [524288, 524289]])
    for head, (L, H, D) in lp.HEADS.items():
        for gated in (1, 0):
            for n in N:
                n = int(n)
                assert lp.dh2_bf16_ok(n, H, D, gated) == b["dh2_bf16_ok"](n, H, D, gated), (head, gated, n)
                fused = bool(gated) and D == 256 and b["fused_fwd2_ok"](n, L, H, D)
                assert lp.bf16_fused_route(n, L, H, D, gated) == fused, (head, gated, n)
    # the wide projection never takes the K split (linear_ksplit's plan is the small tiles')
    for n in (16384, 20000, 60001, 8192):
        assert b["linear_ksplit"](n, 512, 1024, 1, 1024) == 1


def test_tables_reach_every_plan():
    """Every plan key reachable at any bag size is reached by a case of the GPU tables; remove a case and this names the
    plan it alone reached, with the configuration and the smallest bag that reaches it."""
    reach = lp.all_reachable()
    have = lp.table_keys()
    missing = [f"{k} (e.g. N={n}, {cfg})" for k, (cfg, n) in sorted(reach.items(), key=str) if k not in have]
    assert not missing, "plans no GPU case reaches:\n  " + "\n  ".join(missing)
    unreachable = [k for k in have if k not in reach]
    assert not unreachable, unreachable


def test_each_plan_key_is_the_one_its_case_describes():
    """The plan each table entry names (its comment) is the one it takes: the rows in the comment are the projection's
    and K-dh's heights."""
    for N, head, gated, dropout, train, conc, route, why in lp.ONE_BAG:
        keys = lp.plan(N, head, gated, dropout, train, conc)
        m = re.search(r"(\d+) / (\d+)", why)
        if m:
            lin = [k[2] for k in keys if k[:2] == ("linear", "wide")]
            dh = [k[2] for k in keys if k[:2] == ("dh", "wide")]
            assert lin == [int(m.group(1))] and dh == [int(m.group(2))], (N, head, why, sorted(keys, key=str))
        v = re.search(r"variant (\d)", why)
        if v:
            assert [k[4] for k in keys if k[:2] == ("dh", "wide")] == [int(v.group(1))], (N, why)


def _heights(keys):
    return {k[2] for k in keys if k[:2] in (("linear", "wide"), ("dh", "wide"), ("dh", "wide_seg"))}


def test_wide_cases_end_inside_tiles():
    """Each wide bag (but the two at the threshold itself) ends inside a tile of every wide launch it takes, and every
    half-block height in the tables has a bag (or window) that ends inside that height's 16-row half block."""
    threshold = {(16384, "small"), (8192, "big")}
    in_half = set()
    half_heights = set()
    ends = [(N, head, lp.plan(N, head, g, d, t, c)) for N, head, g, d, t, c, _, _ in lp.ONE_BAG]
    ends += [(sum(s), head, lp.plan(sum(s), head, g, d, t, False, grouped=True)) for s, head, g, K, t, d, _ in lp.GROUPED]
    for N, head, keys in ends:
        for h in _heights(keys):
            if h % 32:
                half_heights.add(h)
                if N % h > h - 16:
                    in_half.add(h)
            if (N, head) not in threshold:
                assert N % h != 0, (N, head, h)
    assert half_heights == {80, 112, 144, 176, 208, 240}
    assert in_half == half_heights, sorted(half_heights - in_half)


def test_grouped_bag_edges():
    """Across the grouped windows a bag boundary falls inside a tile, inside a 16-row half block and exactly on a tile
    edge; there are one-row bags between large ones, a G = 64 window above the wide threshold, an ungated K = 8 window
    and train-mode windows with attention dropout (per-bag masks in the epilogues, TN mode 2)."""
    inside = on_edge = in_half = False
    for sizes, head, gated, K, train, dropout, _ in lp.GROUPED:
        R = sum(sizes)
        keys = lp.plan(R, head, gated, dropout, train, False, grouped=True)
        edges = np.cumsum(sizes)[:-1]
        for h in _heights(keys):
            r = edges % h
            inside |= bool((r != 0).any())
            on_edge |= bool((r == 0).any())
            if h % 32:
                in_half |= bool((r >= h - 16).any())
    assert inside and on_edge and in_half
    assert any(1 in s[1:-1] for s, *_ in lp.GROUPED)
    assert any(len(s) == 64 and bool(lp.use_wide_tiles(sum(s), lp.HEADS[h][1])) for s, h, *_ in lp.GROUPED)
    assert any(not g and K == 8 for _, _, g, K, *_ in lp.GROUPED)
    assert any(("tn", 256, 2) in lp.plan(sum(s), h, g, d, t, False, grouped=True) for s, h, g, K, t, d, _ in lp.GROUPED)
    for sizes, nmod, gated, K, train, dropout, _ in lp.RADIO:
        assert sum(sizes) > 16384


_TILE_W = r"mmf::Tile<(\d+), 256, 1, 8, true, (true|false), 4, false>"


def _compiled_wide_keys():
    """Plan keys of the wide-tile kernels compiled into the library (their template arguments carry height and variant)."""
    from multimodalfusion_amd import _lib
    out = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    keys = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = re.search(r"mmf::linear_nt_kernel<" + _TILE_W + r", (true|false)>", line)
        if m and m.group(2) == "true":
            keys.add(("linear", "wide", int(m.group(1)), m.group(3) == "true"))
        m = re.search(r"mmf::bwd_dh_kernel<" + _TILE_W + r", (true|false), (-?\d), (true|false)>", line)
        if m and m.group(2) == "false":
            rows, fused, mode, seg = int(m.group(1)), m.group(3) == "true", int(m.group(4)), m.group(5) == "true"
            if seg:
                keys.add(("dh", "wide_seg", rows))
            else:
                keys.add(("dh", "wide", rows, fused, (3 if mode < 0 else mode) if fused else None))
    return keys


# Compiled, and launched by no stack configuration: K-dh without fused K-prep is compiled at the whole-block heights only
# (DhWide, csrc/mmf_amil_bwd.hip: its epilogue has no half-block code), and of those the stack reaches 128, 160, 192 and 224
# rows, where K-prep takes more than PREP_GROUPS tiles.  The scorer's backward with dx (mmf_attn_net_backward), which never
# fuses K-prep, takes the other two at and just above the wide threshold: tests/test_gpu_attn_net.py runs the 96-row tile
# at N = 20011 and the 64-row tile at N = 16384 (H = 256, gated).
SCORER_ONLY = {("dh", "wide", r, False, None) for r in (64, 96)}


@pytest.mark.skipif(shutil.which("nm") is None, reason="needs binutils nm")
def test_compiled_wide_kernels_are_the_reachable_ones():
    compiled = _compiled_wide_keys()
    reach = set()
    for cfg in lp.configs():
        reach |= {k for k in lp.reachable(cfg) if k[:2] in (("linear", "wide"), ("dh", "wide"), ("dh", "wide_seg"))}
    assert reach <= compiled, sorted(reach - compiled, key=str)
    assert compiled - reach == SCORER_ONLY, sorted((compiled - reach) ^ SCORER_ONLY, key=str)
    # ... and the scorer does reach them: without fused K-prep, not concurrent (the library's plan at those sizes)
    b = lp.bound()
    for n, rows in ((16384, 64), (20011, 96)):
        pl = b["plan_bwd_dh"](n, 256, 256, 1, 0, 0, 0, 0, lp.PREP_GROUPS)
        assert (pl.kind, pl.rows, pl.fused) == (lp.DH_WIDE, rows, 0), (n, pl.kind, pl.rows, pl.fused)


def test_tables_hold_the_named_cases():
    """The cases the coverage alone would not keep: both sides of the wide threshold, the headline plan (50k `small`
    gated train with the concurrent hint, by nll_step and through BagsInFlight), a bag with K-prep of its own launch,
    the autograd route on both heads, and a radio window above the wide threshold."""
    one = {(N, head, route, conc) for N, head, _, _, _, conc, route, _ in lp.ONE_BAG}
    for case in ((16383, "small", "step", False), (16384, "small", "step", False), (16385, "small", "step", False),
                 (8192, "big", "step", False), (50000, "small", "step", True), (50000, "small", "flight", True)):
        assert case in one, case
    assert ("dh", "prep", "own launch") in lp.plan(60001, "small", True, False, True, False)
    assert any(N > 57345 and head == "small" and train for N, head, _, _, train, *_ in lp.ONE_BAG)
    assert {head for _, head, *_, route, _ in lp.ONE_BAG if route == "autograd"} == {"small", "big"}
    assert lp.RADIO and all(sum(sizes) > 16384 and nmod == 4 for sizes, nmod, *_ in lp.RADIO)
    assert {(head, train) for _, head, _, _, train, _ in lp.BF16} == {("small", False), ("big", True)}
