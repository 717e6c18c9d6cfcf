"""CPU checks of the large-bag launch planner (tests/launch_plans.py) and of the GPU size tables that run its plans.

The Python restatement of the planner is pinned to the library's own exported functions, bag size by bag size; every
plan any bag size reaches (both heads, gated or not, attention dropout, eval / train, the concurrent hint, one bag,
grouped pathology and radio windows, fp32 and bf16 storage) must be reached by a case of the GPU tables
(tests/test_gpu_tile_plans.py); and the wide-tile kernels compiled into the library are exactly the reachable ones, the
split-operand projection, gate forward and TN kernels exactly the kinds their plans return.
Needs the built library, not a GPU."""
import ctypes as C
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
    for conc in (0, 1):
        for allow_half, max_rows in ((True, 240), (True, 224), (False, 224), (False, 240)):
            np.testing.assert_array_equal(
                lp.pick_wide_rows(N, H // 256, allow_half, conc, max_rows),
                _lib_vec(b["pick_wide_rows"], N, H // 256, allow_half, bool(conc), max_rows),
                err_msg=f"pick_wide_rows {head} allow_half={allow_half} concurrent={conc} max_rows={max_rows}")
        for gated in (1, 0):
            np.testing.assert_array_equal(lp.bwd_dh_fused_groups(N, H, conc),
                                          np.array([b["plan_bwd_dh"](int(n), H, D, gated, 0, 0, conc, 1, 2**31 - 1).dbc_groups
                                                    for n in N]),
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


def _lib_plans(f, N, *args):
    """The library's plan (a POD of ints) for every N, as {field: array}; a nested array (GatePlan.reg) keeps its shape."""
    out = (f.restype * len(N))()
    for i, n in enumerate(N):
        out[i] = f(int(n), *args)
    flat = np.frombuffer(out, np.int32).reshape(len(N), -1)
    cols, at = {}, 0
    for name, typ in f.restype._fields_:
        width = C.sizeof(typ) // 4
        cols[name] = flat[:, at] if typ is C.c_int else flat[:, at:at + width].reshape(len(N), typ._length_, -1)
        at += width
    return cols


def _same_plan(want, got, tag):
    for field, w in want.items():
        np.testing.assert_array_equal(w, got[field], err_msg=f"{field}: {tag}")


@pytest.mark.parametrize("head", ["small", "big"])
def test_projection_plan_matches_library(head):
    """plan_linear over every bag size: the stack's projection (exact fp32 and split-operand, whole or half blocks, the
    concurrent hint, tick words on offer or not) and, once, the radio window's reduce_dim over 2 to 4 segments."""
    f = lp.bound()["plan_linear"]
    L, H, D = lp.HEADS[head]
    N = _sizes()
    for allow_half in (1, 0):
        for conc in (0, 1):
            for ticks in (0, 512):
                args = (H, L, 1, L, allow_half, conc, 0, ticks)
                _same_plan(lp.linear_plan(N, *args), _lib_plans(f, N, *args), f"{head} {args}")
    for ticks in (0, 512):      # the split-operand core: its own wide threshold, one wide height, no K split
        args = (H, L, 1, L, 1, 0, 1, ticks)
        _same_plan(lp.linear_plan(N, *args), _lib_plans(f, N, *args), f"{head} split {args}")
    if head == "small":
        for nseg in (2, 3, 4):
            R = N[N <= lp.RADIO_R_MAX[nseg]]
            for ticks in (0, 512):
                args = (L, nseg * L, nseg, L, 0, 0, 0, ticks)
                _same_plan(lp.linear_plan(R, *args), _lib_plans(f, R, *args), f"reduce_dim {args}")


@pytest.mark.parametrize("head", ["small", "big"])
def test_gate_plan_matches_library_and_covers_the_rows(head):
    """plan_gate_fwd over every bag size, gated or not, both operand modes; and of the library's own plan: the regions of
    a mixed launch cover rows 0 .. N - 1 exactly once and in order, each begins at the running sum of the grid, the grid
    is the total, and there are at most five."""
    b = lp.bound()
    L, H, D = lp.HEADS[head]
    N = _sizes()
    for gated in (1, 0):
        assert b["gate_parts"](D, gated) == lp.gate_parts(D, gated)
        for split in (0, 1):
            got = _lib_plans(b["plan_gate_fwd"], N, H, D, gated, split)
            _same_plan(lp.gate_plan(N, H, D, gated, split), got, f"{head} gated={gated} split={split}")
            nt = lp.gate_parts(D, gated)
            mixed = got["kind"] == lp.GATE_MIXED
            assert mixed.any() == (512 % (2 * nt) == 0), (head, gated)
            assert (got["nreg"][~mixed] == 0).all() and (got["nreg"][mixed] >= 1).all() and (got["nreg"] <= 5).all()
            row = np.zeros(N.shape, np.int64)
            grid = np.zeros(N.shape, np.int64)
            for i in range(5):
                on = mixed & (i < got["nreg"])
                row0, mt, begin, tall = (got["reg"][:, i, j] for j in range(4))
                assert (row0[on] == row[on]).all() and (begin[on] == grid[on]).all() and (mt[on] > 0).all(), (head, gated, split, i)
                assert (got["reg"][~on, i] == 0).all()
                # only the last region may end past the bag, and by less than a tall tile (the rounds are counted in those)
                rows = mt * np.where(tall == 1, 128, 64)
                last = on & (i == got["nreg"] - 1)
                assert (row[on & ~last] + rows[on & ~last] <= N[on & ~last]).all()
                assert ((row[last] + rows[last] >= N[last]) & (row[last] + rows[last] - N[last] < 128)).all()
                row = row + np.where(on, rows, 0)
                grid = grid + np.where(on, lp.grid_for_tiles(mt, nt), 0)
            assert (grid[mixed] == got["grid"][mixed]).all()
            one = ~mixed      # one tile height: the grid holds every tile, the tiles every row
            height = np.where(got["kind"] == lp.GATE_128, 128, 64)
            assert ((got["mt_count"][one] * height[one] >= N[one]) & ((got["mt_count"][one] - 1) * height[one] < N[one])).all()
            assert (got["grid"][one] >= got["mt_count"][one] * nt).all()


def _tn_problem_lists():
    """(tag, split modes, shapes): the stack's two problems (both heads, gated or not; the only list with a bf16x3 mode), the
    scorer's gate problem alone (also at an attention width that is no multiple of the tile), mmf_linear_backward's dW
    and the radio window's dW_r per modality."""
    out = []
    for head, (L, H, D) in lp.HEADS.items():
        for gated in (1, 0):
            out.append((f"stack {head} gated={gated}", (0, 1), lp.stack_tn_shapes(L, H, D, gated)))
            out.append((f"scorer {head} gated={gated}", (0,), [(2 * D if gated else D, H, 1)]))
    out.append(("scorer H=1024 D=160 gated", (0,), [(320, 1024, 1)]))
    for Nn, K in ((1024, 4096), (256, 1024), (36, 100), (4, 4)):
        out.append((f"linear_backward {Nn} x {K}", (0,), [(Nn, K, 0)]))
    for nseg in (2, 3, 4):
        out.append((f"radio dW_r {nseg} modalities", (0,), [(1024, 1024, 0)] * nseg))
    return out


def test_tn_plan_matches_library_and_keeps_its_bounds():
    """plan_tn over every bag size for every problem list the ABI plans; and of the library's own plan: splits cut at
    multiples of 4 instances cover K, no split is shorter than 128 instances' worth, and the 256 x 256 tiles (one
    workgroup per CU) never take more than 256 workgroups."""
    f = lp.bound()["plan_tn"]
    K = _sizes()
    for tag, splits, shapes in _tn_problem_lists():
        arr = (lp.TnShape * len(shapes))(*[lp.TnShape(*sh) for sh in shapes])
        t_plain = lambda tile: sum(-(-M // tile) * -(-Nc // tile) for M, Nc, g in shapes if not g)
        t_gate = lambda tile: sum(-(-M // tile) * -(-Nc // tile) for M, Nc, g in shapes if g)
        for split in splits:
            got = _lib_plans(f, K, split, arr, len(shapes))
            _same_plan(lp.tn_plan(K, split, shapes), got, f"{tag} split={split}")
            for s, kps in (("splits", "k_per_split"), ("splits_g", "k_per_split_g")):
                assert (got[kps] % 4 == 0).all() and (got[s] >= 1).all(), tag
                assert (got[s].astype(np.int64) * got[kps] >= K).all(), tag
            assert (got["splits"] <= (K + 127) // 128).all(), tag
            assert (got["splits_g"] >= got["splits"]).all(), tag
            wide = got["tile"] == 256
            assert (wide == (K >= 12288)).all()
            if t_plain(256) + t_gate(256) <= 256:
                assert (t_plain(256) * got["splits"][wide] + t_gate(256) * got["splits_g"][wide] <= 256).all(), tag
            if not (t_plain(256) and t_gate(256)):      # the left-over workgroups go to a gate problem beside a plain one only
                assert (got["splits_g"] == got["splits"]).all(), tag


def test_tn_plan_of_an_empty_or_negative_k_is_one_split():
    """No instances (mmf_linear_backward does not refuse M = 0: its workspace query gives the one-split 256 bytes and the launch
    refuses the zero-length split) and a negative count: one split of no rows, as the split count is capped first and raised
    to 1 afterwards."""
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    for K in (0, -1, -5, -127, -128, -129, -100000):
        for tag, splits, shapes in _tn_problem_lists():
            for split in splits:
                pl = lp.lib_plan_tn(K, split, shapes)
                assert (pl.splits, pl.splits_g, pl.tile) == (1, 1, 128), (K, tag)
                assert pl.k_per_split <= 0 and pl.k_per_split_g <= 0 and pl.k_per_split % 4 == 0, (K, tag, pl.k_per_split)
        for Nn, Kk in ((1024, 4096), (36, 100), (4, 4)):
            assert l.mmf_linear_backward_workspace_bytes(K, Nn, Kk) == 256, (K, Nn, Kk)
    dummy = C.c_void_p(256)         # refused before anything is read: the zero-length split
    segs = (C.c_void_p * 1)(256)
    assert l.mmf_linear_backward(dummy, segs, 1, 32, 0, None, 32, dummy, None, None, None, 0, None) == -1      # MMF_ERR_ARG


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
    # the wide projection never takes the K split (it is the 64 x 64 tiles'), whatever tick words are on offer
    for n in (16384, 20000, 60001, 8192):
        assert b["plan_linear"](n, 512, 1024, 1, 1024, 0, 0, 0, 2**31 - 1).ksplit == 1


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
    # a window on the gate's mixed launch with per-bag masks has a bag edge inside a tall tile and one inside a short tile
    # (the library's own regions)
    tall_edge = short_edge = False
    for sizes, head, gated, K, train, dropout, _ in lp.GROUPED:
        L, H, D = lp.HEADS[head]
        if ("gate", "mixed", True) not in lp.plan(sum(sizes), head, gated, dropout, train, False, grouped=True):
            continue
        pl = lp.bound()["plan_gate_fwd"](sum(sizes), H, D, int(gated), 0)
        for e in np.cumsum(sizes)[:-1]:
            r = [pl.reg[i] for i in range(pl.nreg) if pl.reg[i].row0 <= e][-1]
            inside = (e - r.row0) % (128 if r.tall else 64) != 0
            tall_edge |= inside and bool(r.tall)
            short_edge |= inside and not r.tall
    assert tall_edge and short_edge


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


_TILE_ANY = r"mmf::(Tile|TileSp)<(\d+), (\d+)[^>]*>"


def _compiled_family_keys():
    """The host-side symbols of the projection's split-operand kernels, the gate forward's and the TN GEMM's, as the tiles
    and template switches they carry: ("linear_split", rows, cols), ("gate", tall rows, short rows or None, split, gated,
    seg_masks), ("tn", tile, split, mode)."""
    from multimodalfusion_amd import _lib
    out = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    keys = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = re.search(r"mmf::linear_nt_split_kernel<" + _TILE_ANY + r" >", line)
        if m:
            keys.add(("linear_split", int(m.group(2)), int(m.group(3))))
        m = re.search(r"mmf::gate_fwd_kernel<" + _TILE_ANY + r", (true|false), (true|false)>", line)
        if m:
            keys.add(("gate", int(m.group(2)), None, m.group(1) == "TileSp", m.group(4) == "true", m.group(5) == "true"))
        m = re.search(r"mmf::gate_fwd_mixed_kernel<" + _TILE_ANY + ", " + _TILE_ANY + r", (true|false), (true|false)>", line)
        if m:
            assert m.group(1) == m.group(4)
            keys.add(("gate", int(m.group(2)), int(m.group(5)), m.group(1) == "TileSp", m.group(7) == "true", m.group(8) == "true"))
        m = re.search(r"mmf::tn_kernel<" + _TILE_ANY + r", (-?\d+)>", line)
        if m:
            assert m.group(2) == m.group(3)
            keys.add(("tn", int(m.group(2)), m.group(1) == "TileSp", int(m.group(4))))
    return keys


# what each plan kind launches (csrc/mmf_amil_fwd.hip launch_linear_impl, launch_gate_fwd_impl; csrc/mmf_amil_bwd.hip launch_tn)
LINEAR_SPLIT_TILES = {lp.LIN_SPLIT_WIDE: (224, 256), lp.LIN_SPLIT_64: (64, 64)}
GATE_TILES = {lp.GATE_64: (64, None), lp.GATE_128: (128, None), lp.GATE_MIXED: (128, 64)}
TN_TILES = {lp.TN_128: (128, False), lp.TN_256: (256, False), lp.TN_SPLIT_128: (128, True), lp.TN_SPLIT_256: (256, True)}
# launch_tn_grid: the exact-fp32 128 x 128 tile keeps the run-time switches (-1) but for the grouped step's per-bag masks (2),
# which no split-operand tile has; every other tile is compiled per attention-dropout state (0, 1)
TN_MODES = {lp.TN_128: (-1, 2), lp.TN_256: (0, 1, 2), lp.TN_SPLIT_128: (0, 1), lp.TN_SPLIT_256: (0, 1)}


@pytest.mark.skipif(shutil.which("nm") is None, reason="needs binutils nm")
def test_compiled_plan_kernels_are_the_kinds_the_plans_return():
    """The host-side stubs of linear_nt_split_kernel, gate_fwd*_kernel and tn_kernel are exactly the tiles of the kinds
    plan_linear, plan_gate_fwd and plan_tn can return, in the forms their launchers pick, and the library's plans do
    return every one of those kinds."""
    b = lp.bound()
    want = {("linear_split",) + t for t in LINEAR_SPLIT_TILES.values()}
    for kind, (tall, short) in GATE_TILES.items():
        for split in (False, True):
            for gated in (False, True):
                for seg in (False,) if split else (False, True):      # launch_gate_fwd_seg refuses the split-operand mode
                    want.add(("gate", tall, short, split, gated, seg))
    for kind, (tile, split) in TN_TILES.items():
        want |= {("tn", tile, split, mode) for mode in TN_MODES[kind]}
    compiled = _compiled_family_keys()
    assert compiled == want, sorted(compiled ^ want, key=str)
    # the kinds over every bag size, from the restatement the tests above pin to the library (small gated head) ...
    N = _sizes()
    L, H, D = lp.HEADS["small"]
    lin = set(lp.linear_plan(N, H, L, 1, L, 1, 0, 1, 0)["kind"])
    assert lin == set(LINEAR_SPLIT_TILES), lin
    for split in (0, 1):
        g = lp.gate_plan(N, H, D, 1, split)
        assert set(zip(g["kind"], g["split"])) == {(k, split) for k in GATE_TILES}
    tn = set().union(*(set(lp.tn_plan(N, split, lp.stack_tn_shapes(L, H, D, True))["kind"]) for split in (0, 1)))
    assert tn == set(TN_TILES), tn
    # ... and from the library itself at the first size of each kind
    for split in (0, 1):
        for n in (1000, 14000, 20000, 50000):
            assert b["plan_linear"](n, H, L, 1, L, 1, 0, split, 0).kind == lp.linear_plan([n], H, L, 1, L, 1, 0, split, 0)["kind"][0]
            assert b["plan_gate_fwd"](n, H, D, 1, split).kind == lp.gate_kind(n, D, 1)
            assert lp.lib_plan_tn(n, split, lp.stack_tn_shapes(L, H, D, True)).kind == lp.tn_plan([n], split, lp.stack_tn_shapes(L, H, D, True))["kind"][0]


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
