"""The launch planner of the large-bag attention stack, restated for the tests (helper module, not collected by pytest).

Above 16,384 rows (8,192 for the `big` head) the fp32 stack's projection and K-dh stop using one fixed tile: the planner
picks a tile height per bag size, and each height (and each K-dh variant) is its own compiled kernel.  This module

  * binds the library's exported planner functions with ctypes, by their mangled names (`bound()`),
  * restates them in Python (vectorised over N where the CPU test sweeps them), each with the function it restates:
    the plans of the projection, the gate forward, K-dh and the split-K TN GEMM, and the rules they are built from,
  * `plan(...)`: the set of large-bag kernel instantiations one training step takes, as plan keys,
  * `reachable()`: every plan key any bag size reaches, per configuration,
  * the size tables the GPU tests run (ONE_BAG, GROUPED, RADIO, BF16), each case with the plan it is meant to reach.

tests/test_launch_plans_cpu.py pins the restatement to the library and the tables to `reachable()`: a planner change
that makes a new tile plan reachable fails on CPU until a case reaches it.

Plan keys (what `plan` returns; only the launches whose tile depends on the bag size above the small-bag tiles):
  ("linear", "wide", rows, seg_masks)          projection, linear_nt_kernel<TileW<rows>, seg_masks>
  ("dh", "wide", rows, fused, variant)         K-dh, bwd_dh_kernel<Tile<rows, 256 ...>, fused, variant, false>;
                                                variant (gated ? 2 : 0) + (attention dropout ? 1 : 0) when fused (3: the
                                                kernel's run-time switches, template argument -1), None when not
  ("dh", "64x128")                             K-dh's 64 x 128 tiles (fused K-prep, gated, 13,000 rows up to the wide tiles)
  ("dh", "prep", "own launch")                 K-prep as its own launch before a wide K-dh (more than PREP_GROUPS tiles)
  ("dh", "wide_seg", rows)                     grouped K-dh, bwd_dh_kernel<Tile<rows, 256 ...>, false, -1, true>
  ("tn", 256, mode)                            split-K TN on 256 x 256 tiles, tn_kernel<T, mode>: 0 plain, 1 attention
                                                dropout, 2 per-bag attention-dropout masks (grouped step)
  ("tn", 128, mode)                            ... on 128 x 128 tiles (below 12,288 rows): None the run-time switches, 2 as above
  ("gate", "128")                              gate forward on uniform 128-row tiles
  ("gate", "mixed", seg_masks)                 gate forward on 128- and 64-row tiles in one launch (gate_fwd_mixed_kernel);
                                                seg_masks: the grouped step's per-bag attention-dropout masks
  ("linear_bf16", 256), ("gate_bf16", 256)     bf16 storage, unfused route: 256-row tiles (pick_bm)
  ("dh_bf16", gated)                           bf16 storage, unfused route: dh_bf16_kernel<TileB128, gated>
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

# ---- shapes and limits ----------------------------------------------------------------------------------------------
HEADS = {"small": (1024, 256, 256), "big": (1024, 512, 384)}       # (L, H, D): models/model_modules.py AMIL_SIZES
# check_desc (csrc/mmf_api.hip): N * max(L, H, 2 D) * bytes < 2 GiB; L = 1024 >= H, 2 D for both heads (the rule for every
# admitted stack: tests/abi_shapes.py stack_row_cap)
N_MAX = {"fp32": (2**31 - 1) // (1024 * 4), "bf16": (2**31 - 1) // (1024 * 2)}
# mmf_radio_nll_step_group (csrc/mmf_api.hip radio_operands): the [sum N x nseg * kseg] input < 2 GiB, kseg = L = 1024
RADIO_R_MAX = {nseg: min(N_MAX["fp32"], (2**31 - 1) // (nseg * 1024 * 4)) for nseg in (2, 3, 4)}
PREP_GROUPS = 512          # csrc/mmf_kernels.h PREP_GROUPS
DH_MAX_ROWS = 224          # csrc/mmf_amil_bwd.hip DH_MAX_ROWS
LINEAR_MAX_ROWS = 240      # csrc/mmf_amil_fwd.hip plan_linear's pick_wide_rows call
CUS, CUS_CONCURRENT = 256, 224      # csrc/mmf_amil_fwd.hip pick_wide_rows


# ---- the library's exported planner functions -----------------------------------------------------------------------
class DhPlan(C.Structure):
    """csrc/mmf_kernels.h DhPlan"""
    _fields_ = [(f, C.c_int) for f in ("kind", "rows", "fused", "variant", "deep", "mt_count", "nt_count", "grid",
                                       "extra_lds", "dbc_groups")]


DH_SPLIT_WIDE, DH_SPLIT_64, DH_WIDE, DH_128, DH_64X128, DH_64 = range(6)      # csrc/mmf_kernels.h DH_*


class LinearPlan(C.Structure):
    """csrc/mmf_kernels.h LinearPlan"""
    _fields_ = [(f, C.c_int) for f in ("kind", "rows", "ksplit", "deep", "mt_count", "nt_count", "grid", "kpart_floats")]


LIN_SPLIT_WIDE, LIN_WIDE, LIN_128, LIN_SPLIT_64, LIN_KSPLIT_64, LIN_64 = range(6)      # csrc/mmf_kernels.h LIN_*


class GateRegion(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("row0", "mt_count", "grid_begin", "tall")]


class GatePlan(C.Structure):
    """csrc/mmf_kernels.h GatePlan"""
    _fields_ = [(f, C.c_int) for f in ("kind", "split", "deep", "mt_count", "nt_count", "grid", "nreg")] + [("reg", GateRegion * 5)]


GATE_64, GATE_128, GATE_MIXED = range(3)      # csrc/mmf_kernels.h GATE_*


class TnShape(C.Structure):
    """csrc/mmf_kernels.h TnShape"""
    _fields_ = [(f, C.c_int) for f in ("M", "Ncols", "gate")]


class TnPlan(C.Structure):
    """csrc/mmf_kernels.h TnPlan"""
    _fields_ = [(f, C.c_int) for f in ("kind", "tile", "splits", "k_per_split", "splits_g", "k_per_split_g", "tiles")]


TN_128, TN_256, TN_SPLIT_128, TN_SPLIT_256 = range(4)      # csrc/mmf_kernels.h TN_*
KC, SKC = 32, 16       # csrc/mmf_gemm_core.h KC, csrc/mmf_gemm_split.h SKC: k-values per staged chunk

SYMBOLS = {
    # name: (mangled, restype, argtypes) -- the C++ signatures of csrc/mmf_kernels.h and csrc/mmf_bf16.h
    "pick_wide_rows": ("_ZN3mmf14pick_wide_rowsElibbi", C.c_int, [C.c_int64, C.c_int, C.c_bool, C.c_bool, C.c_int]),
    "use_wide_tiles": ("_ZN3mmf14use_wide_tilesElii", C.c_bool, [C.c_int64, C.c_int, C.c_int]),
    # (N, H, D, gated, dropout, split, concurrent, can_fuse, dbc_cap)
    "plan_bwd_dh": ("_ZN3mmf11plan_bwd_dhEliiiiiiii", DhPlan, [C.c_int64] + [C.c_int] * 8),
    # (M, N, K, nseg, kseg, allow_half, concurrent, split, tick_words)
    "plan_linear": ("_ZN3mmf11plan_linearEliiiiiiii", LinearPlan, [C.c_int64] + [C.c_int] * 8),
    # (N, H, D, gated, split)
    "plan_gate_fwd": ("_ZN3mmf13plan_gate_fwdEliiii", GatePlan, [C.c_int64] + [C.c_int] * 4),
    "gate_parts": ("_ZN3mmf10gate_partsEii", C.c_int, [C.c_int, C.c_int]),
    # (K, split, shapes, nshape): lib_plan_tn() below builds the array
    "plan_tn": ("_ZN3mmf7plan_tnEliPKNS_7TnShapeEi", TnPlan, [C.c_int64, C.c_int, C.POINTER(TnShape), C.c_int]),
    "fused_fwd2_ok": ("_ZN3mmf13fused_fwd2_okEliii", C.c_bool, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "dh2_bf16_ok": ("_ZN3mmf11dh2_bf16_okEliii", C.c_bool, [C.c_int64, C.c_int, C.c_int, C.c_int]),
}


class PlannerBindingError(RuntimeError):
    pass


_bound = None


def bound():
    """{name: ctypes function} of the planner functions exported by libmmf_amil.so.  A renamed function or a changed
    signature changes the mangled name: binding then fails and names the symbol."""
    global _bound
    if _bound is None:
        from multimodalfusion_amd import _lib
        lib = _lib.lib()
        out = {}
        for name, (sym, res, args) in SYMBOLS.items():
            try:
                f = getattr(lib, sym)
            except AttributeError:
                raise PlannerBindingError(f"libmmf_amil.so exports no {sym} (mmf::{name}): the planner's signature "
                                          f"changed; update tests/launch_plans.py") from None
            f.restype, f.argtypes = res, args
            out[name] = f
        _bound = out
    return _bound


def lib_plan_tn(K, split, shapes):
    """The library's plan_tn for a list of (M, Ncols, gate) problem shapes."""
    arr = (TnShape * len(shapes))(*[TnShape(*sh) for sh in shapes])
    return bound()["plan_tn"](int(K), int(split), arr, len(shapes))


# ---- the Python restatement ---------------------------------------------------------------------------------------
def use_wide_tiles(M, N, split=0):
    """csrc/mmf_amil_fwd.hip use_wide_tiles (no tuning overrides).  M may be an array."""
    min_rows = 80 * 256 if split else 64 * 256
    return (N % 256 == 0) & (np.asarray(M, np.int64) * (N // 256) >= min_rows)


def pick_wide_rows(M, ntn, allow_half, concurrent, max_rows):
    """csrc/mmf_amil_fwd.hip pick_wide_rows: the height (multiple of 16, 64..max_rows; odd multiples only with allow_half) with
    the least rounds x (rows / 32 + 0.35); ties keep the taller tile.  M may be an array."""
    Ms = np.atleast_1d(np.asarray(M, np.int64))
    cus = CUS_CONCURRENT if concurrent else CUS
    best = np.full(Ms.shape, 224, np.int64)
    bestc = np.full(Ms.shape, 1e30)
    for rows in range(max_rows, 63, -16):
        if rows % 32 != 0 and not allow_half:
            continue
        tiles = ((Ms + rows - 1) // rows) * ntn
        c = ((tiles + cus - 1) // cus).astype(np.float64) * (rows / 32.0 + 0.35)
        better = c < bestc
        best = np.where(better, rows, best)
        bestc = np.where(better, c, bestc)
    return best if np.ndim(M) else int(best[0])


def dh_short_grid(N, H):
    """plan_bwd_dh's `short_64` (csrc/mmf_amil_bwd.hip; split 0): the 64 x 64 K-dh tiles on at most 1,024 workgroups."""
    N = np.asarray(N, np.int64)
    return ~use_wide_tiles(N, H) & ((N // 128) * ((H + 127) // 128) < 256) & (((N + 63) // 64) * ((H + 63) // 64) <= 1024)


def bwd_dh_fused_groups(N, H, concurrent):
    """plan_bwd_dh's dbc_groups with split 0 (the fp32 stack: amil_backward_impl, csrc/mmf_api.hip) for a caller that can fuse
    and a dbc_part of any size: > 0: the number of K-prep tiles when K-dh does K-prep itself; 0: it does not."""
    N = np.asarray(N, np.int64)
    rows = pick_wide_rows(N, H // 256, True, concurrent, DH_MAX_ROWS)
    wide = use_wide_tiles(N, H)
    return np.where(dh_short_grid(N, H), (N + 63) // 64, np.where(wide, (N + rows - 1) // rows, 0))


def dh_fused(N, H, concurrent):
    """plan_bwd_dh's `fused`: K-prep runs inside K-dh when it takes at most PREP_GROUPS (the dbc_cap of dh_plan,
    csrc/mmf_api.hip) tiles."""
    g = bwd_dh_fused_groups(N, H, concurrent)
    return (g > 0) & (g <= PREP_GROUPS)


def dh_allow_half(fused, relu_bits=True):
    """plan_bwd_dh's wide height: the half-block K-dh tile needs fused K-prep and the forward's relu bits, which the
    stack's backward has (carve, csrc/mmf_api.hip: all but inference) and a caller that can fuse offers."""
    return bool(fused) and relu_bits


def dh_64x128(N, H, D, gated, fused):
    """plan_bwd_dh's DH_64X128: below the wide tiles, K-dh takes 64 x 128 tiles from 13,000 rows (fused K-prep,
    gated, H % 128 == 0, (2 D / 32) % 4 == 0)."""
    return ~use_wide_tiles(N, H) & (np.asarray(N) >= 13000) & fused & bool(gated and H % 128 == 0 and (2 * D // 32) % 4 == 0)


def dh_plan(N, H, D, gated, p_att, concurrent, can_fuse):
    """K-dh's plan as plan() below derives it, for an array N (fp32, split 0): the DhPlan fields kind, rows, fused,
    variant and dbc_groups.  can_fuse False: the grouped chain and the scorer, which run K-prep on their own.  Below the
    wide and the 64 x 128 tiles the kind is 128 x 128 where those fill the chip (the projection's rule), else 64 x 64."""
    N = np.asarray(N, np.int64)
    wide = use_wide_tiles(N, H)
    fused = dh_fused(N, H, concurrent) if can_fuse else np.zeros(N.shape, bool)
    mid = dh_64x128(N, H, D, gated, fused)
    kind = np.where(wide, DH_WIDE, np.where(mid, DH_64X128, np.where(use_big_tiles(N, H), DH_128, DH_64)))
    rows = np.where(fused, pick_wide_rows(N, H // 256, dh_allow_half(True), concurrent, DH_MAX_ROWS),
                    pick_wide_rows(N, H // 256, dh_allow_half(False), concurrent, DH_MAX_ROWS))
    rows = np.where(wide, rows, np.where(kind == DH_128, 128, 64))
    mode = (2 if gated else 0) + (1 if p_att else 0)
    variant = np.where(wide & fused, -1 if mode == 3 else mode, -1)       # 3: the run-time switches, template argument -1
    groups = np.where(fused, bwd_dh_fused_groups(N, H, concurrent), 0)
    return {"kind": kind, "rows": rows, "fused": fused.astype(np.int64), "variant": variant, "dbc_groups": groups}


def tn_tile_dim(K):
    """csrc/mmf_amil_bwd.hip plan_tn's tile: 256 x 256 TN tiles from 12,288 rows."""
    return np.where(np.asarray(K, np.int64) >= 12288, 256, 128)


def tn_plan(K, split, shapes):
    """csrc/mmf_amil_bwd.hip plan_tn (no tuning overrides) for an array K: the TnPlan fields.  shapes: (M, Ncols, gate) per
    problem; a gate problem's M is 2 D (gated) or D."""
    K = np.asarray(K, np.int64)
    tile = tn_tile_dim(K)
    kind = np.where(tile == 256, TN_SPLIT_256 if split else TN_256, TN_SPLIT_128 if split else TN_128)
    count = lambda want: sum((((M + tile - 1) // tile) * ((Nc + tile - 1) // tile) for M, Nc, g in shapes if bool(g) == want),
                             np.zeros(K.shape, np.int64))
    t_plain, t_gate = count(False), count(True)
    tiles = t_plain + t_gate
    splits = np.maximum(1, np.minimum(np.where(tile == 256, 256, 512) // np.maximum(tiles, 1), (K + 127) // 128))
    kps = lambda sp: ((K + sp - 1) // sp + 3) // 4 * 4
    splits_g = splits
    if any(g for _, _, g in shapes) and not all(g for _, _, g in shapes):
        # the workgroups the uniform split leaves over go to the gate problem, at most 12 % more splits
        left = (256 - t_plain * splits) // t_gate
        cap = splits + (splits * 12 + 99) // 100
        splits_g = np.where((tile == 256) & (splits >= 8), np.minimum(np.maximum(left, splits), cap), splits)
    return {"kind": kind, "tile": tile, "splits": splits, "k_per_split": kps(splits), "splits_g": splits_g,
            "k_per_split_g": kps(splits_g), "tiles": tiles}


def stack_tn_shapes(L, H, D, gated):
    """csrc/mmf_api.hip stack_tn_plan: dW1 [H x L] beside the gate problem d[Wa ; Wb] [2 D (gated) or D x H]"""
    return [(H, L, 0), (2 * D if gated else D, H, 1)]


def use_big_tiles(M, N):
    """csrc/mmf_amil_fwd.hip use_big_tiles: the projection's 128 x 128 tiles below the wide ones (plan_bwd_dh's `big` is
    the same rule for K-dh)."""
    return (np.asarray(M, np.int64) // 128) * ((N + 127) // 128) >= 256


def grid_for_tiles(mt, nt):
    """csrc/mmf_gemm_core.h grid_for_tiles: row tiles in groups of 8 per column tile"""
    return ((mt + 7) // 8) * 8 * nt


def short_grid(workgroups):
    """csrc/mmf_amil_fwd.hip short_grid (no tuning overrides)"""
    return workgroups <= 1024


def linear_plan(M, N, K, nseg, kseg, allow_half, concurrent, split, tick_words):
    """csrc/mmf_amil_fwd.hip plan_linear (no tuning overrides) for an array M: the LinearPlan fields."""
    M = np.asarray(M, np.int64)
    can_split = bool(split) and K % (4 * SKC) == 0 and nseg == 1
    split_wide = use_wide_tiles(M, N, 1) & can_split
    wide = ~split_wide & use_wide_tiles(M, N, int(can_split))
    small = ~split_wide & ~wide
    big = small & use_big_tiles(M, N) & (not can_split)
    kind = np.select([split_wide, wide, big, small & can_split], [LIN_SPLIT_WIDE, LIN_WIDE, LIN_128, LIN_SPLIT_64], LIN_64)
    rows = np.select([split_wide, wide, big], [224, pick_wide_rows(M, N // 256, allow_half, concurrent, LINEAR_MAX_ROWS), 128], 64)
    bn = np.where(split_wide | wide, 256, rows)
    mt, nt = (M + rows - 1) // rows, (N + bn - 1) // bn
    tiles, nk = mt * nt, K // KC
    seg_ok = nseg == 1 or kseg % (4 * KC) == 0
    ksplit = np.ones(M.shape, np.int64)
    if N % 4 == 0 and K % KC == 0 and seg_ok:
        for S in (2, 4):        # the larger split where both fit
            if nk % (4 * S) == 0 and nk // S >= 8:
                ksplit = np.where((kind == LIN_64) & (tiles <= min(tick_words, 128)) & (tiles * S <= 512), S, ksplit)
    kind = np.where(ksplit > 1, LIN_KSPLIT_64, kind)
    deep = np.where(ksplit > 1, short_grid(tiles * ksplit), (kind == LIN_64) & short_grid(tiles) & (nk % 4 == 0) & seg_ok)
    return {"kind": kind, "rows": rows, "mt_count": mt, "nt_count": nt, "ksplit": ksplit, "deep": deep.astype(np.int64),
            "grid": grid_for_tiles(mt, nt * ksplit), "kpart_floats": np.where(ksplit > 1, ksplit * tiles * 64 * 64, 0)}


GATE_BIG_MIN = 400     # csrc/mmf_amil_fwd.hip plan_gate_fwd: the fp32 gate's 128-row tiles from 400 of them


def gate_parts(D, gated):
    """csrc/mmf_amil_fwd.hip gate_parts"""
    return (D + 63) // 64 if gated else (D + 127) // 128


def gate_big_tiles(N, D, gated):
    return (np.asarray(N, np.int64) // 128) * gate_parts(D, gated) >= GATE_BIG_MIN


def gate_kind(N, D, gated):
    """plan_gate_fwd's kind (the same in both operand modes), for an array N"""
    N = np.asarray(N, np.int64)
    nt = gate_parts(D, gated)
    mixed = (((N + 127) // 128) * nt // 512 >= 2) & (512 % (2 * nt) == 0)      # two whole rounds of tall tiles
    big = gate_big_tiles(N, D, gated)
    return np.where(big & mixed, GATE_MIXED, np.where(big, GATE_128, GATE_64))


def gate_plan(N, H, D, gated, split):
    """csrc/mmf_amil_fwd.hip plan_gate_fwd (no tuning overrides) for an array N: the GatePlan fields, `reg` as an
    [len(N), 5, 4] array of (row0, mt_count, grid_begin, tall), zero past nreg."""
    N = np.asarray(N, np.int64)
    nt = gate_parts(D, gated)
    split_k = bool(split) and H % (4 * SKC) == 0
    kind = gate_kind(N, D, gated)
    big, mixed = kind != GATE_64, kind == GATE_MIXED
    mt128 = (N + 127) // 128
    total = mt128 * nt
    R = total // 512          # whole rounds of 512 tall tiles (two workgroups per CU)
    half_m = 256 // nt
    if split_k:               # one tall region over the whole rounds, then short tiles
        lens = [(1, (total - total % 512) // nt)]
    else:                     # the dephased launch: tall, short, tall, short, then short tiles
        lens = [(1, half_m + 0 * R), (0, half_m + 0 * R), (1, half_m * (2 * R - 2)), (0, half_m + 0 * R)]
    reg = np.zeros(N.shape + (5, 4), np.int64)
    row = np.zeros(N.shape, np.int64)
    grid = np.zeros(N.shape, np.int64)
    for i, (tall, m) in enumerate(lens):
        reg[:, i] = np.stack([row, m, grid, np.full(N.shape, tall)], 1)
        grid = grid + grid_for_tiles(m, nt)
        row = row + m * (128 if tall else 64)
    last = (N - row + 63) // 64
    reg[:, len(lens)] = np.where((last > 0)[:, None], np.stack([row, last, grid, np.zeros(N.shape, np.int64)], 1), 0)
    nreg = len(lens) + (last > 0)
    grid = grid + np.where(last > 0, grid_for_tiles(last, nt), 0)
    reg = np.where(mixed[:, None, None], reg, 0)
    mt = np.where(mixed, reg[:, :, 1].sum(1), np.where(big, mt128, (N + 63) // 64))
    deep = (kind == GATE_64) & (not split_k) & short_grid(mt * nt) & ((H // KC) % 4 == 0)
    return {"kind": kind, "split": np.full(N.shape, int(split_k)), "nt_count": np.full(N.shape, nt), "mt_count": mt,
            "deep": deep.astype(np.int64), "grid": np.where(mixed, grid, grid_for_tiles(mt, nt)),
            "nreg": np.where(mixed, nreg, 0), "reg": reg}


def pick_bm(rows, ntn):
    """csrc/mmf_amil_bf16.hip pick_bm (static there): 256-row bf16 tiles unless 128-row ones take fewer half-length rounds."""
    rows = np.asarray(rows, np.int64)
    t256 = ((rows + 255) // 256) * ntn
    t128 = ((rows + 127) // 128) * ntn
    c256 = ((t256 + 255) // 256).astype(np.float64) * 2.15
    c128 = ((t128 + 255) // 256).astype(np.float64) * 1.15
    return np.where(c128 < c256, 128, 256)


def gate_parts_bf16(D, gated):
    """csrc/mmf_amil_bf16.hip gate_parts_bf16"""
    return (D + 127) // 128 if gated else (D + 255) // 256


def bf16_fused_route(N, L, H, D, gated):
    """csrc/mmf_api.hip amil_bf16_forward_impl and stack_cvt_bf16: the `small` gated head's bf16 forward is one fused kernel (fused_fwd2_ok /
    fused_fwd_ok, mmf_amil_bf16*.hip), its K-dh the dh2 form (dh2_bf16_ok); every other head takes the unfused route."""
    return bool(gated) and H == 256 and D == 256 and L % 128 == 0 and (N + 127) // 128 <= 4096


def dh2_bf16_ok(N, H, D, gated):
    """csrc/mmf_amil_bf16_dh2.hip dh2_bf16_ok"""
    return bool(gated) and H == 256 and D == 256 and N > 0


# ---- plans ----------------------------------------------------------------------------------------------------------
def plan(N, head="small", gated=True, attn_dropout=False, train=False, concurrent=False, grouped=False, dtype="fp32",
         radio_nseg=0):
    """The large-bag kernel instantiations of one training step (forward + backward) over N rows (grouped: the window's
    total rows), as a frozenset of plan keys (module docstring).  attn_dropout: the model was built with dropout=True
    (attention dropout is on in train mode only); train: train mode (the projection's dropout 0.25).  radio_nseg > 1:
    the radiology head's grouped step, whose stack is the `small` head's over reduce_dim's output."""
    L, H, D = HEADS["small" if radio_nseg else head]
    N = int(N)
    p_h = train
    p_att = train and attn_dropout
    keys = set()
    if dtype == "bf16":
        assert not grouped and not radio_nseg
        if bf16_fused_route(N, L, H, D, gated):
            return frozenset()
        if pick_bm(N, H // 256) == 256:
            keys.add(("linear_bf16", 256))
        if pick_bm(N, gate_parts_bf16(D, gated)) == 256:
            keys.add(("gate_bf16", 256))
        if not dh2_bf16_ok(N, H, D, gated):
            keys.add(("dh_bf16", bool(gated)))
        return frozenset(keys)

    ntn = H // 256
    wide = bool(use_wide_tiles(N, H))
    if grouped or radio_nseg:
        if radio_nseg and use_wide_tiles(N, L):     # reduce_dim: LinearParams zeroed, so whole blocks, not concurrent
            keys.add(("linear", "wide", pick_wide_rows(N, L // 256, False, False, LINEAR_MAX_ROWS), False))
        if wide:
            # launch_linear_seg (csrc/mmf_amil_fwd.hip): the per-bag-mask instantiation only with dropout
            keys.add(("linear", "wide", pick_wide_rows(N, ntn, True, concurrent, LINEAR_MAX_ROWS), p_h))
            # the grouped chain cannot fuse K-prep (dh_plan(dp, false), csrc/mmf_api.hip): whole blocks only
            keys.add(("dh", "wide_seg", pick_wide_rows(N, ntn, False, concurrent, DH_MAX_ROWS)))
        if tn_tile_dim(N) == 256:
            keys.add(("tn", 256, 2 if p_att else 0))        # launch_tn_grid (csrc/mmf_amil_bwd.hip)
        else:
            keys.add(("tn", 128, 2 if p_att else None))
        keys |= gate_keys(N, D, gated, bool(p_att))
        return frozenset(keys)

    fused = bool(dh_fused(N, H, concurrent))
    if wide:
        keys.add(("linear", "wide", pick_wide_rows(N, ntn, True, concurrent, LINEAR_MAX_ROWS), False))
        if not fused:
            keys.add(("dh", "prep", "own launch"))
        rows = pick_wide_rows(N, ntn, dh_allow_half(fused), concurrent, DH_MAX_ROWS)
        variant = ((2 if gated else 0) + (1 if p_att else 0)) if fused else None
        keys.add(("dh", "wide", rows, fused, variant))
    elif dh_64x128(N, H, D, gated, fused):
        keys.add(("dh", "64x128"))
    if tn_tile_dim(N) == 256:
        keys.add(("tn", 256, 1 if p_att else 0))
    else:
        keys.add(("tn", 128, None))
    keys |= gate_keys(N, D, gated, False)
    return frozenset(keys)


def gate_keys(N, D, gated, seg_masks):
    """The gate forward's plan keys; seg_masks: the grouped step with attention dropout (launch_gate_fwd_seg)"""
    kind = int(gate_kind(N, D, gated))
    return {GATE_64: set(), GATE_128: {("gate", "128")}, GATE_MIXED: {("gate", "mixed", seg_masks)}}[kind]


def cover_keys(keys):
    """The keys a size table must reach, from plan keys.  Not every instantiation is required, only every tile mechanic:
      * fused K-dh: every height, and each of the 4 variants at a half-block and at a whole-block height (not all 44);
      * K-dh after its own K-prep (bags above ~50k rows): that route once, not each of its heights;
      * the grouped projection with per-bag masks: a half-block and a whole-block height (the mask-free instantiation
        of the same tile, every height, comes from the one-bag cases);
    every other key as it is."""
    out = set()
    for k in keys:
        if k[:2] == ("dh", "wide"):
            _, _, rows, fused, variant = k
            if fused:
                out.add(("dh", "wide", rows, True))
                out.add(("dh", "variant", variant, "half" if rows % 32 else "whole"))
            else:
                out.add(("dh", "wide", "after own prep"))
        elif k[:2] == ("linear", "wide") and k[3]:
            out.add(("linear", "wide_seg_masks", "half" if k[2] % 32 else "whole"))
        else:
            out.add(k)
    return frozenset(out)


@dataclass(frozen=True)
class Config:
    head: str = "small"
    gated: bool = True
    attn_dropout: bool = False
    train: bool = False
    concurrent: bool = False
    grouped: bool = False
    dtype: str = "fp32"
    radio_nseg: int = 0

    def limit(self):
        return RADIO_R_MAX[self.radio_nseg] if self.radio_nseg else N_MAX[self.dtype]

    def plan(self, N):
        return plan(N, self.head, self.gated, self.attn_dropout, self.train, self.concurrent, self.grouped, self.dtype,
                    self.radio_nseg)


def configs():
    """Every configuration the enumeration covers: both heads, gated or not, attention dropout on / off, eval / train,
    the concurrent hint 0 / 1; one bag in fp32 and bf16 storage, the grouped pathology step, the grouped radio step."""
    out = []
    for head in HEADS:
        for gated in (True, False):
            for att in (False, True):
                for train in (False, True):
                    for conc in (False, True):
                        out.append(Config(head, gated, att, train, conc, False, "fp32"))
                        out.append(Config(head, gated, att, train, conc, True, "fp32"))
                    out.append(Config(head, gated, att, train, False, False, "bf16"))
    for nseg in (2, 3, 4):
        for gated in (True, False):
            for att in (False, True):
                for train in (False, True):
                    for conc in (False, True):
                        out.append(Config("small", gated, att, train, conc, True, "fp32", nseg))
    return out


def _signature(cfg, N):
    """The quantities plan() reads from N, for every N of the array at once: plan(N) is a function of these columns."""
    L, H, D = HEADS["small" if cfg.radio_nseg else cfg.head]
    ntn, conc = H // 256, cfg.concurrent
    if cfg.dtype == "bf16":
        return np.stack([pick_bm(N, ntn), pick_bm(N, gate_parts_bf16(D, cfg.gated)), (N + 127) // 128 <= 4096], 1)
    cols = [use_wide_tiles(N, H), tn_tile_dim(N), gate_kind(N, D, cfg.gated), dh_fused(N, H, conc), N >= 13000,
            pick_wide_rows(N, ntn, True, conc, LINEAR_MAX_ROWS), pick_wide_rows(N, ntn, True, conc, DH_MAX_ROWS),
            pick_wide_rows(N, ntn, False, conc, DH_MAX_ROWS)]
    if cfg.radio_nseg:
        cols += [use_wide_tiles(N, L), pick_wide_rows(N, L // 256, False, False, LINEAR_MAX_ROWS)]
    return np.stack([np.asarray(c, np.int64) for c in cols], 1)


_reps = {}


def _representatives(cfg):
    """One N per distinct signature over [1, limit], the smallest; cached per the columns' inputs."""
    key = (cfg.head if not cfg.radio_nseg else "radio", cfg.concurrent, cfg.dtype, cfg.radio_nseg,
           cfg.gated)
    if key not in _reps:
        N = np.arange(1, cfg.limit() + 1, dtype=np.int64)
        _, first = np.unique(_signature(cfg, N), axis=0, return_index=True)
        _reps[key] = sorted(int(N[i]) for i in first)
    return _reps[key]


def reachable(cfg):
    """{plan key: smallest N that reaches it} for one configuration, over every N up to the ABI's limit."""
    out = {}
    for n in _representatives(cfg):
        for k in cfg.plan(n):
            out.setdefault(k, n)
    return out


def all_reachable():
    """{cover key: (config, N)} over every configuration and every N up to the ABI's limit."""
    out = {}
    for cfg in configs():
        for k, n in reachable(cfg).items():
            for c in cover_keys({k}):
                out.setdefault(c, (cfg, n))
    return out


# ---- the GPU size tables --------------------------------------------------------------------------------------------
# One bag, fp32, through model.nll_step (route "step"), model -> NLLSurvLoss -> backward ("autograd"), or the headline's
# BagsInFlight(model, 2) ("flight").  K-dh variants: 0 ungated, 1 ungated + attention dropout, 2 gated, 3 gated +
# attention dropout; "half": the height ends in a 16-row half block.  The `big` head (two 256-column tiles per row tile)
# reaches each height at half the rows.
# (N, head, gated, dropout, train, concurrent, route, the plan it is meant to reach: projection / K-dh rows)
ONE_BAG = [
    (16383, "small", True, False, True, False, "step", "one row below the wide tiles: 64 x 128 K-dh tiles"),
    (16384, "small", True, False, True, False, "step", "exactly the wide threshold: 64 / 64, variant 2"),
    (16385, "small", False, True, True, False, "step", "one row above: 80 / 80, variant 1 (half), ends in the half block"),
    (8192, "big", False, False, False, False, "step", "big at exactly the wide threshold: 64 / 64, variant 0, eval"),
    (8225, "big", False, True, True, False, "step", "80 / 80, variant 1 (half), ends in the half block"),
    (10301, "big", True, True, True, False, "step", "96 / 96, variant 3 (whole)"),
    (12305, "big", False, False, False, False, "step", "112 / 112, variant 0 (half), ends in the half block, eval"),
    (14401, "big", False, True, True, False, "step", "128 / 128, variant 1 (whole)"),
    (16401, "big", True, True, True, False, "step", "144 / 144, variant 3 (half), ends in the half block"),
    (18500, "big", False, False, True, False, "step", "160 / 160, variant 0 (whole)"),
    (20577, "big", False, True, True, False, "step", "176 / 176, variant 1 (half), ends in the half block"),
    (22600, "big", True, False, True, False, "step", "192 / 192, variant 2 (whole)"),
    (24737, "big", True, True, True, False, "autograd", "208 / 208, variant 3 (half), ends in the half block"),
    (26700, "big", False, False, False, False, "step", "224 / 224, variant 0 (whole), eval"),
    (29030, "big", True, False, True, False, "step", "240 / 80, variant 2 (half); ends in both half blocks"),
    (24625, "small", True, False, False, False, "autograd", "112 / 112, variant 2 (half), ends in the half block, eval"),
    (60001, "small", True, False, True, False, "step", "240-row projection; K-prep as its own launch, 128-row K-dh"),
    (50000, "small", True, False, True, True, "step", "the headline: concurrent hint, 224 / 224, variant 2"),
    (50000, "small", True, False, True, True, "flight", "the headline through BagsInFlight(model, 2)"),
]

# Grouped pathology windows through model.nll_step_group; bag boundaries inside tiles, in half blocks and on tile edges.
# (sizes, head, gated, K, train, dropout, the plan: projection / grouped K-dh rows)
G64 = [300 + (53 * g) % 97 for g in range(64)]
G64[5] = 1
GROUPED = [
    ([4096, 1, 8287, 1, 3999], "small", True, 4, True, True,
     "16,384 rows: 64 (masks) / 64, TN mode 2; a bag edge on a tile edge, one-row bags"),
    ([8070, 1, 8350], "small", False, 8, True, False, "16,421 rows: 80 (masks, a bag edge in the half block) / 96; ungated"),
    (G64, "big", True, 4, True, True, "G = 64, 21,791 rows: 176 (masks) / 192, TN mode 2, a one-row bag"),
    ([12000, 1, 12577], "small", True, 8, False, False, "24,578 rows, eval: 112 / 128"),
    ([9935, 1, 6466], "big", False, 4, True, True, "16,402 rows: 144 (masks, a bag edge in the half block) / 160"),
    ([8064, 8193, 1, 10442], "big", True, 8, True, True, "26,700 rows: 224 (masks) / 224, a bag edge on a tile edge"),
    ([5000, 5000, 1, 22700], "small", True, 4, True, True,
     "32,701 rows: the gate's tall and short tiles in one launch with per-bag masks, a bag edge inside a tall tile (row 5,000) "
     "and inside a short one (row 10,000); 128 (masks) / 128"),
    ([300, 1, 200], "small", True, 4, True, True, "501 rows: the 128 x 128 TN tile with per-bag masks (mode 2)"),
]

# Grouped radio windows through MIL_Attention_fc_surv_radio.nll_step_group.  (sizes, n_mod, gated, K, train, dropout, plan)
RADIO = [
    ([450] * 40, 4, True, 4, True, True, "18,000 rows: wide reduce_dim; 80 (masks) / 96, TN mode 2"),
]

# bf16 storage, unfused route, through the autograd surface.  (N, head, gated, dropout, train, the plan)
BF16 = [
    (33001, "small", False, False, False, "small ungated, eval: 256-row linear / gate tiles, dh_bf16<false>"),
    (16501, "big", True, True, True, "big gated, train: 256-row linear / gate tiles, dh_bf16<true>"),
]


def table_keys():
    """{cover key: [case descriptions]} of every case in the tables."""
    out = {}

    def add(keys, tag):
        for k in cover_keys(keys):
            out.setdefault(k, []).append(tag)
    for N, head, gated, dropout, train, conc, route, why in ONE_BAG:
        add(plan(N, head, gated, dropout, train, conc), f"one bag N={N} {head}: {why}")
    for sizes, head, gated, K, train, dropout, why in GROUPED:
        add(plan(sum(sizes), head, gated, dropout, train, False, grouped=True), f"window {sum(sizes)} {head}: {why}")
    for sizes, nmod, gated, K, train, dropout, why in RADIO:
        add(plan(sum(sizes), "small", gated, dropout, train, False, grouped=True, radio_nseg=nmod),
            f"radio window {sum(sizes)}: {why}")
    for N, head, gated, dropout, train, why in BF16:
        add(plan(N, head, gated, dropout, train, dtype="bf16"), f"bf16 N={N} {head}: {why}")
    return out
