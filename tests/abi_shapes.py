"""The shapes the C ABI admits, restated for the tests (helper module, not collected by pytest).

The GPU suite runs the dimensions of the three shipped models; include/mmf_amil.h and the check_* functions of
csrc/mmf_api.hip admit far more.  For the scorer, the dense layer and the stack this module

  * restates the admission rule (`*_rule(case)` -> the return code the library gives the shape before any launch), each
    with the header line and the check it restates,
  * names the shape classes the rule makes reachable (`*_tags(case)`: what a case exercises; `REQUIRED[...]`: what the
    tables must exercise between them) -- K-loop chunk counts, ragged or full column / attention-dim tiles, row counts
    around a tile edge, segment counts, and the values tests/test_gpu_abi_shapes.py is asked to run,
  * holds the case tables that file runs.  Each case says what it is there for.

tests/test_abi_shapes_cpu.py pins the rules to the library where a refusal returns before any HIP call, the planner
restated here to the library's, and the tables to REQUIRED: every class has a case, and every case is the only one of
its table for some class, so that dropping any case names the class it leaves uncovered.

K loops run in chunks of KC = 32 (csrc/mmf_gemm_core.h:31).  Chunk classes:
  one    1 chunk: prologue and epilogue of the main loop, no steady state
  odd    an odd count >= 3: (K / KC) % 4 != 0, the launchers stay out of the deep-prefetch loop (gemm_mainloop_deep)
  four   exactly 4: one round of the deep loop on a short grid
  mult4  a multiple of 4 above 4: the deep loop's steady state

The tensor-fusion tail (mmf_xfusion_infer_group, mmf_xfusion_group_forward / _backward) has a table of its own, XFUSION,
run by tests/test_gpu_xfusion_shapes.py.  Its kernels are VALU code with fixed work units, restated below beside
XFusion: classes are named after what a dimension does to a work unit -- lanes of a wave_dot round, rows of a dW block,
passes and wave quarters of the dkr launch, chunks a lane of dense_segs_group_kernel keeps, slices and column blocks of
dense_bwd_kernel, which layer sizes the shared backward buffers, patient groups and shares.
"""
from __future__ import annotations

from dataclasses import dataclass

OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN = 0, -1, -2, -3      # csrc/mmf_common.h:29-32
ERR_WORKSPACE = -4                                       # csrc/mmf_common.h:33
KC = 32
SKC = 16                                                 # csrc/mmf_gemm_split.h:27
TILE = 64                                                # rows and columns of the small-shape tiles (TileNT64, K-nn, K-dh)


def chunks(K):
    n = K // KC
    if n == 1:
        return "one"
    if n == 4:
        return "four"
    if n % 2 == 1:
        return "odd"
    if n % 4 == 0:
        return "mult4"
    return "even"


def rows_class(M, tile=TILE):
    """Rows against one tile's height."""
    return {1: "1", tile - 1: "tile-1", tile: "tile", tile + 1: "tile+1"}.get(M, "blocks" if M > tile + 1 else "few")


# ---- mmf_linear_forward -----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LinFwd:
    M: int
    N: int
    nseg: int
    kseg: int
    act: int = 0                 # MMF_ACT_*
    drop_p: float = 0.0
    ws: bool = False             # with workspace and tick words: the K-split plan, where the planner splits
    misalign: str = ""           # "y" / "bias": that pointer 4 bytes off a 16-byte boundary
    why: str = ""

    @property
    def K(self):
        return self.nseg * self.kseg


def linear_forward_rule(c):
    """include/mmf_amil.h "Dense layer on MFMA"; csrc/mmf_api.hip mmf_linear_forward, csrc/mmf_amil_fwd.hip
    launch_linear_impl -- in the library's order."""
    if c.nseg < 1 or c.nseg > 4 or c.act < 0 or c.act > 4 or not 0.0 <= c.drop_p < 1.0:
        return ERR_ARG
    if c.M * c.kseg * 4 >= 2**31 or c.N * c.K * 4 >= 2**31:
        return ERR_SHAPE
    if c.misalign:
        return ERR_ALIGN                                  # x segments, W, y, a non-null bias: 16 bytes
    if c.K % KC != 0 or (c.nseg > 1 and c.kseg % KC != 0):
        return ERR_SHAPE
    if c.N % 4 != 0:
        return ERR_SHAPE                                  # float4 stores of y, float4 loads of the bias
    return OK


def use_wide_tiles(M, N, split=0):
    return N % 256 == 0 and M * (N // 256) >= (80 * 256 if split else 64 * 256)      # csrc/mmf_amil_fwd.hip use_wide_tiles


def use_big_tiles(M, N):
    return (M // 128) * ((N + 127) // 128) >= 256                                    # csrc/mmf_amil_fwd.hip use_big_tiles


def linear_ksplit(M, N, K, nseg, kseg):
    """csrc/mmf_amil_fwd.hip linear_ksplit (no tuning overrides): the K split of a short grid of 64 x 64 tiles."""
    if M <= 0 or N % 4 != 0 or K % KC != 0 or use_wide_tiles(M, N) or use_big_tiles(M, N):
        return 1
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    nk = K // KC
    if nseg > 1 and kseg % (4 * KC) != 0:
        return 1
    if tiles > 128:
        return 1
    for S in (4, 2):
        if tiles * S <= 512 and nk % (4 * S) == 0 and nk // S >= 8:
            return S
    return 1


def linear_forward_tags(c):
    code = linear_forward_rule(c)
    if code != OK:
        what = ("misaligned " + c.misalign) if c.misalign else f"N={c.N} K={c.K} nseg={c.nseg} kseg={c.kseg} act={c.act}"
        return {("refused", code, what)}
    t = {("N", c.N), ("M", c.M), ("rows", rows_class(c.M)), ("column tile", "ragged" if c.N % TILE else "full")}
    S = linear_ksplit(c.M, c.N, c.K, c.nseg, c.kseg) if c.ws else 1
    if S > 1:
        t |= {("ksplit", S), ("ksplit shape", (c.M, c.N, c.K))}
    elif c.nseg == 1:
        t |= {("K", c.K), ("chunks", chunks(c.K))}
    else:
        t |= {("nseg", c.nseg), ("kseg", c.kseg), ("segments", "kseg % 128 != 0" if c.kseg % (4 * KC) else "kseg % 128 == 0")}
    if c.N % TILE:
        t.add(("act on a ragged N", c.act))
    if c.drop_p > 0:
        t.add(("dropout", c.N))
    return t


LINEAR_FORWARD = [
    LinFwd(1, 4, 1, 32, why="one row, one float4 of columns, a one-chunk K loop"),
    LinFwd(63, 36, 1, 96, act=1, drop_p=0.25, why="tile - 1 rows, odd chunk count, ReLU + dropout indices row * 36 + col"),
    LinFwd(64, 64, 1, 128, why="exactly one full tile; four chunks: one round of the deep loop"),
    LinFwd(65, 100, 1, 160, act=2, drop_p=0.25, why="tile + 1 rows, five chunks, tanh + dropout on N = 100"),
    LinFwd(130, 260, 1, 256, act=3, why="three row tiles, five column tiles (the last 4 wide), eight chunks, sigmoid"),
    LinFwd(5, 36, 1, 64, act=4, why="SELU on a ragged N; two chunks"),
    LinFwd(63, 100, 2, 32, why="two segments of one chunk each"),
    LinFwd(65, 36, 3, 96, why="three segments of three chunks: kseg % 128 != 0, no deep loop, no K-split"),
    LinFwd(130, 260, 4, 128, why="four segments of four chunks: the deep loop over segment edges"),
    LinFwd(65, 100, 1, 512, ws=True, why="K-split two ways: 16 chunks"),
    LinFwd(130, 36, 1, 768, ws=True, act=1, drop_p=0.25, why="K-split two ways: 24 chunks, ragged N, ReLU + dropout in the last arriver"),
    LinFwd(64, 100, 1, 1024, ws=True, why="K-split four ways: 32 chunks, ragged N"),
    # refused
    LinFwd(5, 1, 1, 32, why="N % 4: the st4 at column 0 would cover columns 1..3"),
    LinFwd(5, 6, 1, 32, why="N % 4: the st4 at column 4 would write two floats into the next row"),
    LinFwd(5, 30, 1, 32, why="N % 4: the issue's example, the st4 at column 28"),
    LinFwd(5, 36, 1, 48, why="K % 32"),
    LinFwd(5, 36, 2, 48, why="K = 96 but kseg % 32 != 0: a chunk would straddle two segments"),
    LinFwd(5, 36, 5, 32, why="nseg > 4"),
    LinFwd(5, 36, 1, 32, act=5, why="unknown activation"),
    LinFwd(5, 36, 1, 32, misalign="y", why="y is stored as float4"),
    LinFwd(5, 36, 1, 32, misalign="bias", why="the bias is loaded as float4"),
]

REQUIRED_LINEAR_FORWARD = (
    {("K", k) for k in (32, 96, 128, 160)} | {("chunks", c) for c in ("one", "odd", "four", "mult4")}
    | {("N", n) for n in (4, 36, 64, 100, 260)} | {("column tile", c) for c in ("ragged", "full")}
    | {("M", m) for m in (1, 63, 64, 65, 130)} | {("rows", r) for r in ("1", "tile-1", "tile", "tile+1", "blocks")}
    | {("nseg", n) for n in (2, 3, 4)} | {("kseg", k) for k in (32, 96, 128)}
    | {("segments", s) for s in ("kseg % 128 != 0", "kseg % 128 == 0")}
    | {("act on a ragged N", a) for a in range(5)} | {("dropout", 100), ("dropout", 36)}
    | {("ksplit", 2), ("ksplit", 4)} | {("ksplit shape", s) for s in ((65, 100, 512), (130, 36, 768), (64, 100, 1024))}
    | {("refused", ERR_SHAPE, f"N={n} K=32 nseg=1 kseg=32 act=0") for n in (1, 6, 30)}
    | {("refused", ERR_SHAPE, "N=36 K=48 nseg=1 kseg=48 act=0"), ("refused", ERR_SHAPE, "N=36 K=96 nseg=2 kseg=48 act=0"),
       ("refused", ERR_ARG, "N=36 K=160 nseg=5 kseg=32 act=0"), ("refused", ERR_ARG, "N=36 K=32 nseg=1 kseg=32 act=5"),
       ("refused", ERR_ALIGN, "misaligned y"), ("refused", ERR_ALIGN, "misaligned bias")})


# ---- mmf_linear_backward ----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LinBwd:
    M: int
    N: int
    nseg: int
    kseg: int
    db: bool = True
    dx: bool = False
    why: str = ""

    @property
    def K(self):
        return self.nseg * self.kseg


def linear_backward_rule(c):
    """include/mmf_amil.h mmf_linear_backward; csrc/mmf_api.hip mmf_linear_backward -- all before the first launch."""
    if c.nseg < 1 or c.nseg > 4 or (c.dx and c.nseg != 1):
        return ERR_ARG
    if c.N % 4 != 0 or c.kseg % 4 != 0:
        return ERR_SHAPE
    if c.dx and c.N % KC != 0:
        return ERR_SHAPE                                  # dx = dy . W runs the NN GEMM over K = N in 32-chunks
    if c.M * max(c.N, c.kseg) * 4 >= 2**31 or c.N * c.K * 4 >= 2**31:
        return ERR_SHAPE
    return OK


def tn_splits(K, total_tiles, tile):
    """csrc/mmf_amil_bwd.hip tn_splits (no tuning overrides)."""
    splits = (256 if tile == 256 else 512) // max(total_tiles, 1)
    return max(1, min(splits, (K + 127) // 128))


def linear_bwd_splits(M, N, K):
    """csrc/mmf_api.hip linear_bwd_splits; 128 x 128 TN tiles below 12,288 rows (tn_tile_dim)."""
    td = 256 if M >= 12288 else 128
    return tn_splits(M, ((N + td - 1) // td) * ((K + td - 1) // td), td)


def linear_backward_tags(c):
    code = linear_backward_rule(c)
    if code != OK:
        return {("refused", code, f"N={c.N} nseg={c.nseg} kseg={c.kseg} dx={int(c.dx)}")}
    t = {("M", c.M), ("nseg", c.nseg), ("db", c.db), ("splits", "several" if linear_bwd_splits(c.M, c.N, c.K) > 1 else "one")}
    if c.dx:
        t |= {("dx N", c.N), ("dx kseg", c.kseg), ("dx chunks", chunks(c.N))}
    else:
        t |= {("N", c.N), ("kseg", c.kseg)}
    return t


LINEAR_BACKWARD = [
    LinBwd(1, 4, 1, 4, why="one instance, one float4 each way: a TN tile that is almost all zero fill"),
    LinBwd(3, 36, 2, 36, db=False, why="k_per_split rounds 3 up to 4; two segments 36 columns apart in dW; no db"),
    LinBwd(5, 100, 3, 100, why="three segments, ragged 128-tiles both ways"),
    LinBwd(64, 256, 4, 1024, why="four segments of eight column tiles, two full row tiles, two chunks"),
    LinBwd(1000, 36, 1, 100, why="8 splits of 128 instances (the last 104): slabs + reduce, db from the split column sums"),
    LinBwd(65, 32, 1, 36, dx=True, why="dx over a one-chunk K loop, ragged 36-wide output tile, tile + 1 rows"),
    LinBwd(3, 96, 1, 100, dx=True, db=False, why="dx over three chunks, two output tiles (the second 36 wide)"),
    LinBwd(64, 256, 1, 36, dx=True, why="dx over eight chunks, one full row tile"),
    # refused
    LinBwd(5, 36, 1, 6, why="kseg % 4"),
    LinBwd(5, 6, 1, 36, why="N % 4"),
    LinBwd(5, 36, 1, 36, dx=True, why="dx needs N % 32 == 0"),
    LinBwd(5, 32, 2, 36, dx=True, why="dx of a concatenated input is not provided"),
]

REQUIRED_LINEAR_BACKWARD = (
    {("N", n) for n in (4, 36, 100, 256)} | {("kseg", k) for k in (4, 36, 100, 1024)}
    | {("M", m) for m in (1, 3, 5, 64, 65, 1000)} | {("nseg", n) for n in (1, 2, 3, 4)} | {("db", True), ("db", False)}
    | {("splits", "one"), ("splits", "several")}
    | {("dx N", n) for n in (32, 96, 256)} | {("dx kseg", k) for k in (36, 100)}
    | {("dx chunks", c) for c in ("one", "odd", "mult4")}
    | {("refused", ERR_SHAPE, "N=36 nseg=1 kseg=6 dx=0"), ("refused", ERR_SHAPE, "N=6 nseg=1 kseg=36 dx=0"),
       ("refused", ERR_SHAPE, "N=36 nseg=1 kseg=36 dx=1"), ("refused", ERR_ARG, "N=32 nseg=2 kseg=36 dx=1")})


# ---- mmf_attn_net_forward / _backward -----------------------------------------------------------------------------------
@dataclass(frozen=True)
class Attn:
    N: int
    H: int
    D: int
    gated: bool
    dropout: bool = False
    dx: bool = True
    why: str = ""


def attn_rule(c):
    """include/mmf_amil.h "The attention scorer on its own": H % 32 == 0, D % 32 == 0; csrc/mmf_api.hip check_attn."""
    if c.N < 1 or c.H % KC != 0 or c.D % 32 != 0:
        return ERR_SHAPE
    if c.N * max(c.H, 2 * c.D) * 4 >= 2**31:
        return ERR_SHAPE
    return OK


def attn_tags(c):
    code = attn_rule(c)
    if code != OK:
        return {("refused", code, f"N={c.N} H={c.H} D={c.D}")}
    per_tile = 64 if c.gated else 128          # attention dims of one K-gate tile (csrc/mmf_amil_fwd.hip gate_parts)
    return {("H", c.H), ("chunks", chunks(c.H)), ("D", c.D), ("N", c.N), ("rows", rows_class(c.N)),
            ("gated" if c.gated else "ungated", "ragged D tile" if c.D % per_tile else "full D tile"),
            ("TN rows M = 2D" if c.gated else "TN rows M = D", (2 if c.gated else 1) * c.D),
            ("dropout", c.dropout), ("dx", c.dx)}


ATTN = [
    Attn(1, 32, 32, True, why="one instance, one chunk, half a gated tile (TN: 64 stacked rows of a 128 tile)"),
    Attn(63, 96, 96, False, dropout=True, why="three chunks, 96 of an ungated tile's 128 dims, the a-branch mask"),
    Attn(65, 128, 160, True, dropout=True, dx=False, why="one deep round; 2.5 gated tiles (TN: 320 rows); both masks; no dx"),
    Attn(777, 160, 256, False, dx=False, why="five chunks, two full ungated tiles, 13 row tiles, 7 TN splits"),
    Attn(777, 128, 256, True, dropout=True, why="four full gated tiles with both masks and dx"),
    Attn(65, 96, 96, True, why="1.5 gated tiles (TN: 192 rows against 128 / 256 tiles)"),
    # refused
    Attn(5, 48, 32, True, why="H % 32"),
    Attn(5, 32, 48, True, why="D % 32"),
    Attn(0, 32, 32, True, why="N < 1"),
]

REQUIRED_ATTN = (
    {("H", h) for h in (32, 96, 128, 160)} | {("chunks", c) for c in ("one", "odd", "four")}
    | {("D", d) for d in (32, 96, 160, 256)} | {("N", n) for n in (1, 63, 65, 777)}
    | {("rows", r) for r in ("1", "tile-1", "tile+1", "blocks")}
    | {(g, t) for g in ("gated", "ungated") for t in ("ragged D tile", "full D tile")}
    | {("TN rows M = 2D", m) for m in (64, 192, 320)}
    | {("dropout", True), ("dropout", False), ("dx", True), ("dx", False)}
    | {("refused", ERR_SHAPE, "N=5 H=48 D=32"), ("refused", ERR_SHAPE, "N=5 H=32 D=48"), ("refused", ERR_SHAPE, "N=0 H=32 D=32")})


# ---- the stack: mmf_amil_forward / _backward / _nll_step, the grouped entry points, bf16 storage --------------------------
@dataclass(frozen=True)
class Stack:
    L: int
    H: int
    D: int
    gated: bool
    bf16: bool = False
    why: str = ""

    @property
    def size(self):
        return (self.L, self.H, self.D)


def stack_rule(c):
    """include/mmf_amil.h mmf_amil_desc and "bf16-storage variant"; csrc/mmf_api.hip check_desc / check_desc_bf16."""
    if c.L % KC != 0 or c.H % KC != 0 or c.H not in (256, 512, 1024) or c.D % 128 != 0:
        return ERR_SHAPE
    if c.bf16 and (c.L % 64 != 0 or c.H % 256 != 0):
        return ERR_SHAPE
    return OK


def split_core(L):
    """csrc/mmf_amil_fwd.hip launch_linear_impl: gemm = MMF_GEMM_BF16X3 takes the split-operand tiles only when
    K % (4 * SKC) == 0; the projection of any other L runs the exact-fp32 tiles whatever the mode."""
    return L % (4 * SKC) == 0


def bf16_fused2(c):
    """csrc/mmf_amil_bf16_fwd2.hip fused_fwd2_ok: the two-workgroup fused forward, whose K loop steps 128 wide."""
    return c.gated and c.H == 256 and c.D == 256 and c.L % 128 == 0


def stack_tags(c):
    code = stack_rule(c)
    if code != OK:
        return {("refused", code, f"L={c.L} H={c.H} D={c.D} bf16={int(c.bf16)}")}
    t = {("shape", (c.L, c.H, c.D, c.gated))}
    if c.bf16:
        t.add(("bf16 forward", "fused, two-step L" if bf16_fused2(c) and c.L == 128 else
               "not the two-workgroup fused form" if c.gated and c.H == 256 and c.D == 256 else "unfused kernels"))
        return t
    per_tile = 64 if c.gated else 128
    t |= {("L chunks", chunks(c.L)), ("H", c.H), ("D tiles", c.D // per_tile),
          ("bf16x3 projection", "split core" if split_core(c.L) else "exact-fp32 fallback")}
    return t


STACK_F32 = [
    Stack(32, 256, 128, False, why="a one-chunk projection; D = 128 ungated: a single full gate tile"),
    Stack(96, 256, 128, True, why="three chunks: no deep loop, no split core; two gated tiles"),
    Stack(160, 512, 640, True, why="five chunks; D = 640: ten gated tiles, K-dh over 40 chunks"),
    Stack(32, 1024, 384, False, why="H = 1024 with a short L: 16 column tiles of a one-chunk loop, the widest pooling rows"),
    Stack(128, 1024, 128, True, why="four chunks: one deep round, the split core's shortest loop"),
    # refused
    Stack(128, 256, 96, True, why="D % 128"),
    Stack(128, 768, 128, True, why="H outside {256, 512, 1024}"),
    Stack(48, 256, 128, True, why="L % 32"),
]
STACK_BAGS = (1, 65, 300)           # rows of one bag: one row, tile + 1, five tiles ending inside one

STACK_BF16 = [
    Stack(64, 256, 128, True, bf16=True, why="one 64-wide K step; D = 128: one gated bf16 tile"),
    Stack(192, 256, 256, True, bf16=True, why="L % 128 != 0: not the two-workgroup fused forward"),
    Stack(128, 256, 256, True, bf16=True, why="the fused route with a two-step L"),
    Stack(64, 512, 384, False, bf16=True, why="ungated, D = 384 against 256-dim tiles, H = 512"),
    Stack(96, 256, 128, True, bf16=True, why="refused: L % 64"),
]
BF16_BAGS = (65, 300)

# grouped entry points: (entry point, sizes of the window, (L, H, D), gated)
GROUPED = [
    ("mmf_amil_nll_step_group", (1, 65, 300), (96, 256, 128), False),
    ("mmf_amil_infer_group", (1, 65, 300), (96, 256, 128), False),
    ("mmf_amil_nll_step_group", (1, 65, 300), (160, 512, 640), True),
]

REQUIRED_STACK = (
    {("shape", s) for s in ((32, 256, 128, False), (96, 256, 128, True), (160, 512, 640, True), (32, 1024, 384, False),
                            (128, 1024, 128, True))}
    | {("L chunks", c) for c in ("one", "odd", "four")} | {("H", h) for h in (256, 512, 1024)}
    | {("D tiles", 1), ("D tiles", 10)} | {("bf16x3 projection", "split core"), ("bf16x3 projection", "exact-fp32 fallback")}
    | {("refused", ERR_SHAPE, "L=128 H=256 D=96 bf16=0"), ("refused", ERR_SHAPE, "L=128 H=768 D=128 bf16=0"),
       ("refused", ERR_SHAPE, "L=48 H=256 D=128 bf16=0")})
REQUIRED_BF16 = (
    {("shape", s) for s in ((64, 256, 128, True), (192, 256, 256, True), (128, 256, 256, True), (64, 512, 384, False))}
    | {("bf16 forward", f) for f in ("fused, two-step L", "not the two-workgroup fused form", "unfused kernels")}
    | {("refused", ERR_SHAPE, "L=96 H=256 D=128 bf16=1")})

# ---- the tensor-fusion tail: mmf_xfusion_infer_group, mmf_xfusion_group_forward / _backward -------------------------------
GROUP_MAX = 64                                           # include/mmf_amil.h MMF_GROUP_MAX
XF_S1 = 17                                               # sdim + 1 (csrc/mmf_xfusion_group.hip:19, csrc/mmf_mlp.hip:433)
XB_PG = 16                                               # csrc/mmf_xfusion_group.hip:20: patients per workgroup, dkr launch
XB_NC = 512                                              # csrc/mmf_xfusion_group.hip:21: rows of encoder1 staged per pass
XB_ROWS = 32                                             # csrc/mmf_xfusion_group.hip:22: rows of dWe1 per workgroup
DENSE_SEGS_MAXC = 24                                     # csrc/mmf_mlp.h:93: chunks of 64 weights a lane keeps
XF_CAP = 64 * DENSE_SEGS_MAXC                            # 1536
WAVE_DOT_ROUND = 256                                     # csrc/mmf_mlp.hip:212: one float4 per lane and round
DENSE_BWD_DX_COLS, DENSE_BWD_DW_COLS = 64, 256           # csrc/mmf_mlp.hip:689: columns of a dx / a dW block


def group_shares(G):
    return min(G, 4)                                     # csrc/mmf_mlp.hip:573


@dataclass(frozen=True)
class XFusion:
    m: int
    dim: int
    mmhid1: int
    mmhid2: int
    nhid: int
    G: int
    lddhid_pad: int = 0          # dhid's leading dimension is nhid + lddhid_pad
    why: str = ""
    sdim: int = 16
    seed: int = 1                # of the weights and the patients' masks, chosen on the CPU (tests/xfusion_cases.py): no ReLU
                                 # pre-activation of the fp64 oracle within KINK of 0, no patient or gradient all zero

    @property
    def K2(self):
        return self.mmhid1 + self.m * self.dim

    @property
    def E(self):
        return (self.sdim + 1) ** self.m

    @property
    def lddhid(self):
        return self.nhid + self.lddhid_pad


def xfusion_window_ok(m, sdim, mmhid1, G):
    """csrc/mmf_api.hip xfusion_shape_ok: all that mmf_xfusion_group_infer_workspace_bytes(m, sdim, mmhid1, G) sees."""
    return 2 <= m <= 3 and sdim == 16 and 1 <= mmhid1 <= XF_CAP and 1 <= G <= GROUP_MAX


def xfusion_infer_rule(c):
    """include/mmf_amil.h mmf_xfusion_infer_group ("Returns MMF_ERR_SHAPE for m outside 2..3, sdim != 16, dim % 4 != 0,
    mmhid1 + m * dim or mmhid2 > 1536, G outside 1..MMF_GROUP_MAX"); csrc/mmf_api.hip xfusion_shape_ok and the checks of
    mmf_xfusion_infer_group.  nhid has no cap here: classifier[0]'s rows are the grid, its K is mmhid2."""
    if not xfusion_window_ok(c.m, c.sdim, c.mmhid1, c.G):
        return ERR_SHAPE
    if c.dim < 4 or c.dim % 4 != 0 or c.mmhid2 < 1 or c.nhid < 1:
        return ERR_SHAPE
    if c.K2 > XF_CAP or c.mmhid2 > XF_CAP:
        return ERR_SHAPE
    return OK


def xfusion_train_rule(c):
    """include/mmf_amil.h mmf_xfusion_group_forward / _backward ("... mmhid1 % 4 != 0, mmhid1 + m * dim, mmhid2 or nhid >
    1536, G outside 1..MMF_GROUP_MAX, lddhid < nhid"); csrc/mmf_api.hip xfusion_train_shape, and mmf_xfusion_group_backward
    for lddhid."""
    if xfusion_infer_rule(c) != OK:
        return ERR_SHAPE
    if c.mmhid1 % 4 != 0 or c.nhid > XF_CAP:
        return ERR_SHAPE
    if c.lddhid < c.nhid:
        return ERR_SHAPE
    return OK


def _dense_bwd_tags(N, K):
    """dense_bwd_kernel (csrc/mmf_mlp.hip:642-684): a dx block sums N in four slices of (N + 3) / 4, four at a time with a
    scalar remainder loop, over 64 columns of K; a dW block takes 256 columns of K."""
    sl = (N + 3) // 4
    lens = [max(0, min(N, (s + 1) * sl) - s * sl) for s in range(4)]
    t = set()
    if 0 in lens:
        t.add(("dense_bwd N", "empty slices"))
    if any(n % 4 for n in lens):
        t.add(("dense_bwd N", "scalar remainder"))
    if K == 1:
        t.add(("dense_bwd K", "1"))
    elif K % DENSE_BWD_DX_COLS:
        t.add(("dense_bwd K", "% 64 != 0"))
    elif K % DENSE_BWD_DW_COLS:
        t.add(("dense_bwd K", "% 256 != 0"))
    else:
        t.add(("dense_bwd K", "% 256 == 0"))
    return t


def xfusion_tags(c):
    """What a case of XFUSION exercises.  A case the forward-only pass admits and the training pair refuses carries both
    the refusal and the forward-only classes."""
    infer, train = xfusion_infer_rule(c), xfusion_train_rule(c)
    what = f"m={c.m} sdim={c.sdim} dim={c.dim} mmhid1={c.mmhid1} mmhid2={c.mmhid2} nhid={c.nhid} G={c.G} pad={c.lddhid_pad}"
    if infer != OK:
        return {("refused", "both", what)}
    t = {("m", c.m)}
    if train != OK:
        t.add(("refused", "training", what))
    # wave_dot: lane l reads the float4 at 4 l, 4 l + 256, ...
    t.add(("dim", "4: one lane" if c.dim == 4 else "below one round, an idle tail lane" if c.dim < WAVE_DOT_ROUND else
           "256: one full round" if c.dim == WAVE_DOT_ROUND else "just past one round" if c.dim < 2 * WAVE_DOT_ROUND else
           "two rounds or more"))
    # encoder1's rows: XB_ROWS per workgroup of the dW launch, XB_NC per pass of the dkr launch (a wave takes a quarter)
    rows = ("one ragged row block" if c.mmhid1 < XB_ROWS else "several row blocks, the last ragged" if c.mmhid1 % XB_ROWS else
            "whole row blocks")
    passes = ("below one pass" if c.mmhid1 < XB_NC else "512: one full pass" if c.mmhid1 == XB_NC else
              "a second pass inside the first wave's quarter" if c.mmhid1 <= XB_NC + XB_NC // 4 else
              "three passes, the last ragged" if c.mmhid1 > 2 * XB_NC and c.mmhid1 % XB_NC else "other")
    t |= {("mmhid1 rows", rows), ("mmhid1 passes", passes), ("mmhid1 rows", rows, "m", c.m), ("mmhid1 passes", passes, "m", c.m)}
    if c.mmhid1 % 4:
        t.add(("mmhid1", "% 4 != 0: e1's segment of encoder2 unaligned (forward-only)"))
    # dense_segs_group_kernel: lane l keeps W[n][l + 64 c], c < DENSE_SEGS_MAXC
    if c.K2 <= 64:
        t.add(("K2", "one chunk"))
    if c.K2 % 64:
        t.add(("K2", "% 64 != 0"))
    if c.K2 == XF_CAP:
        t.add(("K2", "1536: all 24 chunks full"))
    t.add(("mmhid2", "1" if c.mmhid2 == 1 else "1536" if c.mmhid2 == XF_CAP else "% 4 != 0" if c.mmhid2 % 4 else "% 4 == 0"))
    t.add(("nhid", "1" if c.nhid == 1 else "1536" if c.nhid == XF_CAP else
           "% 4 != 0, lddhid > nhid" if c.nhid % 4 and c.lddhid_pad > 0 else "above the training cap" if c.nhid > XF_CAP else
           "other"))
    t.add(("G", "1" if c.G == 1 else "2..3: group_shares < 4" if group_shares(c.G) < 4 else
           "64" if c.G == GROUP_MAX else "17: a ragged second patient group, G % 4 != 0" if c.G == XB_PG + 1 else "other"))
    if train == OK:
        # carve_xfusion_train (csrc/mmf_api.hip:1443-1457): dpre / tmpb and tmpW are sized by the larger of two layers
        t.add(("dpre / tmpb", "classifier[0] the larger" if c.nhid > c.mmhid2 else "encoder2 the larger"))
        t.add(("tmpW", "classifier[0] the larger" if c.nhid * c.mmhid2 > c.mmhid2 * c.K2 else "encoder2 the larger"))
        t |= _dense_bwd_tags(c.nhid, c.mmhid2) | _dense_bwd_tags(c.mmhid2, c.K2)
    return t


XFUSION = [
    XFusion(2, 4, 4, 1, 1, 1, why="every dimension at its minimum: one-wave grids, K = 1 for classifier[0], one patient", seed=2),
    XFusion(2, 4, 4, 8, 40, 3, 6, why="nhid > mmhid2 and nhid > K2 = 12: classifier[0] sizes dpre, tmpb and tmpW; three patients", seed=1),
    XFusion(3, 20, 20, 6, 7, 5, 1, why="m = 3 on one ragged row block; mmhid2 % 4, nhid % 4 with lddhid = nhid + 1", seed=1),
    XFusion(2, 100, 100, 36, 12, 17, 6, why="m = 2, four row blocks (the last 4 rows); 17 patients: a second patient group of one", seed=1),
    XFusion(3, 4, 516, 8, 4, 4, 6, why="m = 3, 17 row blocks (the last 4 rows) and a second pass of 4 rows: three waves of the dkr launch have empty ranges", seed=1),
    XFusion(2, 4, 1528, 4, 4, 4, 6, why="m = 2, three passes (the last 504 rows); K2 = 1536: all 24 chunks of a lane full", seed=1),
    XFusion(2, 8, 16, 1536, 4, 4, why="mmhid2 = 1536: classifier[0] over 24 full chunks, encoder2's widest grid", seed=1),
    XFusion(2, 8, 16, 4, 1536, 4, 6, why="nhid = 1536: the widest dpre staging of dense_bwd_kernel", seed=1),
    XFusion(2, 260, 32, 16, 8, 1, why="dim = 260: a second wave_dot round of one lane", seed=1),
    XFusion(3, 256, 512, 64, 32, 4, 6, why="the shipped dim and mmhid1 (one round, one pass) with m = 3, narrow behind", seed=1),
    XFusion(2, 8, 8, 8, 8, 64, 6, why="a full window of 64 patients at small dimensions", seed=31),
    # the training pair refuses these three; the forward-only pass admits them
    XFusion(2, 8, 5, 6, 3, 4, why="mmhid1 % 4 != 0: refused for training; forward-only, e1's segment of encoder2 is unaligned", seed=1),
    XFusion(2, 8, 8, 4, 1537, 4, why="nhid = 1537: refused for training; forward-only, nhid has no cap", seed=2),
    XFusion(2, 8, 8, 8, 8, 4, -1, why="lddhid < nhid: refused for training (the forward-only pass has no dhid)"),
    # refused by both
    XFusion(2, 6, 8, 8, 8, 2, why="dim % 4"),
    XFusion(2, 4, 1532, 8, 8, 2, why="K2 = 1540"),
    XFusion(2, 8, 8, 1537, 8, 2, why="mmhid2 = 1537"),
    XFusion(2, 8, 8, 8, 8, 0, why="G = 0"),
    XFusion(2, 8, 8, 8, 8, 65, why="G = 65"),
    XFusion(1, 8, 8, 8, 8, 2, why="m = 1"),
    XFusion(4, 8, 8, 8, 8, 2, why="m = 4"),
    XFusion(2, 8, 8, 8, 8, 2, why="sdim = 8", sdim=8),
]

_XF_REFUSED = "m={} sdim={} dim={} mmhid1={} mmhid2={} nhid={} G={} pad={}"
REQUIRED_XFUSION = (
    {("m", 2), ("m", 3)}
    | {("dim", d) for d in ("4: one lane", "below one round, an idle tail lane", "just past one round", "256: one full round")}
    | {("mmhid1 rows", r) for r in ("one ragged row block", "several row blocks, the last ragged")}
    | {("mmhid1 rows", "several row blocks, the last ragged", "m", m) for m in (2, 3)}
    | {("mmhid1 passes", p) for p in ("a second pass inside the first wave's quarter", "three passes, the last ragged",
                                      "512: one full pass")}
    | {("mmhid1 passes", "a second pass inside the first wave's quarter", "m", 3),
       ("mmhid1 passes", "three passes, the last ragged", "m", 2)}
    | {("mmhid1", "% 4 != 0: e1's segment of encoder2 unaligned (forward-only)")}
    | {("K2", k) for k in ("one chunk", "% 64 != 0", "1536: all 24 chunks full")}
    | {("mmhid2", v) for v in ("1", "% 4 != 0", "1536")}
    | {("nhid", v) for v in ("1", "% 4 != 0, lddhid > nhid", "1536", "above the training cap")}
    | {("dpre / tmpb", s) for s in ("classifier[0] the larger", "encoder2 the larger")}
    | {("tmpW", s) for s in ("classifier[0] the larger", "encoder2 the larger")}
    | {("G", g) for g in ("1", "2..3: group_shares < 4", "17: a ragged second patient group, G % 4 != 0", "64")}
    | {("dense_bwd N", "empty slices"), ("dense_bwd N", "scalar remainder"), ("dense_bwd K", "1"), ("dense_bwd K", "% 64 != 0")}
    | {("refused", "training", _XF_REFUSED.format(2, 16, 8, 5, 6, 3, 4, 0)),
       ("refused", "training", _XF_REFUSED.format(2, 16, 8, 8, 4, 1537, 4, 0)),
       ("refused", "training", _XF_REFUSED.format(2, 16, 8, 8, 8, 8, 4, -1))}
    | {("refused", "both", _XF_REFUSED.format(*v)) for v in (
        (2, 16, 6, 8, 8, 8, 2, 0), (2, 16, 4, 1532, 8, 8, 2, 0), (2, 16, 8, 8, 1537, 8, 2, 0), (2, 16, 8, 8, 8, 8, 0, 0),
        (2, 16, 8, 8, 8, 8, 65, 0), (1, 16, 8, 8, 8, 8, 2, 0), (4, 16, 8, 8, 8, 8, 2, 0), (2, 8, 8, 8, 8, 8, 2, 0))})

TABLES = {
    "XFUSION": (XFUSION, xfusion_tags, REQUIRED_XFUSION),
    "mmf_linear_forward": (LINEAR_FORWARD, linear_forward_tags, REQUIRED_LINEAR_FORWARD),
    "mmf_linear_backward": (LINEAR_BACKWARD, linear_backward_tags, REQUIRED_LINEAR_BACKWARD),
    "mmf_attn_net": (ATTN, attn_tags, REQUIRED_ATTN),
    "mmf_amil (fp32)": (STACK_F32, stack_tags, REQUIRED_STACK),
    "mmf_amil_bf16": (STACK_BF16, stack_tags, REQUIRED_BF16),
}


def uncovered(name, cases=None):
    """The required classes of one entry point that no case of `cases` (default: its table) exercises."""
    table, tags, required = TABLES[name]
    have = set()
    for c in (table if cases is None else cases):
        have |= tags(c)
    return required - have


def accepted(table, rule):
    return [c for c in table if rule(c) == OK]


def refused(table, rule):
    return [c for c in table if rule(c) != OK]
