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

The stack's row cap (stack_row_cap, group_row_cap) is restated beside stack_rule, with a census per chain of every operand
whose size grows with N (census): tests/test_abi_shapes_cpu.py holds each below 2 GiB at the cap the library enforces, and
tests/test_gpu_row_caps.py runs every chain at its cap on the inputs of tests/cap_cases.py.

The tensor-fusion tail (mmf_xfusion_infer_group, mmf_xfusion_group_forward / _backward) has a table of its own, XFUSION,
run by tests/test_gpu_xfusion_shapes.py.  Its kernels are VALU code with fixed work units, restated below beside
XFusion: classes are named after what a dimension does to a work unit -- lanes of a wave_dot round, rows of a dW block,
passes and wave quarters of the dkr launch, chunks a lane of dense_segs_group_kernel keeps, slices and column blocks of
dense_bwd_kernel, which layer sizes the shared backward buffers, patient groups and shares.

The other half of the ABI -- the single-workgroup and one-thread-per-element kernels every training step ends in: the
survival head, nll_surv, Cox, the ranking loss, the hazard head, the highway mix, batch norm, the Adam + L1 step, abs_sum and
the dense backward -- has one table per entry point below XFUSION, run by tests/test_gpu_small_shapes.py on the inputs and
float64 references of tests/small_cases.py.  Their classes: a size against the 256-thread stride (1, stride - 1, stride,
stride + 1, three strides or more), the caps from both sides, every combination of optional pointers the header allows.

The entry points that were reached only through the models -- the dense forward and its _rows form, gate_mul, the Kronecker
product, the fused gating stage (xreduce) and the omic head's one-launch step -- follow below DENSE_BWD, run by
tests/test_gpu_tail_shapes.py on the inputs, references and bars of tests/small_cases.py.

The radiology window (mmf_radio_nll_step_group, mmf_radio_infer_group) and the grouped half chains (mmf_amil_group_forward /
_backward, mmf_radio_group_forward / _backward) have the RADIO and HALF tables above TABLES, run by
tests/test_gpu_radio_shapes.py on the inputs and float64 references of tests/radio_cases.py and pinned to the library by
tests/test_radio_shapes_cpu.py; census() covers their chains ("radio", "radio infer") and radio_row_cap restates their cap.

Integrated gradients (mmf_amil_ig) has the IG table above TABLES with its window planner (ig_row_limit, ig_window_steps,
ig_windows), refusal order (ig_rule) and attribution tile (attr_tile) restated, pinned to the library by
tests/test_ig_shapes_cpu.py and run by tests/test_gpu_ig_shapes.py on the inputs and float64 oracle of tests/ig_cases.py;
census("ig") holds the operands of carve_ig.
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
    """csrc/mmf_amil_fwd.hip plan_linear's ksplit (exact fp32, tick words on offer; no tuning overrides): the K split of a short
    grid of 64 x 64 tiles."""
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
    """csrc/mmf_amil_bwd.hip plan_tn's splits over total_tiles tiles (no tuning overrides)."""
    splits = (256 if tile == 256 else 512) // max(total_tiles, 1)
    return max(1, min(splits, (K + 127) // 128))


def linear_bwd_splits(M, N, K):
    """csrc/mmf_api.hip linear_bwd_plan; 128 x 128 TN tiles below 12,288 rows (plan_tn)."""
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


def stack_widest(c):
    """The widest row of an operand that grows with N: the bag [N x L], h / du [N x H], the gate rows [N x 2 D]
    (include/mmf_amil.h mmf_amil_desc::N; csrc/mmf_api.hip check_desc `widest`)."""
    return max(c.L, c.H, 2 * c.D)


def stack_row_cap(c):
    """The largest N the stack admits: N * max(L, H, 2 D) * elem_bytes < 2^31 (include/mmf_amil.h mmf_amil_desc::N and
    "bf16-storage variant"; csrc/mmf_api.hip check_desc, which check_desc_bf16 calls with 2-byte elements)."""
    return (2**31 - 1) // (stack_widest(c) * (2 if c.bf16 else 4))


def stack_rule(c, N=1):
    """include/mmf_amil.h mmf_amil_desc and "bf16-storage variant"; csrc/mmf_api.hip check_desc / check_desc_bf16 -- in
    the library's order."""
    if N < 1:
        return ERR_SHAPE
    if c.L % KC != 0 or c.H % KC != 0 or c.H not in (256, 512, 1024) or c.D % 128 != 0:
        return ERR_SHAPE
    # the 32-bit mask index.  It can never bind: D % 128 == 0 makes 2 D >= 256, so the row cap below holds N to
    # (2^31 - 1) / (4 max(L, H, 2 D)) (or / 2 for bf16), and N max(H, D) <= N max(L, H, 2 D) < 2^30 < 2^32
    if N * max(c.H, c.D) >= 2**32:
        return ERR_SHAPE
    if N > stack_row_cap(c):
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

# ---- the row cap: every operand that grows with N, per chain ----------------------------------------------------------------
# The kernels address each of these through a buffer resource: 32-bit byte offsets, a record count (unsigned)rows *
# (unsigned)ld * elem, and 0x80000000 as the offset that reads as zero (csrc/mmf_gemm_core.h LoadK / LoadM / OOB), which is
# right only while the operand is below 2^31 bytes.  Read off the carve functions of csrc/mmf_api.hip (AmilWs `carve`,
# AmilWsBf `carve_bf16`, GroupWs `carve_group`, `carve_group_infer`, AttnWs `carve_attn`) and the kernels' make_rsrc calls.
# An entry: (name, rows, row width in elements, element bytes, in the workspace?).  rows is a function of N.
GROUP_POOL_GROUPS, POOL_MAX_ROWS = 256, 8192             # csrc/mmf_kernels.h:277, :107
GROUP_BAG_MAX_PARTIALS = GROUP_POOL_GROUPS + 64          # csrc/mmf_amil_fwd.hip:1089: pooling groups of one bag of a window


def _rows(N):
    return N


def _tiles128(N):
    return (N + 127) // 128                              # fused_fwd_tiles / dh_bf16_row_tiles (csrc/mmf_amil_bf16.hip)


def census(chain, c):
    """The operands of one chain whose size grows with N.  chain: "f32" / "f32 infer" (mmf_amil_forward, _backward,
    _head_forward, _nll_step / mmf_amil_infer), "bf16 fused" / "bf16 unfused" / "bf16 infer" (the same calls on a bf16 bag:
    both training routes carve the same workspace; the fused forward alone writes one pooling partial per 128-row tile),
    "group" / "group infer" (mmf_amil_nll_step_group, mmf_amil_infer_group over sum N rows), "scorer" (mmf_attn_net_*),
    "radio" / "radio infer" (mmf_radio_nll_step_group and the radio half pair / mmf_radio_infer_group on a Radio case: the
    group chains with L = kseg, reduce_dim's output xr and -- training -- its gradient dxr [R x L] (carve_radio,
    carve_radio_infer), each modality segment [R x kseg], and the concatenated input [R x nseg kseg] that radio_operands
    holds below 2 GiB: no kernel reads it as one operand, the refusal is the header's), "ig" (mmf_amil_ig on an Ig case, read
    off carve_ig: the bag and attr [N x L], U and Gacc [N x H], the attribution GEMM's row partials [(L / 32) x N], and the
    grouped chain's operands over the R = steps x N rows of one window, steps = ig_window_steps at that N)."""
    if chain == "ig":
        L, H, D = c.size
        R = lambda N: N * ig_window_steps(N, H, D, c.total, c.window_steps)
        parts = (D + 63) // 64 if c.gated else (D + 127) // 128
        ops = [("x", _rows, L, 4, False), ("attr", _rows, L, 4, False), ("row_sum", _rows, 1, 4, False), ("row_abs", _rows, 1, 4, False),
               ("U", _rows, H, 4, True), ("Gacc", _rows, H, 4, True), ("rs_part", _rows, L // 32, 4, True), ("ra_part", _rows, L // 32, 4, True),
               ("h", R, H, 4, True), ("relu_bits", lambda N: (R(N) + 15) // 16 + 2, (H // 32) * 8, 8, True), ("a", R, D, 4, True),
               ("s_part", R, parts, 4, True), ("p", R, 1, 4, True), ("ds", R, 1, 4, True), ("du", R, H, 4, True), ("A_raw", R, 1, 4, True),
               ("ridx_h", R, 1, 4, True), ("ridx_d", R, 1, 4, True), ("bag", R, 1, 4, True)]
        return ops + ([("b", R, D, 4, True)] if c.gated else [])
    if chain in ("radio", "radio infer"):
        ops = census("group" if chain == "radio" else "group infer", c)
        ops += [("xr", _rows, c.L, 4, True)] + ([("dxr", _rows, c.L, 4, True)] if chain == "radio" else [])
        ops += [(f"x[{m}]", _rows, c.kseg, 4, False) for m in range(c.nseg)]
        return ops + [("x concatenated", _rows, c.nseg * c.kseg, 4, False)]
    L, H, D, mstk = getattr(c, "L", c.H), c.H, c.D, (2 if c.gated else 1) * c.D
    parts = (D + 63) // 64 if c.gated else (D + 127) // 128          # gate_parts (csrc/mmf_amil_fwd.hip)
    parts16 = (D + 127) // 128 if c.gated else (D + 255) // 256      # gate_parts_bf16 (csrc/mmf_amil_bf16.hip)
    relu_bits = ("relu_bits", lambda N: (N + 15) // 16 + 2, (H // 32) * 8, 8, True)
    if chain == "scorer":
        ops = [("x", _rows, H, 4, False), ("A", _rows, 1, 4, False), ("dx", _rows, H, 4, False),
               ("a", _rows, D, 4, True), ("s_part", _rows, parts, 4, True)]
        return ops + ([("b", _rows, D, 4, True)] if c.gated else [])
    if chain in ("f32", "f32 infer", "group", "group infer"):
        ops = [("x", _rows, L, 4, False), ("A_raw", _rows, 1, 4, False), ("h", _rows, H, 4, True), ("s_part", _rows, parts, 4, True)]
        if chain in ("f32", "group"):
            ops += [relu_bits, ("a", _rows, D, 4, True), ("p", _rows, 1, 4, True), ("ds", _rows, 1, 4, True), ("du", _rows, H, 4, True)]
            ops += [("b", _rows, D, 4, True)] if c.gated else []
        if chain == "group":
            ops += [("ridx_h", _rows, 1, 4, True), ("ridx_d", _rows, 1, 4, True), ("bag", _rows, 1, 4, True)]
        return ops
    assert chain in ("bf16 fused", "bf16 unfused", "bf16 infer"), chain
    ops = [("x", _rows, L, 2, False), ("A_raw", _rows, 1, 4, False), ("h", _rows, H, 2, True), ("s_part", _rows, parts16, 4, True)]
    if chain != "bf16 unfused":
        ops += [("partials", _tiles128, 2 + H, 4, True)]
    if chain != "bf16 infer":
        ops += [("a", _rows, D, 2, True), ("du", _rows, H, 2, True), ("dP", _rows, mstk, 2, True), ("p", _rows, 1, 4, True),
                ("ds", _rows, 1, 4, True), ("dbc_part", _tiles128, 1, 4, True), ("dwc_part", _tiles128, D, 4, True)]
        ops += [("b", _rows, D, 2, True)] if c.gated else []
    return ops


def census_bytes(chain, c, N):
    """{operand: bytes} of one chain at N rows."""
    return {name: rows(N) * width * elem for name, rows, width, elem, _ in census(chain, c)}


def census_workspace(chain, c, N):
    """What the chain's census puts into the workspace, each slot rounded up to the carver's 256 bytes."""
    return sum((rows(N) * width * elem + 255) // 256 * 256 for _, rows, width, elem, ws in census(chain, c) if ws)


def census_slack(chain, c):
    """stack_widest over the widest row the chain really holds.  1 wherever L or H is the widest, and for every bf16
    training chain (dP is [N x 2 D] when gated).  Above 1 only where 2 D is the widest of an fp32 chain or of an ungated
    bf16 chain: those keep a and b apart ([N x D] each) and store no dP, so check_desc's 2 D term -- one formula for both
    storages -- refuses such a stack while its largest operand is still `slack` times below 2 GiB.  Conservative, not a
    hole: see DESIGN.md 7p."""
    widest = max(width for _, rows, width, _, _ in census(chain, c) if rows is _rows)
    scorer = chain == "scorer"
    return (max(c.H, 2 * c.D) if scorer else stack_widest(c)) / widest


def bf16_chain(c):
    return "bf16 fused" if c.gated and c.H == 256 and c.D == 256 else "bf16 unfused"


def group_row_cap(c):
    """sum N of a window: the one-bag cap, and group_plan's 256 pooling groups of at most 8192 rows (csrc/mmf_api.hip).  A
    single bag of a window may span at most GROUP_BAG_MAX_PARTIALS groups (launch_group_pool_partial), which at 8192-row
    groups is more rows than any window holds: the per-bag limit never binds below the window's."""
    return min(stack_row_cap(c), GROUP_POOL_GROUPS * POOL_MAX_ROWS)


def group_rule(c, sizes):
    """include/mmf_amil.h "Grouped training step" / "Grouped forward-only pass"; csrc/mmf_api.hip group_plan, window_plan."""
    if not 1 <= len(sizes) <= GROUP_MAX or any(n < 1 for n in sizes):
        return ERR_SHAPE
    if sum(sizes) > GROUP_POOL_GROUPS * POOL_MAX_ROWS:
        return ERR_SHAPE
    return stack_rule(c, sum(sizes))


SHIPPED_HEADS = {"small": (1024, 256, 256), "big": (1024, 512, 384)}     # multimodalfusion_amd/models/model_modules.py AMIL_SIZES


def cap_stacks():
    """(chain, stack) for every admitted stack of the tables and the shipped heads: what the row-cap census covers."""
    out = [("f32", c) for c in STACK_F32 if stack_rule(c) == OK] + [("f32 infer", c) for c in STACK_F32 if stack_rule(c) == OK]
    for c in STACK_BF16:
        if stack_rule(c) == OK:
            out += [(bf16_chain(c), c), ("bf16 infer", c)]
    for _, _, size, gated in GROUPED:
        out += [("group", Stack(*size, gated)), ("group infer", Stack(*size, gated))]
    for size in SHIPPED_HEADS.values():
        out += [("f32", Stack(*size, True)), ("f32 infer", Stack(*size, True)), ("group", Stack(*size, True)),
                ("group infer", Stack(*size, True))]
        b = Stack(*size, True, bf16=True)
        out += [(bf16_chain(b), b), ("bf16 infer", b)]
    seen, uniq = set(), []
    for k in out:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    return uniq


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

# ---- the single-workgroup and one-thread-per-element half: csrc/mmf_small.hip, the stage-2 block and the dense backward -----
# of csrc/mmf_mlp.hip.  Run by tests/test_gpu_small_shapes.py on the inputs of tests/small_cases.py.  Classes are named after
# the work unit: the 256-thread stride of a single-workgroup loop or of a one-thread-per-element grid, the 4-wave and
# 64-lane strides of the head forward, the 4-float vector of the Adam step, the 512 x 256 grid of abs_sum.
NT = 256                                                 # threads of every kernel below
HEAD_MAX_BK = 256                                        # csrc/mmf_small.hip:14: B * K values of the head kept in LDS
COX_MAX_B = 8192                                         # csrc/mmf_small.hip launch_cox: exp(theta) and w, 2 * B floats of LDS
HAZ_MAX_K = 32                                           # csrc/mmf_mlp.hip hazard_bwd_kernel: float h[32]
ABS_GRID = 512 * NT                                      # csrc/mmf_small.hip launch_abs_sum: 512 blocks of 256 threads
DENSE_MAX_N, DENSE_MAX_B = 2048, 256                     # csrc/mmf_mlp.hip:629: above either, launch_dense_bwd takes three launches


def stride_class(n, stride=NT):
    """n against a loop or a grid that advances `stride` at a time."""
    return {1: "1", stride - 1: "stride - 1", stride: "stride", stride + 1: "stride + 1"}.get(
        n, "three strides or more" if n > 2 * stride else "other")


def _stride_tags(key, n):
    c = stride_class(n)
    return set() if c == "other" else {(key, c)}


# mmf_surv_head_forward / _backward
@dataclass(frozen=True)
class Head:
    B: int
    F: int
    K: int
    steep: bool = False          # the bias puts logits at +-30: hazards at the ends of (0, 1), S underflowing
    why: str = ""


def head_rule(c):
    """include/mmf_amil.h "Survival head" (B * K <= 256); csrc/mmf_api.hip mmf_surv_head_forward / _backward (B, K < 1),
    csrc/mmf_small.hip launch_head_fwd / launch_head_bwd -- before any launch."""
    if c.B < 1 or c.K < 1:
        return ERR_ARG
    if c.B * c.K > HEAD_MAX_BK or c.B > NT:
        return ERR_SHAPE
    return OK


def head_tags(c):
    code = head_rule(c)
    if code != OK:
        return {("refused", code, f"B={c.B} K={c.K}")}
    t = set()
    if c.B * c.K in (3, 4, 5):
        t.add(("B*K against the 4-wave stride", c.B * c.K))
    if c.F in (1, 63, 64, 65, 1024):
        t.add(("F against the 64-lane stride", c.F))
    if c.F == NT + 1:
        t.add(("backward: F against the 256-column stride", c.F))
    if c.B * c.K == HEAD_MAX_BK:
        t.add(("cap B*K = 256", (c.B, c.K)))
    if c.steep:
        t.add(("logits", "+-30"))
    return t


HEAD = [
    Head(3, 1, 1, why="B*K = 3: the fourth wave idle; F = 1: one lane of the dot product"),
    Head(1, 63, 4, why="B*K = 4: one output per wave; F = 63: the last lane idle"),
    Head(5, 64, 1, why="B*K = 5: a second round of wave 0 alone; F = 64: every lane once"),
    Head(2, 65, 3, steep=True, why="F = 65: a second round of lane 0; logits at +-30: (1 - h) underflows in the cumprod backward"),
    Head(2, 1024, 4, why="F = 1024: sixteen rounds of the lane loop"),
    Head(3, 257, 4, why="backward: F = 257, a second round of thread 0 over the columns"),
    Head(8, 8, 32, why="the cap B*K = 256 as (8, 32): the deepest cumprod"),
    Head(256, 8, 1, why="the cap B*K = 256 as (256, 1): every thread a sample"),
    # refused
    Head(9, 8, 29, why="B*K = 261"),
    Head(257, 8, 1, why="B = 257"),
]
REQUIRED_HEAD = (
    {("B*K against the 4-wave stride", v) for v in (3, 4, 5)} | {("F against the 64-lane stride", v) for v in (1, 63, 64, 65, 1024)}
    | {("backward: F against the 256-column stride", 257), ("cap B*K = 256", (8, 32)), ("cap B*K = 256", (256, 1)), ("logits", "+-30")}
    | {("refused", ERR_SHAPE, "B=9 K=29"), ("refused", ERR_SHAPE, "B=257 K=1")})


# mmf_nll_surv
@dataclass(frozen=True)
class Nll:
    B: int
    K: int
    bad_row: int = -1            # the row whose device label is K (out of range), or -1
    why: str = ""


def nll_rule(c):
    """include/mmf_amil.h mmf_nll_surv; csrc/mmf_api.hip mmf_nll_surv -- any B >= 1, K >= 1: one workgroup strides over B."""
    return ERR_ARG if c.B < 1 or c.K < 1 else OK


def nll_tags(c):
    if nll_rule(c) != OK:
        return {("refused", nll_rule(c), f"B={c.B} K={c.K}")}
    t = _stride_tags("B", c.B)
    if c.bad_row >= 0:
        t.add(("label", "out of range in a row >= 256" if c.bad_row >= NT else "out of range"))
    return t


NLL = [
    Nll(1, 1, why="one sample, one bin: S_padded[y] is the padding, S_padded[y + 1] the only S"),
    Nll(255, 4, why="the last thread idle"),
    Nll(256, 4, why="every thread one sample"),
    Nll(257, 4, why="thread 0 takes a second sample"),
    Nll(700, 4, why="three rounds of the stride loop, the last ragged"),
    Nll(300, 4, bad_row=280, why="label K on a device label in row 280: NaN loss, that row's gradients zero, the others right"),
    Nll(0, 4, why="refused: B = 0"),
]
REQUIRED_NLL = ({("B", s) for s in ("1", "stride - 1", "stride", "stride + 1", "three strides or more")}
                | {("label", "out of range in a row >= 256"), ("refused", ERR_ARG, "B=0 K=4")})


# mmf_cox_surv
@dataclass(frozen=True)
class Cox:
    B: int
    all_censored: bool = False
    why: str = ""


def cox_rule(c):
    """include/mmf_amil.h mmf_cox_surv (B <= 8192); csrc/mmf_api.hip mmf_cox_surv, csrc/mmf_small.hip launch_cox."""
    if c.B < 1:
        return ERR_ARG
    return ERR_SHAPE if c.B > COX_MAX_B else OK


def cox_tags(c):
    if cox_rule(c) != OK:
        return {("refused", cox_rule(c), f"B={c.B}")}
    return {("censoring", "all censored")} if c.all_censored else {("B", c.B)}


COX = [
    Cox(2, why="the smallest batch with a risk set of two"),
    Cox(256, why="every thread one sample"),
    Cox(257, why="thread 0 takes a second sample"),
    Cox(1000, why="four rounds, the last ragged; beyond the sizes the suite's bar was set on"),
    Cox(6145, why="2 * 6145 * 4 bytes of dynamic LDS: the first B above 48 KiB"),
    Cox(8192, why="the cap: 64 KiB of dynamic LDS on top of 1 KiB static"),
    Cox(5, all_censored=True, why="all censored: loss 0, gradient 0, log(D_i) still finite"),
    Cox(8193, why="refused: above the cap"),
]
REQUIRED_COX = ({("B", b) for b in (2, 256, 257, 1000, 6145, 8192)} | {("censoring", "all censored"), ("refused", ERR_SHAPE, "B=8193")})


# mmf_ranking_loss
@dataclass(frozen=True)
class Rank:
    B: int
    phi: int                     # 0 sigmoid, 1 relu
    reduction: int               # 0 mean, 1 sum
    kind: str = "many"           # many / none / one / tied / equal risks: what tests/small_cases.py rank_inputs generates
    why: str = ""


def rank_rule(c):
    """include/mmf_amil.h mmf_ranking_loss (B >= 2); csrc/mmf_api.hip mmf_ranking_loss, csrc/mmf_mlp.hip launch_rank_loss."""
    if c.phi not in (0, 1) or c.reduction not in (0, 1):
        return ERR_ARG
    return ERR_SHAPE if c.B < 2 else OK


def rank_tags(c):
    if rank_rule(c) != OK:
        return {("refused", rank_rule(c), f"B={c.B}")}
    t = _stride_tags("B", c.B) | {("phi, reduction", (c.phi, c.reduction))}
    t.add({"many": ("pairs", "many"), "none": ("pairs", "none"), "one": ("pairs", "one"), "tied": ("times", "tied"),
           "equal risks": ("risks", "equal under phi = relu")}[c.kind])
    return t


RANK = [
    Rank(255, 0, 0, why="sigmoid / mean; the last thread idle"),
    Rank(256, 1, 1, why="relu / sum; every thread one sample"),
    Rank(257, 0, 1, why="sigmoid / sum; thread 0 takes a second sample"),
    Rank(700, 1, 0, why="relu / mean; three rounds of the stride loop"),
    Rank(4, 0, 0, "none", why="no comparable pair: loss 0, gradient 0"),
    Rank(4, 0, 0, "one", why="exactly one comparable pair: n = 1"),
    Rank(6, 0, 1, "tied", why="tied times: a tie is not comparable in either order"),
    Rank(6, 1, 0, "equal risks", why="equal risks under relu: phi(0) = 0 with derivative 0"),
    Rank(1, 0, 0, why="refused: B = 1"),
]
REQUIRED_RANK = ({("B", s) for s in ("stride - 1", "stride", "stride + 1", "three strides or more")}
                 | {("phi, reduction", (p, r)) for p in (0, 1) for r in (0, 1)}
                 | {("pairs", "none"), ("pairs", "one"), ("times", "tied"), ("risks", "equal under phi = relu"),
                    ("refused", ERR_SHAPE, "B=1")})


# mmf_hazards_forward / _backward
@dataclass(frozen=True)
class Haz:
    B: int
    K: int
    Y_hat: bool = True           # optional outputs of the forward: given or NULL
    risk: bool = True
    gH: bool = True              # optional gradients of the backward: given or NULL
    gS: bool = True
    gR: bool = True
    steep: bool = False
    why: str = ""


def haz_rule(c):
    """include/mmf_amil.h mmf_hazards_forward / _backward (K <= 32); csrc/mmf_mlp.hip launch_hazard_fwd / _bwd."""
    return ERR_SHAPE if c.B < 1 or c.K < 1 or c.K > HAZ_MAX_K else OK


def haz_tags(c):
    if haz_rule(c) != OK:
        return {("refused", haz_rule(c), f"B={c.B} K={c.K}")}
    t = _stride_tags("B", c.B) | {("forward: Y_hat, risk", (c.Y_hat, c.risk)), ("backward: g_hazards, g_S, g_risk", (c.gH, c.gS, c.gR))}
    if c.K in (1, 4, HAZ_MAX_K):
        t.add(("K", c.K))
    if c.steep:
        t.add(("logits", "+-30"))
    return t


HAZ = [
    Haz(1, 1, Y_hat=False, risk=False, gH=False, gS=False, gR=False, why="one sample, K = 1; no optional pointer at all: dlogits = 0"),
    Haz(255, 4, Y_hat=True, risk=False, gH=True, gS=False, gR=False, why="the last thread idle; Y_hat alone; g_hazards alone"),
    Haz(256, 32, Y_hat=False, risk=True, gH=False, gS=True, gR=False, why="one full block, K = 32: the whole h[32]; risk alone; g_S alone"),
    Haz(257, 4, gH=False, gS=False, gR=True, why="a second block of one sample; g_risk alone"),
    Haz(700, 4, gH=True, gS=True, gR=False, why="three blocks; g_hazards and g_S"),
    Haz(3, 4, gH=True, gS=False, gR=True, why="g_hazards and g_risk"),
    Haz(3, 5, gH=False, gS=True, gR=True, why="g_S and g_risk"),
    Haz(3, 32, steep=True, why="all three gradients; logits at +-30 over K = 32: S underflows, (1 - h) rounds to 0"),
    Haz(3, 0, why="refused: K = 0"),
    Haz(3, 33, why="refused: K = 33"),
]
REQUIRED_HAZ = ({("B", s) for s in ("1", "stride - 1", "stride", "stride + 1", "three strides or more")} | {("K", k) for k in (1, 4, 32)}
                | {("forward: Y_hat, risk", (a, b)) for a in (True, False) for b in (True, False)}
                | {("backward: g_hazards, g_S, g_risk", (a, b, d)) for a in (True, False) for b in (True, False) for d in (True, False)}
                | {("logits", "+-30"), ("refused", ERR_SHAPE, "B=3 K=0"), ("refused", ERR_SHAPE, "B=3 K=33")})


# mmf_highway_mix_forward / _backward
@dataclass(frozen=True)
class Highway:
    n: int
    why: str = ""


def highway_rule(c):
    """include/mmf_amil.h mmf_highway_mix_*; csrc/mmf_api.hip mmf_highway_mix_forward / _backward: any n >= 1."""
    return ERR_ARG if c.n < 1 else OK


def highway_tags(c):
    return {("refused", ERR_ARG, f"n={c.n}")} if c.n < 1 else _stride_tags("n", c.n)


HIGHWAY = [Highway(1, why="one element"), Highway(255, why="the last thread idle"), Highway(256, why="one full block"),
           Highway(257, why="a second block of one element"), Highway(700, why="three blocks, the last ragged"),
           Highway(0, why="refused: n = 0")]
REQUIRED_HIGHWAY = ({("n", s) for s in ("1", "stride - 1", "stride", "stride + 1", "three strides or more")}
                    | {("refused", ERR_ARG, "n=0")})


# mmf_batchnorm_forward / _backward
@dataclass(frozen=True)
class Bn:
    B: int
    F: int
    training: bool = True
    act: int = 0
    drop_p: float = 0.0
    res: bool = False
    affine: bool = False         # gamma and beta given
    running: bool = False        # running statistics given (eval mode needs them)
    dres: bool = False
    dgb: bool = False            # dgamma and dbeta given
    shifted: bool = False        # every feature has mean 8 and std 1/8
    why: str = ""


def bn_rule(c):
    """include/mmf_amil.h mmf_batchnorm_forward ("B >= 2" in training mode); csrc/mmf_api.hip mmf_batchnorm_forward,
    csrc/mmf_mlp.hip launch_bn_fwd.  The backward has no B >= 2 rule of its own."""
    if c.B < 1 or c.F < 1 or (not c.training and not c.running) or not 0 <= c.act <= 4 or not 0.0 <= c.drop_p < 1.0:
        return ERR_ARG
    return ERR_SHAPE if c.training and c.B < 2 else OK


def bn_tags(c):
    if bn_rule(c) != OK:
        return {("refused", bn_rule(c), f"B={c.B} training={int(c.training)}")}
    t = _stride_tags("F", c.F) | {("act", c.act), ("drop_p", c.drop_p), ("res", c.res), ("gamma / beta", c.affine),
                                  ("dres", c.dres), ("dgamma / dbeta", c.dgb)}
    if c.training:
        t |= {("training B", c.B), ("running statistics", c.running)}
    else:
        t |= {("eval B", c.B), ("backward", "eval mode")}
    if c.shifted:
        t.add(("feature", "mean 8, std 1/8"))
    return t


BN = [
    Bn(2, 1, why="the smallest training batch, one feature; every optional pointer NULL"),
    Bn(32, 255, act=1, drop_p=0.25, res=True, affine=True, running=True, dres=True, dgb=True,
       why="the shipped B; the last thread idle; ReLU + dropout + residual, every optional pointer given"),
    Bn(300, 256, act=2, affine=True, running=True, dgb=True, why="B = 300: the longest sums; one full block; tanh"),
    Bn(1, 257, training=False, act=3, affine=True, running=True, dgb=True, why="eval mode with B = 1; a second block of one feature; sigmoid"),
    Bn(4, 700, act=4, res=True, dres=True, why="three blocks of features; SELU"),
    Bn(32, 8, affine=True, running=True, dgb=True, shifted=True, why="features of mean 8 and std 1/8: the two-pass variance"),
    Bn(1, 8, why="refused: training with B = 1"),
]
REQUIRED_BN = ({("F", s) for s in ("1", "stride - 1", "stride", "stride + 1", "three strides or more")}
               | {("training B", b) for b in (2, 32, 300)} | {("eval B", 1), ("backward", "eval mode")}
               | {(k, v) for k in ("res", "gamma / beta", "running statistics", "dres", "dgamma / dbeta") for v in (True, False)}
               | {("act", a) for a in range(5)} | {("drop_p", 0.0), ("drop_p", 0.25), ("feature", "mean 8, std 1/8"),
                                                   ("refused", ERR_SHAPE, "B=1 training=1")})


# mmf_adam_l1_step
@dataclass(frozen=True)
class Adam:
    n: int
    mask: bool = False
    l1: float = 3e-4
    wd: float = 1e-3
    step: int = 1
    misalign: bool = False
    why: str = ""


def adam_rule(c):
    """include/mmf_amil.h "Per-step tail"; csrc/mmf_api.hip mmf_adam_l1_step: w, g, m, v and a non-null mask 16-byte aligned."""
    if c.n < 1 or c.step < 1:
        return ERR_ARG
    return ERR_ALIGN if c.misalign else OK


def adam_tags(c):
    if adam_rule(c) != OK:
        return {("refused", adam_rule(c), "misaligned w" if c.misalign else f"n={c.n} step={c.step}")}
    t = {("n", c.n), ("mask", c.mask), ("step", c.step)}
    if c.l1 == 0:
        t.add(("l1", 0))
    if c.wd == 0:
        t.add(("wd", 0))
    return t


ADAM = [
    Adam(1, why="n = 1: the tail branch alone, one element"),
    Adam(3, mask=True, why="n = 3: the tail branch alone, with a mask"),
    Adam(4, step=2, why="n = 4: one vector, no tail; step 2"),
    Adam(5, l1=0.0, why="n = 5: one vector and a tail of one; l1 = 0"),
    Adam(1023, mask=True, wd=0.0, why="n = 1023: 255 vectors and a tail of three in the last thread, both under a mask; wd = 0"),
    Adam(1024, step=1000, why="n = 1024: one full block; step 1000: both bias corrections near 1"),
    Adam(1025, why="n = 1025: a second block that is all tail"),
    Adam(1027, mask=True, why="n = 1027: a second block with a tail of three; a mask over full vectors and the tail"),
    Adam(8, step=0, why="refused: step 0"),
    Adam(8, misalign=True, why="refused: w 4 bytes off a 16-byte boundary"),
]
REQUIRED_ADAM = ({("n", n) for n in (1, 3, 4, 5, 1023, 1024, 1025, 1027)} | {("mask", True), ("mask", False), ("l1", 0), ("wd", 0)}
                 | {("step", s) for s in (1, 2, 1000)} | {("refused", ERR_ARG, "n=8 step=0"), ("refused", ERR_ALIGN, "misaligned w")})


# mmf_abs_sum
@dataclass(frozen=True)
class AbsSum:
    n: int
    why: str = ""


def abs_sum_rule(c):
    """include/mmf_amil.h mmf_abs_sum; csrc/mmf_api.hip mmf_abs_sum: any n >= 1."""
    return ERR_ARG if c.n < 1 else OK


def abs_sum_chain(n):
    """The longest add chain of mmf_abs_sum: a thread's share of the grid-stride loop, wave_sum (6) and the four waves (3)
    in the first launch; two partials a thread, wave_sum and the four waves again in the second."""
    return -(-n // ABS_GRID) + 6 + 3 + 2 + 6 + 3


def abs_sum_tags(c):
    if c.n < 1:
        return {("refused", ERR_ARG, f"n={c.n}")}
    t = {("n against the 512 x 256 grid", stride_class(c.n, ABS_GRID))}
    if -(-c.n // ABS_GRID) >= 8:
        t.add(("per-thread chain", ">= 8"))
    return t


ABS_SUM = [AbsSum(1, why="below one block: 511 blocks add nothing"), AbsSum(ABS_GRID - 1, why="the last thread of the grid idle"),
           AbsSum(ABS_GRID, why="every thread one element"), AbsSum(ABS_GRID + 1, why="thread 0 of block 0 takes a second element"),
           AbsSum(1000003, why="a per-thread chain of eight, ragged"), AbsSum(0, why="refused: n = 0")]
REQUIRED_ABS_SUM = ({("n against the 512 x 256 grid", s) for s in ("1", "stride - 1", "stride", "stride + 1")}
                    | {("per-thread chain", ">= 8"), ("refused", ERR_ARG, "n=0")})


# mmf_dense_backward / mmf_dense_backward_rows
@dataclass(frozen=True)
class DenseBwd:
    B: int
    K: int
    N: int
    act: int = 0                 # 0 none, 1 relu, 4 selu
    drop_kind: int = 0           # 0 none, 1 nn.Dropout, 2 nn.AlphaDropout (p = 0.25)
    dx: bool = True
    db: bool = True
    rows: int = 0                # > 0: mmf_dense_backward_rows with ldy = lddy = N + rows.  "Both _rows forms" of the backward are
                                 # its two kernels built for row_base: the fused launch and the three-launch fallback; the
                                 # forward _rows entry point is not in this table (tests/test_gpu_mm_group_step.py runs it)
    why: str = ""


def dense_bwd_rule(c):
    """include/mmf_amil.h mmf_dense_backward / _rows; csrc/mmf_api.hip: no cap on B, K or N -- above N = 2048 or B = 256
    launch_dense_bwd (csrc/mmf_mlp.hip) takes the three-launch form."""
    if c.B < 1 or c.K < 1 or c.N < 1 or not 0 <= c.act <= 4 or not 0 <= c.drop_kind <= 2:
        return ERR_ARG
    return ERR_SHAPE if c.rows < 0 else OK


def dense_bwd_path(c):
    if c.B > DENSE_MAX_B:
        return "fallback by B"
    if c.N > DENSE_MAX_N:
        return "fallback by N"
    return "fused at the cap" if (c.B, c.N) == (DENSE_MAX_B, DENSE_MAX_N) else "fused"


def dense_bwd_tags(c):
    if dense_bwd_rule(c) != OK:
        return {("refused", dense_bwd_rule(c), f"act={c.act} drop_kind={c.drop_kind} rows={c.rows}")}
    path = dense_bwd_path(c)
    t = {("path, K", (path, c.K)), ("act", c.act), ("drop_kind", c.drop_kind), ("dx", c.dx), ("db", c.db)}
    if c.rows > 0:
        t.add(("_rows with ldy > N", "fused" if path.startswith("fused") else "fallback"))
    if path != "fused at the cap" and c.dx and c.N % 2:
        t.add(("dense_dx_kernel", "odd N"))
    return t


DENSE_BWD = [
    DenseBwd(256, 36, 2048, act=1, drop_kind=1, why="fused at the cap, K = 36: one ragged dx block, one ragged dW block a row"),
    DenseBwd(256, 257, 2048, act=4, rows=4, why="fused at the cap, K = 257: a second dW block of one column; _rows, ldy = N + 4"),
    DenseBwd(256, 300, 2048, dx=False, why="fused at the cap, K = 300; no dx: dW blocks alone"),
    DenseBwd(257, 36, 8, act=4, drop_kind=2, why="fallback by B, K = 36; SELU + AlphaDropout"),
    DenseBwd(257, 257, 8, act=1, db=False, why="fallback by B, K = 257: a second column block of one; no db"),
    DenseBwd(257, 300, 7, drop_kind=1, rows=3, why="fallback by B, K = 300, odd N = 7: dense_dx_kernel's remainder; _rows, ldy = N + 3"),
    DenseBwd(2, 36, 2052, act=1, drop_kind=1, why="fallback by N = 2052, K = 36"),
    DenseBwd(2, 257, 2052, act=4, drop_kind=2, dx=False, why="fallback by N, K = 257; no dx; SELU + AlphaDropout"),
    DenseBwd(2, 300, 2052, why="fallback by N, K = 300"),
    DenseBwd(2, 8, 8, act=5, why="refused: unknown activation"),
    DenseBwd(2, 8, 8, drop_kind=3, why="refused: unknown dropout kind"),
    DenseBwd(2, 8, 8, rows=-1, why="refused: _rows with ldy < N"),
]
REQUIRED_DENSE_BWD = (
    {("path, K", (p, k)) for p in ("fused at the cap", "fallback by B", "fallback by N") for k in (36, 257, 300)}
    | {("act", a) for a in (0, 1, 4)} | {("drop_kind", d) for d in (0, 1, 2)} | {(k, v) for k in ("dx", "db") for v in (True, False)}
    | {("_rows with ldy > N", f) for f in ("fused", "fallback")} | {("dense_dx_kernel", "odd N")}
    | {("refused", ERR_ARG, "act=5 drop_kind=0 rows=0"), ("refused", ERR_ARG, "act=0 drop_kind=3 rows=0"),
       ("refused", ERR_SHAPE, "act=0 drop_kind=0 rows=-1")})

# ---- the omic step, the dense forward and the fusion ops (tests/test_gpu_tail_shapes.py) -----------------------------------
# Classes are named after each kernel's own work unit: the 64 lanes and the 4 x 64 unrolled round of dense_fwd_kernel's K
# loop and the 4 waves of its blocks, the 256-thread blocks of gate_mul and kron_fwd, the 64 lanes kron_bwd strides over the
# "other" indices with, wave_dot's 256-float round and the 16 waves / 1024 threads of the xreduce pair, and for the omic
# step the first layer's three routes, the 4 rows a workgroup owns, the Cox loop tiers and the 64-thread risk-set stride.
DENSE_FWD_GRID = 65535 * 16                              # csrc/mmf_mlp.hip launch_dense_fwd: blocks of 4 waves, one output each
KRON_MAX_B = 65535                                       # csrc/mmf_api.hip kron_shape_ok: B is grid.y
XR_MAX = 384                                             # csrc/mmf_mlp.hip:202: m * B * sdim values of the gating stage in LDS


# mmf_dense_forward / mmf_dense_forward_rows
@dataclass(frozen=True)
class DenseFwd:
    B: int
    K: int
    N: int
    act: int = 0
    drop_kind: int = 0           # 0 none, 1 nn.Dropout, 2 nn.AlphaDropout
    bias: bool = True
    rows: int = 0                # 0: mmf_dense_forward; 1: the _rows form with ldy = N; > 1: ldy = N + rows; -1: ldy = N - 1
    drop_p: float = 0.25         # used where drop_kind != 0 (and checked by the library whatever drop_kind is)
    base: bool = True            # False: the _rows form with row_base = NULL
    why: str = ""


def dense_fwd_rule(c):
    """include/mmf_amil.h mmf_dense_forward / _rows; csrc/mmf_api.hip -- in the library's order."""
    if c.B < 1 or c.K < 1 or c.N < 1 or (c.rows and not c.base):
        return ERR_ARG
    if not 0 <= c.act <= 4 or not 0 <= c.drop_kind <= 2 or not 0.0 <= c.drop_p < 1.0:
        return ERR_ARG
    if not c.rows and c.drop_kind and c.drop_p > 0 and c.B * c.N >= 2**32:
        return ERR_SHAPE                                  # the plain form's 32-bit mask index b * N + n would repeat
    return ERR_SHAPE if c.rows < 0 else OK


def dense_fwd_tags(c):
    if dense_fwd_rule(c) != OK:
        return {("refused", dense_fwd_rule(c), f"B={c.B} K={c.K} N={c.N} act={c.act} drop_kind={c.drop_kind} drop_p={c.drop_p} rows={c.rows} base={c.base}")}
    t = {("act", c.act), ("drop_kind", c.drop_kind)}
    if c.K in (1, 63, 64, 65, 255, 256, 257, 513):
        t.add(("K against the 64-lane tail and the 4 x 64 round", c.K))
    if c.N == 1:
        t.add(("N", "1"))
    if c.N % 4:
        t.add(("N", "not a multiple of 4"))
    if c.B * c.N in (1, 3, 4, 5):
        t.add(("B*N against the 4 waves of a block", c.B * c.N))
    if c.B * c.N > 4 * DENSE_FWD_GRID:
        t.add(("grid", "the grid-stride loop wraps"))
    if not c.bias:
        t.add(("bias", "NULL"))
    if c.rows:
        t.add(("_rows", "ldy = N" if c.rows == 1 else "ldy > N"))
    return t


DENSE_FWD = [
    DenseFwd(1, 1, 1, why="K = 1: lane 0 alone, once; N = 1; B*N = 1: three waves idle"),
    DenseFwd(1, 63, 3, act=1, why="K = 63: the last lane idle; B*N = 3: the fourth wave idle"),
    DenseFwd(2, 64, 2, act=2, why="K = 64: every lane one tail step; B*N = 4: one output per wave; tanh"),
    DenseFwd(1, 65, 5, act=3, why="K = 65: a second tail step of lane 0; B*N = 5: a second block of one wave; sigmoid"),
    DenseFwd(3, 255, 6, act=4, drop_kind=2, why="K = 255: lane 63 takes three tail steps, the others the unrolled round; SELU + AlphaDropout"),
    DenseFwd(3, 256, 8, act=1, drop_kind=1, why="K = 256: one unrolled round, no tail; ReLU + Dropout"),
    DenseFwd(2, 257, 7, bias=False, why="K = 257: an unrolled round and a tail step of lane 0; no bias"),
    DenseFwd(3, 513, 10, act=4, drop_kind=2, rows=1, why="K = 513: two unrolled rounds and a tail step; _rows with ldy = N"),
    DenseFwd(5, 36, 9, act=1, drop_kind=1, rows=5, why="_rows with ldy = N + 5, every row its own seed"),
    DenseFwd(2049, 1, 2048, act=1, drop_kind=1, why="4,196,352 outputs against 4,194,240 waves: the grid-stride loop wraps"),
    # refused
    DenseFwd(2, 8, 8, drop_kind=1, drop_p=1.0, why="refused: drop_p = 1"),
    DenseFwd(2, 8, 8, act=5, why="refused: unknown activation"),
    DenseFwd(2, 8, 8, drop_kind=3, why="refused: unknown dropout kind"),
    DenseFwd(2, 8, 8, rows=-1, why="refused: _rows with ldy < N"),
    DenseFwd(2, 8, 8, rows=1, base=False, why="refused: _rows with row_base = NULL"),
    DenseFwd(0, 8, 8, why="refused: B = 0"),
    DenseFwd(2, 0, 8, why="refused: K = 0"),
    DenseFwd(2, 8, 0, why="refused: N = 0"),
]
REQUIRED_DENSE_FWD = (
    {("K against the 64-lane tail and the 4 x 64 round", k) for k in (1, 63, 64, 65, 255, 256, 257, 513)}
    | {("N", "1"), ("N", "not a multiple of 4"), ("grid", "the grid-stride loop wraps"), ("bias", "NULL")}
    | {("B*N against the 4 waves of a block", v) for v in (1, 3, 4, 5)} | {("act", a) for a in range(5)}
    | {("drop_kind", d) for d in range(3)} | {("_rows", "ldy = N"), ("_rows", "ldy > N")}
    | {t for c in DENSE_FWD if dense_fwd_rule(c) != OK for t in dense_fwd_tags(c)})


# mmf_gate_mul_forward / _backward
@dataclass(frozen=True)
class GateMul:
    n: int
    why: str = ""


def gate_mul_rule(c):
    """include/mmf_amil.h mmf_gate_mul_*; csrc/mmf_api.hip: any n >= 1."""
    return ERR_ARG if c.n < 1 else OK


def gate_mul_tags(c):
    return {("refused", ERR_ARG, f"n={c.n}")} if c.n < 1 else {("n against the 256-thread block", c.n)}


GATE_MUL = [GateMul(1, why="one element"), GateMul(255, why="the last thread idle"), GateMul(256, why="one full block"),
            GateMul(257, why="a second block of one thread"), GateMul(1000, why="four blocks, the last ragged"),
            GateMul(0, why="refused: n = 0")]
REQUIRED_GATE_MUL = {("n against the 256-thread block", n) for n in (1, 255, 256, 257, 1000)} | {("refused", ERR_ARG, "n=0")}


# mmf_kron_forward / _backward
@dataclass(frozen=True)
class Kron:
    m: int
    dim: int
    B: int = 1
    drop_p: float = 0.0
    null: bool = False           # o[m - 1] = NULL
    why: str = ""


def kron_rule(c):
    """include/mmf_amil.h mmf_kron_*; csrc/mmf_api.hip mmf_kron_forward / _backward, kron_shape_ok -- in the library's order."""
    if c.m not in (2, 3) or c.dim < 1 or c.B < 1 or c.null:
        return ERR_ARG
    if c.B > KRON_MAX_B or c.B * (c.dim + 1) ** c.m >= 2**31:
        return ERR_SHAPE
    return OK


def kron_tags(c):
    if kron_rule(c) != OK:
        return {("refused", kron_rule(c), f"m={c.m} dim={c.dim} B={c.B} null={c.null}")}
    S = c.dim + 1
    t = {("B", c.B), ("dropout", c.drop_p > 0)}
    if (c.m, c.dim) in ((2, 1), (2, 15), (2, 16), (3, 5), (3, 6), (3, 16)):
        t.add(("S^m against the forward's 256-thread blocks", (c.m, S ** c.m)))
    if (c.m, c.dim) in ((2, 63), (2, 64), (3, 7), (3, 8)):
        t.add(("the backward's others against its 64 lanes", (c.m, S ** (c.m - 1))))
    if c.m == 3:
        t |= {("m = 3 backward, operand role", r) for r in range(3)}
    return t


KRON = [
    Kron(2, 1, why="S^2 = 4: four threads of one block"),
    Kron(2, 15, B=3, drop_p=0.25, why="S^2 = 256: one block exactly; three samples"),
    Kron(2, 16, why="S^2 = 289: a second block of 33 threads"),
    Kron(3, 5, B=3, why="S^3 = 216: the last 40 threads idle"),
    Kron(3, 6, drop_p=0.25, why="S^3 = 343: a second block of 87 threads"),
    Kron(3, 16, B=3, drop_p=0.25, why="S^3 = 4913, the shipped size: twenty blocks, the last ragged"),
    Kron(2, 63, drop_p=0.25, why="backward: 64 others, every lane once"),
    Kron(2, 64, B=3, why="backward: 65 others, a second step of lane 0"),
    Kron(3, 7, B=3, drop_p=0.25, why="backward: 8 x 8 = 64 others, every lane once"),
    Kron(3, 8, why="backward: 9 x 9 = 81 others, a ragged second step"),
    # refused
    Kron(1, 4, why="refused: m = 1"),
    Kron(4, 4, why="refused: m = 4"),
    Kron(2, 0, why="refused: dim = 0"),
    Kron(3, 4, null=True, why="refused: a NULL operand"),
    Kron(3, 1290, why="refused: S^3 = 1291^3 >= 2^31"),
    Kron(2, 46340, why="refused: S^2 = 46341^2 >= 2^31"),
    Kron(2, 255, B=32768, why="refused: B * S^2 = 2^31"),
    Kron(2, 1, B=65536, why="refused: B above grid.y"),
]
KRON_CAPS = {(3, 1290, 1), (2, 46340, 1), (2, 255, 32768), (2, 1, 65536)}      # refused by the caps: never given real buffers
REQUIRED_KRON = (
    {("S^m against the forward's 256-thread blocks", v) for v in ((2, 4), (2, 256), (2, 289), (3, 216), (3, 343), (3, 4913))}
    | {("the backward's others against its 64 lanes", v) for v in ((2, 64), (2, 65), (3, 64), (3, 81))}
    | {("B", 1), ("B", 3), ("dropout", True), ("dropout", False)} | {("m = 3 backward, operand role", r) for r in range(3)}
    | {t for c in KRON if kron_rule(c) != OK for t in kron_tags(c)})


# mmf_xreduce_forward / _backward
@dataclass(frozen=True)
class XReduce:
    m: int
    B: int
    dim: int
    sdim: int
    drop_p: float = 0.0
    misalign: bool = False       # v[0] 4 bytes off a 16-byte boundary
    null: str = ""               # that member of modality m - 1 is NULL
    why: str = ""


def _xreduce_args(c):
    if not 1 <= c.m <= 3 or c.B < 1 or c.dim < 1 or c.sdim < 1 or not 0.0 <= c.drop_p < 1.0 or c.null:
        return ERR_ARG
    return OK


def xreduce_fwd_rule(c):
    """include/mmf_amil.h mmf_xreduce_io; csrc/mmf_api.hip xreduce_params, mmf_xreduce_forward (alignment), csrc/mmf_mlp.hip
    launch_xreduce_fwd -- in the library's order."""
    if _xreduce_args(c) != OK:
        return ERR_ARG
    if c.misalign:
        return ERR_ALIGN
    return ERR_SHAPE if c.m * c.B * c.sdim > XR_MAX or c.dim % 4 else OK


def xreduce_bwd_rule(c):
    """The backward reads one float at a time: no dim % 4, no alignment (csrc/mmf_mlp.hip launch_xreduce_bwd)."""
    if _xreduce_args(c) != OK:
        return ERR_ARG
    return ERR_SHAPE if c.m * c.B * c.sdim > XR_MAX else OK


def xreduce_tags(c):
    fw, bw = xreduce_fwd_rule(c), xreduce_bwd_rule(c)
    what = f"m={c.m} B={c.B} dim={c.dim} sdim={c.sdim} drop_p={c.drop_p} misalign={c.misalign} null={c.null}"
    if bw != OK:
        return {("refused", fw, bw, what)}
    if fw != OK:
        return {("forward refused, backward admitted", fw, what)}
    t = {("B", c.B), ("dropout", c.drop_p > 0)}
    if c.dim in (4, 252, 256, 260, 1024, 1028):
        t.add(("dim against wave_dot's 256-float round", c.dim))
    if 2 * c.m * c.B * c.sdim in (2, 64, 96, 768):
        t.add(("h and z values against a sweep of 64", 2 * c.m * c.B * c.sdim))
    if c.sdim in (15, 16, 17):
        t.add(("sdim against the unroll of 16", c.sdim))
    if c.m * c.sdim * c.sdim in (1024, 1089) or c.m * c.sdim * c.sdim > 100 * 1024:
        t.add(("dWo elements against 1024 threads", min(c.m * c.sdim * c.sdim, 100 * 1024 + 1)))
    if c.m == 3 and c.drop_p > 0:
        t.add(("dropout", "three sites"))
    return t


XREDUCE = [
    XReduce(1, 1, 4, 1, why="two values: 14 waves idle; dim = 4: lane 0 alone"),
    XReduce(2, 1, 252, 16, why="64 values: one sweep exactly; dim = 252: the last lane idle"),
    XReduce(3, 1, 256, 16, drop_p=0.25, why="the shipped size: 96 values, dim = 256 one full round; three dropout sites"),
    XReduce(3, 8, 260, 16, drop_p=0.25, why="768 values on the cap m*B*sdim = 384; dim = 260: a second round of lane 0; B = 8"),
    XReduce(1, 2, 1024, 15, why="dim = 1024: the four unrolled rounds; sdim = 15; B = 2"),
    XReduce(1, 1, 1028, 17, why="dim = 1028: a fifth round of lane 0; sdim = 17: one step past the unroll"),
    XReduce(1, 1, 4, 32, why="dWo: 1024 elements, one per thread"),
    XReduce(1, 1, 4, 33, why="dWo: 1089 elements, a second step of 65 threads"),
    XReduce(1, 1, 4, 384, why="sdim = 384, the cap alone: dWo takes 144 strides"),
    XReduce(2, 1, 6, 3, why="dim = 6: the forward refuses (16-byte loads), the backward runs"),
    XReduce(2, 1, 8, 3, misalign=True, why="v[0] 4 bytes off: the forward refuses, the backward runs"),
    # refused by both
    XReduce(3, 8, 4, 17, why="refused: m*B*sdim = 408"),
    XReduce(1, 1, 4, 385, why="refused: sdim = 385"),
    XReduce(0, 1, 4, 4, why="refused: m = 0"),
    XReduce(4, 1, 4, 4, why="refused: m = 4"),
    XReduce(2, 1, 4, 4, null="Wz", why="refused: Wz of the last modality NULL"),
    XReduce(2, 1, 4, 4, null="gm", why="refused: gm of the last modality NULL"),
    XReduce(2, 1, 4, 4, drop_p=1.0, why="refused: drop_p = 1"),
]
REQUIRED_XREDUCE = (
    {("dim against wave_dot's 256-float round", d) for d in (4, 252, 256, 260, 1024, 1028)}
    | {("h and z values against a sweep of 64", v) for v in (2, 64, 96, 768)} | {("sdim against the unroll of 16", v) for v in (15, 16, 17)}
    | {("dWo elements against 1024 threads", v) for v in (1024, 1089, 100 * 1024 + 1)} | {("B", b) for b in (1, 2, 8)}
    | {("dropout", False), ("dropout", True), ("dropout", "three sites")}
    | {t for c in XREDUCE if xreduce_fwd_rule(c) != OK for t in xreduce_tags(c)})


# mmf_maxnet_cox_step
MX_H, MX_R = 256, 4                                      # csrc/mmf_maxnet.hip:31-32: hidden width, rows a workgroup owns
MX_PTRS = ("x", "W0", "b0", "W1", "b1", "Wc", "bc", "sync", "times", "c", "workspace", "risk", "loss",
           "dW0", "db0", "dW1", "db1", "dWc", "dbc")


@dataclass(frozen=True)
class MaxStep:
    B: int
    G: int
    p_drop: float = 0.0
    censor: str = "mixed"        # "mixed" (distinct times, 30 % censored), "none", "all", "tied", "last event" (the only event has the largest time)
    misalign: bool = False       # W0 4 bytes off a 16-byte boundary
    word: int = 0                # non-zero: seed_dev points at this device word, the masks are those of seed + word
    accumulate: int = 0          # 1: the gradients are added onto known values
    loss_scale: float = 1.0
    H0: int = MX_H
    sync_words: int = 3
    ws_short: bool = False       # the workspace one byte short of the query
    null: str = ""               # that pointer NULL (MX_PTRS)
    off: str = ""                # that pointer ("W1", "workspace", "times") 4 bytes off its required alignment
    why: str = ""


def maxstep_workgroups(B):
    return 64 if B > MX_R * 32 else 32                   # csrc/mmf_maxnet.hip maxnet_step_workgroups


def maxstep_workspace_bytes(B):
    """csrc/mmf_maxnet.hip maxnet_step_workspace_floats: y0, y1 [B x 256]; dpre1, dpre0 [256 x 4 workgroups]; dr; the dWc shares."""
    B = max(B, 1)
    return 4 * (2 * B * MX_H + 2 * MX_H * maxstep_workgroups(B) * MX_R + (B + 63) // 64 * 64 + 64 * MX_H)


def maxstep_rule(c):
    """include/mmf_amil.h mmf_maxnet_cox_step; csrc/mmf_api.hip mmf_maxnet_cox_step -- in the library's order."""
    if c.null and c.null != "sync":
        return ERR_ARG
    if not (1 <= c.B <= 256 and 1 <= c.G <= 256 and c.H0 == MX_H):
        return ERR_SHAPE
    if c.null == "sync" or c.sync_words < 3 or not 0.0 <= c.p_drop < 1.0:
        return ERR_ARG
    if c.ws_short:
        return ERR_WORKSPACE
    return ERR_ALIGN if c.off else OK                     # W1, workspace: 16-byte loads and stores; times: double


def maxstep_route(c):
    """Layer 0 of maxnet_cox_step_kernel (csrc/mmf_maxnet.hip:284)."""
    if c.G <= 64 and c.G % 4 == 0:
        return "narrow shape, W0 misaligned: chunked" if c.misalign else "narrow"
    return "chunked"


def maxstep_tags(c):
    if maxstep_rule(c) != OK:
        return {("refused", maxstep_rule(c), f"B={c.B} G={c.G} H0={c.H0} sync_words={c.sync_words} p_drop={c.p_drop} ws_short={c.ws_short} null={c.null} off={c.off}")}
    t = {("layer 0", (maxstep_route(c), c.G)), ("p_drop", c.p_drop), ("seed_dev", "a word" if c.word else "NULL"), ("accumulate", c.accumulate),
         ("loss_scale", "1" if c.loss_scale == 1.0 else "not 1")}
    if c.B in (1, 3, 4, 5, 127, 128, 129, 255, 256):
        t.add(("rows against 4 a workgroup and 32 / 64 workgroups", c.B))
    if c.B in (15, 16, 17, 19):
        t.add(("Cox loop tiers", c.B))
    if c.B in (63, 64, 65):
        t.add(("risk-set gradient, 64-thread stride", c.B))
    if c.censor != "mixed":
        t.add(("censoring", c.censor))
    return t


MAXSTEP = [
    MaxStep(1, 4, censor="none", why="B = 1, an event whose risk set is itself: 31 workgroups own no row; G = 4: the narrow route's partial group alone"),
    MaxStep(3, 16, p_drop=0.25, why="B = 3: one workgroup, its fourth row beyond the batch; G = 16: one full group of the narrow route"),
    MaxStep(4, 36, p_drop=0.25, why="B = 4: one workgroup's rows exactly; G = 36: the shipped narrow shape, two full groups and a partial"),
    MaxStep(5, 36, p_drop=0.25, misalign=True, why="B = 5: a second workgroup with one row; G = 36 with W0 4 bytes off: the chunked route"),
    MaxStep(127, 60, loss_scale=0.5, why="B = 127: the last row of 32 workgroups missing; G = 60: three full groups and three quarters; loss_scale 0.5"),
    MaxStep(128, 1, p_drop=0.25, why="B = 128: 32 workgroups full; G = 1: one column of the chunked route"),
    MaxStep(129, 65, p_drop=0.25, word=77, why="B = 129: the 64-workgroup kernel; G = 65: a second chunk of one column; seed_dev"),
    MaxStep(255, 193, p_drop=0.25, accumulate=1, why="B = 255; G = 193: a fourth chunk, the refetch of staging buffer 1; accumulate"),
    MaxStep(256, 256, p_drop=0.25, why="the cap on both: 64 workgroups full, four full chunks"),
    MaxStep(15, 64, p_drop=0.25, censor="all", why="B = 15: the Cox 4-member tier and the scalar tail only; G = 64: four full groups; all censored"),
    MaxStep(16, 63, censor="tied", why="B = 16: one pass of the 16-member tier; G = 63: one ragged chunk; tied times"),
    MaxStep(17, 128, censor="last event", why="B = 17: 16-member tier and one tail step; G = 128: one round, both staging buffers; one event at the largest time"),
    MaxStep(19, 129, censor="none", why="B = 19: 16-member tier and three tail steps; G = 129: a second round, the refetch of buffer 0; none censored"),
    MaxStep(63, 80, why="B = 63: the last thread of a risk-set row idle"),
    MaxStep(64, 186, p_drop=0.25, why="B = 64: every thread of a risk-set row one member"),
    MaxStep(65, 36, why="B = 65: a second member for thread 0"),
    # refused
    MaxStep(0, 36, why="refused: B = 0"),
    MaxStep(257, 36, why="refused: B = 257"),
    MaxStep(8, 0, why="refused: G = 0"),
    MaxStep(8, 257, why="refused: G = 257"),
    MaxStep(8, 36, H0=128, why="refused: H0 = 128"),
    MaxStep(8, 36, sync_words=2, why="refused: two tick words"),
    MaxStep(8, 36, p_drop=1.0, why="refused: p_drop = 1"),
    MaxStep(8, 36, ws_short=True, why="refused: the workspace one byte short"),
] + [MaxStep(8, 36, null=n, why=f"refused: {n} = NULL") for n in MX_PTRS] + [
    MaxStep(8, 36, off=n, why=f"refused: {n} 4 bytes off") for n in ("W1", "workspace", "times")]
REQUIRED_MAXSTEP = (
    {("layer 0", ("narrow", g)) for g in (4, 16, 36, 60, 64)} | {("layer 0", ("narrow shape, W0 misaligned: chunked", 36))}
    | {("layer 0", ("chunked", g)) for g in (1, 63, 65, 128, 129, 193, 256)}
    | {("rows against 4 a workgroup and 32 / 64 workgroups", b) for b in (1, 3, 4, 5, 127, 128, 129, 255, 256)}
    | {("Cox loop tiers", b) for b in (15, 16, 17, 19)} | {("risk-set gradient, 64-thread stride", b) for b in (63, 64, 65)}
    | {("censoring", k) for k in ("none", "all", "tied", "last event")} | {("p_drop", 0.0), ("p_drop", 0.25)}
    | {("seed_dev", "NULL"), ("seed_dev", "a word"), ("accumulate", 0), ("accumulate", 1), ("loss_scale", "1"), ("loss_scale", "not 1")}
    | {t for c in MAXSTEP if maxstep_rule(c) != OK for t in maxstep_tags(c)})


# ---- the radiology window (mmf_radio_nll_step_group, mmf_radio_infer_group) and the grouped half chains ---------------------
# (mmf_amil_group_forward / _backward, mmf_radio_group_forward / _backward).  Run by tests/test_gpu_radio_shapes.py on the
# inputs and float64 references of tests/radio_cases.py.  reduce_dim is a dense layer over nseg segments of kseg columns
# with N = L = kseg outputs, so the classes are those of a short L: chunks of kseg, the K split of a short grid
# (plan_linear), the splits of the dW_r TN launch over tiles wider than L (plan_tn), and -- for the halves -- where the
# stack's H columns sit in the caller's feature matrix.
SIXTY_FOUR = tuple(1 + (37 * g) % 90 for g in range(64))      # tests/test_gpu_radio_group_step.py SIXTY_FOUR: 64 bags of 1..90 rows
TN_WIDE_MIN = 12288                                      # csrc/mmf_amil_bwd.hip plan_tn: 256-wide TN tiles from here on


def window_class(sizes):
    return {(1, 65, 300): "(1, 65, 300)", SIXTY_FOUR: "64 bags of 1..90 rows"}.get(
        tuple(sizes), "one bag alone" if len(sizes) == 1 else "other")


@dataclass(frozen=True)
class Radio:
    nseg: int
    kseg: int
    H: int
    D: int
    gated: bool
    sizes: tuple
    train: bool                  # True: p_h = p_att = 0.25, both dropout sites (a third, b, when gated); False: eval mode
    accumulate: int = 0          # 1: the gradients are added onto known non-zero values
    stack_L: int = 0             # the stack's L where it is not kseg (refused)
    misalign: str = ""           # "segment" (x[1]), "W", "dW": that pointer 4 bytes off a 16-byte boundary
    seed: int = 1                # of the weights; chosen on the CPU (tests/radio_cases.py) for the ReLU kink condition
    why: str = ""

    @property
    def L(self):
        return self.stack_L or self.kseg

    @property
    def stack(self):
        return Stack(self.L, self.H, self.D, self.gated)

    @property
    def size(self):
        return (self.L, self.H, self.D)

    @property
    def R(self):
        return sum(self.sizes)


def radio_row_cap(c):
    """sum N of a radio window: the stack's window cap, and the [sum N x nseg kseg] input below 2 GiB (include/mmf_amil.h
    mmf_radio_nll_step_group; csrc/mmf_api.hip radio_operands) -- 131,071 rows at four 1024-wide modalities."""
    return min(group_row_cap(c.stack), (2**31 - 1) // (4 * c.nseg * c.kseg))


def radio_rule(c, grads=True):
    """include/mmf_amil.h mmf_radio_nll_step_group / mmf_radio_infer_group / mmf_radio_group_forward / _backward;
    csrc/mmf_api.hip radio_modalities, then group_check / infer_group_check / group_half_check (window_plan), then
    radio_operands -- in the library's order.  grads: the entry point writes dW / db (the step, the backward half)."""
    if c.nseg < 2 or c.nseg > 4:
        return ERR_SHAPE
    code = group_rule(c.stack, c.sizes)
    if code != OK:
        return code
    if c.kseg != c.L:
        return ERR_SHAPE
    if c.R * c.nseg * c.kseg * 4 >= 2**31:
        return ERR_SHAPE
    if c.misalign in ("segment", "W") or (grads and c.misalign == "dW"):
        return ERR_ALIGN
    return OK


def radio_tn_splits(c):
    """csrc/mmf_api.hip carve_radio: the dW_r problems as a TN launch of their own, planned over their own tiles."""
    td = 256 if c.R >= TN_WIDE_MIN else 128
    cdiv = lambda a, b: (a + b - 1) // b
    return tn_splits(c.R, c.nseg * cdiv(c.L, td) * cdiv(c.kseg, td), td)


def radio_tags(c):
    code = radio_rule(c)
    if code != OK:
        return {("refused", code, f"nseg={c.nseg} kseg={c.kseg} L={c.L} H={c.H} D={c.D} misalign={c.misalign}")}
    per_tile = 64 if c.gated else 128
    return {("stack", (c.kseg, c.H, c.D, c.gated)), ("nseg", c.nseg), ("kseg", c.kseg), ("kseg chunks", chunks(c.kseg)), ("H", c.H),
            ("gated" if c.gated else "ungated",), ("D tiles", "one" if c.D // per_tile == 1 else "many"),
            ("window", window_class(c.sizes)),
            ("reduce_dim forward", "K split" if linear_ksplit(c.R, c.L, c.nseg * c.kseg, c.nseg, c.kseg) > 1 else "plain"),
            ("dW_r TN launch", "several" if radio_tn_splits(c) > 1 else "one split"),
            ("mode", "train, both dropout sites" if c.train else "eval"), ("accumulate", c.accumulate)}


RADIO = [
    Radio(2, 32, 256, 128, False, (1, 65, 300), True, seed=3,
          why="two modalities of one chunk: the 128-wide TN tile of modality 0's problem reaches over modality 1's columns of dW_r [32 x 64]; 3 TN splits"),
    Radio(3, 96, 256, 128, True, SIXTY_FOUR, False, seed=1,
          why="three modalities of three chunks, 64 bags: each problem's 128-wide tile ends 32 columns inside the next modality's; eval"),
    Radio(4, 160, 512, 640, True, (65,), True, accumulate=1, seed=1,
          why="four modalities of five chunks, one bag of 65 rows: one TN split, q.M = 160 over two row tiles; accumulate"),
    Radio(4, 128, 1024, 128, True, (1, 65, 300), True, seed=3,
          why="four modalities of four chunks: reduce_dim takes its two-way K split over the segments; H = 1024"),
    Radio(2, 32, 1024, 384, False, (1, 65, 300), False, seed=9,
          why="the H = 1024 stack behind a 32-wide reduce_dim, ungated with three D tiles; eval"),
    # refused
    Radio(1, 32, 256, 128, False, (1, 65, 300), True, why="nseg = 1: no reduce_dim, the pathology calls"),
    Radio(5, 32, 256, 128, False, (1, 65, 300), True, why="nseg = 5"),
    Radio(2, 32, 256, 128, False, (1, 65, 300), True, stack_L=64, why="kseg != L"),
    Radio(2, 128, 768, 128, True, (1, 65, 300), True, why="H outside {256, 512, 1024}: check_desc, through window_plan"),
    Radio(2, 32, 256, 128, False, (1, 65, 300), True, misalign="segment", why="x[1] 4 bytes off: the segments are read 16 bytes at a time"),
    Radio(2, 32, 256, 128, False, (1, 65, 300), True, misalign="W", why="reduce_dim's W 4 bytes off"),
    Radio(2, 32, 256, 128, False, (1, 65, 300), True, misalign="dW", why="dW 4 bytes off: refused where it is written, admitted forward-only"),
]
REQUIRED_RADIO = (
    {("stack", (c.L, c.H, c.D, c.gated)) for c in STACK_F32 if stack_rule(c) == OK}
    | {("nseg", n) for n in (2, 3, 4)} | {("kseg", k) for k in (32, 96, 128, 160)}
    | {("kseg chunks", k) for k in ("one", "odd", "four")} | {("H", h) for h in (256, 512, 1024)} | {("gated",), ("ungated",)}
    | {("D tiles", "one"), ("D tiles", "many")}
    | {("window", w) for w in ("(1, 65, 300)", "one bag alone", "64 bags of 1..90 rows")}
    | {("reduce_dim forward", "K split"), ("reduce_dim forward", "plain")}
    | {("dW_r TN launch", "one split"), ("dW_r TN launch", "several")}
    | {("mode", "train, both dropout sites"), ("mode", "eval")} | {("accumulate", 0), ("accumulate", 1)}
    | {("refused", ERR_SHAPE, f"nseg={n} kseg=32 L=32 H=256 D=128 misalign=") for n in (1, 5)}
    | {("refused", ERR_SHAPE, "nseg=2 kseg=32 L=64 H=256 D=128 misalign="), ("refused", ERR_SHAPE, "nseg=2 kseg=128 L=128 H=768 D=128 misalign=")}
    | {("refused", ERR_ALIGN, f"nseg=2 kseg=32 L=32 H=256 D=128 misalign={m}") for m in ("segment", "W", "dW")})


@dataclass(frozen=True)
class Half:
    radio: int                   # nseg of the radio pair, or 0: mmf_amil_group_forward / _backward
    L: int
    H: int
    D: int
    gated: bool
    sizes: tuple
    ldm_extra: int               # ldm = H + ldm_extra: the width of the caller's feature matrix
    m_offset: int                # the column of that matrix the stack's H columns start at
    train: bool = True           # True: p_h = p_att = 0.25; False: eval mode
    accumulate: int = 0          # of the backward
    misalign: str = ""           # "dM": the backward's dM 4 bytes off a 16-byte boundary
    seed: int = 1
    why: str = ""

    @property
    def ldm(self):
        return self.H + self.ldm_extra

    @property
    def stack(self):
        return Stack(self.L, self.H, self.D, self.gated)

    @property
    def size(self):
        return (self.L, self.H, self.D)

    @property
    def nseg(self):
        return self.radio

    @property
    def kseg(self):
        return self.L

    @property
    def R(self):
        return sum(self.sizes)


def half_rule(c, bwd=True):
    """include/mmf_amil.h mmf_amil_group_forward / _backward and the radio pair; csrc/mmf_api.hip radio_modalities (radio),
    group_half_check, radio_operands (radio) -- in the library's order.  bwd: the backward half, which reads an ungathered
    dM (ldm == H) four floats at a time."""
    if c.radio and (c.radio < 2 or c.radio > 4):
        return ERR_SHAPE
    code = group_rule(c.stack, c.sizes)
    if code != OK:
        return code
    if c.ldm < c.H:
        return ERR_SHAPE
    if bwd and c.ldm == c.H and c.misalign == "dM":
        return ERR_ALIGN
    if c.radio and c.R * c.radio * c.L * 4 >= 2**31:
        return ERR_SHAPE
    return OK


def half_tags(c):
    code = half_rule(c)
    if code != OK:
        return {("refused", code, f"radio={c.radio} H={c.H} ldm={c.ldm} misalign={c.misalign}")}
    ldm = "== H" if c.ldm_extra == 0 else "H + 1" if c.ldm_extra == 1 else "3 H" if c.ldm == 3 * c.H else "other"
    kind = "radio" if c.radio else "plain"
    t = {("ldm", ldm), ("H", c.H), (kind,), ("mode", "train" if c.train else "eval"), ("accumulate", c.accumulate)}
    if c.ldm != c.H:
        t |= {("dM gathered, M merged into a wider matrix", kind), ("slot starts at a non-zero column", c.m_offset > 0)}
    return t


HALF = [
    Half(0, 96, 256, 128, True, SIXTY_FOUR, 0, 0, seed=50, why="the pathology half on a matrix of its own, 64 bags: ldm == H, dM read in place"),
    Half(2, 160, 512, 640, True, (1, 65, 300), 1, 1, train=False, accumulate=1, seed=1,
         why="the radio half, its 512 columns from column 1 of a [3 x 513] matrix: rows of M and dM at every alignment; eval; accumulate"),
    Half(4, 128, 1024, 128, True, (1, 65, 300), 2048, 1024, seed=3,
         why="the radio half in the middle third of a [3 x 3072] matrix: H = 1024, the K-split reduce_dim"),
    Half(0, 32, 1024, 384, False, (1, 65, 300), 1, 1, train=False, seed=83,
         why="the pathology half with a gathered dM: mmf_amil_group_backward's own call of launch_group_dm_gather"),
    # refused
    Half(0, 96, 256, 128, True, (1, 65, 300), -1, 0, why="ldm < H"),
    Half(0, 96, 256, 128, True, (1, 65, 300), 0, 0, misalign="dM", why="ldm == H and dM 4 bytes off: K-dh reads it four floats at a time"),
]
REQUIRED_HALF = (
    {("ldm", l) for l in ("== H", "H + 1", "3 H")} | {("H", h) for h in (256, 512, 1024)} | {("radio",), ("plain",)}
    | {("mode", "train"), ("mode", "eval")} | {("accumulate", 0), ("accumulate", 1)}
    | {("dM gathered, M merged into a wider matrix", k) for k in ("radio", "plain")} | {("slot starts at a non-zero column", True)}
    | {("refused", ERR_SHAPE, "radio=0 H=256 ldm=255 misalign="), ("refused", ERR_ALIGN, "radio=0 H=256 ldm=256 misalign=dM")})


def radio_cap_stacks():
    """(nseg, stack) the radio row-cap census covers: every admitted stack of the tables above (kseg = L) and the shipped
    head, each at nseg 2..4."""
    stacks = [c for c in STACK_F32 if stack_rule(c) == OK] + [Stack(*SHIPPED_HEADS["small"], True)]
    return [Radio(n, s.L, s.H, s.D, s.gated, (337, 338), True) for s in stacks for n in (2, 3, 4)]


# ---- integrated gradients: mmf_amil_ig ------------------------------------------------------------------------------------
# The call runs n_steps + 2 steps (the quadrature's, then alpha = 1 and alpha = 0 with weight 0: the riders) as the bags of
# grouped windows of `steps` steps over the bag's N rows.  Restated below: the window planner, the refusal order, the
# attribution GEMM's tile; census("ig") holds the operands of carve_ig.  tests/test_ig_shapes_cpu.py pins all of it to the
# library; tests/test_gpu_ig_shapes.py runs every accepted case on the inputs and float64 oracle of tests/ig_cases.py.
IG_LIB_WINDOW_ROWS = 2**18                               # csrc/mmf_api.hip ig_window_steps: rows of a window the library cuts itself
IG_BAD = ("", "p_h", "p_att", "gemm", "null row_sum", "attr misaligned", "workspace short")


@dataclass(frozen=True)
class Ig:
    L: int
    H: int
    D: int
    gated: bool
    N: int
    K: int = 4
    n_steps: int = 20
    window_steps: int = 0
    method: str = "gausslegendre"
    n0: int = 0                  # rows of the base bag of a periodic case (row i = base[i mod n0]); 0: the bag itself, direct oracle
    attr: bool = True            # the [N x L] output is requested
    bad: str = ""                # one of IG_BAD: what else is wrong with the call (refused)
    why: str = ""

    @property
    def size(self):
        return (self.L, self.H, self.D)

    @property
    def stack(self):
        return Stack(self.L, self.H, self.D, self.gated)

    @property
    def total(self):
        return self.n_steps + 2

    @property
    def name(self):
        return (f"{self.L}_{self.H}_{self.D}_{'gated' if self.gated else 'ungated'}_n{self.N}_k{self.K}_s{self.n_steps}"
                f"_w{self.window_steps}")


def ig_row_limit(H, D):
    """csrc/mmf_api.hip ig_row_limit: the rows of one window -- the 32-bit mask index over max(H, D), every H- and 2 D-wide
    operand below 2^31 bytes (check_desc on the window without the L-wide bag), group_plan's 256 pooling groups of 8192."""
    return min((2**32 - 1) // max(H, D), (2**31 - 1) // (4 * max(H, 2 * D)), GROUP_POOL_GROUPS * POOL_MAX_ROWS)


def ig_window_steps(N, H, D, total, window_steps):
    """csrc/mmf_api.hip ig_window_steps: steps per window -- the caller's, or (0) windows of at most 2^18 rows cut evenly;
    clamped to the row limit, MMF_GROUP_MAX and the call's steps.  0: not even one step fits."""
    if N < 1 or H < 1 or D < 1:
        return 0
    smax = ig_row_limit(H, D) // N
    if smax < 1:
        return 0
    smax = min(smax, GROUP_MAX, total)
    if window_steps > 0:
        return min(window_steps, smax)
    s = min(max(IG_LIB_WINDOW_ROWS // N, 1), smax)
    nwin = (total + s - 1) // s
    return (total + nwin - 1) // nwin


def ig_windows(c):
    """csrc/mmf_api.hip mmf_amil_ig's window loop: (q0, S, nfold) per window -- its first step in the call, its steps, and how
    many of them are folded into Gacc (the riders carry weight 0 and are not)."""
    steps = ig_window_steps(c.N, c.H, c.D, c.total, c.window_steps)
    out = []
    for q0 in range(0, c.total, steps):
        S = min(steps, c.total - q0)
        out.append((q0, S, max(0, min(S, c.n_steps - q0))))
    return out


def ig_pool_groups(N, S):
    """csrc/mmf_api.hip group_plan on S equal bags of N rows: seg.gbeg[S], the pooling groups of one window."""
    rpg = max(64, (S * N + GROUP_POOL_GROUPS - 1) // GROUP_POOL_GROUPS)
    return S * ((N + rpg - 1) // rpg)


def attr_tile(N, L):
    """csrc/mmf_amil_bwd.hip launch_nn_tiles: the attribution GEMM [N x H] . [H x L] on 128 x 128 tiles once they fill the
    chip, else 64 x 64."""
    return 128 if (N // 128) * ((L + 127) // 128) >= 256 else 64


def ig_projection(N, L, H):
    """The tile of the call's projection U = x . W1^T (csrc/mmf_amil_fwd.hip launch_linear_impl, fp32 mode), by the
    restatements of tests/launch_plans.py and linear_ksplit above."""
    import launch_plans as lp
    if bool(lp.use_wide_tiles(N, H)):
        return "wide"
    if bool(lp.use_big_tiles(N, H)):
        return "128 x 128"
    return "64 x 64, K split" if linear_ksplit(N, H, L, 1, L) > 1 else "64 x 64"


def ig_rule(c):
    """include/mmf_amil.h "Integrated-gradients patch attribution"; csrc/mmf_api.hip mmf_amil_ig -- in the library's order:
    null structs, mode, the step counts and tables, the outputs, the head's operands (all MMF_ERR_ARG); check_desc; the
    head's K; ig_window_steps; check_operands and attr's alignment; the workspace size."""
    assert c.bad in IG_BAD, c.bad
    if c.bad in ("gemm", "p_h", "p_att"):
        return ERR_ARG
    if c.n_steps < 1 or c.n_steps > GROUP_MAX or c.window_steps < 0:
        return ERR_ARG
    if c.bad == "null row_sum":
        return ERR_ARG
    code = stack_rule(c.stack, c.N)
    if code != OK:
        return code
    if c.K < 1 or c.K > 32:
        return ERR_SHAPE
    # "a bag too long for one step to be a window": never after check_desc, whose cap is at or below the window's row limit
    # for every admitted (H, D) (tests/test_ig_shapes_cpu.py); the query, which has no descriptor, does return 0 there
    if ig_window_steps(c.N, c.H, c.D, c.total, c.window_steps) < 1:
        return ERR_SHAPE
    if c.bad == "attr misaligned":
        return ERR_ALIGN
    if c.bad == "workspace short":
        return ERR_WORKSPACE
    return OK


def _ig_sizes(w):
    return tuple(S for _, S, _ in w)


def ig_tags(c):
    code = ig_rule(c)
    if code != OK:
        return {("refused", code, f"N={c.N} K={c.K} n_steps={c.n_steps} window_steps={c.window_steps} {c.bad}".rstrip())}
    t = {("stack", (c.L, c.H, c.D, c.gated)), ("K", c.K), ("attr", "requested" if c.attr else "NULL"),
         ("projection", ig_projection(c.N, c.L, c.H))}
    t |= {("head", name) for name, size in SHIPPED_HEADS.items() if size == c.size}
    tile = attr_tile(c.N, c.L)
    t.add(("attr tile", tile))
    if c.L % tile:
        t.add(("a column tile partly outside L", tile))
    w = ig_windows(c)
    steps = ig_window_steps(c.N, c.H, c.D, c.total, c.window_steps)
    t.add(("window sizes", _ig_sizes(w)))
    if len(w) == 1:
        t.add(("windows", "one window"))
    elif c.window_steps == 0:
        t.add(("windows", "a library cut into even windows" if len(set(_ig_sizes(w))) == 1 else "a library cut with a ragged last window"))
    if any(nfold == 0 for _, _, nfold in w):
        t.add(("windows", "a window of riders alone"))
    if any(q0 == c.n_steps + 1 for q0, _, _ in w):
        t.add(("windows", "the two riders in different windows"))
    if any(S == GROUP_MAX for _, S, _ in w):
        t.add(("windows", "S = GROUP_MAX"))
    if c.window_steps > 0 and steps < min(c.window_steps, c.total, GROUP_MAX):
        t.add(("windows", "window_steps clamped by the row limit"))
    if c.n_steps in (1, GROUP_MAX):
        t.add(("n_steps", c.n_steps))
    if c.N == 1:
        t.add(("N", 1))
    if c.N == stack_row_cap(c.stack):
        widest = "L" if c.L >= max(c.H, 2 * c.D) else "H" if c.H > 2 * c.D else "H = 2 D"
        t.add(("N at the cap, set by", widest))
    if c.n0 and c.N % c.n0:
        t.add(("multiplicities", "two different"))
    return t


_IG_CAP = 2**21 - 1
IG = [
    Ig(96, 256, 128, True, 65, why="three chunks: 3 column blocks for ig_rows_kernel, the second 64-wide column tile half outside L"),
    Ig(160, 512, 640, True, 300, K=32, why="ten gate tiles, five column blocks, the head's 32 classes: every lane of its wave loop and tid-0 loop"),
    Ig(32, 1024, 384, False, 300, K=5, why="H = 1024: the dM loop over four strides, the widest pooling rows, K = 1024 in the attribution GEMM; K % 4 != 0"),
    Ig(32, 1024, 384, False, 1, why="one row: every tile, group and step holds one row"),
    Ig(128, 1024, 128, True, 65, K=1, n_steps=4, method="riemann_middle", why="one gate tile under H = 1024, four column blocks, a one-class head"),
    Ig(32, 256, 128, False, 17, n_steps=64, why="66 steps cannot be one window: the library cuts 33 + 33"),
    Ig(32, 256, 128, False, 17, n_steps=64, window_steps=64, why="a window of 64 fills al[GROUP_MAX] and IgSteps; the two riders are a window of their own, nfold = 0"),
    Ig(32, 256, 128, False, 17, n_steps=1, window_steps=1, method="riemann_middle", why="one node; three one-step windows, alpha = 1 and alpha = 0 each alone"),
    Ig(256, 256, 128, False, 16384, why="the 128 x 128 attribution tile at its threshold, two full column tiles; 11 + 11; the projection on wide tiles; direct oracle"),
    Ig(32, 256, 256, True, 32768, n0=337, why="the 128 tile with 32 of its 128 columns inside L; 8 + 8 + 6: four folded steps and both riders last"),
    Ig(32, 256, 256, True, 131072, n0=337, why="eleven windows of two steps, the last the two riders alone behind ten folds"),
    Ig(128, 1024, 128, True, 30000, window_steps=22, n0=375, why="window_steps 22 clamped to 17 by the row limit: 17 + 5, h of a window at 2.09e9 bytes"),
    Ig(32, 256, 128, False, _IG_CAP, n_steps=4, n0=337, attr=False, why="the cap where H = 2 D binds: six one-step windows, h and du 1 KiB below 2 GiB"),
    Ig(128, 1024, 128, True, 2**19 - 1, n_steps=4, n0=337, attr=False, why="the cap where H binds; 2^19 - 1 is prime: two multiplicities"),
    Ig(1024, 256, 256, True, 2**19 - 1, n_steps=2, method="riemann_middle", n0=337,
       why="the shipped small head at the cap L sets: x and attr each 4 KiB below 2 GiB, eight column tiles of the 128 tile"),
    Ig(1024, 512, 384, True, 33, n_steps=2, method="riemann_middle", why="the shipped big head, gated"),
    # refused
    Ig(32, 256, 128, False, 17, bad="p_h", why="train mode: the integrand would be random"),
    Ig(32, 256, 128, False, 17, bad="gemm", why="MMF_GEMM_BF16X3: exact-fp32 GEMMs only"),
    Ig(32, 256, 128, False, 17, n_steps=0, why="no node"),
    Ig(32, 256, 128, False, 17, n_steps=65, why="more nodes than MMF_GROUP_MAX"),
    Ig(32, 256, 128, False, 17, window_steps=-1, why="window_steps < 0"),
    Ig(32, 256, 128, False, 17, bad="null row_sum", why="a required output missing"),
    Ig(32, 256, 128, False, 17, K=33, why="more classes than the stock head's 32"),
    Ig(32, 256, 128, False, _IG_CAP + 1, n_steps=4, why="cap + 1: h of one step would reach 2 GiB"),
    Ig(32, 256, 128, False, 17, bad="attr misaligned", why="attr 4 bytes off: the epilogue stores four floats at a time"),
    Ig(32, 256, 128, False, 17, bad="workspace short", why="one byte less than the query"),
]
REQUIRED_IG = (
    {("stack", (c.L, c.H, c.D, c.gated)) for c in STACK_F32 if stack_rule(c) == OK} | {("head", "small"), ("head", "big")}
    | {("attr tile", 64), ("attr tile", 128), ("a column tile partly outside L", 64), ("a column tile partly outside L", 128)}
    | {("windows", w) for w in ("one window", "a library cut into even windows", "a library cut with a ragged last window",
                                "a window of riders alone", "the two riders in different windows", "S = GROUP_MAX",
                                "window_steps clamped by the row limit")}
    | {("window sizes", s) for s in ((22,), (33, 33), (64, 2), (1, 1, 1), (11, 11), (8, 8, 6), (2,) * 11, (17, 5), (1,) * 6)}
    | {("K", k) for k in (1, 5, 32)} | {("n_steps", 1), ("n_steps", 64)} | {("N", 1)}
    | {("N at the cap, set by", w) for w in ("L", "H", "H = 2 D")} | {("multiplicities", "two different")}
    | {("projection", "wide"), ("projection", "64 x 64")} | {("attr", "requested"), ("attr", "NULL")}
    | {("refused", ERR_ARG, f"N=17 K=4 n_steps=20 window_steps=0 {b}") for b in ("p_h", "gemm", "null row_sum")}
    | {("refused", ERR_ARG, "N=17 K=4 n_steps=0 window_steps=0"), ("refused", ERR_ARG, "N=17 K=4 n_steps=65 window_steps=0"),
       ("refused", ERR_ARG, "N=17 K=4 n_steps=20 window_steps=-1"), ("refused", ERR_SHAPE, "N=17 K=33 n_steps=20 window_steps=0"),
       ("refused", ERR_SHAPE, f"N={_IG_CAP + 1} K=4 n_steps=4 window_steps=0"),
       ("refused", ERR_ALIGN, "N=17 K=4 n_steps=20 window_steps=0 attr misaligned"),
       ("refused", ERR_WORKSPACE, "N=17 K=4 n_steps=20 window_steps=0 workspace short")})


def ig_cap_stacks():
    """The Ig cases the row-cap census covers: every admitted stack of STACK_F32 and both shipped heads, at 4 and 20 nodes."""
    stacks = [c for c in STACK_F32 if stack_rule(c) == OK] + [Stack(*s, True) for s in SHIPPED_HEADS.values()]
    return [Ig(s.L, s.H, s.D, s.gated, 1, n_steps=n) for s in stacks for n in (4, 20)]


TABLES = {
    "mmf_amil_ig": (IG, ig_tags, REQUIRED_IG),
    "RADIO": (RADIO, radio_tags, REQUIRED_RADIO),
    "HALF": (HALF, half_tags, REQUIRED_HALF),
    "XFUSION": (XFUSION, xfusion_tags, REQUIRED_XFUSION),
    "mmf_linear_forward": (LINEAR_FORWARD, linear_forward_tags, REQUIRED_LINEAR_FORWARD),
    "mmf_linear_backward": (LINEAR_BACKWARD, linear_backward_tags, REQUIRED_LINEAR_BACKWARD),
    "mmf_attn_net": (ATTN, attn_tags, REQUIRED_ATTN),
    "mmf_amil (fp32)": (STACK_F32, stack_tags, REQUIRED_STACK),
    "mmf_amil_bf16": (STACK_BF16, stack_tags, REQUIRED_BF16),
    "mmf_surv_head": (HEAD, head_tags, REQUIRED_HEAD),
    "mmf_nll_surv": (NLL, nll_tags, REQUIRED_NLL),
    "mmf_cox_surv": (COX, cox_tags, REQUIRED_COX),
    "mmf_ranking_loss": (RANK, rank_tags, REQUIRED_RANK),
    "mmf_hazards": (HAZ, haz_tags, REQUIRED_HAZ),
    "mmf_highway_mix": (HIGHWAY, highway_tags, REQUIRED_HIGHWAY),
    "mmf_batchnorm": (BN, bn_tags, REQUIRED_BN),
    "mmf_adam_l1_step": (ADAM, adam_tags, REQUIRED_ADAM),
    "mmf_abs_sum": (ABS_SUM, abs_sum_tags, REQUIRED_ABS_SUM),
    "mmf_dense_backward": (DENSE_BWD, dense_bwd_tags, REQUIRED_DENSE_BWD),
    "mmf_dense_forward": (DENSE_FWD, dense_fwd_tags, REQUIRED_DENSE_FWD),
    "mmf_gate_mul": (GATE_MUL, gate_mul_tags, REQUIRED_GATE_MUL),
    "mmf_kron": (KRON, kron_tags, REQUIRED_KRON),
    "mmf_xreduce": (XREDUCE, xreduce_tags, REQUIRED_XREDUCE),
    "mmf_maxnet_cox_step": (MAXSTEP, maxstep_tags, REQUIRED_MAXSTEP),
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
