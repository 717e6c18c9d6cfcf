// Internal parameter blocks and launcher prototypes shared by the .hip translation units.
// (The public C ABI is include/mmf_amil.h; nothing here is exported.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "mmf_common.h"

namespace mmf {

enum : int { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2, ACT_SIGMOID = 3, ACT_SELU = 4 };

struct LinearParams {      // y[M x N] = drop(act(concat_k(x_s)[M x K] . W[N x K]^T + bias))
  const float* x[4];
  int nseg, kseg, ldx;
  const float* w;
  const float* bias;
  float* y;
  int64_t M;
  int N, K;
  int act;
  float drop_p;
  uint32_t drop_key;
  const uint32_t* seed_dev;   // optional device-resident seed added to every key (graph-replay-safe dropout), or null
  int mt_count, nt_count;
  // optional: one bit per output element, y > 0 (relu'(u) . keep), for K-dh's epilogue -- which then does not have to
  // read h a second time.  Layout: per 16x32 block (rb16 = row / 16, cb = col / 32) 8 words of 64 bits; a word is a
  // wave ballot over the row-major epilogue lanes (lane = 8 rr + c4 holds row rr + 8 t, columns 4 c4 + e of a 32- or
  // 16-row block): rows rr + 8 t with t = 0, 1 go to bit block rb16 as word 4 t + e, t = 2, 3 to rb16 + 1 as word
  // 4 (t - 2) + e.  bits[(rb16 * (N / 32) + cb) * 8 + word].  Needs N % 32 == 0 and tile rows that are multiples of 16.
  unsigned long long* relu_bits;
  int allow_half;          // 1: tile heights that end with a 16-row half block may be chosen (the stack's projection)
  int concurrent;          // mmf_amil_desc::concurrent: plan the wide tiles for 224 of the 256 CUs
  int deep;                // set by launch_linear: short grid, use the deep-prefetch main loop
  int split;               // 1: the split-operand core (mmf_gemm_split.h) where the shape has a tile for it
  // K-split (short grids: a few dozen tiles, each a long serial K loop, on 256 CUs): `ksplit` workgroups share an output tile,
  // each contracts 1 / ksplit of K and writes its partial tile to kpart[(tile * ksplit + s)][BM x BN] with device-scope
  // stores; the LAST to arrive (ktick[tile]: a device-scope counter, zero before the launch and left zero by it) sums the
  // partials in split order -- deterministic -- and runs the epilogue.  No workgroup ever waits for another.
  // launch_linear sets ksplit from the plan (LinearPlan::ksplit: above 1 only when kpart / ktick are given).
  int ksplit;
  float* kpart;
  unsigned* ktick;
  int ktick_words;
  // grouped step (mmf_amil_nll_step_group): [M] per-row dropout index base, (row - bag start) * N + seed term of the
  // row's bag (group_rows_kernel).  Read only by the SEG instantiations; null otherwise.
  const uint32_t* seg_ridx;
};
// The projection's launch plan: every choice between linear_nt_kernel's launch forms, made once.
enum : int { LIN_SPLIT_WIDE, LIN_WIDE, LIN_128, LIN_SPLIT_64, LIN_KSPLIT_64, LIN_64 };
struct LinearPlan {
  int kind;                // LIN_*: split-operand 224 x 256 and 64 x 64; exact fp32 rows x 256, 128 x 128, 64 x 64 K-split, 64 x 64
  int rows;                // the tile's height: 64 .. 240 in steps of 16 for LIN_WIDE (odd multiples end in a half block)
  int ksplit;              // LinearParams::ksplit: 2 or 4 for LIN_KSPLIT_64, else 1
  int deep;                // short grid of 64-row tiles: the deep-prefetch main loop
  int mt_count, nt_count, grid;
  int kpart_floats;        // floats of LinearParams::kpart the launch writes (0: no K split)
};
// tick_words: the tick words on offer with partial-tile space (0: none, so no K split)
LinearPlan plan_linear(int64_t M, int N, int K, int nseg, int kseg, int allow_half, int concurrent, int split, int tick_words);
// size of LinearParams::kpart for this shape, whatever the mode and the tick words on offer: the exact-fp32 plan's
size_t linear_ksplit_floats(int64_t M, int N, int K, int nseg, int kseg);

struct GateFwdParams {
  const float* h;          // [N x H] (post ReLU/dropout)
  const float *Wa, *ba, *Wb, *bb, *Wc;
  float *a, *b;            // [N x D] un-dropped activations, saved for backward
  float* s_part;           // [nt_count x N]
  int64_t N;
  int H, D, gated;
  float drop_p;            // dropout on a / b (model_modules.py:97-99), 0 = off
  uint32_t key_a, key_b;
  const uint32_t* seed_dev;
  int mt_count, nt_count;
  int64_t row_begin, row_end;   // this launch's rows of the bag (set by launch_gate_fwd)
  // mixed launch (gate_fwd_mixed_kernel): up to 5 row regions in workgroup order, each of tall (128-row) or short
  // (64-row) tiles
  struct Region { int64_t row0; int mt_count, grid_begin, tall; } reg[5];
  int nreg;
  int deep;                     // set by launch_gate_fwd: short grid, use the deep-prefetch main loop
  int split;                    // 1: the split-operand core (mmf_gemm_split.h) where the shape has a tile for it
  const uint32_t* seg_ridx;     // grouped step: [N] dropout index base per row (width D), or null (LinearParams::seg_ridx)
};

// Optional tail behind K-merge, ONE single-workgroup launch (head_tail_kernel):
// the classifier + hazard head of models/model_attention_mil_path.py:58-61 and, when Y is given, nll_surv
// (utils/loss_utils.py:22-39) with its backward down to dM -- instead of the three launches surv_head_fwd, nll_surv,
// surv_head_bwd, each ~5 us of pure launch latency.
struct HeadTail {
  const float *Wk, *bk;        // [K x H], [K]; Wk == null: no tail
  int K;
  float *logits, *hazards, *S; // [K] each
  int64_t* Y_hat;              // [1]
  float* risk;                 // [1] = -sum_k S_k, or null
  // nll_surv + backward (Y == null: head only)
  const int64_t* Y; const float* c;
  float alpha, eps, loss_scale;
  float *loss;                 // [1], unscaled
  float *dM;                   // [H]   d(loss * loss_scale)/dM
  float *dWk, *dbk;            // [K x H], [K]; overwritten, or added to when accumulate != 0
  int accumulate;
};

struct PoolParams {
  const float* s_part;
  int n_parts;
  const float* bc;         // device scalar (attention_c.bias)
  const float* h;
  int64_t N;
  int H;
  float* A_raw;            // [N]
  float* partials;         // [n_groups x (2 + H)]
  float* M;                // [H]
  float* stats;            // {max, denom}
  int n_groups, rows_per_group;
  HeadTail tail;
};
constexpr int POOL_MAX_ROWS = 8192;   // rows of one pooling partial group (its scores stay in LDS)

struct BwdPrepParams {     // ds_i = p_i (dM.h_i - dM.M) + gA_i
  const float* h;
  const float* A_raw;
  const float* stats;
  const float* dM;         // [H]
  const float* M;          // [H]
  const float* gA;         // [N] or null
  int64_t N;
  int H;
  float* p;                // [N]
  float* ds;               // [N]
  float* dbc_part;         // [n_groups]
  int n_groups;
};

struct GateBwdCtx {        // what the on-the-fly dP operand needs
  const float *a, *b, *ds, *Wc;
  int D, gated;
  float drop_p;
  uint32_t key_a, key_b;
  const uint32_t* seed_dev;
  // loaders call this once on their private copy: fold the device-resident seed into the keys
  __device__ inline void resolve_seed() {
    if (seed_dev) { const uint32_t sd = *seed_dev; key_a += sd; key_b += sd; seed_dev = nullptr; }
  }
};

// dP[i][k] of one (instance, attention dim): part 0 = d pre-tanh, part 1 = d pre-sigmoid (formulas: mmf_amil_bwd.hip
// header); a_d_b_d returns the dropped a.b product (dWc needs it).  The gate / dropout / part switches are
// compile-time: callers sit in the staging path of a GEMM main loop, where a scalar branch per element costs more
// than the arithmetic it skips (the large-bag kernels are instantiated per (gated, dropout) and pick `part` per chunk).
template <bool GATED, bool DROP, int PART>
__device__ inline float gate_dp_t(const GateBwdCtx& g, float av, float bv, float wc, float dsv,
                                  uint32_t idx, uint32_t thr, float dscale, float& a_d_b_d) {
  float ma = 1.f, mb = 1.f;
  if constexpr (DROP) {
    ma = keep(g.key_a, idx, thr) ? dscale : 0.f;
    if constexpr (GATED) mb = keep(g.key_b, idx, thr) ? dscale : 0.f;
  }
  if constexpr (GATED) {
    a_d_b_d = (av * ma) * (bv * mb);
    return PART == 0 ? dsv * wc * (bv * mb) * ma * (1.f - av * av)
                     : dsv * wc * (av * ma) * mb * bv * (1.f - bv);
  }
  a_d_b_d = av * ma;
  return dsv * wc * ma * (1.f - av * av);
}
// the same with run-time switches (small-tile kernels, where the staging path is not the bottleneck)
__device__ inline float gate_dp(const GateBwdCtx& g, int part, float av, float bv, float wc, float dsv,
                                uint32_t idx, uint32_t thr, float dscale, float& a_d_b_d) {
  float ma = 1.f, mb = 1.f;
  if (g.drop_p > 0.f) {
    ma = keep(g.key_a, idx, thr) ? dscale : 0.f;
    if (g.gated) mb = keep(g.key_b, idx, thr) ? dscale : 0.f;
  }
  if (g.gated) {
    a_d_b_d = (av * ma) * (bv * mb);
    return part == 0 ? dsv * wc * (bv * mb) * ma * (1.f - av * av)
                     : dsv * wc * (av * ma) * mb * bv * (1.f - bv);
  }
  a_d_b_d = av * ma;
  return dsv * wc * ma * (1.f - av * av);
}

struct BwdDhParams {       // du = (dP.Wab + p dM) * relu'(h) * scale_h
  GateBwdCtx g;
  const float *Wa, *Wb;    // [D x H]
  const float* p;          // [N]  (read when !fused_prep)
  const float* dM;         // [H]
  const float* h;          // [N x H]
  const unsigned long long* relu_bits;   // LinearParams::relu_bits of the forward, or null (then h is re-read in the epilogue)
  float* du;               // [N x H]
  int64_t N;
  int H;
  float scale_h;           // 1/(1-p_h) in train mode, 1 in eval
  int mt_count, nt_count;
  int deep;                // DhPlan::deep, as are mt_count and nt_count: set by launch_bwd_dh from the plan
  int allow_half;          // not read: the plan allows half-block heights exactly where it fuses K-prep
  int concurrent;          // mmf_amil_desc::concurrent
  int split;               // 1: the split-operand core (mmf_gemm_split.h) where the plan has a tile for it
  // fused prep (DhPlan::fused, set by launch_bwd_dh): the kernel computes p_i, ds_i itself (K-prep's job), keeps them
  // in LDS for its loader / epilogue and publishes them for the TN kernel
  int fused_prep;
  const float *A_raw, *stats, *Mpool, *gA;
  float *p_out, *ds_out, *dbc_part;
  // grouped step (SEG instantiations, never fused): dM is [G x H], row i takes dM of bag seg_bag[i]; dP's masks index
  // through seg_ridx (GateFwdParams::seg_ridx)
  const uint32_t* seg_ridx;
  const int* seg_bag;
};

enum : int { TN_A_PLAIN = 0, TN_A_GATE = 1 };

struct TnProblem {         // C[M x Ncols] (+)= A^T . B over a slice of the K (instance) range
  int kind;
  const float* A; int lda; int M;          // TN_A_PLAIN: A[k][m]; TN_A_GATE: M = 2D (gated) or D
  const float* B; int ldb; int Ncols;      // B[k][n]
  float* out; size_t split_stride; int ldc;  // slab s at out + s*split_stride
  float* colsum; size_t colsum_stride;       // per split: column sums of A (bias grads), length M; null = skip
  float* colsum2; size_t colsum2_stride;     // TN_A_GATE only: dWc partials, length D
  int tiles_m, tiles_n, block_begin;       // block_begin: first workgroup of the problem in the plain block order
  int tile_begin;                          // first tile index of the problem (over all problems, set by launch_tn)
  int splits, k_per_split;                 // this problem's K split (set by launch_tn: the plan's, a gate problem its own)
};

struct TnParams {
  TnProblem prob[6];
  int nprob;
  int64_t K;               // number of instances (rows of A and B)
  int splits, k_per_split; // TnPlan's, set by launch_tn
  int total_tiles;         // tiles over all problems (set by launch_tn)
  int xcd_map;             // 0: plain order (problem, split, tile); 2: block -> (split, tile) through `map`
  int tile;                // 128 or 256 (TnPlan::tile, set by launch_tn)
  int split;               // 1: split-operand 256 x 256 tiles (mmf_gemm_split.h) when tile == 256
  GateBwdCtx g;
  // xcd_map == 2: map[b] = split << 5 | tile (0xFFFF: no work).  Blocks b, b+8, b+16, ... run on the same XCD, and
  // launch_tn() packs the tiles of one (split, problem) -- which read the same A or B panel -- next to each other
  // there, so a panel is fetched from HBM once per XCD instead of once per tile.
  uint16_t map[512];
  const uint32_t* seg_ridx;   // grouped step with attention dropout: dP's mask index base per instance, or null
};

struct NnParams {          // C[M x N] = A[M x K] . B[K x N]   (plain; radio: dh0 = du.W1)
  const float* A; int lda;
  const float* B; int ldb;
  float* C; int ldc;
  int64_t M;
  int N, K;
  int mt_count, nt_count;
  // attribution epilogue (launch_nn_attr, mmf_amil_ig): the product is multiplied by mulx [M x N] (row pitch ldx) in
  // registers; C may then be null (the product never reaches memory); per row and 32-column block the sum and the sum of
  // absolute values of the products go to rs_part / ra_part [(N / 32) x M], for ig_rows_kernel to add in block order
  const float* mulx; int ldx;
  float *rs_part, *ra_part;
  // segmented attribution (launch_nn_attr_seg, mmf_radio_ig): the N = nseg * kseg columns are nseg modalities side by side,
  // kseg % 32 == 0; 32-column block b belongs to segment b * 32 / kseg, whose multiplier is segx[m] [M x kseg] and whose
  // product, when C is given, goes to C + m * M * kseg [M x kseg]; mulx, ldx and ldc are not read
  const float* segx[4]; int kseg;
};

struct ReduceSeg { const float* in; float* out; int len; int nsplit; size_t stride; int block_begin; int tall; };
struct ReduceParams { ReduceSeg seg[12]; int nseg; int accumulate; };   // accumulate: out += sum instead of out = sum

int launch_linear(LinearParams p, hipStream_t st);
int launch_linear_seg(LinearParams p, hipStream_t st);   // grouped step: the dropout epilogue indexes through p.seg_ridx
// The gate forward's launch plan: 64-row tiles, uniform 128-row tiles, or both heights in one launch (GateFwdParams::reg).
enum : int { GATE_64, GATE_128, GATE_MIXED };
struct GatePlan {
  int kind;                // GATE_*
  int split;               // the split-operand tiles (mmf_gemm_split.h) are taken
  int deep;                // short grid of exact-fp32 64-row tiles: the deep-prefetch main loop
  int mt_count, nt_count, grid;   // nt_count: gate_parts; mt_count: row tiles (GATE_MIXED: over all regions)
  int nreg;                // GATE_MIXED: the regions, in workgroup order (GateFwdParams::Region, rows as int)
  struct Region { int row0, mt_count, grid_begin, tall; } reg[5];
};
GatePlan plan_gate_fwd(int64_t N, int H, int D, int gated, int split);
int gate_parts(int D, int gated);
int launch_gate_fwd(GateFwdParams p, hipStream_t st);
int launch_gate_fwd_seg(GateFwdParams p, hipStream_t st);
int pool_groups(int64_t N);
int launch_pool(PoolParams p, hipStream_t st);
int launch_score_sum(const float* s_part, int n_parts, const float* bc, float* A, int64_t N, hipStream_t st);
int launch_head_tail(PoolParams p, hipStream_t st);    // head_tail_kernel alone on the feature vector p.M [p.H]
int launch_pool_merge(PoolParams p, hipStream_t st);   // single-workgroup merge of p.n_groups partials -> M, stats
int launch_bwd_prep(BwdPrepParams p, hipStream_t st);

// K-dh's launch plan: every choice between bwd_dh_kernel's launch forms, made once.  A caller builds it, runs K-prep as
// its own launch where the plan does not fuse it, hands `dbc_groups` (or its own K-prep's) to the reduce list and the
// plan to the launcher.
constexpr int PREP_GROUPS = 512;           // capacity of dbc_part: K-prep's partials, its own launch's or K-dh's
enum : int { DH_SPLIT_WIDE, DH_SPLIT_64, DH_WIDE, DH_128, DH_64X128, DH_64 };
struct DhPlan {
  int kind;                // DH_*: split-operand rows x 256 and 64 x 64; exact fp32 rows x 256, 128 x 128, 64 x 128, 64 x 64
  int rows;                // the tile's height: 64 .. 224 in steps of 16 for DH_WIDE (odd multiples end in a half block)
  int fused;               // K-prep runs inside K-dh: the caller launches none
  int variant;             // gate / dropout switches compiled in, (gated ? 2 : 0) + (dropout ? 1 : 0); -1: kept at run time
  int deep;                // short grid of 64-row tiles: the deep-prefetch main loop (dh_mainloop_deep)
  int mt_count, nt_count, grid;
  int extra_lds;           // dynamic LDS bytes behind the staging buffers (fused K-prep's ds, p and scratch)
  int dbc_groups;          // dbc partials K-dh writes: mt_count when fused (dbc_part[mt]), else 0
};
// can_fuse: the caller has A_raw, the softmax statistics, M and the forward's relu bits (the stack's one-bag backward; not the
// scorer, not the grouped chain, whose plan is otherwise the same); dbc_cap: the capacity of dbc_part
DhPlan plan_bwd_dh(int64_t N, int H, int D, int gated, int dropout, int split, int concurrent, int can_fuse, int dbc_cap);
int launch_bwd_dh(const DhPlan& pl, BwdDhParams p, hipStream_t st);
// grouped step (the SEG instantiations): per-row bag dM and mask index; refuses a fused or split-operand plan
int launch_bwd_dh_seg(const DhPlan& pl, BwdDhParams p, hipStream_t st);
// split-operand mode on bags below the wide tiles: instances from which the small split tiles (64-row GEMM tiles, 128 x 128
// TN tile) are taken instead of the exact-fp32 ones (default 1: every bag, which keeps an instance's score independent of its bag's size)
int split_min_rows();
// The split-K plan of the TN GEMM, shared by the workspace carving and the launcher.  256 x 256 tiles (8 waves, one workgroup
// per CU) from 12,288 instances; `splits` workgroups share a tile, each over k_per_split instances.
enum : int { TN_128, TN_256, TN_SPLIT_128, TN_SPLIT_256 };
struct TnShape { int M, Ncols, gate; };     // one problem: C[M x Ncols]; gate: TN_A_GATE (M = 2 D gated, D ungated)
struct TnPlan {
  int kind, tile;          // TN_*: exact fp32 128 x 128, 256 x 256; split-operand 128 x 128, 256 x 256; tile: 128 or 256
  int splits, k_per_split; // k_per_split is a multiple of 4
  int splits_g, k_per_split_g;   // the gate problems' split: more, shorter splits beside a plain problem on 256 x 256 tiles
  int tiles;               // tiles over all shapes
};
TnPlan plan_tn(int64_t K, int split, const TnShape* shapes, int nshape);
// sets tile, splits and k_per_split of p and of every problem from the plan
int launch_tn(const TnPlan& pl, TnParams p, hipStream_t st);
// wide (32*MB x 256, one 8-wave workgroup per CU) tile selection, shared by the row-parallel GEMMs
int pick_wide_rows(int64_t M, int ntn, bool allow_half, bool concurrent, int max_rows);
bool use_wide_tiles(int64_t M, int N, int split = 0);   // split: the bf16x3 mode's (later) crossover
// a grid this short leaves every workgroup alone on its CU: the deep-prefetch main loops (projection, gate, K-dh)
bool short_grid(int64_t workgroups);
int launch_nn(NnParams p, hipStream_t st);
int launch_reduce(ReduceParams p, hipStream_t st);

// ---- grouped step (mmf_amil_nll_step_group): G bags of one accumulation window as one launch chain ----------------
constexpr int GROUP_MAX = 64;              // MMF_GROUP_MAX
constexpr int GROUP_POOL_GROUPS = 256;     // pooling partial groups planned over the window (plus at most one per bag)
struct SegTable {
  int G;
  int rows_per_group;                      // pooling: rows per partial group (groups never straddle a bag)
  int64_t off[GROUP_MAX + 1];              // bag g = rows off[g] .. off[g + 1] - 1
  int gbeg[GROUP_MAX + 1];                 // bag g's pooling partials are gbeg[g] .. gbeg[g + 1] - 1
  uint32_t ibase[GROUP_MAX];               // seed_g * inverse(0x9E3779B1): hash_u32(drop_key(0, s), i + ibase) ==
                                           // hash_u32(drop_key(seed_g, s), i)
};
struct GroupRowsParams { SegTable s; int H, D; uint32_t *ridx_h, *ridx_d; int* bag; };
int launch_group_rows(const GroupRowsParams& p, hipStream_t st);
// pooling over every bag (partials never straddle a bag), then one 1024-thread workgroup per bag: merge + head tail.
// p.M / p.stats / p.tail outputs are per-bag arrays ([G x H], [G x 2], [G x K], [G]); tail.dWk / dbk are per-bag slabs
// [G x K x H], [G x K] (overwritten; the reduce launch sums them); tail.dM is [G x H].
int launch_group_pool(PoolParams p, const SegTable& s, hipStream_t st);
// ds_i / p_i with the statistics, M and dM of row i's bag
int launch_group_bwd_prep(BwdPrepParams p, const int* bag, hipStream_t st);
// every pooling launch over a window checks it with this: H, G, rows per partial group, partials per bag
int group_pool_check(const PoolParams& p, const SegTable& s);
// forward-only grouped pass (mmf_amil_infer_group): the pooling partials of launch_group_pool alone, and a tail of one
// workgroup per bag that merges the bag's partials into M_g (p.M [G x H], or null: not stored) and runs the head's
// forward (p.tail per-bag outputs as in launch_group_pool; Y given: loss [G] only; dM / dWk / dbk are not read).  The
// merge and the head are the device functions launch_group_pool's tail runs, the head with its backward compiled out.
int launch_group_pool_partial(PoolParams p, const SegTable& s, hipStream_t st);
int launch_group_infer_tail(PoolParams p, const SegTable& s, hipStream_t st);
// grouped multimodal step: the merge of launch_group_pool without the head tail -- M_g to p.M + g * ldm (the caller's
// feature matrix) and to Mw [G x H], stats_g to p.stats [G x 2] (p.partials from launch_group_pool_partial); the dM
// columns of one stack out of a [G x ld] matrix; and the hazard head of G patients over p.M = feat [G x ldf], p.H = F
// (per-patient p.tail arrays as in launch_group_pool; tail.dM = dfeat [G x F])
int launch_group_merge(PoolParams p, const SegTable& s, int ldm, float* Mw, hipStream_t st);
int launch_group_dm_gather(const float* src, int ld, float* dst, int G, int H, hipStream_t st);
int launch_surv_head_group(PoolParams p, int ldf, int G, hipStream_t st);
// forward-only hazard head of G patients (mmf_surv_head_infer_group): patient g's feature row is the concatenation of
// row g of s.n dense [G x width] buffers (sum width = p.H <= 1024); p.M is null, p.tail as in launch_group_infer_tail
struct HeadSegs { const float* x[3]; int width[3]; int n; };
int launch_surv_head_infer_group(PoolParams p, const HeadSegs& s, int G, hipStream_t st);

// ---- integrated gradients of the pathology head (mmf_amil_ig): the steps of a window stand in as its bags ------------
// step s of the window: interpolation factor alpha[s] and quadrature weight w[s] (kernel arguments: no device table)
struct IgSteps { int S; float alpha[GROUP_MAX]; float w[GROUP_MAX]; };
// h[s * N + i, :] = relu(alpha_s * U[i, :] + b1) and its bits (LinearParams::relu_bits' layout) over the window's S * N rows
struct IgExpandParams {
  const float* U;            // [N x H] = x . W1^T, no bias
  const float* b1;           // [H]
  float* h;                  // [S * N x H]
  unsigned long long* relu_bits;
  int64_t N;
  int H;
  IgSteps st;
};
int launch_ig_expand(const IgExpandParams& p, hipStream_t st);
// The hazard head forward and the backward of risk = -sum_k S_k, one workgroup per step of the window: M [S x H] -> dM
// [S x H] = d risk / d M_s, and the risk where the step's place in the call says -- steps 0 .. n_steps - 1 of the call
// are the quadrature's (step_risk), step n_steps is alpha = 1 (risk_x and the optional head outputs), n_steps + 1 alpha = 0
struct IgHeadParams {
  const float* M;
  const float *Wk, *bk;
  int K, H;
  float* dM;
  int step0, n_steps;        // the window's first step in the call, and the call's quadrature steps
  float *step_risk, *risk_x, *risk_base;
  float *logits, *hazards, *S, *risk;   // [K], [K], [K], [1] at alpha = 1, each may be null
  int64_t* Y_hat;                       // [1] or null
};
int launch_ig_head(const IgHeadParams& p, int S, hipStream_t st);
// The tensor fusion's node launch (mmf_mm_ig_tensor), one workgroup per node s of the window: hid = relu(Wc0 MM_s + bc0)
// kept in LDS, the hazard head over it and the backward of risk (hp, whose H is nhid <= 1024 and whose M / dM are not
// read), dpre0 = dhid . [hid > 0], dMM_s = dpre0 . Wc0 into dMM [S x N2].  MM [S x N2], Wc0 [nhid x N2], N2 <= 1536.
struct XIgHeadParams {
  IgHeadParams hp;
  const float *MM, *Wc0, *bc0;
  float* dMM;
  int N2;
};
int launch_xfusion_ig_head(const XIgHeadParams& p, int S, hipStream_t st);
// G[i, :] (first: =, else +=) sum_s w[s] * du[s * N + i, :] over the first st.S steps of the window, in step order
struct IgFoldParams { const float* du; float* G; int64_t N; int H; int first; IgSteps st; };
int launch_ig_fold(const IgFoldParams& p, hipStream_t st);
// P = A . B times mulx, never stored unless p.C is given, and its per-row sums (NnParams' attribution fields), then
// row_sum / row_abs [M] from the partials in column-block order: fixed order, no atomics
int launch_nn_attr(NnParams p, float* row_sum, float* row_abs, hipStream_t st);
// the radiology head (mmf_radio_ig).  out[j] = b1[j] + sum_l W1[j, l] br[l]: reduce_dim's bias behind the projection [H]
int launch_ig_bias(const float* W1, const float* br, const float* b1, float* out, int H, int L, hipStream_t st);
// launch_nn_attr over nseg = p.N / p.kseg modalities (NnParams' segmented fields): row_sum / row_abs [nseg x M], each
// modality's kseg / 32 partials added in block order
int launch_nn_attr_seg(NnParams p, float* row_sum, float* row_abs, hipStream_t st);
// the multimodal head (mmf_mm_ig): the omic SNN without weight gradients.  x [Gin]; W0 [W0n x Gin], b0; W1 [We x W0n], b1.
// Stages: Z = W0 x once per call; per window the forward (z1, z2 kept; O_s into columns col .. col + We - 1 of feat [S x F])
// and the backward (dfeat's same columns -> dz1 [S x W0n]) with one workgroup per node, and the fold Gz (+)= sum_s w_s
// dz1_s over the first st.S nodes; attr[j] = x[j] sum_c Gz[c] W0[c, j] once per call.  W0n, We <= 1024.
enum : int { IG_OMIC_Z, IG_OMIC_FWD, IG_OMIC_BWD, IG_OMIC_FOLD, IG_OMIC_ATTR };
struct IgOmicParams {
  const float *x, *W0, *b0, *W1, *b1;
  int Gin, W0n, We;
  float *Z, *z1, *z2, *dz1, *Gz;   // [W0n], [S x W0n], [S x We], [S x W0n], [W0n]
  float* feat;
  const float* dfeat;
  int F, col;
  float* attr;                     // [Gin]
  int first;                       // the fold overwrites Gz
  IgSteps st;
};
int launch_ig_omic(int stage, const IgOmicParams& p, hipStream_t st);

// ---- integrated gradients of the stage-2 fusion models (mmf_stage2_ig, csrc/mmf_stage2_ig.hip) ---------------------------
constexpr int S2_MAXW = 768;        // the packed row [v_0 | v_1 | v_2] and the widest layer behind it
constexpr int S2_MAXPROB = 9;       // first-layer matrices of a model: three gates of three Highway blocks
struct S2Bn { const float *w, *b, *mean, *var; float eps; };      // eval-mode BatchNorm1d; w null: none
// one first-layer matrix W [n_out x k_in]: it reads columns in_col .. in_col + k_in - 1 of the packed row (whole
// modalities) and owns columns out_col .. out_col + n_out - 1 of U and G
struct S2Lin { const float *W, *bias; int n_out, k_in, in_col, out_col; };
// the two contractions of a call.  fold_fwd: U [(P + 1) x ldU] = (v . s1) W^T per problem, row P = t1 W^T + bias (in_bn[i]:
// the bn1 that modality i's columns pass, or none).  attr: dx = sum_prob G W, attr[i] [P x 256] (or null) = v_i . s1 . dx and
// its sums mod_sum / mod_abs [P x m]
struct S2FoldParams {
  const float* v[3];
  S2Bn in_bn[3];
  S2Lin prob[S2_MAXPROB];
  int m, P, nprob, ldU;
  float* U;
  const float* G;
  float* attr[3];
  float *mod_sum, *mod_abs;
};
int launch_stage2_fold_fwd(const S2FoldParams& p, hipStream_t st);
int launch_stage2_attr(const S2FoldParams& p, hipStream_t st);
// the node sweep, one workgroup per patient: W units behind the first layer (fcnn: one plane of U, BN bn[j / bn_span] and
// ReLU; highway: the planes gate | nonlinear | linear, the mix and bn2 = bn[j / bn_span]), the classifier Wk [K x W] and
// the hazard head (nll) or the scalar risk (cox, K = 1; late_cox: Wk [1 x W / 128] over the blocks' own Linear(128, 1) W4,
// b4).  alpha / weight: the n_steps nodes, then the riders alpha = 1 and alpha = 0.  G [P x ldU] = sum_k w_k d risk_k / d U
struct S2SweepParams {
  const float* U;
  float* G;
  int ldU, W, P, K, n_steps, highway, cox, late_cox, bn_span;
  S2Bn bn[3];
  const float *Wk, *bk;
  const float *W4[3], *b4[3];
  float alpha[GROUP_MAX + 2], weight[GROUP_MAX + 2];
  float *step_risk, *risk, *risk_base, *hazards, *S;   // [P x n_steps], [P], [P], [P x K] or null twice
};
int launch_stage2_sweep(const S2SweepParams& p, hipStream_t st);
// kronecker: the launches around the tensor fusion's grouped tail for one window of S (patient, node) rows, row g0 + s of
// the call = patient * T + node, T = n_steps + 2.  EXPAND: the embedding columns of x2 [S x K2] (first column N1) = alpha_node
// v_i; HEAD: MM [S x 256] -> the risks at the rows' places and dMM [S x 256] = d risk / d MM (Wk [K x 256]; cox: K = 1, the
// scalar); FOLD: Gacc [P x m 256] (=, +=) sum_node w_node dx2's embedding columns, in node order whatever the windows are;
// ATTR, once per call: attr_i = v_i . Gacc, mod_sum / mod_abs [P x m].  alpha / weight: T values, the riders' weights 0
enum : int { S2_KRON_EXPAND, S2_KRON_HEAD, S2_KRON_FOLD, S2_KRON_ATTR };
struct S2KronParams {
  const float* v[3];
  int m, P, n_steps, T, g0, S, N1, K2, K, cox;
  float alpha[GROUP_MAX + 2], weight[GROUP_MAX + 2];
  float* x2;
  const float *MM, *dx2;
  float *dMM, *Gacc;
  const float *Wk, *bk;
  float *step_risk, *risk, *risk_base, *hazards, *S_out;
  float* attr[3];
  float *mod_sum, *mod_abs;
};
int launch_stage2_kron(int stage, const S2KronParams& p, hipStream_t st);
// highway with n_layers >= 2: the launches around the window's layers >= 1 (dense row kernels and the highway mix), rows as
// for kronecker, up to S2_HW_ROWS a window.  Activations lie block by block (W / wd Highways of wd units): unit j of row
// s at [(j / wd) * blk_stride + s * wd + j % wd].  BEGIN: X0 = layer 0's output from U [(P + 1) x 3 W]; HEAD: XL (the last
// layer's output) -> bn2, the risks at the rows' places, dXL = d risk / d XL; END: G [P x 3 W] (=, +=) sum_node w_node d
// risk / d z_* of layer 0, from dX0 and U, in node order whatever the windows are
constexpr int S2_HW_ROWS = 256;      // the dense backward's one-launch form takes up to 256 rows
enum : int { S2_HW_BEGIN, S2_HW_HEAD, S2_HW_END };
struct S2HwParams {
  const float* U;
  int ldU, W, wd, P, n_steps, T, g0, S, K, cox;
  size_t blk_stride;
  float alpha[GROUP_MAX + 2], weight[GROUP_MAX + 2];
  float* X0;
  const float* XL;
  float* dXL;
  const float* dX0;
  float* G;
  S2Bn bn2[3];
  const float *Wk, *bk;
  float *step_risk, *risk, *risk_base, *hazards, *S_out;
};
int launch_stage2_hw(int stage, const S2HwParams& p, hipStream_t st);
int launch_stage2_hw_add3(const float* a, const float* b, const float* c, float* out, int n, hipStream_t st);

// ---- one-call training step of the stage-2 fcnn and highway models (csrc/mmf_stage2_step.hip) -----------------------------------
// A "branch" is one fcnn block or one Highway: the early types have one over the cat, the late types one per modality (the
// forward runs all three, the head and the backward the ones the mode keeps).  Activations lie feature-major, [feature x ldB].
struct S2sBn { const float *w, *b; float *rmean, *rvar; float eps, momentum; };
enum : int { S2S_LOSS_NLL, S2S_LOSS_COX, S2S_LOSS_RANK, S2S_LOSS_RANK_NLL };
// the loss over the head's outputs: risk [B], hazards / S [B x K] (nll family); scale multiplies the gradient alone
struct S2sLoss {
  int kind, phi, reduction, K, B, cox;
  float alpha, ratio, scale;
  const int64_t* Y;
  const float* c;
  const double* times;
  const float *risk, *hazards, *S;
  float* loss;
};
struct S2sFcnnFwdBr {
  const float* x[3];                 // the block's input: nseg embeddings [B x 256]
  int nseg;
  const float *W0, *b0;              // [128 x 256 nseg], [128]
  S2sBn bn;
  uint32_t key;                      // drop_key(seed, site)
  float *uT, *yT, *stat;             // pre-BN [128 x ldB]; output [128 x ldB] or null (the dropped modality); mean | invstd [256]
};
struct S2sFcnnFwd {
  S2sFcnnFwdBr br[3];
  int nbr, B, ldB, training;
  float p;
  const uint32_t* seed_dev;
};
int launch_s2s_fcnn_fwd(const S2sFcnnFwd& p, hipStream_t st);
struct S2sBn1FwdBr {
  const float* x[3];
  S2sBn bn;
  uint32_t key;
  float *xT, *xR, *stat;             // x0 feature-major [D x ldB] and row-major [B x D]; mean | invstd [2 D]
};
struct S2sBn1Fwd {
  S2sBn1FwdBr br[3];
  int nbr, D, B, ldB, training;
  float p;
  const uint32_t* seed_dev;
};
int launch_s2s_bn1_fwd(const S2sBn1Fwd& p, hipStream_t st);
struct S2sHwFwdBr {
  const float* xT;                   // the layer's input [D x ldB]
  const float *W[3], *bias[3];       // gate | nonlinear | linear
  float* zT[3];                      // the three pre-activations [D x ldB]
  float *yT, *yR;                    // the mix [D x ldB]; row-major [B x D] unless last
  S2sBn bn2;                         // last layer
  float *stat2, *fT;                 // mean | invstd [2 D]; bn2's output [D x ldB] or null (the dropped modality)
};
struct S2sHwFwd {
  S2sHwFwdBr br[3];
  int nbr, D, B, ldB, training, last;
};
int launch_s2s_hw_fwd(const S2sHwFwd& p, hipStream_t st);
// the classifier over fT [W x ldB], the hazard head (nll) or the scalar (cox); late_cox: m blocks of 128 features pass their
// own W4 [128], b4 [1] first (the scalars kept in sblk [B x 3]), Wk [m].  with_loss: one workgroup, which ends with the loss
struct S2sHead {
  const float* fT;
  int W, B, ldB, K, cox, late_cox, m, with_loss;
  const float *Wk, *bk;
  const float *W4[3], *b4[3];
  float* sblk;
  float *risk, *hazards, *S;
  S2sLoss loss;
};
int launch_s2s_head(const S2sHead& p, hipStream_t st);
struct S2sFcnnBwdBr {
  const float* x[3];
  int nseg, ycol0, slot;             // the block's first column in the classifier's input; its place in the cat
  const float *uT, *stat;
  S2sBn bn;
  const float* W4;
  float *dW0, *db0, *dgamma, *dbeta, *dW4, *db4;
};
struct S2sFcnnBwd {
  S2sFcnnBwdBr br[3];                // the blocks the mode keeps
  int nbr, B, ldB, training, accumulate, late_cox, W;
  float p;
  const float* yT;                   // [W x ldB], as the head read it
  const float *Wk, *sblk;
  float *dWk, *dbk;
  S2sLoss loss;
};
int launch_s2s_fcnn_bwd(const S2sFcnnBwd& p, hipStream_t st);
enum : int { S2S_HW_TOP, S2S_HW_MID, S2S_HW_BN1 };
struct S2sHwBwdBr {
  const float *dzT_in[3], *Wup[3];   // MID, BN1: dz of the layer above [D x ldB] and its weights
  const float *fT, *yT, *stat2;      // TOP: bn2's output and input, its statistics
  int fcol0;                         // TOP: the Highway's first column in the classifier's input
  S2sBn bn2;
  float *dgamma2, *dbeta2;
  const float* zT[3];                // TOP, MID: this layer's pre-activations, its input row-major, where dz and the
  float* dzT_out[3];                 // gradients go
  const float* xR;
  float *dW[3], *db[3];
  const float* x[3];                 // BN1: the embeddings, bn1, its statistics, the dropout key
  S2sBn bn1;
  const float* stat1;
  uint32_t key;
  float *dgamma1, *dbeta1;
};
struct S2sHwBwd {
  S2sHwBwdBr br[3];                  // the Highways the mode keeps
  int nbr, D, B, ldB, training, mode, accumulate, W;
  float p;
  const uint32_t* seed_dev;
  const float* Wk;
  float *dWk, *dbk;
  S2sLoss loss;
};
int launch_s2s_hw_bwd(const S2sHwBwd& p, hipStream_t st);

int set_dyn_lds(const void* kern, int bytes);

// Optional per-kernel timing with HIP events on the launch stream: records into the mmf_trace of the ABI call in
// progress (mmf_amil_desc::trace, thread-local while the call runs); no cost when the call carries none.
void prof_begin(const char* name, hipStream_t st);
void prof_end(hipStream_t st);
struct ProfScope {
  hipStream_t st;
  ProfScope(const char* name, hipStream_t s) : st(s) { prof_begin(name, s); }
  ~ProfScope() { prof_end(st); }
};

// a wide tile's height (64 .. MAX rows in steps of 16) as a compile-time constant: f(std::integral_constant<int, rows>)
template <int MAX, int R = 64, class F>
int with_wide_rows(int rows, F&& f) {
  if constexpr (R <= MAX) return rows == R ? f(std::integral_constant<int, R>{}) : with_wide_rows<MAX, R + 16>(rows, f);
  else return MMF_ERR_ARG;
}

// One launch of a tiled kernel: T::NT threads, T's dynamic LDS and `extra_bytes` behind it
template <class T, class P>
int launch_tiled(const char* name, void (*kern)(P), const P& p, int grid, hipStream_t st, int extra_bytes = 0) {
  const int bytes = T::LDS_BYTES + extra_bytes;
  if (int e = set_dyn_lds(reinterpret_cast<const void*>(kern), bytes)) return e;
  ProfScope ps(name, st);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(T::NT), bytes, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

}  // namespace mmf
