// C ABI (include/mmf_amil.h): argument checks, workspace carving, kernel sequencing.
// No allocation, no host synchronisation, no global mutable state except the (mutex-guarded)
// "dynamic LDS attribute already set" set.  The device-resident dropout seed and the kernel trace are per-call
// arguments; the trace of the call in progress is held in a thread_local for the launchers (ProfScope).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/mmf_amil.h"
#include "mmf_common.h"
#include "mmf_gemm_core.h"
#include "mmf_kernels.h"
#include "mmf_small.h"
#include "mmf_mlp.h"
#include "mmf_bf16.h"

namespace mmf {

int set_dyn_lds(const void* kern, int bytes) {
  if (bytes <= 48 * 1024) return MMF_OK;
  static std::mutex mu;
  static std::unordered_set<const void*> done;
  std::lock_guard<std::mutex> lock(mu);
  if (done.count(kern)) return MMF_OK;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return MMF_ERR_LAUNCH;
  done.insert(kern);
  return MMF_OK;
}

}  // namespace mmf

// Caller-owned kernel trace (include/mmf_amil.h "Kernel trace"): HIP event pairs recorded on the launch stream.
struct mmf_trace {
  struct Rec { const char* name; hipEvent_t a, b; };
  std::mutex mu;
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;      // events are reused across dumps
  int cap = 0;
};

namespace mmf {

static thread_local mmf_trace* tls_trace = nullptr;
struct TraceScope {                  // the ABI entry that carries a trace makes it current for its launches
  mmf_trace* prev;
  explicit TraceScope(mmf_trace* t) : prev(tls_trace) { tls_trace = t; }
  ~TraceScope() { tls_trace = prev; }
};

void prof_begin(const char* name, hipStream_t st) {
  mmf_trace* t = tls_trace;
  if (!t) return;
  std::lock_guard<std::mutex> lock(t->mu);
  if ((int)t->recs.size() >= t->cap) return;
  auto take = [&](hipEvent_t& e) {
    if (!t->pool.empty()) { e = t->pool.back(); t->pool.pop_back(); return true; }
    return hipEventCreate(&e) == hipSuccess;
  };
  mmf_trace::Rec r{name, nullptr, nullptr};
  if (!take(r.a)) return;
  if (!take(r.b)) { t->pool.push_back(r.a); return; }     // the first event goes back to the pool, not lost
  hipEventRecord(r.a, st);
  t->recs.push_back(r);
}
void prof_end(hipStream_t st) {
  mmf_trace* t = tls_trace;
  if (!t) return;
  std::lock_guard<std::mutex> lock(t->mu);
  if (!t->recs.empty()) hipEventRecord(t->recs.back().b, st);
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Bump allocator over a caller's workspace: every slot starts on a 256-byte boundary.  With a null base it only counts
// (the *_workspace_bytes queries); `off` is the size carved so far.
struct Carver {
  uintptr_t base;
  size_t off = 0;
  explicit Carver(void* b = nullptr) : base(reinterpret_cast<uintptr_t>(b)) {}
  template <class T> T* take(size_t n) {
    T* r = reinterpret_cast<T*>(base + off);
    off += align_up(n * sizeof(T), 256);
    return r;
  }
};

// The segments of one reduce launch.  add() refuses a segment past the last slot, and the launch then refuses the list.
struct ReduceList {
  ReduceParams p{};
  int err = MMF_OK;
  int add(const float* in, float* out, int len, int nsplit, size_t stride) {
    constexpr int cap = (int)(sizeof(p.seg) / sizeof(p.seg[0]));
    if (p.nseg == cap) return err = MMF_ERR_SHAPE;
    p.seg[p.nseg++] = ReduceSeg{in, out, len, nsplit, stride, 0, 0};
    return MMF_OK;
  }
  int launch(int accumulate, hipStream_t st) {
    if (err) return err;
    p.accumulate = accumulate;
    return launch_reduce(p, st);
  }
};

// The gradient pointers a stack backward writes, and their alignment (dx: the input gradient, where the entry point
// takes one)
static int check_grads(const mmf_amil_desc* d, const mmf_amil_grads* g) {
  if (!g->dW1 || !g->db1 || !g->dWa || !g->dba || !g->dWc || !g->dbc) return MMF_ERR_ARG;
  if (d->gated && (!g->dWb || !g->dbb)) return MMF_ERR_ARG;
  return MMF_OK;
}
static bool grads_aligned(const mmf_amil_desc* d, const mmf_amil_grads* g) {
  return aligned16(g->dW1) && aligned16(g->dWa) && (!d->gated || aligned16(g->dWb)) && (!g->dx || aligned16(g->dx));
}

struct AmilWs {
  float *M_step, *dM_step;           // [H] each: pooled embedding and its gradient inside mmf_amil_nll_step
  unsigned long long* relu_bits;     // [ceil(N/16)][H/32][8]: h > 0 per element (LinearParams::relu_bits)
  float *h, *a, *b, *s_part, *partials, *stats, *p, *ds, *dbc_part, *du;
  float *slab_w1, *slab_wab, *cs_b1, *cs_bab, *cs_wc;
  float* kpart;                      // partial tiles of a K-split projection (LinearParams::kpart), or null
  int parts, groups, mstk;
  TnPlan tn;                         // the split-K plan of the stack's two problems (its splits size the slabs)
  size_t bytes;
};

static AmilWs carve(Carver& c, int64_t N, int L, int H, int D, int gated, bool infer = false) {
  AmilWs w{};
  auto take = [&](size_t n) { return c.take<float>(n); };
  w.parts = gate_parts(D, gated);
  w.groups = pool_groups(N);
  w.mstk = gated ? 2 * D : D;
  const TnShape shapes[2] = {{H, L, 0}, {w.mstk, H, 1}};       // dW1 beside the gate problem d[Wa ; Wb]
  w.tn = plan_tn(N, 0, shapes, 2);
  const int splits = w.tn.splits;
  w.M_step = take(H);
  w.dM_step = take(H);
  w.h = take((size_t)N * H);
  w.s_part = take((size_t)w.parts * N);
  w.partials = take((size_t)w.groups * (2 + H));
  w.stats = take(4);
  {
    const size_t kf = linear_ksplit_floats(N, H, L, 1, L);
    w.kpart = kf ? take(kf) : nullptr;
  }
  if (infer) {            // forward-only: nothing is kept for a backward (relu_bits, a, b stay null: K-gate skips their stores)
    w.bytes = c.off;
    return w;
  }
  w.relu_bits = c.take<unsigned long long>((size_t)((N + 15) / 16 + 2) * (H / 32) * 8);
  w.a = take((size_t)N * D);
  w.b = take(gated ? (size_t)N * D : 0);
  w.p = take((size_t)N);
  w.ds = take((size_t)N);
  w.dbc_part = take(PREP_GROUPS);
  w.du = take((size_t)N * H);
  w.slab_w1 = take((size_t)splits * H * L);
  w.slab_wab = take((size_t)w.tn.splits_g * w.mstk * H);
  w.cs_b1 = take((size_t)splits * H);
  w.cs_bab = take((size_t)w.tn.splits_g * w.mstk);
  w.cs_wc = take((size_t)w.tn.splits_g * D);
  w.bytes = c.off;
  return w;
}

static int check_desc(const mmf_amil_desc* d, int elem_bytes = 4) {
  if (!d || !d->W1 || !d->b1 || !d->Wa || !d->ba || !d->Wc || !d->bc) return MMF_ERR_ARG;
  if (d->gated && (!d->Wb || !d->bb)) return MMF_ERR_ARG;
  if (d->N < 1) return MMF_ERR_SHAPE;
  if (d->L % KC != 0 || d->H % KC != 0) return MMF_ERR_SHAPE;
  if (d->H != 256 && d->H != 512 && d->H != 1024) return MMF_ERR_SHAPE;
  if (d->D % 128 != 0) return MMF_ERR_SHAPE;
  if (d->N * (int64_t)(d->H > d->D ? d->H : d->D) >= (int64_t)1 << 32) return MMF_ERR_SHAPE;  // 32-bit mask index
  // buffer loads: 32-bit byte offsets, and the "reads as zero" sentinel is 2^31 => every operand < 2 GiB: the bag
  // [N x L], h / du [N x H], the gate rows [N x 2 D] (check_attn and ig_row_limit take the same three)
  int64_t widest = d->L > 2 * d->D ? d->L : 2 * d->D;
  if (d->H > widest) widest = d->H;
  if (d->N * widest * elem_bytes >= (int64_t)1 << 31) return MMF_ERR_SHAPE;
  if (d->p_h < 0.f || d->p_h >= 1.f || d->p_att < 0.f || d->p_att >= 1.f) return MMF_ERR_ARG;
  if (d->gemm != MMF_GEMM_F32 && d->gemm != MMF_GEMM_BF16X3) return MMF_ERR_ARG;
  return MMF_OK;
}

// the pointers every stack forward takes, and their alignment (the bf16 kernels read converted weights: any alignment)
static int check_operands(const mmf_amil_desc* d, const void* x, const void* workspace, const float* A_raw, bool bf16) {
  if (!x || !workspace || !A_raw) return MMF_ERR_ARG;
  if (!aligned16(x) || !aligned16(workspace)) return MMF_ERR_ALIGN;
  if (!bf16 && (!aligned16(d->W1) || !aligned16(d->Wa) || (d->gated && !aligned16(d->Wb)))) return MMF_ERR_ALIGN;
  return MMF_OK;
}

// ---- the fp32 attention stack's launch parameters ------------------------------------------------------------------
// Built once from the descriptor, the workspace, the input and the seed of the dropout keys for the one-bag chain
// (amil_forward_impl / amil_backward_impl) and the grouped chain (group_chain); the standalone scorer (mmf_attn_net_*)
// uses the gate builders with h = x.  Each chain then sets only what is its own.
//
// The grouped chain runs the same fields through its `_seg` launchers, where they end up the same or are not read:
// `split` is derived from desc->gemm and is 0 there, because group_check refuses bf16x3; K-dh's plan is asked for without
// fused K-prep (dh_plan).  A carve for inference leaves relu_bits, a and b null.

static GateFwdParams gate_fwd_params(const mmf_amil_desc* d, const float* h, float* a, float* b, float* s_part,
                                     uint32_t seed) {
  GateFwdParams gp{};
  gp.h = h; gp.Wa = d->Wa; gp.ba = d->ba; gp.Wb = d->Wb; gp.bb = d->bb; gp.Wc = d->Wc;
  gp.a = a; gp.b = b; gp.s_part = s_part;
  gp.N = d->N; gp.H = d->H; gp.D = d->D; gp.gated = d->gated;
  gp.drop_p = d->p_att; gp.key_a = drop_key(seed, 1); gp.key_b = drop_key(seed, 2); gp.seed_dev = d->seed_dev;
  return gp;
}

static GateBwdCtx gate_bwd_ctx(const mmf_amil_desc* d, const float* a, const float* b, const float* ds, uint32_t seed) {
  GateBwdCtx gc{};
  gc.a = a; gc.b = b; gc.ds = ds; gc.Wc = d->Wc; gc.D = d->D; gc.gated = d->gated;
  gc.drop_p = d->p_att; gc.key_a = drop_key(seed, 1); gc.key_b = drop_key(seed, 2); gc.seed_dev = d->seed_dev;
  return gc;
}

// d[Wa ; Wb] = dP^T . B ; (dba | dbb) = colsum(dP) ; dWc = colsum(ds . a_d . b_d), dP built from the launch's GateBwdCtx
static TnProblem tn_gate_problem(const mmf_amil_desc* d, const float* B, float* out, float* cs_bab, float* cs_wc) {
  const int mstk = d->gated ? 2 * d->D : d->D;
  TnProblem q{};
  q.kind = TN_A_GATE; q.A = nullptr; q.lda = 0; q.M = mstk;
  q.B = B; q.ldb = d->H; q.Ncols = d->H;
  q.out = out; q.split_stride = (size_t)mstk * d->H; q.ldc = d->H;
  q.colsum = cs_bab; q.colsum_stride = mstk; q.colsum2 = cs_wc; q.colsum2_stride = d->D;
  return q;
}

static LinearParams stack_linear(const mmf_amil_desc* d, const AmilWs& w, const float* x, uint32_t seed) {
  LinearParams lp{};
  lp.x[0] = x; lp.nseg = 1; lp.kseg = d->L; lp.ldx = d->L;
  lp.w = d->W1; lp.bias = d->b1; lp.y = w.h;
  lp.M = d->N; lp.N = d->H; lp.K = d->L;
  lp.act = ACT_RELU; lp.drop_p = d->p_h; lp.drop_key = drop_key(seed, 0); lp.seed_dev = d->seed_dev;
  lp.relu_bits = w.relu_bits;
  lp.allow_half = 1; lp.concurrent = d->concurrent ? 1 : 0;
  lp.split = d->gemm == MMF_GEMM_BF16X3;
  lp.kpart = w.kpart; lp.ktick = d->sync; lp.ktick_words = d->sync ? d->sync_words : 0;
  return lp;
}

static GateFwdParams stack_gate_fwd(const mmf_amil_desc* d, const AmilWs& w, uint32_t seed) {
  GateFwdParams gp = gate_fwd_params(d, w.h, w.a, w.b, w.s_part, seed);
  gp.split = d->gemm == MMF_GEMM_BF16X3;
  return gp;
}

// the pooling launch but for where its partials, M, statistics and head tail go
static PoolParams stack_pool(const mmf_amil_desc* d, const AmilWs& w, float* A_raw) {
  PoolParams pp{};
  pp.s_part = w.s_part; pp.n_parts = w.parts; pp.bc = d->bc; pp.h = w.h; pp.N = d->N; pp.H = d->H;
  pp.A_raw = A_raw;
  return pp;
}

// K-prep as its own launch (softmax weights p, ds = dL/dA and the dbc partials)
static BwdPrepParams stack_prep(const mmf_amil_desc* d, const AmilWs& w, const float* A_raw, const float* stats,
                                const float* M, const float* dM, const float* gA) {
  BwdPrepParams bp{};
  bp.h = w.h; bp.A_raw = A_raw; bp.stats = stats; bp.dM = dM; bp.M = M; bp.gA = gA;
  bp.N = d->N; bp.H = d->H; bp.p = w.p; bp.ds = w.ds; bp.dbc_part = w.dbc_part;
  bp.n_groups = (int)((d->N + 3) / 4 < PREP_GROUPS ? (d->N + 3) / 4 : PREP_GROUPS);
  return bp;
}

// K-dh: du = (dP.Wab + p dM) * relu'(h) * scale_h, without the inputs of a fused K-prep (the one-bag chain adds them)
static BwdDhParams stack_dh(const mmf_amil_desc* d, const AmilWs& w, const GateBwdCtx& gc, const float* dM) {
  BwdDhParams dp{};
  dp.g = gc; dp.Wa = d->Wa; dp.Wb = d->Wb; dp.p = w.p; dp.dM = dM; dp.h = w.h; dp.du = w.du;
  dp.relu_bits = w.relu_bits;
  dp.concurrent = d->concurrent ? 1 : 0;
  dp.split = d->gemm == MMF_GEMM_BF16X3;
  dp.N = d->N; dp.H = d->H; dp.scale_h = d->p_h > 0.f ? 1.0f / (1.0f - d->p_h) : 1.0f;
  return dp;
}

// K-dh's plan for these parameters; can_fuse: the caller can hand K-dh what K-prep reads (DhPlan)
static DhPlan dh_plan(const BwdDhParams& p, bool can_fuse) {
  return plan_bwd_dh(p.N, p.H, p.g.D, p.g.gated, p.g.drop_p > 0.f, p.split, p.concurrent, can_fuse, PREP_GROUPS);
}

// d(input) = du . W1
static NnParams stack_dx(const mmf_amil_desc* d, const AmilWs& w, float* dx) {
  NnParams np{};
  np.A = w.du; np.lda = d->H; np.B = d->W1; np.ldb = d->L; np.C = dx; np.ldc = d->L;
  np.M = d->N; np.N = d->L; np.K = d->H;
  return np;
}

// the stack's two problems: dW1[H x L] = du^T . x ; db1 = colsum(du), and the gate problem over h, which takes the plan's
// own (more, shorter) splits.  Returns the carving's plan; the bf16x3 mode, which the carving does not know, changes its
// tile's kind alone (a function of K and the mode), never the splits the slabs are sized by.
static TnPlan stack_tn(const mmf_amil_desc* d, const AmilWs& w, const float* x, const GateBwdCtx& gc, TnParams& tp) {
  tp.nprob = 2; tp.K = d->N; tp.g = gc;
  tp.split = d->gemm == MMF_GEMM_BF16X3;
  TnProblem& q1 = tp.prob[0];
  q1.kind = TN_A_PLAIN; q1.A = w.du; q1.lda = d->H; q1.M = d->H;
  q1.B = x; q1.ldb = d->L; q1.Ncols = d->L;
  q1.out = w.slab_w1; q1.split_stride = (size_t)d->H * d->L; q1.ldc = d->L;
  q1.colsum = w.cs_b1; q1.colsum_stride = d->H; q1.colsum2 = nullptr; q1.colsum2_stride = 0;
  tp.prob[1] = tn_gate_problem(d, w.h, w.slab_wab, w.cs_bab, w.cs_wc);
  TnPlan pl = w.tn;
  if (tp.split) pl.kind = plan_tn(d->N, 1, nullptr, 0).kind;
  return pl;
}

// a stack backward's split-K sums, fp32 or bf16 (W: AmilWs / AmilWsBf): dW1 / db1 over `splits` slabs, the gate's over `splits_g`
template <class W>
static void reduce_slabs(const mmf_amil_desc* d, const W& w, const mmf_amil_grads* g, int splits, int splits_g, ReduceList& rl) {
  const size_t wab_stride = (size_t)w.mstk * d->H;
  rl.add(w.slab_w1, g->dW1, d->H * d->L, splits, (size_t)d->H * d->L);
  rl.add(w.slab_wab, g->dWa, d->D * d->H, splits_g, wab_stride);
  if (d->gated) rl.add(w.slab_wab + (size_t)d->D * d->H, g->dWb, d->D * d->H, splits_g, wab_stride);
  rl.add(w.cs_b1, g->db1, d->H, splits, d->H);
  rl.add(w.cs_bab, g->dba, d->D, splits_g, w.mstk);
  if (d->gated) rl.add(w.cs_bab + d->D, g->dbb, d->D, splits_g, w.mstk);
}

// the stack's eight sums (six when ungated): its split-K slabs and the dbc partials of K-prep
static void stack_reduce(const mmf_amil_desc* d, const AmilWs& w, const mmf_amil_grads* g, int dbc_parts, ReduceList& rl) {
  reduce_slabs(d, w, g, w.tn.splits, w.tn.splits_g, rl);
  rl.add(w.cs_wc, g->dWc, d->D, w.tn.splits_g, d->D);
  rl.add(w.dbc_part, g->dbc, 1, dbc_parts, 1);
}

// ---- bf16-storage path (mmf_bf16.h) ----------------------------------------------------------
struct AmilWsBf {
  float *M_step, *dM_step;
  bf16_t *w1, *wab, *wabT, *h, *a, *b, *du, *dP;
  float *s_part, *partials, *stats, *p, *ds, *dbc_part, *dwc_part;
  float *slab_w1, *slab_wab, *cs_b1, *cs_bab;
  int parts, groups, splits, k_per_split, mstk, dbc_cap;
  size_t bytes;
};

static AmilWsBf carve_bf16(Carver& c, int64_t N, int L, int H, int D, int gated, bool infer = false) {
  AmilWsBf w{};
  auto take16 = [&](size_t n) { return c.take<bf16_t>(n); };
  auto take32 = [&](size_t n) { return c.take<float>(n); };
  w.parts = gate_parts_bf16(D, gated);
  w.groups = pool_groups(N);
  w.mstk = gated ? 2 * D : D;
  const int td = TNB_TILE;
  const int tiles = ((H + td - 1) / td) * ((L + td - 1) / td) + ((w.mstk + td - 1) / td) * ((H + td - 1) / td);
  w.splits = tn_bf16_splits(N, tiles);
  const int64_t kps = (N + w.splits - 1) / w.splits;
  w.k_per_split = (int)((kps + TNB_KCH - 1) / TNB_KCH * TNB_KCH);
  w.dbc_cap = dh_bf16_row_tiles(N);
  w.M_step = take32(H);
  w.dM_step = take32(H);
  w.w1 = take16((size_t)H * L);
  w.wab = take16((size_t)w.mstk * H);
  w.wabT = take16((size_t)H * w.mstk);
  w.h = take16((size_t)N * H);
  w.s_part = take32((size_t)w.parts * N);
  {
    const int tiles = fused_fwd_tiles(N);          // the fused forward writes one pooling partial per 128-row tile
    w.partials = take32((size_t)(w.groups > tiles ? w.groups : tiles) * (2 + H));
  }
  w.stats = take32(4);
  if (infer) {
    w.bytes = c.off;
    return w;
  }
  w.a = take16((size_t)N * D);
  w.b = take16(gated ? (size_t)N * D : 0);
  w.du = take16((size_t)N * H);
  w.dP = take16((size_t)N * w.mstk);
  w.p = take32((size_t)N);
  w.ds = take32((size_t)N);
  w.dbc_part = take32((size_t)w.dbc_cap);
  w.dwc_part = take32((size_t)w.dbc_cap * D);
  w.slab_w1 = take32((size_t)w.splits * H * L);
  w.slab_wab = take32((size_t)w.splits * w.mstk * H);
  w.cs_b1 = take32((size_t)w.splits * H);
  w.cs_bab = take32((size_t)w.splits * w.mstk);
  w.bytes = c.off;
  return w;
}

static int check_desc_bf16(const mmf_amil_desc* d) {
  if (int e = check_desc(d, 2)) return e;        // the bag and every [N x *] activation are 2-byte here
  if (d->L % 64 != 0 || d->H % 256 != 0) return MMF_ERR_SHAPE;
  return MMF_OK;
}

// The bf16 stack's forward launch parameters, as the fp32 builders above, for the one-bag chain (amil_bf16_forward_impl,
// unfused) and the window's (group_infer_chain_bf16).  The weights as bf16 in the workspace -- fused2: in MFMA-fragment
// order (same bytes, same slots); bwd: [Wa ; Wb]^T too, in K-dh's k order (mmf_amil_bf16.hip: LoadPB) or its second form's
static CvtParams stack_cvt_bf16(const mmf_amil_desc* d, const AmilWsBf& w, bool fused2, bool bwd) {
  CvtParams cp{};
  auto cvt = [&](const float* src, bf16_t* dst, int rows, int cols, int dst_ld, int c0, int transpose) {
    cp.seg[cp.nseg++] = CvtSeg{src, dst, rows, cols, dst_ld, c0, transpose, 0};
  };
  const bool dh2 = bwd && dh2_bf16_ok(d->N, d->H, d->D, d->gated);
  cvt(d->W1, w.w1, d->H, d->L, d->L, 0, fused2 ? 3 : 0);
  cvt(d->Wa, w.wab, d->D, d->H, d->H, 0, fused2 ? 4 : 0);
  if (bwd) cvt(d->Wa, w.wabT, d->D, d->H, w.mstk, 0, dh2 ? 5 : (d->gated ? 2 : 1));
  if (d->gated) {
    if (fused2) cvt(d->Wb, w.wab, d->D, d->H, d->H, 16, 4);
    else cvt(d->Wb, w.wab + (size_t)d->D * d->H, d->D, d->H, d->H, 0, 0);
    if (bwd) cvt(d->Wb, w.wabT, d->D, d->H, w.mstk, 32, dh2 ? 5 : 2);
  }
  return cp;
}

static LinearBfParams stack_linear_bf16(const mmf_amil_desc* d, const AmilWsBf& w, const uint16_t* x, uint32_t seed) {
  LinearBfParams lp{};
  lp.x = x; lp.w = w.w1; lp.bias = d->b1; lp.y = w.h;
  lp.M = d->N; lp.N = d->H; lp.K = d->L;
  lp.drop_p = d->p_h; lp.drop_key = drop_key(seed, 0); lp.seed_dev = d->seed_dev;
  return lp;
}

static GateBfParams stack_gate_bf16(const mmf_amil_desc* d, const AmilWsBf& w, uint32_t seed) {
  GateBfParams gp{};
  gp.h = w.h; gp.Wa = w.wab; gp.Wb = d->gated ? w.wab + (size_t)d->D * d->H : nullptr;
  gp.ba = d->ba; gp.bb = d->bb; gp.Wc = d->Wc;
  gp.a = w.a; gp.b = w.b; gp.s_part = w.s_part;           // a / b are null when carved for inference
  gp.N = d->N; gp.H = d->H; gp.D = d->D; gp.gated = d->gated;
  gp.drop_p = d->p_att; gp.key_a = drop_key(seed, 1); gp.key_b = drop_key(seed, 2); gp.seed_dev = d->seed_dev;
  return gp;
}

// the pooling launch over the bf16 h but for where its partials, M, statistics and head tail go
static PoolBfParams stack_pool_bf16(const mmf_amil_desc* d, const AmilWsBf& w, float* A_raw) {
  PoolBfParams pb{};
  PoolParams& pp = pb.base;
  pp.s_part = w.s_part; pp.n_parts = w.parts; pp.bc = d->bc; pp.h = nullptr; pp.N = d->N; pp.H = d->H;
  pp.A_raw = A_raw;
  pb.h = w.h;
  return pb;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_abi_version(void) { return 12; }

const char* mmf_strerror(int code) {
  switch (code) {
    case MMF_OK: return "ok";
    case MMF_ERR_ARG: return "invalid argument (null pointer or bad flag)";
    case MMF_ERR_SHAPE: return "unsupported shape (need L,H % 32 == 0, H in {256,512,1024}, D % 128 == 0, K % 32 == 0, N % 4 == 0 of a dense layer, every operand < 2 GiB)";
    case MMF_ERR_ALIGN: return "pointer or leading dimension not 16-byte aligned";
    case MMF_ERR_WORKSPACE: return "workspace too small (see mmf_*_workspace_bytes)";
    case MMF_ERR_LAUNCH: return "HIP launch failed";
    default: return "unknown mmf error";
  }
}

size_t mmf_amil_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated) {
  if (N < 1) N = 1;
  Carver c;
  return carve(c, N, L, H, D, gated).bytes;
}

static int amil_forward_impl(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes,
                             float* M, float* A_raw, void* stream, bool infer, const HeadTail* tail = nullptr) {
  if (int e = check_desc(d)) return e;
  if (int e = check_operands(d, x, workspace, A_raw, false)) return e;
  Carver c(workspace);
  AmilWs w = carve(c, d->N, d->L, d->H, d->D, d->gated, infer);
  if (w.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  if (!M) M = w.M_step;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);

  if (int e = launch_linear(stack_linear(d, w, x, d->seed), st)) return e;
  if (int e = launch_gate_fwd(stack_gate_fwd(d, w, d->seed), st)) return e;
  PoolParams pp = stack_pool(d, w, A_raw);
  pp.partials = w.partials; pp.M = M; pp.stats = w.stats;
  if (tail) { pp.tail = *tail; pp.tail.dM = w.dM_step; }
  return launch_pool(pp, st);
}

int mmf_amil_forward(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes,
                     float* M, float* A_raw, void* stream) {
  return amil_forward_impl(d, x, workspace, workspace_bytes, M, A_raw, stream, false);
}

size_t mmf_amil_infer_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated) {
  if (N < 1) N = 1;
  Carver c;
  return carve(c, N, L, H, D, gated, true).bytes;
}

int mmf_amil_infer(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes,
                   float* M, float* A_raw, void* stream) {
  return amil_forward_impl(d, x, workspace, workspace_bytes, M, A_raw, stream, true);
}

static int amil_backward_impl(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes,
                              const float* M, const float* A_raw, const float* dM, const float* gA,
                              const mmf_amil_grads* g, void* stream, int accumulate) {
  if (int e = check_desc(d)) return e;
  if (!x || !workspace || !A_raw || !g) return MMF_ERR_ARG;
  if (int e = check_grads(d, g)) return e;
  if (!grads_aligned(d, g)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  AmilWs w = carve(c, d->N, d->L, d->H, d->D, d->gated);
  if (w.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  if (!M) M = w.M_step;          // inside mmf_amil_nll_step the pooled embedding and its gradient live in the workspace
  if (!dM) dM = w.dM_step;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);

  const GateBwdCtx gc = gate_bwd_ctx(d, w.a, w.b, w.ds, d->seed);
  BwdDhParams dp = stack_dh(d, w, gc, dM);
  // K-prep (softmax weights, ds) either inside K-dh or as its own launch
  const DhPlan pl = dh_plan(dp, true);
  int dbc_groups = pl.dbc_groups;
  if (pl.fused) {
    dp.A_raw = A_raw; dp.stats = w.stats; dp.Mpool = M; dp.gA = gA;
    dp.p_out = w.p; dp.ds_out = w.ds; dp.dbc_part = w.dbc_part;
  } else {
    const BwdPrepParams bp = stack_prep(d, w, A_raw, w.stats, M, dM, gA);
    dbc_groups = bp.n_groups;
    if (int e = launch_bwd_prep(bp, st)) return e;
  }
  if (int e = launch_bwd_dh(pl, dp, st)) return e;
  if (g->dx) {   // radio: the input is reduce_dim's output
    if (int e = launch_nn(stack_dx(d, w, g->dx), st)) return e;
  }

  TnParams tp{};
  const TnPlan tn = stack_tn(d, w, x, gc, tp);
  if (int e = launch_tn(tn, tp, st)) return e;

  ReduceList rl;
  stack_reduce(d, w, g, dbc_groups, rl);
  return rl.launch(accumulate, st);
}

int mmf_amil_backward(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes,
                      const float* M, const float* A_raw, const float* dM, const float* gA,
                      const mmf_amil_grads* g, void* stream) {
  if (!M || !dM) return MMF_ERR_ARG;
  return amil_backward_impl(d, x, workspace, workspace_bytes, M, A_raw, dM, gA, g, stream, 0);
}

size_t mmf_amil_bf16_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated) {
  if (N < 1) N = 1;
  Carver c;
  return carve_bf16(c, N, L, H, D, gated).bytes;
}

static int amil_bf16_forward_impl(const mmf_amil_desc* d, const uint16_t* x, void* workspace, size_t workspace_bytes,
                                  float* M, float* A_raw, void* stream, bool infer, const HeadTail* tail = nullptr) {
  if (int e = check_desc_bf16(d)) return e;
  if (int e = check_operands(d, x, workspace, A_raw, true)) return e;
  Carver c(workspace);
  AmilWsBf w = carve_bf16(c, d->N, d->L, d->H, d->D, d->gated, infer);
  if (w.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  if (!M) M = w.M_step;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  HeadTail tl{};
  if (tail) { tl = *tail; tl.dM = w.dM_step; }

  const bool fused2 = d->gated && fused_fwd2_ok(d->N, d->L, d->H, d->D);
  if (int e = launch_cvt_bf16(stack_cvt_bf16(d, w, fused2, !infer), st)) return e;

  if (fused2 || (d->gated && d->D == 256 && fused_fwd_ok(d->N, d->L, d->H, d->D))) {   // `small` gated stack: one kernel for projection + scoring + pooling partials
    FusedFwdParams fp{};
    fp.x = x; fp.w1 = w.w1; fp.b1 = d->b1;
    fp.Wa = w.wab; fp.Wb = d->gated ? w.wab + (size_t)d->D * d->H : nullptr;
    fp.w1f = w.w1; fp.wabf = w.wab;
    fp.ba = d->ba; fp.bb = d->bb; fp.Wc = d->Wc; fp.bc = d->bc;
    fp.h = infer ? nullptr : w.h; fp.a = w.a; fp.b = w.b;       // a / b are null when carved for inference
    fp.A_raw = A_raw; fp.partials = w.partials;
    fp.N = d->N; fp.L = d->L; fp.D = d->D;
    fp.p_h = d->p_h; fp.p_att = d->p_att;
    fp.key_h = drop_key(d->seed, 0); fp.key_a = drop_key(d->seed, 1); fp.key_b = drop_key(d->seed, 2);
    fp.seed_dev = d->seed_dev;
    if (fused2) {
      if (int e = launch_fused_fwd2_bf16(fp, d->gated, st)) return e;
    } else
    if (int e = launch_fused_fwd_bf16(fp, d->gated, st)) return e;
    // (Tried: sending the rows of a sparse last round -- 782 tiles at 100k = 3 rounds of 256 + 14 -- through the three
    // unfused kernels instead.  The fused kernel drops 173 -> 141 us, but the three small launches cost 48 us.)
    PoolParams pm{};
    pm.N = d->N; pm.H = d->H; pm.partials = w.partials; pm.M = M; pm.stats = w.stats;
    pm.n_groups = fused_fwd_tiles(d->N);
    pm.tail = tl;
    return launch_pool_merge(pm, st);
  }

  if (int e = launch_linear_bf16(stack_linear_bf16(d, w, x, d->seed), st)) return e;
  if (int e = launch_gate_bf16(stack_gate_bf16(d, w, d->seed), st)) return e;
  PoolBfParams pb = stack_pool_bf16(d, w, A_raw);
  pb.base.partials = w.partials; pb.base.M = M; pb.base.stats = w.stats; pb.base.tail = tl;
  return launch_pool_bf16(pb, st);
}

int mmf_amil_bf16_forward(const mmf_amil_desc* d, const uint16_t* x, void* workspace, size_t workspace_bytes,
                          float* M, float* A_raw, void* stream) {
  return amil_bf16_forward_impl(d, x, workspace, workspace_bytes, M, A_raw, stream, false);
}

size_t mmf_amil_bf16_infer_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated) {
  if (N < 1) N = 1;
  Carver c;
  return carve_bf16(c, N, L, H, D, gated, true).bytes;
}

int mmf_amil_bf16_infer(const mmf_amil_desc* d, const uint16_t* x, void* workspace, size_t workspace_bytes,
                        float* M, float* A_raw, void* stream) {
  return amil_bf16_forward_impl(d, x, workspace, workspace_bytes, M, A_raw, stream, true);
}

static int amil_bf16_backward_impl(const mmf_amil_desc* d, const uint16_t* x, void* workspace, size_t workspace_bytes,
                                   const float* M, const float* A_raw, const float* dM, const float* gA,
                                   const mmf_amil_grads* g, void* stream, int accumulate) {
  if (int e = check_desc_bf16(d)) return e;
  if (!x || !workspace || !A_raw || !g) return MMF_ERR_ARG;
  if (int e = check_grads(d, g)) return e;
  if (g->dx) return MMF_ERR_ARG;     // the bf16 bag is a leaf: no input gradient on this path
  if (!grads_aligned(d, g)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  AmilWsBf w = carve_bf16(c, d->N, d->L, d->H, d->D, d->gated);
  if (w.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  if (!M) M = w.M_step;
  if (!dM) dM = w.dM_step;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  const uint32_t* const seed_dev = d->seed_dev;

  GateBwdBf gc{};
  gc.a = w.a; gc.b = w.b; gc.ds = w.ds; gc.Wc = d->Wc; gc.D = d->D; gc.gated = d->gated;
  gc.drop_p = d->p_att; gc.key_a = drop_key(d->seed, 1); gc.key_b = drop_key(d->seed, 2); gc.seed_dev = seed_dev;

  DhBfParams dp{};
  dp.g = gc; dp.WabT = w.wabT; dp.dM = dM; dp.h = w.h; dp.du = w.du;
  dp.N = d->N; dp.H = d->H; dp.scale_h = d->p_h > 0.f ? 1.0f / (1.0f - d->p_h) : 1.0f;
  dp.A_raw = A_raw; dp.stats = w.stats; dp.Mpool = M; dp.gA = gA;
  dp.p_out = w.p; dp.ds_out = w.ds; dp.dbc_part = w.dbc_part; dp.dP = w.dP; dp.dwc_part = w.dwc_part;
  if (dh2_bf16_ok(d->N, d->H, d->D, d->gated)) {
    if (int e = launch_dh2_bf16(dp, st)) return e;
  } else if (int e = launch_dh_bf16(dp, st)) return e;
  const int ntn = d->H / 256;

  TnBfParams tp{};
  tp.nprob = 2; tp.K = d->N; tp.splits = w.splits; tp.k_per_split = w.k_per_split;
  TnBfProblem& q1 = tp.prob[0];   // dW1[H x L] = du^T . x ; db1 = colsum(du)
  q1.A = w.du; q1.lda = d->H; q1.M = d->H;
  q1.B = x; q1.ldb = d->L; q1.Ncols = d->L;
  q1.out = w.slab_w1; q1.split_stride = (size_t)d->H * d->L; q1.ldc = d->L;
  q1.colsum = w.cs_b1; q1.colsum_stride = d->H;
  TnBfProblem& q2 = tp.prob[1];   // dWab[(2)D x H] = dP^T . h ; (dba|dbb) = colsum(dP)
  q2.A = w.dP; q2.lda = w.mstk; q2.M = w.mstk;
  q2.B = w.h; q2.ldb = d->H; q2.Ncols = d->H;
  q2.out = w.slab_wab; q2.split_stride = (size_t)w.mstk * d->H; q2.ldc = d->H;
  q2.colsum = w.cs_bab; q2.colsum_stride = w.mstk;
  if (int e = launch_tn_bf16(tp, st)) return e;

  ReduceList rl;
  reduce_slabs(d, w, g, w.splits, w.splits, rl);
  rl.add(w.dwc_part, g->dWc, d->D, dh_bf16_tiles_used(d->N, ntn), d->D);
  rl.add(w.dbc_part, g->dbc, 1, dh_bf16_tiles_used(d->N, ntn), 1);
  return rl.launch(accumulate, st);
}

int mmf_amil_bf16_backward(const mmf_amil_desc* d, const uint16_t* x, void* workspace, size_t workspace_bytes,
                           const float* M, const float* A_raw, const float* dM, const float* gA,
                           const mmf_amil_grads* g, void* stream) {
  if (!M || !dM) return MMF_ERR_ARG;
  return amil_bf16_backward_impl(d, x, workspace, workspace_bytes, M, A_raw, dM, gA, g, stream, 0);
}

// ---- attention stack + hazard head [+ nll_surv + the whole backward] in one call ------------------------------
// grads: the target carries the classifier's gradient (training); the forward-only form takes its labels and loss alone
static int head_tail_of(const mmf_surv_head* h, const mmf_nll_target* t, HeadTail& tl, bool grads = true) {
  if (!h || !h->Wk || !h->bk || !h->logits || !h->hazards || !h->S || !h->Y_hat) return MMF_ERR_ARG;
  if (h->K < 1 || h->K > 32) return MMF_ERR_SHAPE;
  tl = HeadTail{};
  tl.Wk = h->Wk; tl.bk = h->bk; tl.K = h->K;
  tl.logits = h->logits; tl.hazards = h->hazards; tl.S = h->S; tl.Y_hat = h->Y_hat; tl.risk = h->risk;
  if (t) {
    if (!t->Y || !t->c || !t->loss || (grads && (!t->dWk || !t->dbk))) return MMF_ERR_ARG;
    tl.Y = t->Y; tl.c = t->c; tl.alpha = t->alpha; tl.eps = t->eps; tl.loss = t->loss;
    if (grads) { tl.loss_scale = t->loss_scale; tl.dWk = t->dWk; tl.dbk = t->dbk; tl.accumulate = t->accumulate; }
  }
  return MMF_OK;
}

int mmf_amil_head_forward(const mmf_amil_desc* d, const void* x, int32_t x_bf16, void* workspace, size_t workspace_bytes,
                          const mmf_surv_head* head, float* M, float* A_raw, void* stream) {
  if (!d || !M) return MMF_ERR_ARG;
  HeadTail tl;
  if (int e = head_tail_of(head, nullptr, tl)) return e;
  return x_bf16 ? amil_bf16_forward_impl(d, static_cast<const uint16_t*>(x), workspace, workspace_bytes, M, A_raw, stream, false, &tl)
                : amil_forward_impl(d, static_cast<const float*>(x), workspace, workspace_bytes, M, A_raw, stream, false, &tl);
}

int mmf_amil_nll_step(const mmf_amil_desc* d, const void* x, int32_t x_bf16, void* workspace, size_t workspace_bytes,
                      const mmf_surv_head* head, const mmf_nll_target* target, float* A_raw,
                      const mmf_amil_grads* grads, void* stream) {
  if (!d || !target || !grads) return MMF_ERR_ARG;
  HeadTail tl;
  if (int e = head_tail_of(head, target, tl)) return e;
  const int acc = target->accumulate ? 1 : 0;
  if (x_bf16) {
    const uint16_t* xb = static_cast<const uint16_t*>(x);
    if (int e = amil_bf16_forward_impl(d, xb, workspace, workspace_bytes, nullptr, A_raw, stream, false, &tl)) return e;
    return amil_bf16_backward_impl(d, xb, workspace, workspace_bytes, nullptr, A_raw, nullptr, nullptr, grads, stream, acc);
  }
  const float* xf = static_cast<const float*>(x);
  if (int e = amil_forward_impl(d, xf, workspace, workspace_bytes, nullptr, A_raw, stream, false, &tl)) return e;
  return amil_backward_impl(d, xf, workspace, workspace_bytes, nullptr, A_raw, nullptr, nullptr, grads, stream, acc);
}

// ---- grouped step: the bags of one accumulation window as one launch chain ------------------------------------
namespace mmf {
// hash_u32(key, i) = mix(i * 0x9E3779B1 + key), so bag g's masks -- key drop_key(seed_g, site), bag-local index i -- are
// those of key drop_key(0, site) at index i + seed_g * inverse(0x9E3779B1) (mod 2^32): one key per launch, and the bag
// enters through the per-row index base that group_rows_kernel writes.
static uint32_t hash_mul_inverse() {
  const uint32_t a = 0x9E3779B1u;
  uint32_t x = a;                       // Newton: correct to 3, 6, 12, 24, 48 bits
  for (int i = 0; i < 5; ++i) x *= 2u - a * x;
  return x;
}

static int group_plan(const int64_t* offsets, int G, SegTable& s) {
  if (!offsets) return MMF_ERR_ARG;
  if (G < 1 || G > GROUP_MAX) return MMF_ERR_SHAPE;
  if (offsets[0] != 0) return MMF_ERR_SHAPE;
  for (int g = 0; g < G; ++g)
    if (offsets[g + 1] <= offsets[g]) return MMF_ERR_SHAPE;      // empty or decreasing
  s = SegTable{};
  s.G = G;
  const int64_t R = offsets[G];
  int64_t rpg = (R + GROUP_POOL_GROUPS - 1) / GROUP_POOL_GROUPS;   // ~one pooling group per CU over the window
  if (rpg < 64) rpg = 64;
  if (rpg > 8192) return MMF_ERR_SHAPE;                               // POOL_MAX_ROWS
  s.rows_per_group = (int)rpg;
  int gb = 0;
  for (int g = 0; g <= G; ++g) {
    s.off[g] = offsets[g];
    s.gbeg[g] = gb;
    if (g < G) gb += (int)((offsets[g + 1] - offsets[g] + rpg - 1) / rpg);
  }
  return MMF_OK;
}

// what every window of bags carries -- the grouped chain's, and integrated gradients' steps (IgWs)
struct WindowWs {
  AmilWs w;                  // the window's rows
  float *M, *dM, *stats, *partials;
  uint32_t *ridx_h, *ridx_d;
  int* bag;
};
struct GroupWs : WindowWs {
  float *wk, *bk;
  size_t bytes;
};
static GroupWs carve_group(Carver& c, const SegTable& s, int L, int H, int D, int gated) {
  GroupWs g{};
  const int64_t R = s.off[s.G];
  g.w = carve(c, R, L, H, D, gated);
  auto take = [&](size_t n) { return c.take<float>(n); };
  g.M = take((size_t)s.G * H);
  g.dM = take((size_t)s.G * H);
  g.stats = take((size_t)2 * s.G);
  g.wk = take((size_t)s.G * 32 * H);          // per-bag classifier gradients (K <= 32), summed by the reduce launch
  g.bk = take((size_t)s.G * 32);
  g.partials = take((size_t)s.gbeg[s.G] * (2 + H));
  g.ridx_h = c.take<uint32_t>((size_t)R);
  g.ridx_d = c.take<uint32_t>((size_t)R);
  g.bag = c.take<int>((size_t)R);
  g.bytes = c.off;
  return g;
}
}  // namespace mmf

namespace mmf {
// reduce_dim's backward on the grouped chain's launches (mmf_radio_nll_step_group): its input gradient du . W1 over every
// row, its weight-gradient problems in a TN launch of their own after the stack's, planned over their own tiles.  Its
// sums are entries on the stack's reduce list.
struct GroupExtra {
  float* dx;                    // [R x L] <- du . W1
  TnProblem prob[4]; int nprob;
  TnPlan tn;
};

// the window contract every grouped entry point checks after its own refusals and before the head and check_operands
static int window_plan(const mmf_amil_desc* d, const mmf_bag_group* group, int bf16, SegTable& s) {
  if (int e = group_plan(group->offsets, group->G, s)) return e;
  if (d->N != s.off[s.G]) return MMF_ERR_SHAPE;
  return bf16 ? check_desc_bf16(d) : check_desc(d);
}

// the call contract both grouped entry points share; fills the segment table (with each bag's mask index base) and the tail
static int group_check(const mmf_amil_desc* d, const mmf_bag_group* group, const void* x, const void* workspace,
                       const mmf_surv_head* head, const mmf_nll_target* target, const float* A_raw,
                       const mmf_amil_grads* g, SegTable& s, HeadTail& tl) {
  if (!d || !group || !target || !g) return MMF_ERR_ARG;
  if (d->gemm != MMF_GEMM_F32 || g->dx) return MMF_ERR_ARG;
  if (!group->seeds) return MMF_ERR_ARG;
  if (int e = window_plan(d, group, 0, s)) return e;
  if (int e = head_tail_of(head, target, tl)) return e;
  if (int e = check_grads(d, g)) return e;                   // every null pointer before any alignment
  if (int e = check_operands(d, x, workspace, A_raw, false)) return e;
  if (!grads_aligned(d, g)) return MMF_ERR_ALIGN;
  const uint32_t inv = hash_mul_inverse();
  for (int b = 0; b < s.G; ++b) s.ibase[b] = group->seeds[b] * inv;
  return MMF_OK;
}

// The stack's chain over the window's rows x [sum N x L], in three parts.  The masks are those of the seed-0 keys at each
// row's index base (group_rows_kernel).
// The launch groups a window of integrated-gradients steps (ig_window) takes as they are.  The per-row tables:
static int window_rows(const mmf_amil_desc* d, const SegTable& s, const WindowWs& g, hipStream_t st) {
  GroupRowsParams rp{};
  rp.s = s; rp.H = d->H; rp.D = d->D; rp.ridx_h = g.ridx_h; rp.ridx_d = g.ridx_d; rp.bag = g.bag;
  return launch_group_rows(rp, st);
}
// the pooling partials, then the per-bag merge: M_g into M's rows, ldm floats apart, and into the workspace with its statistics
static int window_pool(const mmf_amil_desc* d, const SegTable& s, const WindowWs& g, float* M, int ldm, float* A_raw,
                       hipStream_t st) {
  PoolParams pp = stack_pool(d, g.w, A_raw);
  pp.partials = g.partials; pp.M = M; pp.stats = g.stats;
  if (int e = launch_group_pool_partial(pp, s, st)) return e;
  return launch_group_merge(pp, s, ldm, g.M, st);
}
// K-prep per bag and the segmented K-dh, from dM [G x H]; dbc_parts: the dbc partials K-prep leaves for a reduce launch
static int window_dh(const mmf_amil_desc* d, const WindowWs& g, const GateBwdCtx& gc, const float* dM, const float* A_raw,
                     int& dbc_parts, hipStream_t st) {
  const BwdPrepParams bp = stack_prep(d, g.w, A_raw, g.stats, g.M, dM, nullptr);
  dbc_parts = bp.n_groups;
  if (int e = launch_group_bwd_prep(bp, g.bag, st)) return e;
  BwdDhParams dp = stack_dh(d, g.w, gc, dM);
  dp.seg_ridx = g.ridx_d; dp.seg_bag = g.bag;
  return launch_bwd_dh_seg(dh_plan(dp, false), dp, st);
}

// Forward, up to the scores: per-row tables, projection, gate.
static int group_chain_fwd(const mmf_amil_desc* d, const SegTable& s, const float* x, const GroupWs& gw, hipStream_t st) {
  const AmilWs& w = gw.w;
  if (int e = window_rows(d, s, gw, st)) return e;

  LinearParams lp = stack_linear(d, w, x, 0);
  lp.seg_ridx = gw.ridx_h;
  if (int e = launch_linear_seg(lp, st)) return e;

  GateFwdParams gp = stack_gate_fwd(d, w, 0);
  gp.seg_ridx = gw.ridx_d;
  return launch_gate_fwd_seg(gp, st);
}

// Backward, from dM [G x H] (M and the softmax statistics per bag are in the workspace): K-prep, K-dh, (du . W1),
// split-K TN.  The stack's sums go on `rl`, for the caller's reduce launch.
static int group_chain_bwd(const mmf_amil_desc* d, const float* x, const GroupWs& gw, const float* dM, const float* A_raw,
                           const mmf_amil_grads* g, const GroupExtra* ex, ReduceList& rl, hipStream_t st) {
  const AmilWs& w = gw.w;
  const GateBwdCtx gc = gate_bwd_ctx(d, w.a, w.b, w.ds, 0);
  int dbc_parts;
  if (int e = window_dh(d, gw, gc, dM, A_raw, dbc_parts, st)) return e;

  if (ex && ex->dx) {   // d(x) = du . W1: du carries every bag's ReLU and dropout masks
    if (int e = launch_nn(stack_dx(d, w, ex->dx), st)) return e;
  }

  TnParams tp{};
  const TnPlan tn = stack_tn(d, w, x, gc, tp);
  tp.seg_ridx = gw.ridx_d;
  if (int e = launch_tn(tn, tp, st)) return e;
  if (ex) {
    TnParams tr{};
    for (int i = 0; i < ex->nprob; ++i) tr.prob[i] = ex->prob[i];
    tr.nprob = ex->nprob; tr.K = d->N;
    if (int e = launch_tn(ex->tn, tr, st)) return e;
  }

  stack_reduce(d, w, g, dbc_parts, rl);
  return MMF_OK;
}

// The single-head chain: forward, pooling + head tail per bag (which leaves dM in the workspace), backward.  The
// classifier's sums go on `rl` behind the stack's.
static int group_chain(const mmf_amil_desc* d, const SegTable& s, const float* x, const GroupWs& gw, const HeadTail& tl,
                       int K, const mmf_nll_target* target, float* A_raw, const mmf_amil_grads* g,
                       const GroupExtra* ex, ReduceList& rl, hipStream_t st) {
  if (int e = group_chain_fwd(d, s, x, gw, st)) return e;

  PoolParams pp = stack_pool(d, gw.w, A_raw);
  pp.partials = gw.partials; pp.M = gw.M; pp.stats = gw.stats;
  pp.tail = tl; pp.tail.dM = gw.dM; pp.tail.dWk = gw.wk; pp.tail.dbk = gw.bk;
  if (int e = launch_group_pool(pp, s, st)) return e;

  if (int e = group_chain_bwd(d, x, gw, gw.dM, A_raw, g, ex, rl, st)) return e;
  rl.add(gw.wk, target->dWk, K * d->H, s.G, (size_t)K * d->H);      // classifier: the bags' slabs in bag order
  rl.add(gw.bk, target->dbk, K, s.G, (size_t)K);
  return MMF_OK;
}

// The multimodal window's halves of that chain (mmf_amil_group_forward / _backward, and the radio pair): the forward
// ends in the per-bag merge, which writes M_g into the caller's feature matrix; the backward starts from the caller's
// dM, whose H columns of this stack it first brings together as [G x H] (they are, when ldm == H).
static int group_half_fwd(const mmf_amil_desc* d, const SegTable& s, const float* x, const GroupWs& gw, float* M, int ldm,
                          float* A_raw, hipStream_t st) {
  if (int e = group_chain_fwd(d, s, x, gw, st)) return e;
  return window_pool(d, s, gw, M, ldm, A_raw, st);
}
static int group_half_bwd(const mmf_amil_desc* d, const SegTable& s, const float* x, const GroupWs& gw, const float* dM,
                          int ldm, const float* A_raw, const mmf_amil_grads* g, const GroupExtra* ex, ReduceList& rl,
                          hipStream_t st) {
  if (ldm != d->H) {
    if (int e = launch_group_dm_gather(dM, ldm, gw.dM, s.G, d->H, st)) return e;
    dM = gw.dM;
  }
  return group_chain_bwd(d, x, gw, dM, A_raw, g, ex, rl, st);
}

// what the four half entry points check, in group_check's order without the head: fills the segment table (forward:
// with each bag's mask index base).  g: the backward's gradients, null for a forward.
static int group_half_check(const mmf_amil_desc* d, const mmf_bag_group* group, const void* x, const void* workspace,
                            const float* M, int ldm, const float* A_raw, const mmf_amil_grads* g, bool bwd, SegTable& s) {
  if (!d || !group || !M || (bwd && !g)) return MMF_ERR_ARG;
  if (d->gemm != MMF_GEMM_F32 || (g && g->dx)) return MMF_ERR_ARG;
  if (!group->seeds) return MMF_ERR_ARG;
  if (int e = window_plan(d, group, 0, s)) return e;
  if (ldm < d->H) return MMF_ERR_SHAPE;
  if (g) if (int e = check_grads(d, g)) return e;
  if (int e = check_operands(d, x, workspace, A_raw, false)) return e;
  if (g && !grads_aligned(d, g)) return MMF_ERR_ALIGN;
  if (bwd && ldm == d->H && !aligned16(M)) return MMF_ERR_ALIGN;     // K-dh reads an ungathered dM four floats at a time
  const uint32_t inv = hash_mul_inverse();
  for (int b = 0; b < s.G; ++b) s.ibase[b] = group->seeds[b] * inv;
  return MMF_OK;
}

// the radio window's workspace: the stack's (carve_group, L = kseg) and reduce_dim's output, its gradient, the split-K
// slabs of dW_r / db_r and the partial tiles of a K-split reduce_dim forward
struct RadioWs {
  GroupWs gw;
  float *xr, *dxr, *slab, *cs, *kpart;
  TnPlan tn;                    // dW_r's launch: one problem per modality, planned over their own tiles
  size_t bytes;
};
static RadioWs carve_radio(Carver& c, const SegTable& s, int nseg, int kseg, int H, int D, int gated) {
  RadioWs r{};
  const int64_t R = s.off[s.G];
  const int L = kseg;
  r.gw = carve_group(c, s, L, H, D, gated);
  auto take = [&](size_t n) { return c.take<float>(n); };
  // dW_r as a TN launch of its own after the stack's, planned over its own tiles, not as more problems of the stack's
  // launch (fewer splits).  Measured: the separate launch is faster, 1.295 vs 1.366 ms at 16 x 512 rows.
  TnShape shapes[4];
  for (int m = 0; m < nseg; ++m) shapes[m] = {L, kseg, 0};
  r.tn = plan_tn(R, 0, shapes, nseg);
  r.xr = take((size_t)R * L);
  r.dxr = take((size_t)R * L);
  r.slab = take((size_t)r.tn.splits * L * nseg * kseg);
  r.cs = take((size_t)r.tn.splits * L);
  const size_t kf = linear_ksplit_floats(R, L, nseg * kseg, nseg, kseg);
  r.kpart = kf ? take(kf) : nullptr;
  r.bytes = c.off;
  return r;
}

// What both radio entry points check around the window's contract: the modality list before it (x[0] is the stack's
// input there), reduce_dim's operands after it.  grads: dW / db are written (training); forward-only reads neither.
static int radio_modalities(const mmf_radio_reduce* rd) {
  if (!rd || !rd->x) return MMF_ERR_ARG;
  return rd->nseg < 2 || rd->nseg > 4 ? MMF_ERR_SHAPE : MMF_OK;
}
static int radio_operands(const mmf_amil_desc* d, const mmf_radio_reduce* rd, bool grads) {
  const int nseg = rd->nseg, kseg = rd->kseg;
  if (kseg != d->L) return MMF_ERR_SHAPE;
  if (d->N * nseg * (int64_t)kseg * 4 >= (int64_t)1 << 31) return MMF_ERR_SHAPE;     // the [sum N x nseg*kseg] input < 2 GiB
  if (!rd->W || !rd->bias || (grads && (!rd->dW || !rd->db))) return MMF_ERR_ARG;
  for (int m = 0; m < nseg; ++m)
    if (!rd->x[m]) return MMF_ERR_ARG;
  for (int m = 0; m < nseg; ++m)
    if (!aligned16(rd->x[m])) return MMF_ERR_ALIGN;
  if (!aligned16(rd->W) || (grads && !aligned16(rd->dW))) return MMF_ERR_ALIGN;
  return MMF_OK;
}

// reduce_dim over the modality segments, every row of the window, into y: mmf_linear_forward's plan (a short window takes
// its K split over the segments, under desc->sync).  seed_dev: training passes desc->seed_dev on, forward-only none.
static LinearParams radio_linear(const mmf_amil_desc* d, const mmf_radio_reduce* rd, float* y, float* kpart,
                                 const uint32_t* seed_dev) {
  LinearParams lr{};
  for (int m = 0; m < rd->nseg; ++m) lr.x[m] = rd->x[m];
  lr.nseg = rd->nseg; lr.kseg = rd->kseg; lr.ldx = rd->kseg;
  lr.w = rd->W; lr.bias = rd->bias; lr.y = y; lr.M = d->N; lr.N = d->L; lr.K = rd->nseg * rd->kseg;
  lr.act = ACT_NONE; lr.drop_p = 0.f; lr.drop_key = drop_key(0, 0); lr.seed_dev = seed_dev;
  if (kpart && d->sync && d->sync_words > 0) { lr.kpart = kpart; lr.ktick = d->sync; lr.ktick_words = d->sync_words; }
  return lr;
}
// reduce_dim's backward as the chain's extra work: dW_r[:, m kseg : (m + 1) kseg] = dxr^T . x_m ; db_r = colsum(dxr) with the first
static GroupExtra radio_extra(const mmf_amil_desc* d, const mmf_radio_reduce* rd, const RadioWs& r) {
  const int nseg = rd->nseg, kseg = rd->kseg, L = d->L;
  GroupExtra ex{};
  ex.dx = r.dxr;
  ex.tn = r.tn;
  ex.nprob = nseg;
  for (int m = 0; m < nseg; ++m) {
    TnProblem& q = ex.prob[m];
    q.kind = TN_A_PLAIN; q.A = r.dxr; q.lda = L; q.M = L;
    q.B = rd->x[m]; q.ldb = kseg; q.Ncols = kseg;
    q.out = r.slab + (size_t)m * kseg; q.split_stride = (size_t)L * nseg * kseg; q.ldc = nseg * kseg;
    q.colsum = m == 0 ? r.cs : nullptr; q.colsum_stride = L;
  }
  return ex;
}
// reduce_dim's two sums, behind the stack's on the reduce list (gated: the stack's 10 + these 2 = every slot)
static void radio_reduce(const mmf_amil_desc* d, const mmf_radio_reduce* rd, const RadioWs& r, ReduceList& rl) {
  const int n = d->L * rd->nseg * rd->kseg;
  rl.add(r.slab, rd->dW, n, r.tn.splits, (size_t)n);
  rl.add(r.cs, rd->db, d->L, r.tn.splits, (size_t)d->L);
}
}  // namespace mmf

size_t mmf_amil_group_workspace_bytes(const int64_t* offsets, int32_t G, int32_t L, int32_t H, int32_t D, int32_t gated) {
  SegTable s;
  if (group_plan(offsets, G, s)) return 0;
  Carver c;
  return carve_group(c, s, L, H, D, gated).bytes;
}

int mmf_amil_nll_step_group(const mmf_amil_desc* d, const mmf_bag_group* group, const float* x, void* workspace,
                            size_t workspace_bytes, const mmf_surv_head* head, const mmf_nll_target* target,
                            float* A_raw, const mmf_amil_grads* g, void* stream) {
  SegTable s;
  HeadTail tl;
  if (int e = group_check(d, group, x, workspace, head, target, A_raw, g, s, tl)) return e;
  Carver c(workspace);
  GroupWs gw = carve_group(c, s, d->L, d->H, d->D, d->gated);
  if (gw.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  ReduceList rl;
  if (int e = group_chain(d, s, x, gw, tl, head->K, target, A_raw, g, nullptr, rl, st)) return e;
  return rl.launch(target->accumulate ? 1 : 0, st);
}

size_t mmf_radio_group_workspace_bytes(const int64_t* offsets, int32_t G, int32_t nseg, int32_t kseg, int32_t H,
                                       int32_t D, int32_t gated) {
  SegTable s;
  if (group_plan(offsets, G, s) || nseg < 2 || nseg > 4 || kseg < 1) return 0;
  Carver c;
  return carve_radio(c, s, nseg, kseg, H, D, gated).bytes;
}

int mmf_radio_nll_step_group(const mmf_amil_desc* d, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                             void* workspace, size_t workspace_bytes, const mmf_surv_head* head,
                             const mmf_nll_target* target, float* A_raw, const mmf_amil_grads* g, void* stream) {
  if (int e = radio_modalities(rd)) return e;
  SegTable s;
  HeadTail tl;
  if (int e = group_check(d, group, rd->x[0], workspace, head, target, A_raw, g, s, tl)) return e;
  if (int e = radio_operands(d, rd, true)) return e;
  Carver c(workspace);
  RadioWs r = carve_radio(c, s, rd->nseg, rd->kseg, d->H, d->D, d->gated);
  if (r.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  if (int e = launch_linear(radio_linear(d, rd, r.xr, r.kpart, d->seed_dev), st)) return e;

  const GroupExtra ex = radio_extra(d, rd, r);
  ReduceList rl;
  if (int e = group_chain(d, s, r.xr, r.gw, tl, head->K, target, A_raw, g, &ex, rl, st)) return e;
  radio_reduce(d, rd, r, rl);
  return rl.launch(target->accumulate ? 1 : 0, st);
}

// ---- grouped multimodal step: the two stacks' halves, the window's hazard head ------------------------------------
int mmf_amil_group_forward(const mmf_amil_desc* d, const mmf_bag_group* group, const float* x, void* workspace,
                           size_t workspace_bytes, float* M, int32_t ldm, float* A_raw, void* stream) {
  SegTable s;
  if (int e = group_half_check(d, group, x, workspace, M, ldm, A_raw, nullptr, false, s)) return e;
  Carver c(workspace);
  const GroupWs gw = carve_group(c, s, d->L, d->H, d->D, d->gated);
  if (gw.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  TraceScope ts(d->trace);
  return group_half_fwd(d, s, x, gw, M, ldm, A_raw, static_cast<hipStream_t>(stream));
}

int mmf_amil_group_backward(const mmf_amil_desc* d, const mmf_bag_group* group, const float* x, void* workspace,
                            size_t workspace_bytes, const float* dM, int32_t ldm, const float* A_raw,
                            const mmf_amil_grads* g, int32_t accumulate, void* stream) {
  SegTable s;
  if (int e = group_half_check(d, group, x, workspace, dM, ldm, A_raw, g, true, s)) return e;
  Carver c(workspace);
  const GroupWs gw = carve_group(c, s, d->L, d->H, d->D, d->gated);
  if (gw.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  ReduceList rl;
  if (int e = group_half_bwd(d, s, x, gw, dM, ldm, A_raw, g, nullptr, rl, st)) return e;
  return rl.launch(accumulate ? 1 : 0, st);
}

int mmf_radio_group_forward(const mmf_amil_desc* d, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                            void* workspace, size_t workspace_bytes, float* M, int32_t ldm, float* A_raw, void* stream) {
  if (int e = radio_modalities(rd)) return e;
  SegTable s;
  if (int e = group_half_check(d, group, rd->x[0], workspace, M, ldm, A_raw, nullptr, false, s)) return e;
  if (int e = radio_operands(d, rd, false)) return e;
  Carver c(workspace);
  const RadioWs r = carve_radio(c, s, rd->nseg, rd->kseg, d->H, d->D, d->gated);
  if (r.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  if (int e = launch_linear(radio_linear(d, rd, r.xr, r.kpart, d->seed_dev), st)) return e;
  return group_half_fwd(d, s, r.xr, r.gw, M, ldm, A_raw, st);
}

int mmf_radio_group_backward(const mmf_amil_desc* d, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                             void* workspace, size_t workspace_bytes, const float* dM, int32_t ldm, const float* A_raw,
                             const mmf_amil_grads* g, int32_t accumulate, void* stream) {
  if (int e = radio_modalities(rd)) return e;
  SegTable s;
  if (int e = group_half_check(d, group, rd->x[0], workspace, dM, ldm, A_raw, g, true, s)) return e;
  if (int e = radio_operands(d, rd, true)) return e;
  Carver c(workspace);
  const RadioWs r = carve_radio(c, s, rd->nseg, rd->kseg, d->H, d->D, d->gated);
  if (r.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  const GroupExtra ex = radio_extra(d, rd, r);
  ReduceList rl;
  if (int e = group_half_bwd(d, s, r.xr, r.gw, dM, ldm, A_raw, g, &ex, rl, st)) return e;
  radio_reduce(d, rd, r, rl);
  return rl.launch(accumulate ? 1 : 0, st);
}

namespace mmf {
// the window head's workspace: the per-patient classifier slabs the reduce launch sums
struct HeadGroupWs { float *wk, *bk; size_t bytes; };
static HeadGroupWs carve_head_group(Carver& c, int F, int K, int G) {
  HeadGroupWs w{};
  w.wk = c.take<float>((size_t)G * K * F);
  w.bk = c.take<float>((size_t)G * K);
  w.bytes = c.off;
  return w;
}
}  // namespace mmf

size_t mmf_surv_head_group_workspace_bytes(int32_t F, int32_t K, int32_t G) {
  if (F < 1 || F > 1024 || K < 1 || K > 32 || G < 1 || G > GROUP_MAX) return 0;
  Carver c;
  return carve_head_group(c, F, K, G).bytes;
}

int mmf_surv_head_nll_step_group(const float* feat, int32_t ldf, int32_t F, int32_t G, const mmf_surv_head* head,
                                 const mmf_nll_target* target, float* dfeat, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (!feat || !target || !dfeat || !workspace) return MMF_ERR_ARG;
  if (F < 1 || F > 1024 || ldf < F || G < 1 || G > GROUP_MAX) return MMF_ERR_SHAPE;
  PoolParams p{};
  if (int e = head_tail_of(head, target, p.tail)) return e;
  if (!aligned16(workspace)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  const HeadGroupWs w = carve_head_group(c, F, head->K, G);
  if (w.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  p.tail.dM = dfeat; p.tail.dWk = w.wk; p.tail.dbk = w.bk;
  p.M = const_cast<float*>(feat);        // read only
  p.H = F;
  if (int e = launch_surv_head_group(p, ldf, G, st)) return e;
  ReduceList rl;
  rl.add(w.wk, target->dWk, head->K * F, G, (size_t)head->K * F);     // the patients' slabs in patient order
  rl.add(w.bk, target->dbk, head->K, G, (size_t)head->K);
  return rl.launch(target->accumulate ? 1 : 0, st);
}

// ---- forward-only grouped pass: the bags of an evaluation window as one launch chain -----------------------------
namespace mmf {
// the window's forward-only workspace: the one-bag inference carve of R rows (fp32, or bf16: no SEG tables, no masks) and
// the per-bag pooling partials
struct GroupInferWs {
  AmilWs w;
  AmilWsBf wb;
  float* partials;
  size_t bytes;
};
static GroupInferWs carve_group_infer(Carver& c, const SegTable& s, int L, int H, int D, int gated, int bf16) {
  GroupInferWs g{};
  const int64_t R = s.off[s.G];
  if (bf16) g.wb = carve_bf16(c, R, L, H, D, gated, true);
  else g.w = carve(c, R, L, H, D, gated, true);
  g.partials = c.take<float>((size_t)s.gbeg[s.G] * (2 + H));
  g.bytes = c.off;
  return g;
}

// A bf16 stack whose one-bag route takes a fused forward form (amil_bf16_forward_impl: gated, H = D = 256).  The grouped
// pass runs the unfused bf16 kernels, which give such a bag other bf16 roundings than its one-bag route, so it refuses
// those windows; every other bf16 stack takes the unfused kernels one bag at a time too.
static bool infer_group_bf16_fused(const mmf_amil_desc* d) {
  return d->gated && d->H == 256 && d->D == 256;
}

// the call contract both forward-only grouped entry points share; fills the segment table and the head (no gradients)
static int infer_group_check(const mmf_amil_desc* d, const mmf_bag_group* group, const void* x, int bf16,
                             const void* workspace, const mmf_surv_head* head, const mmf_nll_target* target,
                             const float* M, const float* A_raw, SegTable& s, HeadTail& tl) {
  if (!d || !group) return MMF_ERR_ARG;
  if (d->gemm != MMF_GEMM_F32 || d->p_h != 0.f || d->p_att != 0.f) return MMF_ERR_ARG;
  if (int e = window_plan(d, group, bf16, s)) return e;
  if (bf16 && infer_group_bf16_fused(d)) return MMF_ERR_SHAPE;
  tl = HeadTail{};
  if (head) {
    if (int e = head_tail_of(head, target, tl, false)) return e;
  } else if (target || !M) {
    return MMF_ERR_ARG;             // a loss needs the head; without a head the call exists for M
  }
  return check_operands(d, x, workspace, A_raw, bf16);
}

// the fp32 chain over the window's rows x [R x L]: projection and gate with the one-bag plans of R rows (rows are
// independent, nothing is masked), the pooling partials per bag, the forward-only tail per bag
static int group_infer_chain(const mmf_amil_desc* d, const SegTable& s, const float* x, const GroupInferWs& gw,
                             const HeadTail& tl, float* M, float* A_raw, hipStream_t st) {
  const AmilWs& w = gw.w;
  if (int e = launch_linear(stack_linear(d, w, x, 0), st)) return e;
  if (int e = launch_gate_fwd(stack_gate_fwd(d, w, 0), st)) return e;
  PoolParams pp = stack_pool(d, w, A_raw);
  pp.partials = gw.partials; pp.M = M; pp.tail = tl;
  if (int e = launch_group_pool_partial(pp, s, st)) return e;
  return launch_group_infer_tail(pp, s, st);
}

// the bf16 chain (stacks whose one-bag route is unfused: infer_group_bf16_fused): weight conversion once per window, then
// the same unfused bf16 kernels over all R rows (their tiles may straddle bags: rows are independent), the pooling
// partials per bag from the bf16 h, the forward-only tail per bag
static int group_infer_chain_bf16(const mmf_amil_desc* d, const SegTable& s, const uint16_t* x, const GroupInferWs& gw,
                                  const HeadTail& tl, float* M, float* A_raw, hipStream_t st) {
  const AmilWsBf& w = gw.wb;
  if (int e = launch_cvt_bf16(stack_cvt_bf16(d, w, false, false), st)) return e;
  LinearBfParams lp = stack_linear_bf16(d, w, x, 0);
  lp.seed_dev = nullptr;              // nothing is masked (infer_group_check): this chain passes no seed word on
  if (int e = launch_linear_bf16(lp, st)) return e;
  GateBfParams gp = stack_gate_bf16(d, w, 0);
  gp.seed_dev = nullptr;
  if (int e = launch_gate_bf16(gp, st)) return e;
  PoolBfParams pb = stack_pool_bf16(d, w, A_raw);
  pb.base.partials = gw.partials; pb.base.M = M; pb.base.tail = tl;
  if (int e = launch_group_pool_partial_bf16(pb, s, st)) return e;
  return launch_group_infer_tail(pb.base, s, st);
}

// the radio window's forward-only workspace: the stack's (L = kseg), reduce_dim's output, its K-split partial tiles
struct RadioInferWs { GroupInferWs gw; float *xr, *kpart; size_t bytes; };
static RadioInferWs carve_radio_infer(Carver& c, const SegTable& s, int nseg, int kseg, int H, int D, int gated) {
  RadioInferWs r{};
  const int64_t R = s.off[s.G];
  r.gw = carve_group_infer(c, s, kseg, H, D, gated, 0);
  r.xr = c.take<float>((size_t)R * kseg);
  const size_t kf = linear_ksplit_floats(R, kseg, nseg * kseg, nseg, kseg);
  r.kpart = kf ? c.take<float>(kf) : nullptr;
  r.bytes = c.off;
  return r;
}
}  // namespace mmf

size_t mmf_amil_group_infer_workspace_bytes(const int64_t* offsets, int32_t G, int32_t L, int32_t H, int32_t D,
                                            int32_t gated, int32_t x_bf16) {
  SegTable s;
  if (group_plan(offsets, G, s)) return 0;
  Carver c;
  const size_t f32 = carve_group_infer(c, s, L, H, D, gated, 0).bytes;
  if (!x_bf16) return f32;
  Carver cb;
  const size_t b16 = carve_group_infer(cb, s, L, H, D, gated, 1).bytes;
  return b16 > f32 ? b16 : f32;        // one buffer serves a window of either storage (header)
}

int mmf_amil_infer_group(const mmf_amil_desc* d, const mmf_bag_group* group, const void* x, int32_t x_bf16,
                         void* workspace, size_t workspace_bytes, const mmf_surv_head* head, const mmf_nll_target* target,
                         float* M, float* A_raw, void* stream) {
  SegTable s;
  HeadTail tl;
  const int bf16 = x_bf16 ? 1 : 0;
  if (int e = infer_group_check(d, group, x, bf16, workspace, head, target, M, A_raw, s, tl)) return e;
  Carver c(workspace);
  const GroupInferWs gw = carve_group_infer(c, s, d->L, d->H, d->D, d->gated, bf16);
  if (gw.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  return bf16 ? group_infer_chain_bf16(d, s, static_cast<const uint16_t*>(x), gw, tl, M, A_raw, st)
              : group_infer_chain(d, s, static_cast<const float*>(x), gw, tl, M, A_raw, st);
}

size_t mmf_radio_group_infer_workspace_bytes(const int64_t* offsets, int32_t G, int32_t nseg, int32_t kseg, int32_t H,
                                             int32_t D, int32_t gated) {
  SegTable s;
  if (group_plan(offsets, G, s) || nseg < 2 || nseg > 4 || kseg < 1) return 0;
  Carver c;
  return carve_radio_infer(c, s, nseg, kseg, H, D, gated).bytes;
}

int mmf_radio_infer_group(const mmf_amil_desc* d, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                          void* workspace, size_t workspace_bytes, const mmf_surv_head* head,
                          const mmf_nll_target* target, float* M, float* A_raw, void* stream) {
  if (int e = radio_modalities(rd)) return e;
  SegTable s;
  HeadTail tl;
  if (int e = infer_group_check(d, group, rd->x[0], 0, workspace, head, target, M, A_raw, s, tl)) return e;
  if (int e = radio_operands(d, rd, false)) return e;
  Carver c(workspace);
  const RadioInferWs r = carve_radio_infer(c, s, rd->nseg, rd->kseg, d->H, d->D, d->gated);
  if (r.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  if (int e = launch_linear(radio_linear(d, rd, r.xr, r.kpart, nullptr), st)) return e;
  return group_infer_chain(d, s, r.xr, r.gw, tl, M, A_raw, st);
}

// ---- integrated gradients of the pathology head: the quadrature's steps as the bags of grouped windows ----------------
namespace mmf {
// The call evaluates n_steps + 2 steps: the quadrature's, then alpha = 1 and alpha = 0 with weight 0 (risk_x, risk_base).
// A window is `steps` of them over the bag's N rows, steps * N rows of H- and D-wide operands: the grouped chain's row
// limits (check_desc on sum N, without the L-wide bag, and group_plan's pooling groups).
static int64_t ig_row_limit(int H, int D) {
  const int64_t hd = H > D ? H : D, wide = H > 2 * D ? H : 2 * D;
  int64_t lim = (((int64_t)1 << 32) - 1) / hd;
  const int64_t bytes = (((int64_t)1 << 31) - 1) / (4 * wide), pool = (int64_t)GROUP_POOL_GROUPS * POOL_MAX_ROWS;
  if (bytes < lim) lim = bytes;
  return pool < lim ? pool : lim;
}
// steps per window: the caller's, or -- 0 -- windows of at most 2^18 rows (enough to fill the chip; the workspace stays
// near 1 GB for the small head) cut evenly; clamped to the row limit.  0: not even one step fits.
static int ig_window_steps(int64_t N, int H, int D, int total, int window_steps) {
  if (N < 1 || H < 1 || D < 1) return 0;
  int64_t smax = ig_row_limit(H, D) / N;
  if (smax < 1) return 0;
  if (smax > GROUP_MAX) smax = GROUP_MAX;
  if (smax > total) smax = total;
  if (window_steps > 0) return (int)(window_steps < smax ? window_steps : smax);
  int64_t s = ((int64_t)1 << 18) / N;
  if (s < 1) s = 1;
  if (s > smax) s = smax;
  const int64_t nwin = (total + s - 1) / s;
  return (int)((total + nwin - 1) / nwin);
}

struct IgWs : WindowWs {     // w: h, relu_bits, a, b, s_part, p, ds, dbc_part, du (nothing else is set)
  float *U, *G;              // [N x H]: x . W1^T, and the folded sum_s w_s du_s
  float *rs_part, *ra_part;  // [(attr_cols / 32) x N]: the attribution GEMM's per-block row sums
  float* kpart;              // the projection's K-split partial tiles, or null
  float* A_raw;
  size_t bytes;
};
// attr_cols: the attribution GEMM's columns -- L, or the radiology head's nseg * kseg (0: L)
static IgWs carve_ig(Carver& c, int64_t N, int L, int H, int D, int gated, int steps, int attr_cols = 0) {
  IgWs g{};
  if (attr_cols == 0) attr_cols = L;
  auto take = [&](size_t n) { return c.take<float>(n); };
  const int64_t R = N * steps;
  g.U = take((size_t)N * H);
  g.G = take((size_t)N * H);
  g.rs_part = take((size_t)(attr_cols / 32) * N);
  g.ra_part = take((size_t)(attr_cols / 32) * N);
  {
    const size_t kf = linear_ksplit_floats(N, H, L, 1, L);
    g.kpart = kf ? take(kf) : nullptr;
  }
  AmilWs& w = g.w;
  w.parts = gate_parts(D, gated);
  w.h = take((size_t)R * H);
  w.relu_bits = c.take<unsigned long long>((size_t)((R + 15) / 16 + 2) * (H / 32) * 8);
  w.a = take((size_t)R * D);
  w.b = take(gated ? (size_t)R * D : 0);
  w.s_part = take((size_t)w.parts * R);
  w.p = take((size_t)R);
  w.ds = take((size_t)R);
  w.dbc_part = take(PREP_GROUPS);
  w.du = take((size_t)R * H);
  g.M = take((size_t)steps * H);
  g.dM = take((size_t)steps * H);
  g.stats = take((size_t)2 * steps);
  g.partials = take((size_t)(GROUP_POOL_GROUPS + 2 * GROUP_MAX) * (2 + H));   // sum_s ceil(N / rpg) <= R / rpg + S
  g.A_raw = take((size_t)R);
  g.ridx_h = c.take<uint32_t>((size_t)R);
  g.ridx_d = c.take<uint32_t>((size_t)R);
  g.bag = c.take<int>((size_t)R);
  g.bytes = c.off;
  return g;
}

// The halves of one window, steps q0 .. q0 + S - 1 of the call, which the multimodal call (mmf_mm_ig) interleaves around its
// one head launch and the single-head calls run back to back (ig_window).
// the call's steps: the quadrature's, then the two riders alpha = 1 and alpha = 0 with weight 0 (risk_x, risk_base)
struct IgNodes { int n, total; float alpha[GROUP_MAX + 2], weight[GROUP_MAX + 2]; };
static IgNodes ig_nodes(int n_steps, const float* alpha, const float* weight) {
  IgNodes q{};
  q.n = n_steps; q.total = n_steps + 2;
  for (int k = 0; k < n_steps; ++k) { q.alpha[k] = alpha[k]; q.weight[k] = weight[k]; }
  q.alpha[n_steps] = 1.f; q.alpha[n_steps + 1] = 0.f;
  q.weight[n_steps] = q.weight[n_steps + 1] = 0.f;
  return q;
}
static IgSteps ig_steps(const IgNodes& q, int q0, int S) {
  IgSteps t{};
  t.S = S;
  for (int s = 0; s < S; ++s) { t.alpha[s] = q.alpha[q0 + s]; t.w[s] = q.weight[q0 + s]; }
  return t;
}
// of the window's S steps, the first `nfold` are the quadrature's: the two riders carry weight 0 and are not folded
static int ig_nfold(const IgNodes& q, int q0, int S) {
  int nfold = q.n - q0;
  if (nfold > S) nfold = S;
  return nfold < 0 ? 0 : nfold;
}

// forward, to the steps' embeddings: M_s into row s of M, ldm floats apart (and into g.M [S x H], with its statistics)
static int ig_window_fwd(const mmf_amil_desc* d, const IgWs& g, const IgSteps& steps, float* M, int ldm, hipStream_t st) {
  const int64_t N = d->N;
  const int S = steps.S;
  mmf_amil_desc dw = *d;                  // the window as a bag of S * N rows
  dw.N = N * S;
  int64_t offsets[GROUP_MAX + 1];
  for (int s = 0; s <= S; ++s) offsets[s] = s * N;
  SegTable seg;
  if (int e = group_plan(offsets, S, seg)) return e;
  if (seg.gbeg[S] > GROUP_POOL_GROUPS + 2 * GROUP_MAX) return MMF_ERR_SHAPE;
  const AmilWs& w = g.w;

  IgExpandParams ep{};
  ep.U = g.U; ep.b1 = d->b1; ep.h = w.h; ep.relu_bits = w.relu_bits; ep.N = N; ep.H = d->H;
  ep.st = steps;
  if (int e = launch_ig_expand(ep, st)) return e;
  if (int e = window_rows(&dw, seg, g, st)) return e;

  GateFwdParams gp = stack_gate_fwd(&dw, w, 0);
  gp.seg_ridx = g.ridx_d;
  if (int e = launch_gate_fwd_seg(gp, st)) return e;
  return window_pool(&dw, seg, g, M, ldm, g.A_raw, st);
}
// backward, from dM [S x H]: K-prep, K-dh, and the first `nfold` steps folded into g.G
static int ig_window_bwd(const mmf_amil_desc* d, const IgWs& g, const IgSteps& steps, const float* dM, int nfold, bool first,
                         hipStream_t st) {
  mmf_amil_desc dw = *d;
  dw.N = d->N * steps.S;
  const AmilWs& w = g.w;
  int dbc_parts;                                     // no weight gradients: nothing reduces them
  if (int e = window_dh(&dw, g, gate_bwd_ctx(&dw, w.a, w.b, w.ds, 0), dM, g.A_raw, dbc_parts, st)) return e;

  IgFoldParams fp{};
  fp.du = w.du; fp.G = g.G; fp.N = d->N; fp.H = d->H; fp.first = first ? 1 : 0;
  fp.st = steps; fp.st.S = nfold;
  return launch_ig_fold(fp, st);
}
// one window of a single head: the head's launch between the halves
static int ig_window(const mmf_amil_desc* d, const IgWs& g, const IgNodes& q, int q0, int S, IgHeadParams hp, hipStream_t st) {
  const IgSteps steps = ig_steps(q, q0, S);
  if (int e = ig_window_fwd(d, g, steps, g.M, d->H, st)) return e;
  hp.M = g.M; hp.dM = g.dM; hp.step0 = q0;
  if (int e = launch_ig_head(hp, S, st)) return e;
  return ig_window_bwd(d, g, steps, g.dM, ig_nfold(q, q0, S), q0 == 0, st);
}

// what both heads' calls refuse first: a null pointer, or a setting the call does not take
static int ig_args(const mmf_amil_desc* d, const mmf_surv_head* head, const mmf_ig_desc* ig) {
  if (!d || !ig || !head) return MMF_ERR_ARG;
  if (d->gemm != MMF_GEMM_F32 || d->p_h != 0.f || d->p_att != 0.f) return MMF_ERR_ARG;
  if (ig->n_steps < 1 || ig->n_steps > GROUP_MAX || ig->window_steps < 0 || !ig->alpha || !ig->weight) return MMF_ERR_ARG;
  if (!ig->row_sum || !ig->row_abs || !ig->risk_x || !ig->risk_base || !ig->step_risk) return MMF_ERR_ARG;
  return !head->Wk || !head->bk ? MMF_ERR_ARG : MMF_OK;
}

// the stack's projection without bias, activation or bits: g.U = rows . W1^T, once per call
static int ig_project(const mmf_amil_desc* d, const float* rows, const IgWs& g, hipStream_t st) {
  AmilWs wp{};
  wp.h = g.U; wp.kpart = g.kpart;
  LinearParams lp = stack_linear(d, wp, rows, 0);
  lp.bias = nullptr; lp.act = ACT_NONE; lp.drop_p = 0.f; lp.seed_dev = nullptr;
  return launch_linear(lp, st);
}
// the head's launch parameters over embeddings `width` wide, but for the window's M, dM and first step
static IgHeadParams ig_head_params(const mmf_surv_head* head, int width, int n_steps, float* step_risk, float* risk_x,
                                   float* risk_base) {
  IgHeadParams hp{};
  hp.Wk = head->Wk; hp.bk = head->bk; hp.K = head->K; hp.H = width; hp.n_steps = n_steps;
  hp.step_risk = step_risk; hp.risk_x = risk_x; hp.risk_base = risk_base;
  hp.logits = head->logits; hp.hazards = head->hazards; hp.S = head->S; hp.risk = head->risk; hp.Y_hat = head->Y_hat;
  return hp;
}

// The quadrature over the stack d behind its projection (g.U): the windows, `steps` steps each, which leave the folded
// sum_s w_s du_s in g.G and the risks where ig says.
static int ig_windows(const mmf_amil_desc* d, const IgWs& g, int steps, const mmf_surv_head* head, const mmf_ig_desc* ig,
                      hipStream_t st) {
  const IgNodes q = ig_nodes(ig->n_steps, ig->alpha, ig->weight);
  const IgHeadParams hp = ig_head_params(head, d->H, q.n, ig->step_risk, ig->risk_x, ig->risk_base);
  for (int q0 = 0; q0 < q.total; q0 += steps) {
    const int S = q.total - q0 < steps ? q.total - q0 : steps;
    if (int e = ig_window(d, g, q, q0, S, hp, st)) return e;
  }
  return MMF_OK;
}
// the pathology head's last launch: attr = x * (Gacc . W1), and its row sums
static int ig_attr(const mmf_amil_desc* d, const float* x, const IgWs& g, float* row_sum, float* row_abs, float* attr,
                   hipStream_t st) {
  NnParams np{};
  np.A = g.G; np.lda = d->H; np.B = d->W1; np.ldb = d->L; np.C = attr; np.ldc = d->L;
  np.M = d->N; np.N = d->L; np.K = d->H;
  np.mulx = x; np.ldx = d->L; np.rs_part = g.rs_part; np.ra_part = g.ra_part;
  return launch_nn_attr(np, row_sum, row_abs, st);
}
}  // namespace mmf

size_t mmf_amil_ig_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated, int32_t n_steps,
                                   int32_t window_steps) {
  if (n_steps < 1 || n_steps > GROUP_MAX || window_steps < 0 || L < 32 || H < 32) return 0;
  const int steps = ig_window_steps(N, H, D, n_steps + 2, window_steps);
  if (steps < 1) return 0;
  Carver c;
  return carve_ig(c, N, L, H, D, gated, steps).bytes;
}

int mmf_amil_ig(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes,
                const mmf_surv_head* head, const mmf_ig_desc* ig, void* stream) {
  if (int e = ig_args(d, head, ig)) return e;
  if (int e = check_desc(d)) return e;
  if (head->K < 1 || head->K > 32) return MMF_ERR_SHAPE;
  const int steps = ig_window_steps(d->N, d->H, d->D, ig->n_steps + 2, ig->window_steps);
  if (steps < 1) return MMF_ERR_SHAPE;
  if (int e = check_operands(d, x, workspace, ig->row_sum, false)) return e;
  if (ig->attr && !aligned16(ig->attr)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  const IgWs g = carve_ig(c, d->N, d->L, d->H, d->D, d->gated, steps);
  if (g.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  if (int e = ig_project(d, x, g, st)) return e;
  if (int e = ig_windows(d, g, steps, head, ig, st)) return e;
  return ig_attr(d, x, g, ig->row_sum, ig->row_abs, ig->attr, st);
}

// ---- integrated gradients of the radiology head: reduce_dim folded into the same windows -------------------------------
namespace mmf {
struct RadioIgWs {
  IgWs g;
  float* Y;        // [N x L]: X Wr^T without bias, then P = Gacc W1 (Y is dead once U is formed)
  float* b1c;      // [H]: b1 + W1 br
  float* kpart;    // reduce_dim's K-split partial tiles, or null
  size_t bytes;
};
static RadioIgWs carve_radio_ig(Carver& c, int64_t N, int nseg, int kseg, int H, int D, int gated, int steps) {
  RadioIgWs r{};
  r.Y = c.take<float>((size_t)N * kseg);
  r.b1c = c.take<float>((size_t)H);
  const size_t kf = linear_ksplit_floats(N, kseg, nseg * kseg, nseg, kseg);
  r.kpart = kf ? c.take<float>(kf) : nullptr;
  r.g = carve_ig(c, N, kseg, H, D, gated, steps, nseg * kseg);
  r.bytes = c.off;
  return r;
}
// what mmf_radio_ig refuses of rd before the descriptor's rules: the null pointers, then the modality count
static int radio_ig_args(const mmf_radio_reduce* rd) {
  if (!rd || !rd->x || !rd->W || !rd->bias) return MMF_ERR_ARG;
  const bool nseg_ok = rd->nseg >= 2 && rd->nseg <= 4;
  for (int m = 0; nseg_ok && m < rd->nseg; ++m)
    if (!rd->x[m]) return MMF_ERR_ARG;
  return nseg_ok ? MMF_OK : MMF_ERR_SHAPE;
}
// once per call, before the windows: Y = X Wr^T, b1' = b1 + W1 br and, through the stack `db` behind reduce_dim (u =
// alpha U + b1'), U = Y W1^T
static int radio_ig_project(const mmf_amil_desc* d, const mmf_radio_reduce* rd, const RadioIgWs& r, mmf_amil_desc& db,
                            hipStream_t st) {
  {   // reduce_dim over the segments without its bias, the forward-only pass's plan for N rows
    LinearParams lr = radio_linear(d, rd, r.Y, r.kpart, nullptr);
    lr.bias = nullptr;
    if (int e = launch_linear(lr, st)) return e;
  }
  if (int e = launch_ig_bias(d->W1, rd->bias, d->b1, r.b1c, d->H, d->L, st)) return e;
  db = *d;
  db.b1 = r.b1c;
  return ig_project(&db, r.Y, r.g, st);
}
// once per call, behind the windows: P = Gacc W1 [N x L] in Y's place, then attr_m = x_m * (P Wr)[:, m kseg ..] and its row
// sums per modality
static int radio_ig_attr(const mmf_amil_desc* d, const mmf_radio_reduce* rd, const RadioIgWs& r, float* row_sum,
                         float* row_abs, float* attr, hipStream_t st) {
  const int nseg = rd->nseg, kseg = rd->kseg, L = d->L, H = d->H;
  const IgWs& g = r.g;
  float* P = r.Y;
  NnParams np{};
  np.A = g.G; np.lda = H; np.B = d->W1; np.ldb = L; np.C = P; np.ldc = L;
  np.M = d->N; np.N = L; np.K = H;
  if (int e = launch_nn(np, st)) return e;
  NnParams nq{};
  nq.A = P; nq.lda = L; nq.B = rd->W; nq.ldb = nseg * kseg; nq.C = attr;
  nq.M = d->N; nq.N = nseg * kseg; nq.K = L;
  for (int m = 0; m < nseg; ++m) nq.segx[m] = rd->x[m];
  nq.kseg = kseg; nq.rs_part = g.rs_part; nq.ra_part = g.ra_part;
  return launch_nn_attr_seg(nq, row_sum, row_abs, st);
}
}  // namespace mmf

size_t mmf_radio_ig_workspace_bytes(int64_t N, int32_t nseg, int32_t kseg, int32_t H, int32_t D, int32_t gated,
                                    int32_t n_steps, int32_t window_steps) {
  if (n_steps < 1 || n_steps > GROUP_MAX || window_steps < 0 || N < 1 || nseg < 2 || nseg > 4 || kseg < 32 || H < 32)
    return 0;
  if (N * nseg * (int64_t)kseg * 4 >= (int64_t)1 << 31) return 0;
  const int steps = ig_window_steps(N, H, D, n_steps + 2, window_steps);
  if (steps < 1) return 0;
  Carver c;
  return carve_radio_ig(c, N, nseg, kseg, H, D, gated, steps).bytes;
}

int mmf_radio_ig(const mmf_amil_desc* d, const mmf_radio_reduce* rd, void* workspace, size_t workspace_bytes,
                 const mmf_surv_head* head, const mmf_ig_desc* ig, void* stream) {
  if (int e = ig_args(d, head, ig)) return e;
  if (int e = radio_ig_args(rd)) return e;
  if (int e = check_desc(d)) return e;
  const int nseg = rd->nseg, kseg = rd->kseg, L = d->L, H = d->H;
  if (kseg != L) return MMF_ERR_SHAPE;
  if (d->N * nseg * (int64_t)kseg * 4 >= (int64_t)1 << 31) return MMF_ERR_SHAPE;     // mmf_radio_nll_step_group's input rule
  if (head->K < 1 || head->K > 32) return MMF_ERR_SHAPE;
  const int steps = ig_window_steps(d->N, d->H, d->D, ig->n_steps + 2, ig->window_steps);
  if (steps < 1) return MMF_ERR_SHAPE;
  if (int e = radio_operands(d, rd, false)) return e;                                // what is left of it: the alignments
  if (int e = check_operands(d, rd->x[0], workspace, ig->row_sum, false)) return e;
  if (ig->attr && !aligned16(ig->attr)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  const RadioIgWs r = carve_radio_ig(c, d->N, nseg, kseg, H, d->D, d->gated, steps);
  if (r.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  mmf_amil_desc db;
  if (int e = radio_ig_project(d, rd, r, db, st)) return e;
  if (int e = ig_windows(&db, r.g, steps, head, ig, st)) return e;
  return radio_ig_attr(d, rd, r, ig->row_sum, ig->row_abs, ig->attr, st);
}

// ---- integrated gradients of the multimodal concat head: two stacks and the omic SNN around one head launch -------------
namespace mmf {
struct MmIgWs {
  IgWs gp;                   // the pathology stack's
  RadioIgWs gr;              // the radiology stack's
  float *Z, *z1, *z2, *dz1, *Gz;   // omic: [W0], [S x W0], [S x We], [S x W0], [W0]
  float *feat, *dfeat;       // [S x F] each
  size_t bytes;
};
// a branch is absent with Np = 0, Nr = 0, Gin = 0
static MmIgWs carve_mm_ig(Carver& c, int64_t Np, int Lp, int Hp, int Dp, int gated_p, int64_t Nr, int nseg, int kseg, int Hr,
                          int Dr, int gated_r, int Gin, int W0, int We, int F, int steps) {
  MmIgWs m{};
  if (Np > 0) m.gp = carve_ig(c, Np, Lp, Hp, Dp, gated_p, steps);
  if (Nr > 0) m.gr = carve_radio_ig(c, Nr, nseg, kseg, Hr, Dr, gated_r, steps);
  if (Gin > 0) {
    m.Z = c.take<float>((size_t)W0);
    m.z1 = c.take<float>((size_t)steps * W0);
    m.z2 = c.take<float>((size_t)steps * We);
    m.dz1 = c.take<float>((size_t)steps * W0);
    m.Gz = c.take<float>((size_t)W0);
  }
  m.feat = c.take<float>((size_t)steps * F);
  m.dfeat = c.take<float>((size_t)steps * F);
  m.bytes = c.off;
  return m;
}
// one S for the whole call: the smaller of what ig_window_steps gives each present stack; 0: some stack admits no window
static int mm_ig_steps(int64_t Np, int Hp, int Dp, int64_t Nr, int Hr, int Dr, int total, int window_steps) {
  int steps = total;
  if (Np > 0) {
    const int s = ig_window_steps(Np, Hp, Dp, total, window_steps);
    if (s < steps) steps = s;
  }
  if (Nr > 0) {
    const int s = ig_window_steps(Nr, Hr, Dr, total, window_steps);
    if (s < steps) steps = s;
  }
  return steps;
}
// the present branches' column ranges must tile 0 .. F - 1
static bool mm_ig_columns(const int* col, const int* width, int n, int F) {
  int at = 0;
  for (int done = 0; done < n; ++done) {
    int k = -1;
    for (int i = 0; i < n; ++i)
      if (col[i] == at) k = i;
    if (k < 0) return false;
    at += width[k];
  }
  return at == F;
}
// a stack in eval mode with the exact-fp32 GEMMs, as ig_args asks of the single heads
static int mm_ig_stack_args(const mmf_amil_desc* d, const float* row_sum, const float* row_abs) {
  if (!row_sum || !row_abs) return MMF_ERR_ARG;
  return d->gemm != MMF_GEMM_F32 || d->p_h != 0.f || d->p_att != 0.f ? MMF_ERR_ARG : MMF_OK;
}
}  // namespace mmf

size_t mmf_mm_ig_workspace_bytes(int64_t N_p, int32_t L_p, int32_t H_p, int32_t D_p, int32_t gated_p, int64_t N_r,
                                 int32_t nseg, int32_t kseg, int32_t H_r, int32_t D_r, int32_t gated_r, int32_t Gin,
                                 int32_t W0, int32_t We, int32_t n_steps, int32_t window_steps) {
  if (n_steps < 1 || n_steps > GROUP_MAX || window_steps < 0 || N_p < 0 || N_r < 0 || Gin < 0) return 0;
  if ((N_p > 0) + (N_r > 0) + (Gin > 0) < 2) return 0;
  int64_t F = 0;
  if (N_p > 0) {
    if (!mmf_amil_ig_workspace_bytes(N_p, L_p, H_p, D_p, gated_p, n_steps, window_steps)) return 0;
    F += H_p;
  }
  if (N_r > 0) {
    if (!mmf_radio_ig_workspace_bytes(N_r, nseg, kseg, H_r, D_r, gated_r, n_steps, window_steps)) return 0;
    F += H_r;
  }
  if (Gin > 0) {
    if (W0 < 1 || W0 > 1024 || We < 1) return 0;
    F += We;
  }
  if (F > 1024) return 0;
  const int steps = mm_ig_steps(N_p, H_p, D_p, N_r, H_r, D_r, n_steps + 2, window_steps);
  if (steps < 1) return 0;
  Carver c;
  return carve_mm_ig(c, N_p, L_p, H_p, D_p, gated_p, N_r, nseg, kseg, H_r, D_r, gated_r, Gin, W0, We, (int)F, steps).bytes;
}

// mmf_mm_ig and mmf_mm_ig_tensor: one body, behind the fusion tail it may run (mm_ig_call, below)

int mmf_surv_head_nll_step(const float* feat, int32_t F, const mmf_surv_head* head, const mmf_nll_target* target,
                           float* dfeat, void* stream) {
  if (!feat || !target || !dfeat) return MMF_ERR_ARG;
  if (F < 1 || F > 1024) return MMF_ERR_SHAPE;
  PoolParams p{};
  if (int e = head_tail_of(head, target, p.tail)) return e;
  p.tail.dM = dfeat;
  p.M = const_cast<float*>(feat);        // read only: the launch neither merges nor stores M
  p.H = F;
  return launch_head_tail(p, static_cast<hipStream_t>(stream));
}

// ---- forward-only grouped pass of the multimodal head: the fusion tail and the hazard head of a window -----------------
int mmf_surv_head_infer_group(const float* const* segs, const int32_t* widths, int32_t nseg, int32_t G,
                              const mmf_surv_head* head, const mmf_nll_target* target, void* stream) {
  if (!segs || !widths) return MMF_ERR_ARG;
  if (nseg < 1 || nseg > 3 || G < 1 || G > GROUP_MAX) return MMF_ERR_SHAPE;
  HeadSegs s{};
  s.n = nseg;
  int F = 0;
  for (int i = 0; i < nseg; ++i) {
    if (!segs[i]) return MMF_ERR_ARG;
    if (widths[i] < 1 || widths[i] > 1024) return MMF_ERR_SHAPE;
    s.x[i] = segs[i]; s.width[i] = widths[i];
    F += widths[i];
  }
  if (F > 1024) return MMF_ERR_SHAPE;
  PoolParams p{};
  if (int e = head_tail_of(head, target, p.tail, false)) return e;
  p.H = F;
  return launch_surv_head_infer_group(p, s, G, static_cast<hipStream_t>(stream));
}

namespace mmf {
// the window's fusion workspace: o of the gating stage and encoder1's output
struct XFusionWs { float *o, *e1; size_t bytes; };
static XFusionWs carve_xfusion(Carver& c, int m, int sdim, int mmhid1, int G) {
  XFusionWs w{};
  w.o = c.take<float>((size_t)G * m * sdim);
  w.e1 = c.take<float>((size_t)G * mmhid1);
  w.bytes = c.off;
  return w;
}
static bool xfusion_shape_ok(int m, int sdim, int mmhid1, int G) {
  return m >= 2 && m <= 3 && sdim == 16 && mmhid1 >= 1 && mmhid1 <= 64 * DENSE_SEGS_MAXC && G >= 1 && G <= GROUP_MAX;
}
}  // namespace mmf

size_t mmf_xfusion_group_infer_workspace_bytes(int32_t m, int32_t sdim, int32_t mmhid1, int32_t G) {
  if (!xfusion_shape_ok(m, sdim, mmhid1, G)) return 0;
  Carver c;
  return carve_xfusion(c, m, sdim, mmhid1, G).bytes;
}

int mmf_xfusion_infer_group(const mmf_xfusion_weights* w, const float* const* v, int32_t G, void* workspace,
                            size_t workspace_bytes, float* MM, float* hid, void* stream) {
  if (!w || !v || !workspace || !MM || !hid) return MMF_ERR_ARG;
  if (!xfusion_shape_ok(w->m, w->sdim, w->mmhid1, G)) return MMF_ERR_SHAPE;
  if (w->dim < 4 || w->dim % 4 != 0 || w->mmhid2 < 1 || w->nhid < 1) return MMF_ERR_SHAPE;
  if (w->mmhid1 + w->m * w->dim > 64 * DENSE_SEGS_MAXC || w->mmhid2 > 64 * DENSE_SEGS_MAXC) return MMF_ERR_SHAPE;
  if (!w->We1 || !w->be1 || !w->We2 || !w->be2 || !w->Wc0 || !w->bc0) return MMF_ERR_ARG;
  XGateGroupParams gp{};
  gp.m = w->m; gp.G = G; gp.dim = w->dim; gp.sdim = w->sdim;
  for (int i = 0; i < w->m; ++i) {
    if (!v[i] || !w->Wh[i] || !w->bh[i] || !w->Wz[i] || !w->bz[i] || !w->Wo[i] || !w->bo[i]) return MMF_ERR_ARG;
    if (!aligned16(v[i]) || !aligned16(w->Wh[i]) || !aligned16(w->Wz[i])) return MMF_ERR_ALIGN;     // float4 loads
    gp.v[i] = v[i]; gp.Wh[i] = w->Wh[i]; gp.bh[i] = w->bh[i]; gp.Wz[i] = w->Wz[i]; gp.bz[i] = w->bz[i];
    gp.Wo[i] = w->Wo[i]; gp.bo[i] = w->bo[i];
  }
  if (!aligned16(workspace)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  const XFusionWs ws = carve_xfusion(c, w->m, w->sdim, w->mmhid1, G);
  if (ws.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  gp.o = ws.o;
  if (int e = launch_xgate_group(gp, st)) return e;
  KronDenseGroupParams kp{w->m, G, w->mmhid1, ws.o, w->We1, w->be1, ws.e1};
  if (int e = launch_kron_dense_group(kp, st)) return e;
  DenseSegsParams e2{};                 // encoder2 on [e1 | v_0 | v_1 (| v_2)], read where the parts lie
  e2.nseg = 1 + w->m; e2.G = G; e2.N = w->mmhid2; e2.K = w->mmhid1 + w->m * w->dim;
  e2.x[0] = ws.e1; e2.width[0] = w->mmhid1;
  for (int i = 0; i < w->m; ++i) { e2.x[1 + i] = v[i]; e2.width[1 + i] = w->dim; }
  e2.W = w->We2; e2.bias = w->be2; e2.y = MM;
  if (int e = launch_dense_segs_group(e2, st)) return e;
  DenseSegsParams c0{};                 // classifier[0] + ReLU
  c0.nseg = 1; c0.G = G; c0.N = w->nhid; c0.K = w->mmhid2;
  c0.x[0] = MM; c0.width[0] = w->mmhid2;
  c0.W = w->Wc0; c0.bias = w->bc0; c0.y = hid;
  return launch_dense_segs_group(c0, st);
}

// ---- grouped training step of the tensor fusion: the forward and the backward of the fusion tail of a window ----------
static DropSpec make_drop(int kind, float p, uint32_t seed, uint32_t site, const uint32_t* seed_dev);
namespace mmf {
// What the forward keeps for the backward (o dropped, h, z, gm, the post-fusion keep bits) and the backward's own buffers.
struct XFusionTrainWs {
  float *o, *h, *z, *gm, *dpo, *dz, *dph, *dkr, *dMM, *dpre, *tmpW, *tmpb;
  uint32_t* bits;
  size_t bytes;
};
static int xfusion_elems(int m) { return m == 3 ? 17 * 17 * 17 : 17 * 17; }
static XFusionTrainWs carve_xfusion_train(Carver& c, int m, int dim, int mmhid1, int mmhid2, int nhid, int G) {
  XFusionTrainWs w{};
  const size_t gate = (size_t)G * m * 16, K2 = (size_t)mmhid1 + (size_t)m * dim;
  w.o = c.take<float>(gate); w.h = c.take<float>(gate); w.z = c.take<float>(gate); w.gm = c.take<float>(gate);
  w.bits = c.take<uint32_t>((size_t)G * xfusion_bit_words(m));
  w.dpo = c.take<float>(gate); w.dz = c.take<float>(gate); w.dph = c.take<float>(gate);
  w.dkr = c.take<float>((size_t)G * xfusion_elems(m));
  w.dMM = c.take<float>((size_t)G * mmhid2);
  w.dpre = c.take<float>((size_t)G * (mmhid2 > nhid ? mmhid2 : nhid));
  const size_t w2 = (size_t)mmhid2 * K2, w0 = (size_t)nhid * mmhid2;      // accumulate: the dense backward's fresh dW, db
  w.tmpW = c.take<float>(w2 > w0 ? w2 : w0);
  w.tmpb = c.take<float>(mmhid2 > nhid ? mmhid2 : nhid);
  w.bytes = c.off;
  return w;
}
static int xfusion_train_shape(const mmf_xfusion_weights* w, int G) {
  if (!xfusion_shape_ok(w->m, w->sdim, w->mmhid1, G)) return MMF_ERR_SHAPE;
  if (w->dim < 4 || w->dim % 4 != 0 || w->mmhid1 % 4 != 0 || w->mmhid2 < 1 || w->nhid < 1) return MMF_ERR_SHAPE;
  if (w->mmhid1 + w->m * w->dim > 64 * DENSE_SEGS_MAXC || w->mmhid2 > 64 * DENSE_SEGS_MAXC || w->nhid > 64 * DENSE_SEGS_MAXC)
    return MMF_ERR_SHAPE;
  return MMF_OK;
}
// the null pointers of the weights (m is clamped: mm_ig_call asks before the shape is known), then the float4 operands
static int xfusion_weights_args(const mmf_xfusion_weights* w) {
  if (!w->We1 || !w->be1 || !w->We2 || !w->be2 || !w->Wc0 || !w->bc0) return MMF_ERR_ARG;
  for (int i = 0; i < w->m && i < 3; ++i)
    if (!w->Wh[i] || !w->bh[i] || !w->Wz[i] || !w->bz[i] || !w->Wo[i] || !w->bo[i]) return MMF_ERR_ARG;
  return MMF_OK;
}
static int xfusion_weights_aligned(const mmf_xfusion_weights* w) {
  for (int i = 0; i < w->m; ++i)
    if (!aligned16(w->Wh[i]) || !aligned16(w->Wz[i])) return MMF_ERR_ALIGN;     // float4 loads
  return MMF_OK;
}
static int xfusion_train_weights(const mmf_xfusion_weights* w) {
  if (int e = xfusion_weights_args(w)) return e;
  return xfusion_weights_aligned(w);
}
static XTrainParams xtrain(float p, uint32_t site, const uint32_t* row_base, const uint32_t* seed_dev) {
  XTrainParams t{};
  t.p = p; t.key = drop_key(0, site); t.dev = seed_dev; t.row_base = row_base;
  return t;
}
// the gating stage, the Kronecker product fused into encoder1 and encoder2 over the rows of x2 [G x K2], whose embedding
// columns the caller filled: e1 into x2's first columns, MM [G x mmhid2] (mmf_xfusion_group_forward; mm_ig_call at p = 0)
static int xfusion_group_fwd_launches(const mmf_xfusion_weights* w, float* x2, int G, float drop_p, const uint32_t* row_base,
                                      const uint32_t* seed_dev, const XFusionTrainWs& ws, float* MM, hipStream_t st) {
  const int K2 = w->mmhid1 + w->m * w->dim;
  XGateGroupParams gp{};
  gp.m = w->m; gp.G = G; gp.dim = w->dim; gp.sdim = w->sdim;
  for (int i = 0; i < w->m; ++i) {
    gp.v[i] = x2 + w->mmhid1 + i * w->dim; gp.Wh[i] = w->Wh[i]; gp.bh[i] = w->bh[i]; gp.Wz[i] = w->Wz[i];
    gp.bz[i] = w->bz[i]; gp.Wo[i] = w->Wo[i]; gp.bo[i] = w->bo[i];
  }
  gp.o = ws.o;
  XTrainParams tg = xtrain(drop_p, 0, row_base, seed_dev);
  tg.key8 = drop_key(0, 8); tg.ld = K2; tg.h = ws.h; tg.z = ws.z; tg.gm = ws.gm; tg.bits = ws.bits;
  if (int e = launch_xgate_group_train(gp, tg, st)) return e;
  KronDenseGroupParams kp{w->m, G, w->mmhid1, ws.o, w->We1, w->be1, x2};      // e1 into the first columns of x2
  XTrainParams tk = xtrain(drop_p, 9, row_base, seed_dev);
  tk.ld = K2; tk.bits = ws.bits;
  if (int e = launch_kron_dense_group_train(kp, tk, st)) return e;
  DenseSegsParams e2{};                 // encoder2 on the rows of x2 = [e1 | v_0 | v_1 (| v_2)]
  e2.nseg = 1; e2.G = G; e2.N = w->mmhid2; e2.K = K2;
  e2.x[0] = x2; e2.width[0] = K2;
  e2.W = w->We2; e2.bias = w->be2; e2.y = MM;
  return launch_dense_segs_group_train(e2, xtrain(drop_p, 10, row_base, seed_dev), st);
}
// the parameter block of the backward in front of encoder2; g null: the input-gradient launches alone read it
static XFusionBwdParams xfusion_bwd_params(const mmf_xfusion_weights* w, const float* x2, float* dx2, int G, float drop_p,
                                           int accumulate, const XFusionTrainWs& ws, const mmf_xfusion_grads* g) {
  const int K2 = w->mmhid1 + w->m * w->dim;
  XFusionBwdParams p{};
  p.m = w->m; p.G = G; p.dim = w->dim; p.N1 = w->mmhid1; p.K2 = K2; p.p = drop_p; p.accumulate = accumulate;
  p.x2 = x2; p.dx2 = dx2; p.o = ws.o; p.h = ws.h; p.z = ws.z; p.gm = ws.gm; p.bits = ws.bits; p.dkr = ws.dkr;
  p.dpo = ws.dpo; p.dz = ws.dz; p.dph = ws.dph; p.We1 = w->We1;
  for (int i = 0; i < w->m; ++i) {
    p.Wh[i] = w->Wh[i]; p.Wz[i] = w->Wz[i]; p.Wo[i] = w->Wo[i];
    if (g) {
      p.dWh[i] = g->dWh[i]; p.dbh[i] = g->dbh[i]; p.dWz[i] = g->dWz[i]; p.dbz[i] = g->dbz[i];
      p.dWo[i] = g->dWo[i]; p.dbo[i] = g->dbo[i];
    }
  }
  if (g) { p.dWe1 = g->dWe1; p.dbe1 = g->dbe1; }
  return p;
}
}  // namespace mmf

size_t mmf_xfusion_group_workspace_bytes(int32_t m, int32_t dim, int32_t sdim, int32_t mmhid1, int32_t mmhid2,
                                         int32_t nhid, int32_t G) {
  mmf_xfusion_weights w{};
  w.m = m; w.dim = dim; w.sdim = sdim; w.mmhid1 = mmhid1; w.mmhid2 = mmhid2; w.nhid = nhid;
  if (xfusion_train_shape(&w, G)) return 0;
  Carver c;
  return carve_xfusion_train(c, m, dim, mmhid1, mmhid2, nhid, G).bytes;
}

int mmf_xfusion_group_forward(const mmf_xfusion_weights* w, float* x2, int32_t G, float drop_p, float cls_drop_p,
                              const uint32_t* row_base, const uint32_t* seed_dev, void* workspace, size_t workspace_bytes,
                              float* MM, float* hid, void* stream) {
  if (!w || !x2 || !row_base || !workspace || !MM || !hid) return MMF_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f) || !(cls_drop_p >= 0.f && cls_drop_p < 1.f)) return MMF_ERR_ARG;
  if (int e = xfusion_train_shape(w, G)) return e;
  if (int e = xfusion_train_weights(w)) return e;
  if (!aligned16(x2) || !aligned16(workspace)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  const XFusionTrainWs ws = carve_xfusion_train(c, w->m, w->dim, w->mmhid1, w->mmhid2, w->nhid, G);
  if (ws.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int e = xfusion_group_fwd_launches(w, x2, G, drop_p, row_base, seed_dev, ws, MM, st)) return e;
  DenseSegsParams c0{};                 // classifier[0] + ReLU + Dropout
  c0.nseg = 1; c0.G = G; c0.N = w->nhid; c0.K = w->mmhid2;
  c0.x[0] = MM; c0.width[0] = w->mmhid2;
  c0.W = w->Wc0; c0.bias = w->bc0; c0.y = hid;
  return launch_dense_segs_group_train(c0, xtrain(cls_drop_p, 11, row_base, seed_dev), st);
}

int mmf_xfusion_group_backward(const mmf_xfusion_weights* w, const float* x2, int32_t G, float drop_p, float cls_drop_p,
                               const uint32_t* row_base, const uint32_t* seed_dev, const float* MM, const float* hid,
                               const float* dhid, int32_t lddhid, void* workspace, size_t workspace_bytes, float* dx2,
                               const mmf_xfusion_grads* grads, int32_t accumulate, void* stream) {
  if (!w || !x2 || !row_base || !MM || !hid || !dhid || !workspace || !dx2 || !grads) return MMF_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f) || !(cls_drop_p >= 0.f && cls_drop_p < 1.f)) return MMF_ERR_ARG;
  if (int e = xfusion_train_shape(w, G)) return e;
  if (lddhid < w->nhid) return MMF_ERR_SHAPE;
  if (int e = xfusion_train_weights(w)) return e;
  const mmf_xfusion_grads* g = grads;
  if (!g->dWe1 || !g->dbe1 || !g->dWe2 || !g->dbe2 || !g->dWc0 || !g->dbc0) return MMF_ERR_ARG;
  for (int i = 0; i < w->m; ++i)
    if (!g->dWh[i] || !g->dbh[i] || !g->dWz[i] || !g->dbz[i] || !g->dWo[i] || !g->dbo[i]) return MMF_ERR_ARG;
  if (!aligned16(x2) || !aligned16(workspace)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  const XFusionTrainWs ws = carve_xfusion_train(c, w->m, w->dim, w->mmhid1, w->mmhid2, w->nhid, G);
  if (ws.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int K2 = w->mmhid1 + w->m * w->dim;
  // classifier[0] and encoder2: the dense backward on B = G rows (accumulate: into the workspace, then added)
  DenseBwdParams c0{dhid, hid, MM, w->Wc0, ws.dpre, ws.dMM, accumulate ? ws.tmpW : g->dWc0, accumulate ? ws.tmpb : g->dbc0,
                    G, w->mmhid2, w->nhid, ACT_RELU, make_drop(1, cls_drop_p, 0, 11, seed_dev), row_base, w->nhid, lddhid};
  if (int e = launch_dense_bwd(c0, st)) return e;
  if (accumulate) {
    if (int e = launch_add_into(g->dWc0, ws.tmpW, (int64_t)w->nhid * w->mmhid2, st)) return e;
    if (int e = launch_add_into(g->dbc0, ws.tmpb, w->nhid, st)) return e;
  }
  DenseBwdParams e2{ws.dMM, MM, x2, w->We2, ws.dpre, dx2, accumulate ? ws.tmpW : g->dWe2, accumulate ? ws.tmpb : g->dbe2,
                    G, K2, w->mmhid2, ACT_RELU, make_drop(1, drop_p, 0, 10, seed_dev), row_base, w->mmhid2, w->mmhid2};
  if (int e = launch_dense_bwd(e2, st)) return e;
  if (accumulate) {
    if (int e = launch_add_into(g->dWe2, ws.tmpW, (int64_t)w->mmhid2 * K2, st)) return e;
    if (int e = launch_add_into(g->dbe2, ws.tmpb, w->mmhid2, st)) return e;
  }
  const XFusionBwdParams p = xfusion_bwd_params(w, x2, dx2, G, drop_p, accumulate, ws, g);
  return launch_xfusion_group_bwd(p, st);
}

// ---- integrated gradients of the multimodal head, both fusions: mmf_mm_ig and mmf_mm_ig_tensor ------------------------
namespace mmf {
// The tensor fusion's buffers at S rows: encoder2's input rows and their gradient, encoder2's output, the seed table the
// forward launches ask for (read, never used at p = 0) and the training tail's own (tmpW / tmpb are not carved: no weight
// gradient is formed).
struct MmIgTailWs {
  XFusionTrainWs x;
  float *x2, *dx2, *MM;
  uint32_t* row_base;
};
static MmIgTailWs carve_mm_ig_tail(Carver& c, int m, int dim, int mmhid1, int mmhid2, int S) {
  MmIgTailWs t{};
  const size_t gate = (size_t)S * m * 16, K2 = (size_t)mmhid1 + (size_t)m * dim;
  t.x2 = c.take<float>(S * K2); t.dx2 = c.take<float>(S * K2);
  t.MM = c.take<float>((size_t)S * mmhid2); t.x.dMM = c.take<float>((size_t)S * mmhid2);
  t.x.o = c.take<float>(gate); t.x.h = c.take<float>(gate); t.x.z = c.take<float>(gate); t.x.gm = c.take<float>(gate);
  t.x.bits = c.take<uint32_t>((size_t)S * xfusion_bit_words(m));
  t.x.dkr = c.take<float>((size_t)S * xfusion_elems(m));
  t.x.dpo = c.take<float>(gate); t.x.dz = c.take<float>(gate); t.x.dph = c.take<float>(gate);
  t.x.dpre = c.take<float>((size_t)S * mmhid2);
  t.row_base = c.take<uint32_t>((size_t)S);
  t.x.bytes = c.off;
  return t;
}
// what the tensor fusion adds to the shape rules, for a window of S nodes: the tail's own, one embedding per modality,
// each xf->dim wide, and the node kernel's bound on nhid
static int mm_ig_tail_shape(const mmf_xfusion_weights* xf, int S, const int* width, int nb) {
  if (int e = xfusion_train_shape(xf, S)) return e;
  if (xf->m != nb) return MMF_ERR_SHAPE;
  for (int i = 0; i < nb; ++i)
    if (width[i] != xf->dim) return MMF_ERR_SHAPE;
  return xf->nhid > 1024 ? MMF_ERR_SHAPE : MMF_OK;
}
// The tail of a window between the branches' forward and backward halves, seven launches: the gating stage, the Kronecker
// product fused into encoder1 and encoder2 (the training forward's launches at p = 0), the node kernel (classifier[0], the
// hazard head, the backward of risk, classifier[0]'s input gradient), encoder2's input gradient (the dense backward's dx
// blocks), dkr and the gating stage's backward.  dx2's embedding columns then hold d risk / d v_i of every node.
static int mm_ig_tail(const mmf_xfusion_weights* xf, const MmIgTailWs& t, const IgHeadParams& hp, int S, hipStream_t st) {
  if (int e = xfusion_group_fwd_launches(xf, t.x2, S, 0.f, t.row_base, nullptr, t.x, t.MM, st)) return e;
  XIgHeadParams xp{};
  xp.hp = hp; xp.MM = t.MM; xp.Wc0 = xf->Wc0; xp.bc0 = xf->bc0; xp.dMM = t.x.dMM; xp.N2 = xf->mmhid2;
  if (int e = launch_xfusion_ig_head(xp, S, st)) return e;
  const int K2 = xf->mmhid1 + xf->m * xf->dim;
  DenseBwdParams e2{t.x.dMM, t.MM, t.x2, xf->We2, t.x.dpre, t.dx2, nullptr, nullptr,
                    S, K2, xf->mmhid2, ACT_RELU, make_drop(1, 0.f, 0, 10, nullptr), nullptr, xf->mmhid2, xf->mmhid2};
  if (int e = launch_dense_bwd(e2, st)) return e;
  return launch_xfusion_group_bwd_dx(xfusion_bwd_params(xf, t.x2, t.dx2, S, 0.f, 0, t.x, nullptr), st);
}

// Both fusions' call.  xf null: the concat head -- the embeddings side by side in feat [S x F], one head launch over them.
// xf given: the tensor fusion -- the embeddings in their columns of encoder2's input rows x2 [S x K2], mm_ig_tail between
// the halves.  Everything else is the same code.
static int mm_ig_call(const mmf_mm_ig_desc* mm, const mmf_xfusion_weights* xf, bool tensor, void* workspace,
                      size_t workspace_bytes, const mmf_surv_head* head, void* stream) {
  // MMF_ERR_ARG
  if (!mm || !head || !head->Wk || !head->bk) return MMF_ERR_ARG;
  if (mm->n_steps < 1 || mm->n_steps > GROUP_MAX || mm->window_steps < 0 || !mm->alpha || !mm->weight) return MMF_ERR_ARG;
  if (!mm->risk_x || !mm->risk_base || !mm->step_risk) return MMF_ERR_ARG;
  const mmf_amil_desc *dp = mm->path, *dr = mm->radio;
  const mmf_radio_reduce* rd = mm->rd;
  const bool omic = mm->omic_x != nullptr;
  if ((dp != nullptr) + (dr != nullptr) + (omic ? 1 : 0) < 2) return MMF_ERR_ARG;
  int radio_shape = MMF_OK;                          // nseg outside 2..4: refused behind every null pointer
  if (dp) {
    if (!mm->path_x) return MMF_ERR_ARG;
    if (int e = mm_ig_stack_args(dp, mm->path_row_sum, mm->path_row_abs)) return e;
  }
  if (dr) {
    if (int e = mm_ig_stack_args(dr, mm->radio_row_sum, mm->radio_row_abs)) return e;
    radio_shape = radio_ig_args(rd);
    if (radio_shape == MMF_ERR_ARG) return radio_shape;
  }
  if (omic && (!mm->omic_W0 || !mm->omic_b0 || !mm->omic_W1 || !mm->omic_b1 || !mm->omic_attr)) return MMF_ERR_ARG;
  if (dp)
    if (int e = check_desc(dp); e == MMF_ERR_ARG) return e;
  if (dr)
    if (int e = check_desc(dr); e == MMF_ERR_ARG) return e;
  if (tensor) {
    if (!xf) return MMF_ERR_ARG;
    if (int e = xfusion_weights_args(xf)) return e;
  }
  // MMF_ERR_SHAPE
  if (radio_shape) return radio_shape;
  int col[3], width[3], nb = 0;
  if (dp) {
    if (int e = check_desc(dp)) return e;
    col[nb] = mm->path_col; width[nb++] = dp->H;
  }
  if (dr) {
    if (int e = check_desc(dr)) return e;
    if (rd->kseg != dr->L) return MMF_ERR_SHAPE;
    if (dr->N * rd->nseg * (int64_t)rd->kseg * 4 >= (int64_t)1 << 31) return MMF_ERR_SHAPE;
    col[nb] = mm->radio_col; width[nb++] = dr->H;
  }
  if (omic) {
    if (mm->omic_Gin < 1 || mm->omic_W0n < 1 || mm->omic_W0n > 1024 || mm->omic_We < 1) return MMF_ERR_SHAPE;
    col[nb] = mm->omic_col; width[nb++] = mm->omic_We;
  }
  const int steps = mm_ig_steps(dp ? dp->N : 0, dp ? dp->H : 0, dp ? dp->D : 0, dr ? dr->N : 0, dr ? dr->H : 0,
                                dr ? dr->D : 0, mm->n_steps + 2, mm->window_steps);
  int64_t F64 = 0;
  for (int i = 0; i < nb; ++i) F64 += width[i];
  if (steps < 1) return MMF_ERR_SHAPE;
  if (tensor) {
    if (int e = mm_ig_tail_shape(xf, steps, width, nb)) return e;        // bounds F: every width is xf->dim, K2 <= 1536
  } else if (F64 > 1024) return MMF_ERR_SHAPE;
  const int F = (int)F64;                            // the embeddings' columns: the fused row, or m dim of x2's K2
  if (!mm_ig_columns(col, width, nb, F)) return MMF_ERR_SHAPE;
  if (head->K < 1 || head->K > 32) return MMF_ERR_SHAPE;
  // MMF_ERR_ALIGN
  if (!workspace) return MMF_ERR_ARG;
  if (dp) {
    if (int e = check_operands(dp, mm->path_x, workspace, mm->path_row_sum, false)) return e;
    if (mm->path_attr && !aligned16(mm->path_attr)) return MMF_ERR_ALIGN;
  }
  if (dr) {
    if (int e = radio_operands(dr, rd, false)) return e;
    if (int e = check_operands(dr, rd->x[0], workspace, mm->radio_row_sum, false)) return e;
    if (mm->radio_attr && !aligned16(mm->radio_attr)) return MMF_ERR_ALIGN;
  }
  if (!aligned16(workspace)) return MMF_ERR_ALIGN;
  if (tensor)
    if (int e = xfusion_weights_aligned(xf)) return e;
  Carver c(workspace);
  const MmIgWs w = carve_mm_ig(c, dp ? dp->N : 0, dp ? dp->L : 0, dp ? dp->H : 0, dp ? dp->D : 0, dp ? dp->gated : 0,
                               dr ? dr->N : 0, dr ? rd->nseg : 0, dr ? rd->kseg : 0, dr ? dr->H : 0, dr ? dr->D : 0,
                               dr ? dr->gated : 0, omic ? mm->omic_Gin : 0, mm->omic_W0n, mm->omic_We, tensor ? 0 : F, steps);
  MmIgTailWs t{};
  if (tensor) t = carve_mm_ig_tail(c, xf->m, xf->dim, xf->mmhid1, xf->mmhid2, steps);
  if (c.off > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(dp && dp->trace ? dp->trace : dr ? dr->trace : nullptr);   // either stack's descriptor may carry it
  // where the embeddings of a window stand, and their gradient: S rows, `ld` floats apart
  float* emb = tensor ? t.x2 + xf->mmhid1 : w.feat;
  const float* demb = tensor ? t.dx2 + xf->mmhid1 : w.dfeat;
  const int ld = tensor ? xf->mmhid1 + F : F;

  // 1. once per call
  mmf_amil_desc db{};                                // the radiology stack behind reduce_dim
  IgOmicParams op{};
  if (dp)
    if (int e = ig_project(dp, mm->path_x, w.gp, st)) return e;
  if (dr)
    if (int e = radio_ig_project(dr, rd, w.gr, db, st)) return e;
  if (omic) {
    op.x = mm->omic_x; op.W0 = mm->omic_W0; op.b0 = mm->omic_b0; op.W1 = mm->omic_W1; op.b1 = mm->omic_b1;
    op.Gin = mm->omic_Gin; op.W0n = mm->omic_W0n; op.We = mm->omic_We;
    op.Z = w.Z; op.z1 = w.z1; op.z2 = w.z2; op.dz1 = w.dz1; op.Gz = w.Gz;
    op.feat = emb; op.dfeat = demb; op.F = ld; op.col = mm->omic_col; op.attr = mm->omic_attr;
    if (int e = launch_ig_omic(IG_OMIC_Z, op, st)) return e;
  }
  // 2. the windows
  const IgNodes q = ig_nodes(mm->n_steps, mm->alpha, mm->weight);
  IgHeadParams hp = ig_head_params(head, tensor ? xf->nhid : F, q.n, mm->step_risk, mm->risk_x, mm->risk_base);
  if (!tensor) { hp.M = w.feat; hp.dM = w.dfeat; }
  for (int q0 = 0; q0 < q.total; q0 += steps) {
    const int S = q.total - q0 < steps ? q.total - q0 : steps;
    const int nfold = ig_nfold(q, q0, S);
    const bool first = q0 == 0;
    const IgSteps sw = ig_steps(q, q0, S);
    if (dp)
      if (int e = ig_window_fwd(dp, w.gp, sw, emb + mm->path_col, ld, st)) return e;
    if (dr)
      if (int e = ig_window_fwd(&db, w.gr.g, sw, emb + mm->radio_col, ld, st)) return e;
    if (omic) {
      op.st = sw;
      if (int e = launch_ig_omic(IG_OMIC_FWD, op, st)) return e;
    }
    hp.step0 = q0;
    if (tensor) {
      if (int e = mm_ig_tail(xf, t, hp, S, st)) return e;
    } else if (int e = launch_ig_head(hp, S, st)) return e;
    if (dp) {
      if (int e = launch_group_dm_gather(demb + mm->path_col, ld, w.gp.dM, S, dp->H, st)) return e;
      if (int e = ig_window_bwd(dp, w.gp, sw, w.gp.dM, nfold, first, st)) return e;
    }
    if (dr) {
      if (int e = launch_group_dm_gather(demb + mm->radio_col, ld, w.gr.g.dM, S, dr->H, st)) return e;
      if (int e = ig_window_bwd(&db, w.gr.g, sw, w.gr.g.dM, nfold, first, st)) return e;
    }
    if (omic) {
      if (int e = launch_ig_omic(IG_OMIC_BWD, op, st)) return e;
      op.st.S = nfold; op.first = first ? 1 : 0;
      if (int e = launch_ig_omic(IG_OMIC_FOLD, op, st)) return e;
    }
  }
  // 3. once per call
  if (dp)
    if (int e = ig_attr(dp, mm->path_x, w.gp, mm->path_row_sum, mm->path_row_abs, mm->path_attr, st)) return e;
  if (dr)
    if (int e = radio_ig_attr(dr, rd, w.gr, mm->radio_row_sum, mm->radio_row_abs, mm->radio_attr, st)) return e;
  if (omic)
    if (int e = launch_ig_omic(IG_OMIC_ATTR, op, st)) return e;
  return MMF_OK;
}
}  // namespace mmf

int mmf_mm_ig(const mmf_mm_ig_desc* mm, void* workspace, size_t workspace_bytes, const mmf_surv_head* head, void* stream) {
  return mm_ig_call(mm, nullptr, false, workspace, workspace_bytes, head, stream);
}

size_t mmf_mm_ig_tensor_workspace_bytes(int64_t N_p, int32_t L_p, int32_t H_p, int32_t D_p, int32_t gated_p, int64_t N_r,
                                        int32_t nseg, int32_t kseg, int32_t H_r, int32_t D_r, int32_t gated_r, int32_t Gin,
                                        int32_t W0, int32_t We, int32_t n_steps, int32_t window_steps, int32_t dim,
                                        int32_t sdim, int32_t mmhid1, int32_t mmhid2, int32_t nhid) {
  if (n_steps < 1 || n_steps > GROUP_MAX || window_steps < 0 || N_p < 0 || N_r < 0 || Gin < 0) return 0;
  mmf_xfusion_weights xf{};
  xf.m = (N_p > 0) + (N_r > 0) + (Gin > 0); xf.dim = dim; xf.sdim = sdim; xf.mmhid1 = mmhid1; xf.mmhid2 = mmhid2;
  xf.nhid = nhid;
  if (xf.m < 2) return 0;
  int width[3], nb = 0;
  if (N_p > 0) {
    if (!mmf_amil_ig_workspace_bytes(N_p, L_p, H_p, D_p, gated_p, n_steps, window_steps)) return 0;
    width[nb++] = H_p;
  }
  if (N_r > 0) {
    if (!mmf_radio_ig_workspace_bytes(N_r, nseg, kseg, H_r, D_r, gated_r, n_steps, window_steps)) return 0;
    width[nb++] = H_r;
  }
  if (Gin > 0) {
    if (W0 < 1 || W0 > 1024 || We < 1) return 0;
    width[nb++] = We;
  }
  const int steps = mm_ig_steps(N_p, H_p, D_p, N_r, H_r, D_r, n_steps + 2, window_steps);
  if (steps < 1 || mm_ig_tail_shape(&xf, steps, width, nb)) return 0;
  Carver c;
  carve_mm_ig(c, N_p, L_p, H_p, D_p, gated_p, N_r, nseg, kseg, H_r, D_r, gated_r, Gin, W0, We, 0, steps);
  carve_mm_ig_tail(c, xf.m, dim, mmhid1, mmhid2, steps);
  return c.off;
}

int mmf_mm_ig_tensor(const mmf_mm_ig_desc* mm, const mmf_xfusion_weights* xf, void* workspace, size_t workspace_bytes,
                     const mmf_surv_head* head, void* stream) {
  return mm_ig_call(mm, xf, true, workspace, workspace_bytes, head, stream);
}

// ---- integrated gradients of the stage-2 fusion models --------------------------------------------------------------
namespace mmf {
constexpr int S2_PMAX = 1 << 20;
constexpr int S2_HW_LAYERS = 8;     // a Highway's depth: the window keeps every layer's pre-activations
static bool s2_highway(int tt) { return tt == MMF_STAGE2_EARLY_HIGHWAY || tt == MMF_STAGE2_LATE_HIGHWAY; }
static bool s2_late(int tt) { return tt == MMF_STAGE2_LATE_FCNN || tt == MMF_STAGE2_LATE_HIGHWAY; }
// U's and G's row: the units behind the first layer (one plane per fcnn block, three per Highway)
static int s2_ldu(int tt, int m) {
  return tt == MMF_STAGE2_EARLY_FCNN ? 128 : tt == MMF_STAGE2_LATE_FCNN ? 128 * m : 3 * 256 * m;
}
// what the call and the query refuse by shape
static int s2_shape(int family, int tt, int m, int n_layers, int P, int K, int n_steps) {
  if (m < 2 || m > 3 || P < 1 || P > S2_PMAX || n_steps < 1 || n_steps > GROUP_MAX || n_layers < 1) return MMF_ERR_SHAPE;
  if (K < 1 || K > 32 || (family == MMF_STAGE2_COX && K != 1)) return MMF_ERR_SHAPE;
  if (s2_highway(tt) && n_layers > S2_HW_LAYERS) return MMF_ERR_SHAPE;
  return MMF_OK;
}
// highway with n_layers >= 2: the windows hold up to S2_HW_ROWS of the call's P (n_steps + 2) rows
static int s2_hw_rows(int P, int n_steps) {
  const int64_t R = (int64_t)P * (n_steps + 2);
  return R < S2_HW_ROWS ? (int)R : S2_HW_ROWS;
}
// kronecker: the windows hold up to GROUP_MAX of the call's P (n_steps + 2) rows
static int s2_kron_rows(int P, int n_steps) {
  const int64_t R = (int64_t)P * (n_steps + 2);
  return R < GROUP_MAX ? (int)R : GROUP_MAX;
}
// the stage-2 models' XlinearFusion: its widths are the class's (models/nll_models_pretrained.py:124)
static void s2_kron_tail(mmf_xfusion_weights& x, int m) {
  x.m = m; x.dim = 256; x.sdim = 16; x.mmhid1 = 256; x.mmhid2 = 256; x.nhid = 256;
}
static bool s2_bn_ok(const mmf_bn1d& b) { return b.weight && b.bias && b.mean && b.var; }
static S2Bn s2_bn(const mmf_bn1d& b, int off) { return S2Bn{b.weight + off, b.bias + off, b.mean + off, b.var + off, b.eps}; }
// deep Highways: per window the layers' outputs X[l], the pre-activations Z[l][gate, nonlinear, linear] of layers >= 1,
// the running gradient dX, a layer's dZ and its three input gradients, each [rows x 256 m] block by block
struct S2Ws { float *U, *G; MmIgTailWs t; float *X[S2_HW_LAYERS], *Z[S2_HW_LAYERS][3], *dX, *dZ[3], *dx3[3], *dpre; };
static S2Ws carve_s2(Carver& c, int tt, int m, int P, int n_steps, int n_layers) {
  S2Ws w{};
  if (tt == MMF_STAGE2_KRONECKER) {
    w.G = c.take<float>((size_t)P * m * 256);
    w.t = carve_mm_ig_tail(c, m, 256, 256, 256, s2_kron_rows(P, n_steps));
    return w;
  }
  const size_t ld = (size_t)s2_ldu(tt, m);
  w.U = c.take<float>(((size_t)P + 1) * ld);
  w.G = c.take<float>((size_t)P * ld);
  if (s2_highway(tt) && n_layers > 1) {
    const size_t n = (size_t)s2_hw_rows(P, n_steps) * 256 * m;
    for (int l = 0; l < n_layers; ++l) {
      w.X[l] = c.take<float>(n);
      if (l > 0)
        for (int g = 0; g < 3; ++g) w.Z[l][g] = c.take<float>(n);
    }
    w.dX = c.take<float>(n); w.dpre = c.take<float>(n);
    for (int g = 0; g < 3; ++g) { w.dZ[g] = c.take<float>(n); w.dx3[g] = c.take<float>(n); }
  }
  return w;
}
// highway with n_layers >= 2, between the folded forward and the attribution launch: layer 0 from U per row, layers >= 1
// per window through the dense row kernels (the input gradient alone) and the highway mix, the head, and the fold of layer
// 0's gradient into G in node order
static int s2_hw_chain(const mmf_stage2_ig_desc* d, int m, bool late, const S2Ws& w, const IgNodes& q, hipStream_t st) {
  const int L = d->n_layers, W = 256 * m, nblk = late ? m : 1, wd = W / nblk;
  const int cap = s2_hw_rows(d->P, d->n_steps);
  const size_t stride = (size_t)cap * wd;
  S2HwParams hp{};
  hp.U = w.U; hp.ldU = 3 * W; hp.W = W; hp.wd = wd; hp.P = d->P; hp.n_steps = d->n_steps; hp.T = q.total; hp.K = d->K;
  hp.cox = d->family == MMF_STAGE2_COX; hp.blk_stride = stride;
  for (int k = 0; k < q.total; ++k) { hp.alpha[k] = q.alpha[k]; hp.weight[k] = q.weight[k]; }
  hp.X0 = w.X[0]; hp.XL = w.X[L - 1]; hp.dXL = w.dX; hp.dX0 = w.dX; hp.G = w.G;
  for (int b = 0; b < nblk; ++b) hp.bn2[b] = s2_bn(d->blk[b].bn2, 0);
  hp.Wk = d->Wk; hp.bk = d->bk; hp.step_risk = d->step_risk; hp.risk = d->risk; hp.risk_base = d->risk_base;
  hp.hazards = hp.cox ? nullptr : d->hazards; hp.S_out = hp.cox ? nullptr : d->S;
  const DropSpec none = make_drop(0, 0.f, 0, 0, nullptr);
  const int64_t R = (int64_t)d->P * q.total;
  for (int64_t g0 = 0; g0 < R; g0 += cap) {
    const int S = R - g0 < cap ? (int)(R - g0) : cap;
    hp.g0 = (int)g0; hp.S = S;
    if (int e = launch_stage2_hw(S2_HW_BEGIN, hp, st)) return e;
    for (int l = 1; l < L; ++l)
      for (int b = 0; b < nblk; ++b) {
        const mmf_stage2_block& k = d->blk[b];
        const float* Wl[3] = {k.Wgate[l], k.Wnl[l], k.Wlin[l]};
        const float* bl[3] = {k.bgate[l], k.bnl[l], k.blin[l]};
        const size_t o = b * stride;
        for (int g = 0; g < 3; ++g) {
          DenseParams dp{w.X[l - 1] + o, Wl[g], bl[g], w.Z[l][g] + o, S, wd, wd, ACT_NONE, none, nullptr, wd};
          if (int e = launch_dense_fwd(dp, st)) return e;
        }
        HighwayParams mix{w.Z[l][0] + o, w.Z[l][1] + o, w.Z[l][2] + o, w.X[l] + o, nullptr, nullptr, nullptr, nullptr,
                          (int64_t)S * wd};
        if (int e = launch_highway_fwd(mix, st)) return e;
      }
    if (int e = launch_stage2_hw(S2_HW_HEAD, hp, st)) return e;
    for (int l = L - 1; l >= 1; --l)
      for (int b = 0; b < nblk; ++b) {
        const mmf_stage2_block& k = d->blk[b];
        const float* Wl[3] = {k.Wgate[l], k.Wnl[l], k.Wlin[l]};
        const size_t o = b * stride;
        HighwayParams mix{w.Z[l][0] + o, w.Z[l][1] + o, w.Z[l][2] + o, nullptr, w.dX + o, w.dZ[0] + o, w.dZ[1] + o,
                          w.dZ[2] + o, (int64_t)S * wd};
        if (int e = launch_highway_bwd(mix, st)) return e;
        for (int g = 0; g < 3; ++g) {     // the input gradient alone: no dW, no db
          DenseBwdParams bp{w.dZ[g] + o, w.Z[l][g] + o, w.X[l - 1] + o, Wl[g], w.dpre, w.dx3[g] + o, nullptr, nullptr,
                            S, wd, wd, ACT_NONE, none, nullptr, wd, wd};
          if (int e = launch_dense_bwd(bp, st)) return e;
        }
        if (int e = launch_stage2_hw_add3(w.dx3[0] + o, w.dx3[1] + o, w.dx3[2] + o, w.dX + o, S * wd, st)) return e;
      }
    if (int e = launch_stage2_hw(S2_HW_END, hp, st)) return e;
  }
  return MMF_OK;
}
// kronecker: nothing folds.  The call's P (n_steps + 2) rows (patient-major, a patient's nodes then its two riders) pass in
// windows of up to GROUP_MAX rows, which may straddle patients, through mmf_mm_ig_tensor's seven tail launches -- the
// gating stage, the product fused into encoder1, encoder2; the head launch (here without classifier[0]); encoder2's input
// gradient, dkr, the gating stage's backward -- between an expansion and a fold; one attribution launch ends the call.
static int s2_kron_chain(const mmf_stage2_ig_desc* d, const mmf_xfusion_weights& xf, int m, const S2Ws& w, const IgNodes& q,
                         hipStream_t st) {
  const int K2 = xf.mmhid1 + m * xf.dim;
  S2KronParams kp{};
  for (int i = 0; i < m; ++i) { kp.v[i] = d->v[i]; kp.attr[i] = d->attr[i]; }
  kp.m = m; kp.P = d->P; kp.n_steps = d->n_steps; kp.T = q.total; kp.N1 = xf.mmhid1; kp.K2 = K2; kp.K = d->K;
  kp.cox = d->family == MMF_STAGE2_COX;
  for (int k = 0; k < q.total; ++k) { kp.alpha[k] = q.alpha[k]; kp.weight[k] = q.weight[k]; }
  kp.x2 = w.t.x2; kp.MM = w.t.MM; kp.dx2 = w.t.dx2; kp.dMM = w.t.x.dMM; kp.Gacc = w.G;
  kp.Wk = d->Wk; kp.bk = d->bk; kp.step_risk = d->step_risk; kp.risk = d->risk; kp.risk_base = d->risk_base;
  kp.hazards = kp.cox ? nullptr : d->hazards; kp.S_out = kp.cox ? nullptr : d->S;
  kp.mod_sum = d->mod_sum; kp.mod_abs = d->mod_abs;
  const int64_t R = (int64_t)d->P * q.total;
  const int rows = s2_kron_rows(d->P, d->n_steps);
  for (int64_t g0 = 0; g0 < R; g0 += rows) {
    const int S = R - g0 < rows ? (int)(R - g0) : rows;
    kp.g0 = (int)g0; kp.S = S;
    if (int e = launch_stage2_kron(S2_KRON_EXPAND, kp, st)) return e;
    if (int e = xfusion_group_fwd_launches(&xf, w.t.x2, S, 0.f, w.t.row_base, nullptr, w.t.x, w.t.MM, st)) return e;
    if (int e = launch_stage2_kron(S2_KRON_HEAD, kp, st)) return e;
    DenseBwdParams e2{w.t.x.dMM, w.t.MM, w.t.x2, xf.We2, w.t.x.dpre, w.t.dx2, nullptr, nullptr,
                      S, K2, xf.mmhid2, ACT_RELU, make_drop(1, 0.f, 0, 10, nullptr), nullptr, xf.mmhid2, xf.mmhid2};
    if (int e = launch_dense_bwd(e2, st)) return e;
    if (int e = launch_xfusion_group_bwd_dx(xfusion_bwd_params(&xf, w.t.x2, w.t.dx2, S, 0.f, 0, w.t.x, nullptr), st)) return e;
    if (int e = launch_stage2_kron(S2_KRON_FOLD, kp, st)) return e;
  }
  kp.g0 = 0; kp.S = 1;
  return launch_stage2_kron(S2_KRON_ATTR, kp, st);
}
}  // namespace mmf

size_t mmf_stage2_ig_workspace_bytes(int32_t family, int32_t train_type, int32_t m, int32_t n_layers, int32_t P, int32_t K,
                                     int32_t n_steps) {
  if (family < MMF_STAGE2_NLL || family > MMF_STAGE2_COX || train_type < 0 || train_type > MMF_STAGE2_KRONECKER) return 0;
  if (s2_shape(family, train_type, m, n_layers, P, K, n_steps)) return 0;
  Carver c;
  carve_s2(c, train_type, m, P, n_steps, n_layers);
  return c.off;
}

int mmf_stage2_ig(const mmf_stage2_ig_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
  // MMF_ERR_ARG
  if (!d || !d->alpha || !d->weight || !d->Wk || !d->bk) return MMF_ERR_ARG;
  if (!d->mod_sum || !d->mod_abs || !d->risk || !d->risk_base || !d->step_risk) return MMF_ERR_ARG;
  if (d->family < MMF_STAGE2_NLL || d->family > MMF_STAGE2_COX || d->train_type < 0 || d->train_type > MMF_STAGE2_KRONECKER)
    return MMF_ERR_ARG;
  const int tt = d->train_type, m = (d->radio != 0) + (d->path != 0) + (d->omic != 0);
  const bool hw = s2_highway(tt), late = s2_late(tt), cox = d->family == MMF_STAGE2_COX;
  const int nblk = late ? m : 1;
  for (int i = 0; i < m; ++i)
    if (!d->v[i]) return MMF_ERR_ARG;
  if (tt == MMF_STAGE2_KRONECKER) {
    const mmf_xfusion_weights* x = d->xf;
    if (!x || !x->We1 || !x->be1 || !x->We2 || !x->be2) return MMF_ERR_ARG;
    for (int i = 0; i < m; ++i)
      if (!x->Wh[i] || !x->bh[i] || !x->Wz[i] || !x->bz[i] || !x->Wo[i] || !x->bo[i]) return MMF_ERR_ARG;
  } else {
    for (int i = 0; i < nblk; ++i) {
      const mmf_stage2_block& b = d->blk[i];
      if (hw) {
        if (!s2_bn_ok(b.bn1) || !s2_bn_ok(b.bn2)) return MMF_ERR_ARG;
        if (!b.Wgate || !b.bgate || !b.Wnl || !b.bnl || !b.Wlin || !b.blin) return MMF_ERR_ARG;
        for (int l = 0; l < d->n_layers; ++l)
          if (!b.Wgate[l] || !b.bgate[l] || !b.Wnl[l] || !b.bnl[l] || !b.Wlin[l] || !b.blin[l]) return MMF_ERR_ARG;
      } else {
        if (!b.W0 || !b.b0 || !s2_bn_ok(b.bn)) return MMF_ERR_ARG;
        if (cox && late && (!b.W4 || !b.b4)) return MMF_ERR_ARG;
      }
    }
  }
  // MMF_ERR_SHAPE
  if (int e = s2_shape(d->family, tt, m, d->n_layers, d->P, d->K, d->n_steps)) return e;
  mmf_xfusion_weights xf{};
  if (tt == MMF_STAGE2_KRONECKER) {
    xf = *d->xf;
    if (xf.m != m || xf.dim != 256 || xf.sdim != 16 || xf.mmhid1 != 256 || xf.mmhid2 != 256) return MMF_ERR_SHAPE;
    s2_kron_tail(xf, m);                            // nhid is not read: the classifier stands on encoder2's output
    if (int e = xfusion_train_shape(&xf, s2_kron_rows(d->P, d->n_steps))) return e;
  }
  // MMF_ERR_ALIGN
  if (!workspace) return MMF_ERR_ARG;
  for (int i = 0; i < m; ++i)
    if (!aligned16(d->v[i]) || (d->attr[i] && !aligned16(d->attr[i]))) return MMF_ERR_ALIGN;
  if (!aligned16(workspace)) return MMF_ERR_ALIGN;
  if (tt == MMF_STAGE2_KRONECKER)
    if (int e = xfusion_weights_aligned(&xf)) return e;
  Carver c(workspace);
  const S2Ws w = carve_s2(c, tt, m, d->P, d->n_steps, d->n_layers);
  if (c.off > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  const IgNodes q = ig_nodes(d->n_steps, d->alpha, d->weight);
  if (tt == MMF_STAGE2_KRONECKER) return s2_kron_chain(d, xf, m, w, q, st);

  // the first-layer matrices: which columns of the packed row each reads, which columns of U it owns
  const int ldU = s2_ldu(tt, m), W = hw ? 256 * m : ldU, kin = late ? 256 : 256 * m, nout = hw ? kin : 128;
  S2FoldParams fp{};
  fp.m = m; fp.P = d->P; fp.ldU = ldU; fp.U = w.U; fp.G = w.G; fp.mod_sum = d->mod_sum; fp.mod_abs = d->mod_abs;
  for (int i = 0; i < m; ++i) {
    fp.v[i] = d->v[i]; fp.attr[i] = d->attr[i];
    if (hw) fp.in_bn[i] = late ? s2_bn(d->blk[i].bn1, 0) : s2_bn(d->blk[0].bn1, 256 * i);
  }
  for (int i = 0; i < nblk; ++i) {
    const mmf_stage2_block& b = d->blk[i];
    if (hw) {
      const float* Wg[3] = {b.Wgate[0], b.Wnl[0], b.Wlin[0]};
      const float* bg[3] = {b.bgate[0], b.bnl[0], b.blin[0]};
      for (int g = 0; g < 3; ++g) fp.prob[fp.nprob++] = S2Lin{Wg[g], bg[g], nout, kin, kin * i, g * W + nout * i};
    } else {
      fp.prob[fp.nprob++] = S2Lin{b.W0, b.b0, nout, kin, kin * i, nout * i};
    }
  }
  S2SweepParams sp{};
  sp.U = w.U; sp.G = w.G; sp.ldU = ldU; sp.W = W; sp.P = d->P; sp.K = d->K; sp.n_steps = d->n_steps;
  sp.highway = hw; sp.cox = cox; sp.late_cox = cox && tt == MMF_STAGE2_LATE_FCNN; sp.bn_span = nout;
  for (int i = 0; i < nblk; ++i) {
    sp.bn[i] = s2_bn(hw ? d->blk[i].bn2 : d->blk[i].bn, 0);
    sp.W4[i] = d->blk[i].W4; sp.b4[i] = d->blk[i].b4;
  }
  sp.Wk = d->Wk; sp.bk = d->bk;
  for (int k = 0; k < q.total; ++k) { sp.alpha[k] = q.alpha[k]; sp.weight[k] = q.weight[k]; }
  sp.step_risk = d->step_risk; sp.risk = d->risk; sp.risk_base = d->risk_base;
  sp.hazards = cox ? nullptr : d->hazards; sp.S = cox ? nullptr : d->S;
  if (int e = launch_stage2_fold_fwd(fp, st)) return e;
  if (hw && d->n_layers > 1) {
    if (int e = s2_hw_chain(d, m, late, w, q, st)) return e;
  } else if (int e = launch_stage2_sweep(sp, st)) return e;
  return launch_stage2_attr(fp, st);
}

// ---- one-call training step of the stage-2 fcnn and highway models ------------------------------------------------------------
namespace mmf {
static int s2s_shape(int family, int tt, int m, int n_layers, int B, int K, int training) {
  if (m < 2 || m > 3 || B < 1 || B > 256 || (training && B < 2) || K < 1 || K > 32 || (family == MMF_STAGE2_COX && K != 1))
    return MMF_ERR_SHAPE;
  if (s2_highway(tt) && (n_layers < 1 || n_layers > 8)) return MMF_ERR_SHAPE;
  return MMF_OK;
}
struct S2sWs {
  int ldB;
  float *uT[3], *stat[3], *yT, *sblk;                          // fcnn
  float *xT[3][9], *xR[3][8], *zT[3][8][3], *dzT[3][2][3], *stat1[3], *stat2[3], *fT;   // highway
};
static S2sWs carve_s2s(Carver& c, int tt, int m, int n_layers, int B) {
  S2sWs w{};
  const bool hw = s2_highway(tt), late = s2_late(tt);
  const int nb = late ? 3 : 1;
  const size_t ldB = (size_t)((B + 3) / 4 * 4);
  w.ldB = (int)ldB;
  if (!hw) {
    for (int i = 0; i < nb; ++i) w.uT[i] = c.take<float>(128 * ldB);
    w.yT = c.take<float>((size_t)128 * (late ? m : 1) * ldB);
    for (int i = 0; i < nb; ++i) w.stat[i] = c.take<float>(256);
    w.sblk = c.take<float>((size_t)3 * B);
    return w;
  }
  const size_t D = late ? 256 : 256 * (size_t)m;
  for (int i = 0; i < nb; ++i) {
    for (int l = 0; l <= n_layers; ++l) w.xT[i][l] = c.take<float>(D * ldB);
    for (int l = 0; l < n_layers; ++l) w.xR[i][l] = c.take<float>((size_t)B * D);
    for (int l = 0; l < n_layers; ++l)
      for (int q = 0; q < 3; ++q) w.zT[i][l][q] = c.take<float>(D * ldB);
    for (int s = 0; s < 2; ++s)
      for (int q = 0; q < 3; ++q) w.dzT[i][s][q] = c.take<float>(D * ldB);
    w.stat1[i] = c.take<float>(2 * D);
    w.stat2[i] = c.take<float>(2 * D);
  }
  w.fT = c.take<float>((size_t)256 * m * ldB);
  return w;
}
static bool s2s_bn_ok(const mmf_stage2_bn_train& b) { return b.weight && b.bias && b.running_mean && b.running_var; }
static S2sBn s2s_bn(const mmf_stage2_bn_train& b) {
  return S2sBn{b.weight, b.bias, b.running_mean, b.running_var, b.eps, b.momentum};
}
}  // namespace mmf

size_t mmf_stage2_step_workspace_bytes(int32_t family, int32_t train_type, int32_t m, int32_t n_layers, int32_t B, int32_t K,
                                       int32_t training) {
  if (family < MMF_STAGE2_NLL || family > MMF_STAGE2_COX || train_type < 0 || train_type > MMF_STAGE2_LATE_HIGHWAY) return 0;
  if (s2s_shape(family, train_type, m, n_layers, B, K, training)) return 0;
  Carver c;
  carve_s2s(c, train_type, m, n_layers, B);
  return c.off;
}

int mmf_stage2_step(const mmf_stage2_step_desc* d, const mmf_stage2_target* t, void* workspace, size_t workspace_bytes,
                    float* risk, float* hazards, float* S, float* loss, const mmf_stage2_step_grads* grads,
                    int32_t accumulate, void* stream) {
  // MMF_ERR_ARG
  if (!d || !t || !d->Wk || !d->bk || !risk || !loss || !t->c) return MMF_ERR_ARG;
  if (d->family < MMF_STAGE2_NLL || d->family > MMF_STAGE2_COX || d->train_type < 0 || d->train_type > MMF_STAGE2_KRONECKER)
    return MMF_ERR_ARG;
  if (t->loss < MMF_STAGE2_LOSS_NLL || t->loss > MMF_STAGE2_LOSS_RANK_NLL || t->phi < 0 || t->phi > 1 || t->reduction < 0 ||
      t->reduction > 1)
    return MMF_ERR_ARG;
  if (d->train_type == MMF_STAGE2_KRONECKER) return MMF_ERR_ARG;
  const int tt = d->train_type, L = d->n_layers;
  const bool hw = s2_highway(tt), late = s2_late(tt), cox = d->family == MMF_STAGE2_COX;
  const bool has_nll = t->loss == MMF_STAGE2_LOSS_NLL || t->loss == MMF_STAGE2_LOSS_RANK_NLL;
  if (cox && has_nll) return MMF_ERR_ARG;
  if (!(d->p_drop >= 0.f && d->p_drop < 1.f)) return MMF_ERR_ARG;
  const bool present[3] = {d->radio != 0, d->path != 0, d->omic != 0};
  const int m = present[0] + present[1] + present[2];
  // the cat order: [radio, path] | [radio, omic] | [omic, path] | [radio, path, omic]
  int ord[3] = {0, 1, 2}, slot[3] = {-1, -1, -1};
  if (m == 2) {
    if (!present[2]) { ord[0] = 0; ord[1] = 1; }
    else if (!present[1]) { ord[0] = 0; ord[1] = 2; }
    else { ord[0] = 2; ord[1] = 1; }
  }
  for (int i = 0; i < m && m >= 2; ++i) slot[ord[i]] = i;
  const int nb = late ? 3 : 1;
  for (int i = 0; i < 3; ++i)
    if ((late || present[i]) && !d->h[i]) return MMF_ERR_ARG;
  const int Lc = L < 0 ? 0 : L > 8 ? 8 : L;           // the per-layer entries that exist to be looked at
  for (int i = 0; i < nb; ++i) {
    const mmf_stage2_step_block& b = d->blk[i];
    if (hw) {
      if (!s2s_bn_ok(b.bn1) || !s2s_bn_ok(b.bn2)) return MMF_ERR_ARG;
      if (!b.Wgate || !b.bgate || !b.Wnl || !b.bnl || !b.Wlin || !b.blin) return MMF_ERR_ARG;
      for (int l = 0; l < Lc; ++l)
        if (!b.Wgate[l] || !b.bgate[l] || !b.Wnl[l] || !b.bnl[l] || !b.Wlin[l] || !b.blin[l]) return MMF_ERR_ARG;
    } else {
      if (!b.W0 || !b.b0 || !s2s_bn_ok(b.bn)) return MMF_ERR_ARG;
      if (cox && late && (!b.W4 || !b.b4)) return MMF_ERR_ARG;
    }
  }
  if (!cox && (!hazards || !S)) return MMF_ERR_ARG;
  if (has_nll && !t->Y) return MMF_ERR_ARG;
  if (!has_nll && !t->times) return MMF_ERR_ARG;
  if (grads) {
    if (!grads->dWk || !grads->dbk) return MMF_ERR_ARG;
    for (int i = 0; i < nb; ++i) {
      if (late && slot[i] < 0 && m >= 2) continue;   // the dropped modality's block gets no gradient
      const mmf_stage2_block_grads& g = grads->blk[i];
      if (hw) {
        if (!g.dbn1_weight || !g.dbn1_bias || !g.dbn2_weight || !g.dbn2_bias) return MMF_ERR_ARG;
        if (!g.dWgate || !g.dbgate || !g.dWnl || !g.dbnl || !g.dWlin || !g.dblin) return MMF_ERR_ARG;
        for (int l = 0; l < Lc; ++l)
          if (!g.dWgate[l] || !g.dbgate[l] || !g.dWnl[l] || !g.dbnl[l] || !g.dWlin[l] || !g.dblin[l]) return MMF_ERR_ARG;
      } else {
        if (!g.dW0 || !g.db0 || !g.dbn_weight || !g.dbn_bias) return MMF_ERR_ARG;
        if (cox && late && (!g.dW4 || !g.db4)) return MMF_ERR_ARG;
      }
    }
  }
  // MMF_ERR_SHAPE
  if (int e = s2s_shape(d->family, tt, m, L, d->B, d->K, d->training)) return e;
  const bool has_rank = t->loss == MMF_STAGE2_LOSS_RANK || t->loss == MMF_STAGE2_LOSS_RANK_NLL;
  if (has_rank && d->B < 2) return MMF_ERR_SHAPE;
  // MMF_ERR_ALIGN
  if (!workspace) return MMF_ERR_ARG;
  for (int i = 0; i < 3; ++i)
    if ((late || present[i]) && !aligned16(d->h[i])) return MMF_ERR_ALIGN;
  if (hw)
    for (int i = 0; i < nb; ++i)
      for (int l = 0; l < L; ++l)
        if (!aligned16(d->blk[i].Wgate[l]) || !aligned16(d->blk[i].Wnl[l]) || !aligned16(d->blk[i].Wlin[l])) return MMF_ERR_ALIGN;
  if (!aligned16(workspace)) return MMF_ERR_ALIGN;
  if (t->times && (reinterpret_cast<uintptr_t>(t->times) & 7)) return MMF_ERR_ALIGN;
  Carver c(workspace);
  const S2sWs w = carve_s2s(c, tt, m, L, d->B);
  if (c.off > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);

  const int B = d->B, K = d->K, ldB = w.ldB, training = d->training != 0, acc = accumulate != 0;
  const float p = training ? d->p_drop : 0.f;
  S2sLoss lq{};
  lq.kind = t->loss; lq.phi = t->phi; lq.reduction = t->reduction; lq.K = K; lq.B = B; lq.cox = cox;
  lq.alpha = t->alpha; lq.ratio = t->nll_ratio; lq.scale = t->loss_scale;
  lq.Y = t->Y; lq.c = t->c; lq.times = t->times; lq.risk = risk; lq.hazards = hazards; lq.S = S; lq.loss = loss;
  // the branches the head and the backward see, in their own order; early: the one block over the cat
  int act[3], nact = 0;
  for (int i = 0; i < nb; ++i)
    if (!late || slot[i] >= 0) act[nact++] = i;

  S2sHead hp{};
  hp.B = B; hp.ldB = ldB; hp.K = K; hp.cox = cox; hp.m = m; hp.with_loss = grads ? 0 : 1;
  hp.Wk = d->Wk; hp.bk = d->bk; hp.risk = risk; hp.hazards = hazards; hp.S = S; hp.loss = lq; hp.sblk = w.sblk;

  if (!hw) {
    const int wb = 128;                                        // a block's width in the classifier's input
    S2sFcnnFwd fp{};
    fp.nbr = nb; fp.B = B; fp.ldB = ldB; fp.training = training; fp.p = p; fp.seed_dev = d->seed_dev;
    for (int i = 0; i < nb; ++i) {
      S2sFcnnFwdBr& br = fp.br[i];
      const mmf_stage2_step_block& b = d->blk[i];
      if (late) { br.x[0] = d->h[i]; br.nseg = 1; }
      else { for (int s = 0; s < m; ++s) br.x[s] = d->h[ord[s]]; br.nseg = m; }
      br.W0 = b.W0; br.b0 = b.b0; br.bn = s2s_bn(b.bn); br.key = drop_key(d->seed, (uint32_t)i);
      br.uT = w.uT[i]; br.stat = w.stat[i];
      br.yT = late ? (slot[i] >= 0 ? w.yT + (size_t)slot[i] * wb * ldB : nullptr) : w.yT;
    }
    if (int e = launch_s2s_fcnn_fwd(fp, st)) return e;
    hp.fT = w.yT; hp.W = late ? wb * m : wb; hp.late_cox = cox && late;
    for (int a = 0; a < nact && late; ++a) { hp.W4[slot[act[a]]] = d->blk[act[a]].W4; hp.b4[slot[act[a]]] = d->blk[act[a]].b4; }
    if (int e = launch_s2s_head(hp, st)) return e;
    if (!grads) return MMF_OK;
    S2sFcnnBwd bp{};
    bp.nbr = nact; bp.B = B; bp.ldB = ldB; bp.training = training; bp.accumulate = acc; bp.late_cox = hp.late_cox;
    bp.W = hp.W; bp.p = p; bp.yT = w.yT; bp.Wk = d->Wk; bp.sblk = w.sblk; bp.dWk = grads->dWk; bp.dbk = grads->dbk; bp.loss = lq;
    for (int a = 0; a < nact; ++a) {
      const int i = act[a];
      S2sFcnnBwdBr& br = bp.br[a];
      const mmf_stage2_step_block& b = d->blk[i];
      const mmf_stage2_block_grads& g = grads->blk[i];
      for (int s = 0; s < 3; ++s) br.x[s] = fp.br[i].x[s];
      br.nseg = fp.br[i].nseg; br.slot = late ? slot[i] : 0; br.ycol0 = br.slot * wb;
      br.uT = w.uT[i]; br.stat = w.stat[i]; br.bn = s2s_bn(b.bn); br.W4 = b.W4;
      br.dW0 = g.dW0; br.db0 = g.db0; br.dgamma = g.dbn_weight; br.dbeta = g.dbn_bias; br.dW4 = g.dW4; br.db4 = g.db4;
    }
    return launch_s2s_fcnn_bwd(bp, st);
  }

  const int D = late ? 256 : 256 * m;
  S2sBn1Fwd b1{};
  b1.nbr = nb; b1.D = D; b1.B = B; b1.ldB = ldB; b1.training = training; b1.p = p; b1.seed_dev = d->seed_dev;
  for (int i = 0; i < nb; ++i) {
    S2sBn1FwdBr& br = b1.br[i];
    if (late) br.x[0] = d->h[i];
    else for (int s = 0; s < m; ++s) br.x[s] = d->h[ord[s]];
    br.bn = s2s_bn(d->blk[i].bn1); br.key = drop_key(d->seed + (uint32_t)i, 0u);
    br.xT = w.xT[i][0]; br.xR = w.xR[i][0]; br.stat = w.stat1[i];
  }
  if (int e = launch_s2s_bn1_fwd(b1, st)) return e;
  for (int l = 0; l < L; ++l) {
    S2sHwFwd fp{};
    fp.nbr = nb; fp.D = D; fp.B = B; fp.ldB = ldB; fp.training = training; fp.last = l == L - 1;
    for (int i = 0; i < nb; ++i) {
      S2sHwFwdBr& br = fp.br[i];
      const mmf_stage2_step_block& b = d->blk[i];
      br.xT = w.xT[i][l];
      br.W[0] = b.Wgate[l]; br.W[1] = b.Wnl[l]; br.W[2] = b.Wlin[l];
      br.bias[0] = b.bgate[l]; br.bias[1] = b.bnl[l]; br.bias[2] = b.blin[l];
      for (int q = 0; q < 3; ++q) br.zT[q] = w.zT[i][l][q];
      br.yT = w.xT[i][l + 1]; br.yR = fp.last ? nullptr : w.xR[i][l + 1];
      br.bn2 = s2s_bn(b.bn2); br.stat2 = w.stat2[i];
      br.fT = late ? (slot[i] >= 0 ? w.fT + (size_t)slot[i] * 256 * ldB : nullptr) : w.fT;
    }
    if (int e = launch_s2s_hw_fwd(fp, st)) return e;
  }
  hp.fT = w.fT; hp.W = 256 * m; hp.late_cox = 0;
  if (int e = launch_s2s_head(hp, st)) return e;
  if (!grads) return MMF_OK;
  for (int l = L; l >= 0; --l) {                               // level l: the gradient arrives at x_l
    S2sHwBwd bp{};
    bp.nbr = nact; bp.D = D; bp.B = B; bp.ldB = ldB; bp.training = training; bp.accumulate = acc; bp.W = 256 * m; bp.p = p;
    bp.mode = l == L ? S2S_HW_TOP : l == 0 ? S2S_HW_BN1 : S2S_HW_MID;
    bp.seed_dev = d->seed_dev; bp.Wk = d->Wk; bp.dWk = grads->dWk; bp.dbk = grads->dbk; bp.loss = lq;
    for (int a = 0; a < nact; ++a) {
      const int i = act[a];
      S2sHwBwdBr& br = bp.br[a];
      const mmf_stage2_step_block& b = d->blk[i];
      const mmf_stage2_block_grads& g = grads->blk[i];
      if (l < L) {                                             // from the layer above: layer index l (0-based) reads x_l
        for (int q = 0; q < 3; ++q) br.dzT_in[q] = w.dzT[i][(l + 1) & 1][q];
        br.Wup[0] = b.Wgate[l]; br.Wup[1] = b.Wnl[l]; br.Wup[2] = b.Wlin[l];
      } else {
        br.fcol0 = late ? slot[i] * 256 : 0;
        br.fT = w.fT + (size_t)br.fcol0 * ldB; br.yT = w.xT[i][L]; br.stat2 = w.stat2[i]; br.bn2 = s2s_bn(b.bn2);
        br.dgamma2 = g.dbn2_weight; br.dbeta2 = g.dbn2_bias;
      }
      if (l > 0) {                                             // x_l is the mix of layer index l - 1 over x_{l-1}
        for (int q = 0; q < 3; ++q) { br.zT[q] = w.zT[i][l - 1][q]; br.dzT_out[q] = w.dzT[i][l & 1][q]; }
        br.xR = w.xR[i][l - 1];
        br.dW[0] = g.dWgate[l - 1]; br.dW[1] = g.dWnl[l - 1]; br.dW[2] = g.dWlin[l - 1];
        br.db[0] = g.dbgate[l - 1]; br.db[1] = g.dbnl[l - 1]; br.db[2] = g.dblin[l - 1];
      } else {
        for (int s = 0; s < 3; ++s) br.x[s] = b1.br[i].x[s];
        br.bn1 = s2s_bn(b.bn1); br.stat1 = w.stat1[i]; br.key = b1.br[i].key;
        br.dgamma1 = g.dbn1_weight; br.dbeta1 = g.dbn1_bias;
      }
    }
    if (int e = launch_s2s_hw_bwd(bp, st)) return e;
  }
  return MMF_OK;
}

// ---- standalone attention scorer: Attn_Net / Attn_Net_Gated .forward(x) -> (A, x) ------------------------------
namespace mmf {
struct AttnWs {
  float *a, *b, *s_part, *slab, *cs_bab, *cs_wc;
  int parts, mstk;
  TnPlan tn;                    // the gate problem alone (exact fp32: the scorer has no bf16x3 mode)
  size_t bytes;
};
static AttnWs carve_attn(void* base, int64_t N, int H, int D, int gated) {
  AttnWs w{};
  Carver c(base);
  auto take = [&](size_t n) { return c.take<float>(n); };
  w.parts = gate_parts(D, gated);
  w.mstk = gated ? 2 * D : D;
  const TnShape shape = {w.mstk, H, 1};
  w.tn = plan_tn(N, 0, &shape, 1);
  w.a = take((size_t)N * D);
  w.b = take(gated ? (size_t)N * D : 0);
  w.s_part = take((size_t)w.parts * N);
  w.slab = take((size_t)w.tn.splits_g * w.mstk * H);
  w.cs_bab = take((size_t)w.tn.splits_g * w.mstk);
  w.cs_wc = take((size_t)w.tn.splits_g * D);
  w.bytes = c.off;
  return w;
}
static int check_attn(const mmf_amil_desc* d) {
  if (!d || !d->Wa || !d->ba || !d->Wc || !d->bc) return MMF_ERR_ARG;
  if (d->gated && (!d->Wb || !d->bb)) return MMF_ERR_ARG;
  if (d->N < 1 || d->H % KC != 0 || d->D % 32 != 0) return MMF_ERR_SHAPE;
  const int64_t widest = d->H > 2 * d->D ? d->H : 2 * d->D;
  if (d->N * widest * 4 >= (int64_t)1 << 31) return MMF_ERR_SHAPE;
  if (d->p_att < 0.f || d->p_att >= 1.f) return MMF_ERR_ARG;
  return MMF_OK;
}
}  // namespace mmf

size_t mmf_attn_net_workspace_bytes(int64_t N, int32_t H, int32_t D, int32_t gated) {
  if (N < 1) N = 1;
  return carve_attn(nullptr, N, H, D, gated).bytes;
}

int mmf_attn_net_forward(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes, float* A,
                         void* stream) {
  if (int e = check_attn(d)) return e;
  if (!x || !workspace || !A) return MMF_ERR_ARG;
  if (!aligned16(x) || !aligned16(workspace) || !aligned16(d->Wa) || (d->gated && !aligned16(d->Wb))) return MMF_ERR_ALIGN;
  AttnWs w = carve_attn(workspace, d->N, d->H, d->D, d->gated);
  if (w.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  if (int e = launch_gate_fwd(gate_fwd_params(d, x, w.a, w.b, w.s_part, d->seed), st)) return e;
  return launch_score_sum(w.s_part, w.parts, d->bc, A, d->N, st);
}

int mmf_attn_net_backward(const mmf_amil_desc* d, const float* x, void* workspace, size_t workspace_bytes,
                          const float* gA, const mmf_amil_grads* g, void* stream) {
  if (int e = check_attn(d)) return e;
  if (!x || !workspace || !gA || !g) return MMF_ERR_ARG;
  if (!g->dWa || !g->dba || !g->dWc || !g->dbc || (d->gated && (!g->dWb || !g->dbb))) return MMF_ERR_ARG;
  if (!aligned16(g->dWa) || (d->gated && !aligned16(g->dWb)) || (g->dx && !aligned16(g->dx))) return MMF_ERR_ALIGN;
  AttnWs w = carve_attn(workspace, d->N, d->H, d->D, d->gated);
  if (w.bytes > workspace_bytes) return MMF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TraceScope ts(d->trace);
  const GateBwdCtx gc = gate_bwd_ctx(d, w.a, w.b, gA, d->seed);   // ds_i = dL/dA_i: the scorer has no softmax behind it here
  if (g->dx) {          // dx = dP . [Wa ; Wb]  (K-dh without relu' mask and pooling term)
    BwdDhParams dp{};
    dp.g = gc; dp.Wa = d->Wa; dp.Wb = d->Wb; dp.du = g->dx; dp.N = d->N; dp.H = d->H; dp.scale_h = 1.0f;
    if (int e = launch_bwd_dh(dh_plan(dp, false), dp, st)) return e;
  }
  TnParams tp{};
  tp.nprob = 1; tp.K = d->N; tp.g = gc;
  tp.prob[0] = tn_gate_problem(d, x, w.slab, w.cs_bab, w.cs_wc);
  if (int e = launch_tn(w.tn, tp, st)) return e;
  ReduceList rl;
  rl.add(w.slab, g->dWa, d->D * d->H, w.tn.splits_g, (size_t)w.mstk * d->H);
  if (d->gated) rl.add(w.slab + (size_t)d->D * d->H, g->dWb, d->D * d->H, w.tn.splits_g, (size_t)w.mstk * d->H);
  rl.add(w.cs_bab, g->dba, d->D, w.tn.splits_g, w.mstk);
  if (d->gated) rl.add(w.cs_bab + d->D, g->dbb, d->D, w.tn.splits_g, w.mstk);
  rl.add(w.cs_wc, g->dWc, d->D, w.tn.splits_g, d->D);
  rl.add(gA, g->dbc, 1, (int)d->N, 1);         // d(bc) = sum_i dL/dA_i
  return rl.launch(0, st);
}

size_t mmf_linear_forward_workspace_bytes(int64_t M, int32_t N, int32_t nseg, int32_t kseg) {
  if (nseg < 1 || nseg > 4 || kseg < 1) return 0;
  return linear_ksplit_floats(M, N, nseg * kseg, nseg, kseg) * sizeof(float);
}

int mmf_linear_forward(const float* const* x_segs, int32_t nseg, int32_t kseg, int64_t M,
                       const float* W, const float* bias, int32_t N, int32_t act,
                       float drop_p, uint32_t drop_seed, uint32_t drop_site, const uint32_t* seed_dev,
                       float* y, void* workspace, size_t workspace_bytes, uint32_t* sync, int32_t sync_words, void* stream) {
  if (!x_segs || nseg < 1 || nseg > 4 || !W || !y) return MMF_ERR_ARG;
  if (act < 0 || act > ACT_SELU || drop_p < 0.f || drop_p >= 1.f) return MMF_ERR_ARG;
  if (M * (int64_t)kseg * 4 >= (int64_t)1 << 31 || (int64_t)N * nseg * kseg * 4 >= (int64_t)1 << 31) return MMF_ERR_SHAPE;
  LinearParams lp{};
  for (int i = 0; i < nseg; ++i) {
    if (!x_segs[i]) return MMF_ERR_ARG;
    if (!aligned16(x_segs[i])) return MMF_ERR_ALIGN;
    lp.x[i] = x_segs[i];
  }
  if (!aligned16(W) || !aligned16(y) || (bias && !aligned16(bias))) return MMF_ERR_ALIGN;   // y, bias: float4 in the epilogue
  lp.nseg = nseg; lp.kseg = kseg; lp.ldx = kseg;
  lp.w = W; lp.bias = bias; lp.y = y; lp.M = M; lp.N = N; lp.K = nseg * kseg;
  lp.act = act; lp.drop_p = drop_p; lp.drop_key = drop_key(drop_seed, drop_site); lp.seed_dev = seed_dev;
  if (workspace && sync && sync_words > 0 && aligned16(workspace) &&
      workspace_bytes >= linear_ksplit_floats(M, N, lp.K, nseg, kseg) * sizeof(float) && workspace_bytes > 0) {
    lp.kpart = static_cast<float*>(workspace); lp.ktick = sync; lp.ktick_words = sync_words;
  }
  return launch_linear(lp, static_cast<hipStream_t>(stream));
}

// dW[N x K] as one problem over all K columns: the workspace query has no segments, so the splits are planned over
// ceil(K / tile) column tiles even where the launch's nseg problems of kseg columns round up to more
static TnPlan linear_bwd_plan(int64_t M, int N, int K) { const TnShape shape = {N, K, 0}; return plan_tn(M, 0, &shape, 1); }

// mmf_linear_backward's split-K slabs: dW's, then db's
struct LinearBwdWs { float *slab, *cs; size_t bytes; };
static LinearBwdWs carve_linear_bwd(void* base, int splits, int N, int K) {
  Carver c(base);
  LinearBwdWs w;
  w.slab = c.take<float>((size_t)splits * N * K);
  w.cs = c.take<float>((size_t)splits * N);
  w.bytes = c.off;
  return w;
}

size_t mmf_linear_backward_workspace_bytes(int64_t M, int32_t N, int32_t K) {
  const int s = linear_bwd_plan(M, N, K).splits;
  if (s == 1) return 256;
  return carve_linear_bwd(nullptr, s, N, K).bytes;
}

int mmf_linear_backward(const float* dy, const float* const* x_segs, int32_t nseg, int32_t kseg, int64_t M,
                        const float* W, int32_t N, float* dW, float* db, float* dx,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (!dy || !x_segs || nseg < 1 || nseg > 4 || !dW) return MMF_ERR_ARG;
  if (dx && (nseg != 1 || !W)) return MMF_ERR_ARG;
  const int K = nseg * kseg;
  if (N % 4 != 0 || kseg % 4 != 0) return MMF_ERR_SHAPE;
  if (dx && N % KC != 0) return MMF_ERR_SHAPE;           // dx = dy . W contracts over N in 32-chunks (launch_nn); every refusal comes before the first launch
  if (M * (int64_t)(N > kseg ? N : kseg) * 4 >= (int64_t)1 << 31 || (int64_t)N * K * 4 >= (int64_t)1 << 31) return MMF_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TnPlan tn = linear_bwd_plan(M, N, K);
  const int splits = tn.splits;
  if (splits > 1 && (!workspace || workspace_bytes < mmf_linear_backward_workspace_bytes(M, N, K))) return MMF_ERR_WORKSPACE;
  const LinearBwdWs lw = carve_linear_bwd(workspace, splits, N, K);
  float* slab = splits > 1 ? lw.slab : dW;
  float* cs = splits > 1 ? lw.cs : db;

  TnParams tp{};
  tp.nprob = nseg; tp.K = M;
  for (int i = 0; i < nseg; ++i) {
    if (!x_segs[i]) return MMF_ERR_ARG;
    TnProblem& q = tp.prob[i];
    q.kind = TN_A_PLAIN; q.A = dy; q.lda = N; q.M = N;
    q.B = x_segs[i]; q.ldb = kseg; q.Ncols = kseg;
    q.out = slab + (size_t)i * kseg; q.split_stride = (size_t)N * K; q.ldc = K;
    q.colsum = (i == 0 && db) ? cs : nullptr; q.colsum_stride = N;
  }
  if (int e = launch_tn(tn, tp, st)) return e;
  if (splits > 1) {
    ReduceList rl;
    rl.add(slab, dW, N * K, splits, (size_t)N * K);
    if (db) rl.add(cs, db, N, splits, (size_t)N);
    if (int e = rl.launch(0, st)) return e;
  }
  if (dx) {
    NnParams np{};
    np.A = dy; np.lda = N; np.B = W; np.ldb = K; np.C = dx; np.ldc = K; np.M = M; np.N = K; np.K = N;
    return launch_nn(np, st);
  }
  return MMF_OK;
}

int mmf_linear_input_grad(const float* dy, const float* W, int32_t nseg, int32_t kseg, int64_t M, int32_t N,
                          float* const* dx_segs, void* stream) {
  if (!dy || !W || !dx_segs || nseg < 1 || nseg > 4) return MMF_ERR_ARG;
  for (int i = 0; i < nseg; ++i)
    if (!dx_segs[i]) return MMF_ERR_ARG;
  if (M < 1 || N < KC || N % KC != 0 || kseg < 4 || kseg % 4 != 0) return MMF_ERR_SHAPE;
  const int K = nseg * kseg;
  if (M * (int64_t)(N > kseg ? N : kseg) * 4 >= (int64_t)1 << 31 || (int64_t)N * K * 4 >= (int64_t)1 << 31) return MMF_ERR_SHAPE;
  if (!aligned16(dy) || !aligned16(W)) return MMF_ERR_ALIGN;
  for (int i = 0; i < nseg; ++i)
    if (!aligned16(dx_segs[i])) return MMF_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int i = 0; i < nseg; ++i) {       // dx_i = dy . W[:, i kseg : (i + 1) kseg]
    NnParams np{};
    np.A = dy; np.lda = N; np.B = W + (size_t)i * kseg; np.ldb = K; np.C = dx_segs[i]; np.ldc = kseg;
    np.M = M; np.N = kseg; np.K = N;
    if (int e = launch_nn(np, st)) return e;
  }
  return MMF_OK;
}

int mmf_surv_head_forward(const float* feat, const float* Wk, const float* bk, int32_t B, int32_t F, int32_t K,
                          float* logits, float* hazards, float* S, int64_t* Y_hat, void* stream) {
  if (!feat || !Wk || !bk || !logits || !hazards || !S || !Y_hat || B < 1 || K < 1) return MMF_ERR_ARG;
  HeadParams p{feat, Wk, bk, B, F, K, logits, hazards, S, Y_hat};
  return launch_head_fwd(p, static_cast<hipStream_t>(stream));
}

int mmf_surv_head_backward(const float* g_hazards, const float* g_S, const float* hazards, const float* feat,
                           const float* Wk, int32_t B, int32_t F, int32_t K,
                           float* dfeat, float* dWk, float* dbk, void* stream) {
  if (!hazards || !feat || !Wk || !dfeat || !dWk || !dbk || B < 1 || K < 1) return MMF_ERR_ARG;
  HeadBwdParams p{g_hazards, g_S, hazards, feat, Wk, B, F, K, dfeat, dWk, dbk};
  return launch_head_bwd(p, static_cast<hipStream_t>(stream));
}

int mmf_nll_surv(const float* hazards, const float* S, const int64_t* Y, const float* c, int32_t B, int32_t K,
                 float alpha, float eps, float* loss, float* g_hazards, float* g_S, void* stream) {
  if (!hazards || !S || !Y || !c || !loss || !g_hazards || !g_S || B < 1 || K < 1) return MMF_ERR_ARG;
  NllParams p{hazards, S, Y, c, B, K, alpha, eps, loss, g_hazards, g_S};
  return launch_nll(p, static_cast<hipStream_t>(stream));
}

int mmf_cox_surv(const float* risks, const double* times, const float* c, int32_t B,
                 float* loss, float* d_risks, void* stream) {
  if (!risks || !times || !c || !loss || !d_risks || B < 1) return MMF_ERR_ARG;
  CoxParams p{risks, times, c, B, loss, d_risks};
  return launch_cox(p, static_cast<hipStream_t>(stream));
}

size_t mmf_maxnet_cox_step_workspace_bytes(int32_t B) {
  return maxnet_step_workspace_floats(B < 1 ? 1 : B) * sizeof(float);
}

int mmf_maxnet_cox_step(const mmf_maxnet_desc* d, const double* times, const float* c, float loss_scale,
                        void* workspace, size_t workspace_bytes, float* risk, float* loss,
                        const mmf_maxnet_grads* g, int32_t accumulate, void* stream) {
  if (!d || !times || !c || !workspace || !risk || !loss || !g) return MMF_ERR_ARG;
  if (!d->x || !d->W0 || !d->b0 || !d->W1 || !d->b1 || !d->Wc || !d->bc) return MMF_ERR_ARG;
  if (!g->dW0 || !g->db0 || !g->dW1 || !g->db1 || !g->dWc || !g->dbc) return MMF_ERR_ARG;
  if (!maxnet_step_ok(d->B, d->G, d->H0, d->H1)) return MMF_ERR_SHAPE;
  if (!d->sync || d->sync_words < 3) return MMF_ERR_ARG;          // the two grid barriers live in the caller's tick words
  if (d->p_drop < 0.f || d->p_drop >= 1.f) return MMF_ERR_ARG;
  if (workspace_bytes < mmf_maxnet_cox_step_workspace_bytes(d->B)) return MMF_ERR_WORKSPACE;
  // layer 1 and phase 3 read W1 with 16-byte loads, dpre1 / dpre0 leave as 16-byte stores into the workspace; times is double
  if (!aligned16(d->W1) || !aligned16(workspace) || (reinterpret_cast<uintptr_t>(times) & 7) != 0) return MMF_ERR_ALIGN;
  MaxnetStepParams p{};
  p.B = d->B; p.G = d->G;
  p.x = d->x; p.W0 = d->W0; p.b0 = d->b0; p.W1 = d->W1; p.b1 = d->b1; p.Wc = d->Wc; p.bc = d->bc;
  p.times = times; p.c = c;
  p.p = d->p_drop; p.key0 = drop_key(d->seed, 0); p.key1 = drop_key(d->seed, 1); p.seed_dev = d->seed_dev;
  p.loss_scale = loss_scale;
  float* w = static_cast<float*>(workspace);
  const size_t n = (size_t)d->B * 256;
  const size_t nt = (size_t)256 * maxnet_step_dp_pitch(d->B);
  p.y0 = w; p.y1 = w + n; p.dp1 = w + 2 * n; p.dp0 = p.dp1 + nt; p.dr = p.dp0 + nt;
  p.dwc_part = p.dr + (size_t)((d->B + 63) / 64 * 64);
  p.bar = d->sync;
  p.risk = risk; p.loss = loss;
  p.dW0 = g->dW0; p.db0 = g->db0; p.dW1 = g->dW1; p.db1 = g->db1; p.dWc = g->dWc; p.dbc = g->dbc;
  p.accumulate = accumulate ? 1 : 0;
  TraceScope ts(d->trace);
  return launch_maxnet_cox_step(p, static_cast<hipStream_t>(stream));
}


int mmf_adam_l1_step(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float l1_coeff, const float* l1_mask, int32_t step, void* stream) {
  if (!w || !g || !m || !v || n < 1 || step < 1) return MMF_ERR_ARG;
  if (l1_mask && !aligned16(l1_mask)) return MMF_ERR_ALIGN;
  if (!aligned16(w) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return MMF_ERR_ALIGN;
  AdamParams p{};
  p.w = w; p.g = g; p.m = m; p.v = v; p.n = n; p.l1_mask = l1_mask;
  p.b1 = beta1; p.b2 = beta2; p.eps = eps; p.wd = weight_decay; p.l1 = l1_coeff;
  // bias corrections in double, as torch computes them on the host
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  p.step_size = (float)((double)lr / bc1);
  p.bc2_sqrt = (float)std::sqrt(bc2);
  return launch_adam_l1(p, static_cast<hipStream_t>(stream));
}

int mmf_abs_sum(const float* w, int64_t n, float* partials, float* out, void* stream) {
  if (!w || !partials || !out || n < 1) return MMF_ERR_ARG;
  return launch_abs_sum(w, n, partials, out, static_cast<hipStream_t>(stream));
}

static DropSpec make_drop(int kind, float p, uint32_t seed, uint32_t site, const uint32_t* seed_dev) {
  DropSpec d;
  d.kind = p > 0.f ? kind : 0;
  d.p = p;
  d.key = drop_key(seed, site);
  d.dev = seed_dev;
  return d;
}

int mmf_dense_forward(const float* x, const float* W, const float* bias, int32_t B, int32_t K, int32_t N,
                      int32_t act, int32_t drop_kind, float drop_p, uint32_t seed, uint32_t site,
                      const uint32_t* seed_dev, float* y, void* stream) {
  if (!x || !W || !y || B < 1 || K < 1 || N < 1) return MMF_ERR_ARG;
  if (act < 0 || act > ACT_SELU || drop_kind < 0 || drop_kind > 2 || drop_p < 0.f || drop_p >= 1.f) return MMF_ERR_ARG;
  // the mask of element (b, n) is drawn at the 32-bit index b * N + n: beyond 2^32 elements indices would repeat
  if (drop_kind != 0 && drop_p > 0.f && (int64_t)B * N >= ((int64_t)1 << 32)) return MMF_ERR_SHAPE;
  DenseParams p{x, W, bias, y, B, K, N, act, make_drop(drop_kind, drop_p, seed, site, seed_dev)};
  return launch_dense_fwd(p, static_cast<hipStream_t>(stream));
}

int mmf_dense_backward(const float* dy, const float* y, const float* x, const float* W,
                       int32_t B, int32_t K, int32_t N, int32_t act,
                       int32_t drop_kind, float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev,
                       float* dpre_scratch, float* dx, float* dW, float* db, void* stream) {
  if (!dy || !y || !x || !W || !dpre_scratch || B < 1 || K < 1 || N < 1) return MMF_ERR_ARG;
  if (act < 0 || act > ACT_SELU || drop_kind < 0 || drop_kind > 2) return MMF_ERR_ARG;
  DenseBwdParams p{dy, y, x, W, dpre_scratch, dx, dW, db, B, K, N, act, make_drop(drop_kind, drop_p, seed, site, seed_dev)};
  return launch_dense_bwd(p, static_cast<hipStream_t>(stream));
}

uint32_t mmf_dropout_row_base(uint32_t seed) { return seed * hash_mul_inverse(); }

int mmf_dense_forward_rows(const float* x, const float* W, const float* bias, int32_t B, int32_t K, int32_t N,
                           int32_t act, int32_t drop_kind, float drop_p, uint32_t site, const uint32_t* seed_dev,
                           const uint32_t* row_base, float* y, int32_t ldy, void* stream) {
  if (!x || !W || !y || !row_base || B < 1 || K < 1 || N < 1) return MMF_ERR_ARG;
  if (act < 0 || act > ACT_SELU || drop_kind < 0 || drop_kind > 2 || drop_p < 0.f || drop_p >= 1.f) return MMF_ERR_ARG;
  if (ldy < N) return MMF_ERR_SHAPE;
  DenseParams p{x, W, bias, y, B, K, N, act, make_drop(drop_kind, drop_p, 0, site, seed_dev), row_base, ldy};
  return launch_dense_fwd(p, static_cast<hipStream_t>(stream));
}

int mmf_dense_backward_rows(const float* dy, int32_t lddy, const float* y, int32_t ldy, const float* x, const float* W,
                            int32_t B, int32_t K, int32_t N, int32_t act, int32_t drop_kind, float drop_p, uint32_t site,
                            const uint32_t* seed_dev, const uint32_t* row_base, float* dpre_scratch, float* dx, float* dW,
                            float* db, void* stream) {
  if (!dy || !y || !x || !W || !row_base || !dpre_scratch || B < 1 || K < 1 || N < 1) return MMF_ERR_ARG;
  if (act < 0 || act > ACT_SELU || drop_kind < 0 || drop_kind > 2) return MMF_ERR_ARG;
  if (ldy < N || lddy < N) return MMF_ERR_SHAPE;
  DenseBwdParams p{dy, y, x, W, dpre_scratch, dx, dW, db, B, K, N, act, make_drop(drop_kind, drop_p, 0, site, seed_dev),
                   row_base, ldy, lddy};
  return launch_dense_bwd(p, static_cast<hipStream_t>(stream));
}

int mmf_gate_mul_forward(const float* z, const float* h, float* o, int32_t n, void* stream) {
  if (!z || !h || !o || n < 1) return MMF_ERR_ARG;
  return launch_gate_mul(z, h, o, n, static_cast<hipStream_t>(stream));
}
int mmf_gate_mul_backward(const float* g, const float* z, const float* h, float* dz, float* dh, int32_t n, void* stream) {
  if (!g || !z || !h || !dz || !dh || n < 1) return MMF_ERR_ARG;
  return launch_gate_mul_bwd(g, z, h, dz, dh, n, static_cast<hipStream_t>(stream));
}

// The kron kernels index an element as b * S^m + e in int (S = dim + 1), hash that index into the 32-bit mask counter, and
// put B in grid.y: B * S^m < 2^31 and B <= 65535, or the call is refused before any launch.
static bool kron_shape_ok(int m, int dim, int B) {
  const int64_t S = (int64_t)dim + 1;
  if (B > 65535 || S > 46340) return false;                // 46341^2 > 2^31 already; below it S^3 fits int64
  const int64_t total = m == 3 ? S * S * S : S * S;
  return (int64_t)B * total < ((int64_t)1 << 31);
}

int mmf_kron_forward(const float* const* o, int32_t m, int32_t dim, int32_t B,
                     float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev, float* out, void* stream) {
  if (!o || (m != 2 && m != 3) || dim < 1 || B < 1 || !out) return MMF_ERR_ARG;
  KronParams p{};
  for (int i = 0; i < m; ++i) { if (!o[i]) return MMF_ERR_ARG; p.o[i] = o[i]; }
  if (!kron_shape_ok(m, dim, B)) return MMF_ERR_SHAPE;
  p.out = out; p.m = m; p.dim = dim; p.B = B; p.drop = make_drop(1, drop_p, seed, site, seed_dev);
  return launch_kron_fwd(p, static_cast<hipStream_t>(stream));
}
int mmf_kron_backward(const float* g, const float* const* o, int32_t m, int32_t dim, int32_t B,
                      float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev, float* const* d_o,
                      void* stream) {
  if (!g || !o || !d_o || (m != 2 && m != 3) || dim < 1 || B < 1) return MMF_ERR_ARG;
  KronParams p{};
  for (int i = 0; i < m; ++i) { if (!o[i] || !d_o[i]) return MMF_ERR_ARG; p.o[i] = o[i]; p.d[i] = d_o[i]; }
  if (!kron_shape_ok(m, dim, B)) return MMF_ERR_SHAPE;
  p.g = g; p.m = m; p.dim = dim; p.B = B; p.drop = make_drop(1, drop_p, seed, site, seed_dev);
  return launch_kron_bwd(p, static_cast<hipStream_t>(stream));
}

static int xreduce_params(const mmf_xreduce_io* io, float drop_p, uint32_t seed, const uint32_t* seed_dev, bool bwd,
                          XReduceParams& p) {
  if (!io || io->m < 1 || io->m > 3 || io->B < 1 || io->dim < 1 || io->sdim < 1) return MMF_ERR_ARG;
  if (drop_p < 0.f || drop_p >= 1.f) return MMF_ERR_ARG;
  p = XReduceParams{};
  p.m = io->m; p.B = io->B; p.dim = io->dim; p.sdim = io->sdim;
  for (int i = 0; i < io->m; ++i) {
    if (!io->v[i] || !io->Wh[i] || !io->bh[i] || !io->Wz[i] || !io->bz[i] || !io->Wo[i] || !io->bo[i]) return MMF_ERR_ARG;
    if (!io->h[i] || !io->z[i] || !io->gm[i] || !io->o[i]) return MMF_ERR_ARG;
    p.v[i] = io->v[i]; p.Wh[i] = io->Wh[i]; p.bh[i] = io->bh[i]; p.Wz[i] = io->Wz[i]; p.bz[i] = io->bz[i];
    p.Wo[i] = io->Wo[i]; p.bo[i] = io->bo[i];
    p.h[i] = io->h[i]; p.z[i] = io->z[i]; p.gm[i] = io->gm[i]; p.o[i] = io->o[i];
    if (bwd) {
      if (!io->d_o[i] || !io->dv[i] || !io->dWh[i] || !io->dbh[i] || !io->dWz[i] || !io->dbz[i] || !io->dWo[i] || !io->dbo[i])
        return MMF_ERR_ARG;
      p.d_o[i] = io->d_o[i]; p.dv[i] = io->dv[i];
      p.dWh[i] = io->dWh[i]; p.dbh[i] = io->dbh[i]; p.dWz[i] = io->dWz[i]; p.dbz[i] = io->dbz[i];
      p.dWo[i] = io->dWo[i]; p.dbo[i] = io->dbo[i];
    }
  }
  p.drop = make_drop(1, drop_p, seed, 0, seed_dev);
  return MMF_OK;
}
int mmf_xreduce_forward(const mmf_xreduce_io* io, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream) {
  XReduceParams p;
  if (int e = xreduce_params(io, drop_p, seed, seed_dev, false, p)) return e;
  for (int i = 0; i < p.m; ++i)       // wave_dot's 16-byte loads (the backward reads scalars and needs neither this nor dim % 4)
    if (!aligned16(p.v[i]) || !aligned16(p.Wh[i]) || !aligned16(p.Wz[i])) return MMF_ERR_ALIGN;
  return launch_xreduce_fwd(p, static_cast<hipStream_t>(stream));
}
int mmf_xreduce_backward(const mmf_xreduce_io* io, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream) {
  XReduceParams p;
  if (int e = xreduce_params(io, drop_p, seed, seed_dev, true, p)) return e;
  return launch_xreduce_bwd(p, static_cast<hipStream_t>(stream));
}

int mmf_batchnorm_forward(const float* x, const float* res, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int32_t B, int32_t F, int32_t training,
                          float eps, float momentum, int32_t act, float drop_p, uint32_t seed, uint32_t site,
                          const uint32_t* seed_dev, float* y, float* save_mean, float* save_invstd, void* stream) {
  if (!x || !y || !save_mean || !save_invstd || B < 1 || F < 1) return MMF_ERR_ARG;
  if (!training && (!running_mean || !running_var)) return MMF_ERR_ARG;
  if (act < 0 || act > ACT_SELU || drop_p < 0.f || drop_p >= 1.f) return MMF_ERR_ARG;
  BnParams p{x, res, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, B, F, training, act, eps, momentum,
             make_drop(1, drop_p, seed, site, seed_dev)};
  return launch_bn_fwd(p, static_cast<hipStream_t>(stream));
}
int mmf_batchnorm_backward(const float* dy, const float* y, const float* x, const float* gamma,
                           const float* save_mean, const float* save_invstd, int32_t B, int32_t F, int32_t training,
                           int32_t act, float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev,
                           float* dx, float* dres, float* dgamma, float* dbeta, void* stream) {
  if (!dy || !y || !x || !save_mean || !save_invstd || !dx || B < 1 || F < 1) return MMF_ERR_ARG;
  if (act < 0 || act > ACT_SELU || drop_p < 0.f || drop_p >= 1.f) return MMF_ERR_ARG;
  BnBwdParams p{dy, y, x, gamma, save_mean, save_invstd, dx, dres, dgamma, dbeta, B, F, training, act,
                make_drop(1, drop_p, seed, site, seed_dev)};
  return launch_bn_bwd(p, static_cast<hipStream_t>(stream));
}
int mmf_highway_mix_forward(const float* zg, const float* zn, const float* zl, int64_t n, float* y, void* stream) {
  if (!zg || !zn || !zl || !y || n < 1) return MMF_ERR_ARG;
  HighwayParams p{zg, zn, zl, y, nullptr, nullptr, nullptr, nullptr, n};
  return launch_highway_fwd(p, static_cast<hipStream_t>(stream));
}
int mmf_highway_mix_backward(const float* dy, const float* zg, const float* zn, const float* zl, int64_t n,
                             float* dzg, float* dzn, float* dzl, void* stream) {
  if (!dy || !zg || !zn || !zl || !dzg || !dzn || !dzl || n < 1) return MMF_ERR_ARG;
  HighwayParams p{zg, zn, zl, nullptr, dy, dzg, dzn, dzl, n};
  return launch_highway_bwd(p, static_cast<hipStream_t>(stream));
}
int mmf_ranking_loss(const float* risks, const double* times, const float* c, int32_t B, int32_t phi, int32_t reduction,
                     float* loss, float* d_risks, void* stream) {
  if (!risks || !times || !c || !loss || !d_risks) return MMF_ERR_ARG;
  if (phi < 0 || phi > 1 || reduction < 0 || reduction > 1) return MMF_ERR_ARG;
  RankParams p{risks, times, c, B, phi, reduction, loss, d_risks};
  return launch_rank_loss(p, static_cast<hipStream_t>(stream));
}
int mmf_hazards_forward(const float* logits, int32_t B, int32_t K, float* hazards, float* S, int64_t* Y_hat, float* risk,
                        void* stream) {
  if (!logits || !hazards || !S) return MMF_ERR_ARG;
  HazardParams p{logits, hazards, S, risk, Y_hat, nullptr, nullptr, nullptr, nullptr, B, K};
  return launch_hazard_fwd(p, static_cast<hipStream_t>(stream));
}
int mmf_hazards_backward(const float* g_hazards, const float* g_S, const float* g_risk, const float* hazards,
                         int32_t B, int32_t K, float* dlogits, void* stream) {
  if (!hazards || !dlogits) return MMF_ERR_ARG;
  HazardParams p{nullptr, const_cast<float*>(hazards), nullptr, nullptr, nullptr, g_hazards, g_S, g_risk, dlogits, B, K};
  return launch_hazard_bwd(p, static_cast<hipStream_t>(stream));
}

mmf_trace* mmf_trace_create(int32_t capacity) {
  if (capacity < 1) return nullptr;
  mmf_trace* t = new (std::nothrow) mmf_trace();
  if (t) { t->cap = capacity; t->recs.reserve(capacity); }
  return t;
}

void mmf_trace_destroy(mmf_trace* t) {
  if (!t) return;
  for (auto& r : t->recs) { if (r.a) hipEventDestroy(r.a); if (r.b) hipEventDestroy(r.b); }
  for (auto e : t->pool) hipEventDestroy(e);
  delete t;
}

// Synchronises on the recorded events, writes "name count total_ms\n" lines, clears the records.
int mmf_trace_dump(mmf_trace* t, char* buf, size_t buf_bytes) {
  if (!t) return MMF_ERR_ARG;
  std::lock_guard<std::mutex> lock(t->mu);
  std::map<std::string, std::pair<int, double>> agg;
  for (auto& r : t->recs) {
    float ms = 0.f;
    if (r.a && r.b && hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      auto& e = agg[r.name];
      e.first += 1;
      e.second += ms;
    }
    if (r.a) t->pool.push_back(r.a);
    if (r.b) t->pool.push_back(r.b);
  }
  t->recs.clear();
  std::string out;
  char line[256];
  for (auto& kv : agg) {
    snprintf(line, sizeof line, "%s %d %.6f\n", kv.first.c_str(), kv.second.first, kv.second.second);
    out += line;
  }
  if (!buf || buf_bytes == 0) return (int)out.size();
  size_t n = out.size() < buf_bytes - 1 ? out.size() : buf_bytes - 1;
  memcpy(buf, out.data(), n);
  buf[n] = 0;
  return (int)n;
}

int mmf_dropout_keep_host(uint32_t seed, uint32_t site, uint32_t index, float p) {
  return keep(drop_key(seed, site), index, drop_threshold(p)) ? 1 : 0;
}

}  // extern "C"
