// Forward kernels of the attention-MIL stack on MI355X (gfx950).
//
//   K-lin   y = drop(act(x.W^T + b))                 models/model_attention_mil_path.py:20-21 (Linear+ReLU+Dropout)
//                                                    models/model_attention_mil_radio.py:80-82 (cat + reduce_dim)
//   K-gate  a = tanh(h.Wa^T+ba), b = sigmoid(h.Wb^T+bb), s_part = sum_d a.b.Wc   models/model_modules.py:105-110 (gated)
//           a = tanh(h.Wa^T+ba),                          s_part = sum_d a.Wc     models/model_modules.py:73-85  (ungated)
//   K-pool  A_raw = sum(s_part)+bc ; per-group online-softmax partials (max, sum e, sum e.h)
//   K-merge M = softmax(A_raw).h, (max, denom)        models/model_attention_mil_path.py:53-56
#include <cstdlib>

#include "mmf_gemm_core.h"
#include "mmf_gemm_split.h"
#include "mmf_kernels.h"
#include "mmf_ig_head.h"

namespace mmf {

// =============================================================================================
// K-lin : NT GEMM + bias + activation + dropout
// =============================================================================================
__device__ inline float apply_act(float v, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(v, 0.f);
    case ACT_TANH: return fast_tanh(v);
    case ACT_SIGMOID: return fast_sigmoid(v);
    case ACT_SELU: {
      const float alpha = 1.6732632423543772f, scale = 1.0507009873554805f;
      return scale * (v > 0.f ? v : alpha * (__expf(v) - 1.0f));
    }
    default: return v;
  }
}

// Epilogue of K-lin.  The activation and the dropout switch are compile-time: with run-time `switch (p.act)` /
// `if (p.drop_p > 0)` inside the element loop the tile's 448 elements per lane each went through three scalar
// branches (every taken branch refills the instruction buffer); the kernel dispatches ONCE per workgroup instead.
// ACT = -1: any activation, decided per element (the rarely used tanh / sigmoid / SELU projections).
// K-split launches: where the last-arriving workgroup of a tile finds the tile's partial sums (LinearParams::kpart)
struct PartSrc {
  unsigned bytes;       // size of the whole kpart buffer (the buffer resource is rebuilt where it is used: kept in the
                        // struct it lived in scratch)
  unsigned base;        // byte offset of this tile's first partial
  unsigned slab;        // bytes per partial tile (BM x BN floats)
  int S;                // partials per tile
};

template <class T, int ACT, bool DROP, bool SEG = false>
__device__ inline void linear_epilogue(const LinearParams& p, f32x16 (&acc)[T::MB][T::NB], f32x4acc (*acch)[2], float* lds,
                                       int row0, int col0, const PartSrc ps = PartSrc{}) {
  const uint32_t thr = drop_threshold(p.drop_p);
  const float scale = DROP ? 1.0f / (1.0f - p.drop_p) : 1.0f;
  const uint32_t dkey = p.drop_key + (p.seed_dev ? *p.seed_dev : 0u);   // device-resident part of the seed, if any
  float4 bias4[T::NB];                       // per column strip, loaded once, before any store
#pragma unroll
  for (int nb = 0; nb < T::NB; ++nb) {
    const int col = col0 + epilogue_col<T>(nb);
    bias4[nb] = (p.bias && col < p.N) ? ld4(p.bias + col) : zero4();
  }
  const int lane = threadIdx.x & 63;
  // one transposed block: NT row groups (rows r + 8 t) of 4 consecutive columns per lane; NT = 4 for a 32-row block,
  // 2 for the 16-row half block
  auto rows_op = [&](auto nt_c, int nb, int r, int c, const float4* v) {
    constexpr int NTR = decltype(nt_c)::value;
    const int col = col0 + c;
    const bool col_ok = col < p.N;           // N % 4 == 0: a float4 never straddles the edge
    const float4 b4 = bias4[nb];
    unsigned long long mine = 0ull;          // lane 4 t + e keeps ballot (t, e) of this block (LinearParams::relu_bits)
#pragma unroll
    for (int t = 0; t < NTR; ++t) {
      const int row = row0 + r + 8 * t;
      const bool ok = col_ok && row < p.M;
      float y[4] = {v[t].x + b4.x, v[t].y + b4.y, v[t].z + b4.z, v[t].w + b4.w};
      uint32_t idx;
      if constexpr (SEG) idx = (row < p.M ? p.seg_ridx[row] : 0u) + (uint32_t)col;   // bag-local index + bag seed term
      else idx = (uint32_t)row * (uint32_t)p.N + (uint32_t)col;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (ACT == ACT_RELU) y[e] = fmaxf(y[e], 0.f);
        else if constexpr (ACT < 0) y[e] = apply_act(y[e], p.act);
        if constexpr (DROP) y[e] = keep(dkey, idx + e, thr) ? y[e] * scale : 0.f;
      }
      // (Tried: taking these ballots in K-gate's A loader instead, where h streams through staging registers anyway.
      // The projection got 2 us back, K-gate lost 11: its first-column tiles became the launch's critical path.)
      if (p.relu_bits) {                     // wave-uniform; the ballots are taken by every lane, valid or not
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned long long bal = __ballot(ok && y[e] > 0.f);
          if (lane == 4 * t + e) mine = bal;
        }
      }
      if (ok) st4(p.y + (size_t)row * p.N + col, make_float4(y[0], y[1], y[2], y[3]));
    }
    if (p.relu_bits && lane < 4 * NTR) {
      // 16-row granularity: rows r0 + rr + 8 t with t = 0, 1 are bit block r0 / 16, t = 2, 3 bit block r0 / 16 + 1
      const size_t rb16 = ((size_t)(row0 + r - (lane >> 3)) >> 4) + (lane >> 3), cb = (size_t)(col0 + c - 4 * (lane & 7)) >> 5;
      if ((int64_t)rb16 * 16 < p.M && (int)(cb * 32) < p.N) p.relu_bits[(rb16 * (size_t)(p.N >> 5) + cb) * 8 + (lane & 7)] = mine;
    }
  };
  if (ps.S > 0) {
    // the tile's sum comes from memory, already row-major: partial s of the tile, rows r + 8 t, columns c .. c + 3 of this
    // lane -- added in split order (bit-reproducible); the loads of block b + 1 are issued before block b's stores
    const int wave = threadIdx.x >> 6, wm = wave / T::WN, wn = wave % T::WN;
    const int rr = lane >> 3, c4 = lane & 7;
    constexpr int NBLK = T::MB * T::NB;
    const rsrc_t prs = make_rsrc(p.kpart, ps.bytes);
    float4 buf[2][4];
    auto fetch = [&](int b, int rows4, float4 (&v)[4]) {
      const int mb = b / T::NB, nb = b % T::NB;
      const int r = wm * (T::BM / T::WM) + mb * 32 + rr, c = (wn * T::NB + nb) * 32 + 4 * c4;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t >= rows4) break;
        const unsigned o = ps.base + (unsigned)((r + 8 * t) * T::BN + c) * 4u;
        float4 a = bld4_dev(prs, o, 0);
        for (int k = 1; k < ps.S; ++k) {
          const float4 q = bld4_dev(prs, o, (unsigned)k * ps.slab);
          a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
        }
        v[t] = a;
      }
    };
    fetch(0, 4, buf[0]);
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
      const int mb = b / T::NB, nb = b % T::NB;
      if (b + 1 < NBLK) fetch(b + 1, 4, buf[(b + 1) & 1]);
      else if constexpr (T::HALF) fetch(T::MB * T::NB, 2, buf[(b + 1) & 1]);
      rows_op(std::integral_constant<int, 4>{}, nb, wm * (T::BM / T::WM) + mb * 32 + rr, (wn * T::NB + nb) * 32 + 4 * c4, buf[b & 1]);
    }
    if constexpr (T::HALF) {
#pragma unroll
      for (int nb = 0; nb < T::NB; ++nb) {
        if (nb + 1 < T::NB) fetch(T::MB * T::NB + nb + 1, 2, buf[(NBLK + nb + 1) & 1]);
        rows_op(std::integral_constant<int, 2>{}, nb, wm * (T::BM / T::WM) + T::MB * 32 + rr, (wn * T::NB + nb) * 32 + 4 * c4,
                buf[(NBLK + nb) & 1]);
      }
    }
    return;
  }
  epilogue_rows<T>(acc, lds, [&](int mb, int nb, int r, int c, const float4 (&v)[4]) {
    rows_op(std::integral_constant<int, 4>{}, nb, r, c, v);
  });
  if constexpr (T::HALF) {
    const int wave = threadIdx.x >> 6, wm = wave / T::WN, wn = wave % T::WN;
    float* blk = lds + wave * (32 * EPI_STRIDE);
#pragma unroll
    for (int nb = 0; nb < T::NB; ++nb) {
      float4 v[2];
      transpose_half(acch[nb][0], acch[nb][1], blk, lane, v);
      rows_op(std::integral_constant<int, 2>{}, nb, wm * (T::BM / T::WM) + T::MB * 32 + (lane >> 3),
              (wn * T::NB + nb) * 32 + 4 * (lane & 7), v);
    }
  }
}

// K-split: this workgroup's accumulators -> its partial tile (device-scope stores), then a ticket.  Returns true for the
// workgroup that arrived LAST at the tile (all partials are in memory then): it runs the epilogue from the partials.
template <class T>
__device__ inline bool ksplit_publish(const LinearParams& p, f32x16 (&acc)[T::MB][T::NB], f32x4acc (*acch)[2], float* lds,
                                      int tile, int ks, PartSrc& ps) {
  const int S = p.ksplit;
  ps.bytes = (unsigned)((size_t)p.mt_count * p.nt_count * S * T::BM * T::BN * 4u);
  const rsrc_t prs = make_rsrc(p.kpart, ps.bytes);
  ps.slab = (unsigned)(T::BM * T::BN * 4);
  ps.base = (unsigned)tile * (unsigned)S * ps.slab;
  ps.S = S;
  const unsigned mine = ps.base + (unsigned)ks * ps.slab;
  epilogue_rows<T>(acc, lds, [&](int mb, int nb, int r, int c, const float4 (&v)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) bst4_dev(prs, mine + (unsigned)((r + 8 * t) * T::BN + c) * 4u, 0, v[t]);
  });
  if constexpr (T::HALF) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave / T::WN, wn = wave % T::WN;
    float* blk = lds + wave * (32 * EPI_STRIDE);
#pragma unroll
    for (int nb = 0; nb < T::NB; ++nb) {
      float4 v[2];
      transpose_half(acch[nb][0], acch[nb][1], blk, lane, v);
      const int r = wm * (T::BM / T::WM) + T::MB * 32 + (lane >> 3), c = (wn * T::NB + nb) * 32 + 4 * (lane & 7);
#pragma unroll
      for (int t = 0; t < 2; ++t) bst4_dev(prs, mine + (unsigned)((r + 8 * t) * T::BN + c) * 4u, 0, v[t]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's partial rows have reached device scope
  __syncthreads();                                        // ... and every wave's
  unsigned* flag = reinterpret_cast<unsigned*>(lds + (T::NT / 64) * 32 * EPI_STRIDE);     // behind the transpose scratch
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(p.ktick + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (unsigned)(S - 1)) __hip_atomic_store(p.ktick + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // left zero for the next launch
    flag[0] = old;
  }
  __syncthreads();
  return flag[0] == (unsigned)(S - 1);
}

template <class T, bool SEG = false>
__global__ __launch_bounds__(T::NT) void linear_nt_kernel(LinearParams p) {
  extern __shared__ __align__(16) float lds[];
  const int S = p.ksplit > 1 ? p.ksplit : 1;
  int mt, ntk;
  // the (column tile, K split) pairs of one row tile are 8 workgroups apart: one XCD, whose L2 serves the shared x rows
  if (!tile_of_block(blockIdx.x, p.mt_count, p.nt_count * S, mt, ntk)) return;
  const int nt = ntk % p.nt_count, ks = ntk / p.nt_count;
  const int row0 = mt * T::BM, col0 = nt * T::BN;
  const int nk = p.K / KC / S;

  LoadK<T::BM, T::NT> la;
  la.init_segments(p.x, p.nseg, p.kseg, p.ldx, row0, (int)p.M);
  LoadK<T::BN, T::NT> lb;
  lb.init(p.w, p.K, col0, p.N);
  la.kt0 = lb.kt0 = ks * nk;

  f32x16 acc[T::MB][T::NB];
  f32x4acc acch[T::NB][2];                   // the half block's accumulators (Tile::HALF; unused otherwise)
  if constexpr (T::NT == 256 && T::BM <= 64) {
    if (p.deep) gemm_mainloop_deep<T, 4>(la, lb, nk, lds, acc);      // short grid: see gemm_mainloop_deep
    else gemm_mainloop<T>(la, lb, nk, lds, acc);
  } else {
    gemm_mainloop<T>(la, lb, nk, lds, acc, acch);
  }
  PartSrc ps{};                              // S = 0: the epilogue takes the tile from the accumulators
  if (S > 1) {
    if (!ksplit_publish<T>(p, acc, acch, lds, mt * p.nt_count + nt, ks, ps)) return;
  }
  const bool drop = p.drop_p > 0.f;
  if constexpr (SEG) {          // grouped step: ReLU + dropout with per-bag masks (launch_linear_seg)
    linear_epilogue<T, ACT_RELU, true, true>(p, acc, acch, lds, row0, col0, ps);
    return;
  }
  if (p.act == ACT_RELU) {
    if (drop) linear_epilogue<T, ACT_RELU, true>(p, acc, acch, lds, row0, col0, ps);
    else linear_epilogue<T, ACT_RELU, false>(p, acc, acch, lds, row0, col0, ps);
  } else if (p.act == ACT_NONE && !drop) {
    linear_epilogue<T, ACT_NONE, false>(p, acc, acch, lds, row0, col0, ps);
  } else if (drop) {
    linear_epilogue<T, -1, true>(p, acc, acch, lds, row0, col0, ps);
  } else {
    linear_epilogue<T, -1, false>(p, acc, acch, lds, row0, col0, ps);
  }
}

// The same projection on the bf16 matrix cores (mmf_gemm_split.h: 3-way operand split, fp32-equivalent accuracy).
template <class T>
__global__ __launch_bounds__(T::NT) void linear_nt_split_kernel(LinearParams p) {
  extern __shared__ __align__(16) float lds[];
  int mt, nt;
  if (!tile_of_block(blockIdx.x, p.mt_count, p.nt_count, mt, nt)) return;
  const int row0 = mt * T::BM, col0 = nt * T::BN;
  SplitK<T::BM, T::NT> la;
  la.init(p.x[0], p.ldx, row0, (int)p.M);
  SplitK<T::BN, T::NT> lb;
  lb.init(p.w, p.K, col0, p.N);
  f32x16 acc[T::MB][T::NB];
  split_mainloop<T, 4>(la, lb, p.K / SKC, lds, acc);
  const bool drop = p.drop_p > 0.f;
  if (p.act == ACT_RELU) {
    if (drop) linear_epilogue<T, ACT_RELU, true>(p, acc, nullptr, lds, row0, col0);
    else linear_epilogue<T, ACT_RELU, false>(p, acc, nullptr, lds, row0, col0);
  } else if (p.act == ACT_NONE && !drop) {
    linear_epilogue<T, ACT_NONE, false>(p, acc, nullptr, lds, row0, col0);
  } else if (drop) {
    linear_epilogue<T, -1, true>(p, acc, nullptr, lds, row0, col0);
  } else {
    linear_epilogue<T, -1, false>(p, acc, nullptr, lds, row0, col0);
  }
}

// =============================================================================================
// K-gate : NT GEMM of h against an interleaved [Wa-block | Wb-block] tile, fused gate epilogue
// =============================================================================================
// B-operand loader: tile row j -> 32-row block jb = j/32.  Gated: blocks alternate a, b for the
// same 32 attention dims, so a wave's (nb = 2t, 2t+1) accumulators hold the tanh- and the
// sigmoid-branch pre-activations of the SAME (instance, d) in the SAME lane and register.
// HALVES = false: 32-row blocks alternate (a, b) for the same 32 attention dims (2x2-wave tiles: a wave's
//                 nb = 2t, 2t+1 accumulators are the tanh and sigmoid branch of the same (instance, d));
// HALVES = true : rows [0, ROWS/2) are the a-branch, [ROWS/2, ROWS) the b-branch of dims d0 .. d0+ROWS/2-1
//                 (1x8-wave tiles: waves 0-3 hold a, waves 4-7 hold b; they meet through LDS in the epilogue).
template <int ROWS, int NT, bool GATED, bool HALVES>
struct LoadGateW {
  using Map = KMap<ROWS, NT>;
  rsrc_t ra, rb;
  int tid;
  int which[Map::NV];          // wave-uniform (a wave-instruction covers 8 consecutive tile rows)
  unsigned voff[Map::NV];
  float4 r[Map::NV];
  __device__ inline void init(const float* wa, const float* wb, int H, int D, int d0) {
    tid = threadIdx.x;
    ra = make_rsrc(wa, (unsigned)D * (unsigned)H * 4u);
    rb = make_rsrc(GATED ? wb : wa, (unsigned)D * (unsigned)H * 4u);
#pragma unroll
    for (int i = 0; i < Map::NV; ++i) {
      const int j = Map::row(tid, i);
      int w, d;
      if (!GATED) { w = 0; d = d0 + j; }
      else if (HALVES) { w = j >= ROWS / 2 ? 1 : 0; d = d0 + j - w * (ROWS / 2); }
      else { w = (j >> 5) & 1; d = d0 + (j >> 6) * 32 + (j & 31); }
      which[i] = __builtin_amdgcn_readfirstlane(w);
      voff[i] = (Map::valid(tid, i) && d < D) ? ((unsigned)d * (unsigned)H + 4u * Map::c4(tid, i)) * 4u : OOB;
    }
  }
  __device__ inline void load(int kt) {
    const unsigned soff = (unsigned)(kt * KC) * 4u;
#pragma unroll
    for (int i = 0; i < Map::NV; ++i) r[i] = bld4(which[i] ? rb : ra, voff[i], soff);
  }
  __device__ inline void store(float* lds) const {
#pragma unroll
    for (int i = 0; i < Map::NV; ++i)
      if (Map::valid(tid, i)) st4(lds + Map::lds(tid, i), r[i]);
  }
};

template <class T, bool GATED, bool SEG = false>
__device__ inline void gate_fwd_tile(const GateFwdParams& p, float* lds, int row0, int nt);

template <class T, bool GATED, bool SEG = false>
__global__ __launch_bounds__(T::NT) void gate_fwd_kernel(GateFwdParams p) {
  extern __shared__ __align__(16) float lds[];
  int mt, nt;
  if (!tile_of_block(blockIdx.x, p.mt_count, p.nt_count, mt, nt)) return;
  gate_fwd_tile<T, GATED, SEG>(p, lds, (int)p.row_begin + mt * T::BM, nt);
}

// Two tile heights in ONE launch: the bag's rows are cut into regions of tall (TB) or short (TS) tiles, taken by
// consecutive ranges of workgroups (GateFwdParams::reg; launch_gate_fwd plans them).  TB and TS have the same thread
// count and column width.
template <class TB, class TS, bool GATED, bool SEG = false>
__global__ __launch_bounds__(TB::NT) void gate_fwd_mixed_kernel(GateFwdParams p) {
  static_assert(TB::NT == TS::NT && TB::BN == TS::BN, "mixed tiles share the launch shape");
  extern __shared__ __align__(16) float lds[];
  int r = 0;
  for (int i = 1; i < p.nreg; ++i)
    if ((int)blockIdx.x >= p.reg[i].grid_begin) r = i;
  int mt, nt;
  if (!tile_of_block(blockIdx.x - p.reg[r].grid_begin, p.reg[r].mt_count, p.nt_count, mt, nt)) return;
  if (p.reg[r].tall) gate_fwd_tile<TB, GATED, SEG>(p, lds, (int)p.reg[r].row0 + mt * TB::BM, nt);
  else gate_fwd_tile<TS, GATED, SEG>(p, lds, (int)p.reg[r].row0 + mt * TS::BM, nt);
}

template <class T, bool GATED, bool SEG>
__device__ inline void gate_fwd_tile(const GateFwdParams& p, float* lds, int row0, int nt) {
  constexpr int DT = GATED ? T::BN / 2 : T::BN;   // attention dims covered by one tile
  const int d0 = nt * DT;

  std::conditional_t<T::SPLIT, SplitK<T::BM, T::NT>, LoadK<T::BM, T::NT>> la;
  la.init(p.h, p.H, row0, (int)p.row_end);
  std::conditional_t<T::SPLIT, SplitGateW<T::BN, T::NT, GATED>, LoadGateW<T::BN, T::NT, GATED, false>> lb;
  lb.init(p.Wa, p.Wb, p.H, p.D, d0);

  f32x16 acc[T::MB][T::NB];
  if constexpr (T::SPLIT) {
    split_mainloop<T, 4>(la, lb, p.H / SKC, lds, acc);
  } else if constexpr (T::BM <= 64) {
    if (p.deep) gemm_mainloop_deep<T, 4>(la, lb, p.H / KC, lds, acc);      // short grid: see gemm_mainloop_deep
    else gemm_mainloop<T>(la, lb, p.H / KC, lds, acc);
  } else {
    gemm_mainloop<T>(la, lb, p.H / KC, lds, acc);
  }

  // ---- epilogue (row-major, float4): activations, stores of a / b, per-row partial score ----------------
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / T::WN, wn = wave % T::WN;
  const int rr = lane >> 3, c4 = lane & 7;
  const uint32_t thr = drop_threshold(p.drop_p);
  const bool drop = p.drop_p > 0.f;
  const float dscale = drop ? 1.0f / (1.0f - p.drop_p) : 1.0f;
  const uint32_t sdev = p.seed_dev ? *p.seed_dev : 0u;
  const uint32_t key_a = p.key_a + sdev, key_b = p.key_b + sdev;
  float* blk = lds + wave * (32 * EPI_STRIDE);
  float* sred = lds + (T::NT / 64) * (32 * EPI_STRIDE);   // [WN][BM] row partials, behind the transpose scratch

  constexpr int NPAIR = GATED ? T::NB / 2 : T::NB;
  float4 ba_r[NPAIR], bb_r[NPAIR], wc_r[NPAIR];   // per column strip, loaded once, before any store
#pragma unroll
  for (int t = 0; t < NPAIR; ++t) {
    const int d = d0 + (wn * NPAIR + t) * 32 + 4 * c4;
    const bool dok = d < p.D;
    ba_r[t] = dok ? ld4(p.ba + d) : zero4();
    bb_r[t] = (GATED && dok) ? ld4(p.bb + d) : zero4();
    wc_r[t] = dok ? ld4(p.Wc + d) : zero4();
  }
#pragma unroll
  for (int mb = 0; mb < T::MB; ++mb) {
    float rowsum[4] = {0.f, 0.f, 0.f, 0.f};     // rows rr + 8t of this 32-row block, this lane's columns
#pragma unroll
    for (int t = 0; t < NPAIR; ++t) {
      const int d = d0 + (wn * NPAIR + t) * 32 + 4 * c4;
      const bool dok = d < p.D;
      float4 va[4], vb[4];
      transpose_block(acc[mb][GATED ? 2 * t : t], blk, lane, va);
      if constexpr (GATED) transpose_block(acc[mb][2 * t + 1], blk, lane, vb);
      const float4 ba4 = ba_r[t], bb4 = bb_r[t], wc4 = wc_r[t];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = row0 + (wm * T::MB + mb) * 32 + rr + 8 * q;
        float av[4] = {fast_tanh(va[q].x + ba4.x), fast_tanh(va[q].y + ba4.y), fast_tanh(va[q].z + ba4.z), fast_tanh(va[q].w + ba4.w)};
        float bv[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (GATED) {
          bv[0] = fast_sigmoid(vb[q].x + bb4.x); bv[1] = fast_sigmoid(vb[q].y + bb4.y);
          bv[2] = fast_sigmoid(vb[q].z + bb4.z); bv[3] = fast_sigmoid(vb[q].w + bb4.w);
        }
        if (row < p.row_end && dok) {
          const size_t o = (size_t)row * p.D + d;
          if (p.a) {     // null in forward-only (inference) calls: nothing is saved for a backward
            st4(p.a + o, make_float4(av[0], av[1], av[2], av[3]));
            if constexpr (GATED) st4(p.b + o, make_float4(bv[0], bv[1], bv[2], bv[3]));
          }
          const float wc[4] = {wc4.x, wc4.y, wc4.z, wc4.w};
          uint32_t idx;
          if constexpr (SEG) idx = p.seg_ridx[row] + (uint32_t)d;     // grouped step: bag-local mask index
          else idx = (uint32_t)row * (uint32_t)p.D + (uint32_t)d;
          if (drop) {       // decided once per row, not per element
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float ad = keep(key_a, idx + e, thr) ? av[e] * dscale : 0.f;
              float bd = bv[e];
              if constexpr (GATED) bd = keep(key_b, idx + e, thr) ? bd * dscale : 0.f;
              rowsum[q] += ad * bd * wc[e];
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) rowsum[q] += av[e] * bv[e] * wc[e];
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {       // the 8 lanes that share a row hold 4 columns each
      float s = rowsum[q];
      s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
      if (c4 == 0) sred[wn * T::BM + (wm * T::MB + mb) * 32 + rr + 8 * q] = s;
    }
  }
  __syncthreads();
  for (int i = tid; i < T::BM; i += T::NT) {
    int row = row0 + i;
    if (row < p.row_end) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < T::WN; ++w) s += sred[w * T::BM + i];
      p.s_part[(size_t)nt * p.N + row] = s;
    }
  }
}

// =============================================================================================
// K-pool : scores + per-group online-softmax partials.  HBM-bound (reads h once).
// =============================================================================================

// one partial group: rows r0 .. r1 - 1 -> A_raw of those rows and partials[g] = {max, sum e, sum e h}
__device__ __forceinline__ void pool_partial_rows(const PoolParams& p, int g, int64_t r0, int64_t r1) {
  __shared__ float s_lds[POOL_MAX_ROWS];
  __shared__ float red[256];
  __shared__ __align__(16) float vred[1024];   // RG * VPR == 256 float4 slots
  const int tid = threadIdx.x;
  const int nrows = r1 > r0 ? (int)(r1 - r0) : 0;
  const float bc = p.bc ? p.bc[0] : 0.f;

  float lmax = -INFINITY;
  for (int i = tid; i < nrows; i += 256) {
    float s = bc;
    for (int t = 0; t < p.n_parts; ++t) s += p.s_part[(size_t)t * p.N + r0 + i];
    p.A_raw[r0 + i] = s;
    s_lds[i] = s;
    lmax = fmaxf(lmax, s);
  }
  lmax = wave_max(lmax);
  if ((tid & 63) == 0) red[tid >> 6] = lmax;
  __syncthreads();
  const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();

  const int VPR = p.H / 4;          // float4 per row: 64 (H=256), 128 (H=512), 256 (H=1024)
  const int RG = 256 / VPR;         // row groups processed concurrently
  const int cv = tid % VPR, rg = tid / VPR;
  float4 v = zero4();
  float lsum = 0.f;
  int i = rg;
  for (; i + 7 * RG < nrows; i += 8 * RG) {        // 8 independent row loads in flight (the loop is latency-bound)
    float4 hv[8];
    float e[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) hv[u] = ld4(p.h + (size_t)(r0 + i + u * RG) * p.H + 4 * cv);
#pragma unroll
    for (int u = 0; u < 8; ++u) e[u] = __expf(s_lds[i + u * RG] - m);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v.x += e[u] * hv[u].x; v.y += e[u] * hv[u].y; v.z += e[u] * hv[u].z; v.w += e[u] * hv[u].w;
      if (cv == 0) lsum += e[u];
    }
  }
  for (; i < nrows; i += RG) {
    float e = __expf(s_lds[i] - m);
    float4 hv = ld4(p.h + (size_t)(r0 + i) * p.H + 4 * cv);
    v.x += e * hv.x; v.y += e * hv.y; v.z += e * hv.z; v.w += e * hv.w;
    if (cv == 0) lsum += e;
  }
  st4(vred + (rg * VPR + cv) * 4, v);
  if (cv == 0) red[rg] = lsum;
  __syncthreads();
  float* out = p.partials + (size_t)g * (2 + p.H);
  if (tid < VPR) {
    float4 s = zero4();
    for (int q = 0; q < RG; ++q) {
      float4 t = ld4(vred + (q * VPR + tid) * 4);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    out[2 + 4 * tid + 0] = s.x; out[2 + 4 * tid + 1] = s.y;
    out[2 + 4 * tid + 2] = s.z; out[2 + 4 * tid + 3] = s.w;
  }
  if (tid == 0) {
    float l = 0.f;
    for (int q = 0; q < RG; ++q) l += red[q];
    out[0] = nrows > 0 ? m : -INFINITY;
    out[1] = l;
  }
}

__global__ __launch_bounds__(256) void pool_partial_kernel(PoolParams p) {
  const int g = blockIdx.x;
  const int64_t r0 = (int64_t)g * p.rows_per_group;
  const int64_t r1 = r0 + p.rows_per_group < p.N ? r0 + p.rows_per_group : p.N;
  pool_partial_rows(p, g, r0, r1);
}

// Head tail (HeadTail; head_tail_kernel below): the classifier, the hazards and -- when a label is given -- nll_surv
// with its backward down to dM, on 1024 threads.  Everything it needs that does not depend on M (classifier rows /
// columns, bias, label, censorship) is requested at kernel entry (TailPre): the tail is a chain of dependent steps,
// and each global load left inside it costs a memory round trip.
struct TailPre {
  float wk_row[16];   // wave k < K: Wk[k][lane + 64 j]        (H <= 1024)
  float wk_col[8];    // thread c < H: Wk[k][c], k < min(K, 8)
  float bk;           // lane 0 of wave k
  float c;            // thread 0
  long long y;        // thread 0
};
__device__ inline void tail_preload(const PoolParams& p, TailPre& r) {
  const HeadTail& t = p.tail;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < 16; ++j) r.wk_row[j] = (wave < t.K && lane + 64 * j < p.H) ? t.Wk[(size_t)wave * p.H + lane + 64 * j] : 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.wk_col[k] = (k < t.K && tid < p.H) ? t.Wk[(size_t)k * p.H + tid] : 0.f;
  r.bk = (wave < t.K && lane == 0) ? t.bk[wave] : 0.f;
  r.c = (tid == 0 && t.c) ? t.c[0] : 0.f;
  r.y = (tid == 0 && t.Y) ? (long long)t.Y[0] : 0;
}
// M_IN_LDS: the caller has merged the bag itself and left M in sm[0 .. H) (else M is read from p.M).  BWD = false is
// the forward-only tail: logits, hazards, S, Y_hat, risk and -- when Y is given -- the loss value, no dz / dM / dWk / dbk.
template <bool M_IN_LDS, bool BWD = true>
__device__ inline void head_tail(const PoolParams& p, const TailPre& r, float* sm /* 1024 + 160 floats */) {
  const HeadTail& t = p.tail;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = p.H, K = t.K;
  float* Ml = sm;                 // [H]
  float* z = sm + 1024;           // [K] logits, then dz
  float *hz = z + 32, *S = z + 64, *gH = z + 96, *gS = z + 128;   // K <= 32; in LDS: indexed arrays in registers would go to scratch
  if constexpr (!M_IN_LDS)        // M comes from the launch in front
    for (int c = tid; c < H; c += 1024) Ml[c] = p.M[c];
  __syncthreads();
  if (wave < K) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (lane + 64 * j < H) acc += Ml[lane + 64 * j] * r.wk_row[j];
    acc = wave_sum(acc);
    if (lane == 0) z[wave] = acc + r.bk;
  }
  for (int k = 16 + wave; k < K; k += 16) {          // K > 16: the rows that were not preloaded
    float acc = 0.f;
    for (int c = lane; c < H; c += 64) acc += Ml[c] * t.Wk[(size_t)k * H + c];
    acc = wave_sum(acc);
    if (lane == 0) z[k] = acc + t.bk[k];
  }
  __syncthreads();
  if (tid == 0) {
    // forward (surv_head_fwd_kernel) ...
    float run = 1.f, best = -INFINITY, ssum = 0.f;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      const float zz = z[k];
      hz[k] = 1.0f / (1.0f + expf(-zz));
      run *= (1.0f - hz[k]);
      S[k] = run;
      ssum += run;
      t.logits[k] = zz; t.hazards[k] = hz[k]; t.S[k] = run;
      if (zz > best) { best = zz; arg = k; }
    }
    t.Y_hat[0] = arg;
    if (t.risk) t.risk[0] = -ssum;
    if (t.Y) {
      // ... nll_surv for the one sample (nll_surv_kernel) ...
      if constexpr (BWD)
        for (int k = 0; k < K; ++k) { gH[k] = 0.f; gS[k] = 0.f; }
      const long long y64 = r.y;
      float l;
      if (y64 < 0 || y64 >= K) {
        l = __builtin_nanf("");
      } else {
        const int y = (int)y64;
        const float c = r.c;
        const float sp_y = y == 0 ? 1.0f : S[y - 1];
        const float hy = hz[y];
        const float unc = -(1.f - c) * (logf(fmaxf(sp_y, t.eps)) + logf(fmaxf(hy, t.eps)));
        const float sp_y1 = S[y];
        const float cen = -c * logf(fmaxf(sp_y1, t.eps));
        if constexpr (BWD) {
          if (y > 0 && sp_y >= t.eps) gS[y - 1] += -(1.f - c) / sp_y;
          if (hy >= t.eps) gH[y] += -(1.f - c) / hy;
          if (sp_y1 >= t.eps) gS[y] += -(1.f - t.alpha) * c / sp_y1;
        }
        l = (1.f - t.alpha) * (cen + unc) + t.alpha * unc;
      }
      t.loss[0] = l;
      // ... and the head's backward (surv_head_bwd_kernel): dz_t = (gH_t - sum_{j>=t} gS_j prod_{u<=j,u!=t}(1-h_u)) h_t (1-h_t)
      if constexpr (BWD)
        for (int k = 0; k < K; ++k) {
          float g = gH[k];
          for (int j = k; j < K; ++j) {
            float prod = 1.f;
            for (int u = 0; u <= j; ++u)
              if (u != k) prod *= (1.0f - hz[u]);
            g -= gS[j] * prod;
          }
          z[k] = g * hz[k] * (1.0f - hz[k]) * t.loss_scale;
        }
    }
  }
  if (!BWD || !t.Y) return;
  __syncthreads();
  for (int c = tid; c < H; c += 1024) {
    float acc = 0.f;
    if (c == tid) {                   // the preloaded columns (every c when H <= 1024)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < K) acc += z[k] * r.wk_col[k];
      for (int k = 8; k < K; ++k) acc += z[k] * t.Wk[(size_t)k * H + c];
    } else {
      for (int k = 0; k < K; ++k) acc += z[k] * t.Wk[(size_t)k * H + c];
    }
    t.dM[c] = acc;
    for (int k = 0; k < K; ++k) {
      float* o = t.dWk + (size_t)k * H + c;
      const float v = z[k] * Ml[c];
      *o = t.accumulate ? *o + v : v;
    }
  }
  if (tid < K) t.dbk[tid] = t.accumulate ? t.dbk[tid] + z[tid] : z[tid];
}

// H/32 workgroups of 1024 threads: merge the per-group partials.  The grouped routes merge one
// bag per workgroup instead (bag_merge below) and share this kernel's order of additions: the one-bag and the grouped
// forward-only passes agree to the bit (tests/test_gpu_pool_tails.py).
// Group weights exp(m_g - m) are computed once into LDS; the column sums then run as independent, unrolled
// loads (the first version's serial dependent loop over groups cost 115 us).
constexpr int MERGE_MAX_GROUPS = 4096;
__global__ __launch_bounds__(1024) void pool_merge_kernel(PoolParams p) {
  __shared__ float wl[MERGE_MAX_GROUPS];
  __shared__ float red[32];
  __shared__ float colred[1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int stride = 2 + p.H;
  float m = -INFINITY;
  for (int g = tid; g < p.n_groups; g += 1024) {
    float mg = p.partials[(size_t)g * stride];
    wl[g] = mg;
    m = fmaxf(m, mg);
  }
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
  float l = 0.f;
  for (int g = tid; g < p.n_groups; g += 1024) {
    float mg = wl[g];
    float w = mg > -INFINITY ? __expf(mg - m) : 0.f;
    wl[g] = w;
    l += p.partials[(size_t)g * stride + 1] * w;
  }
  l = wave_sum(l);
  if (lane == 0) red[16 + wave] = l;
  __syncthreads();
  l = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) l += red[16 + i];
  // Column sums: workgroup b owns columns 32 b .. 32 b + 31 (a single workgroup reading all n_groups x H partials
  // was bound by what one CU can pull: 264 KB = 10 us at 256 groups); its 1024 threads are 32 columns x 32 group
  // slices of independent loads.  m and l above are recomputed by every workgroup (2 floats per group).
  const int cl = tid & 31, sl = tid >> 5;
  const int c = blockIdx.x * 32 + cl;
  float acc = 0.f;
  const float* q = p.partials + 2 + c;
#pragma unroll 8
  for (int g = sl; g < p.n_groups; g += 32) acc += q[(size_t)g * stride] * wl[g];
  colred[tid] = acc;
  __syncthreads();
  if (tid < 32) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s += colred[i * 32 + tid];
    p.M[c] = s / l;
  }
  if (blockIdx.x == 0 && tid == 0) { p.stats[0] = m; p.stats[1] = l; }
}

// The head tail as its own single-workgroup launch behind K-merge (HeadTail).
// (First version: tail run by the LAST workgroup of K-merge, found with a ticket counter -- the fences, the atomic and
// the re-read of M through L2 cost 12 us, more than the 5 us of this launch.)
__global__ __launch_bounds__(1024) void head_tail_kernel(PoolParams p) {
  __shared__ float tail_sm[1024 + 160];
  TailPre pre;
  tail_preload(p, pre);
  head_tail<false>(p, pre, tail_sm);
}

// A[i] = sum_t s_part[t][i] + bc : the scores alone (standalone Attn_Net / Attn_Net_Gated forward, no pooling)
__global__ __launch_bounds__(256) void score_sum_kernel(const float* s_part, int n_parts, const float* bc, float* A, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float s = bc ? bc[0] : 0.f;
  for (int t = 0; t < n_parts; ++t) s += s_part[(size_t)t * N + i];
  A[i] = s;
}
int launch_score_sum(const float* s_part, int n_parts, const float* bc, float* A, int64_t N, hipStream_t st) {
  { ProfScope ps("score_sum_kernel", st);
    hipLaunchKernelGGL(score_sum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, s_part, n_parts, bc, A, N); }
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// =============================================================================================
// host launchers
// =============================================================================================
// a grid this short leaves every workgroup alone on its CU: nothing hides a memory round trip but deeper prefetch
bool short_grid(int64_t workgroups) {
  static const int env = tune_int("MMF_DEEP", 1);     // A/B switch
  static const int cap = tune_int("MMF_DEEP_MAX", 1024);   // tuning override (10k bag, 628 workgroups: 252 -> 242 us per step)
  return env && workgroups <= cap;
}

using TileNT128 = Tile<128, 128, 2, 2, true, true>;
using TileNT64 = Tile<64, 64, 2, 2, true, true>;

// rows-per-tile choice: big tiles once there is enough work to fill 256 CUs twice over
static inline bool use_big_tiles(int64_t M, int N) { return (M / 128) * ((N + 127) / 128) >= 256; }

// Wide tiles: (32*MB) x 256, ONE 8-wave workgroup per CU (wave w owns the 32-column strip w of every row).
// Measured (profiles/r01/load_rate.txt): a CU pulls ~11.5 B/clk of streamed and ~29 B/clk of L2-hot operand
// into LDS; two 128x128 workgroups per CU need 64 KB per 8192 MFMA cycles and stall on it.  A 224x256 tile
// needs 60 KB per 14336 MFMA cycles (60 FLOP/B instead of 32) and, at N = 50k, gives exactly 224 tiles.
template <int ROWS>
using TileW = Tile<ROWS, 256, 1, 8, true, true>;

// tile height that minimises rounds x blocks over the 256 CUs (0.35: per-tile prologue / epilogue, in 32-row blocks).
// Heights are the multiples of 16 from 64 to 240 rows; an odd multiple ends with a 16-row half block (Tile::HALF):
// 208 rows put a 50k bag on 241 CUs instead of 224, 96 rows a 24k bag on 250 instead of 188 (128 rows), 160 rows a 40k
// bag on 250 instead of 209 (192), 240 rows a 60k bag on 250 in ONE round instead of 289 tiles of 208 rows in two.
// 256 rows need > 256 VGPRs with double-buffered fragments (spills).
// concurrent (mmf_amil_desc::concurrent: other bags' kernels run beside this one): plan for 224 of the 256 CUs, which
// keeps the measured choice at 50k (224 tiles of 224 rows; 1376 vs 1337 bags/s with 208-row tiles and bags in flight)
// and, unlike the former "no half blocks when concurrent", does not push a 60k bag into two rounds of 224-row tiles.
int pick_wide_rows(int64_t M, int ntn, bool allow_half, bool concurrent, int max_rows) {
  static const int env = tune_int("MMF_WIDE_ROWS", 0);   // tuning override
  if (env > 0 && (env % 32 == 0 || allow_half)) return env;
  const int cus = concurrent ? 224 : 256;
  int best = 224;
  double bestc = 1e30;
  for (int rows = max_rows; rows >= 64; rows -= 16) {
    if (rows % 32 != 0 && !allow_half) continue;
    int64_t tiles = ((M + rows - 1) / rows) * ntn;
    int64_t rounds = (tiles + cus - 1) / cus;
    double c = (double)rounds * (rows / 32.0 + 0.35);
    if (c < bestc) { bestc = c; best = rows; }
  }
  return best;
}
bool use_wide_tiles(int64_t M, int N, int split) {
  static const int env = tune_int("MMF_WIDE", 1);
  static const int min_env = tune_int("MMF_WIDE_MIN", 0);   // tuning override
  // crossover against the 64-row tiles, one bag per step: exact fp32 16,384 rows (0.300 vs 0.329 ms there); the
  // split-operand tiles cross later -- 16,384: 0.307 wide vs 0.284 small, 24,000: 0.355 vs 0.412
  const int min_rows = min_env > 0 ? min_env : (split ? 80 * 256 : 64 * 256);
  return env && N % 256 == 0 && M * (int64_t)(N / 256) >= min_rows;
}

int split_min_rows() {
  // measured one bag per step, exact fp32 -> bf16x3: 1k 0.101 -> 0.096 ms, 2k 0.115 -> 0.106, 4,096 0.137 -> 0.127,
  // 6k 0.165 -> 0.140, 10k 0.235 -> 0.190, 14k 0.285 -> 0.235 (profiles/r02/d_split_sizes.txt): never slower.  Default 1:
  // every bag takes the split tiles, so that an instance's score does not depend on the size of the bag it is scored
  // in, bit for bit (heat-map batches of 512 patches vs the whole slide: tests/test_gpu_infer.py) -- the accumulation
  // order is the same on every split tile shape, but not between a split tile and an exact-fp32 one
  static const int env = tune_int("MMF_SPLIT_MIN", 1);   // tuning override
  return env;
}

// ---- the projection: one plan, one launcher ------------------------------------------------------------------------
// K split of the 64 x 64 projection tiles on short grids (LinearParams::ksplit).  A bag of 1,000 instances is 64 tiles, each
// a serial loop over 32 k-chunks (~25 us whatever the tile does: one MFMA block per wave and chunk), on 256 CUs; the radio
// head's reduce_dim (M = 512, K = 4 x 1024) is 128 tiles of 128 chunks.  Split S ways they are S times as many workgroups with
// loops 1 / S as long; the partial tiles (S x M x N floats) cross L2 / Infinity Cache once each way.
LinearPlan plan_linear(int64_t M, int N, int K, int nseg, int kseg, int allow_half, int concurrent, int split, int tick_words) {
  static const int max_wg = tune_int("MMF_KSPLIT_MAX_WG", 512);     // tuning override: 0 = never split
  // measured (round 4, path bags, projection kernel us unsplit -> split): 512 rows 25.4 -> 23.2, 1,000 26.4 -> 20.3, 2,000
  // 26.5 -> 24.5, 4,096 (256 tiles, two ways) 26.4 -> 29.3: from one tile per CU on, splitting only adds the partial traffic
  static const int max_tiles = tune_int("MMF_KSPLIT_MAX_TILES", 128);
  static const int deep_seg = tune_int("MMF_DEEP_SEG", 1);      // A/B switch: deep prefetch for segmented inputs too
  LinearPlan pl{};
  pl.kind = LIN_64; pl.rows = 64; pl.ksplit = 1;
  if (M <= 0) return pl;
  const bool can_split = split && K % (4 * SKC) == 0 && nseg == 1;
  if (can_split && use_wide_tiles(M, N, 1)) {
    pl.kind = LIN_SPLIT_WIDE; pl.rows = 224;
  } else if (use_wide_tiles(M, N, can_split)) {      // a height no tile is compiled for (an override's) runs as 224 rows
    const int r = pick_wide_rows(M, N / 256, allow_half != 0, concurrent != 0, 240);
    pl.kind = LIN_WIDE; pl.rows = r >= 64 && r <= 240 && r % 16 == 0 ? r : 224;
  } else if (!can_split && use_big_tiles(M, N)) {
    pl.kind = LIN_128; pl.rows = 128;
  } else if (can_split && M >= split_min_rows()) {
    pl.kind = LIN_SPLIT_64;
  }
  const int bn = pl.kind == LIN_SPLIT_WIDE || pl.kind == LIN_WIDE ? 256 : pl.rows;
  pl.mt_count = (int)((M + pl.rows - 1) / pl.rows); pl.nt_count = (N + bn - 1) / bn;
  const int64_t tiles = (int64_t)pl.mt_count * pl.nt_count;
  const int nk = K / KC;
  const bool seg_deep = nseg == 1 || kseg % (4 * KC) == 0;      // a segment boundary never falls inside a four-chunk step
  if (pl.kind == LIN_64) {
    if (tiles <= tick_words && tiles <= max_tiles && N % 4 == 0 && K % KC == 0 && seg_deep)
      for (int S = 4; S >= 2 && pl.ksplit == 1; S -= 2)
        if (tiles * S <= max_wg && nk % (4 * S) == 0 && nk / S >= 8) pl.ksplit = S;
    if (pl.ksplit > 1) {
      pl.kind = LIN_KSPLIT_64;
      pl.deep = short_grid(tiles * pl.ksplit) ? 1 : 0;        // (K / KC / S) % 4 == 0 by the rule above
      pl.kpart_floats = pl.ksplit * (int)tiles * 64 * 64;
    } else {
      pl.deep = short_grid(tiles) && nk % 4 == 0 && (nseg == 1 || (deep_seg && seg_deep)) ? 1 : 0;
    }
  }
  pl.grid = grid_for_tiles(pl.mt_count, pl.nt_count * pl.ksplit);
  return pl;
}
size_t linear_ksplit_floats(int64_t M, int N, int K, int nseg, int kseg) {
  return (size_t)plan_linear(M, N, K, nseg, kseg, 0, 0, 0, 0x7fffffff).kpart_floats;
}

// SEG: the grouped step's projection (ReLU + dropout with per-bag masks, fp32 mode only); the plan is the same
template <bool SEG>
static int launch_linear_impl(LinearParams p, hipStream_t st) {
  if (p.K % KC != 0 || (p.nseg > 1 && p.kseg % KC != 0)) return MMF_ERR_SHAPE;
  if (p.N % 4 != 0) return MMF_ERR_SHAPE;     // linear_epilogue: float4 stores of y and loads of the bias, never across the edge
  if (p.ldx % 4 != 0) return MMF_ERR_ALIGN;
  if (p.M <= 0) return MMF_OK;
  const LinearPlan pl = plan_linear(p.M, p.N, p.K, p.nseg, p.kseg, p.allow_half, p.concurrent, p.split,
                                    p.kpart && p.ktick ? p.ktick_words : 0);
  p.mt_count = pl.mt_count; p.nt_count = pl.nt_count; p.ksplit = pl.ksplit; p.deep = pl.deep;
  auto go = [&](auto tile) -> int {
    using T = decltype(tile);
    void (*kern)(LinearParams);       // the split-operand tiles have no grouped form: launch_linear_seg refuses them
    if constexpr (T::SPLIT) kern = linear_nt_split_kernel<T>; else kern = linear_nt_kernel<T, SEG>;
    return launch_tiled<T>(T::SPLIT ? "linear_nt_split_kernel" : "linear_nt_kernel", kern, p, pl.grid, st);
  };
  switch (pl.kind) {
    case LIN_SPLIT_WIDE: return go(TileSp<224, 256, 1, 8>{});
    case LIN_SPLIT_64: return go(TileSp<64, 64, 2, 2>{});
    case LIN_128: return go(TileNT128{});
    case LIN_KSPLIT_64:
    case LIN_64: return go(TileNT64{});
    case LIN_WIDE: return with_wide_rows<240>(pl.rows, [&](auto r) { return go(TileW<decltype(r)::value>{}); });
  }
  return MMF_ERR_ARG;
}

int launch_linear(LinearParams p, hipStream_t st) { return launch_linear_impl<false>(p, st); }
int launch_linear_seg(LinearParams p, hipStream_t st) {
  if (!p.seg_ridx || p.split || p.act != ACT_RELU) return MMF_ERR_ARG;
  return p.drop_p > 0.f ? launch_linear_impl<true>(p, st) : launch_linear_impl<false>(p, st);
}

// ---- the gate forward: one plan, one launcher ------------------------------------------------------------------------
// one s_part row per attention-dim tile: BN = 128 always (64 gated dims, or 128 ungated dims, per tile), whatever the bag size
int gate_parts(int D, int gated) { return gated ? (D + 63) / 64 : (D + 127) / 128; }

GatePlan plan_gate_fwd(int64_t N, int H, int D, int gated, int split) {
  // 128-row tiles only once they fill most of the 512 slots (two workgroups per CU): a 10k bag is 316 tall tiles -- every
  // CU busy for a tall tile's time, 60 of them twice -- or 628 short ones in 1.2 rounds: measured 40.6 vs 35.1 us (round 4,
  // DESIGN.md §5, profiles/r04/d_mid_size_knobs.txt; 12,288 rows: 40.3 vs 35.3; from 12,800 rows the tall tiles win, 14k: 41.0 vs 44.0)
  static const int big_min = tune_int("MMF_GATE_BIG_MIN", 400);
  static const int env_gate = tune_int("MMF_GATE_MIXED", -1);   // A/B switch
  GatePlan pl{};
  pl.kind = GATE_64; pl.nt_count = gate_parts(D, gated);
  if (N <= 0) return pl;
  const bool split_k = split && H % (4 * SKC) == 0;
  if ((N / 128) * pl.nt_count < big_min) {
    pl.split = split_k && N >= split_min_rows(); pl.mt_count = (int)((N + 63) / 64);
    pl.deep = !pl.split && short_grid((int64_t)pl.mt_count * pl.nt_count) && (H / KC) % 4 == 0 ? 1 : 0;
    pl.grid = grid_for_tiles(pl.mt_count, pl.nt_count);
    return pl;
  }
  // 128x128 tiles run two per CU: 512 slots.  Two things cost this launch time: a sparse last round (a 50k bag is
  // 1564 tiles = 3 rounds + 28 tiles, which cost most of a 4th round: 132 us against 116 us for the 1536 tiles of
  // 49,152 rows) and the two workgroups of a CU running IN PHASE -- both in their main loops, then both in their
  // epilogues (tanh / sigmoid pairs, 64 KB of a, b stores each) with the MFMA pipe idle.  Both are answered by the
  // ORDER and the HEIGHT of the tiles in one launch (workgroups start in block order as slots free up; the first 512
  // start at once, the dispatcher placing one per CU before the second):
  //   A  256 tall tiles          -> slot 1 of every CU, finishing at T, 2T, 3T ...
  //   B  256 short (64-row) ones -> slot 2, finishing at T/2: from here on slot 2 runs half a tile out of phase
  //   C  256 (2R - 2) tall tiles -> taken alternately by slot 2 (at T/2, 3T/2, ...) and slot 1 (at T, 2T, ...)
  //   D  256 short tiles         -> slot 2's last, so that both slots end at R T
  //   E  the remaining rows as short tiles (twice as many CUs work on them, each for half the time)
  // R = whole rounds of 512 tall tiles in the bag.  MMF_GATE_MIXED=2: A + E only (the first version of this: 133 -> 128 us).
  // split-operand tiles: their main loop is short against their epilogue, and the out-of-phase plan's extra short tiles
  // cost more than the phase offset wins (A + E only: 91.2 us; dephased: 96.4; uniform tiles: 94.5)
  pl.split = split_k;
  const int mixed = env_gate >= 0 ? env_gate : (split_k ? 2 : 1);
  const int64_t mt = (N + 127) / 128, slots = 512, total = mt * pl.nt_count;
  const int R = (int)(total / slots);
  if (!mixed || R < 2 || slots % (2 * pl.nt_count) != 0) {
    pl.kind = GATE_128; pl.mt_count = (int)mt;
    pl.grid = grid_for_tiles(pl.mt_count, pl.nt_count);
    return pl;
  }
  pl.kind = GATE_MIXED;
  const int half_m = (int)(slots / 2 / pl.nt_count);          // m-tiles in a wave of 256 workgroups
  int64_t row = 0;
  auto region = [&](int tall, int64_t m_tiles) {
    if (m_tiles <= 0) return;
    pl.reg[pl.nreg++] = {(int)row, (int)m_tiles, pl.grid, tall};
    pl.grid += grid_for_tiles((int)m_tiles, pl.nt_count);
    pl.mt_count += (int)m_tiles;
    row += m_tiles * (tall ? 128 : 64);
  };
  if (mixed == 2) {
    region(1, (total - total % slots) / pl.nt_count);
  } else {
    region(1, half_m);
    region(0, half_m);
    region(1, (int64_t)half_m * (2 * R - 2));
    region(0, half_m);
  }
  region(0, (N - row + 63) / 64);
  return pl;
}

template <bool SEG>
static int launch_gate_fwd_impl(GateFwdParams p, hipStream_t st) {
  if (p.H % KC != 0 || p.D % 32 != 0) return MMF_ERR_SHAPE;
  if (p.N <= 0) return MMF_OK;
  const GatePlan pl = plan_gate_fwd(p.N, p.H, p.D, p.gated, p.split);
  p.nt_count = pl.nt_count; p.mt_count = pl.mt_count; p.deep = pl.deep; p.nreg = pl.nreg;
  p.row_begin = 0; p.row_end = p.N;
  for (int i = 0; i < pl.nreg; ++i) p.reg[i] = {pl.reg[i].row0, pl.reg[i].mt_count, pl.reg[i].grid_begin, pl.reg[i].tall};
  // ts: the short tile of a mixed launch, of tb's thread count and column width.  The split-operand tiles have no grouped
  // form: launch_gate_fwd_seg refuses them.
  auto go = [&](auto tb, auto... ts) -> int {
    using TB = decltype(tb);
    constexpr bool S = SEG && !TB::SPLIT;
    void (*kern)(GateFwdParams);
    if constexpr (sizeof...(ts) == 0) kern = p.gated ? gate_fwd_kernel<TB, true, S> : gate_fwd_kernel<TB, false, S>;
    else kern = p.gated ? gate_fwd_mixed_kernel<TB, decltype(ts)..., true, S> : gate_fwd_mixed_kernel<TB, decltype(ts)..., false, S>;
    return launch_tiled<TB>(TB::SPLIT ? "gate_fwd_split_kernel" : "gate_fwd_kernel", kern, p, pl.grid, st);
  };
  using TS = Tile<64, 128, 2, 2, true, true>;
  using SB = TileSp<128, 128, 2, 2>;
  using SS = TileSp<64, 128, 2, 2>;
  switch (pl.kind) {
    case GATE_64: return pl.split ? go(SS{}) : go(TS{});
    case GATE_128: return pl.split ? go(SB{}) : go(TileNT128{});
    case GATE_MIXED: return pl.split ? go(SB{}, SS{}) : go(TileNT128{}, TS{});
  }
  return MMF_ERR_ARG;
}

int launch_gate_fwd(GateFwdParams p, hipStream_t st) { return launch_gate_fwd_impl<false>(p, st); }
int launch_gate_fwd_seg(GateFwdParams p, hipStream_t st) {
  if (!p.seg_ridx || p.split) return MMF_ERR_ARG;
  return p.drop_p > 0.f ? launch_gate_fwd_impl<true>(p, st) : launch_gate_fwd_impl<false>(p, st);
}

int pool_groups(int64_t N) {
  // one 4-wave workgroup per CU: the partial kernel streams h at ~5 TB/s with 256, 512 or 1024 groups alike
  // (measured), and the merge reads one partial per group
  static const int cap = tune_int("MMF_POOL_GROUPS", 256);   // tuning override
  int64_t g = (N + 63) / 64;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  while ((N + g - 1) / g > POOL_MAX_ROWS) g *= 2;
  return (int)g;
}

int launch_pool(PoolParams p, hipStream_t st) {
  if (p.H != 256 && p.H != 512 && p.H != 1024) return MMF_ERR_SHAPE;
  p.n_groups = pool_groups(p.N);
  p.rows_per_group = (int)((p.N + p.n_groups - 1) / p.n_groups);
  if (p.rows_per_group > POOL_MAX_ROWS) return MMF_ERR_SHAPE;
  { ProfScope ps("pool_partial_kernel", st); hipLaunchKernelGGL(pool_partial_kernel, dim3(p.n_groups), dim3(256), 0, st, p); }
  return launch_pool_merge(p, st);
}

int launch_pool_merge(PoolParams p, hipStream_t st) {
  if (p.n_groups < 1 || p.n_groups > MERGE_MAX_GROUPS || p.H > 1024 || p.H % 32 != 0) return MMF_ERR_SHAPE;
  if (p.tail.Wk && (p.tail.K < 1 || p.tail.K > 32)) return MMF_ERR_SHAPE;
  // Always a merge launch of its own.  Letting the single-workgroup tail kernel merge a bag of <= 64 partials saved a
  // launch and lost more than that: measured, one bag per step, separate merge vs merge in the tail: 1k 0.0995 vs
  // 0.1016 ms, 2k 0.1085 vs 0.1146, 4,096 (64 groups) 0.1236 vs 0.1370.
  {
    ProfScope ps("pool_merge_kernel", st);
    hipLaunchKernelGGL(pool_merge_kernel, dim3(p.H / 32), dim3(1024), 0, st, p);
  }
  if (p.tail.Wk) {
    ProfScope ps("head_tail_kernel", st);
    hipLaunchKernelGGL(head_tail_kernel, dim3(1), dim3(1024), 0, st, p);
  }
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// The head tail on a feature vector that is already there (p.M [p.H <= 1024]; the multimodal step: the branches' embeddings
// side by side): classifier, hazards, nll_surv and its backward down to d(feature), one single-workgroup launch.
int launch_head_tail(PoolParams p, hipStream_t st) {
  if (!p.M || !p.tail.Wk || p.H < 1 || p.H > 1024 || p.tail.K < 1 || p.tail.K > 32) return MMF_ERR_SHAPE;
  ProfScope ps("head_tail_kernel", st);
  hipLaunchKernelGGL(head_tail_kernel, dim3(1), dim3(1024), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

}  // namespace mmf

// =============================================================================================
// Grouped step (mmf_amil_nll_step_group): the per-row segment tables, pooling per bag, merge + head tail per bag
// =============================================================================================
namespace mmf {

// row -> bag, and the bag-local dropout index base of the row for the H-wide (h) and D-wide (a, b) mask sites
__global__ __launch_bounds__(256) void group_rows_kernel(GroupRowsParams p) {
  __shared__ int64_t off[GROUP_MAX + 1];
  const int G = p.s.G;
  for (int i = threadIdx.x; i <= G; i += 256) off[i] = p.s.off[i];
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= off[G]) return;
  int lo = 0, hi = G - 1;                  // last bag whose first row is <= row
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= row) lo = mid; else hi = mid - 1;
  }
  const uint32_t local = (uint32_t)(row - off[lo]), base = p.s.ibase[lo];
  p.ridx_h[row] = local * (uint32_t)p.H + base;
  p.ridx_d[row] = local * (uint32_t)p.D + base;
  p.bag[row] = lo;
}

int launch_group_rows(const GroupRowsParams& p, hipStream_t st) {
  const int64_t R = p.s.off[p.s.G];
  ProfScope ps("group_rows_kernel", st);
  hipLaunchKernelGGL(group_rows_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// partial group b of the window: the rows of one bag only
__global__ __launch_bounds__(256) void group_pool_partial_kernel(PoolParams p, SegTable s) {
  const int b = blockIdx.x;
  int g = 0;
  for (int i = 1; i < s.G; ++i)            // wave-uniform: scalar loads of the table
    if (b >= s.gbeg[i]) g = i;
  const int64_t r0 = s.off[g] + (int64_t)(b - s.gbeg[g]) * s.rows_per_group;
  const int64_t r1 = r0 + s.rows_per_group < s.off[g + 1] ? r0 + s.rows_per_group : s.off[g + 1];
  pool_partial_rows(p, b, r0, r1);
}

constexpr int GROUP_BAG_MAX_PARTIALS = GROUP_POOL_GROUPS + 64;

// One bag's merge on one 1024-thread workgroup: the n partials at `part` -> m, l (every thread) and, returned, column
// tid of M (threads tid < H; 0 on the others).  wl [GROUP_BAG_MAX_PARTIALS] and red [32] are the caller's LDS.  The
// column sums take pool_merge_kernel's order: 32 interleaved slices, then the slices in order.
__device__ __forceinline__ float bag_merge(const float* part, int n, int H, float* wl, float* red, float& m, float& l) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int stride = 2 + H;
  m = -INFINITY;
  for (int i = tid; i < n; i += 1024) m = fmaxf(m, part[(size_t)i * stride]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
  l = 0.f;
  for (int i = tid; i < n; i += 1024) {
    const float mg = part[(size_t)i * stride];
    const float w = mg > -INFINITY ? __expf(mg - m) : 0.f;
    wl[i] = w;
    l += part[(size_t)i * stride + 1] * w;
  }
  l = wave_sum(l);
  if (lane == 0) red[16 + wave] = l;
  __syncthreads();
  l = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) l += red[16 + i];
  float mv = 0.f;
  if (tid < H) {
    const float* col = part + 2 + tid;
    float acc = 0.f;
    for (int sl = 0; sl < 32; ++sl) {
      float a = 0.f;
      for (int i = sl; i < n; i += 32) a += col[(size_t)i * stride] * wl[i];
      acc += a;
    }
    mv = acc / l;
  }
  return mv;
}

// Bag g's slice of every per-bag array of a window's PoolParams / HeadTail; ldm is the row stride of M (H, or the
// width of a wider feature matrix).  Optional pointers that are null stay null; the gradient slabs are per bag, so
// accumulate is off (the reduce launch behind sums them over the bags).
__device__ __forceinline__ PoolParams bag_slice(const PoolParams& p, int g, int ldm) {
  PoolParams q = p;
  const int H = p.H, K = p.tail.K;
  if (q.M) q.M += (size_t)g * ldm;
  if (q.stats) q.stats += 2 * g;
  HeadTail& t = q.tail;
  t.logits += (size_t)g * K; t.hazards += (size_t)g * K; t.S += (size_t)g * K; t.Y_hat += g;
  if (t.risk) t.risk += g;
  if (t.Y) t.Y += g;
  if (t.c) t.c += g;
  if (t.loss) t.loss += g;
  if (t.dM) t.dM += (size_t)g * H;
  if (t.dWk) t.dWk += (size_t)g * K * H;
  if (t.dbk) t.dbk += (size_t)g * K;
  t.accumulate = 0;
  return q;
}

// one workgroup per bag: merge the bag's partials (M_g, stats_g), then the head tail of that bag
__global__ __launch_bounds__(1024) void group_tail_kernel(PoolParams p, SegTable s) {
  __shared__ float tail_sm[1024 + 160];
  __shared__ float wl[GROUP_BAG_MAX_PARTIALS];
  __shared__ float red[32];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int gb = s.gbeg[g], n = s.gbeg[g + 1] - gb, H = p.H;
  const PoolParams q = bag_slice(p, g, H);
  TailPre pre;
  tail_preload(q, pre);
  float m, l;
  const float mv = bag_merge(p.partials + (size_t)gb * (2 + H), n, H, wl, red, m, l);
  if (tid < H) {
    q.M[tid] = mv;
    tail_sm[tid] = mv;
  }
  if (tid == 0) { q.stats[0] = m; q.stats[1] = l; }
  head_tail<true>(q, pre, tail_sm);
}

// What every pooling launch over a window checks: H of the pooling kernels, the window's size, the rows of a partial
// group, and no bag with more partials than one workgroup merges.
int group_pool_check(const PoolParams& p, const SegTable& s) {
  if (p.H != 256 && p.H != 512 && p.H != 1024) return MMF_ERR_SHAPE;
  if (s.G < 1 || s.G > GROUP_MAX || s.rows_per_group < 1 || s.rows_per_group > POOL_MAX_ROWS) return MMF_ERR_SHAPE;
  for (int g = 0; g < s.G; ++g)
    if (s.gbeg[g + 1] - s.gbeg[g] > GROUP_BAG_MAX_PARTIALS) return MMF_ERR_SHAPE;
  return MMF_OK;
}

int launch_group_pool_partial(PoolParams p, const SegTable& s, hipStream_t st) {
  if (int e = group_pool_check(p, s)) return e;
  ProfScope ps("group_pool_partial_kernel", st);
  hipLaunchKernelGGL(group_pool_partial_kernel, dim3(s.gbeg[s.G]), dim3(256), 0, st, p, s);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

int launch_group_pool(PoolParams p, const SegTable& s, hipStream_t st) {
  if (!p.tail.Wk || p.tail.K < 1 || p.tail.K > 32) return MMF_ERR_SHAPE;
  if (int e = launch_group_pool_partial(p, s, st)) return e;
  ProfScope ps("group_tail_kernel", st);
  hipLaunchKernelGGL(group_tail_kernel, dim3(s.G), dim3(1024), 0, st, p, s);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// ---- grouped multimodal step (mmf_amil_group_forward / _backward, mmf_surv_head_nll_step_group) ---------------------
// One workgroup per bag: group_tail_kernel's merge (bag_merge) without the head tail behind it.  M_g goes to the caller's
// M + g * ldm -- a stack writes straight into its columns of the window's [G x F] feature matrix -- and, with stats_g,
// to the workspace (Mw [G x H], p.stats [G x 2]), where the backward half reads them.
__global__ __launch_bounds__(1024) void group_merge_kernel(PoolParams p, SegTable s, int ldm, float* Mw) {
  __shared__ float wl[GROUP_BAG_MAX_PARTIALS];
  __shared__ float red[32];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int gb = s.gbeg[g], n = s.gbeg[g + 1] - gb, H = p.H;
  float m, l;
  const float mv = bag_merge(p.partials + (size_t)gb * (2 + H), n, H, wl, red, m, l);
  if (tid < H) {
    p.M[(size_t)g * ldm + tid] = mv;
    Mw[(size_t)g * H + tid] = mv;
  }
  if (tid == 0) { p.stats[2 * g] = m; p.stats[2 * g + 1] = l; }
}

int launch_group_merge(PoolParams p, const SegTable& s, int ldm, float* Mw, hipStream_t st) {
  if (int e = group_pool_check(p, s)) return e;
  if (ldm < p.H || !p.M || !Mw || !p.stats) return MMF_ERR_SHAPE;
  ProfScope ps("group_merge_kernel", st);
  hipLaunchKernelGGL(group_merge_kernel, dim3(s.G), dim3(1024), 0, st, p, s, ldm, Mw);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// dst [G x H] <- the H columns of src [G x ld] that belong to one stack: the backward half's dM, which K-prep and K-dh
// read as one [G x H] block
__global__ __launch_bounds__(256) void group_dm_gather_kernel(const float* src, int ld, float* dst, int G, int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= G * H) return;
  const int g = i / H, c = i - g * H;
  dst[i] = src[(size_t)g * ld + c];
}
int launch_group_dm_gather(const float* src, int ld, float* dst, int G, int H, hipStream_t st) {
  if (!src || !dst || G < 1 || G > GROUP_MAX || H < 1 || ld < H) return MMF_ERR_SHAPE;
  ProfScope ps("group_dm_gather_kernel", st);
  hipLaunchKernelGGL(group_dm_gather_kernel, dim3((G * H + 255) / 256), dim3(256), 0, st, src, ld, dst, G, H);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// The hazard head of a window: one workgroup per patient g over feat [G x ldf] -- head_tail (the one-patient step's
// device code, head_tail_kernel) on row g: classifier, sigmoid, cumprod, argmax, risk, nll_surv and its backward.  The
// per-patient arrays of p.tail are G long; tail.dM is dfeat [G x F]; tail.dWk / dbk are per-patient slabs [G x K x F],
// [G x K] (dbk_g = dlogits_g), overwritten: the reduce launch behind sums them in patient order.
__global__ __launch_bounds__(1024) void surv_head_group_kernel(PoolParams p, int ldf) {
  __shared__ float tail_sm[1024 + 160];
  const PoolParams q = bag_slice(p, blockIdx.x, ldf);
  TailPre pre;
  tail_preload(q, pre);
  head_tail<false>(q, pre, tail_sm);
}

int launch_surv_head_group(PoolParams p, int ldf, int G, hipStream_t st) {
  if (!p.M || !p.tail.Wk || !p.tail.Y || !p.tail.dM || !p.tail.dWk || !p.tail.dbk) return MMF_ERR_ARG;
  if (p.H < 1 || p.H > 1024 || ldf < p.H || p.tail.K < 1 || p.tail.K > 32 || G < 1 || G > GROUP_MAX) return MMF_ERR_SHAPE;
  ProfScope ps("surv_head_group_kernel", st);
  hipLaunchKernelGGL(surv_head_group_kernel, dim3(G), dim3(1024), 0, st, p, ldf);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// The hazard head of a window, forward only (mmf_surv_head_infer_group): one workgroup per patient, whose feature row is
// the concatenation of row g of up to three dense [G x width] buffers -- the branch embeddings of the concat fusion where
// the stacks left them (torch.cat of models/model_mm_attention_mil.py:168-187 is never a launch), or `hid` of the tensor
// fusion.  The row is gathered into LDS and head_tail runs on it with its backward compiled out: logits, hazards, S,
// Y_hat, risk and -- with labels -- the loss value.
__global__ __launch_bounds__(1024) void surv_head_infer_group_kernel(PoolParams p, HeadSegs s) {
  __shared__ float tail_sm[1024 + 160];
  const int g = blockIdx.x, tid = threadIdx.x;
  const PoolParams q = bag_slice(p, g, 0);            // p.M is null: the row comes from the segments
  TailPre pre;
  tail_preload(q, pre);
  int off = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (i < s.n) {
      for (int c = tid; c < s.width[i]; c += 1024) tail_sm[off + c] = s.x[i][(size_t)g * s.width[i] + c];
      off += s.width[i];
    }
  }
  head_tail<true, false>(q, pre, tail_sm);
}

int launch_surv_head_infer_group(PoolParams p, const HeadSegs& s, int G, hipStream_t st) {
  if (!p.tail.Wk || p.M) return MMF_ERR_ARG;
  if (s.n < 1 || s.n > 3 || p.tail.K < 1 || p.tail.K > 32 || G < 1 || G > GROUP_MAX) return MMF_ERR_SHAPE;
  int F = 0;
  for (int i = 0; i < s.n; ++i) {
    if (!s.x[i]) return MMF_ERR_ARG;
    if (s.width[i] < 1 || s.width[i] > 1024) return MMF_ERR_SHAPE;
    F += s.width[i];
  }
  if (F != p.H || F > 1024) return MMF_ERR_SHAPE;
  ProfScope ps("surv_head_infer_group_kernel", st);
  hipLaunchKernelGGL(surv_head_infer_group_kernel, dim3(G), dim3(1024), 0, st, p, s);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// ---- forward-only grouped pass (mmf_amil_infer_group) ----------------------------------------------------------------
// One workgroup per bag: group_tail_kernel with the forward-only head tail -- merge the bag's partials into M_g (written
// when p.M is given), then the classifier, hazards, S, Y_hat, risk and -- when labels are given -- the bag's nll_surv
// value.  No dM, no classifier gradient.  Without a head (p.tail.Wk null) it is the merge alone.
__global__ __launch_bounds__(1024) void group_infer_tail_kernel(PoolParams p, SegTable s) {
  __shared__ float tail_sm[1024 + 160];
  __shared__ float wl[GROUP_BAG_MAX_PARTIALS];
  __shared__ float red[32];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int gb = s.gbeg[g], n = s.gbeg[g + 1] - gb, H = p.H;
  const PoolParams q = bag_slice(p, g, H);
  TailPre pre;
  if (q.tail.Wk) tail_preload(q, pre);
  float m, l;
  const float mv = bag_merge(p.partials + (size_t)gb * (2 + H), n, H, wl, red, m, l);
  if (tid < H) {
    if (q.M) q.M[tid] = mv;
    tail_sm[tid] = mv;
  }
  if (!q.tail.Wk) return;
  head_tail<true, false>(q, pre, tail_sm);
}

int launch_group_infer_tail(PoolParams p, const SegTable& s, hipStream_t st) {
  if (int e = group_pool_check(p, s)) return e;
  if (p.tail.Wk && (p.tail.K < 1 || p.tail.K > 32)) return MMF_ERR_SHAPE;
  ProfScope ps("group_infer_tail_kernel", st);
  hipLaunchKernelGGL(group_infer_tail_kernel, dim3(s.G), dim3(1024), 0, st, p, s);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// ---- integrated gradients (mmf_amil_ig) -------------------------------------------------------------------------------
// With a zero baseline the projection is linear in the interpolation factor: relu(alpha_s x W1^T + b1) = relu(alpha_s U +
// b1), U = x W1^T computed once.  One wave per 16 x 32 block of the window's [S * N x H] rows: lane 8 rr + c4 takes rows
// rr, rr + 8 and columns 4 c4 .. 4 c4 + 3, K-lin's epilogue lanes, so the ballots are LinearParams::relu_bits words.
__global__ __launch_bounds__(256) void ig_expand_kernel(IgExpandParams p) {
  __shared__ float al[GROUP_MAX];
  for (int i = threadIdx.x; i < p.st.S; i += 256) al[i] = p.st.alpha[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rr = lane >> 3, c4 = lane & 7;
  const int64_t R = (int64_t)p.st.S * p.N, rb16 = blockIdx.x;
  const int cbn = p.H >> 5;
  bool ok[2];
  float a[2];
  const float* u[2];
  float* y[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int64_t row = rb16 * 16 + rr + 8 * t;
    ok[t] = row < R;
    const int s = ok[t] ? (int)(row / p.N) : 0;
    a[t] = al[s];
    u[t] = p.U + (size_t)(row - (int64_t)s * p.N) * p.H;
    y[t] = p.h + (size_t)row * p.H;
  }
  for (int cb = wave; cb < cbn; cb += 4) {
    const int col = cb * 32 + 4 * c4;
    const float4 b4 = ld4(p.b1 + col);
    unsigned long long mine = 0ull;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (ok[t]) {
        const float4 u4 = ld4(u[t] + col);
        v[0] = fmaxf(fmaf(a[t], u4.x, b4.x), 0.f); v[1] = fmaxf(fmaf(a[t], u4.y, b4.y), 0.f);
        v[2] = fmaxf(fmaf(a[t], u4.z, b4.z), 0.f); v[3] = fmaxf(fmaf(a[t], u4.w, b4.w), 0.f);
        st4(y[t] + col, make_float4(v[0], v[1], v[2], v[3]));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned long long bal = __ballot(ok[t] && v[e] > 0.f);
        if (lane == 4 * t + e) mine = bal;
      }
    }
    if (lane < 8) p.relu_bits[((size_t)rb16 * cbn + cb) * 8 + lane] = mine;
  }
}

int launch_ig_expand(const IgExpandParams& p, hipStream_t st) {
  if (!p.U || !p.b1 || !p.h || !p.relu_bits) return MMF_ERR_ARG;
  if (p.H % 32 != 0 || p.N < 1 || p.st.S < 1 || p.st.S > GROUP_MAX) return MMF_ERR_SHAPE;
  const int64_t R = (int64_t)p.st.S * p.N;
  ProfScope ps("ig_expand_kernel", st);
  hipLaunchKernelGGL(ig_expand_kernel, dim3((unsigned)((R + 15) / 16)), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// The radiology head (mmf_radio_ig): reduce_dim's bias passes through the projection once per call, out[j] = b1[j] +
// sum_l W1[j, l] br[l].  One wave per output, four outputs per workgroup: lane t adds its products l = t, t + 64, ... in
// that order (ceil(L / 64) fused multiply-adds), the xor butterfly adds the 64 lanes (6), then b1 -- a dependent chain of
// ceil(L / 64) + 7 additions, the same in every call; no atomics.
__global__ __launch_bounds__(256) void ig_bias_kernel(const float* W1, const float* br, const float* b1, float* out,
                                                      int H, int L) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= H) return;
  float t = 0.f;
  for (int l = lane; l < L; l += 64) t = fmaf(W1[(size_t)j * L + l], br[l], t);
  t = wave_sum(t);
  if (lane == 0) out[j] = t + b1[j];
}

int launch_ig_bias(const float* W1, const float* br, const float* b1, float* out, int H, int L, hipStream_t st) {
  if (!W1 || !br || !b1 || !out) return MMF_ERR_ARG;
  if (H < 1 || L < 1) return MMF_ERR_SHAPE;
  ProfScope ps("ig_bias_kernel", st);
  hipLaunchKernelGGL(ig_bias_kernel, dim3((unsigned)((H + 3) / 4)), dim3(256), 0, st, W1, br, b1, out, H, L);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// The hazard head of models/model_attention_mil_path.py:58-61 on a step's pooled embedding and the gradient of
// risk = -sum_k S_k back to it: the head and d risk / d logits are ig_hazard_body (mmf_ig_head.h), the one body the
// tensor fusion's node kernel shares; this launch takes the logits' gradient on to the embedding.
__global__ __launch_bounds__(256) void ig_head_kernel(IgHeadParams p) {
  __shared__ float lg[32], hz[32], sv[32], dl[32];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int H = p.H, K = p.K;
  ig_hazard_body<4>(p, p.M + (size_t)s * H, s, lg, hz, sv, dl);
  for (int c = tid; c < H; c += 256) {
    float t = 0.f;
    for (int j = 0; j < K; ++j) t += dl[j] * p.Wk[(size_t)j * H + c];
    p.dM[(size_t)s * H + c] = t;
  }
}

int launch_ig_head(const IgHeadParams& p, int S, hipStream_t st) {
  if (!p.M || !p.Wk || !p.bk || !p.dM || !p.step_risk || !p.risk_x || !p.risk_base) return MMF_ERR_ARG;
  if (p.K < 1 || p.K > 32 || p.H < 1 || S < 1 || S > GROUP_MAX) return MMF_ERR_SHAPE;
  ProfScope ps("ig_head_kernel", st);
  hipLaunchKernelGGL(ig_head_kernel, dim3(S), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// ---- the omic branch of the multimodal head's integrated gradients (mmf_mm_ig) ----------------------------------------
// The two SNN blocks of models/model_mm_attention_mil.py:44-47 in eval mode, O = selu(W1 selu(W0 x + b0) + b1).  With a zero
// baseline the first pre-activation is linear in the node, z1 = alpha Z + b0 with Z = W0 x formed once, and the input
// gradient is linear in dz1: sum_k w_k dx_k = W0^T (sum_k w_k dz1_k).  Per node only the two hidden layers run.
constexpr float IG_SELU_ALPHA = 1.6732632423543772f;
constexpr float IG_SELU_SCALE = 1.0507009873554805f;
__device__ inline float ig_selu(float z) { return IG_SELU_SCALE * (z > 0.f ? z : IG_SELU_ALPHA * (expf(z) - 1.0f)); }
__device__ inline float ig_selu_grad(float z) { return z > 0.f ? IG_SELU_SCALE : IG_SELU_SCALE * IG_SELU_ALPHA * expf(z); }

// Z[c] = sum_j W0[c, j] x[j].  One wave per output, four per workgroup: lane t adds its products j = t, t + 64, ... in that
// order, the xor butterfly adds the lanes -- ceil(Gin / 64) + 6 dependent additions, the same in every call.
__global__ __launch_bounds__(256) void ig_omic_z_kernel(IgOmicParams p) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= p.W0n) return;
  float t = 0.f;
  for (int j = lane; j < p.Gin; j += 64) t = fmaf(p.W0[(size_t)c * p.Gin + j], p.x[j], t);
  t = wave_sum(t);
  if (lane == 0) p.Z[c] = t;
}

// One workgroup of 16 waves per node s of the window: z1 = alpha_s Z + b0 (kept), h1 = selu(z1) in LDS; then one wave per
// output of the second layer, as above over the W0n hidden units (ceil(W0n / 64) + 7 additions with the bias): z2 (kept),
// and O_s = selu(z2) into the omic columns of row s of feat [S x F].  A wave takes four outputs at a time, so that their
// loads are in flight together: the window has few nodes, and a node's outputs one after the other wait for memory.
__global__ __launch_bounds__(1024) void ig_omic_fwd_kernel(IgOmicParams p) {
  __shared__ float h1[1024];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float a = p.st.alpha[s];
  for (int c = tid; c < p.W0n; c += 1024) {
    const float z = fmaf(a, p.Z[c], p.b0[c]);
    p.z1[(size_t)s * p.W0n + c] = z;
    h1[c] = ig_selu(z);
  }
  __syncthreads();
  for (int e0 = 4 * wave; e0 < p.We; e0 += 64) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    const float* w[4];                     // a row past the last output reads the last one again and is not stored: no branch
#pragma unroll                             // between the loads, so the compiler keeps all of an iteration's in flight
    for (int i = 0; i < 4; ++i) w[i] = p.W1 + (size_t)(e0 + i < p.We ? e0 + i : p.We - 1) * p.W0n;
#pragma unroll 4
    for (int c = lane; c < p.W0n; c += 64) {
      const float h = h1[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = fmaf(w[i][c], h, t[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = wave_sum(t[i]);
      if (lane == 0 && e0 + i < p.We) {
        const float z = v + p.b1[e0 + i];
        p.z2[(size_t)s * p.We + e0 + i] = z;
        p.feat[(size_t)s * p.F + p.col + e0 + i] = ig_selu(z);
      }
    }
  }
}

// One workgroup per node: dz2 = dO_s selu'(z2) in LDS; then dz1[c] = selu'(z1[c]) sum_e W1[e, c] dz2[e].  Four groups of 256
// threads take a quarter of the outputs e each, in order, one thread per hidden unit c (W1 is read along c: coalesced);
// the four partial sums of a unit are added in group order.
__global__ __launch_bounds__(1024) void ig_omic_bwd_kernel(IgOmicParams p) {
  __shared__ float dz2[1024];
  __shared__ float part[4][1024];
  const int s = blockIdx.x, tid = threadIdx.x, g = tid >> 8, t256 = tid & 255;
  for (int e = tid; e < p.We; e += 1024)
    dz2[e] = p.dfeat[(size_t)s * p.F + p.col + e] * ig_selu_grad(p.z2[(size_t)s * p.We + e]);
  __syncthreads();
  const int per = (p.We + 3) / 4, e_beg = g * per, e_end = e_beg + per < p.We ? e_beg + per : p.We;
  for (int c = t256; c < p.W0n; c += 256) {
    float t = 0.f;
#pragma unroll 8
    for (int e = e_beg; e < e_end; ++e) t = fmaf(p.W1[(size_t)e * p.W0n + c], dz2[e], t);
    part[g][c] = t;
  }
  __syncthreads();
  for (int c = tid; c < p.W0n; c += 1024) {
    const float t = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
    p.dz1[(size_t)s * p.W0n + c] = t * ig_selu_grad(p.z1[(size_t)s * p.W0n + c]);
  }
}

// Gz[c] (first: =, else +=) sum_s w_s dz1[s, c] over the first st.S nodes of the window, in node order: ig_fold_kernel's
// sum for a width that need be no multiple of four
__global__ __launch_bounds__(256) void ig_omic_fold_kernel(IgOmicParams p) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= p.W0n) return;
  float acc = p.first ? 0.f : p.Gz[c];
  for (int s = 0; s < p.st.S; ++s) acc = fmaf(p.st.w[s], p.dz1[(size_t)s * p.W0n + c], acc);
  p.Gz[c] = acc;
}

// attr[j] = x[j] sum_c Gz[c] W0[c, j]: one wave per gene, four per workgroup -- lane t adds its hidden units c = t, t + 64,
// ... in that order, the butterfly adds the lanes (W0 is 320 KB at most: its columns come from L2)
__global__ __launch_bounds__(256) void ig_omic_attr_kernel(IgOmicParams p) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p.Gin) return;
  float t = 0.f;
  for (int c = lane; c < p.W0n; c += 64) t = fmaf(p.Gz[c], p.W0[(size_t)c * p.Gin + j], t);
  t = wave_sum(t);
  if (lane == 0) p.attr[j] = p.x[j] * t;
}

int launch_ig_omic(int stage, const IgOmicParams& p, hipStream_t st) {
  if (!p.x || !p.W0 || !p.b0 || !p.W1 || !p.b1 || !p.Z || !p.z1 || !p.z2 || !p.dz1 || !p.Gz) return MMF_ERR_ARG;
  if (p.Gin < 1 || p.W0n < 1 || p.W0n > 1024 || p.We < 1 || p.We > 1024) return MMF_ERR_SHAPE;
  const int S = p.st.S;
  const bool per_node = stage == IG_OMIC_FWD || stage == IG_OMIC_BWD;
  if (per_node && (S < 1 || S > GROUP_MAX || p.col < 0 || p.col + p.We > p.F)) return MMF_ERR_SHAPE;
  switch (stage) {
    case IG_OMIC_Z: {
      ProfScope ps("ig_omic_z_kernel", st);
      hipLaunchKernelGGL(ig_omic_z_kernel, dim3((unsigned)((p.W0n + 3) / 4)), dim3(256), 0, st, p);
      break;
    }
    case IG_OMIC_FWD: {
      if (!p.feat) return MMF_ERR_ARG;
      ProfScope ps("ig_omic_fwd_kernel", st);
      hipLaunchKernelGGL(ig_omic_fwd_kernel, dim3(S), dim3(1024), 0, st, p);
      break;
    }
    case IG_OMIC_BWD: {
      if (!p.dfeat) return MMF_ERR_ARG;
      ProfScope ps("ig_omic_bwd_kernel", st);
      hipLaunchKernelGGL(ig_omic_bwd_kernel, dim3(S), dim3(1024), 0, st, p);
      break;
    }
    case IG_OMIC_FOLD: {
      if (S < 0 || S > GROUP_MAX) return MMF_ERR_SHAPE;
      if (S == 0 && !p.first) return MMF_OK;           // a window of riders: nothing to add (launch_ig_fold)
      ProfScope ps("ig_omic_fold_kernel", st);
      hipLaunchKernelGGL(ig_omic_fold_kernel, dim3((unsigned)((p.W0n + 255) / 256)), dim3(256), 0, st, p);
      break;
    }
    case IG_OMIC_ATTR: {
      if (!p.attr) return MMF_ERR_ARG;
      ProfScope ps("ig_omic_attr_kernel", st);
      hipLaunchKernelGGL(ig_omic_attr_kernel, dim3((unsigned)((p.Gin + 3) / 4)), dim3(256), 0, st, p);
      break;
    }
    default: return MMF_ERR_ARG;
  }
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

}  // namespace mmf
