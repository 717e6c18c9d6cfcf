// Backward of the XlinearFusion tail for the G patients of one accumulation window (mmf_xfusion_group_backward;
// models/model_modules.py:156-178 under autograd, once per patient in the reference): everything in front of encoder2,
// whose own backward and classifier[0]'s are the existing dense_bwd_kernel<true> on the [G x K2] input matrix.
//
//   kron_dense_dkr_group_kernel   dkr[g][e]  = sum_n dpre1[g][n] We1[n][e]           (d of the dropped product)
//   kron_dense_dw_group_kernel    dWe1[n][e] = sum_g dpre1[g][n] kr_g[e], dbe1[n]    (kr_g rebuilt from [o, 1] and keep bits)
//   xgate_bwd_group_kernel        per patient: d o_t from dkr, then xreduce_bwd_kernel's arithmetic for B = 1; dv_i added
//   xgate_dw_group_kernel         dWh, dWz, dWo, dbh, dbz, dbo: one thread per element, patients in order
//
// dpre1[g][n] = d e1[g][n] / (1 - p) where the dropped e1[g][n] > 0, else 0: a ReLU output that survived its dropout is
// positive, so the mask of site 9 is not hashed again.  Latency- and L2-bound VALU work: no MFMA, no atomics, no
// workgroup waits for another, every sum runs in an order fixed by its output element (patients in patient order).
#include "mmf_common.h"
#include "mmf_kernels.h"
#include "mmf_mlp.h"

namespace mmf {

constexpr int XB_S1 = 17;                       // sdim + 1
constexpr int XB_PG = 16;                       // patients per workgroup of the dkr launch
constexpr int XB_NC = 512;                      // rows of We1 staged per pass of the dkr launch
constexpr int XB_ROWS = 32;                     // rows of dWe1 per workgroup of the dW launch

__device__ inline float xb_dpre1(const XFusionBwdParams& p, int g, int n, float inv) {
  const size_t at = (size_t)g * p.K2 + n;
  return p.x2[at] > 0.f ? p.dx2[at] * inv : 0.f;
}
__device__ inline bool xb_bit(const XFusionBwdParams& p, int nwb, int g, int e) {
  return (p.bits[(size_t)g * nwb + (e >> 5)] >> (e & 31)) & 1u;
}

// Work unit: 64 consecutive elements e (one per lane: a row of We1 is read coalesced) x 16 patients.  The four waves split
// the rows n of every 512-row pass into quarters; dpre1 of the pass is staged in LDS as [n][patient] (four 16-byte
// broadcast reads per row).  We1 is fetched from memory once (the other patient groups hit L2).
__global__ __launch_bounds__(256) void kron_dense_dkr_group_kernel(XFusionBwdParams p, int E) {
  __shared__ __align__(16) float sdp[XB_NC][XB_PG];
  __shared__ float red[4][XB_PG][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = blockIdx.x * 64 + lane, g0 = blockIdx.y * XB_PG;
  const float inv = p.p > 0.f ? 1.0f / (1.0f - p.p) : 1.0f;
  float acc[XB_PG];
#pragma unroll
  for (int u = 0; u < XB_PG; ++u) acc[u] = 0.f;
  for (int n0 = 0; n0 < p.N1; n0 += XB_NC) {
    __syncthreads();
    for (int i = tid; i < XB_NC * XB_PG; i += 256) {
      const int nn = i / XB_PG, u = i % XB_PG, g = g0 + u, n = n0 + nn;
      sdp[nn][u] = g < p.G && n < p.N1 ? xb_dpre1(p, g, n, inv) : 0.f;
    }
    __syncthreads();
    const int nc = p.N1 - n0 < XB_NC ? p.N1 - n0 : XB_NC;
    const int hi = (wave + 1) * (XB_NC / 4) < nc ? (wave + 1) * (XB_NC / 4) : nc;
    if (e < E) {
#pragma unroll 4
      for (int nn = wave * (XB_NC / 4); nn < hi; ++nn) {
        const float w = p.We1[(size_t)(n0 + nn) * E + e];
#pragma unroll
        for (int u4 = 0; u4 < XB_PG; u4 += 4) {
          const float4 d = *reinterpret_cast<const float4*>(&sdp[nn][u4]);
          acc[u4] += d.x * w; acc[u4 + 1] += d.y * w; acc[u4 + 2] += d.z * w; acc[u4 + 3] += d.w * w;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < XB_PG; ++u) red[wave][u][lane] = acc[u];
  __syncthreads();
  for (int i = tid; i < XB_PG * 64; i += 256) {
    const int u = i >> 6, l = i & 63, g = g0 + u, ee = blockIdx.x * 64 + l;
    if (g < p.G && ee < E) p.dkr[(size_t)g * E + ee] = (red[0][u][l] + red[1][u][l]) + (red[2][u][l] + red[3][u][l]);
  }
}

// Work unit: 256 consecutive elements e (one per thread: dWe1 is written coalesced, once) x 32 rows n.  A thread keeps
// kr_g[e] of every patient in registers -- [o_g0, 1] x [o_g1, 1] (x [o_g2, 1]) at e, dropped under its keep bit -- and sums
// dpre1[g][n] kr_g[e] over the patients in order for each of its rows; absent patients are zeros.
template <int M>
__global__ __launch_bounds__(256) void kron_dense_dw_group_kernel(XFusionBwdParams p) {
  constexpr int E = M == 3 ? XB_S1 * XB_S1 * XB_S1 : XB_S1 * XB_S1, NWB = xfusion_bit_words(M);
  __shared__ float so[GROUP_MAX * M * XB_S1];
  __shared__ __align__(16) float sdp[XB_ROWS][GROUP_MAX];
  const int tid = threadIdx.x, e = blockIdx.x * 256 + tid, n0 = blockIdx.y * XB_ROWS;
  const float inv = p.p > 0.f ? 1.0f / (1.0f - p.p) : 1.0f;
  for (int i = tid; i < GROUP_MAX * M * XB_S1; i += 256) {
    const int r = i / XB_S1, k = i - r * XB_S1;
    so[i] = r < p.G * M ? (k < XB_S1 - 1 ? p.o[(size_t)r * (XB_S1 - 1) + k] : 1.f) : 0.f;
  }
  for (int i = tid; i < XB_ROWS * GROUP_MAX; i += 256) {
    const int r = i / GROUP_MAX, g = i % GROUP_MAX, n = n0 + r;
    sdp[r][g] = g < p.G && n < p.N1 ? xb_dpre1(p, g, n, inv) : 0.f;
  }
  __syncthreads();
  const bool live = e < E;
  const int ec = live ? e : 0;
  const int i0 = M == 3 ? ec / (XB_S1 * XB_S1) : ec / XB_S1, i1 = M == 3 ? (ec / XB_S1) % XB_S1 : ec % XB_S1, i2 = ec % XB_S1;
  float kr[GROUP_MAX];
#pragma unroll
  for (int g = 0; g < GROUP_MAX; ++g) {
    const float* og = so + g * M * XB_S1;
    float v = og[i0] * og[XB_S1 + i1];
    if (M == 3) v *= og[2 * XB_S1 + i2];
    const bool k = live && g < p.G && xb_bit(p, NWB, g, ec);
    kr[g] = k ? v * inv : 0.f;
  }
  for (int r = 0; r < XB_ROWS; ++r) {
    const int n = n0 + r;
    if (n >= p.N1) break;
    float acc = 0.f;
#pragma unroll
    for (int g4 = 0; g4 < GROUP_MAX; g4 += 4) {
      const float4 d = *reinterpret_cast<const float4*>(&sdp[r][g4]);
      acc += d.x * kr[g4]; acc += d.y * kr[g4 + 1]; acc += d.z * kr[g4 + 2]; acc += d.w * kr[g4 + 3];
    }
    if (live) {
      float* out = p.dWe1 + (size_t)n * E + e;
      *out = p.accumulate ? *out + acc : acc;
    }
  }
  if (blockIdx.x == 0 && tid < XB_ROWS && n0 + tid < p.N1) {
    float acc = 0.f;
    for (int g = 0; g < p.G; ++g) acc += sdp[tid][g];
    float* out = p.dbe1 + n0 + tid;
    *out = p.accumulate ? *out + acc : acc;
  }
}

// One workgroup per patient.  d o_t[i] = sum over the other indices of dkr . keep / (1 - p) . (product of the other
// operands): kron_bwd_kernel's sum, one wave per output; then xreduce_bwd_kernel's arithmetic for B = 1 (dpo, dgm, dz, dph
// through 48 floats of LDS each).  dpo, dz, dph go to memory for the weight gradients; dv_t -- the h path of modality t and
// the v_cat path through every Wz -- is added to the skip-connection gradient encoder2's backward left in dx2.
__global__ __launch_bounds__(1024) void xgate_bwd_group_kernel(XFusionBwdParams p) {
  constexpr int S = XB_S1 - 1;
  __shared__ float s_o[3 * XB_S1], s_do[3 * S], s_dpo[3 * S], s_dz[3 * S], s_dph[3 * S];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int total = p.m * S, KZ = p.m * p.dim;
  const int E = p.m == 3 ? XB_S1 * XB_S1 * XB_S1 : XB_S1 * XB_S1, others = E / XB_S1, nwb = xfusion_bit_words(p.m);
  const float inv = p.p > 0.f ? 1.0f / (1.0f - p.p) : 1.0f;
  if (tid < p.m * XB_S1) {
    const int i = tid / XB_S1, k = tid % XB_S1;
    s_o[tid] = k < S ? p.o[(size_t)g * total + i * S + k] : 1.f;
  }
  __syncthreads();
  const float* dk = p.dkr + (size_t)g * E;
  for (int out = wave; out < total; out += 16) {
    const int t = out / S, i = out % S;
    float acc = 0.f;
    for (int q = lane; q < others; q += 64) {
      int e;
      float prod;
      if (p.m == 3) {
        const int q0 = q / XB_S1, q1 = q % XB_S1;
        int i0, i1, i2;
        if (t == 0) { i0 = i; i1 = q0; i2 = q1; }
        else if (t == 1) { i0 = q0; i1 = i; i2 = q1; }
        else { i0 = q0; i1 = q1; i2 = i; }
        e = (i0 * XB_S1 + i1) * XB_S1 + i2;
        const float v0 = s_o[i0], v1 = s_o[XB_S1 + i1], v2 = s_o[2 * XB_S1 + i2];
        prod = t == 0 ? v1 * v2 : (t == 1 ? v0 * v2 : v0 * v1);
      } else {
        const int i0 = t == 0 ? i : q, i1 = t == 0 ? q : i;
        e = i0 * XB_S1 + i1;
        prod = t == 0 ? s_o[XB_S1 + i1] : s_o[i0];
      }
      acc += xb_bit(p, nwb, g, e) ? dk[e] * inv * prod : 0.f;
    }
    acc = wave_sum(acc);
    if (lane == 0) s_do[out] = acc;
  }
  __syncthreads();
  if (tid < total) s_dpo[tid] = p.o[(size_t)g * total + tid] > 0.f ? s_do[tid] * inv : 0.f;   // d(pre-activation of o)
  __syncthreads();
  if (tid < total) {                                 // d gm = dpo . Wo ; then dz, dh
    const int i = tid / S, u = tid % S;
    const size_t at = (size_t)g * total + tid;
    float acc = 0.f;
#pragma unroll 16
    for (int j = 0; j < S; ++j) acc += s_dpo[i * S + j] * p.Wo[i][j * S + u];
    const float hv = p.h[at], sg = 1.0f / (1.0f + expf(-p.z[at]));
    const float dz = acc * hv * sg * (1.f - sg), dph = hv > 0.f ? acc * sg : 0.f;
    s_dz[tid] = dz; s_dph[tid] = dph;
    p.dpo[at] = s_dpo[tid]; p.dz[at] = dz; p.dph[at] = dph;
  }
  __syncthreads();
  for (int q = tid; q < KZ; q += 1024) {
    const int t = q / p.dim, k = q % p.dim;
    float acc = 0.f;
#pragma unroll 16
    for (int j = 0; j < S; ++j) acc += s_dph[t * S + j] * p.Wh[t][(size_t)j * p.dim + k];
    for (int i = 0; i < p.m; ++i) {
      float a2 = 0.f;
#pragma unroll 16
      for (int j = 0; j < S; ++j) a2 += s_dz[i * S + j] * p.Wz[i][(size_t)j * KZ + q];
      acc += a2;
    }
    p.dx2[(size_t)g * p.K2 + p.N1 + q] += acc;
  }
}

// The gating stage's weight gradients, one thread per output element, the patients summed in order.  Per modality i the
// elements are dWh [16 x dim], dWz [16 x m dim], dWo [16 x 16], dbh, dbz, dbo [16]; v_cat of patient g is x2's row g from
// column N1 on.
__global__ __launch_bounds__(256) void xgate_dw_group_kernel(XFusionBwdParams p) {
  constexpr int S = XB_S1 - 1;
  const int KZ = p.m * p.dim, nh = S * p.dim, nz = S * KZ, per = nh + nz + S * S + 3 * S, total = p.m * S;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.m * per) return;
  const int i = idx / per;
  int r = idx % per;
  const float* a;            // [G x total] factor, read at column ca
  const float* b = nullptr;  // second factor: row stride ldb, column cb; null: a bias (sum of a)
  int ca, cb = 0, ldb = 0;
  float* out;
  if (r < nh) {
    a = p.dph; ca = i * S + r / p.dim; b = p.x2; ldb = p.K2; cb = p.N1 + i * p.dim + r % p.dim; out = p.dWh[i] + r;
  } else if ((r -= nh) < nz) {
    a = p.dz; ca = i * S + r / KZ; b = p.x2; ldb = p.K2; cb = p.N1 + r % KZ; out = p.dWz[i] + r;
  } else if ((r -= nz) < S * S) {
    a = p.dpo; ca = i * S + r / S; b = p.gm; ldb = total; cb = i * S + r % S; out = p.dWo[i] + r;
  } else {
    r -= S * S;
    const int which = r / S, j = r % S;
    a = which == 0 ? p.dph : (which == 1 ? p.dz : p.dpo); ca = i * S + j;
    out = (which == 0 ? p.dbh[i] : (which == 1 ? p.dbz[i] : p.dbo[i])) + j;
  }
  float acc = 0.f;
  if (b) for (int g = 0; g < p.G; ++g) acc += a[(size_t)g * total + ca] * b[(size_t)g * ldb + cb];
  else for (int g = 0; g < p.G; ++g) acc += a[(size_t)g * total + ca];
  *out = p.accumulate ? *out + acc : acc;
}

__global__ __launch_bounds__(256) void add_into_kernel(float* out, const float* in, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] += in[i];
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int launched() { return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH; }

int launch_add_into(float* out, const float* in, int64_t n, hipStream_t st) {
  if (n < 1) return MMF_OK;
  { ProfScope ps("add_into_kernel", st); hipLaunchKernelGGL(add_into_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, out, in, n); }
  return launched();
}

static int xfusion_bwd_check(const XFusionBwdParams& p) {
  if (p.m < 2 || p.m > 3 || p.G < 1 || p.G > GROUP_MAX || p.N1 < 1 || p.dim < 1 || p.K2 != p.N1 + p.m * p.dim) return MMF_ERR_SHAPE;
  return MMF_OK;
}
static inline int xfusion_elems_of(int m) { return m == 3 ? XB_S1 * XB_S1 * XB_S1 : XB_S1 * XB_S1; }
static int launch_kron_dense_dkr(const XFusionBwdParams& p, hipStream_t st) {
  const int E = xfusion_elems_of(p.m);
  { ProfScope ps("kron_dense_dkr_group_kernel", st);
    hipLaunchKernelGGL(kron_dense_dkr_group_kernel, dim3(cdiv(E, 64), cdiv(p.G, XB_PG)), dim3(256), 0, st, p, E); }
  return launched();
}
static int launch_xgate_bwd(const XFusionBwdParams& p, hipStream_t st) {
  { ProfScope ps("xgate_bwd_group_kernel", st); hipLaunchKernelGGL(xgate_bwd_group_kernel, dim3(p.G), dim3(1024), 0, st, p); }
  return launched();
}

int launch_xfusion_group_bwd(XFusionBwdParams p, hipStream_t st) {
  if (int e = xfusion_bwd_check(p)) return e;
  const int E = xfusion_elems_of(p.m);
  if (int e = launch_kron_dense_dkr(p, st)) return e;
  { ProfScope ps("kron_dense_dw_group_kernel", st);
    const dim3 grid(cdiv(E, 256), cdiv(p.N1, XB_ROWS));
    if (p.m == 3) hipLaunchKernelGGL(kron_dense_dw_group_kernel<3>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(kron_dense_dw_group_kernel<2>, grid, dim3(256), 0, st, p); }
  if (int e = launched()) return e;
  if (int e = launch_xgate_bwd(p, st)) return e;
  const int S = XB_S1 - 1, per = S * p.dim + S * p.m * p.dim + S * S + 3 * S;
  { ProfScope ps("xgate_dw_group_kernel", st);
    hipLaunchKernelGGL(xgate_dw_group_kernel, dim3(cdiv((int64_t)p.m * per, 256)), dim3(256), 0, st, p); }
  return launched();
}

int launch_xfusion_group_bwd_dx(XFusionBwdParams p, hipStream_t st) {
  if (int e = xfusion_bwd_check(p)) return e;
  if (int e = launch_kron_dense_dkr(p, st)) return e;
  return launch_xgate_bwd(p, st);
}

}  // namespace mmf
