// Integrated gradients of the stage-2 fusion models (mmf_stage2_ig), a cohort of P patients per call: the three launches of
// the folded train types -- early-fcnn, late-fcnn and, with one Highway layer, early-highway and late-highway --, the
// launches around the row kernels for deeper Highways and around the tensor fusion's tail for kronecker
// (models/nll_models_pretrained.py:66-197, models/coxranking_models_pretrained.py:62-200 in eval mode, and their autograd).
//
// In eval mode BatchNorm1d is a per-feature affine map (x s + t, s = weight / sqrt(var + eps), t = bias - mean s) and a
// row's result depends on that row alone.  With a zero baseline node alpha feeds alpha v, and the first layer of every
// folded type is linear in alpha:
//   fcnn block      u(alpha)   = alpha (v W0^T) + b0
//   Highway layer 0 z_*(alpha) = alpha ((v . s1) W_*^T) + (W_* t1 + b_*)      * in {gate, nonlinear, linear}, bn1 = (s1, t1)
// so the packed row [v_0 | .. | v_{m-1}] meets the first-layer weights ONCE per patient, and one more row -- t1, or 0 where
// there is no bn1 -- gives the constants.  What remains per node is elementwise work and a K <= 32 row classifier.
//
//   stage2_fold_fwd_kernel   U [(P + 1) x ldU] = rows . W^T for every first-layer matrix of the model (a list of problems:
//                            which columns of the packed row, which columns of U).  Row P holds the constants, bias added.
//                            One wave per output column, eight rows at a time: lane l adds its products c = l, l + 64, ...
//                            in that order, the xor butterfly adds the lanes.
//   stage2_sweep_kernel      one workgroup per patient, its pre-activations and accumulators in registers (three units a
//                            thread): for every node the activations (BN + ReLU, or sigmoid / ReLU mix + bn2) into LDS, the
//                            hazard head and the backward of risk (mmf_ig_head.h) or the cox scalar, the gradient down to
//                            the pre-activations, G += w_k d.  Per node it writes step_risk only; at the end G [P x ldU].
//   stage2_attr_kernel       dx = sum over the problems that read a modality of G W (the transposed first layer), eight
//                            patients and one modality per workgroup, one thread per column and quarter of the units; the
//                            quarters are added in order, attr = v . s1 . dx, and its sums per patient and modality.
// No atomics, no workgroup waits for another, every sum runs in an order fixed by its output element.
#include "mmf_common.h"
#include "mmf_kernels.h"
#include "mmf_ig_head.h"

namespace mmf {

constexpr int S2_ROWS = 8;        // patients per workgroup of the two folded contractions
constexpr int S2_COLS = 64;       // outputs per workgroup of the forward one
constexpr int S2_DIM = 256;       // an embedding's width

// eval-mode BatchNorm1d as scale and shift of feature f
__device__ inline void s2_bn_affine(const S2Bn& b, int f, float& s, float& t) {
  s = b.w[f] / sqrtf(b.var[f] + b.eps);
  t = b.b[f] - b.mean[f] * s;
}

__global__ __launch_bounds__(256) void stage2_fold_fwd_kernel(S2FoldParams p) {
  __shared__ float xs[S2_ROWS][S2_MAXW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * S2_ROWS;
  int chunk = blockIdx.y, pi = 0;
  while (pi < p.nprob - 1 && chunk >= (p.prob[pi].n_out + S2_COLS - 1) / S2_COLS) {
    chunk -= (p.prob[pi].n_out + S2_COLS - 1) / S2_COLS;
    ++pi;
  }
  const S2Lin pr = p.prob[pi];
  for (int c = tid; c < pr.k_in; c += 256) {
    const int col = pr.in_col + c, mod = col / S2_DIM, f = col % S2_DIM;
    float s = 1.f, t = 0.f;
    if (p.in_bn[mod].w) s2_bn_affine(p.in_bn[mod], f, s, t);
#pragma unroll
    for (int r = 0; r < S2_ROWS; ++r) {
      const int row = r0 + r;
      xs[r][c] = row < p.P ? p.v[mod][(size_t)row * S2_DIM + f] * s : row == p.P ? t : 0.f;
    }
  }
  __syncthreads();
  for (int jj = 0; jj < S2_COLS / 4; ++jj) {
    const int j = chunk * S2_COLS + wave * (S2_COLS / 4) + jj;
    if (j >= pr.n_out) break;
    const float* w = pr.W + (size_t)j * pr.k_in;
    float acc[S2_ROWS];
#pragma unroll
    for (int r = 0; r < S2_ROWS; ++r) acc[r] = 0.f;
    for (int c = lane; c < pr.k_in; c += 64) {
      const float wv = w[c];
#pragma unroll
      for (int r = 0; r < S2_ROWS; ++r) acc[r] = fmaf(wv, xs[r][c], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < S2_ROWS; ++r) {
      const float t = wave_sum(acc[r]);
      const int row = r0 + r;
      if (lane == 0 && row <= p.P) p.U[(size_t)row * p.ldU + pr.out_col + j] = row == p.P ? t + pr.bias[j] : t;
    }
  }
}

__global__ __launch_bounds__(256) void stage2_sweep_kernel(S2SweepParams p) {
  __shared__ float act[S2_MAXW];
  __shared__ float wke[S2_MAXW];          // cox late-fcnn: the blocks' last layers under the classifier's weights
  __shared__ float lg[32], hz[32], sv[32], dl[32];
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pt = blockIdx.x, W = p.W, K = p.K;
  const float* Up = p.U + (size_t)pt * p.ldU;
  const float* Uc = p.U + (size_t)p.P * p.ldU;
  constexpr int UPT = S2_MAXW / 256;
  float u[3][UPT], c[3][UPT], g[3][UPT], s[UPT], t[UPT];
  const int planes = p.highway ? 3 : 1;
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int j = tid + 256 * i;
    s[i] = 1.f; t[i] = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) { u[q][i] = 0.f; c[q][i] = 0.f; g[q][i] = 0.f; }
    if (j < W) {
      s2_bn_affine(p.bn[j / p.bn_span], j % p.bn_span, s[i], t[i]);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (q < planes) { u[q][i] = Up[q * W + j]; c[q][i] = Uc[q * W + j]; }
    }
  }
  const float* wk = p.Wk;
  float bias0 = p.cox ? p.bk[0] : 0.f;
  if (p.late_cox) {
    for (int j = tid; j < W; j += 256) wke[j] = p.Wk[j / 128] * p.W4[j / 128][j % 128];
    for (int b = 0; b < W / 128; ++b) bias0 += p.Wk[b] * p.b4[b][0];
    wk = wke;
  }
  IgHeadParams hp{};
  hp.Wk = p.Wk; hp.bk = p.bk; hp.K = K; hp.H = W; hp.step0 = 0; hp.n_steps = p.n_steps;
  hp.step_risk = p.step_risk + (size_t)pt * p.n_steps; hp.risk_x = p.risk + pt; hp.risk_base = p.risk_base + pt;
  hp.hazards = p.hazards ? p.hazards + (size_t)pt * K : nullptr;
  hp.S = p.S ? p.S + (size_t)pt * K : nullptr;
  __syncthreads();
  for (int q = 0; q < p.n_steps + 2; ++q) {
    const float a = p.alpha[q], wq = p.weight[q];
    float zg[UPT], zn[UPT], zl[UPT], gt[UPT];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int j = tid + 256 * i;
      float o;
      if (p.highway) {
        zg[i] = fmaf(a, u[0][i], c[0][i]); zn[i] = fmaf(a, u[1][i], c[1][i]); zl[i] = fmaf(a, u[2][i], c[2][i]);
        gt[i] = 1.0f / (1.0f + __expf(-zg[i]));
        o = fmaf(s[i], gt[i] * fmaxf(zn[i], 0.f) + (1.0f - gt[i]) * zl[i], t[i]);
      } else {
        zn[i] = fmaf(s[i], fmaf(a, u[0][i], c[0][i]), t[i]);
        o = fmaxf(zn[i], 0.f);
      }
      if (j < W) act[j] = o;
    }
    __syncthreads();
    if (p.cox) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < UPT; ++i) {
        const int j = tid + 256 * i;
        if (j < W) d = fmaf(wk[j], act[j], d);
      }
      d = wave_sum(d);
      if (lane == 0) part[wave] = d;
      __syncthreads();
      if (tid == 0) {
        const float risk = ((part[0] + part[1]) + part[2]) + part[3] + bias0;
        if (q < p.n_steps) hp.step_risk[q] = risk;
        else if (q == p.n_steps) hp.risk_x[0] = risk;
        else hp.risk_base[0] = risk;
      }
      __syncthreads();
    } else {
      ig_hazard_body<4>(hp, act, q, lg, hz, sv, dl);
    }
    if (q >= p.n_steps) continue;            // the riders alpha = 1 and alpha = 0 carry no weight
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int j = tid + 256 * i;
      if (j >= W) continue;
      float da;
      if (p.cox) da = wk[j];
      else {
        da = 0.f;
        for (int k = 0; k < K; ++k) da = fmaf(dl[k], p.Wk[(size_t)k * W + j], da);
      }
      if (p.highway) {
        const float dy = s[i] * da;
        g[0][i] = fmaf(wq, dy * (fmaxf(zn[i], 0.f) - zl[i]) * gt[i] * (1.0f - gt[i]), g[0][i]);
        g[1][i] = fmaf(wq, zn[i] > 0.f ? dy * gt[i] : 0.f, g[1][i]);
        g[2][i] = fmaf(wq, dy * (1.0f - gt[i]), g[2][i]);
      } else {
        g[0][i] = fmaf(wq, zn[i] > 0.f ? s[i] * da : 0.f, g[0][i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int j = tid + 256 * i;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (j < W && q < planes) p.G[(size_t)pt * p.ldU + q * W + j] = g[q][i];
  }
}

__global__ __launch_bounds__(1024) void stage2_attr_kernel(S2FoldParams p) {
  __shared__ float gs[S2_ROWS][256];
  __shared__ float part[4][S2_ROWS][S2_DIM];
  __shared__ float red[2][S2_ROWS][4];
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 8, cx = tid & 255;
  const int r0 = blockIdx.x * S2_ROWS, mod = blockIdx.y, col = mod * S2_DIM + cx;
  float acc[S2_ROWS];
#pragma unroll
  for (int r = 0; r < S2_ROWS; ++r) acc[r] = 0.f;
  for (int pi = 0; pi < p.nprob; ++pi) {
    const S2Lin pr = p.prob[pi];
    if (col < pr.in_col || col >= pr.in_col + pr.k_in) continue;       // the same for every thread: a modality's columns
    const float* w = pr.W + (col - pr.in_col);
    for (int j0 = 0; j0 < pr.n_out; j0 += 256) {
      __syncthreads();
      for (int e = tid; e < S2_ROWS * 256; e += 1024) {
        const int r = e >> 8, jj = e & 255, row = r0 + r;
        gs[r][jj] = row < p.P && j0 + jj < pr.n_out ? p.G[(size_t)row * p.ldU + pr.out_col + j0 + jj] : 0.f;
      }
      __syncthreads();
      const int j_end = pr.n_out - j0 < 256 ? pr.n_out - j0 : 256;
      const int b = ks * 64, e = b + 64 < j_end ? b + 64 : j_end;
#pragma unroll 8
      for (int jj = b; jj < e; ++jj) {
        const float wv = w[(size_t)(j0 + jj) * pr.k_in];
#pragma unroll
        for (int r = 0; r < S2_ROWS; ++r) acc[r] = fmaf(wv, gs[r][jj], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < S2_ROWS; ++r) part[ks][r][cx] = acc[r];
  __syncthreads();
  float s1 = 1.f, t1 = 0.f;
  if (p.in_bn[mod].w) s2_bn_affine(p.in_bn[mod], cx, s1, t1);
#pragma unroll
  for (int h = 0; h < S2_ROWS / 4; ++h) {
    const int r = ks * (S2_ROWS / 4) + h, row = r0 + r;
    float a = 0.f;
    if (row < p.P) {
      const float d = ((part[0][r][cx] + part[1][r][cx]) + part[2][r][cx]) + part[3][r][cx];
      a = p.v[mod][(size_t)row * S2_DIM + cx] * s1 * d;
      if (p.attr[mod]) p.attr[mod][(size_t)row * S2_DIM + cx] = a;
    }
    const float sa = wave_sum(a), sb = wave_sum(fabsf(a));
    if (lane == 0) { red[0][r][cx >> 6] = sa; red[1][r][cx >> 6] = sb; }
  }
  __syncthreads();
  if (tid < 2 * S2_ROWS) {
    const int which = tid / S2_ROWS, r = tid % S2_ROWS, row = r0 + r;
    if (row < p.P) {
      const float v = ((red[which][r][0] + red[which][r][1]) + red[which][r][2]) + red[which][r][3];
      (which ? p.mod_abs : p.mod_sum)[(size_t)row * p.m + mod] = v;
    }
  }
}

static int s2_fold_check(const S2FoldParams& p) {
  if (!p.U || p.m < 2 || p.m > 3 || p.P < 1 || p.nprob < 1 || p.nprob > S2_MAXPROB) return MMF_ERR_ARG;
  for (int i = 0; i < p.m; ++i)
    if (!p.v[i]) return MMF_ERR_ARG;
  for (int i = 0; i < p.nprob; ++i) {
    const S2Lin& q = p.prob[i];
    if (!q.W || !q.bias) return MMF_ERR_ARG;
    if (q.n_out < 1 || q.k_in < 1 || q.in_col < 0 || q.in_col % S2_DIM || q.k_in % S2_DIM || q.in_col + q.k_in > p.m * S2_DIM ||
        q.out_col < 0 || q.out_col + q.n_out > p.ldU)
      return MMF_ERR_SHAPE;
  }
  return MMF_OK;
}

int launch_stage2_fold_fwd(const S2FoldParams& p, hipStream_t st) {
  if (int e = s2_fold_check(p)) return e;
  int chunks = 0;
  for (int i = 0; i < p.nprob; ++i) chunks += (p.prob[i].n_out + S2_COLS - 1) / S2_COLS;
  ProfScope ps("stage2_fold_fwd_kernel", st);
  hipLaunchKernelGGL(stage2_fold_fwd_kernel, dim3((p.P + 1 + S2_ROWS - 1) / S2_ROWS, chunks), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

int launch_stage2_sweep(const S2SweepParams& p, hipStream_t st) {
  if (!p.U || !p.G || !p.Wk || !p.bk || !p.step_risk || !p.risk || !p.risk_base) return MMF_ERR_ARG;
  if (p.P < 1 || p.W < 1 || p.W > S2_MAXW || p.ldU != (p.highway ? 3 : 1) * p.W || p.n_steps < 1 || p.n_steps > GROUP_MAX ||
      p.K < 1 || p.K > 32 || (p.cox && p.K != 1) || p.bn_span < 1 || (p.W + p.bn_span - 1) / p.bn_span > 3 ||
      (p.late_cox && (!p.cox || p.highway || p.W % 128)))
    return MMF_ERR_SHAPE;
  for (int b = 0; b < (p.W + p.bn_span - 1) / p.bn_span; ++b)
    if (!p.bn[b].w || !p.bn[b].b || !p.bn[b].mean || !p.bn[b].var) return MMF_ERR_ARG;
  if (p.late_cox)
    for (int b = 0; b < p.W / 128; ++b)
      if (!p.W4[b] || !p.b4[b]) return MMF_ERR_ARG;
  ProfScope ps("stage2_sweep_kernel", st);
  hipLaunchKernelGGL(stage2_sweep_kernel, dim3(p.P), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

int launch_stage2_attr(const S2FoldParams& p, hipStream_t st) {
  if (int e = s2_fold_check(p)) return e;
  if (!p.G || !p.mod_sum || !p.mod_abs) return MMF_ERR_ARG;
  ProfScope ps("stage2_attr_kernel", st);
  hipLaunchKernelGGL(stage2_attr_kernel, dim3((p.P + S2_ROWS - 1) / S2_ROWS, p.m), dim3(1024), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// ---- kronecker: windows of (patient, node) rows through the tensor fusion's grouped tail -----------------------------------
// Row g = patient * T + node of the call, T = n_steps + 2 (the riders alpha = 1 and alpha = 0 behind every patient's nodes);
// a window holds rows g0 .. g0 + S - 1 and may straddle patients.

// x2[s][N1 + i 256 + c] = alpha_node v_i[patient][c]: the embedding columns of encoder2's input rows
__global__ __launch_bounds__(256) void stage2_kron_expand_kernel(S2KronParams p) {
  const int s = blockIdx.x, g = p.g0 + s, pt = g / p.T, k = g % p.T;
  const float a = p.alpha[k];
  for (int e = threadIdx.x; e < p.m * S2_DIM; e += 256)
    p.x2[(size_t)s * p.K2 + p.N1 + e] = a * p.v[e / S2_DIM][(size_t)pt * S2_DIM + e % S2_DIM];
}

// one workgroup per row: the classifier on MM_s, the hazard head and the backward of risk (or the cox scalar), the risk
// where the row's place in the call says, dMM_s[c] = sum_j dl[j] Wk[j][c] (encoder2's ReLU is the dense backward's)
__global__ __launch_bounds__(256) void stage2_kron_head_kernel(S2KronParams p) {
  __shared__ float mm[S2_DIM];
  __shared__ float lg[32], hz[32], sv[32], dl[32];
  __shared__ float part[4];
  const int s = blockIdx.x, g = p.g0 + s, pt = g / p.T, k = g % p.T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = p.K;
  mm[tid] = p.MM[(size_t)s * S2_DIM + tid];
  __syncthreads();
  float d;
  if (p.cox) {
    const float t = wave_sum(p.Wk[tid] * mm[tid]);
    if (lane == 0) part[wave] = t;
    __syncthreads();
    if (tid == 0) {
      const float risk = ((part[0] + part[1]) + part[2]) + part[3] + p.bk[0];
      if (k < p.n_steps) p.step_risk[(size_t)pt * p.n_steps + k] = risk;
      else if (k == p.n_steps) p.risk[pt] = risk;
      else p.risk_base[pt] = risk;
    }
    d = p.Wk[tid];
  } else {
    IgHeadParams hp{};
    hp.Wk = p.Wk; hp.bk = p.bk; hp.K = K; hp.H = S2_DIM; hp.step0 = 0; hp.n_steps = p.n_steps;
    hp.step_risk = p.step_risk + (size_t)pt * p.n_steps; hp.risk_x = p.risk + pt; hp.risk_base = p.risk_base + pt;
    hp.hazards = p.hazards ? p.hazards + (size_t)pt * K : nullptr;
    hp.S = p.S_out ? p.S_out + (size_t)pt * K : nullptr;
    ig_hazard_body<4>(hp, mm, k, lg, hz, sv, dl);
    d = 0.f;
    for (int j = 0; j < K; ++j) d = fmaf(dl[j], p.Wk[(size_t)j * S2_DIM + tid], d);
  }
  p.dMM[(size_t)s * S2_DIM + tid] = d;
}

// Gacc[patient][e] (=, or += when the patient's node 0 lies in an earlier window) sum over the patient's quadrature rows of
// the window, in node order, of w_node dx2[s][N1 + e]: one workgroup per patient of the window and 256 columns
__global__ __launch_bounds__(256) void stage2_kron_fold_kernel(S2KronParams p) {
  const int pt = p.g0 / p.T + blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
  const int g_beg = pt * p.T > p.g0 ? pt * p.T : p.g0;
  const int g_stop = pt * p.T + p.n_steps < p.g0 + p.S ? pt * p.T + p.n_steps : p.g0 + p.S;
  if (g_beg >= g_stop) return;                      // only riders of this patient in the window
  float* dst = p.Gacc + (size_t)pt * p.m * S2_DIM + e;
  float t = g_beg == pt * p.T ? 0.f : *dst;
  for (int g = g_beg; g < g_stop; ++g) t = fmaf(p.weight[g - pt * p.T], p.dx2[(size_t)(g - p.g0) * p.K2 + p.N1 + e], t);
  *dst = t;
}

// attr_i = v_i . Gacc's columns of modality i, and its sums: one workgroup per patient and modality
__global__ __launch_bounds__(256) void stage2_kron_attr_kernel(S2KronParams p) {
  __shared__ float red[2][4];
  const int pt = blockIdx.x, mod = blockIdx.y, tid = threadIdx.x;
  const float a = p.v[mod][(size_t)pt * S2_DIM + tid] * p.Gacc[((size_t)pt * p.m + mod) * S2_DIM + tid];
  if (p.attr[mod]) p.attr[mod][(size_t)pt * S2_DIM + tid] = a;
  const float sa = wave_sum(a), sb = wave_sum(fabsf(a));
  if ((tid & 63) == 0) { red[0][tid >> 6] = sa; red[1][tid >> 6] = sb; }
  __syncthreads();
  if (tid < 2) (tid ? p.mod_abs : p.mod_sum)[(size_t)pt * p.m + mod] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

static int s2_kron_check(const S2KronParams& p) {
  if (!p.v[0] || !p.v[1] || (p.m == 3 && !p.v[2]) || !p.Gacc) return MMF_ERR_ARG;
  if (p.m < 2 || p.m > 3 || p.P < 1 || p.n_steps < 1 || p.n_steps > GROUP_MAX || p.T != p.n_steps + 2 || p.S < 1 ||
      p.S > GROUP_MAX || p.g0 < 0 || (int64_t)p.g0 + p.S > (int64_t)p.P * p.T || p.N1 < 0 || p.K2 != p.N1 + p.m * S2_DIM ||
      p.K < 1 || p.K > 32 || (p.cox && p.K != 1))
    return MMF_ERR_SHAPE;
  return MMF_OK;
}

int launch_stage2_kron(int stage, const S2KronParams& p, hipStream_t st) {
  if (int e = s2_kron_check(p)) return e;
  const int p_first = p.g0 / p.T, p_last = (p.g0 + p.S - 1) / p.T;
  switch (stage) {
    case S2_KRON_EXPAND: {
      if (!p.x2) return MMF_ERR_ARG;
      ProfScope ps("stage2_kron_expand_kernel", st);
      hipLaunchKernelGGL(stage2_kron_expand_kernel, dim3(p.S), dim3(256), 0, st, p);
      break;
    }
    case S2_KRON_HEAD: {
      if (!p.MM || !p.dMM || !p.Wk || !p.bk || !p.step_risk || !p.risk || !p.risk_base) return MMF_ERR_ARG;
      ProfScope ps("stage2_kron_head_kernel", st);
      hipLaunchKernelGGL(stage2_kron_head_kernel, dim3(p.S), dim3(256), 0, st, p);
      break;
    }
    case S2_KRON_FOLD: {
      if (!p.dx2) return MMF_ERR_ARG;
      ProfScope ps("stage2_kron_fold_kernel", st);
      hipLaunchKernelGGL(stage2_kron_fold_kernel, dim3(p_last - p_first + 1, p.m), dim3(256), 0, st, p);
      break;
    }
    case S2_KRON_ATTR: {
      if (!p.mod_sum || !p.mod_abs) return MMF_ERR_ARG;
      ProfScope ps("stage2_kron_attr_kernel", st);
      hipLaunchKernelGGL(stage2_kron_attr_kernel, dim3(p.P, p.m), dim3(256), 0, st, p);
      break;
    }
    default: return MMF_ERR_ARG;
  }
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

// ---- highway with n_layers >= 2: layer 0 folds, layers >= 1 run per window of (patient, node) rows ----------------------
// Rows as for kronecker: g = patient * T + node.  Between these launches the window's layers >= 1 run through the dense row
// kernels and the highway mix (csrc/mmf_mlp.hip).  Activations lie block by block (one Highway each): unit j of row s at
// [(j / wd) * blk_stride + s * wd + j % wd].
__device__ inline size_t s2_hw_at(const S2HwParams& p, int s, int j) {
  return (size_t)(j / p.wd) * p.blk_stride + (size_t)s * p.wd + j % p.wd;
}

// layer 0 of every row: x0 = sigmoid(zg) relu(zn) + (1 - sigmoid(zg)) zl, z_* = alpha_node U_* + c_*
__global__ __launch_bounds__(256) void stage2_hw_begin_kernel(S2HwParams p) {
  const int s = blockIdx.x, g = p.g0 + s, pt = g / p.T, k = g % p.T, W = p.W;
  const float a = p.alpha[k];
  const float* Up = p.U + (size_t)pt * p.ldU;
  const float* Uc = p.U + (size_t)p.P * p.ldU;
  for (int j = threadIdx.x; j < W; j += 256) {
    const float zg = fmaf(a, Up[j], Uc[j]), zn = fmaf(a, Up[W + j], Uc[W + j]), zl = fmaf(a, Up[2 * W + j], Uc[2 * W + j]);
    const float gt = 1.0f / (1.0f + __expf(-zg));
    p.X0[s2_hw_at(p, s, j)] = gt * fmaxf(zn, 0.f) + (1.0f - gt) * zl;
  }
}

// one workgroup per row: bn2 of the last layer's output into LDS, the classifier, the hazard head and the backward of risk
// (or the cox scalar), the risk where the row's place in the call says, d risk / d (last layer's output)
__global__ __launch_bounds__(256) void stage2_hw_head_kernel(S2HwParams p) {
  __shared__ float act[S2_MAXW];
  __shared__ float lg[32], hz[32], sv[32], dl[32];
  __shared__ float part[4];
  const int s = blockIdx.x, g = p.g0 + s, pt = g / p.T, k = g % p.T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = p.W, K = p.K;
  for (int j = tid; j < W; j += 256) {
    float sc, sh;
    s2_bn_affine(p.bn2[j / p.wd], j % p.wd, sc, sh);
    act[j] = fmaf(sc, p.XL[s2_hw_at(p, s, j)], sh);
  }
  __syncthreads();
  if (p.cox) {
    float d = 0.f;
    for (int j = tid; j < W; j += 256) d = fmaf(p.Wk[j], act[j], d);
    d = wave_sum(d);
    if (lane == 0) part[wave] = d;
    __syncthreads();
    if (tid == 0) {
      const float risk = ((part[0] + part[1]) + part[2]) + part[3] + p.bk[0];
      if (k < p.n_steps) p.step_risk[(size_t)pt * p.n_steps + k] = risk;
      else if (k == p.n_steps) p.risk[pt] = risk;
      else p.risk_base[pt] = risk;
    }
  } else {
    IgHeadParams hp{};
    hp.Wk = p.Wk; hp.bk = p.bk; hp.K = K; hp.H = W; hp.step0 = 0; hp.n_steps = p.n_steps;
    hp.step_risk = p.step_risk + (size_t)pt * p.n_steps; hp.risk_x = p.risk + pt; hp.risk_base = p.risk_base + pt;
    hp.hazards = p.hazards ? p.hazards + (size_t)pt * K : nullptr;
    hp.S = p.S_out ? p.S_out + (size_t)pt * K : nullptr;
    ig_hazard_body<4>(hp, act, k, lg, hz, sv, dl);
  }
  for (int j = tid; j < W; j += 256) {
    float sc, sh, da;
    s2_bn_affine(p.bn2[j / p.wd], j % p.wd, sc, sh);
    if (p.cox) da = p.Wk[j];
    else {
      da = 0.f;
      for (int q = 0; q < K; ++q) da = fmaf(dl[q], p.Wk[(size_t)q * W + j], da);
    }
    p.dXL[s2_hw_at(p, s, j)] = sc * da;
  }
}

// out = a + b + c: the three input gradients of a layer (gate, nonlinear, linear), in that order
__global__ __launch_bounds__(256) void stage2_hw_add3_kernel(const float* a, const float* b, const float* c, float* out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (a[i] + b[i]) + c[i];
}

// G[patient] (=, or += when the patient's node 0 lies in an earlier window) sum over the patient's quadrature rows of the
// window, in node order, of w_node d risk / d z_* of layer 0, rebuilt from U: one thread per patient and unit
__global__ __launch_bounds__(256) void stage2_hw_end_kernel(S2HwParams p) {
  const int pt = p.g0 / p.T + blockIdx.x, j = blockIdx.y * 256 + threadIdx.x, W = p.W;
  if (j >= W) return;
  const int g_beg = pt * p.T > p.g0 ? pt * p.T : p.g0;
  const int g_stop = pt * p.T + p.n_steps < p.g0 + p.S ? pt * p.T + p.n_steps : p.g0 + p.S;
  if (g_beg >= g_stop) return;
  const float* Up = p.U + (size_t)pt * p.ldU;
  const float* Uc = p.U + (size_t)p.P * p.ldU;
  const float ug = Up[j], un = Up[W + j], ul = Up[2 * W + j], cg = Uc[j], cn = Uc[W + j], cl = Uc[2 * W + j];
  float* G = p.G + (size_t)pt * p.ldU;
  const bool first = g_beg == pt * p.T;
  float a0 = first ? 0.f : G[j], a1 = first ? 0.f : G[W + j], a2 = first ? 0.f : G[2 * W + j];
  for (int g = g_beg; g < g_stop; ++g) {
    const float a = p.alpha[g - pt * p.T], wq = p.weight[g - pt * p.T];
    const float zg = fmaf(a, ug, cg), zn = fmaf(a, un, cn), zl = fmaf(a, ul, cl);
    const float gt = 1.0f / (1.0f + __expf(-zg)), dy = p.dX0[s2_hw_at(p, g - p.g0, j)];
    a0 = fmaf(wq, dy * (fmaxf(zn, 0.f) - zl) * gt * (1.0f - gt), a0);
    a1 = fmaf(wq, zn > 0.f ? dy * gt : 0.f, a1);
    a2 = fmaf(wq, dy * (1.0f - gt), a2);
  }
  G[j] = a0; G[W + j] = a1; G[2 * W + j] = a2;
}

int launch_stage2_hw(int stage, const S2HwParams& p, hipStream_t st) {
  if (!p.U || p.P < 1 || p.n_steps < 1 || p.n_steps > GROUP_MAX || p.T != p.n_steps + 2 || p.S < 1 || p.S > S2_HW_ROWS ||
      p.g0 < 0 || (int64_t)p.g0 + p.S > (int64_t)p.P * p.T || p.W < 1 || p.W > S2_MAXW || p.wd < 1 || p.W % p.wd ||
      p.W / p.wd > 3 || p.ldU != 3 * p.W || p.blk_stride < (size_t)p.S * p.wd || p.K < 1 || p.K > 32 || (p.cox && p.K != 1))
    return MMF_ERR_SHAPE;
  const int p_first = p.g0 / p.T, p_last = (p.g0 + p.S - 1) / p.T;
  switch (stage) {
    case S2_HW_BEGIN: {
      if (!p.X0) return MMF_ERR_ARG;
      ProfScope ps("stage2_hw_begin_kernel", st);
      hipLaunchKernelGGL(stage2_hw_begin_kernel, dim3(p.S), dim3(256), 0, st, p);
      break;
    }
    case S2_HW_HEAD: {
      if (!p.XL || !p.dXL || !p.Wk || !p.bk || !p.step_risk || !p.risk || !p.risk_base) return MMF_ERR_ARG;
      for (int b = 0; b < p.W / p.wd; ++b)
        if (!p.bn2[b].w || !p.bn2[b].b || !p.bn2[b].mean || !p.bn2[b].var) return MMF_ERR_ARG;
      ProfScope ps("stage2_hw_head_kernel", st);
      hipLaunchKernelGGL(stage2_hw_head_kernel, dim3(p.S), dim3(256), 0, st, p);
      break;
    }
    case S2_HW_END: {
      if (!p.dX0 || !p.G) return MMF_ERR_ARG;
      ProfScope ps("stage2_hw_end_kernel", st);
      hipLaunchKernelGGL(stage2_hw_end_kernel, dim3(p_last - p_first + 1, (p.W + 255) / 256), dim3(256), 0, st, p);
      break;
    }
    default: return MMF_ERR_ARG;
  }
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

int launch_stage2_hw_add3(const float* a, const float* b, const float* c, float* out, int n, hipStream_t st) {
  if (!a || !b || !c || !out || n < 1) return MMF_ERR_ARG;
  ProfScope ps("stage2_hw_add3_kernel", st);
  hipLaunchKernelGGL(stage2_hw_add3_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a, b, c, out, n);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

}  // namespace mmf
