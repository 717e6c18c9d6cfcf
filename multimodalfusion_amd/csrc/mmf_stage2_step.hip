// One training step of the stage-2 fcnn and highway models (mmf_stage2_step): forward, loss, every parameter gradient and
// the BatchNorm running statistics of early-fcnn, late-fcnn, early-highway and late-highway, both families
// (models/nll_models_pretrained.py:66-197, models/coxranking_models_pretrained.py:62-200, utils/loss_utils.py and the
// backward autograd derives from them).
//
// No workgroup waits for another: launch boundaries are the only ordering between workgroups.  BatchNorm needs a feature's
// statistics over the whole batch, so the unit of work is a COLUMN OWNER: a workgroup of 256 threads owns S2S_NC = 4
// features for all B <= 256 rows, thread b is row b.  What it owns it finishes without leaving the CU:
//   forward   the contraction that produces its features (the weights' rows staged in LDS, the row's operand streamed),
//             the batch statistics (two passes over registers), BN, ReLU or the highway mix, dropout, the running statistics;
//   backward  the gradient that arrives at its features (from the classifier, or sum_n dz[:, n] W[n, j] of the layer above),
//             the BN / mix / dropout backward, dgamma, dbeta, db and its rows of dW = dpre^T x: each one thread's or one
//             workgroup's ordered sum over the batch.
// Activations a later launch contracts over lie FEATURE-MAJOR ([feature x ldB], thread b reads its row coalesced); the ones
// a dW needs lie row-major as well ([B x D], thread k reads coalesced).
//
//   s2s_fcnn_fwd_kernel   u = x W0^T + b0, statistics, y = drop(relu(bn(u))); every block of a late type in one launch
//   s2s_bn1_fwd_kernel    Highway: x0 = drop(bn1(h))
//   s2s_hw_fwd_kernel     one Highway layer: the three contractions and the mix; bn2 folded into the last layer
//   s2s_head_kernel       row tiles of 64: the classifier (cox late-fcnn: the blocks' Linear(128, 1) first), hazards, S,
//                         risk; as ONE workgroup it also takes the loss (a forward-only call ends here)
//   s2s_fcnn_bwd_kernel   every workgroup rebuilds d loss / d logits of all rows (<= 256^2 pair terms); its columns' dy,
//                         dropout / ReLU / BN backward, dW0 rows, db0; the classifier's gradient by output element
//   s2s_hw_bwd_kernel     TOP: the same from the classifier, bn2's backward, the last layer's mix backward, dz, dW rows;
//                         MID: dx[:, j] = sum dz_* W_* of the layer above, this layer's mix backward, dz, dW rows;
//                         BN1: dx[:, j] of layer 0, dropout and bn1's backward
// No atomics; every sum runs in an order fixed by its output element: two calls agree bit for bit.
#include "mmf_common.h"
#include "mmf_kernels.h"

namespace mmf {

constexpr int S2S_NC = 4;          // features a workgroup owns
constexpr float S2S_NLL_EPS = 1e-7f;

// sums over the workgroup's 256 threads, the same value in every thread: the xor butterfly per wave, the waves in order
__device__ inline float s2s_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ inline void s2s_block_sum4(float (&v)[S2S_NC], float* red) {
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) v[c] = wave_sum(v[c]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) red[c * 4 + (threadIdx.x >> 6)] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) v[c] = ((red[c * 4] + red[c * 4 + 1]) + red[c * 4 + 2]) + red[c * 4 + 3];
}
__device__ inline int s2s_block_sumi(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ inline void s2s_out(float* dst, float v, int accumulate) { *dst = accumulate ? *dst + v : v; }
__device__ inline float s2s_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// a feature's batch statistics (train) or running statistics (eval); u: thread b's value, 0 beyond B.  Thread 0 moves the
// running statistics (momentum, unbiased variance) and saves (mean, invstd) for the backward
__device__ inline void s2s_bn_stats(const S2sBn& bn, int f0, const float (&u)[S2S_NC], bool on, int B, int training,
                                    float* stat, int F, float* red, float (&mean)[S2S_NC], float (&invstd)[S2S_NC]) {
  if (training) {
    float s[S2S_NC];
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) s[c] = u[c];
    s2s_block_sum4(s, red);
    float v[S2S_NC];
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) {
      mean[c] = s[c] / (float)B;
      const float d = on ? u[c] - mean[c] : 0.f;
      v[c] = d * d;
    }
    s2s_block_sum4(v, red);
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) {
      invstd[c] = rsqrtf(v[c] / (float)B + bn.eps);                      // biased: what normalises the batch
      if (threadIdx.x == 0) {
        bn.rmean[f0 + c] = (1.f - bn.momentum) * bn.rmean[f0 + c] + bn.momentum * mean[c];
        bn.rvar[f0 + c] = (1.f - bn.momentum) * bn.rvar[f0 + c] + bn.momentum * (v[c] / (float)(B - 1));   // unbiased
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) {
      mean[c] = bn.rmean[f0 + c];
      invstd[c] = rsqrtf(bn.rvar[f0 + c] + bn.eps);
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) { stat[f0 + c] = mean[c]; stat[F + f0 + c] = invstd[c]; }
  }
}

// BatchNorm1d's backward of the owned features: dgamma, dbeta (written by thread 0) and dpre -> dx in place
__device__ inline void s2s_bn_bwd(const S2sBn& bn, int f0, float (&d)[S2S_NC], const float (&xhat)[S2S_NC],
                                  const float (&invstd)[S2S_NC], int B, int training, float* dgamma, float* dbeta,
                                  int accumulate, float* red) {
  float s1[S2S_NC], s2[S2S_NC];
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) { s1[c] = d[c]; s2[c] = d[c] * xhat[c]; }
  s2s_block_sum4(s1, red);
  s2s_block_sum4(s2, red);
  const float invB = 1.0f / (float)B;
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    if (threadIdx.x == 0) {
      s2s_out(dgamma + f0 + c, s2[c], accumulate);
      s2s_out(dbeta + f0 + c, s1[c], accumulate);
    }
    const float g = bn.w[f0 + c] * invstd[c];
    d[c] = training ? g * (d[c] - invB * s1[c] - xhat[c] * invB * s2[c]) : g * d[c];
  }
}

// ---- the loss of a batch and its gradient with respect to the logits ---------------------------------------------------------
struct S2sLossLds {
  double t[256];
  float risk[256], c[256], et[256], w[256];
  float red[16];                       // s2s_block_sum4's partials
  int redi[4];
};

// Every thread of the workgroup; thread b is row b.  Returns the unscaled loss (the same in every thread) and, with dlT,
// writes d (loss * scale) / d logits[b][k] to dlT[k * 256 + b] (0 beyond B).  Ties, the all-censored batch and the batch
// without a comparable pair as mmf_cox_surv / mmf_ranking_loss / mmf_nll_surv have them.
__device__ inline float s2s_loss_rows(const S2sLoss& q, S2sLossLds& s, float* dlT) {
  const int b = threadIdx.x, B = q.B, K = q.K;
  const bool on = b < B;
  const bool has_rank = q.kind == S2S_LOSS_RANK || q.kind == S2S_LOSS_RANK_NLL;
  const bool has_nll = q.kind == S2S_LOSS_NLL || q.kind == S2S_LOSS_RANK_NLL;
  const float invB = 1.0f / (float)B;
  if (on) {
    s.risk[b] = q.risk[b];
    s.c[b] = q.c[b];
    s.t[b] = q.kind == S2S_LOSS_RANK_NLL ? (double)q.Y[b] : has_nll ? 0.0 : q.times[b];
  }
  __syncthreads();
  float g = 0.f, total = 0.f;               // d loss / d risk[b]
  if (q.kind == S2S_LOSS_COX) {
    if (on) s.et[b] = expf(s.risk[b]);
    __syncthreads();
    float l = 0.f;
    if (on) {
      const double ti = s.t[b];
      float Di = 0.f;
      for (int j = 0; j < B; ++j) Di += (s.t[j] >= ti) ? s.et[j] : 0.f;
      const float unc = 1.f - s.c[b];
      l = (s.risk[b] - logf(Di)) * unc;
      s.w[b] = unc / Di;
    }
    __syncthreads();
    if (on) {
      const double tk = s.t[b];
      float acc = 0.f;
      for (int i = 0; i < B; ++i) acc += (tk >= s.t[i]) ? s.w[i] : 0.f;
      g = -invB * ((1.f - s.c[b]) - s.et[b] * acc);
    }
    total = -s2s_block_sum(l, s.red) * invB;
  } else if (has_rank) {
    float sum = 0.f, gi = 0.f;
    int cnt = 0;
    if (on) {
      const int i = b;
      const double ti = s.t[i];
      const bool ei = (1.f - s.c[i]) != 0.f;
      const float ri = s.risk[i];
      for (int j = 0; j < B; ++j) {
        if (j == i) continue;
        const double tj = s.t[j];
        const bool ej = (1.f - s.c[j]) != 0.f;
        const bool i_is_a = i < j;                   // the reference's index-ordered rule: a = min(i, j), b = max(i, j)
        const double ta = i_is_a ? ti : tj, tb = i_is_a ? tj : ti;
        const bool ea = i_is_a ? ei : ej, eb = i_is_a ? ej : ei;
        int more;
        if (ta < tb && ea) more = 0;
        else if (tb < ta && eb) more = 1;
        else continue;
        const bool i_more = (more == 0) == i_is_a;
        const float r = i_more ? ri - s.risk[j] : s.risk[j] - ri;
        float phi, dphi;
        if (q.phi == 0) { phi = 1.0f / (1.0f + expf(-r)); dphi = phi * (1.f - phi); }
        else { phi = fmaxf(r, 0.f); dphi = r > 0.f ? 1.f : 0.f; }
        gi += i_more ? dphi : -dphi;
        if (i_is_a) { sum += phi; ++cnt; }
      }
    }
    const float S = s2s_block_sum(sum, s.red);
    const int n = s2s_block_sumi(cnt, s.redi);
    const float scale = n == 0 ? 0.f : (q.reduction == 0 ? -1.0f / (float)n : -1.0f);
    total = n == 0 ? 0.f : S * scale;
    g = gi * scale;
  }
  // nll_surv's terms of row b: the value, and its gradients with respect to S[y - 1], S[y] and hazards[y]
  float gS_ym1 = 0.f, gS_y = 0.f, gH_y = 0.f;
  int y = -1;
  if (has_nll) {
    const float ratio = q.kind == S2S_LOSS_RANK_NLL ? q.ratio : 1.f;
    float l = 0.f;
    if (on) {
      const int64_t y64 = q.Y[b];
      if (y64 < 0 || y64 >= K) {
        l = __builtin_nanf("");                         // as mmf_nll_surv: NaN loss, no gradient from this row
      } else {
        y = (int)y64;
        const float* hz = q.hazards + (size_t)b * K;
        const float* Sv = q.S + (size_t)b * K;
        const float c = s.c[b], coef = ratio * invB;
        const float sp_y = y == 0 ? 1.0f : Sv[y - 1], hy = hz[y], sp_y1 = Sv[y];
        const float unc = -(1.f - c) * (logf(fmaxf(sp_y, S2S_NLL_EPS)) + logf(fmaxf(hy, S2S_NLL_EPS)));
        const float cen = -c * logf(fmaxf(sp_y1, S2S_NLL_EPS));
        if (y > 0 && sp_y >= S2S_NLL_EPS) gS_ym1 = -(1.f - c) / sp_y * coef;
        if (hy >= S2S_NLL_EPS) gH_y = -(1.f - c) / hy * coef;
        if (sp_y1 >= S2S_NLL_EPS) gS_y = -(1.f - q.alpha) * c / sp_y1 * coef;
        l = (1.f - q.alpha) * (cen + unc) + q.alpha * unc;
      }
    }
    total += ratio * (s2s_block_sum(l, s.red) * invB);
  }
  if (!dlT) return total;
  if (q.cox) {
    dlT[b] = on ? g * q.scale : 0.f;
    return total;
  }
  // the hazard head's backward (hazard_bwd_kernel): d S_j / d h_t = -prod_{u <= j, u != t} (1 - h_u) for j >= t
  const float* hz = q.hazards + (size_t)(on ? b : 0) * K;
  float pre = 1.f;
  for (int t = 0; t < K; ++t) {
    float dl = 0.f;
    if (on) {
      if (t > 0) pre *= 1.f - hz[t - 1];
      float prod = pre, acc = 0.f;
      for (int j = t; j < K; ++j) {
        if (j > t) prod *= 1.f - hz[j];
        const float gS = (j == y - 1 ? gS_ym1 : 0.f) + (j == y ? gS_y : 0.f) - g;
        acc -= gS * prod;
      }
      const float gh = (t == y ? gH_y : 0.f) + acc;
      dl = gh * hz[t] * (1.f - hz[t]) * q.scale;
    }
    dlT[t * 256 + b] = dl;
  }
  return total;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void s2s_fcnn_fwd_kernel(S2sFcnnFwd p) {
  __shared__ __align__(16) float Ws[S2S_NC][768];
  __shared__ float red[16];
  const S2sFcnnFwdBr& br = p.br[blockIdx.y];
  const int tid = threadIdx.x, b = tid, n0 = blockIdx.x * S2S_NC, kin = br.nseg * 256;
  const bool on = b < p.B;
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c)
    for (int k = tid; k < kin; k += 256) Ws[c][k] = br.W0[(size_t)(n0 + c) * kin + k];
  __syncthreads();
  float acc[S2S_NC] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    for (int sg = 0; sg < br.nseg; ++sg) {
      const float* xr = br.x[sg] + (size_t)b * 256;
#pragma unroll 8
      for (int k = 0; k < 256; k += 4) {
        const float4 xv = ld4(xr + k);
#pragma unroll
        for (int c = 0; c < S2S_NC; ++c) {
          const float4 w = ld4(&Ws[c][sg * 256 + k]);
          acc[c] = fmaf(xv.x, w.x, acc[c]); acc[c] = fmaf(xv.y, w.y, acc[c]);
          acc[c] = fmaf(xv.z, w.z, acc[c]); acc[c] = fmaf(xv.w, w.w, acc[c]);
        }
      }
    }
  }
  float u[S2S_NC], mean[S2S_NC], invstd[S2S_NC];
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) u[c] = on ? acc[c] + br.b0[n0 + c] : 0.f;
  s2s_bn_stats(br.bn, n0, u, on, p.B, p.training, br.stat, 128, red, mean, invstd);
  if (!on) return;
  const bool drop = p.training && p.p > 0.f;
  const uint32_t key = br.key + (p.seed_dev ? *p.seed_dev : 0u), thr = drop_threshold(p.p);
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    const int n = n0 + c;
    float y = fmaxf((u[c] - mean[c]) * invstd[c] * br.bn.w[n] + br.bn.b[n], 0.f);
    if (drop) y = keep(key, (uint32_t)(b * 128 + n), thr) ? y / (1.0f - p.p) : 0.f;
    br.uT[(size_t)n * p.ldB + b] = u[c];
    if (br.yT) br.yT[(size_t)n * p.ldB + b] = y;
  }
}

__global__ __launch_bounds__(256) void s2s_bn1_fwd_kernel(S2sBn1Fwd p) {
  __shared__ float red[16];
  const S2sBn1FwdBr& br = p.br[blockIdx.y];
  const int tid = threadIdx.x, b = tid, j0 = blockIdx.x * S2S_NC, D = p.D;
  const bool on = b < p.B;
  float u[S2S_NC] = {0.f, 0.f, 0.f, 0.f}, mean[S2S_NC], invstd[S2S_NC];
  if (on) {
    const float4 v = ld4(br.x[j0 / 256] + (size_t)b * 256 + j0 % 256);
    u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
  }
  s2s_bn_stats(br.bn, j0, u, on, p.B, p.training, br.stat, D, red, mean, invstd);
  if (!on) return;
  const bool drop = p.training && p.p > 0.f;
  const uint32_t key = br.key + (p.seed_dev ? *p.seed_dev : 0u), thr = drop_threshold(p.p);
  float y[S2S_NC];
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    const int j = j0 + c;
    y[c] = (u[c] - mean[c]) * invstd[c] * br.bn.w[j] + br.bn.b[j];
    if (drop) y[c] = keep(key, (uint32_t)(b * D + j), thr) ? y[c] / (1.0f - p.p) : 0.f;
    br.xT[(size_t)j * p.ldB + b] = y[c];
  }
  st4(br.xR + (size_t)b * D + j0, make_float4(y[0], y[1], y[2], y[3]));
}

__global__ __launch_bounds__(256) void s2s_hw_fwd_kernel(S2sHwFwd p) {
  __shared__ __align__(16) float Wst[256 * 12];                 // [k of the chunk][gate | nonlinear | linear][owned feature]
  __shared__ float red[16];
  const S2sHwFwdBr& br = p.br[blockIdx.y];
  const int tid = threadIdx.x, b = tid, n0 = blockIdx.x * S2S_NC, D = p.D;
  const bool on = b < p.B;
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < D; k0 += 256) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 12; ++i) Wst[tid * 12 + i] = br.W[i / 4][(size_t)(n0 + i % 4) * D + k0 + tid];
    __syncthreads();
    if (on) {
      const float* xc = br.xT + (size_t)k0 * p.ldB + b;
#pragma unroll 16
      for (int kk = 0; kk < 256; ++kk) {
        const float xv = xc[(size_t)kk * p.ldB];
        const float4 w0 = ld4(&Wst[kk * 12]), w1 = ld4(&Wst[kk * 12 + 4]), w2 = ld4(&Wst[kk * 12 + 8]);
        acc[0] = fmaf(xv, w0.x, acc[0]); acc[1] = fmaf(xv, w0.y, acc[1]); acc[2] = fmaf(xv, w0.z, acc[2]); acc[3] = fmaf(xv, w0.w, acc[3]);
        acc[4] = fmaf(xv, w1.x, acc[4]); acc[5] = fmaf(xv, w1.y, acc[5]); acc[6] = fmaf(xv, w1.z, acc[6]); acc[7] = fmaf(xv, w1.w, acc[7]);
        acc[8] = fmaf(xv, w2.x, acc[8]); acc[9] = fmaf(xv, w2.y, acc[9]); acc[10] = fmaf(xv, w2.z, acc[10]); acc[11] = fmaf(xv, w2.w, acc[11]);
      }
    }
  }
  float y[S2S_NC];
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    const int n = n0 + c;
    y[c] = 0.f;
    if (on) {
      const float zg = acc[c] + br.bias[0][n], zn = acc[4 + c] + br.bias[1][n], zl = acc[8 + c] + br.bias[2][n];
      const float g = s2s_sigmoid(zg);
      y[c] = g * fmaxf(zn, 0.f) + (1.f - g) * zl;
      br.zT[0][(size_t)n * p.ldB + b] = zg;
      br.zT[1][(size_t)n * p.ldB + b] = zn;
      br.zT[2][(size_t)n * p.ldB + b] = zl;
      br.yT[(size_t)n * p.ldB + b] = y[c];
    }
  }
  if (!p.last) {
    if (on) st4(br.yR + (size_t)b * D + n0, make_float4(y[0], y[1], y[2], y[3]));
    return;
  }
  float mean[S2S_NC], invstd[S2S_NC];
  s2s_bn_stats(br.bn2, n0, y, on, p.B, p.training, br.stat2, D, red, mean, invstd);
  if (!on || !br.fT) return;
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    const int n = n0 + c;
    br.fT[(size_t)n * p.ldB + b] = (y[c] - mean[c]) * invstd[c] * br.bn2.w[n] + br.bn2.b[n];
  }
}

__global__ __launch_bounds__(256) void s2s_head_kernel(S2sHead p) {
  __shared__ float lg[64][33];
  __shared__ S2sLossLds ll;
  const int tid = threadIdx.x, r = tid & 63, kg = tid >> 6, K = p.K, W = p.W;
  for (int r0 = blockIdx.x * 64; r0 < p.B; r0 += gridDim.x * 64) {
    const int b = r0 + r;
    const bool on = b < p.B;
    if (p.late_cox) {
      if (on && kg < p.m) {
        float sv = p.b4[kg][0];
#pragma unroll 16
        for (int j = 0; j < 128; ++j) sv = fmaf(p.W4[kg][j], p.fT[(size_t)(kg * 128 + j) * p.ldB + b], sv);
        lg[r][kg] = sv;
        p.sblk[b * 3 + kg] = sv;
      }
      __syncthreads();
      if (on && kg == 0) {
        float z = p.bk[0];
        for (int i = 0; i < p.m; ++i) z = fmaf(p.Wk[i], lg[r][i], z);
        p.risk[b] = z;
      }
    } else {
      if (on) {
        for (int k = kg; k < K; k += 4) {
          const float* wk = p.Wk + (size_t)k * W;
          float z = p.bk[k];
#pragma unroll 16
          for (int j = 0; j < W; ++j) z = fmaf(wk[j], p.fT[(size_t)j * p.ldB + b], z);
          lg[r][k] = z;
        }
      }
      __syncthreads();
      if (on && kg == 0) {
        if (p.cox) {
          p.risk[b] = lg[r][0];
        } else {
          float sv = 1.f, rs = 0.f;
          for (int k = 0; k < K; ++k) {
            const float h = s2s_sigmoid(lg[r][k]);
            sv *= 1.f - h;
            p.hazards[(size_t)b * K + k] = h;
            p.S[(size_t)b * K + k] = sv;
            rs += sv;
          }
          p.risk[b] = -rs;
        }
      }
    }
    __syncthreads();
  }
  if (p.with_loss) {                       // one workgroup holds every row: the forward-only call ends with the loss
    __syncthreads();
    const float total = s2s_loss_rows(p.loss, ll, nullptr);
    if (tid == 0) p.loss.loss[0] = total;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// dWk[k][col] of the owned columns = sum_b dl[b][k] f[b][col] (fc: the columns' activations, [c][b]); dbk by the call's
// first workgroup
__device__ inline void s2s_classifier_grads(const float* dlT, const float* fc, int B, int K, int W, int col0, float* dWk,
                                            float* dbk, bool first, int accumulate) {
  const int tid = threadIdx.x;
  if (tid < K * S2S_NC) {
    const int k = tid / S2S_NC, c = tid % S2S_NC;
    float a = 0.f;
    for (int bb = 0; bb < B; ++bb) a = fmaf(dlT[k * 256 + bb], fc[c * 256 + bb], a);
    s2s_out(dWk + (size_t)k * W + col0 + c, a, accumulate);
  } else if (first && tid >= 128 && tid - 128 < K) {
    const int k = tid - 128;
    float a = 0.f;
    for (int bb = 0; bb < B; ++bb) a += dlT[k * 256 + bb];
    s2s_out(dbk + k, a, accumulate);
  }
}

__global__ __launch_bounds__(256) void s2s_fcnn_bwd_kernel(S2sFcnnBwd p) {
  __shared__ float dlT[32 * 256];
  __shared__ float fc[S2S_NC * 256];
  __shared__ __align__(16) float cb[256 * S2S_NC];             // du of the owned features, [b][c]
  __shared__ S2sLossLds ll;
  const S2sFcnnBwdBr& br = p.br[blockIdx.y];
  const int tid = threadIdx.x, b = tid, n0 = blockIdx.x * S2S_NC, B = p.B, K = p.loss.K;
  const bool on = b < B, first = blockIdx.x == 0 && blockIdx.y == 0;
  const float total = s2s_loss_rows(p.loss, ll, dlT);
  if (first && tid == 0) p.loss.loss[0] = total;
  const int col0 = br.ycol0 + n0;
  float yv[S2S_NC], d[S2S_NC];
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    yv[c] = on ? p.yT[(size_t)(col0 + c) * p.ldB + b] : 0.f;
    fc[c * 256 + b] = yv[c];
  }
  __syncthreads();
  if (p.late_cox) {
    const float wk = p.Wk[br.slot];
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) d[c] = dlT[b] * wk * br.W4[n0 + c];
    if (tid < S2S_NC) {
      float a = 0.f;
      for (int bb = 0; bb < B; ++bb) a = fmaf(dlT[bb], fc[tid * 256 + bb], a);
      s2s_out(br.dW4 + n0 + tid, wk * a, p.accumulate);
    } else if (blockIdx.x == 0 && tid == 64) {
      float a = 0.f, sd = 0.f;
      for (int bb = 0; bb < B; ++bb) { a = fmaf(dlT[bb], p.sblk[bb * 3 + br.slot], a); sd += dlT[bb]; }
      s2s_out(p.dWk + br.slot, a, p.accumulate);
      s2s_out(br.db4, wk * sd, p.accumulate);
    } else if (first && tid == 128) {
      float sd = 0.f;
      for (int bb = 0; bb < B; ++bb) sd += dlT[bb];
      s2s_out(p.dbk, sd, p.accumulate);
    }
  } else {
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) {
      float a = 0.f;
      for (int k = 0; k < K; ++k) a = fmaf(dlT[k * 256 + b], p.Wk[(size_t)k * p.W + col0 + c], a);
      d[c] = a;
    }
    s2s_classifier_grads(dlT, fc, B, K, p.W, col0, p.dWk, p.dbk, first, p.accumulate);
  }
  // dropout and ReLU (the dropped output is positive where both let the value through), then BatchNorm
  const float dscale = (p.training && p.p > 0.f) ? 1.0f / (1.0f - p.p) : 1.0f;
  float xhat[S2S_NC], invstd[S2S_NC];
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    const int n = n0 + c;
    invstd[c] = br.stat[128 + n];
    d[c] = on && yv[c] > 0.f ? d[c] * dscale : 0.f;
    xhat[c] = on ? (br.uT[(size_t)n * p.ldB + b] - br.stat[n]) * invstd[c] : 0.f;
  }
  s2s_bn_bwd(br.bn, n0, d, xhat, invstd, B, p.training, br.dgamma, br.dbeta, p.accumulate, ll.red);
  float s[S2S_NC];
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) { d[c] = on ? d[c] : 0.f; s[c] = d[c]; cb[b * S2S_NC + c] = d[c]; }
  s2s_block_sum4(s, ll.red);                       // its barriers also publish cb
  if (tid < S2S_NC) s2s_out(br.db0 + n0 + tid, s[tid], p.accumulate);
  const int kin = br.nseg * 256;
  for (int k = tid; k < kin; k += 256) {
    const float* xc = br.x[k / 256] + k % 256;
    float a[S2S_NC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int bb = 0; bb < B; ++bb) {
      const float xv = xc[(size_t)bb * 256];
      const float4 dv = ld4(&cb[bb * S2S_NC]);
      a[0] = fmaf(dv.x, xv, a[0]); a[1] = fmaf(dv.y, xv, a[1]); a[2] = fmaf(dv.z, xv, a[2]); a[3] = fmaf(dv.w, xv, a[3]);
    }
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) s2s_out(br.dW0 + (size_t)(n0 + c) * kin + k, a[c], p.accumulate);
  }
}

__global__ __launch_bounds__(256) void s2s_hw_bwd_kernel(S2sHwBwd p) {
  __shared__ __align__(16) float big[32 * 256];                  // TOP: dlT [K][256]; MID, BN1: the staged weights [n of the chunk][12]
  __shared__ float fc[S2S_NC * 256];
  __shared__ __align__(16) float cb[256 * 12];                   // dz of the owned features, [b][gate | nonlinear | linear][c]
  __shared__ S2sLossLds ll;
  const S2sHwBwdBr& br = p.br[blockIdx.y];
  const int tid = threadIdx.x, b = tid, j0 = blockIdx.x * S2S_NC, B = p.B, D = p.D;
  const bool on = b < B, first = blockIdx.x == 0 && blockIdx.y == 0;
  float d[S2S_NC] = {0.f, 0.f, 0.f, 0.f};
  if (p.mode == S2S_HW_TOP) {
    const int K = p.loss.K, col0 = br.fcol0 + j0;
    const float total = s2s_loss_rows(p.loss, ll, big);
    if (first && tid == 0) p.loss.loss[0] = total;
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) fc[c * 256 + b] = on ? br.fT[(size_t)(j0 + c) * p.ldB + b] : 0.f;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) {
      float a = 0.f;
      for (int k = 0; k < K; ++k) a = fmaf(big[k * 256 + b], p.Wk[(size_t)k * p.W + col0 + c], a);
      d[c] = on ? a : 0.f;
    }
    s2s_classifier_grads(big, fc, B, K, p.W, col0, p.dWk, p.dbk, first, p.accumulate);
    float xhat[S2S_NC], invstd[S2S_NC];
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) {
      invstd[c] = br.stat2[D + j0 + c];
      xhat[c] = on ? (br.yT[(size_t)(j0 + c) * p.ldB + b] - br.stat2[j0 + c]) * invstd[c] : 0.f;
    }
    s2s_bn_bwd(br.bn2, j0, d, xhat, invstd, B, p.training, br.dgamma2, br.dbeta2, p.accumulate, ll.red);
  } else {
    for (int n0 = 0; n0 < D; n0 += 256) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 3; ++q) st4(&big[tid * 12 + q * 4], ld4(br.Wup[q] + (size_t)(n0 + tid) * D + j0));
      __syncthreads();
      if (on) {
        const float* g0 = br.dzT_in[0] + (size_t)n0 * p.ldB + b;
        const float* g1 = br.dzT_in[1] + (size_t)n0 * p.ldB + b;
        const float* g2 = br.dzT_in[2] + (size_t)n0 * p.ldB + b;
#pragma unroll 8
        for (int nn = 0; nn < 256; ++nn) {
          const float a0 = g0[(size_t)nn * p.ldB], a1 = g1[(size_t)nn * p.ldB], a2 = g2[(size_t)nn * p.ldB];
          const float4 w0 = ld4(&big[nn * 12]), w1 = ld4(&big[nn * 12 + 4]), w2 = ld4(&big[nn * 12 + 8]);
          d[0] = fmaf(a0, w0.x, d[0]); d[1] = fmaf(a0, w0.y, d[1]); d[2] = fmaf(a0, w0.z, d[2]); d[3] = fmaf(a0, w0.w, d[3]);
          d[0] = fmaf(a1, w1.x, d[0]); d[1] = fmaf(a1, w1.y, d[1]); d[2] = fmaf(a1, w1.z, d[2]); d[3] = fmaf(a1, w1.w, d[3]);
          d[0] = fmaf(a2, w2.x, d[0]); d[1] = fmaf(a2, w2.y, d[1]); d[2] = fmaf(a2, w2.z, d[2]); d[3] = fmaf(a2, w2.w, d[3]);
        }
      }
    }
  }
  if (p.mode == S2S_HW_BN1) {
    // x0 = drop(bn1(h)): the mask again, then bn1's backward; the embeddings are leaves, so no dx
    const bool drop = p.training && p.p > 0.f;
    const uint32_t key = br.key + (p.seed_dev ? *p.seed_dev : 0u), thr = drop_threshold(p.p);
    float xhat[S2S_NC], invstd[S2S_NC], h[S2S_NC] = {0.f, 0.f, 0.f, 0.f};
    if (on) {
      const float4 v = ld4(br.x[j0 / 256] + (size_t)b * 256 + j0 % 256);
      h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < S2S_NC; ++c) {
      const int j = j0 + c;
      invstd[c] = br.stat1[D + j];
      xhat[c] = on ? (h[c] - br.stat1[j]) * invstd[c] : 0.f;
      if (!on) d[c] = 0.f;
      else if (drop) d[c] = keep(key, (uint32_t)(b * D + j), thr) ? d[c] / (1.0f - p.p) : 0.f;
    }
    s2s_bn_bwd(br.bn1, j0, d, xhat, invstd, B, p.training, br.dgamma1, br.dbeta1, p.accumulate, ll.red);
    return;
  }
  // the mix's backward at the owned features, dz for the launch below, db and the dW rows
#pragma unroll
  for (int c = 0; c < S2S_NC; ++c) {
    const size_t o = (size_t)(j0 + c) * p.ldB + b;
    float dg = 0.f, dn = 0.f, dl = 0.f;
    if (on) {
      const float zg = br.zT[0][o], zn = br.zT[1][o], zl = br.zT[2][o];
      const float g = s2s_sigmoid(zg);
      dg = d[c] * (fmaxf(zn, 0.f) - zl) * g * (1.f - g);
      dn = zn > 0.f ? d[c] * g : 0.f;
      dl = d[c] * (1.f - g);
      br.dzT_out[0][o] = dg; br.dzT_out[1][o] = dn; br.dzT_out[2][o] = dl;
    }
    cb[b * 12 + c] = dg; cb[b * 12 + 4 + c] = dn; cb[b * 12 + 8 + c] = dl;
  }
  __syncthreads();
  if (tid < 12) {
    float a = 0.f;
    for (int bb = 0; bb < B; ++bb) a += cb[bb * 12 + tid];
    s2s_out(br.db[tid / 4] + j0 + tid % 4, a, p.accumulate);
  }
  for (int k = tid; k < D; k += 256) {
    float a[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) a[i] = 0.f;
#pragma unroll 8
    for (int bb = 0; bb < B; ++bb) {
      const float xv = br.xR[(size_t)bb * D + k];
      const float4 c0 = ld4(&cb[bb * 12]), c1 = ld4(&cb[bb * 12 + 4]), c2 = ld4(&cb[bb * 12 + 8]);
      a[0] = fmaf(c0.x, xv, a[0]); a[1] = fmaf(c0.y, xv, a[1]); a[2] = fmaf(c0.z, xv, a[2]); a[3] = fmaf(c0.w, xv, a[3]);
      a[4] = fmaf(c1.x, xv, a[4]); a[5] = fmaf(c1.y, xv, a[5]); a[6] = fmaf(c1.z, xv, a[6]); a[7] = fmaf(c1.w, xv, a[7]);
      a[8] = fmaf(c2.x, xv, a[8]); a[9] = fmaf(c2.y, xv, a[9]); a[10] = fmaf(c2.z, xv, a[10]); a[11] = fmaf(c2.w, xv, a[11]);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) s2s_out(br.dW[i / 4] + (size_t)(j0 + i % 4) * D + k, a[i], p.accumulate);
  }
}

// ---- launchers: the shapes are the ABI's, checked there; these refuse what would index out of bounds ------------------------
static bool s2s_rows_ok(int B, int ldB) { return B >= 1 && B <= 256 && ldB >= B; }

int launch_s2s_fcnn_fwd(const S2sFcnnFwd& p, hipStream_t st) {
  if (!s2s_rows_ok(p.B, p.ldB) || p.nbr < 1 || p.nbr > 3 || (p.training && p.B < 2)) return MMF_ERR_SHAPE;
  for (int i = 0; i < p.nbr; ++i)
    if (p.br[i].nseg < 1 || p.br[i].nseg > 3) return MMF_ERR_SHAPE;
  ProfScope ps("s2s_fcnn_fwd_kernel", st);
  hipLaunchKernelGGL(s2s_fcnn_fwd_kernel, dim3(128 / S2S_NC, p.nbr), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}
int launch_s2s_bn1_fwd(const S2sBn1Fwd& p, hipStream_t st) {
  if (!s2s_rows_ok(p.B, p.ldB) || p.nbr < 1 || p.nbr > 3 || p.D < 256 || p.D > 768 || p.D % 256 || (p.training && p.B < 2))
    return MMF_ERR_SHAPE;
  ProfScope ps("s2s_bn1_fwd_kernel", st);
  hipLaunchKernelGGL(s2s_bn1_fwd_kernel, dim3(p.D / S2S_NC, p.nbr), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}
int launch_s2s_hw_fwd(const S2sHwFwd& p, hipStream_t st) {
  if (!s2s_rows_ok(p.B, p.ldB) || p.nbr < 1 || p.nbr > 3 || p.D < 256 || p.D > 768 || p.D % 256 || (p.training && p.B < 2))
    return MMF_ERR_SHAPE;
  ProfScope ps("s2s_hw_fwd_kernel", st);
  hipLaunchKernelGGL(s2s_hw_fwd_kernel, dim3(p.D / S2S_NC, p.nbr), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}
static bool s2s_loss_ok(const S2sLoss& q, int B) {
  return q.B == B && q.K >= 1 && q.K <= 32 && (!q.cox || q.K == 1) && q.kind >= S2S_LOSS_NLL && q.kind <= S2S_LOSS_RANK_NLL;
}
int launch_s2s_head(const S2sHead& p, hipStream_t st) {
  if (!s2s_rows_ok(p.B, p.ldB) || p.K < 1 || p.K > 32 || p.W < 1 || (p.late_cox && (p.m < 2 || p.m > 3 || p.W != 128 * p.m)) ||
      (p.with_loss && !s2s_loss_ok(p.loss, p.B)))
    return MMF_ERR_SHAPE;
  ProfScope ps("s2s_head_kernel", st);
  hipLaunchKernelGGL(s2s_head_kernel, dim3(p.with_loss ? 1 : (p.B + 63) / 64), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}
int launch_s2s_fcnn_bwd(const S2sFcnnBwd& p, hipStream_t st) {
  if (!s2s_rows_ok(p.B, p.ldB) || p.nbr < 1 || p.nbr > 3 || !s2s_loss_ok(p.loss, p.B)) return MMF_ERR_SHAPE;
  for (int i = 0; i < p.nbr; ++i)
    if (p.br[i].nseg < 1 || p.br[i].nseg > 3 || p.br[i].slot < 0 || p.br[i].slot > 2) return MMF_ERR_SHAPE;
  ProfScope ps("s2s_fcnn_bwd_kernel", st);
  hipLaunchKernelGGL(s2s_fcnn_bwd_kernel, dim3(128 / S2S_NC, p.nbr), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}
int launch_s2s_hw_bwd(const S2sHwBwd& p, hipStream_t st) {
  if (!s2s_rows_ok(p.B, p.ldB) || p.nbr < 1 || p.nbr > 3 || p.D < 256 || p.D > 768 || p.D % 256 || p.mode < S2S_HW_TOP ||
      p.mode > S2S_HW_BN1 || (p.mode == S2S_HW_TOP && !s2s_loss_ok(p.loss, p.B)))
    return MMF_ERR_SHAPE;
  ProfScope ps("s2s_hw_bwd_kernel", st);
  hipLaunchKernelGGL(s2s_hw_bwd_kernel, dim3(p.D / S2S_NC, p.nbr), dim3(256), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

}  // namespace mmf
