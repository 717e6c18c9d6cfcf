// The node launch of the tensor-fusion head's integrated gradients (mmf_mm_ig_tensor): classifier[0] + ReLU, the hazard
// head, the backward of risk = -sum(S) and classifier[0]'s input gradient for the S nodes of a window, one workgroup per
// node (models/model_mm_attention_mil.py:182-191 in eval mode and their autograd).  It stands where the concat head's
// chain has ig_head_kernel, and for three launches of the training chain (classifier[0] forward, head, classifier[0]
// backward): hid and dhid never travel through memory.
//
//   hid[n]   = relu(bc0[n] + sum_c Wc0[n][c] MM_s[c])     one wave per output, four outputs at a time: lane l adds its
//                                                         products c = l, l + 64, ... in that order, the xor butterfly
//                                                         adds the lanes, then the bias
//   head     ig_hazard_body over hid (mmf_ig_head.h): the risks, the alpha = 1 outputs, dl = d risk / d logits
//   dpre0[n] = [hid[n] > 0] sum_j dl[j] Wk[j][n]          one thread per unit, j in order, in hid's place
//   dMM_s[c] = sum_n dpre0[n] Wc0[n][c]                   four groups of 256 threads take a quarter of the units n each, in
//                                                         order, one thread per column c (Wc0 is read along c: coalesced);
//                                                         the four partial sums of a column are added in group order
//
// Latency-bound VALU work on S <= 64 workgroups: no MFMA, no atomics, no workgroup waits for another, every sum runs in an
// order fixed by its output element.
#include "mmf_common.h"
#include "mmf_kernels.h"
#include "mmf_mlp.h"
#include "mmf_ig_head.h"

namespace mmf {

constexpr int XI_MAX_N2 = 64 * DENSE_SEGS_MAXC;   // mmhid2: what xfusion_train_shape admits
constexpr int XI_MAX_NH = 1024;                   // nhid: hid is kept in LDS

__global__ __launch_bounds__(1024) void xfusion_ig_head_kernel(XIgHeadParams p) {
  __shared__ float mm[XI_MAX_N2];
  __shared__ float hid[XI_MAX_NH];
  __shared__ float part[4][XI_MAX_N2];
  __shared__ float lg[32], hz[32], sv[32], dl[32];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N2 = p.N2, NH = p.hp.H, K = p.hp.K;
  for (int c = tid; c < N2; c += 1024) mm[c] = p.MM[(size_t)s * N2 + c];
  __syncthreads();
  for (int n0 = 4 * wave; n0 < NH; n0 += 64) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    const float* w[4];                     // a row past the last unit reads the last one again and is not stored
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = p.Wc0 + (size_t)(n0 + i < NH ? n0 + i : NH - 1) * N2;
#pragma unroll 4
    for (int c = lane; c < N2; c += 64) {
      const float x = mm[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = fmaf(w[i][c], x, t[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = wave_sum(t[i]);
      if (lane == 0 && n0 + i < NH) hid[n0 + i] = fmaxf(v + p.bc0[n0 + i], 0.f);
    }
  }
  __syncthreads();
  ig_hazard_body<16>(p.hp, hid, s, lg, hz, sv, dl);
  for (int n = tid; n < NH; n += 1024) {
    float t = 0.f;
    for (int j = 0; j < K; ++j) t += dl[j] * p.hp.Wk[(size_t)j * NH + n];
    hid[n] = hid[n] > 0.f ? t : 0.f;
  }
  __syncthreads();
  const int g = tid >> 8, t256 = tid & 255;
  const int per = (NH + 3) / 4, n_beg = g * per < NH ? g * per : NH, n_end = n_beg + per < NH ? n_beg + per : NH;
  for (int c = t256; c < N2; c += 256) {
    float t = 0.f;
#pragma unroll 8
    for (int n = n_beg; n < n_end; ++n) t = fmaf(p.Wc0[(size_t)n * N2 + c], hid[n], t);
    part[g][c] = t;
  }
  __syncthreads();
  for (int c = tid; c < N2; c += 1024)
    p.dMM[(size_t)s * N2 + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

int launch_xfusion_ig_head(const XIgHeadParams& p, int S, hipStream_t st) {
  const IgHeadParams& h = p.hp;
  if (!p.MM || !p.Wc0 || !p.bc0 || !p.dMM || !h.Wk || !h.bk || !h.step_risk || !h.risk_x || !h.risk_base) return MMF_ERR_ARG;
  if (h.K < 1 || h.K > 32 || h.H < 1 || h.H > XI_MAX_NH || p.N2 < 1 || p.N2 > XI_MAX_N2 || S < 1 || S > GROUP_MAX)
    return MMF_ERR_SHAPE;
  ProfScope ps("xfusion_ig_head_kernel", st);
  hipLaunchKernelGGL(xfusion_ig_head_kernel, dim3(S), dim3(1024), 0, st, p);
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}

}  // namespace mmf
