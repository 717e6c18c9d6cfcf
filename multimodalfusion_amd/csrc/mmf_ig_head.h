// The hazard head of a quadrature node and the backward of risk = -sum_k S_k to its logits: the one device body of
// ig_head_kernel (mmf_amil_fwd.hip) and xfusion_ig_head_kernel (mmf_xfusion_ig.hip).
#pragma once
#include "mmf_common.h"
#include "mmf_kernels.h"

namespace mmf {

// One workgroup of NW waves per node s.  M: the node's embedding, p.H wide (memory or LDS); lg, hz, sv, dl: 32 floats of the
// workgroup's LDS each.  Writes the node's risk where its place in the call says (IgHeadParams) and leaves
// dl[j] = d risk / d logit_j behind a barrier.  S_k = prod_{i <= k} (1 - h_i), so d risk / d h_j = sum_{k >= j}
// prod_{i <= k, i != j} (1 - h_i): built from the products themselves, never divided by 1 - h_j.
template <int NW>
__device__ inline void ig_hazard_body(const IgHeadParams& p, const float* M, int s, float* lg, float* hz, float* sv,
                                      float* dl) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = p.H, K = p.K;
  for (int k = wave; k < K; k += NW) {
    float t = 0.f;
    for (int c = lane; c < H; c += 64) t += p.Wk[(size_t)k * H + c] * M[c];
    t = wave_sum(t);
    if (lane == 0) lg[k] = t + p.bk[k];
  }
  __syncthreads();
  if (tid == 0) {
    float surv = 1.f, risk = 0.f;
    int best = 0;
    for (int k = 0; k < K; ++k) {
      const float h = 1.0f / (1.0f + __expf(-lg[k]));
      hz[k] = h;
      surv *= 1.0f - h;
      sv[k] = surv;
      risk -= surv;
      if (lg[k] > lg[best]) best = k;
    }
    float pre = 1.f;                       // prod_{i < j} (1 - h_i)
    for (int j = 0; j < K; ++j) {
      float run = pre, g = pre;
      for (int k = j + 1; k < K; ++k) { run *= 1.0f - hz[k]; g += run; }
      dl[j] = g * hz[j] * (1.0f - hz[j]);
      pre *= 1.0f - hz[j];
    }
    const int q = p.step0 + s;
    if (q < p.n_steps) p.step_risk[q] = risk;
    else if (q == p.n_steps) {
      p.risk_x[0] = risk;
      if (p.risk) p.risk[0] = risk;
      if (p.Y_hat) p.Y_hat[0] = best;
      for (int k = 0; k < K; ++k) {
        if (p.logits) p.logits[k] = lg[k];
        if (p.hazards) p.hazards[k] = hz[k];
        if (p.S) p.S[k] = sv[k];
      }
    } else p.risk_base[0] = risk;
  }
  __syncthreads();
}

}  // namespace mmf
