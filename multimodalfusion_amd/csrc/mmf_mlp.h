// Parameter blocks of the small dense / fusion kernels (mmf_mlp.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmf {

struct DropSpec {            // kind: 0 none, 1 Dropout, 2 AlphaDropout
  int kind; float p; uint32_t key;
  const uint32_t* dev;       // optional device-resident seed added to the key (graph-replay-safe dropout)
};

struct DenseParams {
  const float *x, *W, *bias;
  float* y;
  int B, K, N, act;
  DropSpec drop;
  // Per-row mask index base [B], or null.  Given: element (b, n) hashes row_base[b] + n under drop.key where the plain
  // form hashes b * N + n.  With drop.key the seed-0 key of the site and row_base[b] = seed_b * inverse(0x9E3779B1)
  // (mmf_api.hip: hash_mul_inverse), row b gets the mask a one-row call with seed_b draws at index n.
  const uint32_t* row_base;
  int ldy;                     // row_base given: leading dimension of y (>= N)
};
struct DenseBwdParams {
  const float *dy, *y, *x, *W;
  float *dpre, *dx, *dW, *db;
  int B, K, N, act;
  DropSpec drop;
  const uint32_t* row_base;   // as DenseParams::row_base
  int ldy, lddy;              // row_base given: leading dimensions of y and dy (>= N)
};
struct KronParams {
  const float* o[3];
  float* out;          // forward
  const float* g;      // backward: d out
  float* d[3];         // backward: d o_t
  int m, dim, B;
  DropSpec drop;
};

int launch_dense_fwd(DenseParams p, hipStream_t st);
int launch_dense_bwd(DenseBwdParams p, hipStream_t st);
int launch_gate_mul(const float* z, const float* h, float* o, int n, hipStream_t st);
int launch_gate_mul_bwd(const float* g, const float* z, const float* h, float* dz, float* dh, int n, hipStream_t st);
int launch_kron_fwd(KronParams p, hipStream_t st);
int launch_kron_bwd(KronParams p, hipStream_t st);

}  // namespace mmf

namespace mmf {
// Fused per-modality gating stage of XlinearFusion (models/model_modules.py:158-165), all m modalities in ONE launch:
//   h_i = relu(Wh_i v_i + bh_i) ; z_i = Wz_i v_cat + bz_i ; gm_i = sigmoid(z_i) * h_i ; o_i = drop(relu(Wo_i gm_i + bo_i))
struct XReduceParams {
  int m, B, dim, sdim;                  // modalities (2|3), batch, 256, 16
  const float* v[3];                    // [B x dim]
  const float *Wh[3], *bh[3];           // [sdim x dim]
  const float *Wz[3], *bz[3];           // [sdim x m*dim]
  const float *Wo[3], *bo[3];           // [sdim x sdim]
  float *h[3], *z[3], *gm[3], *o[3];    // [B x sdim] (forward outputs / backward inputs)
  // backward
  const float* d_o[3];                  // [B x sdim]
  float* dv[3];                         // [B x dim]  (overwritten: includes the v_cat contribution)
  float *dWh[3], *dbh[3], *dWz[3], *dbz[3], *dWo[3], *dbo[3];
  DropSpec drop;                        // key of site 0; site i uses key + i*0x632BE5AB (see drop_key)
};
int launch_xreduce_fwd(XReduceParams p, hipStream_t st);
int launch_xreduce_bwd(XReduceParams p, hipStream_t st);

// ---- forward-only XlinearFusion of a window of G patients (mmf_xfusion_infer_group): eval mode, nothing saved --------
// the gating stage per patient: XReduceParams' arithmetic for B = 1 in workgroup g; only o leaves the kernel
struct XGateGroupParams {
  int m, G, dim, sdim;
  const float* v[3];                    // [G x dim]
  const float *Wh[3], *bh[3], *Wz[3], *bz[3], *Wo[3], *bo[3];
  float* o;                             // [G x m x sdim]
};
// y[g][n] = relu(bias[n] + sum_e kron_g[e] W[n][e]), kron_g = [o_g0, 1] x [o_g1, 1] (x [o_g2, 1]) formed on the fly
struct KronDenseGroupParams {
  int m, G, N;                          // sdim = 16: rows of W are 17^m wide
  const float* o;                       // [G x m x 16]
  const float *W, *bias;                // [N x 17^m], [N]
  float* y;                             // [G x N]
};
// y[g][n] = relu(bias[n] + sum_s sum_k x_s[g][k] W[n][off_s + k]): a dense layer whose input row is the concatenation
// of up to 4 dense [G x width_s] buffers (encoder2's skip connection; one segment: a plain layer)
struct DenseSegsParams {
  int nseg, G, N, K;                    // K = sum width <= 64 * DENSE_SEGS_MAXC
  const float* x[4];
  int width[4];
  const float *W, *bias;                // [N x K], [N]
  float* y;                             // [G x N]
};
constexpr int DENSE_SEGS_MAXC = 24;
int launch_xgate_group(XGateGroupParams p, hipStream_t st);
int launch_kron_dense_group(KronDenseGroupParams p, hipStream_t st);
int launch_dense_segs_group(DenseSegsParams p, hipStream_t st);

// ---- training step of the same window (mmf_xfusion_group_forward / mmf_xfusion_group_backward) ------------------------
// What the TRAIN instantiations of the three kernels above take beside their parameter block (a trailing kernel argument:
// the forward-only instantiations keep their argument offsets).  Patient g's mask of a site is that of the site's seed-0
// key at index row_base[g] + column (DenseParams::row_base); p == 0 (eval mode) hashes nothing.
struct XTrainParams {
  float p;                      // dropout probability of the launch's site(s)
  uint32_t key;                 // seed-0 key: xgate site 0 (site i adds i * 0x632BE5AB), kron_dense site 9, dense_segs its own
  uint32_t key8;                // xgate: seed-0 key of the post-fusion site 8
  int ld;                       // xgate: row stride of v_i; kron_dense: row stride of y
  const uint32_t* dev;          // optional device seed word added to the keys
  const uint32_t* row_base;     // [G]
  float *h, *z, *gm;            // xgate keeps these for its backward: [G x m x sdim]
  uint32_t* bits;               // post-fusion keep bits [G x xfusion_bit_words(m)]: xgate writes, kron_dense reads
};
constexpr int xfusion_bit_words(int m) { return ((m == 3 ? 17 * 17 * 17 : 17 * 17) + 63) / 64 * 2; }
int launch_xgate_group_train(XGateGroupParams p, XTrainParams t, hipStream_t st);
int launch_kron_dense_group_train(KronDenseGroupParams p, XTrainParams t, hipStream_t st);
int launch_dense_segs_group_train(DenseSegsParams p, XTrainParams t, hipStream_t st);

// The backward of the fusion tail in front of encoder2 (mmf_xfusion_group.hip).  x2 [G x K2] is encoder2's input row
// [e1 (dropped) | v_0 | v_1 (| v_2)], dx2 its gradient as encoder2's backward left it: the kernels read d e1 from its first
// N1 columns and ADD the gating stage's dv_i to the others (one thread per element).
struct XFusionBwdParams {
  int m, G, dim, N1, K2;        // sdim = 16; N1 = mmhid1; K2 = N1 + m * dim
  float p;                      // dropout probability of sites 0 .. 10 (0: eval mode)
  int accumulate;
  const float* x2;
  float* dx2;
  const float *o, *h, *z, *gm;  // [G x m x 16], o dropped
  const uint32_t* bits;         // [G x xfusion_bit_words(m)]
  float* dkr;                   // [G x 17^m]: d of the dropped product
  float *dpo, *dz, *dph;        // [G x m x 16]: the gating stage's pre-activation gradients, for the weight gradients
  const float* We1;
  const float *Wh[3], *Wz[3], *Wo[3];
  float *dWe1, *dbe1;
  float *dWh[3], *dbh[3], *dWz[3], *dbz[3], *dWo[3], *dbo[3];
};
int launch_xfusion_group_bwd(XFusionBwdParams p, hipStream_t st);
// its two input-gradient launches alone (mmf_mm_ig_tensor): dkr, then the gating stage's backward, which still writes dpo,
// dz and dph; We1's and the gating stage's weight gradients are neither launched nor read (dW*, db* may be null)
int launch_xfusion_group_bwd_dx(XFusionBwdParams p, hipStream_t st);
int launch_add_into(float* out, const float* in, int64_t n, hipStream_t st);
}  // namespace mmf

// ---- stage-2 (embedding-level) building blocks: SURVEY.md 8f row N3 --------------------------------------------
namespace mmf {
struct BnParams {            // y = drop(act(BatchNorm1d(x) [+ res]))      x, y: [B x F]
  const float *x, *res, *gamma, *beta;
  float *running_mean, *running_var;     // updated in training mode (momentum, unbiased variance), read in eval
  float *y, *save_mean, *save_invstd;    // save_*: [F], what backward needs
  int B, F, training, act;
  float eps, momentum;
  DropSpec drop;
};
struct BnBwdParams {
  const float *dy, *y, *x, *gamma, *save_mean, *save_invstd;
  float *dx, *dres, *dgamma, *dbeta;     // dres may be null
  int B, F, training, act;
  DropSpec drop;
};
struct HighwayParams {       // y = sigmoid(zg) * relu(zn) + (1 - sigmoid(zg)) * zl        all [n]
  const float *zg, *zn, *zl;
  float* y;
  const float* dy;                       // backward
  float *dzg, *dzn, *dzl;
  int64_t n;
};
struct RankParams {          // loss = -mean|sum over comparable pairs of phi(risk_more - risk_less)
  const float* risks; const double* times; const float* c;
  int B, phi, reduction;                 // phi: 0 sigmoid, 1 relu; reduction: 0 mean, 1 sum
  float *loss, *d_risks;
};
struct HazardParams {        // logits [B x K] -> hazards, S, Y_hat, risk = -sum_k S
  const float* logits;
  float *hazards, *S, *risk; int64_t* Y_hat;
  const float *g_hazards, *g_S, *g_risk;  // backward (any may be null)
  float* dlogits;
  int B, K;
};
int launch_bn_fwd(BnParams p, hipStream_t st);
int launch_bn_bwd(BnBwdParams p, hipStream_t st);
int launch_highway_fwd(HighwayParams p, hipStream_t st);
int launch_highway_bwd(HighwayParams p, hipStream_t st);
int launch_rank_loss(RankParams p, hipStream_t st);
int launch_hazard_fwd(HazardParams p, hipStream_t st);
int launch_hazard_bwd(HazardParams p, hipStream_t st);
// ---- omic head, one training step in one launch (mmf_maxnet.hip) ------------------------------------------------------
struct MaxnetStepParams {
  int B, G;
  const float *x, *W0, *b0, *W1, *b1, *Wc, *bc;
  const double* times;
  const float* c;
  float p;                           // AlphaDropout probability of both blocks (0: eval)
  uint32_t key0, key1;
  const uint32_t* seed_dev;
  float loss_scale;
  float *y0, *y1, *dp1, *dp0, *dr;   // workspace: y0, y1 [B][256]; dp1, dp0 TRANSPOSED [256][maxnet_step_dp_pitch(B)]; dr [B]
  float* dwc_part;                   // workspace: [32 workgroups][256] shares of dWc
  unsigned* bar;                     // 3 tick words
  float *risk, *loss;
  float *dW0, *db0, *dW1, *db1, *dWc, *dbc;
  int accumulate;
};
size_t maxnet_step_workspace_floats(int B);
int maxnet_step_dp_pitch(int B);
bool maxnet_step_ok(int B, int G, int H0, int H1);
int launch_maxnet_cox_step(MaxnetStepParams p, hipStream_t st);

}  // namespace mmf
