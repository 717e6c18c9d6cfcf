/* mmf_amil.h -- C ABI of libmmf_amil.so: the MI355X (gfx950) attention-MIL + survival-loss hot path.
 *
 * The reference (MultimodalFusion/multimodalfusion) has no FFI / plugin API: its boundary is
 * the Python nn.Module surface.  This header is the C ABI that sits directly beneath that
 * surface -- the entry points a binding for this path binds (ctypes in this repo, see
 * INTEGRATION.md).  Each entry point names the reference lines it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (fp32, row-major, 16-byte aligned)
 *     unless the comment says "host";  the library allocates nothing and keeps no state (no globals: the optional
 *     device-resident dropout seed and the optional kernel trace are passed per call);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream), performs no host synchronisation, and is re-entrant / thread-safe (autograd
 *     calls backward from another thread);
 *   - return value: 0 on success, negative mmf error code otherwise (mmf_strerror()).
 *   - "workspace": a caller-owned scratch buffer; forward fills it with the saved activations
 *     (h, a, b, scores, softmax statistics) that backward reads, so the SAME buffer must be
 *     passed to the matching backward call, unmodified in between.
 */
#ifndef MMF_AMIL_H
#define MMF_AMIL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMF_ACT_NONE 0
#define MMF_ACT_RELU 1
#define MMF_ACT_TANH 2
#define MMF_ACT_SIGMOID 3
#define MMF_ACT_SELU 4

const char* mmf_strerror(int code);
/* ABI version; bumped on any signature change. */
int mmf_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Attention-MIL stack:  Sequential(Linear(L,H), ReLU, Dropout(0.25), Attn_Net[_Gated](H,D,1))
 * followed by softmax pooling over the instances.
 *   replaces models/model_attention_mil_path.py:20-29 (construction), :52-56 (forward),
 *            models/model_modules.py:70-85 (Attn_Net), :87-110 (Attn_Net_Gated),
 *            and the same stack in model_attention_mil_radio.py:88-99 / model_mm_attention_mil.py:146-160.
 * ------------------------------------------------------------------------------------------- */
struct mmf_trace;

typedef struct mmf_amil_desc {
  int64_t N;          /* instances in the bag.  Row cap: every operand that grows with N is addressed with 32-bit byte
                       * offsets and stays below 2 GiB, so N * max(L, H, 2 * D) * 4 < 2^31 (fp32 storage), else
                       * MMF_ERR_SHAPE before any launch: 524,287 rows where the widest of L, H, 2 D is 1024 (both
                       * shipped heads), 2,097,151 where it is 256.  Every entry point that takes this descriptor
                       * applies it; the grouped ones apply it to sum N. */
  int32_t L, H, D;    /* feature dim, hidden dim, attention dim: small 1024/256/256, big 1024/512/384.
                       * L % 32 == 0, H in {256, 512, 1024}, D % 128 == 0, else MMF_ERR_SHAPE. */
  int32_t gated;      /* 1 = Attn_Net_Gated, 0 = Attn_Net */
  const float* W1;    /* [H x L]  attention_net.0.weight */
  const float* b1;    /* [H] */
  const float* Wa;    /* [D x H]  attention_a.0.weight (gated) / module.0.weight (ungated) */
  const float* ba;    /* [D] */
  const float* Wb;    /* [D x H]  attention_b.0.weight (gated only, else NULL) */
  const float* bb;    /* [D] */
  const float* Wc;    /* [1 x D]  attention_c.weight / module.{2|3}.weight */
  const float* bc;    /* [1] */
  float p_h;          /* dropout prob after the ReLU (0.25 in train mode, 0 in eval) */
  float p_att;        /* dropout prob on the tanh / sigmoid branches (0.25 iff dropout=True and training) */
  uint32_t seed;      /* dropout seed of this call; masks are regenerated, never stored */
  const uint32_t* seed_dev;  /* optional DEVICE word added to `seed` by every kernel of the call (uint32 wrap), or NULL.
                              * By-value seeds are frozen into a captured hipGraph; a graph whose first node bumps this
                              * word draws fresh masks on every replay.  Forward and backward must see the same value. */
  struct mmf_trace* trace;   /* optional kernel trace (mmf_trace_create), or NULL: see "Kernel trace" below */
  int32_t concurrent;        /* scheduling hint; results agree to fp32 rounding whatever it is (bit for bit unless the two
                              * tile plans put a row into a 16-row half block, v_mfma_f32_16x16x4_f32, in one and into a
                              * 32-row block in the other: same k order, rounded per instruction).  0: the call has the GPU to itself -- the
                              * row-parallel GEMMs take the tile height that finishes ONE bag soonest (208 rows: a 50k
                              * bag on 241 of 256 CUs, one bag per step 0.816 -> 0.801 ms).  1: other bags' kernels run
                              * beside it on other streams (pipeline.BagsInFlight) -- 224-row tiles, which leave 32 CUs
                              * to the neighbours, gave the higher aggregate rate in two of three same-run comparisons
                              * (1376 vs 1337 bags/s with three bags in flight) and the same rate in the third. */
  int32_t gemm;              /* how the stack's four large fp32 contractions are multiplied (fp32 calls only; inputs,
                              * outputs, saved activations and accumulation are fp32 either way):
                              *   MMF_GEMM_F32    (0) v_mfma_f32_32x32x2_f32, the exact-fp32 matrix instruction;
                              *   MMF_GEMM_BF16X3 (1) every fp32 operand as the exact sum of three bf16 values, the six
                              *                       leading products on v_mfma_f32_32x32x16_bf16, fp32 accumulation
                              *                       (csrc/mmf_gemm_split.h).  Same error against an fp64 product as
                              *                       mode 0 (tests/test_gpu_split.py), 2.67 x its instruction rate.
                              *                       Every bag size, gated or not (which tile a bag size takes is a
                              *                       tuning detail of the launcher, not a contract); the radio head's
                              *                       segmented projection and the stand-alone scorer run mode 0.
                              *                       Finite operands stay finite (values beyond the largest bf16 are
                              *                       split around a clamped first plane); infinite operands give NaN,
                              *                       as in mode 0. */
  uint32_t* sync;            /* optional DEVICE array of `sync_words` 32-bit words, or NULL.  Tick words of the launches in
                              * which several workgroups share an output tile (K-split projections of short grids: each
                              * writes a partial tile, the last to arrive -- found through one of these words -- sums them
                              * in a fixed order and finishes the tile; no workgroup waits for another).  Contract: zero
                              * before the first call that sees it; every call leaves it zero; calls that may run at the
                              * same time (different streams) need different arrays.  NULL / too few words: such launches
                              * fall back to one workgroup per tile (same results to fp32 rounding, slower small bags). */
  int32_t sync_words;        /* 1024 covers every shape */
} mmf_amil_desc;
#define MMF_GEMM_F32 0
#define MMF_GEMM_BF16X3 1

typedef struct mmf_amil_grads {
  float* dW1; float* db1;
  float* dWa; float* dba;
  float* dWb; float* dbb;   /* NULL when ungated */
  float* dWc; float* dbc;
  float* dx;                /* [N x L] or NULL (path bags need no input gradient; radio does) */
} mmf_amil_grads;

size_t mmf_amil_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated);

/* x [N x L] -> M [H] (pooled embedding), A_raw [N] (pre-softmax scores, what heat-maps consume). */
int mmf_amil_forward(const mmf_amil_desc* desc, const float* x, void* workspace, size_t workspace_bytes,
                     float* M, float* A_raw, void* stream);

/* dM [H], gA [N] (gradient w.r.t. A_raw, may be NULL) -> parameter grads (overwritten, not accumulated). */
int mmf_amil_backward(const mmf_amil_desc* desc, const float* x, void* workspace, size_t workspace_bytes,
                      const float* M, const float* A_raw, const float* dM, const float* gA,
                      const mmf_amil_grads* grads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16-storage variant of the same stack (BASELINE config 5: 100k x 1024 bags, HBM-bound).
 *   x is a bf16 bag [N x L] (raw bits, row-major).  Parameters and returned gradients stay fp32;
 *   per call the library makes bf16 copies of W1 / Wa / Wb in the workspace, keeps h, a, b, du in
 *   bf16, multiplies on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, and runs every epilogue
 *   (bias, ReLU, tanh, sigmoid, dropout, scores, softmax pooling) in fp32.  M and A_raw are fp32.
 *   Same desc, same dropout masks as the fp32 entry points.  Needs L % 64 == 0, H % 256 == 0.
 *   Row cap: mmf_amil_desc::N's with 2-byte elements, N * max(L, H, 2 * D) * 2 < 2^31 (1,048,575 rows for both
 *   shipped heads), else MMF_ERR_SHAPE.
 *   grads->dx must be NULL (the bag is a leaf).
 * ------------------------------------------------------------------------------------------- */
size_t mmf_amil_bf16_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated);
int mmf_amil_bf16_forward(const mmf_amil_desc* desc, const uint16_t* x, void* workspace, size_t workspace_bytes,
                          float* M, float* A_raw, void* stream);
int mmf_amil_bf16_backward(const mmf_amil_desc* desc, const uint16_t* x, void* workspace, size_t workspace_bytes,
                           const float* M, const float* A_raw, const float* dM, const float* gA,
                           const mmf_amil_grads* grads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention stack + classifier / hazard head in one call, and the whole training step of one bag in one call.
 *   The path head's forward is stack -> classifier -> sigmoid / cumprod / argmax (models/model_attention_mil_path.py:
 *   52-61); the training loop then applies nll_surv and calls backward (utils/core_utils.py:200-243).  After the
 *   pooling kernel these are single-workgroup launches of a few microseconds each; here they run as the tail of the
 *   pooling merge (one single-workgroup launch behind it; for small bags the merge runs there too), so a bag costs 7-8 launches instead of 13 -- what matters for 1k-10k bags.
 *   x_bf16 != 0: x is a bf16 bag (uint16_t bits) and the bf16-storage kernels run (see above).
 *   workspace: mmf_amil_workspace_bytes / mmf_amil_bf16_workspace_bytes of the same shape.
 * mmf_amil_head_forward: stack + head; M [H], A_raw [N] and the head outputs are written; backward as usual
 *   (mmf_surv_head_backward, then mmf_amil[_bf16]_backward with the same workspace).
 * mmf_amil_nll_step: forward + head + nll_surv + backward.  Writes the head outputs, loss (unscaled) and A_raw, and the
 *   gradients of loss * loss_scale w.r.t. every parameter: grads (attention stack) and target->dWk / dbk
 *   (classifier), overwritten, or ADDED to what the buffers hold when target->accumulate != 0 (gradient accumulation
 *   over the `gc` bags of a window, utils/core_utils.py:242-247, with loss_scale = 1 / gc).  grads->dx must be NULL.
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_surv_head {
  const float* Wk;      /* [K x H] classifier.weight */
  const float* bk;      /* [K] */
  int32_t K;            /* <= 32 */
  float* logits;        /* [K] out */
  float* hazards;       /* [K] out */
  float* S;             /* [K] out */
  int64_t* Y_hat;       /* [1] out */
  float* risk;          /* [1] out = -sum_k S_k (what the loop logs, utils/core_utils.py:207), or NULL */
} mmf_surv_head;

typedef struct mmf_nll_target {
  const int64_t* Y;     /* [1] device: discrete time bin */
  const float* c;       /* [1] device: censorship */
  float alpha, eps;     /* NLLSurvLoss(alpha), eps = 1e-7 */
  float loss_scale;     /* gradients are those of loss * loss_scale */
  float* loss;          /* [1] out, unscaled */
  float* dWk;           /* [K x H] */
  float* dbk;           /* [K] */
  int32_t accumulate;   /* 0: every gradient buffer is overwritten; 1: added to */
} mmf_nll_target;

int mmf_amil_head_forward(const mmf_amil_desc* desc, const void* x, int32_t x_bf16, void* workspace, size_t workspace_bytes,
                          const mmf_surv_head* head, float* M, float* A_raw, void* stream);
int mmf_amil_nll_step(const mmf_amil_desc* desc, const void* x, int32_t x_bf16, void* workspace, size_t workspace_bytes,
                      const mmf_surv_head* head, const mmf_nll_target* target, float* A_raw,
                      const mmf_amil_grads* grads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped training step: the G bags of one gradient-accumulation window in ONE launch chain.
 *   The reference trains with batch_size = 1 and accumulates gc bags before each optimizer step
 *   (utils/core_utils.py:200-247: loss / gc + loss_reg; loss.backward(); step every gc bags), over the per-bag forward of
 *   models/model_attention_mil_path.py:50-61 and nll_surv (utils/loss_utils.py:22-39).  The parameters do not change inside
 *   a window, so its bags are independent forward passes on the same weights and their summed gradient is ONE contraction
 *   over all of their rows.  Here the row-parallel GEMMs and the split-K weight-gradient GEMMs run once over the
 *   concatenated rows (sum N); only pooling, the head, the loss and K-prep are per bag (one workgroup per bag, one launch).
 *   x: the bags' rows concatenated, [sum N x L] fp32 (bf16 bags are not supported here: the bf16 path serves 100k-row
 *   bags, which fill the GPU on their own).  desc->N = offsets[G]; desc->seed is not read (each bag has its own seed);
 *   desc->seed_dev, sync and trace as usual.
 *   head / target: the per-bag arrays are G long -- logits, hazards, S [G x K]; Y_hat, risk, loss, Y, c [G].
 *   Gradients: those of sum_g loss_g * loss_scale, overwritten, or added under target->accumulate, as G calls of
 *   mmf_amil_nll_step with accumulate would leave them (to fp32 rounding).  Bag g's dropout masks are the ones
 *   mmf_amil_nll_step draws for that bag alone with desc->seed = seeds[g] (bag-local row indices).
 *   Returns MMF_ERR_ARG for gemm = MMF_GEMM_BF16X3 or grads->dx != NULL; MMF_ERR_SHAPE for G outside 1..MMF_GROUP_MAX, an
 *   empty bag, offsets that are not strictly increasing from 0, desc->N != offsets[G], or totals beyond the limits of the
 *   single-bag entry points (mmf_amil_desc::N's row cap applied to sum N) or beyond 256 pooling groups of 8192 rows
 *   (sum N <= 2,097,152).  No workgroup waits for another; calls are deterministic.
 * mmf_amil_group_workspace_bytes: the workspace of that window, or 0 when the offset table is invalid.
 * ------------------------------------------------------------------------------------------- */
#define MMF_GROUP_MAX 64
typedef struct mmf_bag_group {
  int32_t G;                 /* bags in the group, 1 .. MMF_GROUP_MAX */
  const int64_t* offsets;    /* HOST [G + 1]: bag g = rows offsets[g] .. offsets[g + 1] - 1 of x; offsets[0] = 0 */
  const uint32_t* seeds;     /* HOST [G]: dropout seed of each bag */
} mmf_bag_group;

size_t mmf_amil_group_workspace_bytes(const int64_t* offsets, int32_t G, int32_t L, int32_t H, int32_t D, int32_t gated);
int mmf_amil_nll_step_group(const mmf_amil_desc* desc, const mmf_bag_group* group, const float* x, void* workspace,
                            size_t workspace_bytes, const mmf_surv_head* head, const mmf_nll_target* target,
                            float* A_raw /* [sum N] */, const mmf_amil_grads* grads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped training step of the radiology head: mmf_amil_nll_step_group behind the head's reduce_dim
 *   (models/model_attention_mil_radio.py:80-82: cat(modalities, axis=1) -> Linear(nseg * kseg, L), no activation).  The
 *   bags' modality segments are concatenated by rows, segment by segment; reduce_dim runs once over all rows into the
 *   workspace, the stack chain of mmf_amil_nll_step_group follows on that, and reduce_dim's backward joins the chain:
 *   its input gradient du . W1 over all rows, its weight gradient as one split-K TN launch of nseg problems (d
 *   reduce_dim.bias folded into one of them), its sums in the stack's reduce launch.  What bag g gets -- outputs,
 *   dropout masks, its share of every gradient -- is what MIL_Attention_fc_surv_radio.nll_step computes for it alone
 *   with desc->seed = seeds[g].
 *   desc: the stack (desc->L == kseg, the width of reduce_dim's output); desc->N = offsets[G].  grads->dx must be NULL
 *   (the gradient of reduce_dim's output stays in the workspace).  rd->dW / rd->db follow target->accumulate, as the
 *   stack's gradients do.
 *   Returns as mmf_amil_nll_step_group, and MMF_ERR_SHAPE for nseg outside 2..4, kseg != desc->L or an
 *   [offsets[G] x nseg * kseg] input of 2 GiB or more; MMF_ERR_ALIGN for a misaligned segment, reduce_dim weight or dW.
 * mmf_radio_group_workspace_bytes: the workspace of that window (L = kseg), or 0 when the offset table is invalid, nseg is
 *   outside 2..4 or kseg < 1 (the widths are the descriptor's to refuse: the query does not see it).
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_radio_reduce {
  const float* const* x;     /* HOST [nseg] device pointers, each [sum N x kseg]: modality m of every bag, in bag order */
  int32_t nseg, kseg;        /* 2..4 modalities of kseg features each */
  const float* W;            /* reduce_dim.weight [kseg x nseg * kseg] */
  const float* bias;         /* reduce_dim.bias [kseg] */
  float* dW;                 /* [kseg x nseg * kseg] */
  float* db;                 /* [kseg] */
} mmf_radio_reduce;

size_t mmf_radio_group_workspace_bytes(const int64_t* offsets, int32_t G, int32_t nseg, int32_t kseg, int32_t H,
                                       int32_t D, int32_t gated);
int mmf_radio_nll_step_group(const mmf_amil_desc* desc, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                             void* workspace, size_t workspace_bytes, const mmf_surv_head* head,
                             const mmf_nll_target* target, float* A_raw /* [sum N] */, const mmf_amil_grads* grads,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped forward-only pass: G bags evaluated with fixed weights in ONE launch chain -- the per-epoch validation pass
 *   (utils/core_utils.py:267-355), the final summary (:358-430), embedding export (pre_trained_feature.py:116-162) and
 *   heat-map scoring (utils/heatmap_utils.py:111-150) run one forward per bag in the reference.  The bags are independent
 *   forward passes on the same weights: the row-parallel GEMMs run once over the concatenated rows with the one-bag plans of
 *   sum N rows; only pooling and the head are per bag (one workgroup per bag, one launch).  Nothing is kept for a backward.
 *   x: the bags' rows concatenated, [sum N x L], fp32 or (x_bf16 != 0) bf16 (uint16_t bits; the one-bag bf16 constraints
 *   L % 64 == 0, H % 256 == 0 apply).  bf16 windows run the unfused bf16 kernels, which the one-bag route runs for every
 *   stack but the gated one with H = D = 256; that stack's one-bag route takes a fused forward form, which rounds
 *   differently, so its bf16 windows return MMF_ERR_SHAPE (evaluate those bags one at a time).  desc->N = offsets[G]; desc->seed and desc->seed_dev are not read (no dropout);
 *   sync and trace as usual.  group->seeds is not read and may be NULL.
 *   head: the per-bag arrays are G long -- logits, hazards, S [G x K]; Y_hat, risk (optional) [G]; head == NULL: M only
 *   (embedding export; M must then be given).  target (optional, needs head): each bag's nll_surv VALUE; only Y, c [G],
 *   alpha, eps and loss [G] are read (dWk, dbk, loss_scale, accumulate are not).  M: [G x H] or NULL (not stored).
 *   A_raw: [sum N].  What bag g gets -- A_raw rows, M_g, head outputs, loss_g -- is what the one-bag forward-only route
 *   (mmf_amil[_bf16]_infer, then mmf_surv_head_forward and mmf_nll_surv) computes for that bag alone, to fp32 rounding.
 *   Eval mode only: desc->p_h and desc->p_att must be 0, else MMF_ERR_ARG; MMF_ERR_ARG also for gemm = MMF_GEMM_BF16X3.
 *   MMF_ERR_SHAPE for G outside 1..MMF_GROUP_MAX, an empty bag, offsets that are not strictly increasing from 0,
 *   desc->N != offsets[G], a head with K > 32, a bf16 window of a gated H = D = 256 stack, or totals beyond the limits of
 *   the one-bag entry points (mmf_amil_desc::N's row cap, or the bf16 section's, applied to sum N) or beyond 256 pooling
 *   groups of 8192 rows (sum N <= 2,097,152).
 *   No workgroup waits for another; calls are deterministic; the call allocates nothing and keeps no state.
 * mmf_amil_group_infer_workspace_bytes: the workspace of that window, or 0 when the offset table is invalid.  With x_bf16 it
 *   is at least the fp32 size, so one buffer serves a window of either storage.
 * mmf_radio_infer_group: the same behind the radiology head's reduce_dim (mmf_radio_nll_step_group's layout; desc->L ==
 *   kseg, nseg 2..4, fp32); rd->dW / rd->db are not read.  Returns as mmf_amil_infer_group, and as
 *   mmf_radio_nll_step_group for rd.  mmf_radio_group_infer_workspace_bytes: its workspace, or 0 (invalid table, nseg
 *   outside 2..4 or kseg < 1).
 * ------------------------------------------------------------------------------------------- */
size_t mmf_amil_group_infer_workspace_bytes(const int64_t* offsets, int32_t G, int32_t L, int32_t H, int32_t D,
                                            int32_t gated, int32_t x_bf16);
int mmf_amil_infer_group(const mmf_amil_desc* desc, const mmf_bag_group* group, const void* x, int32_t x_bf16,
                         void* workspace, size_t workspace_bytes, const mmf_surv_head* head, const mmf_nll_target* target,
                         float* M /* [G x H] or NULL */, float* A_raw /* [sum N] */, void* stream);
size_t mmf_radio_group_infer_workspace_bytes(const int64_t* offsets, int32_t G, int32_t nseg, int32_t kseg, int32_t H,
                                             int32_t D, int32_t gated);
int mmf_radio_infer_group(const mmf_amil_desc* desc, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                          void* workspace, size_t workspace_bytes, const mmf_surv_head* head,
                          const mmf_nll_target* target, float* M, float* A_raw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Integrated-gradients patch attribution of the pathology head in one call: how much each patch of a slide contributes to
 *   the predicted risk.  The reference computes it with captum (create_attributions.py:94-102: IntegratedGradients of
 *   risk = -sum(S) from a zero baseline, n_steps = 20, reduced per patch by sum |attr|) through the captum methods of its
 *   models (models/model_mm_attention_mil.py:246-301) -- n_steps forward and backward passes of the bag through autograd.
 *   With baseline 0 the interpolated input is alpha_k x, so the projection is linear in alpha, u_k = alpha_k (x W1^T) + b1,
 *   and the input gradient is linear in du: sum_k w_k dx_k = (sum_k w_k du_k) W1.  The two L-wide contractions run ONCE
 *   per call and the weight gradients not at all; only the H-wide part (ReLU, gate, pooling, head, K-prep, K-dh) runs per
 *   step, the steps of a window standing in as the bags of the grouped chain.  The chain:
 *     1. U = x W1^T, one launch of the projection (no bias, no activation);
 *     2. per window of steps: h[s N + i, :] = relu(alpha_s U[i, :] + b1) and its ReLU bits; the grouped gate forward,
 *        per-step pooling and merge; the hazard head forward and the backward of risk over the [steps x H] embeddings;
 *        K-prep and K-dh; Gacc[N x H] += sum_s w_s du[s N + i, :], in step order whatever the windows are;
 *     3. P = Gacc W1 with an epilogue that multiplies by x in registers and reduces each row: attr = x * P.
 *   No weight-gradient (TN) launch, no reduce list.
 * desc: the stack, fp32, exact-fp32 GEMMs, gated or not, both head sizes; desc->N rows.  Eval mode: desc->p_h and p_att must
 *   be 0 (with dropout the integrand would be random).  head: the stock hazard head -- Wk, bk, K <= 32 are read; logits,
 *   hazards, S, Y_hat and risk are optional outputs (NULL: not written) and receive the head's values at alpha = 1, the
 *   bag itself.  The target is risk = -sum_k S_k.
 * ig->alpha / weight: HOST arrays of the quadrature's n_steps nodes and weights -- the caller supplies the rule, the library
 *   knows none.  ig->window_steps: steps evaluated per grouped window; 0 lets the library choose; either is clamped to
 *   what the row limits of the grouped chain admit (window_steps x N rows of H- and D-wide operands, as
 *   mmf_amil_nll_step_group's sum N).  alpha = 1 and alpha = 0 ride along as two more forward steps of weight 0.
 * Outputs (device): row_sum [N] = sum_l attr[i, l]; row_abs [N] = sum_l |attr[i, l]|; attr [N x L] or NULL -- with NULL
 *   the N x L product never reaches memory; risk_x [1], risk_base [1]: the risk at alpha = 1 and at alpha = 0 (with row_sum
 *   they give the completeness gap); step_risk [n_steps]: the risk at each node.
 * Every sum is taken in a fixed order and there are no float atomics: two calls agree bit for bit.  No workgroup waits for
 *   another; the call allocates nothing and keeps no state.
 * Returns, before any launch: MMF_ERR_ARG for a null pointer, p_h or p_att != 0, gemm = MMF_GEMM_BF16X3, n_steps outside
 *   1..MMF_GROUP_MAX or window_steps < 0 (a bf16 bag has no entry here: the call takes fp32 rows only); MMF_ERR_SHAPE,
 *   MMF_ERR_ALIGN and MMF_ERR_WORKSPACE as the one-bag entry points, MMF_ERR_SHAPE also for a head with K > 32 and a bag
 *   too long for one step to be a window.
 * mmf_amil_ig_workspace_bytes: the workspace of that call, or 0 for n_steps outside 1..MMF_GROUP_MAX, window_steps < 0,
 *   N < 1, L < 32, H < 32, or N above the row limit of one window -- min(2^32 / max(H, D), 2^31 / (4 max(H, 2 D)),
 *   2,097,152) rows: not even one step fits.  The query has no descriptor: it applies neither mmf_amil_desc::N's row cap
 *   (which the L-wide bag can set below that limit; the call then returns MMF_ERR_SHAPE) nor the rules for L, H and D, so a
 *   non-zero answer does not say that the call admits the shape.  For a shape the call admits it is never 0: the row cap is
 *   at or below the window's limit.  It does not shrink as window_steps grows.
 * Out of scope (the radiology head: mmf_radio_ig; the multimodal head: mmf_mm_ig for fusion = 'concat', mmf_mm_ig_tensor for
 *   fusion = 'tensor'): non-zero baselines (they need a second projection,
 *   U' + alpha (U - U')); bf16 bags; targets other than risk.
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_ig_desc {
  int32_t n_steps;           /* quadrature nodes, 1 .. MMF_GROUP_MAX */
  const float* alpha;        /* HOST [n_steps] nodes in [0, 1] */
  const float* weight;       /* HOST [n_steps] weights */
  int32_t window_steps;      /* steps per grouped window; 0: the library chooses */
  float* row_sum;            /* [N] out */
  float* row_abs;            /* [N] out */
  float* attr;               /* [N x L] out, or NULL */
  float* risk_x;             /* [1] out */
  float* risk_base;          /* [1] out */
  float* step_risk;          /* [n_steps] out */
} mmf_ig_desc;
size_t mmf_amil_ig_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated, int32_t n_steps,
                                   int32_t window_steps);
int mmf_amil_ig(const mmf_amil_desc* desc, const float* x, void* workspace, size_t workspace_bytes,
                const mmf_surv_head* head, const mmf_ig_desc* ig, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Integrated-gradients attribution of the radiology head in one call: which MRI sequence and which slices carry the
 *   predicted risk.  The reference attributes its radiology branch with captum as it does the pathology one
 *   (create_attributions.py:94-147 through the captum methods of models/model_mm_attention_mil.py:202-355, on the forward
 *   of models/model_attention_mil_radio.py:73-115): n_steps autograd passes, each through reduce_dim and the stack, each
 *   computing weight gradients nobody reads.  The identity of mmf_amil_ig survives reduce_dim, bias included.  With X =
 *   [x_0 | ... | x_{nseg-1}], reduce_dim (Wr, br) and a zero baseline, node alpha feeds alpha X:
 *     xr(alpha) = alpha (X Wr^T) + br,   u(alpha) = alpha U + b1',   U = (X Wr^T) W1^T,   b1' = W1 br + b1,
 *   so u is still linear in alpha with a composed bias that does not depend on the bag, and the input gradient is still
 *   linear in du: sum_k w_k dX_k = ((sum_k w_k du_k) W1) Wr, attr_m = x_m * (that product's columns m kseg .. (m + 1) kseg
 *   - 1).  The two nseg kseg-wide contractions and the two L-wide ones run ONCE per call, the weight gradients never; only
 *   the H-wide part runs per node, in mmf_amil_ig's windows unchanged.  The chain:
 *     1. Y = X Wr^T, reduce_dim over the segments without its bias (the plan of mmf_radio_infer_group for N rows);
 *     2. U = Y W1^T, the stack's projection (no bias, no activation);
 *     3. b1' = b1 + W1 br, one wave per output: a dependent chain of ceil(L / 64) + 7 additions;
 *     4. mmf_amil_ig's windows on U and b1';
 *     5. P = Gacc W1 [N x L], a plain GEMM (P takes Y's place);
 *     6. Q = P Wr with an epilogue that multiplies each 32-column block by the modality that owns it, in registers, and
 *        reduces each row of the block: nothing N x nseg kseg wide reaches memory unless attr is given;
 *     7. per modality, the kseg / 32 partials of each row added in block order.
 *   No weight-gradient (TN) launch, no reduce list.
 * desc: the stack, as for mmf_amil_ig, with desc->L == rd->kseg and desc->N rows.  rd: as in mmf_radio_infer_group -- x[m]
 *   [N x kseg] fp32, nseg 2..4; dW and db are not read.  head: as for mmf_amil_ig; the optional outputs receive the values
 *   at alpha = 1.
 * ig: mmf_ig_desc with modality-major extents -- row_sum, row_abs [nseg x N]; attr [nseg x N x kseg] or NULL, so that
 *   attr + m N kseg has x[m]'s layout; alpha, weight, window_steps, risk_x, risk_base, step_risk and the two riders as for
 *   mmf_amil_ig.
 * Every sum is taken in a fixed order and there are no float atomics: two calls agree bit for bit.  No workgroup waits for
 *   another; the call allocates nothing and keeps no state.
 * Returns, before any launch and in this order: MMF_ERR_ARG for what mmf_amil_ig refuses with it and for a null rd, rd->x,
 *   rd->x[m], rd->W or rd->bias; MMF_ERR_SHAPE for nseg outside 2..4, what the descriptor's rules refuse, kseg != desc->L,
 *   N nseg kseg 4 >= 2^31 (mmf_radio_nll_step_group's rule), a head with K outside 1..32, or a bag too long for one step to
 *   be a window; MMF_ERR_ALIGN for a segment, rd->W, a stack weight, the workspace or attr off 16 bytes; MMF_ERR_WORKSPACE.
 * mmf_radio_ig_workspace_bytes: the workspace of that call, or 0 for n_steps outside 1..MMF_GROUP_MAX, window_steps < 0,
 *   N < 1, nseg outside 2..4, kseg < 32, H < 32, N above the row limit of one window (mmf_amil_ig_workspace_bytes) or
 *   N nseg kseg 4 >= 2^31.  It does not shrink as window_steps grows.
 * Out of scope (the multimodal head -- the chain cut at the embedding, the omic network per node -- has mmf_mm_ig and, for
 *   the tensor fusion, mmf_mm_ig_tensor): non-zero baselines; bf16 bags; targets other than risk.
 * ------------------------------------------------------------------------------------------- */
size_t mmf_radio_ig_workspace_bytes(int64_t N, int32_t nseg, int32_t kseg, int32_t H, int32_t D, int32_t gated,
                                    int32_t n_steps, int32_t window_steps);
int mmf_radio_ig(const mmf_amil_desc* desc, const mmf_radio_reduce* rd, void* workspace, size_t workspace_bytes,
                 const mmf_surv_head* head, const mmf_ig_desc* ig, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Integrated-gradients attribution of the multimodal concat head in one call: how much of a patient's predicted risk comes
 *   from radiology, pathology and omics.  The reference's attribution script (create_attributions.py:93-164) runs captum's
 *   IntegratedGradients(n_steps = 20) on risk = -sum(S) from a joint zero baseline over all inputs through the captum
 *   methods of models/model_mm_attention_mil.py:202-396 and reduces each modality by sum |attr| (radio_attr, path_attr,
 *   omic_attr): n_steps autograd passes of the whole multimodal step.  captum interpolates all inputs with one alpha, so
 *   at node alpha, with a zero baseline,
 *     pathology  u_p = alpha (x_p W1p^T) + b1p                                   (mmf_amil_ig)
 *     radiology  u_r = alpha U_r + b1',  U_r = (X Wr^T) W1r^T,  b1' = W1r br + b1r  (mmf_radio_ig)
 *     omic       z1 = alpha Z + b_o0,  Z = W_o0 x_o;  h1 = selu(z1), z2 = W_o1 h1 + b_o1, O = selu(z2)
 *   and the input gradient is linear in the first pre-activation's gradient in all three: sum_k w_k dx_p,k = (sum_k w_k
 *   du_p,k) W1p;  sum_k w_k dX_r,k = ((sum_k w_k du_r,k) W1r) Wr;  sum_k w_k dx_o,k = W_o0^T (sum_k w_k dz1_k).  The L-wide
 *   contractions, reduce_dim, their transposes and W_o0 x_o run ONCE per call, the weight gradients never; only the H-wide
 *   part of each stack, the omic hidden layers and one head launch run per node.  The chain:
 *     1. once: U_p (the projection, no bias, no activation); Y = X Wr^T, U_r = Y W1r^T and b1' as mmf_radio_ig's steps 1-3;
 *        Z = W_o0 x_o, one wave per output (ceil(Gin / 64) + 6 dependent additions);
 *     2. per window of S nodes -- one S for the whole call: the smaller of what the window rule of mmf_amil_ig gives each
 *        present stack for window_steps -- for each stack its expansion, per-row tables, gate forward and pooling, whose merge
 *        writes the node's embedding into the stack's columns of feat [S x F]; the omic forward, one workgroup per node,
 *        O_s into its columns; the hazard head forward and the backward of risk over feat, giving dfeat [S x F] and the
 *        risks; for each stack the gather of its columns of dfeat, K-prep, K-dh and the fold into its Gacc; the omic
 *        backward, one workgroup per node, and the fold Gz += sum_s w_s dz1_s, in node order whatever the windows are;
 *     3. once: the pathology attribution GEMM (mmf_amil_ig's step 3); the radiology P = Gacc W1r and the segmented
 *        Q = P Wr (mmf_radio_ig's steps 5-7); attr_o[j] = x_o[j] sum_c Gz[c] W_o0[c, j], one wave per gene in a fixed order.
 *   No weight-gradient (TN) launch, no reduce list.  A branch that is absent contributes no launch.
 * mm: which branches are present (at least two) and where each one's embedding stands in the fused row -- path_col,
 *   radio_col, omic_col, the caller's order (the reference puts omic first when radiology is absent).  F = the sum of the
 *   present widths (path->H, radio->H, omic_We) <= 1024; the column ranges must tile 0 .. F - 1.  path / path_x: as desc / x
 *   of mmf_amil_ig, or path = NULL: no pathology branch.  radio / rd: as desc / rd of mmf_radio_ig, or radio = NULL.
 *   omic_x [Gin], or NULL: no omic branch; omic_W0 [W0 x Gin], omic_b0 [W0], omic_W1 [We x W0], omic_b1 [We]: fc_omic.0.0
 *   and fc_omic.1.0; Gin >= 1, W0 in 1..1024, We >= 1.  n_steps, alpha, weight, window_steps and the two riders as in
 *   mmf_ig_desc.  head: Wk [K x F], bk, K in 1..32; the optional outputs receive the values at alpha = 1.
 * Outputs (device): path_row_sum, path_row_abs [N_p], path_attr [N_p x L] or NULL; radio_row_sum, radio_row_abs
 *   [nseg x N_r], radio_attr [nseg x N_r x kseg] or NULL; omic_attr [Gin]; risk_x [1], risk_base [1], step_risk [n_steps].
 *   The outputs of an absent branch are neither read nor written.
 * Eval mode (dropout in either descriptor is refused), fp32 rows, exact-fp32 GEMMs.  Every sum is taken in a fixed order and
 *   there are no float atomics: two calls agree bit for bit.  No workgroup waits for another; the call allocates nothing,
 *   keeps no state and runs on one stream.
 * Returns, before any launch and in this order:
 *   MMF_ERR_ARG for a null mm, head, head->Wk or bk; n_steps outside 1..MMF_GROUP_MAX, window_steps < 0, a null alpha,
 *     weight, risk_x, risk_base or step_risk; fewer than two branches; then per present branch in the order pathology,
 *     radiology, omic: a null input, row_sum / row_abs (omic: omic_attr, a weight or a bias), p_h or p_att != 0, gemm =
 *     MMF_GEMM_BF16X3, a null rd, rd->x, rd->W, rd->bias or (nseg in 2..4) rd->x[m];
 *   MMF_ERR_SHAPE for what mmf_amil_ig / mmf_radio_ig refuse of a stack with it (nseg outside 2..4, the descriptor's rules,
 *     kseg != radio->L, N_r nseg kseg 4 >= 2^31), Gin < 1, W0 outside 1..1024, We < 1, F > 1024, columns that overlap or
 *     leave 0 .. F - 1, K outside 1..32, or a bag too long for one step to be a window;
 *   MMF_ERR_ALIGN for what the single-head calls refuse with it (the omic operands are read element by element: any
 *     alignment; a null workspace is MMF_ERR_ARG and is found here, as in the single-head calls); MMF_ERR_WORKSPACE.
 * mmf_mm_ig_workspace_bytes: the workspace of that call; a branch is absent with N_p = 0, N_r = 0 or Gin = 0.  0 for
 *   n_steps outside 1..MMF_GROUP_MAX, window_steps < 0, fewer than two branches, a negative extent, and for a present branch
 *   what mmf_amil_ig_workspace_bytes / mmf_radio_ig_workspace_bytes answer 0 for, W0 outside 1..1024, We < 1 or
 *   F > 1024.  It does not shrink as window_steps grows.
 * fusion = 'tensor' has mmf_mm_ig_tensor (below, behind mmf_xfusion_weights).  Out of scope: radio_fusion = 'tensor'; non-zero
 *   baselines; bf16 bags; targets other than risk; the omic-only MaxNet.  The stage-2 pretrained models have mmf_stage2_ig.
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_mm_ig_desc {
  int32_t n_steps;               /* quadrature nodes, 1 .. MMF_GROUP_MAX */
  int32_t window_steps;          /* nodes per window; 0: the library chooses */
  const float* alpha;            /* HOST [n_steps] */
  const float* weight;           /* HOST [n_steps] */
  const mmf_amil_desc* path;     /* the pathology stack, or NULL: no pathology branch */
  const float* path_x;           /* [N_p x L] */
  float* path_row_sum;           /* [N_p] out */
  float* path_row_abs;           /* [N_p] out */
  float* path_attr;              /* [N_p x L] out, or NULL */
  const mmf_amil_desc* radio;    /* the radiology stack, or NULL: no radiology branch */
  const mmf_radio_reduce* rd;    /* reduce_dim and the modalities, nseg 2..4 */
  float* radio_row_sum;          /* [nseg x N_r] out */
  float* radio_row_abs;          /* [nseg x N_r] out */
  float* radio_attr;             /* [nseg x N_r x kseg] out, or NULL */
  const float* omic_x;           /* [Gin], or NULL: no omic branch */
  const float* omic_W0;          /* [W0 x Gin] fc_omic.0.0.weight */
  const float* omic_b0;          /* [W0] */
  const float* omic_W1;          /* [We x W0] fc_omic.1.0.weight */
  const float* omic_b1;          /* [We] */
  float* omic_attr;              /* [Gin] out */
  int32_t omic_Gin, omic_W0n, omic_We;
  int32_t path_col, radio_col, omic_col;   /* first column of each present branch in the fused row */
  float* risk_x;                 /* [1] out */
  float* risk_base;              /* [1] out */
  float* step_risk;              /* [n_steps] out */
} mmf_mm_ig_desc;
size_t mmf_mm_ig_workspace_bytes(int64_t N_p, int32_t L_p, int32_t H_p, int32_t D_p, int32_t gated_p, int64_t N_r,
                                 int32_t nseg, int32_t kseg, int32_t H_r, int32_t D_r, int32_t gated_r, int32_t Gin,
                                 int32_t W0, int32_t We, int32_t n_steps, int32_t window_steps);
int mmf_mm_ig(const mmf_mm_ig_desc* mm, void* workspace, size_t workspace_bytes, const mmf_surv_head* head, void* stream);

/* The hazard head's training step on a feature vector that is already on the device: what
 *   `hazards, S, Y_hat = head(classifier(feat)); loss = NLLSurvLoss(alpha)(hazards, S, Y, c); (loss * loss_scale).backward()`
 * computes between the embedding and the loss (models/model_mm_attention_mil.py:190-191 with fusion = 'concat': feat is the
 * concatenation of the branch embeddings, which the caller lets the branches write side by side; utils/loss_utils.py:22-39)
 * in ONE single-workgroup launch: classifier, sigmoid, cumprod, argmax, the loss, dWk / dbk (target->accumulate as above) and
 * dfeat [F] = d(loss * loss_scale) / d feat, which the caller hands to the branches' backward calls.  F <= 1024, K <= 32. */
int mmf_surv_head_nll_step(const float* feat, int32_t F, const mmf_surv_head* head, const mmf_nll_target* target,
                           float* dfeat, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped training step of the multimodal concat head: the G patients of one accumulation window, each with up to three
 *   branches, as one launch chain per branch around ONE head launch.  The reference runs models/model_mm_attention_mil.py:
 *   128-200 once per patient inside the window of utils/core_utils.py:200-247; with fixed weights the patients are
 *   independent forward passes, each stack's GEMMs run once over the window's concatenated rows (as in
 *   mmf_amil_nll_step_group) and the classifier reads row g of a [G x F] feature matrix that the branches write side by
 *   side (torch.cat of model_mm_attention_mil.py:168-187 is never a launch).  The caller sequences, on one stream:
 *   radio forward, pathology forward, omic forward, mmf_surv_head_nll_step_group, then the three backward halves.
 *
 * mmf_amil_group_forward: the forward half of mmf_amil_nll_step_group's chain on the pathology stack
 *   (model_mm_attention_mil.py:154-160 for every patient): per-row tables, projection, gate, pooling partials, and a per-bag
 *   merge that writes M_g to M + g * ldm (ldm >= H floats: the stack's columns of the feature matrix) and A_raw [sum N].
 *   Everything the backward half needs -- h, a, b, the row tables, M_g and the softmax statistics -- stays in the workspace
 *   (mmf_amil_group_workspace_bytes), which must reach mmf_amil_group_backward unmodified.  desc, group, x and the masks as
 *   in mmf_amil_nll_step_group.
 * mmf_amil_group_backward: the backward half from dM (row g at dM + g * ldm: the stack's columns of
 *   mmf_surv_head_nll_step_group's dfeat): K-prep, K-dh, split-K TN and the reduce launch.  grads: overwritten, or added
 *   to when accumulate != 0; grads->dx must be NULL.  group->seeds is not read again (the row tables are in the workspace)
 *   but must be given.  ldm == H: dM itself is read, and must be 16-byte aligned.
 * mmf_radio_group_forward / mmf_radio_group_backward: the same pair behind reduce_dim (model_mm_attention_mil.py:132-150),
 *   mmf_radio_nll_step_group's launches cut at the same point; rd and the workspace (mmf_radio_group_workspace_bytes) as there;
 *   the forward reads neither rd->dW nor rd->db.
 * All four return what mmf_amil_nll_step_group / mmf_radio_nll_step_group return for the same arguments, in the same order,
 *   and MMF_ERR_SHAPE for ldm < H.  No workgroup waits for another; calls are deterministic.
 *
 * mmf_surv_head_nll_step_group: mmf_surv_head_nll_step for the G patients of the window (model_mm_attention_mil.py:190-194,
 *   utils/loss_utils.py:22-39, utils/core_utils.py:207 per patient): one workgroup per patient over feat [G x F] (row g at
 *   feat + g * ldf; F <= 1024, K <= 32, G <= MMF_GROUP_MAX) and one reduce launch.  The per-patient arrays of head / target
 *   are G long, as in mmf_amil_nll_step_group.  dfeat [G x F] (row g at dfeat + g * F) = d(loss_g * loss_scale) / d feat_g.
 *   dWk / dbk: the sum over the patients, in patient order, overwritten or (target->accumulate) added to.
 *   workspace: mmf_surv_head_group_workspace_bytes(F, K, G) -- the per-patient slabs -- which is 0 for an F, K or G out of range.
 * ------------------------------------------------------------------------------------------- */
int mmf_amil_group_forward(const mmf_amil_desc* desc, const mmf_bag_group* group, const float* x, void* workspace,
                           size_t workspace_bytes, float* M, int32_t ldm, float* A_raw /* [sum N] */, void* stream);
int mmf_amil_group_backward(const mmf_amil_desc* desc, const mmf_bag_group* group, const float* x, void* workspace,
                            size_t workspace_bytes, const float* dM, int32_t ldm, const float* A_raw,
                            const mmf_amil_grads* grads, int32_t accumulate, void* stream);
int mmf_radio_group_forward(const mmf_amil_desc* desc, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                            void* workspace, size_t workspace_bytes, float* M, int32_t ldm, float* A_raw, void* stream);
int mmf_radio_group_backward(const mmf_amil_desc* desc, const mmf_bag_group* group, const mmf_radio_reduce* rd,
                             void* workspace, size_t workspace_bytes, const float* dM, int32_t ldm, const float* A_raw,
                             const mmf_amil_grads* grads, int32_t accumulate, void* stream);
size_t mmf_surv_head_group_workspace_bytes(int32_t F, int32_t K, int32_t G);
int mmf_surv_head_nll_step_group(const float* feat, int32_t ldf, int32_t F, int32_t G, const mmf_surv_head* head,
                                 const mmf_nll_target* target, float* dfeat, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped forward-only pass of the multimodal head, both fusions: what the validation pass and the summary
 *   (utils/core_utils.py:267-430) compute for G patients by running models/model_mm_attention_mil.py:128-200 once per
 *   patient under no_grad.  The stacks and the omic branch need nothing new: mmf_amil_infer_group / mmf_radio_infer_group
 *   with head = NULL write M [G x H] (model_mm_attention_mil.py:132-160), and the eval-mode SNN (:162-166,
 *   models/model_modules.py:64-68) is mmf_dense_forward on a B = G batch.  Behind them, on the same stream:
 *
 * mmf_xfusion_infer_group (fusion = 'tensor'): the XlinearFusion block (models/model_modules.py:156-178 with gate = 1,
 *   skip = 1) and classifier[0] + ReLU (model_mm_attention_mil.py:182-188) for G patients in FOUR launches:
 *     1. the gating stage, one workgroup per patient (model_modules.py:158-165: h, z, sigmoid(z) * h, o);
 *     2. the Kronecker product of [o_i, 1] (:164-171) fused into encoder1 (:172): the (sdim + 1)^m-wide product is never
 *        written, and every row of encoder1's weight is fetched from memory once per window, not once per patient;
 *     3. encoder2 (:173-176), which reads its skip connection [e1 | v_0 | v_1 (| v_2)] from where the parts lie;
 *     4. classifier[0] + ReLU.
 *   v: HOST array of m device pointers, each a dense [G x dim] matrix (16-byte aligned).  MM [G x mmhid2]: encoder2's
 *   output (what forward(return_features=True) returns); hid [G x nhid].  Eval mode only: there is no dropout argument
 *   and nothing is kept for a backward.  Every output element is summed in an order that depends on the element alone:
 *   what a patient gets is bit for bit what the same call gives it alone (G = 1).
 *   Returns MMF_ERR_SHAPE for m outside 2..3, sdim != 16, dim % 4 != 0, mmhid1 + m * dim or mmhid2 > 1536, G outside
 *   1..MMF_GROUP_MAX; MMF_ERR_ARG for a null pointer; MMF_ERR_ALIGN for a misaligned v_i, Wh_i, Wz_i or workspace;
 *   MMF_ERR_WORKSPACE.  Each refusal happens before any launch.
 * mmf_xfusion_group_infer_workspace_bytes: its workspace (o and encoder1's output), or 0 for arguments out of range.
 *
 * mmf_surv_head_infer_group: the hazard head (model_mm_attention_mil.py:190-194; utils/loss_utils.py:22-39 and
 *   utils/core_utils.py:207 when a target is given) for G patients, forward only, in ONE launch of one workgroup per
 *   patient.  Patient g's feature row is the concatenation of row g of nseg (1..3) dense [G x widths[s]] device buffers
 *   (segs, widths: HOST arrays) -- the branch embeddings of the concat fusion in the model's order, so torch.cat
 *   (:168-187) is never a launch, or hid of the tensor fusion as one segment.  sum widths <= 1024, K <= 32,
 *   G <= MMF_GROUP_MAX.  head: the per-patient arrays are G long, Wk is [K x sum widths].  target (optional): each
 *   patient's nll_surv VALUE; only Y, c [G], alpha, eps and loss [G] are read, as in mmf_amil_infer_group.  The head is
 *   the device code of mmf_surv_head_nll_step_group with its backward compiled out: the same outputs bit for bit.
 *   Returns MMF_ERR_SHAPE / MMF_ERR_ARG on the lines of mmf_surv_head_nll_step_group, before any launch.
 * No workgroup waits for another; no float atomics; the calls allocate nothing and keep no state.
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_xfusion_weights {
  int32_t m;                         /* modalities, 2 or 3 */
  int32_t dim, sdim;                 /* embedding width (256), gated width (16) */
  int32_t mmhid1, mmhid2, nhid;      /* rows of encoder1, encoder2, classifier[0] */
  const float *Wh[3], *bh[3];        /* reduce.i.0.0: [sdim x dim], [sdim] */
  const float *Wz[3], *bz[3];        /* reduce.i.1.0: [sdim x m * dim], [sdim] */
  const float *Wo[3], *bo[3];        /* reduce.i.2.0: [sdim x sdim], [sdim] */
  const float *We1, *be1;            /* encoder1.0: [mmhid1 x (sdim + 1)^m], [mmhid1] */
  const float *We2, *be2;            /* encoder2.0: [mmhid2 x mmhid1 + m * dim], [mmhid2] */
  const float *Wc0, *bc0;            /* classifier.0: [nhid x mmhid2], [nhid] */
} mmf_xfusion_weights;
size_t mmf_xfusion_group_infer_workspace_bytes(int32_t m, int32_t sdim, int32_t mmhid1, int32_t G);
int mmf_xfusion_infer_group(const mmf_xfusion_weights* w, const float* const* v, int32_t G, void* workspace,
                            size_t workspace_bytes, float* MM, float* hid, void* stream);
int mmf_surv_head_infer_group(const float* const* segs, const int32_t* widths, int32_t nseg, int32_t G,
                              const mmf_surv_head* head, const mmf_nll_target* target, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped training step of the tensor fusion: the XlinearFusion block (models/model_modules.py:156-178, gate = 1,
 *   skip = 1) and classifier[0] + ReLU + Dropout (models/model_mm_attention_mil.py:182-188), forward and backward, for
 *   the G patients of one accumulation window -- what the reference computes once per patient under autograd.  The
 *   stacks and the omic branch write their embeddings with the existing grouped calls (mmf_amil_group_forward,
 *   mmf_radio_group_forward, mmf_dense_forward_rows, all through a leading dimension); the hazard head on hid is
 *   mmf_surv_head_nll_step_group with classifier[3].
 *
 * x2 [G x K2], K2 = mmhid1 + m * dim, dense, 16-byte aligned: encoder2's input matrix.  The caller puts v_i of patient
 *   g at x2[g][mmhid1 + i * dim ..] (the branches write there: torch.cat is never a launch); the forward fills the first
 *   mmhid1 columns with encoder1's output.  x2, MM, hid and the workspace must reach the backward unmodified.
 * Dropout: patient g draws its own masks -- site i for o_i, 8 for the product, 9 encoder1, 10 encoder2 (drop_p) and 11
 *   classifier[0] (cls_drop_p); within a site the mask index is the column index, as a B = 1 call draws it.  row_base:
 *   DEVICE [G], row_base[g] = mmf_dropout_row_base(fusion seed of patient g); seed_dev as everywhere.  Both
 *   probabilities 0: eval mode, MM and hid are those of mmf_xfusion_infer_group bit for bit.
 * mmf_xfusion_group_forward, FOUR launches: the gating stage per patient (keeps h, z, gm and the dropped o, and hashes the
 *   post-fusion mask once per patient and element into packed keep bits); the Kronecker product fused into encoder1 (the
 *   product is never written, a row of encoder1's weight is fetched once per window, the keep bits are staged in LDS);
 *   encoder2; classifier[0].  MM [G x mmhid2], hid [G x nhid].
 * mmf_xfusion_group_backward, from dhid (row g at dhid + g * lddhid: mmf_surv_head_nll_step_group's dfeat): classifier[0]
 *   and encoder2 through the dense backward on B = G rows; d of the product [G x (sdim + 1)^m] in one pass over encoder1's
 *   weight; encoder1's weight gradient, written once, with the product rebuilt from [o, 1] and the keep bits (no
 *   [G x mmhid1 x (sdim + 1)^m] intermediate); the gating stage per patient; the gating weights, one thread per element.
 *   dx2 [G x K2]: columns mmhid1 + i * dim .. hold dv_i, skip connection included (the first mmhid1 columns hold d e1).
 *   grads: sums over the patients in patient order, overwritten, or added to when accumulate != 0.
 * No float atomics, no workgroup waits for another, calls are deterministic; what patient g gets (MM, hid, dx2 rows)
 *   depends neither on G nor on its position.  The calls allocate nothing and keep no state.
 * Returns, before any launch: MMF_ERR_SHAPE for m outside 2..3, sdim != 16, dim % 4 != 0, mmhid1 % 4 != 0, mmhid1 + m * dim,
 *   mmhid2 or nhid > 1536, G outside 1..MMF_GROUP_MAX, lddhid < nhid; MMF_ERR_ARG for a null pointer or a probability
 *   outside [0, 1); MMF_ERR_ALIGN for a misaligned x2, Wh_i, Wz_i or workspace; MMF_ERR_WORKSPACE.
 * mmf_xfusion_group_workspace_bytes: the workspace of the pair, or 0 for arguments out of range.
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_xfusion_grads {     /* mmf_xfusion_weights' order */
  float *dWh[3], *dbh[3];
  float *dWz[3], *dbz[3];
  float *dWo[3], *dbo[3];
  float *dWe1, *dbe1;
  float *dWe2, *dbe2;
  float *dWc0, *dbc0;
} mmf_xfusion_grads;
size_t mmf_xfusion_group_workspace_bytes(int32_t m, int32_t dim, int32_t sdim, int32_t mmhid1, int32_t mmhid2,
                                         int32_t nhid, int32_t G);
int mmf_xfusion_group_forward(const mmf_xfusion_weights* w, float* x2, int32_t G, float drop_p, float cls_drop_p,
                              const uint32_t* row_base, const uint32_t* seed_dev, void* workspace, size_t workspace_bytes,
                              float* MM, float* hid, void* stream);
int mmf_xfusion_group_backward(const mmf_xfusion_weights* w, const float* x2, int32_t G, float drop_p, float cls_drop_p,
                               const uint32_t* row_base, const uint32_t* seed_dev, const float* MM, const float* hid,
                               const float* dhid, int32_t lddhid, void* workspace, size_t workspace_bytes, float* dx2,
                               const mmf_xfusion_grads* grads, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Integrated-gradients attribution of the multimodal tensor-fusion head in one call (fusion = 'tensor', the model's
 *   default): mmf_mm_ig's question for the head whose embeddings meet in the XlinearFusion block.  The reference's captum
 *   methods (models/model_mm_attention_mil.py:202-396) take that branch like any other: n_steps autograd passes, each with
 *   every weight gradient of both stacks and of the tail, encoder1's 10 MB weight gradient among them.
 * The identity of mmf_mm_ig holds unchanged up to the embeddings: the L-wide contractions, reduce_dim, their transposes
 *   and W_o0 x_o run once per call, the H-wide part of each stack and the omic hidden layers per node.  The tail -- the
 *   gating stage, the Kronecker product fused into encoder1, encoder2 with its skip connection, classifier[0] and
 *   classifier[3] -- is nonlinear in the embeddings: nothing of it folds, and for the S nodes of a window it is the
 *   "G patients of a window" problem of mmf_xfusion_group_forward / _backward with G = S in eval mode, without its weight
 *   gradients.  The chain, on one stream, nothing allocated:
 *     1. once: step 1 of mmf_mm_ig;
 *     2. per window of S nodes (S as in mmf_mm_ig; S <= MMF_GROUP_MAX): the branches' forward halves as in mmf_mm_ig, each
 *        writing its embedding into its columns of encoder2's input rows x2 [S x K2], K2 = mmhid1 + m dim, column
 *        mmhid1 + {path,radio,omic}_col; then SEVEN launches: the gating stage, the product fused into encoder1, encoder2
 *        (mmf_xfusion_group_forward's first three at p = 0); one workgroup per node for hid = relu(Wc0 MM_s + bc0) kept in
 *        LDS, the hazard head and the backward of risk (the device body of mmf_mm_ig's head launch), dpre0 = dhid . [hid >
 *        0] and dMM_s = dpre0 Wc0; encoder2's input gradient (the dense backward's dx blocks alone); d of the product in one
 *        pass over encoder1's weight; the gating stage's backward, which adds dv_i to the skip connection's gradient in
 *        dx2.  Then the branches' backward halves as in mmf_mm_ig on their columns of dx2 (pitch K2);
 *     3. once: step 3 of mmf_mm_ig.
 *   No weight-gradient launch (no TN, no dWe1, no gating dW), no add-into, no float atomics, no workgroup waits for another;
 *   every sum is taken in an order fixed by its output element: two calls agree bit for bit.
 * mm: mmf_mm_ig_desc as for mmf_mm_ig, except that path_col / radio_col / omic_col are the branch's first column within the
 *   m dim embedding columns of encoder2's input row: they must tile 0 .. m dim - 1 in steps of dim, every present width
 *   (path->H, radio->H, omic_We) must equal xf->dim, and xf->m the number of present branches.  xf: the tail's weights,
 *   classifier[0] included, as for mmf_xfusion_group_forward.  head: classifier[3], Wk [K x nhid], bk, K in 1..32; the
 *   optional outputs receive the values at alpha = 1.  Outputs as mmf_mm_ig.
 * Returns, before any launch and in this order:
 *   MMF_ERR_ARG for everything mmf_mm_ig refuses with it, a null xf, or a null weight or bias of xf;
 *   MMF_ERR_SHAPE for everything mmf_mm_ig refuses of the stacks and the omic widths, what mmf_xfusion_group_forward
 *     refuses of xf with G = S, xf->m != the number of branches, a width != xf->dim, columns that do not tile, nhid > 1024
 *     (hid is kept in LDS), K outside 1..32, or a bag too long for one step to be a window;
 *   MMF_ERR_ALIGN for everything mmf_mm_ig refuses with it, then Wh_i or Wz_i off 16 bytes; MMF_ERR_WORKSPACE.
 * mmf_mm_ig_tensor_workspace_bytes: mmf_mm_ig_workspace_bytes' arguments, then the tail's extents (m is the number of
 *   present branches).  0 for what that query answers 0 for but F > 1024, and for a tail refused by shape.  Otherwise that
 *   query's stack and omic parts (no feat / dfeat) plus, with S the window's nodes and every array rounded up to 256 bytes,
 *     4 S (2 K2 + 3 mmhid2 + 7 m 16 + (sdim + 1)^m + 1) + 4 S words((sdim + 1)^m)  bytes:
 *   x2, dx2 [S x K2]; MM, dMM and the dense backward's dpre [S x mmhid2]; o, h, z, gm, dpo, dz, dph [S x m x 16]; dkr
 *   [S x (sdim + 1)^m]; the seed table the forward launches ask for [S]; the keep bits, words(E) = 2 ceil(E / 64) per node.
 *   Monotone in S; it does not shrink as window_steps grows.
 * Out of scope: radio_fusion = 'tensor'; non-zero baselines; bf16 bags; targets other than risk; the omic-only MaxNet.  The
 *   stage-2 pretrained models have mmf_stage2_ig.
 * ------------------------------------------------------------------------------------------- */
size_t mmf_mm_ig_tensor_workspace_bytes(int64_t N_p, int32_t L_p, int32_t H_p, int32_t D_p, int32_t gated_p, int64_t N_r,
                                        int32_t nseg, int32_t kseg, int32_t H_r, int32_t D_r, int32_t gated_r, int32_t Gin,
                                        int32_t W0, int32_t We, int32_t n_steps, int32_t window_steps, int32_t dim,
                                        int32_t sdim, int32_t mmhid1, int32_t mmhid2, int32_t nhid);
int mmf_mm_ig_tensor(const mmf_mm_ig_desc* mm, const mmf_xfusion_weights* xf, void* workspace, size_t workspace_bytes,
                     const mmf_surv_head* head, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Integrated-gradients attribution of the stage-2 fusion models, a cohort of P patients in one call: how much of each
 *   patient's predicted risk comes from the radiology, pathology and omic embeddings.  This is what the reference's
 *   attribution script runs (create_attributions.py:93-164): captum's IntegratedGradients(n_steps = 20) from a zero
 *   baseline through the captum* methods of a multimodal_pretrained (models/nll_models_pretrained.py:200-320, the
 *   cox / ranking twin likewise), one patient at a time, reduced per modality to sum attr (attr_orig.csv) and sum |attr|
 *   (attr.csv): n_steps autograd passes per patient through 10-30 small launches, weight gradients included.
 * In eval mode BatchNorm1d is a per-feature affine map (s = weight / sqrt(var + eps), t = bias - mean s) and dropout is
 *   off, so a row's result depends on that row alone: P patients x S nodes are independent rows.  The first layer of every
 *   train type but kronecker is linear in alpha -- fcnn blocks: u(alpha) = alpha (v W0^T) + b0; Highway layer 0 behind bn1:
 *   z_*(alpha) = alpha ((v . s1) W_*^T) + (W_* t1 + b_*) for * in {gate, nonlinear, linear} -- and the input gradient
 *   folds the same way: sum_k w_k d risk / d(alpha_k v) = (sum_k w_k du_k) W0, respectively s1 . sum_* (sum_k w_k dz_*,k) W_*.
 *   With n_layers = 1 nothing that remains per node is a contraction wider than the K-row classifier.  The chain, on one
 *   stream, THREE launches whatever P and n_steps are:
 *     1. U [(P + 1) x ldU] = the packed rows [v_0 | .. | v_{m-1}] (times s1) against every first-layer matrix of the model;
 *        row P is t1 (0 without a bn1) and receives the biases: the constants of every pre-activation;
 *     2. the node sweep, one workgroup per patient: pre-activations and accumulators in registers; per node the activations
 *        (BN + ReLU, or the sigmoid / ReLU mix and bn2), the classifier, the hazard head and the backward of risk (or the cox
 *        scalar), the gradient down to the pre-activations, G += w_k d.  Per node it writes step_risk only;
 *     3. dx = G against the transposed first layer, attr = v . s1 . dx, and its sums per patient and modality.
 *   No weight-gradient launch, no float atomics, no workgroup waits for another; every sum is taken in an order fixed by
 *   its output element: two calls agree bit for bit, and a patient's results do not depend on the cohort around it.
 * Highway with n_layers >= 2 (up to 8): layer 0 folds as above (launches 1 and 3 unchanged); in the sweep's place the call's
 *   P (n_steps + 2) rows -- patient-major, a patient's nodes, then its riders alpha = 1 and alpha = 0 -- pass in windows
 *   of up to 256 rows, which may straddle patients: a launch that forms layer 0's output of every row from U; per layer
 *   >= 1 and Highway the three dense forwards and the mix (the kernels of mmf_dense_forward and mmf_highway_mix_forward);
 *   a head launch (bn2, the classifier, the hazard head and the backward of risk, or the cox scalar); per layer and
 *   Highway, backwards, the mix's backward, the three dense input gradients (mmf_dense_backward's kernel without dW and
 *   db) and their sum; and a launch that rebuilds layer 0's derivative from U and adds w_k d risk / d z_* to the patient's
 *   G in node order whatever the windows are.  No weight-gradient launch.
 * kronecker: nothing folds.  The call's P (n_steps + 2) rows -- patient-major, a patient's nodes, then its riders alpha = 1
 *   and alpha = 0 -- are the "G patients" of mmf_xfusion_group_forward in eval mode and pass in windows of up to
 *   MMF_GROUP_MAX rows, which may straddle patients: an expansion launch (alpha_k v_i into encoder2's input rows), the SEVEN
 *   tail launches of mmf_mm_ig_tensor's step 2 -- the gating stage, the product fused into encoder1, encoder2; a head
 *   launch without classifier[0] (the stage-2 classifier is Linear(256, K) on the fusion's output); encoder2's input
 *   gradient, d of the product, the gating stage's backward -- and a fold launch that adds w_k d risk / d(alpha_k v) to
 *   each patient's accumulator in node order whatever the windows are.  One launch ends the call: attr = v . accumulator
 *   and its sums.  No weight-gradient launch (encoder1's 10 MB gradient among them).
 * desc: family (MMF_STAGE2_NLL: risk = -sum_k S_k of the sigmoid hazards, K in 1..32; MMF_STAGE2_COX: the model's scalar
 *   output, K = 1); train_type; radio / path / omic != 0: the modalities the mode keeps -- two or three, in the reference's
 *   cat / v_list order [radio, path] | [radio, omic] | [omic, path] | [radio, path, omic]; v[i] [P x 256], blk[i] and attr[i]
 *   follow that order, m is their number.  A modality the mode drops takes no part (the late types evaluate it in forward,
 *   captum_* does not take it as an input).  n_layers: the Highways' depth.  alpha / weight: HOST arrays of the n_steps
 *   nodes and weights, as in mmf_ig_desc; alpha = 1 and alpha = 0 ride along with weight 0.
 *   blk: the early types use blk[0] (over the 256 m wide cat), the late types blk[i] for v[i].  fcnn: W0 [128 x Kin], b0, bn
 *   (BatchNorm1d(128)); the cox late-fcnn blocks end in their own Linear(128, 1): W4 [1 x 128], b4 [1].  highway: bn1, bn2
 *   [Kin], and HOST arrays of n_layers device pointers Wgate, bgate, Wnl, bnl, Wlin, blin ([Kin x Kin], [Kin] each).
 *   Wk, bk: the classifier behind them -- [K x 128] early-fcnn, [K x 128 m] late-fcnn (cox: [1 x m], over the blocks'
 *   scalars), [K x 256 m] the highway types, [K x 256] kronecker (xf: the XlinearFusion weights; Wc0, bc0 and nhid are
 *   not read).
 * Outputs (device): mod_sum, mod_abs [P x m] = sum attr, sum |attr| over a modality's 256 columns; attr[i] [P x 256] or
 *   NULL; risk [P] at alpha = 1, risk_base [P] at alpha = 0, step_risk [P x n_steps]; hazards, S [P x K] at alpha = 1 (nll;
 *   each may be NULL; not written for cox).
 * Returns, before any launch and in this order:
 *   MMF_ERR_ARG for a null desc, alpha, weight, Wk, bk, mod_sum, mod_abs, risk, risk_base or step_risk, a family or
 *     train_type the header does not name, a null v[i], a null weight, bias or BatchNorm array of a block the type reads
 *     (a null entry of the per-layer arrays included), kronecker without xf;
 *   MMF_ERR_SHAPE for fewer than two modalities, P outside 1..1,048,576, n_steps outside 1..MMF_GROUP_MAX, K outside 1..32
 *     (cox: K != 1), n_layers < 1, a highway type with n_layers > 8, an xf that is not the stage-2 fusion's (m modalities,
 *     dim 256, sdim 16, mmhid1 = mmhid2 = 256);
 *   MMF_ERR_ALIGN for a v[i], a non-null attr[i] or the workspace off 16 bytes (a null workspace is MMF_ERR_ARG, found
 *     here), kronecker: Wh_i or Wz_i off 16 bytes; MMF_ERR_WORKSPACE.
 * mmf_stage2_ig_workspace_bytes: U [(P + 1) x ldU] and G [P x ldU] floats, each rounded up to 256 bytes, ldU = 128
 *   (early-fcnn), 128 m (late-fcnn) or 768 m (highway); m: the number of modalities.  highway with n_layers >= 2: 4 n_layers +
 *   5 more buffers of S x 256 m floats, S = min(256, P (n_steps + 2)).  kronecker: the accumulator
 *   [P x 256 m] and the tail's buffers of mmf_mm_ig_tensor_workspace_bytes' formula for S = min(MMF_GROUP_MAX, P (n_steps +
 *   2)) rows (K2 = 256 + 256 m, mmhid2 = 256).  0 for what the call refuses by shape or for an unknown enum.  Monotone in P
 *   and in n_steps.
 * The ABI version is unchanged: the entry points are additive.
 * Out of scope: unimonal_pretrained; the `residual` type; train mode; non-zero baselines; targets other than risk.
 * ------------------------------------------------------------------------------------------- */
#define MMF_STAGE2_NLL 0
#define MMF_STAGE2_COX 1
#define MMF_STAGE2_EARLY_FCNN 0
#define MMF_STAGE2_LATE_FCNN 1
#define MMF_STAGE2_EARLY_HIGHWAY 2
#define MMF_STAGE2_LATE_HIGHWAY 3
#define MMF_STAGE2_KRONECKER 4
typedef struct mmf_bn1d {            /* nn.BatchNorm1d in eval mode */
  const float* weight;               /* [F] */
  const float* bias;                 /* [F] */
  const float* mean;                 /* [F] running_mean */
  const float* var;                  /* [F] running_var */
  float eps;                         /* 1e-5 */
} mmf_bn1d;
typedef struct mmf_stage2_block {
  const float* W0;                   /* fcnn: [128 x Kin] */
  const float* b0;                   /* [128] */
  mmf_bn1d bn;                       /* fcnn: BatchNorm1d(128) */
  const float* W4;                   /* cox late-fcnn: [1 x 128] */
  const float* b4;                   /* [1] */
  mmf_bn1d bn1, bn2;                 /* highway: [Kin] each */
  const float* const* Wgate;         /* highway: HOST [n_layers] device pointers, [Kin x Kin] */
  const float* const* bgate;         /* HOST [n_layers], [Kin] */
  const float* const* Wnl;
  const float* const* bnl;
  const float* const* Wlin;
  const float* const* blin;
} mmf_stage2_block;
typedef struct mmf_stage2_ig_desc {
  int32_t family, train_type;
  int32_t radio, path, omic;         /* != 0: the mode keeps the modality */
  int32_t n_layers;
  int32_t P, K, n_steps;
  const float* alpha;                /* HOST [n_steps] */
  const float* weight;               /* HOST [n_steps] */
  const float* v[3];                 /* [P x 256] each, the present modalities in cat order */
  mmf_stage2_block blk[3];
  const mmf_xfusion_weights* xf;     /* kronecker, else NULL */
  const float* Wk;
  const float* bk;
  float* mod_sum;                    /* [P x m] out */
  float* mod_abs;                    /* [P x m] out */
  float* attr[3];                    /* [P x 256] out each, or NULL */
  float* risk;                       /* [P] out */
  float* risk_base;                  /* [P] out */
  float* step_risk;                  /* [P x n_steps] out */
  float* hazards;                    /* [P x K] out (nll), or NULL */
  float* S;                          /* [P x K] out (nll), or NULL */
  struct mmf_trace* trace;           /* optional kernel trace, or NULL */
} mmf_stage2_ig_desc;
size_t mmf_stage2_ig_workspace_bytes(int32_t family, int32_t train_type, int32_t m, int32_t n_layers, int32_t P, int32_t K,
                                     int32_t n_steps);
int mmf_stage2_ig(const mmf_stage2_ig_desc* desc, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stage-2 fcnn and highway models, ONE training step in ONE call: the forward of a batch [B x 256] per modality, the loss,
 *   every parameter gradient and the BatchNorm running statistics.
 *   replaces multimodal_pretrained.forward of both families (models/nll_models_pretrained.py:66-197: the hazards head, risk =
 *   -sum S; models/coxranking_models_pretrained.py:62-200: the scalar output) for train_type early-fcnn, late-fcnn,
 *   early-highway and late-highway, the Highway and the fcnn blocks (models/model_modules.py:5-27, nll_models_pretrained.py:
 *   82-90), NLLSurvLoss / CoxSurvLoss / RankingSurvLoss / RankingNLLSurvLoss (utils/loss_utils.py:22-39, 58-101, 124-164) and
 *   the backward autograd derives from them, as utils/core_utils_pretrained.py:185-232 runs them per batch: 20 to 45
 *   launches through the composable entry points below (mmf_dense_*, mmf_batchnorm_*, mmf_highway_mix_*, mmf_hazards_*,
 *   mmf_nll_surv / mmf_cox_surv / mmf_ranking_loss).
 * No workgroup waits for another; launch boundaries are the only ordering between workgroups, there are no tick words and
 *   no atomics, and every sum runs in an order fixed by its output element: two calls agree bit for bit.  A workgroup owns
 *   four features for all B rows, so a feature's batch statistics, its BatchNorm, the activation, dropout, the running
 *   statistics and, on the way back, dgamma, dbeta, db and its rows of dW never leave the CU.  The chain, on one stream:
 *   fcnn types, THREE launches (forward only: two):
 *     1. per block (every block of a late type in the same launch): u = x W0^T + b0, the statistics, y = drop(relu(bn(u))),
 *        the running statistics;
 *     2. row tiles: the classifier (the cox late blocks' own Linear(128, 1) first), hazards, S, risk;
 *     3. every workgroup rebuilds d loss / d logits of all rows from the B risks, labels and times (at most 256^2 pair
 *        terms); the first one writes the loss; each then takes its columns' dy, the dropout / ReLU / BatchNorm backward,
 *        its rows of dW0, db0 and its elements of the classifier's gradient.
 *   highway types, 2 n_layers + 3 launches (forward only: n_layers + 2):
 *     1. x0 = drop(bn1(h)) and the running statistics;  2 .. n_layers + 1. one launch per layer: the three contractions and
 *        the mix, bn2 and its running statistics folded into the last;  then the head as above;
 *     backwards: the owners of the last layer's features take d loss / d logits as above, the classifier's gradient, bn2's
 *        backward, the mix's backward, dz and the layer's dW rows and db; per layer below, the owner of column j forms dx[:, j]
 *        = sum_n dz_*[:, n] W_*[n, j] of the layer above and does the same; the last launch takes dx of layer 0 through the
 *        dropout mask and bn1's backward.
 *   A forward-only call (grads == NULL: validation) runs its head as one workgroup, which ends with the loss.
 * desc: family, train_type (MMF_STAGE2_*; kronecker is not taken); radio / path / omic != 0: the modalities the mode keeps, two or
 *   three, the classifier's input in the reference's cat order [radio, path] | [radio, omic] | [omic, path] | [radio, path,
 *   omic]; n_layers: the Highways' depth, 1..8; B rows; K logits (cox: 1); training != 0: batch statistics (B >= 2), running
 *   statistics updated in place with bn.momentum and the unbiased variance, dropout p_drop; training == 0: running statistics,
 *   no dropout.  h[0..2]: the radio, path and omic embeddings [B x 256].  The early types read the present ones and blk[0]
 *   (over the 256 m wide cat); the late types read ALL THREE and blk[0..2] = the radio, path and omic block: the forward
 *   evaluates the block of the modality the mode drops too, as the reference's does, so its running statistics move in
 *   train mode; it feeds nothing and its gradients are neither read nor written.  Blocks as mmf_stage2_block, with mutable
 *   running statistics.  Wk, bk: the classifier, [K x 128] early-fcnn, [K x 128 m] late-fcnn (cox: [1 x m] over the blocks'
 *   scalars), [K x 256 m] the highway types.
 *   Dropout draws the composable route's masks: the keep-hash of (seed, site, element b * F + f), F the BatchNorm's width:
 *   fcnn block i site i of seed (early: site 0); Highway i site 0 of seed + i (early: seed).  seed_dev: optional device word
 *   added to the seed, or NULL.
 * target: loss = MMF_STAGE2_LOSS_NLL (Y, c, alpha), _COX (times, c), _RANK (times, c, phi, reduction) or _RANK_NLL (ranking
 *   over the labels Y + nll_ratio x nll(alpha)); phi 0 = sigmoid, 1 = relu; reduction 0 = mean, 1 = sum; times: DEVICE float64
 *   [B]; Y: int64 [B]; c: float [B].  Ties, an all-censored Cox batch and a batch without a comparable pair (loss 0, every
 *   gradient 0) as in mmf_cox_surv / mmf_ranking_loss; nll_surv's eps is 1e-7.
 * Outputs: risk [B]; hazards, S [B x K] (nll family; not written for cox); loss [1], unscaled.  grads: the gradients of
 *   loss x loss_scale, written or (accumulate != 0) added; members mirror the blocks; NULL: forward and loss only.
 * Returns, before any launch and in this order:
 *   MMF_ERR_ARG for a null desc, target, Wk, bk, risk, loss or c; a family, train_type, loss, phi or reduction the header does
 *     not name; kronecker; nll or rank_nll on the cox family; p_drop outside [0, 1); a null h[i], weight, bias or BatchNorm
 *     array the type reads (the per-layer arrays' entries included); null hazards or S with the nll family; a null Y or
 *     times the loss reads; a null gradient of a parameter that takes part, when grads is given;
 *   MMF_ERR_SHAPE for fewer than two modalities, B outside 1..256, training with B = 1, K outside 1..32 (cox: K != 1), a
 *     highway type with n_layers outside 1..8, a ranking loss with B < 2;
 *   MMF_ERR_ALIGN for an h[i] the type reads, a Highway weight matrix or the workspace off 16 bytes (a null workspace is
 *     MMF_ERR_ARG, found here), times off 8 bytes;  MMF_ERR_WORKSPACE.
 * mmf_stage2_step_workspace_bytes (m: the number of modalities the mode keeps), with ldB = B rounded up to 4, nb = 1 (early)
 *   or 3 (late), every slot rounded up to 256 bytes, in floats: fcnn: nb slots of 128 ldB, one of 128 m' ldB (m' = 1 early, m
 *   late), nb of 256, one of 3 B; highway, D = 256 m (early) or 256 (late): per Highway (nb of them) n_layers + 1 slots of
 *   D ldB, n_layers of B D, 3 n_layers + 6 of D ldB, two of 2 D; one slot of 256 m ldB.  0 for what the call refuses by
 *   shape or for an unknown enum; monotone in B.
 * The ABI version is unchanged: the entry points are additive.
 * Out of scope: kronecker, `residual`, unimonal_pretrained, bf16 embeddings.
 * ------------------------------------------------------------------------------------------- */
#define MMF_STAGE2_LOSS_NLL 0
#define MMF_STAGE2_LOSS_COX 1
#define MMF_STAGE2_LOSS_RANK 2
#define MMF_STAGE2_LOSS_RANK_NLL 3
typedef struct mmf_stage2_bn_train {  /* nn.BatchNorm1d whose running statistics a training step moves */
  const float* weight;               /* [F] */
  const float* bias;                 /* [F] */
  float* running_mean;               /* [F] */
  float* running_var;                /* [F] */
  float eps;                         /* 1e-5 */
  float momentum;                    /* 0.1 */
} mmf_stage2_bn_train;
typedef struct mmf_stage2_step_block {
  const float* W0;                   /* fcnn: [128 x Kin] */
  const float* b0;                   /* [128] */
  mmf_stage2_bn_train bn;            /* fcnn: BatchNorm1d(128) */
  const float* W4;                   /* cox late-fcnn: [1 x 128] */
  const float* b4;                   /* [1] */
  mmf_stage2_bn_train bn1, bn2;      /* highway: [Kin] each */
  const float* const* Wgate;         /* highway: HOST [n_layers] device pointers, [Kin x Kin] */
  const float* const* bgate;         /* HOST [n_layers], [Kin] */
  const float* const* Wnl;
  const float* const* bnl;
  const float* const* Wlin;
  const float* const* blin;
} mmf_stage2_step_block;
typedef struct mmf_stage2_step_desc {
  int32_t family, train_type;
  int32_t radio, path, omic;         /* != 0: the mode keeps the modality */
  int32_t n_layers;
  int32_t B, K, training;
  const float* h[3];                 /* [B x 256]: radio, path, omic */
  mmf_stage2_step_block blk[3];
  const float* Wk;
  const float* bk;
  float p_drop;                      /* 0.7 */
  uint32_t seed;
  const uint32_t* seed_dev;          /* optional device word added to the seed, or NULL */
  struct mmf_trace* trace;           /* optional kernel trace, or NULL */
} mmf_stage2_step_desc;
typedef struct mmf_stage2_target {
  int32_t loss;                      /* MMF_STAGE2_LOSS_* */
  const int64_t* Y;                  /* [B] bin labels (nll, rank_nll) */
  const float* c;                    /* [B] censorship */
  const double* times;               /* [B] event times (cox, rank) */
  float alpha, nll_ratio;
  int32_t phi, reduction;
  float loss_scale;
} mmf_stage2_target;
typedef struct mmf_stage2_block_grads {
  float *dW0, *db0, *dbn_weight, *dbn_bias, *dW4, *db4;
  float *dbn1_weight, *dbn1_bias, *dbn2_weight, *dbn2_bias;
  float* const* dWgate;              /* HOST [n_layers] device pointers, as the block's */
  float* const* dbgate;
  float* const* dWnl;
  float* const* dbnl;
  float* const* dWlin;
  float* const* dblin;
} mmf_stage2_block_grads;
typedef struct mmf_stage2_step_grads {
  mmf_stage2_block_grads blk[3];
  float* dWk;
  float* dbk;
} mmf_stage2_step_grads;
size_t mmf_stage2_step_workspace_bytes(int32_t family, int32_t train_type, int32_t m, int32_t n_layers, int32_t B, int32_t K,
                                       int32_t training);
int mmf_stage2_step(const mmf_stage2_step_desc* desc, const mmf_stage2_target* target, void* workspace,
                    size_t workspace_bytes, float* risk, float* hazards, float* S, float* loss,
                    const mmf_stage2_step_grads* grads, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Forward-only variants for the inference consumers of the path -- embedding export
 * (pre_trained_feature.py:116-162: model(..., return_features=True) under no_grad), per-patient inference and
 * attention heat-map scoring (utils/heatmap_utils.py:111-150,249-275: A_raw per bag / per 512-patch batch).
 * Same results as mmf_amil[_bf16]_forward, but nothing is saved for a backward: the a / b activations are never
 * written and the workspace is the small one returned here.  desc->p_h / p_att should be 0 (eval mode).
 * ------------------------------------------------------------------------------------------- */
size_t mmf_amil_infer_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated);
int mmf_amil_infer(const mmf_amil_desc* desc, const float* x, void* workspace, size_t workspace_bytes,
                   float* M, float* A_raw, void* stream);
size_t mmf_amil_bf16_infer_workspace_bytes(int64_t N, int32_t L, int32_t H, int32_t D, int32_t gated);
int mmf_amil_bf16_infer(const mmf_amil_desc* desc, const uint16_t* x, void* workspace, size_t workspace_bytes,
                        float* M, float* A_raw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The attention scorer on its own: Attn_Net(L, D).forward(x) / Attn_Net_Gated(L, D).forward(x) -> (A, x)
 *   (models/model_modules.py:84-85 and :105-110; n_classes = 1):  A[i] = (tanh(x_i Wa^T + ba) [. sigmoid(x_i Wb^T + bb)]) Wc^T + bc,
 *   with Dropout(0.25) on the branches when desc->p_att > 0.  Same kernels as inside the stack (K-gate, K-dh, K-tn).
 *   desc: N, H (= the scorer's input width L), D, gated, Wa..bc, p_att, seed[, seed_dev, trace]; L, W1, b1, p_h are ignored.
 *   H % 32 == 0, D % 32 == 0, and mmf_amil_desc::N's row cap without L: N * max(H, 2 * D) * 4 < 2^31, else
 *   MMF_ERR_SHAPE.  forward keeps a, b in the workspace for the matching backward.
 *   backward: gA [N] = dL/dA -> grads->dWa, dba, (dWb, dbb,) dWc, dbc and, when grads->dx != NULL, dx [N x H].
 * ------------------------------------------------------------------------------------------- */
size_t mmf_attn_net_workspace_bytes(int64_t N, int32_t H, int32_t D, int32_t gated);
int mmf_attn_net_forward(const mmf_amil_desc* desc, const float* x, void* workspace, size_t workspace_bytes, float* A,
                         void* stream);
int mmf_attn_net_backward(const mmf_amil_desc* desc, const float* x, void* workspace, size_t workspace_bytes,
                          const float* gA, const mmf_amil_grads* grads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense layer on MFMA:  y = dropout(act(concat_k(x_0..x_{nseg-1}) . W^T + bias))
 *   replaces torch.cat + nn.Linear of model_attention_mil_radio.py:80-82 (reduce_dim; the modality
 *   bags are never concatenated in memory) and the instance projections generally.
 *   x_segs: HOST array of nseg (<= 4) device pointers, each [M x kseg]; K = nseg*kseg; K % 32 == 0 (and kseg % 32 == 0
 *   when nseg > 1); N % 4 == 0 (the epilogue stores y and loads the bias four columns at a time): MMF_ERR_SHAPE
 *   otherwise, before any launch.  Every x segment, W, y and a non-null bias are 16-byte aligned: MMF_ERR_ALIGN otherwise.
 *   workspace / sync (both optional, may be NULL): scratch for the K-split plan of short grids (a 512-row radiology bag
 *   against the 4096-wide reduce_dim is 128 output tiles with a 128-chunk K loop each: split four ways -- one modality
 *   segment per workgroup -- it fills the chip) and the tick words it needs, under mmf_amil_desc::sync's contract.
 * ------------------------------------------------------------------------------------------- */
size_t mmf_linear_forward_workspace_bytes(int64_t M, int32_t N, int32_t nseg, int32_t kseg);   /* 0: the shape is not split */
int mmf_linear_forward(const float* const* x_segs, int32_t nseg, int32_t kseg, int64_t M,
                       const float* W, const float* bias, int32_t N, int32_t act,
                       float drop_p, uint32_t drop_seed, uint32_t drop_site, const uint32_t* seed_dev,
                       float* y, void* workspace, size_t workspace_bytes, uint32_t* sync, int32_t sync_words, void* stream);

size_t mmf_linear_backward_workspace_bytes(int64_t M, int32_t N, int32_t K);
/* dy [M x N] (gradient w.r.t. the pre-activation output) -> dW [N x K], db [N] (may be NULL),
 * dx [M x K] single buffer (may be NULL; only nseg == 1).  N % 4 == 0, kseg % 4 == 0, and N % 32 == 0 when dx is asked for:
 * MMF_ERR_SHAPE otherwise, before any launch (nothing is written). */
int mmf_linear_backward(const float* dy, const float* const* x_segs, int32_t nseg, int32_t kseg, int64_t M,
                        const float* W, int32_t N, float* dW, float* db, float* dx,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The input gradient of a linear layer over nseg (1..4) concatenated segments, which mmf_linear_backward leaves out because
 * training bags are leaves: dx_segs[i] [M x kseg] = dy [M x N] . W[:, i kseg : (i + 1) kseg], W [N x nseg kseg]; dx_segs is
 * a HOST array of device pointers.  One plain GEMM launch per segment.  Attribution by autograd needs it (one pass per
 * quadrature node through reduce_dim: infer.radio_integrated_gradients_autograd).  MMF_ERR_ARG for a null pointer or nseg
 * outside 1..4; MMF_ERR_SHAPE unless N % 32 == 0, kseg % 4 == 0, M >= 1 and every operand stays below 2 GiB;
 * MMF_ERR_ALIGN unless dy, W and every segment are 16-byte aligned; all before any launch. */
int mmf_linear_input_grad(const float* dy, const float* W, int32_t nseg, int32_t kseg, int64_t M, int32_t N,
                          float* const* dx_segs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Survival head:  logits = f.Wk^T + bk; hazards = sigmoid(logits); S = cumprod(1-hazards); Y_hat = argmax
 *   replaces models/model_attention_mil_path.py:58-61.
 * One workgroup keeps the B x K logits in LDS: B * K <= 256 (hence B <= 256), any F >= 1; a larger batch is
 * MMF_ERR_SHAPE, before any launch (nothing is written).  B < 1 or K < 1: MMF_ERR_ARG.
 * The backward reads the forward's hazards; g_hazards / g_S are the loss's gradients (mmf_nll_surv writes both).
 * ------------------------------------------------------------------------------------------- */
int mmf_surv_head_forward(const float* feat, const float* Wk, const float* bk, int32_t B, int32_t F, int32_t K,
                          float* logits, float* hazards, float* S, int64_t* Y_hat, void* stream);
int mmf_surv_head_backward(const float* g_hazards, const float* g_S, const float* hazards, const float* feat,
                           const float* Wk, int32_t B, int32_t F, int32_t K,
                           float* dfeat, float* dWk, float* dbk, void* stream);

/* nll_surv loss (utils/loss_utils.py:22-39): loss [1], and its gradients g_hazards, g_S [B x K].
 * A label outside [0, K) (the reference's gather raises an index error) poisons the result instead of the memory:
 * loss = NaN, that sample's gradients = 0; nothing is read or written out of bounds.
 * One workgroup strides over the samples: any B >= 1, K >= 1 (MMF_ERR_ARG below that). */
int mmf_nll_surv(const float* hazards, const float* S, const int64_t* Y, const float* c, int32_t B, int32_t K,
                 float alpha, float eps, float* loss, float* g_hazards, float* g_S, void* stream);

/* Cox partial-likelihood loss (utils/loss_utils.py:124-139): loss [1], d_risks [B].  times is float64.
 * One workgroup keeps exp(risk) and the risk-set weights of the whole batch in LDS (8 bytes a sample): B <= 8192,
 * MMF_ERR_SHAPE above, before any launch (nothing is written).  B < 1: MMF_ERR_ARG. */
int mmf_cox_surv(const float* risks, const double* times, const float* c, int32_t B,
                 float* loss, float* d_risks, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Small dense layers (any B, K, N >= 1; sized for batches of a few hundred rows at most) and the Kronecker fusion block.
 *   replaces SNN_Block (models/model_modules.py:64-68: Linear+SELU+AlphaDropout), the Linear+ReLU+Dropout
 *   stacks and gating of XlinearFusion (models/model_modules.py:133-178), and the fusion classifiers
 *   (models/model_mm_attention_mil.py:91,95).
 *   drop_kind: 0 none, 1 nn.Dropout, 2 nn.AlphaDropout; the mask is the keep-hash of (seed, site, element).
 *   seed_dev (everywhere below): optional device word added to `seed`, or NULL -- see mmf_amil_desc.
 * mmf_dense_forward / _rows: y = drop(act(x W^T + bias)), x [B x K], W [N x K], bias [N] or NULL (no bias), y [B x N].  Any
 *   B, K, N >= 1; no alignment requirement.  act in MMF_ACT_NONE..MMF_ACT_SELU, drop_kind in 0..2, 0 <= drop_p < 1,
 *   non-null x, W, y (and row_base): MMF_ERR_ARG otherwise.  mmf_dense_forward draws the mask of element (b, n) at the
 *   32-bit index b * N + n: with dropout on (drop_kind != 0, drop_p > 0) B * N >= 2^32 is MMF_ERR_SHAPE.  The _rows form
 *   draws at row_base[b] + n and has no such limit; ldy < N there: MMF_ERR_SHAPE.  Every refusal returns before any launch.
 * ------------------------------------------------------------------------------------------- */
int mmf_dense_forward(const float* x, const float* W, const float* bias, int32_t B, int32_t K, int32_t N,
                      int32_t act, int32_t drop_kind, float drop_p, uint32_t seed, uint32_t site,
                      const uint32_t* seed_dev, float* y, void* stream);
/* dy, y (the forward OUTPUT) -> dx [B x K] (may be NULL), dW [N x K], db [N] (may be NULL);
 * dpre_scratch: [B x N] floats.  No cap on B, K or N: with N <= 2048 and B <= 256 the backward is one launch that rebuilds
 * dpre in LDS and leaves dpre_scratch untouched; above either it is three launches through dpre_scratch.  act outside
 * MMF_ACT_NONE..MMF_ACT_SELU or drop_kind outside 0..2: MMF_ERR_ARG; the _rows forms with ldy < N or lddy < N: MMF_ERR_SHAPE. */
int mmf_dense_backward(const float* dy, const float* y, const float* x, const float* W,
                       int32_t B, int32_t K, int32_t N, int32_t act,
                       int32_t drop_kind, float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev,
                       float* dpre_scratch, float* dx, float* dW, float* db, void* stream);
/* The dense pair on a batch whose rows are the patients of one accumulation window (the omic branch of the grouped
 * multimodal step: models/model_mm_attention_mil.py:164-165 once per patient becomes one B = G batch): row b draws the
 * mask of ITS OWN seed.  row_base: DEVICE [B], row_base[b] = mmf_dropout_row_base(seed_b) (host helper: seed_b times the
 * inverse of the hash multiplier mod 2^32); element (b, n) then gets the mask mmf_dense_forward draws for a one-row call
 * with seed_b at index n -- nn.Dropout and nn.AlphaDropout forms alike.  y (and dy) may be columns of a wider matrix:
 * ldy / lddy >= N floats between rows.  Otherwise as mmf_dense_forward / mmf_dense_backward (dW, db: sums over the rows). */
uint32_t mmf_dropout_row_base(uint32_t seed);
int mmf_dense_forward_rows(const float* x, const float* W, const float* bias, int32_t B, int32_t K, int32_t N,
                           int32_t act, int32_t drop_kind, float drop_p, uint32_t site, const uint32_t* seed_dev,
                           const uint32_t* row_base, float* y, int32_t ldy, void* stream);
int mmf_dense_backward_rows(const float* dy, int32_t lddy, const float* y, int32_t ldy, const float* x, const float* W,
                            int32_t B, int32_t K, int32_t N, int32_t act, int32_t drop_kind, float drop_p, uint32_t site,
                            const uint32_t* seed_dev, const uint32_t* row_base, float* dpre_scratch, float* dx, float* dW,
                            float* db, void* stream);
/* o = sigmoid(z) * h (n elements) and its backward (dz, dh from g, z, h).  Any n >= 1; n < 1 or a NULL pointer: MMF_ERR_ARG. */
int mmf_gate_mul_forward(const float* z, const float* h, float* o, int32_t n, void* stream);
int mmf_gate_mul_backward(const float* g, const float* z, const float* h, float* dz, float* dh, int32_t n, void* stream);
/* out[b] = [o0,1] (x) [o1,1] ((x) [o2,1]) followed by Dropout(drop_p); o_t: [B x dim]; m = 2 or 3 (HOST array of ptrs).
 * out and g: [B x S^m], S = dim + 1.  m outside {2, 3}, dim < 1, B < 1 or a NULL pointer (o_t, d_o[t] for t < m included):
 * MMF_ERR_ARG.  An element is indexed, and its mask drawn, at the 32-bit b * S^m + e, and B is a grid dimension:
 * B * S^m < 2^31 and B <= 65535, MMF_ERR_SHAPE otherwise -- both entry points, before any launch. */
int mmf_kron_forward(const float* const* o, int32_t m, int32_t dim, int32_t B,
                     float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev, float* out, void* stream);
int mmf_kron_backward(const float* g, const float* const* o, int32_t m, int32_t dim, int32_t B,
                      float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev, float* const* d_o,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-step tail on flat fp32 buffers: the gradient of l1_reg_all + torch.optim.Adam(weight_decay) in one launch.
 *   replaces utils/utils.py:249-257 (l1_reg_all, through autograd) + utils/utils.py:144-146 (Adam) as used by
 *   utils/core_utils.py:216-219,242-247.  l1_coeff = lambda_reg x (micro-batches accumulated since the last step);
 *   step = 1-based optimizer step count.  w, m, v are updated in place.
 *   l1_mask: NULL = the L1 term covers every element (l1_reg_all); else [n] floats in {0, 1} selecting the elements it
 *   covers (l1_reg_modules, utils/utils.py:259-268: fc_omic and mm only).
 * mmf_abs_sum: out[0] = sum_i |w_i| (the value of l1_reg_all); partials = 512 floats of scratch.
 * Any n >= 1 (a tail of n % 4 elements is updated one by one); n < 1 or step < 1: MMF_ERR_ARG.  w, g, m, v and a non-null
 * l1_mask must be 16-byte aligned: MMF_ERR_ALIGN otherwise.  An element with w = +-0 gets no L1 term (sign(0) = 0).
 * ------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------
 * Omic head, ONE training step in ONE launch:  MaxNet forward (two SNN blocks + classifier -> risk), CoxSurvLoss, and
 * every parameter gradient.
 *   replaces models/model_genomic.py:53-72 (MaxNet.forward, bag_loss = cox_surv), models/model_modules.py:64-68 (SNN_Block:
 *   Linear + SELU + AlphaDropout), utils/loss_utils.py:124-139 (CoxSurvLoss) and the backward autograd derives from them --
 *   ~20 framework launches in the reference, 9 through the composable entry points above (mmf_dense_*, mmf_cox_surv).
 *   `small` net only (H0 = H1 = 256), any 1 <= B <= 256 and any 1 <= G <= 256; other shapes: MMF_ERR_SHAPE (use the
 *   composable entry points).  W1 and the workspace are read and written 16 bytes at a time and must be 16-byte aligned,
 *   times 8-byte aligned: MMF_ERR_ALIGN otherwise.  Every other pointer is read or written one float at a time; W0 too may sit on any
 *   4-byte boundary: with G <= 64, G % 4 == 0 and a
 *   16-byte aligned W0 the first layer keeps each row of W0 in registers (16-byte loads); any other G or a W0 off a 16-byte
 *   boundary takes the chunked route through LDS -- the same sums in another order.  A batch with every sample censored
 *   gives loss 0 and every gradient 0.  p_drop outside [0, 1), sync_words < 3 or a NULL pointer: MMF_ERR_ARG; a workspace
 *   smaller than mmf_maxnet_cox_step_workspace_bytes(B): MMF_ERR_WORKSPACE; all before any launch.
 *   times: DEVICE float64 [B] (the reference compares event times in float64); loss: unscaled; gradients are those of
 *   loss * loss_scale, written or (accumulate) added.  Needs 3 tick words (mmf_amil_desc::sync's contract).
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_maxnet_desc {
  int32_t B, G, H0, H1;      /* batch, input genes, hidden widths */
  const float* x;            /* [B x G] */
  const float* W0;           /* [H0 x G]  fc_omic.0.0.weight */
  const float* b0;           /* [H0] */
  const float* W1;           /* [H1 x H0] fc_omic.1.0.weight */
  const float* b1;           /* [H1] */
  const float* Wc;           /* [1 x H1]  classifier.weight */
  const float* bc;           /* [1] */
  float p_drop;              /* AlphaDropout probability of both blocks (0.25 in train mode, 0 in eval) */
  uint32_t seed;             /* dropout seed: block i draws with site i, element index b * 256 + n (as mmf_dense_forward) */
  const uint32_t* seed_dev;  /* optional device word added to the seed (graph replays), or NULL */
  uint32_t* sync;            /* tick words, >= 3 */
  int32_t sync_words;
  struct mmf_trace* trace;
} mmf_maxnet_desc;
typedef struct mmf_maxnet_grads { float *dW0, *db0, *dW1, *db1, *dWc, *dbc; } mmf_maxnet_grads;
size_t mmf_maxnet_cox_step_workspace_bytes(int32_t B);
int mmf_maxnet_cox_step(const mmf_maxnet_desc* desc, const double* times, const float* c, float loss_scale,
                        void* workspace, size_t workspace_bytes, float* risk, float* loss,
                        const mmf_maxnet_grads* grads, int32_t accumulate, void* stream);

int mmf_adam_l1_step(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float l1_coeff, const float* l1_mask, int32_t step, void* stream);
int mmf_abs_sum(const float* w, int64_t n, float* partials, float* out, void* stream);

/* Fused per-modality gating stage of XlinearFusion (models/model_modules.py:158-165), all m <= 3 modalities in ONE
 * single-workgroup launch:  h_i = relu(Wh_i v_i + bh_i); z_i = Wz_i [v_0|..|v_{m-1}] + bz_i;
 * gm_i = sigmoid(z_i) * h_i;  o_i = Dropout(relu(Wo_i gm_i + bo_i))  (dropout site i of `seed`).
 * forward writes h, z, gm, o ([B x sdim] each); backward reads them plus d_o and writes dv (incl. the v_cat path) and
 * every weight gradient.  All arrays are indexed by modality; entries >= m are ignored.  B * m * sdim <= 384
 * (MMF_ERR_SHAPE above: the stage's values live in LDS); m outside 1..3, B, dim or sdim < 1, drop_p outside [0, 1) or a
 * NULL member of a modality < m (h, z, gm, o in both directions; d_o, dv and the weight gradients in the backward):
 * MMF_ERR_ARG.  The forward reads v_i, Wh_i and Wz_i with 16-byte loads: dim % 4 == 0 (MMF_ERR_SHAPE otherwise) and
 * 16-byte aligned v_i, Wh_i, Wz_i (MMF_ERR_ALIGN otherwise).  The backward reads one float at a time and takes any dim
 * and any 4-byte aligned pointer.  Every refusal returns before any launch. */
typedef struct mmf_xreduce_io {
  int32_t m, B, dim, sdim;
  const float* v[3];
  const float* Wh[3]; const float* bh[3];
  const float* Wz[3]; const float* bz[3];
  const float* Wo[3]; const float* bo[3];
  float* h[3]; float* z[3]; float* gm[3]; float* o[3];
  const float* d_o[3];
  float* dv[3];
  float* dWh[3]; float* dbh[3]; float* dWz[3]; float* dbz[3]; float* dWo[3]; float* dbo[3];
} mmf_xreduce_io;
int mmf_xreduce_forward(const mmf_xreduce_io* io, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
int mmf_xreduce_backward(const mmf_xreduce_io* io, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stage-2 building blocks: the embedding-level fusion models trained on the exported [B x 256] features
 * (models/nll_models_pretrained.py:13-197, models/coxranking_models_pretrained.py:14-200) and their batched losses.
 * ------------------------------------------------------------------------------------------- */
/* y = dropout(act(BatchNorm1d(x) [+ res])), x / y / res: [B x F].  training != 0: batch statistics (biased variance),
 * running_mean / running_var updated in place with `momentum` and the unbiased variance (torch semantics; B >= 2);
 * training == 0: running statistics (required then: MMF_ERR_ARG without them; any B >= 1).  Training with B = 1 is
 * MMF_ERR_SHAPE, before any launch.  res, gamma / beta, and in training mode the running statistics may be NULL; so may
 * dres and dgamma / dbeta of the backward, which takes the same `training` flag (eval mode: dx = gamma * invstd * dpre).
 * Any F >= 1.  save_mean / save_invstd [F] are what backward reads.
 * Replaces nn.BatchNorm1d (+ the ReLU / Dropout / residual add that follow it) in models/model_modules.py:5-49 and
 * models/nll_models_pretrained.py:82-90. */
int mmf_batchnorm_forward(const float* x, const float* res, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int32_t B, int32_t F, int32_t training,
                          float eps, float momentum, int32_t act, float drop_p, uint32_t seed, uint32_t site,
                          const uint32_t* seed_dev, float* y, float* save_mean, float* save_invstd, void* stream);
int mmf_batchnorm_backward(const float* dy, const float* y, const float* x, const float* gamma,
                           const float* save_mean, const float* save_invstd, int32_t B, int32_t F, int32_t training,
                           int32_t act, float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_dev,
                           float* dx, float* dres /* or NULL */, float* dgamma, float* dbeta, void* stream);
/* Highway mix, models/model_modules.py:21-25: y = sigmoid(zg) * relu(zn) + (1 - sigmoid(zg)) * zl, elementwise over any
 * n >= 1 (MMF_ERR_ARG below).  The derivative of relu at zn = 0 is 0. */
int mmf_highway_mix_forward(const float* zg, const float* zn, const float* zl, int64_t n, float* y, void* stream);
int mmf_highway_mix_backward(const float* dy, const float* zg, const float* zn, const float* zl, int64_t n,
                             float* dzg, float* dzn, float* dzl, void* stream);
/* ranking_loss, utils/loss_utils.py:58-101 (a Python loop over all pairs): loss = -(mean | sum) over comparable pairs of
 * phi(risk_more - risk_less); phi 0 = sigmoid, 1 = relu; reduction 0 = mean, 1 = sum; 0 when no pair is comparable.
 * times: device double[B] (event times, or the bin labels for RankingNLLSurvLoss, loss_utils.py:160).  Writes the loss
 * and its gradient w.r.t. risks.  B >= 2 (B < 2: MMF_ERR_SHAPE, before any launch; the reference raises); no upper cap: one
 * workgroup strides over the samples.  phi or reduction outside 0..1: MMF_ERR_ARG. */
int mmf_ranking_loss(const float* risks, const double* times, const float* c, int32_t B, int32_t phi, int32_t reduction,
                     float* loss, float* d_risks, void* stream);
/* logits [B x K] -> hazards = sigmoid, S = cumprod(1 - hazards), Y_hat = argmax, risk = -sum_k S
 * (models/nll_models_pretrained.py:58-62,193-197).  Any B >= 1; 1 <= K <= 32 (the backward keeps a sample's hazards in
 * registers): MMF_ERR_SHAPE outside, before any launch.  Y_hat and risk may be NULL. */
int mmf_hazards_forward(const float* logits, int32_t B, int32_t K, float* hazards, float* S, int64_t* Y_hat, float* risk,
                        void* stream);
int mmf_hazards_backward(const float* g_hazards, const float* g_S, const float* g_risk /* each may be NULL */,
                         const float* hazards, int32_t B, int32_t K, float* dlogits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bag feed: a grouped window out of bags that stay resident in HBM across epochs (feed.ResidentBagCache).
 * ------------------------------------------------------------------------------------------- */
/* Rows of G bags, each contiguous somewhere in HBM, into rows offsets[g] .. offsets[g+1]-1 of one [offsets[G] x L]
 * matrix per plane (a pathology window: 1 plane; a radio window: one per modality), in ONE launch.
 * Storage types: src_bf16 / dst_bf16 != 0 say bf16, else fp32, for every source / every destination.  fp32 -> fp32 and
 * bf16 -> bf16 copy bit for bit; bf16 -> fp32 widens exactly; fp32 -> bf16 rounds to nearest even (the bits of torch's
 * tensor.to(torch.bfloat16) for every finite value, +-0, +-inf and denormals; a NaN stays a NaN, its payload does not).
 * Refused before any launch, nothing written: MMF_ERR_SHAPE for G outside 1..MMF_GROUP_MAX, nplane outside 1..4, an empty
 * bag or offsets not strictly increasing from 0, L % 8 != 0 (the unit of work is 16 bytes of the narrower type);
 * MMF_ERR_ARG for a null pointer (offsets, src, dst, or any entry of src / dst); MMF_ERR_ALIGN for a source or a
 * destination that is not 16-byte aligned.
 * Rows of a destination beyond offsets[G] are not touched.  Whether a source overlaps a destination is the caller's
 * business: the result is then unspecified.  The call keeps no state, allocates nothing and copies no table to the
 * device (the pointer and offset tables travel in the kernel arguments); no workgroup waits for another and there are no
 * atomics, so the result is deterministic.  Byte offsets are 64-bit: sources and destinations may lie anywhere. */
int mmf_bag_gather(const int64_t* offsets /* HOST [G+1] */, int32_t G, int32_t nplane /* 1..4 */,
                   const void* const* src /* HOST [nplane*G] device pointers, plane-major */,
                   void* const* dst /* HOST [nplane] device pointers, row pitch L */,
                   int32_t L, int32_t src_bf16, int32_t dst_bf16, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel trace: per-kernel device time of the attention-stack entry points, from HIP events recorded on the LAUNCH
 * stream around every kernel of a call whose desc->trace is set (bench.py's roofline leg).  A trace is a caller-owned
 * object (create / destroy); calls that carry the same trace must not run concurrently.  capacity = kernel launches
 * it can hold; further launches go unrecorded.  mmf_trace_dump synchronises on the recorded events, writes
 * "kernel_name launches total_ms" lines into buf, clears the records and returns the number of bytes written
 * (or needed when buf == NULL).
 * ------------------------------------------------------------------------------------------- */
typedef struct mmf_trace mmf_trace;
mmf_trace* mmf_trace_create(int32_t capacity);
void mmf_trace_destroy(mmf_trace* trace);
int mmf_trace_dump(mmf_trace* trace, char* buf, size_t buf_bytes);

/* Host-side restatement of the device dropout keep-hash (1 = kept).  For tests / mask inspection only. */
int mmf_dropout_keep_host(uint32_t seed, uint32_t site, uint32_t index, float p);

#ifdef __cplusplus
}
#endif
#endif /* MMF_AMIL_H */
