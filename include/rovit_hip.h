/* rovit_hip.h -- C ABI of librovit_hip.so: the MI355X (gfx950) kernels behind the RoViT-KAN hot path.
 *
 * The reference (nishitbohra/RoViT-KAN-...) has no native / FFI layer: its hot path is the Python nn.Module
 * surface of models/rovit_kan.py, models/backbone.py, models/kan.py and models/heads.py.  This header is the
 * boundary a maintainer would bind from those files (via ctypes); every entry point cites
 * the reference code it replaces.
 *
 * Conventions
 *   - plain C types only; all pointers are DEVICE pointers unless stated, owned by the caller;
 *   - "bf16" buffers are passed as void* (16-bit brain-float, row-major, 16-byte aligned, leading dimension in
 *     elements); float buffers are fp32 row-major;
 *   - every function only ENQUEUES work on `stream` (a hipStream_t); it never allocates, never synchronises;
 *   - return value: ROVIT_OK (0) or a negative error code; rovit_last_error_string() describes the failure
 *     (thread-local).  There is no CPU fallback: without a GPU the launch fails and the code says so.
 */
#ifndef ROVIT_HIP_H
#define ROVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rovit_stream_t; /* hipStream_t */

enum {
  ROVIT_OK = 0,
  ROVIT_ERR_SHAPE = -1,  /* unsupported / inconsistent shape */
  ROVIT_ERR_ALIGN = -2,  /* pointer or leading dimension not aligned */
  ROVIT_ERR_NULL = -3,   /* required pointer is NULL */
  ROVIT_ERR_LAUNCH = -4  /* HIP reported a launch / memset error */
};

/* activation applied to a KAN layer's output (models/kan.py:141 ReLU between layers, :147 3*sigmoid) */
enum { ROVIT_ACT_NONE = 0, ROVIT_ACT_RELU = 1, ROVIT_ACT_SIGMOID3 = 2 };
/* flags of rovit_linear_fwd */
enum { ROVIT_LIN_RELU = 1, ROVIT_LIN_CLAMP10 = 2 };
/* epilogues of rovit_gemm_nt */
enum { ROVIT_EPI_BF16 = 0, ROVIT_EPI_GELU = 1, ROVIT_EPI_RESID = 2, ROVIT_EPI_MUL = 3, ROVIT_EPI_PATCH = 4 };
/* OR-ed into rovit_gemm_nt's `epi`: run the LDS-tiled kernel (128 x 192 / 128 x 96 tiles; the path of shapes the weight-stationary
 * kernels do not cover) even where a weight-stationary kernel applies -- per call, for tests of that path */
enum { ROVIT_GEMM_TILED_192 = 0x100, ROVIT_GEMM_TILED_96 = 0x200 };

int rovit_version(void);
const char* rovit_last_error_string(void);

/* ------------------------------------------------------------------------------------------------------------
 * KAN head.  Replaces KANLayer.forward (models/kan.py:70-95) incl. BSplineBasis.compute_basis (:8-44) and the
 * activation that follows the layer in KANSeverityModule.forward (:138-149); backward replaces autograd of same.
 *   x (B,in)  spline_w (in,out,nb)  knots (n_knots,) with nb = n_knots-4 (degree 3)  lin_w (out,in)  lin_b (out)
 *   out (B,out) = act(Linear(x) + sum_i sum_k basis_k(tanh x_i) spline_w[i,:,k])
 * ------------------------------------------------------------------------------------------------------------ */
/* BSplineBasis.compute_basis (models/kan.py:8-44) for degree 3: x_norm (n,) -> basis (n, n_knots-4) */
int rovit_kan_basis(const float* x_norm, const float* knots, float* basis, int n, int n_knots, rovit_stream_t stream);
int rovit_kan_layer_fwd(const float* x, const float* spline_w, const float* knots, const float* lin_w, const float* lin_b,
                        float* out, int batch, int in_f, int out_f, int n_knots, int act, rovit_stream_t stream);
/* out = the forward's post-activation output; dx may be NULL; d_spline_w/d_lin_w/d_lin_b NULL together */
int rovit_kan_layer_bwd(const float* x, const float* spline_w, const float* knots, const float* lin_w, const float* out,
                        const float* grad_out, float* dx, float* d_spline_w, float* d_lin_w, float* d_lin_b, int batch,
                        int in_f, int out_f, int n_knots, int act, int accumulate_dx, rovit_stream_t stream);
/* Backward of the whole KANSeverityModule stack in two launches (autograd of models/kan.py:138-149): the per-sample chain
 * dL/dz_n -> dx_n -> ... -> dx_1 in one launch (writes dL/dz of every layer into gz[l] (batch, out_l) and dx), then the
 * parameter gradients of ALL layers in one launch.  Host arrays of n_layers device pointers; grad_outs[l] = gradient w.r.t.
 * layer l's output from outside the stack (NULL entries allowed, the last must be set); d_spline_w NULL = no parameter
 * gradients; dx NULL = no input gradient.  Same arithmetic and summation order as rovit_kan_layer_bwd per layer. */
int rovit_kan_stack_bwd(const float* x, const float* const* spline_w, const float* const* knots, const float* const* lin_w,
                        const float* const* outs, const float* const* grad_outs, float* const* gz, float* dx, float* const* d_spline_w,
                        float* const* d_lin_w, float* const* d_lin_b, int batch, const int* dims, const int* n_knots, const int* acts,
                        int n_layers, rovit_stream_t stream);
/* Prepared weight layouts of one KAN layer for rovit_kan_stack_fwd (re-run whenever the parameters change):
 * spline_w (in, out, nb) -> spline_wt (in, nb, out); lin_w (out, in) -> lin_wt (in, out). */
int rovit_kan_prepare(const float* spline_w, const float* lin_w, float* spline_wt, float* lin_wt, int in_f, int out_f, int n_basis,
                      rovit_stream_t stream);
/* KANSeverityModule.forward (models/kan.py:138-149) in ONE launch: every layer with its activation; the activations
 * stay on the CU between layers.  spline_wt / knots / lin_wt / lin_b / outs are HOST arrays of n_layers device pointers
 * (spline_wt, lin_wt: the prepared layouts above), dims the n_layers + 1 widths (widths after the input <= 64), acts the
 * ROVIT_ACT_* after each layer.  outs[l] (batch, dims[l+1]) receives layer l's post-activation output: the last is the
 * module output, the others are what rovit_kan_layer_bwd and get_activation_trajectory (:154-167) need. */
int rovit_kan_stack_fwd(const float* x, const float* const* spline_wt, const float* const* knots, const float* const* lin_wt,
                        const float* const* lin_b, float* const* outs, int batch, const int* dims, const int* n_knots,
                        const int* acts, int n_layers, rovit_stream_t stream);
/* The same stack on the matrix cores for large batches (models/kan.py:70-95 as the dense contraction
 * sum_j sum_s R[b,j,s] Wd[j,s,o]: slots s = the num_basis truncated-basis values of tanh(x_j) followed by the raw x_j of
 * the layer's Linear term; v_mfma_f32_32x32x2_f32, fp32 operands and accumulation).  rovit_kan_mfma_prepared_floats gives
 * the size of one layer's prepared weight layout, or 0 when the kernel does not cover the layer (it covers in_f % 8 == 0,
 * out_f <= 64 and n_basis 7 or 34, i.e. num_knots 5 and 32 of the reference's configs); rovit_kan_prepare_mfma fills it
 * (re-run whenever the parameters change); wm / knots / lin_b / outs are HOST arrays of n_layers device pointers. */
size_t rovit_kan_mfma_prepared_floats(int in_f, int out_f, int n_basis);
int rovit_kan_prepare_mfma(const float* spline_w, const float* lin_w, float* wm, int in_f, int out_f, int n_basis, rovit_stream_t stream);
int rovit_kan_stack_fwd_mfma(const float* x, const float* const* wm, const float* const* knots, const float* const* lin_b,
                             float* const* outs, int batch, const int* dims, const int* n_knots, const int* acts, int n_layers,
                             rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * MLP heads.  rovit_linear_* are the building block (nn.Linear [+ReLU] [*dropout mask] [clamp +-10]);
 * rovit_heads_* run ClassificationHead / OrdinalHead / UncertaintyHead.forward (models/heads.py:17-22, 38-43,
 * 91-102) with the curriculum gate of RoViTKAN.forward (models/rovit_kan.py:93-116).
 * params[14] / grads[14] order: cls.fc1.{w,b} cls.fc2.{w,b} ord.fc1.{w,b} ord.fc2.{w,b} unc.fc1.{w,b}
 * unc.fc_mu.{w,b} unc.fc_logvar.{w,b}.  masks: HOST array of 3 device pointers (B,hid) holding the scaled
 * dropout keep-mask, or NULL / NULL entries in eval mode.  hidden: (3,B,hid) workspace kept for backward;
 * rovit_heads_bwd's scratch is (3,B,hid) as well.
 * ------------------------------------------------------------------------------------------------------------ */
int rovit_linear_fwd(const float* x, const float* w, const float* bias, const float* mask, float* y, int batch, int in_f,
                     int out_f, int flags, rovit_stream_t stream);
int rovit_linear_bwd(const float* x, const float* w, const float* grad_y, const float* y_clamped, const float* dx_mul,
                     const float* dx_pos, float* dx, float* dw, float* db, int batch, int in_f, int out_f, int accumulate_dx,
                     rovit_stream_t stream);
int rovit_heads_fwd(const float* features, const float* const* params, const float* const* masks, float* hidden,
                    float* cls_logits, float* ordinal_logits, float* mu, float* log_var, int batch, int embed, int hid,
                    int num_classes, int stage, rovit_stream_t stream);
int rovit_heads_bwd(const float* features, const float* const* params, const float* const* masks, const float* hidden,
                    const float* log_var, const float* g_cls, const float* g_ord, const float* g_mu, const float* g_lv,
                    float* d_features, float* const* grads, float* scratch, int batch, int embed, int hid, int num_classes,
                    int accumulate_dfeat, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Head phase in three launches (round 4): everything RoViTKAN.forward does with the backbone features --
 * the three heads (models/heads.py:17-22, 38-43, 91-102, gated by the curriculum stage, models/rovit_kan.py:93-116)
 * AND KANSeverityModule.forward (models/kan.py:138-149) -- as ONE forward launch, and its autograd backward as
 * two (the per-sample gradient chain down to d_features; then every parameter gradient).  One workgroup owns one
 * sample for the whole phase; parameters are read in the reference layouts (no prepared copies).
 *   Limits: embed <= 768 and a multiple of 4; hid <= 256 and a multiple of 4; num_classes <= 8; 1..4 KAN layers
 *   (kan_layers == 0: no KAN stack, stage < 4) whose widths after the input are <= 64; 8..64 knots per layer.
 *   Dropout on the hidden layers: masks[h] (B,hid) = scaled keep-mask, or -- masks[h] == NULL and drop_p > 0 -- drawn
 *   in the kernel (Philox4x32-10 keyed by `seed`, counter (sample * hid + unit, offset); kept units scaled by
 *   1 / (1 - drop_p)); the backward needs no mask then (a kept unit is one whose stored hidden value is > 0).
 *   Arrays in this struct are HOST arrays of device pointers; every pointer is a device pointer of fp32 data.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rovit_head_phase {
  int batch, embed, hid, num_classes, stage;
  int kan_layers;
  int kan_dims[5];
  int kan_knots[4];
  int kan_acts[4];                /* ROVIT_ACT_* after each layer */
  float drop_p;
  unsigned long long seed, offset;
  const float* features;          /* (B, embed) */
  const float* head_params[14];   /* order of rovit_heads_fwd */
  const float* masks[3];
  const float* kan_w[4];          /* (in, out, nb) */
  const float* kan_knots_p[4];
  const float* kan_lw[4];         /* (out, in) */
  const float* kan_lb[4];
  /* forward outputs, kept for the backward */
  float* hidden;                  /* (3, B, hid) post-ReLU / dropout */
  float* cls; float* ord; float* mu; float* lv;
  float* kan_out[4];              /* (B, kan_dims[l+1]) post-activation */
  /* backward inputs: gradients w.r.t. the outputs (NULL: none); g_kan is the last KAN layer's */
  const float* g_cls; const float* g_ord; const float* g_mu; const float* g_lv; const float* g_kan;
  /* backward outputs */
  float* d_features;              /* (B, embed) or NULL */
  float* dpre;                    /* (3, B, hid) scratch: gradient w.r.t. the heads' pre-activations */
  float* kan_gz[4];               /* (B, kan_dims[l+1]) scratch: gradient w.r.t. each layer's pre-activation */
  float* head_grads[14];          /* mirrors head_params; all NULL with want_param_grads == 0 */
  float* kan_dw[4]; float* kan_dlw[4]; float* kan_dlb[4];
  int want_param_grads;
} rovit_head_phase;
int rovit_head_phase_fwd(const rovit_head_phase* p, rovit_stream_t stream);
int rovit_head_phase_bwd(const rovit_head_phase* p, rovit_stream_t stream);
/* the parameter-gradient launch of rovit_head_phase_bwd alone (after a want_param_grads == 0 call; e.g. on another stream) */
int rovit_head_phase_bwd_params(const rovit_head_phase* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Monte-Carlo dropout over the heads in ONE launch (csrc/mc_dropout.hip): what the reference's recipe -- the
 * heads' nn.Dropout modules in training mode (experiments/baselines.py:48-52), T forwards -- gives, from the
 * backbone features of ONE forward (DeiT-Tiny has no dropout).  Per image: each active head's relu(fc1(x))
 * once; per sample t < num_samples the masks (Philox4x32-10, key = seed, counter (image * hid + unit, t,
 * offset lo, offset hi), words x / y / z -> heads 0 / 1 / 2, kept iff (word >> 8) * 2^-24 < 1 - drop_p, kept
 * units scaled by 1 / (1 - drop_p): sample 0 is rovit_head_phase_fwd's draw), the output linears (log_var
 * clamped to +-10), and the per-image statistics over the samples (variances divided by T).
 *   Limits: those of rovit_head_phase (embed <= 768, hid <= 256, both multiples of 4; 2 <= num_classes <= 8)
 *   and 1 <= num_samples <= 4096.  Outputs (fp32, device): class_probs / class_probs_std (B, C), pred_entropy /
 *   exp_entropy / mutual_info (B); stage >= 2: ord_probs (B, C), ord_severity / ord_severity_std (B); stage
 *   >= 3: unc_mu, epistemic_var (variance of mu), aleatoric_var (mean of exp(log_var)), unc_std (B).
 *   s_cls (T, B, C), s_ord (T, B, C - 1), s_mu / s_lv (T, B): optional per-sample outputs (NULL: not written).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rovit_head_mc {
  int batch, embed, hid, num_classes, stage, num_samples;
  float drop_p;
  unsigned long long seed, offset;
  const float* features;          /* (B, embed) */
  const float* head_params[14];   /* order of rovit_heads_fwd */
  float* class_probs; float* class_probs_std; float* pred_entropy; float* exp_entropy; float* mutual_info;
  float* ord_probs; float* ord_severity; float* ord_severity_std;
  float* unc_mu; float* epistemic_var; float* aleatoric_var; float* unc_std;
  float* s_cls; float* s_ord; float* s_mu; float* s_lv;
} rovit_head_mc;
int rovit_head_mc_fwd(const rovit_head_mc* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * DeiT-Tiny backbone (models/backbone.py:23-25 -> timm VisionTransformer.forward).
 * params / grads: HOST arrays of rovit_vit_num_params(depth) device pointers (fp32, timm layouts):
 *   [0] cls_token (192) [1] pos_embed (197,192) [2] patch_embed.proj.weight (192,768) [3] .bias [4] norm.weight
 *   [5] norm.bias, then per block b at 6+12b: norm1.{w,b} attn.qkv.{w,b} attn.proj.{w,b} norm2.{w,b} mlp.fc1.{w,b}
 *   mlp.fc2.{w,b}.
 * prep: rovit_vit_prep_bytes(depth) bytes, filled by rovit_vit_prepare (re-run after every parameter update).
 * workspace: rovit_vit_workspace_bytes(batch, depth, training) bytes; in training mode it carries the saved
 * activations from rovit_vit_forward to rovit_vit_backward.
 * ------------------------------------------------------------------------------------------------------------ */
int rovit_vit_num_params(int depth);
size_t rovit_vit_prep_bytes(int depth);
size_t rovit_vit_workspace_bytes(int batch, int depth, int training);
int rovit_vit_prepare(const float* const* params, void* prep, int depth, rovit_stream_t stream);
/* mlp_path: which kernels run the MLP half of every block -- an argument, not library state, because a training step's forward and
 * backward must agree on it (the one-launch kernels keep act / gelu' / dpre chunk-major, the two-launch kernels row-major): pass the SAME
 * value to rovit_vit_forward and to the rovit_vit_backward(_notify) calls that consume its workspace.  ROVIT_MLP_AUTO (what the module
 * passes) selects by size: one launch from 34 000 token rows (batch 173), the measured crossover; the other two values force a path
 * (parity tests run every batch size through both). */
enum { ROVIT_MLP_AUTO = 0, ROVIT_MLP_TWO_LAUNCH = 1, ROVIT_MLP_ONE_LAUNCH = 2 };
int rovit_vit_forward(const float* images, const float* const* params, const void* prep, void* workspace, float* features,
                      int batch, int depth, int training, int mlp_path, rovit_stream_t stream);
/* rovit_vit_prepare + rovit_vit_forward in one call (every training step re-prepares the weights): the per-block weight images are
 * written on the library's second stream beside the patch embedding, not in front of the forward (41 us per step at depth 12).
 * write_tables != 0 also writes prep's constant look-up tables: needed the first time a prep buffer is used. */
int rovit_vit_forward_prepare(const float* images, const float* const* params, void* prep, void* workspace, float* features, int batch,
                              int depth, int training, int mlp_path, int write_tables, rovit_stream_t stream);
/* forward + explainability taps: attn_taps is a HOST array of `depth` device pointers (bf16 (B*197,192)) that receive
 * each block's attention-module output -- what DeiTTinyBackbone.get_attention_maps collects through forward hooks on
 * `blocks[i].attn` (models/backbone.py:37-62).  prob_taps (optional, like attn_taps): fp32 (B,3,197,197) softmax
 * probabilities per block, what explainability/attention_maps.py:18-105 means to roll out.  Inference workspace. */
int rovit_vit_forward_taps(const float* images, const float* const* params, const void* prep, void* workspace, float* features,
                           void* const* attn_taps, float* const* prob_taps, int batch, int depth, rovit_stream_t stream);
/* forward + attention rollout (explainability/attention_maps.py:40-95, ViTAttentionRollout.generate): rollout fp32 (B,197)
 * receives row 0 of  A^_1 ... A^_depth,  A^_l = the block's head-fused softmax probabilities (head_fusion 0 mean, 1 max, 2 min)
 * plus the identity, rows renormalised.  Computed behind every block's attention; no probability matrix is stored.
 * Inference workspace; bf16 engine. */
int rovit_vit_forward_rollout(const float* images, const float* const* params, const void* prep, void* workspace, float* features,
                              float* rollout, int head_fusion, int batch, int depth, rovit_stream_t stream);
/* the reference's map from a rollout (attention_maps.py:96-103): rollout[:, 1:] as 14x14, bilinear (half-pixel centres, edges
 * clamped: cv2.resize INTER_LINEAR / F.interpolate align_corners=False) to 224x224, then (m - min) / (max - min + 1e-8) per
 * image.  map224 fp32 (B,224,224). */
int rovit_rollout_map(const float* rollout, float* map224, int batch, rovit_stream_t stream);
/* forward + per-head attention statistics (no counterpart in the reference; Dosovitskiy et al. 2021 fig. 11, Raghu et al. 2021).  For
 * image b, block l, head h with softmax probabilities P (197 x 197), class token 0, patch t >= 1 at (r, c) = divmod(t - 1, 14),
 * dist(i, j) = 16 sqrt((r_i - r_j)^2 + (c_i - c_j)^2) pixels and 0 ln 0 = 0, per query row i:
 *   H_i = -sum_j P_ij ln P_ij (nats);  D_i = sum_{j>=1} P_ij dist(i, j) / sum_{j>=1} P_ij for i >= 1 (0 for i = 0, and where the patches'
 *   mass is 0);  C_i = P_i0;  M_i = max_j P_ij.
 * summary fp32 (B, depth, 3, 8): [0] mean H_i over the 197 queries, [1] mean D_i over the 196 patch queries, [2] mean C_i over the patch
 * queries, [3] mean P_ii over the 197 queries, [4] H_0, [5] P_00, [6] mean M_i over the 197 queries, [7] mean over the patch queries of
 * sum P_ij over the patch keys j within Chebyshev grid distance 1 of i (self included, not renormalised).
 * cls_attention fp32 (B, depth, 3, 196): P_0j, j = 1..196.  per_token (NULL, or fp32 (B, depth, 3, 197, 4), 16-byte aligned): H, D, C, M of
 * every query row.  The probabilities are the bits rovit_attention_probs writes and are never stored; every sum has a fixed order (csrc/
 * head_stats.hip), so a call is bit-identical run to run at a given batch.  Inference workspace, bf16 engine, one stream, every query row
 * of the last block: `features` are the bits rovit_vit_forward_taps gives at the same batch. */
int rovit_vit_forward_head_stats(const float* images, const float* const* params, const void* prep, void* workspace, float* features,
                                 float* summary, float* cls_attention, float* per_token, int batch, int depth, rovit_stream_t stream);
/* one block's step of the above on its saved qkv (bf16 (B*197, 576), scale 1/8): writes slice `block` of summary, cls_attention and
 * per_token (NULL or as above).  partial: fp32 scratch of batch x 13 x 24 floats.  Two launches. */
int rovit_attention_head_stats_step(const void* qkv, float* summary, float* cls_attention, float* per_token, float* partial, int batch,
                                    int block, int depth, rovit_stream_t stream);
/* Data-set reduction of n recorded rows: summary fp32 (n, depth*heads*8), cls_attention fp32 (n, depth*heads*196), labels int32 (n) or
 * NULL with classes = 0.  block receives rovit_head_stats_block_words(depth, heads, classes) doubles: for group 0 (every row) and groups
 * 1 + c (rows labelled c; labels outside 0..classes-1 count in group 0 only), [count, mean (R), unbiased variance (R), mean cls_attention
 * (Q)] with R = depth*heads*8 and Q = depth*heads*196.  fp64, the rows walked in storage order; a group of no rows gives zeros, of one row
 * variance 0. */
size_t rovit_head_stats_block_words(int depth, int heads, int classes);
int rovit_head_stats_finalize(const float* summary, const float* cls_attention, const int* labels, double* block, int n, int depth,
                              int heads, int classes, rovit_stream_t stream);
/* Grad-CAM++ at blocks[depth-1].norm1 (explainability/gradcam.py:34-104, GradCAMPlusPlus.compute), batched, bf16 engine, eval
 * semantics (no dropout).  Workspace: rovit_vit_gradcam_workspace_bytes(batch, depth) bytes (the inference workspace plus the last
 * block's class-token backward temporaries; 0 for a bad batch / depth).  rovit_vit_forward_gradcam = the inference forward, keeping
 * what the last block's class-token backward reads. */
size_t rovit_vit_gradcam_workspace_bytes(int batch, int depth);
int rovit_vit_forward_gradcam(const float* images, const float* const* params, const void* prep, void* workspace, float* features,
                              int batch, int depth, rovit_stream_t stream);
/* ... then, on the same workspace and features: the classification head (head_w1 (hidden,192), head_b1, head_w2 (classes,hidden),
 * head_b2; fp32; hidden and classes in [1, 2048]) -> logits fp32 (B,classes); the target of image b is targets[b] (int32; NULL: the
 * first argmax of its logits), written to chosen (int32 (B), may be NULL); an out-of-range target gives a NaN cam for that image.
 * With a = the norm1 output and g = d logits[b, c_b] / d a: cam fp32 (B,196) = relu(w[n] * sum_d a[n,d]) for the 196 patch tokens,
 * w[n] = sum_d g^2 / (2 g^2 + sum_n' a g^3) * relu(g).  act / grad: fp32 (B,197,192) copies of a and g, each may be NULL.
 * Writes no parameter gradient and leaves the backward's stream state alone; may run more than once on one forward. */
int rovit_vit_gradcam(const float* const* params, const void* prep, void* workspace, const float* features, const float* head_w1,
                      const float* head_b1, const float* head_w2, const float* head_b2, int hidden, int classes, const int* targets,
                      float* logits, int* chosen, float* cam, float* act, float* grad, int batch, int depth, rovit_stream_t stream);
/* Grad-CAM++ of the severity and uncertainty outputs.  rovit_explain_seed: the targets' scalar per image and d target / d features,
 * from the backbone features and the heads / KAN parameters of a rovit_head_phase descriptor (batch, embed = 192, hid, num_classes,
 * stage, kan_*, features, head_params; the forward / backward buffers and the dropout fields are not read: eval semantics).  kinds:
 * HOST array of n_targets (1..4) distinct ROVIT_TARGET_* other than CLASS (whose seed is rovit_vit_gradcam's), each produced at the
 * descriptor's stage (ordinal_severity from 2, mu / log_var from 3, kan_severity at 4 with a one-output KAN stack).  Targets:
 *   ORDINAL_SEVERITY  sum_k k P(y = k) from the cumulative sigmoids (models/heads.py:45-77); gradient -sum_k sigma'(z_k) dz_k
 *   MU, LOG_VAR       the uncertainty head's mu, clamp(log_var, -10, 10) (gradient where -10 <= pre-clamp value <= 10)
 *   KAN_SEVERITY      KANSeverityModule's output (models/kan.py:138-149), gradient as rovit_head_phase_bwd computes it
 * values fp32 (n_targets, B), seeds fp32 (n_targets, B, 192).  Limits: those of rovit_head_phase.  fp32, no atomics, deterministic. */
enum { ROVIT_TARGET_CLASS = 0, ROVIT_TARGET_ORDINAL_SEVERITY = 1, ROVIT_TARGET_MU = 2, ROVIT_TARGET_LOG_VAR = 3, ROVIT_TARGET_KAN_SEVERITY = 4 };
int rovit_explain_seed(const rovit_head_phase* p, const int* kinds, int n_targets, float* values, float* seeds, rovit_stream_t stream);
/* rovit_vit_gradcam with the caller's d_features (B,192) fp32 (16-byte aligned; e.g. a target's rows of rovit_explain_seed's seeds)
 * instead of the classification head's seed: cam / act / grad as there.  Runs on the workspace of rovit_vit_forward_gradcam and may
 * run once per target on one forward; writes no parameter gradient. */
int rovit_vit_gradcam_seeded(const float* const* params, const void* prep, void* workspace, const float* d_features, float* cam, float* act,
                             float* grad, int batch, int depth, rovit_stream_t stream);
/* the reference's map from a raw cam (gradcam.py:89-101): bilinear 14x14 -> 224x224 as rovit_rollout_map, then (m - min) / (max - min)
 * when max > 0 -- no epsilon: an all-equal positive map gives 0/0 = NaN, as the reference's numpy division does -- else m unchanged.
 * map224 fp32 (B,224,224). */
int rovit_gradcam_map(const float* cam, float* map224, int batch, rovit_stream_t stream);
/* images: the batch the forward ran on (read by the patch-embedding weight gradient, which gathers its pixels from it:
 * there is no im2col buffer); may be NULL for ranges with last_block > 0. */
int rovit_vit_backward(const float* images, const float* d_features, const float* const* params, const void* prep, void* workspace,
                       float* const* grads, int batch, int depth, int first_block, int last_block, int mlp_path, rovit_stream_t stream);
/* fp32 reference-precision forward (inference only; parity / evaluation mode, not the fast path): the same arithmetic
 * with every operand, product and sum in fp32 -- the mode in which BASELINE.json's "logits/severity within 1e-3 (fp32),
 * class argmax bit-exact" is checked end to end.  params: the ORIGINAL fp32 parameters (no prepared weights);
 * workspace: rovit_vit_f32_workspace_bytes(batch) bytes.  From batch 192 up the call runs the batch as two half-batch
 * chains, one on `stream` and one on the library's side stream (forked from and joined back into `stream`: to the caller it
 * is one stream-ordered call); the result does not depend on the batch an image travels in. */
size_t rovit_vit_f32_workspace_bytes(int batch);
int rovit_vit_forward_f32(const float* images, const float* const* params, void* workspace, float* features, int batch, int depth,
                          rovit_stream_t stream);
/* Where an activation of the fp32 forward lives inside its workspace (rovit_vit_f32_workspace_bytes(batch)): byte offset in *offset,
 * extent in *bytes; host-only, no launch.  All fp32, row-major, M = batch * 197 token rows:
 *   X: (M,192) the residual stream;  QKV: (M,576);  ATTN_O: (M,192) the attention output before proj;  ACT: (M,768) gelu(fc1)
 * After rovit_vit_forward_f32(..., depth = d) they hold block d-1's values (X: the stream leaving it) for EVERY row, in the one-chain
 * and in the two-chain schedule alike (the chains write disjoint row ranges of the same buffers). */
enum { ROVIT_F32_WS_X = 0, ROVIT_F32_WS_QKV = 1, ROVIT_F32_WS_ATTN_O = 2, ROVIT_F32_WS_ACT = 3 };
int rovit_vit_f32_workspace_field(int batch, int field, size_t* offset, size_t* bytes);
/* Where a saved activation / backward temporary of block `block` lives inside a TRAINING workspace
 * (rovit_vit_workspace_bytes(batch, depth, 1)): byte offset in *offset, extent in *bytes.  This is what the
 * explainability taps read (reference explainability/gradcam.py:18-60 hooks blocks[-1].norm1 for activations and
 * gradients; attention_maps.py:24-32 hooks blocks[i].attn): the fused kernels' own buffers, no extra copy.
 *   XHAT1 / XHAT2: bf16 (M,192) normalised rows before the norm1 / norm2 affine; RSTD1 / RSTD2: fp32 (M)
 *   QKV: bf16 (M,576); ATTN_O: bf16 (M,192) attention output before proj; ACT: bf16 gelu(fc1), (M,768) row-major when the
 *   two-launch MLP half ran (mlp_path, see rovit_vit_forward), CHUNK-MAJOR [24][M][32] when the one-launch half did
 *   DACT: bf16 gelu'(fc1 pre-activation), the layout of ACT (chunk-major when the one-launch half ran)
 *   LSE: fp32 (batch,3,197) log-sum-exp of the scaled attention logits per (image, head, query), in log2 units
 *   XHAT_CLS: fp32 (batch,192) class-token rows before the final norm's affine; RSTD_CLS: fp32 (batch) (`block` is not used)
 * The backward's rotating buffers (block i uses x0[i % 3], x1[i & 1], dpre[i & 1], dqkv[i & 1]; they are reused two or three blocks
 * later): each field is valid right after rovit_vit_backward(first_block = last_block = block) has returned and before the next block's
 * range is issued:
 *   DX_IN:  bf16 (M,192) gradient w.r.t. the residual stream leaving `block` (what enters its backward)
 *   DPRE:   bf16 (M,768) gradient w.r.t. the fc1 pre-activation, the layout of ACT
 *   DX_MID: bf16 (M,192) gradient w.r.t. the stream between the attention half and the MLP half
 *   DO:     bf16 (M,192) gradient w.r.t. the attention output before proj
 *   DQKV:   bf16 (M,576) gradient w.r.t. the qkv output of `block` (valid until block-2 is processed)
 *   DX_OUT: bf16 (M,192) gradient w.r.t. the stream entering `block`; block 0's are the rows the patch-embedding, position and
 *           class-token gradients are built from (DX_OUT of block i is DX_IN of block i-1: the same buffer)
 * The last block (block = depth-1) runs everything behind its attention on the class-token rows alone: its ATTN_O, XHAT2, RSTD2, ACT
 * and DACT, its LSE (query 0 of every head) and its DX_IN, DPRE, DX_MID and DO are written on rows b*197 (b < batch) only; the other
 * rows of those buffers are never written and must not be read (ACT, DACT and DPRE are row-major there).  Its DQKV and DX_OUT hold
 * every row. */
enum { ROVIT_WS_XHAT1 = 0, ROVIT_WS_RSTD1 = 1, ROVIT_WS_QKV = 2, ROVIT_WS_ATTN_O = 3, ROVIT_WS_XHAT2 = 4, ROVIT_WS_RSTD2 = 5,
       ROVIT_WS_ACT = 6, ROVIT_WS_DQKV = 7, ROVIT_WS_DACT = 8, ROVIT_WS_LSE = 9, ROVIT_WS_XHAT_CLS = 10, ROVIT_WS_RSTD_CLS = 11,
       ROVIT_WS_DX_IN = 12, ROVIT_WS_DX_MID = 13, ROVIT_WS_DPRE = 14, ROVIT_WS_DO = 15, ROVIT_WS_DX_OUT = 16 };
int rovit_vit_workspace_field(int batch, int depth, int field, int block, size_t* offset, size_t* bytes);
/* rovit_vit_backward for a data-parallel caller: for last_block > 0 the call does not wait for the range's weight
 * gradients on `stream`; `notify_stream` (the caller's reduction stream) is made to wait for them instead.  Issue the
 * ranges in order down to last_block == 0; that call joins everything into `stream`. */
int rovit_vit_backward_notify(const float* images, const float* d_features, const float* const* params, const void* prep,
                              void* workspace, float* const* grads, int batch, int depth, int first_block, int last_block,
                              int mlp_path, rovit_stream_t stream, rovit_stream_t notify_stream);
/* rovit_vit_backward that can also produce the gradient with respect to the input images, and can skip the weight gradients.
 *   d_images: NULL = no image gradient; else fp32 (batch/copies,3,224,224), written by the range that ends at block 0
 *             (rovit_patch_embed_dgrad with `copies`, `scale`, `accumulate`: batch must be a multiple of copies, image b's copies being
 *             batch rows s*(batch/copies) + b).  Ranges with last_block > 0 must pass NULL.
 *   grads:    NULL = the dgrad chain only: no weight-gradient launch, no write to any gradient or slab buffer, and neither the library's
 *             side stream nor its event state is used, so a pending data-parallel range sequence of another backward is left intact.
 *             The dgrad chain's launches are those of the full backward, so its d_images are bit-identical to a full backward's.
 * With grads != NULL and d_images == NULL this is rovit_vit_backward. */
int rovit_vit_backward_input(const float* images, const float* d_features, const float* const* params, const void* prep, void* workspace,
                             float* const* grads, int batch, int depth, int first_block, int last_block, int mlp_path, rovit_stream_t stream,
                             float* d_images, int copies, float scale, int accumulate);
/* Gradient-weighted attention relevance (Chefer, Gur & Wolf, ICCV 2021) of one scalar per image, on the workspace of a TRAINING
 * rovit_vit_forward (training = 1; same batch, depth and mlp_path).  d_features fp32 (B,192) = d target / d features seeds the dgrad
 * chain from block depth-1 down to block 0, run as rovit_vit_backward_input with grads == NULL (no weight gradient, no image gradient,
 * no side stream); behind each block's attention-output gradient dO one rovit_attention_relevance_step (first = 1 in the last block),
 * and block 0's attention backward and qkv dgrad are skipped.  relevance fp32 (B,197) receives row 0 of R_L = (I + A_L) ... (I + A_1),
 * A_l = mean_h relu(dP_{l,h} * P_{l,h}) (index 0, the class token, included); scratch: fp32, batch * 3 * 197 floats. */
int rovit_vit_backward_relevance(const float* d_features, const float* const* params, const void* prep, void* workspace, int batch, int depth,
                                 int mlp_path, float* relevance, float* scratch, rovit_stream_t stream);
/* Deletion / insertion curves (perturb.hip).  The patch embedding is a 16x16 convolution with stride 16, so every token row of an image
 * perturbed patch by patch is a row of the clean image's or of its baseline's token table: embed both once, then assemble sequences.
 * rovit_vit_embed: tokens fp32 (n,197,192) receives the rows rovit_vit_forward starts from -- its first two launches (rovit_cls_rows,
 * rovit_patch_embed_fwd): row 0 = cls + pos[0], row 1 + p = patch(p) W^T + bias + pos[1 + p], p = 14 * row + column. */
int rovit_vit_embed(const float* images, const float* const* params, const void* prep, float* tokens, int n, int depth, rovit_stream_t stream);
/* The inference forward (training = 0) of n_seq sequences of `tokens` rows (1..197).  Row r of sequence s is v = src[s * tokens + r]:
 * v >= 0 row v of img_tokens[seq_img[s]], v < 0 row -1 - v of base_tokens[base_shared ? 0 : seq_img[s]]; the tables hold n_img images
 * (base_tokens: n_img, or 1 when base_shared) of 197 rows from rovit_vit_embed.  seq_img (n_seq) and src (n_seq * tokens): int32 device
 * arrays; every index is clamped into its table.  Workspace: rovit_vit_workspace_bytes(n_seq, depth, 0), of which a shorter sequence
 * uses a prefix.  From block 0's LayerNorm on, the launches of rovit_vit_forward at n_seq * tokens rows (mlp_path as there): with
 * tokens = 197 and src[s * 197 + r] in {r, -1 - r} the features equal rovit_vit_forward's of the pixel image made from those patches. */
int rovit_vit_forward_tokens(const float* img_tokens, const float* base_tokens, int n_img, int base_shared, const int* seq_img, const int* src,
                             int tokens, const float* const* params, const void* prep, void* workspace, float* features, int n_seq, int depth,
                             int mlp_path, rovit_stream_t stream);
/* The same forward of n_seq sequences of DIFFERENT lengths in one call (token-dropped sequences).  The sequences are packed back to
 * back: sequence s owns rows [off[s], off[s + 1]) of src (one entry per packed row, as above) and row off[s] is its class token;
 * off: int32, n_seq + 1 entries, off[0] = 0, every length in [1, 197].  The array is passed twice.  seq_offsets_host is checked before
 * anything is launched (null, first entry, order, lengths) and plans the call; no device-to-host copy is made.  The kernels read
 * seq_offsets_dev and clamp what they find (length into [1, 197], rows into the buffers), so a device array that disagrees with the
 * host's computes on wrong rows but stays inside the buffers.  features fp32 (n_seq,192).  A sequence's features do not depend on the
 * others of the call and equal rovit_vit_forward_tokens' of that sequence alone at the same explicit mlp_path (ROVIT_MLP_AUTO picks by
 * off[n_seq]).  Batches of 16 sequences and more run as two halves on two streams, cut at the sequence boundary where the first half
 * first reaches half of the rows.  Workspace: rovit_vit_ragged_workspace_bytes(max_rows, depth) with max_rows >= off[n_seq] (the
 * inference plan of max_rows rows; it holds any n_seq <= max_rows); the entry is not told its size, the caller answers for it. */
size_t rovit_vit_ragged_workspace_bytes(int max_rows, int depth);
int rovit_vit_forward_ragged(const float* img_tokens, const float* base_tokens, int n_img, int base_shared, const int* seq_img, const int* src,
                             const int* seq_offsets_dev, const int* seq_offsets_host, const float* const* params, const void* prep,
                             void* workspace, float* features, int n_seq, int depth, int mlp_path, rovit_stream_t stream);

/* ---- PatchDropout training (Liu et al., WACV 2023): forward and backward on a kept subset of the 196 patches (patch_dropout.hip) ----
 * rovit_patch_dropout_draw: for each of `batch` samples a uniformly random subset of k (1..196) patches, one launch, no host read.
 * Patch p of sample b gets the key word (p % 4) of Philox4x32-10(key = seed, counter = (b, ROVIT_PATCH_DROPOUT_STREAM + p / 4,
 * step lo, step hi)); the patches are ranked by the integer pair (key, p) and those of rank < k are kept.  Outputs, int32:
 *   keep (batch, k)     the kept patches in ascending order
 *   src  (batch, 1 + k) the rows rovit_gather_token_rows reads: 0 (the class token), then 1 + keep
 *   inv  (batch, 197)   a token's row in the short sequence (0 for the class token), -1 for a dropped patch
 * Integer compares only, no atomics: the same (seed, step, b, k) gives the same bits on every run and grid. */
#define ROVIT_PATCH_DROPOUT_STREAM 0x50447200u      /* "PDr\0": counter word 1, + patch / 4 (0..48) */
int rovit_patch_dropout_draw(unsigned long long seed, unsigned long long step, int* keep, int* src, int* inv, int batch, int k,
                             rovit_stream_t stream);
/* The inverse of the token gather for gradients: dense bf16 (batch*197,192) row (b, t) = rows bf16 (batch*tokens,192) row
 * (b, inv[b*197 + t]) when that is in [0, tokens), else zeros.  Every dense row is written exactly once with 16-byte stores; no
 * memset, no atomics.  rows, dense: 16-byte aligned. */
int rovit_scatter_token_rows(const void* rows, const int* inv, void* dense, int batch, int tokens, rovit_stream_t stream);
/* The training forward on kept tokens.  All 197 rows of every image are embedded (rovit_vit_embed's two launches, position embedding
 * included) into token_table, fp32 (batch,197,192); rows src[b * tokens + r] (r < tokens, as rovit_vit_forward_tokens reads them; row 0
 * the class token) of image seq_img[b] are gathered; from block 0's LayerNorm on the launches are those of rovit_vit_forward with
 * training = 1 at batch * tokens rows, and the activations the backward reads are kept.  tokens in [2, 197].  workspace:
 * rovit_vit_workspace_bytes(batch, depth, 1) -- the plan of `tokens` rows is no larger.  prepare: 0 = prep is current, 1 = prepare the
 * weight images inside the call (rovit_vit_forward_prepare), 2 = ... and write the constant tables.  With tokens = 197 and
 * src[b * 197 + r] = r the features and saved activations are rovit_vit_forward's bits. */
int rovit_vit_forward_train_tokens(const float* images, const int* seq_img, const int* src, int tokens, const float* const* params, void* prep,
                                   void* workspace, float* token_table, float* features, int batch, int depth, int mlp_path, int prepare,
                                   rovit_stream_t stream);
/* The backward of rovit_vit_forward_train_tokens (same batch, depth, tokens, mlp_path and workspace), every block in one call: the
 * launches of rovit_vit_backward at batch * tokens rows down to block 0's input gradient, rovit_scatter_token_rows through inv
 * (batch,197) into dense_grad (bf16, batch*197*192 elements), then the patch-embedding, position and class-token gradients at 197
 * tokens as in rovit_vit_backward: a dropped patch contributes exact zeros.  grads as there; every entry is overwritten. */
int rovit_vit_backward_tokens(const float* images, const float* d_features, const int* inv, int tokens, const float* const* params,
                              const void* prep, void* workspace, void* dense_grad, float* const* grads, int batch, int depth, int mlp_path,
                              rovit_stream_t stream);

/* ---- the individual backbone kernels (used by rovit_vit_* and exposed for unit tests / profiling) ---------- */
/* C = A(M,K) W(N,K)^T + bias with a fused epilogue:
 *   BF16  out bf16 (M,N)                      GELU  out = gelu(c), out2 = gelu'(c)  (both bf16, ld = ldo)
 *   RESID xres fp32 (M,N) += c                MUL   out = c * mul (bf16)
 *   PATCH row m=(b,p) of M=B*(tokens-1) -> xres[b*tokens+1+p] = c + pos[1+p]                                 */
int rovit_gemm_nt(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, int epi, void* out,
                  int ldo, void* out2, float* xres, int ldx, const void* mul, int ldm, const float* pos, int tokens,
                  rovit_stream_t stream);
/* X(M,192) += bf16(A W^T + bias), fused with the LayerNorm that follows the residual add (timm Block: x = x + f(x);
 * norm(x)): xhat_out bf16 (M,192) and rstd_out (M) of the updated rows; xhat_out NULL = residual add only. */
int rovit_gemm_resid_ln(const void* A, int lda, const void* W, int ldw, int M, int K, const float* bias, float* X, void* xhat_out,
                        float* rstd_out, float eps, rovit_stream_t stream);
/* The MLP half of a block in ONE launch (round 3; timm Block: x = x + mlp(norm2(x)), then the next norm1 -- timm `Mlp` and
 * `Block` reached through models/backbone.py:23-25):  X (M,192) += fc2(GELU(fc1(xhat2))) + biases, xhat_out / rstd_out = the
 * LayerNorm of the updated rows (xhat_out NULL = residual add only).  act / dact (bf16 (M,768): GELU(pre) and GELU'(pre), what
 * the backward needs) may both be NULL (inference: nothing is kept), or dact alone.  `wstream` is the weight image written
 * by rovit_mlp_prepare_stream (rovit_mlp_stream_bytes() bytes) from w1f = the bf16 fc1 weight with the norm2 affine folded in
 * (rovit_prep_weight's Wf, (768,192)) and w2 = the bf16 fc2 weight (192,768); b1 = the folded fc1 bias (768), b2 (192).
 * The VALUES of act and dact are bit-identical to rovit_gemm_nt(ROVIT_EPI_GELU)'s outputs; their LAYOUT is chunk-major: element
 * (row m, hidden unit h) of a tensor of act_rows rows at ((h / 32) * act_rows + m) * 32 + h % 32, so that a 16-row tile's store is one
 * contiguous kilobyte (row-major the launch took 94 us once its 155 MB of outputs no longer fit the Infinity Cache, chunk-major 76).
 * A launch may cover a row range of the tensors: pass act / dact advanced by first_row * 32 elements, M = rows of the range,
 * act_rows = rows of the whole tensors (= M for a whole-batch call). */
size_t rovit_mlp_stream_bytes(void);
int rovit_mlp_prepare_stream(const void* w1f, const void* w2, void* wstream, rovit_stream_t stream);
int rovit_mlp_fused_fwd(const void* xhat2, const void* wstream, const float* b1, const float* b2, void* act, void* dact, float* X,
                        void* xhat_out, float* rstd_out, float eps, int M, int act_rows, rovit_stream_t stream);
/* Everything of a block behind the attention in ONE launch (timm Block: x = x + proj(attn(norm1 x)); x = x + mlp(norm2 x); then the next
 * block's norm1 -- models/backbone.py:23-25):  X += o Wp^T + bp;  xhat2 / rstd2 = LayerNorm(X) (kept for the backward; NULL: inference);
 * X += fc2(GELU(fc1(xhat2)));  xhat_out / rstd_out = LayerNorm(X) (NULL: none).  o: bf16 (M,192) attention output; wstream from
 * rovit_mlp_prepare_stream_tail (w1f, w2 as rovit_mlp_prepare_stream; wproj = the bf16 (192,192) proj weight); act / dact chunk-major
 * as rovit_mlp_fused_fwd.  The residual stream stays in fp32 registers between the halves (nothing staged through bf16: closer to the
 * fp32 reference than proj + rovit_mlp_fused_fwd as two launches, not bit-identical to them).
 * With wqkv_next (the NEXT block's bf16 qkv weight (576,192), its norm1 affine folded in) given to the preparation and bq_next / qkv_next
 * given to the launch, the launch also writes that block's qkv projection qkv_next (M,576) = xhat_out Wqkv^T + bq_next: the forward
 * of a block is then two launches, attention and this one. */
int rovit_mlp_prepare_stream_tail(const void* w1f, const void* w2, const void* wproj, const void* wqkv_next, void* wstream,
                                  rovit_stream_t stream);
int rovit_block_tail_fwd(const void* o, const void* wstream, const float* bp, const float* b1, const float* b2, float* X, void* xhat2,
                         float* rstd2, void* act, void* dact, void* xhat_out, float* rstd_out, const float* bq_next, void* qkv_next,
                         float eps, int M, int act_rows, rovit_stream_t stream);
/* The dgrad chain of the same half in ONE launch (autograd of the above, training/trainer.py:119,136):
 *   dpre (M,768) = (dY (M,192) W2T^T) * dact        -- kept: the fc1 weight gradient reads it (bit-identical to rovit_gemm_nt(ROVIT_EPI_MUL))
 *   dX (M,192) += rstd2 (g - mean(g) - xhat2 mean(g xhat2)),  g = dpre W1T^T;   dXb = bf16(dX)     (= rovit_gemm_ln_bwd)
 * wstream_bwd: rovit_mlp_prepare_stream(w1f := W2T bf16 (768,192), w2 := W1T bf16 (192,768), norm2 affine folded in).
 * dact (input) and dpre (output) are chunk-major [24][M][32] like the forward's act / dact; rovit_wgrad_multi_ex reads them as such. */
/* dX == NULL (round 4, what rovit_vit_backward does): the residual gradient travels in bf16 -- the incoming gradient is dY itself,
 * dXb = bf16(float(dY) + the LayerNorm-backward term), and no fp32 dX is read or written. */
int rovit_mlp_fused_bwd(const void* dY, const void* wstream_bwd, const void* dact, void* dpre, const void* xhat2, const float* rstd2,
                        float* dX, void* dXb, int M, rovit_stream_t stream);
/* The row-local part of the backward between two attention backwards in ONE launch (what rovit_vit_backward runs on the one-launch MLP
 * path): the qkv dgrad + norm1 backward of block i in front of the MLP dgrad chain of block i-1,
 *   xout (M,192) = bf16(float(xmid_in) + rstd1 (g - mean(g) - xhat1 mean(g xhat1))),  g = bf16(dqkv (M,576) WqkvT^T)
 *                  -- rovit_gemm_ln_bwd(dqkv, K = 576, ..., dXb_in = xmid_in, dXb = xout): same MFMA chain, same staged row arithmetic
 *   then rovit_mlp_fused_bwd(dY = xout, ..., dX = NULL, dXb) of block i-1, on the rows just computed: they stay in LDS as the B
 *   fragments of the fc2 dgrad and as the residual rows of the norm2 backward, so dpre and dXb are bit-identical to that call's;
 *   xout is written (the fc2 weight gradient reads it) and never read by the launch.
 * wstream_bwd: rovit_mlp_prepare_stream_bwd(w2T (768,192), w1T folded (192,768), wqkvT_next = block i's bf16 TRANSPOSED qkv weight
 * (192,576), norm1 affine folded in, wstream): rovit_mlp_prepare_stream's dgrad image plus 18 entries of WqkvT fragments.
 * Partial modes: dqkv == NULL = the MLP part alone (xout is then the INPUT dY; exactly rovit_mlp_fused_bwd); dact == NULL = the front
 * part alone (dpre, xhat2, rstd2, dXb unused). */
int rovit_mlp_prepare_stream_bwd(const void* w2T, const void* w1T, const void* wqkvT_next, void* wstream, rovit_stream_t stream);
int rovit_block_bwd_fused(const void* dqkv, const void* xhat1, const float* rstd1, const void* xmid_in, void* xout, const void* wstream_bwd,
                          const void* dact, void* dpre, const void* xhat2, const float* rstd2, void* dXb, int M, rovit_stream_t stream);
/* The same launch for the class-token block as block i (the last block, whose post-attention half runs on the class-token rows alone):
 * xmid_step > 0 says that only the rows m with m % xmid_step == 0 of xmid_in carry a gradient (xmid_step = 197: one row per image).
 * Every other row is taken as exact zeros by a select, so what xmid_in holds there (stale rows, NaN) never reaches an output; the rows
 * are still addressed, so xmid_in must be a readable (M,192) buffer.  xout is bit-identical to
 * rovit_gemm_ln_bwd_cls(dqkv, K = 576, ..., dXb_in = xmid_in, cls_step = xmid_step, dXb = xout), dpre / dXb to rovit_mlp_fused_bwd on it.
 * xmid_step == 0 is rovit_block_bwd_fused; xmid_step < 0 is refused.  Partial modes as rovit_block_bwd_fused. */
int rovit_block_bwd_fused_cls(const void* dqkv, const void* xhat1, const float* rstd1, const void* xmid_in, int xmid_step, void* xout,
                              const void* wstream_bwd, const void* dact, void* dpre, const void* xhat2, const float* rstd2, void* dXb, int M,
                              rovit_stream_t stream);
/* dgrad through a Linear that follows a LayerNorm, fused with that LayerNorm's backward:
 * dxhat = dY W^T;  dX += rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat));  dXb = bf16(dX).
 * dXb_in != NULL (round 4): the incoming residual gradient as bf16 rows (M,192); then dXb = bf16(float(dXb_in) + that term) and the fp32
 * dX (may be NULL) is neither read nor written: 58 MB less per launch at batch 256. */
int rovit_gemm_ln_bwd(const void* dY, int ldy, const void* W, int ldw, int M, int K, const void* xhat, const float* rstd, float* dX,
                      const void* dXb_in, void* dXb, rovit_stream_t stream);
/* rovit_gemm_ln_bwd with a bf16 incoming gradient dXb_in that is non-zero on every cls_step-th row only (cls_step > 0; the class-token
 * block of rovit_vit_backward): the other rows count as zeros and are not read.  dXb = bf16(that row or zero + the LayerNorm-backward term). */
int rovit_gemm_ln_bwd_cls(const void* dY, int ldy, const void* W, int ldw, int M, int K, const void* xhat, const float* rstd,
                          const void* dXb_in, int cls_step, void* dXb, rovit_stream_t stream);
/* G(N,K) = dY(M,N)^T A(M,K) and colsum(dY), split over M into `splits` fp32 slabs inside ws */
int rovit_wgrad_splits(int M, int N, int K);
size_t rovit_wgrad_workspace_bytes(int N, int K, int splits);
int rovit_wgrad(const void* dY, int ldy, const void* A, int lda, int M, int N, int K, int splits, int patch_tokens, float* ws,
                rovit_stream_t stream);
/* Up to 4 weight gradients that share M (the four linears of a transformer block) in ONE launch: 96 x 192 output tiles,
 * `splits` M-splits for all of them (24 tiles per split for a DeiT-Tiny block, so 16 splits fill the chip and the fp32
 * partial slabs are 28 MB instead of 75.6 MB per block).  Arrays of n entries; ws[j] sized by
 * rovit_wgrad_workspace_bytes(N[j], K[j], splits) and finished by rovit_wgrad_reduce with the same `splits`. */
int rovit_wgrad_multi(const void* const* dY, const int* ldy, const void* const* A, const int* lda, const int* N, const int* K,
                      float* const* ws, int n, int M, int splits, rovit_stream_t stream);
/* the same with per-problem operand layouts: a_blk[j] / y_blk[j] != 0 = A / dY of problem j is chunk-major [cols / 32][M][32]
 * (rovit_mlp_fused_fwd's act, rovit_mlp_fused_bwd's dpre); NULL = all row-major */
int rovit_wgrad_multi_ex(const void* const* dY, const int* ldy, const void* const* A, const int* lda, const int* N, const int* K,
                         float* const* ws, const int* a_blk, const int* y_blk, int n, int M, int splits, rovit_stream_t stream);
int rovit_wgrad_reduce(const float* ws, int splits, int N, int K, const float* gamma, const float* beta, const float* W,
                       float* dW, float* db, float* dgamma, float* dbeta, float* g_scratch, rovit_stream_t stream);
/* softmax(q k^T * scale) v per (image, head); qkv bf16 (B*T, 3*H*64) = [q|k|v]; out bf16 (B*T, H*64);
 * lse2 (B,H,T) = log2 sum exp(scale q.k); tokens 1 .. 208, head_dim 64.
 * THE SCALE RULE of every attention entry: a call whose scale the kernel would not honour exactly is refused with ROVIT_ERR_SHAPE and a
 * message naming the value, before anything is launched.
 *   - the forwards (rovit_attention_fwd, _cls_fwd, _fwd_ragged, _cls_fwd_ragged) and rovit_attention_cls_bwd take any finite scale > 0
 *     (they take the row maximum and mask padded keys on the unscaled scores: a maximum and a mask only for scale > 0);
 *   - rovit_attention_bwd takes scale == 0.125f only: its kernel folds head_dim^-1/2 = 2^-3 into the exponent offset and the dV store
 *     (exact in binary floating point), and with another value dQ and dK would come out multiplied by 0.125 / scale.
 * The engine passes 0.125f everywhere; rovit_attention_relevance_step and the rollout kernels take no scale and use 1/8. */
int rovit_attention_fwd(const void* qkv, void* out, float* lse2, int batch, int tokens, int heads, int head_dim, float scale,
                        rovit_stream_t stream);
/* softmax(scale q k^T) as fp32 (B,H,T,T) from a saved qkv tensor -- explainability only */
int rovit_attention_probs(const void* qkv, float* probs, int batch, int tokens, int heads, int head_dim, float scale,
                          rovit_stream_t stream);
int rovit_attention_bwd(const void* qkv, const void* out, const float* lse2, const void* dout, void* dqkv, int batch, int tokens,
                        int heads, int head_dim, float scale, rovit_stream_t stream);
/* The same attention when ONLY THE CLASS TOKEN'S output is consumed -- the last block of the backbone, whose other rows nothing reads
 * (timm VisionTransformer.forward_head takes x[:, 0], reached through models/backbone.py:23-25): 197 scores per (image, head) instead
 * of 197 x 197.  Forward writes out[b, 0, :] and lse2[b, h, 0] only.  Backward takes the gradient of that row (dout[b, 0, :]; the other
 * rows of dout are not read) and writes the WHOLE dqkv: dK, dV for every token, dQ for the class token, zeros in every other dQ row. */
int rovit_attention_cls_fwd(const void* qkv, void* out, float* lse2, int batch, int tokens, int heads, int head_dim, float scale,
                            rovit_stream_t stream);
int rovit_attention_cls_bwd(const void* qkv, const void* out, const float* lse2, const void* dout, void* dqkv, int batch, int tokens,
                            int heads, int head_dim, float scale, rovit_stream_t stream);
/* The two attention forwards on a RAGGED batch (rovit_vit_forward_ragged: offsets as there, host copy checked, device copy clamped):
 * qkv bf16 (total_rows, 3*H*64), total_rows = off[n_seq]; one workgroup (rovit_attention_fwd_ragged) or one wave (_cls_) per
 * (sequence, head), and a sequence of t tokens costs t tokens: key tiles, P V blocks and staged rows beyond t are skipped, exactly.
 * Every sequence's result equals rovit_attention_fwd / rovit_attention_cls_fwd on its rows alone at tokens = t.  lse2: fp32
 * (H, total_rows) -- the class-token form writes column off[s] only -- or NULL.  rovit_attention_fwd_ragged: out bf16 (total_rows,
 * H*64).  rovit_attention_cls_fwd_ragged: out bf16 (n_seq, H*64), COMPACT, one row per sequence; with x_rows fp32 (total_rows, H*64)
 * and x_cls fp32 (n_seq, H*64) (both or neither) it also copies row off[s] of x_rows to row s of x_cls. */
int rovit_attention_fwd_ragged(const void* qkv, void* out, float* lse2, const int* seq_offsets_dev, const int* seq_offsets_host, int n_seq,
                               int heads, int head_dim, float scale, rovit_stream_t stream);
int rovit_attention_cls_fwd_ragged(const void* qkv, void* out, float* lse2, const float* x_rows, float* x_cls, const int* seq_offsets_dev,
                                   const int* seq_offsets_host, int n_seq, int heads, int head_dim, float scale, rovit_stream_t stream);
int rovit_layernorm_fwd(const float* x, void* xhat, float* rstd, int rows, int dim, float eps, rovit_stream_t stream);
int rovit_layernorm_bwd(const void* dxhat, const void* xhat, const float* rstd, float* dX, void* dXb, int rows, int dim,
                        rovit_stream_t stream);
int rovit_im2col(const float* x, void* col, int batch, rovit_stream_t stream);
/* PatchEmbed (timm conv k16 s16, reached through models/backbone.py:12-25) without the im2col buffer: the GEMM and the
 * weight-gradient kernel gather their pixel operand from the fp32 NCHW images and round it to bf16 on the way into LDS.
 *   fwd:   X[b*tokens + 1 + p][:] = patch(b, p) W^T + bias + pos[1 + p]      (W bf16 (192,768), X fp32 (batch*tokens,192))
 *   wgrad: slabs of G[n][k] = sum_(b,p) dY[b*tokens + 1 + p][n] pixel(b,p,k) in ws (rovit_wgrad_workspace_bytes(N,768,splits)),
 *          finished by rovit_wgrad_reduce; dY bf16 (batch*tokens, N). */
int rovit_patch_embed_fwd(const float* images, const void* W, const float* bias, const float* pos, float* X, int batch, int tokens,
                          rovit_stream_t stream);
int rovit_patch_embed_wgrad(const void* dY, int ldy, const float* images, int batch, int tokens, int N, int splits, float* ws,
                            rovit_stream_t stream);
/* the patch embedding's data gradient, the transpose of rovit_patch_embed_fwd (input_grad.hip):
 *   d_images[b,c,16py+ky,16px+kx] (+)= scale * sum_{s<copies} sum_n dY[(s*b_out + b)*197 + 1 + 14py + px][n] W[n][c*256 + ky*16 + kx]
 * dY bf16 (copies*b_out*197, ldy) token rows (class-token rows not read); W the prepared bf16 (192,768) patch weight; d_images fp32 NCHW
 * (b_out,3,224,224), each element written once: scale * sum when accumulate == 0, added to what it holds otherwise.  The copies are
 * summed in the fp32 accumulators in the order s = 0, 1, ... before the scale.  bf16 MFMA, fp32 accumulation; no atomics. */
int rovit_patch_embed_dgrad(const void* dY, int ldy, const void* W, float* d_images, int b_out, int copies, float scale, int accumulate,
                            rovit_stream_t stream);
/* one block's relevance step (relevance.hip): u fp32 (B,197) <- u + u A,  A[i,j] = (1/3) sum_h relu(P_h[i,j] dP_h[i,j]), with
 * P_h = exp2(log2(e)/8 Q_h K_h^T - lse2) from the block's saved qkv bf16 (B*197,576) and lse2 fp32 (B,3,197) (the forward's log2-sum-exp),
 * dP_h = dO_h V_h^T from dout bf16 (B*197,192), the gradient with respect to the attention output.  first != 0: u is taken as e_0 and not
 * read, and of Q, dout and lse2 only row 0 of every image is read (the training forward's last block writes no other row of lse2 or dO).
 * scratch: fp32, batch * 3 * 197 floats.  Two launches; bf16 MFMA, fp32 sums in a fixed order, no atomics: bit-identical run to run.
 * qkv and dout 16-byte aligned. */
int rovit_attention_relevance_step(const void* qkv, const float* lse2, const void* dout, float* u, float* scratch, int batch, int first,
                                   rovit_stream_t stream);
int rovit_cls_rows(const float* cls, const float* pos, float* X, int batch, int tokens, rovit_stream_t stream);
int rovit_cls_norm_fwd(const float* X, const float* gamma, const float* beta, float* feat, float* xhat, float* rstd, int batch,
                       int tokens, float eps, rovit_stream_t stream);
/* backward of the final LayerNorm on the class tokens: writes the CLS rows of dX (fp32) / dXb (bf16); zero_fill != 0 first zeroes both
 * for all tokens (rovit_vit_backward passes 0: only CLS rows are read behind it) */
int rovit_cls_norm_bwd(const float* dfeat, const float* xhat, const float* rstd, const float* gamma, float* dX, void* dXb,
                       float* dgamma, float* dbeta, int batch, int tokens, int zero_fill, rovit_stream_t stream);
/* dpos[t] = sum over images of the token gradient, dcls = dpos[0]; the gradient as fp32 rows (dX) or bf16 rows (dXb): exactly one */
int rovit_pos_grad(const float* dX, const void* dXb, float* dpos, float* dcls, int batch, int tokens, rovit_stream_t stream);
int rovit_prep_weight(const float* W, const float* bias, const float* gamma, const float* beta, void* Wf, void* WfT,
                      float* bias_f, int N, int K, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Batch augmentation on the device: the data movement of `cutmix_or_mixup` (call site training/trainer.py:84-96;
 * its module data/transforms.py is absent from the reference checkout, so this follows the published MixUp / CutMix
 * definitions).  mode 0: out[b] = lam x[b] + (1-lam) x[perm[b]];  mode 1: out[b] = x[perm[b]] inside rows [y0,y1) x
 * cols [x0,x1), x[b] elsewhere.  images/out fp32 (B,C,H,W) distinct buffers, perm int64 (B) on the device.
 * ------------------------------------------------------------------------------------------------------------ */
int rovit_mix_images(const float* images, float* out, const long long* perm, int batch, int channels, int height, int width,
                     int mode, float lam, int y0, int y1, int x0, int x1, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer step on flat fp32 buffers: global-norm clipping + AdamW as the reference applies them
 * (training/trainer.py:123-128,137-141 clip_grad_norm_(1.0); training/optimizer.py:7-32 AdamW).
 * rovit_sq_norm_accum: *out_sq += sum g^2 (caller zeroes out_sq; several buffers may accumulate into one norm).
 *   scratch: NULL, or >= 520 floats zeroed ONCE by the caller and then owned by this function (block partials are then
 *   combined in a fixed order: bit-reproducible; with NULL they are combined with float atomics).
 * rovit_adamw_flat: torch.optim.AdamW semantics; grad_scale = device scalar multiplied into g (clip coefficient)
 * or NULL; t = 1-based step count for the bias correction.
 * ------------------------------------------------------------------------------------------------------------ */
int rovit_sq_norm_accum(const float* g, size_t n, float* out_sq, float* scratch, rovit_stream_t stream);
/* clip_grad_norm_ coefficient on the device: *norm_out = sqrt(*sq) (optional), *coef = min(1, max_norm / (norm + 1e-6)).
 * NON-FINITE NORMS, as torch's clamp gives them: a NaN squared norm (any NaN gradient) gives *norm_out = NaN and *coef = NaN, so that
 * the step it scales is poisoned as a whole, not applied unscaled; a norm of +inf gives *coef = 0; a norm of 0 gives *coef = 1 exactly. */
int rovit_clip_coef(const float* sq, float max_norm, float* coef, float* norm_out, rovit_stream_t stream);
int rovit_adamw_flat(float* p, const float* g, float* m, float* v, size_t n, const float* grad_scale, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int t, rovit_stream_t stream);
/* The same two steps as ONE launch each (round 4).  rovit_sq_norm_clip: squared norm over up to four buffers (HOST arrays bufs /
 * counts; 16-byte aligned, counts multiples of 4), block partials added in block order by the block that finishes last, then the
 * coefficient, by the same rule as rovit_clip_coef (NaN norm -> NaN coefficient, +inf -> 0, 0 -> 1: the two are one device function);
 * scratch >= 264 floats, zeroed ONCE by the caller (the kernel re-arms its ticket).
 * rovit_adamw_flat_multi: rovit_adamw_flat over up to four segments with their own lr and step count t (HOST arrays). */
int rovit_sq_norm_clip(const float* const* bufs, const size_t* counts, int n_bufs, float max_norm, float* coef, float* norm_out,
                       float* scratch, size_t scratch_floats, rovit_stream_t stream);
int rovit_adamw_flat_multi(float* const* p, const float* const* g, float* const* m, float* const* v, const size_t* n, const float* lr,
                           const int* t, int n_segs, const float* grad_scale, float beta1, float beta2, float eps, float weight_decay,
                           rovit_stream_t stream);
/* rovit_adamw_flat_multi with an exponential moving average of the parameters updated in the same launch (the reference has none:
 * parity unpinned).  Same segments, pieces and AdamW arithmetic (p, m, v come out bit-identical); after an element's new p,
 * ema += omd * (p - ema) with omd = (float)(1 - (double)ema_decay[i]) -- the lerp form, which leaves ema == p exactly as it is.
 * Per segment: g[i] == NULL = EMA only (p is read; p, m, v are not written; m[i], v[i] may be NULL, t[i] is ignored); ema[i] == NULL =
 * plain AdamW; both NULL is ROVIT_ERR_NULL.  ema_decay[i] outside [0, 1) is ROVIT_ERR_SHAPE.  ema 16-byte aligned like the others.
 * rovit_swap_flat_multi exchanges the contents of up to four buffer pairs a[i] <-> b[i] (n[i] floats each, 16-byte aligned, a pair
 * does not overlap) in one launch: the parameters and their average change places for validation. */
int rovit_adamw_ema_flat_multi(float* const* p, const float* const* g, float* const* m, float* const* v, float* const* ema,
                               const size_t* n, const float* lr, const int* t, const float* ema_decay, int n_segs,
                               const float* grad_scale, float beta1, float beta2, float eps, float weight_decay, rovit_stream_t stream);
int rovit_swap_flat_multi(float* const* a, float* const* b, const size_t* n, int n_segs, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Joint multi-task loss, forward + gradient in one launch: JointLoss.forward (training/losses.py:139-181) with
 * FocalLoss (:15-38), OrdinalBCELoss (:48-72), UncertaintyLoss (:80-101), KANRegressionLoss (:109-114).
 * Class targets are int64 (torch.long); severity targets fp32, or int64 labels with severity_is_int64 != 0 (the reference casts
 * them with .float(), :89-90, :110-111 -- done inside the kernel; ordinal targets are (severity > k), :55-56).  A class label outside [0, num_classes) makes every loss NaN
 * instead of reading out of bounds.  NULL head pointers = head inactive at this curriculum stage.
 * d_* = d(total)/d(head output) for an upstream gradient of 1; losses_out = [cls, ord, unc, kan, total].
 * rovit_scale_buffers multiplies up to 5 buffers by a device scalar (chain rule with the upstream gradient).
 * ------------------------------------------------------------------------------------------------------------ */
int rovit_joint_loss(const float* cls_logits, const float* ordinal_logits, const float* mu, const float* log_var,
                     const float* kan_severity, const long long* class_targets, const void* severity_targets, int severity_is_int64,
                     const float* focal_alpha, float* d_cls, float* d_ord, float* d_mu, float* d_lv, float* d_kan,
                     float* losses_out, int batch, int num_classes, float lambda_ord, float mu_unc, float nu_kan, float focal_gamma,
                     rovit_stream_t stream);
int rovit_scale_buffers(float* const* bufs, const int* counts, int n, const float* scale, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * A training epoch with one synchronisation (train_epoch.hip).
 * rovit_joint_loss_mixed replaces the CutMix / MixUp branch of Trainer.train_epoch (training/trainer.py:104-111: the loss twice on the
 * same head outputs, then lam * a[k] + (1 - lam) * b[k] on the five dict entries) and the bookkeeping of :144-153 (five loss .item(),
 * max / eq / sum and a sixth .item() per step) with ONE launch of rovit_joint_loss's shape and arithmetic (one shared statement of the
 * per-row formulas, csrc/joint_loss_row.h).
 *   class_targets_b == NULL: every loss and every gradient is bit-identical to rovit_joint_loss on the same inputs; lam is not read.
 *   class_targets_b != NULL: the focal term of a row is lam f(t_a) + (1 - lam) f(t_b) and its gradient is mixed the same way; softmax
 *     and lse are computed once per row; the ordinal, heteroscedastic and KAN terms do not depend on the class label and are computed
 *     once (the reference's lam x + (1 - lam) x equals x to rounding).  0 <= lam <= 1, passed by value: the host drew it.
 *   A class label outside [0, num_classes) in either column makes the class loss and the total NaN instead of reading out of bounds.
 * table != NULL: the launch also writes row `row` (< capacity) of the caller's epoch table, ROVIT_TRAIN_ROW_WORDS 4-byte words per row:
 *   float [ROVIT_TRAIN_ROW_LOSS + 0..4] = losses_out;  int [ROVIT_TRAIN_ROW_CORRECT] rows whose FIRST-maximum argmax of cls_logits (a NaN
 *   counts as the maximum, as in torch.max) equals class_targets_a (trainer.py:151-153);  int [ROVIT_TRAIN_ROW_BATCH] = batch;
 *   int [ROVIT_TRAIN_ROW_NONFINITE] = 1 when the total is not finite.  The host hands out the row index, so a row has one writer: plain
 *   stores, no atomics, no device counter, no synchronisation.
 * rovit_train_finalize reduces rows [0, n_rows) to `result`, ROVIT_TRAIN_RESULT_WORDS 8-byte words:
 *   int64  [ROVIT_TRAIN_N_ROWS], [ROVIT_TRAIN_SAMPLES], [ROVIT_TRAIN_CORRECT], [ROVIT_TRAIN_NONFINITE] (rows whose flag is set)
 *   double [ROVIT_TRAIN_LOSS + 0..4] column sums of the five losses, each row widened to fp64, added in a fixed order (strided over 256
 *          threads, then a fixed tree): bit-identical from run to run.  It is the epoch's one device-to-host copy.
 * Both refuse a bad descriptor before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_TRAIN_MAX_ROWS (1 << 20)
enum {
  ROVIT_TRAIN_ROW_LOSS = 0, ROVIT_TRAIN_ROW_CORRECT = 5, ROVIT_TRAIN_ROW_BATCH = 6, ROVIT_TRAIN_ROW_NONFINITE = 7, ROVIT_TRAIN_ROW_WORDS = 8,
  ROVIT_TRAIN_N_ROWS = 0, ROVIT_TRAIN_SAMPLES = 1, ROVIT_TRAIN_CORRECT = 2, ROVIT_TRAIN_NONFINITE = 3, ROVIT_TRAIN_LOSS = 4,
  ROVIT_TRAIN_RESULT_WORDS = 9
};
typedef struct rovit_train_loss {
  int batch, num_classes, severity_is_int64, row, capacity;
  float lam, lambda_ord, mu_unc, nu_kan, focal_gamma;
  const float* cls_logits;            /* (batch, C) */
  const float* ordinal_logits;        /* (batch, C - 1) or NULL: head gated, as in rovit_joint_loss */
  const float* mu; const float* log_var; const float* kan_severity;      /* (batch) or NULL */
  const long long* class_targets_a;   /* (batch) */
  const long long* class_targets_b;   /* (batch) or NULL: not mixed */
  const void* severity_targets;       /* (batch) fp32, or int64 with severity_is_int64 != 0 */
  const float* focal_alpha;           /* (C) or NULL */
  float* d_cls; float* d_ord; float* d_mu; float* d_lv; float* d_kan;    /* d(total)/d(head output) for an upstream gradient of 1 */
  float* losses_out;                  /* [5]: cls, ord, unc, kan, total */
  void* table;                        /* (capacity, ROVIT_TRAIN_ROW_WORDS) 4-byte words, or NULL: nothing recorded */
} rovit_train_loss;
typedef struct rovit_train_final {
  int n_rows, capacity;
  const void* table;
  void* result;                       /* ROVIT_TRAIN_RESULT_WORDS 8-byte words */
} rovit_train_final;
int rovit_joint_loss_mixed(const rovit_train_loss* p, rovit_stream_t stream);
int rovit_train_finalize(const rovit_train_final* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Test-set evaluation and validation without a per-batch host round trip (evaluate.hip).
 * rovit_eval_accumulate replaces the collection part of Evaluator.evaluate (evaluation/evaluator.py:37-67: softmax, argmax,
 * squeeze, exp(0.5 log_var) and five device-to-host copies per batch) and of Trainer.val_epoch (training/trainer.py:183-231: six
 * .item() per batch): ONE launch per batch writes rows [offset, offset + batch) of the caller's record arrays (capacity rows each):
 *   probs (capacity, C) = softmax with expf(logit - row max);  pred = FIRST argmax of those fp32 probabilities (torch.argmax /
 *   np.argmax);  label (a class label outside [0, C) is recorded as -1 and counted by the finalise);  sev_pred = kan_severity, or the
 *   severity label as float when kan_severity is NULL (evaluator.py:50-53);  sev_true;  uncertainty = exp(0.5 log_var) (NaN when
 *   log_var is NULL).  losses (the five floats rovit_joint_loss left on the device) go to row loss_row of loss_table (loss_capacity, 5).
 * The host knows the row offset, so there is no device counter and no synchronisation; every value is per-sample.
 * rovit_eval_finalize replaces evaluation/metrics.py:9-61,96-122 (accuracy, f1_score, confusion_matrix,
 * precision_recall_fscore_support, mae, spearmanr, brier_score, ece): once per epoch it reduces the n recorded rows to `result`,
 * ROVIT_EVAL_RESULT_WORDS 8-byte words:
 *   int64  [ROVIT_EVAL_CONFUSION + t * C + p] confusion matrix   [ROVIT_EVAL_BIN_COUNT + k], [ROVIT_EVAL_BIN_CORRECT + k] per ECE bin
 *          [ROVIT_EVAL_RANK + 0..2] sum (Ra-n-1)(Rb-n-1), sum (Ra-n-1)^2, sum (Rb-n-1)^2 with the doubled tie-averaged rank
 *          R_i = 2 #{x_j < x_i} + #{x_j == x_i} + 1 of sev_true (a) and sev_pred (b), counted, not sorted (exact for n <= 2^20)
 *          [ROVIT_EVAL_NONFINITE + 0..1] non-finite values in sev_true / sev_pred   [ROVIT_EVAL_BAD_LABELS]   [ROVIT_EVAL_N]
 *   double [ROVIT_EVAL_BIN_CONF + k] sum of confidences per bin (lo < conf <= hi against bin_edges, n_bins + 1 doubles, conf widened)
 *          [ROVIT_EVAL_BRIER] sum_i sum_c (p_ic - onehot_ic)^2   [ROVIT_EVAL_ABS_ERR] sum |sev_true - sev_pred|
 *          [ROVIT_EVAL_LOSS + 0..4] column sums of the first n_loss_rows rows of loss_table
 * Integers are added with integer atomics (order cannot change them); every floating sum is fp64 over a fixed partition of the rows
 * (256-row chunks, fixed tree inside and across chunks): bit-identical from run to run and independent of the batch split.
 * The whole block is zeroed first, so words nothing writes (bins beyond n_bins, padding) are 0 and blocks compare byte for byte.
 * Workspaces (device, caller's): rank_counts 4 n uint32, partials rovit_eval_partials_doubles(n) doubles.
 * Both refuse a bad descriptor before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_EVAL_MAX_CLASSES 8
#define ROVIT_EVAL_MAX_BINS 64
#define ROVIT_EVAL_MAX_ROWS (1 << 20)
enum {
  ROVIT_EVAL_CONFUSION = 0, ROVIT_EVAL_BIN_COUNT = 64, ROVIT_EVAL_BIN_CORRECT = 128, ROVIT_EVAL_RANK = 192, ROVIT_EVAL_NONFINITE = 195,
  ROVIT_EVAL_BAD_LABELS = 197, ROVIT_EVAL_N = 198, ROVIT_EVAL_INT_WORDS = 200,
  ROVIT_EVAL_BIN_CONF = 200, ROVIT_EVAL_BRIER = 264, ROVIT_EVAL_ABS_ERR = 265, ROVIT_EVAL_LOSS = 266, ROVIT_EVAL_RESULT_WORDS = 272
};
typedef struct rovit_eval_batch {
  int batch, num_classes, offset, capacity, severity_is_int64, loss_row, loss_capacity;
  const float* cls_logits;          /* (batch, C) */
  const float* kan_severity;        /* (batch) or NULL */
  const float* log_var;             /* (batch) or NULL */
  const long long* class_labels;    /* (batch) */
  const void* severity_labels;      /* (batch) fp32, or int64 with severity_is_int64 != 0 */
  const float* losses;              /* [5] or NULL */
  float* probs; int* pred; int* label; float* sev_pred; float* sev_true; float* uncertainty;
  float* loss_table;                /* (loss_capacity, 5); required with losses */
} rovit_eval_batch;
typedef struct rovit_eval_final {
  int n, num_classes, n_bins, n_loss_rows;
  const float* probs; const int* pred; const int* label; const float* sev_pred; const float* sev_true;
  const float* loss_table;          /* required when n_loss_rows > 0 */
  const double* bin_edges;          /* n_bins + 1 */
  unsigned int* rank_counts;        /* workspace, 4 n */
  double* partials;                 /* workspace, rovit_eval_partials_doubles(n) */
  void* result;                     /* ROVIT_EVAL_RESULT_WORDS 8-byte words */
} rovit_eval_final;
size_t rovit_eval_partials_doubles(int n);
int rovit_eval_accumulate(const rovit_eval_batch* p, rovit_stream_t stream);
int rovit_eval_finalize(const rovit_eval_final* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Non-parametric bootstrap of that score card (eval_bootstrap.hip): what the reference's ablation table (experiments/ablation.py:
 * get_component_importance, the "delta Acc" column) lacks -- an interval per metric and, through equal draws for two models, a paired test.
 * rovit_eval_bootstrap reads the accumulator's record arrays and the `less` counts the finalise left in rank_counts (words [0, n) of
 * sev_true, [2n, 3n) of sev_pred), so rovit_eval_finalize must have run on the same rows first.
 * Draw j of replicate r: Philox4x32-10, key = seed, counter = (j / 4, r, ROVIT_EVAL_BOOT_STREAM, 0); word j % 4 gives
 *   idx = (word * n) >> 32 in 64-bit arithmetic (bias at most n / 2^32).  A function of (seed, r, j, n) alone: two accumulators of the
 *   same length resample the same rows.
 * Stratified (perm and starts both non-NULL): perm is a permutation of the rows grouped by true class, rows with a bad label last;
 *   starts holds the C + 2 segment starts (starts[0] = 0, starts[C + 1] = n).  Draw j belongs to the segment s that contains j and picks
 *   perm[starts[s] + ((word * n_s) >> 32)], n_s the segment's length: every replicate has the data's class supports.
 * Ranks without a sort: with H[less[idx_j]] += 1 over the draws and P the exclusive prefix sum of H, the doubled tie-averaged rank of draw
 *   j inside the resample is 2 P[v] + H[v] + 1, v = less[idx_j] (less[i] is the first sorted slot of row i's tie group).
 * table (num_resamples, ROVIT_EVAL_BOOT_COLS) doubles, row r from replicate r's sums with the arithmetic of rovit_hip/evaluation.py
 *   (metrics_from_block, f1_averages): accuracy, macro F1 (over the classes present in that replicate's labels or predictions), weighted
 *   F1 (percent), MAE, Spearman's rho (NaN for a constant column or any non-finite value), Brier, ECE, then per class c precision,
 *   recall, F1 (percent) at ROVIT_EVAL_BOOT_PRECISION / _RECALL / _F1 + c (0 for c >= C); zero division gives 0; the last column is 0.
 * blocks, when not NULL: (num_resamples, ROVIT_EVAL_RESULT_WORDS) 8-byte words, replicate r's full result block in the ROVIT_EVAL_*
 *   layout, every word written (unwritten words and the loss sums 0; the rank sums 0 beside a non-finite severity).
 * Integers are added with integer atomics; every floating sum follows an order fixed by (n, the workgroup size, the draws): table and
 * blocks are bit-identical from run to run, for every grid and on both sides of the threshold below.
 * H lives in LDS for n <= ROVIT_EVAL_BOOT_LDS_ROWS.  Above it each workgroup uses 2 n words of `workspace`
 * (rovit_eval_bootstrap_workspace_bytes(n, num_resamples) bytes), and the grid is capped at ROVIT_EVAL_BOOT_WORKSPACE_GRID workgroups:
 * 1 GiB at the row limit.  max_workgroups > 0 lowers the grid further (one workgroup then serves several replicates in turn).
 * Limits: those of the finalise; 1 <= num_resamples <= ROVIT_EVAL_BOOT_MAX_RESAMPLES.  A bad descriptor is refused before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_EVAL_BOOT_STREAM 0x426F6F74u      /* "Boot": counter word 2, apart from the dropout and augmentation streams */
#define ROVIT_EVAL_BOOT_LDS_ROWS 16384
#define ROVIT_EVAL_BOOT_WORKSPACE_GRID 128
#define ROVIT_EVAL_BOOT_MAX_RESAMPLES 65536
enum {
  ROVIT_EVAL_BOOT_ACCURACY = 0, ROVIT_EVAL_BOOT_MACRO_F1 = 1, ROVIT_EVAL_BOOT_WEIGHTED_F1 = 2, ROVIT_EVAL_BOOT_MAE = 3,
  ROVIT_EVAL_BOOT_RHO = 4, ROVIT_EVAL_BOOT_BRIER = 5, ROVIT_EVAL_BOOT_ECE = 6, ROVIT_EVAL_BOOT_PRECISION = 7,
  ROVIT_EVAL_BOOT_RECALL = 15, ROVIT_EVAL_BOOT_F1 = 23, ROVIT_EVAL_BOOT_COLS = 32
};
typedef struct rovit_eval_boot {
  int n, num_classes, n_bins, num_resamples, max_workgroups;
  unsigned long long seed;
  const float* probs; const int* pred; const int* label; const float* sev_pred; const float* sev_true;
  const double* bin_edges;          /* n_bins + 1 */
  const unsigned int* rank_counts;  /* 4 n, as rovit_eval_finalize left it */
  const int* perm;                  /* (n) or NULL */
  const int* starts;                /* (C + 2) or NULL */
  unsigned int* workspace;          /* required for n > ROVIT_EVAL_BOOT_LDS_ROWS */
  size_t workspace_bytes;
  double* table;                    /* (num_resamples, ROVIT_EVAL_BOOT_COLS) */
  void* blocks;                     /* (num_resamples, ROVIT_EVAL_RESULT_WORDS) 8-byte words, or NULL */
} rovit_eval_boot;
size_t rovit_eval_bootstrap_workspace_bytes(int n, int num_resamples);
int rovit_eval_bootstrap(const rovit_eval_boot* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Selective prediction on that record (selective.hip): does the model know which rows it gets wrong?  The reference collects
 * all_uncertainties (evaluation/evaluator.py:35,64-65) and drops them; rovit_eval_selective is the first reader of the `uncertainty`
 * column.  It scores S score columns u (higher = less certain) against K risk columns l >= 0 of the same n rows, all fp32:
 *   scores  ROVIT_EVAL_SEL_CONFIDENCE 1 - max_c p (one IEEE subtraction)   _ENTROPY -sum_c p logf(p), a term of 0 at p == 0
 *           _SIGMA the recorded uncertainty   _SCORE_COLUMN score_column[s], n floats of the caller's
 *   risks   ROVIT_EVAL_SEL_ERROR 1.0f where pred != label   _ABS_ERR |sev_true - sev_pred| in fp32   _RISK_COLUMN risk_column[k]
 * Order: rows by ascending u; rows with equal u (==, so -0 equals +0) form a tie group [g, g + m) of sorted slots, and every row of a
 *   group counts with the group's mean risk (the expectation over random tie-breaking: the result cannot depend on the row order).
 *   With Pref[k] the fp64 sum of the first k sorted risks (ties in row order), the selective risk at k kept rows, g < k <= g + m, is
 *   r_k = (Pref[g] + (k - g) (Pref[g + m] - Pref[g]) / m) / k.
 * Ranks are counted, not sorted, every one of the S + K columns once: less_i = #{x_j < x_i}, eq_i = #{x_j == x_i},
 *   before_i = #{j < i : x_j == x_i}; row i sits in sorted slot less_i + before_i and its group is [less_i, less_i + eq_i).
 * result, ROVIT_EVAL_SEL_WORDS(S, K, P) 8-byte words with P = num_coverages and k_p = ceil(p n / P) in integers, p = 1..P:
 *   int64  [ROVIT_EVAL_SEL_NONFINITE_KEYS] non-finite score values   [_NONFINITE_RISKS], [_NEGATIVE_RISKS] of the risk values
 *          [_BAD_LABELS] recorded labels of -1   [_N]   (words up to ROVIT_EVAL_SEL_HEADER are 0)
 *   double per risk k at ROVIT_EVAL_SEL_HEADER + k (2 + P): mean = r_n, oracle_aurc (the risk ordered by itself), oracle_curve[P]
 *          per (score s, risk k) behind the risks at (s K + k)(1 + P): aurc = (1/n) sum_k r_k, curve[p] = r_{k_p}
 *          per score s behind the pairs at s P: thresholds[p] = the score value in sorted slot k_p - 1, widened
 * keys_out (S, n) and risks_out (K, n), when not NULL, receive the fp32 columns that were ranked.
 * Integers are added with integer atomics; the prefix sums and sum_k r_k run over 256-slot chunks in a fixed tree inside and across
 * chunks, and no floating-point atomic is used: the block is bit-identical from run to run, for every split of the rows into batches
 * and for every grid (max_workgroups > 0 caps the grid of every kernel; a workgroup then serves several work items in turn).
 * The whole block is zeroed first.  workspace: rovit_eval_selective_workspace_bytes(n, S, K) bytes, 16-byte aligned (0 for sizes
 * outside the limits).  With a non-finite key the order is undefined; the counters say so and the other words are then meaningless.
 * Limits: 1 <= n <= ROVIT_EVAL_MAX_ROWS, 1 <= S <= 8, 1 <= K <= 4, 1 <= P <= 256.  A bad descriptor is refused before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_EVAL_SEL_MAX_SCORES 8
#define ROVIT_EVAL_SEL_MAX_RISKS 4
#define ROVIT_EVAL_SEL_MAX_COVERAGES 256
enum { ROVIT_EVAL_SEL_CONFIDENCE = 0, ROVIT_EVAL_SEL_ENTROPY = 1, ROVIT_EVAL_SEL_SIGMA = 2, ROVIT_EVAL_SEL_SCORE_COLUMN = 3 };
enum { ROVIT_EVAL_SEL_ERROR = 0, ROVIT_EVAL_SEL_ABS_ERR = 1, ROVIT_EVAL_SEL_RISK_COLUMN = 2 };
enum {
  ROVIT_EVAL_SEL_NONFINITE_KEYS = 0, ROVIT_EVAL_SEL_NONFINITE_RISKS = 1, ROVIT_EVAL_SEL_NEGATIVE_RISKS = 2, ROVIT_EVAL_SEL_BAD_LABELS = 3,
  ROVIT_EVAL_SEL_N = 4, ROVIT_EVAL_SEL_HEADER = 8
};
#define ROVIT_EVAL_SEL_WORDS(S, K, P) \
  ((size_t)ROVIT_EVAL_SEL_HEADER + (size_t)(K) * (2 + (P)) + (size_t)(S) * (K) * (1 + (P)) + (size_t)(S) * (P))
typedef struct rovit_eval_sel {
  int n, num_classes, num_scores, num_risks, num_coverages, max_workgroups;
  int score_kind[ROVIT_EVAL_SEL_MAX_SCORES];
  int risk_kind[ROVIT_EVAL_SEL_MAX_RISKS];
  const float* score_column[ROVIT_EVAL_SEL_MAX_SCORES];   /* (n) each; read for ROVIT_EVAL_SEL_SCORE_COLUMN only */
  const float* risk_column[ROVIT_EVAL_SEL_MAX_RISKS];     /* (n) each; read for ROVIT_EVAL_SEL_RISK_COLUMN only */
  const float* probs; const int* pred; const int* label; const float* sev_pred; const float* sev_true; const float* uncertainty;
  void* workspace;
  size_t workspace_bytes;
  void* result;                      /* ROVIT_EVAL_SEL_WORDS(S, K, P) 8-byte words */
  float* keys_out;                   /* (S, n) or NULL */
  float* risks_out;                  /* (K, n) or NULL */
} rovit_eval_sel;
size_t rovit_eval_selective_workspace_bytes(int n, int num_scores, int num_risks);
int rovit_eval_selective(const rovit_eval_sel* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Post-hoc calibration on that record (calibrate.hip): the first code here that ACTS on the score card.  rovit_eval_calibrate fits
 * one temperature for the classifier (Guo et al. 2017) and one scale for the Gaussian head's sigma (Levi et al. 2019; Laves et al.
 * 2020) on the n recorded rows, and counts the observed coverage of the central Gaussian intervals (Kuleshov et al. 2018).
 * Log-probabilities: l[i,c] = max(log((double)probs[i,c]), ROVIT_EVAL_CAL_LOG_FLOOR = ln 2^-100); the clamp is part of the definition
 *   (a bf16 model records exact zeros).  Rows with label -1 are left out of the classification part and counted.
 * Temperature: with beta = 1/T, u = ln beta, w = softmax(beta l[i,:]) the fit is a root search on
 *   g(u) = sum_i (sum_c w[i,c] l[i,c] - l[i,y_i]), non-decreasing in u (the NLL's derivative in beta), over T in [1/32, 32]:
 *   ROVIT_EVAL_CAL_ROUNDS rounds of ROVIT_EVAL_CAL_CANDIDATES candidates u_j = lo + (hi - lo) (j / 63), u_63 = hi exactly; round 0 spans
 *   [-ln 32, ln 32]; there g(u_0) >= 0 ends the search at T = 32 (_AT_MAX) and no g(u_j) >= 0 at T = 1/32 (_AT_MIN); otherwise, and in
 *   every later round, j* is the first j >= 1 with g(u_j) >= 0 (63 if none) and the next bracket is [u_{j*-1}, u_{j*}].  u* is the secant
 *   point of the last bracket (lo when both g are equal), _INTERIOR.  The bracket's g values are the bits an earlier round computed
 *   at the same u, so g(lo) < 0 <= g(hi) holds in every round and u* lies inside a bracket 2 ln 32 / 63^4 wide.
 * Sigma scale: rows with a non-finite or non-positive sigma, or a non-finite mu or sev_true, are left out and counted; for the rest
 *   d = (double)sev_true - (double)mu, z = d / sigma; the block holds sum z^2 and sum ln sigma (s = sqrt(mean z^2) is the host's).
 * Coverage: count[k] = #{|d| <= half_widths[k] * (double)sigma}, one subtraction, one multiplication, one compare: exact integers.
 * result, ROVIT_EVAL_CAL_WORDS(L) 8-byte words, L = num_levels:
 *   int64  [ROVIT_EVAL_CAL_N_VALID] rows with a label in [0, C)   [_BAD_LABELS]   [_N_REG] rows of the regression part   [_BAD_SIGMA]
 *          [_STATUS]   [_N]   [ROVIT_EVAL_CAL_COVERAGE + k] coverage counts
 *   double [_U] u* = -ln T*   [_NLL] sum_i NLL_i at T = 1   [_NLL_CAL] at T*   [_G_LO], [_G_HI] g at the ends of the last bracket
 *          [_U_LO], [_U_HI] the last bracket   [_SUM_Z2]   [_SUM_LOG_SIGMA]
 * The search kernel gives every lane of a wave one candidate: a workgroup stages a 256-row chunk as fp64 l plus the label in LDS
 * (16 KB at 8 classes), each of its four waves walks 64 of those rows, every lane reads the same LDS address (a broadcast) and keeps
 * its own candidate's fp64 sum; waves, then chunks, are folded in a fixed order by a one-workgroup step kernel that applies the
 * bracket rule to a device-resident state the next round's launch reads.  The NLLs come from a fifth launch of the same row code.
 * Chunks depend on n alone, integers are added with integer atomics and no floating-point atomic is used: the block is bit-identical
 * from run to run, for every split of the rows into batches and for every grid (max_workgroups > 0 caps it).  No cooperative launch:
 * rounds are separate launches, and their number does not depend on the data.  The whole block is zeroed first.
 * mu and uncertainty both NULL: no regression part (its words stay 0).  workspace: rovit_eval_calibrate_workspace_bytes(n, C) bytes,
 * 16-byte aligned (0 for sizes outside the limits).  Limits: those of the finalise; 0 <= L <= ROVIT_EVAL_CAL_MAX_LEVELS.
 * rovit_eval_recalibrate applies a calibration in ONE elementwise launch: probs_out = fp32(softmax(beta l)) with the l above,
 * uncertainty_out = fp32(sigma_scale * (double)uncertainty) (both NULL: not touched).  A bad descriptor is refused before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_EVAL_CAL_ROUNDS 4
#define ROVIT_EVAL_CAL_CANDIDATES 64
#define ROVIT_EVAL_CAL_MAX_LEVELS 64
#define ROVIT_EVAL_CAL_LOG_FLOOR (-69.314718055994530942)    /* ln 2^-100 */
#define ROVIT_EVAL_CAL_U_MAX 3.4657359027997265471           /* ln 32 */
enum { ROVIT_EVAL_CAL_INTERIOR = 0, ROVIT_EVAL_CAL_AT_MIN = 1, ROVIT_EVAL_CAL_AT_MAX = 2 };
enum {
  ROVIT_EVAL_CAL_N_VALID = 0, ROVIT_EVAL_CAL_BAD_LABELS = 1, ROVIT_EVAL_CAL_N_REG = 2, ROVIT_EVAL_CAL_BAD_SIGMA = 3,
  ROVIT_EVAL_CAL_STATUS = 4, ROVIT_EVAL_CAL_N = 5,
  ROVIT_EVAL_CAL_U = 8, ROVIT_EVAL_CAL_NLL = 9, ROVIT_EVAL_CAL_NLL_CAL = 10, ROVIT_EVAL_CAL_G_LO = 11, ROVIT_EVAL_CAL_G_HI = 12,
  ROVIT_EVAL_CAL_U_LO = 13, ROVIT_EVAL_CAL_U_HI = 14, ROVIT_EVAL_CAL_SUM_Z2 = 15, ROVIT_EVAL_CAL_SUM_LOG_SIGMA = 16,
  ROVIT_EVAL_CAL_COVERAGE = 24
};
#define ROVIT_EVAL_CAL_WORDS(L) ((size_t)ROVIT_EVAL_CAL_COVERAGE + (size_t)(L))
typedef struct rovit_eval_cal {
  int n, num_classes, num_levels, max_workgroups;
  const float* probs; const int* label; const float* sev_true; const float* uncertainty;
  const float* mu;                   /* (n), or NULL together with uncertainty */
  const double* half_widths;         /* (num_levels) on the device; required when num_levels > 0 and the regression part exists */
  void* workspace;
  size_t workspace_bytes;
  void* result;                      /* ROVIT_EVAL_CAL_WORDS(num_levels) 8-byte words */
} rovit_eval_cal;
typedef struct rovit_eval_recal {
  int n, num_classes;
  double beta, sigma_scale;
  const float* probs; const float* uncertainty;
  float* probs_out; float* uncertainty_out;
} rovit_eval_recal;
size_t rovit_eval_calibrate_workspace_bytes(int n, int num_classes);
int rovit_eval_calibrate(const rovit_eval_cal* p, rovit_stream_t stream);
int rovit_eval_recalibrate(const rovit_eval_recal* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-edge activation statistics of one KAN layer over a data set (kan_stats.hip): what the edge functions of models/kan.py:70-95 do
 * ON DATA, where KANLayer.plot_activation (:97-114) and explainability/kan_viz.py only draw a few of them over [-1, 1].
 * For the layer's n input rows x (n, in_f), with s_ij(v) = sum_k spline_w[i,j,k] B_k(tanh v), phi_ij(v) = lin_w[j,i] v + s_ij(v) and
 * z_nj = lin_b[j] + sum_i phi_ij(x_ni), rovit_kan_edge_stats writes this layer's section of the caller's result buffer,
 * rovit_kan_stats_words(in_f, out_f, n_knots) 8-byte words with E = in_f * out_f:
 *   double [q E + i out_f + j], q = ROVIT_KAN_STATS_SUM / _SQ / _ABS / _SPLINE_ABS / _LINEAR_ABS: sum phi, sum phi^2, sum |phi|, sum |s|
 *          and |lin_w[j,i]| sum |x_i| (the linear term's L1 share) of edge (i, j)
 *   double [5E + j], [5E + out_f + j]: sum z_j, sum z_j^2         double [5E + 2 out_f + i]: sum |x_i|
 *   int64  [5E + 2 out_f + in_f + i n_knots + t]: rows whose tanh(x_i) lies in knot interval t, the index the forward's basis search
 *          finds after its clamp (t >= n_knots - 4: the truncated basis is zero there; t = n_knots - 1 only for tanh == knots[last])
 *   int64  [.. + in_f n_knots]: non-finite inputs      int64 [.. + 1]: n
 * The basis, the interval and the cutoff decisions are the forward kernels' own (kan_device.h).  No (n, in, out) intermediate exists: the
 * sums are kept in registers as fp32 over at most 16 rows and folded into fp64, then added over a partition of the rows that depends on n
 * and the layer shape only, in a fixed order: the section is bit-identical from run to run, and the error does not grow with n.
 * Integers are added with integer atomics.  The section is zeroed first.  Shapes: in_f, out_f >= 1, 5 <= n_knots <= 64.
 * partials: device workspace of rovit_kan_stats_partials_doubles(n, in_f, out_f, n_knots) doubles.
 * rovit_kan_curves: ys (in_f, out_f, num_points) = s_ij(xs[p]) (+ lin_w[j,i] xs[p] when lin_w is not NULL) with xs the NORMALISED
 * coordinate (no tanh), plot_activation's convention, for every edge in one launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_KAN_STATS_MAX_ROWS (1 << 22)
enum { ROVIT_KAN_STATS_SUM = 0, ROVIT_KAN_STATS_SQ = 1, ROVIT_KAN_STATS_ABS = 2, ROVIT_KAN_STATS_SPLINE_ABS = 3, ROVIT_KAN_STATS_LINEAR_ABS = 4 };
typedef struct rovit_kan_stats {
  int n, in_f, out_f, n_knots;
  const float* x;                   /* (n, in_f) */
  const float* spline_w;            /* (in_f, out_f, n_knots - 4) */
  const float* knots;               /* (n_knots) */
  const float* lin_w;               /* (out_f, in_f) */
  const float* lin_b;               /* (out_f) */
  double* partials;                 /* workspace */
  void* result;                     /* this layer's section */
} rovit_kan_stats;
size_t rovit_kan_stats_words(int in_f, int out_f, int n_knots);
size_t rovit_kan_stats_partials_doubles(int n, int in_f, int out_f, int n_knots);
int rovit_kan_edge_stats(const rovit_kan_stats* p, rovit_stream_t stream);
int rovit_kan_curves(const float* xs, const float* spline_w, const float* knots, const float* lin_w, float* ys, int in_f, int out_f,
                     int n_knots, int num_points, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * KAN grid extension (kan_grid.hip): move every edge spline of one layer from its stored knots k (nk of them, nb = nk - 4) to a new
 * uniform knot vector k' (nk', nb' = nk' - 4) by least squares on data.  models/kan.py:8-44 fixes the grid at construction; the
 * definitions below are this repository's own ("parity unpinned").  b(v), b'(v): the truncated cubic bases of the
 * two grids as the forward evaluates them (kan_device.h), v = tanh(x).
 *
 * rovit_kan_regrid_moments: for every input i over its FINITE rows x_ni (N_i of them; a non-finite x_ni is skipped for input i and
 * counted) the sums  G_i = sum_n b' b'^T,  M_i = sum_n b' b^T,  O_i = sum_n b b^T  into the moment block,
 * rovit_kan_regrid_moment_words(in_f, nk, nk') 8-byte words:
 *   double G [i][a][d], a < nb', d < 4: entry (a, a - d) of G_i (0 for a < d)        at 0
 *   double M [i][a][b], a < nb', b < nb                                              at 4 in_f nb'
 *   double O [i][b][d], b < nb, d < 4                                                at 4 in_f nb' + in_f nb' nb
 *   int64  N_i [i], then non-finite inputs [i]                                       at .. + 4 in_f nb
 * Each (row, input) takes tanhf and the two bases once; products are summed in fp32 over at most 16 rows and folded into fp64; the rows
 * are cut into ranges of whole 256-row chunks, a function of n and in_f only, and the ranges are added in order: the block is
 * bit-identical from run to run.  Integers are added with integer atomics.  No (n, in, nb) tensor exists.
 * workspace: rovit_kan_regrid_workspace_bytes(n, in_f, nk, nk') bytes, 8-byte aligned (0 for sizes outside the limits).  It holds
 * R in_f (2 nb' + 2 nb - 1) blocks of 16 doubles with R <= 64 row ranges and R in_f < 1024 + in_f: at most (1024 + in_f) * 30 592 bytes,
 * whatever n is.
 *
 * rovit_kan_regrid_solve: per input, in fp64,  A = G_i / N_i + prior_g,  delta = 2^-40 tr(A) / nb' added to the diagonal entries that
 * are <= delta (the bases neither the data nor D reach: their row of M is zero and they get coefficient 0; every other entry is left
 * exact), Cholesky,  T_i = A^-1 (M_i / N_i + prior_m)  and  c'_ij = T_i c_ij  for every output j (N_i = 0: the priors alone).  prior_g (nb', nb')
 * and prior_m (nb', nb) are the caller's (eps / L) int_D b' b'^T dv and (eps / L) int_D b' b^T dv, row-major fp64 on the device.
 * It writes spline_w_new (in_f, out_f, nb') and the diagnostics block, rovit_kan_regrid_diag_words(in_f, out_f) 8-byte words, E = in_f out_f:
 *   double fit_ms [i][j] = c'^T G c' - 2 c'^T M c + c^T O c  (data parts / N_i, c' before its rounding to fp32; may be -0 within rounding)
 *   double target_ms [i][j] = c^T O c        at E          double pivot ratio [i] (smallest / largest Cholesky pivot)   at 2E
 *   int64 N_i [i]  at 2E + in_f      int64 non-finite inputs [i]  at 2E + 2 in_f      int64 status  at 2E + 3 in_f
 * status counts the inputs whose factorisation met a non-positive pivot; their pivot ratio is 0 and their new coefficients are 0.
 *
 * Limits of both: in_f, out_f >= 1, 8 <= nk, nk' <= 64, 1 <= n <= ROVIT_KAN_STATS_MAX_ROWS; anything else is ROVIT_ERR_SHAPE before
 * any launch, a missing pointer ROVIT_ERR_NULL.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rovit_kan_regrid {
  int n, in_f, n_knots_old, n_knots_new;
  const float* x;                   /* (n, in_f) inputs of the layer */
  const float* knots_old;           /* (n_knots_old) */
  const float* knots_new;           /* (n_knots_new) */
  void* workspace;
  size_t workspace_bytes;
  void* moments;                    /* the moment block */
} rovit_kan_regrid;
typedef struct rovit_kan_regrid_fit {
  int in_f, out_f, n_knots_old, n_knots_new;
  const void* moments;              /* rovit_kan_regrid_moments' block */
  const double* prior_g;            /* (nb', nb') */
  const double* prior_m;            /* (nb', nb) */
  const float* spline_w;            /* (in_f, out_f, nb) */
  float* spline_w_new;              /* (in_f, out_f, nb') */
  void* diagnostics;                /* the diagnostics block */
} rovit_kan_regrid_fit;
size_t rovit_kan_regrid_moment_words(int in_f, int n_knots_old, int n_knots_new);
size_t rovit_kan_regrid_diag_words(int in_f, int out_f);
size_t rovit_kan_regrid_workspace_bytes(int n, int in_f, int n_knots_old, int n_knots_new);
int rovit_kan_regrid_moments(const rovit_kan_regrid* p, rovit_stream_t stream);
int rovit_kan_regrid_solve(const rovit_kan_regrid_fit* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-sample augmentation of a device-resident uint8 image store (augment_batch.hip).  Serves the batches of
 * training/trainer.py:79-82 (`images, class_labels, severity_labels`, moved with .to(device)) and the loaders scripts/train.py:73-84
 * builds with create_dataloaders(..., augmented_transform=, original_transform=): the data set is decoded ONCE and kept on the device
 * as uint8, and ONE launch per batch gathers by index, draws each sample's augmentation, resamples, colour-transforms, normalises and
 * writes the fp32 NCHW batch the backbone reads.  The reference's data/transforms.py is not in its checkout: the transform is this
 * repository's definition ("parity unpinned"), stated in full in rovit_hip/augment.py.
 *   src (n_images, 3, src_h, src_w) uint8   indices (batch) int64 into the store   out (batch, 3, out_h, out_w) fp32
 *   row of sample n, 12 floats: [flip_h, flip_v, area, log_ratio, ux, uy, theta, brightness, contrast, saturation, hue, 0]
 * Geometry: r = exp(log_ratio), w = min(Ws, Ws sqrt(area r)), h = min(Hs, Hs sqrt(area / r)), cx = ux (Ws - w) + w/2, cy likewise;
 *   dx = ((j + .5)/Wo - .5) w (1 - 2 flip_h), dy = ((i + .5)/Ho - .5) h (1 - 2 flip_v), sx = cx + cos dx - sin dy - .5,
 *   sy = cy + sin dx + cos dy - .5, clamped to the image; bilinear on u8/255 with the upper taps clamped to the last row / column
 *   (= grid_sample(mode='bilinear', padding_mode='border', align_corners=False)); no antialiasing.
 * Colour: A = T^-1 diag(1, saturation Rot(2 pi hue)) T with T the NTSC RGB->YIQ matrix; z = clamp(brightness (.5 + contrast (A v - .5)),
 *   0, 1); out = (z - mean_c) / std_c with the ImageNet constants.
 * params != NULL: the rows are read from it.  params == NULL: each row is drawn from Philox4x32-10, key = seed, counter =
 *   (index in the STORE, r, epoch lo, epoch hi), r = 0, 1, 2, u = (word >> 8) 2^-24:  r = 0: flip_h = u < p_hflip, flip_v = u < p_vflip,
 *   area = scale_lo + u (scale_hi - scale_lo), log_ratio likewise;  r = 1: ux, uy, theta = (2u - 1) theta_max, brightness = 1 + (2u - 1)
 *   jitter;  r = 2: contrast, saturation likewise, hue = (2u - 1) hue jitter.  An image's row depends on (index, seed, epoch) alone, and
 *   a pixel's arithmetic on its row alone: out rows are bit-identical for every batch size, order and split.
 * params_out != NULL: the rows used are written there (batch, 12).
 * An index outside [0, n_images) is not dereferenced: that sample's output and params_out row are NaN.
 * Refused before any launch: null pointers, out overlapping src, out_w % 4 != 0, out not 16-byte aligned, an empty store or batch,
 * 0 < scale_lo <= scale_hi <= 1 violated, probabilities outside [0, 1], unordered or negative ranges (config is checked when given;
 * it may be NULL only with params).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rovit_augment_config {
  float p_hflip, p_vflip;              /* probabilities */
  float scale_lo, scale_hi;            /* crop area as a fraction of the source */
  float log_ratio_lo, log_ratio_hi;    /* log of the crop's aspect ratio */
  float theta_max;                     /* radians */
  float brightness, contrast, saturation, hue;   /* jitter half-widths */
} rovit_augment_config;
int rovit_augment_batch(const unsigned char* src, int n_images, int src_h, int src_w, const long long* indices, int batch,
                        const float* params, float* params_out, const rovit_augment_config* config, unsigned long long seed,
                        unsigned long long epoch, float* out, int out_h, int out_w, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Image corruptions of the same store (corrupt.hip): the eleven corruptions of a corruption-robustness benchmark (Hendrycks &
 * Dietterich, ICLR 2019) at the store's own resolution, ONE launch per batch; the definitions, the severity tables and the draw rule are
 * stated in full in rovit_hip/corrupt.py ("parity unpinned" where ImageNet-C has no parameter of the same meaning).
 *   src (n_images, 3, h, w) uint8, h, w >= 8   indices (batch) int64 into the store   out (batch, 3, h, w) fp32
 *   out_u8 (batch, 3, h, w) uint8 or NULL
 * All arithmetic is on v = u8 / 255; the result is z = clamp(., 0, 1), out = (z - mean_c) / std_c with the ImageNet constants (no
 * quantisation), out_u8 = floor(255 z + 0.5).  desc->param is sigma (gaussian_noise, gaussian_blur), c (shot_noise, brightness,
 * contrast), p (impulse_noise), r (defocus_blur), R (motion_blur, integer), s (saturate), b (pixelate, integer) or the quality (jpeg,
 * integer).  Draws: Philox4x32-10, key = desc->seed, counter = (pixel index y w + x, index in the STORE, kind, 0); the motion blur's angle
 * from the counter (index in the STORE, 0, kind, 1).  Output rows are bit-identical for every batch size, order and split.
 * rovit_corrupt_stats: sums (batch, 3) int64 = the integer sum of each sample's three uint8 planes (fixed-order integer reduction; 0 for an
 * index outside the store); rovit_corrupt_batch reads them for ROVIT_CORRUPT_CONTRAST alone (`sums` may be NULL otherwise).
 * An index outside [0, n_images) is not dereferenced: that sample's output is NaN (its out_u8 rows 0).
 * Refused before any launch: null pointers, out or out_u8 overlapping src, a side below 8, an unknown kind, a parameter outside its range
 * (stencil radii above ROVIT_CORRUPT_MAX_RADIUS: gaussian ceil(3 sigma), defocus r, motion R + 1).
 * ------------------------------------------------------------------------------------------------------------ */
enum {
  ROVIT_CORRUPT_GAUSSIAN_NOISE = 0, ROVIT_CORRUPT_SHOT_NOISE = 1, ROVIT_CORRUPT_IMPULSE_NOISE = 2, ROVIT_CORRUPT_GAUSSIAN_BLUR = 3,
  ROVIT_CORRUPT_DEFOCUS_BLUR = 4, ROVIT_CORRUPT_MOTION_BLUR = 5, ROVIT_CORRUPT_BRIGHTNESS = 6, ROVIT_CORRUPT_CONTRAST = 7,
  ROVIT_CORRUPT_SATURATE = 8, ROVIT_CORRUPT_PIXELATE = 9, ROVIT_CORRUPT_JPEG = 10, ROVIT_CORRUPT_COUNT = 11
};
#define ROVIT_CORRUPT_MAX_RADIUS 18
typedef struct rovit_corruption {
  int kind;                  /* ROVIT_CORRUPT_* */
  float param;
  unsigned long long seed;
} rovit_corruption;
int rovit_corrupt_stats(const unsigned char* src, int n_images, int src_h, int src_w, const long long* indices, int batch, long long* sums,
                        rovit_stream_t stream);
int rovit_corrupt_batch(const unsigned char* src, int n_images, int src_h, int src_w, const long long* indices, int batch,
                        const rovit_corruption* desc, const long long* sums, float* out, unsigned char* out_u8, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Feature-space density (density.hip): is a feature row anything like the training features?  Every score of the score card above reads
 * the heads; these three entries read outputs['features'] (models/rovit_kan.py) alone.  Mahalanobis distance to class-conditional
 * Gaussians with a tied covariance (Lee et al., NeurIPS 2018), its relative form (Ren et al. 2021), and the AUROC / AUPR / FPR@TPR of
 * an in-distribution against an out-of-distribution score population.  All matrix work is exact fp32 (v_mfma_f32_32x32x2_f32).
 *
 * rovit_density_moments: features (n, E) fp32 row-major, labels (n) int32, C classes.  A row whose label lies outside [0, C) is left out
 * and counted in BAD_LABELS; a row with a label inside and a non-finite feature is left out and counted in BAD_ROWS; the others are the
 * n_valid valid rows.  result, ROVIT_DENSITY_WORDS(E, C) 8-byte words:
 *   int64  [ROVIT_DENSITY_N]  [_N_VALID]  [_BAD_LABELS]  [_BAD_ROWS]  [_COUNTS + c] valid rows of class c (words up to _HEADER are 0)
 *   double at _HEADER: mean[c][e] (C, E), 0 for an empty class; then the mean of the valid rows (E); then the pooled within-class
 *          scatter S_w[a][b] = sum_i (f_ia - mu32[y_i][a]) (f_ib - mu32[y_i][b]) (E, E), mu32 the class mean rounded to fp32, exactly
 *          symmetric (the upper tile triangle is computed and mirrored)
 * A chunk is R = ROVIT_DENSITY_CHUNK_ROWS * ceil(n / (256 ROVIT_DENSITY_CHUNK_ROWS)) consecutive rows: 256 rows up to n = 65536, never more
 * than 256 chunks.  Sums: fp64 in row order inside a chunk, chunks in order.  Scatter: fp32 centring (one subtraction), per chunk and
 * element one fp32 fma chain over the chunk's rows in order on the matrix instruction, chunk partials added in fp64 in chunk order.  No
 * floating-point atomic: the block is bit-identical from run to run, for every way the rows arrived and for every grid (max_workgroups
 * > 0 caps the grid of every kernel; a workgroup then serves several chunks in turn).  Every word of the block is written.
 * workspace: rovit_density_workspace_bytes(n, E, C) bytes, 16-byte aligned (0 for sizes outside the limits).
 * Limits: E a multiple of 32 in 32..256, 2 <= C <= ROVIT_EVAL_MAX_CLASSES, 1 <= n <= ROVIT_KAN_STATS_MAX_ROWS; features 16-byte aligned.
 *
 * rovit_density_score: for the rows f of features (B, E), any B >= 1, with z = W f and z0 = W0 f (W = whitening, W0 =
 * background_whitening, both (E, E) row-major and LOWER-TRIANGULAR: the tiles of 32 x 32 right of the diagonal tile are never read and
 * the entries above the diagonal inside the diagonal tile must be zero), M = class_means (C, E) and m0 = background_mean (E) in the
 * whitened space:
 *   class_distances (B, C) d_c = ||z - M_c||^2   background_distance (B) d0 = ||z0 - m0||^2   mahalanobis (B) min_c d_c
 *   nearest_class (B) int32, the lowest index on a tie   relative_mahalanobis (B) min_c (d_c - d0)
 *   with cls_logits (B, C) not NULL: energy (B) = -logsumexp(l) and max_prob_score (B) = 1 - max softmax(l), evaluated in fp64 as
 *   -(m + log1p(r)) and r / (1 + r), m the first maximum and r the sum of exp(l_c - m) over the other classes, then rounded to fp32
 * One launch; a workgroup owns ROVIT_DENSITY_SCORE_TILE rows (the last tile may be partial), z never goes to memory.  z_a is one fp32
 * fma chain over k in a fixed order, d_c one fp32 fma chain over a in a fixed order: the same bits from run to run and for every grid.
 * Limits: E and C as above.  features and both whitening matrices 16-byte aligned.
 *
 * rovit_ood_metrics: scores_in (n_in) and scores_out (n_out) fp32, higher = more anomalous.  Ranks are counted, not sorted: for every row
 * x of either population less_in = #{in < x}, eq_in = #{in == x}, less_out, eq_out.  result, ROVIT_OOD_WORDS 8-byte words, zeroed first:
 *   int64  [ROVIT_OOD_N_IN]  [_N_OUT]  [_BAD] non-finite scores (the other words are then meaningless)
 *          [_TWO_U] sum over the out rows of 2 less_in + eq_in: AUROC = TWO_U / (2 n_in n_out) exactly
 *          [_K + l] k_l = min(max(ceil(tpr_levels[l] * n_in), 1), n_in), the product and ceil in fp64
 *          [_OUT_BELOW + l] #{out <= t_l}: FPR at TPR level l = OUT_BELOW / n_out
 *   double [_THRESHOLD + l] t_l, the k_l-th smallest in-distribution score (the in row with less_in < k_l <= less_in + eq_in), widened,
 *          -0 as +0
 *          [_AP_OUT_SUM] sum over the out rows of ge_out / (ge_out + ge_in), ge_* = #{* >= x}: AUPR with out as the positives = sum / n_out
 *          [_AP_IN_SUM] sum over the in rows of le_in / (le_in + le_out), le_* = #{* <= x}: AUPR with in as the positives = sum / n_in
 * Integers are added with integer atomics; the two fp64 sums run over 256-row chunks of the concatenation (in, out) in a fixed tree, the
 * chunk sums in a fixed order: bit-identical from run to run and for every grid (max_workgroups as above).
 * workspace: rovit_ood_metrics_workspace_bytes(n_in, n_out) bytes, 16-byte aligned (0 outside the limits).
 * Limits: n_in, n_out >= 1, n_in + n_out <= ROVIT_EVAL_MAX_ROWS, 0 <= num_levels <= ROVIT_OOD_MAX_LEVELS, 0 < level <= 1.
 * A bad descriptor is refused before any launch, by all three.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_DENSITY_CHUNK_ROWS 256
#define ROVIT_DENSITY_SCORE_TILE 64
enum {
  ROVIT_DENSITY_N = 0, ROVIT_DENSITY_N_VALID = 1, ROVIT_DENSITY_BAD_LABELS = 2, ROVIT_DENSITY_BAD_ROWS = 3, ROVIT_DENSITY_COUNTS = 4,
  ROVIT_DENSITY_HEADER = 16
};
#define ROVIT_DENSITY_WORDS(E, C) ((size_t)ROVIT_DENSITY_HEADER + ((size_t)(C) + 1) * (E) + (size_t)(E) * (E))
typedef struct rovit_density_fit {
  int n, embed, num_classes, max_workgroups;
  const float* features;             /* (n, embed) */
  const int* labels;                 /* (n) */
  void* workspace;
  size_t workspace_bytes;
  void* result;                      /* ROVIT_DENSITY_WORDS(embed, num_classes) 8-byte words */
} rovit_density_fit;
typedef struct rovit_density_scores {
  int batch, embed, num_classes, max_workgroups;
  const float* features;             /* (batch, embed) */
  const float* whitening;            /* (embed, embed), lower-triangular */
  const float* class_means;          /* (num_classes, embed), whitened */
  const float* background_whitening; /* (embed, embed), lower-triangular */
  const float* background_mean;      /* (embed), whitened */
  const float* cls_logits;           /* (batch, num_classes) or NULL */
  float* class_distances;            /* (batch, num_classes) */
  float* background_distance; float* mahalanobis; int* nearest_class; float* relative_mahalanobis;   /* (batch) each */
  float* energy; float* max_prob_score;                                                               /* (batch) each; with cls_logits */
} rovit_density_scores;
#define ROVIT_OOD_MAX_LEVELS 8
enum {
  ROVIT_OOD_N_IN = 0, ROVIT_OOD_N_OUT = 1, ROVIT_OOD_BAD = 2, ROVIT_OOD_TWO_U = 3, ROVIT_OOD_K = 4, ROVIT_OOD_THRESHOLD = 12,
  ROVIT_OOD_OUT_BELOW = 20, ROVIT_OOD_AP_OUT_SUM = 28, ROVIT_OOD_AP_IN_SUM = 29, ROVIT_OOD_WORDS = 32
};
typedef struct rovit_ood {
  int n_in, n_out, num_levels, max_workgroups;
  double tpr_levels[ROVIT_OOD_MAX_LEVELS];
  const float* scores_in; const float* scores_out;
  void* workspace;
  size_t workspace_bytes;
  void* result;                      /* ROVIT_OOD_WORDS 8-byte words */
} rovit_ood;
size_t rovit_density_workspace_bytes(int n, int embed, int num_classes);
int rovit_density_moments(const rovit_density_fit* p, rovit_stream_t stream);
int rovit_density_score(const rovit_density_scores* p, rovit_stream_t stream);
size_t rovit_ood_metrics_workspace_bytes(int n_in, int n_out);
int rovit_ood_metrics(const rovit_ood* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device radix sort of fp32 columns and the ranks that follow from it (sort_rank.hip; device functions in sort_device.h).  The
 * counting rank of the three score cards above is O(n^2); this is the O(n) path behind the same words, and the library's only sort.
 * Key of a value v: the order-preserving uint32 of v + 0.0f (sign bit flipped for v >= 0, all bits for v < 0), so -0 and +0 share a key;
 *   every NaN, of either sign and any payload, has the key 0xFFFFFFFF, which no number has: NaNs sort behind +inf.
 * Sorted element: the pair (key, row).  Its 64-bit form (key << 32) | row has no duplicates, so the ascending order is unique: any
 *   correct algorithm, grid and run gives the same bytes.  rovit_sort_f32 writes, per column c of n[c] rows,
 *   keys_sorted[c][n[c]] uint32 ascending and perm[c][n[c]] uint32, the row in each sorted slot: the STABLE argsort, NaN rows last.
 * Algorithm: LSD radix sort, four passes of 8 bits, each three launches on the caller's stream: a digit histogram per tile of
 *   ROVIT_SORT_TILE rows (LDS counters; the column's digit totals by integer atomics: only the sum matters), an exclusive scan of the
 *   (digit, tile) table, and a scatter that is stable inside the tile: a row's place among the tile's rows of its digit comes from wave
 *   ballots and a fixed walk over the tile's 32 (wave, round) groups, never from an atomic.  No kernel waits for another workgroup;
 *   every loop is bounded by n or a constant; every destination is checked against n before the store; integer compares only.
 *   Up to ROVIT_SORT_MAX_COLUMNS columns of individual lengths share the twelve launches.
 * Ranks: for row i with key k in slot s, less = lower_bound(k), eq = upper_bound(k) - less, before = s - less over the sorted keys;
 *   a NaN row gets less = eq = before = 0 and is counted for no other row.  These are the values the counting kernels produce
 *   (less = #{x_j < x_i}, eq = #{x_j == x_i}, before = #{j < i : x_j == x_i}, a NaN comparing false).  rovit_rank_f32 returns them with
 *   perm per column.  method: ROVIT_RANK_COUNT counts on rank_count.h's tile (perm[less + before] = row; NaN rows behind the numbers in
 *   row order, so perm equals the sort's), ROVIT_RANK_SORT sorts, ROVIT_RANK_AUTO sorts columns of at least ROVIT_RANK_SORT_ROWS rows
 *   (decided by the longest column of the call).  Both methods give the same words for every input.
 * rovit_eval_finalize_ex / rovit_eval_selective_ex / rovit_ood_metrics_ex: the three score cards with the rank step by `method`; every
 *   other launch and every result word is that of the plain entry point, which is the _ex call with ROVIT_RANK_COUNT and no workspace.
 *   rank_workspace (16-byte aligned, *_rank_workspace_bytes bytes; 0 outside the limits) is read only when the method resolves to
 *   ROVIT_RANK_SORT.  AUTO goes by n, and by n_in + n_out for the OOD card.  The blocks are byte-identical between the methods wherever
 *   the counting path is defined (rovit_eval_selective: every key a number; there only the counters agree otherwise).
 * workspace of rovit_sort_f32 / rovit_rank_f32: rovit_sort_workspace_bytes / rovit_rank_workspace_bytes bytes, 16-byte aligned.
 * Limits: 1 <= num_columns <= ROVIT_SORT_MAX_COLUMNS, 1 <= n[c] <= ROVIT_EVAL_MAX_ROWS; x 4-byte aligned, outputs 4-byte aligned.
 * max_workgroups > 0 caps every grid and changes no output.  A bad descriptor is refused before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
enum { ROVIT_RANK_AUTO = 0, ROVIT_RANK_COUNT = 1, ROVIT_RANK_SORT = 2 };
#define ROVIT_RANK_SORT_ROWS 32768                /* AUTO's threshold, measured: tools/time_rank.py, profiles/rank_time.jsonl, DESIGN.md section 2 */
#define ROVIT_SORT_MAX_COLUMNS 16
#define ROVIT_SORT_TILE 2048
typedef struct rovit_sort {
  int num_columns, max_workgroups;
  int n[ROVIT_SORT_MAX_COLUMNS];
  const float* x[ROVIT_SORT_MAX_COLUMNS];                /* (n[c]) each */
  unsigned int* keys_sorted[ROVIT_SORT_MAX_COLUMNS];     /* (n[c]) each */
  unsigned int* perm[ROVIT_SORT_MAX_COLUMNS];            /* (n[c]) each */
  void* workspace;
  size_t workspace_bytes;
} rovit_sort;
typedef struct rovit_rank {
  int num_columns, method, max_workgroups, reserved;
  int n[ROVIT_SORT_MAX_COLUMNS];
  const float* x[ROVIT_SORT_MAX_COLUMNS];                /* (n[c]) each */
  unsigned int* less[ROVIT_SORT_MAX_COLUMNS];            /* (n[c]) each, as eq, before and perm */
  unsigned int* eq[ROVIT_SORT_MAX_COLUMNS];
  unsigned int* before[ROVIT_SORT_MAX_COLUMNS];
  unsigned int* perm[ROVIT_SORT_MAX_COLUMNS];
  void* workspace;                                       /* read for ROVIT_RANK_SORT only */
  size_t workspace_bytes;
} rovit_rank;
size_t rovit_sort_workspace_bytes(const int* n, int num_columns);
int rovit_sort_f32(const rovit_sort* p, rovit_stream_t stream);
size_t rovit_rank_workspace_bytes(const int* n, int num_columns, int method);
int rovit_rank_f32(const rovit_rank* p, rovit_stream_t stream);
size_t rovit_eval_finalize_rank_workspace_bytes(int n);
int rovit_eval_finalize_ex(const rovit_eval_final* p, int method, void* rank_workspace, size_t rank_workspace_bytes, rovit_stream_t stream);
size_t rovit_eval_selective_rank_workspace_bytes(int n, int num_scores, int num_risks);
int rovit_eval_selective_ex(const rovit_eval_sel* p, int method, void* rank_workspace, size_t rank_workspace_bytes, rovit_stream_t stream);
size_t rovit_ood_metrics_rank_workspace_bytes(int n_in, int n_out);
int rovit_ood_metrics_ex(const rovit_ood* p, int method, void* rank_workspace, size_t rank_workspace_bytes, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Split conformal prediction on the evaluation record (conformal.hip; the score functions live in conformal_device.h and are shared
 * by the fit and the application).  rovit_eval_conformal fits the thresholds of M nonconformity scores at A levels for G groups
 * (G = 1: all rows with a label in [0, C); class_conditional: G = 1 + C, group 1 + c the rows of true class c).
 * Scores (fp32, every one normalised with v + 0.0f so that -0 becomes +0):
 *   _LAC 1 - p_y   _APS fma(-u, p_y, cum(y))   _RAPS fma(lambda, max(0, r(y) - raps_k), aps)   _KAN_ABS |sev_true - sev_pred|
 *   _MU_ABS |sev_true - mu|   _MU_SCALED |sev_true - mu| / sigma   _COLUMN score_column[m][i]
 *   The classes are ordered by p descending, ties by lower index first (an insertion sort in registers); r(c) is the 1-based rank,
 *   cum(c) the fp32 running sum in rank order up to and including c; a NaN probability makes the row's aps and raps NaN.
 *   u = 0 unless randomized; then w = word 0 of Philox4x32-10 with key = seed and counter (row_offset + i, 0, ROVIT_EVAL_CONF_STREAM, 0)
 *   and u = ((float)(w >> 8) + 0.5f) * 2^-24, two IEEE fp32 operations (the addition rounds to even from w >> 8 >= 2^23 on).
 * A row is valid for column m when its label is in [0, C), its score is finite and, for _MU_SCALED, sigma is finite and positive.
 * For entry e = (m G + g) A + a with n_g valid rows: k = n_g + 1 - floor((n_g + 1) alpha_num[a] / alpha_den[a]) in 64-bit integers
 * on the device; the threshold is the k-th smallest valid score of the group, an element of the column; k > n_g: +inf, trivial.
 * The select is a most-significant-byte-first radix select over the key b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000): four rounds of a
 * histogram kernel (LDS histograms [group][level][256], integer atomics) and a one-wave-per-entry step kernel; the launch count
 * does not depend on the data, only integer atomics are used, and work items are walked with a stride of the grid: the block is
 * bit-identical from run to run, for every batch split and every grid (max_workgroups > 0 caps it).
 * result, ROVIT_EVAL_CONF_WORDS(M, G, A) 8-byte integer words:
 *   [ROVIT_EVAL_CONF_N]   [_BAD_LABELS]   [_N_LABELLED] rows with a label in [0, C)   [_BAD_ROWS + m] labelled rows left out of column m
 *   per entry at ROVIT_EVAL_CONF_ENTRIES + 6 e: n_g, k, less = #{valid < threshold}, equal = #{valid == threshold}, the threshold's
 *   fp32 bits (zero-extended), trivial (0 / 1; then less = n_g, equal = 0, threshold +inf)
 * scores_out (M, n) and u_out (n), both optional, leave the columns and the drawn u behind.
 * rovit_eval_conformal_apply scores the rows of another record against thresholds (M, G, A) on the device: one thread per row.
 * result, ROVIT_EVAL_CONF_APPLY_WORDS(M, A) words; per score at ROVIT_EVAL_CONF_APPLY_SCORES + m (16 + 32 A):
 *   [0] valid rows   [1] labelled rows left out   [2] double: sum of sigma over the valid rows (_MU_SCALED only)   [8 + c] valid rows of
 *   class c (class scores); per level at + 16 + 32 a: [0..8] set-size histogram, [9..17] covered rows by set size, [18..25] covered rows
 *   by class (class scores), [26] covered rows (every kind).  A class c is in the set iff s(c) <= threshold[m][g][a] with g = 1 + c
 *   under class_conditional and 0 otherwise; the other kinds use group 0.  Integer tallies go through LDS and integer atomics; the sum
 *   of sigma is one fixed tree per 256-row chunk and the chunk sums in a fixed order.  member_out (n, M_cls, A) bytes, optional: bit c
 *   of the byte says whether class c is in the set (M_cls counts the class scores, in descriptor order).  label == NULL: no tallies
 *   (result and workspace may be NULL, every score must be a class score): the deployment path.
 * Limits: those of the finalise; 1 <= M <= 8, 1 <= A <= 8, 0 < num < den <= 2^20.  A bad descriptor is refused before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_EVAL_CONF_MAX_SCORES 8
#define ROVIT_EVAL_CONF_MAX_LEVELS 8
#define ROVIT_EVAL_CONF_MAX_DEN (1u << 20)
#define ROVIT_EVAL_CONF_STREAM 0x436F6E66u      /* "Conf": counter word 2, apart from the other Philox streams */
enum {
  ROVIT_EVAL_CONF_LAC = 0, ROVIT_EVAL_CONF_APS = 1, ROVIT_EVAL_CONF_RAPS = 2, ROVIT_EVAL_CONF_KAN_ABS = 3, ROVIT_EVAL_CONF_MU_ABS = 4,
  ROVIT_EVAL_CONF_MU_SCALED = 5, ROVIT_EVAL_CONF_COLUMN = 6
};
enum {
  ROVIT_EVAL_CONF_N = 0, ROVIT_EVAL_CONF_BAD_LABELS = 1, ROVIT_EVAL_CONF_N_LABELLED = 2, ROVIT_EVAL_CONF_BAD_ROWS = 8,
  ROVIT_EVAL_CONF_ENTRIES = 16, ROVIT_EVAL_CONF_ENTRY_WORDS = 6, ROVIT_EVAL_CONF_APPLY_SCORES = 8
};
#define ROVIT_EVAL_CONF_WORDS(M, G, A) ((size_t)ROVIT_EVAL_CONF_ENTRIES + (size_t)ROVIT_EVAL_CONF_ENTRY_WORDS * (M) * (G) * (A))
#define ROVIT_EVAL_CONF_APPLY_WORDS(M, A) ((size_t)ROVIT_EVAL_CONF_APPLY_SCORES + (size_t)(M) * (16 + 32 * (size_t)(A)))
typedef struct rovit_eval_conf {
  int n, num_classes, num_scores, num_levels, class_conditional, randomized, raps_k, max_workgroups;
  float raps_lambda;
  unsigned row_offset;               /* the index of row 0 in the Philox counter */
  unsigned long long seed;
  int score_kind[ROVIT_EVAL_CONF_MAX_SCORES];
  unsigned alpha_num[ROVIT_EVAL_CONF_MAX_LEVELS], alpha_den[ROVIT_EVAL_CONF_MAX_LEVELS];      /* the fit only */
  const float* score_column[ROVIT_EVAL_CONF_MAX_SCORES];   /* (n) each; read for ROVIT_EVAL_CONF_COLUMN only */
  const float* probs; const int* label; const float* sev_pred; const float* sev_true; const float* uncertainty;
  const float* mu;                   /* (n); required by _MU_ABS and _MU_SCALED */
  const float* thresholds;           /* the application only: (M, G, A) fp32 on the device */
  void* workspace;
  size_t workspace_bytes;
  void* result;
  float* scores_out; float* u_out;   /* the fit only; or NULL */
  unsigned char* member_out;         /* the application only; or NULL */
} rovit_eval_conf;
size_t rovit_eval_conformal_workspace_bytes(int n, int num_scores, int num_groups, int num_levels);
int rovit_eval_conformal(const rovit_eval_conf* p, rovit_stream_t stream);
size_t rovit_eval_conformal_apply_workspace_bytes(int n, int num_scores);
int rovit_eval_conformal_apply(const rovit_eval_conf* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Nearest neighbours in feature space (neighbors.hip): the k nearest recorded rows r_j, j in [0, n), of every query row q_i, with no
 * (batch, n) matrix in memory; the neighbour-weighted vote on top.  Rows are fp32 (n, embed) row-major.
 *   ROVIT_KNN_L2      d(q, r) = max(0, (|q|^2 + |r|^2) - 2 q.r)
 *   ROVIT_KNN_COSINE  d(q, r) = max(0, 1 - q^.r^), x^ = x / sqrt(|x|^2) element by element (IEEE sqrt and division)
 * Every term is fp32; q.r and the squared norms are fma chains in ascending feature index from 0 (q.r on v_mfma_f32_32x32x2_f32, whose
 * result is that chain); the other operations are single fp32 operations in the order written.  d is a function of the two rows alone.
 * A recorded row is valid when every feature and its squared norm are finite and, with _COSINE, the squared norm is positive; other rows
 * never are neighbours.  A query row that is not valid in the same sense gets index -1 and distance +inf in every slot.  A pair whose
 * fp32 distance is not finite (with _L2, norms so large that |q|^2 + |r|^2 or 2 q.r overflows fp32: above about 1.7e38) is no candidate.
 * Order: the 64-bit key (bits(d) << 32) | j; d >= 0, so the keys order as unsigned integers and keys of distinct rows are distinct.  The
 * k smallest keys are the answer, ascending: ties in distance go to the lower index.  Fewer valid rows than k: the remaining slots hold
 * index -1 and distance +inf.  exclude (batch) int32 or NULL: per query one row index that is left out (any value outside [0, n): none).
 *
 * rovit_knn_build: one launch, a thread per row: norms[j] = |r_j|^2, valid[j] = 0 / 1, with _COSINE normalized[j] = r^_j (zeros for a
 * row that is not valid; with _L2 the pointer is NULL), result = ROVIT_KNN_WORDS int64 words [ROVIT_KNN_N] [_N_VALID] [_BAD_ROWS].
 * rovit_knn_search: rows = the recorded rows with _L2, the normalized copy with _COSINE.  Three kernels: the queries' norms and flags; the
 * search over (query tiles of ROVIT_KNN_QUERY_TILE rows) x (reference splits), every split leaving its smallest keys per query in the
 * workspace; the merge, which takes the k smallest keys per query and writes
 *   distances (batch, k) fp32, indices (batch, k) int32; with ref_labels: labels (batch, k) int32 (-1 in an empty slot); with
 *   ref_severity: severities (batch, k) fp32 (NaN in an empty slot) and severity (batch) = sum w_j s_j / sum w_j;
 *   kth_distance (batch): the distance in the last valid slot; mean_distance (batch): the mean over the valid slots (both +inf with none);
 *   with ref_labels and num_classes = C >= 1: class_probs (batch, C) = sum w_j [y_j = c] / sum w_j (labels outside [0, C) carry no vote)
 *   and cls (batch) = the first argmax of the fp64 sums (-1 without a valid slot).
 *   w_j = exp(-(d_j - d_1) / temperature) over the valid slots, everything in fp64 in slot order, rounded to fp32 once.
 * Only integer compares decide membership, work items are walked with a stride of the grid, no floating-point atomic: every output is
 * bit-identical from run to run, for every grid (max_workgroups > 0 caps it) and for every number of reference splits (a function of
 * batch and n alone).  workspace: rovit_knn_workspace_bytes(batch, n, embed, k) bytes, 16-byte aligned (0 outside the limits).
 * Limits: embed a multiple of 32 in 32..256, 1 <= n <= ROVIT_KAN_STATS_MAX_ROWS, batch >= 1, 1 <= k <= ROVIT_KNN_MAX_K,
 * 0 <= num_classes <= ROVIT_KNN_MAX_CLASSES, temperature > 0; queries, rows and the normalized copy 16-byte aligned.  A bad descriptor is
 * refused before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_KNN_MAX_K 32
#define ROVIT_KNN_MAX_CLASSES 1024
#define ROVIT_KNN_QUERY_TILE 64
enum { ROVIT_KNN_L2 = 0, ROVIT_KNN_COSINE = 1 };
enum { ROVIT_KNN_N = 0, ROVIT_KNN_N_VALID = 1, ROVIT_KNN_BAD_ROWS = 2, ROVIT_KNN_WORDS = 4 };
typedef struct rovit_knn_index {
  int n, embed, metric, max_workgroups;
  const float* features;             /* (n, embed) */
  float* norms;                      /* (n) */
  int* valid;                        /* (n) */
  float* normalized;                 /* (n, embed) with ROVIT_KNN_COSINE, else NULL */
  void* result;                      /* ROVIT_KNN_WORDS 8-byte words */
} rovit_knn_index;
typedef struct rovit_knn_query {
  int batch, n, embed, k, metric, num_classes, max_workgroups, reserved;
  double temperature;
  const float* queries;              /* (batch, embed) */
  const float* rows;                 /* (n, embed): the recorded rows (_L2) or their normalized copy (_COSINE) */
  const float* norms;                /* (n) */
  const int* valid;                  /* (n) */
  const int* exclude;                /* (batch) or NULL */
  const int* ref_labels;             /* (n) or NULL */
  const float* ref_severity;         /* (n) or NULL */
  void* workspace;
  size_t workspace_bytes;
  float* distances; int* indices;    /* (batch, k) each */
  int* labels; float* severities;    /* (batch, k) each; with ref_labels / ref_severity */
  float* class_probs;                /* (batch, num_classes); with ref_labels and num_classes >= 1 */
  int* cls;                          /* (batch); with class_probs */
  float* severity;                   /* (batch); with ref_severity */
  float* kth_distance; float* mean_distance;   /* (batch) each */
} rovit_knn_query;
size_t rovit_knn_workspace_bytes(int batch, int n, int embed, int k);
int rovit_knn_build(const rovit_knn_index* p, rovit_stream_t stream);
int rovit_knn_search(const rovit_knn_query* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Last-layer Laplace approximation of the heads (laplace.hip): how well do the training rows determine a head's last linear layer at
 * this feature row?  Generalised Gauss-Newton Hessian over the last layer (Kristiadi et al., ICML 2020; Daxberger et al., NeurIPS 2021).
 * A head is fc1 (hid, E) + bias, ReLU, then the last layer; a = [relu(fc1 f + b1); 1] is the augmented hidden row of a feature row f,
 * D = hid + 1 wide, and P = hid + 32 is D padded to a multiple of 32 with exact zeros.  The Grams and the whitening are exact fp32
 * (v_mfma_f32_32x32x2_f32); a is the correctly rounded hidden row (fp64 accumulation).  Eval semantics (no dropout).
 *
 * rovit_laplace_weights, one pointwise launch.  With cls_logits (n, C) not NULL: cls_weights (n, K), K = C (C + 1) / 2, column k the
 * pair (c, d), c <= d, row-major over the upper triangle: lambda_cc = p_c (1 - p_c), lambda_cd = -p_c p_d, p = softmax(logits) in fp64
 * as e_c = exp(l_c - max), p_c (1 - p_c) = e_c (sum_{d != c} e_d) / s^2, rounded to fp32 once.  With log_var (n) not NULL: mu_weights (n)
 * = exp(-log_var) in fp64, rounded once.  A row with a non-finite logit (a non-finite log_var, or one whose weight is not finite in
 * fp32) gets weight 0 in every column and is counted: counts[ROVIT_LAPLACE_BAD_LOGITS], counts[ROVIT_LAPLACE_BAD_LOG_VAR] (int64, zeroed
 * first, integer atomics).  Limits: 1 <= n <= ROVIT_KAN_STATS_MAX_ROWS, 1 <= C <= ROVIT_EVAL_MAX_CLASSES; at least one of the two inputs.
 *
 * rovit_laplace_gram: features (n, E), fc1_weight (hid, E), fc1_bias (hid), weights (n, K) fp32.  result, ROVIT_LAPLACE_WORDS(hid, K)
 * 8-byte words:
 *   int64  [ROVIT_LAPLACE_N]  [_N_VALID]  [_BAD_ROWS]   (words up to _HEADER are 0)
 *   double at _HEADER: G_k[a][b] = sum_i w_ik a_ia a_ib, (K, D, D), every matrix exactly symmetric
 * A row with a non-finite feature or a non-finite weight is left out and counted in BAD_ROWS.  Three kernels: the hidden rows of 64-row
 * tiles (fc1 accumulated in fp64 on the vector unit, rounded to fp32 once after the bias and the ReLU) into the workspace, padded to P;
 * per (chunk, k) the upper tile triangle of A^T (w_k A) over 32-row slabs in LDS, rows of the chunk in order along k of the matrix
 * instruction, one partial per (chunk, k); the fold, per element the chunk partials in fp64 in chunk order, written to [a][b] and [b][a].
 * A chunk is R = 256 ceil(n / (256 ROVIT_LAPLACE_MAX_CHUNKS)) consecutive rows, a function of n alone.  No floating-point atomic: the
 * block is bit-identical from run to run, for every way the rows arrived and for every grid (max_workgroups > 0 caps the grid of every
 * kernel; work items are walked with a stride of the grid).  Every word of the block is written.
 * workspace: rovit_laplace_workspace_bytes(n, E, hid, K) bytes, 16-byte aligned (0 for sizes outside the limits).
 * Limits: E a multiple of 32 in 32..256, hid a multiple of 32 in 32..256, 1 <= K <= ROVIT_LAPLACE_MAX_WEIGHTS, 1 <= n <=
 * ROVIT_KAN_STATS_MAX_ROWS; features and fc1_weight 16-byte aligned.
 *
 * rovit_laplace_predict: features (B, E), any B >= 1, fc1 as above, whitening W (C P, C P) fp32 row-major, W = R^-1 of the posterior
 * precision R R^T in the padded, class-major parameter order (index c P + a).  W is LOWER-TRIANGULAR: of row tile (class block t, tile
 * at) the kernel reads the columns of the class blocks c < t in full and of block t up to the diagonal tile; nothing right of it is read,
 * and the entries above the diagonal inside the diagonal tile must be zero.  With z_c = W[:, block c] a (length C P):
 *   logit_cov (B, C, C) S[c][d] = z_c . z_d, symmetric (computed once, written twice)      logit_var (B, C) S[c][c]
 *   with cls_logits (B, C) not NULL: probs (B, C) = softmax(l_c / sqrt(1 + (pi / 8) S_cc)) in fp64, rounded once; confidence_score (B)
 *   = 1 - max probs, as rest / sum; mean_logit_var (B) = the mean of S_cc in fp64, rounded once
 * C = 1 serves a Gaussian head: logit_var is then the epistemic variance of mu.  One launch; a workgroup owns ROVIT_LAPLACE_TILE rows
 * (the last tile may be partial), forms their hidden rows in LDS (never in memory) and streams W in 32-row tiles, one query row per
 * lane of the accumulators; S is one fp32 fma chain per lane in a fixed order, four partial chains added in a fixed order: the same bits
 * from run to run and for every grid.  A non-finite feature gives non-finite outputs in its own row only.
 * Limits: E and hid as above, 1 <= C <= ROVIT_EVAL_MAX_CLASSES; features, fc1_weight and whitening 16-byte aligned.
 * A bad descriptor is refused before any launch, by all three.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_LAPLACE_MAX_WEIGHTS 36
#define ROVIT_LAPLACE_MAX_CHUNKS 64
#define ROVIT_LAPLACE_TILE 64
enum { ROVIT_LAPLACE_BAD_LOGITS = 0, ROVIT_LAPLACE_BAD_LOG_VAR = 1, ROVIT_LAPLACE_COUNT_WORDS = 2 };
enum { ROVIT_LAPLACE_N = 0, ROVIT_LAPLACE_N_VALID = 1, ROVIT_LAPLACE_BAD_ROWS = 2, ROVIT_LAPLACE_HEADER = 8 };
#define ROVIT_LAPLACE_WORDS(hid, K) ((size_t)ROVIT_LAPLACE_HEADER + (size_t)(K) * ((hid) + 1) * ((hid) + 1))
typedef struct rovit_laplace_weight_args {
  int n, num_classes, max_workgroups, reserved;
  const float* cls_logits;           /* (n, num_classes) or NULL */
  const float* log_var;              /* (n) or NULL */
  float* cls_weights;                /* (n, C (C + 1) / 2); with cls_logits */
  float* mu_weights;                 /* (n); with log_var */
  long long* counts;                 /* ROVIT_LAPLACE_COUNT_WORDS */
} rovit_laplace_weight_args;
typedef struct rovit_laplace_fit {
  int n, embed, hid, num_weights, max_workgroups, reserved;
  const float* features;             /* (n, embed) */
  const float* fc1_weight;           /* (hid, embed) */
  const float* fc1_bias;             /* (hid) */
  const float* weights;              /* (n, num_weights) */
  void* workspace;
  size_t workspace_bytes;
  void* result;                      /* ROVIT_LAPLACE_WORDS(hid, num_weights) 8-byte words */
} rovit_laplace_fit;
typedef struct rovit_laplace_query {
  int batch, embed, hid, num_classes, max_workgroups, reserved;
  const float* features;             /* (batch, embed) */
  const float* fc1_weight;           /* (hid, embed) */
  const float* fc1_bias;             /* (hid) */
  const float* whitening;            /* (C P, C P), P = hid + 32, lower-triangular */
  const float* cls_logits;           /* (batch, num_classes) or NULL */
  float* logit_cov;                  /* (batch, num_classes, num_classes) */
  float* logit_var;                  /* (batch, num_classes) */
  float* probs;                      /* (batch, num_classes); with cls_logits */
  float* confidence_score; float* mean_logit_var;   /* (batch) each; with cls_logits */
} rovit_laplace_query;
int rovit_laplace_weights(const rovit_laplace_weight_args* p, rovit_stream_t stream);
size_t rovit_laplace_workspace_bytes(int n, int embed, int hid, int num_weights);
int rovit_laplace_gram(const rovit_laplace_fit* p, rovit_stream_t stream);
int rovit_laplace_predict(const rovit_laplace_query* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training-data influence through the last layer (influence.hip): which recorded rows made this output, which argue against it, and
 * which recorded labels are suspect (Koh & Liang, ICML 2017; Pruthi et al., NeurIPS 2020; Barshan et al., AISTATS 2020).  Notation of
 * the Laplace section: a (padded to P = hid + 32), the whitening table W = R^-1 of H + tau I = R R^T taken as given, parameters
 * class-major (index c P + a), N = C P.  With the last-layer gradient g[c P + a] = r_c a_a of a row:
 *   whitened gradient u = W g (N; the padding's entries exactly 0)      score s(t, j) = u_t . u_j = g_t^T (H + tau I)^-1 g_j
 *   self-influence |u_j|^2                                              relative score s(t, j) / |u_j|
 * Sign and scale: to first order, removing recorded row j changes the query's target by + s(t, j) (H is a sum over rows, not a mean).
 * Residual r, fp64 rounded to fp32 once:
 *   head ROVIT_INFLUENCE_CLS, target _LOSS    r = softmax(l) - e_y, y = labels[i], or the first argmax of l with labels NULL
 *   head ROVIT_INFLUENCE_CLS, target _OUTPUT  r = e_c, c = labels[i] or the first argmax
 *   head ROVIT_INFLUENCE_MU (C = 1), _LOSS    r = (mu - severity) exp(-log_var)          _OUTPUT  r = 1
 *
 * rovit_influence_embed, one launch: a workgroup owns ROVIT_LAPLACE_TILE rows, forms r in the prologue, the hidden rows in LDS as
 * rovit_laplace_predict does, streams W tile by tile (lower-triangular: nothing right of the diagonal tile is read) and stores per output
 * tile of class block cb  u = sum_{c <= cb} r_c z_c, z_c = W[:, block c] a on the exact-fp32 matrix instruction, one fma chain in
 * ascending c.  Outputs, all at the pointers given (the host offsets them to the batch's first row):
 *   rows (n, N)   residual (n, C) (NaN for a row whose inputs are bad)   norm2 (n) = |u|^2, accumulated in fp64 and rounded once
 *   valid (n) int: 0 for a row with a non-finite feature, logit, mu, log_var or severity, a residual that is not finite in fp32 or a
 *   non-finite entry of u (BAD_ROWS), a label outside [0, C) (BAD_LABELS; a row that is both counts as BAD_ROWS), or u = 0 throughout;
 *   such a row is stored as zeros with norm2 = 0
 *   counts: int64 [ROVIT_INFLUENCE_N] [_N_VALID] [_BAD_ROWS] [_BAD_LABELS], ADDED to with integer atomics (the host zeroes them)
 * Limits as rovit_laplace_predict; features, fc1_weight, whitening and rows 16-byte aligned.
 *
 * rovit_influence_search: queries (B, dim) against rows (n, dim) with their norm2 and valid columns.  A row is a candidate when it is
 * valid, is not exclude[b], has norm2 > 0 under relative, and its score is finite.  Score: q . r on the exact-fp32 matrix instruction, one
 * accumulator chain per (query, row) over the dim in ascending slabs of 64; relative divides by sqrtf(norm2[j]) in fp32; -0 becomes +0.
 *   pro_scores / pro_indices (B, k): by (score descending, index ascending)      opp_scores / opp_indices: (score ascending, index ascending)
 *   the two lists are independent (they overlap when fewer than 2 k candidates exist); empty slots hold -1 / NaN; a query whose
 *   query_valid is 0 has every slot empty.  With ref_labels / ref_severity: pro_labels, opp_labels (-1), pro_severities, opp_severities (NaN).
 * Only integer compares on the key (orderable score bits << 32) | index decide membership.  No (B, n) matrix exists: a work item is (64
 * queries, a split of the rows); per-lane ascending key lists for both ends, the splits' lists in the workspace, a merge kernel ranks them.
 * No floating-point atomic; every output is bit-identical from run to run, for every max_workgroups and for every max_splits (> 0 caps
 * the grid / the number of reference splits; 0: the defaults).
 * workspace: rovit_influence_workspace_bytes(batch, n, dim, k) bytes, 16-byte aligned (0 for sizes outside the limits).
 * Limits: dim a multiple of 32 in 32..ROVIT_INFLUENCE_MAX_DIM, 1 <= k <= ROVIT_INFLUENCE_MAX_K, 1 <= n <= ROVIT_KAN_STATS_MAX_ROWS,
 * batch >= 1; queries, rows and the workspace 16-byte aligned.  A bad descriptor is refused before any launch, by both.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_INFLUENCE_MAX_K 32
#define ROVIT_INFLUENCE_MAX_DIM 2304           /* 8 classes x (256 + 32) */
enum { ROVIT_INFLUENCE_CLS = 0, ROVIT_INFLUENCE_MU = 1 };
enum { ROVIT_INFLUENCE_LOSS = 0, ROVIT_INFLUENCE_OUTPUT = 1 };
enum { ROVIT_INFLUENCE_N = 0, ROVIT_INFLUENCE_N_VALID = 1, ROVIT_INFLUENCE_BAD_ROWS = 2, ROVIT_INFLUENCE_BAD_LABELS = 3,
       ROVIT_INFLUENCE_COUNT_WORDS = 4 };
typedef struct rovit_influence_rows {
  int n, embed, hid, num_classes, head, target, max_workgroups, reserved;
  const float* features;             /* (n, embed) */
  const float* fc1_weight;           /* (hid, embed) */
  const float* fc1_bias;             /* (hid) */
  const float* whitening;            /* (C P, C P), P = hid + 32, lower-triangular */
  const float* cls_logits;           /* (n, num_classes); head CLS */
  const int* labels;                 /* (n) or NULL; head CLS */
  const float* mu; const float* log_var; const float* severity;   /* (n) each; head MU with target LOSS */
  float* rows;                       /* (n, C P) */
  float* residual;                   /* (n, num_classes) */
  float* norm2;                      /* (n) */
  int* valid;                        /* (n) */
  long long* counts;                 /* ROVIT_INFLUENCE_COUNT_WORDS, added to */
} rovit_influence_rows;
typedef struct rovit_influence_query {
  int batch, n, dim, k, relative, max_workgroups, max_splits, reserved;
  const float* queries;              /* (batch, dim) */
  const int* query_valid;            /* (batch) or NULL: every query is good */
  const float* rows;                 /* (n, dim) */
  const float* norm2;                /* (n) */
  const int* valid;                  /* (n) */
  const int* exclude;                /* (batch) or NULL */
  const int* ref_labels;             /* (n) or NULL */
  const float* ref_severity;         /* (n) or NULL */
  void* workspace;
  size_t workspace_bytes;
  float* pro_scores; int* pro_indices; float* opp_scores; int* opp_indices;   /* (batch, k) each */
  int* pro_labels; int* opp_labels;                  /* (batch, k); with ref_labels */
  float* pro_severities; float* opp_severities;      /* (batch, k); with ref_severity */
} rovit_influence_query;
int rovit_influence_embed(const rovit_influence_rows* p, rovit_stream_t stream);
size_t rovit_influence_workspace_bytes(int batch, int n, int dim, int k);
int rovit_influence_search(const rovit_influence_query* p, rovit_stream_t stream);

/* ---- KernelSHAP over groups of patches (csrc/shap.hip; rovit_hip/shap.py holds the host plan and the numpy fp64 reference) ----------
 * P players (2 <= P <= ROVIT_SHAP_PATCHES), M samples (even, 2 <= M <= ROVIT_SHAP_MAX_SAMPLES); sample 2k + 1 is the complement of
 * sample 2k.  A coalition is ROVIT_SHAP_WORDS 32-bit words: player i is bit i % 32 of word i / 32, the bits from P on are zero.
 *
 * rovit_shap_coalitions: one workgroup per pair k, from the host's plan tables (device memory, the host never reads anything back):
 *   pairs (M / 2, 4) int: class s (the coalition's size, 1 <= s < P), enumerated?, rank, reserved     pair_weights (M / 2) double
 *   enumerated: the coalition is the rank-th s-subset of 0..P-1 in lexicographic order (itertools.combinations), unranked with exact
 *   64-bit binomials (the host enumerates a class only when all of it fits the budget, so C(P, s) <= ROVIT_SHAP_MAX_SAMPLES)
 *   sampled: player i has the key (word << 32) | i, word = word i % 4 of Philox4x32-10 with key = seed and counter
 *   (i / 4, rank, ROVIT_SHAP_STREAM, 0); the coalition is the s players with the smallest keys, ranked by counting in LDS: integer
 *   compares alone decide membership
 * It writes bits (M, 7), weights (M) (both samples of a pair carry the pair's) and, with players (196: patch -> player id) not NULL,
 * the src rows of rovit_vit_forward_tokens for the patches of the ABSENT players perturbed:
 *   src_replace (M, 197): row 0 the class token, row 1 + p = 1 + p (kept) or -2 - p (the baseline's row)
 *   src_drop: sample m's sequence -- 0, then 1 + p of the kept patches in patch order -- starts at word drop_offsets[m] of a buffer of
 *   drop_words ints (the host packs sequences of equal length together); a store outside the buffer is skipped
 * src_replace / src_drop may be NULL each.
 *
 * rovit_shap_gram: gram (P, P) double, A[i][j] = sum_m w_m z_mi z_mj, every element one thread's sum over m ascending; then ONE
 * workgroup factors A = L L^T in fp64 in place in the factor block, which lives in global memory and is read through L2 (the packed
 * triangle of 196 rows would fill 154 448 B of the 160 KB LDS; the factorisation is 2.5 MFLOP, once per call):
 *   factor: ROVIT_SHAP_FACTOR_WORDS(P) doubles: L (P, P) row-major (upper part zero), u = A^-1 1 (P), 1^T u, the smallest pivot
 *   (before its square root), ok (1.0; 0.0 after a pivot that is not > 0: u is then NaN and L is left half factored), the sum of
 *   the weights
 *
 * rovit_shap_solve: one workgroup per (image b, target t): b_i = sum_m w_m z_mi (values[m][b][t] - v_empty[b][t]) in fp64 over m
 * ascending (each product rounded, then added), x = A^-1 b by the two triangular solves, lambda = (1^T x - (v_full - v_empty)) / 1^T u,
 *   phi (B, T, P) double = x - lambda u, phi32 the same in fp32      ok (B, T) int: the factor block's
 *   fit_rmse (B, T) double = sqrt(sum_m w_m (z_m . phi - y_m)^2 / sum_m w_m)
 *   patch_map (B, T, 196) fp32 with players not NULL: phi[players[p]] / (patches of that player)
 * ok = 0 gives NaN phi, fit_rmse and patch_map.
 * No floating-point atomic anywhere; every sum has a fixed order and no partition depends on the grid: all outputs are bit-identical
 * from run to run and for every max_workgroups (> 0 caps the grid; work items are walked with a stride of the grid).
 * A bad descriptor is refused before any launch, by all three.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_SHAP_STREAM 0x53686170u          /* "Shap": counter word 2, apart from the other Philox streams */
#define ROVIT_SHAP_PATCHES 196
#define ROVIT_SHAP_WORDS 7
#define ROVIT_SHAP_MAX_SAMPLES (1 << 20)
#define ROVIT_SHAP_FACTOR_WORDS(P) ((size_t)(P) * (P) + (P) + 4)
typedef struct rovit_shap_coalition_args {
  int num_players, num_samples, max_workgroups, reserved;
  unsigned long long seed;
  const int* pairs;                  /* (M / 2, 4) */
  const double* pair_weights;        /* (M / 2) */
  const int* players;                /* (196) or NULL */
  const long long* drop_offsets;     /* (M); with src_drop */
  long long drop_words;
  unsigned* bits;                    /* (M, 7) */
  double* weights;                   /* (M) */
  int* src_replace;                  /* (M, 197) or NULL */
  int* src_drop;                     /* drop_words ints or NULL */
} rovit_shap_coalition_args;
typedef struct rovit_shap_gram_args {
  int num_players, num_samples, max_workgroups, reserved;
  const unsigned* bits;              /* (M, 7) */
  const double* weights;             /* (M) */
  double* gram;                      /* (P, P) */
  double* factor;                    /* ROVIT_SHAP_FACTOR_WORDS(P) */
} rovit_shap_gram_args;
typedef struct rovit_shap_solve_args {
  int num_players, num_samples, batch, num_targets, max_workgroups, reserved;
  const unsigned* bits;              /* (M, 7) */
  const double* weights;             /* (M) */
  const double* factor;              /* rovit_shap_gram's */
  const float* values;               /* (M, batch, num_targets) */
  const float* v_empty;              /* (batch, num_targets) */
  const float* v_full;               /* (batch, num_targets) */
  const int* players;                /* (196) or NULL */
  double* phi;                       /* (batch, num_targets, P) */
  float* phi32;                      /* (batch, num_targets, P) */
  float* patch_map;                  /* (batch, num_targets, 196); with players */
  double* fit_rmse;                  /* (batch, num_targets) */
  int* ok;                           /* (batch, num_targets) */
} rovit_shap_solve_args;
int rovit_shap_coalitions(const rovit_shap_coalition_args* p, rovit_stream_t stream);
int rovit_shap_gram(const rovit_shap_gram_args* p, rovit_stream_t stream);
int rovit_shap_solve(const rovit_shap_solve_args* p, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Exact t-SNE of feature rows (tsne.hip; van der Maaten & Hinton 2008): the dense affinities P and the gradient descent on a 2-D map.
 * Rows x_i are fp32 (n, embed) row-major; all state is fp32; u = 2^-24.
 *
 * rovit_tsne_affinities, in stream order (P holds D, then the conditional rows, then P):
 *   rows        a row is valid when every feature and its squared norm (an fp32 fma chain) are finite and, with ROVIT_KNN_COSINE, the
 *               squared norm is positive.  With _COSINE the kernels below run on the unit rows x / sqrt(|x|^2), formed element by
 *               element as rovit_knn_build forms them.  Every later step treats a row that is not valid as absent.
 *   distances   D_ij = sum_k (x_ik - x_jk)^2 as ONE fp32 chain acc = fma(x_ik - x_jk, x_ik - x_jk, acc), k ascending from 0: every term
 *               is non-negative, |D - exact| <= (embed + 2) u D, D_ii = 0 and D_ij = D_ji bit for bit; 0 where i or j is not valid.
 *               distances_only != 0 stops here (P = D; beta, entropy and status are not written).
 *   perplexity  a workgroup per valid row i over its candidates (the valid j != i): d_j = D_ij - min_j D_ij, beta = 1, then exactly 64
 *               steps: H(beta) = log S + beta sum_j d_j w_j / S with w_j = exp(-(beta d_j)) and S = sum_j w_j; H > log(perplexity): beta
 *               becomes the lower bracket and doubles (or moves half way to the upper one when there is one); otherwise it becomes the
 *               upper bracket and halves (or moves half way to the lower one).  beta is kept in fp64 and used rounded to fp32; w in fp32
 *               (expf); the sums as described below.  After the loop p_j|i = w_j / S (an fp64 division rounded once), 0 on the diagonal
 *               and at rows that are not valid; beta[i] and entropy[i] = H at the final beta.  A row with fewer than two brackets after
 *               the loop is counted as unconverged: it has at least `perplexity` exact duplicates, its beta ends at 2^64 and its row is
 *               uniform over the duplicates.  beta d is formed so that d = 0 gives 0: no NaN arises.  A row that is not valid gets a zero
 *               row, beta 0 and entropy 0.
 *   symmetrise  (symmetrize != 0) P_ij = max((p_j|i + p_i|j) / (2 n_valid), 1e-12) for valid i != j (one fp32 add, one IEEE division),
 *               0 on the diagonal and in rows and columns that are not valid; in place by tile pairs, symmetric bit for bit.
 *   status      ROVIT_TSNE_WORDS int64 words: [_N] [_N_VALID] [_BAD_ROWS] [_UNCONVERGED] and the fp32 bit patterns of the smallest and
 *               largest beta of a valid row [_MIN_BETA] [_MAX_BETA].
 *
 * rovit_tsne_run: n_iter iterations on the caller's stream, two launches each, nothing waits for the host.  A map row with a NaN
 * coordinate is absent (the caller marks the rows that are not valid this way; P is 0 there): it keeps its NaN and adds to nothing.
 *   forces      for row i over the present j != i, w_ij = 1 / (1 + |y_i - y_j|^2): a_i = sum_j P_ij w_ij (y_i - y_j),
 *               r_i = sum_j w_ij^2 (y_i - y_j), z_i = sum_j w_ij; on the iterations t with t % kl_every == 0, and on the last one (kl_every
 *               0: never), A_i = sum_j P_ij (log P_ij - log w_ij) over P_ij > 0 and B_i = sum_j P_ij.
 *   update      Z = sum_i z_i (every workgroup folds it itself); g = 4 (alpha a - r / Z); gain = (v g < 0) ? gain + 0.2 : gain 0.8, then
 *               max(gain, 0.01); v = m v - eta gain g; y += v: sklearn's _gradient_descent.  KL_t = sum A + log Z sum B goes to the next
 *               free slot of trace.  alpha = early_exaggeration and m = momentum_early for t < exaggeration_iter, then 1 and momentum_late.
 *               learning_rate <= 0 stands for sklearn's 'auto', max(n_present / early_exaggeration / 4, 50), resolved on the device:
 *               the host does not know n_present without a copy.  grad_out (n, 2) and z_out (1), when given, receive g and Z of the last
 *               iteration.
 *   center != 0 subtracts the mean of the present rows once, after the last iteration.
 *   status      [_N] [_N_VALID] (present rows) [_BAD_ROWS] [_RUN_ITERATIONS] [_RUN_TRACE] (slots written) [_RUN_NONFINITE] (present rows
 *               with an infinite coordinate, before centring).
 * Sums (S, the forces, Z, the KL parts, the mean): a lane or thread adds its own elements in ascending index in fp32 (element j belongs
 * to lane j % 64 of its row's wave, or to thread j % 256), the wave folds by a fixed butterfly in fp32, the four waves fold in wave
 * order in fp64.  No atomic, no cooperative launch, no kernel that waits on another workgroup; work items are walked with a stride of
 * the grid: every output is bit-identical from run to run and for every max_workgroups (> 0 caps every grid).
 * rovit_tsne_random_init: Y[e] = 1e-4 sqrt(-2 ln u1) cos(2 pi u2), e in [0, 2 n), u1 = ((x >> 8) + 1) 2^-24 and u2 = (y >> 8) 2^-24 from
 * words x, y of Philox4x32-10 with key = seed and counter (e, 0, ROVIT_TSNE_STREAM, 0).
 * workspace: rovit_tsne_workspace_bytes(n, embed) bytes, 16-byte aligned (0 outside the limits); the same block serves both entries.
 * Limits: embed a multiple of 32 in 32..256 with 16-byte aligned rows, 4 <= n <= ROVIT_TSNE_MAX_ROWS (dense P is 1 GiB there),
 * 1 < perplexity < n - 1 (n_valid is known on the device only: fewer valid rows than the perplexity allows show in status, as
 * unconverged rows), 1 <= n_iter <= ROVIT_TSNE_MAX_ITER, Y 8-byte aligned.  A bad descriptor returns ROVIT_ERR_SHAPE (_NULL, _ALIGN)
 * before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_TSNE_MAX_ROWS 16384
#define ROVIT_TSNE_MAX_ITER 100000
#define ROVIT_TSNE_STREAM 0x54534E45u          /* "TSNE": counter word 2, apart from the other Philox streams */
enum { ROVIT_TSNE_N = 0, ROVIT_TSNE_N_VALID = 1, ROVIT_TSNE_BAD_ROWS = 2, ROVIT_TSNE_UNCONVERGED = 3, ROVIT_TSNE_MIN_BETA = 4,
       ROVIT_TSNE_MAX_BETA = 5, ROVIT_TSNE_WORDS = 8 };
enum { ROVIT_TSNE_RUN_ITERATIONS = 3, ROVIT_TSNE_RUN_TRACE = 4, ROVIT_TSNE_RUN_NONFINITE = 5 };
typedef struct rovit_tsne_affinity {
  int n, embed, metric, symmetrize, distances_only, max_workgroups;
  double perplexity;
  const float* features;             /* (n, embed) */
  void* workspace;
  size_t workspace_bytes;
  float* P;                          /* (n, n) */
  float* beta; float* entropy;       /* (n) each */
  void* status;                      /* ROVIT_TSNE_WORDS 8-byte words */
} rovit_tsne_affinity;
typedef struct rovit_tsne_descent {
  int n, n_iter, exaggeration_iter, kl_every, center, max_workgroups, trace_capacity, reserved;
  float early_exaggeration, momentum_early, momentum_late, learning_rate;
  const float* P;                    /* (n, n) */
  float* Y;                          /* (n, 2): the initial map on entry, the map on exit */
  float* V; float* G;                /* (n, 2) each: the velocities and the gains, carried from call to call */
  void* workspace;
  size_t workspace_bytes;
  float* trace;                      /* trace_capacity values; NULL with kl_every 0 */
  void* status;                      /* ROVIT_TSNE_WORDS 8-byte words */
  float* grad_out;                   /* (n, 2) or NULL */
  float* z_out;                      /* (1) or NULL */
} rovit_tsne_descent;
size_t rovit_tsne_workspace_bytes(int n, int embed);
int rovit_tsne_affinities(const rovit_tsne_affinity* p, rovit_stream_t stream);
int rovit_tsne_run(const rovit_tsne_descent* p, rovit_stream_t stream);
int rovit_tsne_random_init(unsigned long long seed, float* Y, int n, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * k-means of the feature space (kmeans.hip): k-means++ seeding, Lloyd iterations with the exact stopping rule, the per-cluster score
 * card and the cluster x class contingency table.  Rows are fp32 (n, embed) row-major, embed a multiple of 32 in 32..256,
 * 1 <= n <= ROVIT_KMEANS_MAX_ROWS, 1 <= k <= ROVIT_KMEANS_MAX_K.
 * Rows.  Validity is rovit_knn_build's: a row with a non-finite feature or squared norm (with ROVIT_KNN_COSINE also a zero row) is
 * absent: label -1, distance and second distance +inf, silhouette 0, counted in [_BAD_ROWS], and it enters no sum and no pick.  With
 * _COSINE every kernel works on the unit rows x^ = x / sqrt(|x|^2) (element by element, as rovit_knn_build forms them; `normalized`).
 * Distance of a row x to a centroid c: the neighbours' definition.  _L2: max(0, (|x|^2 + |c|^2) - 2 x.c); _COSINE: max(0, 1 - x^.c) with
 * c of unit length (spherical k-means).  Every term fp32, x.c and the squared norms fma chains in ascending feature index from 0: on the
 * vector units in the seeding kernel, on v_mfma_f32_32x32x2_f32 in the assignment kernel, the same bits.
 * Order.  A row belongs to the centroid with the smallest key (bits(d) << 32) | c, an unsigned 64-bit integer: ties go to the lower
 * cluster index, only integer compares decide.  The second smallest key gives second_distance (+inf with k = 1).
 * Seeding (Arthur & Vassilvitskii 2007, one trial per seed), exact in integers.  Seed j of restart r draws r64 = (w.x << 32) | w.y from
 * Philox4x32-10(key = seed, counter = (j, r, ROVIT_KMEANS_STREAM, 0)).  Seed 0 is the floor(r64 * n_valid / 2^64)-th valid row in
 * ascending index.  Seed j > 0: d_i = the smallest distance of row i to the seeds chosen so far (fp32), dmax = max_i d_i = m * 2^e with
 * m in [1/2, 1), w_i = floor(d_i * 2^(40 - e)) (exact, below 2^40), W = sum w_i, t = floor(r64 * W / 2^64), and the seed is the smallest i
 * with sum_{i' <= i} w_i' > t.  W = 0 (every valid row coincides with a seed): w_i = 1 for every valid row, counted in [_W0_EVENTS].
 * More seeds than valid rows: [_SHORT] = 1 (and -1 seeds when there is no valid row at all).  The chosen index is read from device
 * memory by the next launch; three launches per seed (distances and maximum; weights and block sums; the pick), two for seed 0.
 * tap (m, n) or NULL: row j >= 1 receives the d_i that seed j was drawn from.
 * Lloyd iteration it = 1 .. max_iter: assign (labels, both distances, the integer count of rows whose label changed); when no label
 * changed [_DONE] = 1, [_N_ITER] = it and every later launch of the run returns at once; otherwise update: the rows are brought into
 * (cluster, ascending row index) order by a two-level counting sort (per 256-row block counts, a scan per cluster, a scatter; integers
 * only), every cluster's members are cut into segments of ROVIT_KMEANS_SEGMENT, a segment is summed in fp64 in member order, the
 * segments are added in ascending order, the sum is divided by the count and rounded once to fp32.  With _COSINE the fp64 mean of the
 * unit rows is divided by its fp64 length (sum of squares in ascending feature index) and rounded once.  The order is a function of
 * (n, labels) alone.  An empty cluster keeps its centroid ([_EMPTY_EVENTS] counts them over the run), and so does a _COSINE cluster
 * whose mean has zero length ([_ZERO_MEANS]); nothing is relocated.  No tolerance: the stopping rule is the exact one.  Without
 * convergence [_N_ITER] = max_iter.  All launches are enqueued at once; nothing waits for the host.
 * Final pass: one more assign against the final centroids, the same sort, and per cluster c into the status block:
 *   counts; medoids: the member with the smallest key (bits(d) << 32) | row (-1 for an empty cluster); inertia: the fp64 sum of the
 *   members' fp32 distances (per 1024-member segment: member s of the segment belongs to thread s % 256, which adds its members in
 *   ascending order; the threads are added by the fixed tree of common.h; segments in ascending order); silhouette sums likewise;
 *   radii: the largest member distance.  [_EMPTY] = the number of empty clusters.
 * Silhouette (simplified) of a row: (b - a) / max(a, b) in fp32 with a, b = sqrtf of the two distances with _L2, the distances with
 * _COSINE; 0 when k = 1, when max(a, b) = 0 and for an absent row.
 * status: ROVIT_KMEANS_WORDS + 5 k 8-byte words: the words below, then k int64 counts, k int64 medoids, k fp64 inertias, k fp64
 * silhouette sums, k fp64 radii (each the fp32 value).  rovit_kmeans_seed fills only the first ROVIT_KMEANS_WORDS.
 * rovit_kmeans_seed: m seeds (1 <= m <= ROVIT_KMEANS_MAX_K) into seeds (m) and their rows (unit rows with _COSINE) into centroids (m, embed).
 * rovit_kmeans_run: centroids (k, embed) hold the initial centroids on entry (unit length with _COSINE) and the final ones on exit.
 * rovit_kmeans_assign: the assignment alone of n rows against k given centroids (out-of-sample rows).
 * rovit_kmeans_contingency: table (k * num_classes + 1 int64): table[c * num_classes + y] counts the rows with cluster c and class y by
 * integer atomics; a row whose cluster is outside [0, k) or whose class is outside [0, num_classes) is counted in the last word.
 * No floating-point atomic anywhere; work items are walked with a stride of the grid: every output is bit-identical from run to run
 * and for every max_workgroups.  workspace: rovit_kmeans_workspace_bytes(n, embed, k) bytes (0 outside the limits), 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_KMEANS_MAX_ROWS (1 << 20)
#define ROVIT_KMEANS_MAX_K 256
#define ROVIT_KMEANS_MAX_ITER 100000
#define ROVIT_KMEANS_SEGMENT 1024
#define ROVIT_KMEANS_STREAM 0x4B4D6E73u   /* "KMns" */
enum { ROVIT_KMEANS_N = 0, ROVIT_KMEANS_N_VALID = 1, ROVIT_KMEANS_BAD_ROWS = 2, ROVIT_KMEANS_N_ITER = 3, ROVIT_KMEANS_DONE = 4,
       ROVIT_KMEANS_EMPTY = 5, ROVIT_KMEANS_EMPTY_EVENTS = 6, ROVIT_KMEANS_ZERO_MEANS = 7, ROVIT_KMEANS_W0_EVENTS = 8,
       ROVIT_KMEANS_SHORT = 9, ROVIT_KMEANS_CHANGED = 10 /* two words */, ROVIT_KMEANS_WORDS = 16 };
typedef struct rovit_kmeans_problem {
  int n, embed, k, metric, max_iter, max_workgroups, restart, m;
  unsigned long long seed;
  const float* features;             /* (n, embed) */
  float* normalized;                 /* (n, embed) scratch with ROVIT_KNN_COSINE, else NULL */
  float* centroids;                  /* (k, embed); rovit_kmeans_seed: (m, embed) */
  int* seeds;                        /* (m); rovit_kmeans_seed only */
  float* tap;                        /* (m, n) or NULL; rovit_kmeans_seed only */
  int* labels;                       /* (n) */
  float* distance; float* second_distance; float* silhouette;   /* (n) each */
  void* workspace;
  size_t workspace_bytes;
  void* status;
} rovit_kmeans_problem;
size_t rovit_kmeans_workspace_bytes(int n, int embed, int k);
int rovit_kmeans_seed(const rovit_kmeans_problem* p, rovit_stream_t stream);
int rovit_kmeans_run(const rovit_kmeans_problem* p, rovit_stream_t stream);
int rovit_kmeans_assign(const rovit_kmeans_problem* p, rovit_stream_t stream);
int rovit_kmeans_contingency(const int* clusters, const int* classes, int n, int k, int num_classes, long long* table, rovit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Adversarial perturbations (attack.hip): the projected step and the random start of a PGD attack (Madry et al. 2018) on normalised
 * images.  The specification of record, in numpy, is rovit_hip/attack.py (step_reference, init_reference).
 * Tensors: x, g, delta, x_adv, best_delta fp32 (B, 3, H, W) contiguous, n = H W >= 1 (any H, W; the model passes 224 x 224); x the
 * clean normalised images, g the objective's gradient at x_adv (ascent), delta the perturbation in normalised units (read and
 * overwritten), x_adv written.  eps, alpha: (B) fp32 DEVICE arrays, radius and step length per image in pixel units (image in
 * [0, 1]); they are not checked: a negative or NaN entry gives that image an undefined perturbation and touches no other image.
 * Host arrays of 3: inv_s[c] = fl32(1 / std_c), s[c] = std_c (L2 only), lo[c], hi[c] = the normalised values of pixel 0 and 1, or
 * -inf / +inf for no box.  Per image and channel r = fl32(eps_b inv_s_c), a = fl32(alpha_b inv_s_c).
 * clamp(v, l, h) below is: l when v < l, h when v > h, else v itself (a zero keeps its sign, a NaN passes through).
 * copy_mask (B) bytes with best_delta, or both NULL: where copy_mask[b] != 0, best_delta[b] <- the delta the call was entered with
 * (the perturbation whose objective value the caller has just found to be its best), before anything else.
 *
 * rovit_attack_step_linf, one launch.  Per element, every operation rounded once to fp32 and none contracted:
 *   sg = +1, -1, 0 for g > 0, g < 0, and g == 0 or NaN;  d1 = delta + sg a;  d2 = clamp(d1, -r, r);  y = clamp(x + d2, lo_c, hi_c);
 *   delta' = clamp(y - x, -r, r);  x_adv = clamp(x + delta', lo_c, hi_c).
 * |delta'| <= r and lo_c <= x_adv <= hi_c hold exactly; eps_b == 0 gives x_adv == x wherever x is inside the box.  x_adv - x may
 * differ from delta' by the one rounding of x + delta' (half an ulp of x_adv: 2^-23 at |x_adv| in [2, 4) against r >= 0.017 at
 * eps = 1/255).
 *
 * rovit_attack_step_l2, three launches.  The ball is in pixel units, u = delta s_c.  gh = g inv_s_c (0 where g is not finite),
 * G = sqrt(sum gh^2) over the image; d1 = delta + (alpha_b gh / G) inv_s_c (no move when G == 0: d1 == delta); the box in delta space,
 * db = fl32(clamp(d1, lo_c - x, hi_c - x)) (the move is bounded before it meets x, so no rounding of x enters delta); U = sqrt(sum
 * (db s_c)^2); delta' = fl32(db min(1, eps_b / U)) (the box is convex and holds x, so the shrink stays inside);
 * x_adv = clamp(fl32(x + delta'), lo_c, hi_c).  Everything before each fl32 is fp64.  Both sums are fp64 sums in a fixed order: a
 * workgroup sums its slab (thread-major, then the fixed tree of block_sum_t), the slab partials go to scratch, and every workgroup of
 * the image adds the image's partials in index order.  No atomic; the same bits from run to run.
 * scratch: rovit_attack_scratch_doubles(B, H, W) doubles (0 for a shape the kernels refuse), 8-byte aligned.
 *
 * rovit_attack_init: the random start.  Element e (its index in the (3, H, W) image) of image b takes word e % 4 of
 * Philox4x32-10(key = seed, counter = (e / 4, (unsigned)ids[b], ROVIT_ATTACK_STREAM, restart)): a draw depends on (seed, ids[b], e,
 * restart) alone.  ROVIT_ATTACK_LINF (one launch): d1 = fl32((2 u01(w) - 1) r), u01(w) = (w >> 8) 2^-24, then d2 .. x_adv as in the
 * step.  ROVIT_ATTACK_L2 (three launches): Box-Muller normals in fp64 -- words (x, y) of a call give z(4k) = R cos(T), z(4k + 1) =
 * R sin(T) with R = sqrt(-2 ln(((x >> 8) + 1) 2^-24)), T = 2 pi (y >> 8) 2^-24, words (z, w) give z(4k + 2), z(4k + 3) the same way --
 * rounded once to fp32; d1 = (eps_b z / |z|_2) inv_s_c; then db .. x_adv as in the L2 step.  eps_b == 0 gives delta == 0.
 *
 * Every entry checks on the host, before any launch: null pointers, B >= 1, H, W >= 1, norm, inv_s and s finite and positive, lo / hi
 * finite or -inf / +inf with lo <= hi, 4-byte alignment, and that x, g, delta, x_adv and best_delta do not overlap.
 * ------------------------------------------------------------------------------------------------------------ */
#define ROVIT_ATTACK_STREAM 0x41646176u          /* "Adav": counter word 2, apart from the other Philox streams */
enum { ROVIT_ATTACK_LINF = 0, ROVIT_ATTACK_L2 = 1 };
size_t rovit_attack_scratch_doubles(int B, int H, int W);
int rovit_attack_step_linf(const float* x, const float* g, float* delta, float* x_adv, float* best_delta, const unsigned char* copy_mask,
                           const float* eps, const float* alpha, const float* inv_s, const float* lo, const float* hi, int B, int H, int W,
                           rovit_stream_t stream);
int rovit_attack_step_l2(const float* x, const float* g, float* delta, float* x_adv, float* best_delta, const unsigned char* copy_mask,
                         const float* eps, const float* alpha, const float* inv_s, const float* s, const float* lo, const float* hi,
                         double* scratch, int B, int H, int W, rovit_stream_t stream);
int rovit_attack_init(const float* x, float* delta, float* x_adv, const long long* ids, const float* eps, int norm, unsigned long long seed,
                      unsigned restart, const float* inv_s, const float* s, const float* lo, const float* hi, double* scratch, int B, int H,
                      int W, rovit_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVIT_HIP_H */
