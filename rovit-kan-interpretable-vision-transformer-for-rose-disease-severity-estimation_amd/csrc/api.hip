// Library-level entry points: version and the thread-local error string.
#include <stdarg.h>

#include "common.h"

static thread_local char g_err[512] = "";

void rovit_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// 100: round 1.  200: round 2 changed rovit_vit_backward(_notify) (leading `images`) and rovit_joint_loss (float severity targets).
// 300: round 3 adds the fused MLP entry points and the prepared-weight stream they read (rovit_vit_prep_bytes grew).
// 400: round 4 -- rovit_vit_forward / _backward(_notify) take `mlp_path`; every rovit_set_* knob and the experiments that lost left the ABI.
// 410: round 4 -- rovit_joint_loss takes int64 severity labels (severity_is_int64); rovit_head_phase_*, rovit_sq_norm_clip, rovit_adamw_flat_multi added.
// 420: rovit_vit_forward_rollout and rovit_rollout_map added (attention rollout, rollout.hip).
// 430: rovit_vit_gradcam_workspace_bytes, rovit_vit_forward_gradcam, rovit_vit_gradcam and rovit_gradcam_map added (Grad-CAM++, gradcam.hip).
// 440: rovit_head_mc_fwd added (Monte-Carlo dropout over the heads, mc_dropout.hip).
// (rovit_explain_seed and rovit_vit_gradcam_seeded were added at 440: new entries only, no argument list changed, and the binding
// resolves every symbol it declares at load time.)
// (rovit_patch_embed_dgrad and rovit_vit_backward_input were added at 440 the same way: image gradients, input_grad.hip; the argument
// lists of rovit_vit_backward and rovit_vit_backward_notify did not change.)
// (rovit_attention_relevance_step and rovit_vit_backward_relevance were added at 440 the same way: attention relevance, relevance.hip.)
// (rovit_vit_embed and rovit_vit_forward_tokens were added at 440 the same way: deletion / insertion curves, perturb.hip.)
// (rovit_vit_f32_workspace_field was added at 440 the same way: a host-only view of the fp32 forward's workspace, vit_f32.hip.)
// (rovit_eval_accumulate, rovit_eval_finalize and rovit_eval_partials_doubles were added at 440 the same way: test-set evaluation and
// validation with one synchronisation per epoch, evaluate.hip.)
// (rovit_kan_stats_words, rovit_kan_stats_partials_doubles, rovit_kan_edge_stats and rovit_kan_curves were added at 440 the same way:
// per-edge KAN activation statistics, kan_stats.hip.)
// (rovit_augment_batch was added at 440 the same way: per-sample augmentation of a device-resident uint8 image store, augment_batch.hip.)
// (rovit_joint_loss_mixed and rovit_train_finalize were added at 440 the same way: the CutMix / MixUp loss with a per-batch record and the
// per-epoch reduction, train_epoch.hip.)
// (rovit_block_bwd_fused_cls and rovit_gemm_ln_bwd_cls were added at 440 the same way: the class-token forms of the backward's fused
// launch and of the qkv dgrad it replaces, mlp_fused.hip / gemm.hip.)
// (rovit_adamw_ema_flat_multi and rovit_swap_flat_multi were added at 440 the same way: weight EMA inside the AdamW launch, optim.hip.)
// (rovit_eval_calibrate_workspace_bytes, rovit_eval_calibrate and rovit_eval_recalibrate were added at 440 the same way: temperature and
// sigma scaling of the evaluation record, calibrate.hip.)
// (rovit_density_workspace_bytes, rovit_density_moments, rovit_density_score, rovit_ood_metrics_workspace_bytes and rovit_ood_metrics were
// added at 440 the same way: feature-space density and OOD metrics, density.hip.  The number stays: no argument list changed, and
// tests/test_evaluation_cpu.py and tests/test_mc_dropout_cpu.py pin 440.)
// (rovit_eval_conformal_workspace_bytes, rovit_eval_conformal, rovit_eval_conformal_apply_workspace_bytes and rovit_eval_conformal_apply
// were added at 440 the same way: split conformal prediction on the evaluation record, conformal.hip.)
// (rovit_knn_workspace_bytes, rovit_knn_build and rovit_knn_search were added at 440 the same way: nearest neighbours in feature space,
// neighbors.hip.  The number stays for the reason given above: no argument list changed and two test files pin 440.)
// (rovit_corrupt_stats and rovit_corrupt_batch were added at 440 the same way: image corruptions of the uint8 store, corrupt.hip.)
// (rovit_vit_ragged_workspace_bytes, rovit_vit_forward_ragged, rovit_attention_fwd_ragged and rovit_attention_cls_fwd_ragged were added
// at 440 the same way: sequences of different lengths in one inference forward, attention.hip / perturb.hip / vit.hip.)
// (rovit_patch_dropout_draw, rovit_scatter_token_rows, rovit_vit_forward_train_tokens and rovit_vit_backward_tokens were added at 440 the
// same way: PatchDropout training on kept tokens, patch_dropout.hip / vit.hip.)
// (rovit_sort_workspace_bytes, rovit_sort_f32, rovit_rank_workspace_bytes, rovit_rank_f32 and the three score cards' _ex forms with their
// *_rank_workspace_bytes were added at 440 the same way: the device radix sort and the ranks behind it, sort_rank.hip.  rovit_eval_finalize,
// rovit_eval_selective and rovit_ood_metrics keep their argument lists and their launches.)
// (rovit_tsne_workspace_bytes, rovit_tsne_affinities, rovit_tsne_run and rovit_tsne_random_init were added at 440 the same way: exact t-SNE
// of the feature space, tsne.hip.)
// (rovit_kmeans_workspace_bytes, rovit_kmeans_seed, rovit_kmeans_run, rovit_kmeans_assign and rovit_kmeans_contingency were added at 440
// the same way: k-means of the feature space, kmeans.hip.)
// (rovit_vit_forward_head_stats, rovit_attention_head_stats_step, rovit_head_stats_finalize and rovit_head_stats_block_words were added at
// 440 the same way: per-head attention statistics, head_stats.hip / vit.hip.)
// (rovit_attack_scratch_doubles, rovit_attack_step_linf, rovit_attack_step_l2 and rovit_attack_init were added at 440 the same way: the
// projected step and the random start of a PGD attack, attack.hip.)
extern "C" int rovit_version(void) { return 440; }
extern "C" const char* rovit_last_error_string(void) { return g_err; }

#include <mutex>
#include <utility>
#include <vector>

bool rovit_set_max_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lock(mu);
  for (const auto& d : done)
    if (d.first == fn && d.second == dev) return true;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
  done.emplace_back(fn, dev);
  return true;
}

#ifdef ROVIT_DEV
#include <stdlib.h>
#include <string.h>
int g_rovit_knob[ROVIT_KNOB_COUNT] = {0};
bool g_rovit_knob_set[ROVIT_KNOB_COUNT] = {false};
// ROVIT_DEV_KNOBS="id=value,id=value" (the developer library's ONE environment variable), read when the library is loaded
static int g_rovit_knob_env = [] {
  const char* e = getenv("ROVIT_DEV_KNOBS");
  while (e && *e) {
    int id = -1, v = 0, n = 0;
    if (sscanf(e, "%d=%d%n", &id, &v, &n) == 2 && id >= 0 && id < ROVIT_KNOB_COUNT) { g_rovit_knob[id] = v; g_rovit_knob_set[id] = true; }
    e = strchr(e, ',');
    if (e) ++e;
  }
  return 0;
}();
// developer library only (make dev): override / clear (value < 0 with clear != 0) a knob of common.h's RovitKnob list
extern "C" int rovit_dev_set_knob(int id, int value, int clear) {
  ROVIT_CHECK_ARG(id >= 0 && id < ROVIT_KNOB_COUNT, ROVIT_ERR_SHAPE, "dev knob %d out of range", id);
  g_rovit_knob[id] = value;
  g_rovit_knob_set[id] = !clear;
  return ROVIT_OK;
}
#endif
