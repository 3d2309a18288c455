"""ctypes binding of librovit_hip.so (C ABI declared in include/rovit_hip.h).

No libtorch linkage: tensors cross the boundary as raw device pointers plus the caller's current HIP stream.
There is NO fallback: if the shared library is missing, or a tensor is not on a CUDA/HIP device, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get('ROVIT_HIP_LIB') or os.path.join(_PKG_ROOT, 'lib', 'librovit_hip.so')   # env override: developer A/B builds

_lib: Optional[C.CDLL] = None
ABI_VERSION = 440          # rovit_version() this binding matches (csrc/api.hip)

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# mlp_path of rovit_vit_forward / rovit_vit_backward (include/rovit_hip.h); rovit_gemm_nt's per-call tile flags
MLP_AUTO, MLP_TWO_LAUNCH, MLP_ONE_LAUNCH = 0, 1, 2
GEMM_TILED_192, GEMM_TILED_96 = 0x100, 0x200
MLP_FUSED_MIN_ROWS = 34000          # ROVIT_MLP_AUTO's threshold (csrc/vit.hip): one-launch MLP half from this many token rows

# name -> (restype, argtypes); mirrors include/rovit_hip.h one to one
SIGNATURES = {
    'rovit_version': (_i, []),
    'rovit_last_error_string': (C.c_char_p, []),
    'rovit_kan_basis': (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    'rovit_kan_layer_fwd': (_i, [_vp] * 6 + [_i] * 5 + [_vp]),
    'rovit_kan_prepare': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'rovit_kan_stack_fwd': (_i, [_vp] * 6 + [_i, _vp, _vp, _vp, _i, _vp]),
    'rovit_kan_mfma_prepared_floats': (_sz, [_i, _i, _i]),
    'rovit_kan_prepare_mfma': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    'rovit_kan_stack_fwd_mfma': (_i, [_vp] * 5 + [_i, _vp, _vp, _vp, _i, _vp]),
    'rovit_kan_stack_bwd': (_i, [_vp] * 11 + [_i, _vp, _vp, _vp, _i, _vp]),
    'rovit_kan_layer_bwd': (_i, [_vp] * 10 + [_i] * 6 + [_vp]),
    'rovit_linear_fwd': (_i, [_vp] * 5 + [_i] * 4 + [_vp]),
    'rovit_linear_bwd': (_i, [_vp] * 9 + [_i] * 4 + [_vp]),
    'rovit_heads_fwd': (_i, [_vp] * 8 + [_i] * 5 + [_vp]),
    'rovit_heads_bwd': (_i, [_vp] * 12 + [_i] * 5 + [_vp]),
    'rovit_head_phase_fwd': (_i, [_vp, _vp]),
    'rovit_head_phase_bwd': (_i, [_vp, _vp]),
    'rovit_head_phase_bwd_params': (_i, [_vp, _vp]),
    'rovit_head_mc_fwd': (_i, [_vp, _vp]),
    'rovit_vit_num_params': (_i, [_i]),
    'rovit_vit_prep_bytes': (_sz, [_i]),
    'rovit_vit_workspace_bytes': (_sz, [_i, _i, _i]),
    'rovit_vit_f32_workspace_bytes': (_sz, [_i]),
    'rovit_vit_forward_f32': (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    'rovit_vit_f32_workspace_field': (_i, [_i, _i, _vp, _vp]),
    'rovit_vit_workspace_field': (_i, [_i, _i, _i, _i, _vp, _vp]),
    'rovit_vit_prepare': (_i, [_vp, _vp, _i, _vp]),
    'rovit_vit_forward': (_i, [_vp] * 5 + [_i] * 4 + [_vp]),
    'rovit_vit_forward_prepare': (_i, [_vp] * 5 + [_i] * 5 + [_vp]),
    'rovit_vit_forward_taps': (_i, [_vp] * 7 + [_i, _i, _vp]),
    'rovit_vit_forward_rollout': (_i, [_vp] * 6 + [_i, _i, _i, _vp]),
    'rovit_rollout_map': (_i, [_vp, _vp, _i, _vp]),
    'rovit_vit_forward_head_stats': (_i, [_vp] * 8 + [_i, _i, _vp]),
    'rovit_attention_head_stats_step': (_i, [_vp] * 5 + [_i, _i, _i, _vp]),
    'rovit_head_stats_block_words': (_sz, [_i, _i, _i]),
    'rovit_head_stats_finalize': (_i, [_vp] * 4 + [_i, _i, _i, _i, _vp]),
    'rovit_vit_gradcam_workspace_bytes': (_sz, [_i, _i]),
    'rovit_vit_forward_gradcam': (_i, [_vp] * 5 + [_i, _i, _vp]),
    'rovit_vit_gradcam': (_i, [_vp] * 8 + [_i, _i] + [_vp] * 6 + [_i, _i, _vp]),
    'rovit_gradcam_map': (_i, [_vp, _vp, _i, _vp]),
    'rovit_explain_seed': (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    'rovit_vit_gradcam_seeded': (_i, [_vp] * 7 + [_i, _i, _vp]),
    'rovit_attention_probs': (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    'rovit_vit_backward': (_i, [_vp] * 6 + [_i] * 5 + [_vp]),
    'rovit_vit_backward_notify': (_i, [_vp] * 6 + [_i] * 5 + [_vp] + [_vp]),
    'rovit_vit_backward_input': (_i, [_vp] * 6 + [_i] * 5 + [_vp] + [_vp, _i, _f, _i]),
    'rovit_vit_backward_relevance': (_i, [_vp] * 4 + [_i] * 3 + [_vp] * 3),
    'rovit_attention_relevance_step': (_i, [_vp] * 5 + [_i, _i, _vp]),
    'rovit_vit_embed': (_i, [_vp] * 4 + [_i, _i, _vp]),
    'rovit_vit_forward_tokens': (_i, [_vp, _vp, _i, _i, _vp, _vp, _i] + [_vp] * 4 + [_i, _i, _i, _vp]),
    'rovit_vit_ragged_workspace_bytes': (_sz, [_i, _i]),
    'rovit_vit_forward_ragged': (_i, [_vp, _vp, _i, _i] + [_vp] * 8 + [_i, _i, _i, _vp]),
    'rovit_patch_dropout_draw': (_i, [C.c_ulonglong, C.c_ulonglong, _vp, _vp, _vp, _i, _i, _vp]),
    'rovit_scatter_token_rows': (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    'rovit_vit_forward_train_tokens': (_i, [_vp, _vp, _vp, _i] + [_vp] * 5 + [_i] * 4 + [_vp]),
    'rovit_vit_backward_tokens': (_i, [_vp, _vp, _vp, _i] + [_vp] * 5 + [_i] * 3 + [_vp]),
    'rovit_gemm_nt': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp]),
    'rovit_gemm_resid_ln': (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp]),
    'rovit_mlp_stream_bytes': (_sz, []),
    'rovit_mlp_prepare_stream': (_i, [_vp, _vp, _vp, _vp]),
    'rovit_mlp_fused_fwd': (_i, [_vp] * 9 + [_f, _i, _i, _vp]),
    'rovit_mlp_prepare_stream_tail': (_i, [_vp] * 6),
    'rovit_block_tail_fwd': (_i, [_vp] * 14 + [_f, _i, _i, _vp]),
    'rovit_mlp_fused_bwd': (_i, [_vp] * 8 + [_i, _vp]),
    'rovit_mlp_prepare_stream_bwd': (_i, [_vp] * 5),
    'rovit_block_bwd_fused': (_i, [_vp] * 11 + [_i, _vp]),
    'rovit_block_bwd_fused_cls': (_i, [_vp] * 4 + [_i] + [_vp] * 7 + [_i, _vp]),
    'rovit_gemm_ln_bwd_cls': (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    'rovit_gemm_ln_bwd': (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'rovit_wgrad_splits': (_i, [_i, _i, _i]),
    'rovit_wgrad_workspace_bytes': (_sz, [_i, _i, _i]),
    'rovit_wgrad': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'rovit_wgrad_multi': (_i, [_vp] * 7 + [_i, _i, _i, _vp]),
    'rovit_wgrad_multi_ex': (_i, [_vp] * 9 + [_i, _i, _i, _vp]),
    'rovit_wgrad_reduce': (_i, [_vp, _i, _i, _i] + [_vp] * 8 + [_vp]),
    'rovit_attention_fwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    'rovit_attention_bwd': (_i, [_vp] * 5 + [_i] * 4 + [_f, _vp]),
    'rovit_attention_cls_fwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    'rovit_attention_cls_bwd': (_i, [_vp] * 5 + [_i] * 4 + [_f, _vp]),
    'rovit_attention_fwd_ragged': (_i, [_vp] * 5 + [_i, _i, _i, _f, _vp]),
    'rovit_attention_cls_fwd_ragged': (_i, [_vp] * 7 + [_i, _i, _i, _f, _vp]),
    'rovit_layernorm_fwd': (_i, [_vp, _vp, _vp, _i, _i, _f, _vp]),
    'rovit_layernorm_bwd': (_i, [_vp] * 5 + [_i, _i, _vp]),
    'rovit_im2col': (_i, [_vp, _vp, _i, _vp]),
    'rovit_patch_embed_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    'rovit_patch_embed_wgrad': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    'rovit_patch_embed_dgrad': (_i, [_vp, _i, _vp, _vp, _i, _i, _f, _i, _vp]),
    'rovit_cls_rows': (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    'rovit_cls_norm_fwd': (_i, [_vp] * 6 + [_i, _i, _f, _vp]),
    'rovit_cls_norm_bwd': (_i, [_vp] * 8 + [_i, _i, _i, _vp]),
    'rovit_pos_grad': (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    'rovit_prep_weight': (_i, [_vp] * 7 + [_i, _i, _vp]),
    'rovit_joint_loss': (_i, [_vp] * 7 + [_i] + [_vp] * 7 + [_i, _i, _f, _f, _f, _f, _vp]),
    'rovit_scale_buffers': (_i, [_vp, _vp, _i, _vp, _vp]),
    'rovit_sq_norm_accum': (_i, [_vp, _sz, _vp, _vp, _vp]),
    'rovit_mix_images': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _vp]),
    'rovit_clip_coef': (_i, [_vp, _f, _vp, _vp, _vp]),
    'rovit_adamw_flat': (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _f, _f, _f, _f, _f, _i, _vp]),
    'rovit_sq_norm_clip': (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    'rovit_adamw_flat_multi': (_i, [_vp] * 7 + [_i, _vp, _f, _f, _f, _f, _vp]),
    'rovit_adamw_ema_flat_multi': (_i, [_vp] * 9 + [_i, _vp, _f, _f, _f, _f, _vp]),
    'rovit_swap_flat_multi': (_i, [_vp, _vp, _vp, _i, _vp]),
    'rovit_joint_loss_mixed': (_i, [_vp, _vp]),
    'rovit_train_finalize': (_i, [_vp, _vp]),
    'rovit_eval_partials_doubles': (_sz, [_i]),
    'rovit_eval_accumulate': (_i, [_vp, _vp]),
    'rovit_eval_finalize': (_i, [_vp, _vp]),
    'rovit_eval_bootstrap_workspace_bytes': (_sz, [_i, _i]),
    'rovit_eval_bootstrap': (_i, [_vp, _vp]),
    'rovit_eval_selective_workspace_bytes': (_sz, [_i, _i, _i]),
    'rovit_eval_selective': (_i, [_vp, _vp]),
    'rovit_eval_calibrate_workspace_bytes': (_sz, [_i, _i]),
    'rovit_eval_calibrate': (_i, [_vp, _vp]),
    'rovit_eval_recalibrate': (_i, [_vp, _vp]),
    'rovit_kan_stats_words': (_sz, [_i, _i, _i]),
    'rovit_kan_stats_partials_doubles': (_sz, [_i, _i, _i, _i]),
    'rovit_kan_edge_stats': (_i, [_vp, _vp]),
    'rovit_kan_curves': (_i, [_vp] * 5 + [_i] * 4 + [_vp]),
    'rovit_kan_regrid_moment_words': (_sz, [_i, _i, _i]),
    'rovit_kan_regrid_diag_words': (_sz, [_i, _i]),
    'rovit_kan_regrid_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'rovit_kan_regrid_moments': (_i, [_vp, _vp]),
    'rovit_kan_regrid_solve': (_i, [_vp, _vp]),
    'rovit_shap_coalitions': (_i, [_vp, _vp]),
    'rovit_shap_gram': (_i, [_vp, _vp]),
    'rovit_shap_solve': (_i, [_vp, _vp]),
    'rovit_density_workspace_bytes': (_sz, [_i, _i, _i]),
    'rovit_density_moments': (_i, [_vp, _vp]),
    'rovit_density_score': (_i, [_vp, _vp]),
    'rovit_ood_metrics_workspace_bytes': (_sz, [_i, _i]),
    'rovit_ood_metrics': (_i, [_vp, _vp]),
    'rovit_sort_workspace_bytes': (_sz, [_vp, _i]),
    'rovit_sort_f32': (_i, [_vp, _vp]),
    'rovit_rank_workspace_bytes': (_sz, [_vp, _i, _i]),
    'rovit_rank_f32': (_i, [_vp, _vp]),
    'rovit_eval_finalize_rank_workspace_bytes': (_sz, [_i]),
    'rovit_eval_finalize_ex': (_i, [_vp, _i, _vp, _sz, _vp]),
    'rovit_eval_selective_rank_workspace_bytes': (_sz, [_i, _i, _i]),
    'rovit_eval_selective_ex': (_i, [_vp, _i, _vp, _sz, _vp]),
    'rovit_ood_metrics_rank_workspace_bytes': (_sz, [_i, _i]),
    'rovit_ood_metrics_ex': (_i, [_vp, _i, _vp, _sz, _vp]),
    'rovit_knn_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'rovit_knn_build': (_i, [_vp, _vp]),
    'rovit_knn_search': (_i, [_vp, _vp]),
    'rovit_eval_conformal_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'rovit_eval_conformal': (_i, [_vp, _vp]),
    'rovit_eval_conformal_apply_workspace_bytes': (_sz, [_i, _i]),
    'rovit_eval_conformal_apply': (_i, [_vp, _vp]),
    'rovit_augment_batch': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, C.c_ulonglong, C.c_ulonglong, _vp, _i, _i, _vp]),
    'rovit_corrupt_stats': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    'rovit_corrupt_batch': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    'rovit_laplace_weights': (_i, [_vp, _vp]),
    'rovit_laplace_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'rovit_laplace_gram': (_i, [_vp, _vp]),
    'rovit_laplace_predict': (_i, [_vp, _vp]),
    'rovit_influence_embed': (_i, [_vp, _vp]),
    'rovit_influence_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'rovit_influence_search': (_i, [_vp, _vp]),
    'rovit_tsne_workspace_bytes': (_sz, [_i, _i]),
    'rovit_tsne_affinities': (_i, [_vp, _vp]),
    'rovit_tsne_run': (_i, [_vp, _vp]),
    'rovit_tsne_random_init': (_i, [C.c_ulonglong, _vp, _i, _vp]),
    'rovit_kmeans_workspace_bytes': (_sz, [_i, _i, _i]),
    'rovit_kmeans_seed': (_i, [_vp, _vp]),
    'rovit_kmeans_run': (_i, [_vp, _vp]),
    'rovit_kmeans_assign': (_i, [_vp, _vp]),
    'rovit_kmeans_contingency': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    'rovit_attack_scratch_doubles': (_sz, [_i, _i, _i]),
    'rovit_attack_step_linf': (_i, [_vp] * 11 + [_i, _i, _i, _vp]),
    'rovit_attack_step_l2': (_i, [_vp] * 13 + [_i, _i, _i, _vp]),
    'rovit_attack_init': (_i, [_vp] * 5 + [_i, C.c_ulonglong, C.c_uint] + [_vp] * 5 + [_i, _i, _i, _vp]),
}


class HeadPhase(C.Structure):
    """``rovit_head_phase`` of include/rovit_hip.h, field for field (HOST arrays of device pointers inside)."""
    _fields_ = [('batch', _i), ('embed', _i), ('hid', _i), ('num_classes', _i), ('stage', _i), ('kan_layers', _i),
                ('kan_dims', _i * 5), ('kan_knots', _i * 4), ('kan_acts', _i * 4), ('drop_p', _f),
                ('seed', C.c_ulonglong), ('offset', C.c_ulonglong),
                ('features', _vp), ('head_params', _vp * 14), ('masks', _vp * 3), ('kan_w', _vp * 4), ('kan_knots_p', _vp * 4),
                ('kan_lw', _vp * 4), ('kan_lb', _vp * 4),
                ('hidden', _vp), ('cls', _vp), ('ord', _vp), ('mu', _vp), ('lv', _vp), ('kan_out', _vp * 4),
                ('g_cls', _vp), ('g_ord', _vp), ('g_mu', _vp), ('g_lv', _vp), ('g_kan', _vp),
                ('d_features', _vp), ('dpre', _vp), ('kan_gz', _vp * 4), ('head_grads', _vp * 14), ('kan_dw', _vp * 4),
                ('kan_dlw', _vp * 4), ('kan_dlb', _vp * 4), ('want_param_grads', _i)]


class HeadMC(C.Structure):
    """``rovit_head_mc`` of include/rovit_hip.h, field for field."""
    _fields_ = [('batch', _i), ('embed', _i), ('hid', _i), ('num_classes', _i), ('stage', _i), ('num_samples', _i), ('drop_p', _f),
                ('seed', C.c_ulonglong), ('offset', C.c_ulonglong), ('features', _vp), ('head_params', _vp * 14),
                ('class_probs', _vp), ('class_probs_std', _vp), ('pred_entropy', _vp), ('exp_entropy', _vp), ('mutual_info', _vp),
                ('ord_probs', _vp), ('ord_severity', _vp), ('ord_severity_std', _vp),
                ('unc_mu', _vp), ('epistemic_var', _vp), ('aleatoric_var', _vp), ('unc_std', _vp),
                ('s_cls', _vp), ('s_ord', _vp), ('s_mu', _vp), ('s_lv', _vp)]


class EvalBatch(C.Structure):
    """``rovit_eval_batch`` of include/rovit_hip.h, field for field."""
    _fields_ = [('batch', _i), ('num_classes', _i), ('offset', _i), ('capacity', _i), ('severity_is_int64', _i), ('loss_row', _i),
                ('loss_capacity', _i), ('cls_logits', _vp), ('kan_severity', _vp), ('log_var', _vp), ('class_labels', _vp),
                ('severity_labels', _vp), ('losses', _vp), ('probs', _vp), ('pred', _vp), ('label', _vp), ('sev_pred', _vp),
                ('sev_true', _vp), ('uncertainty', _vp), ('loss_table', _vp)]


class EvalFinal(C.Structure):
    """``rovit_eval_final`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('num_classes', _i), ('n_bins', _i), ('n_loss_rows', _i), ('probs', _vp), ('pred', _vp), ('label', _vp),
                ('sev_pred', _vp), ('sev_true', _vp), ('loss_table', _vp), ('bin_edges', _vp), ('rank_counts', _vp), ('partials', _vp),
                ('result', _vp)]


# word offsets inside rovit_eval_finalize's result block (the ROVIT_EVAL_* enum of include/rovit_hip.h)
EVAL_CONFUSION, EVAL_BIN_COUNT, EVAL_BIN_CORRECT, EVAL_RANK, EVAL_NONFINITE, EVAL_BAD_LABELS, EVAL_N = 0, 64, 128, 192, 195, 197, 198
EVAL_BIN_CONF, EVAL_BRIER, EVAL_ABS_ERR, EVAL_LOSS, EVAL_RESULT_WORDS = 200, 264, 265, 266, 272
EVAL_MAX_CLASSES, EVAL_MAX_BINS, EVAL_MAX_ROWS = 8, 64, 1 << 20


class EvalBoot(C.Structure):
    """``rovit_eval_boot`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('num_classes', _i), ('n_bins', _i), ('num_resamples', _i), ('max_workgroups', _i), ('seed', C.c_ulonglong),
                ('probs', _vp), ('pred', _vp), ('label', _vp), ('sev_pred', _vp), ('sev_true', _vp), ('bin_edges', _vp),
                ('rank_counts', _vp), ('perm', _vp), ('starts', _vp), ('workspace', _vp), ('workspace_bytes', _sz), ('table', _vp),
                ('blocks', _vp)]


# rovit_eval_bootstrap: the Philox stream word, the row threshold between H in LDS and H in the workspace, the workspace path's grid
# cap, the resample limit and the metric table's columns (the ROVIT_EVAL_BOOT_* constants of include/rovit_hip.h)
EVAL_BOOT_STREAM, EVAL_BOOT_LDS_ROWS, EVAL_BOOT_WORKSPACE_GRID, EVAL_BOOT_MAX_RESAMPLES = 0x426F6F74, 16384, 128, 65536
EVAL_BOOT_ACCURACY, EVAL_BOOT_MACRO_F1, EVAL_BOOT_WEIGHTED_F1, EVAL_BOOT_MAE, EVAL_BOOT_RHO, EVAL_BOOT_BRIER, EVAL_BOOT_ECE = range(7)
EVAL_BOOT_PRECISION, EVAL_BOOT_RECALL, EVAL_BOOT_F1, EVAL_BOOT_COLS = 7, 15, 23, 32


# rovit_eval_selective: limits, score and risk kinds, and the result block's layout (the ROVIT_EVAL_SEL_* names of include/rovit_hip.h)
EVAL_SEL_MAX_SCORES, EVAL_SEL_MAX_RISKS, EVAL_SEL_MAX_COVERAGES = 8, 4, 256
EVAL_SEL_CONFIDENCE, EVAL_SEL_ENTROPY, EVAL_SEL_SIGMA, EVAL_SEL_SCORE_COLUMN = 0, 1, 2, 3
EVAL_SEL_ERROR, EVAL_SEL_ABS_ERR, EVAL_SEL_RISK_COLUMN = 0, 1, 2
EVAL_SEL_NONFINITE_KEYS, EVAL_SEL_NONFINITE_RISKS, EVAL_SEL_NEGATIVE_RISKS, EVAL_SEL_BAD_LABELS, EVAL_SEL_N, EVAL_SEL_HEADER = 0, 1, 2, 3, 4, 8


class EvalSel(C.Structure):
    """``rovit_eval_sel`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('num_classes', _i), ('num_scores', _i), ('num_risks', _i), ('num_coverages', _i), ('max_workgroups', _i),
                ('score_kind', _i * EVAL_SEL_MAX_SCORES), ('risk_kind', _i * EVAL_SEL_MAX_RISKS),
                ('score_column', _vp * EVAL_SEL_MAX_SCORES), ('risk_column', _vp * EVAL_SEL_MAX_RISKS),
                ('probs', _vp), ('pred', _vp), ('label', _vp), ('sev_pred', _vp), ('sev_true', _vp), ('uncertainty', _vp),
                ('workspace', _vp), ('workspace_bytes', _sz), ('result', _vp), ('keys_out', _vp), ('risks_out', _vp)]


def eval_selective_offsets(S: int, K: int, P: int) -> dict:
    """Word offsets inside rovit_eval_selective's result block; ``words`` equals ROVIT_EVAL_SEL_WORDS(S, K, P)."""
    risks = EVAL_SEL_HEADER
    pairs = risks + K * (2 + P)
    thresholds = pairs + S * K * (1 + P)
    return {'risks': risks, 'pairs': pairs, 'thresholds': thresholds, 'words': thresholds + S * P}


# rovit_eval_calibrate: the search's shape, the limits, the clamp of the log-probabilities, the statuses and the result block's layout
# (the ROVIT_EVAL_CAL_* names of include/rovit_hip.h)
EVAL_CAL_ROUNDS, EVAL_CAL_CANDIDATES, EVAL_CAL_MAX_LEVELS = 4, 64, 64
EVAL_CAL_LOG_FLOOR, EVAL_CAL_U_MAX = -69.314718055994530942, 3.4657359027997265471          # ln 2^-100, ln 32
EVAL_CAL_INTERIOR, EVAL_CAL_AT_MIN, EVAL_CAL_AT_MAX = 0, 1, 2
EVAL_CAL_N_VALID, EVAL_CAL_BAD_LABELS, EVAL_CAL_N_REG, EVAL_CAL_BAD_SIGMA, EVAL_CAL_STATUS, EVAL_CAL_N = 0, 1, 2, 3, 4, 5
EVAL_CAL_U, EVAL_CAL_NLL, EVAL_CAL_NLL_CAL, EVAL_CAL_G_LO, EVAL_CAL_G_HI, EVAL_CAL_U_LO, EVAL_CAL_U_HI = 8, 9, 10, 11, 12, 13, 14
EVAL_CAL_SUM_Z2, EVAL_CAL_SUM_LOG_SIGMA, EVAL_CAL_COVERAGE = 15, 16, 24


class EvalCal(C.Structure):
    """``rovit_eval_cal`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('num_classes', _i), ('num_levels', _i), ('max_workgroups', _i), ('probs', _vp), ('label', _vp),
                ('sev_true', _vp), ('uncertainty', _vp), ('mu', _vp), ('half_widths', _vp), ('workspace', _vp), ('workspace_bytes', _sz),
                ('result', _vp)]


class EvalRecal(C.Structure):
    """``rovit_eval_recal`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('num_classes', _i), ('beta', C.c_double), ('sigma_scale', C.c_double), ('probs', _vp), ('uncertainty', _vp),
                ('probs_out', _vp), ('uncertainty_out', _vp)]


class TrainLoss(C.Structure):
    """``rovit_train_loss`` of include/rovit_hip.h, field for field."""
    _fields_ = [('batch', _i), ('num_classes', _i), ('severity_is_int64', _i), ('row', _i), ('capacity', _i),
                ('lam', _f), ('lambda_ord', _f), ('mu_unc', _f), ('nu_kan', _f), ('focal_gamma', _f),
                ('cls_logits', _vp), ('ordinal_logits', _vp), ('mu', _vp), ('log_var', _vp), ('kan_severity', _vp),
                ('class_targets_a', _vp), ('class_targets_b', _vp), ('severity_targets', _vp), ('focal_alpha', _vp),
                ('d_cls', _vp), ('d_ord', _vp), ('d_mu', _vp), ('d_lv', _vp), ('d_kan', _vp), ('losses_out', _vp), ('table', _vp)]


class TrainFinal(C.Structure):
    """``rovit_train_final`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n_rows', _i), ('capacity', _i), ('table', _vp), ('result', _vp)]


# rovit_joint_loss_mixed's epoch-table row (4-byte words) and rovit_train_finalize's result block (8-byte words): the ROVIT_TRAIN_* enum
TRAIN_ROW_LOSS, TRAIN_ROW_CORRECT, TRAIN_ROW_BATCH, TRAIN_ROW_NONFINITE, TRAIN_ROW_WORDS = 0, 5, 6, 7, 8
TRAIN_N_ROWS, TRAIN_SAMPLES, TRAIN_CORRECT, TRAIN_NONFINITE, TRAIN_LOSS, TRAIN_RESULT_WORDS = 0, 1, 2, 3, 4, 9
TRAIN_MAX_ROWS = 1 << 20


class KANStats(C.Structure):
    """``rovit_kan_stats`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('in_f', _i), ('out_f', _i), ('n_knots', _i), ('x', _vp), ('spline_w', _vp), ('knots', _vp), ('lin_w', _vp),
                ('lin_b', _vp), ('partials', _vp), ('result', _vp)]


# rovit_kan_edge_stats' section of one layer (the ROVIT_KAN_STATS_* enum and the layout comment of include/rovit_hip.h)
KAN_STATS_SUM, KAN_STATS_SQ, KAN_STATS_ABS, KAN_STATS_SPLINE_ABS, KAN_STATS_LINEAR_ABS = 0, 1, 2, 3, 4
KAN_STATS_MAX_ROWS, KAN_MAX_KNOTS = 1 << 22, 64


def kan_stats_offsets(in_f: int, out_f: int, n_knots: int) -> dict:
    """Word offsets inside one layer's section; ``words`` equals rovit_kan_stats_words(in_f, out_f, n_knots)."""
    e = in_f * out_f
    pre = 5 * e
    abs_in = pre + 2 * out_f
    occ = abs_in + in_f
    bad = occ + in_f * n_knots
    return {'edge': 0, 'pre': pre, 'abs_in': abs_in, 'occupancy': occ, 'nonfinite': bad, 'n': bad + 1, 'words': bad + 2}


class KANRegridMoments(C.Structure):
    """``rovit_kan_regrid`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('in_f', _i), ('n_knots_old', _i), ('n_knots_new', _i), ('x', _vp), ('knots_old', _vp), ('knots_new', _vp),
                ('workspace', _vp), ('workspace_bytes', _sz), ('moments', _vp)]


class KANRegridFit(C.Structure):
    """``rovit_kan_regrid_fit`` of include/rovit_hip.h, field for field."""
    _fields_ = [('in_f', _i), ('out_f', _i), ('n_knots_old', _i), ('n_knots_new', _i), ('moments', _vp), ('prior_g', _vp), ('prior_m', _vp),
                ('spline_w', _vp), ('spline_w_new', _vp), ('diagnostics', _vp)]


KAN_REGRID_MIN_KNOTS, KAN_REGRID_CHUNK_ROWS = 8, 256          # kan_grid.hip: the knot-count floor and the rows of one chunk


def kan_regrid_moment_offsets(in_f: int, n_knots_old: int, n_knots_new: int) -> dict:
    """Word offsets inside rovit_kan_regrid_moments' block; ``words`` equals rovit_kan_regrid_moment_words(in_f, nk, nk')."""
    nb, nbn = n_knots_old - 4, n_knots_new - 4
    m = 4 * in_f * nbn
    o = m + in_f * nbn * nb
    rows = o + 4 * in_f * nb
    return {'G': 0, 'M': m, 'O': o, 'rows': rows, 'nonfinite': rows + in_f, 'words': rows + 2 * in_f}


def kan_regrid_diag_offsets(in_f: int, out_f: int) -> dict:
    """Word offsets inside rovit_kan_regrid_solve's diagnostics block; ``words`` equals rovit_kan_regrid_diag_words(in_f, out_f)."""
    e = in_f * out_f
    return {'fit_ms': 0, 'target_ms': e, 'pivot_ratio': 2 * e, 'rows': 2 * e + in_f, 'nonfinite': 2 * e + 2 * in_f, 'status': 2 * e + 3 * in_f,
            'words': 2 * e + 3 * in_f + 1}


# rovit_density_moments / rovit_density_score / rovit_ood_metrics: limits, tile sizes and the result blocks' layouts (the ROVIT_DENSITY_* and
# ROVIT_OOD_* names of include/rovit_hip.h)
DENSITY_CHUNK_ROWS, DENSITY_SCORE_TILE, DENSITY_MAX_CHUNKS = 256, 64, 256
DENSITY_N, DENSITY_N_VALID, DENSITY_BAD_LABELS, DENSITY_BAD_ROWS, DENSITY_COUNTS, DENSITY_HEADER = 0, 1, 2, 3, 4, 16
OOD_MAX_LEVELS = 8
OOD_N_IN, OOD_N_OUT, OOD_BAD, OOD_TWO_U, OOD_K, OOD_THRESHOLD, OOD_OUT_BELOW, OOD_AP_OUT_SUM, OOD_AP_IN_SUM, OOD_WORDS = 0, 1, 2, 3, 4, 12, 20, 28, 29, 32


class DensityFit(C.Structure):
    """``rovit_density_fit`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('embed', _i), ('num_classes', _i), ('max_workgroups', _i), ('features', _vp), ('labels', _vp),
                ('workspace', _vp), ('workspace_bytes', _sz), ('result', _vp)]


class DensityScores(C.Structure):
    """``rovit_density_scores`` of include/rovit_hip.h, field for field."""
    _fields_ = [('batch', _i), ('embed', _i), ('num_classes', _i), ('max_workgroups', _i), ('features', _vp), ('whitening', _vp),
                ('class_means', _vp), ('background_whitening', _vp), ('background_mean', _vp), ('cls_logits', _vp),
                ('class_distances', _vp), ('background_distance', _vp), ('mahalanobis', _vp), ('nearest_class', _vp),
                ('relative_mahalanobis', _vp), ('energy', _vp), ('max_prob_score', _vp)]


class Ood(C.Structure):
    """``rovit_ood`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n_in', _i), ('n_out', _i), ('num_levels', _i), ('max_workgroups', _i), ('tpr_levels', C.c_double * OOD_MAX_LEVELS),
                ('scores_in', _vp), ('scores_out', _vp), ('workspace', _vp), ('workspace_bytes', _sz), ('result', _vp)]


# rovit_sort_f32 / rovit_rank_f32 and the rank method of the three score cards (the ROVIT_RANK_* and ROVIT_SORT_* names of
# include/rovit_hip.h).  RANK_SORT_ROWS: 'auto' sorts from this many rows on (measured, profiles/rank_time.jsonl).
RANK_AUTO, RANK_COUNT, RANK_SORT = 0, 1, 2
RANK_METHODS = {'auto': RANK_AUTO, 'count': RANK_COUNT, 'sort': RANK_SORT}
RANK_SORT_ROWS, SORT_MAX_COLUMNS, SORT_TILE, SORT_NAN_KEY = 32768, 16, 2048, 0xFFFFFFFF


class Sort(C.Structure):
    """``rovit_sort`` of include/rovit_hip.h, field for field."""
    _fields_ = [('num_columns', _i), ('max_workgroups', _i), ('n', _i * SORT_MAX_COLUMNS), ('x', _vp * SORT_MAX_COLUMNS),
                ('keys_sorted', _vp * SORT_MAX_COLUMNS), ('perm', _vp * SORT_MAX_COLUMNS), ('workspace', _vp), ('workspace_bytes', _sz)]


class Rank(C.Structure):
    """``rovit_rank`` of include/rovit_hip.h, field for field."""
    _fields_ = [('num_columns', _i), ('method', _i), ('max_workgroups', _i), ('reserved', _i), ('n', _i * SORT_MAX_COLUMNS),
                ('x', _vp * SORT_MAX_COLUMNS), ('less', _vp * SORT_MAX_COLUMNS), ('eq', _vp * SORT_MAX_COLUMNS),
                ('before', _vp * SORT_MAX_COLUMNS), ('perm', _vp * SORT_MAX_COLUMNS), ('workspace', _vp), ('workspace_bytes', _sz)]


def rank_method(method, n: int, what: str = 'rank') -> int:
    """``'auto'`` / ``'count'`` / ``'sort'`` as ROVIT_RANK_COUNT or ROVIT_RANK_SORT for n rows (ROVIT_RANK_AUTO resolved as the library does)."""
    if method not in RANK_METHODS:
        raise RovitHipError(f"{what}: the rank method must be one of {sorted(RANK_METHODS)}, got {method!r}")
    m = RANK_METHODS[method]
    return (RANK_SORT if n >= RANK_SORT_ROWS else RANK_COUNT) if m == RANK_AUTO else m


def density_chunk_rows(n: int) -> int:
    """Rows of one chunk of rovit_density_moments: 256 up to 65536 rows, then as many as keep the chunks at 256."""
    return DENSITY_CHUNK_ROWS * max(1, -(-n // (DENSITY_CHUNK_ROWS * DENSITY_MAX_CHUNKS)))


def density_offsets(E: int, C: int) -> dict:
    """Word offsets inside rovit_density_moments' result block; ``words`` equals ROVIT_DENSITY_WORDS(E, C)."""
    means = DENSITY_HEADER
    mean = means + C * E
    scatter = mean + E
    return {'means': means, 'mean': mean, 'scatter': scatter, 'words': scatter + E * E}


# rovit_knn_build / rovit_knn_search: limits, metrics and the build's result block (the ROVIT_KNN_* names of include/rovit_hip.h)
KNN_MAX_K, KNN_MAX_CLASSES, KNN_QUERY_TILE = 32, 1024, 64
KNN_L2, KNN_COSINE = 0, 1
KNN_N, KNN_N_VALID, KNN_BAD_ROWS, KNN_WORDS = 0, 1, 2, 4


class KnnIndex(C.Structure):
    """``rovit_knn_index`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('embed', _i), ('metric', _i), ('max_workgroups', _i), ('features', _vp), ('norms', _vp), ('valid', _vp),
                ('normalized', _vp), ('result', _vp)]


class KnnQuery(C.Structure):
    """``rovit_knn_query`` of include/rovit_hip.h, field for field."""
    _fields_ = [('batch', _i), ('n', _i), ('embed', _i), ('k', _i), ('metric', _i), ('num_classes', _i), ('max_workgroups', _i),
                ('reserved', _i), ('temperature', C.c_double), ('queries', _vp), ('rows', _vp), ('norms', _vp), ('valid', _vp),
                ('exclude', _vp), ('ref_labels', _vp), ('ref_severity', _vp), ('workspace', _vp), ('workspace_bytes', _sz),
                ('distances', _vp), ('indices', _vp), ('labels', _vp), ('severities', _vp), ('class_probs', _vp), ('cls', _vp),
                ('severity', _vp), ('kth_distance', _vp), ('mean_distance', _vp)]


# rovit_tsne_affinities / rovit_tsne_run: limits, the Philox stream word and the status blocks (the ROVIT_TSNE_* names of include/rovit_hip.h)
TSNE_MAX_ROWS, TSNE_MAX_ITER, TSNE_STREAM = 16384, 100000, 0x54534E45
TSNE_N, TSNE_N_VALID, TSNE_BAD_ROWS, TSNE_UNCONVERGED, TSNE_MIN_BETA, TSNE_MAX_BETA, TSNE_WORDS = 0, 1, 2, 3, 4, 5, 8
TSNE_RUN_ITERATIONS, TSNE_RUN_TRACE, TSNE_RUN_NONFINITE = 3, 4, 5


class TsneAffinity(C.Structure):
    """``rovit_tsne_affinity`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('embed', _i), ('metric', _i), ('symmetrize', _i), ('distances_only', _i), ('max_workgroups', _i),
                ('perplexity', C.c_double), ('features', _vp), ('workspace', _vp), ('workspace_bytes', _sz), ('P', _vp), ('beta', _vp),
                ('entropy', _vp), ('status', _vp)]


class TsneDescent(C.Structure):
    """``rovit_tsne_descent`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('n_iter', _i), ('exaggeration_iter', _i), ('kl_every', _i), ('center', _i), ('max_workgroups', _i),
                ('trace_capacity', _i), ('reserved', _i), ('early_exaggeration', _f), ('momentum_early', _f), ('momentum_late', _f),
                ('learning_rate', _f), ('P', _vp), ('Y', _vp), ('V', _vp), ('G', _vp), ('workspace', _vp), ('workspace_bytes', _sz),
                ('trace', _vp), ('status', _vp), ('grad_out', _vp), ('z_out', _vp)]


# rovit_kmeans_*: limits, the Philox stream word ("KMns") and the status block (the ROVIT_KMEANS_* names of include/rovit_hip.h)
KMEANS_MAX_ROWS, KMEANS_MAX_K, KMEANS_MAX_ITER, KMEANS_SEGMENT, KMEANS_STREAM = 1 << 20, 256, 100000, 1024, 0x4B4D6E73
(KMEANS_N, KMEANS_N_VALID, KMEANS_BAD_ROWS, KMEANS_N_ITER, KMEANS_DONE, KMEANS_EMPTY, KMEANS_EMPTY_EVENTS, KMEANS_ZERO_MEANS, KMEANS_W0_EVENTS,
 KMEANS_SHORT, KMEANS_CHANGED, KMEANS_WORDS) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16


ATTACK_STREAM, ATTACK_LINF, ATTACK_L2 = 0x41646176, 0, 1          # ROVIT_ATTACK_STREAM ("Adav"), the norms of rovit_attack_init


class KMeansProblem(C.Structure):
    """``rovit_kmeans_problem`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('embed', _i), ('k', _i), ('metric', _i), ('max_iter', _i), ('max_workgroups', _i), ('restart', _i), ('m', _i),
                ('seed', C.c_ulonglong), ('features', _vp), ('normalized', _vp), ('centroids', _vp), ('seeds', _vp), ('tap', _vp),
                ('labels', _vp), ('distance', _vp), ('second_distance', _vp), ('silhouette', _vp), ('workspace', _vp),
                ('workspace_bytes', _sz), ('status', _vp)]


# rovit_eval_conformal / rovit_eval_conformal_apply: limits, score kinds, the Philox stream word and the result blocks' layouts (the
# ROVIT_EVAL_CONF_* names of include/rovit_hip.h)
EVAL_CONF_MAX_SCORES, EVAL_CONF_MAX_LEVELS, EVAL_CONF_MAX_DEN, EVAL_CONF_STREAM = 8, 8, 1 << 20, 0x436F6E66
EVAL_CONF_LAC, EVAL_CONF_APS, EVAL_CONF_RAPS, EVAL_CONF_KAN_ABS, EVAL_CONF_MU_ABS, EVAL_CONF_MU_SCALED, EVAL_CONF_COLUMN = range(7)
EVAL_CONF_N, EVAL_CONF_BAD_LABELS, EVAL_CONF_N_LABELLED, EVAL_CONF_BAD_ROWS, EVAL_CONF_ENTRIES, EVAL_CONF_ENTRY_WORDS = 0, 1, 2, 8, 16, 6
EVAL_CONF_APPLY_SCORES = 8


class EvalConf(C.Structure):
    """``rovit_eval_conf`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('num_classes', _i), ('num_scores', _i), ('num_levels', _i), ('class_conditional', _i), ('randomized', _i),
                ('raps_k', _i), ('max_workgroups', _i), ('raps_lambda', _f), ('row_offset', C.c_uint), ('seed', C.c_ulonglong),
                ('score_kind', _i * EVAL_CONF_MAX_SCORES), ('alpha_num', C.c_uint * EVAL_CONF_MAX_LEVELS),
                ('alpha_den', C.c_uint * EVAL_CONF_MAX_LEVELS), ('score_column', _vp * EVAL_CONF_MAX_SCORES),
                ('probs', _vp), ('label', _vp), ('sev_pred', _vp), ('sev_true', _vp), ('uncertainty', _vp), ('mu', _vp), ('thresholds', _vp),
                ('workspace', _vp), ('workspace_bytes', _sz), ('result', _vp), ('scores_out', _vp), ('u_out', _vp), ('member_out', _vp)]


def eval_conformal_words(M: int, G: int, A: int) -> int:
    """ROVIT_EVAL_CONF_WORDS(M, G, A): entry e = (m G + g) A + a sits at EVAL_CONF_ENTRIES + 6 e."""
    return EVAL_CONF_ENTRIES + EVAL_CONF_ENTRY_WORDS * M * G * A


def eval_conformal_apply_words(M: int, A: int) -> int:
    """ROVIT_EVAL_CONF_APPLY_WORDS(M, A): score m sits at EVAL_CONF_APPLY_SCORES + m (16 + 32 A), its level a at + 16 + 32 a."""
    return EVAL_CONF_APPLY_SCORES + M * (16 + 32 * A)


class AugmentConfigC(C.Structure):
    """``rovit_augment_config`` of include/rovit_hip.h, field for field."""
    _fields_ = [(k, _f) for k in ('p_hflip', 'p_vflip', 'scale_lo', 'scale_hi', 'log_ratio_lo', 'log_ratio_hi', 'theta_max',
                                  'brightness', 'contrast', 'saturation', 'hue')]


class CorruptionC(C.Structure):
    """``rovit_corruption`` of include/rovit_hip.h, field for field."""
    _fields_ = [('kind', _i), ('param', _f), ('seed', C.c_ulonglong)]


CORRUPT_MAX_RADIUS = 18          # ROVIT_CORRUPT_MAX_RADIUS: gaussian ceil(3 sigma), defocus r, motion R + 1


# rovit_laplace_weights / rovit_laplace_gram / rovit_laplace_predict: limits, tile sizes and the result blocks' layouts (the ROVIT_LAPLACE_*
# names of include/rovit_hip.h)
LAPLACE_MAX_WEIGHTS, LAPLACE_MAX_CHUNKS, LAPLACE_TILE = 36, 64, 64
LAPLACE_BAD_LOGITS, LAPLACE_BAD_LOG_VAR, LAPLACE_COUNT_WORDS = 0, 1, 2
LAPLACE_N, LAPLACE_N_VALID, LAPLACE_BAD_ROWS, LAPLACE_HEADER = 0, 1, 2, 8


class LaplaceWeightArgs(C.Structure):
    """``rovit_laplace_weight_args`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('num_classes', _i), ('max_workgroups', _i), ('reserved', _i), ('cls_logits', _vp), ('log_var', _vp),
                ('cls_weights', _vp), ('mu_weights', _vp), ('counts', _vp)]


class LaplaceFit(C.Structure):
    """``rovit_laplace_fit`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('embed', _i), ('hid', _i), ('num_weights', _i), ('max_workgroups', _i), ('reserved', _i), ('features', _vp),
                ('fc1_weight', _vp), ('fc1_bias', _vp), ('weights', _vp), ('workspace', _vp), ('workspace_bytes', _sz), ('result', _vp)]


class LaplaceQuery(C.Structure):
    """``rovit_laplace_query`` of include/rovit_hip.h, field for field."""
    _fields_ = [('batch', _i), ('embed', _i), ('hid', _i), ('num_classes', _i), ('max_workgroups', _i), ('reserved', _i), ('features', _vp),
                ('fc1_weight', _vp), ('fc1_bias', _vp), ('whitening', _vp), ('cls_logits', _vp), ('logit_cov', _vp), ('logit_var', _vp),
                ('probs', _vp), ('confidence_score', _vp), ('mean_logit_var', _vp)]


def laplace_words(hid: int, K: int) -> int:
    """ROVIT_LAPLACE_WORDS(hid, K): matrix k sits at LAPLACE_HEADER + k (hid + 1)^2."""
    return LAPLACE_HEADER + K * (hid + 1) * (hid + 1)


# rovit_influence_embed / rovit_influence_search: limits, heads, targets and the counts (the ROVIT_INFLUENCE_* names of include/rovit_hip.h)
INFLUENCE_MAX_K, INFLUENCE_MAX_DIM = 32, 2304
INFLUENCE_CLS, INFLUENCE_MU = 0, 1
INFLUENCE_LOSS, INFLUENCE_OUTPUT = 0, 1
INFLUENCE_N, INFLUENCE_N_VALID, INFLUENCE_BAD_ROWS, INFLUENCE_BAD_LABELS, INFLUENCE_COUNT_WORDS = 0, 1, 2, 3, 4


class InfluenceRows(C.Structure):
    """``rovit_influence_rows`` of include/rovit_hip.h, field for field."""
    _fields_ = [('n', _i), ('embed', _i), ('hid', _i), ('num_classes', _i), ('head', _i), ('target', _i), ('max_workgroups', _i),
                ('reserved', _i), ('features', _vp), ('fc1_weight', _vp), ('fc1_bias', _vp), ('whitening', _vp), ('cls_logits', _vp),
                ('labels', _vp), ('mu', _vp), ('log_var', _vp), ('severity', _vp), ('rows', _vp), ('residual', _vp), ('norm2', _vp),
                ('valid', _vp), ('counts', _vp)]


class InfluenceQuery(C.Structure):
    """``rovit_influence_query`` of include/rovit_hip.h, field for field."""
    _fields_ = [('batch', _i), ('n', _i), ('dim', _i), ('k', _i), ('relative', _i), ('max_workgroups', _i), ('max_splits', _i),
                ('reserved', _i), ('queries', _vp), ('query_valid', _vp), ('rows', _vp), ('norm2', _vp), ('valid', _vp), ('exclude', _vp),
                ('ref_labels', _vp), ('ref_severity', _vp), ('workspace', _vp), ('workspace_bytes', _sz),
                ('pro_scores', _vp), ('pro_indices', _vp), ('opp_scores', _vp), ('opp_indices', _vp), ('pro_labels', _vp),
                ('opp_labels', _vp), ('pro_severities', _vp), ('opp_severities', _vp)]


# rovit_shap_coalitions / rovit_shap_gram / rovit_shap_solve: the Philox stream word, the limits and the factor block's layout (the
# ROVIT_SHAP_* names of include/rovit_hip.h)
SHAP_STREAM, SHAP_PATCHES, SHAP_WORDS, SHAP_MAX_SAMPLES = 0x53686170, 196, 7, 1 << 20


class ShapCoalitionArgs(C.Structure):
    """``rovit_shap_coalition_args`` of include/rovit_hip.h, field for field."""
    _fields_ = [('num_players', _i), ('num_samples', _i), ('max_workgroups', _i), ('reserved', _i), ('seed', C.c_ulonglong), ('pairs', _vp),
                ('pair_weights', _vp), ('players', _vp), ('drop_offsets', _vp), ('drop_words', C.c_longlong), ('bits', _vp), ('weights', _vp),
                ('src_replace', _vp), ('src_drop', _vp)]


class ShapGramArgs(C.Structure):
    """``rovit_shap_gram_args`` of include/rovit_hip.h, field for field."""
    _fields_ = [('num_players', _i), ('num_samples', _i), ('max_workgroups', _i), ('reserved', _i), ('bits', _vp), ('weights', _vp),
                ('gram', _vp), ('factor', _vp)]


class ShapSolveArgs(C.Structure):
    """``rovit_shap_solve_args`` of include/rovit_hip.h, field for field."""
    _fields_ = [('num_players', _i), ('num_samples', _i), ('batch', _i), ('num_targets', _i), ('max_workgroups', _i), ('reserved', _i),
                ('bits', _vp), ('weights', _vp), ('factor', _vp), ('values', _vp), ('v_empty', _vp), ('v_full', _vp), ('players', _vp),
                ('phi', _vp), ('phi32', _vp), ('patch_map', _vp), ('fit_rmse', _vp), ('ok', _vp)]


def shap_factor_offsets(P: int) -> dict:
    """Word offsets inside rovit_shap_gram's factor block (ROVIT_SHAP_FACTOR_WORDS(P) doubles): the lower Cholesky factor L (P, P)
    row-major, u = A^-1 1 (P), 1^T u, the smallest pivot, ok (1.0 / 0.0) and the sum of the weights."""
    return {'L': 0, 'u': P * P, 'sum_u': P * P + P, 'min_pivot': P * P + P + 1, 'ok': P * P + P + 2, 'sum_w': P * P + P + 3,
            'words': P * P + P + 4}


# entry points only the developer library exports (round-2 / round-3 experiments that lost; tools/ A/B them)
DEV_SIGNATURES = {
    'rovit_gemm_mlp_bwd': (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    'rovit_mlp_prepare_stream_tail_bwd': (_i, [_vp] * 5),
    'rovit_block_tail_bwd': (_i, [_vp] * 9 + [_i, _vp]),
}


class RovitHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the shared library (once).  Raises if it has not been built -- there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RovitHipError(
                f'{LIB_PATH} not found: build it with `python __graft_entry__.py` (or `make -C csrc`). '
                'The RoViT-KAN HIP path has no CPU fallback.')
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        if hasattr(lib, 'rovit_dev_set_knob'):           # developer library (make -C csrc dev; tools/ only)
            lib.rovit_dev_set_knob.restype, lib.rovit_dev_set_knob.argtypes = _i, [_i, _i, _i]
            for name, (res, args) in DEV_SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            # A/B of whole steps with the developer library: ROVIT_DEV_KNOBS="id=value,id=value" (common.h RovitKnob ids).
            # The product library exports no such entry point, so the variable does nothing there.
            for kv in filter(None, os.environ.get('ROVIT_DEV_KNOBS', '').split(',')):
                k, v = kv.split('=')
                lib.rovit_dev_set_knob(int(k), int(v), 0)
        if lib.rovit_version() != ABI_VERSION:
            raise RovitHipError(f'{LIB_PATH} has ABI version {lib.rovit_version()}, this binding was written for {ABI_VERSION}: '
                                'rebuild the library (`make -C csrc`); argument lists changed between versions')
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().rovit_last_error_string()
        raise RovitHipError(f'{what} failed (code {rc}): {msg.decode() if msg else ""}')


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RovitHipError('RoViT-KAN HIP kernels need tensors on a CUDA/HIP device (got a CPU tensor); '
                            'there is no CPU fallback in the product path')
    if not t.is_contiguous():
        raise RovitHipError('non-contiguous tensor passed to a HIP kernel')
    if t.device.index != torch.cuda.current_device():
        # kernels are enqueued on the CURRENT device's stream (stream_ptr): one process (or at least one current device)
        # per GPU, as the data-parallel launcher sets it up; a tensor of another device would be read by the wrong GPU
        raise RovitHipError(f'tensor on cuda:{t.device.index} but the current device is cuda:{torch.cuda.current_device()}: '
                            'call torch.cuda.set_device() / use `with torch.cuda.device(...)` around the model call')
    return t.data_ptr()


def ptr_array(tensors: Sequence[Optional[torch.Tensor]]):
    """HOST array of device pointers (kept alive by the caller for the duration of the call)."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = ptr(t)
    return arr


def call(name: str, *args) -> None:
    check(getattr(load(), name)(*args), name)
