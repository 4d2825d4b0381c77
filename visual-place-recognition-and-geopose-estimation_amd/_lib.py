"""ctypes binding of libvpr_amd.so — one prototype per entry point of include/vpr_amd.h and of its extension headers.

There is no fallback: if the library is missing, `lib()` raises with the build command.
"""
import ctypes
import os

import torch  # noqa: F401  MUST precede loading libvpr_amd.so: the library has to bind to the HIP
              # runtime PyTorch ships (torch/lib/libamdhip64.so), not to a second copy from /opt/rocm —
              # two runtimes in one process make every launch fail with hipErrorNoDevice.
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t,
                    c_uint32, c_uint64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ABI_VERSION = 6

STATUS_OK = 0


class SaladWeightsC(Structure):
    """struct vpr_salad_weights (device pointers; the two *_frag members may be null)."""
    _fields_ = [(n, c_void_p) for n in
                ("w1_sc", "b1_sc", "w2_s", "b2_s", "w2_c", "b2_c", "w1_t", "b1_t", "w2_t", "b2_t", "w2_s_frag", "w2_c_frag")]


class SaladWeightsF32C(Structure):
    """struct vpr_salad_weights_f32 (device pointers)."""
    _fields_ = [(n, c_void_p) for n in
                ("w1_sc", "b1_sc", "w2_s", "b2_s", "w2_c", "b2_c", "w1_t", "b1_t", "w2_t", "b2_t")]


class GemmProblemC(Structure):
    """struct vpr_gemm_problem (one member of vpr_gemm_nt_group_bf16)."""
    _fields_ = [("A", c_void_p), ("lda", c_int), ("a_group_rows", c_int), ("a_group_stride", c_longlong),
                ("W", c_void_p), ("ldw", c_int), ("bias", c_void_p), ("relu", c_int),
                ("C", c_void_p), ("ldc", c_int), ("out_is_bf16", c_int), ("M", c_int), ("N", c_int), ("K", c_int)]


_P = c_void_p
_GEMM = [_P, c_int, c_int, c_longlong, _P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P]    # vpr_gemm_problem fields, stream
# kNN family: operands (bf16: q, gallery; generic / fp8: q, q_scale, gallery, gallery_scale [, is_fp8 flag]), then B N D k,
# then index_base vals idx, then ws ws_bytes; the checked forms add norm_bound, status, uncertified; stream last
_KNN_BF16, _KNN_FP8 = [_P, _P] + [c_int] * 4, [_P, _P, _P, _P] + [c_int] * 4
_KNN_ANY = [_P, _P, _P, _P] + [c_int] * 5
_KNN_OUT, _KNN_WS, _KNN_CERT = [c_int, _P, _P], [_P, c_size_t], [c_float, _P, _P]
# head training: X ldx idx | order n batch, Y ldy, dims, six parameter / moment pointers, step, lr beta1 beta2 eps wd, loss kind, delta, loss out
_TRAIN_TAIL = [_P] * 6 + [c_int] + [c_double] * 5 + [c_int, c_double, _P]
_TRAIN_STEP = [_P, c_longlong, _P, _P, c_longlong] + [c_int] * 4 + _TRAIN_TAIL
_TRAIN_EPOCH = [_P, c_longlong, _P, c_int, c_int, _P, c_longlong] + [c_int] * 3 + _TRAIN_TAIL

# name -> (restype, argtypes); kept in one table so tests can check every symbol is exported
PROTOTYPES = {
    "vpr_status_string": (c_char_p, [c_int]),
    "vpr_abi_version": (c_int, []),
    "vpr_tuning_set": (c_int, [c_char_p, c_int, c_int]),
    "vpr_tuning_get": (c_int, [c_char_p, POINTER(c_int)]),
    "vpr_salad_workspace_bytes": (c_size_t, [c_int] * 7),
    "vpr_salad_aggregate": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(SaladWeightsC), c_float,
                                    c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "vpr_salad_aggregate_split": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(SaladWeightsC), c_float,
                                          c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_size_t, c_void_p]),
    "vpr_salad_stage_token": (c_int, [c_void_p, c_longlong, c_int, c_int, c_int, POINTER(SaladWeightsC), c_int, c_int, c_int, c_int,
                                      c_void_p, c_size_t, c_void_p]),
    "vpr_salad_stage_mlps": (c_int, [c_void_p, c_longlong, c_int, c_int, c_int, POINTER(SaladWeightsC), c_int, c_int, c_int, c_int,
                                     c_void_p, c_size_t, c_void_p]),
    "vpr_salad_stage_aggregate": (c_int, [c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_size_t, c_void_p]),
    "vpr_salad_f32_workspace_bytes": (c_size_t, [c_int] * 7),
    "vpr_salad_pack_w2_fragments": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "vpr_salad_aggregate_f32": (c_int, [c_void_p, c_longlong, c_void_p, c_longlong, c_int, c_int, c_int,
                                        POINTER(SaladWeightsF32C), c_float, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vpr_salad_aggregate_train": (c_int, [c_void_p, c_longlong, c_void_p, c_longlong, c_int, c_int, c_int, POINTER(SaladWeightsC),
                                          c_float, c_int, c_int, c_int, c_int, c_int, c_double, c_uint64, c_uint32, c_longlong,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vpr_salad_sinkhorn_aggregate": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                             c_int, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "vpr_gemm_nt_bf16": (c_int, _GEMM),
    "vpr_gemm256_nt_bf16": (c_int, _GEMM),
    "vpr_gemm_nt_group_bf16": (c_int, [POINTER(GemmProblemC), c_int, c_void_p]),
    "vpr_knn_workspace_bytes": (c_size_t, [c_int] * 4),
    "vpr_knn_topk": (c_int, _KNN_BF16 + _KNN_OUT + _KNN_WS + [_P]),
    "vpr_knn_topk_fp8": (c_int, _KNN_FP8 + _KNN_OUT + _KNN_WS + [_P]),
    "vpr_knn_topk_checked": (c_int, _KNN_BF16 + _KNN_OUT + _KNN_WS + _KNN_CERT + [_P]),
    "vpr_knn_select_checked": (c_int, _KNN_BF16 + _KNN_OUT + _KNN_WS + _KNN_CERT + [_P]),
    "vpr_knn_topk_fp8_checked": (c_int, _KNN_FP8 + _KNN_OUT + _KNN_WS + _KNN_CERT + [_P]),
    "vpr_knn_topk_exhaustive": (c_int, _KNN_ANY + _KNN_OUT + _KNN_WS + [_P]),
    "vpr_quantize_fp8_rows": (c_int, [c_void_p, c_longlong, c_int, c_void_p, c_void_p, c_void_p]),
    "vpr_knn_scores": (c_int, [_P, _P, c_int, c_int, c_int] + _KNN_WS + [_P]),
    "vpr_knn_select": (c_int, _KNN_BF16 + _KNN_OUT + _KNN_WS + [_P]),
    "vpr_knn_topk_scores_stage": (c_int, _KNN_ANY + _KNN_WS + [_P]),
    "vpr_knn_topk_select_stage": (c_int, _KNN_ANY + _KNN_OUT + _KNN_WS + _KNN_CERT + [_P]),
    "vpr_knn_scores_kernel_name": (c_char_p, [c_int, c_int, c_int]),
    "vpr_knn_scores_ptr": (c_void_p, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int)]),
    "vpr_topk_merge": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vpr_pose_head_workspace_bytes": (c_size_t, [c_int] * 4),
    "vpr_pose_head": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                              c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "vpr_ln_meanpool_head": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float,
                                     c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "vpr_preprocess_workspace_bytes": (c_size_t, [c_int] * 3),
    "vpr_preprocess_resize_normalize": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                                c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                                POINTER(c_float), POINTER(c_float),
                                                c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vpr_layernorm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_longlong, c_int, c_void_p]),
    "vpr_bias_layernorm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_longlong, c_int, c_void_p]),
    "vpr_attention_qkv_split_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_longlong, c_int, c_int, c_float, c_void_p]),
    "vpr_skinny_linear_bf16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int,
                                       c_int, c_int, c_int, c_void_p]),
    "vpr_bias_layernorm_cls_linear_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_longlong,
                                                   c_int, c_longlong, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                                   c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "vpr_skinny_linear_stats_bf16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int,
                                             c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vpr_pose_head_pack_w1": (c_int, [c_void_p, c_longlong, c_void_p, c_void_p, c_void_p]),
    "vpr_pose_head_split_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "vpr_pose_head_fused_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "vpr_pose_head_fused_counter_bytes": (c_size_t, [c_int, c_int, c_int]),
    "vpr_pose_head_pack_w1_frag": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vpr_pose_head_fused": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "vpr_pose_head_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "vpr_head_train_workspace_bytes": (c_size_t, [c_int] * 4),
    "vpr_head_train_state_floats": (c_longlong, [c_int] * 3),
    "vpr_head_train_step": (c_int, _TRAIN_STEP + [_P, c_size_t, _P]),
    "vpr_head_train_epoch": (c_int, _TRAIN_EPOCH + [_P, c_size_t, _P]),
    "vpr_head_train_step_dropout": (c_int, _TRAIN_STEP + [c_double, c_uint64, _P, _P, c_size_t, _P]),      # p, seed, mask out
    "vpr_head_train_epoch_dropout": (c_int, _TRAIN_EPOCH + [c_double, c_uint64, _P, c_size_t, _P]),
    "vpr_patchify_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vpr_add_layernorm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p,
                                       c_longlong, c_int, c_void_p]),
    "vpr_attention_qkv_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "vpr_f32_to_bf16": (c_int, [c_void_p, c_void_p, c_longlong, c_void_p]),
}

# Additive extensions of ABI 6, one header each beside include/vpr_amd.h (present iff the symbol is exported); bound after
# PROTOTYPES, which stays the exact symbol list of vpr_amd.h.
POSE_TOP1, POSE_WEIGHTED = 0, 1
EXTENSION_PROTOTYPES = {
    # include/vpr_amd_retrieval.h: vals idx B k | labels n_labels | mode temperature | q_targets tau | scaler (host) |
    # pose64 pose4 hit_tau hit_region | stream
    "vpr_retrieval_pose": (c_int, [_P, _P, c_int, c_int, _P, c_longlong, c_int, c_double, _P, c_double, _P,
                                   _P, _P, _P, _P, _P]),
}
# include/vpr_amd_expand.h, a table of its own beside the one above
EXPAND_PROTOTYPES = {
    # q vals idx B D k | rows row_scales n_local index_base | n_use alpha q_weight add_query | partial out_f32 out_bf16 | stream
    "vpr_query_expand": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, c_double, c_double, c_int,
                                 _P, _P, _P, _P]),
    # partials R q B D | out_f32 out_bf16 | stream
    "vpr_query_expand_finish": (c_int, [_P, c_int, _P, c_int, c_int, _P, _P, _P]),
}
# include/vpr_amd_project.h, the third table
PROJECT_STREAM_MAX_ROWS = 128          # VPR_PROJECT_STREAM_MAX_ROWS: the largest `rows` on route 0
PROJECT_PROTOTYPES = {
    "vpr_project_workspace_bytes": (c_size_t, [c_int] * 3),                 # rows D d
    "vpr_project_route": (c_int, [c_int] * 3),                              # rows D d
    # x x_stride rows D | P c d normalize | out_f32 out_bf16 | workspace workspace_bytes | stream
    "vpr_project_rows": (c_int, [_P, c_longlong, c_int, c_int, _P, _P, c_int, c_int, _P, _P, _P, c_size_t, _P]),
}
# include/vpr_amd_rerank.h, the fourth table
RERANK_MAX_KC, RERANK_MAX_D = 128, 16384      # VPR_RERANK_MAX_KC, VPR_RERANK_MAX_D
RERANK_PROTOTYPES = {
    "vpr_rerank_workspace_bytes": (c_size_t, [c_int] * 2),                  # B kc
    # q q_is_f32 | idx B D kc | rows rows_are_f32 n_local index_base | k_out vals_out idx_out | workspace workspace_bytes | stream
    "vpr_rerank_rows": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
}

# include/vpr_amd_salad_stages.h, the fifth table
_PP = POINTER(c_void_p)
SALAD_STAGES_PROTOTYPES = {
    # workspace workspace_bytes | B n C m l t hidden | S F g H (out pointers) | slabs slab_rows
    "vpr_salad_stage_outputs": (c_int, [_P, c_size_t] + [c_int] * 7 + [_PP, _PP, _PP, _PP, POINTER(c_int), POINTER(c_longlong)]),
}

# include/vpr_amd_salad_anyres.h, the sixth table: the aggregation for a run-time patch-token count
SALAD_MAX_N = 576                             # VPR_SALAD_MAX_N
SALAD_ANYRES_PROTOTYPES = {
    # scores feats tokfeat | B n m l t | dustbin iters | out_f32 out_bf16 | stream
    "vpr_salad_sinkhorn_aggregate_n": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_float, c_int, _P, _P, _P]),
    # patch patch_img_stride cls cls_stride | B n C | weights dustbin | m l t hidden iters | out_f32 out_bf16 | workspace bytes | stream
    "vpr_salad_aggregate_n": (c_int, [_P, c_longlong, _P, c_longlong, c_int, c_int, c_int, POINTER(SaladWeightsC), c_float,
                                      c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "vpr_salad_aggregate_f32_n": (c_int, [_P, c_longlong, _P, c_longlong, c_int, c_int, c_int, POINTER(SaladWeightsF32C), c_float,
                                          c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
}

# include/vpr_amd_salad_hires.h, the seventh table: the aggregation for 65 .. 1369 patch tokens (448 / 518 px); the parameter
# lists of the sixth table
SALAD_HIRES_MAX_N = 1369                      # VPR_SALAD_HIRES_MAX_N
SALAD_HIRES_PROTOTYPES = {
    "vpr_salad_sinkhorn_aggregate_hires": SALAD_ANYRES_PROTOTYPES["vpr_salad_sinkhorn_aggregate_n"],
    "vpr_salad_aggregate_hires": SALAD_ANYRES_PROTOTYPES["vpr_salad_aggregate_n"],
    "vpr_salad_aggregate_f32_hires": SALAD_ANYRES_PROTOTYPES["vpr_salad_aggregate_f32_n"],
}

# include/vpr_amd_local.h, the eighth table: local-feature re-ranking by mutual-nearest-neighbour patch matches
LOCAL_MAX_N, LOCAL_MAX_L, LOCAL_MAX_KC = 256, 256, 128      # VPR_LOCAL_MAX_N, VPR_LOCAL_MAX_L, VPR_LOCAL_MAX_KC
LOCAL_SUM_ROUNDINGS = 10                                    # VPR_LOCAL_SUM_ROUNDINGS: L_sum of the score
LOCAL_PROTOTYPES = {
    "vpr_local_workspace_bytes": (c_size_t, [c_int] * 2),                   # B kc
    # q_local n_q | idx B kc | g_local n_g l n_local index_base min_sim | k_out vals_out idx_out matches_out |
    # pair_score pair_matches row_nn col_nn | workspace workspace_bytes | stream
    "vpr_local_rerank": (c_int, [_P, c_int, _P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_float, c_int, _P, _P, _P,
                                 _P, _P, _P, _P, _P, c_size_t, _P]),
}

# include/vpr_amd_salad_f32_stages.h, the ninth table: where the f32-accurate aggregation leaves planes, hidden values, S / F / g
SALAD_F32_STAGES_PROTOTYPES = {
    # workspace workspace_bytes | B n C m l t hidden | H Ht S F g | A1 cls3 W1 H2 | W1t W2s W2c W2t Ht2 (optional)
    "vpr_salad_f32_stage_outputs": (c_int, [_P, c_size_t] + [c_int] * 7 + [_PP] * 14),
}

# include/vpr_amd_patch_fp8.h, the tenth table: the local-feature re-ranking on e4m3 bytes of x * 2^PATCH_FP8_SHIFT
PATCH_FP8_SHIFT = 8                                         # VPR_PATCH_FP8_SHIFT
PATCH_FP8_MIN_L, PATCH_FP8_MAX_L = 64, 256                  # VPR_PATCH_FP8_MIN_L, VPR_PATCH_FP8_MAX_L
PATCH_FP8_PROTOTYPES = {
    "vpr_patch_quantize_fp8": (c_int, [_P, c_int, c_longlong, _P, _P]),     # x x_is_bf16 count out stream
    "vpr_patch_workspace_bytes_fp8": (c_size_t, [c_int] * 2),               # B kc
    "vpr_patch_rerank_fp8": LOCAL_PROTOTYPES["vpr_local_rerank"],           # the parameter list of the eighth table's call
}

# include/vpr_amd_local_hires.h, the eleventh table: both element types of the re-ranking for up to 1369 patches per image
LOCAL_HIRES_MAX_N = 1369                                    # VPR_LOCAL_HIRES_MAX_N
LOCAL_HIRES_PROTOTYPES = {
    "vpr_hires_local_workspace_bytes": LOCAL_PROTOTYPES["vpr_local_workspace_bytes"],
    "vpr_hires_local_rerank": LOCAL_PROTOTYPES["vpr_local_rerank"],         # the parameter list of the eighth table's call
    "vpr_hires_patch_rerank_fp8": LOCAL_PROTOTYPES["vpr_local_rerank"],
}

# include/vpr_amd_spatial.h, the twelfth table: spatial verification of the patch matches (a dominant-shift vote on the grid)
SPATIAL_MAX_N, SPATIAL_MAX_BINS, SPATIAL_MAX_TOL = 1369, 5329, 8     # VPR_SPATIAL_MAX_N, VPR_SPATIAL_MAX_BINS, VPR_SPATIAL_MAX_TOL
SPATIAL_PROTOTYPES = {
    "vpr_spatial_workspace_bytes": (c_size_t, [c_int] * 3),                 # B kc n_g
    # partner sim | P n_q gw_q n_g gw_g tol | score inliers matches shift inlier_mask | stream
    "vpr_spatial_verify": (c_int, [_P, _P] + [c_int] * 6 + [_P] * 6),
    # q_local n_q | idx B kc | g_local n_g l n_local index_base min_sim | k_out vals_out idx_out inliers_out |
    # pair_score pair_inliers pair_matches pair_shift row_nn col_nn | feat_is_fp8 gw_q gw_g tol | workspace workspace_bytes | stream
    "vpr_spatial_local_rerank": (c_int, [_P, c_int, _P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_float, c_int, _P, _P, _P]
                                 + [_P] * 6 + [c_int] * 4 + [_P, c_size_t, _P]),
}

# include/vpr_amd_similarity.h, the thirteenth table: the patch matches verified under scale, rotation and shift (256 two-match
# hypotheses of a similarity transform)
SIM_MAX_N, SIM_MAX_SIDE, SIM_HYPOTHESES, SIM_MAX_SCALE, SIM_MAX_TOL = 1369, 37, 256, 2, 8   # the VPR_SIM_* macros
SIMILARITY_PROTOTYPES = {
    "vpr_similarity_workspace_bytes": (c_size_t, [c_int] * 3),              # B kc n_g
    # partner sim | P n_q gw_q n_g gw_g tol | score inliers matches model inlier_mask | stream
    "vpr_similarity_verify": (c_int, [_P, _P] + [c_int] * 6 + [_P] * 6),
    # the parameter list of vpr_spatial_local_rerank; pair_model in the place of pair_shift
    "vpr_similarity_local_rerank": SPATIAL_PROTOTYPES["vpr_spatial_local_rerank"],
}


def local_hires_sum_roundings(n_g: int) -> int:
    """VPR_LOCAL_HIRES_SUM_ROUNDINGS: L_sum of the score summed in blocks of 256 columns."""
    return LOCAL_SUM_ROUNDINGS + (n_g + 255) // 256


def rerank_roundings(D: int, rows_are_f32: bool) -> int:
    """VPR_RERANK_ROUNDINGS: L of the fine score, the roundings on the longest path from a product to the result."""
    return (D + 255) // 256 + 2 + 6 if rows_are_f32 else (D + 511) // 512 + 3 + 6


def library_path() -> str:
    """The in-tree library; VPR_AMD_LIBRARY points an A/B run at another build of it."""
    return os.environ.get("VPR_AMD_LIBRARY") or os.path.join(_HERE, "libvpr_amd.so")


def lib() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raises if it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} not found: the HIP extension is required (there is no CPU fallback). "
                "Build it with `python -c \"import __graft_entry__ as g; g.build()\"` "
                "or `make -C visual-place-recognition-and-geopose-estimation_amd/csrc`.")
        handle = ctypes.CDLL(path)
        for name, (restype, argtypes) in (list(PROTOTYPES.items()) + list(EXTENSION_PROTOTYPES.items())
                                          + list(EXPAND_PROTOTYPES.items()) + list(PROJECT_PROTOTYPES.items())
                                          + list(RERANK_PROTOTYPES.items()) + list(SALAD_STAGES_PROTOTYPES.items())
                                          + list(SALAD_ANYRES_PROTOTYPES.items()) + list(SALAD_HIRES_PROTOTYPES.items())
                                          + list(LOCAL_PROTOTYPES.items()) + list(SALAD_F32_STAGES_PROTOTYPES.items())
                                          + list(PATCH_FP8_PROTOTYPES.items()) + list(LOCAL_HIRES_PROTOTYPES.items())
                                          + list(SPATIAL_PROTOTYPES.items()) + list(SIMILARITY_PROTOTYPES.items())):
            fn = getattr(handle, name)   # AttributeError if a declared symbol is not exported
            fn.restype = restype
            fn.argtypes = argtypes
        if handle.vpr_abi_version() != ABI_VERSION:
            raise RuntimeError("libvpr_amd.so ABI version mismatch; rebuild the library")
        _LIB = handle
    return _LIB


def tuning_set(name: str, value=None) -> None:
    """Set (or, with value None, unset) one of the library's A/B switches.  The library reads the VPR_* environment
    variables once at load; afterwards this call is the only way to change them (scripts/, tests)."""
    st = lib().vpr_tuning_set(name.encode(), 0 if value is None else int(value), int(value is None))
    check(st, f"vpr_tuning_set({name})")


def tuning_get(name: str):
    v = c_int(0)
    st = lib().vpr_tuning_get(name.encode(), ctypes.byref(v))
    if st == 1:
        return None
    check(st, f"vpr_tuning_get({name})")
    return v.value


class tuning:
    """Context manager: `with _lib.tuning(VPR_KNN_VARIANT=6): ...` sets the switches and restores the old values."""

    def __init__(self, **switches):
        self.switches, self.old = switches, {}

    def __enter__(self):
        for k, v in self.switches.items():
            self.old[k] = tuning_get(k)
            tuning_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            tuning_set(k, v)
        return False


def check(status: int, what: str) -> None:
    if status != STATUS_OK:
        msg = lib().vpr_status_string(status).decode()
        raise RuntimeError(f"{what} failed: {msg} (status {status})")
