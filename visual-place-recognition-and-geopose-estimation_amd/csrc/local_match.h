// local_match.h — what local_match.hip (the two local-feature match kernels, their one launch path, the order stage) shares with
// the verification stages spatial.hip and similarity.hip: the workspace rules, the argument checks in the order the contracts
// state, the score's block sum (also the verification kernels'), and the two launches the verified calls use: the match launch
// with the match list, and the order stage.
#pragma once
#include <float.h>
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_local.h"
#include "../../include/vpr_amd_patch_fp8.h"
#include "../../include/vpr_amd_local_hires.h"

namespace vpr {

inline size_t lm_ws_half(int B, int kc) { return align_up((size_t)(B > 0 ? B : 1) * kc * sizeof(float), 256); }
inline size_t lm_ws_bytes(int B, int kc) {
  if (B < 0 || kc < 1 || kc > VPR_LOCAL_MAX_KC) return 0;
  return 2 * lm_ws_half(B, kc);                                       // f32 scores | i32 match counts
}

// The workspace of a verified call (spatial.hip, similarity.hip): the order stage's arrays, then the match list.
inline size_t sv_ws_list(int B, int kc, int n_g) { return align_up((size_t)(B > 0 ? B : 1) * kc * n_g * sizeof(int32_t), 256); }
inline size_t sv_ws_bytes(int B, int kc, int n_g) {
  if (lm_ws_bytes(B, kc) == 0 || n_g < 1 || n_g > VPR_LOCAL_HIRES_MAX_N) return 0;
  return lm_ws_bytes(B, kc) + 2 * sv_ws_list(B, kc, n_g);            // f32 scores | i32 counts | i32 partners | f32 similarities
}

// The status of a call, in the order the headers state; VPR_OK = launch.  max_n = the form's patch limit, l_step = the
// width's granule (32 bf16, 64 e4m3).  Three parts, so that a call with arguments of its own (spatial.hip, similarity.hip) can append its
// refusals to each group: the invalid arguments, the unsupported shapes, the alignment.
inline int lm_check_args(const void* q_local, int n_q, const int32_t* idx, int B, int kc, const void* g_local, int n_g, int l,
                         int n_local, int index_base, float min_sim, int k_out, const float* vals_out, const int32_t* idx_out,
                         const void* workspace) {
  if (!q_local || !idx || !g_local || !vals_out || !idx_out || !workspace) return VPR_ERR_INVALID_ARG;
  if (B < 0 || n_q < 0 || n_g < 0 || l < 0 || kc < 0 || n_local < 0 || index_base < 0) return VPR_ERR_INVALID_ARG;
  if (k_out < 1 || k_out > kc) return VPR_ERR_INVALID_ARG;
  if (isnan(min_sim)) return VPR_ERR_INVALID_ARG;
  return VPR_OK;
}
inline int lm_check_shape(int n_q, int kc, int n_g, int l, int l_step, int max_n) {
  if (kc > VPR_LOCAL_MAX_KC || n_q == 0 || n_q > max_n || n_g == 0 || n_g > max_n) return VPR_ERR_UNSUPPORTED;
  if (l == 0 || l % l_step != 0 || l > VPR_LOCAL_MAX_L) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}
inline int lm_check_align(const void* q_local, const int32_t* idx, const void* g_local, const float* vals_out, const int32_t* idx_out,
                          const int32_t* matches_out, const float* pair_score, const int32_t* pair_matches, const int32_t* row_nn,
                          const int32_t* col_nn, const void* workspace) {
  if (!aligned16(q_local) || !aligned16(g_local) || !aligned16(workspace)) return VPR_ERR_UNSUPPORTED;   // read as 16-byte chunks
  if (!aligned4(idx) || !aligned4(vals_out) || !aligned4(idx_out) || !aligned4(matches_out) || !aligned4(pair_score) ||
      !aligned4(pair_matches) || !aligned4(row_nn) || !aligned4(col_nn)) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}
inline int lm_check(const void* q_local, int n_q, const int32_t* idx, int B, int kc, const void* g_local, int n_g, int l, int l_step,
                    int max_n, int n_local, int index_base, float min_sim, int k_out, const float* vals_out, const int32_t* idx_out,
                    const int32_t* matches_out, const float* pair_score, const int32_t* pair_matches, const int32_t* row_nn,
                    const int32_t* col_nn, const void* workspace, size_t workspace_bytes) {
  VPR_TRY_LAUNCH(lm_check_args(q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out, idx_out, workspace));
  VPR_TRY_LAUNCH(lm_check_shape(n_q, kc, n_g, l, l_step, max_n));
  VPR_TRY_LAUNCH(lm_check_align(q_local, idx, g_local, vals_out, idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace));
  if (workspace_bytes < lm_ws_bytes(B, kc)) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

// The score sum that the three contracts state (vpr_amd_local.h inside a block of 256 columns, vpr_amd_local_hires.h over the
// blocks), shared by the two match kernels and the verification kernels (spatial.hip, similarity.hip).
// lm_block_partials: waves 0 .. 3, block t: thread j - 256 t holds column j's contribution (+0 where it does not count) and
// whether it counts; the wave_sum butterfly, the wave's sum and count to s_part / s_cnt [t][4].
__device__ __forceinline__ void lm_block_partials(float contrib, int counted, int t, int lane, int wave, float* s_part, int* s_cnt) {
  const float ws = wave_sum(contrib);
  int wc = counted;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wc += __shfl_xor(wc, o, 64);
  if (lane == 0) { s_part[t * 4 + wave] = ws; s_cnt[t * 4 + wave] = wc; }
}
// lm_fold_block: one thread, after a barrier: block t's four wave sums added to +0 in wave order and clamped (the score of
// vpr_amd_local.h when there is one block); its four counts added to `count`.
__device__ __forceinline__ float lm_fold_block(const float* s_part, const int* s_cnt, int t, int& count) {
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) { s += s_part[t * 4 + w]; count += s_cnt[t * 4 + w]; }
  return fminf(fmaxf(s, -FLT_MAX), FLT_MAX);                          // every term is finite; an overflowing sum is clamped
}
// lm_fold_blocks: the block sums added to a running +0 in block order, the running sum clamped after each addition
// (vpr_amd_local_hires.h).  With one block this is lm_fold_block followed by +0 + x, and x is never -0 (it is itself
// +0 + ...): the same bits.
__device__ __forceinline__ void lm_fold_blocks(const float* s_part, const int* s_cnt, int ncb, float& score, int& count) {
  float run = 0.f;
  int c = 0;
  for (int t = 0; t < ncb; ++t) run = fminf(fmaxf(run + lm_fold_block(s_part, s_cnt, t, c), -FLT_MAX), FLT_MAX);
  score = run;
  count = c;
}

// local_match.hip: the order stage of both forms, B workgroups of 128 threads (order_rank of vpr_common.h)
int launch_local_order(const float* scores, const int32_t* matches, const int32_t* idx, int B, int kc, int n_local, int index_base,
                       int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out, hipStream_t stream);

// The match launch alone of either element type (fp8: e4m3 bytes), for a caller that has checked its arguments against the
// limits of include/vpr_amd_local_hires.h; local_match.hip chooses the kernel.  match_q / match_sim [B, kc, n_g], both non-null:
// the match list, c(j) and S[c(j)][j] of a matched column, (-1, +0) of any other and of a non-live candidate.
int launch_local_match_list(bool fp8, const void* q_local, int n_q, const int32_t* idx, int B, int kc, const void* g_local, int n_g,
                            int l, int n_local, int index_base, float min_sim, float* ws_score, int32_t* ws_matches, int32_t* row_nn,
                            int32_t* col_nn, int32_t* match_q, float* match_sim, hipStream_t stream);

}  // namespace vpr
