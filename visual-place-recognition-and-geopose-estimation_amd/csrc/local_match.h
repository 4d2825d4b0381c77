// local_match.h — what the two local-feature match kernels share (local_match.hip: up to 256 patches, a candidate whole in LDS;
// local_match_hires.hip: up to 1369, tiled over both patch axes): the comparison of the argmax folds, the swizzle of the staged
// features, the workspace rule, the argument checks in the order both contracts state, and the order stage's launch.
#pragma once
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_local.h"
#include "../../include/vpr_amd_patch_fp8.h"

namespace vpr {

constexpr int LM_WAVES = 8;                         // = 256 / 32 row tiles of a row block
constexpr int LM_THREADS = LM_WAVES * WAVE;

// a beats b: a exists and (b does not, or a's value is larger, or equal with the lower index)
__device__ __forceinline__ bool lm_better(float av, int ai, float bv, int bi) {
  return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi));
}

// Swizzle of the staged features: chunk c of row r (a row is CPR chunks of 16 B: L / 8 for bf16, L / 16 for e4m3) sits at
// chunk c ^ f(r) of its row, f(r) = (r >> SH) & MASK with (SH, MASK) = (0, 15) if 16 | CPR, (1, 7) if 8 | CPR, else (2, 3): the
// 16 rows of a ds_read_b128 lane group at one logical chunk fall into 16 distinct 16-byte slots of the 256-byte bank row.  CPR
// is a multiple of 4, and f(r) stays below the largest power of two (<= 16) dividing CPR: the XOR stays inside the row, and
// chunks 2 m and 2 m + 1 (the two reads of an e4m3 operand) stay a pair.  Restated and checked exhaustively on the host for
// every supported width of both elements (tests/test_local_match_fp8_cpu.py).
template <int CPR>
__device__ __forceinline__ int lm_off(int row, int chunk) {
  static_assert(CPR % 4 == 0 && CPR <= 32, "a row is a whole number of 64-byte groups");
  constexpr int SH = CPR % 16 == 0 ? 0 : CPR % 8 == 0 ? 1 : 2, MASK = CPR % 16 == 0 ? 15 : CPR % 8 == 0 ? 7 : 3;
  return (row * CPR + (chunk ^ ((row >> SH) & MASK))) << 4;
}

inline size_t lm_ws_half(int B, int kc) { return align_up((size_t)(B > 0 ? B : 1) * kc * sizeof(float), 256); }
inline size_t lm_ws_bytes(int B, int kc) {
  if (B < 0 || kc < 1 || kc > VPR_LOCAL_MAX_KC) return 0;
  return 2 * lm_ws_half(B, kc);                                       // f32 scores | i32 match counts
}

// The status of a call, in the order the headers state; VPR_OK = launch.  max_n = the form's patch limit, l_step = the
// width's granule (32 bf16, 64 e4m3).
inline int lm_check(const void* q_local, int n_q, const int32_t* idx, int B, int kc, const void* g_local, int n_g, int l, int l_step,
                    int max_n, int n_local, int index_base, float min_sim, int k_out, const float* vals_out, const int32_t* idx_out,
                    const int32_t* matches_out, const float* pair_score, const int32_t* pair_matches, const int32_t* row_nn,
                    const int32_t* col_nn, const void* workspace, size_t workspace_bytes) {
  if (!q_local || !idx || !g_local || !vals_out || !idx_out || !workspace) return VPR_ERR_INVALID_ARG;
  if (B < 0 || n_q < 0 || n_g < 0 || l < 0 || kc < 0 || n_local < 0 || index_base < 0) return VPR_ERR_INVALID_ARG;
  if (k_out < 1 || k_out > kc) return VPR_ERR_INVALID_ARG;
  if (isnan(min_sim)) return VPR_ERR_INVALID_ARG;
  if (kc > VPR_LOCAL_MAX_KC || n_q == 0 || n_q > max_n || n_g == 0 || n_g > max_n) return VPR_ERR_UNSUPPORTED;
  if (l == 0 || l % l_step != 0 || l > VPR_LOCAL_MAX_L) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(q_local) || !aligned16(g_local) || !aligned16(workspace)) return VPR_ERR_UNSUPPORTED;   // read as 16-byte chunks
  if (!aligned4(idx) || !aligned4(vals_out) || !aligned4(idx_out) || !aligned4(matches_out) || !aligned4(pair_score) ||
      !aligned4(pair_matches) || !aligned4(row_nn) || !aligned4(col_nn)) return VPR_ERR_UNSUPPORTED;
  if (workspace_bytes < lm_ws_bytes(B, kc)) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

// local_match.hip: the order stage of both forms, B workgroups of 128 threads (order_rank of vpr_common.h)
int launch_local_order(const float* scores, const int32_t* matches, const int32_t* idx, int B, int kc, int n_local, int index_base,
                       int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out, hipStream_t stream);

}  // namespace vpr
