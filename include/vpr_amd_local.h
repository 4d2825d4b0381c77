/* vpr_amd_local.h — local-feature re-ranking: mutual-nearest-neighbour matching of patch features, on the device.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the eighth one: it adds two entry points and changes nothing that
 * vpr_amd.h or an earlier extension header declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_local_rerank (dlsym / ctypes lookup; vpr_local_workspace_bytes comes with it); a
 * library built before it simply lacks the symbols.  Status codes and the stream / graph-capture rules are those of vpr_amd.h.
 *
 * What it computes.  A search by global descriptors leaves query b with kc candidate images, idx[b, j].  Every image also
 * has LOCAL features: n patch descriptors of width l (SALAD's cluster_features output, L2-normalised, bf16).  This call
 * scores each candidate by the patches it shares with the query as mutual nearest neighbours and returns the k_out best by
 * that score.  The local features may be sharded like the gallery: a shard scores the candidates it owns, and the per-shard
 * lists go through vpr_topk_merge.
 *
 * vpr_local_rerank
 *   q_local    [B, n_q, l] bf16: the queries' local features.
 *   idx        [B, kc] int32 candidates, global gallery rows, as vpr_knn_topk* and vpr_topk_merge emit them.
 *   g_local    this shard's local features [n_local, n_g, l] bf16.  The shard owns global rows index_base ..
 *              index_base + n_local - 1 (index_base >= 0).
 *   Live candidate.  Exactly as in vpr_rerank_rows: candidate j is live iff index_base <= idx[b, j] < index_base + n_local.
 *     Anything else (-1, a row another shard owns, INT32_MIN, INT32_MAX, any other number) is never dereferenced: liveness
 *     is decided from the index alone, before any access, and no index can make a kernel read outside g_local.
 *   Similarity.  For a (query, live candidate) pair, S[i][j] = sum_d q[i][d] * g[j][d], i < n_q, j < n_g: the bf16 products
 *     are exact in f32 and accumulated in f32 by v_mfma_f32_32x32x16_bf16, one accumulator per S[i][j] starting at +0, the
 *     l / 16 k-steps in ascending order.  The order of the sum depends on l only.  A non-finite S[i][j] (NaN, +Inf, -Inf)
 *     counts as "no similarity": it compares below every number and is never a nearest neighbour.
 *   Nearest neighbours.  r(i) = argmax over j < n_g of S[i][.], c(j) = argmax over i < n_q of S[.][j]; ties (+0 and -0 are
 *     a tie) go to the lowest index; -1 if the row / column has no finite entry.  Rows and columns past n_q / n_g do not
 *     exist: the kernel pads its tiles to 32 and masks the padding out of both argmaxes.
 *   Match.  Column j is matched iff c(j) >= 0, r(c(j)) == j and S[c(j)][j] >= min_sim (f32 comparison).  matches = the
 *     number of matched columns; score = the f32 sum of S[c(j)][j] over the matched columns, in this fixed order: thread j
 *     owns column j (an unmatched column contributes +0); the 64 values of a wave are added by the wave_sum butterfly
 *     (v += v of lane xor 32, 16, 8, 4, 2, 1); the four wave sums are added to +0 in ascending wave order.  Roundings on
 *     the longest path from a similarity to the score: L_sum = VPR_LOCAL_SUM_ROUNDINGS = 6 + 4 = 10, so
 *     |score - exact sum| <= gamma_10 * sum_matched |S[c(j)][j]|, gamma_L = L u / (1 - L u), u = 2^-24.
 *     The score is always finite: a sum that overflows f32 is written as +-FLT_MAX (3.4028235e38).
 *   Order.  As vpr_rerank_rows (shared code): the live candidates by the key of vpr_topk_merge — score descending (the
 *     total order of the f32 bit patterns, +0 above -0), index ascending; the first k_out go to vals_out / idx_out /
 *     matches_out [B, k_out]; positions after the last live candidate are (-inf, -1) with matches 0.  matches_out[b][p]
 *     belongs to the entry at position p.  An index that occurs several times is scored and emitted as often as it occurs.
 *   Optional outputs, each NULL = not wanted; whether they are asked for changes no other output.
 *     pair_score / pair_matches [B, kc], candidate order: score and matches of candidate j; a non-live one is (-inf, 0).
 *     row_nn [B, kc, n_q] / col_nn [B, kc, n_g]: r(i) / c(j) of each pair; -1 throughout for a non-live candidate.
 *   Limits.  1 <= n_q, n_g <= VPR_LOCAL_MAX_N = 256 (224 px at patch 14).  l % 32 == 0, 32 <= l <= VPR_LOCAL_MAX_L = 256.
 *     1 <= k_out <= kc <= VPR_LOCAL_MAX_KC = 128.  q_local, g_local and workspace 16-byte aligned (read as 16-byte chunks).
 *   workspace  vpr_local_workspace_bytes(B, kc) bytes, 16-byte aligned: scores and match counts [B, kc] between the launches.
 *
 *   Two launches.  Match: (B, ceil(kc / 4)) workgroups of 8 waves; a workgroup walks its 4 candidates with the query's MFMA
 *   A-fragments in registers (wave w owns query rows 32 w .. 32 w + 31) and stages each live candidate's features in LDS
 *   (up to 128 KB + 17 KB, through the dynamic-LDS opt-in); a workgroup without a live candidate ends before it loads or
 *   stages anything.  Order: B workgroups of 128 threads, the order stage of vpr_rerank_rows.
 *
 * vpr_local_workspace_bytes(B, kc): bytes of workspace for that shape, monotone in B and kc, > 0 for every supported shape
 *   (B = 0 included); 0 = unsupported (B < 0, kc < 1, kc > 128).
 *
 * Determinism.  Query b's outputs depend on its own features, row b of idx and the shard only: not on B, not on its
 * position in the batch, not on kc beyond its live entries' relative order, not on the grid, not on which optional outputs
 * were asked for.  No atomics, no arrival counters, no spinning, no allocation; asynchronous on `stream`; safe under graph
 * capture.
 *
 * Status, decided before anything is launched, in this order; a refused call writes nothing:
 *   VPR_ERR_INVALID_ARG   NULL q_local, idx, g_local, vals_out, idx_out or workspace; B, n_q, n_g, l, kc, n_local or
 *                         index_base negative; k_out outside 1..kc; min_sim NaN.
 *   VPR_ERR_UNSUPPORTED   kc > 128; n_q or n_g 0 or > 256; l == 0, l % 32 != 0 or l > 256; q_local, g_local or workspace not
 *                         16-byte aligned; idx or an output not 4-byte aligned; then workspace_bytes <
 *                         vpr_local_workspace_bytes(B, kc).
 *   B == 0                VPR_OK, nothing is launched.
 */
#ifndef VPR_AMD_LOCAL_H
#define VPR_AMD_LOCAL_H

#include "vpr_amd.h"

#define VPR_LOCAL_MAX_N 256
#define VPR_LOCAL_MAX_L 256
#define VPR_LOCAL_MAX_KC 128
/* L_sum of the score: the six butterfly steps + the four adds in wave order */
#define VPR_LOCAL_SUM_ROUNDINGS 10

#ifdef __cplusplus
extern "C" {
#endif

size_t vpr_local_workspace_bytes(int B, int kc);

int vpr_local_rerank(const uint16_t* q_local, int n_q,
                     const int32_t* idx, int B, int kc,
                     const uint16_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                     int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                     float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                     void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_LOCAL_H */
