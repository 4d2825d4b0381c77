/* vpr_amd_rerank.h — two-tier retrieval: re-rank a coarse candidate list on full-precision rows, on the device.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the fourth one beside include/vpr_amd_retrieval.h,
 * include/vpr_amd_expand.h and include/vpr_amd_project.h: it adds two entry points and changes nothing that vpr_amd.h
 * declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff libvpr_amd.so exports the symbol vpr_rerank_rows
 * (dlsym / ctypes lookup; vpr_rerank_workspace_bytes comes with it); a library built before it simply lacks the symbols.
 * Status codes and the stream / graph-capture rules are those of vpr_amd.h.
 *
 * What it computes.  A search of a cheap gallery (e4m3 rows, PCA-projected rows) leaves query b with kc candidate rows,
 * idx[b, j], in the order of the coarse scores.  This call scores those candidates against the FINE rows — the full-width
 * descriptors in bf16 or f32 — and returns the k_out best by that fine score.  The fine gallery may be sharded like the
 * coarse one: a shard scores the candidates it owns, and the per-shard lists go through vpr_topk_merge.
 *
 * vpr_rerank_rows
 *   q          [B, D] queries of the fine rows' width: bf16 (q_is_f32 = 0) or f32 (q_is_f32 = 1).
 *   idx        [B, kc] int32 candidates, global gallery rows, as vpr_knn_topk* and vpr_topk_merge emit them.  Coarse scores
 *              are not an input.
 *   rows       this shard's fine rows [n_local, D]: bf16 (rows_are_f32 = 0) or f32 (rows_are_f32 = 1).  The shard owns global
 *              rows index_base .. index_base + n_local - 1 (index_base >= 0).
 *   Live candidate.  Candidate j is live iff index_base <= idx[b, j] < index_base + n_local.  Anything else (the -1 padding
 *     of a short list, a row another shard owns, INT32_MIN, INT32_MAX, any other number) is never dereferenced: liveness
 *     is decided from the index alone, before any row access, and no index can make a kernel read outside `rows`.
 *   Fine score.  s_j = sum_d q[b, d] * row_j[d] in f32, one fmaf per element; a bf16 operand is widened to f32 first
 *     (exact).  The order of the sum is fixed:
 *       - the row is cut into 16-byte chunks of E elements, E = VPR_RERANK_CHUNK_BF16 = 8 (bf16 rows) or
 *         VPR_RERANK_CHUNK_F32 = 4 (f32 rows); chunk c covers elements c*E .. c*E + E - 1;
 *       - lane l of a 64-lane wave owns chunks l, l + 64, l + 128, ...  and keeps E accumulators, a[e] for element e of
 *         a chunk, each starting at +0: a[e] = fmaf(q[c*E + e], row[c*E + e], a[e]) over its chunks in ascending c;
 *       - the lane's E accumulators are added pairwise: (a[0] + a[1]) + (a[2] + a[3]) for E = 4,
 *         ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])) for E = 8;
 *       - the 64 lane sums are added by a butterfly: v += v of lane (l xor 32), then xor 16, 8, 4, 2, 1.
 *     The order depends on D and the row dtype only: not on the query dtype, B, kc, the candidate's position, the position
 *     in the batch or the grid.  Roundings on the longest path from a product to the result:
 *       L = VPR_RERANK_ROUNDINGS(D, rows_are_f32) = ceil(D / (64 * E)) + log2(E) + 6
 *     (bf16 rows: D = 8448 -> 17 + 3 + 6 = 26; f32 rows: D = 8448 -> 33 + 2 + 6 = 41), so
 *     |s_j - exact| <= gamma_L * sum_d |q[b, d] * row_j[d]| with gamma_L = L u / (1 - L u), u = 2^-24.
 *     A lane requests up to 8 of its chunks before it adds the first, so the scattered row reads overlap; this does not
 *     change the order.
 *   Order.  The live candidates are sorted by the key of vpr_topk_merge: score descending (the total order of the f32 bit
 *     patterns, +0 above -0), index ascending.  The first k_out are written to vals_out / idx_out [B, k_out]; positions
 *     after the last live candidate, and thus every non-live candidate, are (-inf, -1).
 *   NaN fine score.  A live candidate whose fine score is NaN (a NaN or Inf in its row or in the query) is ordered after
 *     every numeric score (-inf included) and ahead of the padding, NaNs among themselves by ascending index, and is written
 *     as -inf with its index: the output stays inside the input contract of vpr_topk_merge and vpr_retrieval_pose.
 *   Duplicates.  An index that occurs several times is scored and emitted as often as it occurs (adjacent in the output).
 *     (vpr_knn_topk* and vpr_topk_merge emit distinct indices, and vpr_topk_merge expects them: a list with duplicates is
 *     this call's to order, not the merge's.)
 *   Limits.  1 <= k_out <= kc <= VPR_RERANK_MAX_KC = 128 (the limit of vpr_query_expand, so a merged list fits; one coarse
 *     search yields at most 64).  D % 64 == 0 and 64 <= D <= VPR_RERANK_MAX_D = 16384: the query is staged once per
 *     workgroup as f32 in LDS, 4 * D bytes, and 64 KB is what a workgroup gets without an opt-in.
 *   workspace  vpr_rerank_workspace_bytes(B, kc) bytes, 16-byte aligned: the f32 scores [B, kc] between the two launches.
 *
 *   Two launches.  Score: (B, ceil(kc / 8)) workgroups of 8 waves, one wave per candidate; a workgroup without a live
 *   candidate ends before it stages the query, a wave without one ends before any row access.  Order: B workgroups of 128
 *   threads; thread j counts the keys ahead of candidate j's (kc^2 comparisons per query; equal keys by position) and
 *   writes it if that rank is below k_out.
 *
 * vpr_rerank_workspace_bytes(B, kc): bytes of workspace for that shape, monotone in B and kc, > 0 for every supported shape
 *   (B = 0 included); 0 = unsupported (B < 0, kc < 1, kc > 128).
 *
 * Determinism.  Query b's outputs depend on row b of q / idx (and on the shard) only: not on B, not on its position in
 * the batch, not on kc beyond its live entries' relative order, not on the grid.  No atomics, no arrival counters, no
 * spinning, no allocation; asynchronous on `stream`; safe under graph capture.
 *
 * Status, decided before anything is launched; a refused call writes nothing:
 *   VPR_ERR_INVALID_ARG   NULL q, idx, rows, vals_out, idx_out or workspace; B, D, kc, n_local or index_base negative;
 *                         k_out outside 1..kc; q_is_f32 or rows_are_f32 not 0 or 1.
 *   VPR_ERR_UNSUPPORTED   kc > 128; D == 0, D % 64 != 0 or D > 16384; q, rows or workspace not 16-byte aligned (they are read
 *                         and written as 16-byte chunks; idx, vals_out and idx_out, accessed by element, need their natural
 *                         4 bytes, so a row slice of a list with odd kc is accepted); workspace_bytes <
 *                         vpr_rerank_workspace_bytes(B, kc).
 *   B == 0                VPR_OK, nothing is launched.
 */
#ifndef VPR_AMD_RERANK_H
#define VPR_AMD_RERANK_H

#include "vpr_amd.h"

#define VPR_RERANK_MAX_KC 128
#define VPR_RERANK_MAX_D 16384
#define VPR_RERANK_CHUNK_BF16 8
#define VPR_RERANK_CHUNK_F32 4
/* L of the fine score: chunk passes per lane + pairwise adds inside the lane + the six butterfly steps */
#define VPR_RERANK_ROUNDINGS(D, rows_are_f32) \
  ((rows_are_f32) ? ((D) + 255) / 256 + 2 + 6 : ((D) + 511) / 512 + 3 + 6)

#ifdef __cplusplus
extern "C" {
#endif

size_t vpr_rerank_workspace_bytes(int B, int kc);

int vpr_rerank_rows(const void* q, int q_is_f32,
                    const int32_t* idx, int B, int D, int kc,
                    const void* rows, int rows_are_f32, int n_local, int index_base,
                    int k_out, float* vals_out, int32_t* idx_out,
                    void* workspace, size_t workspace_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_RERANK_H */
