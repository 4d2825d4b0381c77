/* vpr_amd_expand.h — query expansion (alpha-QE) and gallery-side augmentation (DBA) from a top-k list, on the device.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the second one beside include/vpr_amd_retrieval.h: it adds two entry
 * points and changes nothing that vpr_amd.h declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_query_expand (dlsym / ctypes lookup; vpr_query_expand_finish comes with it); a
 * library built before it simply lacks the symbols.  Status codes and the stream / graph-capture rules are those of
 * vpr_amd.h.
 *
 * What it computes.  After a search, query b has its k best gallery rows: vals[b, j] (cosine score, f32, descending in j)
 * and idx[b, j] (global gallery row, int32), as vpr_knn_topk* and vpr_topk_merge emit them.  The expanded query is the
 * L2-normalised weighted mean of the query and its n_use best rows, with weights score^alpha; searching again with it is
 * alpha-QE, and doing the same once for every gallery row (which finds itself at rank 0) is DBA.  The gallery may be
 * sharded: each shard adds up the rows it owns (vpr_query_expand), the partial sums are gathered, and
 * vpr_query_expand_finish adds them in shard order and normalises.
 *
 * vpr_query_expand — one shard's contribution.
 *   q          [B, D] bf16, the queries that were searched.
 *   vals, idx  [B, k] f32 / int32; only columns j < n_use are read (1 <= n_use <= k <= 128).
 *   rows       this shard, [n_local, D]: bf16 when row_scales == NULL, else e4m3 bytes with row_scales [n_local] f32 and
 *              row value = scale * e4m3 (the gallery formats of vpr_knn_topk / vpr_knn_topk_fp8).  The shard owns global
 *              rows index_base .. index_base + n_local - 1.
 *   Local neighbour.  Neighbour j < n_use is local iff index_base <= idx[b, j] < index_base + n_local.  Anything else (the
 *     -1 padding of a short list, a row another shard owns, any other number) is never dereferenced: no index can make the
 *     kernel read outside `rows` or `row_scales`.
 *   Weight.  w_j = (float) pow((double) vals[b, j], alpha) if vals[b, j] > 0, else 0 (a NaN score fails the comparison):
 *     formed in f64 and rounded to f32 once.  alpha = 0 gives 1 for every positive score.  A neighbour whose weight is 0
 *     contributes nothing, and its row is not read.
 *   partial[b, d] = add_query * q_weight * q[b, d] + sum_j w_j * row_j[d] over the local j of non-zero weight, in f32, in
 *     ascending j.  The first term is one rounded product of q_weight rounded to f32 and the element (absent, i.e. +0,
 *     when add_query == 0); every neighbour is then
 *     added with one fused multiply-add, c_j * x + acc, where for bf16 rows c_j = w_j and x = the element, and for e4m3
 *     rows c_j = w_j * scale_r (one rounded f32 product) and x = float(byte).  With a sharded gallery exactly one shard
 *     passes add_query = 1.
 *   partial    [B, D] f32, written in full (every element, also for a query without a local neighbour).
 *   out_f32, out_bf16   both NULL: the call ends with `partial`.  Otherwise the single-shard form: the same call goes on
 *     to vpr_query_expand_finish(partial, 1, q, B, D, out_f32, out_bf16, stream), whose rules apply.
 *   Grid: (B, ceil(D / E / 128)) workgroups of 128 threads, E = 8 (bf16) or 16 (e4m3) elements = one 16-byte row chunk per
 *   thread.  Each workgroup forms the query's weights once (wave-uniform from then on), and every thread requests its chunk
 *   of up to 16 neighbours before it adds them in order, so the scattered row reads overlap while the order of the sum
 *   stays fixed.
 *
 * vpr_query_expand_finish — shard partials to expanded queries.
 *   partials   [R, B, D] f32, 1 <= R <= 64 (R = 1: one shard's `partial`).
 *   s[b, d] = partials[0, b, d] + partials[1, b, d] + ... in ascending r, in f32; n2 = sum_d s[b, d]^2 in f32 (a fixed
 *   reduction tree that depends on D only); out_f32[b, d] = s[b, d] * (1 / sqrt(n2)), out_bf16[b, d] = the round-to-nearest-
 *   even bf16 of out_f32[b, d].  Either output may be NULL (not written), not both.
 *   Fallback.  If n2 is 0 or not finite (no live neighbour with q_weight = 0, every weight zero, an Inf or NaN in a row
 *   that contributed), that query's outputs are q[b] unchanged: out_bf16[b] = q[b] bit for bit, out_f32[b] = its f32 value.
 *   Grid: B workgroups of 1024 threads.
 *
 * Determinism.  Query b's outputs depend on row b of q / vals / idx (and on the shard) only: not on B, not on its position
 * in the batch, not on the grid.  No atomics, no allocation, no workspace beyond the caller's `partial`; asynchronous on
 * `stream`; safe under graph capture.
 *
 * Status, decided before anything is launched:
 *   VPR_ERR_INVALID_ARG   NULL q, vals, idx, rows or partial (expand); NULL partials or q, or both outputs NULL (finish);
 *                         B, D, k or n_local negative; n_use outside 1..k; R < 1; alpha or q_weight negative or NaN;
 *                         add_query not 0 or 1.
 *   VPR_ERR_UNSUPPORTED   k > 128; D == 0 or D % 64 != 0; R > 64; q, rows, partial(s), out_f32 or out_bf16 not 16-byte
 *                         aligned.
 *   B == 0                VPR_OK, nothing is launched.
 */
#ifndef VPR_AMD_EXPAND_H
#define VPR_AMD_EXPAND_H

#include "vpr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vpr_query_expand(const uint16_t* q, const float* vals, const int32_t* idx, int B, int D, int k,
                     const void* rows, const float* row_scales, int n_local, int index_base,
                     int n_use, double alpha, double q_weight, int add_query,
                     float* partial, float* out_f32, uint16_t* out_bf16,
                     void* stream);

int vpr_query_expand_finish(const float* partials, int R, const uint16_t* q, int B, int D,
                            float* out_f32, uint16_t* out_bf16,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_EXPAND_H */
