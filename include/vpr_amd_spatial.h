/* vpr_amd_spatial.h — local re-ranking with spatial verification: patch matches only count when they agree on one shift of the
 * patch grid.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the twelfth one: it adds three entry points and changes nothing that
 * vpr_amd.h or an earlier extension header declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_spatial_verify (dlsym / ctypes lookup; vpr_spatial_local_rerank and
 * vpr_spatial_workspace_bytes come with it); a library built before it simply lacks the symbols.  Status codes and the
 * stream / graph-capture rules are those of vpr_amd.h.
 * (The older contracts are referred to by file, never by symbol, as the tenth and eleventh extensions do.)
 *
 * The model is an all-integer dominant-shift vote, not a RANSAC: no scale, no rotation, no homography.
 *
 *   Grid.  An image's n patches are in raster order on a grid gw wide: patch p sits at x = p % gw, y = p / gw; gh = n / gw.
 *     1 <= gw <= n and n % gw == 0, on the query side (n_q, gw_q) and on the candidate side (n_g, gw_g).
 *
 *   Shift bins.  A match (query patch i, candidate patch j) has the shift dx = x_q(i) - x_g(j), dy = y_q(i) - y_g(j).
 *     W = gw_q + gw_g - 1, H = gh_q + gh_g - 1, bin = (dy + gh_g - 1) * W + (dx + gw_g - 1).
 *     W * H <= VPR_SPATIAL_MAX_BINS = 5329 (73 x 73: 37 x 37 against 37 x 37), otherwise VPR_ERR_UNSUPPORTED.
 *
 * vpr_spatial_verify — the verification stage on its own, driven by a match list.  Per pair p < P:
 *   partner [P, n_g] int32: the query patch matched to candidate column j;  sim [P, n_g] f32: that match's similarity.
 *   Column j is a match iff 0 <= partner < n_q and sim is finite.  Any other partner (-1, INT32_MIN, INT32_MAX, n_q, ...)
 *     is "no match": it is decided from the value alone and never used as an index.
 *   1. votes[bin] = the number of matches with that shift.
 *   2. support[bin] = the sum of votes over the (2 tol + 1)^2 window centred on the bin; bins outside W x H count as 0.
 *   3. The dominant shift is the bin that comes first under the key: support descending, then the bin's own votes
 *      descending, then the bin index ascending.
 *   4. A match is an inlier iff its shift lies in the window of the dominant bin (Chebyshev distance <= tol), so
 *      inliers = support[dominant].  0 <= tol <= VPR_SPATIAL_MAX_TOL = 8.
 *   5. score = the f32 sum of sim over the inlier columns in the order of vpr_amd_local_hires.h, word for word: blocks of
 *      256 columns; thread j - 256 t owns column j, a non-inlier contributes +0; the wave_sum butterfly; the four wave sums
 *      added to +0 in wave order; the block sums added to a running +0 in block order, each block sum and the running sum
 *      clamped to +-FLT_MAX.  L_sum is that header's, 10 + ceil(n_g / 256); the score is always finite.
 *   Outputs.  score f32 [P], inliers int32 [P], matches int32 [P] (the number of matches), shift int32 [P, 2] = (dx, dy) of
 *     the dominant bin.  A pair without any match gives score +0, inliers 0, matches 0, shift (INT32_MIN, INT32_MIN).
 *     inlier_mask uint8 [P, n_g], optional (NULL = not wanted; asking for it changes nothing else): 1 for an inlier column.
 *   Limits.  1 <= n_q, n_g <= VPR_SPATIAL_MAX_N = 1369, the limit of the hires header.
 *   Status, decided before anything is launched, in this order; a refused call writes nothing:
 *     VPR_ERR_INVALID_ARG   NULL partner, sim, score, inliers, matches or shift; P, n_q, n_g, gw_q, gw_g or tol negative.
 *     VPR_ERR_UNSUPPORTED   n_q or n_g 0 or > 1369; gw_q or gw_g 0 or not dividing its n; tol > 8; W * H > 5329; partner,
 *                           sim or an int32 / f32 output not 4-byte aligned.
 *     P == 0                VPR_OK, nothing is launched.
 *
 * vpr_spatial_local_rerank — the whole second stage: match, verify, order.
 *   The parameters of the hires bf16 call (vpr_amd_local_hires.h) in its order, with q_local / g_local as const void* and
 *   feat_is_fp8 (0: bf16 features, 1: e4m3 bytes as the patch-fp8 header's quantiser writes them) after them, then gw_q,
 *   gw_g, tol.  inliers_out [B, k_out] takes the place of matches_out and vals_out is the verified score.
 *   Matching, liveness, min_sim, the order stage (order_rank; the payload is the inlier count), duplicates, determinism, "a
 *   refused call writes nothing" and the order of the status checks are those of the 256-patch and hires headers.  The match
 *   list is: partner[j] = c(j) if column j is matched, else -1; sim[j] = S[c(j)][j] if matched, else +0.
 *   Optional outputs, each NULL = not wanted; whether they are asked for changes no other output: pair_score f32,
 *   pair_inliers, pair_matches int32 [B, kc], pair_shift int32 [B, kc, 2], row_nn [B, kc, n_q] / col_nn [B, kc, n_g].  A
 *   non-live candidate is (-inf, 0, 0, (INT32_MIN, INT32_MIN)) and -1 throughout row_nn / col_nn; in the main outputs it
 *   comes after the live ones as (-inf, -1) with inliers 0.
 *   Routing.  n_q, n_g <= 256: the match kernel of vpr_amd_local.h / the patch-fp8 header; otherwise that of the hires
 *   header.  Both write the same list bit for bit where both apply.
 *   Limits.  Those of the hires calls: n <= 1369, bf16 l % 32 == 0, e4m3 l % 64 == 0, l <= 256, 1 <= k_out <= kc <= 128.
 *   Status.  As the hires calls, with these refusals appended to their groups:
 *     VPR_ERR_INVALID_ARG   gw_q, gw_g or tol negative; feat_is_fp8 not 0 or 1.
 *     VPR_ERR_UNSUPPORTED   gw_q or gw_g 0 or not dividing its n; tol > 8; W * H > 5329 — after the checks of kc, n and l,
 *                           before the alignment checks; then workspace_bytes < vpr_spatial_workspace_bytes(B, kc, n_g).
 *
 * vpr_spatial_workspace_bytes(B, kc, n_g): the scores and counts of the order stage plus the match list, 8 bytes per
 *   (pair, column).  Monotone in every argument, > 0 for every supported shape (B = 0 included); 0 = unsupported (B < 0,
 *   kc < 1, kc > 128, n_g < 1, n_g > 1369).
 *
 * Launches.  Match (one of the two kernels above, which write the list where they write col_nn), verify, order.  Verify:
 *   one 256-thread workgroup per pair; a workgroup whose candidate is not live writes its sentinels and ends before any
 *   list read.  Votes are counted with integer adds into LDS: the counts do not depend on the order of arrival, so
 *   determinism holds.  The window sum is separable (rows, then columns); votes and row sums are two int32 planes of at
 *   most 5329 bins in static LDS (about 43 KB, no dynamic-LDS opt-in).  Nothing is accumulated in global memory: no arrival
 *   counters, no spinning, no allocation; asynchronous on `stream`; safe under graph capture.
 *
 * If every match of a pair is an inlier, the pair's score and inlier count equal the hires call's pair_score /
 * pair_matches bit for bit.  This always holds when tol >= max(W, H) - 1, and whenever all matches share one shift.
 */
#ifndef VPR_AMD_SPATIAL_H
#define VPR_AMD_SPATIAL_H

#include "vpr_amd.h"
#include "vpr_amd_local_hires.h"

/* = the patch limit of include/vpr_amd_local_hires.h, 37 x 37 */
#define VPR_SPATIAL_MAX_N 1369
/* 73 x 73: the shifts of a 37 x 37 grid against a 37 x 37 grid */
#define VPR_SPATIAL_MAX_BINS 5329
#define VPR_SPATIAL_MAX_TOL 8

#ifdef __cplusplus
extern "C" {
#endif

size_t vpr_spatial_workspace_bytes(int B, int kc, int n_g);

int vpr_spatial_verify(const int32_t* partner, const float* sim, int P, int n_q, int gw_q, int n_g, int gw_g, int tol,
                       float* score, int32_t* inliers, int32_t* matches, int32_t* shift, uint8_t* inlier_mask, void* stream);

int vpr_spatial_local_rerank(const void* q_local, int n_q,
                             const int32_t* idx, int B, int kc,
                             const void* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                             int k_out, float* vals_out, int32_t* idx_out, int32_t* inliers_out,
                             float* pair_score, int32_t* pair_inliers, int32_t* pair_matches, int32_t* pair_shift,
                             int32_t* row_nn, int32_t* col_nn,
                             int feat_is_fp8, int gw_q, int gw_g, int tol,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_SPATIAL_H */
