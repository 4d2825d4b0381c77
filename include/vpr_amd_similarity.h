/* vpr_amd_similarity.h — local re-ranking verified under a similarity transform: patch matches only count when they agree on
 * one scale, rotation and shift of the patch grid.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the thirteenth one: it adds three entry points and changes nothing that
 * vpr_amd.h or an earlier extension header declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_similarity_verify (dlsym / ctypes lookup; vpr_similarity_local_rerank and
 * vpr_similarity_workspace_bytes come with it); a library built before it simply lacks the symbols.  Status codes and the
 * stream / graph-capture rules are those of vpr_amd.h.
 * (The older contracts are referred to by file, never by symbol, as the tenth to twelfth extensions do.)
 *
 * The sibling of include/vpr_amd_spatial.h: that header's dominant-shift vote is the right model for a sideways step; under a
 * zoom (driving toward or away from the scene) the shift of a match grows with its distance from the centre and the votes
 * smear.  Here 256 two-match hypotheses of a similarity transform (scale in [1/2, 2], rotation within +-45 degrees, any shift)
 * are drawn by a fixed rule and the one with the most inliers wins.  All-integer except the score's f32 sum; no random numbers,
 * no least-squares refinement, no affine model, no homography.
 *
 *   Grid.  As in vpr_amd_spatial.h: an image's n patches are in raster order on a grid gw wide: patch p sits at x = p % gw,
 *     y = p / gw; gh = n / gw; 1 <= gw <= n and n % gw == 0, on the query side (n_q, gw_q) and the candidate side (n_g, gw_g).
 *     In addition every side fits: gw_q, n_q / gw_q, gw_g, n_g / gw_g <= VPR_SIM_MAX_SIDE = 37, so that every coordinate fits
 *     6 bits (a difference of two fits an int8) and every product below fits 24 bits; otherwise VPR_ERR_UNSUPPORTED (a
 *     1369 x 1 grid is refused).  1 <= n <= 1369.
 *     There is no bin limit, because there are no bins.
 *
 *   Match list.  The rule of vpr_amd_spatial.h word for word: column j is a match iff 0 <= partner < n_q and sim is finite;
 *     any other partner (-1, INT32_MIN, INT32_MAX, n_q, ...) is "no match": it is decided from the value alone and never used
 *     as an index.  The matches in ascending column order are m_0 .. m_{M-1}.  Match m has the candidate position
 *     g = (j % gw_g, j / gw_g) and the query position q = (partner % gw_q, partner / gw_q), both read as integer complex numbers.
 *
 *   Hypotheses.  Exactly VPR_SIM_HYPOTHESES = 256, a pure function of M.  For M >= 2 hypothesis h (0 <= h < 256) is defined by
 *     the two matches  s = floor(h * M / 256)  and  t = (s + 1 + (97 * h) % (M - 1)) % M  (s != t always).
 *     dg = g_t - g_s, dq = q_t - q_s, c = dq * conj(dg):  re = dq.x dg.x + dq.y dg.y,  im = dq.y dg.x - dq.x dg.y.
 *     The hypothesis is admissible iff  |dg|^2 > 0 and |dq|^2 > 0;  |dg|^2 <= 4 |dq|^2 and |dq|^2 <= 4 |dg|^2 (scale within
 *     [1/2, 2], VPR_SIM_MAX_SCALE = 2);  re > 0 and |im| <= re (rotation within +-45 degrees).
 *     Its model is  q^(g) = q_s + (c / |dg|^2) (g - g_s):  scale |c| / |dg|^2, rotation atan2(im, re).
 *
 *   Inliers.  Match (g, q) is an inlier of h iff  |(q - q_s) dg - dq (g - g_s)|^2 <= tol^2 |dg|^2  in complex integer
 *     arithmetic: |q - q^(g)| <= tol patches, Euclidean, without a division.  Both sides are int32-safe (each component of the
 *     left side is at most 4 * 36 * 36 = 5184 in magnitude, so |.|^2 <= 2 * 5184^2).  0 <= tol <= VPR_SIM_MAX_TOL = 8.  The two
 *     defining matches are always inliers.  The count of a hypothesis that is not admissible is 0.
 *
 *   Winner.  The admissible hypothesis that comes first under (inlier count descending, h ascending).  If M < 2 or no
 *     hypothesis is admissible there is no model.
 *
 * vpr_similarity_verify — the verification stage on its own, driven by a match list.  Per pair p < P:
 *   partner [P, n_g] int32, sim [P, n_g] f32: as vpr_amd_spatial.h takes them.
 *   Outputs.  score f32 [P]: the f32 sum of sim over the winner's inlier columns in the order of vpr_amd_local_hires.h, word
 *     for word: blocks of 256 columns; thread j - 256 t owns column j, a non-inlier contributes +0; the wave_sum butterfly;
 *     the four wave sums added to +0 in wave order; the block sums added to a running +0 in block order, each block sum and
 *     the running sum clamped to +-FLT_MAX.  L_sum is that header's, 10 + ceil(n_g / 256); the score is always finite.
 *     inliers int32 [P]; matches int32 [P] = M; model int32 [P, 6] = (h, the column of m_s, the column of m_t, re, im, |dg|^2)
 *     of the winner.  inlier_mask uint8 [P, n_g], optional (NULL = not wanted; asking for it changes nothing else): 1 for an
 *     inlier column.
 *     No model: score +0, inliers 0, model six times INT32_MIN, the mask all 0; matches is still M.  This differs from
 *     vpr_amd_spatial.h at M = 1: one match is one inlier of the shift vote, and no inlier here (a single match fixes no
 *     scale and no rotation).
 *   Status, decided before anything is launched, in this order; a refused call writes nothing:
 *     VPR_ERR_INVALID_ARG   NULL partner, sim, score, inliers, matches or model; P, n_q, n_g, gw_q, gw_g or tol negative.
 *     VPR_ERR_UNSUPPORTED   n_q or n_g 0 or > 1369; gw_q or gw_g 0 or not dividing its n; tol > 8; a grid side > 37; partner,
 *                           sim or an int32 / f32 output not 4-byte aligned.
 *     P == 0                VPR_OK, nothing is launched.
 *
 * vpr_similarity_local_rerank — the whole second stage: match, verify, order.
 *   The parameter list of the composed call of vpr_amd_spatial.h in its order; pair_model int32 [B, kc, 6] takes the place of
 *   pair_shift.  Matching, the match list, liveness, min_sim, routing between the two match kernels, the order stage (the
 *   payload is the inlier count), duplicates, the limits (n <= 1369, bf16 l % 32 == 0, e4m3 l % 64 == 0, l <= 256,
 *   1 <= k_out <= kc <= 128) and the order of the status checks are that call's, with the side limit where it has the bin limit:
 *     VPR_ERR_INVALID_ARG   gw_q, gw_g or tol negative; feat_is_fp8 not 0 or 1.
 *     VPR_ERR_UNSUPPORTED   gw_q or gw_g 0 or not dividing its n; tol > 8; a grid side > 37 — after the checks of kc, n and l,
 *                           before the alignment checks; then workspace_bytes < vpr_similarity_workspace_bytes(B, kc, n_g).
 *   A non-live candidate is (-inf, 0, 0, six times INT32_MIN) in pair_score, pair_inliers, pair_matches, pair_model and -1
 *   throughout row_nn / col_nn; in the main outputs it comes after the live ones as (-inf, -1) with inliers 0.  A refused call
 *   writes nothing.
 *
 * vpr_similarity_workspace_bytes(B, kc, n_g): equal to the workspace rule of vpr_amd_spatial.h for every argument — the scores
 *   and counts of the order stage plus the match list, 8 bytes per (pair, column); 0 = unsupported.
 *
 * Launches.  Match, verify, order.  Verify: one 256-thread workgroup per pair; a workgroup whose candidate is not live writes
 *   its sentinels and ends before any list read.  The matches are compacted in column order into static LDS (four
 *   coordinates per word, about 5.5 KB) by wave ballots and popcounts — no atomic; thread h evaluates hypothesis h over all M
 *   matches (two 4 x int8 dot products and two 24-bit squares per test); a packed integer argmax; the score through the
 *   block sum of the match kernels.  There are no atomics on floats, nothing is accumulated in global memory, there are no
 *   arrival counters, no spinning and no allocation; asynchronous on `stream`; safe under graph capture; the same inputs give
 *   the same bits.
 *
 * If all matches of a pair share one shift and M >= 2, every hypothesis has dq = dg (scale 1, no rotation, admissible) and every
 * match is an inlier at any tol: the pair's score and inlier count then equal the hires call's pair_score / pair_matches bit
 * for bit.
 */
#ifndef VPR_AMD_SIMILARITY_H
#define VPR_AMD_SIMILARITY_H

#include "vpr_amd.h"
#include "vpr_amd_local_hires.h"

/* = the patch limit of include/vpr_amd_local_hires.h, 37 x 37 */
#define VPR_SIM_MAX_N 1369
/* every grid side: coordinates fit 6 bits, products of two coordinate differences fit 24 bits */
#define VPR_SIM_MAX_SIDE 37
#define VPR_SIM_HYPOTHESES 256
/* scale within [1 / VPR_SIM_MAX_SCALE, VPR_SIM_MAX_SCALE] */
#define VPR_SIM_MAX_SCALE 2
#define VPR_SIM_MAX_TOL 8

#ifdef __cplusplus
extern "C" {
#endif

size_t vpr_similarity_workspace_bytes(int B, int kc, int n_g);

int vpr_similarity_verify(const int32_t* partner, const float* sim, int P, int n_q, int gw_q, int n_g, int gw_g, int tol,
                          float* score, int32_t* inliers, int32_t* matches, int32_t* model, uint8_t* inlier_mask, void* stream);

int vpr_similarity_local_rerank(const void* q_local, int n_q,
                                const int32_t* idx, int B, int kc,
                                const void* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                int k_out, float* vals_out, int32_t* idx_out, int32_t* inliers_out,
                                float* pair_score, int32_t* pair_inliers, int32_t* pair_matches, int32_t* pair_model,
                                int32_t* row_nn, int32_t* col_nn,
                                int feat_is_fp8, int gw_q, int gw_g, int tol,
                                void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_SIMILARITY_H */
