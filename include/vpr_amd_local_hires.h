/* vpr_amd_local_hires.h — local-feature re-ranking for up to 1369 patch tokens per image (322, 448 and 518 px at patch 14).
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the eleventh one: it adds three entry points and changes nothing that
 * vpr_amd.h or an earlier extension header declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_hires_local_rerank (dlsym / ctypes lookup; vpr_hires_patch_rerank_fp8 and
 * vpr_hires_local_workspace_bytes come with it); a library built before it simply lacks the symbols.  Status codes and the
 * stream / graph-capture rules are those of vpr_amd.h.
 *
 * vpr_hires_local_rerank — the 22 parameters of the bf16 call of include/vpr_amd_local.h (the eighth extension) in its order.
 * vpr_hires_patch_rerank_fp8 — the 22 parameters of the e4m3 call of the tenth extension (the patch-fp8 header next to this
 *   one): features are e4m3 bytes of x * 2^8 as its quantiser writes them.
 * (The 256-patch contracts are referred to by file, never by symbol, as the tenth extension does.)
 *
 * The contract is that of those two headers, word for word — liveness from the index alone; S[i][j] by the same MFMA
 * instruction (v_mfma_f32_32x32x16_bf16; v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales and the exact 2^-16), one f32
 * accumulator per S[i][j] starting at +0, the k-steps in ascending order, so the order of the sum depends on l only (and the
 * accuracy of the e4m3 S is the one that header states); a non-finite S counts as no similarity; r(i) and c(j) with ties to
 * the lowest index, -1 where a row / column has no finite entry; the match rule with min_sim; the order stage (order_rank);
 * the optional outputs and their sentinels; determinism; the order of the status checks; a refused call writes nothing; no
 * atomics, no arrival counters, no spinning, no allocation; asynchronous on `stream`; safe under graph capture — except for:
 *
 *   Limits.  1 <= n_q, n_g <= VPR_LOCAL_HIRES_MAX_N = 1369 (37 x 37: 518 px), independent of each other.  l and kc as the
 *     256-patch forms: bf16 l % 32 == 0, e4m3 l % 64 == 0, l <= 256; 1 <= k_out <= kc <= 128.
 *
 *   Score.  matches = the number of matched columns; score = the f32 sum of S[c(j)][j] over the matched columns in this fixed
 *     order.  Columns go in blocks of 256: block t holds columns 256 t .. 256 t + 255.  A block's sum is formed exactly as
 *     vpr_amd_local.h states: thread j - 256 t owns column j (an unmatched or absent column contributes +0); the 64 values of
 *     a wave are added by the wave_sum butterfly (v += v of lane xor 32, 16, 8, 4, 2, 1); the four wave sums are added to +0
 *     in ascending wave order.  The block sums are then added, in ascending block order, to a running f32 that starts at +0.
 *     Each block sum, and the running sum after each addition, is clamped to +-FLT_MAX: the score is always finite and no
 *     Inf - Inf can arise.  Roundings on the longest path from a similarity to the score:
 *     L_sum = VPR_LOCAL_HIRES_SUM_ROUNDINGS(n_g) = 10 + ceil(n_g / 256) <= 16, so
 *     |score - exact sum| <= gamma_L * sum_matched |S[c(j)][j]|, gamma_L = L u / (1 - L u), u = 2^-24.
 *     For n_g <= 256 this is the rule of vpr_amd_local.h followed by +0 + x, and x is never -0 (it is itself +0 + ...): at
 *     n_q, n_g <= 256 every output of these calls equals the 256-patch calls' bit for bit.
 *
 *   Launches.  Match: (B, kc) workgroups of 8 waves, one per (query, candidate) pair; a workgroup whose candidate is not live
 *     writes the optional outputs' sentinels and ends before any load.  Neither image fits in LDS or registers, so both patch
 *     axes are tiled: the candidate's columns in chunks of 256 (128 where a feature row exceeds 256 bytes), each staged once
 *     in LDS; under a chunk the query's rows in blocks of 256 (wave w owns rows 32 w .. 32 w + 31 of a block, its MFMA
 *     A-fragments read from global memory).  LDS: chunk (<= 64 KB) + 16 * chunk columns * 4 + 8 * (n_g + n_q) + 192 bytes with
 *     n_g rounded up to 32 and n_q to 256, at most 103 KB, through the dynamic-LDS opt-in.  Order: the order stage of the
 *     256-patch forms.
 *
 *   Status.  As the 256-patch forms, with "n_q or n_g 0 or > 1369" in place of "> 256".
 *
 * vpr_hires_local_workspace_bytes(B, kc): bytes of workspace for either call, the rule of the 256-patch forms:
 *   monotone in B and kc, > 0 for every supported shape (B = 0 included); 0 = unsupported (B < 0, kc < 1, kc > 128).
 *
 * The 256-patch forms remain the route for n <= 256: they keep four candidates per workgroup with the query in registers.
 */
#ifndef VPR_AMD_LOCAL_HIRES_H
#define VPR_AMD_LOCAL_HIRES_H

#include "vpr_amd.h"
#include "vpr_amd_local.h"

/* = the largest token count of include/vpr_amd_salad_hires.h, 37 x 37 */
#define VPR_LOCAL_HIRES_MAX_N 1369
/* L_sum of the score: VPR_LOCAL_SUM_ROUNDINGS inside a block of 256 columns + one addition per block */
#define VPR_LOCAL_HIRES_SUM_ROUNDINGS(n_g) (VPR_LOCAL_SUM_ROUNDINGS + ((n_g) + 255) / 256)

#ifdef __cplusplus
extern "C" {
#endif

size_t vpr_hires_local_workspace_bytes(int B, int kc);

int vpr_hires_local_rerank(const uint16_t* q_local, int n_q,
                           const int32_t* idx, int B, int kc,
                           const uint16_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                           int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                           float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                           void* workspace, size_t workspace_bytes, void* stream);

int vpr_hires_patch_rerank_fp8(const uint8_t* q_local, int n_q,
                               const int32_t* idx, int B, int kc,
                               const uint8_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                               int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                               float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                               void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_LOCAL_HIRES_H */
