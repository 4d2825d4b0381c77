/* vpr_amd_patch_fp8.h — local-feature re-ranking on OCP e4m3 patch features: half the feature store, block-scaled fp8 MFMA.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the tenth one: it adds three entry points and changes nothing that
 * vpr_amd.h or an earlier extension header declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_patch_rerank_fp8 (dlsym / ctypes lookup; vpr_patch_quantize_fp8 and
 * vpr_patch_workspace_bytes_fp8 come with it); a library built before it simply lacks the symbols.  Status codes and the
 * stream / graph-capture rules are those of vpr_amd.h.
 *
 * The store.  A patch feature is L2-normalised, so its entries lie in [-1, 1].  It is stored as one OCP e4m3fn byte per entry
 * holding x * 2^VPR_PATCH_FP8_SHIFT = x * 256: the e4m3 normal range then covers |x| from 2^-14 to 1.75 and the subnormals go
 * down to 2^-17, so one fixed power-of-two scale serves every row and no scale tensor exists.  [N, n, l] bytes: half of the bf16
 * store of include/vpr_amd_local.h.
 *
 * vpr_patch_quantize_fp8
 *   x          `count` values, f32 (x_is_bf16 == 0) or bf16 (x_is_bf16 != 0; exact in f32).
 *   out        `count` bytes: out[i] = e4m3fn(x[i] * 256), round-to-nearest-even in ONE rounding from the f32 value, the
 *              subnormal results (below 2^-6 after the scale) included.  A finite value whose scaled magnitude is above 448
 *              saturates to +-448 (0x7E / 0xFE), decided by an explicit clamp before the conversion.  +-0 keeps its sign
 *              (0x00 / 0x80), and so does a value that rounds to zero.  NaN, +Inf and -Inf become the NaN byte 0x7F: they stay
 *              "no similarity" downstream, as a non-finite feature does in the bf16 contract.
 *   Elementwise: out[i] depends on x[i] only, not on i, count or the alignment of x / out.  One launch (a grid-stride kernel,
 *   16-byte loads where x and out allow, a scalar tail); asynchronous on `stream`; safe under graph capture.
 *   Status, before any launch: VPR_ERR_INVALID_ARG for NULL x or out or count < 0; VPR_ERR_UNSUPPORTED for x not aligned to
 *   its element (4 bytes f32, 2 bytes bf16); count == 0 is VPR_OK and launches nothing.
 *
 * vpr_patch_rerank_fp8 — the 22 parameters of the bf16 call of include/vpr_amd_local.h in its order; q_local [B, n_q, l] and
 * g_local [n_local, n_g, l] are e4m3 bytes as the quantiser writes them.  The contract is that header's, word for word —
 * liveness from the index alone, the two argmaxes and their ties, the match rule with min_sim, the fixed order of the score's
 * sum with its VPR_LOCAL_SUM_ROUNDINGS roundings, the clamp to +-FLT_MAX, the order stage, the optional outputs, determinism
 * (no atomics, no counters, no spinning, no allocation), the order of the status checks — except for:
 *   Similarity.  S[i][j] = 2^-16 * sum_d a[i][d] * b[j][d] over the values the bytes encode (that is, the dot product of the
 *     features the store stands for), summed by v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (E8M0 127 on both
 *     operands), one f32 accumulator per S[i][j] starting at +0, the l / 64 k-steps in ascending order.  The order and the
 *     arithmetic depend on l only.  The 2^-16 is applied in the epilogue as one f32 multiplication of the accumulator: it is
 *     exact (|sum| <= 256 * 448^2 < 2^26, the smallest nonzero product is 2^-18), so S has the accumulator's significand.
 *     A NaN byte (0x7F / 0xFF) makes every S it enters non-finite: no similarity.
 *   Accuracy of S.  The instruction does not add exact products in f32.  Measured with exact powers of two on an MI355X
 *     (scripts/mfma_e4m3_probe.py): a step forms its 64 products in groups of 8 consecutive d; inside a group every product
 *     is aligned to the group's largest one, 2^E, and its bits below 2^(E - 13) are dropped, towards zero; the group sums and
 *     the accumulator are then added in a window of at least 27 bits and rounded to f32 once per step.  So
 *     |S - exact| <= 7 * 2^-13 * sum over the groups of max_d |a b| + l * 2^-24 * sum_d |a b|  (in units of S),
 *     and S is exact when every group's products fit 14 bits below its largest (small integers, one-hot rows).
 *   Limits.  l % 64 == 0, 64 <= l <= VPR_PATCH_FP8_MAX_L = 256.  1 <= n_q, n_g <= 256.  1 <= k_out <= kc <= 128.
 *     q_local, g_local and workspace 16-byte aligned.
 *   Launches.  Match: (B, ceil(kc / 4)) workgroups of 8 waves, the kernel of the bf16 form instantiated for bytes (one
 *     epilogue for both); LDS n_g * l + 16 * n_g * 4 + 1 KB with n_g rounded up to 32.  Order: the order stage of the bf16 form.
 *   Status: as the bf16 call, with "l == 0, l % 64 != 0 or l > 256" for the width.
 *
 * vpr_patch_workspace_bytes_fp8(B, kc): the rule of the bf16 form: monotone in B and kc, > 0 for every supported shape (B = 0
 *   included); 0 = unsupported (B < 0, kc < 1, kc > 128).
 */
#ifndef VPR_AMD_PATCH_FP8_H
#define VPR_AMD_PATCH_FP8_H

#include "vpr_amd.h"

/* a stored byte encodes x * 2^8 */
#define VPR_PATCH_FP8_SHIFT 8
#define VPR_PATCH_FP8_MIN_L 64
#define VPR_PATCH_FP8_MAX_L 256

#ifdef __cplusplus
extern "C" {
#endif

int vpr_patch_quantize_fp8(const void* x, int x_is_bf16, long long count, uint8_t* out, void* stream);

size_t vpr_patch_workspace_bytes_fp8(int B, int kc);

int vpr_patch_rerank_fp8(const uint8_t* q_local, int n_q,
                         const int32_t* idx, int B, int kc,
                         const uint8_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                         int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                         float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_PATCH_FP8_H */
