/* vpr_amd_salad_f32_stages.h — where the f32-accurate SALAD aggregation leaves its operand planes, its hidden values and
 * the operands of stage A inside its workspace.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the ninth one: it adds one entry point and changes nothing that
 * vpr_amd.h or another extension header declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_salad_f32_stage_outputs (dlsym / ctypes lookup); a library built before it simply
 * lacks the symbol.  Status codes are those of vpr_amd.h.
 *
 * What it is for.  vpr_salad_aggregate_f32, vpr_salad_aggregate_f32_n and vpr_salad_aggregate_f32_hires compute every linear
 * layer on the bf16 matrix pipe: each f32 operand x is split into three bf16 planes, x = h + m + q exactly (h = bf16(x),
 * m = bf16(x - h), q = bf16(x - h - m), each rounding to nearest, ties to even; both residuals are exact in f32), and one
 * GEMM over a K axis of 6 x K sums the six products kept, smallest first:
 *
 *     segment           0      1      2      3      4      5
 *     activation plane  q      h      m      m      h      h          ("activation order")
 *     weight plane      h      q      m      h      m      h          ("weight order")
 *
 * The dropped products (m q, q m, q q) are below 2^-24 of the leading one.  The hidden values stay f32 and are split again
 * for the second layers.  The layout of the workspace is internal and may change between builds; this call answers from the
 * very plan the three entries run on (the one behind vpr_salad_f32_workspace_bytes), so a test can compare planes, hidden
 * values and scores element by element, before Sinkhorn and three normalisations blur them.  Like vpr_salad_stage_outputs
 * it launches nothing, touches no device and reads no memory: it is pointer arithmetic on `workspace`.
 *
 * vpr_salad_f32_stage_outputs
 *   workspace, workspace_bytes, B, n, C, m, l, t, hidden: as passed to the aggregation (n = patch tokens per image).
 *   Required (INVALID_ARG when NULL).  All matrices are dense and row-major; "planes" are bf16 bit patterns (uint16_t):
 *   *H     f32 [B*n, 2*hidden]   relu(x W1_sc^T + b1_sc): score head in columns 0 .. hidden-1, cluster head behind it.
 *   *Ht    f32 [B, hidden]       relu(cls W1_t^T + b1_t).
 *   *S     f32 [B*n, m]          cluster scores, b2_s included.       Row b*n + r is patch token r of image b, whatever
 *   *F     f32 [B*n, l]          cluster features, b2_c included.     the layout the tokens came in.
 *   *g     f32 [B, t]            token features, b2_t included.
 *   *A1    planes [B*n, 6*C]     the patch tokens: six segments of C columns in activation order.
 *   *cls3  planes [B, 6*C]       the cls rows, activation order.
 *   *W1    planes [2*hidden, 6*C]  w1_sc, weight order.
 *   *H2    planes [B*n, 12*hidden] the planes of *H: the score head's six segments of `hidden` columns (activation order) in
 *                                columns 0 .. 6*hidden-1, then the cluster head's six.
 *   Optional (may be NULL):
 *   *W1t   planes [hidden, 6*C], *W2s planes [m, 6*hidden], *W2c planes [l, 6*hidden], *W2t planes [t, 6*hidden]: weight order.
 *   *Ht2   planes [B, 6*hidden]  the planes of *Ht, activation order.
 *
 * Domain of the values.  The split is exact for every finite f32 whose three planes are normal bf16 numbers or zero:
 * |x| below 2^128 (1 - 2^-9) (h must not round to infinity) and, as a sufficient condition, |x| >= 2^-102 (a non-zero plane
 * is a multiple of ulp(x) > 2^-24 |x|, so none of them is a bf16 subnormal, below 2^-126, which the matrix pipe may flush).
 * Values outside it — and NaN or infinity — are outside the domain of the f32 path; its tests keep magnitudes in
 * [2^-60, 2^60].
 *
 * What cancels.  As include/vpr_amd_salad_stages.h says of the bf16 path: b2_s adds a per-cluster constant to S, which the
 * first Sinkhorn update absorbs exactly — it is observable in *S only, never in a descriptor.
 *
 * Status, in this order — that of the three aggregation entries on the same arguments: VPR_ERR_INVALID_ARG for a NULL
 * required output or workspace, or B <= 0, n < 1, C <= 0; VPR_ERR_UNSUPPORTED for m != 64, l != 128, t != 256, C % 64 != 0,
 * hidden % 64 != 0 or n outside 65 .. VPR_SALAD_HIRES_MAX_N (the widest of the three domains; n = 256 and the any-n range
 * lie inside it); VPR_ERR_UNSUPPORTED for a workspace that is not 16-byte aligned; VPR_ERR_INVALID_ARG for hidden <= 0;
 * VPR_ERR_WORKSPACE for workspace_bytes < vpr_salad_f32_workspace_bytes(...).  A refused call writes nothing.
 */
#ifndef VPR_AMD_SALAD_F32_STAGES_H
#define VPR_AMD_SALAD_F32_STAGES_H

#include "vpr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vpr_salad_f32_stage_outputs(void* workspace, size_t workspace_bytes,
                                int B, int n, int C, int m, int l, int t, int hidden,
                                float** H, float** Ht, float** S, float** F, float** g,
                                uint16_t** A1, uint16_t** cls3, uint16_t** W1, uint16_t** H2,
                                uint16_t** W1t, uint16_t** W2s, uint16_t** W2c, uint16_t** W2t, uint16_t** Ht2);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_SALAD_F32_STAGES_H */
