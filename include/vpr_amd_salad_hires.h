/* vpr_amd_salad_hires.h — the SALAD aggregation for 65 .. 1369 patch tokens (448 px images: 32 x 32 = 1024; 518 px: 37 x 37 = 1369).
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the seventh one beside include/vpr_amd_retrieval.h,
 * include/vpr_amd_expand.h, include/vpr_amd_project.h, include/vpr_amd_rerank.h, include/vpr_amd_salad_stages.h and
 * include/vpr_amd_salad_anyres.h: it adds three entry points and changes nothing that the older headers declare;
 * VPR_AMD_ABI_VERSION stays 6.  The extension is present iff libvpr_amd.so exports the symbol
 * vpr_salad_sinkhorn_aggregate_hires (dlsym / ctypes lookup; the other two come with it); a library built before it simply
 * lacks the symbols.  Status codes and the stream / graph-capture rules are those of vpr_amd.h.
 *
 * Why.  The run-time-n calls of vpr_amd_salad_anyres.h stop at VPR_SALAD_MAX_N = 576 tokens (336 px) because their stage A
 * keeps one image's score matrix in one CU's LDS; they keep refusing n > 576.  DINOv2's own position table is 37 x 37, so
 * 518 px (n = 1369) is the resolution the backbone was pre-trained at and the largest grid it covers without extrapolating;
 * 448 px (n = 1024) is the other size its descriptors are evaluated at.  The calls below take m < n <= VPR_SALAD_HIRES_MAX_N,
 * with m = 64 clusters, l = 128 cluster dims, t = 256 token dims (descriptor width t + l*m = 8448).
 *
 * What they compute.  The published algorithm with the actual n (oracle/salad.py::sinkhorn_aggregate), exactly as stated in
 * vpr_amd_salad_anyres.h: dustbin row, Sinkhorn with marginals a_i = 1/(n+m), a_dust = (n-m)/(n+m), b_j = 1/(n+m),
 * sinkhorn_iters iterations; P scaled by (n+m), dustbin row dropped; V = F^T P^T [l, m]; F.normalize over l per cluster,
 * F.normalize of the token vector g, F.normalize of the concatenation (each eps 1e-12); output [g | V flattened l-major].
 * out_bf16 (may be NULL) = round-to-nearest-even of out_f32.
 *
 * vpr_salad_sinkhorn_aggregate_hires — stage A alone: scores [B, n, m] f32, feats [B, n, l] f32, tokfeat [B, t] f32, all
 *   dense -> out_f32 [B, t + l*m] (and out_bf16).  ALWAYS the high-resolution kernel, for every n of the domain (an A/B
 *   against vpr_salad_sinkhorn_aggregate at n = 256 and vpr_salad_sinkhorn_aggregate_n at n <= 576).  One workgroup per
 *   image.  The kernel stores no score matrix: K = exp(M - rowmax) is recomputed from the image's score slab on each of
 *   its 2 + sinkhorn_iters passes (a thread owns token columns tid, tid + 256, ... and needs only its own column for
 *   beta_j; the row sums for alpha are reduced over the workgroup once per pass).  The last pass forms P block by block of
 *   512 token columns as two bf16 planes in LDS and aggregates each block on the matrix pipe.  Exp-domain iterations, P as
 *   (hi, lo) bf16 pairs, three exact-product v_mfma_f32_32x32x16_bf16 per 16-token step: the arithmetic of the other two
 *   stage-A kernels; bit equality with them is not promised, the distance to f64 is (tests/test_salad_hires_gpu.py).
 * vpr_salad_aggregate_hires — the whole aggregation from bf16 tokens; the parameter list, addressing and workspace
 *   (vpr_salad_workspace_bytes) of vpr_salad_aggregate_n.  Stage A is chosen by n:
 *     n == 256            the stages of vpr_salad_aggregate_split                               — the same bits;
 *     other n <= 576      the chain of vpr_salad_aggregate_n                                    — the same bits;
 *     577 .. 1369         token MLP, the unfused score / cluster MLP route, the high-resolution stage A.
 * vpr_salad_aggregate_f32_hires — the parameter list and the precision of vpr_salad_aggregate_f32_n; workspace
 *   vpr_salad_f32_workspace_bytes(...).  The same choice by n: the bits of vpr_salad_aggregate_f32 at 256, of
 *   vpr_salad_aggregate_f32_n at other n <= 576, the same GEMM chain ending in the high-resolution stage A above that.
 *
 * Domain.  m = 64, l = 128, t = 256; m < n <= VPR_SALAD_HIRES_MAX_N; C % 64 == 0, hidden % 64 == 0.  scores, feats,
 *   workspace, patch, cls and the weight matrices 16-byte aligned; bf16 strides % 8 == 0 (f32 form: % 4 == 0,
 *   patch_img_stride >= n*C, cls_stride >= C), cls_stride < 2^31.  B * n must fit an int (B = 64 at n = 1369 is 87,616 rows).
 *
 * Determinism.  Image b's output is a function of image b's inputs, n, dustbin and sinkhorn_iters only: not of B, not of
 * b's position in the batch, not of the grid; two runs give identical bits.  Nothing outside scores[b], feats[b],
 * tokfeat[b] is read for image b: score loads are predicated on their token index (a column >= n is answered with -inf,
 * i.e. K = 0 and P = +0, and nothing is fetched for it), feature loads go through a buffer descriptor that spans feats[b]
 * alone, so a token slot >= n inside the last 16-token step is answered with 0 by the bounds check.
 * No atomics, no arrival counters, no spinning, no allocation, no workspace of its own; asynchronous on `stream`; safe
 * under graph capture.
 *
 * Status, decided before anything is launched; a refused call writes nothing.  The order is that of the _n entries:
 *   VPR_ERR_INVALID_ARG   sinkhorn_iters < 1 (ahead of everything); a NULL scores, feats, tokfeat, patch, cls, weights (or
 *                         one of their ten members), out_f32 or workspace; B <= 0, n < 1, C <= 0.
 *   VPR_ERR_UNSUPPORTED   shape outside the domain above (n <= 64, n > 1369, other m / l / t, C or hidden not a multiple of
 *                         64); then a misaligned operand — ahead of
 *   VPR_ERR_WORKSPACE     workspace_bytes below the size call's answer.
 *
 * Out of scope.  n > 1369.  The fused MLP kernel serves whole 256-row tiles per image only, so n != 256 pays the hidden
 * activations' round trip through HBM (179 MB at B = 64, n = 1369).  Train-mode aggregation (vpr_salad_aggregate_train)
 * keeps refusing n != 256.  Which kernel serves n <= 576 does not change.
 */
#ifndef VPR_AMD_SALAD_HIRES_H
#define VPR_AMD_SALAD_HIRES_H

#include "vpr_amd.h"

#define VPR_SALAD_HIRES_MAX_N 1369   /* 37 x 37: 518 px at patch 14, DINOv2's own position grid */

#ifdef __cplusplus
extern "C" {
#endif

int vpr_salad_sinkhorn_aggregate_hires(const float* scores, const float* feats, const float* tokfeat,
                                       int B, int n, int m, int l, int t, float dustbin, int sinkhorn_iters,
                                       float* out_f32, uint16_t* out_bf16, void* stream);

int vpr_salad_aggregate_hires(const uint16_t* patch, long long patch_img_stride,
                              const uint16_t* cls, long long cls_stride,
                              int B, int n, int C, const vpr_salad_weights* w, float dustbin,
                              int m, int l, int t, int hidden, int sinkhorn_iters,
                              float* out_f32, uint16_t* out_bf16,
                              void* workspace, size_t workspace_bytes, void* stream);

int vpr_salad_aggregate_f32_hires(const float* patch, long long patch_img_stride,
                                  const float* cls, long long cls_stride,
                                  int B, int n, int C, const vpr_salad_weights_f32* w, float dustbin,
                                  int m, int l, int t, int hidden, int sinkhorn_iters,
                                  float* out_f32, uint16_t* out_bf16,
                                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_SALAD_HIRES_H */
