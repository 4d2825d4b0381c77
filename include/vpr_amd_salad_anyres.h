/* vpr_amd_salad_anyres.h — the SALAD aggregation for any patch-token count 65 .. 576 (e.g. 322 px images: 23 x 23 = 529).
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the sixth one beside include/vpr_amd_retrieval.h,
 * include/vpr_amd_expand.h, include/vpr_amd_project.h, include/vpr_amd_rerank.h and include/vpr_amd_salad_stages.h: it adds
 * three entry points and changes nothing that vpr_amd.h declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff
 * libvpr_amd.so exports the symbol vpr_salad_sinkhorn_aggregate_n (dlsym / ctypes lookup; the other two come with it); a
 * library built before it simply lacks the symbols.  Status codes and the stream / graph-capture rules are those of vpr_amd.h.
 *
 * Why.  Every SALAD entry point of vpr_amd.h computes for exactly n = 256 patch tokens (224 x 224 images at patch 14) and
 * returns VPR_ERR_UNSUPPORTED otherwise; they keep doing so.  The calls below take the token count as a run-time argument,
 * m < n <= VPR_SALAD_MAX_N, with m = 64 clusters, l = 128 cluster dims, t = 256 token dims (descriptor width t + l*m = 8448).
 *
 * What they compute.  The published algorithm with the actual n (oracle/salad.py::sinkhorn_aggregate): the score matrix
 * [n, m] gets a dustbin row; Sinkhorn with marginals a_i = 1/(n+m) per cluster, a_dust = (n-m)/(n+m), b_j = 1/(n+m) per
 * token, sinkhorn_iters iterations; P scaled by (n+m), dustbin row dropped; V = F^T P^T [l, m]; F.normalize over l per
 * cluster, F.normalize of the token vector g, F.normalize of the concatenation (each eps 1e-12); output [g | V flattened
 * l-major].  out_bf16 (may be NULL) = round-to-nearest-even of out_f32.  n <= m has no SALAD (the dustbin marginal is
 * log(n - m)) and is refused.
 *
 * vpr_salad_sinkhorn_aggregate_n — stage A alone: scores [B, n, m] f32, feats [B, n, l] f32, tokfeat [B, t] f32, all dense
 *   -> out_f32 [B, t + l*m] (and out_bf16).  ALWAYS the run-time-n kernel, n = 256 included (an A/B against
 *   vpr_salad_sinkhorn_aggregate).  One workgroup per image; the score matrix of an image lives in one CU's LDS as f32
 *   [65][n + 1 or n + 2], which at n = 576 is 153,664 B of the 163,840 B a workgroup may declare: that is the limit.
 * vpr_salad_aggregate_n — the whole aggregation from bf16 tokens.  Patch row r of image b at patch + b*patch_img_stride +
 *   r*C, the cls row at cls + b*cls_stride (elements; the addressing of vpr_salad_aggregate_train): the hub layout
 *   [B, 1+n, C] is patch = tokens + C with both strides (1+n)*C, the split layout patch_img_stride = n*C, cls_stride = C.
 *   workspace: vpr_salad_workspace_bytes(B, n, C, m, l, t, hidden) bytes.
 *   n == 256: the stages of vpr_salad_aggregate_split (fused MLP kernel, n = 256 Sinkhorn kernel) — the same bits.
 *   n != 256: token MLP, then the score / cluster MLPs on the UNFUSED route (layer 1 on 256-row tiles, ragged at the end,
 *   hidden activations through HBM as bf16, the second layers as one grouped launch), then the run-time-n stage A.
 * vpr_salad_aggregate_f32_n — the parameter list and the precision of vpr_salad_aggregate_f32 (f32 tokens and weights, every
 *   linear layer to f32 accuracy); workspace vpr_salad_f32_workspace_bytes(...).  n == 256: the bits of
 *   vpr_salad_aggregate_f32; otherwise the same GEMM chain ending in the run-time-n stage A.
 *
 * Domain.  m = 64, l = 128, t = 256; m < n <= VPR_SALAD_MAX_N; C % 64 == 0, hidden % 64 == 0.  scores, feats, workspace,
 *   patch, cls and the weight matrices 16-byte aligned; bf16 strides % 8 == 0 (f32 form: % 4 == 0, patch_img_stride >= n*C,
 *   cls_stride >= C), cls_stride < 2^31.
 *
 * Determinism.  Image b's output is a function of image b's inputs, n, dustbin and sinkhorn_iters only: not of B, not of
 * b's position in the batch, not of the grid.  Nothing outside scores[b], feats[b], tokfeat[b] is read for image b: score
 * loads are predicated on their index, feature loads go through a buffer descriptor that spans feats[b] alone, so a token
 * slot >= n inside the last 16-token step is answered with 0 by the bounds check and nothing is fetched for it.
 * No atomics, no arrival counters, no spinning, no allocation; asynchronous on `stream`; safe under graph capture.
 *
 * Status, decided before anything is launched; a refused call writes nothing:
 *   VPR_ERR_INVALID_ARG   a NULL scores, feats, tokfeat, patch, cls, weights (or one of their ten members), out_f32 or
 *                         workspace; B <= 0, n < 1, C <= 0, sinkhorn_iters < 1.
 *   VPR_ERR_UNSUPPORTED   shape or alignment outside the domain above.
 *   VPR_ERR_WORKSPACE     workspace_bytes below the size call's answer.
 *
 * Out of scope.  n > 576 (448 / 518 px) is served by include/vpr_amd_salad_hires.h, whose stage A keeps no score matrix in LDS;
 * the calls here keep refusing it.  The fused MLP kernel serves whole 256-row tiles per image only, so n != 256 pays the hidden activations' round trip through
 * HBM.  Train-mode aggregation (vpr_salad_aggregate_train) keeps refusing n != 256: its dropout mask lives in the fused kernel.
 */
#ifndef VPR_AMD_SALAD_ANYRES_H
#define VPR_AMD_SALAD_ANYRES_H

#include "vpr_amd.h"

#define VPR_SALAD_MAX_N 576      /* 24 x 24: 336 px at patch 14 */

#ifdef __cplusplus
extern "C" {
#endif

int vpr_salad_sinkhorn_aggregate_n(const float* scores, const float* feats, const float* tokfeat,
                                   int B, int n, int m, int l, int t, float dustbin, int sinkhorn_iters,
                                   float* out_f32, uint16_t* out_bf16, void* stream);

int vpr_salad_aggregate_n(const uint16_t* patch, long long patch_img_stride,
                          const uint16_t* cls, long long cls_stride,
                          int B, int n, int C, const vpr_salad_weights* w, float dustbin,
                          int m, int l, int t, int hidden, int sinkhorn_iters,
                          float* out_f32, uint16_t* out_bf16,
                          void* workspace, size_t workspace_bytes, void* stream);

int vpr_salad_aggregate_f32_n(const float* patch, long long patch_img_stride,
                              const float* cls, long long cls_stride,
                              int B, int n, int C, const vpr_salad_weights_f32* w, float dustbin,
                              int m, int l, int t, int hidden, int sinkhorn_iters,
                              float* out_f32, uint16_t* out_bf16,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_SALAD_ANYRES_H */
