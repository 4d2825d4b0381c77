/* vpr_amd_salad_stages.h — where stages T and M of the SALAD aggregation leave their results inside the workspace.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the fifth one beside include/vpr_amd_retrieval.h,
 * include/vpr_amd_expand.h, include/vpr_amd_project.h and include/vpr_amd_rerank.h: it adds one entry point and changes
 * nothing that vpr_amd.h declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff libvpr_amd.so exports the
 * symbol vpr_salad_stage_outputs (dlsym / ctypes lookup); a library built before it simply lacks the symbol.  Status codes
 * are those of vpr_amd.h.
 *
 * What it is for.  vpr_salad_stage_token (T) and vpr_salad_stage_mlps (M) — alone or inside vpr_salad_aggregate*,
 * vpr_salad_aggregate_train — leave the token features g, the cluster scores S and the cluster features F in the
 * workspace, where vpr_salad_stage_aggregate (A) reads them.  The layout of the workspace is internal and may change
 * between builds; this call answers from the very plan and slab rule the stages use, so a test (or a debugger) can look
 * at what the MLP kernels computed, element by element, before Sinkhorn and three normalisations blur it.  Like
 * vpr_knn_scores_ptr it launches nothing, touches no device and reads no memory: it is pointer arithmetic on `workspace`.
 *
 * vpr_salad_stage_outputs
 *   workspace, workspace_bytes, B, n, C, m, l, t, hidden: as passed to the stage calls.
 *   *S          [slabs][B*n, m] f32 — slab s starts *slab_rows * m elements after slab s - 1.
 *   *F          [slabs][B*n, l] f32 — slab s starts *slab_rows * l elements after slab s - 1.
 *   *g          [B, t] f32.
 *   *H          [B*n, 2*hidden] bf16, the hidden activations relu(x W1^T + b1): score head in columns 0 .. hidden-1,
 *               cluster head behind it.  Written on the unfused route only (*slabs == 1); on the fused route the hidden
 *               tile never leaves the chip and *H points at memory nobody writes.  H may be NULL (not asked for).
 *   *slabs      2 on the fused route (gemm256_fuse2_kernel: hidden == 512, C % 64 == 0, C >= 128, and VPR_SALAD_VARIANT
 *               is not 1): slab 0 = b2 + the product over hidden columns 0 .. 255, slab 1 = the product over hidden
 *               columns 256 .. 511, no bias; stage A adds them in f32, slab 0 first.  1 on the unfused route: slab 0 is
 *               the whole second layer, bias included.  The value follows the A/B switch as it is set at the time of the call.
 *   *slab_rows  B*n.
 *
 * What cancels.  Stage A row-normalises the score matrix (Sinkhorn), so a constant added to ONE cluster's scores over all
 * tokens of an image — b2_s[i] is such a constant — changes no descriptor entry: the first u-update absorbs it exactly.
 * b2_s is therefore observable in S only, never in a descriptor.
 *
 * Status: VPR_ERR_INVALID_ARG for a NULL workspace, S, F, g, slabs or slab_rows, or B <= 0, n < 1, C <= 0;
 * VPR_ERR_UNSUPPORTED for n != 256, m != 64, l != 128, t != 256, C % 64 != 0 or hidden % 64 != 0; VPR_ERR_WORKSPACE for
 * workspace_bytes < vpr_salad_workspace_bytes(...) — in that order, the checks of the stage calls themselves.  A refused
 * call writes nothing.
 */
#ifndef VPR_AMD_SALAD_STAGES_H
#define VPR_AMD_SALAD_STAGES_H

#include "vpr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vpr_salad_stage_outputs(void* workspace, size_t workspace_bytes,
                            int B, int n, int C, int m, int l, int t, int hidden,
                            float** S, float** F, float** g, uint16_t** H,
                            int* slabs, long long* slab_rows);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_SALAD_STAGES_H */
