/* vpr_amd_project.h — descriptor projection (PCA / whitening) with L2 re-normalisation, on the device.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h), the third one beside include/vpr_amd_retrieval.h and
 * include/vpr_amd_expand.h: it adds three entry points and changes nothing that vpr_amd.h declares; VPR_AMD_ABI_VERSION stays
 * 6.  The extension is present iff libvpr_amd.so exports the symbol vpr_project_rows (dlsym / ctypes lookup; the two queries
 * come with it); a library built before it simply lacks the symbols.  Status codes and the stream / graph-capture rules are
 * those of vpr_amd.h.
 *
 * What it computes.  A learned linear map from the D-wide descriptor to d < D dimensions (the top d principal axes of the
 * gallery, optionally whitened), followed by L2 re-normalisation, so that kNN rows are d wide instead of D.  The host fits
 * the map (projection.fit_projection) and folds the centring into a bias: z = P (x - mean) = P x + c with c = -P mean.
 *
 * vpr_project_rows
 *   x          [rows, D] bf16, row r at x + r * x_stride (elements): the kNN query / gallery format, so the projection sees the
 *              same rounded descriptor a full-width search would.
 *   P          [d, D] bf16 row-major (the nn.Linear layout), c [d] f32.
 *   out_f32, out_bf16   [rows, d] contiguous; either may be NULL (not written), not both.
 *   z[r, j] = c[j] + sum_k x[r, k] * P[j, k].  Every product is exact in f32 (bf16 x bf16 on the bf16 matrix pipe); the sums
 *     are f32, in an order that is a function of (route, D, d) only — not of rows, of the row's position, or of the grid.
 *   normalize = 0: out_f32 = z.
 *   normalize = 1: n2 = sum_j z[r, j]^2 in f32 over a fixed tree that depends on d only; out_f32 = z * (1 / sqrt(n2)).  If n2
 *     is 0 or not finite (an all-zero row with c = 0, an Inf or NaN in the row), that row's outputs are all +0: a zero row
 *     scores 0 against everything.  No other row is affected.
 *   out_bf16 = the round-to-nearest-even bf16 of out_f32, bit for bit.
 *
 * Routes.  vpr_project_route(rows, D, d) is the call's own description of the route it takes (as vpr_knn_scores_kernel_name
 * is for the score kernel), a function of its three arguments only: 0 for rows <= VPR_PROJECT_STREAM_MAX_ROWS, else 1; a
 * negative value is the status vpr_project_rows would return for these shapes.
 *   Route 0, split-K streaming (a query batch).  Grid (d / 64, slices, ceil(rows / 64)) workgroups of 4 waves: a workgroup owns
 *     64 outputs x 64 rows x one K slice, its waves split the slice's K-steps of 32 (one 16x16x32 bf16 MFMA per 16 x 16 block
 *     and step) and add their parts in LDS in wave order; the slice's sums go to slab `slice` of the workspace.  The slice
 *     count depends on (D, d) only: steps = max(floor((D / 32) / min(64, ceil(256 / (d / 64)))), ceil((D / 32) / 64), 1) K-steps
 *     per slice, slices = ceil((D / 32) / steps) <= 64 — at D = 8448, d = 512: 8 output tiles x 33 slices of 8 K-steps.
 *   Route 1, tiled (gallery building, tens of thousands of rows per call).  The library's bf16 GEMM (256 x 256 tiles for D >= 128 and d >= 256, else 128-row
 *     tiles) writes z without the bias into the workspace as a single slab.
 *   Both end in the same finish kernel, one workgroup of 256 threads per row: the slabs are added in ascending slice order,
 *   then c[j], then the norm and both outputs.
 *
 * Workspace.  vpr_project_workspace_bytes(rows, D, d) bytes (0 for shapes the call refuses), monotone in rows; contents are
 * scratch.  16-byte aligned.
 *
 * Determinism.  Row r's outputs depend on row r, P, c and the route only; results are bitwise reproducible run to run.  No
 * atomics, no allocation; asynchronous on `stream`; safe under graph capture.
 *
 * Status, decided before anything is launched (outputs untouched on refusal):
 *   VPR_ERR_INVALID_ARG   NULL x, P, c or workspace; both outputs NULL; rows, D or d negative; normalize not 0 or 1;
 *                         x_stride < D.
 *   VPR_ERR_UNSUPPORTED   D == 0 or D % 64 != 0; d == 0, d % 64 != 0 or d > 4096; x_stride % 8 != 0 (or, on route 1, beyond
 *                         2^31 - 1); x, P, c, out_f32, out_bf16 or workspace not 16-byte aligned.
 *   VPR_ERR_WORKSPACE     workspace_bytes < vpr_project_workspace_bytes(rows, D, d).
 *   rows == 0             VPR_OK, nothing is launched.
 */
#ifndef VPR_AMD_PROJECT_H
#define VPR_AMD_PROJECT_H

#include "vpr_amd.h"

/* Largest `rows` that takes route 0.  From the sweep of scripts/project_bench.py (profiles/project_bench.txt):
 * 128 rows is the verified setting.  The sweep shows the split-K route ahead of route 1 up to about 2700 rows at D = 8448,
 * d = 512 (route 1 is two 256-column tiles per 256 rows, a grid that fills the device only from tens of thousands of rows on),
 * so a higher boundary is the open item.  A timing-only build of the library may define another value to measure a route
 * beyond its range. */
#ifndef VPR_PROJECT_STREAM_MAX_ROWS
#define VPR_PROJECT_STREAM_MAX_ROWS 128
#endif

#ifdef __cplusplus
extern "C" {
#endif

size_t vpr_project_workspace_bytes(int rows, int D, int d);

int vpr_project_route(int rows, int D, int d);

int vpr_project_rows(const uint16_t* x, long long x_stride, int rows, int D,
                     const uint16_t* P, const float* c, int d, int normalize,
                     float* out_f32, uint16_t* out_bf16,
                     void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_PROJECT_H */
