/* vpr_amd_retrieval.h — retrieval geopose and first-hit ranks from a merged top-k list, on the device.
 *
 * An ADDITIVE EXTENSION of ABI 6 (include/vpr_amd.h): it adds one entry point and two constants and changes nothing
 * that vpr_amd.h declares; VPR_AMD_ABI_VERSION stays 6.  The extension is present iff libvpr_amd.so exports the symbol
 * vpr_retrieval_pose (dlsym / ctypes lookup); a library built before it simply lacks the symbol.  Status codes and the
 * stream / graph-capture rules are those of vpr_amd.h.
 *
 * What it computes.  The retrieval leg ends with, per query b, the k best gallery rows: vals[b, j] (cosine score, f32,
 * descending in j) and idx[b, j] (global gallery row, int32), as vpr_knn_topk* and vpr_topk_merge emit them.  `labels`
 * is the gallery's side table on the device, row r = (latitude, longitude, angle in degrees, Region_ID) in f64 — the
 * label CSV columns of the gallery format.  One wave64 works on one query, lane j on neighbour j; 256 threads = four
 * queries per workgroup, grid = ceil(B / 4).  All arithmetic is f64; sums across lanes use one fixed xor butterfly over
 * the 64 lanes, so a query's outputs depend on that query's row alone: not on B, not on its position in the batch.
 * No workspace, no allocation, no atomics; asynchronous on `stream`; safe under graph capture (`scaler` is read on the
 * host during the call and travels as kernel arguments).
 *
 * Live neighbour.  Neighbour j is live iff 0 <= idx[b, j] < n_labels.  Anything else (the -1 padding of a short list, or
 *   an index past the table) is padding: its value and its label are never read, so no index can make the kernel read
 *   outside `labels`.
 * Weights (VPR_POSE_WEIGHTED).  w_j = exp((vals[b, j] - vals[b, 0]) / temperature) for live j, else 0 (softmax of
 *   score / temperature with column 0 as the shift).
 *     lat = sum_j w_j lat_j / sum_j w_j, lon likewise;
 *     S = sum_j w_j sin(theta_j) / sum_j w_j, C likewise with cos, theta_j = angle_j in radians;
 *     angle = (atan2(S, C) in degrees) mod 360.
 * VPR_POSE_TOP1.  The labels of neighbour 0, the angle taken mod 360.
 * No live neighbour 0.  Every pose output of that query is NaN, in both modes, and both hits are -1.
 * pose64 [B, 3] f64   (lat, lon, angle in degrees in [0, 360)).
 * pose4  [B, 4] f32   ((lat - mean_lat) / scale_lat, (lon - mean_lon) / scale_lon, sin(angle), cos(angle)), formed in
 *   f64 and rounded to f32 once: the 4-wide output format of the fused pose head (standardised position, unit
 *   (sin, cos) pair), so a retrieval pose and a head pose compare directly.
 *   scaler: HOST pointer to (mean_lat, mean_lon, scale_lat, scale_lon); NULL = (0, 0, 1, 1).
 * Hits (q_targets given: device [B, 3] f64 = the query's own lat, lon, Region_ID).
 *     hit_tau[b]    = the smallest j whose neighbour is live and (lat_j - qlat)^2 + (lon_j - qlon)^2 <= tau^2;
 *     hit_region[b] = the smallest live j with Region_ID_j == q_region;
 *   -1 where there is none; both are -1 for every query when q_targets is NULL.  The squared distance and tau^2 are
 *   evaluated as separately rounded f64 products and one f64 add (no fused multiply-add), i.e. they are bit for bit the
 *   numbers a host evaluation of ((q - g) ** 2).sum() <= tau * tau compares.  Recall@j over a query set is then
 *   mean(0 <= hit < j).
 * Any of pose64, pose4, hit_tau, hit_region may be NULL (that output is not written).
 *
 * Status, decided before anything is launched:
 *   VPR_ERR_INVALID_ARG   NULL vals, idx or labels; B < 0; n_labels < 1; unknown mode; temperature not > 0 in weighted
 *                         mode (NaN included); tau negative or NaN with q_targets; a scale not > 0 (NaN included).
 *   VPR_ERR_UNSUPPORTED   k outside 1..64; labels, q_targets, scaler or pose64 not 8-byte aligned.
 *   B == 0                VPR_OK, nothing is launched.
 */
#ifndef VPR_AMD_RETRIEVAL_H
#define VPR_AMD_RETRIEVAL_H

#include "vpr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPR_POSE_TOP1 0
#define VPR_POSE_WEIGHTED 1

int vpr_retrieval_pose(const float* vals, const int32_t* idx, int B, int k,
                       const double* labels, long long n_labels,
                       int mode, double temperature,
                       const double* q_targets, double tau,
                       const double* scaler,
                       double* pose64, float* pose4,
                       int32_t* hit_tau, int32_t* hit_region,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPR_AMD_RETRIEVAL_H */
