// retrieval_pose.hip — geopose and first-hit ranks from the merged top-k (contract: include/vpr_amd_retrieval.h).
// One wave64 per query, lane j = neighbour j, four queries per 256-thread workgroup.  The waves of a workgroup share
// nothing (no LDS, no barrier), so a wave past the batch simply leaves.
#include <math.h>
#include <string.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_retrieval.h"

// every product below is rounded before it is added: the host formulas this kernel restates have no fused multiply-add
#pragma clang fp contract(off)

namespace vpr {

constexpr double DEG2RAD = 0.017453292519943295;      // pi / 180 and 180 / pi as numpy's deg2rad / rad2deg multiply by
constexpr double RAD2DEG = 57.29577951308232;

struct PoseScaler { double mean_lat, mean_lon, scale_lat, scale_lon; };

__device__ __forceinline__ double mod360(double a) {
  double r = fmod(a, 360.0);                           // sign of a; |r| < 360
  if (r < 0.0) r += 360.0;
  return r >= 360.0 ? 0.0 : r;                         // -tiny + 360 rounds to 360
}

__global__ __launch_bounds__(256) void retrieval_pose_kernel(
    const float* __restrict__ vals, const int32_t* __restrict__ idx, int B, int k,
    const double* __restrict__ labels, long long n_labels, int mode, double temperature,
    const double* __restrict__ q_targets, double tau, PoseScaler sc,
    double* __restrict__ pose64, float* __restrict__ pose4, int32_t* __restrict__ hit_tau, int32_t* __restrict__ hit_region) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                                  // wave-uniform

  // lane j < k holds neighbour j; padding and lanes >= k carry weight 0 and zero labels and read nothing
  long long row = -1;
  if (lane < k) row = idx[b * k + lane];
  const bool live = row >= 0 && row < n_labels;
  double lat = 0.0, lon = 0.0, ang = 0.0, region = 0.0, v = 0.0;
  if (live) {
    const double* l = labels + row * 4;
    lat = l[0]; lon = l[1]; ang = l[2]; region = l[3];
    v = (double)vals[b * k + lane];
  }
  const unsigned long long live_mask = __ballot(live);
  const bool any = (live_mask & 1ull) != 0;            // neighbour 0 live: the query has an answer

  double o_lat, o_lon, o_ang;
  if (mode == VPR_POSE_WEIGHTED) {
    const double v0 = __shfl(v, 0, 64);
    const double w = live ? exp((v - v0) / temperature) : 0.0;
    double sn, cs;
    sincos(ang * DEG2RAD, &sn, &cs);
    const double sw = wave_sum_f64(w);
    o_lat = wave_sum_f64(w * lat) / sw;
    o_lon = wave_sum_f64(w * lon) / sw;
    const double S = wave_sum_f64(w * sn) / sw, C = wave_sum_f64(w * cs) / sw;
    o_ang = mod360(atan2(S, C) * RAD2DEG);
  } else {
    o_lat = __shfl(lat, 0, 64);
    o_lon = __shfl(lon, 0, 64);
    o_ang = mod360(__shfl(ang, 0, 64));
  }

  int h_tau = -1, h_reg = -1;
  if (q_targets && any) {
    const double qlat = q_targets[b * 3], qlon = q_targets[b * 3 + 1], qreg = q_targets[b * 3 + 2];
    const double dlat = lat - qlat, dlon = lon - qlon;
    const double d2 = __dadd_rn(__dmul_rn(dlat, dlat), __dmul_rn(dlon, dlon));
    const unsigned long long m_tau = __ballot(live && d2 <= __dmul_rn(tau, tau));
    const unsigned long long m_reg = __ballot(live && region == qreg);
    h_tau = m_tau ? __ffsll(m_tau) - 1 : -1;
    h_reg = m_reg ? __ffsll(m_reg) - 1 : -1;
  }

  if (lane == 0) {
    if (!any) o_lat = o_lon = o_ang = __builtin_nan("");
    if (pose64) {
      pose64[b * 3] = o_lat; pose64[b * 3 + 1] = o_lon; pose64[b * 3 + 2] = o_ang;
    }
    if (pose4) {
      double sn, cs;
      sincos(o_ang * DEG2RAD, &sn, &cs);
      pose4[b * 4] = (float)((o_lat - sc.mean_lat) / sc.scale_lat);
      pose4[b * 4 + 1] = (float)((o_lon - sc.mean_lon) / sc.scale_lon);
      pose4[b * 4 + 2] = (float)sn;
      pose4[b * 4 + 3] = (float)cs;
    }
    if (hit_tau) hit_tau[b] = h_tau;
    if (hit_region) hit_region[b] = h_reg;
  }
}

}  // namespace vpr

using namespace vpr;

extern "C" int vpr_retrieval_pose(const float* vals, const int32_t* idx, int B, int k,
                                  const double* labels, long long n_labels, int mode, double temperature,
                                  const double* q_targets, double tau, const double* scaler,
                                  double* pose64, float* pose4, int32_t* hit_tau, int32_t* hit_region, void* stream) {
  if (!vals || !idx || !labels || B < 0 || n_labels < 1) return VPR_ERR_INVALID_ARG;
  if (mode != VPR_POSE_TOP1 && mode != VPR_POSE_WEIGHTED) return VPR_ERR_INVALID_ARG;
  if (mode == VPR_POSE_WEIGHTED && !(temperature > 0.0)) return VPR_ERR_INVALID_ARG;      // NaN fails the comparison
  if (q_targets && !(tau >= 0.0)) return VPR_ERR_INVALID_ARG;
  PoseScaler sc = {0.0, 0.0, 1.0, 1.0};
  if (scaler) memcpy(&sc, scaler, sizeof(sc));                                            // host memory, any alignment
  if (!(sc.scale_lat > 0.0) || !(sc.scale_lon > 0.0)) return VPR_ERR_INVALID_ARG;
  if (k < 1 || k > 64) return VPR_ERR_UNSUPPORTED;
  const uintptr_t doubles = reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(q_targets) |
                            reinterpret_cast<uintptr_t>(scaler) | reinterpret_cast<uintptr_t>(pose64);
  if (doubles & 7) return VPR_ERR_UNSUPPORTED;
  if (B == 0) return VPR_OK;
  VPR_TRY_LAUNCH(launch_kernel(retrieval_pose_kernel, dim3((unsigned)(((long long)B + 3) / 4)), dim3(256), 0,
                               static_cast<hipStream_t>(stream), vals, idx, B, k, labels, n_labels, mode, temperature,
                               q_targets, tau, sc, pose64, pose4, hit_tau, hit_region));
  return VPR_OK;
}
