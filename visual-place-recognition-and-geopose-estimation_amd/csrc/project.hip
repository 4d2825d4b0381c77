// project.hip — descriptor projection z = P x + c with L2 re-normalisation (contract: include/vpr_amd_project.h).
// Route 0 (up to VPR_PROJECT_STREAM_MAX_ROWS rows: a query batch): project_split_kernel, the bf16 sibling of
// pose_l1_split_tile (pose_head.hip): a workgroup owns 64 outputs x 64 rows x one K slice, its four waves split the slice's
// K-steps of 32 and meet in LDS in wave order; both operands are bf16 already, so a 16 x 16 block is ONE 16x16x32 MFMA per
// step.  The slice's sums go to slab [slice][rows][d].
// Route 1 (gallery building): the library's tiled bf16 GEMM writes z without the bias as a single slab.
// Both end in project_finish_kernel, one workgroup per row: slabs in ascending slice order, c, the norm, both outputs.
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_project.h"

namespace vpr {

constexpr int PJ_MAX_SLICES = 64;
constexpr int PJ_MAX_D_OUT = 4096;
constexpr int PJ_GRID_TARGET = 256;                                       // workgroups the (tile, slice) grid aims for: the CUs of an MI355X
constexpr int PJ_WAVES = 4;
constexpr size_t PJ_SPLIT_LDS = PJ_WAVES * 16 * 64 * sizeof(f32x4);      // [4 waves][4 cb][4 mb][64 lanes][4] = 64 KB
constexpr int PJ_FIN_THREADS = 256;
constexpr int PJ_FIN_VEC = PJ_MAX_D_OUT / (4 * PJ_FIN_THREADS);          // float4 columns a finish thread owns at most (4)

// K-steps per slice and slice count: a function of (D, d) only
struct PjPlan { int steps, nslice; };
static PjPlan pj_plan(int D, int d) {
  const int ksteps = D / 32, ntiles = d / 64;
  int want = (PJ_GRID_TARGET + ntiles - 1) / ntiles;
  if (want > PJ_MAX_SLICES) want = PJ_MAX_SLICES;
  int steps = ksteps / want;
  const int least = (ksteps + PJ_MAX_SLICES - 1) / PJ_MAX_SLICES;
  if (steps < least) steps = least;
  if (steps < 1) steps = 1;
  return PjPlan{steps, (ksteps + steps - 1) / steps};
}

// grid (d / 64, nslice, ceil(rows / 64)), 256 threads.  part[slice][rows][d].
__global__ __launch_bounds__(PJ_WAVES * 64) void project_split_kernel(
    const uint16_t* __restrict__ x, long long x_stride, int rows, int D, const uint16_t* __restrict__ P, int d,
    float* __restrict__ part, int steps_per_slice) {
  extern __shared__ __attribute__((aligned(16))) float red[];        // PJ_SPLIT_LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 64, ks = blockIdx.y, m0 = blockIdx.z * 64;
  const int ksteps = D >> 5;
  const int s_begin = ks * steps_per_slice, s_end = min(ksteps, s_begin + steps_per_slice);
  const int ns = max(s_end - s_begin, 0);
  const int kbeg = s_begin + ns * wave / PJ_WAVES, kend = s_begin + ns * (wave + 1) / PJ_WAVES;
  // operand maps of 16x16x32: row = lane & 15, k = 8 * (lane >> 4) .. + 7.  d % 64 == 0: every P row exists; x rows past the
  // end are clamped (their sums are never stored).
  const uint16_t* pp[4];
  const uint16_t* xp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pp[i] = P + (long long)(n0 + i * 16 + r) * D + 8 * g;
    xp[i] = x + (long long)min(m0 + i * 16 + r, rows - 1) * x_stride + 8 * g;
  }
  f32x4 acc[4][4];     // [cb][mb]
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[cb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](const bf16x8 (&w)[4], const bf16x8 (&a)[4]) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[cb][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[cb], a[mb], acc[cb][mb], 0, 0, 0);
  };
  int s = kbeg;
  for (; s + 2 <= kend; s += 2) {               // two K-steps per round trip: 16 x 16-byte loads in flight per lane
    bf16x8 w[2][4], a[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        w[u][i] = *reinterpret_cast<const bf16x8*>(pp[i] + (s + u) * 32);
        a[u][i] = *reinterpret_cast<const bf16x8*>(xp[i] + (s + u) * 32);
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) compute(w[u], a[u]);
  }
  for (; s < kend; ++s) {                       // an odd step left over
    bf16x8 w[4], a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = *reinterpret_cast<const bf16x8*>(pp[i] + s * 32);
      a[i] = *reinterpret_cast<const bf16x8*>(xp[i] + s * 32);
    }
    compute(w, a);
  }
  auto red_at = [&](int p, int cb, int mb) { return reinterpret_cast<f32x4*>(red + ((((p * 4 + cb) * 4 + mb) * 64 + lane) << 2)); };
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) *red_at(wave, cb, mb) = acc[cb][mb];
  __syncthreads();
  // wave w finishes output block w; C/D: col = row of x (lane & 15) of block mb, rows 4g + e = 4 consecutive outputs
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    f32x4 t = *red_at(0, wave, mb);
#pragma unroll
    for (int p = 1; p < PJ_WAVES; ++p) {        // fixed order: bitwise reproducible
      const f32x4 q = *red_at(p, wave, mb);
      t[0] += q[0]; t[1] += q[1]; t[2] += q[2]; t[3] += q[3];
    }
    const int m = m0 + mb * 16 + r;
    if (m < rows) *reinterpret_cast<f32x4*>(part + ((long long)ks * rows + m) * d + n0 + wave * 16 + 4 * g) = t;
  }
}

// One workgroup per row.  z = slab 0 + slab 1 + ... (ascending) + c; a thread keeps its (at most PJ_FIN_VEC) float4 columns
// tid * 4 + i * 1024 in registers.  n2: thread (its columns ascending), then lanes (wave_sum), then waves in order.
__global__ __launch_bounds__(PJ_FIN_THREADS) void project_finish_kernel(
    const float* __restrict__ part, int nslab, long long slab_stride, const float* __restrict__ c, int d, int normalize,
    float* __restrict__ out_f32, uint16_t* __restrict__ out_bf16) {
  __shared__ float s_part[PJ_FIN_THREADS / WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;
  const float* p = part + b * d;
  f32x4 z[PJ_FIN_VEC];
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < PJ_FIN_VEC; ++i) {
    const int col = (i * PJ_FIN_THREADS + tid) * 4;
    z[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < d) {
      f32x4 s = *reinterpret_cast<const f32x4*>(p + col);
      for (int r = 1; r < nslab; ++r) s += *reinterpret_cast<const f32x4*>(p + r * slab_stride + col);
      s += *reinterpret_cast<const f32x4*>(c + col);
      z[i] = s;
      t = fmaf(s[0], s[0], t); t = fmaf(s[1], s[1], t); t = fmaf(s[2], s[2], t); t = fmaf(s[3], s[3], t);
    }
  }
  float inv = 1.f;
  bool zero = false;
  if (normalize) {                              // uniform over the grid
    const float n2 = block_sum_in_wave_order<PJ_FIN_THREADS / WAVE>(wave_sum(t), s_part, lane, wave);
    zero = norm_unusable(n2);                   // the row becomes +0
    inv = 1.0f / sqrtf(n2);
  }
#pragma unroll
  for (int i = 0; i < PJ_FIN_VEC; ++i) {
    const int col = (i * PJ_FIN_THREADS + tid) * 4;
    if (col < d) {
      f32x4 o = normalize ? z[i] * inv : z[i];
      if (zero) o = f32x4{0.f, 0.f, 0.f, 0.f};
      if (out_f32) *reinterpret_cast<f32x4*>(out_f32 + b * d + col) = o;
      if (out_bf16) *reinterpret_cast<uint2*>(out_bf16 + b * d + col) = pack_bf16x4(o);
    }
  }
}

// the part of the status that the three shape arguments decide
static int pj_shape_status(int rows, int D, int d) {
  if (rows < 0 || D < 0 || d < 0) return VPR_ERR_INVALID_ARG;
  if (D == 0 || D % 64 != 0 || d == 0 || d % 64 != 0 || d > PJ_MAX_D_OUT) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

static int pj_route(int rows) { return rows <= VPR_PROJECT_STREAM_MAX_ROWS ? 0 : 1; }

// Monotone in rows: a route-1 call is never offered less than the largest route-0 call of the same (D, d).
static size_t pj_workspace_bytes(int rows, int D, int d) {
  const size_t slabs = (size_t)pj_plan(D, d).nslice;
  const size_t row_bytes = (size_t)d * sizeof(float);
  if (pj_route(rows) == 0) return slabs * (size_t)rows * row_bytes;
  const size_t streaming = slabs * (size_t)VPR_PROJECT_STREAM_MAX_ROWS * row_bytes, tiled = (size_t)rows * row_bytes;
  return tiled > streaming ? tiled : streaming;
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_project_workspace_bytes(int rows, int D, int d) {
  return pj_shape_status(rows, D, d) == VPR_OK ? pj_workspace_bytes(rows, D, d) : 0;
}

extern "C" int vpr_project_route(int rows, int D, int d) {
  const int st = pj_shape_status(rows, D, d);
  return st != VPR_OK ? st : pj_route(rows);
}

extern "C" int vpr_project_rows(const uint16_t* x, long long x_stride, int rows, int D, const uint16_t* P, const float* c,
                                int d, int normalize, float* out_f32, uint16_t* out_bf16, void* workspace,
                                size_t workspace_bytes, void* stream_) {
  if (!x || !P || !c || !workspace || (!out_f32 && !out_bf16) || rows < 0 || D < 0 || d < 0) return VPR_ERR_INVALID_ARG;
  if ((normalize != 0 && normalize != 1) || x_stride < D) return VPR_ERR_INVALID_ARG;
  VPR_TRY_LAUNCH(pj_shape_status(rows, D, d));
  if (x_stride % 8 != 0) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(P) || !aligned16(c) || !aligned16(out_f32) || !aligned16(out_bf16) || !aligned16(workspace))
    return VPR_ERR_UNSUPPORTED;
  const int route = pj_route(rows);
  if (route == 1 && x_stride > 2147483647ll) return VPR_ERR_UNSUPPORTED;           // the GEMM's leading dimension is an int
  if (workspace_bytes < pj_workspace_bytes(rows, D, d)) return VPR_ERR_WORKSPACE;
  if (rows == 0) return VPR_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* part = static_cast<float*>(workspace);
  int nslab = 1;
  if (route == 0) {
    const PjPlan plan = pj_plan(D, d);
    nslab = plan.nslice;
    VPR_TRY_LAUNCH(launch_kernel_lds<project_split_kernel>(dim3(d / 64, plan.nslice, (rows + 63) / 64), dim3(PJ_WAVES * 64),
                                                           PJ_SPLIT_LDS, stream, x, x_stride, rows, D, P, d, part, plan.steps));
  } else {
    const GemmProblem g = gemm_problem(x, (int)x_stride, P, D, nullptr, 0, part, d, 0, rows, d, D);
    VPR_TRY_LAUNCH(D >= 128 && d >= 256 ? launch_gemm256(g, false, stream) : launch_gemm_nt(g, false, stream));
  }
  return launch_kernel(project_finish_kernel, dim3((unsigned)rows), dim3(PJ_FIN_THREADS), 0, stream, part, nslab,
                       (long long)rows * d, c, d, normalize, out_f32, out_bf16);
}
