// query_expand.hip — query expansion / gallery augmentation from a top-k list (contract: include/vpr_amd_expand.h).
// expand: a (query, column slice) grid of 128-thread workgroups; a thread owns one 16-byte chunk of the row (8 bf16 or 16
// e4m3 elements).  The workgroup first turns the query's n_use neighbours into a compacted list (row offset, coefficient)
// of the ones this shard owns with a non-zero weight, in ascending j, in LDS; from there on everything about a neighbour
// is uniform over the workgroup.  A thread then requests its chunk of up to XQ_NJ neighbours and adds them in list order.
// finish: one 1024-thread workgroup per query; the shard sum is formed twice (norm, then scale) instead of being kept.
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_expand.h"

// Row loads with the nt cache policy (1) or the default one (0): a timing switch of the build (scripts/query_expand_bench.py,
// DESIGN.md §3.6); the result does not depend on it.
#ifndef VPR_EXPAND_NT
#define VPR_EXPAND_NT 0
#endif

namespace vpr {

constexpr int XQ_THREADS = 128;      // = the largest k: thread j prepares neighbour j
constexpr int XQ_MAX_K = 128;
constexpr int XQ_NJ = 16;            // row chunks a thread has in flight
constexpr int XF_THREADS = 1024;
constexpr int XF_MAX_R = 64;

__device__ __forceinline__ i32x4 load_row_chunk(const char* p) {
#if VPR_EXPAND_NT
  return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p));
#else
  return *reinterpret_cast<const i32x4*>(p);
#endif
}

// acc[e] = c * x[e] + acc[e] over the E elements of one 16-byte chunk
template <bool FP8>
__device__ __forceinline__ void add_chunk(float* acc, i32x4 v, float c) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if constexpr (FP8) {
      acc[4 * w + 0] = fmaf(c, __builtin_amdgcn_cvt_f32_fp8(v[w], 0), acc[4 * w + 0]);
      acc[4 * w + 1] = fmaf(c, __builtin_amdgcn_cvt_f32_fp8(v[w], 1), acc[4 * w + 1]);
      acc[4 * w + 2] = fmaf(c, __builtin_amdgcn_cvt_f32_fp8(v[w], 2), acc[4 * w + 2]);
      acc[4 * w + 3] = fmaf(c, __builtin_amdgcn_cvt_f32_fp8(v[w], 3), acc[4 * w + 3]);
    } else {
      acc[2 * w + 0] = fmaf(c, bf16_lo(v[w]), acc[2 * w + 0]);
      acc[2 * w + 1] = fmaf(c, bf16_hi(v[w]), acc[2 * w + 1]);
    }
  }
}

template <bool FP8>
__global__ __launch_bounds__(XQ_THREADS) void query_expand_kernel(
    const uint16_t* __restrict__ q, const float* __restrict__ vals, const int32_t* __restrict__ idx, int D, int k,
    const char* __restrict__ rows, const float* __restrict__ row_scales, int n_local, int index_base,
    int n_use, double alpha, float q_weight, int add_query, float* __restrict__ partial) {
  constexpr int E = FP8 ? 16 : 8;                       // elements of a 16-byte row chunk
  __shared__ long long s_off[XQ_MAX_K];                 // byte offset of the neighbour's row in `rows`
  __shared__ float s_coef[XQ_MAX_K];
  __shared__ int s_count[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                       // queries on x: the grid's y extent is 16 bits
  const long long row_bytes = FP8 ? (long long)D : 2ll * D;

  // thread j: neighbour j.  Nothing of a neighbour that is not local is read beyond its index.
  bool live = false;
  long long off = 0;
  float coef = 0.f;
  if (tid < n_use) {
    long long r;
    if (shard_row(idx[b * k + tid], n_local, index_base, r)) {
      const float v = vals[b * k + tid];
      if (v > 0.f) {
        coef = alpha == 0.0 ? 1.f : (float)pow((double)v, alpha);
        if constexpr (FP8) coef *= row_scales[r];
        live = coef != 0.f;                             // a weight that rounds to 0 contributes nothing either
        off = r * row_bytes;
      }
    }
  }
  const unsigned long long mask = __ballot(live);
  if (lane == 0) s_count[wave] = __popcll(mask);
  __syncthreads();
  const int n_live = s_count[0] + s_count[1];
  if (live) {
    const int pos = (wave ? s_count[0] : 0) + __popcll(mask & ((1ull << lane) - 1ull));
    s_off[pos] = off;
    s_coef[pos] = coef;
  }
  __syncthreads();

  const int chunk = blockIdx.y * XQ_THREADS + tid;
  if (chunk * E >= D) return;                           // the tail of the last column slice; no barrier follows
  const long long d0 = (long long)chunk * E;

  float acc[E];
  if (add_query) {
#pragma unroll
    for (int h = 0; h < E / 8; ++h) {
      const s16x8 qv = *reinterpret_cast<const s16x8*>(q + b * D + d0 + 8 * h);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[8 * h + e] = q_weight * bf16_bits_to_f32((uint16_t)qv[e]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
  }

  const char* base = rows + (long long)chunk * 16;
  for (int j0 = 0; j0 < n_live; j0 += XQ_NJ) {          // uniform over the workgroup
    i32x4 v[XQ_NJ];
#pragma unroll
    for (int i = 0; i < XQ_NJ; ++i)
      if (j0 + i < n_live) v[i] = load_row_chunk(base + s_off[j0 + i]);
#pragma unroll
    for (int i = 0; i < XQ_NJ; ++i)
      if (j0 + i < n_live) add_chunk<FP8>(acc, v[i], s_coef[j0 + i]);
  }

  float* out = partial + b * D + d0;
#pragma unroll
  for (int e = 0; e < E; e += 4)
    *reinterpret_cast<f32x4*>(out + e) = f32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]};
}

// s[d .. d+3] of query b: the shard partials added in ascending r
__device__ __forceinline__ f32x4 shard_sum(const float* __restrict__ p, long long shard_stride, int R) {
  f32x4 s = *reinterpret_cast<const f32x4*>(p);
  for (int r = 1; r < R; ++r) s += *reinterpret_cast<const f32x4*>(p + r * shard_stride);
  return s;
}

__global__ __launch_bounds__(XF_THREADS) void query_expand_finish_kernel(
    const float* __restrict__ partials, int R, const uint16_t* __restrict__ q, int B, int D,
    float* __restrict__ out_f32, uint16_t* __restrict__ out_bf16) {
  __shared__ float s_part[XF_THREADS / WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;
  const long long shard_stride = (long long)B * D;
  const float* p = partials + b * D;

  float t = 0.f;                                        // thread: its columns in ascending d; then lanes, then waves
  for (int d = tid * 4; d < D; d += XF_THREADS * 4) {
    const f32x4 s = shard_sum(p + d, shard_stride, R);
    t = fmaf(s[0], s[0], t); t = fmaf(s[1], s[1], t); t = fmaf(s[2], s[2], t); t = fmaf(s[3], s[3], t);
  }
  const float n2 = block_sum_in_wave_order<XF_THREADS / WAVE>(wave_sum(t), s_part, lane, wave);

  const bool keep_q = norm_unusable(n2);                // the query stays what it was
  const float inv = 1.0f / sqrtf(n2);
  for (int d = tid * 4; d < D; d += XF_THREADS * 4) {
    f32x4 o;
    if (keep_q) {
      const uint2 qv = *reinterpret_cast<const uint2*>(q + b * D + d);
      o = f32x4{bf16_lo(qv.x), bf16_hi(qv.x), bf16_lo(qv.y), bf16_hi(qv.y)};
      if (out_bf16) *reinterpret_cast<uint2*>(out_bf16 + b * D + d) = qv;
    } else {
      o = shard_sum(p + d, shard_stride, R) * inv;
      if (out_bf16) *reinterpret_cast<uint2*>(out_bf16 + b * D + d) = pack_bf16x4(o);
    }
    if (out_f32) *reinterpret_cast<f32x4*>(out_f32 + b * D + d) = o;
  }
}

static int finish_status(const float* partials, int R, const uint16_t* q, int B, int D, float* out_f32, uint16_t* out_bf16) {
  if (!partials || !q || (!out_f32 && !out_bf16) || B < 0 || D < 0 || R < 1) return VPR_ERR_INVALID_ARG;
  if (R > XF_MAX_R || D == 0 || D % 64 != 0) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(partials) || !aligned16(q) || !aligned16(out_f32) || !aligned16(out_bf16)) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

static int launch_finish(const float* partials, int R, const uint16_t* q, int B, int D, float* out_f32, uint16_t* out_bf16,
                         hipStream_t stream) {
  return launch_kernel(query_expand_finish_kernel, dim3((unsigned)B), dim3(XF_THREADS), 0, stream, partials, R, q, B, D,
                       out_f32, out_bf16);
}

}  // namespace vpr

using namespace vpr;

extern "C" int vpr_query_expand(const uint16_t* q, const float* vals, const int32_t* idx, int B, int D, int k,
                                const void* rows, const float* row_scales, int n_local, int index_base,
                                int n_use, double alpha, double q_weight, int add_query,
                                float* partial, float* out_f32, uint16_t* out_bf16, void* stream) {
  if (!q || !vals || !idx || !rows || !partial || B < 0 || D < 0 || k < 0 || n_local < 0) return VPR_ERR_INVALID_ARG;
  if (n_use < 1 || n_use > k) return VPR_ERR_INVALID_ARG;
  if (!(alpha >= 0.0) || !(q_weight >= 0.0)) return VPR_ERR_INVALID_ARG;                  // NaN fails the comparison
  if (add_query != 0 && add_query != 1) return VPR_ERR_INVALID_ARG;
  if (k > XQ_MAX_K || D == 0 || D % 64 != 0) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(q) || !aligned16(rows) || !aligned16(partial)) return VPR_ERR_UNSUPPORTED;
  const bool finish = out_f32 || out_bf16;
  if (finish) VPR_TRY_LAUNCH(finish_status(partial, 1, q, B, D, out_f32, out_bf16));
  if (B == 0) return VPR_OK;
  const bool fp8 = row_scales != nullptr;
  const int chunks = D / (fp8 ? 16 : 8);
  const dim3 grid((unsigned)B, (unsigned)((chunks + XQ_THREADS - 1) / XQ_THREADS));
  const auto kernel = fp8 ? query_expand_kernel<true> : query_expand_kernel<false>;
  VPR_TRY_LAUNCH(launch_kernel(kernel, grid, dim3(XQ_THREADS), 0, static_cast<hipStream_t>(stream), q, vals, idx, D, k,
                               static_cast<const char*>(rows), row_scales, n_local, index_base, n_use, alpha,
                               (float)q_weight, add_query, partial));
  if (finish) VPR_TRY_LAUNCH(launch_finish(partial, 1, q, B, D, out_f32, out_bf16, static_cast<hipStream_t>(stream)));
  return VPR_OK;
}

extern "C" int vpr_query_expand_finish(const float* partials, int R, const uint16_t* q, int B, int D,
                                       float* out_f32, uint16_t* out_bf16, void* stream) {
  VPR_TRY_LAUNCH(finish_status(partials, R, q, B, D, out_f32, out_bf16));
  if (B == 0) return VPR_OK;
  return launch_finish(partials, R, q, B, D, out_f32, out_bf16, static_cast<hipStream_t>(stream));
}
