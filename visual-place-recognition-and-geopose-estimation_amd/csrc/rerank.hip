// rerank.hip — two-tier retrieval: re-rank a coarse candidate list on full-precision rows (contract: include/vpr_amd_rerank.h).
// score: a (query, group of RR_WAVES candidates) grid; wave w of a workgroup owns candidate group * RR_WAVES + w.  Liveness
// comes from the index alone: a workgroup without a live candidate ends before it stages the query, a wave without one ends
// right after the staging barrier, before any row access.  The query is staged once per workgroup as f32 in LDS; a lane then
// requests up to RR_NJ 16-byte chunks of its row before it adds the first (the row's address is wave-uniform, its chunks are
// lane + 64 u), so the scattered row reads overlap while the order of the sum stays the one the header states.
// order: one 128-thread workgroup per query; thread j ranks candidate j (order_rank of vpr_common.h, shared with
// local_match.hip) and writes it if that rank < k_out.
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_rerank.h"

namespace vpr {

constexpr int RR_WAVES = 8;                       // candidates (= waves) per score workgroup
constexpr int RR_THREADS = RR_WAVES * WAVE;
constexpr int RR_NJ = 8;                          // row chunks a lane has in flight
constexpr int RR_MAX_KC = VPR_RERANK_MAX_KC;      // = the order kernel's workgroup: thread j ranks candidate j
static_assert(RR_MAX_KC == ORDER_MAX_KC, "order_rank is written for one thread per candidate");
constexpr int RR_MAX_D = VPR_RERANK_MAX_D;        // 4 * D bytes of LDS <= 64 KB

// a[e] = fmaf(q[e], row[e], a[e]) over the E elements of one 16-byte row chunk; q is the chunk's E staged f32 values
template <bool ROWS_F32>
__device__ __forceinline__ void dot_chunk(float* a, i32x4 v, const float* __restrict__ qs) {
  if constexpr (ROWS_F32) {
    const f32x4 qv = *reinterpret_cast<const f32x4*>(qs);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fmaf(qv[e], __int_as_float(v[e]), a[e]);
  } else {
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(qs), q1 = *reinterpret_cast<const f32x4*>(qs + 4);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float qe = w < 2 ? q0[2 * w] : q1[2 * w - 4], qo = w < 2 ? q0[2 * w + 1] : q1[2 * w - 3];
      a[2 * w + 0] = fmaf(qe, bf16_lo(v[w]), a[2 * w + 0]);
      a[2 * w + 1] = fmaf(qo, bf16_hi(v[w]), a[2 * w + 1]);
    }
  }
}

template <bool Q_F32, bool ROWS_F32>
__global__ __launch_bounds__(RR_THREADS) void rerank_score_kernel(
    const void* __restrict__ q, const int32_t* __restrict__ idx, int D, int kc, const char* __restrict__ rows, int n_local,
    int index_base, float* __restrict__ scores) {
  constexpr int E = ROWS_F32 ? VPR_RERANK_CHUNK_F32 : VPR_RERANK_CHUNK_BF16;
  extern __shared__ __attribute__((aligned(16))) float s_q[];          // [D]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                                     // queries on x: the grid's y extent is 16 bits
  const int j = blockIdx.y * RR_WAVES + wave;

  long long r = 0;
  const bool live = j < kc && shard_row(idx[b * kc + (j < kc ? j : 0)], n_local, index_base, r);   // wave-uniform
  if (!__syncthreads_or(live)) return;                                // nothing of this group is local: no staging

  if constexpr (Q_F32) {
    const float* qrow = static_cast<const float*>(q) + b * D;
    for (int d = tid * 4; d < D; d += RR_THREADS * 4)
      *reinterpret_cast<f32x4*>(s_q + d) = *reinterpret_cast<const f32x4*>(qrow + d);
  } else {
    const uint16_t* qrow = static_cast<const uint16_t*>(q) + b * D;
    for (int d = tid * 8; d < D; d += RR_THREADS * 8) {
      const i32x4 v = *reinterpret_cast<const i32x4*>(qrow + d);
#pragma unroll
      for (int w = 0; w < 4; w += 2)
        *reinterpret_cast<f32x4*>(s_q + d + 2 * w) = f32x4{bf16_lo(v[w]), bf16_hi(v[w]), bf16_lo(v[w + 1]), bf16_hi(v[w + 1])};
    }
  }
  __syncthreads();
  if (!live) return;                                                  // no barrier follows

  const int nchunks = D / E;
  const long long row_bytes = (long long)D * (ROWS_F32 ? 4 : 2);
  const char* row = rows + r * row_bytes;                             // 0 <= r < n_local: inside `rows`
  float a[E];
#pragma unroll
  for (int e = 0; e < E; ++e) a[e] = 0.f;
  for (int c0 = 0; c0 < nchunks; c0 += WAVE * RR_NJ) {                // uniform over the wave
    i32x4 v[RR_NJ];
#pragma unroll
    for (int i = 0; i < RR_NJ; ++i) {
      const int c = c0 + WAVE * i + lane;
      if (c < nchunks) v[i] = *reinterpret_cast<const i32x4*>(row + (long long)c * 16);
    }
#pragma unroll
    for (int i = 0; i < RR_NJ; ++i) {
      const int c = c0 + WAVE * i + lane;
      if (c < nchunks) dot_chunk<ROWS_F32>(a, v[i], s_q + c * E);
    }
  }
  float s;
  if constexpr (E == 4) s = (a[0] + a[1]) + (a[2] + a[3]);
  else s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  s = wave_sum(s);
  if (lane == 0) scores[b * kc + j] = s;
}

__global__ __launch_bounds__(RR_MAX_KC) void rerank_order_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ idx, int kc, int n_local, int index_base, int k_out,
    float* __restrict__ vals_out, int32_t* __restrict__ idx_out) {
  __shared__ unsigned long long s_key[RR_MAX_KC];
  const long long b = blockIdx.x;
  float val;
  int id;
  const int rank = order_rank(scores, idx, b, kc, n_local, index_base, s_key, val, id);
  if (rank >= 0 && rank < k_out) {
    vals_out[b * k_out + rank] = val;
    idx_out[b * k_out + rank] = id;
  }
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_rerank_workspace_bytes(int B, int kc) {
  if (B < 0 || kc < 1 || kc > RR_MAX_KC) return 0;
  return align_up((size_t)(B > 0 ? B : 1) * kc * sizeof(float), 256);
}

extern "C" int vpr_rerank_rows(const void* q, int q_is_f32, const int32_t* idx, int B, int D, int kc,
                               const void* rows, int rows_are_f32, int n_local, int index_base,
                               int k_out, float* vals_out, int32_t* idx_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !idx || !rows || !vals_out || !idx_out || !workspace) return VPR_ERR_INVALID_ARG;
  if (B < 0 || D < 0 || kc < 0 || n_local < 0 || index_base < 0) return VPR_ERR_INVALID_ARG;
  if (k_out < 1 || k_out > kc) return VPR_ERR_INVALID_ARG;
  if ((q_is_f32 != 0 && q_is_f32 != 1) || (rows_are_f32 != 0 && rows_are_f32 != 1)) return VPR_ERR_INVALID_ARG;
  if (kc > RR_MAX_KC || D == 0 || D % 64 != 0 || D > RR_MAX_D) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(q) || !aligned16(rows) || !aligned16(workspace)) return VPR_ERR_UNSUPPORTED;      // read as 16-byte chunks
  if (!aligned4(idx) || !aligned4(vals_out) || !aligned4(idx_out)) return VPR_ERR_UNSUPPORTED;
  if (workspace_bytes < vpr_rerank_workspace_bytes(B, kc)) return VPR_ERR_UNSUPPORTED;
  if (B == 0) return VPR_OK;
  float* scores = static_cast<float*>(workspace);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)B, (unsigned)((kc + RR_WAVES - 1) / RR_WAVES));
  const auto score = q_is_f32 ? (rows_are_f32 ? rerank_score_kernel<true, true> : rerank_score_kernel<true, false>)
                              : (rows_are_f32 ? rerank_score_kernel<false, true> : rerank_score_kernel<false, false>);
  VPR_TRY_LAUNCH(launch_kernel(score, grid, dim3(RR_THREADS), (size_t)D * sizeof(float), s, q, idx, D, kc,
                               static_cast<const char*>(rows), n_local, index_base, scores));
  VPR_TRY_LAUNCH(launch_kernel(rerank_order_kernel, dim3((unsigned)B), dim3(RR_MAX_KC), 0, s,
                               static_cast<const float*>(scores), idx, kc, n_local, index_base, k_out, vals_out, idx_out));
  return VPR_OK;
}
