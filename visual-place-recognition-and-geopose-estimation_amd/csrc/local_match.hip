// local_match.hip — local-feature re-ranking: mutual-nearest-neighbour patch matching (contract: include/vpr_amd_local.h).
// match: a (query, group of LM_GROUP candidates) grid of 8-wave workgroups.  Liveness comes from the index alone: a workgroup
// without a live candidate ends before it loads or stages anything.  Wave w owns query rows 32 w .. 32 w + 31 and keeps their
// MFMA A-fragments (l / 16 of them) in registers while the workgroup walks its candidates; each live candidate's features are
// staged once in LDS with 16-byte loads, rows padded to a multiple of 32 with zeros, chunks XOR-swizzled so the B-fragment
// ds_read_b128 of the 32x32x16 operand map is conflict-free.  S is never stored: a wave forms one 32 x 32 tile of it at a time
// (column on the lane, rows in the 16 registers) and folds it into
//   - a running (value, index) per register for the row argmax r(i): columns ascend per lane, so a strict > keeps the lowest
//     index; the 32 lanes of a half are reduced once per candidate with the index in the comparison;
//   - a per-lane (value, index) over the 16 registers for the column argmax c(j): the two halves are combined through lane
//     xor 32, the 8 waves through LDS in ascending wave (= row) order.
// Thread j < n_g then decides column j's match and the score is summed in the order the header states.
// order: one 128-thread workgroup per query: order_rank of vpr_common.h, the order stage of vpr_rerank_rows.
#include <float.h>
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_local.h"

namespace vpr {

constexpr int LM_WAVES = 8;                         // = VPR_LOCAL_MAX_N / 32 row tiles
constexpr int LM_THREADS = LM_WAVES * WAVE;
constexpr int LM_GROUP = 4;                         // candidates per workgroup
constexpr int LM_MAX_N = VPR_LOCAL_MAX_N;
static_assert(LM_WAVES * 32 == LM_MAX_N && VPR_LOCAL_MAX_KC == ORDER_MAX_KC, "one wave per 32-row tile; order_rank's workgroup");

// a beats b: a exists and (b does not, or a's value is larger, or equal with the lower index)
__device__ __forceinline__ bool lm_better(float av, int ai, float bv, int bi) {
  return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi));
}

// Swizzle of the staged features: chunk c of row r (a row is CPR = L / 8 chunks of 16 B) sits at chunk c ^ f(r) of its row,
// f chosen so that 16 consecutive rows at one logical chunk fall into 16 distinct 16-byte slots of the 256-byte bank row.
// CPR is a multiple of 4, and f(r) stays below the largest power of two (<= 16) dividing CPR: the XOR stays inside the row.
template <int L>
__device__ __forceinline__ int lm_off(int row, int chunk) {
  constexpr int CPR = L / 8;
  constexpr int SH = CPR % 16 == 0 ? 0 : CPR % 8 == 0 ? 1 : 2, MASK = CPR % 16 == 0 ? 15 : CPR % 8 == 0 ? 7 : 3;
  return (row * CPR + (chunk ^ ((row >> SH) & MASK))) << 4;
}

// LDS of one workgroup: features [ngp][L] bf16 | column best value [8][ngp] f32 | column best row [8][ngp] i32 |
// row_nn [256] i32 | wave sums [4] f32 + wave counts [4] i32, ngp = n_g rounded up to 32
inline size_t lm_lds_bytes(int n_g, int l) {
  const size_t ngp = (size_t)(n_g + 31) / 32 * 32;
  return ngp * l * 2 + 2 * LM_WAVES * ngp * 4 + LM_MAX_N * 4 + 32;
}

template <int L>
__global__ __launch_bounds__(LM_THREADS) void local_match_kernel(
    const uint16_t* __restrict__ q_local, int n_q, const int32_t* __restrict__ idx, int kc, const uint16_t* __restrict__ g_local,
    int n_g, int n_local, int index_base, float min_sim, float* __restrict__ ws_score, int32_t* __restrict__ ws_matches,
    float* __restrict__ pair_score, int32_t* __restrict__ pair_matches, int32_t* __restrict__ row_nn, int32_t* __restrict__ col_nn) {
  constexpr int KS = L / 16, CPR = L / 8;
  extern __shared__ __attribute__((aligned(16))) char s_mem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const long long b = blockIdx.x;                                     // queries on x: the grid's y extent is 16 bits
  const int j0 = blockIdx.y * LM_GROUP;
  const int ngp = (n_g + 31) / 32 * 32, ntile = ngp / 32;
  const int nqt = (n_q + 31) / 32;                                    // row tiles that exist
  char* s_g = s_mem;
  float* s_colv = reinterpret_cast<float*>(s_mem + (size_t)ngp * L * 2);
  int* s_coli = reinterpret_cast<int*>(s_colv + LM_WAVES * ngp);
  int* s_rownn = s_coli + LM_WAVES * ngp;
  float* s_part = reinterpret_cast<float*>(s_rownn + LM_MAX_N);
  int* s_cnt = reinterpret_cast<int*>(s_part + 4);

  // liveness of the group, from the index alone; the optional per-pair outputs of a non-live candidate
  bool any = false;
#pragma unroll
  for (int g = 0; g < LM_GROUP; ++g) {
    const int j = j0 + g;
    long long r;
    const bool live = j < kc && shard_row(idx[b * kc + (j < kc ? j : 0)], n_local, index_base, r);   // workgroup-uniform
    any |= live;
    if (j < kc && !live) {
      const long long p = b * kc + j;
      if (pair_score && tid == 0) pair_score[p] = -INFINITY;
      if (pair_matches && tid == 0) pair_matches[p] = 0;
      if (row_nn) for (int i = tid; i < n_q; i += LM_THREADS) row_nn[p * n_q + i] = -1;
      if (col_nn) for (int i = tid; i < n_g; i += LM_THREADS) col_nn[p * n_g + i] = -1;
    }
  }
  if (!any) return;                                                   // nothing of this group is local: no loads, no staging

  // the query's A-fragments: lane holds Q[32 wave + li][16 ks + 8 h .. + 8]; rows past n_q are zero
  bf16x8 a[KS];
  {
    const int row = wave * 32 + li;
    const uint16_t* qrow = q_local + (b * n_q + (row < n_q ? row : 0)) * L + 8 * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      i32x4 v = *reinterpret_cast<const i32x4*>(qrow + 16 * ks);
      if (row >= n_q) v = i32x4{0, 0, 0, 0};
      a[ks] = __builtin_bit_cast(bf16x8, v);
    }
  }

#pragma unroll 1
  for (int g = 0; g < LM_GROUP; ++g) {
    long long grow = 0;
    if (j0 + g >= kc || !shard_row(idx[b * kc + j0 + g], n_local, index_base, grow)) continue;      // uniform
    const long long p = b * kc + j0 + g;
    __syncthreads();                                                  // the previous candidate's LDS is no longer read
    {                                                                 // stage [n_g][L] -> LDS, rows n_g .. ngp - 1 zero
      const uint16_t* gimg = g_local + grow * n_g * L;                // 0 <= grow < n_local: inside g_local
      for (int t = tid; t < ngp * CPR; t += LM_THREADS) {
        const int row = t / CPR, c = t - row * CPR;
        i32x4 v = i32x4{0, 0, 0, 0};
        if (row < n_g) v = *reinterpret_cast<const i32x4*>(gimg + (long long)row * L + 8 * c);
        *reinterpret_cast<i32x4*>(s_g + lm_off<L>(row, c)) = v;
      }
    }
    __syncthreads();

    if (wave < nqt) {                                                 // wave-uniform; no barrier inside
      float rbv[16];
      int rbi[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) { rbv[r] = -INFINITY; rbi[r] = -1; }
      for (int jt = 0; jt < ntile; ++jt) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 bf = *reinterpret_cast<const bf16x8*>(s_g + lm_off<L>(jt * 32 + li, 2 * ks + h));
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks], bf, acc, 0, 0, 0);
        }
        // acc[r] = S[32 wave + (r & 3) + 8 (r >> 2) + 4 h][32 jt + li]
        const int col = jt * 32 + li;
        const bool col_ok = col < n_g;
        float cv = -INFINITY;
        int ci = -1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float v = acc[r];
          const bool ok = col_ok && row < n_q && isfinite(v);
          if (ok && (rbi[r] < 0 || v > rbv[r])) { rbv[r] = v; rbi[r] = col; }     // columns ascend per lane
          if (ok && (ci < 0 || v > cv)) { cv = v; ci = row; }                     // rows ascend with r
        }
        {                                                             // the other half's rows interleave with this one's
          const float ov = __shfl_xor(cv, 32, 64);
          const int oi = __shfl_xor(ci, 32, 64);
          if (lm_better(ov, oi, cv, ci)) { cv = ov; ci = oi; }
        }
        if (h == 0) { s_colv[wave * ngp + col] = cv; s_coli[wave * ngp + col] = ci; }
      }
      // r(i): reduce the 32 lanes of each half
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = rbv[r];
        int i = rbi[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
          const float ov = __shfl_xor(v, o, 64);
          const int oi = __shfl_xor(i, o, 64);
          if (lm_better(ov, oi, v, i)) { v = ov; i = oi; }
        }
        const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (li == 0 && row < n_q) {
          s_rownn[row] = i;
          if (row_nn) row_nn[p * n_q + row] = i;
        }
      }
    }
    __syncthreads();

    // column j = tid: c(j) over the waves in ascending row order, the match, the score
    float contrib = 0.f;
    int matched = 0;
    if (tid < n_g) {
      float cv = -INFINITY;
      int ci = -1;
      for (int w = 0; w < nqt; ++w) {
        const float v = s_colv[w * ngp + tid];
        const int i = s_coli[w * ngp + tid];
        if (i >= 0 && (ci < 0 || v > cv)) { cv = v; ci = i; }
      }
      if (col_nn) col_nn[p * n_g + tid] = ci;
      if (ci >= 0 && s_rownn[ci] == tid && cv >= min_sim) { contrib = cv; matched = 1; }
    }
    if (wave < 4) {                                                   // columns 0 .. 255
      const float ws = wave_sum(contrib);
      int wc = matched;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) wc += __shfl_xor(wc, o, 64);
      if (lane == 0) { s_part[wave] = ws; s_cnt[wave] = wc; }
    }
    __syncthreads();
    if (tid == 0) {
      float s = 0.f;
      int c = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) { s += s_part[w]; c += s_cnt[w]; }
      s = fminf(fmaxf(s, -FLT_MAX), FLT_MAX);                         // every term is finite; an overflowing sum is clamped
      ws_score[p] = s;
      ws_matches[p] = c;
      if (pair_score) pair_score[p] = s;
      if (pair_matches) pair_matches[p] = c;
    }
  }
}

__global__ __launch_bounds__(ORDER_MAX_KC) void local_order_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ matches, const int32_t* __restrict__ idx, int kc, int n_local,
    int index_base, int k_out, float* __restrict__ vals_out, int32_t* __restrict__ idx_out, int32_t* __restrict__ matches_out) {
  __shared__ unsigned long long s_key[ORDER_MAX_KC];
  const long long b = blockIdx.x;
  float val;
  int id;
  const int rank = order_rank(scores, idx, b, kc, n_local, index_base, s_key, val, id);
  if (rank >= 0 && rank < k_out) {
    vals_out[b * k_out + rank] = val;
    idx_out[b * k_out + rank] = id;
    if (matches_out) matches_out[b * k_out + rank] = id >= 0 ? matches[b * kc + threadIdx.x] : 0;
  }
}

template <int L>
int launch_local_match(dim3 grid, size_t lds, hipStream_t s, const uint16_t* q_local, int n_q, const int32_t* idx, int kc,
                       const uint16_t* g_local, int n_g, int n_local, int index_base, float min_sim, float* ws_score,
                       int32_t* ws_matches, float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn) {
  VPR_TRY_LAUNCH(optin_dynamic_lds<local_match_kernel<L>>(lm_lds_bytes(LM_MAX_N, L)));      // the LDS size varies per call: the maximum
  return launch_kernel(local_match_kernel<L>, grid, dim3(LM_THREADS), lds, s, q_local, n_q, idx, kc, g_local, n_g, n_local,
                       index_base, min_sim, ws_score, ws_matches, pair_score, pair_matches, row_nn, col_nn);
}

inline size_t lm_ws_half(int B, int kc) { return align_up((size_t)(B > 0 ? B : 1) * kc * sizeof(float), 256); }

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_local_workspace_bytes(int B, int kc) {
  if (B < 0 || kc < 1 || kc > VPR_LOCAL_MAX_KC) return 0;
  return 2 * lm_ws_half(B, kc);                                       // f32 scores | i32 match counts
}

extern "C" int vpr_local_rerank(const uint16_t* q_local, int n_q, const int32_t* idx, int B, int kc,
                                const uint16_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                                float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!q_local || !idx || !g_local || !vals_out || !idx_out || !workspace) return VPR_ERR_INVALID_ARG;
  if (B < 0 || n_q < 0 || n_g < 0 || l < 0 || kc < 0 || n_local < 0 || index_base < 0) return VPR_ERR_INVALID_ARG;
  if (k_out < 1 || k_out > kc) return VPR_ERR_INVALID_ARG;
  if (isnan(min_sim)) return VPR_ERR_INVALID_ARG;
  if (kc > VPR_LOCAL_MAX_KC || n_q == 0 || n_q > LM_MAX_N || n_g == 0 || n_g > LM_MAX_N) return VPR_ERR_UNSUPPORTED;
  if (l == 0 || l % 32 != 0 || l > VPR_LOCAL_MAX_L) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(q_local) || !aligned16(g_local) || !aligned16(workspace)) return VPR_ERR_UNSUPPORTED;   // read as 16-byte chunks
  if (!aligned4(idx) || !aligned4(vals_out) || !aligned4(idx_out) || !aligned4(matches_out) || !aligned4(pair_score) ||
      !aligned4(pair_matches) || !aligned4(row_nn) || !aligned4(col_nn)) return VPR_ERR_UNSUPPORTED;
  if (workspace_bytes < vpr_local_workspace_bytes(B, kc)) return VPR_ERR_UNSUPPORTED;
  if (B == 0) return VPR_OK;
  float* ws_score = static_cast<float*>(workspace);
  int32_t* ws_matches = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + lm_ws_half(B, kc));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)B, (unsigned)((kc + LM_GROUP - 1) / LM_GROUP));
  const size_t lds = lm_lds_bytes(n_g, l);
#define LM_CASE(LL) case LL: VPR_TRY_LAUNCH(launch_local_match<LL>(grid, lds, s, q_local, n_q, idx, kc, g_local, n_g, n_local, \
    index_base, min_sim, ws_score, ws_matches, pair_score, pair_matches, row_nn, col_nn)); break;
  switch (l) {
    LM_CASE(32) LM_CASE(64) LM_CASE(96) LM_CASE(128) LM_CASE(160) LM_CASE(192) LM_CASE(224) LM_CASE(256)
    default: return VPR_ERR_UNSUPPORTED;
  }
#undef LM_CASE
  VPR_TRY_LAUNCH(launch_kernel(local_order_kernel, dim3((unsigned)B), dim3(ORDER_MAX_KC), 0, s,
                               static_cast<const float*>(ws_score), static_cast<const int32_t*>(ws_matches), idx, kc, n_local,
                               index_base, k_out, vals_out, idx_out, matches_out));
  return VPR_OK;
}
