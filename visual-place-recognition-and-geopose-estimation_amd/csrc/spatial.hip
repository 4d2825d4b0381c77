// spatial.hip — spatial verification of patch matches (contract: include/vpr_amd_spatial.h): a match list per (query, candidate)
// pair votes for shifts of the patch grid; only the matches inside the window of the dominant shift count.
// verify: one 256-thread workgroup per pair.  Everything but the score is integer arithmetic:
//   votes   s_votes[bin] += 1 per match, integer adds into LDS (the counts do not depend on the order of arrival);
//   window  the (2 tol + 1)^2 box sum is separable: s_rows[bin] = the sum of s_votes along the row; the sum of s_rows along
//           the column is formed where it is used, in the argmax, so two int32 planes of <= 5329 bins suffice (static LDS);
//   argmax  the three-part key (support desc, votes desc, bin asc) packed into one 64-bit integer whose maximum is wanted:
//           a per-thread fold, the xor butterfly of a wave, the four waves through LDS;
//   score   thread j - 256 t owns column j of block t, as in the match kernels: lm_block_partials / lm_fold_blocks of
//           local_match.h, the same code, so that a pair whose matches are all inliers reproduces their score bit for bit.
// vpr_spatial_local_rerank: the match launch of local_match.hip (which chooses between its two kernels by the patch count) with
// the match list as its extra output, this file's verify launch, and the order stage with the inlier counts as its payload.
#include <limits.h>
#include "local_match.h"
#include "../../include/vpr_amd_local_hires.h"
#include "../../include/vpr_amd_spatial.h"

namespace vpr {

constexpr int SV_THREADS = 256;                                       // one thread per column of a block of the score sum
constexpr int SV_MAX_BINS = VPR_SPATIAL_MAX_BINS;
constexpr int SV_MAX_N = VPR_SPATIAL_MAX_N;
static_assert(VPR_SPATIAL_MAX_N == VPR_LOCAL_HIRES_MAX_N, "the match kernels' patch limit");
constexpr int SV_MAX_BLOCKS = (SV_MAX_N + SV_THREADS - 1) / SV_THREADS;
static_assert(SV_THREADS == 4 * WAVE, "lm_block_partials: four waves own the 256 columns of a block");
static_assert(SV_MAX_BINS <= 0xffff && SV_MAX_N <= 0xffff, "the argmax key keeps votes and bin in 16 bits each");

// The bin of column j's match, or -1 if the column holds no match: decided from the partner's value alone.
__device__ __forceinline__ int sv_bin(int partner, float sim, int j, int n_q, int gw_q, int gw_g, int gh_g, int W) {
  if (partner < 0 || partner >= n_q || !isfinite(sim)) return -1;
  const int yq = partner / gw_q, xq = partner - yq * gw_q, yg = j / gw_g, xg = j - yg * gw_g;
  return (yq - yg + gh_g - 1) * W + (xq - xg + gw_g - 1);             // 0 <= dx + gw_g - 1 < W, 0 <= dy + gh_g - 1 < H
}

// idx == nullptr: every pair is live (vpr_spatial_verify).  Every output may be null.
__global__ __launch_bounds__(SV_THREADS) void spatial_verify_kernel(
    const int32_t* __restrict__ partner, const float* __restrict__ sim, int n_q, int gw_q, int n_g, int gw_g, int tol,
    const int32_t* __restrict__ idx, int n_local, int index_base, float* __restrict__ ws_score, int32_t* __restrict__ ws_inliers,
    float* __restrict__ score, int32_t* __restrict__ inliers, int32_t* __restrict__ matches, int32_t* __restrict__ shift,
    uint8_t* __restrict__ inlier_mask) {
  __shared__ int s_votes[SV_MAX_BINS];
  __shared__ int s_rows[SV_MAX_BINS];
  __shared__ unsigned long long s_key[4];
  __shared__ float s_part[SV_MAX_BLOCKS * 4];
  __shared__ int s_cnt[SV_MAX_BLOCKS * 4];
  __shared__ int s_nmatch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p = blockIdx.x;
  if (idx) {                                                          // liveness, from the index alone (workgroup-uniform)
    long long r;
    if (!shard_row(idx[p], n_local, index_base, r)) {                 // not local: the sentinels, no list read
      if (tid == 0) {
        if (score) score[p] = -INFINITY;
        if (inliers) inliers[p] = 0;
        if (matches) matches[p] = 0;
        if (shift) { shift[2 * p] = INT_MIN; shift[2 * p + 1] = INT_MIN; }
      }
      return;
    }
  }
  const int gh_q = n_q / gw_q, gh_g = n_g / gw_g;
  const int W = gw_q + gw_g - 1, H = gh_q + gh_g - 1, nb = W * H;     // nb <= SV_MAX_BINS: checked on the host
  const int32_t* pq = partner + p * n_g;
  const float* ps = sim + p * n_g;

  for (int i = tid; i < nb; i += SV_THREADS) s_votes[i] = 0;
  if (tid == 0) s_nmatch = 0;
  __syncthreads();
  {                                                                   // votes
    int mine = 0;
    for (int j = tid; j < n_g; j += SV_THREADS) {
      const int bin = sv_bin(pq[j], ps[j], j, n_q, gw_q, gw_g, gh_g, W);
      if (bin >= 0) { atomicAdd(&s_votes[bin], 1); ++mine; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&s_nmatch, mine);
  }
  __syncthreads();
  for (int i = tid; i < nb; i += SV_THREADS) {                        // window, along the rows
    const int y = i / W, x = i - y * W;
    const int x0 = x - tol < 0 ? 0 : x - tol, x1 = x + tol > W - 1 ? W - 1 : x + tol;
    int s = 0;
    for (int xx = x0; xx <= x1; ++xx) s += s_votes[y * W + xx];
    s_rows[i] = s;
  }
  __syncthreads();
  unsigned long long best = 0;                                        // window along the columns, and the argmax of the key
  for (int i = tid; i < nb; i += SV_THREADS) {
    const int y = i / W, x = i - y * W;
    const int y0 = y - tol < 0 ? 0 : y - tol, y1 = y + tol > H - 1 ? H - 1 : y + tol;
    int s = 0;
    for (int yy = y0; yy <= y1; ++yy) s += s_rows[yy * W + x];
    const unsigned long long key = ((unsigned long long)s << 32) | ((unsigned long long)s_votes[i] << 16) | (unsigned)(0xffff - i);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(best >> 32), o, 64), lo = __shfl_xor((unsigned)best, o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    best = other > best ? other : best;
  }
  if (lane == 0) s_key[wave] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) best = s_key[w] > best ? s_key[w] : best;
  const int dom = 0xffff - (int)(best & 0xffff), by = dom / W, bx = dom - by * W;
  const int nmatch = s_nmatch;

  const int ncb = (n_g + SV_THREADS - 1) / SV_THREADS;
  for (int t = 0; t < ncb; ++t) {                                     // block t: thread j - 256 t owns column j
    const int col = t * SV_THREADS + tid;
    float contrib = 0.f;
    int inl = 0;
    if (col < n_g) {
      const float v = ps[col];
      const int bin = sv_bin(pq[col], v, col, n_q, gw_q, gw_g, gh_g, W);
      if (bin >= 0) {
        const int y = bin / W, x = bin - y * W;
        const int ax = x > bx ? x - bx : bx - x, ay = y > by ? y - by : by - y;
        if (ax <= tol && ay <= tol) { contrib = v; inl = 1; }
      }
      if (inlier_mask) inlier_mask[p * n_g + col] = (uint8_t)inl;
    }
    lm_block_partials(contrib, inl, t, lane, wave, s_part, s_cnt);
  }
  __syncthreads();
  if (tid == 0) {
    float run;
    int c;
    lm_fold_blocks(s_part, s_cnt, ncb, run, c);                        // c = support[dominant]
    if (ws_score) ws_score[p] = run;
    if (ws_inliers) ws_inliers[p] = c;
    if (score) score[p] = run;
    if (inliers) inliers[p] = c;
    if (matches) matches[p] = nmatch;
    if (shift) {
      shift[2 * p] = nmatch ? bx - (gw_g - 1) : INT_MIN;
      shift[2 * p + 1] = nmatch ? by - (gh_g - 1) : INT_MIN;
    }
  }
}

// gw 0 or not dividing n, tol beyond the limit, more bins than the two LDS planes hold; n_q, n_g >= 1 and gw, tol >= 0 here
inline int sv_check_grid(int n_q, int gw_q, int n_g, int gw_g, int tol) {
  if (gw_q == 0 || gw_q > n_q || n_q % gw_q != 0 || gw_g == 0 || gw_g > n_g || n_g % gw_g != 0) return VPR_ERR_UNSUPPORTED;
  if (tol > VPR_SPATIAL_MAX_TOL) return VPR_ERR_UNSUPPORTED;
  const long long W = gw_q + gw_g - 1, H = n_q / gw_q + n_g / gw_g - 1;
  if (W * H > SV_MAX_BINS) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

inline int launch_spatial_verify(const int32_t* partner, const float* sim, long long P, int n_q, int gw_q, int n_g, int gw_g, int tol,
                                 const int32_t* idx, int n_local, int index_base, float* ws_score, int32_t* ws_inliers, float* score,
                                 int32_t* inliers, int32_t* matches, int32_t* shift, uint8_t* inlier_mask, hipStream_t s) {
  return launch_kernel(spatial_verify_kernel, dim3((unsigned)P), dim3(SV_THREADS), 0, s, partner, sim, n_q, gw_q, n_g, gw_g, tol, idx,
                       n_local, index_base, ws_score, ws_inliers, score, inliers, matches, shift, inlier_mask);
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_spatial_workspace_bytes(int B, int kc, int n_g) { return sv_ws_bytes(B, kc, n_g); }

extern "C" int vpr_spatial_verify(const int32_t* partner, const float* sim, int P, int n_q, int gw_q, int n_g, int gw_g, int tol,
                                  float* score, int32_t* inliers, int32_t* matches, int32_t* shift, uint8_t* inlier_mask, void* stream) {
  if (!partner || !sim || !score || !inliers || !matches || !shift) return VPR_ERR_INVALID_ARG;
  if (P < 0 || n_q < 0 || n_g < 0 || gw_q < 0 || gw_g < 0 || tol < 0) return VPR_ERR_INVALID_ARG;
  if (n_q == 0 || n_q > SV_MAX_N || n_g == 0 || n_g > SV_MAX_N) return VPR_ERR_UNSUPPORTED;
  VPR_TRY_LAUNCH(sv_check_grid(n_q, gw_q, n_g, gw_g, tol));
  if (!aligned4(partner) || !aligned4(sim) || !aligned4(score) || !aligned4(inliers) || !aligned4(matches) || !aligned4(shift))
    return VPR_ERR_UNSUPPORTED;
  if (P == 0) return VPR_OK;
  return launch_spatial_verify(partner, sim, P, n_q, gw_q, n_g, gw_g, tol, nullptr, 0, 0, nullptr, nullptr, score, inliers, matches, shift,
                               inlier_mask, static_cast<hipStream_t>(stream));
}

extern "C" int vpr_spatial_local_rerank(const void* q_local, int n_q, const int32_t* idx, int B, int kc,
                                        const void* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                        int k_out, float* vals_out, int32_t* idx_out, int32_t* inliers_out,
                                        float* pair_score, int32_t* pair_inliers, int32_t* pair_matches, int32_t* pair_shift,
                                        int32_t* row_nn, int32_t* col_nn, int feat_is_fp8, int gw_q, int gw_g, int tol,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  VPR_TRY_LAUNCH(lm_check_args(q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out, idx_out, workspace));
  if (gw_q < 0 || gw_g < 0 || tol < 0 || (feat_is_fp8 != 0 && feat_is_fp8 != 1)) return VPR_ERR_INVALID_ARG;
  VPR_TRY_LAUNCH(lm_check_shape(n_q, kc, n_g, l, feat_is_fp8 ? VPR_PATCH_FP8_MIN_L : 32, SV_MAX_N));
  VPR_TRY_LAUNCH(sv_check_grid(n_q, gw_q, n_g, gw_g, tol));
  VPR_TRY_LAUNCH(lm_check_align(q_local, idx, g_local, vals_out, idx_out, inliers_out, pair_score, pair_matches, row_nn, col_nn, workspace));
  if (!aligned4(pair_inliers) || !aligned4(pair_shift)) return VPR_ERR_UNSUPPORTED;
  if (workspace_bytes < sv_ws_bytes(B, kc, n_g)) return VPR_ERR_UNSUPPORTED;
  if (B == 0) return VPR_OK;
  char* ws = static_cast<char*>(workspace);
  float* ws_score = reinterpret_cast<float*>(ws);
  int32_t* ws_count = reinterpret_cast<int32_t*>(ws + lm_ws_half(B, kc));
  int32_t* list_q = reinterpret_cast<int32_t*>(ws + lm_ws_bytes(B, kc));
  float* list_sim = reinterpret_cast<float*>(ws + lm_ws_bytes(B, kc) + sv_ws_list(B, kc, n_g));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  // the match kernels leave the unverified score and match count in ws_score / ws_count; the verify launch replaces them
  VPR_TRY_LAUNCH(launch_local_match_list(feat_is_fp8 != 0, q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, ws_score,
                                         ws_count, row_nn, col_nn, list_q, list_sim, s));
  VPR_TRY_LAUNCH(launch_spatial_verify(list_q, list_sim, (long long)B * kc, n_q, gw_q, n_g, gw_g, tol, idx, n_local, index_base, ws_score,
                                       ws_count, pair_score, pair_inliers, pair_matches, pair_shift, nullptr, s));
  VPR_TRY_LAUNCH(launch_local_order(ws_score, ws_count, idx, B, kc, n_local, index_base, k_out, vals_out, idx_out, inliers_out, s));
  return VPR_OK;
}
