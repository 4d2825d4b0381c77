// similarity.hip — verification of patch matches under a similarity transform (contract: include/vpr_amd_similarity.h): 256
// two-match hypotheses of scale, rotation and shift per (query, candidate) pair; the matches within tol patches of the best
// hypothesis' prediction count.  The sibling of spatial.hip, whose dominant-shift vote smears under a zoom.
// verify: one 256-thread workgroup per pair.  Everything but the score is integer arithmetic:
//   compact  the columns in blocks of 256, thread j - 256 t owns column j: a match's four coordinates (each below 64) packed
//            into the four bytes of one word and written to s_list at its rank in column order; the rank is a wave ballot's
//            popcount below the lane plus the matches of the waves and blocks before it (s_wcnt, one barrier) — no atomic;
//   count    thread h builds hypothesis h from two words of s_list and tests all M matches against it: every lane reads the
//            same word (an LDS broadcast); the residual is linear in the four coordinates, so each of its two components is
//            one 4 x int8 dot product of the word with four coefficients of the hypothesis; the squares fit 24-bit multiplies;
//   argmax   the key (count << 8) | (255 - h), 0 for a hypothesis that is not admissible: the xor butterfly of a wave, the four
//            waves through LDS;
//   score    the winner's test again with thread j - 256 t owning column j, lm_block_partials / lm_fold_blocks of
//            local_match.h: the same code as the match kernels', so that a pair whose matches are all inliers reproduces their
//            score bit for bit.
// vpr_similarity_local_rerank: the match launch of local_match.hip with the match list as its extra output, this file's
// verify launch, and the order stage with the inlier counts as its payload — the composition of spatial.hip.
#include <limits.h>
#include "local_match.h"
#include "../../include/vpr_amd_similarity.h"

namespace vpr {

constexpr int SM_THREADS = 256;                                       // one thread per hypothesis and per column of a block
constexpr int SM_MAX_N = VPR_SIM_MAX_N;
constexpr int SM_MAX_SIDE = VPR_SIM_MAX_SIDE;
static_assert(VPR_SIM_MAX_N == VPR_LOCAL_HIRES_MAX_N, "the match kernels' patch limit");
static_assert(VPR_SIM_HYPOTHESES == SM_THREADS && SM_THREADS == 4 * WAVE, "thread h owns hypothesis h; four waves own a block's columns");
static_assert(SM_MAX_SIDE <= 64 && SM_MAX_SIDE * SM_MAX_SIDE >= SM_MAX_N, "a coordinate fits 6 bits: it and a difference of two fit an int8");
static_assert(SM_MAX_N < (1 << 23) / 256, "(count << 8) | (255 - h) is a positive int; h * M fits an int");
constexpr int SM_MAX_BLOCKS = (SM_MAX_N + SM_THREADS - 1) / SM_THREADS;
constexpr unsigned SM_NONE = 0xffffffffu;                             // a column without a match; every byte of a packed match is < 64

__device__ __forceinline__ unsigned sm_bytes(int a, int b, int c, int d) {
  return (unsigned)(a & 0xff) | (unsigned)(b & 0xff) << 8 | (unsigned)(c & 0xff) << 16 | (unsigned)(d & 0xff) << 24;
}

// Column j's match as one word, the bytes (g.x, g.y, q.x, q.y), or SM_NONE: decided from the partner's value alone.
__device__ __forceinline__ unsigned sm_pack(int partner, float sim, int j, int n_q, int gw_q, int gw_g) {
  if (partner < 0 || partner >= n_q || !isfinite(sim)) return SM_NONE;
  const int yq = partner / gw_q, xq = partner - yq * gw_q, yg = j / gw_g, xg = j - yg * gw_g;
  return sm_bytes(xg, yg, xq, yq);
}

// Hypothesis h of M >= 2 matches.  The residual (q - q_s) dg - dq (g - g_s) of the inlier test is linear in the match's four
// coordinates: its components are the dot products of the word's bytes with (c_re, c_im), int8 each (differences of coordinates),
// plus the products with q_s and g_s, folded into (k_re, k_im) once.  Each component is at most 5184 in magnitude.
struct SmHyp {
  int s, t, n2g, re, im, k_re, k_im;
  unsigned c_re, c_im;
  bool ok;
  __device__ __forceinline__ SmHyp(int h, int M, const unsigned* s_list) {
    s = (h * M) >> 8;
    t = (s + 1 + (97 * h) % (M - 1)) % M;
    const unsigned a = s_list[s], b = s_list[t];
    const int gsx = a & 0xff, gsy = (a >> 8) & 0xff, qsx = (a >> 16) & 0xff, qsy = a >> 24;
    const int dgx = (int)(b & 0xff) - gsx, dgy = (int)((b >> 8) & 0xff) - gsy, dqx = (int)((b >> 16) & 0xff) - qsx, dqy = (int)(b >> 24) - qsy;
    n2g = dgx * dgx + dgy * dgy;
    const int n2q = dqx * dqx + dqy * dqy;
    re = dqx * dgx + dqy * dgy;
    im = dqy * dgx - dqx * dgy;
    ok = n2g > 0 && n2q > 0 && n2g <= 4 * n2q && n2q <= 4 * n2g && re > 0 && (im < 0 ? -im : im) <= re;
    k_re = -(qsx * dgx - qsy * dgy) + (dqx * gsx - dqy * gsy);
    k_im = -(qsx * dgy + qsy * dgx) + (dqx * gsy + dqy * gsx);
    c_re = sm_bytes(-dqx, dqy, dgx, -dgy);                            // re: q.x dg.x - q.y dg.y - dq.x g.x + dq.y g.y
    c_im = sm_bytes(-dqy, -dqx, dgy, dgx);                            // im: q.x dg.y + q.y dg.x - dq.x g.y - dq.y g.x
  }
  __device__ __forceinline__ bool inlier(unsigned w, int bound) const {   // bound = tol^2 |dg|^2
    const int lre = __builtin_amdgcn_sdot4((int)w, (int)c_re, k_re, false);
    const int lim = __builtin_amdgcn_sdot4((int)w, (int)c_im, k_im, false);
    return __mul24(lre, lre) + __mul24(lim, lim) <= bound;
  }
};

// idx == nullptr: every pair is live (vpr_similarity_verify).  Every output may be null.
__global__ __launch_bounds__(SM_THREADS) void similarity_verify_kernel(
    const int32_t* __restrict__ partner, const float* __restrict__ sim, int n_q, int gw_q, int n_g, int gw_g, int tol,
    const int32_t* __restrict__ idx, int n_local, int index_base, float* __restrict__ ws_score, int32_t* __restrict__ ws_inliers,
    float* __restrict__ score, int32_t* __restrict__ inliers, int32_t* __restrict__ matches, int32_t* __restrict__ model,
    uint8_t* __restrict__ inlier_mask) {
  __shared__ unsigned s_list[SM_MAX_N];
  __shared__ int s_wcnt[SM_MAX_BLOCKS * 4];
  __shared__ int s_key[4];
  __shared__ float s_part[SM_MAX_BLOCKS * 4];
  __shared__ int s_cnt[SM_MAX_BLOCKS * 4];
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
      }
      if (model && tid < 6) model[6 * p + tid] = INT_MIN;
      return;
    }
  }
  const int32_t* pq = partner + p * n_g;
  const float* ps = sim + p * n_g;
  const int ncb = (n_g + SM_THREADS - 1) / SM_THREADS;                // <= SM_MAX_BLOCKS: n_g <= SM_MAX_N, checked on the host

  unsigned word[SM_MAX_BLOCKS];                                       // this thread's column of each block, and its rank in
  int rank[SM_MAX_BLOCKS];                                            // the wave's ballot (completed below)
#pragma unroll
  for (int t = 0; t < SM_MAX_BLOCKS; ++t) {                           // compaction: the ballots
    const int col = t * SM_THREADS + tid;
    word[t] = (t < ncb && col < n_g) ? sm_pack(pq[col], ps[col], col, n_q, gw_q, gw_g) : SM_NONE;
    const unsigned long long mask = __ballot(word[t] != SM_NONE);
    rank[t] = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[t * 4 + wave] = __popcll(mask);
  }
  __syncthreads();
  int M = 0;
#pragma unroll
  for (int t = 0; t < SM_MAX_BLOCKS; ++t) {                           // ... and the offsets of (block, wave) in column order
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave) rank[t] += M;
      M += s_wcnt[t * 4 + w];
    }
    if (word[t] != SM_NONE) s_list[rank[t]] = word[t];                // rank < M <= n_g <= SM_MAX_N
  }
  if (tid == 0) s_nmatch = M;
  __syncthreads();

  const int bound_unit = tol * tol;
  int key = 0;                                                        // hypotheses: thread tid owns hypothesis tid
  if (M >= 2) {
    const SmHyp hyp(tid, M, s_list);
    if (hyp.ok) {
      const int bound = bound_unit * hyp.n2g;
      int count = 0;
      for (int m = 0; m < M; ++m) count += hyp.inlier(s_list[m], bound) ? 1 : 0;
      key = (count << 8) | (SM_THREADS - 1 - tid);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) key = s_key[w] > key ? s_key[w] : key;
  const bool has_model = key != 0;                                    // an admissible hypothesis counts its two matches: key >= 512
  const int win = SM_THREADS - 1 - (key & 0xff);
  const SmHyp hyp(has_model ? win : 0, M >= 2 ? M : 2, s_list);       // without a model its fields are not used
  const int bound = bound_unit * hyp.n2g;

#pragma unroll
  for (int t = 0; t < SM_MAX_BLOCKS; ++t) {                           // block t: thread j - 256 t owns column j
    if (t < ncb) {
      const int col = t * SM_THREADS + tid;
      float contrib = 0.f;
      int inl = 0;
      if (col < n_g) {
        if (has_model && word[t] != SM_NONE) {
          if (hyp.inlier(word[t], bound)) { contrib = ps[col]; inl = 1; }
          if (model && rank[t] == hyp.s) model[6 * p + 1] = col;
          if (model && rank[t] == hyp.t) model[6 * p + 2] = col;
        }
        if (inlier_mask) inlier_mask[p * n_g + col] = (uint8_t)inl;
      }
      lm_block_partials(contrib, inl, t, lane, wave, s_part, s_cnt);
    }
  }
  __syncthreads();
  if (tid == 0) {
    float run;
    int c;
    lm_fold_blocks(s_part, s_cnt, ncb, run, c);                        // c = the winner's count (key >> 8)
    if (ws_score) ws_score[p] = run;
    if (ws_inliers) ws_inliers[p] = c;
    if (score) score[p] = run;
    if (inliers) inliers[p] = c;
    if (matches) matches[p] = s_nmatch;
    if (model) {
      model[6 * p] = has_model ? win : INT_MIN;
      if (!has_model) { model[6 * p + 1] = INT_MIN; model[6 * p + 2] = INT_MIN; }
      model[6 * p + 3] = has_model ? hyp.re : INT_MIN;
      model[6 * p + 4] = has_model ? hyp.im : INT_MIN;
      model[6 * p + 5] = has_model ? hyp.n2g : INT_MIN;
    }
  }
}

// gw 0 or not dividing n, tol beyond the limit, a grid side beyond the 6 bits of a coordinate; n_q, n_g >= 1 and gw, tol >= 0 here
inline int sm_check_grid(int n_q, int gw_q, int n_g, int gw_g, int tol) {
  if (gw_q == 0 || gw_q > n_q || n_q % gw_q != 0 || gw_g == 0 || gw_g > n_g || n_g % gw_g != 0) return VPR_ERR_UNSUPPORTED;
  if (tol > VPR_SIM_MAX_TOL) return VPR_ERR_UNSUPPORTED;
  if (gw_q > SM_MAX_SIDE || n_q / gw_q > SM_MAX_SIDE || gw_g > SM_MAX_SIDE || n_g / gw_g > SM_MAX_SIDE) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

inline int launch_similarity_verify(const int32_t* partner, const float* sim, long long P, int n_q, int gw_q, int n_g, int gw_g, int tol,
                                    const int32_t* idx, int n_local, int index_base, float* ws_score, int32_t* ws_inliers, float* score,
                                    int32_t* inliers, int32_t* matches, int32_t* model, uint8_t* inlier_mask, hipStream_t s) {
  return launch_kernel(similarity_verify_kernel, dim3((unsigned)P), dim3(SM_THREADS), 0, s, partner, sim, n_q, gw_q, n_g, gw_g, tol, idx,
                       n_local, index_base, ws_score, ws_inliers, score, inliers, matches, model, inlier_mask);
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_similarity_workspace_bytes(int B, int kc, int n_g) { return sv_ws_bytes(B, kc, n_g); }

extern "C" int vpr_similarity_verify(const int32_t* partner, const float* sim, int P, int n_q, int gw_q, int n_g, int gw_g, int tol,
                                     float* score, int32_t* inliers, int32_t* matches, int32_t* model, uint8_t* inlier_mask, void* stream) {
  if (!partner || !sim || !score || !inliers || !matches || !model) return VPR_ERR_INVALID_ARG;
  if (P < 0 || n_q < 0 || n_g < 0 || gw_q < 0 || gw_g < 0 || tol < 0) return VPR_ERR_INVALID_ARG;
  if (n_q == 0 || n_q > SM_MAX_N || n_g == 0 || n_g > SM_MAX_N) return VPR_ERR_UNSUPPORTED;
  VPR_TRY_LAUNCH(sm_check_grid(n_q, gw_q, n_g, gw_g, tol));
  if (!aligned4(partner) || !aligned4(sim) || !aligned4(score) || !aligned4(inliers) || !aligned4(matches) || !aligned4(model))
    return VPR_ERR_UNSUPPORTED;
  if (P == 0) return VPR_OK;
  return launch_similarity_verify(partner, sim, P, n_q, gw_q, n_g, gw_g, tol, nullptr, 0, 0, nullptr, nullptr, score, inliers, matches,
                                  model, inlier_mask, static_cast<hipStream_t>(stream));
}

extern "C" int vpr_similarity_local_rerank(const void* q_local, int n_q, const int32_t* idx, int B, int kc,
                                           const void* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                           int k_out, float* vals_out, int32_t* idx_out, int32_t* inliers_out,
                                           float* pair_score, int32_t* pair_inliers, int32_t* pair_matches, int32_t* pair_model,
                                           int32_t* row_nn, int32_t* col_nn, int feat_is_fp8, int gw_q, int gw_g, int tol,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  VPR_TRY_LAUNCH(lm_check_args(q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out, idx_out, workspace));
  if (gw_q < 0 || gw_g < 0 || tol < 0 || (feat_is_fp8 != 0 && feat_is_fp8 != 1)) return VPR_ERR_INVALID_ARG;
  VPR_TRY_LAUNCH(lm_check_shape(n_q, kc, n_g, l, feat_is_fp8 ? VPR_PATCH_FP8_MIN_L : 32, SM_MAX_N));
  VPR_TRY_LAUNCH(sm_check_grid(n_q, gw_q, n_g, gw_g, tol));
  VPR_TRY_LAUNCH(lm_check_align(q_local, idx, g_local, vals_out, idx_out, inliers_out, pair_score, pair_matches, row_nn, col_nn, workspace));
  if (!aligned4(pair_inliers) || !aligned4(pair_model)) return VPR_ERR_UNSUPPORTED;
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
  VPR_TRY_LAUNCH(launch_similarity_verify(list_q, list_sim, (long long)B * kc, n_q, gw_q, n_g, gw_g, tol, idx, n_local, index_base, ws_score,
                                          ws_count, pair_score, pair_inliers, pair_matches, pair_model, nullptr, s));
  VPR_TRY_LAUNCH(launch_local_order(ws_score, ws_count, idx, B, kc, n_local, index_base, k_out, vals_out, idx_out, inliers_out, s));
  return VPR_OK;
}
