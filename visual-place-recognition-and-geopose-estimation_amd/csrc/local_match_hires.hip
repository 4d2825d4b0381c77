// local_match_hires.hip — local-feature re-ranking for up to 1369 patches per image (contract: include/vpr_amd_local_hires.h).
// The pieces shared with the 256-patch kernel are in local_match.h; the order stage is that kernel's.
// Neither image fits where local_match.hip keeps it (1369 x 128 bf16 = 350 KB against 160 KB of LDS; a query's A-fragments
// against one wave's registers), so one workgroup of 8 waves per (query, candidate) pair tiles both patch axes:
//   outer loop, candidate columns in chunks of CW = 256 (128 where a feature row exceeds 256 bytes): a chunk is staged once in
//     LDS (16-byte loads, the swizzle of lm_off, padded with NaN rows to a multiple of 32), so the candidate is read from HBM
//     once per pair;
//   inner loop, query rows in blocks of 256: wave w owns rows 32 w .. 32 w + 31 of the block and reads their A-fragments from
//     global memory — the query is shared by the kc workgroups of its row of the grid and stays in L2.
// S is never stored.  A wave forms one 32 x 32 tile at a time, with the instruction sequence of local_match.hip, and folds it
//   - per register into a running (value, column) for r(i): columns ascend per lane, so a strict > keeps the lowest; the 32
//     lanes of a half are reduced once per (chunk, row block) and merged into the row's (value, index) pair in LDS, which
//     only the owning wave touches: chunks ascend, so again a strict > keeps the lowest column;
//   - per lane into a (value, row) for c(j), the halves combined through lane xor 32, then merged into the wave's own
//     [CW] slice of the chunk's column bests: a wave's rows ascend with the row block, strict > keeps the lowest.  When the
//     chunk is done, thread t folds column t's 8 slices into the persistent [n_g] column state; one wave's rows do not all lie
//     below the next wave's, so the row index is in that comparison and the fold order cannot matter.
// After the last chunk the columns are decided and summed in blocks of 256, in the order the header states.
#include <float.h>
#include <math.h>
#include "local_match.h"
#include "../../include/vpr_amd_local_hires.h"

namespace vpr {

constexpr int LH_MAX_N = VPR_LOCAL_HIRES_MAX_N;
constexpr int LH_BLOCK = 256;                                         // rows of a row block; columns of a block of the score sum
constexpr int LH_MAX_BLOCKS = (LH_MAX_N + LH_BLOCK - 1) / LH_BLOCK;   // 6
static_assert(LM_WAVES * 32 == LH_BLOCK && LH_BLOCK <= LM_THREADS, "one wave per 32-row tile of a block; one thread per column of one");

// columns of a chunk: a chunk is at most 64 KB for every (element, l)
constexpr int lh_chunk_cols(int row_bytes) { return row_bytes <= 256 ? 256 : 128; }

// LDS of one workgroup: chunk [CW][L] elements | per-wave column best value [8][CW] f32 | row [8][CW] i32 | column state
// value [ngp] f32 | row [ngp] i32 | row state value [nqp] f32 | column [nqp] i32 | block wave sums [6][4] f32 | counts [6][4]
// i32; ngp = n_g rounded up to 32, nqp = n_q rounded up to 256.  Every carve is a multiple of 16 bytes.
inline size_t lh_lds_bytes(int n_q, int n_g, int l, int es) {
  const size_t cw = lh_chunk_cols(l * es), ngp = (size_t)(n_g + 31) / 32 * 32, nqp = (size_t)(n_q + LH_BLOCK - 1) / LH_BLOCK * LH_BLOCK;
  return cw * l * es + 2 * LM_WAVES * cw * 4 + 8 * (ngp + nqp) + 2 * LH_MAX_BLOCKS * 4 * 4;
}

// LIST: the match list match_q / match_sim is written as well (include/vpr_amd_spatial.h); a flag of the template, as in
// local_match.hip.  The e4m3 form at l <= 128 fits two workgroups into a CU's LDS and needs <= 128 VGPRs for the second one;
// without the list it is compiled to exactly 128, with it the bound has to be asked for.
template <typename Elem, int L, bool LIST>
__global__ __launch_bounds__(LM_THREADS, (LIST && sizeof(Elem) == 1 && L <= 128) ? 4 : 1) void local_match_hires_kernel(
    const Elem* __restrict__ q_local, int n_q, const int32_t* __restrict__ idx, int kc, const Elem* __restrict__ g_local,
    int n_g, int n_local, int index_base, float min_sim, float* __restrict__ ws_score, int32_t* __restrict__ ws_matches,
    float* __restrict__ pair_score, int32_t* __restrict__ pair_matches, int32_t* __restrict__ row_nn, int32_t* __restrict__ col_nn,
    int32_t* __restrict__ match_q, float* __restrict__ match_sim) {
  constexpr bool FP8 = sizeof(Elem) == 1;
  constexpr int EPC = 16 / sizeof(Elem);                              // elements per 16-byte chunk
  constexpr int CPR = L / EPC, KS = FP8 ? L / 64 : L / 16;            // 16-byte chunks per row; MFMA k-steps
  constexpr int CW = lh_chunk_cols(L * sizeof(Elem));
  constexpr int NST = CW * CPR / LM_THREADS;                          // 16-byte pieces of a chunk per thread: 2 .. 8
  static_assert(NST * LM_THREADS == CW * CPR, "a chunk is a whole number of 16-byte pieces per thread");
  using Frag = std::conditional_t<FP8, i32x8, bf16x8>;
  // Padding (query rows past n_q, candidate columns past n_g, up to the tile of 32) holds NaN elements, not zeros: every S it
  // enters is then non-finite, "no similarity", and the test that the contract asks for anyway masks it out of both argmaxes
  constexpr int NAN_WORD = FP8 ? 0x7f7f7f7f : 0x7fc07fc0;
  const i32x4 pad = i32x4{NAN_WORD, NAN_WORD, NAN_WORD, NAN_WORD};
  extern __shared__ __attribute__((aligned(16))) char s_mem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const long long b = blockIdx.x;                                     // queries on x: the grid's y extent is 16 bits
  const int j = blockIdx.y;
  const long long p = b * kc + j;
  const int ngp = (n_g + 31) / 32 * 32, nqp = (n_q + LH_BLOCK - 1) / LH_BLOCK * LH_BLOCK;
  const int nrb = nqp / LH_BLOCK, ncb = (n_g + LH_BLOCK - 1) / LH_BLOCK;
  const int nw = n_q >= LH_BLOCK ? LM_WAVES : (n_q + 31) / 32;        // waves that own a row of the first row block
  char* s_g = s_mem;
  float* s_colv = reinterpret_cast<float*>(s_mem + (size_t)CW * L * sizeof(Elem));
  int* s_coli = reinterpret_cast<int*>(s_colv + LM_WAVES * CW);
  float* s_cv = reinterpret_cast<float*>(s_coli + LM_WAVES * CW);
  int* s_ci = reinterpret_cast<int*>(s_cv + ngp);
  float* s_rowv = reinterpret_cast<float*>(s_ci + ngp);
  int* s_rowi = reinterpret_cast<int*>(s_rowv + nqp);
  float* s_part = reinterpret_cast<float*>(s_rowi + nqp);
  int* s_cnt = reinterpret_cast<int*>(s_part + LH_MAX_BLOCKS * 4);

  // liveness, from the index alone; the optional per-pair outputs of a non-live candidate
  long long grow = 0;
  if (!shard_row(idx[p], n_local, index_base, grow)) {                // workgroup-uniform
    if (pair_score && tid == 0) pair_score[p] = -INFINITY;
    if (pair_matches && tid == 0) pair_matches[p] = 0;
    if (row_nn) for (int i = tid; i < n_q; i += LM_THREADS) row_nn[p * n_q + i] = -1;
    if (col_nn) for (int i = tid; i < n_g; i += LM_THREADS) col_nn[p * n_g + i] = -1;
    if constexpr (LIST) for (int i = tid; i < n_g; i += LM_THREADS) { match_q[p * n_g + i] = -1; match_sim[p * n_g + i] = 0.f; }
    return;                                                           // not local: no loads, no staging
  }
  const Elem* gimg = g_local + grow * n_g * L;                        // 0 <= grow < n_local: inside g_local
  const Elem* qimg = q_local + b * n_q * L;

#pragma unroll 1
  for (int c0 = 0; c0 < n_g; c0 += CW) {
    const int cn = n_g - c0 < CW ? n_g - c0 : CW;                     // columns of this chunk
    const int cnp = (cn + 31) / 32 * 32, ntile = cnp / 32;
    __syncthreads();                                                  // the previous chunk is no longer read, its bests are folded
    {                                                                 // stage [cn][L] -> LDS, rows cn .. cnp - 1 NaN:
      i32x4 v[NST];                                                   // every load of the thread is issued before the first wait
#pragma unroll
      for (int u = 0; u < NST; ++u) {
        const int t = tid + u * LM_THREADS, row = t / CPR, c = t - row * CPR;
        const i32x4 ld = *reinterpret_cast<const i32x4*>(gimg + (long long)(c0 + (row < cn ? row : 0)) * L + EPC * c);   // inside the image
        v[u] = row < cn ? ld : pad;
      }
#pragma unroll
      for (int u = 0; u < NST; ++u) {
        const int t = tid + u * LM_THREADS, row = t / CPR, c = t - row * CPR;
        if (row < cnp) *reinterpret_cast<i32x4*>(s_g + lm_off<CPR>(row, c)) = v[u];
      }
    }
    __syncthreads();

#pragma unroll 1
    for (int rb = 0; rb < nrb; ++rb) {
      const int row0 = rb * LH_BLOCK + wave * 32;
      if (row0 >= n_q) break;                                         // wave-uniform; no barrier inside this loop
      // the A-fragments of rows row0 .. row0 + 31: lane holds Q[row0 + li][16 ks + 8 h .. + 8] (bf16) or
      // Q[row0 + li][64 ks + 32 h .. + 32] (e4m3), as the B side reads its operand; rows past n_q are NaN
      Frag a[KS];
      {
        const int row = row0 + li;
        const Elem* qrow = qimg + (long long)(row < n_q ? row : 0) * L + (FP8 ? 32 : 8) * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          if constexpr (FP8) {
            i32x4 lo = *reinterpret_cast<const i32x4*>(qrow + 64 * ks), hi = *reinterpret_cast<const i32x4*>(qrow + 64 * ks + 16);
            if (row >= n_q) lo = hi = pad;
            a[ks] = e4m3_operand(lo, hi);
          } else {
            i32x4 v = *reinterpret_cast<const i32x4*>(qrow + 16 * ks);
            if (row >= n_q) v = pad;
            a[ks] = __builtin_bit_cast(bf16x8, v);
          }
        }
      }
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
          if constexpr (FP8) {
            const i32x4 lo = *reinterpret_cast<const i32x4*>(s_g + lm_off<CPR>(jt * 32 + li, 4 * ks + 2 * h));
            const i32x4 hi = *reinterpret_cast<const i32x4*>(s_g + lm_off<CPR>(jt * 32 + li, 4 * ks + 2 * h + 1));
            acc = mfma_e4m3_32x32x64(a[ks], e4m3_operand(lo, hi), acc);
          } else {
            const bf16x8 bf = *reinterpret_cast<const bf16x8*>(s_g + lm_off<CPR>(jt * 32 + li, 2 * ks + h));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks], bf, acc, 0, 0, 0);
          }
        }
        if constexpr (FP8) {                                          // both operands carry 2^8: exact, see vpr_amd_patch_fp8.h
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] *= 0x1p-16f;
        }
        // acc[r] = S[row0 + (r & 3) + 8 (r >> 2) + 4 h][c0 + 32 jt + li]
        const int lcol = jt * 32 + li, col = c0 + lcol;
        float cv = -INFINITY;
        int ci = -1;
        // branch-free: what does not count (a non-finite S, padding included) becomes -inf, which no strict > accepts; a running
        // best without an index is -inf, which every finite S beats, so the index needs no test of its own
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float v = isfinite(acc[r]) ? acc[r] : -INFINITY;
          const bool br = v > rbv[r];                                 // columns ascend per lane
          rbv[r] = br ? v : rbv[r];
          rbi[r] = br ? col : rbi[r];
          const bool bc = v > cv;                                     // rows ascend with r
          cv = bc ? v : cv;
          ci = bc ? row : ci;
        }
        {                                                             // the other half's rows interleave with this one's
          const float ov = __shfl_xor(cv, 32, 64);
          const int oi = __shfl_xor(ci, 32, 64);
          if (lm_better(ov, oi, cv, ci)) { cv = ov; ci = oi; }
        }
        if (h == 0) {                                                 // this wave's slice: its earlier row blocks lie below
          float* sv = s_colv + wave * CW + lcol;
          int* si = s_coli + wave * CW + lcol;
          if (rb == 0 || (ci >= 0 && (*si < 0 || cv > *sv))) { *sv = cv; *si = ci; }
        }
      }
      // r(i): reduce the 32 lanes of each half, then merge into the row's state: earlier chunks hold lower columns
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
        const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (li == 0 && row < n_q && (c0 == 0 || (i >= 0 && (s_rowi[row] < 0 || v > s_rowv[row])))) { s_rowv[row] = v; s_rowi[row] = i; }
      }
    }
    __syncthreads();
    if (tid < cn) {                                                   // c(j) of this chunk's columns, complete: all rows were seen
      float cv = -INFINITY;
      int ci = -1;
      for (int w = 0; w < nw; ++w) {
        const float v = s_colv[w * CW + tid];
        const int i = s_coli[w * CW + tid];
        if (lm_better(v, i, cv, ci)) { cv = v; ci = i; }
      }
      s_cv[c0 + tid] = cv;
      s_ci[c0 + tid] = ci;
    }
  }
  __syncthreads();                                                    // r(i) and c(j) are complete

  if (row_nn) for (int i = tid; i < n_q; i += LM_THREADS) row_nn[p * n_q + i] = s_rowi[i];
  // block t: thread j - 256 t owns column j: the match, the block's sum in the order of vpr_amd_local.h
  if (wave < 4) {
    for (int t = 0; t < ncb; ++t) {
      const int col = t * LH_BLOCK + tid;
      float contrib = 0.f;
      int matched = 0;
      if (col < n_g) {
        const float cv = s_cv[col];
        const int ci = s_ci[col];
        if (col_nn) col_nn[p * n_g + col] = ci;
        if (ci >= 0 && s_rowi[ci] == col && cv >= min_sim) { contrib = cv; matched = 1; }
        if constexpr (LIST) { match_q[p * n_g + col] = matched ? ci : -1; match_sim[p * n_g + col] = contrib; }
      }
      lm_block_partials(contrib, matched, t, lane, wave, s_part, s_cnt);
    }
  }
  __syncthreads();
  if (tid == 0) {
    float run;
    int c;
    lm_fold_blocks(s_part, s_cnt, ncb, run, c);
    ws_score[p] = run;
    ws_matches[p] = c;
    if (pair_score) pair_score[p] = run;
    if (pair_matches) pair_matches[p] = c;
  }
}

template <typename Elem, int L, bool LIST>
int launch_local_match_hires(dim3 grid, size_t lds, hipStream_t s, const Elem* q_local, int n_q, const int32_t* idx, int kc,
                             const Elem* g_local, int n_g, int n_local, int index_base, float min_sim, float* ws_score,
                             int32_t* ws_matches, float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                             int32_t* match_q, float* match_sim) {
  VPR_TRY_LAUNCH((optin_dynamic_lds<local_match_hires_kernel<Elem, L, LIST>>(lh_lds_bytes(LH_MAX_N, LH_MAX_N, L, sizeof(Elem)))));   // the LDS size varies per call: the maximum
  return launch_kernel(local_match_hires_kernel<Elem, L, LIST>, grid, dim3(LM_THREADS), lds, s, q_local, n_q, idx, kc, g_local, n_g,
                       n_local, index_base, min_sim, ws_score, ws_matches, pair_score, pair_matches, row_nn, col_nn, match_q, match_sim);
}

// The match launch of one element type: the kernel for the width, with (LIST: match_q and match_sim non-null) or without the
// match list.  The arguments have passed lm_check (or the caller's own).
template <typename Elem, bool LIST>
int local_match_hires_dispatch(const Elem* q_local, int n_q, const int32_t* idx, int B, int kc, const Elem* g_local, int n_g, int l,
                               int n_local, int index_base, float min_sim, float* ws_score, int32_t* ws_matches, float* pair_score,
                               int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn, int32_t* match_q, float* match_sim,
                               hipStream_t s) {
  constexpr bool FP8 = sizeof(Elem) == 1;
  const dim3 grid((unsigned)B, (unsigned)kc);
  const size_t lds = lh_lds_bytes(n_q, n_g, l, sizeof(Elem));
#define LH_CASE(LL) case LL: return launch_local_match_hires<Elem, LL, LIST>(grid, lds, s, q_local, n_q, idx, kc, g_local, n_g, n_local, \
    index_base, min_sim, ws_score, ws_matches, pair_score, pair_matches, row_nn, col_nn, match_q, match_sim);
  if constexpr (FP8) {
    switch (l) {
      LH_CASE(64) LH_CASE(128) LH_CASE(192) LH_CASE(256)
      default: return VPR_ERR_UNSUPPORTED;
    }
  } else {
    switch (l) {
      LH_CASE(32) LH_CASE(64) LH_CASE(96) LH_CASE(128) LH_CASE(160) LH_CASE(192) LH_CASE(224) LH_CASE(256)
      default: return VPR_ERR_UNSUPPORTED;
    }
  }
#undef LH_CASE
}

int launch_local_match_hires_list(bool fp8, const void* q_local, int n_q, const int32_t* idx, int B, int kc, const void* g_local,
                                  int n_g, int l, int n_local, int index_base, float min_sim, float* ws_score, int32_t* ws_matches,
                                  int32_t* row_nn, int32_t* col_nn, int32_t* match_q, float* match_sim, hipStream_t stream) {
  if (fp8)
    return local_match_hires_dispatch<uint8_t, true>(static_cast<const uint8_t*>(q_local), n_q, idx, B, kc, static_cast<const uint8_t*>(g_local), n_g,
                                      l, n_local, index_base, min_sim, ws_score, ws_matches, nullptr, nullptr, row_nn, col_nn, match_q,
                                      match_sim, stream);
  return local_match_hires_dispatch<uint16_t, true>(static_cast<const uint16_t*>(q_local), n_q, idx, B, kc, static_cast<const uint16_t*>(g_local), n_g,
                                    l, n_local, index_base, min_sim, ws_score, ws_matches, nullptr, nullptr, row_nn, col_nn, match_q,
                                    match_sim, stream);
}

// The checks and the two launches of both element types.
template <typename Elem>
int local_rerank_hires_run(const Elem* q_local, int n_q, const int32_t* idx, int B, int kc, const Elem* g_local, int n_g, int l,
                           int n_local, int index_base, float min_sim, int k_out, float* vals_out, int32_t* idx_out,
                           int32_t* matches_out, float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                           void* workspace, size_t workspace_bytes, void* stream) {
  constexpr bool FP8 = sizeof(Elem) == 1;
  constexpr int l_step = FP8 ? VPR_PATCH_FP8_MIN_L : 32;
  VPR_TRY_LAUNCH(lm_check(q_local, n_q, idx, B, kc, g_local, n_g, l, l_step, LH_MAX_N, n_local, index_base, min_sim, k_out, vals_out,
                          idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes));
  if (B == 0) return VPR_OK;
  float* ws_score = static_cast<float*>(workspace);
  int32_t* ws_matches = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + lm_ws_half(B, kc));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  VPR_TRY_LAUNCH((local_match_hires_dispatch<Elem, false>(q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, ws_score,
                                            ws_matches, pair_score, pair_matches, row_nn, col_nn, nullptr, nullptr, s)));
  VPR_TRY_LAUNCH(launch_local_order(ws_score, ws_matches, idx, B, kc, n_local, index_base, k_out, vals_out, idx_out, matches_out, s));
  return VPR_OK;
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_hires_local_workspace_bytes(int B, int kc) { return lm_ws_bytes(B, kc); }

extern "C" int vpr_hires_local_rerank(const uint16_t* q_local, int n_q, const int32_t* idx, int B, int kc,
                                      const uint16_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                      int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                                      float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return local_rerank_hires_run<uint16_t>(q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out,
                                          idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes, stream);
}

extern "C" int vpr_hires_patch_rerank_fp8(const uint8_t* q_local, int n_q, const int32_t* idx, int B, int kc,
                                          const uint8_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                          int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                                          float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return local_rerank_hires_run<uint8_t>(q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out,
                                         idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes, stream);
}
