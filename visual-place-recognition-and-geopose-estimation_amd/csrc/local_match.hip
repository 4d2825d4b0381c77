// local_match.hip — local-feature re-ranking: mutual-nearest-neighbour patch matching (contracts: include/vpr_amd_local.h for
// bf16 features, include/vpr_amd_patch_fp8.h for e4m3 bytes and their quantiser, include/vpr_amd_local_hires.h for up to 1369
// patches).  Two match kernels with one contract where both apply, each a template on the element (the two forms differ in the
// operand fetch, the MFMA step and one exact scale of the accumulator; everything after it — the two argmax folds, the
// reductions, the match decision, the score — is the same code), behind one launch path and one run function: the entries for
// up to 256 patches run local_match_kernel, the hires entries local_match_hires_kernel at every patch count, the call with the
// match list (spatial.hip) chooses by the patch count.  At 256 patches and below the two give the same bits; neither is the
// faster one everywhere (profiles/local_match_unify_bench.txt), which is why both are here.
// local_match_kernel (both sides <= 256 patches): a (query, group of LM_GROUP candidates) grid of 8-wave workgroups.  Liveness
// comes from the index alone: a workgroup without a live candidate ends before it loads or stages anything.  Wave w owns
// query rows 32 w .. 32 w + 31 and keeps their
// MFMA A-fragments (l / 16 bf16 ones, l / 64 e4m3 ones) in registers while the workgroup walks its candidates; each live
// candidate's features are staged once in LDS with 16-byte loads, rows padded to a multiple of 32 with zeros, chunks
// XOR-swizzled so the B-fragment ds_read_b128 of the operand map (32x32x16 bf16: one chunk per step; 32x32x64 e4m3: two) is
// conflict-free.  S is never stored: a wave forms one 32 x 32 tile of it at a time (column on the lane, rows in the 16
// registers) and folds it into
//   - a running (value, index) per register for the row argmax r(i): columns ascend per lane, so a strict > keeps the lowest
//     index; the 32 lanes of a half are reduced once per candidate with the index in the comparison;
//   - a per-lane (value, index) over the 16 registers for the column argmax c(j): the two halves are combined through lane
//     xor 32, the 8 waves through LDS in ascending wave (= row) order.
// Thread j < n_g then decides column j's match and the score is summed in the order the header states.
// local_match_hires_kernel (up to 1369 patches): described where it stands.
// order: one 128-thread workgroup per query: order_rank of vpr_common.h, the order stage of vpr_rerank_rows.
// The workspace rule, the argument checks and the score's block sum are in local_match.h, shared with spatial.hip, which also
// launches this file's match (with the match list) and order stages.
#include <float.h>
#include <math.h>
#include "local_match.h"
#include "../../include/vpr_amd_local_hires.h"

namespace vpr {

constexpr int LM_WAVES = 8;                         // = 256 / 32 row tiles of a row block
constexpr int LM_THREADS = LM_WAVES * WAVE;
constexpr int LM_GROUP = 4;                         // candidates per workgroup
constexpr int LM_MAX_N = VPR_LOCAL_MAX_N;
static_assert(LM_WAVES * 32 == LM_MAX_N && VPR_LOCAL_MAX_KC == ORDER_MAX_KC, "one wave per 32-row tile; order_rank's workgroup");

// a beats b: a exists and (b does not, or a's value is larger, or equal with the lower index)
__device__ __forceinline__ bool lm_better(float av, int ai, float bv, int bi) {
  return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi));
}

// Swizzle of the staged features: chunk c of row r (a row is CPR chunks of 16 B: L / 8 for bf16, L / 16 for e4m3) sits at
// chunk c ^ f(r) of its row, f(r) = (r >> SH) & MASK with (SH, MASK) = (0, 15) if 16 | CPR, (1, 7) if 8 | CPR, else (2, 3): the
// 16 rows of a ds_read_b128 lane group at one logical chunk fall into 16 distinct 16-byte slots of the 256-byte bank row.  CPR
// is a multiple of 4, and f(r) stays below the largest power of two (<= 16) dividing CPR: the XOR stays inside the row, and
// chunks 2 m and 2 m + 1 (the two reads of an e4m3 operand) stay a pair.  Restated and checked exhaustively on the host for
// every supported width of both elements (tests/test_local_match_fp8_cpu.py).
template <int CPR>
__device__ __forceinline__ int lm_off(int row, int chunk) {
  static_assert(CPR % 4 == 0 && CPR <= 32, "a row is a whole number of 64-byte groups");
  constexpr int SH = CPR % 16 == 0 ? 0 : CPR % 8 == 0 ? 1 : 2, MASK = CPR % 16 == 0 ? 15 : CPR % 8 == 0 ? 7 : 3;
  return (row * CPR + (chunk ^ ((row >> SH) & MASK))) << 4;
}

// LDS of one workgroup: features [ngp][L] elements of es bytes | column best value [8][ngp] f32 | column best row [8][ngp] i32 |
// row_nn [256] i32 | wave sums [4] f32 + wave counts [4] i32, ngp = n_g rounded up to 32
inline size_t lm_lds_bytes(int n_g, int l, int es) {
  const size_t ngp = (size_t)(n_g + 31) / 32 * 32;
  return ngp * l * es + 2 * LM_WAVES * ngp * 4 + LM_MAX_N * 4 + 32;
}

// Elem = uint16_t: bf16 features, S = the accumulator.  Elem = uint8_t: e4m3 bytes of x * 2^8, S = 2^-16 * the accumulator.
// The e4m3 form at l <= 128 asks for 4 waves per SIMD (<= 128 VGPRs): with its 49 KB of LDS two workgroups then share a CU.
// LIST: the match list match_q / match_sim is written as well (include/vpr_amd_spatial.h); a flag of the template, so that the
// kernels of the calls without a list are compiled without a trace of it.
template <typename Elem, int L, bool LIST>
__global__ __launch_bounds__(LM_THREADS, (sizeof(Elem) == 1 && L <= 128) ? 4 : 1) void local_match_kernel(
    const Elem* __restrict__ q_local, int n_q, const int32_t* __restrict__ idx, int kc, const Elem* __restrict__ g_local,
    int n_g, int n_local, int index_base, float min_sim, float* __restrict__ ws_score, int32_t* __restrict__ ws_matches,
    float* __restrict__ pair_score, int32_t* __restrict__ pair_matches, int32_t* __restrict__ row_nn, int32_t* __restrict__ col_nn,
    int32_t* __restrict__ match_q, float* __restrict__ match_sim) {
  constexpr bool FP8 = sizeof(Elem) == 1;
  constexpr int EPC = 16 / sizeof(Elem);                              // elements per 16-byte chunk
  constexpr int CPR = L / EPC, KS = FP8 ? L / 64 : L / 16;            // chunks per row; MFMA k-steps
  using Frag = std::conditional_t<FP8, i32x8, bf16x8>;
  extern __shared__ __attribute__((aligned(16))) char s_mem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const long long b = blockIdx.x;                                     // queries on x: the grid's y extent is 16 bits
  const int j0 = blockIdx.y * LM_GROUP;
  const int ngp = (n_g + 31) / 32 * 32, ntile = ngp / 32;
  const int nqt = (n_q + 31) / 32;                                    // row tiles that exist
  char* s_g = s_mem;
  float* s_colv = reinterpret_cast<float*>(s_mem + (size_t)ngp * L * sizeof(Elem));
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
      if constexpr (LIST) for (int i = tid; i < n_g; i += LM_THREADS) { match_q[p * n_g + i] = -1; match_sim[p * n_g + i] = 0.f; }
    }
  }
  if (!any) return;                                                   // nothing of this group is local: no loads, no staging

  // the query's A-fragments: lane holds Q[32 wave + li][16 ks + 8 h .. + 8] (bf16) or Q[32 wave + li][64 ks + 32 h .. + 32]
  // (e4m3: chunks 4 ks + 2 h and 4 ks + 2 h + 1 of its row, as the B side reads them); rows past n_q are zero
  Frag a[KS];
  {
    const int row = wave * 32 + li;
    const Elem* qrow = q_local + (b * n_q + (row < n_q ? row : 0)) * L + (FP8 ? 32 : 8) * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (FP8) {
        i32x4 lo = *reinterpret_cast<const i32x4*>(qrow + 64 * ks), hi = *reinterpret_cast<const i32x4*>(qrow + 64 * ks + 16);
        if (row >= n_q) lo = hi = i32x4{0, 0, 0, 0};
        a[ks] = e4m3_operand(lo, hi);
      } else {
        i32x4 v = *reinterpret_cast<const i32x4*>(qrow + 16 * ks);
        if (row >= n_q) v = i32x4{0, 0, 0, 0};
        a[ks] = __builtin_bit_cast(bf16x8, v);
      }
    }
  }

#pragma unroll 1
  for (int g = 0; g < LM_GROUP; ++g) {
    long long grow = 0;
    if (j0 + g >= kc || !shard_row(idx[b * kc + j0 + g], n_local, index_base, grow)) continue;      // uniform
    const long long p = b * kc + j0 + g;
    __syncthreads();                                                  // the previous candidate's LDS is no longer read
    {                                                                 // stage [n_g][L] -> LDS, rows n_g .. ngp - 1 zero
      const Elem* gimg = g_local + grow * n_g * L;                     // 0 <= grow < n_local: inside g_local
      for (int t = tid; t < ngp * CPR; t += LM_THREADS) {
        const int row = t / CPR, c = t - row * CPR;
        i32x4 v = i32x4{0, 0, 0, 0};
        if (row < n_g) v = *reinterpret_cast<const i32x4*>(gimg + (long long)row * L + EPC * c);
        *reinterpret_cast<i32x4*>(s_g + lm_off<CPR>(row, c)) = v;
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
          if constexpr (FP8) {
            const i32x4 lo = *reinterpret_cast<const i32x4*>(s_g + lm_off<CPR>(jt * 32 + li, 4 * ks + 2 * h));
            const i32x4 hi = *reinterpret_cast<const i32x4*>(s_g + lm_off<CPR>(jt * 32 + li, 4 * ks + 2 * h + 1));
            acc = mfma_e4m3_32x32x64(a[ks], e4m3_operand(lo, hi), acc);
          } else {
            const bf16x8 bf = *reinterpret_cast<const bf16x8*>(s_g + lm_off<CPR>(jt * 32 + li, 2 * ks + h));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks], bf, acc, 0, 0, 0);
          }
        }
        if constexpr (FP8) {                                          // both operands carry 2^8: exact, see the header
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] *= 0x1p-16f;
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
      if constexpr (LIST) { match_q[p * n_g + tid] = matched ? ci : -1; match_sim[p * n_g + tid] = contrib; }
    }
    if (wave < 4) lm_block_partials(contrib, matched, 0, lane, wave, s_part, s_cnt);      // columns 0 .. 255: one block
    __syncthreads();
    if (tid == 0) {
      int c = 0;
      const float s = lm_fold_block(s_part, s_cnt, 0, c);
      ws_score[p] = s;
      ws_matches[p] = c;
      if (pair_score) pair_score[p] = s;
      if (pair_matches) pair_matches[p] = c;
    }
  }
}

// ---- the kernel for up to 1369 patches per image (contract: include/vpr_amd_local_hires.h) ------------------------------
// Neither image fits where local_match_kernel keeps it (1369 x 128 bf16 = 350 KB against 160 KB of LDS; a query's A-fragments
// against one wave's registers), so one workgroup of 8 waves per (query, candidate) pair tiles both patch axes:
//   outer loop, candidate columns in chunks of CW = 256 (128 where a feature row exceeds 256 bytes): a chunk is staged once in
//     LDS (16-byte loads, the swizzle of lm_off, padded with NaN rows to a multiple of 32), so the candidate is read from HBM
//     once per pair;
//   inner loop, query rows in blocks of 256: wave w owns rows 32 w .. 32 w + 31 of the block and reads their A-fragments from
//     global memory — the query is shared by the kc workgroups of its row of the grid and stays in L2.
// S is never stored.  A wave forms one 32 x 32 tile at a time, with the instruction sequence of local_match_kernel, and folds it
//   - per register into a running (value, column) for r(i): columns ascend per lane, so a strict > keeps the lowest; the 32
//     lanes of a half are reduced once per (chunk, row block) and merged into the row's (value, index) pair in LDS, which
//     only the owning wave touches: chunks ascend, so again a strict > keeps the lowest column;
//   - per lane into a (value, row) for c(j), the halves combined through lane xor 32, then merged into the wave's own
//     [CW] slice of the chunk's column bests: a wave's rows ascend with the row block, strict > keeps the lowest.  When the
//     chunk is done, thread t folds column t's 8 slices into the persistent [n_g] column state; one wave's rows do not all lie
//     below the next wave's, so the row index is in that comparison and the fold order cannot matter.
// After the last chunk the columns are decided and summed in blocks of 256, in the order the header states.
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
// local_match_kernel.  The e4m3 form at l <= 128 fits two workgroups into a CU's LDS and needs <= 128 VGPRs for the second one;
// without the list it is compiled to exactly 128, with it the bound has to be asked for: <uint8_t, 128, true> then spills
// 20 bytes per lane to scratch, the only instantiation of this kernel with any.
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

int launch_local_order(const float* scores, const int32_t* matches, const int32_t* idx, int B, int kc, int n_local, int index_base,
                       int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out, hipStream_t stream) {
  return launch_kernel(local_order_kernel, dim3((unsigned)B), dim3(ORDER_MAX_KC), 0, stream, scores, matches, idx, kc, n_local,
                       index_base, k_out, vals_out, idx_out, matches_out);
}

// One match launch: HIRES chooses the kernel, and with it the grid and the LDS rule.  The LDS size varies per call, so the
// opt-in asks for the kernel's maximum.
template <typename Elem, int L, bool LIST, bool HIRES>
int launch_local_match(hipStream_t s, const Elem* q_local, int n_q, const int32_t* idx, int B, int kc, const Elem* g_local, int n_g,
                       int n_local, int index_base, float min_sim, float* ws_score, int32_t* ws_matches, float* pair_score,
                       int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn, int32_t* match_q, float* match_sim) {
  constexpr auto kernel = HIRES ? local_match_hires_kernel<Elem, L, LIST> : local_match_kernel<Elem, L, LIST>;
  constexpr int es = sizeof(Elem);
  const size_t most = HIRES ? lh_lds_bytes(LH_MAX_N, LH_MAX_N, L, es) : lm_lds_bytes(LM_MAX_N, L, es);
  const size_t lds = HIRES ? lh_lds_bytes(n_q, n_g, L, es) : lm_lds_bytes(n_g, L, es);
  const dim3 grid((unsigned)B, (unsigned)(HIRES ? kc : (kc + LM_GROUP - 1) / LM_GROUP));
  VPR_TRY_LAUNCH(optin_dynamic_lds<kernel>(most));
  return launch_kernel(kernel, grid, dim3(LM_THREADS), lds, s, q_local, n_q, idx, kc, g_local, n_g, n_local, index_base, min_sim,
                       ws_score, ws_matches, pair_score, pair_matches, row_nn, col_nn, match_q, match_sim);
}

// The match launch of one element type: the kernel `hires` names (false: both sides hold at most LM_MAX_N patches) for the
// width, with (LIST: match_q and match_sim non-null) or without the match list.  The arguments have passed lm_check (or the
// caller's own).
template <typename Elem, bool LIST>
int local_match_dispatch(bool hires, const Elem* q_local, int n_q, const int32_t* idx, int B, int kc, const Elem* g_local, int n_g,
                         int l, int n_local, int index_base, float min_sim, float* ws_score, int32_t* ws_matches, float* pair_score,
                         int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn, int32_t* match_q, float* match_sim, hipStream_t s) {
  constexpr bool FP8 = sizeof(Elem) == 1;
#define LM_ARGS s, q_local, n_q, idx, B, kc, g_local, n_g, n_local, index_base, min_sim, ws_score, ws_matches, pair_score, pair_matches, \
    row_nn, col_nn, match_q, match_sim
#define LM_CASE(LL) case LL: return hires ? launch_local_match<Elem, LL, LIST, true>(LM_ARGS) : launch_local_match<Elem, LL, LIST, false>(LM_ARGS);
  if constexpr (FP8) {
    switch (l) {
      LM_CASE(64) LM_CASE(128) LM_CASE(192) LM_CASE(256)
      default: return VPR_ERR_UNSUPPORTED;
    }
  } else {
    switch (l) {
      LM_CASE(32) LM_CASE(64) LM_CASE(96) LM_CASE(128) LM_CASE(160) LM_CASE(192) LM_CASE(224) LM_CASE(256)
      default: return VPR_ERR_UNSUPPORTED;
    }
  }
#undef LM_CASE
#undef LM_ARGS
}

// With the match list, the kernel goes by the patch count.
int launch_local_match_list(bool fp8, const void* q_local, int n_q, const int32_t* idx, int B, int kc, const void* g_local, int n_g,
                            int l, int n_local, int index_base, float min_sim, float* ws_score, int32_t* ws_matches, int32_t* row_nn,
                            int32_t* col_nn, int32_t* match_q, float* match_sim, hipStream_t stream) {
  const bool hires = n_q > LM_MAX_N || n_g > LM_MAX_N;
  if (fp8)
    return local_match_dispatch<uint8_t, true>(hires, static_cast<const uint8_t*>(q_local), n_q, idx, B, kc, static_cast<const uint8_t*>(g_local),
                                n_g, l, n_local, index_base, min_sim, ws_score, ws_matches, nullptr, nullptr, row_nn, col_nn, match_q, match_sim,
                                stream);
  return local_match_dispatch<uint16_t, true>(hires, static_cast<const uint16_t*>(q_local), n_q, idx, B, kc, static_cast<const uint16_t*>(g_local),
                              n_g, l, n_local, index_base, min_sim, ws_score, ws_matches, nullptr, nullptr, row_nn, col_nn, match_q, match_sim,
                              stream);
}

// The checks and the two launches of the four rerank entries; max_n = the entry's patch limit (LM_MAX_N, or LH_MAX_N for the
// hires entries, which run the hires kernel at every patch count), l_step = the width's granule (32 bf16, 64 e4m3).
template <typename Elem>
int local_rerank_run(int max_n, const Elem* q_local, int n_q, const int32_t* idx, int B, int kc, const Elem* g_local, int n_g, int l,
                     int n_local, int index_base, float min_sim, int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                     float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn, void* workspace,
                     size_t workspace_bytes, void* stream) {
  constexpr bool FP8 = sizeof(Elem) == 1;
  constexpr int l_step = FP8 ? VPR_PATCH_FP8_MIN_L : 32;
  VPR_TRY_LAUNCH(lm_check(q_local, n_q, idx, B, kc, g_local, n_g, l, l_step, max_n, n_local, index_base, min_sim, k_out, vals_out,
                          idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes));
  if (B == 0) return VPR_OK;
  float* ws_score = static_cast<float*>(workspace);
  int32_t* ws_matches = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + lm_ws_half(B, kc));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  VPR_TRY_LAUNCH((local_match_dispatch<Elem, false>(max_n > LM_MAX_N, q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim,
                                      ws_score, ws_matches, pair_score, pair_matches, row_nn, col_nn, nullptr, nullptr, s)));
  VPR_TRY_LAUNCH(launch_local_order(ws_score, ws_matches, idx, B, kc, n_local, index_base, k_out, vals_out, idx_out, matches_out, s));
  return VPR_OK;
}

// ---- the quantiser of include/vpr_amd_patch_fp8.h ---------------------------------------------------------------------
// One value -> the e4m3fn byte of x * 2^8.  The scale is exact in f32 (an overflow to +-Inf is a finite x beyond the range:
// it saturates); the clamp decides saturation, the hardware convert only ever sees |v| <= 448 and rounds once, to nearest
// even, subnormals included; fmaxf / fminf keep the sign of a zero.
__device__ __forceinline__ float pq_scaled(float x) { return fminf(fmaxf(x * 256.0f, -448.0f), 448.0f); }
__device__ __forceinline__ bool pq_nonfinite(float x) { return !(fabsf(x) <= FLT_MAX); }
__device__ __forceinline__ uint32_t pq_byte(float x) {
  const uint32_t b = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(pq_scaled(x), 0.f, 0, false) & 0xffu;
  return pq_nonfinite(x) ? 0x7fu : b;
}
// four values -> four bytes, element 0 lowest
__device__ __forceinline__ uint32_t pq_word(float x0, float x1, float x2, float x3) {
  int pk = __builtin_amdgcn_cvt_pk_fp8_f32(pq_scaled(x0), pq_scaled(x1), 0, false);
  pk = __builtin_amdgcn_cvt_pk_fp8_f32(pq_scaled(x2), pq_scaled(x3), pk, true);
  uint32_t w = (uint32_t)pk;
  if (pq_nonfinite(x0)) w = (w & 0xffffff00u) | 0x0000007fu;
  if (pq_nonfinite(x1)) w = (w & 0xffff00ffu) | 0x00007f00u;
  if (pq_nonfinite(x2)) w = (w & 0xff00ffffu) | 0x007f0000u;
  if (pq_nonfinite(x3)) w = (w & 0x00ffffffu) | 0x7f000000u;
  return w;
}
template <bool BF16>
__device__ __forceinline__ float pq_load(const void* x, long long i) {
  if constexpr (BF16) return bf16_bits_to_f32(static_cast<const uint16_t*>(x)[i]);
  else return static_cast<const float*>(x)[i];
}

constexpr int PQ_THREADS = 256;
// Elements [0, head) and [head + 16 nvec, count) one per thread; the nvec groups of 16 between them with 16-byte loads and
// one 16-byte store (the host chose head so that both x + head and out + head are 16-byte aligned, or nvec = 0).
template <bool BF16>
__global__ __launch_bounds__(PQ_THREADS) void patch_quantize_fp8_kernel(const void* __restrict__ x, long long count, long long head,
                                                                        long long nvec, uint8_t* __restrict__ out) {
  const long long t0 = (long long)blockIdx.x * PQ_THREADS + threadIdx.x, stride = (long long)gridDim.x * PQ_THREADS;
  for (long long v = t0; v < nvec; v += stride) {
    const long long e = head + 16 * v;
    uint32_t w[4];
    if constexpr (BF16) {
      const i32x4* src = reinterpret_cast<const i32x4*>(static_cast<const uint16_t*>(x) + e);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const i32x4 u = src[c];
        w[2 * c] = pq_word(bf16_lo(u[0]), bf16_hi(u[0]), bf16_lo(u[1]), bf16_hi(u[1]));
        w[2 * c + 1] = pq_word(bf16_lo(u[2]), bf16_hi(u[2]), bf16_lo(u[3]), bf16_hi(u[3]));
      }
    } else {
      const f32x4* src = reinterpret_cast<const f32x4*>(static_cast<const float*>(x) + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 u = src[c];
        w[c] = pq_word(u[0], u[1], u[2], u[3]);
      }
    }
    *reinterpret_cast<i32x4*>(out + e) = i32x4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  }
  const long long tail0 = head + 16 * nvec, nscalar = head + (count - tail0);
  for (long long t = t0; t < nscalar; t += stride) {
    const long long e = t < head ? t : tail0 + (t - head);
    out[e] = (uint8_t)pq_byte(pq_load<BF16>(x, e));
  }
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_local_workspace_bytes(int B, int kc) { return lm_ws_bytes(B, kc); }

extern "C" int vpr_local_rerank(const uint16_t* q_local, int n_q, const int32_t* idx, int B, int kc,
                                const uint16_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                                float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return local_rerank_run<uint16_t>(LM_MAX_N, q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out,
                                    idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes, stream);
}

extern "C" size_t vpr_patch_workspace_bytes_fp8(int B, int kc) { return lm_ws_bytes(B, kc); }

extern "C" int vpr_patch_rerank_fp8(const uint8_t* q_local, int n_q, const int32_t* idx, int B, int kc,
                                    const uint8_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                    int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                                    float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  return local_rerank_run<uint8_t>(LM_MAX_N, q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out,
                                   idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes, stream);
}

extern "C" size_t vpr_hires_local_workspace_bytes(int B, int kc) { return lm_ws_bytes(B, kc); }

extern "C" int vpr_hires_local_rerank(const uint16_t* q_local, int n_q, const int32_t* idx, int B, int kc,
                                      const uint16_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                      int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                                      float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return local_rerank_run<uint16_t>(LH_MAX_N, q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out,
                                    idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes, stream);
}

extern "C" int vpr_hires_patch_rerank_fp8(const uint8_t* q_local, int n_q, const int32_t* idx, int B, int kc,
                                          const uint8_t* g_local, int n_g, int l, int n_local, int index_base, float min_sim,
                                          int k_out, float* vals_out, int32_t* idx_out, int32_t* matches_out,
                                          float* pair_score, int32_t* pair_matches, int32_t* row_nn, int32_t* col_nn,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return local_rerank_run<uint8_t>(LH_MAX_N, q_local, n_q, idx, B, kc, g_local, n_g, l, n_local, index_base, min_sim, k_out, vals_out,
                                   idx_out, matches_out, pair_score, pair_matches, row_nn, col_nn, workspace, workspace_bytes, stream);
}

extern "C" int vpr_patch_quantize_fp8(const void* x, int x_is_bf16, long long count, uint8_t* out, void* stream) {
  if (!x || !out || count < 0) return VPR_ERR_INVALID_ARG;
  const size_t es = x_is_bf16 ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(x) % es != 0) return VPR_ERR_UNSUPPORTED;
  if (count == 0) return VPR_OK;
  long long head = (long long)((16 - reinterpret_cast<uintptr_t>(out) % 16) % 16);
  if (head > count) head = count;
  const bool vec = (reinterpret_cast<uintptr_t>(x) + (size_t)head * es) % 16 == 0;
  const long long nvec = vec ? (count - head) / 16 : 0;
  const long long work = nvec > count - 16 * nvec ? nvec : count - 16 * nvec;
  long long blocks = (work + PQ_THREADS - 1) / PQ_THREADS;
  if (blocks > 8192) blocks = 8192;                                   // grid-stride beyond
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (x_is_bf16) {
    VPR_TRY_LAUNCH(launch_kernel(patch_quantize_fp8_kernel<true>, dim3((unsigned)blocks), dim3(PQ_THREADS), 0, s, x, count, head, nvec, out));
  } else {
    VPR_TRY_LAUNCH(launch_kernel(patch_quantize_fp8_kernel<false>, dim3((unsigned)blocks), dim3(PQ_THREADS), 0, s, x, count, head, nvec, out));
  }
  return VPR_OK;
}
