// salad_hires.hip — stage A of the SALAD aggregation (Sinkhorn, V = F^T P^T, the three L2 normalisations) for a RUN-TIME
// patch-token count m < n <= VPR_SALAD_HIRES_MAX_N (include/vpr_amd_salad_hires.h): 448 px images are 32 x 32 = 1024 tokens,
// 518 px images 37 x 37 = 1369.
//
// sinkhorn_aggregate_n_kernel (salad_anyres.hip) keeps an image's K matrix [65][n + 1] f32 in one CU's LDS and therefore
// ends at n = 576.  At n = 1369, K is 356 KB, and so are its (hi, lo) planes: neither fits.  This kernel keeps the
// arithmetic — exp-domain iterations on K = exp(M - rowmax), then the shared back half of salad_stage_a.h (P planes,
// aggregation, normalisations, stores) — and stores NO K: it is recomputed from the image's
// score slab (n x 64 f32 = 350 KB at n = 1369, in L2 / Infinity Cache right behind the MLP stage) on every pass.
//   * thread tid owns token columns tid, tid + 256, ... (at most 6) and holds one column's 64 scores in registers at a
//     time (16 x 16-byte loads; the next column's loads fly under the current column's arithmetic);
//   * beta_j needs column j alone: no cross-thread traffic.  alpha_i needs the row sums sum_j K_ij beta_j: every thread
//     accumulates 65 partial sums over its columns in the same sweep that computes beta, and they are reduced over the
//     workgroup ONCE per sweep — through a [256][65] f32 transpose in LDS (conflict-free at the odd stride), the 64 threads
//     of a wave in fixed order (four interleaved chains), then the four waves in fixed order;
//   * passes: (1) row maxima; (2) row sums with beta = 1; (3) per iteration alpha from the row sums, one sweep for beta and
//     the next row sums; (4) the last iteration's sweep forms P instead: block by block of HR_CB = 512 columns the two bf16
//     planes [64][520] go to LDS (133,120 B, over the dead transpose area), the block's 16-token steps run on the matrix pipe
//     against features streamed as in salad_anyres.hip (chunks of four 16-token steps, FOUR chunk buffers = 128 registers
//     in flight, so that a block's 8 chunks are two turns of the buffers), barrier, next block;
//   * alpha and the row maxima live in registers, lane i of every wave holding row i's value; a column loop gets them as
//     v_readlane scalars, as the other two kernels do.  The dustbin row is constant: its K is exp(dustbin - dustbin) = 1.
// Tokens j >= n contribute exactly nothing: their scores are answered with -inf without a fetch (K = 0, P = +0 in both
// planes, 0 to every row sum) and their feature operand is 0 — the feature loads go through a buffer descriptor that spans
// feats[b] alone.  Threads without a column run the same code on such columns: there is no barrier or cross-lane exchange
// inside divergent code (only the loads are predicated).
// One workgroup per image, no atomics, no counters, no workspace: image b's output depends on image b's inputs, n, dustbin
// and iters only.
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "salad_stage_a.h"

namespace vpr {
namespace {

constexpr int HR_CB = 512;                              // token columns per P block: two per thread
constexpr int HR_PLD = HR_CB + 8;                       // row stride (bf16) of a P plane: rows of 16-byte chunks, 4 banks apart
constexpr int HR_RLD = SA_M + 1;                        // row stride (f32) of the reduction transpose: odd
// LDS: [two P planes 64 x 520 bf16 | earlier: the reduction transpose 256 x 65 f32] then wsum[4][68] | ssq[4][64] | red[8]
constexpr unsigned HR_BIG_BYTES = 2u * SA_M * HR_PLD * sizeof(uint16_t);                  // 133,120
static_assert(256u * HR_RLD * sizeof(float) <= HR_BIG_BYTES && HR_BIG_BYTES % 16 == 0, "the transpose shares the planes' LDS");
constexpr unsigned HR_LDS = HR_BIG_BYTES + (4 * 68 + 4 * SA_M + 8) * (unsigned)sizeof(float);   // 135,264 of 163,840

// Column j of the image's scores (64 consecutive f32); j >= n: -inf and no fetch.
__device__ __forceinline__ void hr_load_col(float (&c)[SA_M], const float4* __restrict__ sb4, int j, int n) {
  if (j < n) {
#pragma unroll
    for (int e = 0; e < SA_M / 4; ++e) {
      const float4 q = sb4[j * (SA_M / 4) + e];
      c[4 * e + 0] = q.x; c[4 * e + 1] = q.y; c[4 * e + 2] = q.z; c[4 * e + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < SA_M; ++i) c[i] = -INFINITY;
  }
}

// Reduction over the workgroup's 256 threads of 64 per-thread values (sum or max) and, for sums, of one more value `vd`
// (the dustbin row).  Returns row `lane`'s total in every wave; *dust receives the total of vd.  Fixed order throughout.
template <bool MAX>
__device__ __forceinline__ float hr_block_reduce(const float (&v)[SA_M], float vd, float* part, float* wsum, float* dust) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
  lds_barrier();                                   // the readers of part / wsum of the reduction before this one are done
#pragma unroll
  for (int i = 0; i < SA_M; ++i) part[tid * HR_RLD + i] = v[i];
  const float d = MAX ? 0.f : wave_sum(vd);
  lds_barrier();
  const float* col = part + (64 * wave) * HR_RLD + lane;
  float s0 = col[0], s1 = col[HR_RLD], s2 = col[2 * HR_RLD], s3 = col[3 * HR_RLD];
#pragma unroll
  for (int k = 4; k < 64; k += 4) {
    s0 = op(s0, col[(k + 0) * HR_RLD]);
    s1 = op(s1, col[(k + 1) * HR_RLD]);
    s2 = op(s2, col[(k + 2) * HR_RLD]);
    s3 = op(s3, col[(k + 3) * HR_RLD]);
  }
  wsum[wave * 68 + lane] = op(op(s0, s1), op(s2, s3));
  if (lane == 0) wsum[wave * 68 + SA_M] = d;
  lds_barrier();
  *dust = (wsum[SA_M] + wsum[68 + SA_M]) + (wsum[2 * 68 + SA_M] + wsum[3 * 68 + SA_M]);
  return op(op(wsum[lane], wsum[68 + lane]), op(wsum[2 * 68 + lane], wsum[3 * 68 + lane]));
}

// c: the column's raw scores -> K in place; returns beta_j = b_col / sum_i K_ij alpha_i (dustbin row: kd * a_d).
__device__ __forceinline__ float hr_col_beta(float (&c)[SA_M], float r_lane, float a_lane, float a_d, float kd, float b_col) {
  float s0 = kd * a_d, s1 = 0.f;                                      // two chains: half the dependent-FMA latency
#pragma unroll
  for (int i = 0; i < SA_M; i += 2) {
    c[i] = __expf(c[i] - lane_bcast(r_lane, i));
    c[i + 1] = __expf(c[i + 1] - lane_bcast(r_lane, i + 1));
    s0 = fmaf(c[i], lane_bcast(a_lane, i), s0);
    s1 = fmaf(c[i + 1], lane_bcast(a_lane, i + 1), s1);
  }
  return b_col / (s0 + s1);
}

__global__ __launch_bounds__(256, 1) void sinkhorn_aggregate_hires_kernel(
    const float* __restrict__ scores,   // [B, n, m]
    const float* __restrict__ feats,    // [B, n, l]
    const float* __restrict__ tokfeat,  // [B, t]
    int n, float dustbin, int iters, float* __restrict__ out_f32, uint16_t* __restrict__ out_bf16) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* part = reinterpret_cast<float*>(smem);             // [256][65] reduction transpose; later the two P planes
  uint16_t* Phi = reinterpret_cast<uint16_t*>(smem);        // [64][HR_PLD] bf16: hi plane of the current P block
  uint16_t* Plo = Phi + SA_M * HR_PLD;                      // lo plane: P = hi + lo to 2^-17
  float* wsum = reinterpret_cast<float*>(smem + HR_BIG_BYTES);   // [4][68] per-wave totals of a reduction
  float* ssq = wsum + 4 * 68;                               // [4][64]
  float* red = ssq + 4 * SA_M;                              // [4] (+4 pad)
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  float g = tokfeat[(long long)b * SA_T + tid];
  const float4* sb4 = reinterpret_cast<const float4*>(scores + (long long)b * n * SA_M);
  const int nq = (n + 255) >> 8;                            // columns per thread, 1 .. 6
  const float kd = __expf(dustbin - dustbin);               // K of the dustbin row: 1 for any finite dustbin

  // ---- pass 1: row maxima r_i = max_j M_ij; lane i of every wave ends with r_i ----
  float r_lane;
  {
    float mx[SA_M], ca[SA_M], cb[SA_M], unused;
#pragma unroll
    for (int i = 0; i < SA_M; ++i) mx[i] = -INFINITY;
    hr_load_col(ca, sb4, tid, n);
#pragma unroll 1
    for (int q = 0; q < nq; q += 2) {
      hr_load_col(cb, sb4, tid + 256 * (q + 1), n);
#pragma unroll
      for (int i = 0; i < SA_M; ++i) mx[i] = fmaxf(mx[i], ca[i]);
      hr_load_col(ca, sb4, tid + 256 * (q + 2), n);
#pragma unroll
      for (int i = 0; i < SA_M; ++i) mx[i] = fmaxf(mx[i], cb[i]);
    }
    r_lane = hr_block_reduce<true>(mx, 0.f, part, wsum, &unused);
  }

  // ---- Sinkhorn in the exp domain: alpha_i = a_i / sum_j K_ij beta_j, beta_j = b_j / sum_i K_ij alpha_i (beta = 1 at the
  // start).  One sweep over the thread's columns = the beta update and the row sums the next alpha needs. ----
  const StageAMarginals mg = stage_a_marginals(n);
  float a_lane = 0.f, a_d = 0.f, rs_lane, rs_d;
  auto sweep = [&](bool beta_one) {
    float acc[SA_M], accd = 0.f, ca[SA_M], cb[SA_M];
#pragma unroll
    for (int i = 0; i < SA_M; ++i) acc[i] = 0.f;
    auto column = [&](float (&c)[SA_M], int j) {
      float beta;
      if (beta_one) {                                                  // uniform
#pragma unroll
        for (int i = 0; i < SA_M; ++i) c[i] = __expf(c[i] - lane_bcast(r_lane, i));
        beta = 1.f;
      } else {
        beta = hr_col_beta(c, r_lane, a_lane, a_d, kd, mg.b_col);
      }
#pragma unroll
      for (int i = 0; i < SA_M; ++i) acc[i] = fmaf(c[i], beta, acc[i]);
      accd += j < n ? kd * beta : 0.f;                                 // a column >= n has no dustbin entry either
    };
    hr_load_col(ca, sb4, tid, n);
#pragma unroll 1
    for (int q = 0; q < nq; q += 2) {
      const int j = tid + 256 * q;
      hr_load_col(cb, sb4, j + 256, n);
      column(ca, j);
      hr_load_col(ca, sb4, j + 512, n);
      if (q + 1 < nq) column(cb, j + 256);
    }
    rs_lane = hr_block_reduce<false>(acc, accd, part, wsum, &rs_d);
  };
  sweep(true);
#pragma unroll 1
  for (int it = 0; it + 1 < iters; ++it) {
    a_lane = mg.a_reg / rs_lane;
    a_d = mg.a_dust / rs_d;
    sweep(false);
  }
  a_lane = mg.a_reg / rs_lane;
  a_d = mg.a_dust / rs_d;

  // ---- cluster features: this wave's 32 cluster dims, 64 tokens per chunk, four chunk buffers ----
  const int npad = (n + 15) & ~15, nch = (npad + 63) >> 6;            // nch >= 2: n > 64
  const int kh = lane >> 5, li = lane & 31;
  const FeatureStream fs(feats + (long long)b * n * SA_L, n, lane, wave);
  float f0[32], f1[32], f2[32], f3[32];
  fs.load_chunk(f0, 0);
  fs.load_chunk(f1, 1);
  if (2 < nch) fs.load_chunk(f2, 2);
  if (3 < nch) fs.load_chunk(f3, 3);

  // ---- the last sweep: beta, then P = K alpha beta (n + m) with the dustbin row dropped, as the two bf16 planes of one
  // block of HR_CB columns; V[l][m] += sum_j F[j][l] * P[m][j] over the block (salad_stage_a.h). ----
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
  auto planes = [&](float (&c)[SA_M], int jl) {                        // jl: the column inside the block
    const float bj = hr_col_beta(c, r_lane, a_lane, a_d, kd, mg.b_col) * mg.scale;
#pragma unroll
    for (int i = 0; i < SA_M; ++i) p_plane_entry(c[i], lane_bcast(a_lane, i), bj, Phi[i * HR_PLD + jl], Plo[i * HR_PLD + jl]);
  };
  auto mma_chunk = [&](const float (&f)[32], int c, int c0) {
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int j0 = 64 * c + 16 * st;
      if (j0 < npad) aggregate_step16(f, 8 * st, Phi, Plo, HR_PLD, j0 - c0 + 8 * kh, li, acc0, acc1);   // uniform; no step at or behind npad
    }
  };
  const int nblk = (n + HR_CB - 1) / HR_CB;                            // 1 .. 3
#pragma unroll 1
  for (int k = 0; k < nblk; ++k) {
    const int c0 = HR_CB * k;
    {
      float ca[SA_M], cb[SA_M];
      hr_load_col(ca, sb4, c0 + tid, n);
      hr_load_col(cb, sb4, c0 + 256 + tid, n);
      planes(ca, tid);                                                 // every column of the block is written: +0 at and behind n
      planes(cb, 256 + tid);
    }
    lds_barrier();
#pragma unroll
    for (int h = 0; h < 2; ++h) {        // a block is 8 chunks: two turns of the four chunk buffers, in fixed registers
      const int c = 8 * k + 4 * h;       // nothing is requested at or behind nch
      mma_chunk(f0, c, c0);
      if (c + 4 < nch) fs.load_chunk(f0, c + 4);
      mma_chunk(f1, c + 1, c0);
      if (c + 5 < nch) fs.load_chunk(f1, c + 5);
      mma_chunk(f2, c + 2, c0);
      if (c + 6 < nch) fs.load_chunk(f2, c + 6);
      mma_chunk(f3, c + 3, c0);
      if (c + 7 < nch) fs.load_chunk(f3, c + 7);
    }
    lds_barrier();                                                     // the planes are about to be rewritten
  }

  const float gden = stage_a_norms<true>(acc0, acc1, g, ssq, red);      // <true>: this kernel's bits (sum_squares16)
  stage_a_store(acc0, acc1, g, gden, b, out_f32, out_bf16);
}

}  // namespace

int launch_sinkhorn_aggregate_hires(const float* scores, const float* feats, const float* tokfeat,
                                    int B, int n, int m, int l, int t, float dustbin, int iters,
                                    float* out_f32, uint16_t* out_bf16, hipStream_t stream) {
  VPR_TRY_LAUNCH(stage_a_check(SaladDomain::HiRes, scores, feats, tokfeat, B, n, m, l, t, iters, out_f32, out_bf16));
  return launch_kernel_lds<sinkhorn_aggregate_hires_kernel>(dim3(B), dim3(256), HR_LDS, stream, scores, feats, tokfeat, n, dustbin,
                                                            iters, out_f32, out_bf16);
}

}  // namespace vpr

extern "C" int vpr_salad_sinkhorn_aggregate_hires(const float* scores, const float* feats, const float* tokfeat,
                                                  int B, int n, int m, int l, int t, float dustbin, int sinkhorn_iters,
                                                  float* out_f32, uint16_t* out_bf16, void* stream) {
  return vpr::launch_sinkhorn_aggregate_hires(scores, feats, tokfeat, B, n, m, l, t, dustbin, sinkhorn_iters, out_f32, out_bf16,
                                              static_cast<hipStream_t>(stream));
}
