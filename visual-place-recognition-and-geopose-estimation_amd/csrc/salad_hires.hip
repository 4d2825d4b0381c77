// salad_hires.hip — stage A of the SALAD aggregation (Sinkhorn, V = F^T P^T, the three L2 normalisations) for a RUN-TIME
// patch-token count m < n <= VPR_SALAD_HIRES_MAX_N (include/vpr_amd_salad_hires.h): 448 px images are 32 x 32 = 1024 tokens,
// 518 px images 37 x 37 = 1369.
//
// sinkhorn_aggregate_n_kernel (salad_anyres.hip) keeps an image's K matrix [65][n + 1] f32 in one CU's LDS and therefore
// ends at n = 576.  At n = 1369, K is 356 KB, and so are its (hi, lo) planes: neither fits.  This kernel keeps the
// arithmetic — exp-domain iterations on K = exp(M - rowmax), P as (hi, lo) bf16 planes, three exact-product
// v_mfma_f32_32x32x16_bf16 per 16-token step, smallest terms first — and stores NO K: it is recomputed from the image's
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

namespace vpr {
namespace {

constexpr int HR_M = SA_M, HR_L = SA_L, HR_T = SA_T;   // clusters, cluster dim, token dim (= threads per workgroup)
constexpr int HR_CB = 512;                              // token columns per P block: two per thread
constexpr int HR_PLD = HR_CB + 8;                       // row stride (bf16) of a P plane: rows of 16-byte chunks, 4 banks apart
constexpr int HR_RLD = HR_M + 1;                        // row stride (f32) of the reduction transpose: odd
// LDS: [two P planes 64 x 520 bf16 | earlier: the reduction transpose 256 x 65 f32] then wsum[4][68] | ssq[4][64] | red[8]
constexpr unsigned HR_BIG_BYTES = 2u * HR_M * HR_PLD * sizeof(uint16_t);                  // 133,120
static_assert(256u * HR_RLD * sizeof(float) <= HR_BIG_BYTES && HR_BIG_BYTES % 16 == 0, "the transpose shares the planes' LDS");
constexpr unsigned HR_LDS = HR_BIG_BYTES + (4 * 68 + 4 * HR_M + 8) * (unsigned)sizeof(float);   // 135,264 of 163,840

__device__ __forceinline__ float hr_lane_bcast(float v, int i) {      // lane i (constant) of v as a scalar operand
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i));
}

// Column j of the image's scores (64 consecutive f32); j >= n: -inf and no fetch.
__device__ __forceinline__ void hr_load_col(float (&c)[HR_M], const float4* __restrict__ sb4, int j, int n) {
  if (j < n) {
#pragma unroll
    for (int e = 0; e < HR_M / 4; ++e) {
      const float4 q = sb4[j * (HR_M / 4) + e];
      c[4 * e + 0] = q.x; c[4 * e + 1] = q.y; c[4 * e + 2] = q.z; c[4 * e + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < HR_M; ++i) c[i] = -INFINITY;
  }
}

// Reduction over the workgroup's 256 threads of 64 per-thread values (sum or max) and, for sums, of one more value `vd`
// (the dustbin row).  Returns row `lane`'s total in every wave; *dust receives the total of vd.  Fixed order throughout.
template <bool MAX>
__device__ __forceinline__ float hr_block_reduce(const float (&v)[HR_M], float vd, float* part, float* wsum, float* dust) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
  lds_barrier();                                   // the readers of part / wsum of the reduction before this one are done
#pragma unroll
  for (int i = 0; i < HR_M; ++i) part[tid * HR_RLD + i] = v[i];
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
  if (lane == 0) wsum[wave * 68 + HR_M] = d;
  lds_barrier();
  *dust = (wsum[HR_M] + wsum[68 + HR_M]) + (wsum[2 * 68 + HR_M] + wsum[3 * 68 + HR_M]);
  return op(op(wsum[lane], wsum[68 + lane]), op(wsum[2 * 68 + lane], wsum[3 * 68 + lane]));
}

__device__ __forceinline__ float hr_block_sum_256(float v, float* red) {   // wave butterflies, then the 4 wave totals in fixed order
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// c: the column's raw scores -> K in place; returns beta_j = b_col / sum_i K_ij alpha_i (dustbin row: kd * a_d).
__device__ __forceinline__ float hr_col_beta(float (&c)[HR_M], float r_lane, float a_lane, float a_d, float kd, float b_col) {
  float s0 = kd * a_d, s1 = 0.f;                                      // two chains: half the dependent-FMA latency
#pragma unroll
  for (int i = 0; i < HR_M; i += 2) {
    c[i] = __expf(c[i] - hr_lane_bcast(r_lane, i));
    c[i + 1] = __expf(c[i + 1] - hr_lane_bcast(r_lane, i + 1));
    s0 = fmaf(c[i], hr_lane_bcast(a_lane, i), s0);
    s1 = fmaf(c[i + 1], hr_lane_bcast(a_lane, i + 1), s1);
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
  uint16_t* Plo = Phi + HR_M * HR_PLD;                      // lo plane: P = hi + lo to 2^-17
  float* wsum = reinterpret_cast<float*>(smem + HR_BIG_BYTES);   // [4][68] per-wave totals of a reduction
  float* ssq = wsum + 4 * 68;                               // [4][64]
  float* red = ssq + 4 * HR_M;                              // [4] (+4 pad)
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int D_OUT = HR_T + HR_L * HR_M;

  float g = tokfeat[(long long)b * HR_T + tid];
  const float4* sb4 = reinterpret_cast<const float4*>(scores + (long long)b * n * HR_M);
  const int nq = (n + 255) >> 8;                            // columns per thread, 1 .. 6
  const float kd = __expf(dustbin - dustbin);               // K of the dustbin row: 1 for any finite dustbin

  // ---- pass 1: row maxima r_i = max_j M_ij; lane i of every wave ends with r_i ----
  float r_lane;
  {
    float mx[HR_M], ca[HR_M], cb[HR_M], unused;
#pragma unroll
    for (int i = 0; i < HR_M; ++i) mx[i] = -INFINITY;
    hr_load_col(ca, sb4, tid, n);
#pragma unroll 1
    for (int q = 0; q < nq; q += 2) {
      hr_load_col(cb, sb4, tid + 256 * (q + 1), n);
#pragma unroll
      for (int i = 0; i < HR_M; ++i) mx[i] = fmaxf(mx[i], ca[i]);
      hr_load_col(ca, sb4, tid + 256 * (q + 2), n);
#pragma unroll
      for (int i = 0; i < HR_M; ++i) mx[i] = fmaxf(mx[i], cb[i]);
    }
    r_lane = hr_block_reduce<true>(mx, 0.f, part, wsum, &unused);
  }

  // ---- Sinkhorn in the exp domain: alpha_i = a_i / sum_j K_ij beta_j, beta_j = b_j / sum_i K_ij alpha_i (beta = 1 at the
  // start).  One sweep over the thread's columns = the beta update and the row sums the next alpha needs. ----
  const float inv_nm = 1.f / (float)(n + HR_M);
  const float a_reg = inv_nm, a_dust = (float)(n - HR_M) * inv_nm, b_col = inv_nm;
  float a_lane = 0.f, a_d = 0.f, rs_lane, rs_d;
  auto sweep = [&](bool beta_one) {
    float acc[HR_M], accd = 0.f, ca[HR_M], cb[HR_M];
#pragma unroll
    for (int i = 0; i < HR_M; ++i) acc[i] = 0.f;
    auto column = [&](float (&c)[HR_M], int j) {
      float beta;
      if (beta_one) {                                                  // uniform
#pragma unroll
        for (int i = 0; i < HR_M; ++i) c[i] = __expf(c[i] - hr_lane_bcast(r_lane, i));
        beta = 1.f;
      } else {
        beta = hr_col_beta(c, r_lane, a_lane, a_d, kd, b_col);
      }
#pragma unroll
      for (int i = 0; i < HR_M; ++i) acc[i] = fmaf(c[i], beta, acc[i]);
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
    a_lane = a_reg / rs_lane;
    a_d = a_dust / rs_d;
    sweep(false);
  }
  a_lane = a_reg / rs_lane;
  a_d = a_dust / rs_d;

  // ---- cluster features: this wave's 32 cluster dims, 64 tokens per chunk (32x32x16 A-operand map: A[i = lane & 31]
  // [k = 8 * (lane >> 5) + e]); f[8 * st + e] = F[64 c + 16 st + 8 kh + e][l0 + li].  The loads go through a buffer
  // descriptor whose range is feats[b] and nothing else: for a token >= n the bounds check returns 0 and fetches nothing. ----
  const int npad = (n + 15) & ~15, nch = (npad + 63) >> 6;            // nch >= 2: n > 64
  const int l0 = 32 * wave, kh = lane >> 5, li = lane & 31;
  const auto frsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(feats + (long long)b * n * HR_L), 0,
                                                       n * HR_L * (int)sizeof(float), 0x00020000);      // wave-uniform operands only
  const int foff = (l0 + li) * (int)sizeof(float);
  auto load_chunk = [&](float (&f)[32], int c) {
    const int t0 = 64 * c + 8 * kh;
#pragma unroll
    for (int i = 0; i < 32; ++i)
      f[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                 frsrc, (t0 + 16 * (i >> 3) + (i & 7)) * (HR_L * (int)sizeof(float)) + foff, 0, 0));
  };
  float f0[32], f1[32], f2[32], f3[32];
  load_chunk(f0, 0);
  load_chunk(f1, 1);
  if (2 < nch) load_chunk(f2, 2);
  if (3 < nch) load_chunk(f3, 3);

  // ---- the last sweep: beta, then P = K alpha beta (n + m) with the dustbin row dropped, as two bf16 planes
  // (hi = bf16(P), lo = bf16(P - hi)) of one block of HR_CB columns; V[l][m] += sum_j F[j][l] * P[m][j] over the block on
  // the bf16 matrix pipe at f32 accuracy: three MFMAs (lo*hi, hi*lo, hi*hi) with exact products and f32 accumulation.
  // 32x32x16 operand maps: A[i = lane&31][k = 8*(lane>>5) + e], B[k = 8*(lane>>5) + e][j = lane&31]. ----
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
  const float scale = (float)(n + HR_M);
  auto planes = [&](float (&c)[HR_M], int jl) {                        // jl: the column inside the block
    const float bj = hr_col_beta(c, r_lane, a_lane, a_d, kd, b_col) * scale;
#pragma unroll
    for (int i = 0; i < HR_M; ++i) {
      const float pv = c[i] * hr_lane_bcast(a_lane, i) * bj;
      const __bf16 h = (__bf16)pv;
      const __bf16 l = (__bf16)(pv - (float)h);
      Phi[i * HR_PLD + jl] = __builtin_bit_cast(uint16_t, h);
      Plo[i * HR_PLD + jl] = __builtin_bit_cast(uint16_t, l);
    }
  };
  auto mma_chunk = [&](const float (&f)[32], int c, int c0) {
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int j0 = 64 * c + 16 * st;
      if (j0 < npad) {                                                 // uniform; no step at or behind npad
        bf16x8 fh, fl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          fh[e] = (__bf16)f[8 * st + e];
          fl[e] = (__bf16)(f[8 * st + e] - (float)fh[e]);
        }
        const int jj = j0 - c0 + 8 * kh;
        const bf16x8 p0h = *reinterpret_cast<const bf16x8*>(Phi + li * HR_PLD + jj);
        const bf16x8 p0l = *reinterpret_cast<const bf16x8*>(Plo + li * HR_PLD + jj);
        const bf16x8 p1h = *reinterpret_cast<const bf16x8*>(Phi + (32 + li) * HR_PLD + jj);
        const bf16x8 p1l = *reinterpret_cast<const bf16x8*>(Plo + (32 + li) * HR_PLD + jj);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, p0h, acc0, 0, 0, 0);     // smallest terms first
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, p1h, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p0l, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p1l, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p0h, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p1h, acc1, 0, 0, 0);
      }
    }
  };
  const int nblk = (n + HR_CB - 1) / HR_CB;                            // 1 .. 3
#pragma unroll 1
  for (int k = 0; k < nblk; ++k) {
    const int c0 = HR_CB * k;
    {
      float ca[HR_M], cb[HR_M];
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
      if (c + 4 < nch) load_chunk(f0, c + 4);
      mma_chunk(f1, c + 1, c0);
      if (c + 5 < nch) load_chunk(f1, c + 5);
      mma_chunk(f2, c + 2, c0);
      if (c + 6 < nch) load_chunk(f2, c + 6);
      mma_chunk(f3, c + 3, c0);
      if (c + 7 < nch) load_chunk(f3, c + 7);
    }
    lds_barrier();                                                     // the planes are about to be rewritten
  }

  // ---- per-cluster L2 norm over l (F.normalize dim=1, eps 1e-12) ----
  {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { s0 += acc0[e] * acc0[e]; s1 += acc1[e] * acc1[e]; }
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    if (lane < 32) { ssq[wave * HR_M + lane] = s0; ssq[wave * HR_M + 32 + lane] = s1; }
  }
  __syncthreads();
  const float den0 = fmaxf(sqrtf((ssq[li] + ssq[HR_M + li]) + (ssq[2 * HR_M + li] + ssq[3 * HR_M + li])), 1e-12f);
  const float den1 = fmaxf(sqrtf((ssq[32 + li] + ssq[HR_M + 32 + li]) + (ssq[2 * HR_M + 32 + li] + ssq[3 * HR_M + 32 + li])), 1e-12f);
  float psq = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = acc0[e] / den0;
    acc1[e] = acc1[e] / den1;
    psq += acc0[e] * acc0[e] + acc1[e] * acc1[e];
  }
  // ---- token vector: F.normalize(g); then the global L2 over the concatenation [g | V.flatten] ----
  const float gn = fmaxf(sqrtf(hr_block_sum_256(g * g, red)), 1e-12f);
  g = g / gn;
  const float tot = hr_block_sum_256(psq + g * g, red);
  const float gden = fmaxf(sqrtf(tot), 1e-12f);

  float* ob = out_f32 + (long long)b * D_OUT;
  uint16_t* obh = out_bf16 ? out_bf16 + (long long)b * D_OUT : nullptr;
  {
    const float o = g / gden;
    ob[tid] = o;
    if (obh) obh[tid] = f32_to_bf16_bits(o);
  }
  // C/D map of 32x32: col (cluster) = lane&31, row (l) = (e&3) + 8*(e>>2) + 4*(lane>>5)
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int l = l0 + (e & 3) + 8 * (e >> 2) + 4 * kh;
    const float o0 = acc0[e] / gden, o1 = acc1[e] / gden;
    const int base = HR_T + l * HR_M;
    ob[base + li] = o0;
    ob[base + 32 + li] = o1;
    if (obh) { obh[base + li] = f32_to_bf16_bits(o0); obh[base + 32 + li] = f32_to_bf16_bits(o1); }
  }
}

}  // namespace

int launch_sinkhorn_aggregate_hires(const float* scores, const float* feats, const float* tokfeat,
                                    int B, int n, int m, int l, int t, float dustbin, int iters,
                                    float* out_f32, uint16_t* out_bf16, hipStream_t stream) {
  if (iters < 1) return VPR_ERR_INVALID_ARG;
  if (!scores || !feats || !tokfeat || !out_f32 || B <= 0 || n < 1) return VPR_ERR_INVALID_ARG;
  if (!salad_in_domain(SaladDomain::HiRes, n, m, l, t)) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(scores) || !aligned16(feats) || !aligned4(tokfeat) || !aligned4(out_f32) || (reinterpret_cast<uintptr_t>(out_bf16) & 1))
    return VPR_ERR_UNSUPPORTED;
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
