// salad_stage_a.h — the back half of SALAD's stage A, shared by the three kernels that differ in where the Sinkhorn matrix K
// lives (salad.hip: registers, n = 256; salad_anyres.hip: LDS, 65 .. 576 tokens; salad_hires.hip: recomputed, .. 1369 tokens).
// Past the iterations all three do the same thing, and this is the one place it is written:
//   P = K alpha beta (n + m) as two bf16 planes (hi = bf16(P), lo = bf16(P - hi): P = hi + lo to 2^-17) in LDS, row = cluster;
//   V[l][m] = sum_j F[j][l] * P[m][j] on the bf16 matrix pipe at f32 accuracy: F split the same way, three
//   v_mfma_f32_32x32x16_bf16 per 16 tokens and 32-cluster block (lo*hi, hi*lo, hi*hi) with exact products and f32 accumulation
//   (the lo x lo term is 2^-34 of the product: below f32 resolution, dropped);
//   the three L2 normalisations (per cluster over l, the token vector, the concatenation [g | V.flatten]; F.normalize, eps
//   1e-12) and the 8448 outputs, f32 and optionally bf16.
// Workgroup of 256 threads; wave w owns cluster dims 32 w .. 32 w + 31 and both 32-cluster column blocks (acc0: clusters
// 0 .. 31, acc1: 32 .. 63).  32x32x16 operand maps: A[i = lane&31][k = 8*(lane>>5) + e], B[k = 8*(lane>>5) + e][j = lane&31];
// C/D: col (cluster) = lane&31, row (l) = (e&3) + 8*(e>>2) + 4*(lane>>5).
// The order and form of every floating-point expression here is part of the descriptor's bits: two-chain sums, (a + b) +
// (c + d), divisions (no reciprocals), smallest MFMA terms first.  Device code; included by the three stage-A sources only.
#pragma once
#include "vpr_common.h"
#include "vpr_internal.h"

namespace vpr {

// value of lane `i` (compile-time constant) of a wave-distributed register, as a scalar operand: v_readlane_b32
__device__ __forceinline__ float lane_bcast(float v, int i) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i));
}

// deterministic: wave butterflies, then a fixed-order sum of the 4 wave totals through red[4] (LDS)
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The marginals of the transport problem on n tokens, m clusters and the dustbin row: a_i = 1 / (n + m) for a cluster row,
// (n - m) / (n + m) for the dustbin, b_j = 1 / (n + m) per token; `scale` = n + m turns the plan back into P.
struct StageAMarginals { float a_reg, a_dust, b_col, scale; };
__device__ __forceinline__ StageAMarginals stage_a_marginals(int n) {
  const float inv_nm = 1.f / (float)(n + SA_M);
  return {inv_nm, (float)(n - SA_M) * inv_nm, inv_nm, (float)(n + SA_M)};
}

// One entry of P = K alpha beta (n + m) as its two plane values; bj = beta_j * (n + m).  hi / lo may be LDS: written once each.
__device__ __forceinline__ void p_plane_entry(float k, float alpha_i, float bj, uint16_t& hi, uint16_t& lo) {
  uint16_t h, l;
  split_hi_lo(k * alpha_i * bj, h, l);
  hi = h;
  lo = l;
}

// 16 tokens of V += F^T P^T for this wave: f[e0 .. e0 + 7] are the lane's 8 feature values (A map: cluster dim l0 + li, tokens
// 8 * (lane >> 5) + e of the step), `col` the lane's first column of the step in the planes (rows `pld` bf16 apart, 16-byte
// aligned), li = lane & 31.
template <int N>
__device__ __forceinline__ void aggregate_step16(const float (&f)[N], int e0, const uint16_t* Phi, const uint16_t* Plo, int pld,
                                                 int col, int li, f32x16& acc0, f32x16& acc1) {
  bf16x8 fh, fl;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    fh[e] = (__bf16)f[e0 + e];
    fl[e] = (__bf16)(f[e0 + e] - (float)fh[e]);
  }
  const bf16x8 p0h = *reinterpret_cast<const bf16x8*>(Phi + li * pld + col);
  const bf16x8 p0l = *reinterpret_cast<const bf16x8*>(Plo + li * pld + col);
  const bf16x8 p1h = *reinterpret_cast<const bf16x8*>(Phi + (32 + li) * pld + col);
  const bf16x8 p1l = *reinterpret_cast<const bf16x8*>(Plo + (32 + li) * pld + col);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, p0h, acc0, 0, 0, 0);     // smallest terms first
  acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, p1h, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p0l, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p1l, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p0h, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p1h, acc1, 0, 0, 0);
}

// The A operand of a run-time token count, streamed from global memory in chunks of 64 tokens (four 16-token steps):
// f[8 * st + e] = F[64 c + 16 st + 8 (lane >> 5) + e][32 wave + li].  The loads go through a buffer descriptor whose range is
// feats[b] and nothing else: for a token >= n the hardware's bounds check returns 0 and fetches nothing, without a branch per
// element (32 predicated flat loads per chunk made the compiler spill ~2 KB per lane).  How many chunk buffers are in flight
// is the caller's business.
struct FeatureStream {
  __amdgpu_buffer_rsrc_t rsrc;
  int kh, foff;         // the lane's half of a step's 16 tokens; its cluster dim in bytes
  __device__ __forceinline__ FeatureStream(const float* feats_b, int n, int lane, int wave)      // feats_b, n: wave-uniform
      : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(feats_b), 0, n * SA_L * (int)sizeof(float), 0x00020000)),
        kh(lane >> 5), foff((32 * wave + (lane & 31)) * (int)sizeof(float)) {}
  __device__ __forceinline__ void load_chunk(float (&f)[32], int c) const {
    const int t0 = 64 * c + 8 * kh;
#pragma unroll
    for (int i = 0; i < 32; ++i)
      f[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                 rsrc, (t0 + 16 * (i >> 3) + (i & 7)) * (SA_L * (int)sizeof(float)) + foff, 0, 0));
  }
};

// F.normalize's denominator from a sum of squares: max(||v||, eps)
__device__ __forceinline__ float l2_den(float sumsq) { return fmaxf(sqrtf(sumsq), 1e-12f); }

// Token vector g (one entry per thread) normalised in place, then the denominator of the global L2 over [g | V.flatten];
// `part`: this thread's sum of squares of its entries of the cluster-normalised V.  red: [4] LDS.
__device__ __forceinline__ float token_and_global_norm(float& g, float part, float* red) {
  g = g / l2_den(block_sum_256(g * g, red));
  return l2_den(block_sum_256(part + g * g, red));
}

// a[0]^2 + a[1]^2 + ... + a[15]^2 in e order, every step one fma.  The first two terms are a sum of two products, which the
// compiler contracts either way depending on the code around it, so their form is spelled out: fma(a0, a0, a1 * a1), or with
// A0_ROUNDED fma(a1, a1, a0 * a0).  The three kernels had the same source line here and not the same bits: the
// high-resolution kernel has summed its clusters 0 .. 31 the second way since it was written.
template <bool A0_ROUNDED>
__device__ __forceinline__ float sum_squares16(const f32x16& a) {
  float s = A0_ROUNDED ? fmaf(a[1], a[1], a[0] * a[0]) : fmaf(a[0], a[0], a[1] * a[1]);
#pragma unroll
  for (int e = 2; e < 16; ++e) s += a[e] * a[e];
  return s;
}

// Epilogue, first half: per-cluster L2 norm over l of the workgroup's V (acc0 / acc1 normalised in place; ssq: [4][64] LDS,
// one row per wave), F.normalize(g) in place; returns the global denominator gden.  ACC0_A0_ROUNDED: see sum_squares16; a
// kernel keeps the bits it has always produced.
template <bool ACC0_A0_ROUNDED = false>
__device__ __forceinline__ float stage_a_norms(f32x16& acc0, f32x16& acc1, float& g, float* ssq, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31;
  {
    float s0 = sum_squares16<ACC0_A0_ROUNDED>(acc0), s1 = sum_squares16<false>(acc1);
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    if (lane < 32) { ssq[wave * SA_M + lane] = s0; ssq[wave * SA_M + 32 + lane] = s1; }
  }
  __syncthreads();
  const float den0 = l2_den((ssq[li] + ssq[SA_M + li]) + (ssq[2 * SA_M + li] + ssq[3 * SA_M + li]));
  const float den1 = l2_den((ssq[32 + li] + ssq[SA_M + 32 + li]) + (ssq[2 * SA_M + 32 + li] + ssq[3 * SA_M + 32 + li]));
  float part = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = acc0[e] / den0;
    acc1[e] = acc1[e] / den1;
    part += acc0[e] * acc0[e] + acc1[e] * acc1[e];
  }
  return token_and_global_norm(g, part, red);
}

// Epilogue, second half: image b's descriptor [g | V.flatten] / gden to out_f32 and, where given, its bf16 twin.
__device__ __forceinline__ void stage_a_store(const f32x16& acc0, const f32x16& acc1, float g, float gden, int b,
                                              float* __restrict__ out_f32, uint16_t* __restrict__ out_bf16) {
  constexpr int D_OUT = SA_T + SA_L * SA_M;
  const int tid = threadIdx.x, lane = tid & 63, l0 = 32 * (tid >> 6), kh = lane >> 5, li = lane & 31;
  float* ob = out_f32 + (long long)b * D_OUT;
  uint16_t* obh = out_bf16 ? out_bf16 + (long long)b * D_OUT : nullptr;
  {
    const float o = g / gden;
    ob[tid] = o;
    if (obh) obh[tid] = f32_to_bf16_bits(o);
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int l = l0 + (e & 3) + 8 * (e >> 2) + 4 * kh;
    const float o0 = acc0[e] / gden, o1 = acc1[e] / gden;
    const int base = SA_T + l * SA_M;
    ob[base + li] = o0;
    ob[base + 32 + li] = o1;
    if (obh) { obh[base + li] = f32_to_bf16_bits(o0); obh[base + 32 + li] = f32_to_bf16_bits(o1); }
  }
}

}  // namespace vpr
