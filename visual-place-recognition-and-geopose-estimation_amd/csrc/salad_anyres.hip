// salad_anyres.hip — stage A of the SALAD aggregation (Sinkhorn, V = F^T P^T, the three L2 normalisations) for a RUN-TIME
// patch-token count m < n <= VPR_SALAD_MAX_N (include/vpr_amd_salad_anyres.h): 322 px images are 23 x 23 = 529 tokens.
//
// sinkhorn_aggregate_kernel (salad.hip) is written around n = 256: one score column per thread, the whole K matrix and all
// cluster features of a wave in registers.  This kernel keeps its arithmetic — exp-domain iterations on K = exp(M - rowmax),
// P as (hi, lo) bf16 planes over the dead score matrix, three exact-product v_mfma_f32_32x32x16_bf16 per 16-token step,
// lds_barrier() so that feature loads keep flying across the score-dependent phases — and changes where the operands live:
//   * K stays in LDS as f32 [65][ld], ld = (n + 1) | 1 (odd: the transposing stores of the staging loop and the column pass
//     are conflict-free); dynamic LDS sized from n, 153,664 B at n = 576 of the 163,840 B a workgroup may declare;
//   * row pass (row maxima, alpha): a 32-lane half-wave owns a row and walks it in strides of 32 — one LDS cycle per
//     half-wave access whatever ld is; 8 rows in flight, 9 rounds for the 65 rows; the half's sum is four DPP steps and one
//     xor-16 exchange, all inside the half, so the halves without a row in the last round simply sit it out;
//   * column pass (beta, P): thread tid owns columns tid, tid + 256, tid + 512 that are < n; alpha reaches the loop as one
//     LDS read per lane + v_readlane, as in the n = 256 kernel;
//   * P: every thread first computes its columns' packed (hi, lo) pairs into registers from K, alpha, beta; after a barrier
//     (nobody reads K any more) the planes [64][npad + 8] bf16 go over K's LDS, npad = n rounded up to 16, pad columns +0;
//   * features: wave w owns cluster dims 32 w .. 32 w + 31 and streams its A operand from global memory in chunks of four
//     16-token steps, three chunks (96 registers) in flight: the first three are requested before the Sinkhorn starts, chunk
//     c + 3 as soon as chunk c's MFMAs are issued.
// Tokens j >= n contribute exactly nothing: their P entries are +0 and their feature operand is 0 — the feature loads go
// through a buffer descriptor that spans feats[b] alone, and its bounds check answers 0 for them without fetching anything.
// Threads without a column and half-waves without a row take part in every barrier; there is no barrier or cross-half
// exchange inside divergent code.
// One workgroup per image, no atomics, no counters: image b's output depends on image b's inputs, n, dustbin and iters only.
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "../../include/vpr_amd_salad_anyres.h"

namespace vpr {
namespace {

constexpr int AN_M = SA_M, AN_L = SA_L, AN_T = SA_T;   // the kernel's names for clusters, cluster dim, token dim (= threads per workgroup)
constexpr int AN_QMAX = 18;  // score float4 per thread and staging batch: n <= 288 in one round trip, n <= 576 in two
constexpr int AN_RC = VPR_SALAD_MAX_N / 32;   // 18: row entries per lane of a half-wave
constexpr int AN_CQ = (VPR_SALAD_MAX_N + 255) / 256;   // 3: columns per thread

// LDS: [K 65 x ld f32 | later: two P planes 64 x pld bf16] then alpha[68] | ssq[4][64] | red[8] | beta[npad]
struct AnyresLds { int ld, npad, pld; unsigned small_off, total; };
__host__ __device__ inline AnyresLds anyres_lds(int n) {
  AnyresLds g;
  g.ld = (n + 1) | 1;
  g.npad = (n + 15) & ~15;
  g.pld = g.npad + 8;                    // rows of 16-byte chunks, 4 banks apart (as SA_PLD)
  const unsigned kbytes = (unsigned)(AN_M + 1) * g.ld * sizeof(float);
  const unsigned pbytes = 2u * AN_M * g.pld * sizeof(uint16_t);        // larger than K for small n
  g.small_off = ((kbytes > pbytes ? kbytes : pbytes) + 15u) / 16u * 16u;
  g.total = g.small_off + (68 + 4 * AN_M + 8 + g.npad) * (unsigned)sizeof(float);
  return g;
}

__device__ __forceinline__ float an_lane_bcast(float v, int i) {      // lane i (constant) of v as a scalar operand
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i));
}
// all-reduce over the 32 lanes of a half-wave; never leaves the half
__device__ __forceinline__ float half32_sum(float v) { v = row16_sum(v); return v + __shfl_xor(v, 16, 64); }
__device__ __forceinline__ float half32_max(float v) { v = row16_max(v); return fmaxf(v, __shfl_xor(v, 16, 64)); }

__device__ __forceinline__ float an_block_sum_256(float v, float* red) {   // wave butterflies, then the 4 wave totals in fixed order
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256, 1) void sinkhorn_aggregate_n_kernel(
    const float* __restrict__ scores,   // [B, n, m]
    const float* __restrict__ feats,    // [B, n, l]
    const float* __restrict__ tokfeat,  // [B, t]
    int n, float dustbin, int iters, float* __restrict__ out_f32, uint16_t* __restrict__ out_bf16) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AnyresLds geo = anyres_lds(n);
  const int ld = geo.ld, npad = geo.npad, pld = geo.pld;
  float* Kx = reinterpret_cast<float*>(smem);               // [65][ld] raw scores, then K; later the two P planes
  uint16_t* Phi = reinterpret_cast<uint16_t*>(smem);        // [64][pld] bf16: hi plane of P (16-byte aligned rows)
  uint16_t* Plo = Phi + AN_M * pld;                         // lo plane: P = hi + lo to 2^-17
  float* al = reinterpret_cast<float*>(smem + geo.small_off);   // [65] (+3 pad): alpha
  float* ssq = al + 68;                                     // [4][64]
  float* red = ssq + 4 * AN_M;                              // [4] (+4 pad)
  float* be = red + 8;                                      // [npad] beta
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int D_OUT = AN_T + AN_L * AN_M;

  float g = tokfeat[(long long)b * AN_T + tid];

  // ---- scores transposed into LDS: Kx[i][j] = scores[b][j][i]; up to AN_QMAX float4 per thread in flight ----
  {
    const float4* sb4 = reinterpret_cast<const float4*>(scores + (long long)b * n * AN_M);
    const int n16 = n * (AN_M / 4);
    for (int base = 0; base < n16; base += 256 * AN_QMAX) {
      float4 q[AN_QMAX];
#pragma unroll
      for (int it = 0; it < AN_QMAX; ++it) {
        const int e4 = base + tid + 256 * it;
        q[it] = e4 < n16 ? sb4[e4] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < AN_QMAX; ++it) {
        const int e4 = base + tid + 256 * it;
        if (e4 < n16) {
          const int j = e4 >> 4, i = (e4 & 15) * 4;
          Kx[(i + 0) * ld + j] = q[it].x;
          Kx[(i + 1) * ld + j] = q[it].y;
          Kx[(i + 2) * ld + j] = q[it].z;
          Kx[(i + 3) * ld + j] = q[it].w;
        }
      }
    }
  }
  for (int j = tid; j < n; j += 256) {       // dustbin row i = m; beta = 1
    Kx[AN_M * ld + j] = dustbin;
    be[j] = 1.f;
  }

  // ---- cluster features: this wave's 32 cluster dims, 64 tokens per chunk (32x32x16 A-operand map: A[i = lane & 31]
  // [k = 8 * (lane >> 5) + e]); f[8 * st + e] = F[64 c + 16 st + 8 kh + e][l0 + li].  The loads go through a buffer
  // descriptor whose range is feats[b] and nothing else: for a token >= n the hardware's bounds check returns 0 and fetches
  // nothing, without a branch per element (32 predicated flat loads per chunk made the compiler spill ~2 KB per lane). ----
  const int l0 = 32 * wave, kh = lane >> 5, li = lane & 31;
  const auto frsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(feats + (long long)b * n * AN_L), 0,
                                                       n * AN_L * (int)sizeof(float), 0x00020000);      // wave-uniform operands only
  const int foff = (l0 + li) * (int)sizeof(float);
  auto load_chunk = [&](float (&f)[32], int c) {
    const int t0 = 64 * c + 8 * kh;
#pragma unroll
    for (int i = 0; i < 32; ++i)
      f[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                 frsrc, (t0 + 16 * (i >> 3) + (i & 7)) * (AN_L * (int)sizeof(float)) + foff, 0, 0));
  };
  float f0[32], f1[32], f2[32];
  const int nch = (npad + 63) >> 6;          // >= 2: n > 64
  load_chunk(f0, 0);
  load_chunk(f1, 1);
  if (2 < nch) load_chunk(f2, 2);
  lds_barrier();

  // ---- row maxima, K = exp(M - rowmax) in place: half-wave `half` owns rows half, half + 8, ... ----
  const int half = tid >> 5, l32 = tid & 31;
#pragma unroll 1
  for (int p = 0; p < 9; ++p) {
    const int i = half + 8 * p;
    if (i <= AN_M) {                                                   // per half-wave; nothing below leaves the half
      float* row = Kx + i * ld;
      float kv[AN_RC];
#pragma unroll
      for (int c = 0; c < AN_RC; ++c) {
        const int j = l32 + 32 * c;
        kv[c] = j < n ? row[j] : -INFINITY;
      }
      float mx = kv[0];
#pragma unroll
      for (int c = 1; c < AN_RC; ++c) mx = fmaxf(mx, kv[c]);
      mx = half32_max(mx);
#pragma unroll
      for (int c = 0; c < AN_RC; ++c) {
        const int j = l32 + 32 * c;
        if (j < n) row[j] = __expf(kv[c] - mx);
      }
    }
  }
  lds_barrier();

  // ---- Sinkhorn in the exp domain: alpha_i = a_i / sum_j K_ij beta_j, beta_j = b_j / sum_i K_ij alpha_i ----
  const float inv_nm = 1.f / (float)(n + AN_M);
  const float a_reg = inv_nm, a_dust = (float)(n - AN_M) * inv_nm, b_col = inv_nm;
  for (int it = 0; it < iters; ++it) {
    {
      float bv[AN_RC];
#pragma unroll
      for (int c = 0; c < AN_RC; ++c) {
        const int j = l32 + 32 * c;
        bv[c] = j < n ? be[j] : 0.f;
      }
#pragma unroll 1
      for (int p = 0; p < 9; ++p) {
        const int i = half + 8 * p;
        if (i <= AN_M) {
          const float* row = Kx + i * ld;
          float kv[AN_RC];
#pragma unroll
          for (int c = 0; c < AN_RC; ++c) {
            const int j = l32 + 32 * c;
            kv[c] = j < n ? row[j] : 0.f;
          }
          float sx = 0.f;
#pragma unroll
          for (int c = 0; c < AN_RC; ++c) sx = fmaf(kv[c], bv[c], sx);
          sx = half32_sum(sx);
          if (l32 == 0) al[i] = (i == AN_M ? a_dust : a_reg) / sx;
        }
      }
    }
    lds_barrier();
    {
      const float a_lane = al[lane], a_d = al[AN_M];
#pragma unroll
      for (int q = 0; q < AN_CQ; ++q) {
        const int j = tid + 256 * q;
        if (j < n) {
          const float* col = Kx + j;
          float s0 = col[AN_M * ld] * a_d, s1 = 0.f;                  // two chains: half the dependent-FMA latency
#pragma unroll
          for (int i = 0; i < AN_M; i += 2) {
            s0 = fmaf(col[i * ld], an_lane_bcast(a_lane, i), s0);
            s1 = fmaf(col[(i + 1) * ld], an_lane_bcast(a_lane, i + 1), s1);
          }
          be[j] = b_col / (s0 + s1);
        }
      }
    }
    lds_barrier();
  }

  // ---- P = K alpha beta (n + m); dustbin row dropped.  Packed (hi = bf16(P), lo = bf16(P - hi)) pairs of this thread's
  // columns in registers first: the planes overwrite K, which other threads' columns still live in. ----
  {
    uint32_t pk[AN_CQ][AN_M];
    const float a_lane = al[lane];
#pragma unroll
    for (int q = 0; q < AN_CQ; ++q) {
      const int j = tid + 256 * q;
#pragma unroll
      for (int i = 0; i < AN_M; ++i) pk[q][i] = 0u;                   // pad columns: +0 in both planes
      if (j < n) {
        const float* col = Kx + j;
        const float bj = be[j] * (float)(n + AN_M);
#pragma unroll
        for (int i = 0; i < AN_M; ++i) {
          const float pv = col[i * ld] * an_lane_bcast(a_lane, i) * bj;
          const __bf16 h = (__bf16)pv;
          const __bf16 l = (__bf16)(pv - (float)h);
          pk[q][i] = (uint32_t)__builtin_bit_cast(uint16_t, h) | ((uint32_t)__builtin_bit_cast(uint16_t, l) << 16);
        }
      }
    }
    lds_barrier();                                                     // every thread is done reading K, alpha, beta
#pragma unroll
    for (int q = 0; q < AN_CQ; ++q) {
      const int j = tid + 256 * q;
      if (j < npad) {
#pragma unroll
        for (int i = 0; i < AN_M; ++i) {
          Phi[i * pld + j] = (uint16_t)(pk[q][i] & 0xffffu);
          Plo[i * pld + j] = (uint16_t)(pk[q][i] >> 16);
        }
      }
    }
  }
  lds_barrier();

  // ---- V[l][m] = sum_j F[j][l] * P[m][j] on the bf16 matrix pipe at f32 accuracy: F and P each as two bf16 terms, three
  // MFMAs (lo*hi, hi*lo, hi*hi; smallest terms first) with exact products and f32 accumulation, as in salad.hip.
  // 32x32x16 operand maps: A[i = lane&31][k = 8*(lane>>5) + e], B[k = 8*(lane>>5) + e][j = lane&31]. ----
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
  auto mma_chunk = [&](const float (&f)[32], int c) {
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int j0 = 64 * c + 16 * st;
      if (j0 < npad) {                                                 // uniform; the planes end at column npad
        bf16x8 fh, fl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          fh[e] = (__bf16)f[8 * st + e];
          fl[e] = (__bf16)(f[8 * st + e] - (float)fh[e]);
        }
        const int jj = j0 + 8 * kh;
        const bf16x8 p0h = *reinterpret_cast<const bf16x8*>(Phi + li * pld + jj);
        const bf16x8 p0l = *reinterpret_cast<const bf16x8*>(Plo + li * pld + jj);
        const bf16x8 p1h = *reinterpret_cast<const bf16x8*>(Phi + (32 + li) * pld + jj);
        const bf16x8 p1l = *reinterpret_cast<const bf16x8*>(Plo + (32 + li) * pld + jj);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, p0h, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, p1h, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p0l, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p1l, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p0h, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, p1h, acc1, 0, 0, 0);
      }
    }
  };
#pragma unroll 1
  for (int c = 0; c < nch; c += 3) {       // three chunk buffers in fixed registers; nothing is requested at or behind nch
    mma_chunk(f0, c);
    if (c + 3 < nch) load_chunk(f0, c + 3);
    mma_chunk(f1, c + 1);
    if (c + 4 < nch) load_chunk(f1, c + 4);
    mma_chunk(f2, c + 2);
    if (c + 5 < nch) load_chunk(f2, c + 5);
  }

  // ---- per-cluster L2 norm over l (F.normalize dim=1, eps 1e-12) ----
  {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { s0 += acc0[e] * acc0[e]; s1 += acc1[e] * acc1[e]; }
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    if (lane < 32) { ssq[wave * AN_M + lane] = s0; ssq[wave * AN_M + 32 + lane] = s1; }
  }
  __syncthreads();
  const float den0 = fmaxf(sqrtf((ssq[li] + ssq[AN_M + li]) + (ssq[2 * AN_M + li] + ssq[3 * AN_M + li])), 1e-12f);
  const float den1 = fmaxf(sqrtf((ssq[32 + li] + ssq[AN_M + 32 + li]) + (ssq[2 * AN_M + 32 + li] + ssq[3 * AN_M + 32 + li])), 1e-12f);
  float part = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = acc0[e] / den0;
    acc1[e] = acc1[e] / den1;
    part += acc0[e] * acc0[e] + acc1[e] * acc1[e];
  }
  // ---- token vector: F.normalize(g); then the global L2 over the concatenation [g | V.flatten] ----
  const float gn = fmaxf(sqrtf(an_block_sum_256(g * g, red)), 1e-12f);
  g = g / gn;
  const float tot = an_block_sum_256(part + g * g, red);
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
    const int base = AN_T + l * AN_M;
    ob[base + li] = o0;
    ob[base + 32 + li] = o1;
    if (obh) { obh[base + li] = f32_to_bf16_bits(o0); obh[base + 32 + li] = f32_to_bf16_bits(o1); }
  }
}

}  // namespace

int launch_sinkhorn_aggregate_n(const float* scores, const float* feats, const float* tokfeat,
                                int B, int n, int m, int l, int t, float dustbin, int iters,
                                float* out_f32, uint16_t* out_bf16, hipStream_t stream) {
  if (!scores || !feats || !tokfeat || !out_f32 || B <= 0 || n < 1 || iters < 1) return VPR_ERR_INVALID_ARG;
  if (!salad_in_domain(SaladDomain::AnyN, n, m, l, t)) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(scores) || !aligned16(feats) || !aligned4(tokfeat) || !aligned4(out_f32) || (reinterpret_cast<uintptr_t>(out_bf16) & 1))
    return VPR_ERR_UNSUPPORTED;
  // the opt-in once per device, for the largest n (smaller n then needs no second call)
  VPR_TRY_LAUNCH(optin_dynamic_lds<sinkhorn_aggregate_n_kernel>(anyres_lds(VPR_SALAD_MAX_N).total));
  return launch_kernel(sinkhorn_aggregate_n_kernel, dim3(B), dim3(256), anyres_lds(n).total, stream, scores, feats, tokfeat, n,
                       dustbin, iters, out_f32, out_bf16);
}

}  // namespace vpr

extern "C" int vpr_salad_sinkhorn_aggregate_n(const float* scores, const float* feats, const float* tokfeat,
                                              int B, int n, int m, int l, int t, float dustbin, int sinkhorn_iters,
                                              float* out_f32, uint16_t* out_bf16, void* stream) {
  return vpr::launch_sinkhorn_aggregate_n(scores, feats, tokfeat, B, n, m, l, t, dustbin, sinkhorn_iters, out_f32, out_bf16,
                                          static_cast<hipStream_t>(stream));
}
