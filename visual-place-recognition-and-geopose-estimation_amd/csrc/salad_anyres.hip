// salad_anyres.hip — stage A of the SALAD aggregation (Sinkhorn, V = F^T P^T, the three L2 normalisations) for a RUN-TIME
// patch-token count m < n <= VPR_SALAD_MAX_N (include/vpr_amd_salad_anyres.h): 322 px images are 23 x 23 = 529 tokens.
//
// sinkhorn_aggregate_kernel (salad.hip) is written around n = 256: one score column per thread, the whole K matrix and all
// cluster features of a wave in registers.  This kernel keeps its arithmetic — exp-domain iterations on K = exp(M - rowmax),
// the shared back half of salad_stage_a.h (P planes over the dead score matrix, aggregation, normalisations, stores),
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
#include "salad_stage_a.h"
#include "../../include/vpr_amd_salad_anyres.h"

namespace vpr {
namespace {

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
  const unsigned kbytes = (unsigned)(SA_M + 1) * g.ld * sizeof(float);
  const unsigned pbytes = 2u * SA_M * g.pld * sizeof(uint16_t);        // larger than K for small n
  g.small_off = ((kbytes > pbytes ? kbytes : pbytes) + 15u) / 16u * 16u;
  g.total = g.small_off + (68 + 4 * SA_M + 8 + g.npad) * (unsigned)sizeof(float);
  return g;
}

// all-reduce over the 32 lanes of a half-wave; never leaves the half
__device__ __forceinline__ float half32_sum(float v) { v = row16_sum(v); return v + __shfl_xor(v, 16, 64); }
__device__ __forceinline__ float half32_max(float v) { v = row16_max(v); return fmaxf(v, __shfl_xor(v, 16, 64)); }

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
  uint16_t* Plo = Phi + SA_M * pld;                         // lo plane: P = hi + lo to 2^-17
  float* al = reinterpret_cast<float*>(smem + geo.small_off);   // [65] (+3 pad): alpha
  float* ssq = al + 68;                                     // [4][64]
  float* red = ssq + 4 * SA_M;                              // [4] (+4 pad)
  float* be = red + 8;                                      // [npad] beta
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  float g = tokfeat[(long long)b * SA_T + tid];

  // ---- scores transposed into LDS: Kx[i][j] = scores[b][j][i]; up to AN_QMAX float4 per thread in flight ----
  {
    const float4* sb4 = reinterpret_cast<const float4*>(scores + (long long)b * n * SA_M);
    const int n16 = n * (SA_M / 4);
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
    Kx[SA_M * ld + j] = dustbin;
    be[j] = 1.f;
  }

  // ---- cluster features: this wave's 32 cluster dims, 64 tokens per chunk, three chunk buffers ----
  const int kh = lane >> 5, li = lane & 31;
  const FeatureStream fs(feats + (long long)b * n * SA_L, n, lane, wave);
  float f0[32], f1[32], f2[32];
  const int nch = (npad + 63) >> 6;          // >= 2: n > 64
  fs.load_chunk(f0, 0);
  fs.load_chunk(f1, 1);
  if (2 < nch) fs.load_chunk(f2, 2);
  lds_barrier();

  // ---- row maxima, K = exp(M - rowmax) in place: half-wave `half` owns rows half, half + 8, ... ----
  const int half = tid >> 5, l32 = tid & 31;
#pragma unroll 1
  for (int p = 0; p < 9; ++p) {
    const int i = half + 8 * p;
    if (i <= SA_M) {                                                   // per half-wave; nothing below leaves the half
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
  const StageAMarginals mg = stage_a_marginals(n);
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
        if (i <= SA_M) {
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
          if (l32 == 0) al[i] = (i == SA_M ? mg.a_dust : mg.a_reg) / sx;
        }
      }
    }
    lds_barrier();
    {
      const float a_lane = al[lane], a_d = al[SA_M];
#pragma unroll
      for (int q = 0; q < AN_CQ; ++q) {
        const int j = tid + 256 * q;
        if (j < n) {
          const float* col = Kx + j;
          float s0 = col[SA_M * ld] * a_d, s1 = 0.f;                  // two chains: half the dependent-FMA latency
#pragma unroll
          for (int i = 0; i < SA_M; i += 2) {
            s0 = fmaf(col[i * ld], lane_bcast(a_lane, i), s0);
            s1 = fmaf(col[(i + 1) * ld], lane_bcast(a_lane, i + 1), s1);
          }
          be[j] = mg.b_col / (s0 + s1);
        }
      }
    }
    lds_barrier();
  }

  // ---- P = K alpha beta (n + m); dustbin row dropped.  Packed (hi, lo) pairs of this thread's columns in registers first:
  // the planes overwrite K, which other threads' columns still live in. ----
  {
    uint32_t pk[AN_CQ][SA_M];
    const float a_lane = al[lane];
#pragma unroll
    for (int q = 0; q < AN_CQ; ++q) {
      const int j = tid + 256 * q;
#pragma unroll
      for (int i = 0; i < SA_M; ++i) pk[q][i] = 0u;                   // pad columns: +0 in both planes
      if (j < n) {
        const float* col = Kx + j;
        const float bj = be[j] * mg.scale;
#pragma unroll
        for (int i = 0; i < SA_M; ++i) {
          uint16_t h, l;
          p_plane_entry(col[i * ld], lane_bcast(a_lane, i), bj, h, l);
          pk[q][i] = (uint32_t)h | ((uint32_t)l << 16);
        }
      }
    }
    lds_barrier();                                                     // every thread is done reading K, alpha, beta
#pragma unroll
    for (int q = 0; q < AN_CQ; ++q) {
      const int j = tid + 256 * q;
      if (j < npad) {
#pragma unroll
        for (int i = 0; i < SA_M; ++i) {
          Phi[i * pld + j] = (uint16_t)(pk[q][i] & 0xffffu);
          Plo[i * pld + j] = (uint16_t)(pk[q][i] >> 16);
        }
      }
    }
  }
  lds_barrier();

  // ---- V[l][m] = sum_j F[j][l] * P[m][j], the normalisations and the outputs (salad_stage_a.h) ----
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
  auto mma_chunk = [&](const float (&f)[32], int c) {
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int j0 = 64 * c + 16 * st;
      if (j0 < npad) aggregate_step16(f, 8 * st, Phi, Plo, pld, j0 + 8 * kh, li, acc0, acc1);   // uniform; the planes end at column npad
    }
  };
#pragma unroll 1
  for (int c = 0; c < nch; c += 3) {       // three chunk buffers in fixed registers; nothing is requested at or behind nch
    mma_chunk(f0, c);
    if (c + 3 < nch) fs.load_chunk(f0, c + 3);
    mma_chunk(f1, c + 1);
    if (c + 4 < nch) fs.load_chunk(f1, c + 4);
    mma_chunk(f2, c + 2);
    if (c + 5 < nch) fs.load_chunk(f2, c + 5);
  }
  const float gden = stage_a_norms(acc0, acc1, g, ssq, red);
  stage_a_store(acc0, acc1, g, gden, b, out_f32, out_bf16);
}

}  // namespace

int launch_sinkhorn_aggregate_n(const float* scores, const float* feats, const float* tokfeat,
                                int B, int n, int m, int l, int t, float dustbin, int iters,
                                float* out_f32, uint16_t* out_bf16, hipStream_t stream) {
  VPR_TRY_LAUNCH(stage_a_check(SaladDomain::AnyN, scores, feats, tokfeat, B, n, m, l, t, iters, out_f32, out_bf16));
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
