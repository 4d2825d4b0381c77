// skinny.hip — out[M, N] = epilogue(in[M, K] * W[N, K]^T) for a handful of rows (M <= 64 per launch
// row-group): the cls-token rows of the ViT backbone, which the split row layout keeps out of the
// big GEMMs so that those see an exact number of 256-row tiles.  A library GEMM spends 9-14 us on
// each of these (four per block, 1.0 ms per step); the work is a weight stream — N*K*2 bytes
// (2-8 MB, L2/Infinity-Cache resident between steps) against 2*M*N*K <= 0.5 GFLOP.
// Workgroup = 16 output columns (16 W rows, 32-128 KB of weights) x up to 64 input rows; its 4 / 8 /
// 16 waves split K so that a wave has one or two 128-deep slices (the kernel is one or two memory
// round trips long, not a streaming loop); a wave issues all 20 fragment loads of a slice before
// the MFMAs (v_mfma_f32_16x16x32_bf16, W rows as the A operand so a lane ends up with 4
// consecutive output columns), partial sums meet in LDS, wave w finishes row block w.
// A fragment is fetched by quads (QUAD: four neighbouring lanes read 64 contiguous bytes of one row) and crosses to the lane
// that feeds it to the MFMA; fetched by that lane itself, neighbouring lanes read 16 different rows and the kernel is bound by
// the rate at which the load path takes such requests, not by bytes (backbone_rows.h, SkinnyOperands: 7.4 / 5.1 / 7.7 / 10.3 us for the cls rows'
// qkv / proj / fc1 / fc2 that way, 5.0 / 4.0 / 5.5 / 6.4 us by quads).  Same K partition, same sums, same bits either way.
#include "backbone_rows.h"

namespace vpr {

template <typename BiasT, int NW, int MBW, bool QUAD>
__global__ __launch_bounds__(NW * 64) void skinny_linear_kernel(
    const uint16_t* __restrict__ in, int ldi, const uint16_t* __restrict__ W, int ldw,
    const BiasT* __restrict__ bias, int mode, uint16_t* __restrict__ out, int ldo, int M, int N, int K,
    const float* __restrict__ stats_bias, float* __restrict__ row_stats) {
  constexpr int UNR = MBW == 4 ? 4 : 8;          // K-steps per batch: (1 + MBW) * UNR fragment loads in flight
  __shared__ float red[NW][MBW][64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * (16 * MBW);
  const int ksteps = K >> 5;
  const int kbeg = (int)((long long)ksteps * wave / NW), kend = (int)((long long)ksteps * (wave + 1) / NW);
  const int m = m0 + wave * 16 + r, n = n0 + 4 * g;
  const bool live = wave < MBW && m < M && n < N;
  uint16_t* op = out + (long long)min(m, M - 1) * ldo + min(n, N - 1);      // (bf16 modes)
  const auto bias_at = [&](int j) -> float {
    if constexpr (sizeof(BiasT) == 2) return bf16_bits_to_f32((uint16_t)bias[j]); else return bias[j];
  };
  // what the epilogue adds (the residual or the bias), requested before the K-slice: no second round trip after the reduction
  float add[4] = {0.f, 0.f, 0.f, 0.f};
  if (live)
    for (int e = 0; e < 4 && n + e < N; ++e) add[e] = mode == SK_ACCUMULATE ? bf16_bits_to_f32(op[e]) : bias_at(n + e);
  const SkinnyOperands<MBW, QUAD> ops(W, ldw, n0, N, in, ldi, m0, M, lane);
  f32x4 acc[MBW], s;
  skinny_k_slice<UNR>(ops, kbeg, kend, acc);
  if (!skinny_reduce(acc, red, lane, wave, s)) return;
  if (mode == SK_BIAS_F32) {                    // f32 output, bias only
    if (live) {
      float* of = reinterpret_cast<float*>(out) + (long long)m * ldo + n;
      for (int e = 0; e < 4 && n + e < N; ++e) of[e] = s[e] + add[e];
    }
    return;
  }
  float v[4] = {s[0], s[1], s[2], s[3]};
  uint16_t ob[4] = {0, 0, 0, 0};
  if (live) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (n + e >= N) break;
      v[e] += add[e];
      if (mode == SK_BIAS_GELU) v[e] = gelu_tanh(v[e]);
      if (mode == SK_BIAS_GELU_ERF) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752f));   // nn.GELU() of DINOv2
      if (mode == SK_BIAS_RELU) v[e] = fmaxf(v[e], 0.f);
      ob[e] = f32_to_bf16_bits(v[e]);
    }
    skinny_store4(op, ob, n, N, ldo);
  }
  if (row_stats != nullptr) row_stats_write16(row_stats, blockIdx.x, m, M, ob, stats_bias, n, N, lane);   // N % 16 == 0
}

int launch_skinny_linear(const uint16_t* in, int ldi, const uint16_t* W, int ldw, const void* bias,
                         int bias_is_bf16, int mode, uint16_t* out, int ldo, int M, int N, int K,
                         const float* stats_bias, float* row_stats, void* stream) {
  if (row_stats != nullptr && (N % 16)) return VPR_ERR_UNSUPPORTED;
  if (!in || !W || !out || M < 0 || N <= 0 || K <= 0 || mode < 0 || mode > 5) return VPR_ERR_INVALID_ARG;
  if (mode != SK_ACCUMULATE && !bias) return VPR_ERR_INVALID_ARG;
  if (M == 0) return VPR_OK;
  if ((K % 32) || (ldi % 8) || (ldw % 8) || ldi < K || ldw < K || ldo < N) return VPR_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(W)) & 15) return VPR_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(out) & 7) return VPR_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ksteps = K / 32;
  const int nw_auto = ksteps >= 64 ? 16 : (ksteps >= 32 ? 8 : 4);
  const int nw_env = tune_or(TUNE_SKINNY_NW, 0);
  const int nw = (nw_env == 4 || nw_env == 8 || nw_env == 16) ? nw_env : nw_auto;
  // few column blocks (N <= 2048: at most 128 workgroups): one 16-row block per workgroup so the
  // launch still covers the chip and a workgroup pulls 1/4 of the input rows through its L1
  const int mbw_env = tune_or(TUNE_SKINNY_MBW, 0);              // A/B switch
  const int mbw = (mbw_env == 1 || mbw_env == 4) ? mbw_env : ((N + 15) / 16 <= 128 && M > 16 ? 1 : 4);
  const dim3 grid((unsigned)((N + 15) / 16), (unsigned)((M + 16 * mbw - 1) / (16 * mbw)));
  const bool bf = bias_is_bf16 || !bias;
  const bool quad = tune_or(TUNE_SKINNY_FETCH, 1) != 0;        // A/B switch: 0 = a lane fetches the fragment it feeds to the MFMA
#define VPR_SKINNY_LAUNCH(T, NWV, MBV)                                                                              \
  VPR_TRY_LAUNCH(launch_kernel(quad ? skinny_linear_kernel<T, NWV, MBV, true> : skinny_linear_kernel<T, NWV, MBV, false>, grid, \
                               dim3(NWV * 64), 0, st, in, ldi, W, ldw, static_cast<const T*>(bias), mode, out, ldo, M, N, K, \
                               stats_bias, row_stats))
#define VPR_SKINNY_NW(T, MBV)                                                                                       \
  do {                                                                                                              \
    if (nw == 16) VPR_SKINNY_LAUNCH(T, 16, MBV); else if (nw == 8) VPR_SKINNY_LAUNCH(T, 8, MBV); else VPR_SKINNY_LAUNCH(T, 4, MBV); \
  } while (0)
  if (bf) { if (mbw == 1) VPR_SKINNY_NW(uint16_t, 1); else VPR_SKINNY_NW(uint16_t, 4); }
  else    { if (mbw == 1) VPR_SKINNY_NW(float, 1); else VPR_SKINNY_NW(float, 4); }
#undef VPR_SKINNY_NW
#undef VPR_SKINNY_LAUNCH
  return VPR_OK;
}
}  // namespace vpr

using namespace vpr;

extern "C" int vpr_skinny_linear_bf16(const uint16_t* in, int ldi, const uint16_t* W, int ldw, const void* bias,
                                      int bias_is_bf16, int mode, uint16_t* out, int ldo, int M, int N, int K,
                                      void* stream) {
  return launch_skinny_linear(in, ldi, W, ldw, bias, bias_is_bf16, mode, out, ldo, M, N, K, nullptr, nullptr, stream);
}

extern "C" int vpr_skinny_linear_stats_bf16(const uint16_t* in, int ldi, const uint16_t* W, int ldw, const void* bias,
                                            int bias_is_bf16, int mode, uint16_t* out, int ldo, int M, int N, int K,
                                            const float* stats_bias, float* row_stats, void* stream) {
  if (!row_stats) return VPR_ERR_INVALID_ARG;
  return launch_skinny_linear(in, ldi, W, ldw, bias, bias_is_bf16, mode, out, ldo, M, N, K, stats_bias, row_stats, stream);
}
