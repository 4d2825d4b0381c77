// ln_cls_linear.hip — one launch for "LayerNorm of every row" + "linear layer on the LayerNorm of the
// few cls rows".  In the split row layout the cls rows' linear layers are 64-row launches that cost
// ~7 us each (dispatch latency + two memory round trips, measured by doubling them: +0.33 ms per 48
// launches) for ~3 us of work.  The two that directly follow a LayerNorm (qkv, fc1) need nothing
// but the residual rows the LayerNorm itself reads, so their workgroups ride in the LayerNorm's
// grid: blocks [0, sk_blocks) take the statistics of the cls rows from the per-16-column partials
// the producer of those rows left behind (vpr_skinny_linear_stats_bf16; merged in a fixed order,
// no pass over the rows) and run the skinny GEMM of skinny.hip on the RAW rows, the normalisation
// being applied to the 64 x 16 result instead of the 64 x C input (identity in the comment below;
// normalising the operand fragments in every workgroup repeats the LayerNorm's VALU work N/16
// times and made the launch 2x longer); the remaining blocks are the LayerNorm of layernorm.hip.  The skinny
// blocks come first in the grid so they are resident while the LayerNorm blocks stream.  Both halves are the
// shared code of backbone_rows.h: this file holds the statistics merge, the epilogue and the block split.
#include "backbone_rows.h"

namespace vpr {

struct LnClsArgs {
  const uint16_t* x; const float* pre_bias; const uint16_t* gamma; const uint16_t* beta; float eps;
  uint16_t* y; long long M; int C;
  long long cls_row0; int n_cls; const float* row_stats; int stat_parts;
  const uint16_t* W; int ldw; const float* colsum; const float* cprime; const float* bprime; int gelu; uint16_t* out; int ldo; int N;
  int sk_blocks_x, sk_blocks;
};

// ---- the cls-row linear of LayerNorm(x + pre_bias), without normalising anything element-wise:
//   LN(v) W^T + b = rstd * (x W'^T + c' - mean * colsum(W')) + b',   v = x + pre_bias,
//   W' = W * diag(gamma), c' = W' pre_bias, b' = b + W beta   (W', c', colsum, b' are static per layer)
// so the raw bf16 rows are the MFMA operand as they are (4 waves split K, 64 rows x 16 columns).
__device__ __forceinline__ void lcl_skinny_block(const LnClsArgs& a, int bx, int by, float (&red)[4][4][64][4], float (&stats)[64][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C;
  const int m0 = by * 64, n0 = bx * 16;
  const int r = lane & 15, g = lane >> 4;
  const SkinnyOperands<4> ops(a.W, a.ldw, n0, a.N, a.x + a.cls_row0 * C, C, m0, a.n_cls, lane);
  const int ksteps = C >> 5;
  f32x4 acc[4], s;
  // two K-steps per round trip (10 fragment loads in flight per lane): the kernel must stay within 64 VGPRs
  // so that the LayerNorm blocks keep 8 waves per SIMD — at 5 the HBM stream of the LayerNorm part slows down
  skinny_k_slice<2>(ops, ksteps * wave / 4, ksteps * (wave + 1) / 4, acc);
  {   // statistics of rows m0 .. m0+63 from the producer's partials, 4 threads per row
    float mean, m2;
    row_stats_merge(a.row_stats, a.stat_parts, a.n_cls, min(m0 + (tid >> 2), a.n_cls - 1), tid & 3, mean, m2);
    if ((tid & 3) == 0) { stats[tid >> 2][0] = mean; stats[tid >> 2][1] = 1.0f / sqrtf(m2 / (float)C + a.eps); }
  }
  skinny_reduce(acc, red, lane, wave, s);        // its barrier publishes stats too
  const int m = m0 + wave * 16 + r, n = n0 + 4 * g;
  if (m >= a.n_cls || n >= a.N) return;
  const float mean = stats[wave * 16 + r][0], rstd = stats[wave * 16 + r][1];
  float v[4] = {s[0], s[1], s[2], s[3]};
  uint16_t ob[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (n + e >= a.N) break;
    v[e] = fmaf(rstd, v[e] + a.cprime[n + e] - mean * a.colsum[n + e], a.bprime[n + e]);
    if (a.gelu) v[e] = gelu_tanh(v[e]);
    ob[e] = f32_to_bf16_bits(v[e]);
  }
  skinny_store4(a.out + (long long)m * a.ldo + n, ob, n, a.N, a.ldo);
}

template <int NCH>
__global__ __launch_bounds__(256, 8) void ln_cls_linear_kernel(LnClsArgs a) {
  __shared__ float red[4][4][64][4];
  __shared__ float stats[64][2];
  if ((int)blockIdx.x < a.sk_blocks) {      // block-uniform
    lcl_skinny_block(a, blockIdx.x % a.sk_blocks_x, blockIdx.x / a.sk_blocks_x, red, stats);
    return;
  }
  // ---- LayerNorm rows: the row pass of layernorm_bf16_kernel (wave per row), gamma / beta fetched as 16-byte chunks ----
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)(blockIdx.x - a.sk_blocks) * 4 + wave;
  if (row >= a.M) return;
  const int C = a.C, nchunks = C >> 3;
  float v[NCH][8];
  float s, mean, rstd;
  ln_load_row<NCH>(a.x, nullptr, nullptr, a.pre_bias, row * C, false, nchunks, lane, v, s);
  ln_stats<NCH>(v, s, C, a.eps, lane, mean, rstd);
  ln_store_row<NCH>(v, mean, rstd, reinterpret_cast<const s16x8*>(a.gamma), reinterpret_cast<const s16x8*>(a.beta), a.y, row * C,
                    nchunks, lane);
}

}  // namespace vpr

using namespace vpr;

extern "C" int vpr_bias_layernorm_cls_linear_bf16(const uint16_t* x, const float* pre_bias, const uint16_t* gamma,
                                                  const uint16_t* beta, float eps, uint16_t* y, long long M, int C,
                                                  long long cls_row0, int n_cls, const float* row_stats,
                                                  const uint16_t* W_scaled, int ldw, const float* colsum,
                                                  const float* cprime, const float* bprime, int gelu,
                                                  uint16_t* out, int ldo, int N, void* stream) {
  if (!row_stats || !colsum || !cprime || !bprime) return VPR_ERR_INVALID_ARG;
  const uint16_t* W = W_scaled;
  if (!x || !gamma || !beta || !y || !W_scaled || !out || M <= 0 || C <= 0 || n_cls <= 0 || N <= 0 || cls_row0 < 0)
    return VPR_ERR_INVALID_ARG;
  if (cls_row0 + n_cls > M) return VPR_ERR_INVALID_ARG;
  if ((C % 32) || !ln_shape_ok(M, C) || (ldw % 8) || ldw < C || ldo < N) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(y) || !aligned16(W) || !aligned16(gamma) || !aligned16(beta) || !aligned16(pre_bias))
    return VPR_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(out) & 7) return VPR_ERR_UNSUPPORTED;
  LnClsArgs a{x, pre_bias, gamma, beta, eps, y, M, C, cls_row0, n_cls, row_stats, C / 16, W, ldw, colsum, cprime, bprime, gelu, out, ldo, N, 0, 0};
  a.sk_blocks_x = (N + 15) / 16;
  a.sk_blocks = a.sk_blocks_x * ((n_cls + 63) / 64);
  const long long blocks = a.sk_blocks + (M + 3) / 4;
  if (blocks > 0x7fffffffLL) return VPR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return ln_dispatch_nch(C, [&](auto nch) {
    return launch_kernel(ln_cls_linear_kernel<decltype(nch)::value>, grid, dim3(256), 0, st, a);
  });
}
