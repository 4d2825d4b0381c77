// layernorm.hip — row LayerNorm for bf16 activations (the DINOv2 backbone calls it 49 times per
// forward: 2 per block + the final norm; PyTorch's kernel reaches ~2 TB/s on [16448, 1024]).
// HBM-bound: algorithmic bytes = 2 * M * C * 2.  One wave per row, 4 rows per workgroup, every
// lane holds its 16-B chunks in registers (chunk = lane + 64*i), two-pass statistics in f32
// (mean, then centred sum of squares) like torch, output rounded once to bf16.  The row pass itself
// (ln_load_row with its three front ends, ln_stats, ln_store_row) is in backbone_rows.h.
#include "backbone_rows.h"

namespace vpr {

template <int NCH, typename ParamT, int RW>
__global__ __launch_bounds__(256) void layernorm_bf16_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ res, uint16_t* __restrict__ sum_out,
    const float* __restrict__ pre_bias, const ParamT* __restrict__ gamma, const ParamT* __restrict__ beta,
    float eps, uint16_t* __restrict__ y, long long M, int C) {
  // RW = 1 or 2 rows per wave, all their 16-byte chunks requested before the first reduction (one round of
  // workgroups for [16448, 1024] instead of two).  It did not pay: see launch_ln.  The second row is spelled
  // out: in a loop over the rows the row-independent address arithmetic of the row pass is hoisted to the top
  // of the kernel, and holding it there costs the two-row forms of C > 512 an occupancy step.
  static_assert(RW == 1 || RW == 2, "one or two rows per wave");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row0 = ((long long)blockIdx.x * 4 + wave) * RW;
  if (row0 >= M) return;
  const int nchunks = C >> 3;
  const bool second = RW == 2 && row0 + 1 < M;
  float v[RW][NCH][8], s[RW], mean, rstd;
  ln_load_row<NCH>(x, res, sum_out, pre_bias, row0 * C, true, nchunks, lane, v[0], s[0]);
  if constexpr (RW == 2)                                          // a clamped duplicate re-reads the last row, stores nothing
    ln_load_row<NCH>(x, res, sum_out, pre_bias, (second ? row0 + 1 : M - 1) * C, second, nchunks, lane, v[1], s[1]);
  ln_stats<NCH>(v[0], s[0], C, eps, lane, mean, rstd);
  ln_store_row<NCH>(v[0], mean, rstd, gamma, beta, y, row0 * C, nchunks, lane);
  if constexpr (RW == 2) {
    if (!second) return;
    ln_stats<NCH>(v[1], s[1], C, eps, lane, mean, rstd);
    ln_store_row<NCH>(v[1], mean, rstd, gamma, beta, y, (row0 + 1) * C, nchunks, lane);
  }
}

template <typename ParamT>
static int launch_ln(const uint16_t* x, const uint16_t* res, uint16_t* sum_out, const float* pb, const ParamT* g, const ParamT* b,
                     float eps, uint16_t* y, long long M, int C, hipStream_t stream) {
  // A/B switch: rows per wave.  Measured in bench.py on one box:
  const int rw = tune_or(TUNE_LN_ROWS, 1);               // 2 rows 11.80/11.80 ms per step, 1 row 11.75/11.72 -> default 1
  return ln_dispatch_nch(C, [&](auto nch) {
    constexpr int NCH = decltype(nch)::value;
    if constexpr (NCH <= 2)
      if (rw == 2)
        return launch_kernel(layernorm_bf16_kernel<NCH, ParamT, 2>, dim3((unsigned)((M + 7) / 8)), dim3(256), 0, stream,
                             x, res, sum_out, pb, g, b, eps, y, M, C);
    return launch_kernel(layernorm_bf16_kernel<NCH, ParamT, 1>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream,
                         x, res, sum_out, pb, g, b, eps, y, M, C);
  });
}

// The three entries: ln_check on the form's chunked pointers, then the parameter type.  res / sum_out / pb are null in the
// forms without them.
static int ln_entry(std::initializer_list<const void*> chunked, const uint16_t* x, const uint16_t* res, uint16_t* sum_out,
                    const float* pb, const void* gamma, const void* beta, int params_are_bf16, float eps, uint16_t* y,
                    long long M, int C, void* stream) {
  const int st = ln_check(chunked, gamma, beta, M, C);
  if (st != VPR_OK || M == 0) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (params_are_bf16)
    return launch_ln(x, res, sum_out, pb, static_cast<const uint16_t*>(gamma), static_cast<const uint16_t*>(beta), eps, y, M, C, s);
  return launch_ln(x, res, sum_out, pb, static_cast<const float*>(gamma), static_cast<const float*>(beta), eps, y, M, C, s);
}

}  // namespace vpr

using namespace vpr;

extern "C" int vpr_layernorm_bf16(const uint16_t* x, const void* gamma, const void* beta, int params_are_bf16,
                                  float eps, uint16_t* y, long long M, int C, void* stream) {
  return ln_entry({x, y}, x, nullptr, nullptr, nullptr, gamma, beta, params_are_bf16, eps, y, M, C, stream);
}

extern "C" int vpr_add_layernorm_bf16(const uint16_t* x, const uint16_t* res, uint16_t* sum_out, const void* gamma,
                                      const void* beta, int params_are_bf16, float eps, uint16_t* y, long long M,
                                      int C, void* stream) {
  return ln_entry({x, y, res, sum_out}, x, res, sum_out, nullptr, gamma, beta, params_are_bf16, eps, y, M, C, stream);
}

extern "C" int vpr_bias_layernorm_bf16(const uint16_t* x, const float* pre_bias, const void* gamma, const void* beta,
                                       int params_are_bf16, float eps, uint16_t* y, long long M, int C, void* stream) {
  return ln_entry({x, y, pre_bias}, x, nullptr, nullptr, pre_bias, gamma, beta, params_are_bf16, eps, y, M, C, stream);
}
