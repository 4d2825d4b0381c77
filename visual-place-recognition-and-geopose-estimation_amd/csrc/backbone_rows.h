// backbone_rows.h — the row kernels every backbone block runs, each piece written once: the LayerNorm row pass of
// layernorm.hip and of the LayerNorm blocks of ln_cls_linear.hip, and the skinny GEMM (a few rows x [N, K]^T) of skinny.hip
// and of the cls-row blocks of ln_cls_linear.hip.  The order and form of every floating-point expression here is part of the
// outputs' bits (tests/test_layernorm_edges_gpu.py asserts the fused launch bit-equal to the LayerNorm entry).
// Device helpers take their state by reference; the host helpers at the end are the LayerNorm entries' shared refusals and
// the chunk-count dispatch.  Included by those three sources only.
#pragma once
#include <initializer_list>
#include "vpr_common.h"
#include "vpr_internal.h"

namespace vpr {

// ---- LayerNorm row pass ---------------------------------------------------------------------------------------------
// One wave per row of C = 8 * nchunks bf16; lane `lane` holds 16-byte chunks lane, lane + 64, ... (NCH of them, those past
// nchunks zero) as f32 in v.  Two-pass statistics in f32 (mean, then centred sum of squares) like torch, one bf16 rounding.

// The lane's chunks of the row at element offset `off` (= row * C) and their running sum s.  What is normalised is one of
//   res != nullptr        v = bf16(x + res), which also goes to sum_out when `store_sum` (the residual add PyTorch would do as a
//                         separate pass: one read of each operand, two writes, instead of add (r2 w1) + LayerNorm (r1 w1));
//   pre_bias != nullptr   v = x + pre_bias in f32: a per-column offset carried outside the bf16 stream (two float4 per chunk);
//   neither               v = x.
// The choice is wave-uniform.
template <int NCH>
__device__ __forceinline__ void ln_load_row(const uint16_t* x, const uint16_t* res, uint16_t* sum_out, const float* pre_bias,
                                            long long off, bool store_sum, int nchunks, int lane, float (&v)[NCH][8], float& s) {
  s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int ch = lane + 64 * i;
    if (ch < nchunks) {
      const s16x8 q = *reinterpret_cast<const s16x8*>(x + off + ch * 8);
      if (res != nullptr) {
        const s16x8 r = *reinterpret_cast<const s16x8*>(res + off + ch * 8);
        s16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint16_t sb = f32_to_bf16_bits(bf16_bits_to_f32((uint16_t)q[e]) + bf16_bits_to_f32((uint16_t)r[e]));
          o[e] = (short)sb;
          v[i][e] = bf16_bits_to_f32(sb);
          s += v[i][e];
        }
        if (store_sum) *reinterpret_cast<s16x8*>(sum_out + off + ch * 8) = o;
      } else if (pre_bias != nullptr) {
        const float4 p0 = *reinterpret_cast<const float4*>(pre_bias + ch * 8);
        const float4 p1 = *reinterpret_cast<const float4*>(pre_bias + ch * 8 + 4);
        const float pb[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i][e] = bf16_bits_to_f32((uint16_t)q[e]) + pb[e]; s += v[i][e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i][e] = bf16_bits_to_f32((uint16_t)q[e]); s += v[i][e]; }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
    }
  }
}

// mean and 1 / sqrt(var + eps) of the row from the lanes' v and s.
template <int NCH>
__device__ __forceinline__ void ln_stats(const float (&v)[NCH][8], float s, int C, float eps, int lane, float& mean, float& rstd) {
  mean = wave_sum(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < (C >> 3)) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; ss = fmaf(d, d, ss); }
    }
  rstd = 1.0f / sqrtf(wave_sum(ss) / (float)C + eps);
}

// Element e of chunk ch of gamma / beta.  ParamT uint16_t (bf16 bits) / float: fetched by element, no alignment asked of the
// vector; s16x8: bf16 in 16-byte chunks (one load per chunk), for the entry that requires aligned parameters.
template <typename ParamT>
__device__ __forceinline__ float ln_param(const ParamT* p, int ch, int e) {
  if constexpr (sizeof(ParamT) == 16) return bf16_bits_to_f32((uint16_t)p[ch][e]);
  else if constexpr (sizeof(ParamT) == 2) return bf16_bits_to_f32((uint16_t)p[ch * 8 + e]);
  else return p[ch * 8 + e];
}

// (v - mean) * rstd * gamma + beta, rounded once to bf16, to the row at element offset `off` of y.
template <int NCH, typename ParamT>
__device__ __forceinline__ void ln_store_row(const float (&v)[NCH][8], float mean, float rstd, const ParamT* gamma,
                                             const ParamT* beta, uint16_t* y, long long off, int nchunks, int lane) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int ch = lane + 64 * i;
    if (ch < nchunks) {
      s16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = ln_param(gamma, ch, e), b = ln_param(beta, ch, e);
        o[e] = (short)f32_to_bf16_bits((v[i][e] - mean) * rstd * g + b);
      }
      *reinterpret_cast<s16x8*>(y + off + ch * 8) = o;
    }
  }
}

// ---- skinny GEMM ----------------------------------------------------------------------------------------------------
// The scheme (16 columns x MBW row blocks per workgroup, NW waves split K) is described at the top of skinny.hip.  C/D of
// v_mfma_f32_16x16x32_bf16 with W as the A operand: col = row m (lane & 15), rows 4 (lane >> 4) + e = 4 consecutive columns.

// The lane's operand streams: W row n0 + row and input rows m0 + 16 mb + row, both clamped into the matrix (a clamped duplicate
// is loaded and its result dropped), offset by the lane's 8 elements (chunk) of a 32-deep K-step.  Which (row, chunk) a lane
// FETCHES is the form's choice:
//   QUAD = false   the pair it feeds to the MFMA, (lane & 15, lane >> 4): neighbouring lanes read 16 different rows, which the
//                  load path serves at a quarter of its rate (measured: the four skinny launches of a block fit 3.2 us +
//                  0.0276 us per KB a workgroup loads, 15 B / clk per CU; by quads 0.0129: profiles/cls_chain_bench.txt);
//   QUAD = true    (lane >> 2, lane & 3): four neighbouring lanes read 64 contiguous bytes of one row, and the fragment then
//                  crosses to the lane that feeds it (skinny_to_mfma_lane: ds_bpermute, no LDS storage).
template <int MBW, bool QUAD = false>
struct SkinnyOperands {
  const uint16_t* wp;
  const uint16_t* ip[MBW];
  __device__ __forceinline__ SkinnyOperands(const uint16_t* W, int ldw, int n0, int N, const uint16_t* in, long long ldi, int m0,
                                            int M, int lane) {
    const int r = QUAD ? lane >> 2 : lane & 15, g = QUAD ? lane & 3 : lane >> 4;
    wp = W + (long long)min(n0 + r, N - 1) * ldw + 8 * g;
#pragma unroll
    for (int mb = 0; mb < MBW; ++mb) ip[mb] = in + (long long)min(m0 + mb * 16 + r, M - 1) * ldi + 8 * g;
  }
};

// The fragment (row lane & 15, chunk lane >> 4) from the lane that fetched it under QUAD: lane 4 (lane & 15) + (lane >> 4).
__device__ __forceinline__ bf16x8 skinny_to_mfma_lane(bf16x8 f) {
  typedef __attribute__((ext_vector_type(4))) int i32x4;
  const int src = 4 * (4 * (int)(threadIdx.x & 15) + (int)((threadIdx.x & 63) >> 4));      // byte index of the source lane
  i32x4 v = __builtin_bit_cast(i32x4, f);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_ds_bpermute(src, v[e]);
  return __builtin_bit_cast(bf16x8, v);
}

// K-steps [kbeg, kend) into acc: UNR steps' (1 + MBW) * UNR fragment loads are requested before their MFMAs (a slice is one or
// two memory round trips, not a streaming loop), then the remainder step by step.  The sums are kept in locals and handed over
// once: through the reference the compiler, which optimises this function before it inlines it, has to assume that they alias
// the operand streams, and the loops it then leaves cost skinny_linear_kernel<*, 4, 4> 16 more AGPRs and an occupancy step.
template <int UNR, int MBW, bool QUAD>
__device__ __forceinline__ void skinny_k_slice(const SkinnyOperands<MBW, QUAD>& o, int kbeg, int kend, f32x4 (&acc)[MBW]) {
  const auto frag = [](const uint16_t* p) -> bf16x8 {
    const bf16x8 f = *reinterpret_cast<const bf16x8*>(p);
    if constexpr (QUAD) return skinny_to_mfma_lane(f); else return f;
  };
  f32x4 a[MBW];
#pragma unroll
  for (int mb = 0; mb < MBW; ++mb) a[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  int ks = kbeg;
  for (; ks + UNR <= kend; ks += UNR) {
    bf16x8 wf[UNR], xf[UNR][MBW];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      wf[u] = frag(o.wp + (ks + u) * 32);
#pragma unroll
      for (int mb = 0; mb < MBW; ++mb) xf[u][mb] = frag(o.ip[mb] + (ks + u) * 32);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int mb = 0; mb < MBW; ++mb) a[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], xf[u][mb], a[mb], 0, 0, 0);
  }
  for (; ks < kend; ++ks) {
    const bf16x8 wf = frag(o.wp + ks * 32);
#pragma unroll
    for (int mb = 0; mb < MBW; ++mb)
      a[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, frag(o.ip[mb] + ks * 32), a[mb], 0, 0, 0);
  }
#pragma unroll
  for (int mb = 0; mb < MBW; ++mb) acc[mb] = a[mb];
}

// The waves' accumulators through red (LDS), one barrier (it also publishes whatever else the waves wrote to LDS before it);
// wave w < MBW gets the sum s of row block w over partials p = 0 .. NW - 1 in that order (deterministic).  False: a wave with
// no row block, which is done.
template <int NW, int MBW>
__device__ __forceinline__ bool skinny_reduce(const f32x4 (&acc)[MBW], float (&red)[NW][MBW][64][4], int lane, int wave, f32x4& s) {
#pragma unroll
  for (int mb = 0; mb < MBW; ++mb) *reinterpret_cast<f32x4*>(&red[wave][mb][lane][0]) = acc[mb];
  __syncthreads();
  if (NW > MBW && wave >= MBW) return false;
  s = *reinterpret_cast<const f32x4*>(&red[0][wave][lane][0]);
#pragma unroll
  for (int p = 1; p < NW; ++p) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(&red[p][wave][lane][0]);
    s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[3] += t[3];
  }
  return true;
}

// Output columns n .. n + 3 (those below N) of one row as bf16 bits to op; rows are ldo elements apart, op 8-byte aligned
// whenever ldo % 4 == 0 (n % 4 == 0, and the entries require an 8-byte aligned out).
__device__ __forceinline__ void skinny_store4(uint16_t* op, const uint16_t (&ob)[4], int n, int N, int ldo) {
  if (n + 3 < N && (ldo & 3) == 0) {
    ushort4 o;
    o.x = ob[0]; o.y = ob[1]; o.z = ob[2]; o.w = ob[3];
    *reinterpret_cast<ushort4*>(op) = o;
  } else {
    for (int e = 0; e < 4 && n + e < N; ++e) op[e] = ob[e];
  }
}

__device__ __forceinline__ float gelu_tanh(float x) {
  // 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) = x * sigmoid(2 u): the form hipBLASLt's epilogue uses
  const float u = 0.7978845608028654f * x * fmaf(0.044715f * x, x, 1.0f);
  return x / (1.0f + __expf(-2.0f * u));
}

// ---- LayerNorm statistics partials ------------------------------------------------------------------------------------
// row_stats[P][M][2] f32, P = N / 16 (N % 16 == 0): entry [p][m] = (mean, centred sum of squares M2) of row m over its columns
// 16 p .. 16 p + 15, of the values the next LayerNorm will read: bf16(out) + stats_bias.  The skinny GEMM that writes the rows
// leaves them (producer); the fused LayerNorm + cls linear merges a row's P partials in a fixed order (consumer; equal counts,
// Chan's formula), so the statistics cost it no pass over the rows.

// Producer: the workgroup of column block p, after its store; ob = the lane's 4 columns n .. n + 3 of row m as stored (0 where
// nothing was), the 4 lanes lane & 15 == m's lane hold the row's 16 columns.  Every lane of the wave calls it.
__device__ __forceinline__ void row_stats_write16(float* __restrict__ row_stats, int p, int m, int M, const uint16_t (&ob)[4],
                                                  const float* __restrict__ stats_bias, int n, int N, int lane) {
  float t[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    t[e] = bf16_bits_to_f32(ob[e]) + (stats_bias != nullptr && n + e < N ? stats_bias[n + e] : 0.f);
  float sm = (t[0] + t[1]) + (t[2] + t[3]);
  sm += __shfl_xor(sm, 16, 64);
  sm += __shfl_xor(sm, 32, 64);
  const float mean = sm * (1.0f / 16.0f);
  float m2 = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { const float d = t[e] - mean; m2 = fmaf(d, d, m2); }
  m2 += __shfl_xor(m2, 16, 64);
  m2 += __shfl_xor(m2, 32, 64);
  if ((lane >> 4) == 0 && m < M) {
    float* dst = row_stats + ((long long)p * M + m) * 2;
    dst[0] = mean; dst[1] = m2;
  }
}

// Consumer: (mean, M2) of row `row` over all 16 P columns, by 4 adjacent lanes `part` = 0 .. 3 (all four get the result):
// mean = avg(mean_p), M2 = sum(M2_p) + 16 * sum((mean_p - mean)^2).
__device__ __forceinline__ void row_stats_merge(const float* __restrict__ row_stats, int P, int M, int row, int part, float& mean,
                                                float& m2) {
  const float* ps = row_stats + (long long)row * 2;
  const long long pstride = (long long)M * 2;
  float sm = 0.f;
#pragma unroll 8
  for (int p = part; p < P; p += 4) sm += ps[p * pstride];
  sm += __shfl_xor(sm, 1, 64);
  sm += __shfl_xor(sm, 2, 64);
  mean = sm / (float)P;
  m2 = 0.f;
#pragma unroll 8
  for (int p = part; p < P; p += 4) {
    const float2 q = *reinterpret_cast<const float2*>(ps + p * pstride);
    const float d = q.x - mean;
    m2 += q.y + 16.0f * d * d;
  }
  m2 += __shfl_xor(m2, 1, 64);
  m2 += __shfl_xor(m2, 2, 64);
}

// ---- host side --------------------------------------------------------------------------------------------------------
// What the row pass is built for: whole 16-byte chunks, at most 4 per lane, and a grid of (M + 3) / 4 workgroups.
inline bool ln_shape_ok(long long M, int C) { return (C % 8) == 0 && C <= 2048 && M <= 0x1fffffffcLL; }

// The argument check of the LayerNorm entries.  `chunked`: the pointers the form reads or writes as 16-byte chunks (all
// required, like gamma / beta, which are read by element and may sit anywhere).  VPR_OK with M == 0: nothing to launch.
inline int ln_check(std::initializer_list<const void*> chunked, const void* gamma, const void* beta, long long M, int C) {
  for (const void* p : chunked)
    if (!p) return VPR_ERR_INVALID_ARG;
  if (!gamma || !beta || M < 0 || C <= 0) return VPR_ERR_INVALID_ARG;
  if (M == 0) return VPR_OK;
  if (!ln_shape_ok(M, C)) return VPR_ERR_UNSUPPORTED;
  for (const void* p : chunked)
    if (!aligned16(p)) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

// f(std::integral_constant<int, NCH>) for the row pass's chunks per lane NCH = ceil(C / 512) in 1 .. 4; f returns a status.
template <typename F>
inline int ln_dispatch_nch(int C, F&& f) {
  switch ((C / 8 + 63) / 64) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return VPR_ERR_UNSUPPORTED;
  }
}

}  // namespace vpr
