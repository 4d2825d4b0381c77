// gemm_nt.hip — C[M,N] = act(A[M,K] * W[N,K]^T + bias), bf16 operands, f32 accumulate (MFMA); and, as a template flag of
// the same tile body, the e4m3 form C[m][n] = a_scale[m] * w_scale[n] * sum_k A[m][k] W[n][k] (gemm_nt_fp8_kernel).
//
// Used for the SALAD token MLPs (score / cluster_features / token_features
// 1x1-conv + Linear layers of the aggregator called at
// dinov2salad/dinov2salad_validation.py:49-51).  MFMA-bound stage of the hot path.
//
// Structure (cdna guide §5, "minimum 2-phase"): 128 x BN output tile per 256-thread workgroup,
// BK = 64, both operand tiles brought in by LDS-DMA (global_load_lds_dwordx4) into a 2-deep LDS
// ring with the XOR swizzle of vpr_common.h on the source address (stage_src_off), fragments read with
// ds_read_b128, v_mfma_f32_32x32x16_bf16 (e4m3: v_mfma_scale_f32_32x32x64_f8f6f4), one barrier per K-step.  Workgroup ids are remapped
// so that the workgroups of one XCD (blockIdx % 8) own a contiguous run of tiles and re-use the
// same A panel out of that XCD's L2.
#include "vpr_common.h"
#include "vpr_internal.h"

namespace vpr {

struct GemmGroup { GemmProblem p[GEMM_MAX_GROUP]; int count; };

// FP8 = true: the e4m3 form (OCP e4m3 bytes, per-row f32 scales): C[m][n] = a_scale[m] * w_scale[n] * sum_k A[m][k] W[n][k],
// the kNN score tile for more than 64 gathered queries against an e4m3 shard (BASELINE config 5 on several GPUs).  Same
// tile, LDS image, staging groups, ring, fragment rows and C/D map — a 128-byte tile row is now 128 K values — with four
// differences: the operand element (Elem, ES bytes: a K-step is 128 / ES of them); the raster; the MFMA step (two
// block-scaled 32x32x64 steps per tile row, mfma_e4m3_32x32x64 of vpr_common.h, against four bf16 32x32x16 steps); the
// epilogue.  The source pointers stay typed by element: as byte pointers the compiler turns the bf16 K-step offset from
// one scalar add into eight 64-bit vector pointer increments per step (+2 VGPRs, +1.5 % on the grouped 128 x 128 launch).
template <int BN, int WM, int WN, int STAGES = 2, bool FP8 = false>
__device__ __forceinline__ void gemm_nt_tile(const GemmProblem& pr, int orig, char* smem) {
  constexpr int BM = 128;
  using Elem = std::conditional_t<FP8, uint8_t, uint16_t>;   // operand element: e4m3 byte or bf16
  constexpr int ES = sizeof(Elem);
  constexpr int TM = BM / WM / 32;  // 32x32 tiles per wave along M
  constexpr int TN = BN / WN / 32;
  constexpr int STAGE_BYTES = (BM + BN) * TILE_ROW_BYTES;
  const Elem* __restrict__ A = reinterpret_cast<const Elem*>(pr.A);
  const Elem* __restrict__ W = reinterpret_cast<const Elem*>(pr.W);
  const float* __restrict__ bias = pr.bias;
  void* __restrict__ Cout = pr.C;
  const int lda = pr.lda, a_group_rows = pr.a_group_rows, ldw = pr.ldw, relu = pr.relu, ldc = pr.ldc;
  const long long a_group_stride = pr.a_group_stride;
  const int out_is_bf16 = pr.out_is_bf16, M = pr.M, N = pr.N, K = pr.K, tiles_m = pr.tiles_m, tiles_n = pr.tiles_n;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WN, wn = wave % WN;

  const int tile = xcd_tile(orig, tiles_m * tiles_n);
  // FP8: tile_m fastest: the (few) query tiles that share a gallery panel run back to back on one XCD
  const int tm = FP8 ? tile % tiles_m : tile / tiles_n, tn = FP8 ? tile / tiles_m : tile % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // Per-lane source row pointers for the staging groups this wave owns (group g = 8 tile rows;
  // wave w stages groups w, w+4, ...).
  constexpr int AG = BM / 8 / 4;  // A groups per wave
  constexpr int BG = BN / 8 / 4;  // W groups per wave
  const Elem* a_src[AG];
  const Elem* w_src[BG];
#pragma unroll
  for (int i = 0; i < AG; ++i) {
    const int tr = (wave + 4 * i) * 8 + (lane >> 3);
    int r = m0 + tr;
    r = r < M ? r : M - 1;
    const Elem* p = a_group_rows > 0
        ? A + (long long)(r / a_group_rows) * a_group_stride + (long long)(r % a_group_rows) * lda
        : A + (long long)r * lda;
    a_src[i] = p + stage_src_off(tr, lane) / ES;
  }
#pragma unroll
  for (int i = 0; i < BG; ++i) {
    const int tr = (wave + 4 * i) * 8 + (lane >> 3);
    int r = n0 + tr;
    r = r < N ? r : N - 1;
    w_src[i] = W + (long long)r * ldw + stage_src_off(tr, lane) / ES;
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  constexpr int KSTEP = TILE_ROW_BYTES / ES;   // elements of every row per K-step: one 128-byte tile row
  const int nk = (K * ES) >> 7;
  auto stage = [&](int buf, int ks) {
    char* ta = smem + buf * STAGE_BYTES;
    char* tw = ta + BM * TILE_ROW_BYTES;
#pragma unroll
    for (int i = 0; i < AG; ++i) glds16(a_src[i] + ks * KSTEP, ta + (wave + 4 * i) * 8 * TILE_ROW_BYTES);
#pragma unroll
    for (int i = 0; i < BG; ++i) glds16(w_src[i] + ks * KSTEP, tw + (wave + 4 * i) * 8 * TILE_ROW_BYTES);
  };

  // STAGES-deep ring, STAGES-1 K-tiles in flight.  Before the barrier of step ks, tile ks must have landed:
  // the (STAGES-2) tiles issued after it may stay outstanding (counted vmcnt; every thread issues AG + BG
  // LDS-DMA instructions per tile).  In the tail fewer tiles follow, so the wait degrades to vmcnt(0).
  constexpr int LOADS_PER_STAGE = AG + BG;
#pragma unroll
  for (int p = 0; p < STAGES - 1; ++p)
    if (p < nk) stage(p, p);
  for (int ks = 0; ks < nk; ++ks) {
    if (STAGES > 2 && ks + STAGES - 2 < nk) {
      if constexpr (STAGES == 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LOADS_PER_STAGE) : "memory");
      else if constexpr (STAGES == 4) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * LOADS_PER_STAGE) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // ... then the barrier: tile ks has landed for every wave and every wave is done reading the buffer
    // that the next issue overwrites (the one read at step ks-1).  A raw s_barrier: __syncthreads() would put
    // `s_waitcnt vmcnt(0)` in front of it (checked in the ISA) and drain the tiles the counted wait left in flight.
    if constexpr (STAGES > 2) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    } else {
      __syncthreads();
    }
    if (ks + STAGES - 1 < nk) stage((ks + STAGES - 1) % STAGES, ks + STAGES - 1);
    const char* ta = smem + (ks % STAGES) * STAGE_BYTES;
    const char* tw = ta + BM * TILE_ROW_BYTES;
    if constexpr (FP8) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {               // two 64-deep MFMA steps per 128-byte row
        i32x8 af[TM], bfr[TN];
        const int ch = 4 * s + 2 * (lane >> 5);   // a lane's 32 contiguous K bytes: chunks ch, ch + 1
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = (wm * TM + i) * 32 + (lane & 31);
          af[i] = e4m3_operand(lds_frag(ta, row, ch), lds_frag(ta, row, ch + 1));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = (wn * TN + j) * 32 + (lane & 31);
          bfr[j] = e4m3_operand(lds_frag(tw, row, ch), lds_frag(tw, row, ch + 1));
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = mfma_e4m3_32x32x64(af[i], bfr[j], acc[i][j]);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 af[TM], bfr[TN];
        const int chunk = (lane >> 5) + 2 * s;
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = lds_frag(ta, (wm * TM + i) * 32 + (lane & 31), chunk);
#pragma unroll
        for (int j = 0; j < TN; ++j) bfr[j] = lds_frag(tw, (wn * TN + j) * 32 + (lane & 31), chunk);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  // Epilogue.  C/D map of 32x32: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5).
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
      // the column's term: the additive bias (may be null), or (FP8) the W row's scale
      const float cv = FP8 ? (n < N ? pr.w_scale[n] : 0.f) : ((bias != nullptr && n < N) ? bias[n] : 0.f);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if constexpr (FP8) {                      // (acc * a_scale) * w_scale: the order of every fp8 score path
          if (m < M && n < N) reinterpret_cast<float*>(Cout)[(long long)m * ldc + n] = acc[i][j][e] * pr.a_scale[m] * cv;
        } else {
          float v = acc[i][j][e] + cv;
          if (relu) v = fmaxf(v, 0.f);
          if (m < M && n < N) {
            if (out_is_bf16)
              reinterpret_cast<uint16_t*>(Cout)[(long long)m * ldc + n] = f32_to_bf16_bits(v);
            else
              reinterpret_cast<float*>(Cout)[(long long)m * ldc + n] = v;
          }
        }
      }
    }
}

template <int BN, int WM, int WN, int STAGES = 2>
__global__ __launch_bounds__(256, STAGES > 2 ? 1 : 2) void gemm_nt_kernel(GemmProblem pr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_nt_tile<BN, WM, WN, STAGES>(pr, blockIdx.x, smem);
}

// Several independent small GEMMs in one launch (the SALAD layer-2 / token-MLP GEMMs are a few
// tiles each: as separate launches each costs a full launch + K-loop latency with the chip idle).
// Workgroup ids are dealt to the problems in order; every problem keeps its own XCD remap.
template <int BN, int WM, int WN, int STAGES>
__global__ __launch_bounds__(256, 2) void gemm_nt_group_kernel(GemmGroup grp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int id = blockIdx.x;
#pragma unroll
  for (int i = 0; i < GEMM_MAX_GROUP; ++i) {
    if (i < grp.count) {
      const int n = grp.p[i].tiles_m * grp.p[i].tiles_n;
      if (id >= 0 && id < n) { gemm_nt_tile<BN, WM, WN, STAGES>(grp.p[i], id, smem); id = -1; }
      else if (id >= 0) id -= n;
    }
  }
}

// The e4m3 form of the 128 x 128 tile (gemm_nt_tile, FP8 = true) under the name kernel traces and gemm_nt_kernel_name know.
__global__ __launch_bounds__(256, 2) void gemm_nt_fp8_kernel(GemmProblem pr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_nt_tile<128, 2, 2, 2, true>(pr, blockIdx.x, smem);
}

// ---- host side: one rule set, one kernel choice, two launchers ---------------------------------------------------------
// The argument rules of every GEMM launch of the library, in bytes; es = operand element size.  INVALID_ARG (nulls,
// non-positive sizes) comes before UNSUPPORTED (shape, pitch, alignment).
int gemm_check(const GemmProblem& g, bool e4m3, GemmTile tile) {
  const long long es = e4m3 ? 1 : 2;
  if (!g.A || !g.W || !g.C || (e4m3 && (!g.a_scale || !g.w_scale)) || g.M <= 0 || g.N <= 0 || g.K <= 0) return VPR_ERR_INVALID_ARG;
  // K is whole 128-byte tile rows; rows do not overlap; every 16-byte LDS-DMA piece of A and W is aligned
  if ((g.K * es % 128) || g.lda < g.K || g.ldw < g.K || g.ldc < g.N) return VPR_ERR_UNSUPPORTED;
  if ((g.lda * es % 16) || (g.ldw * es % 16) || (g.a_group_rows > 0 && (g.a_group_stride * es % 16))) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(g.A) || !aligned16(g.W)) return VPR_ERR_UNSUPPORTED;
  // the e4m3 kernels are the plain scaled product: no bias, no activation, f32 out, dense rows (no caller asks otherwise)
  if (e4m3 && (g.bias || g.relu || g.out_is_bf16 || g.a_group_rows > 0)) return VPR_ERR_UNSUPPORTED;
  const int ktiles = (int)(g.K * es / 128), ksplit = g.ksplit > 1 ? g.ksplit : 1;
  // 128-row tiles have no split-K.  No caller asks for one; until this rule existed the request was silently ignored.
  if (tile == GemmTile::T128) return ksplit > 1 ? VPR_ERR_UNSUPPORTED : VPR_OK;
  // 256 x 256 tiles: the pipeline's prologue issues two K-tiles; the epilogue stores 8 / 16 bytes at once and reads the
  // bias as float4 (a null bias is fine); split-K slabs are linear partial sums of at least two K-tiles each
  if (ktiles < 2 || (g.ldc % 4) || !aligned16(g.C) || !aligned16(g.bias)) return VPR_ERR_UNSUPPORTED;
  if (ksplit > 1 && (g.bias != nullptr || g.relu || ktiles < 2 * ksplit)) return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

// What runs a problem of N output columns: the name a kernel trace prints, the output-tile width, and the launch.
struct GemmNtKernel { const char* name; int bn; int (*launch)(const GemmProblem& g, hipStream_t stream); };

template <auto Kernel, int BN, int STAGES>
static int gemm_nt_run(const GemmProblem& g, hipStream_t stream) {
  return launch_kernel_lds<Kernel>(dim3(g.tiles_m * g.tiles_n), dim3(256), (size_t)STAGES * (128 + BN) * TILE_ROW_BYTES, stream, g);
}

// bf16: 128-column tiles, or one 64-column tile for N <= 64; and the A/B switch VPR_GEMM_NT_STAGES, 3 = three-deep ring
// (96 KB: one workgroup per CU).  Measured on the kNN score tile, 2 vs 3 stages: 128 x 50k 217 / 291 us, 512 x 12.5k
// 141 / 205 us — two workgroups per CU beat the deeper ring.
static GemmNtKernel gemm_nt_choose(bool e4m3, int N) {
  if (e4m3) return {"vpr::gemm_nt_fp8_kernel", 128, gemm_nt_run<gemm_nt_fp8_kernel, 128, 2>};
  if (N > 64 && tune_or(TUNE_GEMM_NT_STAGES, 2) == 3)
    return {"vpr::gemm_nt_kernel<128, 2, 2, 3>", 128, gemm_nt_run<gemm_nt_kernel<128, 2, 2, 3>, 128, 3>};
  if (N > 64) return {"vpr::gemm_nt_kernel<128, 2, 2, 2>", 128, gemm_nt_run<gemm_nt_kernel<128, 2, 2>, 128, 2>};
  return {"vpr::gemm_nt_kernel<64, 4, 1, 2>", 64, gemm_nt_run<gemm_nt_kernel<64, 4, 1>, 64, 2>};
}

const char* gemm_nt_kernel_name(bool e4m3, int N) { return gemm_nt_choose(e4m3, N).name; }

int launch_gemm_nt(const GemmProblem& in, bool e4m3, hipStream_t stream) {
  VPR_TRY_LAUNCH(gemm_check(in, e4m3, GemmTile::T128));
  const GemmNtKernel k = gemm_nt_choose(e4m3, in.N);
  GemmProblem g = in;
  g.tiles_m = (g.M + 127) / 128;
  g.tiles_n = (g.N + k.bn - 1) / k.bn;
  return k.launch(g, stream);
}

// Grouped launch, one tile shape for every member.  The grouped problems are short (K = 512: 8 K-tiles) and about one
// workgroup per CU: with the 2-deep ring each K-step waits out one full memory round trip.  Variant 1 keeps two tiles in
// flight (3-deep ring) on 128 x 64 tiles (72 KB of LDS: still two workgroups per CU, so the ~390 workgroups stay one
// resident round; a 3-deep ring on 128 x 128 tiles is 96 KB = one workgroup per CU and 258 workgroups then need a second
// round: measured 101.6 vs 88.9 us for the whole SALAD stage).  Variant 0: 128 x 128 tiles, 2-deep ring (a member with
// N <= 64 wastes MFMA work on its half-empty tile, which is cheaper than a launch of its own).
int launch_gemm_nt_group(const GemmProblem* probs, int count, hipStream_t stream) {
  if (!probs || count < 1 || count > GEMM_MAX_GROUP) return VPR_ERR_INVALID_ARG;
  const bool narrow = tune_or(TUNE_GEMM_GROUP_VARIANT, 1) == 1;   // A/B switch: 0 = 89.9 us; 1 = default (84.4 us)
  const int bn = narrow ? 64 : 128;
  GemmGroup grp;
  grp.count = count;
  int total = 0;
  for (int i = 0; i < GEMM_MAX_GROUP; ++i) {
    if (i >= count) { grp.p[i] = grp.p[0]; continue; }          // padding: never read by the kernel
    GemmProblem& g = grp.p[i] = probs[i];
    VPR_TRY_LAUNCH(gemm_check(g, false, GemmTile::T128));
    g.tiles_m = (g.M + 127) / 128;
    g.tiles_n = (g.N + bn - 1) / bn;
    total += g.tiles_m * g.tiles_n;
  }
  if (narrow)
    return launch_kernel_lds<gemm_nt_group_kernel<64, 4, 1, 3>>(dim3(total), dim3(256), (size_t)3 * (128 + 64) * TILE_ROW_BYTES, stream, grp);
  return launch_kernel_lds<gemm_nt_group_kernel<128, 2, 2, 2>>(dim3(total), dim3(256), (size_t)2 * (128 + 128) * TILE_ROW_BYTES, stream, grp);
}

}  // namespace vpr

using namespace vpr;

// ---- the three GEMM entries of the C ABI (include/vpr_amd.h) -----------------------------------------------------------
static GemmProblem gemm_problem_c(const vpr_gemm_problem& p) {
  GemmProblem g = gemm_problem(p.A, p.lda, p.W, p.ldw, p.bias, p.relu, p.C, p.ldc, p.out_is_bf16, p.M, p.N, p.K);
  g.a_group_rows = p.a_group_rows; g.a_group_stride = p.a_group_stride;
  return g;
}

extern "C" int vpr_gemm_nt_bf16(const uint16_t* A, int lda, int a_group_rows, long long a_group_stride,
                                const uint16_t* W, int ldw, const float* bias, int relu, void* C, int ldc,
                                int out_is_bf16, int M, int N, int K, void* stream) {
  const vpr_gemm_problem p{A, lda, a_group_rows, a_group_stride, W, ldw, bias, relu, C, ldc, out_is_bf16, M, N, K};
  return launch_gemm_nt(gemm_problem_c(p), false, static_cast<hipStream_t>(stream));
}

// Same contract as vpr_gemm_nt_bf16 (K >= 128, ldc % 4 == 0, C and bias 16-byte aligned), 256 x 256 tiles.
extern "C" int vpr_gemm256_nt_bf16(const uint16_t* A, int lda, int a_group_rows, long long a_group_stride,
                                   const uint16_t* W, int ldw, const float* bias, int relu, void* C, int ldc,
                                   int out_is_bf16, int M, int N, int K, void* stream) {
  const vpr_gemm_problem p{A, lda, a_group_rows, a_group_stride, W, ldw, bias, relu, C, ldc, out_is_bf16, M, N, K};
  return launch_gemm256(gemm_problem_c(p), false, static_cast<hipStream_t>(stream));
}

extern "C" int vpr_gemm_nt_group_bf16(const vpr_gemm_problem* probs, int count, void* stream) {
  if (!probs || count < 1 || count > GEMM_MAX_GROUP) return VPR_ERR_INVALID_ARG;
  GemmProblem g[GEMM_MAX_GROUP];
  for (int i = 0; i < count; ++i) g[i] = gemm_problem_c(probs[i]);
  return launch_gemm_nt_group(g, count, static_cast<hipStream_t>(stream));
}
