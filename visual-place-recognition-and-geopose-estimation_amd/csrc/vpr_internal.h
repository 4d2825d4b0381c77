// vpr_internal.h — launch functions shared between the translation units of libvpr_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>
#include "../../include/vpr_amd.h"
#include "../../include/vpr_amd_salad_anyres.h"
#include "../../include/vpr_amd_salad_hires.h"

namespace vpr {

// One member of a (grouped) GEMM launch: C = act(A W^T + bias); see gemm_nt.hip.  tiles_* and kstagger are filled in by the
// launcher.  The struct is a kernel argument: its layout is part of the kernels' code.
struct GemmProblem {
  const uint16_t* A; int lda; int a_group_rows; long long a_group_stride;
  const uint16_t* W; int ldw; const float* bias; int relu;
  void* C; int ldc; int out_is_bf16; int M, N, K; int tiles_m, tiles_n;
  const float* a_scale; const float* w_scale;       // e4m3 form only (per-row scales of A and W); null otherwise
  int ksplit; long long slab_stride;                // gemm256 split-K: K slices (0 / 1 = none); slice z writes C + z * slab_stride elements
  int kstagger;                                     // gemm256: order in which a tile walks its K-tiles (0 = 0, 1, 2, ...; see g2_mainloop)
};
// The two ways to make one: named operands, everything else zero (no row groups, no split-K: set those by member).
inline GemmProblem gemm_problem(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, int relu,
                                void* C, int ldc, int out_is_bf16, int M, int N, int K) {
  GemmProblem g = {};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.relu = relu;
  g.C = C; g.ldc = ldc; g.out_is_bf16 = out_is_bf16; g.M = M; g.N = N; g.K = K;
  return g;
}
// e4m3 operands (lda / ldw / K in bytes = elements) with per-row f32 scales, f32 out:
// C[m][n] = a_scale[m] * w_scale[n] * sum_k A[m][k] W[n][k]
inline GemmProblem gemm_problem_e4m3(const uint8_t* A, int lda, const float* a_scale, const uint8_t* W, int ldw,
                                     const float* w_scale, float* C, int ldc, int M, int N, int K) {
  GemmProblem g = gemm_problem(reinterpret_cast<const uint16_t*>(A), lda, reinterpret_cast<const uint16_t*>(W), ldw, nullptr, 0,
                               C, ldc, 0, M, N, K);
  g.a_scale = a_scale; g.w_scale = w_scale;
  return g;
}
constexpr int GEMM_MAX_GROUP = 3;
// The one launch entry of each tile family; e4m3: the operands are e4m3 bytes (gemm_problem_e4m3), else bf16.
//   launch_gemm_nt  (gemm_nt.hip): 128-row tiles, any K of whole 128-byte tile rows; no split-K.
//   launch_gemm256  (gemm256.hip): 256 x 256 tiles, at least two K-tiles, stricter C / bias alignment, split-K.
// Both refuse by gemm_check and launch what gemm_nt_kernel_name / gemm256_kernel_name say.
enum class GemmTile { T128, T256 };
int gemm_check(const GemmProblem& g, bool e4m3, GemmTile tile);
int launch_gemm_nt(const GemmProblem& problem, bool e4m3, hipStream_t stream);
int launch_gemm256(const GemmProblem& problem, bool e4m3, hipStream_t stream);
int launch_gemm_nt_group(const GemmProblem* probs, int count, hipStream_t stream);    // bf16, gemm_check(T128) per member
// The kernel such a launch runs (N output columns), by the name a kernel trace prints.
const char* gemm_nt_kernel_name(bool e4m3, int N);
const char* gemm256_kernel_name(bool e4m3);
// gemm256.hip: SALAD score + cluster MLPs with the second layers fused into the layer-1 tile epilogue; S / F receive
// hidden / 256 partial-sum slabs of [M][m] / [M][l] f32 (slab 0 carries the bias), to be added in slab order.
// Fuse2Drop: dropout on the hidden layer (vpr_salad_aggregate_train): unit u of token `token` of image image_base + b is kept
// iff Philox4x32-10 word u & 3 of counter (u >> 2, image, token, pass) under key (k0, k1) is >= t; kept values are scaled by
// s; mask_out (may be null, 4-byte aligned) receives [M][2*hidden] uint8, 1 = kept.
struct Fuse2Drop { uint32_t t, k0, k1, pass, image_base; float s; uint8_t* mask_out; };
int launch_salad_mlps_fused(const uint16_t* X, int ldx, int group_rows, long long group_stride, const uint16_t* W1, const float* b1,
                            const uint16_t* W2s, const float* b2s, const uint16_t* W2c, const float* b2c,
                            float* S, float* F, int M, int C, int hidden, int m, int l, hipStream_t stream,
                            const uint16_t* W2s_frag = nullptr, const uint16_t* W2c_frag = nullptr,
                            const Fuse2Drop* drop = nullptr);
// skinny.hip: out = epilogue(in W^T) for a few rows x [N, K]^T; `mode` is one of
enum { SK_BIAS = 0, SK_BIAS_GELU = 1 /* tanh form */, SK_ACCUMULATE = 2 /* out += in W^T, no bias */, SK_BIAS_RELU = 3,
       SK_BIAS_GELU_ERF = 4, SK_BIAS_F32 = 5 /* out is float*, ldo in floats: SALAD token features */ };
int launch_skinny_linear(const uint16_t* in, int ldi, const uint16_t* W, int ldw, const void* bias, int bias_is_bf16,
                         int mode, uint16_t* out, int ldo, int M, int N, int K, const float* stats_bias,
                         float* row_stats, void* stream);

// ---- SALAD: the one description of what the aggregation is built for (salad.hip, salad_anyres.hip, salad_hires.hip) -
constexpr int SA_N = 256;   // patch tokens of the fixed-n kernels (224 px at patch 14)
constexpr int SA_M = 64;    // clusters
constexpr int SA_L = 128;   // cluster dim
constexpr int SA_T = 256;   // token dim
// n == SA_N (include/vpr_amd.h) / SA_M < n <= VPR_SALAD_MAX_N (the any-n extension) / SA_M < n <= VPR_SALAD_HIRES_MAX_N (the
// high-resolution extension)
enum class SaladDomain { FixedN, AnyN, HiRes };
// The stage-A launchers see neither C nor hidden and leave the defaults.
inline bool salad_in_domain(SaladDomain d, int n, int m, int l, int t, int C = 64, int hidden = 64) {
  if (m != SA_M || l != SA_L || t != SA_T || (C % 64) || (hidden % 64)) return false;
  if (d == SaladDomain::FixedN) return n == SA_N;
  return n > SA_M && n <= (d == SaladDomain::AnyN ? VPR_SALAD_MAX_N : VPR_SALAD_HIRES_MAX_N);
}

int launch_sinkhorn_aggregate(const float* scores, const float* feats, const float* tokfeat,
                              int B, int n, int m, int l, int t, float dustbin, int iters,
                              float* out_f32, uint16_t* out_bf16, hipStream_t stream, int nslab = 1, long long slab_rows = 0,
                              int* counters = nullptr);

// salad_anyres.hip: stage A for a run-time token count m < n <= VPR_SALAD_MAX_N (one dense slab of scores / feats)
int launch_sinkhorn_aggregate_n(const float* scores, const float* feats, const float* tokfeat,
                                int B, int n, int m, int l, int t, float dustbin, int iters,
                                float* out_f32, uint16_t* out_bf16, hipStream_t stream);

// salad_hires.hip: stage A for m < n <= VPR_SALAD_HIRES_MAX_N without an image's score matrix in LDS (one dense slab)
int launch_sinkhorn_aggregate_hires(const float* scores, const float* feats, const float* tokfeat,
                                    int B, int n, int m, int l, int t, float dustbin, int iters,
                                    float* out_f32, uint16_t* out_bf16, hipStream_t stream);

// Launch through hipLaunchKernel(), whose return value is THIS launch's status.  (The
// hipGetLastError() idiom reads a per-thread sticky value that other libraries in the process —
// e.g. hipBLASLt's kernel lookups inside PyTorch — leave set, so it cannot be trusted here.)
template <typename... KArgs>
inline int launch_kernel(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds_bytes,
                         hipStream_t stream, typename std::common_type<KArgs>::type... args) {
  void* ptrs[sizeof...(KArgs)] = {const_cast<void*>(static_cast<const void*>(&args))...};
  const hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds_bytes, stream);
  if (e != hipSuccess) {
    fprintf(stderr, "libvpr_amd: kernel launch failed: %s (grid %u,%u,%u block %u lds %zu)\n",
            hipGetErrorString(e), grid.x, grid.y, grid.z, block.x, lds_bytes);
    return VPR_ERR_LAUNCH;
  }
  return VPR_OK;
}

// ---- process-wide tuning switches (A/B experiments) --------------------------------------------------------------
// Read from the environment ONCE, when the library is loaded (capi.hip); a later setenv() has no effect on the
// library.  scripts/ and tests flip them through vpr_tuning_set().  TUNE_UNSET = the variable was absent.
// TUNE_LNHEAD_VARIANT is reserved (its name stays accepted by vpr_tuning_set); no kernel reads it.
enum TuneOpt {
  TUNE_KNN_VARIANT = 0, TUNE_KNN_GEMM_MIN_B, TUNE_KNN_GEMM_KSPLIT, TUNE_KNN_FP8_GEMM256, TUNE_GEMM_NT_STAGES,
  TUNE_GEMM_GROUP_VARIANT, TUNE_ATTN_VARIANT, TUNE_LN_ROWS, TUNE_POSE_KS, TUNE_SKINNY_NW, TUNE_SKINNY_MBW,
  TUNE_SALAD_VARIANT, TUNE_POSE_VARIANT, TUNE_LNHEAD_VARIANT, TUNE_GEMM256_DEPTH, TUNE_HEAD_TRAIN_VARIANT, TUNE_GEMM256_STAGGER, TUNE_SKINNY_FETCH, TUNE_COUNT
};
constexpr int TUNE_UNSET = -2147483647 - 1;
int tune(TuneOpt o);
inline int tune_or(TuneOpt o, int dflt) { const int v = tune(o); return v == TUNE_UNSET ? dflt : v; }

// ---- per-device launch state ---------------------------------------------------------------------------------------
// hipFuncSetAttribute (the dynamic-LDS opt-in from 64 KB up) and the CU count belong to a DEVICE, not to the process: one
// flag / one cached value per device ordinal, looked up through hipGetDevice() at every launch (~50 ns).  A process
// that drives several GPUs (or switches device between calls) gets the opt-in on each of them.
constexpr int VPR_MAX_DEVICES = 64;
// The opt-in for `bytes` of dynamic LDS of Kernel: nothing to do below 64 KiB; AT 64 KiB it is made, because a kernel may
// hold static LDS beside its dynamic 64 KiB (pose_fused_kernel does).  The per-device flag is a static of this
// instantiation, i.e. of Kernel: no two kernels can share one, which would leave the second without its opt-in.
template <auto Kernel>
inline int optin_dynamic_lds(size_t bytes) {
  static unsigned char done[VPR_MAX_DEVICES] = {};
  if (bytes < 65536) return VPR_OK;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= VPR_MAX_DEVICES) return VPR_ERR_LAUNCH;
  if (!done[dev]) {          // two threads racing here both set the attribute: harmless
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
      return VPR_ERR_LAUNCH;
    done[dev] = 1;
  }
  return VPR_OK;
}
// launch_kernel with the opt-in for the launch's own LDS size.  (A kernel whose LDS size varies per call opts in for its
// maximum through optin_dynamic_lds and then calls launch_kernel: salad_anyres.hip.)
template <auto Kernel, typename... Args>
inline int launch_kernel_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args) {
  const int st = optin_dynamic_lds<Kernel>(lds_bytes);
  return st != VPR_OK ? st : launch_kernel(Kernel, grid, block, lds_bytes, stream, args...);
}
int device_cu_count();      // capi.hip: multiProcessorCount of the current device, cached per device (256 on MI355X)

#define VPR_TRY_LAUNCH(expr) do { const int vpr_st_ = (expr); if (vpr_st_ != VPR_OK) return vpr_st_; } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// Argument checks of pointers read as 16-byte chunks / as 4-byte elements; a null pointer passes both.
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The argument check of the two run-time-n stage-A launchers (salad_anyres.hip, salad_hires.hip): INVALID_ARG (null operand,
// sizes, iterations), then UNSUPPORTED (outside `d`; scores / feats are read as 16-byte chunks, the rest as elements).
inline int stage_a_check(SaladDomain d, const float* scores, const float* feats, const float* tokfeat, int B, int n, int m, int l,
                         int t, int iters, const float* out_f32, const uint16_t* out_bf16) {
  if (!scores || !feats || !tokfeat || !out_f32 || B <= 0 || n < 1 || iters < 1) return VPR_ERR_INVALID_ARG;
  if (!salad_in_domain(d, n, m, l, t)) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(scores) || !aligned16(feats) || !aligned4(tokfeat) || !aligned4(out_f32) || (reinterpret_cast<uintptr_t>(out_bf16) & 1))
    return VPR_ERR_UNSUPPORTED;
  return VPR_OK;
}

}  // namespace vpr
