// salad.hip — SALAD optimal-transport aggregation (arXiv:2311.15937).
//
// Replaces the aggregator inside `feature_extractor(x)` of
// dinov2salad/dinov2salad_validation.py:49-51 (hub model loaded at :65, output width 8448
// pinned at :44).  The arithmetic is not in the reference tree; oracle/salad.py restates the
// published algorithm and tests/test_salad*.py pin both against closed-form known answers.
//
// Stages (round 3; each has its own C entry point, the one-call forms run them in one stream):
//   T  vpr_salad_stage_token      skinny_linear_kernel x2: g = W2_t relu(W1_t cls + b1_t) + b2_t   [B, t] f32   (token MLP; in
//                                 the pipeline it runs on the backbone's cls-row stream)
//   M  vpr_salad_stage_mlps       gemm256_fuse2_kernel: H = relu(X W1_sc^T + b1) tile by tile, each tile multiplied from LDS
//                                 with its W2 slice -> S [2][B*n, m], F [2][B*n, l] f32 partial-sum slabs (no H in HBM)
//   A  vpr_salad_stage_aggregate  sinkhorn_aggregate_kernel (one workgroup per image): slab sum, dustbin row, Sinkhorn in the
//                                 exp domain (K = exp(M - rowmax) once, then alpha / beta updates: matrix-vector products),
//                                 then the back half all stage-A kernels share (salad_stage_a.h): P planes, V = F^T P^T at
//                                 f32 accuracy, the three L2 normalisations, 8448 outputs (f32 + bf16 copy for the kNN stage)
//   vpr_salad_aggregate_f32: the same at the reference's fp32 precision (three bf16 planes per operand, f32 hidden).
//   vpr_salad_aggregate_n / _f32_n (include/vpr_amd_salad_anyres.h): any token count 65 .. 576 — stages T and the unfused M
//   as above, stage A by sinkhorn_aggregate_n_kernel (salad_anyres.hip); everything else here stays n = 256.
//   vpr_salad_aggregate_hires / _f32_hires (include/vpr_amd_salad_hires.h): 65 .. 1369 tokens — the same stages, stage A above
//   576 tokens by sinkhorn_aggregate_hires_kernel (salad_hires.hip), which keeps no score matrix in LDS.
#include <math.h>
#include "vpr_common.h"
#include "vpr_internal.h"
#include "salad_stage_a.h"
#include "../../include/vpr_amd_salad_stages.h"
#include "../../include/vpr_amd_salad_anyres.h"
#include "../../include/vpr_amd_salad_hires.h"

namespace vpr {

// SA_N / SA_M / SA_L / SA_T (patch tokens, clusters, cluster dim, token dim): vpr_internal.h
constexpr int SA_LD = SA_N + 1;   // LDS row stride (words) of the [m+1][n] score matrix
constexpr int SA_PLD = SA_N + 8;  // row stride (bf16) of the P planes: 528 B, 16-byte aligned rows, rows 4 banks apart
// LDS: [score matrix 65 x 257 f32  |  later: two P planes 64 x 264 bf16]  then the small arrays (alpha / beta / norms)
constexpr size_t SA_BIG_BYTES = ((SA_M + 1) * SA_LD * sizeof(float) > 2 * SA_M * SA_PLD * sizeof(uint16_t)
                                     ? (SA_M + 1) * SA_LD * sizeof(float) : 2 * SA_M * SA_PLD * sizeof(uint16_t));
constexpr size_t SA_SMALL_OFF = (SA_BIG_BYTES + 15) / 16 * 16;

// NSLAB = 2: scores / feats arrive as two partial-sum slabs (the fused MLP kernel's K slices of the second layers,
// gemm256_fuse2_kernel), `slab_rows` * m resp. * l elements apart; they are added here, slab 0 first.
//
// Round 3 restructure (29 -> ~15 us at B = 64 with two slabs):
//  * every global load of the kernel — the score slabs AND all 128 KB (x NSLAB) of cluster features — is issued in the
//    first microsecond; the old kernel fetched the features chunk by chunk behind the iterations, eight dependent round
//    trips of ~1 us each;
//  * the iterations run in the exp domain.  With K_ij = exp(M_ij - r_i), r_i = max_j M_ij, alpha_i = exp(u_i + r_i),
//    beta_j = exp(v_j), the log-domain updates u = log a - LSE_j(M + v), v = log b - LSE_i(M + u) are exactly
//        alpha_i = a_i / sum_j K_ij beta_j,      beta_j = b_j / sum_i K_ij alpha_i        (beta = 1 at the start),
//    i.e. one exp per matrix entry ONCE instead of two per entry per iteration (the iterations were exp-issue-bound:
//    2.6 us each), and P = K alpha beta (n + m).  Range: every row holds a K = 1 (its maximum) and so does every column
//    (the dustbin row is constant, so K = 1 along it): all sums are >= one O(1) term and alpha, beta stay within a few
//    orders of magnitude of 1 for any finite scores; entries more than e^87 below their row maximum flush to 0, which is
//    where the log-domain form's exp(x - max) puts them too.
//  * the two bf16 planes of P re-use the LDS of the score matrix (dead once K sits in registers);
//  * barriers up to the aggregation order LDS traffic only (lds_barrier(): no vmcnt(0)), so the 128-256 KB of cluster
//    features keep streaming in behind the score-dependent critical path instead of being waited for at the first
//    __syncthreads() (a CU pulls ~70 GB/s: 384 KB of input are 5.6 us when waited for up front).
// Phase clocks (timing-only build: `make ablation`, scripts/sinkhorn_phases.py): with VPR_ABLATION defined, thread 0 of
// every workgroup stores s_memrealtime (100 MHz) at the phase boundaries into a 16-slot record behind the bf16 output pointer's twin
// (g_sinkhorn_clocks, set through vpr_salad_sinkhorn_set_clocks); compiled out of the shipped library.
#ifdef VPR_ABLATION
__device__ long long* g_sinkhorn_clocks = nullptr;
#define SA_CLOCK(k) do { if (g_sinkhorn_clocks && threadIdx.x == 0) g_sinkhorn_clocks[blockIdx.x * 16 + (k)] = vpr_clock_now(); } while (0)
#else
#define SA_CLOCK(k) do { } while (0)
#endif

//
// NQ = 4 (round 3 experiment, off by default — see launch_sinkhorn_aggregate): FOUR workgroups per image, so that a 64-image
// batch covers all 256 CUs instead of 64 — the front of this kernel is what ONE CU can pull (~70 GB/s).  Every workgroup of an image runs the whole Sinkhorn
// on the scores (redundant, cheap: 128 KB of loads, ~7 us of latency-bound arithmetic) but aggregates only its quarter of the
// cluster dims (32 of 128: a quarter of the feature bytes, of the MFMAs and of the output); inside the workgroup the four
// waves split the TOKENS (64 each) and their partial V meet in LDS.  The per-cluster norm runs over all 128 cluster dims:
// each workgroup stores its un-normalised quarter of V straight into its final place in out_f32 and its partial sums of
// squares into the image's token slots of out_f32 (written last anyway) — agent-scope write-through stores — and bumps the
// image's arrival counter; the workgroup that arrives last (no spinning: the others exit) adds the four partials in quarter
// order, normalises the whole row in place and writes the token part.  Same fixed summation orders whoever finishes:
// bitwise reproducible.  `counters`: one int per image, zero before the first call, left zero (workspace contract).
template <int NSLAB, int NQ>
__global__ __launch_bounds__(256, 1) void sinkhorn_aggregate_kernel(
    const float* __restrict__ scores,   // [NSLAB][B, n, m]
    const float* __restrict__ feats,    // [NSLAB][B, n, l]
    const float* __restrict__ tokfeat,  // [B, t]
    long long slab_rows, float dustbin, int iters,
    float* __restrict__ out_f32, uint16_t* __restrict__ out_bf16, int* __restrict__ counters, int rows_per_xcd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Mx = reinterpret_cast<float*>(smem);        // [65][257] raw scores; later the two P planes
  uint16_t* Phi = reinterpret_cast<uint16_t*>(smem);      // [64][SA_PLD] bf16: hi plane of P (16-byte aligned rows)
  uint16_t* Plo = Phi + SA_M * SA_PLD;                    // lo plane: P = hi + lo to 2^-17
  float* al = reinterpret_cast<float*>(smem + SA_SMALL_OFF);   // [65] (+3 pad): row maxima, then alpha
  float* be = al + 68;                               // [256] beta
  float* ssq = be + SA_N;                            // [4][64]
  float* red = ssq + 4 * SA_M;                       // [4]
  // rows_per_xcd > 0 (A/B, VPR_SALAD_VARIANT=4): workgroup i runs on XCD i & 7 (round-robin dispatch); take the image whose
  // score / feature slabs the MLP kernel's tiles wrote from THAT XCD (gemm256's tile map gives XCD x the row tiles
  // [x * rows_per_xcd, (x + 1) * rows_per_xcd)), in case its L2 still holds them
  const int b = NQ == 4 ? (int)(blockIdx.x >> 2)
                        : rows_per_xcd > 0 ? rows_per_xcd * (int)(blockIdx.x & 7) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int qd = NQ == 4 ? (int)(blockIdx.x & 3) : 0;          // which quarter of the cluster dims this workgroup aggregates
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int D_OUT = SA_T + SA_L * SA_M;

  SA_CLOCK(0);
  // ---- all global loads up front ----
  const float* sb = scores + (long long)b * SA_N * SA_M;
  const float4* sb4 = reinterpret_cast<const float4*>(sb);
  float4 q[16];
#pragma unroll
  for (int it = 0; it < 16; ++it) q[it] = sb4[tid + 256 * it];
  if constexpr (NSLAB == 2) {
    const float4* sb4b = reinterpret_cast<const float4*>(sb + slab_rows * SA_M);
    float4 q2[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) q2[it] = sb4b[tid + 256 * it];
#pragma unroll
    for (int it = 0; it < 16; ++it) { q[it].x += q2[it].x; q[it].y += q2[it].y; q[it].z += q2[it].z; q[it].w += q2[it].w; }
  }
  // cluster features of this wave's 32 cluster-dim rows, all 256 tokens (32x32x16 A-operand map:
  // A[i = lane & 31][k = 8 * (lane >> 5) + e]); token = 32 * ch + 16 * (i >> 3) + 8 * kh + (i & 7).
  // (Tried: requesting them in chunks of 32 loads spread over the score-dependent phases, so that the wave never stalls
  // on its 64-entry load queue — the phases just shift: what bounds the front of this kernel is the ~70 GB/s one CU
  // pulls, 192-384 KB of input, not the order of the requests.)
  const float* fb = feats + (long long)b * SA_N * SA_L;
  const int l0 = NQ == 4 ? 32 * qd : 32 * wave;
  const int kh = lane >> 5, li = lane & 31;
  // NQ = 1: the wave's 32 cluster dims x all 256 tokens (8 chunks of 32 tokens); NQ = 4: the workgroup's 32 cluster dims x
  // the WAVE's 64 tokens (2 chunks): token = tok0 + 32 * ch + 16 * (i >> 3) + 8 * kh + (i & 7)
  constexpr int NCH = NQ == 4 ? 2 : SA_N / 32;
  const int tok0 = NQ == 4 ? 64 * wave : 0;
  float fa[NCH][16];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int i = 0; i < 16; ++i) fa[ch][i] = fb[(tok0 + 32 * ch + 16 * (i >> 3) + 8 * kh + (i & 7)) * SA_L + l0 + li];
  float g = tokfeat[(long long)b * SA_T + tid];

  SA_CLOCK(1);      // loads issued
  // ---- scores transposed into LDS: Mx[i][j] = scores[b][j][i]; dustbin row i = m ----
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int e4 = tid + 256 * it;
    const int j = e4 >> 4, i = (e4 & 15) * 4;
    Mx[(i + 0) * SA_LD + j] = q[it].x;
    Mx[(i + 1) * SA_LD + j] = q[it].y;
    Mx[(i + 2) * SA_LD + j] = q[it].z;
    Mx[(i + 3) * SA_LD + j] = q[it].w;
  }
  Mx[SA_M * SA_LD + tid] = dustbin;
  be[tid] = 1.f;
  // second feature slab: requested now (the score registers are free again), added once K is computed
  float fa2[NSLAB == 2 ? NCH : 1][16];
  if constexpr (NSLAB == 2) {
    const float* fb2 = fb + slab_rows * SA_L;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int i = 0; i < 16; ++i) fa2[ch][i] = fb2[(tok0 + 32 * ch + 16 * (i >> 3) + 8 * kh + (i & 7)) * SA_L + l0 + li];
  }
  lds_barrier();

  SA_CLOCK(2);      // scores arrived and staged
  // every thread keeps its operands of both half-steps in registers: its column (65 values) and its 16 entries of each
  // of its 5 rows (one 16-lane group per matrix row, 16 rows in flight per workgroup)
  const int grp = tid >> 4, l16 = tid & 15;
  float mrow[5][16], mcol[SA_M + 1];
#pragma unroll
  for (int p5 = 0; p5 < 5; ++p5) {
    const int ic = min(16 * p5 + grp, SA_M);        // clamp (EXEC stays full for the DPP steps)
#pragma unroll
    for (int c = 0; c < 16; ++c) mrow[p5][c] = Mx[ic * SA_LD + l16 + 16 * c];
  }
#pragma unroll
  for (int i = 0; i <= SA_M; ++i) mcol[i] = Mx[i * SA_LD + tid];
  // row maxima r_i, then K = exp(M - r) in both register copies
#pragma unroll
  for (int p5 = 0; p5 < 5; ++p5) {
    float mx = mrow[p5][0];
#pragma unroll
    for (int c = 1; c < 16; ++c) mx = fmaxf(mx, mrow[p5][c]);
    mx = row16_max(mx);
    const int i = 16 * p5 + grp;
    if (l16 == 0 && i <= SA_M) al[i] = mx;
#pragma unroll
    for (int c = 0; c < 16; ++c) mrow[p5][c] = __expf(mrow[p5][c] - mx);
  }
  lds_barrier();                                       // (also: every thread is done reading Mx)
  // per-row values (row maxima here, alpha below) reach a thread's column loop as ONE LDS read per lane + v_readlane:
  // 65 broadcast ds_reads, which the compiler serialises behind s_waitcnt one by one under this register pressure,
  // cost 1.5 us per loop (phase clocks, scripts/sinkhorn_phases.py)
  {
    const float r_lane = al[lane], r_dust = al[SA_M];
#pragma unroll
    for (int i = 0; i < SA_M; ++i) mcol[i] = __expf(mcol[i] - lane_bcast(r_lane, i));
    mcol[SA_M] = __expf(mcol[SA_M] - r_dust);
  }
  lds_barrier();                                       // al[] is about to be rewritten as alpha
  if constexpr (NSLAB == 2) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int i = 0; i < 16; ++i) fa[ch][i] += fa2[ch][i];
  }

  SA_CLOCK(3);      // K in registers (and, NSLAB = 2, both feature slabs arrived)
  const StageAMarginals mg = stage_a_marginals(SA_N);
  for (int it = 0; it < iters; ++it) {
    {                                                  // alpha_i = a_i / sum_j K_ij beta_j
      float bv[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) bv[c] = be[l16 + 16 * c];
#pragma unroll
      for (int p5 = 0; p5 < 5; ++p5) {
        float sx = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) sx = fmaf(mrow[p5][c], bv[c], sx);
        sx = row16_sum(sx);
        const int i = 16 * p5 + grp;
        if (l16 == 0 && i <= SA_M) al[i] = (i == SA_M ? mg.a_dust : mg.a_reg) / sx;
      }
    }
    lds_barrier();  
    {                                                  // beta_j = b_j / sum_i K_ij alpha_i
      const float a_lane = al[lane];
      float s0 = mcol[SA_M] * al[SA_M], s1 = 0.f;      // two chains: half the dependent-FMA latency
#pragma unroll
      for (int i = 0; i < SA_M; i += 2) {
        s0 = fmaf(mcol[i], lane_bcast(a_lane, i), s0);
        s1 = fmaf(mcol[i + 1], lane_bcast(a_lane, i + 1), s1);
      }
      be[tid] = mg.b_col / (s0 + s1);
    }
    lds_barrier();
  }

  SA_CLOCK(4);      // iterations done
  // ---- P = K alpha beta (n + m); dustbin row dropped.  The two bf16 planes go over the LDS of the score matrix (nobody
  // reads Mx after the barrier above the iterations). ----
  {
    const int j = tid;
    const float bj = be[j] * mg.scale;
    const float a_lane = al[lane];
#pragma unroll
    for (int i = 0; i < SA_M; ++i) p_plane_entry(mcol[i], lane_bcast(a_lane, i), bj, Phi[i * SA_PLD + j], Plo[i * SA_PLD + j]);
  }
  lds_barrier();

  SA_CLOCK(5);      // P planes in LDS
  // ---- V[l][m] = sum_j F[j][l] * P[m][j] (salad_stage_a.h): error <= 2^-16 per product, ~1e-8 absolute on descriptor
  // entries of 1e-2 (tolerance 1e-4) ----
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
    for (int st = 0; st < 2; ++st)
      aggregate_step16(fa[ch], 8 * st, Phi, Plo, SA_PLD, tok0 + 32 * ch + 16 * st + 8 * kh, li, acc0, acc1);
  }

  SA_CLOCK(6);      // aggregation MFMAs issued (features arrived)
  if constexpr (NQ == 4) {
    // ---- the four waves' partial V [32 l][64 m] (each over its 64 tokens) meet in LDS; thread t then owns cluster m = t & 63,
    //      cluster dims lq + 4 i (lq = t >> 6, i = 0..7) of this quarter ----
    float* vred = red + 4;                                  // [4 waves][32][64] f32 = 32 KB behind the small arrays
    __shared__ int s_last;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int l = (e & 3) + 8 * (e >> 2) + 4 * kh;        // C/D map of 32x32: col (cluster) = lane & 31, row (l) as here
      vred[(wave * 32 + l) * SA_M + li] = acc0[e];
      vred[(wave * 32 + l) * SA_M + 32 + li] = acc1[e];
    }
    __syncthreads();
    const int m = tid & 63, lq = tid >> 6;
    float v[8], s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int l = lq + 4 * i;
      v[i] = (vred[(0 * 32 + l) * SA_M + m] + vred[(1 * 32 + l) * SA_M + m]) + (vred[(2 * 32 + l) * SA_M + m] + vred[(3 * 32 + l) * SA_M + m]);
      s2 = fmaf(v[i], v[i], s2);
    }
    ssq[lq * SA_M + m] = s2;
    float* ob = out_f32 + (long long)b * D_OUT;
#pragma unroll
    for (int i = 0; i < 8; ++i)                             // un-normalised quarter, in its final place (agent-scope write-through)
      __hip_atomic_store(ob + SA_T + (32 * qd + lq + 4 * i) * SA_M + m, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid < SA_M)                                         // this quarter's sums of squares -> the image's token slots (scratch until the end)
      __hip_atomic_store(ob + qd * SA_M + tid, (ssq[tid] + ssq[SA_M + tid]) + (ssq[2 * SA_M + tid] + ssq[3 * SA_M + tid]),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // write-through stores acknowledged = visible device-wide
    __syncthreads();
    if (tid == 0) s_last = (__hip_atomic_fetch_add(counters + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 3);
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (tid == 0) __hip_atomic_store(counters + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SA_CLOCK(7);
    // ---- finisher: per-cluster norm over all 128 cluster dims (quarter order), the whole row normalised in place ----
    const float den = l2_den((ob[m] + ob[SA_M + m]) + (ob[2 * SA_M + m] + ob[3 * SA_M + m]));
    float w[32], part = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) w[i] = ob[SA_T + (lq + 4 * i) * SA_M + m];
#pragma unroll
    for (int i = 0; i < 32; ++i) { w[i] = w[i] / den; part = fmaf(w[i], w[i], part); }
    const float gden = token_and_global_norm(g, part, red);                // (its barriers also fence the reads of the scratch slots)
    uint16_t* obh = out_bf16 ? out_bf16 + (long long)b * D_OUT : nullptr;
    {
      const float o = g / gden;
      ob[tid] = o;
      if (obh) obh[tid] = f32_to_bf16_bits(o);
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const float o = w[i] / gden;
      const int idx = SA_T + (lq + 4 * i) * SA_M + m;
      ob[idx] = o;
      if (obh) obh[idx] = f32_to_bf16_bits(o);
    }
    SA_CLOCK(8);
    return;
  }
  // ---- the three L2 normalisations and the 8448 outputs (salad_stage_a.h) ----
  const float gden = stage_a_norms(acc0, acc1, g, ssq, red);
  SA_CLOCK(7);      // norms done
  stage_a_store(acc0, acc1, g, gden, b, out_f32, out_bf16);
  SA_CLOCK(8);
}

constexpr size_t SINKHORN_LDS = SA_SMALL_OFF + (68 + SA_N + 4 * SA_M + 4) * sizeof(float);
constexpr size_t SINKHORN_LDS_Q = SINKHORN_LDS + 4 * 32 * SA_M * sizeof(float);        // + the cross-wave V buffer of the NQ = 4 form

int launch_sinkhorn_aggregate(const float* scores, const float* feats, const float* tokfeat,
                              int B, int n, int m, int l, int t, float dustbin, int iters,
                              float* out_f32, uint16_t* out_bf16, hipStream_t stream, int nslab, long long slab_rows,
                              int* counters) {
  if (!scores || !feats || !tokfeat || !out_f32 || B <= 0 || iters < 1) return VPR_ERR_INVALID_ARG;
  if (!salad_in_domain(SaladDomain::FixedN, n, m, l, t) || nslab < 1 || nslab > 2) return VPR_ERR_UNSUPPORTED;
  // Four workgroups per image (NQ = 4) — built in round 3 to put all 256 CUs on a 64-image batch, measured, and left OFF:
  // stage A 27.3 us against 20.8 us with one workgroup per image (scripts/salad_ab.py).  Every workgroup needs the whole
  // score matrix, so the batch reads 4 x 8.4 MB of scores + 16.8 MB of features = 50 MB at once and the front becomes
  // HBM-bound (5.9 us to issue the loads instead of 3.1), and the finisher's second pass over the row costs 4.2 us, which
  // eats what the quartered aggregation saves.  VPR_SALAD_VARIANT=3 selects it (A/B); it needs the zeroed counter area.
  const bool quarters = counters != nullptr && 4 * B <= device_cu_count() && tune_or(TUNE_SALAD_VARIANT, 0) == 3;
  const int rpx = (!quarters && nslab == 2 && B % 8 == 0 && tune_or(TUNE_SALAD_VARIANT, 0) == 4) ? B / 8 : 0;
#define VPR_SINKHORN_LAUNCH(NS, NQV, LDS, GRID)                                                                              \
  do {                                                                                                                       \
    VPR_TRY_LAUNCH((launch_kernel_lds<sinkhorn_aggregate_kernel<NS, NQV>>(dim3(GRID), dim3(256), LDS, stream, scores, feats, tokfeat, \
                    nslab == 2 ? slab_rows : 0LL, dustbin, iters, out_f32, out_bf16, counters, rpx)));                       \
  } while (0)
  if (quarters) {
    if (nslab == 2) VPR_SINKHORN_LAUNCH(2, 4, SINKHORN_LDS_Q, 4 * B); else VPR_SINKHORN_LAUNCH(1, 4, SINKHORN_LDS_Q, 4 * B);
  } else {
    if (nslab == 2) VPR_SINKHORN_LAUNCH(2, 1, SINKHORN_LDS, B); else VPR_SINKHORN_LAUNCH(1, 1, SINKHORN_LDS, B);
  }
#undef VPR_SINKHORN_LAUNCH
  return VPR_OK;
}

struct SaladPlan {
  size_t off_cnt, off_H, off_S, off_F, off_Ht, off_g, total;
};
constexpr size_t SALAD_COUNTER_BYTES = 4096;     // arrival counters of the four-workgroups-per-image Sinkhorn kernel: a FIXED area at
                                                 // the head of the workspace (zero before first use, left zero), whatever the shape
static bool salad_plan(int B, int n, int C, int m, int l, int t, int hidden, SaladPlan* p) {
  if (B <= 0 || n <= 0 || C <= 0 || m <= 0 || l <= 0 || t <= 0 || hidden <= 0) return false;
  p->off_cnt = 0;
  size_t off = SALAD_COUNTER_BYTES;
  p->off_H = off;  off += align_up((size_t)B * n * 2 * hidden * sizeof(uint16_t), 256);     // unfused route only
  p->off_S = off;  off += align_up((size_t)2 * B * n * m * sizeof(float), 256);              // up to two partial-sum slabs
  p->off_F = off;  off += align_up((size_t)2 * B * n * l * sizeof(float), 256);
  p->off_Ht = off; off += align_up((size_t)B * hidden * sizeof(uint16_t), 256);
  p->off_g = off;  off += align_up((size_t)B * t * sizeof(float), 256);
  p->total = off;
  return true;
}

// Partial-sum slabs the MLP stage leaves in S / F: 2 = second layers fused into the layer-1 tile epilogue
// (gemm256_fuse2_kernel; hidden = 512 -> two 256-column K slices per head), 1 = separate launches (hidden activations
// through HBM).  One rule, used by the MLP stage and the aggregation stage.  VPR_SALAD_VARIANT=1 forces the unfused route (A/B).
static int salad_slabs(int n, int C, int m, int l, int hidden) {
  if (tune_or(TUNE_SALAD_VARIANT, 0) == 1) return 1;
  const bool fused = n == SA_N && hidden == 512 && (C % 64) == 0 && C >= 128 && m == SA_M && l == SA_L;
  return fused ? 2 : 1;
}

template <typename W>      // vpr_salad_weights / vpr_salad_weights_f32: the same ten member names
static bool salad_weights_complete(const W* w) {
  return w && w->w1_sc && w->b1_sc && w->w2_s && w->b2_s && w->w2_c && w->b2_c && w->w1_t && w->b1_t && w->w2_t && w->b2_t;
}

// A call: shape, weights and the operands of the stages it runs (null / 0 for the others); salad_args() fills ws and p.
struct SaladArgs {
  int B, n, C, m, l, t, hidden;
  const vpr_salad_weights* w;
  const uint16_t* cls; long long cls_stride;                      // stage T
  const uint16_t* patch; long long patch_img_stride;              // stage M
  int sinkhorn_iters; float* out_f32; uint16_t* out_bf16;         // stage A
  bool train; const uint8_t* mask_out;                            // vpr_salad_aggregate_train: the fused route or nothing
  char* ws;
  SaladPlan p;
};
enum : unsigned { STAGE_T = 1, STAGE_M = 2, STAGE_A = 4, STAGE_ALL = 7 };

// What the launchers of `stages` read as 16-byte chunks (the outputs of the run-time-n kernel: as elements), and the strides.
static bool salad_misaligned(const SaladArgs& a, unsigned stages) {
  const vpr_salad_weights* w = a.w;
  const bool run_time_n = (stages & STAGE_A) && a.n != SA_N;
  return (((stages & (STAGE_T | STAGE_M)) || run_time_n) && !aligned16(a.ws)) ||
         ((stages & STAGE_T) && ((a.cls_stride % 8) || a.cls_stride > 0x7fffffffLL || a.cls_stride < 0 || !aligned16(a.cls) ||
                                 !aligned16(w->w1_t) || !aligned16(w->w2_t))) ||
         ((stages & STAGE_M) && ((a.patch_img_stride % 8) || !aligned16(a.patch) || !aligned16(w->w1_sc) || !aligned16(w->w2_s) ||
                                 !aligned16(w->w2_c) || !aligned4(a.mask_out))) ||
         (run_time_n && (!aligned4(a.out_f32) || (reinterpret_cast<uintptr_t>(a.out_bf16) & 1)));
}

// The one pre-check of a call that runs `stages`: every refusal a stage or a launcher below could make, decided here, so
// that a refused call has launched nothing.  The order is the ABI's: INVALID_ARG (sizes, weights), UNSUPPORTED (domain),
// WORKSPACE, then the operands of the stages.  The any-n and high-resolution entries report sinkhorn_iters < 1 ahead of
// everything and, where they leave the n = 256 chain, a misaligned operand ahead of WORKSPACE
// (include/vpr_amd_salad_anyres.h, include/vpr_amd_salad_hires.h).
static int salad_args(SaladArgs* a, SaladDomain domain, unsigned stages, void* workspace, size_t workspace_bytes) {
  const bool iters_bad = (stages & STAGE_A) && a->sinkhorn_iters < 1;
  if (domain != SaladDomain::FixedN && iters_bad) return VPR_ERR_INVALID_ARG;
  if (!workspace || a->B <= 0 || a->n < 1 || a->C <= 0) return VPR_ERR_INVALID_ARG;
  if ((stages & (STAGE_T | STAGE_M)) && !salad_weights_complete(a->w)) return VPR_ERR_INVALID_ARG;
  if (!salad_in_domain(domain, a->n, a->m, a->l, a->t, a->C, a->hidden)) return VPR_ERR_UNSUPPORTED;
  a->ws = static_cast<char*>(workspace);
  if (a->n != SA_N && salad_misaligned(*a, stages)) return VPR_ERR_UNSUPPORTED;
  if (!salad_plan(a->B, a->n, a->C, a->m, a->l, a->t, a->hidden, &a->p)) return VPR_ERR_INVALID_ARG;
  if (workspace_bytes < a->p.total) return VPR_ERR_WORKSPACE;
  if (((stages & STAGE_T) && !a->cls) || ((stages & STAGE_M) && !a->patch) || ((stages & STAGE_A) && !a->out_f32))
    return VPR_ERR_INVALID_ARG;
  if (salad_misaligned(*a, stages)) return VPR_ERR_UNSUPPORTED;
  if ((stages & STAGE_T) && a->cls_stride < a->C) return VPR_ERR_UNSUPPORTED;           // cls rows that overlap
  const bool fused = salad_slabs(a->n, a->C, a->m, a->l, a->hidden) == 2;
  // the fused kernel reads its biases as float4 and the optional fragments as 16-byte chunks
  if ((stages & STAGE_M) && fused && !(aligned16(a->w->b1_sc) && aligned16(a->w->b2_s) && aligned16(a->w->b2_c) &&
                                       aligned16(a->w->w2_s_frag) && aligned16(a->w->w2_c_frag)))
    return VPR_ERR_UNSUPPORTED;
  if (a->train && !fused) return VPR_ERR_UNSUPPORTED;                                   // no dropout mask on the unfused route
  return iters_bad ? VPR_ERR_INVALID_ARG : VPR_OK;
}

// Stage T: token MLP on the B cls rows -> g [B, t] f32 in the workspace.  Independent of stage M (other inputs, other
// workspace regions): a caller with two streams runs it beside the big GEMM (ops.salad_aggregate_split does).
static int salad_stage_token(const SaladArgs& a, hipStream_t stream) {
  uint16_t* Ht = reinterpret_cast<uint16_t*>(a.ws + a.p.off_Ht);
  float* g = reinterpret_cast<float*>(a.ws + a.p.off_g);
  const vpr_salad_weights* w = a.w;
  int st = launch_skinny_linear(a.cls, (int)a.cls_stride, w->w1_t, a.C, w->b1_t, 0, 3, Ht, a.hidden, a.B, a.hidden, a.C, nullptr, nullptr, stream);
  if (st == VPR_ERR_UNSUPPORTED) {
    const GemmProblem l1 = gemm_problem(a.cls, (int)a.cls_stride, w->w1_t, a.C, w->b1_t, 1, Ht, a.hidden, 1, a.B, a.hidden, a.C);
    st = launch_gemm_nt_group(&l1, 1, stream);
  }
  if (st != VPR_OK) return st;
  // layer 2: the same weight-streaming kernel with f32 output (mode 5); 4 us against 9 us on the 128-row GEMM tile
  st = launch_skinny_linear(Ht, a.hidden, w->w2_t, a.hidden, w->b2_t, 0, 5, reinterpret_cast<uint16_t*>(g), a.t, a.B, a.t, a.hidden,
                            nullptr, nullptr, stream);
  if (st != VPR_ERR_UNSUPPORTED) return st;
  const GemmProblem l2 = gemm_problem(Ht, a.hidden, w->w2_t, a.hidden, w->b2_t, 0, g, a.t, 0, a.B, a.t, a.hidden);
  return launch_gemm_nt_group(&l2, 1, stream);
}

// Stage M: score + cluster MLPs on the B*n patch rows -> S, F (salad_slabs() partial-sum slabs) in the workspace.
// patch row r of image b at a.patch + b*a.patch_img_stride + r*C (addressed in place).
// drop (may be null): dropout on the hidden layer — the fused route only (VPR_ERR_UNSUPPORTED on the unfused one).
static int salad_stage_mlps(const SaladArgs& a, hipStream_t stream, const Fuse2Drop* drop = nullptr) {
  uint16_t* H = reinterpret_cast<uint16_t*>(a.ws + a.p.off_H);
  float* S = reinterpret_cast<float*>(a.ws + a.p.off_S);
  float* F = reinterpret_cast<float*>(a.ws + a.p.off_F);
  const vpr_salad_weights* w = a.w;
  const int rows = a.B * a.n, hidden = a.hidden;
  if (salad_slabs(a.n, a.C, a.m, a.l, hidden) == 2)
    return launch_salad_mlps_fused(a.patch, a.C, a.n, a.patch_img_stride, w->w1_sc, w->b1_sc, w->w2_s, w->b2_s, w->w2_c, w->b2_c,
                                   S, F, rows, a.C, hidden, a.m, a.l, stream, w->w2_s_frag, w->w2_c_frag, drop);
  if (drop != nullptr) return VPR_ERR_UNSUPPORTED;
  // unfused: layer 1 on the 256 x 256-tile kernel (34 of SALAD's 38 GFLOP; B tiles x 4 = one full wave of workgroups at
  // B = 64), hidden activations through HBM as bf16, the two second layers as one grouped launch
  GemmProblem l1_sc = gemm_problem(a.patch, a.C, w->w1_sc, a.C, w->b1_sc, 1, H, 2 * hidden, 1, rows, 2 * hidden, a.C);
  l1_sc.a_group_rows = a.n; l1_sc.a_group_stride = a.patch_img_stride;
  int st = launch_gemm256(l1_sc, false, stream);
  if (st == VPR_ERR_UNSUPPORTED) st = launch_gemm_nt_group(&l1_sc, 1, stream);
  if (st != VPR_OK) return st;
  const GemmProblem l2[2] = {
      gemm_problem(H, 2 * hidden, w->w2_s, hidden, w->b2_s, 0, S, a.m, 0, rows, a.m, hidden),
      gemm_problem(H + hidden, 2 * hidden, w->w2_c, hidden, w->b2_c, 0, F, a.l, 0, rows, a.l, hidden)};
  return launch_gemm_nt_group(l2, 2, stream);
}

// The one choice of the stage-A kernel: the n = 256 kernel on `nslab` partial-sum slabs `slab_rows` rows apart (with the arrival
// counters, where the caller has them); for any other n one dense slab, as salad_slabs() says off 256: the run-time-n kernel
// up to VPR_SALAD_MAX_N tokens, above that the high-resolution kernel, which keeps no score matrix in LDS.
static int salad_launch_aggregate(const float* S, const float* F, const float* g, int B, int n, int m, int l, int t, float dustbin,
                                  int iters, float* out_f32, uint16_t* out_bf16, hipStream_t stream, int nslab, long long slab_rows,
                                  int* counters) {
  if (n > VPR_SALAD_MAX_N) return launch_sinkhorn_aggregate_hires(S, F, g, B, n, m, l, t, dustbin, iters, out_f32, out_bf16, stream);
  if (n != SA_N) return launch_sinkhorn_aggregate_n(S, F, g, B, n, m, l, t, dustbin, iters, out_f32, out_bf16, stream);
  return launch_sinkhorn_aggregate(S, F, g, B, n, m, l, t, dustbin, iters, out_f32, out_bf16, stream, nslab, slab_rows, counters);
}

// Stage A: Sinkhorn + aggregation + normalisations on what stages T and M left in the workspace.
static int salad_stage_aggregate(const SaladArgs& a, float dustbin, hipStream_t stream) {
  const float* S = reinterpret_cast<const float*>(a.ws + a.p.off_S);
  const float* F = reinterpret_cast<const float*>(a.ws + a.p.off_F);
  const float* g = reinterpret_cast<const float*>(a.ws + a.p.off_g);
  int* counters = (size_t)a.B * sizeof(int) <= SALAD_COUNTER_BYTES ? reinterpret_cast<int*>(a.ws + a.p.off_cnt) : nullptr;
  return salad_launch_aggregate(S, F, g, a.B, a.n, a.m, a.l, a.t, dustbin, a.sinkhorn_iters, a.out_f32, a.out_bf16, stream,
                                salad_slabs(a.n, a.C, a.m, a.l, a.hidden), (long long)a.B * a.n, counters);
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_salad_workspace_bytes(int B, int n, int C, int m, int l, int t, int hidden) {
  SaladPlan p;
  return salad_plan(B, n, C, m, l, t, hidden, &p) ? p.total : 0;
}

extern "C" int vpr_salad_sinkhorn_aggregate(const float* scores, const float* feats, const float* tokfeat,
                                            int B, int n, int m, int l, int t, float dustbin,
                                            int sinkhorn_iters, float* out_f32, uint16_t* out_bf16,
                                            void* stream) {
  return launch_sinkhorn_aggregate(scores, feats, tokfeat, B, n, m, l, t, dustbin, sinkhorn_iters,
                                   out_f32, out_bf16, static_cast<hipStream_t>(stream));
}

#ifdef VPR_ABLATION
// timing-only build: where the phase clocks of sinkhorn_aggregate_kernel go ([B][16] int64 on the device; null = off)
extern "C" int vpr_salad_sinkhorn_set_clocks(long long* clocks) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_sinkhorn_clocks), &clocks, sizeof(clocks)) == hipSuccess ? VPR_OK : VPR_ERR_LAUNCH;
}
#endif

extern "C" int vpr_salad_stage_token(const uint16_t* cls_tokens, long long cls_stride, int B, int n, int C,
                                     const vpr_salad_weights* w, int m, int l, int t, int hidden,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  SaladArgs a{B, n, C, m, l, t, hidden, w, cls_tokens, cls_stride};
  VPR_TRY_LAUNCH(salad_args(&a, SaladDomain::FixedN, STAGE_T, workspace, workspace_bytes));
  return salad_stage_token(a, static_cast<hipStream_t>(stream));
}

extern "C" int vpr_salad_stage_mlps(const uint16_t* patch_tokens, long long patch_img_stride, int B, int n, int C,
                                    const vpr_salad_weights* w, int m, int l, int t, int hidden,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  SaladArgs a{B, n, C, m, l, t, hidden, w};
  a.patch = patch_tokens, a.patch_img_stride = patch_img_stride;
  VPR_TRY_LAUNCH(salad_args(&a, SaladDomain::FixedN, STAGE_M, workspace, workspace_bytes));
  return salad_stage_mlps(a, static_cast<hipStream_t>(stream));
}

extern "C" int vpr_salad_stage_aggregate(int B, int n, int C, float dustbin, int m, int l, int t, int hidden,
                                         int sinkhorn_iters, float* out_f32, uint16_t* out_bf16,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  SaladArgs a{B, n, C, m, l, t, hidden};
  a.sinkhorn_iters = sinkhorn_iters, a.out_f32 = out_f32, a.out_bf16 = out_bf16;
  VPR_TRY_LAUNCH(salad_args(&a, SaladDomain::FixedN, STAGE_A, workspace, workspace_bytes));
  return salad_stage_aggregate(a, dustbin, static_cast<hipStream_t>(stream));
}

// include/vpr_amd_salad_stages.h: where stages T and M leave g, S, F (and, unfused, H) — the plan and the slab rule the
// stages themselves use, nothing else; no launch, no device access.
extern "C" int vpr_salad_stage_outputs(void* workspace, size_t workspace_bytes, int B, int n, int C, int m, int l, int t,
                                       int hidden, float** S, float** F, float** g, uint16_t** H, int* slabs,
                                       long long* slab_rows) {
  if (!S || !F || !g || !slabs || !slab_rows) return VPR_ERR_INVALID_ARG;
  SaladArgs a{B, n, C, m, l, t, hidden};
  VPR_TRY_LAUNCH(salad_args(&a, SaladDomain::FixedN, 0, workspace, workspace_bytes));
  *S = reinterpret_cast<float*>(a.ws + a.p.off_S);
  *F = reinterpret_cast<float*>(a.ws + a.p.off_F);
  *g = reinterpret_cast<float*>(a.ws + a.p.off_g);
  if (H) *H = reinterpret_cast<uint16_t*>(a.ws + a.p.off_H);
  *slabs = salad_slabs(n, C, m, l, hidden);
  *slab_rows = (long long)B * n;
  return VPR_OK;
}

// The whole aggregation in one stream.  patch row r of image b at patch + b*patch_img_stride + r*C; cls token of image b at
// cls + b*cls_stride.  A whole call names a null operand ahead of its shape (a stage call: after the workspace size).
static int salad_run(SaladDomain domain, const uint16_t* patch, long long patch_img_stride, const uint16_t* cls, long long cls_stride,
                     int B, int n, int C, const vpr_salad_weights* w, float dustbin, int m, int l, int t, int hidden,
                     int sinkhorn_iters, float* out_f32, uint16_t* out_bf16, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!patch || !cls || !out_f32) return VPR_ERR_INVALID_ARG;
  SaladArgs a{B, n, C, m, l, t, hidden, w, cls, cls_stride, patch, patch_img_stride, sinkhorn_iters, out_f32, out_bf16};
  VPR_TRY_LAUNCH(salad_args(&a, domain, STAGE_ALL, workspace, workspace_bytes));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  VPR_TRY_LAUNCH(salad_stage_token(a, stream));
  VPR_TRY_LAUNCH(salad_stage_mlps(a, stream));
  return salad_stage_aggregate(a, dustbin, stream);
}

extern "C" int vpr_salad_aggregate(const uint16_t* tokens, int B, int tokens_per_image, int C,
                                   const vpr_salad_weights* w, float dustbin,
                                   int m, int l, int t, int hidden, int sinkhorn_iters,
                                   float* out_f32, uint16_t* out_bf16,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!tokens || tokens_per_image < 2 || C <= 0) return VPR_ERR_INVALID_ARG;
  const long long img_stride = (long long)tokens_per_image * C;
  return salad_run(SaladDomain::FixedN, tokens + C, img_stride, tokens, img_stride, B, tokens_per_image - 1, C, w, dustbin, m, l, t,
                   hidden, sinkhorn_iters, out_f32, out_bf16, workspace, workspace_bytes, stream);
}

extern "C" int vpr_salad_aggregate_split(const uint16_t* patch_tokens, const uint16_t* cls_tokens, int B,
                                         int patches_per_image, int C,
                                         const vpr_salad_weights* w, float dustbin,
                                         int m, int l, int t, int hidden, int sinkhorn_iters,
                                         float* out_f32, uint16_t* out_bf16,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  if (patches_per_image < 1 || C <= 0) return VPR_ERR_INVALID_ARG;
  return salad_run(SaladDomain::FixedN, patch_tokens, (long long)patches_per_image * C, cls_tokens, C, B, patches_per_image, C, w,
                   dustbin, m, l, t, hidden, sinkhorn_iters, out_f32, out_bf16, workspace, workspace_bytes, stream);
}

// include/vpr_amd_salad_anyres.h: the same run in the any-n domain.  n == 256 takes the stages of vpr_salad_aggregate_split
// (the same bits); any other n the unfused stage M (salad_slabs() is 1 off n == 256) and the run-time-n stage A.
extern "C" int vpr_salad_aggregate_n(const uint16_t* patch, long long patch_img_stride, const uint16_t* cls, long long cls_stride,
                                     int B, int n, int C, const vpr_salad_weights* w, float dustbin,
                                     int m, int l, int t, int hidden, int sinkhorn_iters,
                                     float* out_f32, uint16_t* out_bf16,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return salad_run(SaladDomain::AnyN, patch, patch_img_stride, cls, cls_stride, B, n, C, w, dustbin, m, l, t, hidden, sinkhorn_iters,
                   out_f32, out_bf16, workspace, workspace_bytes, stream);
}

// include/vpr_amd_salad_hires.h: the same run for 64 < n <= 1369.  salad_launch_aggregate() chooses stage A by n, so n == 256 and
// every other n <= 576 are the calls above, bit for bit; above 576 tokens the unfused stage M feeds the high-resolution stage A.
extern "C" int vpr_salad_aggregate_hires(const uint16_t* patch, long long patch_img_stride, const uint16_t* cls, long long cls_stride,
                                         int B, int n, int C, const vpr_salad_weights* w, float dustbin,
                                         int m, int l, int t, int hidden, int sinkhorn_iters,
                                         float* out_f32, uint16_t* out_bf16,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return salad_run(SaladDomain::HiRes, patch, patch_img_stride, cls, cls_stride, B, n, C, w, dustbin, m, l, t, hidden, sinkhorn_iters,
                   out_f32, out_bf16, workspace, workspace_bytes, stream);
}

// Train mode (include/vpr_amd.h, vpr_salad_aggregate_train): the hub model's Dropout layers of score / cluster_features
// active — on the fused route only, which salad_args() insists on; stages T and A are those of the eval form.
extern "C" int vpr_salad_aggregate_train(const uint16_t* patch, long long patch_img_stride, const uint16_t* cls,
                                         long long cls_stride, int B, int n, int C, const vpr_salad_weights* w, float dustbin,
                                         int m, int l, int t, int hidden, int sinkhorn_iters, double dropout_p, uint64_t seed,
                                         uint32_t pass, long long image_base, float* out_f32, uint16_t* out_bf16,
                                         uint8_t* mask_out, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!(dropout_p >= 0.0 && dropout_p < 1.0)) return VPR_ERR_INVALID_ARG;          // NaN fails both comparisons
  if (image_base < 0 || B <= 0 || image_base + B > (1LL << 32)) return VPR_ERR_INVALID_ARG;
  if (!patch || !cls || !out_f32) return VPR_ERR_INVALID_ARG;
  SaladArgs a{B, n, C, m, l, t, hidden, w, cls, cls_stride, patch, patch_img_stride, sinkhorn_iters, out_f32, out_bf16};
  a.train = true, a.mask_out = mask_out;
  VPR_TRY_LAUNCH(salad_args(&a, SaladDomain::FixedN, STAGE_ALL, workspace, workspace_bytes));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const Fuse2Drop d{(uint32_t)floor(dropout_p * 4294967296.0) /* p * 2^32 < 2^32: fits */, (uint32_t)(seed & 0xffffffffu),
                    (uint32_t)(seed >> 32), pass, (uint32_t)image_base, (float)(1.0 / (1.0 - dropout_p)), mask_out};
  const bool drop = dropout_p > 0.0 || mask_out != nullptr;      // p = 0 without a mask: the eval kernel (the same bits)
  VPR_TRY_LAUNCH(salad_stage_mlps(a, stream, drop ? &d : nullptr));
  VPR_TRY_LAUNCH(salad_stage_token(a, stream));
  return salad_stage_aggregate(a, dustbin, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// f32-accurate SALAD (the reference runs the extractor and the aggregator in fp32: dinov2salad_validation.py:65-66,80-81,
// `.cuda()` with no cast).  f32 tokens and f32 weights; every linear layer is computed to f32 accuracy on the bf16 matrix
// pipe by splitting BOTH operands into three bf16 planes, x = h + m + l exactly (8 + 8 + 8 mantissa bits), and keeping the
// six products whose magnitude is above 2^-24 of the leading one:  (l,h) (h,l) (m,m) (m,h) (h,m) (h,h)  — the dropped
// ones (m·l, l·m, l·l) are below 2^-26 relative.  bf16 x bf16 products are exact in f32 and the MFMA accumulates in f32,
// so one ordinary bf16 GEMM over a K axis of 6 x K, smallest terms first, IS the f32 GEMM (error = f32 accumulation
// order, as in any f32 GEMM).  Hidden activations stay f32 and are split again for the second layers: no bf16 rounding
// point anywhere between the tokens and the descriptor.  ~6x the MFMA work of the bf16 stage: a precision mode for
// reference-parity runs (evaluate.*(dtype=torch.float32)), not the benchmark path.
namespace vpr {

// role 0 = activation operand: planes (l, h, m, m, h, h); role 1 = weight operand: planes (h, l, m, h, m, h)
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ src, long long rows, int K, long long ld_src,
                                                     int group_rows, long long group_stride,
                                                     uint16_t* __restrict__ dst, long long ld_dst, int role) {
  const int k4n = K >> 2;
  const long long total = rows * k4n;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / k4n;
    const int k = (int)(i - r * k4n) << 2;
    const float* sp = group_rows > 0 ? src + (r / group_rows) * group_stride + (r % group_rows) * ld_src + k
                                     : src + r * ld_src + k;
    const float4 v = *reinterpret_cast<const float4*>(sp);
    const float x[4] = {v.x, v.y, v.z, v.w};
    ushort4 pl[3];
    uint16_t* ph = reinterpret_cast<uint16_t*>(&pl[0]);
    uint16_t* pm = reinterpret_cast<uint16_t*>(&pl[1]);
    uint16_t* pq = reinterpret_cast<uint16_t*>(&pl[2]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint16_t h = f32_to_bf16_bits(x[e]);
      const float r1 = x[e] - bf16_bits_to_f32(h);          // exact
      const uint16_t m = f32_to_bf16_bits(r1);
      const float r2 = r1 - bf16_bits_to_f32(m);            // exact
      ph[e] = h; pm[e] = m; pq[e] = f32_to_bf16_bits(r2);
    }
    uint16_t* dp = dst + r * ld_dst + k;
    const int order_a[6] = {2, 0, 1, 1, 0, 0}, order_w[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int p = 0; p < 6; ++p)
      *reinterpret_cast<ushort4*>(dp + (long long)p * K) = pl[role ? order_w[p] : order_a[p]];
  }
}

static int launch_split3(const float* src, long long rows, int K, long long ld_src, int group_rows, long long group_stride,
                         uint16_t* dst, long long ld_dst, int role, hipStream_t stream) {
  if (rows <= 0) return VPR_OK;
  long long blocks = (rows * (K >> 2) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  VPR_TRY_LAUNCH(launch_kernel(split3_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, rows, K, ld_src, group_rows,
                               group_stride, dst, ld_dst, role));
  return VPR_OK;
}

struct SaladF32Plan {
  size_t off_A1, off_W1, off_H, off_H2, off_W2s, off_W2c, off_cls, off_W1t, off_Ht, off_Ht2, off_W2t, off_S, off_F, off_g, total;
};
static bool salad_f32_plan(int B, int n, int C, int m, int l, int t, int hidden, SaladF32Plan* p) {
  if (B <= 0 || n <= 0 || C <= 0 || m <= 0 || l <= 0 || t <= 0 || hidden <= 0) return false;
  const size_t rows = (size_t)B * n;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  p->off_A1 = take(rows * 6 * C * 2);
  p->off_W1 = take((size_t)2 * hidden * 6 * C * 2);
  p->off_H = take(rows * 2 * hidden * 4);
  p->off_H2 = take(rows * 12 * hidden * 2);
  p->off_W2s = take((size_t)m * 6 * hidden * 2);
  p->off_W2c = take((size_t)l * 6 * hidden * 2);
  p->off_cls = take((size_t)B * 6 * C * 2);
  p->off_W1t = take((size_t)hidden * 6 * C * 2);
  p->off_Ht = take((size_t)B * hidden * 4);
  p->off_Ht2 = take((size_t)B * 6 * hidden * 2);
  p->off_W2t = take((size_t)t * 6 * hidden * 2);
  p->off_S = take(rows * m * 4);
  p->off_F = take(rows * l * 4);
  p->off_g = take((size_t)B * t * 4);
  p->total = off;
  return true;
}

// The buffers of a plan inside a workspace: what salad_f32_run() writes and vpr_salad_f32_stage_outputs() names.
struct SaladF32Buffers {
  uint16_t *A1, *W1, *H2, *W2s, *W2c, *cls3, *W1t, *Ht2, *W2t;
  float *H, *Ht, *S, *F, *g;
};
static SaladF32Buffers salad_f32_buffers(void* workspace, const SaladF32Plan& p) {
  char* ws = static_cast<char*>(workspace);
  auto u16 = [&](size_t off) { return reinterpret_cast<uint16_t*>(ws + off); };
  auto f32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
  return {u16(p.off_A1), u16(p.off_W1), u16(p.off_H2), u16(p.off_W2s), u16(p.off_W2c), u16(p.off_cls), u16(p.off_W1t),
          u16(p.off_Ht2), u16(p.off_W2t), f32(p.off_H), f32(p.off_Ht), f32(p.off_S), f32(p.off_F), f32(p.off_g)};
}

}  // namespace vpr

extern "C" size_t vpr_salad_f32_workspace_bytes(int B, int n, int C, int m, int l, int t, int hidden) {
  SaladF32Plan p;
  return salad_f32_plan(B, n, C, m, l, t, hidden, &p) ? p.total : 0;
}

// Every refusal comes before the first launch, in the order of salad_args(); the f32 forms always put alignment ahead of
// WORKSPACE.  Stage A is salad_launch_aggregate()'s choice: one dense slab, no counters.
static int salad_f32_run(SaladDomain domain, const float* patch, long long patch_img_stride, const float* cls, long long cls_stride,
                         int B, int n, int C, const vpr_salad_weights_f32* w, float dustbin, int m, int l, int t, int hidden,
                         int sinkhorn_iters, float* out_f32, uint16_t* out_bf16, void* workspace, size_t workspace_bytes, void* stream_) {
  if (domain != SaladDomain::FixedN && sinkhorn_iters < 1) return VPR_ERR_INVALID_ARG;
  if (!patch || !cls || !out_f32 || !workspace || B <= 0 || n < 1 || C <= 0) return VPR_ERR_INVALID_ARG;
  if (!salad_weights_complete(w)) return VPR_ERR_INVALID_ARG;
  if (!salad_in_domain(domain, n, m, l, t, C, hidden)) return VPR_ERR_UNSUPPORTED;
  if ((patch_img_stride % 4) || (cls_stride % 4) || patch_img_stride < (long long)n * C || cls_stride < C) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(patch) || !aligned16(cls) || !aligned16(w->w1_sc) || !aligned16(w->w2_s) || !aligned16(w->w2_c) ||
      !aligned16(w->w1_t) || !aligned16(w->w2_t) || !aligned16(workspace))
    return VPR_ERR_UNSUPPORTED;
  SaladF32Plan p;
  if (!salad_f32_plan(B, n, C, m, l, t, hidden, &p)) return VPR_ERR_INVALID_ARG;
  if (workspace_bytes < p.total) return VPR_ERR_WORKSPACE;
  if (sinkhorn_iters < 1) return VPR_ERR_INVALID_ARG;
  if (n != SA_N && (!aligned4(out_f32) || (reinterpret_cast<uintptr_t>(out_bf16) & 1))) return VPR_ERR_UNSUPPORTED;   // the run-time-n kernels'
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SaladF32Buffers b = salad_f32_buffers(workspace, p);
  uint16_t *A1 = b.A1, *W1 = b.W1, *H2 = b.H2, *W2s = b.W2s, *W2c = b.W2c, *cls3 = b.cls3, *W1t = b.W1t, *Ht2 = b.Ht2, *W2t = b.W2t;
  float *H = b.H, *Ht = b.Ht, *S = b.S, *F = b.F, *g = b.g;
  const long long rows = (long long)B * n;
  const int K1 = 6 * C, K2 = 6 * hidden;
  // operand planes: tokens (row-group addressing resolved here, A1 is dense), cls rows, all five weight matrices
  VPR_TRY_LAUNCH(launch_split3(patch, rows, C, C, n, patch_img_stride, A1, K1, 0, stream));
  VPR_TRY_LAUNCH(launch_split3(cls, B, C, cls_stride, 0, 0, cls3, K1, 0, stream));
  VPR_TRY_LAUNCH(launch_split3(w->w1_sc, 2 * hidden, C, C, 0, 0, W1, K1, 1, stream));
  VPR_TRY_LAUNCH(launch_split3(w->w1_t, hidden, C, C, 0, 0, W1t, K1, 1, stream));
  VPR_TRY_LAUNCH(launch_split3(w->w2_s, m, hidden, hidden, 0, 0, W2s, K2, 1, stream));
  VPR_TRY_LAUNCH(launch_split3(w->w2_c, l, hidden, hidden, 0, 0, W2c, K2, 1, stream));
  VPR_TRY_LAUNCH(launch_split3(w->w2_t, t, hidden, hidden, 0, 0, W2t, K2, 1, stream));
  // layer 1 (f32 out, bias + ReLU in the epilogue)
  const GemmProblem l1_sc = gemm_problem(A1, K1, W1, K1, w->b1_sc, 1, H, 2 * hidden, 0, (int)rows, 2 * hidden, K1);
  int st = launch_gemm256(l1_sc, false, stream);
  if (st == VPR_ERR_UNSUPPORTED) st = launch_gemm_nt_group(&l1_sc, 1, stream);
  if (st != VPR_OK) return st;
  const GemmProblem l1_t = gemm_problem(cls3, K1, W1t, K1, w->b1_t, 1, Ht, hidden, 0, B, hidden, K1);
  VPR_TRY_LAUNCH(launch_gemm_nt_group(&l1_t, 1, stream));
  // hidden activations: f32 -> planes ([score 6h | cluster 6h] per row)
  VPR_TRY_LAUNCH(launch_split3(H, rows, hidden, 2 * hidden, 0, 0, H2, 2 * K2, 0, stream));
  VPR_TRY_LAUNCH(launch_split3(H + hidden, rows, hidden, 2 * hidden, 0, 0, H2 + K2, 2 * K2, 0, stream));
  VPR_TRY_LAUNCH(launch_split3(Ht, B, hidden, hidden, 0, 0, Ht2, K2, 0, stream));
  const GemmProblem l2[3] = {
      gemm_problem(H2, 2 * K2, W2s, K2, w->b2_s, 0, S, m, 0, (int)rows, m, K2),
      gemm_problem(H2 + K2, 2 * K2, W2c, K2, w->b2_c, 0, F, l, 0, (int)rows, l, K2),
      gemm_problem(Ht2, K2, W2t, K2, w->b2_t, 0, g, t, 0, B, t, K2)};
  VPR_TRY_LAUNCH(launch_gemm_nt_group(l2, 3, stream));
  return salad_launch_aggregate(S, F, g, B, n, m, l, t, dustbin, sinkhorn_iters, out_f32, out_bf16, stream, 1, 0, nullptr);
}

extern "C" int vpr_salad_aggregate_f32(const float* patch, long long patch_img_stride, const float* cls, long long cls_stride,
                                       int B, int n, int C, const vpr_salad_weights_f32* w, float dustbin,
                                       int m, int l, int t, int hidden, int sinkhorn_iters,
                                       float* out_f32, uint16_t* out_bf16,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return salad_f32_run(SaladDomain::FixedN, patch, patch_img_stride, cls, cls_stride, B, n, C, w, dustbin, m, l, t, hidden,
                       sinkhorn_iters, out_f32, out_bf16, workspace, workspace_bytes, stream);
}

extern "C" int vpr_salad_aggregate_f32_n(const float* patch, long long patch_img_stride, const float* cls, long long cls_stride,
                                         int B, int n, int C, const vpr_salad_weights_f32* w, float dustbin,
                                         int m, int l, int t, int hidden, int sinkhorn_iters,
                                         float* out_f32, uint16_t* out_bf16,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return salad_f32_run(SaladDomain::AnyN, patch, patch_img_stride, cls, cls_stride, B, n, C, w, dustbin, m, l, t, hidden,
                       sinkhorn_iters, out_f32, out_bf16, workspace, workspace_bytes, stream);
}

extern "C" int vpr_salad_aggregate_f32_hires(const float* patch, long long patch_img_stride, const float* cls, long long cls_stride,
                                             int B, int n, int C, const vpr_salad_weights_f32* w, float dustbin,
                                             int m, int l, int t, int hidden, int sinkhorn_iters,
                                             float* out_f32, uint16_t* out_bf16,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  return salad_f32_run(SaladDomain::HiRes, patch, patch_img_stride, cls, cls_stride, B, n, C, w, dustbin, m, l, t, hidden,
                       sinkhorn_iters, out_f32, out_bf16, workspace, workspace_bytes, stream);
}

// include/vpr_amd_salad_f32_stages.h: where salad_f32_run() leaves its planes, hidden values and stage-A operands — the
// plan it runs on, nothing else; no launch, no device access.  The refusals salad_f32_run() makes on these arguments, in its
// order, in the widest of its three domains (n == 256 and the any-n range lie inside the high-resolution one).
extern "C" int vpr_salad_f32_stage_outputs(void* workspace, size_t workspace_bytes, int B, int n, int C, int m, int l, int t,
                                           int hidden, float** H, float** Ht, float** S, float** F, float** g,
                                           uint16_t** A1, uint16_t** cls3, uint16_t** W1, uint16_t** H2,
                                           uint16_t** W1t, uint16_t** W2s, uint16_t** W2c, uint16_t** W2t, uint16_t** Ht2) {
  if (!H || !Ht || !S || !F || !g || !A1 || !cls3 || !W1 || !H2) return VPR_ERR_INVALID_ARG;
  if (!workspace || B <= 0 || n < 1 || C <= 0) return VPR_ERR_INVALID_ARG;
  if (!salad_in_domain(SaladDomain::HiRes, n, m, l, t, C, hidden)) return VPR_ERR_UNSUPPORTED;
  if (!aligned16(workspace)) return VPR_ERR_UNSUPPORTED;
  SaladF32Plan p;
  if (!salad_f32_plan(B, n, C, m, l, t, hidden, &p)) return VPR_ERR_INVALID_ARG;
  if (workspace_bytes < p.total) return VPR_ERR_WORKSPACE;
  const SaladF32Buffers b = salad_f32_buffers(workspace, p);
  *H = b.H, *Ht = b.Ht, *S = b.S, *F = b.F, *g = b.g;
  *A1 = b.A1, *cls3 = b.cls3, *W1 = b.W1, *H2 = b.H2;
  if (W1t) *W1t = b.W1t;
  if (W2s) *W2s = b.W2s;
  if (W2c) *W2c = b.W2c;
  if (W2t) *W2t = b.W2t;
  if (Ht2) *Ht2 = b.Ht2;
  return VPR_OK;
}
