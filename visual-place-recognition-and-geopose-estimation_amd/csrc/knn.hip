// knn.hip — cosine top-k of bf16 descriptors against a gallery shard.
//
// The reference has no retrieval code; this is the north-star stage that sits between the
// SALAD descriptor (dinov2salad/dinov2salad_validation.py:51) and post-processing (:84).
//
// Pipeline (all on one stream, no host sync):
//   1. knn_scores_kernel   S[b,n] = <q_b, g_n>   — HBM-bound stream of the gallery, MFMA
//                          (v_mfma_f32_16x16x32_bf16) used only because a 64-query tile needs
//                          64 FLOP per gallery byte.  THE dominant kernel (roofline: HBM).
//   2. knn_select_kernel   per (query, 4096-score chunk): top-KP candidates by the MFMA score
//                          (KP = oversampled k), repeated until one chunk is left -> [B][KP].
//   3. knn_rescore_kernel  per (query, candidate): EXACT rescoring of the KP rows (bf16 products
//                          accumulated in f64, fixed order);  knn_order_kernel: final ordering
//                          by (f32(score) desc, index asc), write top-k.
// The exact rescoring makes the result independent of MFMA accumulation order: indices are
// bit-exact against oracle/knn.py as long as the true top-k lie inside the approximate top-KP
// (MFMA f32 error ~1e-6 vs. the k-th..KP-th score gap).
#include <math.h>
#include <stdlib.h>
#include "vpr_common.h"
#include "vpr_internal.h"

namespace vpr {

constexpr int KNN_QT = 64;         // queries per tile (4 waves x 16)
constexpr int KNN_CHUNK = 4096;    // candidates per workgroup of the register-held select levels
constexpr int KNN_STREAM_CHUNK = 8192;   // scores per workgroup of the streaming level-0 select

__host__ __device__ inline int knn_kp(int k) {
  int kp = 2 * k > k + 8 ? 2 * k : k + 8;
  return (kp + 7) / 8 * 8;
}

// ---------------------------------------------------------------------------------------------
// 1. score kernel.  Workgroup w owns gallery rows [N*w/nwg, N*(w+1)/nwg) — a balanced static
// partition over a grid that is fully resident (nwg <= CUs * WGPC), so every workgroup
// streams the same number of HBM bytes and they finish together; its rows are cut into equal
// tiles of <= KNN_TR rows.  Per tile and K-step (128 B of every row = 64 bf16 or 128 fp8): the
// gallery tile [th x 128 B] (HBM) and the query tile [64 x 128 B] (L2) land in LDS by LDS-DMA,
// 2-deep ring, one barrier per K-step.  Wave w multiplies queries 16w..16w+15 (MFMA A operand)
// with every 16-row gallery block (B operand): C[q][n], lane = gallery row n -> coalesced 64-B
// score stores.
// FP8 (OCP e4m3, per-row f32 scale): same LDS image and the same 16-B fragment reads; a lane's two
// 16-B chunks are the 32-byte operand of ONE block-scaled MFMA over the whole 128-byte K-step
// (mfma_e4m3_16x16x128 of vpr_common.h: twice the rate of the four v_mfma_f32_16x16x32_fp8_fp8 it
// replaced) — A and B use the same lane -> K assignment, so the permutation cancels in the dot
// product — and the epilogue multiplies by the two row scales.
// ---------------------------------------------------------------------------------------------
template <bool FP8, int KNN_TR, int WGPC, int ABL>
__global__ __launch_bounds__(256, WGPC) void knn_scores_kernel(
    const void* __restrict__ Qv, const void* __restrict__ Gv, const float* __restrict__ q_scale,
    const float* __restrict__ g_scale, float* __restrict__ S, int B, int N, int row_bytes, int ldS) {
  constexpr int NB = KNN_TR / 16;
  constexpr int GG = KNN_TR / 8;            // gallery staging groups (8 rows each)
  constexpr int NGRP = GG + KNN_QT / 8;     // + query staging groups
  constexpr int GPW = (NGRP + 3) / 4;       // groups per wave (upper bound)
  constexpr int STAGE_BYTES = (KNN_TR + KNN_QT) * TILE_ROW_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const char* Q = static_cast<const char*>(Qv);
  const char* G = static_cast<const char*>(Gv);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwg = gridDim.x;
  const int qb = blockIdx.y;
  // balanced static partition in units of 4 rows (16-byte aligned score-row segments for the epilogue's float4 stores)
  const long long n4 = ((long long)N + 3) >> 2;
  const long long r_begin = 4 * (n4 * blockIdx.x / nwg);
  const long long r_end = min((long long)N, 4 * (n4 * (blockIdx.x + 1) / nwg));
  const int len = (int)(r_end - r_begin);
  if (len <= 0) return;
  const int ntile = (len + KNN_TR - 1) / KNN_TR;
  const int th_nom = ((len + ntile - 1) / ntile + 3) & ~3;      // <= KNN_TR (a multiple of 16)
  // K slice of this workgroup (small shards: gridDim.z > 1 slices, each into its own score slab, summed by the
  // level-0 select in slice order — see knn_ksplit)
  const int nk_all = row_bytes >> 7;
  const int k_lo = (int)((long long)nk_all * blockIdx.z / gridDim.z), k_hi = (int)((long long)nk_all * (blockIdx.z + 1) / gridDim.z);
  const int nk = k_hi - k_lo;
  Q += (long long)k_lo * 128;
  G += (long long)k_lo * 128;
  S += (long long)blockIdx.z * B * ldS;

  for (int t = 0; t < ntile; ++t) {
    const int row0 = (int)r_begin + t * th_nom;
    const int th = min(th_nom, (int)r_end - row0);   // valid rows of this tile
    if (th <= 0) break;                              // uniform; only for absurdly long row ranges

    // Source row pointers (bytes) of the staging groups this wave owns.
    const char* src[GPW];
#pragma unroll
    for (int i = 0; i < GPW; ++i) {
      const int g = wave + 4 * i;
      const int tr = (g < GG ? g : g - GG) * 8 + (lane >> 3);   // row inside its tile
      const int sw = stage_src_off(tr, lane);
      if (g < GG) {
        const int r = row0 + min(tr, th - 1);
        src[i] = G + (long long)r * row_bytes + sw;
      } else {
        const int r = min(qb * KNN_QT + tr, B - 1);
        src[i] = Q + (long long)r * row_bytes + sw;
      }
    }
    const int gvalid = (th + 7) >> 3;   // gallery groups that hold at least one valid row

    auto stage = [&](int buf, int ks) {
      char* base = smem + buf * STAGE_BYTES;
#pragma unroll
      for (int i = 0; i < GPW; ++i) {
        const int g = wave + 4 * i;
        if (g < GG) {
          if (g < gvalid) glds16<(ABL & 4) ? 2 : 0>(src[i] + ks * 128, base + g * 8 * TILE_ROW_BYTES);
        } else if (g < NGRP) {
          if (!(ABL & 2) || ks == 0)
            glds16(src[i] + ks * 128, base + KNN_TR * TILE_ROW_BYTES + (g - GG) * 8 * TILE_ROW_BYTES);
        }
      }
    };

    f32x4 acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    __syncthreads();   // previous tile's last compute is done before its buffers are refilled
    stage(0, 0);
    for (int ks = 0; ks < nk; ++ks) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (ks + 1 < nk) stage((ks + 1) & 1, ks + 1);
      const char* tg = smem + (ks & 1) * STAGE_BYTES;
      const char* tq = tg + KNN_TR * TILE_ROW_BYTES;
      const bf16x8 a0 = lds_frag(tq, 16 * wave + (lane & 15), (lane >> 4));
      const bf16x8 a1 = lds_frag(tq, 16 * wave + (lane & 15), 4 + (lane >> 4));
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if ((ABL & 1) && ks > 0) break;
        if (nb * 16 < th) {
          const bf16x8 b0 = lds_frag(tg, 16 * nb + (lane & 15), (lane >> 4));
          const bf16x8 b1 = lds_frag(tg, 16 * nb + (lane & 15), 4 + (lane >> 4));
          if constexpr (FP8) {
            acc[nb] = mfma_e4m3_16x16x128(e4m3_operand(a0, a1), e4m3_operand(b0, b1), acc[nb]);
          } else {
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[nb], 0, 0, 0);
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[nb], 0, 0, 0);
          }
        }
      }
    }

    // C/D map of 16x16: col (gallery row) = lane&15, row (query) = 4*(lane>>4) + e.
    float qs[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (FP8) {
#pragma unroll
      for (int e = 0; e < 4; ++e) qs[e] = q_scale[min(qb * KNN_QT + 16 * wave + 4 * (lane >> 4) + e, B - 1)];
    }
    if constexpr (ABL & 32) {
      // Score tile out through the (now idle) stage buffers as whole row segments: wave w owns query rows 16w..16w+15
      // of the tile on both sides, so only the first barrier (every wave is past its last operand read) is needed.
      // Pitch KNN_TR + 4 floats: the four query groups of a store land 16 banks apart (conflict-free), rows stay
      // 16-byte aligned.  One 1-KiB float4 store per query row instead of 16 dword stores of four 64-byte segments.
      constexpr int SP = KNN_TR + 4;
      static_assert(KNN_QT * SP * 4 <= 2 * STAGE_BYTES, "score tile must fit the stage buffers");
      float* st = reinterpret_cast<float*>(smem);
      __syncthreads();
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int n = 16 * nb + (lane & 15);
        if (n < th) {
          float gs = 1.f;
          if constexpr (FP8) gs = g_scale[row0 + n];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            st[(16 * wave + 4 * (lane >> 4) + e) * SP + n] = FP8 ? acc[nb][e] * qs[e] * gs : acc[nb][e];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      for (int j = 0; j < 16; ++j) {
        const int q = qb * KNN_QT + 16 * wave + j;
        if (q >= B) break;
        float* dst = S + (long long)q * ldS + row0;
        const float* srow = st + (16 * wave + j) * SP;
        for (int c = lane * 4; c < th; c += 256) {
          if (c + 3 < th) {
            const f32x4 v4 = *reinterpret_cast<const f32x4*>(srow + c);
            if constexpr (ABL & 16) __builtin_nontemporal_store(v4, reinterpret_cast<f32x4*>(dst + c));
            else *reinterpret_cast<f32x4*>(dst + c) = v4;
          } else {
            for (int x = c; x < th; ++x) dst[x] = srow[x];
          }
        }
      }
    } else {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int n = 16 * nb + (lane & 15);
        if (n < th) {
          float gs = 1.f;
          if constexpr (FP8) gs = g_scale[row0 + n];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int q = qb * KNN_QT + 16 * wave + 4 * (lane >> 4) + e;
            // ABL bit 3 (value 8, -DVPR_ABLATION builds only): no score stores (the impossible compare keeps the MFMAs alive)
            if ((ABL & 8) && acc[nb][e] != 12345.678f) continue;
            const float val = FP8 ? acc[nb][e] * qs[e] * gs : acc[nb][e];
            if (q < B) {
              if constexpr (ABL & 16) __builtin_nontemporal_store(val, &S[(long long)q * ldS + row0 + n]);
              else S[(long long)q * ldS + row0 + n] = val;
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 2. Block-wide top-kp selection, shared by every select level, the fused final kernel and the shard merge.
// Key order: value desc, index asc (packed into one u64 so a max-reduction does both).
// ---------------------------------------------------------------------------------------------
// (the packed key itself — f32_orderable .. store_entry, KEY_DEAD — lives in vpr_common.h: rerank.hip orders by it too)
constexpr int SEL_CAP = 4096;                   // candidate list capacity of the register-held selects (= keys per block)

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, true);
  return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

// Top-kp of a block's unique keys without a serial argmax loop, in four steps:
//   a. publish   every group of G threads (G = 1, 2, 4) leaves the max of its keys in tmax;
//   b. threshold T = the kp-th largest published max (two forms below) is a lower bound of the kp-th largest key
//                overall, so every top-kp key is >= T;
//   c. filter    keys >= T are appended to the LDS list cand (typically kp..2kp of them);
//   d. rank      each listed key counts the listed keys above it = its rank; ranks < kp go to outk[rank].
// Invariants every step relies on:
//   - keys are unique (the index is part of the key), so exactly one published max has rank kp - 1: thr has one writer;
//   - thr == 1 means "no threshold" (fewer than kp live published maxes): 1 is below every real key and above
//     KEY_DEAD, so `key >= thr` then takes every live key and still drops the padding;
//   - KEY_DEAD sorts last, so it never outranks a real key and outk[0, kp) ends in the padding it was reset to.
template <int CAP, int NOUT>
struct SelectState {
  unsigned long long tmax[256];    // published maxes
  unsigned long long cand[CAP];    // keys >= thr, unordered
  unsigned long long outk[NOUT];   // the answer, rank-ordered, KEY_DEAD-padded
  unsigned long long thr;
  int cnt;                         // entries of cand
};

// Before the first barrier of a selection.  NT = threads of the block.
template <int NT, int CAP, int NOUT>
__device__ __forceinline__ void select_reset(SelectState<CAP, NOUT>& sm) {
  static_assert(NOUT <= NT, "one thread per output slot");
  if (threadIdx.x == 0) { sm.thr = 1ull; sm.cnt = 0; }
  if (threadIdx.x < NOUT) sm.outk[threadIdx.x] = KEY_DEAD;
}

// Step a: the max over each group of G adjacent lanes (DPP quad permutes) goes to tmax[tid / G].
template <int G, int CAP, int NOUT>
__device__ __forceinline__ void publish_max(SelectState<CAP, NOUT>& sm, unsigned long long best) {
  static_assert(G == 1 || G == 2 || G == 4, "a group lives inside one DPP quad");
  if constexpr (G >= 2) { const unsigned long long o = dpp_u64<0xB1>(best); best = o > best ? o : best; }
  if constexpr (G == 4) { const unsigned long long o = dpp_u64<0x4E>(best); best = o > best ? o : best; }
  if ((threadIdx.x & (G - 1)) == 0) sm.tmax[threadIdx.x / G] = best;
}

// Step b, all-pairs form: thread t < NPUB ranks tmax[t] against all NPUB published maxes.  Returns T to every thread.
template <int NPUB, int CAP, int NOUT>
__device__ __forceinline__ unsigned long long threshold_all_pairs(SelectState<CAP, NOUT>& sm, int kp) {
  __syncthreads();
  if (threadIdx.x < NPUB) {
    const unsigned long long mine = sm.tmax[threadIdx.x];
    int rank = 0;
    for (int s = 0; s < NPUB; s += 2) {
      const ulonglong2 t2 = *reinterpret_cast<const ulonglong2*>(&sm.tmax[s]);
      rank += (t2.x > mine ? 1 : 0) + (t2.y > mine ? 1 : 0);
    }
    if (rank == kp - 1 && mine != KEY_DEAD) sm.thr = mine;
  }
  __syncthreads();
  return sm.thr;
}

// Step b, wave-list form for 256 threads that each publish their own max `best`, without the 256 x 256 all-pairs
// ranking (VALU-bound: 100 us at 1M rows): rank inside the own wave (64 broadcast reads), the top kp of every wave go
// to a sorted list, and the global rank of a listed key = own rank + binary searches in the other three lists.
template <int CAP, int NOUT>
__device__ __forceinline__ unsigned long long threshold_wave_lists(SelectState<CAP, NOUT>& sm,
                                                                   unsigned long long (&wtop)[4][128],
                                                                   unsigned long long best, int kp) {
  const int tid = threadIdx.x, wv = tid >> 6;
  for (int i = tid; i < 4 * 128; i += 256) wtop[i >> 7][i & 127] = KEY_DEAD;
  publish_max<1>(sm, best);
  __syncthreads();
  int wr = 0;
  for (int s = 0; s < 64; s += 2) {
    const ulonglong2 t2 = *reinterpret_cast<const ulonglong2*>(&sm.tmax[wv * 64 + s]);
    wr += (t2.x > best ? 1 : 0) + (t2.y > best ? 1 : 0);
  }
  const bool listed = best != KEY_DEAD && wr < kp;
  if (listed) wtop[wv][wr] = best;
  __syncthreads();
  if (listed) {
    int gr = wr;
    for (int w2 = 0; w2 < 4; ++w2) {
      if (w2 == wv) continue;
      int lo = 0, hi = kp;                      // descending list, KEY_DEAD (= 0) padding at the end
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (wtop[w2][mid] > best) lo = mid + 1; else hi = mid;
      }
      gr += lo;
    }
    if (gr == kp - 1) sm.thr = best;
  }
  __syncthreads();
  return sm.thr;
}

// Step c over a thread's NSLOT slots: kept(i) says whether slot i reaches the threshold, key(i) is its key, asked for
// only then (a caller that holds scores, not keys, builds no key for a score that fails).
// Length of the list, whatever the data (ties, sorted input, all-equal scores): with m keys behind every published
// max, kp - 1 published maxes lie above T and their groups add at most m keys each; the group whose max is T adds
// that one key; every other group's keys are all below T.  So cnt <= m (kp - 1) + 1, and without a threshold
// (fewer than kp live groups) cnt <= m (kp - 1).  Every caller says why its CAP covers that.
// That argument needs kept() and the published maxes to follow ONE order; the slot test below does not: a key that
// finds the list full is dropped (cnt keeps counting, select_rank reads min(cnt, CAP)), so a threshold that is wrong
// for whatever reason costs an answer, never memory.
template <int NSLOT, int CAP, int NOUT, typename P, typename K>
__device__ __forceinline__ void select_filter(SelectState<CAP, NOUT>& sm, P&& kept, K&& key) {
#pragma unroll
  for (int i = 0; i < NSLOT; ++i)
    if (kept(i)) {
      const int slot = atomicAdd(&sm.cnt, 1);
      if (slot < CAP) sm.cand[slot] = key(i);
    }
}

// Step d.  outk[0, kp) is complete and visible to the whole block on return.
template <int NT, int CAP, int NOUT>
__device__ __forceinline__ void select_rank(SelectState<CAP, NOUT>& sm, int kp) {
  __syncthreads();
  const int c = sm.cnt < CAP ? sm.cnt : CAP;      // select_filter never writes past CAP
  for (int ci = threadIdx.x; ci < c; ci += NT) {
    const unsigned long long mine = sm.cand[ci];
    int r = 0;
    for (int cj = 0; cj < c; ++cj) r += sm.cand[cj] > mine ? 1 : 0;
    if (r < kp) sm.outk[r] = mine;
  }
  __syncthreads();
}

// All four steps for NT threads that hold NK keys each.  256 threads and kp <= 64: 64 quad maxes are enough to bound
// kp keys, and ranking 64 values is 4x cheaper than ranking 256; otherwise 256 maxes (of threads, or of thread pairs
// of a 512-thread block).
template <int NT, int NK, int CAP, int NOUT>
__device__ __forceinline__ void block_select(const unsigned long long (&keys)[NK], int kp, SelectState<CAP, NOUT>& sm) {
  static_assert(NT == 256 || NT == 512, "256 published maxes at most");
  static_assert(NT * NK <= CAP, "cand holds every key of the block, so no threshold can overflow it");
  unsigned long long best = keys[0];
#pragma unroll
  for (int i = 1; i < NK; ++i) best = keys[i] > best ? keys[i] : best;
  select_reset<NT>(sm);
  unsigned long long T;
  if (NT == 256 && kp <= 64) {
    publish_max<4>(sm, best);
    T = threshold_all_pairs<64>(sm, kp);
  } else {
    publish_max<NT / 256>(sm, best);
    T = threshold_all_pairs<256>(sm, kp);
  }
  select_filter<NK>(sm, [&](int i) { return keys[i] >= T; }, [&](int i) { return keys[i]; });
  select_rank<NT>(sm, kp);
}

// Branch-free load of up to 16 (value, index) pairs per thread (clamped position, see candidate_key).
__device__ __forceinline__ void load_keys(unsigned long long (&keys)[16], const float* __restrict__ v,
                                          const int32_t* __restrict__ ix, int L, int base) {
  if (ix != nullptr) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = base + i * 256 + (int)threadIdx.x;
      const int pc = p < L ? p : L - 1;
      const int id = ix[pc];
      keys[i] = candidate_key(v[pc], id, p < L);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = base + i * 256 + (int)threadIdx.x;
      keys[i] = candidate_key(v[p < L ? p : L - 1], p, p < L);
    }
  }
}

// 2. select: grid (chunks, B).  in_idx == nullptr -> index = position; else explicit.
// Output [B][nchunk][kp] (value, index), KEY_DEAD -> (-inf, -1).
__global__ __launch_bounds__(256) void knn_select_kernel(
    const float* __restrict__ in_val, const int32_t* __restrict__ in_idx, int L, long long ld_in,
    float* __restrict__ out_val, int32_t* __restrict__ out_idx, int kp, int nchunk) {
  __shared__ SelectState<SEL_CAP, 128> sm;
  const int c = blockIdx.x, b = blockIdx.y;
  const float* v = in_val + (long long)b * ld_in;
  const int32_t* ix = in_idx ? in_idx + (long long)b * ld_in : nullptr;
  unsigned long long keys[16];
  load_keys(keys, v, ix, L, c * KNN_CHUNK);
  block_select<256>(keys, kp, sm);
  if ((int)threadIdx.x < kp)
    store_entry(sm.outk[threadIdx.x], out_val, out_idx, ((long long)b * nchunk + c) * kp + threadIdx.x);
}

// Component e of a float4 by a compile-time-foldable select (keeps the vector in registers).
__device__ __forceinline__ float f4_at(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// 2a. level-0 select straight from the score matrix: grid (chunks, B), chunk = `ch` scores (multiple of 1024,
// <= 8192).  The chunk is read ONCE: every thread requests its (up to) 8 float4 (32 scores, strided by 1024 so a wave
// reads 1 KiB lines) before the first compare and keeps them in registers, as floats, for both passes over them:
//   max     the thread's best (value, then lower index) of its 32 scores, plain f32 compares in index-ascending
//           order (strict '>' keeps ties right); on scores with one zero (-0.0 read as +0.0) that is the key's order;
//   filter  a key is built only for a score that reaches the threshold (32 u64 keys would double the registers).
// The threshold is the wave-list form, the other steps are the shared ones.  m = 32 keys per published max, so the
// list holds at most 32 (kp - 1) + 1 keys: CAP = 1024 for kp <= 32 (k <= 16), 4096 otherwise (kp <= 128).
// Round 1 read the chunk twice with dependent loads (8 round trips per pass) under 35 KB of LDS (4 workgroups per CU):
// 15.7 us at 100k rows, 117 us at 1M; this form needs 15 KB (kp <= 32) and one round trip.
static_assert(32 * (32 - 1) + 1 <= 1024 && 32 * (128 - 1) + 1 <= 4096, "list bound of the streaming select");
template <int CAP>
__global__ __launch_bounds__(256) void knn_select_stream_kernel(
    const float* __restrict__ S, int N, long long ldS, int ch,
    float* __restrict__ out_val, int32_t* __restrict__ out_idx, int kp, int nchunk, int nslab, long long slab_stride) {
  __shared__ SelectState<CAP, 128> sm;
  __shared__ unsigned long long wtop[4][128];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* v = S + (long long)b * ldS;
  const int base = c * ch;
  const int len = min(ch, N - base);          // >= 1
  float4 q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = tid * 4 + i * 1024;
    // rows of S are padded to a multiple of 64 floats (ldS), so a float4 that starts inside the row stays inside it;
    // positions past `len` are masked below
    q[i] = p < len ? *reinterpret_cast<const float4*>(v + base + p) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // K-split shards (small N): the score is the sum of the slices' slabs, added in slice order (deterministic); the sum
  // goes back into slab 0 so that the workspace still holds THE score matrix afterwards (vpr_knn_scores_ptr)
  for (int z = 1; z < nslab; ++z) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int p = tid * 4 + i * 1024;
      if (p < len) {
        const float4 t = *reinterpret_cast<const float4*>(v + z * slab_stride + base + p);
        q[i].x += t.x; q[i].y += t.y; q[i].z += t.z; q[i].w += t.w;
      }
    }
  }
  // -0.0 counts as +0.0 (x + 0.f): the max pass and the filter below compare plain floats, where the two zeros are
  // equal, while the packed key puts +0.0 above -0.0; with one zero both are the same order, which the list bound
  // needs (a chunk of mixed zeros otherwise passes thousands of -0.0 under a (+0.0, index) threshold)
#pragma unroll
  for (int i = 0; i < 8; ++i) { q[i].x += 0.f; q[i].y += 0.f; q[i].z += 0.f; q[i].w += 0.f; }
  if (nslab > 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int p = tid * 4 + i * 1024;
      if (p < len) *reinterpret_cast<float4*>(const_cast<float*>(v) + base + p) = q[i];
    }
  }
  float bv = -INFINITY;
  int bi = -1;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = tid * 4 + i * 1024;
    const float qq[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p + e < len && (qq[e] > bv || bi < 0)) { bv = qq[e]; bi = base + p + e; }
  }
  select_reset<256>(sm);
  const unsigned long long T = threshold_wave_lists(sm, wtop, candidate_key(bv, bi, true), kp);
  // key >= T  <=>  value > Tv, or value == Tv and index <= Ti  (T == 1: no threshold, take all)
  const bool all = T == 1ull;
  const float Tv = all ? -INFINITY : key_val(T);
  const int Ti = all ? 0x7fffffff : key_idx(T);
  // slot i of the thread = component i & 3 of q[i >> 2], at position pos(i) of the chunk
  const auto pos = [&](int i) { return tid * 4 + (i >> 2) * 1024 + (i & 3); };
  select_filter<32>(
      sm,
      [&](int i) {
        const float x = f4_at(q[i >> 2], i & 3);
        return pos(i) < len && (x > Tv || (x == Tv && base + pos(i) <= Ti) || all);
      },
      [&](int i) { return make_key(f4_at(q[i >> 2], i & 3), base + pos(i)); });
  select_rank<256>(sm, kp);
  if (tid < kp) store_entry(sm.outk[tid], out_val, out_idx, ((long long)b * nchunk + c) * kp + tid);
}

// ---------------------------------------------------------------------------------------------
// 3. Exact rescoring and certification.  One operand dispatch (bf16 / e4m3 16-B chunks), one finish of an exact
// score, one |q| and one certificate, shared by the split kernels, the fused kernel and the exhaustive fallback.
// ---------------------------------------------------------------------------------------------
// acc + <q, g> over one 16-B chunk of each operand, in f64: every product is exact.
template <bool FP8>
__device__ __forceinline__ double dot16(const s16x8& qa, const s16x8& ga, double acc) {
  if constexpr (FP8) {
    const i32x4 qi = __builtin_bit_cast(i32x4, qa), gi = __builtin_bit_cast(i32x4, ga);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      acc = fma((double)__builtin_amdgcn_cvt_f32_fp8(qi[w], 0), (double)__builtin_amdgcn_cvt_f32_fp8(gi[w], 0), acc);
      acc = fma((double)__builtin_amdgcn_cvt_f32_fp8(qi[w], 1), (double)__builtin_amdgcn_cvt_f32_fp8(gi[w], 1), acc);
      acc = fma((double)__builtin_amdgcn_cvt_f32_fp8(qi[w], 2), (double)__builtin_amdgcn_cvt_f32_fp8(gi[w], 2), acc);
      acc = fma((double)__builtin_amdgcn_cvt_f32_fp8(qi[w], 3), (double)__builtin_amdgcn_cvt_f32_fp8(gi[w], 3), acc);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc = fma((double)bf16_bits_to_f32((uint16_t)qa[j]), (double)bf16_bits_to_f32((uint16_t)ga[j]), acc);
  }
  return acc;
}

// Sum of squares of one 16-B operand chunk (f32; feeds the error bound of the certification step only).
template <bool FP8>
__device__ __forceinline__ float sumsq16(const s16x8& a) {
  float t = 0.f;
  if constexpr (FP8) {
    const i32x4 w = __builtin_bit_cast(i32x4, a);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float x = __builtin_amdgcn_cvt_f32_fp8(w[i], 0); t = fmaf(x, x, t);
      x = __builtin_amdgcn_cvt_f32_fp8(w[i], 1); t = fmaf(x, x, t);
      x = __builtin_amdgcn_cvt_f32_fp8(w[i], 2); t = fmaf(x, x, t);
      x = __builtin_amdgcn_cvt_f32_fp8(w[i], 3); t = fmaf(x, x, t);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float x = bf16_bits_to_f32((uint16_t)a[j]); t = fmaf(x, x, t); }
  }
  return t;
}

// The f32 scale of row i of an e4m3 operand; 1 for bf16 operands (null scale arrays) and for padding (i < 0).
template <bool FP8>
__device__ __forceinline__ float row_scale(const float* __restrict__ scale, long long i) {
  if constexpr (FP8) return i >= 0 ? scale[i] : 1.f;
  return 1.f;
}

// From the f64 sum of products to the score: scales in the order of oracle/knn.py, (tot * q_scale) * g_scale, then ONE
// rounding to f32.  Padding (id < 0) scores -inf.
template <bool FP8>
__device__ __forceinline__ float finish_exact(double tot, float q_scale, float g_scale, int id) {
  if constexpr (FP8) tot = (tot * (double)q_scale) * (double)g_scale;
  return id < 0 ? -INFINITY : (float)tot;
}

// |q| of the quantised query from the sum of squares of its stored elements.
__device__ __forceinline__ float query_norm(float sumsq, float q_scale) { return sqrtf(sumsq) * fabsf(q_scale); }

// Certification (the exactness contract, made checkable).  The result is the exact top-k iff no row OUTSIDE the
// rescored set has an exact score >= the k-th best exact score e_k of the set.  Every such row lost an
// approximate-score comparison: its MFMA score is <= a_min, the smallest approximate score kept (level-0 lists and
// the top-kp cut both keep the largest keys), and |MFMA score - exact score| <= eps = err_rel * |q| for gallery
// rows inside the norm bound the caller folded into err_rel (any summation order of D f32 additions of exact
// products: gamma_D * sum|q_i g_i| <= D 2^-24 |q| |g|).  So  e_k - eps > a_min  certifies the answer, and so does a
// list that is not full: nothing was cut.
// Otherwise the set is widened to every level-0 candidate with MFMA score >= e_k - eps (they are rescored exactly
// too, status 1); if a level-0 chunk list is itself cut above that bar (>= kp rows of one chunk inside the band),
// or the widened set does not fit, the query is flagged (status 2) and the host re-runs it on exact scores
// (vpr_knn_exact_scores): ops.knn_topk(..., exact_fallback=True).
__device__ __forceinline__ bool knn_certified(float e_k, float eps, bool list_full, float a_min) {
  return !list_full || e_k - eps > a_min;
}

// 3a. exact rescoring: grid (kp, B), one workgroup per (candidate, query).  cand_idx [B][kp] are
// the approximate top-kp gallery rows (-1 = padding).  exact score = sum of bf16*bf16 products
// in f64 (each product is exact), in a fixed order (thread-strided 16-B chunks in sequence, wave
// butterfly, then the 4 wave sums) -> independent of how the candidate was found.  All of a
// thread's loads are issued before the first FMA: one trip to HBM per row.
constexpr int RS_U = 6;   // 16-B chunks per thread per trip
template <bool FP8>
__global__ __launch_bounds__(256) void knn_rescore_kernel(
    const int32_t* __restrict__ cand_idx, const void* __restrict__ Qv, const void* __restrict__ Gv,
    const float* __restrict__ q_scale, const float* __restrict__ g_scale,
    int row_bytes, int kp, float* __restrict__ exact, float* __restrict__ qnorm) {
  __shared__ double red[4];
  __shared__ float redq[4];
  const int c = blockIdx.x, b = blockIdx.y;
  const int id = cand_idx[(long long)b * kp + c];
  if (id < 0 && c != 0) {   // uniform (candidate 0 always runs: it also leaves |q| for the certification step)
    if (threadIdx.x == 0) exact[(long long)b * kp + c] = -INFINITY;
    return;
  }
  const char* qrow = static_cast<const char*>(Qv) + (long long)b * row_bytes;
  const char* grow = static_cast<const char*>(Gv) + (long long)(id < 0 ? 0 : id) * row_bytes;
  const int nchunks = row_bytes >> 4;
  double acc = 0.0;
  float qq = 0.f;
  for (int ch0 = threadIdx.x; ch0 < nchunks; ch0 += 256 * RS_U) {
    s16x8 qa[RS_U], ga[RS_U];
#pragma unroll
    for (int u = 0; u < RS_U; ++u) {
      const int ch = ch0 + 256 * u;
      const int chc = ch < nchunks ? ch : ch0;          // clamp: always a valid address
      qa[u] = *reinterpret_cast<const s16x8*>(qrow + chc * 16);
      ga[u] = *reinterpret_cast<const s16x8*>(grow + chc * 16);
    }
#pragma unroll
    for (int u = 0; u < RS_U; ++u) {
      if (ch0 + 256 * u < nchunks) {
        acc = dot16<FP8>(qa[u], ga[u], acc);
        if (c == 0) qq += sumsq16<FP8>(qa[u]);
      }
    }
  }
  acc = wave_sum_f64(acc);
  qq = wave_sum(qq);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = acc; redq[threadIdx.x >> 6] = qq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = (red[0] + red[1]) + (red[2] + red[3]);
    exact[(long long)b * kp + c] = finish_exact<FP8>(tot, row_scale<FP8>(q_scale, b), row_scale<FP8>(g_scale, id), id);
    if (c == 0) qnorm[b] = query_norm((redq[0] + redq[1]) + (redq[2] + redq[3]), row_scale<FP8>(q_scale, b));
  }
}

// 3c. fused final stage: grid (B), 512 threads.  Takes the candidates of the last select level (<= 4096 per
// query), selects the top-kp by MFMA score, rescoring them exactly (8 waves, every load of a
// row issued before its first FMA, the query row staged once in LDS) and writes the ordered
// top-k — one launch instead of select + rescore + order.  Same arithmetic as the split kernels
// (same per-lane chunk order, same butterfly), so the results are bit-identical to them.
constexpr int FF_NT = 512;        // 8 waves
constexpr int FF_CPW = 3;         // candidates a wave rescoring together (all their loads in flight)
constexpr int FF_MAXCH = 9;       // 16-B chunks per lane per row in flight per trip
constexpr int FF_MAXC = 256;      // rescored candidates per query: kp + what the certification step adds
struct FinalSmem {
  SelectState<SEL_CAP, FF_MAXC> sel;
  float exact[FF_MAXC];
  float red[8];
  float ek;         // k-th best exact score of the rescored set
  int nvalid;       // real (non-padding) entries of the rescored set
  int extra;        // candidates the certification step adds
  int flag;         // 0 certified, 1 widen, 2 cannot be certified from the lists in hand
};

template <bool FP8>
__global__ __launch_bounds__(FF_NT) void knn_final_fused_kernel(
    const float* __restrict__ cand_val, const int32_t* __restrict__ cand_idx, int L,
    const void* __restrict__ Qv, const void* __restrict__ Gv, const float* __restrict__ q_scale,
    const float* __restrict__ g_scale, int row_bytes, int k, int kp, int index_base,
    float* __restrict__ out_val, int32_t* __restrict__ out_idx,
    float err_rel, int level0_lists, int32_t* __restrict__ status, int32_t* __restrict__ uncertified) {
  extern __shared__ __attribute__((aligned(16))) char dyn[];      // [row_bytes] query row
  __shared__ FinalSmem sm;
  unsigned long long (&outk)[FF_MAXC] = sm.sel.outk;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // stage the query row (16-B chunks); |q|^2 on the way
  const char* qrow = static_cast<const char*>(Qv) + (long long)b * row_bytes;
  const int nchunks = row_bytes >> 4;
  float qq = 0.f;
  for (int ch = tid; ch < nchunks; ch += FF_NT) {
    const s16x8 c16 = *reinterpret_cast<const s16x8*>(qrow + ch * 16);
    *reinterpret_cast<s16x8*>(dyn + ch * 16) = c16;
    qq += sumsq16<FP8>(c16);
  }
  qq = wave_sum(qq);
  if (lane == 0) sm.red[wave] = qq;

  // ---- top-kp of the candidates (8 keys per thread) ----
  unsigned long long keys[8];
  const float* v = cand_val + (long long)b * L;
  const int32_t* ix = cand_idx + (long long)b * L;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = i * FF_NT + tid;
    const int pc = p < L ? p : L - 1;
    const int id = ix[pc];
    keys[i] = candidate_key(v[pc], id, p < L);
  }
  if (tid == 0) { sm.extra = 0; sm.flag = 0; sm.nvalid = 0; sm.ek = -INFINITY; }
  block_select<FF_NT>(keys, kp, sm.sel);

  // ---- exact rescoring of outk[c_lo, c_hi): wave w takes candidates c_lo + w + 8*j; FF_CPW of them per trip, with
  // every 16-B chunk of all their rows requested before the first FMA (one HBM round trip per trip) ----
  auto rescore = [&](int c_lo, int c_hi) {
    for (int c0 = c_lo + wave; c0 < c_hi; c0 += 8 * FF_CPW) {
      int id[FF_CPW];
      const char* grow[FF_CPW];
      double acc[FF_CPW];
#pragma unroll
      for (int j = 0; j < FF_CPW; ++j) {
        const int c = c0 + 8 * j;
        const unsigned long long key = c < c_hi ? outk[c] : KEY_DEAD;
        id[j] = key == KEY_DEAD ? -1 : key_idx(key);
        grow[j] = static_cast<const char*>(Gv) + (long long)(id[j] < 0 ? 0 : id[j]) * row_bytes;
        acc[j] = 0.0;
      }
      for (int base = 0; base < nchunks; base += 64 * FF_MAXCH) {   // 2 trips at D = 8448
        s16x8 ga[FF_CPW][FF_MAXCH];
#pragma unroll
        for (int j = 0; j < FF_CPW; ++j)
#pragma unroll
          for (int u = 0; u < FF_MAXCH; ++u) {
            const int ch = base + lane + 64 * u;
            ga[j][u] = *reinterpret_cast<const s16x8*>(grow[j] + (ch < nchunks ? ch : 0) * 16);
          }
#pragma unroll
        for (int u = 0; u < FF_MAXCH; ++u) {
          const int ch = base + lane + 64 * u;
          if (ch < nchunks) {
            const s16x8 qa = *reinterpret_cast<const s16x8*>(dyn + ch * 16);
#pragma unroll
            for (int j = 0; j < FF_CPW; ++j) acc[j] = dot16<FP8>(qa, ga[j][u], acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < FF_CPW; ++j) {
        const int c = c0 + 8 * j;
        const float e = finish_exact<FP8>(wave_sum_f64(acc[j]), row_scale<FP8>(q_scale, b), row_scale<FP8>(g_scale, id[j]), id[j]);
        if (lane == 0 && c < c_hi) sm.exact[c] = e;
      }
    }
  };
  // ---- final order of outk[0, tot) by (f32(exact) desc, index asc); leaves e_k and the entry count ----
  auto order = [&](int tot) {
    if (tid < tot) {
      const unsigned long long ki = outk[tid];
      if (ki != KEY_DEAD) {                          // padding stays behind every real entry: never written here
        const unsigned long long mine = make_key(sm.exact[tid], key_idx(ki));
        int rank = 0;
        for (int j = 0; j < tot; ++j) {
          const unsigned long long kj = outk[j];
          rank += (kj != KEY_DEAD && make_key(sm.exact[j], key_idx(kj)) > mine) ? 1 : 0;
        }
        atomicAdd(&sm.nvalid, 1);
        if (rank == k - 1) sm.ek = sm.exact[tid];
        if (rank < k) store_entry(mine, out_val, out_idx, (long long)b * k + rank, index_base);
      }
    }
  };

  rescore(0, kp);
  __syncthreads();
  order(kp);
  __syncthreads();
  const int nvalid = sm.nvalid;
  if (tid < k && tid >= nvalid) store_entry(KEY_DEAD, out_val, out_idx, (long long)b * k + tid);   // fewer real rows than k
  // ---- certification ----
  const float eps = err_rel * query_norm(((sm.red[0] + sm.red[1]) + (sm.red[2] + sm.red[3])) + ((sm.red[4] + sm.red[5]) + (sm.red[6] + sm.red[7])),
                                         row_scale<FP8>(q_scale, b));
  const unsigned long long kmin = outk[kp - 1];                  // smallest approximate key kept (KEY_DEAD: list not full)
  const float bar = sm.ek - eps;
  const bool certified = knn_certified(sm.ek, eps, kmin != KEY_DEAD, key_val(kmin));
  __syncthreads();                                               // everybody has read nvalid / ek before they are reused
  if (certified) {
    if (tid == 0 && status) status[b] = 0;
    return;
  }
  // widen: every candidate outside the top-kp whose approximate score reaches the bar
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (keys[i] != KEY_DEAD && keys[i] < kmin && key_val(keys[i]) >= bar) {
      const int pos = atomicAdd(&sm.extra, 1);
      if (kp + pos < FF_MAXC) outk[kp + pos] = keys[i];
    }
  }
  if (level0_lists) {                                            // a chunk list cut above the bar hides rows of the band
    const int nch = L / kp;
    for (int c = tid; c < nch; c += FF_NT) {
      const int last = c * kp + kp - 1;
      if (ix[last] >= 0 && v[last] >= bar) sm.flag = 2;
    }
  } else if (tid == 0) {
    sm.flag = 2;                                                 // lists of a later select level: per-chunk cuts unknown here
  }
  if (tid == 0) sm.nvalid = 0;
  __syncthreads();
  int extra = sm.extra;
  const bool overflow = kp + extra > FF_MAXC;
  if (overflow) extra = FF_MAXC - kp;
  rescore(kp, kp + extra);
  __syncthreads();
  order(kp + extra);
  if (tid == 0) {
    const int st = (sm.flag == 2 || overflow) ? 2 : 1;
    if (status) status[b] = st;
    if (st == 2 && uncertified) atomicAdd(uncertified, 1);
  }
}

// 3b. final order: grid (B), 128 threads.  Rank the kp rescored candidates by
// (f32(exact) desc, index asc) by counting; write the top-k with global indices.  Certification as in the
// fused kernel, without the widening step (this path serves rows wider than its LDS budget and galleries of
// more than ~1.4M rows per shard): status 0 or 2.
__global__ __launch_bounds__(128) void knn_order_kernel(
    const int32_t* __restrict__ cand_idx, const float* __restrict__ exact, int k, int kp, int index_base,
    float* __restrict__ out_val, int32_t* __restrict__ out_idx,
    const float* __restrict__ cand_approx, const float* __restrict__ qnorm, float err_rel,
    int32_t* __restrict__ status, int32_t* __restrict__ uncertified) {
  __shared__ unsigned long long key[128];
  __shared__ float ek;
  const int b = blockIdx.x, i = threadIdx.x;
  const unsigned long long mine =
      i < kp ? candidate_key(exact[(long long)b * kp + i], cand_idx[(long long)b * kp + i], true) : KEY_DEAD;
  key[i] = mine;
  if (i == 0) ek = -INFINITY;
  __syncthreads();
  if (i < kp) {
    int rank = i;     // padding already sits behind every real entry (select output is ordered)
    if (mine != KEY_DEAD) {
      rank = 0;
      for (int j = 0; j < kp; ++j) rank += key[j] > mine ? 1 : 0;
      if (rank == k - 1) ek = key_val(mine);
    }
    if (rank < k) store_entry(mine, out_val, out_idx, (long long)b * k + rank, index_base);
  }
  __syncthreads();
  if (i == 0 && (status || uncertified)) {
    const long long last = (long long)b * kp + kp - 1;           // the list is rank-ordered: last entry = a_min
    const bool ok = knn_certified(ek, err_rel * qnorm[b], cand_idx[last] >= 0, cand_approx[last]);
    if (status) status[b] = ok ? 0 : 2;
    if (!ok && uncertified) atomicAdd(uncertified, 1);
  }
}

// Exact score matrix (the fallback of a query the certification step flags): S[b, n] = f32 of the exact (f64) dot
// product, as the rescoring kernels compute it.  One wave per gallery row (its 16-B chunks held in registers, <= 17
// per lane), looped over the (few) queries; grid = ceil(N / 4) workgroups of 4 waves.  HBM-bound on the gallery
// for a handful of queries; a rare path, not tuned further.
constexpr int EX_MAXCH = 17;      // 16-B chunks per lane: rows up to 17408 bytes
template <bool FP8>
__global__ __launch_bounds__(256) void knn_exact_scores_kernel(
    const void* __restrict__ Qv, const void* __restrict__ Gv, const float* __restrict__ q_scale,
    const float* __restrict__ g_scale, float* __restrict__ S, int B, int N, int row_bytes, int ldS) {
  const int lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int nchunks = row_bytes >> 4;
  const char* grow = static_cast<const char*>(Gv) + n * row_bytes;
  s16x8 ga[EX_MAXCH];
#pragma unroll
  for (int u = 0; u < EX_MAXCH; ++u) {
    const int ch = lane + 64 * u;
    ga[u] = *reinterpret_cast<const s16x8*>(grow + (ch < nchunks ? ch : 0) * 16);
  }
  const float gs = row_scale<FP8>(g_scale, n);
  for (int b = 0; b < B; ++b) {
    const char* qrow = static_cast<const char*>(Qv) + (long long)b * row_bytes;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < EX_MAXCH; ++u) {
      const int ch = lane + 64 * u;
      if (ch < nchunks) acc = dot16<FP8>(*reinterpret_cast<const s16x8*>(qrow + ch * 16), ga[u], acc);
    }
    const float e = finish_exact<FP8>(wave_sum_f64(acc), row_scale<FP8>(q_scale, b), gs, 0);
    if (lane == 0) S[(long long)b * ldS + n] = e;
  }
}

// Merge of per-shard lists: vals/idxs [shards, B, k] -> [B, k].  shards*k <= 4096.
__global__ __launch_bounds__(256) void topk_merge_kernel(
    const float* __restrict__ vals, const int32_t* __restrict__ idxs, int shards, int B, int k,
    float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  __shared__ SelectState<SEL_CAP, 128> sm;
  const int b = blockIdx.x;
  const int L = shards * k;
  unsigned long long keys[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = i * 256 + (int)threadIdx.x;
    const int pc = p < L ? p : L - 1;
    const long long o = ((long long)(pc / k) * B + b) * k + pc % k;
    const int id = idxs[o];
    keys[i] = candidate_key(vals[o], id, p < L);
  }
  block_select<256>(keys, k, sm);
  if ((int)threadIdx.x < k) store_entry(sm.outk[threadIdx.x], out_val, out_idx, (long long)b * k + threadIdx.x);
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
struct KnnPlan {
  int Bpad, ldS, kp, ch0;
  int ks_max;            // score slabs the workspace holds (K-split of shards below 106k rows)
  int nrt;               // row tiles of the K-split form
  int nlevel;            // number of select levels before the final kernel
  int L[4], nchunk[4];   // input length / chunk count per level
  size_t off_S, off_cv[2], off_ci[2], off_qn, total;
};

static bool knn_plan(int B, int N, int D, int k, KnnPlan* p) {
  if (B <= 0 || N <= 0 || D <= 0 || k <= 0 || k > 64 || (D % 64) != 0) return false;
  p->Bpad = (B + KNN_QT - 1) / KNN_QT * KNN_QT;
  p->ldS = (N + 63) / 64 * 64;
  p->kp = knn_kp(k);
  // select levels: level 0 streams the score matrix in chunks of ch0 (<= 8192) scores, later
  // levels hold <= 4096 candidates per workgroup in registers; each level turns L entries per
  // query into nchunk*kp, and the last level has one chunk -> the [B][kp] list to rescore.
  p->ch0 = N > KNN_STREAM_CHUNK ? KNN_STREAM_CHUNK : (N + 1023) / 1024 * 1024;
  p->nlevel = 0;
  int L = N;
  for (;;) {
    if (p->nlevel >= 4) return false;
    const int chunk = p->nlevel == 0 ? p->ch0 : KNN_CHUNK;
    p->L[p->nlevel] = L;
    p->nchunk[p->nlevel] = (L + chunk - 1) / chunk;
    L = p->nchunk[p->nlevel] * p->kp;
    ++p->nlevel;
    if (p->nchunk[p->nlevel - 1] == 1) break;
  }
  // Small and medium shards (N < 106k rows: fewer 208-row tiles than the 512 resident workgroup slots).  Cutting the rows
  // finer to fill the chip multiplies the query traffic (every workgroup re-stages all 64 query rows: at 6k rows 16-row
  // tiles read 431 MB of queries for 108 MB of gallery) and leaves each tile a 132-step latency chain.  Instead: tall row
  // tiles (as few as fill the slots together with the K split, at least min(32, N/16)), and the K range of a tile split
  // over up to 16 workgroups, each writing its own score slab; the level-0 select adds the slabs.
  {
    const int by208 = (N + 207) / 208, by16 = (N + 15) / 16;
    const int fill = by16 < 32 ? by16 : 32;
    p->nrt = by208 > fill ? by208 : fill;
    int ks = 512 / p->nrt;
    p->ks_max = ks < 1 ? 1 : (ks > 16 ? 16 : ks);
    // gathered batches (> 64 queries) on the 256 x 256-tile GEMM: K slices until its one-per-CU workgroups fill 256 CUs
    if (B > KNN_QT) {
      const long long tiles = (long long)((B + 255) / 256) * ((N + 255) / 256);
      ks = tiles >= 256 ? 1 : (int)(256 / tiles);
      p->ks_max = ks > 4 ? 4 : ks;
    }
  }
  size_t off = 0;
  p->off_S = off;
  off += align_up((size_t)B * p->ldS * sizeof(float) * p->ks_max, 256);
  const size_t cand = (size_t)B * p->nchunk[0] * p->kp;
  for (int i = 0; i < 2; ++i) {
    p->off_cv[i] = off; off += align_up(cand * sizeof(float), 256);
    p->off_ci[i] = off; off += align_up(cand * sizeof(int32_t), 256);
  }
  p->off_qn = off; off += align_up((size_t)B * sizeof(float), 256);      // |q| per query (general rescore path)
  p->total = off;
  return true;
}

struct KnnOperands {          // bf16: scales are null; fp8: per-row f32 scales
  const void* q; const void* g; const float* q_scale; const float* g_scale; bool fp8;
};

// Where the select stage puts the answer and how it certifies it (status / uncertified may be null).
struct KnnOutputs {
  int index_base; float* val; int32_t* idx; float gallery_norm_bound; int32_t* status; int32_t* uncertified;
};

// f(std::true_type{}) for e4m3 operands, f(std::false_type{}) for bf16: o.fp8 as a template argument.
template <typename F>
static int knn_dispatch_fp8(bool fp8, F&& f) { return fp8 ? f(std::true_type{}) : f(std::false_type{}); }

// rows per workgroup of the fully resident grid (2 per CU): above one 208-row tile (N > 106k rows at 256 CUs); more than
// one 256-row tile (N > 131k rows)
static int knn_rows_per_wg(int N) { return (N + device_cu_count() * 2 - 1) / (device_cu_count() * 2); }
static bool knn_tall_tiles(int N) { return knn_rows_per_wg(N) > 208; }
static bool knn_multi_tile(int N) { return knn_rows_per_wg(N) > 256; }

// 256-row query tiles pay when at least 3/4 of their rows are real queries (256 gathered queries = 4 GPUs, 512 = 8 GPUs);
// VPR_KNN_FP8_GEMM256=0 forces the 128 x 128 kernel (A/B).
static bool knn_query_tile256_pays(int B) {
  if (tune_or(TUNE_KNN_FP8_GEMM256, 1) == 0) return false;
  const int tiles = (B + 255) / 256;
  return 4 * B >= 3 * tiles * 256;
}

static int knn_ksplit(const KnnPlan& p, int row_bytes) {
  int ks = p.ks_max;
  const int nk = row_bytes >> 7;
  if (ks > nk / 8) ks = nk / 8;                 // a slice keeps at least 8 K-steps
  return ks < 1 ? 1 : ks;
}

// Which kernel scores a [B] x [N] problem, and into how many K-slice slabs (the level-0 select adds them).
// More than one 64-query tile against a shard (the all-gathered batch of a multi-GPU job) moves towards a
// compute-bound GEMM: the streaming kernel makes one gallery pass per 64 queries, the 128x128-tile MFMA GEMM one per
// 128.  Measured, stream vs GEMM: 128 x 50k 367 / 222 us, 192 x 33k 406 / 300, 256 x 25k 477 / 185, 512 x 12.5k
// 702 / 151 (scripts/knn_b_sweep.py).  >= 192 of every 256 gathered queries real (256 at 4 GPUs, 512 at 8): the
// 256 x 256-tile kernel with its LDS-DMA stream kept in flight across barriers (gemm256.hip); a 128-query batch would
// leave half of such a tile row empty.
// ksplit_ok: the caller's select stage will add the slabs (vpr_knn_topk*); the stand-alone score entry point writes
// the one score matrix its contract promises.
enum KnnRoute { ROUTE_STREAM, ROUTE_GEMM128, ROUTE_GEMM256 };
static KnnRoute knn_route(const KnnPlan& p, bool fp8, int B, int N, int D, bool ksplit_ok, int* nslab) {
  const int gemm_min_b = tune_or(TUNE_KNN_GEMM_MIN_B, 65);     // A/B switch for the stream / GEMM crossover
  const int rb = fp8 ? D : D * 2;
  *nslab = 1;
  if (B < gemm_min_b) {                                 // streaming kernel; shards below 106k rows split K over tall tiles
    if (ksplit_ok) *nslab = knn_ksplit(p, rb);
    return ROUTE_STREAM;
  }
  if (!knn_query_tile256_pays(B) || (fp8 && D < 256)) return ROUTE_GEMM128;
  // 256 x 256 tiles, one workgroup per CU: with the K split a 512 x 12.5k problem (98 tiles) runs as 196 workgroups.
  // Without it (stand-alone score entry point, or VPR_KNN_GEMM_KSPLIT=0) bf16 needs >= 256 tiles to beat the 128 x 128
  // kernel's 4x as many workgroups.
  int ks = (ksplit_ok && B > KNN_QT && tune_or(TUNE_KNN_GEMM_KSPLIT, 1) != 0) ? knn_ksplit(p, rb) : 1;
  const long long tiles = (long long)((B + 255) / 256) * ((N + 255) / 256);
  if (!fp8 && tiles * ks < 192) return ROUTE_GEMM128;
  *nslab = ks;
  return ROUTE_GEMM256;
}

// ---- the streaming score kernel: which instantiation --------------------------------------------------------------
// Bits of knn_scores_kernel's fourth template argument.
enum KnnStreamFlags {
  // -DVPR_ABLATION builds only (timing: WRONG or no scores): no MFMA / no query staging after the first K-step; no score stores
  KNN_ABL_ONE_KSTEP = 1, KNN_ABL_ONE_QSTAGE = 2, KNN_ABL_NO_STORES = 8,
  KNN_NT_LOADS = 4,          // nt cache policy on the gallery stream (read once; keeps the query tile and the score matrix in
                             // L2 / Infinity Cache): +4.6 % on the bare stream, +5.2 % on this kernel at 100k rows
  KNN_NT_STORES = 16,        // nt policy on the score stores
  KNN_STAGED_STORES = 32,    // the score tile leaves through the idle stage buffers as whole row segments
};

struct KnnStreamKernel { int rows, wgpc, flags; };      // tile rows, workgroups per CU, flag bits

// VPR_KNN_VARIANT -> kernel.  0 is the shipped policy; 1..7 compute the same scores bit for bit and exist for A/B
// tuning in one process:
//   unset / 0   208-row tiles (13 row blocks, 2 workgroups per CU); 256 rows when knn_tall_tiles(N); staged + nt score
//               stores when knn_multi_tile(N)
//   1           (208, 2, 0)   default cache policy (round 1's kernel)
//   2           (144, 3, nt)  the round-1 first cut: 9 row blocks, 3 workgroups per CU
//   3           (256, 2, nt)  16 row blocks, all of the LDS, whatever the shard size
//   4           (208, 2, nt)  13 row blocks whatever the shard size (A/B against the tall tiles)
//   5 / 6 / 7   tile rows as 0, with direct / staged / staged + nt score stores forced
//   11..14      -DVPR_ABLATION builds only (they skip work: WRONG scores, timing only): no MFMA / no query staging /
//               neither after the first K-step; 14 = tile rows as 0, no score stores
//   other       (208, 2, nt)
// Tall tiles: shards whose workgroups own more than one 208-row tile (N > 106k) take 256-row tiles: 16 row blocks,
// 2 x 80 KB = the whole 160 KB of LDS, fewer tiles and 20 % less query re-staging: +2.3 % at 500k bf16 rows, +1.4 % on the
// 1M-row e4m3 call; a 125k-row shard becomes one 244-row tile per workgroup instead of two of 122 (scripts/knn_ab.py,
// knn_ab_fp8.py).
// Store path: shards whose workgroups own several tiles (N > 131k) write each tile's scores as whole row segments staged
// through the idle stage buffers (one 1-KiB float4 store per query row, nt policy) instead of dword stores of four
// 64-byte segments: the stores of a large shard cost far more than their 1.5-3 % share of the bytes (no-store ablation,
// score stage: 1M e4m3 rows 1518 -> 1245 us, 500k bf16 1391 -> 1252, 125k e4m3 170 -> 159, 100k bf16 ~0).  Staged + nt:
// 1M e4m3 1497 -> 1342 us, 500k bf16 1374 -> 1300, 250k bf16 668 -> 642; single-tile shards: no difference, they keep
// the direct stores.
static KnnStreamKernel knn_stream_kernel(int variant, int N) {
  const int by_shard = knn_tall_tiles(N) ? 256 : 208;
  switch (variant) {
    case 0: return {by_shard, 2, KNN_NT_LOADS | (knn_multi_tile(N) ? KNN_STAGED_STORES | KNN_NT_STORES : 0)};
    case 1: return {208, 2, 0};
    case 2: return {144, 3, KNN_NT_LOADS};
    case 3: return {256, 2, KNN_NT_LOADS};
    case 5: return {by_shard, 2, KNN_NT_LOADS};
    case 6: return {by_shard, 2, KNN_NT_LOADS | KNN_STAGED_STORES};
    case 7: return {by_shard, 2, KNN_NT_LOADS | KNN_STAGED_STORES | KNN_NT_STORES};
#ifdef VPR_ABLATION
    case 11: return {208, 2, KNN_NT_LOADS | KNN_ABL_ONE_KSTEP};
    case 12: return {208, 2, KNN_NT_LOADS | KNN_ABL_ONE_QSTAGE};
    case 13: return {208, 2, KNN_NT_LOADS | KNN_ABL_ONE_KSTEP | KNN_ABL_ONE_QSTAGE};
    case 14: return {by_shard, 2, KNN_NT_LOADS | KNN_ABL_NO_STORES};
#endif
    default: return {208, 2, KNN_NT_LOADS};             // 4, and every value without a meaning
  }
}

// The instantiations that exist, each for both operand types: (tile rows, workgroups per CU, flags); 36 = nt loads +
// staged stores, 52 = the same with nt stores.  The launch and the printed name both come from this list.
#ifdef VPR_ABLATION     // timing-only kernels: never in the shipped library
#define VPR_KNN_ABLATION_KERNELS(X) X(208, 2, 5) X(208, 2, 6) X(208, 2, 7) X(208, 2, 12) X(256, 2, 12)
#else
#define VPR_KNN_ABLATION_KERNELS(X)
#endif
#define VPR_KNN_STREAM_KERNELS(X)                                                                       \
  X(208, 2, 4) X(256, 2, 4) X(144, 3, 4) X(208, 2, 0) X(208, 2, 36) X(208, 2, 52) X(256, 2, 36) X(256, 2, 52) \
  VPR_KNN_ABLATION_KERNELS(X)

struct KnnCall;
struct KnnStreamEntry {
  KnnStreamKernel k;
  const char* name[2];      // [fp8], as a kernel trace prints it
  int (*launch)(const KnnCall& c, dim3 grid, float* S, hipStream_t stream);
};

// One resolved description of a call: built once (knn_describe / knn_resolve), read by every stage.
struct KnnCall {
  KnnOperands o; char* ws; int B, N, D, k, row_bytes;
  KnnPlan p;
  KnnRoute route;
  int nslab;                       // score slabs the score stage writes and the level-0 select adds
  const KnnStreamEntry* stream;    // ROUTE_STREAM: the kernel
};

template <int TR, int WGPC, int FLAGS>
static int knn_launch_stream(const KnnCall& c, dim3 grid, float* S, hipStream_t stream) {
  return knn_dispatch_fp8(c.o.fp8, [&](auto fp8) {
    constexpr size_t lds = (size_t)2 * (TR + KNN_QT) * TILE_ROW_BYTES;
    return launch_kernel_lds<knn_scores_kernel<decltype(fp8)::value, TR, WGPC, FLAGS>>(
        grid, dim3(256), lds, stream, c.o.q, c.o.g, c.o.q_scale, c.o.g_scale, S, c.B, c.N, c.row_bytes, c.p.ldS);
  });
}

static const KnnStreamEntry* knn_stream_entry(const KnnStreamKernel& k) {
  static const KnnStreamEntry table[] = {
#define VPR_KNN_ENTRY(TR, W, A)                                                                         \
    {{TR, W, A}, {"vpr::knn_scores_kernel<false, " #TR ", " #W ", " #A ">", "vpr::knn_scores_kernel<true, " #TR ", " #W ", " #A ">"}, \
     knn_launch_stream<TR, W, A>},
    VPR_KNN_STREAM_KERNELS(VPR_KNN_ENTRY)
#undef VPR_KNN_ENTRY
  };
  for (const KnnStreamEntry& e : table)
    if (e.k.rows == k.rows && e.k.wgpc == k.wgpc && e.k.flags == k.flags) return &e;
  return nullptr;
}

// Plan, route, slab count and stream kernel of a [B] x [N] x [D] problem: everything that follows from the shape and the
// tuning switches alone (vpr_knn_scores_kernel_name stops here).
static int knn_describe(bool fp8, int B, int N, int D, int k, bool ksplit_ok, KnnCall* c) {
  if (!knn_plan(B, N, D, k, &c->p)) return VPR_ERR_UNSUPPORTED;
  c->B = B; c->N = N; c->D = D; c->k = k; c->row_bytes = fp8 ? D : D * 2;
  c->route = knn_route(c->p, fp8, B, N, D, ksplit_ok, &c->nslab);
  c->stream = c->route == ROUTE_STREAM ? knn_stream_entry(knn_stream_kernel(tune_or(TUNE_KNN_VARIANT, 0), N)) : nullptr;
  return c->route == ROUTE_STREAM && !c->stream ? VPR_ERR_UNSUPPORTED : VPR_OK;      // outside the list: cannot happen
}

// The argument checks of every entry point, in one order, then the description.  out: null for a score-only call.
// bad_shape: the status of a non-positive B, N, D or k — VPR_ERR_INVALID_ARG, except at vpr_knn_scores / vpr_knn_select
// / vpr_knn_select_checked, which have always answered VPR_ERR_UNSUPPORTED (tests/test_library_cpu.py pins both).
static int knn_resolve(const KnnOperands& o, int B, int N, int D, int k, void* ws, size_t ws_bytes, const KnnOutputs* out,
                       bool ksplit_ok, int bad_shape, KnnCall* c) {
  if (out && (!(out->gallery_norm_bound > 0.f) || !out->val || !out->idx)) return VPR_ERR_INVALID_ARG;
  if (B <= 0 || N <= 0 || D <= 0 || k <= 0) return bad_shape;
  if (!ws || !o.q || !o.g || (o.fp8 && (!o.q_scale || !o.g_scale))) return VPR_ERR_INVALID_ARG;
  VPR_TRY_LAUNCH(knn_describe(o.fp8, B, N, D, k, ksplit_ok, c));
  if (o.fp8 && (D % 128) != 0) return VPR_ERR_UNSUPPORTED;           // 128-B K-steps
  if ((reinterpret_cast<uintptr_t>(o.q) | reinterpret_cast<uintptr_t>(o.g)) & 15) return VPR_ERR_UNSUPPORTED;
  if (ws_bytes < c->p.total) return VPR_ERR_WORKSPACE;
  c->o = o; c->ws = static_cast<char*>(ws);
  return VPR_OK;
}

// Score stage: S[b, n] = <q_b, g_n> into the workspace, c.nslab K-slice slabs of [B][ldS] f32.
static int knn_scores(const KnnCall& c, hipStream_t stream) {
  const KnnOperands& o = c.o; const KnnPlan& p = c.p;
  const int B = c.B, N = c.N, D = c.D;
  float* S = reinterpret_cast<float*>(c.ws + p.off_S);
  const long long slab_stride = (long long)B * p.ldS;
  if (c.route != ROUTE_STREAM) {      // e4m3: block-scaled fp8 MFMA (twice the bf16 rate), scales in the epilogue
    GemmProblem g = o.fp8 ? gemm_problem_e4m3(static_cast<const uint8_t*>(o.q), D, o.q_scale, static_cast<const uint8_t*>(o.g), D,
                                              o.g_scale, S, p.ldS, B, N, D)
                          : gemm_problem(static_cast<const uint16_t*>(o.q), D, static_cast<const uint16_t*>(o.g), D, nullptr, 0,
                                         S, p.ldS, 0, B, N, D);
    g.ksplit = c.nslab; g.slab_stride = slab_stride;      // ROUTE_GEMM128 never splits K (knn_route)
    return (c.route == ROUTE_GEMM256 ? launch_gemm256 : launch_gemm_nt)(g, o.fp8, stream);
  }
  // Streaming kernel.  Fully resident, balanced grid; never more workgroups than 16-row blocks of gallery.
  int nwg = device_cu_count() * c.stream->k.wgpc;
  const int max_useful = (N + 15) / 16;
  if (nwg > max_useful) nwg = max_useful;
  if (c.nslab > 1) nwg = p.nrt;                   // tall tiles: the K split supplies the parallelism
  return c.stream->launch(c, dim3(nwg, p.Bpad / KNN_QT, c.nslab), S, stream);
}

// Default norm bounds of the unchecked entry points: L2-normalised descriptors.  A bf16-rounded unit vector has norm
// within 2^-9 of 1; an e4m3 row (3 mantissa bits, scale = max/448) within 2^-4.
constexpr float NORM_BOUND_BF16 = 1.002f;
constexpr float NORM_BOUND_FP8 = 1.0625f;

// Relative bound of |MFMA score - exact score| / (|q| |g|): D f32 additions of exact products in any order
// (gamma_D = D 2^-24 to first order; 1.1 covers the higher-order terms, the final f32 rounding of the exact score
// and the two scale multiplications of the fp8 path), times the caller's bound on the gallery row norms.
static float knn_err_rel(int D, float gallery_norm_bound) {
  return 1.1f * (float)D * 5.9604645e-8f * gallery_norm_bound;
}

// Select stage: adds the c.nslab score slabs the score stage of this call left, selects, rescores exactly, orders.
static int knn_select(const KnnCall& c, const KnnOutputs& out, hipStream_t stream) {
  const KnnOperands& o = c.o; const KnnPlan& p = c.p;
  const int B = c.B, N = c.N, k = c.k, rb = c.row_bytes;
  const float err_rel = knn_err_rel(c.D, out.gallery_norm_bound);
  const float* cur_v = reinterpret_cast<float*>(c.ws + p.off_S);
  const int32_t* cur_i = nullptr;
  long long ld = p.ldS;
  int L = N;
  const long long slab_stride = (long long)B * p.ldS;
  // the fused final kernel takes over as soon as the candidates of a query fit one workgroup
  // (its LDS = 36 KB of select state + the query row, kept under the 64 KB default limit)
  const auto fits_fused = [&](int lev) { return lev > 0 && L <= SEL_CAP && (size_t)rb <= 24 * 1024; };
  int lev = 0;
  for (; lev < p.nlevel && !fits_fused(lev); ++lev) {
    float* ov = reinterpret_cast<float*>(c.ws + p.off_cv[lev & 1]);
    int32_t* oi = reinterpret_cast<int32_t*>(c.ws + p.off_ci[lev & 1]);
    if (lev == 0)
      VPR_TRY_LAUNCH(launch_kernel(p.kp <= 32 ? knn_select_stream_kernel<1024> : knn_select_stream_kernel<4096>,
                                   dim3(p.nchunk[0], B), dim3(256), 0, stream, cur_v, N, ld, p.ch0, ov, oi, p.kp,
                                   p.nchunk[0], c.nslab, slab_stride));
    else
      VPR_TRY_LAUNCH(launch_kernel(knn_select_kernel, dim3(p.nchunk[lev], B), dim3(256), 0, stream,
                                   cur_v, cur_i, L, ld, ov, oi, p.kp, p.nchunk[lev]));
    cur_v = ov; cur_i = oi;
    L = p.nchunk[lev] * p.kp;
    ld = L;
  }
  if (fits_fused(lev)) {
    const int level0 = lev == 1 ? 1 : 0;       // the lists in hand are level 0's [nchunk][kp] rank-ordered lists
    return knn_dispatch_fp8(o.fp8, [&](auto fp8) {
      return launch_kernel(knn_final_fused_kernel<decltype(fp8)::value>, dim3(B), dim3(FF_NT), (size_t)rb, stream, cur_v,
                           cur_i, L, o.q, o.g, o.q_scale, o.g_scale, rb, k, p.kp, out.index_base, out.val, out.idx,
                           err_rel, level0, out.status, out.uncertified);
    });
  }
  // general path: the last select level left the [B][kp] list; rescore and order it
  float* exact = reinterpret_cast<float*>(c.ws + p.off_cv[p.nlevel & 1]);
  float* qn = reinterpret_cast<float*>(c.ws + p.off_qn);
  VPR_TRY_LAUNCH(knn_dispatch_fp8(o.fp8, [&](auto fp8) {
    return launch_kernel(knn_rescore_kernel<decltype(fp8)::value>, dim3(p.kp, B), dim3(256), 0, stream, cur_i, o.q, o.g,
                         o.q_scale, o.g_scale, rb, p.kp, exact, qn);
  }));
  return launch_kernel(knn_order_kernel, dim3(B), dim3(128), 0, stream, cur_i, exact, k, p.kp, out.index_base, out.val,
                       out.idx, cur_v, qn, err_rel, out.status, out.uncertified);
}

// Per-row symmetric quantisation to OCP e4m3: scale = max|x| / 448 (1 for an all-zero row),
// q = fp8_rne(x / scale).  One workgroup per row; v_cvt_pk_fp8_f32 does the rounding.
__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(const float* __restrict__ x, int D,
                                                                uint8_t* __restrict__ q, float* __restrict__ scale) {
  __shared__ float red[4];
  const long long row = blockIdx.x;
  const float* xr = x + row * D;
  float m = 0.f;
  for (int d = threadIdx.x * 4; d < D; d += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(xr + d);
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float sc = m > 0.f ? m / 448.0f : 1.0f;
  if (threadIdx.x == 0) scale[row] = sc;
  for (int d = threadIdx.x * 4; d < D; d += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(xr + d);
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v.x / sc, v.y / sc, 0, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(v.z / sc, v.w / sc, pk, true);
    *reinterpret_cast<int*>(q + row * D + d) = pk;
  }
}

}  // namespace vpr

using namespace vpr;

extern "C" size_t vpr_knn_workspace_bytes(int B, int N, int D, int k) {
  KnnPlan p;
  return knn_plan(B, N, D, k, &p) ? p.total : 0;
}

extern "C" const char* vpr_knn_scores_kernel_name(int is_fp8, int B, int N) {
  // the score stage of vpr_knn_topk* at the descriptor width of the path, D = 8448, described exactly as a call
  // describes it: what a kernel trace (rocprofv3) will show for this call
  const bool fp8 = is_fp8 != 0;
  KnnCall c;
  if (knn_describe(fp8, B, N, 8448, 10, true, &c) != VPR_OK) return "";
  if (c.route == ROUTE_GEMM256) return gemm256_kernel_name(fp8);
  if (c.route == ROUTE_GEMM128) return gemm_nt_kernel_name(fp8, N);
  return c.stream->name[fp8];
}

extern "C" float* vpr_knn_scores_ptr(void* workspace, int B, int N, int D, int k, int* ld_out) {
  KnnPlan p;
  if (!workspace || !knn_plan(B, N, D, k, &p)) return nullptr;
  if (ld_out) *ld_out = p.ldS;
  return reinterpret_cast<float*>(static_cast<char*>(workspace) + p.off_S);
}

// Every entry point but the exhaustive one: resolve the call once and run the stages asked for on that one description,
// so the select adds exactly the slabs the score stage wrote.  out == null: score stage only; scores == false: select
// stage only, on what a score stage of the same call (ksplit_ok: same value) left in the workspace.
static int knn_run(const KnnOperands& o, int B, int N, int D, int k, bool scores, const KnnOutputs* out, void* workspace,
                   size_t workspace_bytes, void* stream, bool ksplit_ok, int bad_shape) {
  KnnCall c;
  VPR_TRY_LAUNCH(knn_resolve(o, B, N, D, k, workspace, workspace_bytes, out, ksplit_ok, bad_shape, &c));
  if (scores) VPR_TRY_LAUNCH(knn_scores(c, static_cast<hipStream_t>(stream)));
  return out ? knn_select(c, *out, static_cast<hipStream_t>(stream)) : VPR_OK;
}

// The stand-alone stages: one plain score matrix (no K-split).  The plan's score-matrix offset does not depend on k.
extern "C" int vpr_knn_scores(const uint16_t* q, const uint16_t* gallery, int B, int N, int D,
                              void* workspace, size_t workspace_bytes, void* stream) {
  return knn_run({q, gallery, nullptr, nullptr, false}, B, N, D, 1, true, nullptr, workspace, workspace_bytes, stream,
                 false, VPR_ERR_UNSUPPORTED);
}

extern "C" int vpr_knn_select_checked(const uint16_t* q, const uint16_t* gallery, int B, int N, int D, int k,
                                      int index_base, float* out_val, int32_t* out_idx, void* workspace,
                                      size_t workspace_bytes, float gallery_norm_bound, int32_t* status,
                                      int32_t* uncertified, void* stream) {
  const KnnOutputs out{index_base, out_val, out_idx, gallery_norm_bound, status, uncertified};
  return knn_run({q, gallery, nullptr, nullptr, false}, B, N, D, k, false, &out, workspace, workspace_bytes, stream,
                 false, VPR_ERR_UNSUPPORTED);
}

extern "C" int vpr_knn_select(const uint16_t* q, const uint16_t* gallery, int B, int N, int D, int k,
                              int index_base, float* out_val, int32_t* out_idx, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return vpr_knn_select_checked(q, gallery, B, N, D, k, index_base, out_val, out_idx, workspace, workspace_bytes,
                                NORM_BOUND_BF16, nullptr, nullptr, stream);
}

// The two halves of vpr_knn_topk[_fp8]_checked as separate calls (same kernels, same workspace contents in between:
// the score stage may leave K-slice slabs that only this select stage knows to add), for callers that put events or
// other stream work between the HBM-bound score stage and the latency-bound tail.  Each resolves the call on its own.
extern "C" int vpr_knn_topk_scores_stage(const void* q, const float* q_scale, const void* gallery,
                                         const float* gallery_scale, int is_fp8, int B, int N, int D, int k,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return knn_run({q, gallery, q_scale, gallery_scale, is_fp8 != 0}, B, N, D, k, true, nullptr, workspace,
                 workspace_bytes, stream, true, VPR_ERR_INVALID_ARG);
}

extern "C" int vpr_knn_topk_select_stage(const void* q, const float* q_scale, const void* gallery,
                                         const float* gallery_scale, int is_fp8, int B, int N, int D, int k,
                                         int index_base, float* out_val, int32_t* out_idx, void* workspace,
                                         size_t workspace_bytes, float gallery_norm_bound, int32_t* status,
                                         int32_t* uncertified, void* stream) {
  const KnnOutputs out{index_base, out_val, out_idx, gallery_norm_bound, status, uncertified};
  return knn_run({q, gallery, q_scale, gallery_scale, is_fp8 != 0}, B, N, D, k, false, &out, workspace,
                 workspace_bytes, stream, true, VPR_ERR_INVALID_ARG);
}

extern "C" int vpr_knn_topk_checked(const uint16_t* q, const uint16_t* gallery, int B, int N, int D, int k,
                                    int index_base, float* out_val, int32_t* out_idx, void* workspace,
                                    size_t workspace_bytes, float gallery_norm_bound, int32_t* status,
                                    int32_t* uncertified, void* stream) {
  const KnnOutputs out{index_base, out_val, out_idx, gallery_norm_bound, status, uncertified};
  return knn_run({q, gallery, nullptr, nullptr, false}, B, N, D, k, true, &out, workspace, workspace_bytes, stream,
                 true, VPR_ERR_INVALID_ARG);
}

extern "C" int vpr_knn_topk(const uint16_t* q, const uint16_t* gallery, int B, int N, int D, int k,
                            int index_base, float* out_val, int32_t* out_idx, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return vpr_knn_topk_checked(q, gallery, B, N, D, k, index_base, out_val, out_idx, workspace, workspace_bytes,
                              NORM_BOUND_BF16, nullptr, nullptr, stream);
}

extern "C" int vpr_knn_topk_fp8_checked(const uint8_t* q, const float* q_scale, const uint8_t* gallery,
                                        const float* gallery_scale, int B, int N, int D, int k, int index_base,
                                        float* out_val, int32_t* out_idx, void* workspace, size_t workspace_bytes,
                                        float gallery_norm_bound, int32_t* status, int32_t* uncertified,
                                        void* stream) {
  const KnnOutputs out{index_base, out_val, out_idx, gallery_norm_bound, status, uncertified};
  return knn_run({q, gallery, q_scale, gallery_scale, true}, B, N, D, k, true, &out, workspace, workspace_bytes, stream,
                 true, VPR_ERR_INVALID_ARG);
}

extern "C" int vpr_knn_topk_fp8(const uint8_t* q, const float* q_scale, const uint8_t* gallery,
                                const float* gallery_scale, int B, int N, int D, int k, int index_base,
                                float* out_val, int32_t* out_idx, void* workspace, size_t workspace_bytes,
                                void* stream) {
  return vpr_knn_topk_fp8_checked(q, q_scale, gallery, gallery_scale, B, N, D, k, index_base, out_val, out_idx, workspace,
                                  workspace_bytes, NORM_BOUND_FP8, nullptr, nullptr, stream);
}

extern "C" int vpr_knn_topk_exhaustive(const void* q, const float* q_scale, const void* gallery,
                                       const float* gallery_scale, int is_fp8, int B, int N, int D, int k,
                                       int index_base, float* out_val, int32_t* out_idx, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  // the scores are exact already: every cut keeps the true largest keys, whatever the bound says
  const KnnOutputs out{index_base, out_val, out_idx, 1.0f, nullptr, nullptr};
  KnnCall c;      // one slab: the exact kernel writes a plain score matrix
  VPR_TRY_LAUNCH(knn_resolve({q, gallery, q_scale, gallery_scale, is_fp8 != 0}, B, N, D, k, workspace, workspace_bytes,
                             &out, false, VPR_ERR_INVALID_ARG, &c));
  if (c.row_bytes > EX_MAXCH * 64 * 16) return VPR_ERR_UNSUPPORTED;
  float* S = reinterpret_cast<float*>(c.ws + c.p.off_S);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  VPR_TRY_LAUNCH(knn_dispatch_fp8(c.o.fp8, [&](auto fp8) {
    return launch_kernel(knn_exact_scores_kernel<decltype(fp8)::value>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, hs,
                         c.o.q, c.o.g, c.o.q_scale, c.o.g_scale, S, B, N, c.row_bytes, c.p.ldS);
  }));
  return knn_select(c, out, hs);
}

extern "C" int vpr_quantize_fp8_rows(const float* x, long long rows, int D, uint8_t* q, float* scale, void* stream) {
  if (!x || !q || !scale || rows < 0 || D <= 0) return VPR_ERR_INVALID_ARG;
  if ((D % 4) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(q) & 3)) return VPR_ERR_UNSUPPORTED;
  if (rows == 0) return VPR_OK;
  if (rows > 0x7fffffffLL) return VPR_ERR_UNSUPPORTED;
  VPR_TRY_LAUNCH(launch_kernel(quantize_fp8_rows_kernel, dim3((unsigned)rows), dim3(256), 0,
                               static_cast<hipStream_t>(stream), x, D, q, scale));
  return VPR_OK;
}

extern "C" int vpr_topk_merge(const float* vals, const int32_t* idxs, int shards, int B, int k,
                              float* out_val, int32_t* out_idx, void* stream) {
  if (!vals || !idxs || !out_val || !out_idx || shards <= 0 || B <= 0 || k <= 0) return VPR_ERR_INVALID_ARG;
  if (k > 128 || (long long)shards * k > 4096) return VPR_ERR_UNSUPPORTED;
  VPR_TRY_LAUNCH(launch_kernel(topk_merge_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     vals, idxs, shards, B, k, out_val, out_idx));
  return VPR_OK;
}
