// vpr_common.h — shared device helpers for the gfx950 (MI355X / CDNA4) kernels.
// Wavefront = 64 lanes everywhere; LDS tiles are [rows][64 bf16] (128-B rows) filled by
// LDS-DMA (global_load_lds_dwordx4) and read back as MFMA fragments with ds_read_b128.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vpr {

typedef __attribute__((ext_vector_type(8))) short s16x8;     // 8 bf16 = one 16-B chunk
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;   // MFMA A/B fragment type
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;       // one 16-B chunk as loaded: 8 bf16, 16 e4m3 or 4 f32
typedef __attribute__((ext_vector_type(8))) int i32x8;       // two chunks: the 32-byte e4m3 operand of a block-scaled MFMA

constexpr int WAVE = 64;

// 100 MHz constant clock, read where the statement stands (volatile asm with a memory clobber: the compiler may not move
// it across the surrounding code) — phase clocks of the timing-only build.
__device__ __forceinline__ long long vpr_clock_now() {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return (long long)t;
}

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t v) {
  return __uint_as_float(((uint32_t)v) << 16);
}
// Round-to-nearest-even f32 -> bf16 bits.  The compiler emits v_cvt_pk_bf16_f32 for the cast
// (NaN stays NaN; see MI355X_MICROARCH "Correctness boundaries").
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(uint16_t, h);
}

// v = hi + lo to 2^-17 relative: hi = bf16(v), lo = bf16(v - hi), both round-to-nearest-even (the packed W1 planes of the
// pose head and the x operand it splits in registers).
__device__ __forceinline__ void split_hi_lo(float v, uint16_t& hi, uint16_t& lo) {
  hi = f32_to_bf16_bits(v);
  lo = f32_to_bf16_bits(v - bf16_bits_to_f32(hi));
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() compiles to s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier,
// i.e. it also drains every global load the wave has in flight; a kernel that wants its global loads to keep flying
// across barriers (the compiler still waits for each loaded register before its first use) uses this one.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// All-reduce inside each 16-lane row with DPP only (no LDS traffic): xor 1, xor 2 as quad
// permutes, then row_half_mirror and row_mirror (after the first two steps a quad holds one
// value, so mirroring pairs the remaining groups).  Every lane ends with its row's result.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f32<0xB1>(v));    // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_f32<0x4E>(v));    // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_f32<0x141>(v));   // row_half_mirror
  v = fmaxf(v, dpp_f32<0x140>(v));   // row_mirror
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f32<0xB1>(v);
  v += dpp_f32<0x4E>(v);
  v += dpp_f32<0x141>(v);
  v += dpp_f32<0x140>(v);
  return v;
}

// ---- the packed top-k key ---------------------------------------------------------------------------------
// Key order: value desc, index asc (packed into one u64 so a max-reduction does both).  Shared by the kNN selects, the
// shard merge (knn.hip) and the re-rank order stage (order_rank below).
__device__ __forceinline__ uint32_t f32_orderable(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_orderable(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ unsigned long long make_key(float v, int idx) {   // idx >= 0; unique per idx
  return ((unsigned long long)f32_orderable(v) << 32) | (uint32_t)(0x7fffffff - idx);
}
__device__ __forceinline__ int key_idx(unsigned long long k) { return 0x7fffffff - (int)(uint32_t)k; }
__device__ __forceinline__ float key_val(unsigned long long k) { return f32_from_orderable((uint32_t)(k >> 32)); }

constexpr unsigned long long KEY_DEAD = 0ull;   // padding: below every real key (orderable(-inf) > 0), so it sorts last

// The key of an input entry: positions outside the input and padding entries (index < 0) become KEY_DEAD by a select,
// so callers load from a clamped position and stay branch-free (their keys stay in registers).
__device__ __forceinline__ unsigned long long candidate_key(float val, int id, bool in_range) {
  return (in_range && id >= 0) ? make_key(val, id) : KEY_DEAD;
}
// One output entry: KEY_DEAD -> (-inf, -1); a real key -> (value, index + index_base).
__device__ __forceinline__ void store_entry(unsigned long long k, float* __restrict__ out_val,
                                            int32_t* __restrict__ out_idx, long long o, int index_base = 0) {
  out_val[o] = k == KEY_DEAD ? -INFINITY : key_val(k);
  out_idx[o] = k == KEY_DEAD ? -1 : key_idx(k) + index_base;
}

// ---- LDS tile geometry -------------------------------------------------------------------
// A tile row is 64 bf16 = 128 B = 8 chunks of 16 B.  Chunk c of row r is stored at physical
// chunk c ^ ((r >> 1) & 7): with this XOR every ds_read_b128 lane group of both MFMA operand
// maps (16x16x32: row = lane&15, chunk = lane>>4 (+4); 32x32x16: row = lane&31,
// chunk = lane>>5 (+2s)) touches 16 distinct 16-B slots of the 256-B bank row (checked
// exhaustively on the host, tests/test_library_cpu.py::test_lds_swizzle_is_conflict_free) — conflict-free.
constexpr int TILE_ROW_BYTES = 128;
__device__ __forceinline__ int tile_off(int row, int chunk) {
  return row * TILE_ROW_BYTES + ((chunk ^ ((row >> 1) & 7)) << 4);
}
// The inverse, on the filling side.  One LDS-DMA instruction (glds16 below) fills 8 tile rows: lane i writes physical slot
// (tr, i % 8) of tile row tr = first row of the group + i / 8, and therefore fetches logical chunk (i % 8) ^ swz(tr).  This is
// the byte offset of that chunk in the lane's source row (bf16 or e4m3: a tile row is 128 source bytes either way); the
// caller resolves tr -> source row pointer (clamping / grouping).  tile_off(tr, c) then finds chunk c where it landed.
__device__ __forceinline__ int stage_src_off(int tr, int lane) {
  return ((lane & 7) ^ ((tr >> 1) & 7)) << 4;
}

// One LDS-DMA wave-instruction: 64 lanes x 16 B land at lds_wave_base + lane*16 (the LDS side
// is linear; the swizzle is applied to the per-lane SOURCE address, cdna guide rule 21).
// AUX = cache-policy bits of the instruction: 0 default, 2 = nt (non-temporal: for bytes read once, e.g. the gallery
// stream of the kNN score kernel; MI355X_MICROARCH "nt-weights").
template <int AUX = 0>
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, AUX);
}

__device__ __forceinline__ bf16x8 lds_frag(const char* tile, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(tile + tile_off(row, chunk));
}

// ---- the block-scaled e4m3 MFMA step (gemm_nt.hip, gemm256.hip, knn.hip) ------------------------------------------
// v_mfma_scale_f32_{16x16x128,32x32x64}_f8f6f4 on OCP e4m3 bytes with unit block scales: twice the bf16 rate, where the
// plain fp8 MFMA runs at the bf16 rate.  A lane's operand is 32 K bytes = two 16-byte chunks of its tile row, read with
// the same ds_read_b128 as a bf16 fragment; A and B use the same lane -> K assignment, which is all a dot product needs.
template <typename Chunk>
__device__ __forceinline__ i32x8 e4m3_operand(Chunk lo, Chunk hi) {
  const i32x4 l = __builtin_bit_cast(i32x4, lo), h = __builtin_bit_cast(i32x4, hi);
  return i32x8{l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
}
constexpr int E8M0_ONE = 127;   // the E8M0 block scale 2^0, for both operands: the row scales are applied in the epilogues
__device__ __forceinline__ f32x4 mfma_e4m3_16x16x128(i32x8 a, i32x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, E8M0_ONE, 0, E8M0_ONE);
}
__device__ __forceinline__ f32x16 mfma_e4m3_32x32x64(i32x8 a, i32x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, E8M0_ONE, 0, E8M0_ONE);
}

// XCD-aware remap of a workgroup id to a tile (cdna guide §5: "XCD swizzle must be bijective").  Workgroup `orig` of `nwg`
// runs on XCD orig % 8; the workgroups of one XCD get a contiguous run of tiles (the first nwg % 8 XCDs one more each), so
// neighbouring tiles re-use an operand panel out of that XCD's L2.
__device__ __forceinline__ int xcd_tile(int orig, int nwg) {
  const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): ten rounds of two 32x32 -> 64 multiplies.  The dropout
// masks of the head-training step and of the SALAD MLPs (include/vpr_amd.h) are words of it.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// ---- split-K slabs of the heads' first layer ---------------------------------------------------------------
// A slab holds one K-slice's partial sums of x W1^T.  Two layouts; at(slice, b, h) is the address of hidden unit h of batch
// row b in slab `slice` (the four units of an aligned group of 4 are contiguous in both), slice_stride() the distance in
// floats between the same element of two consecutive slabs.  Every writer and reader of a slab addresses it through these.
struct SlabRowMajor {        // part[slice][B][hidden]
  float* part; int B, hidden;
  __device__ __forceinline__ float* at(int slice, int b, int h) const { return part + ((long long)slice * B + b) * hidden + h; }
  __device__ __forceinline__ long long slice_stride() const { return (long long)B * hidden; }
};
struct SlabTiles {           // part[slice][mtiles][ntiles][64 rows][64 cols]: a reader of one (batch, hidden) tile sees 16 KB runs
  float* part; int mtiles, ntiles;
  __device__ __forceinline__ float* at(int slice, int b, int h) const {
    return part + (((long long)slice * mtiles + (b >> 6)) * ntiles + (h >> 6)) * 4096 + (b & 63) * 64 + (h & 63);
  }
  __device__ __forceinline__ long long slice_stride() const { return (long long)mtiles * ntiles * 4096; }
};

// ---- exact-f32 MFMA over one K-slice (v_mfma_f32_16x16x4_f32 == an fmaf chain) ------------------------------
// A wave's 16 rows x 32 columns (acc0: columns 0-15, acc1: 16-31) over the k-steps first, first + STRIDE, ... of
// [s_begin, s_end), a step being 16 of K.  Operand maps of 16x16x4: A[row = lane&15][k = lane>>4], B[k = lane>>4][col =
// lane&15]; a lane loads 4 consecutive k (one float4) and feeds element t to MFMA t — A and B use the same k permutation, so
// it cancels.  xa / wa / wb are the lane's float4 streams of its x row and of its two weight rows, already offset by the
// lane's k-group (lane>>4); step s is element [4 s].  CH steps (3 x 16 B per lane each) are requested before their MFMAs, so a
// slice is a few round trips to HBM/L2 instead of one per step; the guard is wave-uniform.
template <int CH, int STRIDE>
__device__ __forceinline__ void mfma_f32_slice(const float4* xa, const float4* wa, const float4* wb, int first, int s_begin,
                                               int s_end, f32x4& acc0, f32x4& acc1) {
  for (int base = s_begin; base < s_end; base += STRIDE * CH) {     // uniform per workgroup
    float4 a[CH], w0[CH], w1[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int s = min(base + first + STRIDE * i, s_end - 1);
      a[i] = xa[s * 4];
      w0[i] = wa[s * 4];
      w1[i] = wb[s * 4];
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      if (base + first + STRIDE * i < s_end) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, w0[i].x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, w1[i].x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, w0[i].y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, w1[i].y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, w0[i].z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, w1[i].z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, w0[i].w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, w1[i].w, acc1, 0, 0, 0);
      }
    }
  }
}

// The wave's accumulators of mfma_f32_slice to slab `slice`, batch rows b0 .. b0+15 (those below B), hidden units h0 .. h0+31.
// C/D: col (hidden) = lane&15, row (batch) = 4*(lane>>4) + e.
__device__ __forceinline__ void mfma_f32_store_rows(const SlabRowMajor& slab, int slice, int b0, int h0, int lane,
                                                    const f32x4& acc0, const f32x4& acc1) {
  const int r = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = b0 + 4 * kg + e;
    if (b < slab.B) {
      float* p = slab.at(slice, b, h0);
      p[r] = acc0[e];
      p[16 + r] = acc1[e];
    }
  }
}

// ---- 16-byte row chunks (i32x4; query_expand.hip, rerank.hip, project.hip) ---------------------------------------
// The two bf16 of a 32-bit word: element 2w in the low half, 2w + 1 in the high half.
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
// Four f32 -> four bf16 (round-to-nearest-even) in two words, element 0 lowest.
__device__ __forceinline__ uint2 pack_bf16x4(f32x4 v) {
  uint2 h;
  h.x = (uint32_t)f32_to_bf16_bits(v[0]) | ((uint32_t)f32_to_bf16_bits(v[1]) << 16);
  h.y = (uint32_t)f32_to_bf16_bits(v[2]) | ((uint32_t)f32_to_bf16_bits(v[3]) << 16);
  return h;
}

// Global row `id` of a gallery sharded by rows: true iff this shard (rows index_base .. index_base + n_local - 1) owns it,
// r = its local row.  Padding entries (id < 0) and other shards' rows are not owned.
__device__ __forceinline__ bool shard_row(int id, int n_local, int index_base, long long& r) {
  r = (long long)id - index_base;
  return r >= 0 && r < n_local;
}

// ---- the order stage of a re-rank (rerank.hip, local_match.hip) ------------------------------------------------------
// One workgroup of ORDER_MAX_KC threads per query b; thread j builds candidate j's key from scores[b, j] and idx[b, j] (the
// merge key above; a NaN score gets a key below every numeric one and above the padding; a candidate the shard does not own
// is KEY_DEAD, and its score is not read), and counts the keys ahead of it (kc^2 comparisons per query; equal keys by
// position).  Returns that rank, or -1 for a thread past kc; (val, id) is the entry to write at the rank: (score, index),
// (-inf, index) for a NaN score, (-inf, -1) for a candidate that is not live.  One barrier; s_key is LDS.
constexpr int ORDER_MAX_KC = 128;
constexpr unsigned long long KEY_NAN_HI = 1ull << 32;   // above KEY_DEAD, below orderable(-inf) = 0x007fffff
__device__ __forceinline__ int order_rank(const float* __restrict__ scores, const int32_t* __restrict__ idx, long long b, int kc,
                                          int n_local, int index_base, unsigned long long* s_key, float& val, int& id) {
  const int j = threadIdx.x;
  unsigned long long key = KEY_DEAD;
  val = -INFINITY;
  id = -1;
  if (j < kc) {
    const int cand = idx[b * kc + j];
    long long r;
    if (shard_row(cand, n_local, index_base, r)) {                    // only a live candidate's score was written
      const float s = scores[b * kc + j];
      id = cand;
      if (isnan(s)) key = KEY_NAN_HI | (uint32_t)(0x7fffffff - cand);
      else { key = make_key(s, cand); val = s; }
    }
  }
  s_key[j] = key;
  __syncthreads();
  if (j >= kc) return -1;
  int rank = 0;
  for (int i = 0; i < kc; ++i) {                                      // s_key[i]: the same address for every thread
    const unsigned long long o = s_key[i];
    rank += (o > key || (o == key && i < j)) ? 1 : 0;
  }
  return rank;
}

// The sums of a workgroup's NWAVES waves (wave_total = wave_sum(...) of the caller's value) added in ascending wave order
// through s_part[NWAVES] (LDS): the same on every thread.  One barrier; s_part must not be re-used before the next one.
template <int NWAVES>
__device__ __forceinline__ float block_sum_in_wave_order(float wave_total, float* s_part, int lane, int wave) {
  if (lane == 0) s_part[wave] = wave_total;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < NWAVES; ++w) s += s_part[w];
  return s;
}
// A squared norm nothing can be divided by: 0, NaN or Inf.
__device__ __forceinline__ bool norm_unusable(float n2) { return !(n2 > 0.f) || isinf(n2); }

}  // namespace vpr
