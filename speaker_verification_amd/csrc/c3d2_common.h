// Device leaf helpers shared by the C3D2 network kernels (c3d2.hip, c3d2_tail.hip): vector types, PReLU, the (h, l) split of
// the two-piece f16 products and the few statements every two-piece kernel repeats: the piece products of a K = 32 block
// (mfma_pieces), the split-and-park of staged values (park_pieces), the pooled epilogue (prelu_pool_store) and the prologue's
// loads (load_wblk, load_bias_slope).  Leaf code only: item loops, staging schedules, tile walks, prefetch depths, barriers and
// sched_barriers stay in the kernels (c3d2.hip's first block splits its own kernel into phases; those are its own, not shared).
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ float prelu(float v, float slope) { return v > 0.f ? v : slope * v; }
// 0 <= slope <= 1 (nn.PReLU starts at 0.25 and trained slopes stay there): prelu(v) = max(v, slope v), two
// instructions instead of compare / multiply / select (+ a wait state); bit-identical for finite v.
template <bool SLOPE01>
__device__ __forceinline__ float prelu_t(float v, float slope) {
  return SLOPE01 ? fmaxf(v, slope * v) : prelu(v, slope);
}

// prelu for 0 <= slope <= 1 straight off MFMA accumulators: fmaxf() on a value the compiler cannot prove canonical costs a
// third instruction (v_max x, x in front of the real one) and the product is one v_mul per value; written as vectors it is one
// v_pk_mul_f32 per PAIR + one v_max_f32 per value (12 -> 6 instructions per four values; the same product, the same
// maximum: bit-identical for every finite and infinite input, NaN stays NaN).
// (the product is left to the compiler -- it selects v_pk_mul_f32 for a two-float vector product and, unlike for an asm
// statement, counts the wait states between an MFMA and the first instruction that reads its result; the v_max behind it
// depends on that product, so it is issued later still)
__device__ __forceinline__ f32x2 pk_mul(f32x2 a, f32x2 b) { return a * b; }
__device__ __forceinline__ float max_raw(float a, float b) {
  float d;
  asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
template <bool SLOPE01>
__device__ __forceinline__ f32x4 prelu4(f32x4 v, f32x4 slope) {
  f32x4 o;
  if (SLOPE01) {
    const f32x2 m0 = pk_mul(__builtin_shufflevector(v, v, 0, 1), __builtin_shufflevector(slope, slope, 0, 1));
    const f32x2 m1 = pk_mul(__builtin_shufflevector(v, v, 2, 3), __builtin_shufflevector(slope, slope, 2, 3));
    o[0] = max_raw(v[0], m0[0]);
    o[1] = max_raw(v[1], m0[1]);
    o[2] = max_raw(v[2], m1[0]);
    o[3] = max_raw(v[3], m1[1]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = prelu(v[r], slope[r]);
  }
  return o;
}

// (h, l) of two f32 values as two packed-half words: {h0, h1}, {l0, l1}
__device__ __forceinline__ void split2(f32x2 v, unsigned& h, unsigned& l) {
  const f16x2 hh = __builtin_convertvector(v, f16x2);
  h = __builtin_bit_cast(unsigned, hh);
  // l = f16(x - f32(h)) as ONE instruction per value: v_fma_mix reads h as a half and x as a float, multiplies by -1 and rounds the
  // f32 result (exact: x - h has at most 13 significant bits) into one half of the destination -- where the compiler's own code is
  // two v_cvt_f32_f16, a packed subtract and v_cvt_pk_f16_f32.  Bit-identical on 2^22 random pairs incl. denormals, NaN, infinities.
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(h), "v"(v[0]));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(h), "v"(v[1]));
}

// max(x, x of lane ^ 1) as ONE instruction (DPP quad_perm [1, 0, 3, 2] on the first source).  Written out: four calls of
// __builtin_amdgcn_mov_dpp on the four registers of an accumulator came back as one v_mov_b32_dpp of the first (ROCm 7.2).
// (the s_nop: a DPP read of a register the previous vector instruction wrote needs two wait states, and the compiler does not
// count them for asm statements)
__device__ __forceinline__ float max_with_lane_xor1(float x) {
  float d;
  asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(x));
  return d;
}

// acc + W x b through the three piece products of a K = 32 block, in the order H x h, H x l, L x h (W = (WH, WL), b = (bh, bl)).
// `with_l` = false leaves H x l out: a block whose fragment bh already holds [h | l] (conv1_2's last tap)
__device__ __forceinline__ f32x4 mfma_pieces(u32x4 WH, u32x4 WL, u32x4 bh, u32x4 bl, f32x4 acc, bool with_l = true) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, WH), __builtin_bit_cast(f16x8, bh), acc, 0, 0, 0);
  if (with_l) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, WH), __builtin_bit_cast(f16x8, bl), acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, WL), __builtin_bit_cast(f16x8, bh), acc, 0, 0, 0);
}

// The pooled epilogue of conv1_2 and conv2_2: PReLU, max over the column pair (lanes i, i ^ 1: the same depth and row), and the
// lane that holds the pair's maximum for the output (`store`: an even lane inside the item) stores its four channels
template <bool SLOPE01>
__device__ __forceinline__ void prelu_pool_store(f32x4 acc, f32x4 slope, float* dst, bool store) {
  const f32x4 y = prelu4<SLOPE01>(acc, slope);
  f32x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = max_with_lane_xor1(y[r]);
  if (store) *reinterpret_cast<f32x4*>(dst) = o;
}

// Four staged f32 values -> their h halves at dst, their l halves l_off words on.  The split is unconditional and only the two
// stores are under `live` (a thread past the end of the staged region): the guard around the split as well is other code.
__device__ __forceinline__ void park_pieces(unsigned* dst, int l_off, f32x4 v, bool live) {
  unsigned h0, l0, h1, l1;
  split2(__builtin_shufflevector(v, v, 0, 1), h0, l0);
  split2(__builtin_shufflevector(v, v, 2, 3), h1, l1);
  if (live) {
    *reinterpret_cast<u32x2*>(dst) = (u32x2){h0, h1};
    *reinterpret_cast<u32x2*>(dst + l_off) = (u32x2){l0, l1};
  }
}

// bias and slope of channels 16 nt + 4 kk .. + 3: what lane group kk of N tile nt holds of ONE position (A = the weights)
__device__ __forceinline__ void load_bias_slope(const float* bias, const float* slope, int nt, int kk, f32x4& b4, f32x4& sl4) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    b4[r] = bias[16 * nt + 4 * kk + r];
    sl4[r] = slope[16 * nt + 4 * kk + r];
  }
}

// N weight blocks (H, L) of a [..][2][64 lanes] table, from block `first` on
template <int N>
__device__ __forceinline__ void load_wblk(const u32x4* wblk, int first, int lane, u32x4 (&W)[N][2]) {
#pragma unroll
  for (int t = 0; t < N; ++t) {
    W[t][0] = wblk[((first + t) * 2) * 64 + lane];
    W[t][1] = wblk[((first + t) * 2 + 1) * 64 + lane];
  }
}

}  // namespace
