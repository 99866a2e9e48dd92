// mma_tiles.h - the 16x16x32 tile toolkit of the arranger's 16-bit kernels, the attention and the model kernels (recurrent, policy,
// rollout, icm, icm backward, policy eval): the 16-bit conversions, the MFMA wrapper, fragment loads and packed stores, the sums over a
// row, a strip or the four waves, and the small per-element idioms those kernels share.  Device code only, all of it inlined; every
// file that uses a name of this header includes it.  DESIGN.md ("The tile toolkit") has the orientation, what a lane holds and which
// helper owns which layout.  The prefixes arr_ / Arr and atp_ / Atp are historical - the arranger's column kernels and the attention
// were the first users - and kept for the call sites' sake; mt_ is what was added once a third file needed it.
// The unit is built with -ffp-contract=off and results are compared bit for bit: an expression here keeps its order of operations.
#ifndef DYNENV_MMA_TILES_H
#define DYNENV_MMA_TILES_H
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned arr_u4 __attribute__((ext_vector_type(4)));
typedef float arr_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 arr_bf2 __attribute__((ext_vector_type(2)));
typedef _Float16 arr_h2 __attribute__((ext_vector_type(2)));
typedef unsigned short atp_h;   // a 16-bit element, whichever type
typedef float atp_f4 __attribute__((ext_vector_type(4)));
typedef unsigned atp_u2 __attribute__((ext_vector_type(2)));
typedef __bf16 atp_bf8 __attribute__((ext_vector_type(8)));
typedef _Float16 atp_h8 __attribute__((ext_vector_type(8)));

// ---- the 16-bit types (the conversion contract: arranger_cols_kernels.hip)
struct ArrBf16 {
  static __device__ __forceinline__ unsigned pack(float a, float b) {
    const arr_f2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, arr_bf2));
  }
  static __device__ __forceinline__ arr_f2 widen(unsigned w) {
    const arr_f2 v = {__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
    return v;
  }
};
struct ArrF16 {
  static __device__ __forceinline__ unsigned pack(float a, float b) {
    const arr_f2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, arr_h2));
  }
  static __device__ __forceinline__ arr_f2 widen(unsigned w) { return __builtin_convertvector(__builtin_bit_cast(arr_h2, w), arr_f2); }
};

// ---- products and fragments
template <class CV> struct AtpMma;
template <> struct AtpMma<ArrBf16> {
  static __device__ __forceinline__ atp_f4 mma(arr_u4 a, arr_u4 b, atp_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(atp_bf8, a), __builtin_bit_cast(atp_bf8, b), c, 0, 0, 0);
  }
};
template <> struct AtpMma<ArrF16> {
  static __device__ __forceinline__ atp_f4 mma(arr_u4 a, arr_u4 b, atp_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(atp_h8, a), __builtin_bit_cast(atp_h8, b), c, 0, 0, 0);
  }
};

__device__ __forceinline__ arr_u4 atp_ld16(const atp_h* p) { return *reinterpret_cast<const arr_u4*>(p); }
template <class CV> __device__ __forceinline__ void atp_st4(atp_h* p, atp_f4 v) {   // four consecutive elements, rounded to nearest even
  const atp_u2 w = {CV::pack(v.x, v.y), CV::pack(v.z, v.w)};
  *reinterpret_cast<atp_u2*>(p) = w;
}
template <class CV> __device__ __forceinline__ atp_f4 atp_ld4(const atp_h* p) {      // ... widened exactly
  const atp_u2 w = *reinterpret_cast<const atp_u2*>(p);
  const arr_f2 lo = CV::widen(w.x), hi = CV::widen(w.y);
  const atp_f4 v = {lo.x, lo.y, hi.x, hi.y};
  return v;
}
template <class CV> __device__ __forceinline__ atp_f4 atp_round4(atp_f4 v) {         // what the 16-bit store keeps of v
  const arr_f2 lo = CV::widen(CV::pack(v.x, v.y)), hi = CV::widen(CV::pack(v.z, v.w));
  const atp_f4 r = {lo.x, lo.y, hi.x, hi.y};
  return r;
}
__device__ __forceinline__ atp_f4 mt_ldf4(const float* p) { return *reinterpret_cast<const atp_f4*>(p); }
// the four scalar stores of an accumulator into a row of 33 floats (the logits' LDS rows: not 16-byte aligned)
__device__ __forceinline__ void mt_st_f4(float* q, const atp_f4& v) { q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
template <class CV> __device__ __forceinline__ atp_h mt_h(float v) { return (atp_h)(CV::pack(v, 0.f) & 0xffffu); }

// four consecutive elements of a row, packed in lo and hi, down a column of the transposed tile (RS elements per row): t = tile + r
template <int RS> __device__ __forceinline__ void mt_st_tr(atp_h* t, unsigned lo, unsigned hi) {
  t[0] = (atp_h)(lo & 0xffffu); t[RS] = (atp_h)(lo >> 16); t[2 * RS] = (atp_h)(hi & 0xffffu); t[3 * RS] = (atp_h)(hi >> 16);
}
// ... row-major into rm, and into column r of the transposed tile
template <int RS> __device__ __forceinline__ void mt_st_both(atp_h* rm, atp_h* tr, int r, unsigned lo, unsigned hi) {
  const atp_u2 w = {lo, hi};
  *reinterpret_cast<atp_u2*>(rm) = w;
  mt_st_tr<RS>(tr + r, lo, hi);
}
template <class CV, int RS> __device__ __forceinline__ void mt_st4_both(atp_h* rm, atp_h* tr, int r, atp_f4 v) {
  mt_st_both<RS>(rm, tr, r, CV::pack(v.x, v.y), CV::pack(v.z, v.w));
}

// a = hi + lo to 16 significant bits, both bf16 (two values at once): the rounding and what it left, rounded
__device__ __forceinline__ void mt_split(float a, float b, unsigned& hi, unsigned& lo) {
  hi = ArrBf16::pack(a, b);
  const arr_f2 w = ArrBf16::widen(hi);
  lo = ArrBf16::pack(a - w.x, b - w.y);
}
// acc + A B with the bf16 operands as pairs: (ah + al)(bh + bl) without al bl, which lies 16 bits below the product
template <bool SPLIT>
__device__ __forceinline__ atp_f4 mt_mma_split(arr_u4 ah, arr_u4 al, arr_u4 bh, arr_u4 bl, atp_f4 acc) {
  acc = AtpMma<ArrBf16>::mma(ah, bh, acc);
  if constexpr (SPLIT) {
    acc = AtpMma<ArrBf16>::mma(ah, bl, acc);
    acc = AtpMma<ArrBf16>::mma(al, bh, acc);
  }
  return acc;
}

// ---- sums, each in one fixed order
// the sum over a player row: this lane's part, then the three other quarters of the wave (same lane & 15)
__device__ __forceinline__ float atp_row_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float atp_row_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}
__device__ __forceinline__ float atp_sum4(atp_f4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ atp_f4 mt_sum16(atp_f4 v) {   // over the rows of a strip: the 16 lanes of equal lane >> 4
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {
    atp_f4 o;
    o.x = __shfl_xor(v.x, m, 64); o.y = __shfl_xor(v.y, m, 64); o.z = __shfl_xor(v.z, m, 64); o.w = __shfl_xor(v.w, m, 64);
    v += o;
  }
  return v;
}
__device__ __forceinline__ float mt_sum16(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// the four waves' parts of a sum, `stride` floats apart in LDS, added in wave order
__device__ __forceinline__ float mt_wave_sum4(const float* q, int stride) { return ((q[0] + q[stride]) + q[2 * stride]) + q[3 * stride]; }

// ---- per element
__device__ __forceinline__ float mt_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ atp_f4 mt_leaky4(atp_f4 v, float slope) {
  v.x = v.x > 0.f ? v.x : v.x * slope; v.y = v.y > 0.f ? v.y : v.y * slope;
  v.z = v.z > 0.f ? v.z : v.z * slope; v.w = v.w > 0.f ? v.w : v.w * slope;
  return v;
}
__device__ __forceinline__ unsigned mt_pos4(atp_f4 v) {   // bit i: element i > 0
  return (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
}
// v times the LeakyReLU's derivative at the pre-activation whose mt_pos4 is the low four bits of m
__device__ __forceinline__ atp_f4 mt_leaky_grad4(atp_f4 v, unsigned m, float slope) {
  v.x = (m & 1u) ? v.x : v.x * slope; v.y = (m & 2u) ? v.y : v.y * slope;
  v.z = (m & 4u) ? v.z : v.z * slope; v.w = (m & 8u) ? v.w : v.w * slope;
  return v;
}

// ---- the discrete action groups as the host packs them (model_groups, dynenv_host.h): 8 bits per group in group_off - the first
// logit of group g - and 4 bits per group in group_n: n_g - 1
struct MtGroup { int off, n; };   // the first logit of the group, its size
__device__ __forceinline__ MtGroup mt_group(unsigned long long group_off, unsigned group_n, int g) {
  const MtGroup r = {(int)((group_off >> (8 * g)) & 255u), (int)((group_n >> (4 * g)) & 15u) + 1};
  return r;
}
// a stored action of a group whose last action is `last`: rounded to the nearest integer and clamped into the group
__device__ __forceinline__ int mt_stored_action(float value, int last, bool& clamped) {
  const float v = rintf(value);
  const bool ok = v >= 0.f && v <= (float)last;
  clamped |= !ok;
  return ok ? (int)v : v > (float)last ? last : 0;
}
#endif
