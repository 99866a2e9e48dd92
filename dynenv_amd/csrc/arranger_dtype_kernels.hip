// arranger_dtype_kernels.hip — the padded tensor of the arranger in a 16-BIT type (bf16 or fp16) from float32 embeddings, and the backward
// that widens a 16-bit gradient to float32 rows (include/dynenv.h, dynenv_arrange_*_as): the reference's rearrange_outputs
// (DynEnv/models/models.py:252-274, catAndPad :147-180) under torch.autocast, where the embedding blocks end in a LayerNorm and hand over
// float32 while everything behind the input layer reads 16 bits.  Both modes: the default one (counts + base, arranger_kernels.hip K5 /
// K5') and the fixed-shape one (counts + rows, arranger_fixed_kernels.hip KF3 / KF3').  Included at the very END of dynenv_capi.hip,
// behind every kernel the unit had: none of them moves.
//
// The thread-to-data map is K5's: a thread owns one 16-BYTE unit of the padded tensor - now 8 elements, f8 = 0 .. F/8-1 of player p -
// blockIdx.y is the time step, and the thread walks down its player's slots with four slots in flight before their stores.  Per slot:
//   forward   two 16-byte loads of the float32 row (floats 8*f8 .. 8*f8+7), eight conversions, one non-temporal 16-byte store;
//   backward  one non-temporal 16-byte load of the gradient, eight exact widenings, two non-temporal 16-byte stores (of units the lanes
//             of a row exchanged first, so that each store instruction writes whole lines: arrd_widen_st).
// A wave writes 1 KB contiguous per slot in the forward and reads 1 KB per slot in the backward, as K5 / K5' do.
// (Embeddings ALREADY in the padded tensor's 16-bit type need no kernel of their own: a 16-byte unit is a 16-byte unit, so the host
//  launches K5 / K5' / KF3 / KF3' with F/8 units per row instead of F/4 - a bit copy, zeros included, +0.0 being all-zero bits in every type.)
//
// Conversion contract.  float32 -> 16 bit is IEEE round to nearest, ties to even: overflow to infinity, fp16 subnormal results, underflow
// to a signed zero, +-0 and +-inf unchanged; a NaN stays a NaN (its payload is the hardware's).  Written as plain casts of two-element
// vectors, so the compiler picks the packed convert (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 on gfx950).  16 bit -> float32 is exact for every
// bit pattern: a shift for bf16, a cast for fp16 (subnormals included - the unit is built with denormals on, the compiler's default).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"

// ArrFixedRows is declared at the top of dynenv_capi.hip; ARR_BLOCK and arr_f4 are arranger_kernels.hip's.
typedef unsigned arr_u4 __attribute__((ext_vector_type(4)));
typedef float arr_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 arr_bf2 __attribute__((ext_vector_type(2)));
typedef _Float16 arr_h2 __attribute__((ext_vector_type(2)));

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

// one unit of the padded tensor from the two float4s of its embedding row
template <class CV>
__device__ __forceinline__ arr_u4 arrd_narrow(const float4& a, const float4& b) {
  const arr_u4 w = {CV::pack(a.x, a.y), CV::pack(a.z, a.w), CV::pack(b.x, b.y), CV::pack(b.z, b.w)};
  return w;
}
__device__ __forceinline__ void arrd_st(arr_u4* p, arr_u4 w) { __builtin_nontemporal_store(w, p); }
// The widening backward writes 32 bytes per unit it reads.  Stored by the thread that read the unit - two 16-byte stores 16 bytes apart -
// every store instruction of a wave covers every other 16 bytes of 2 KB: half lines, which non-temporal stores do not merge (measured,
// 4096 environments, F = 128: 3.4 TB/s and 1.3 x the float32 backward's TIME on the dense configurations).  So the lanes of a GROUP - the
// G consecutive lanes that share a row, G the largest power of two that divides F/8, at most 64 - exchange their units first
// (ds_bpermute: the LDS crossbar, no memory): lane g of the group stores float4 g of the group's 2 G float4s with the first instruction
// and float4 G + g with the second, so each instruction writes 16 G contiguous bytes per group (F = 128: 256 bytes, two whole lines).
// A group shares its player, hence its counts and its control flow: the lanes a lane reads from are active whenever it is.
// ARRD_BWD_EXCHANGE = 0 rebuilds the direct form (G = 1), ARRD_BWD_NT_STORE = 0 plain stores, for an A/B.
#ifndef ARRD_BWD_EXCHANGE
#define ARRD_BWD_EXCHANGE 1
#endif
#ifndef ARRD_BWD_NT_STORE
#define ARRD_BWD_NT_STORE 1
#endif
struct ArrdLane {
  int srcA, srcB;   // byte index (lane * 4) of the lane whose unit holds this lane's first / second float4
  bool hiA, hiB;    // ... and whether it is that unit's upper half
  int offA, offB;   // floats from the start of the thread's own unit in the row to where this lane stores
};
__device__ __forceinline__ ArrdLane arrd_lane(int G) {
  if (!ARRD_BWD_EXCHANGE) G = 1;
  const int lane = (int)(threadIdx.x & 63), g = lane & (G - 1), l0 = lane - g;
  const int mA = g, mB = G + g;   // float4s of the group this lane stores
  ArrdLane L;
  L.srcA = (l0 + (mA >> 1)) << 2; L.srcB = (l0 + (mB >> 1)) << 2;
  L.hiA = mA & 1; L.hiB = mB & 1;
  L.offA = 4 * mA - 8 * g; L.offB = 4 * mB - 8 * g;
  return L;
}
__device__ __forceinline__ void arrd_st_f4(float* p, arr_f2 lo, arr_f2 hi) {
  const arr_f4 w = {lo.x, lo.y, hi.x, hi.y};
#if ARRD_BWD_NT_STORE
  __builtin_nontemporal_store(w, reinterpret_cast<arr_f4*>(p));
#else
  *reinterpret_cast<arr_f4*>(p) = w;
#endif
}
__device__ __forceinline__ unsigned arrd_from(int src, unsigned v) { return (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)v); }
// the two float4s this lane stores for one slot, from the units its group read; dst is the start of the thread's OWN unit in the row
template <class CV>
__device__ __forceinline__ void arrd_widen_st(float* dst, arr_u4 w, const ArrdLane& L) {
  const unsigned ax = arrd_from(L.srcA, w.x), ay = arrd_from(L.srcA, w.y), az = arrd_from(L.srcA, w.z), aw = arrd_from(L.srcA, w.w);
  const unsigned bx = arrd_from(L.srcB, w.x), by = arrd_from(L.srcB, w.y), bz = arrd_from(L.srcB, w.z), bw = arrd_from(L.srcB, w.w);
  arrd_st_f4(dst + L.offA, CV::widen(L.hiA ? az : ax), CV::widen(L.hiA ? aw : ay));
  arrd_st_f4(dst + L.offB, CV::widen(L.hiB ? bz : bx), CV::widen(L.hiB ? bw : by));
}
__device__ __forceinline__ void arrd_zero_st(float* dst, const ArrdLane& L) {
  const arr_f2 z = {0.f, 0.f};
  arrd_st_f4(dst + L.offA, z, z);
  arrd_st_f4(dst + L.offB, z, z);
}

// The count of type i kept by this player, clamped so that every access stays in bounds whatever the counts hold: to the slots left, to
// rows[i] in the fixed mode, and to zero from below.
template <bool FIXED>
__device__ __forceinline__ int arrd_count(const int32_t* __restrict__ counts, const ArrFixedRows& rw, int i, int TP, int tp, int left) {
  int c = counts[(size_t)i * TP + tp];
  if (FIXED) c = c > rw.rows[i] ? rw.rows[i] : c;
  c = c > left ? left : c;
  return c < 0 ? 0 : c;
}

// forward: FIXED = false is K5's walk (the rows of (t, p) start at base_i(t, p)), FIXED = true KF3's (at tp * rows[i]).  Plain loads of
// the embeddings (what K5 and KF3 settled on), non-temporal stores.
template <class CV, bool FIXED>
__device__ __forceinline__ void arrd_pad_body(const float* e0, const float* e1, const float* e2, const float* e3,
                                              const int32_t* __restrict__ counts, const int32_t* __restrict__ base, const ArrFixedRows& rw,
                                              int nTypes, int T, int P, int maxCount, int F8, arr_u4* __restrict__ padded) {
  const unsigned x = blockIdx.x * ARR_BLOCK + threadIdx.x;
  if (x >= (unsigned)P * (unsigned)F8) return;
  const int p = (int)(x / (unsigned)F8), f = (int)(x % (unsigned)F8);
  const int t = (int)blockIdx.y, TP = T * P, tp = t * P + p;
  const size_t stride = (size_t)P * F8;  // units between consecutive slots of one column
  const size_t F4 = (size_t)F8 * 2;      // float4s of an embedding row
  arr_u4* out = padded + (size_t)t * maxCount * stride + x;
  const arr_u4 zero = {0u, 0u, 0u, 0u};
  int j = 0;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= nTypes || j >= maxCount) break;
    const int c = arrd_count<FIXED>(counts, rw, i, TP, tp, maxCount - j);
    const float* e = i == 0 ? e0 : i == 1 ? e1 : i == 2 ? e2 : e3;
    if (e) {
      const size_t row0 = FIXED ? (size_t)tp * rw.rows[i] : (size_t)base[(size_t)i * TP + tp];
      const float4* src = reinterpret_cast<const float4*>(e) + row0 * F4 + 2 * f;
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        const float4 a0 = src[(size_t)(k + 0) * F4], b0 = src[(size_t)(k + 0) * F4 + 1], a1 = src[(size_t)(k + 1) * F4], b1 = src[(size_t)(k + 1) * F4 + 1],
                     a2 = src[(size_t)(k + 2) * F4], b2 = src[(size_t)(k + 2) * F4 + 1], a3 = src[(size_t)(k + 3) * F4], b3 = src[(size_t)(k + 3) * F4 + 1];
        arrd_st(out, arrd_narrow<CV>(a0, b0)); arrd_st(out + stride, arrd_narrow<CV>(a1, b1));
        arrd_st(out + 2 * stride, arrd_narrow<CV>(a2, b2)); arrd_st(out + 3 * stride, arrd_narrow<CV>(a3, b3));
        out += 4 * stride;
      }
      for (; k < c; ++k) { arrd_st(out, arrd_narrow<CV>(src[(size_t)k * F4], src[(size_t)k * F4 + 1])); out += stride; }
    } else {
      for (int k = 0; k < c; ++k) { arrd_st(out, zero); out += stride; }
    }
    j += c;
  }
  for (; j < maxCount; ++j) { arrd_st(out, zero); out += stride; }
}

// backward: K5' (FIXED = false) / KF3' (FIXED = true).  Every row of every non-NULL g_i is written exactly once - in the fixed mode the
// rows behind the kept ones get +0.0 - a NULL g_i is stepped over unread, padding slots of the gradient are never read.  Non-temporal
// loads and stores (what K5' and KF3' settled on).
template <class CV, bool FIXED>
__device__ __forceinline__ void arrd_unpad_body(const arr_u4* __restrict__ grad, const int32_t* __restrict__ counts, const int32_t* __restrict__ base,
                                                const ArrFixedRows& rw, int nTypes, int T, int P, int maxCount, int F8, int G,
                                                float* __restrict__ g0, float* __restrict__ g1, float* __restrict__ g2, float* __restrict__ g3) {
  const unsigned x = blockIdx.x * ARR_BLOCK + threadIdx.x;
  if (x >= (unsigned)P * (unsigned)F8) return;
  const int p = (int)(x / (unsigned)F8), f = (int)(x % (unsigned)F8);
  const int t = (int)blockIdx.y, TP = T * P, tp = t * P + p;
  const size_t stride = (size_t)P * F8;  // units between consecutive slots of one column
  const size_t F = (size_t)F8 * 8;       // floats of an embedding row
  const arr_u4* in = grad + (size_t)t * maxCount * stride + x;
  const ArrdLane L = arrd_lane(G);
  int j = 0;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= nTypes) break;
    if (!FIXED && j >= maxCount) break;   // (the fixed mode goes on: the later types' rows are still to be zeroed)
    const int n = FIXED ? rw.rows[i] : 0;
    const int c = arrd_count<FIXED>(counts, rw, i, TP, tp, maxCount - j);
    float* g = i == 0 ? g0 : i == 1 ? g1 : i == 2 ? g2 : g3;
    if (g && (FIXED || c > 0)) {
      const size_t row0 = FIXED ? (size_t)tp * n : (size_t)base[(size_t)i * TP + tp];
      float* dst = g + row0 * F + 8 * f;
      const arr_u4* src = in;
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        const arr_u4 v0 = __builtin_nontemporal_load(src), v1 = __builtin_nontemporal_load(src + stride),
                     v2 = __builtin_nontemporal_load(src + 2 * stride), v3 = __builtin_nontemporal_load(src + 3 * stride);
        arrd_widen_st<CV>(dst + (size_t)(k + 0) * F, v0, L); arrd_widen_st<CV>(dst + (size_t)(k + 1) * F, v1, L);
        arrd_widen_st<CV>(dst + (size_t)(k + 2) * F, v2, L); arrd_widen_st<CV>(dst + (size_t)(k + 3) * F, v3, L);
        src += 4 * stride;
      }
      for (; k < c; ++k) { arrd_widen_st<CV>(dst + (size_t)k * F, __builtin_nontemporal_load(src), L); src += stride; }
      if (FIXED)
        for (; k < n; ++k) arrd_zero_st(dst + (size_t)k * F, L);
    }
    in += (size_t)c * stride;
    j += c;
  }
}

#define ARRD_KERNELS(NAME, CV)                                                                                                               \
  extern "C" __global__ void __launch_bounds__(ARR_BLOCK)                                                                                    \
  arr_pad_cols_##NAME##_kernel(const float* __restrict__ e0, const float* __restrict__ e1, const float* __restrict__ e2,                     \
                               const float* __restrict__ e3, const int32_t* __restrict__ counts, const int32_t* __restrict__ base,           \
                               int nTypes, int T, int P, int maxCount, int F8, arr_u4* __restrict__ padded) {                                \
    arrd_pad_body<CV, false>(e0, e1, e2, e3, counts, base, ArrFixedRows(), nTypes, T, P, maxCount, F8, padded);                             \
  }                                                                                                                                          \
  extern "C" __global__ void __launch_bounds__(ARR_BLOCK)                                                                                    \
  arr_unpad_cols_##NAME##_kernel(const arr_u4* __restrict__ grad, const int32_t* __restrict__ counts, const int32_t* __restrict__ base,      \
                                 int nTypes, int T, int P, int maxCount, int F8, int G, float* __restrict__ g0,                              \
                                 float* __restrict__ g1, float* __restrict__ g2, float* __restrict__ g3) {                                   \
    arrd_unpad_body<CV, false>(grad, counts, base, ArrFixedRows(), nTypes, T, P, maxCount, F8, G, g0, g1, g2, g3);                           \
  }                                                                                                                                          \
  extern "C" __global__ void __launch_bounds__(ARR_BLOCK)                                                                                    \
  arrf_pad_cols_##NAME##_kernel(const float* __restrict__ e0, const float* __restrict__ e1, const float* __restrict__ e2,                    \
                                const float* __restrict__ e3, const int32_t* __restrict__ counts, ArrFixedRows rw, int nTypes, int T, int P, \
                                int maxCount, int F8, arr_u4* __restrict__ padded) {                                                         \
    arrd_pad_body<CV, true>(e0, e1, e2, e3, counts, nullptr, rw, nTypes, T, P, maxCount, F8, padded);                                       \
  }                                                                                                                                          \
  extern "C" __global__ void __launch_bounds__(ARR_BLOCK)                                                                                    \
  arrf_unpad_cols_##NAME##_kernel(const arr_u4* __restrict__ grad, const int32_t* __restrict__ counts, ArrFixedRows rw, int nTypes, int T,   \
                                  int P, int maxCount, int F8, int G, float* __restrict__ g0, float* __restrict__ g1,                        \
                                  float* __restrict__ g2, float* __restrict__ g3) {                                                          \
    arrd_unpad_body<CV, true>(grad, counts, nullptr, rw, nTypes, T, P, maxCount, F8, G, g0, g1, g2, g3);                                    \
  }
ARRD_KERNELS(bf16, ArrBf16)
ARRD_KERNELS(f16, ArrF16)
