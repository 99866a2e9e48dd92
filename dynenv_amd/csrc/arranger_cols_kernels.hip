// arranger_cols_kernels.hip — the padded tensor of the arranger in one pass, and its backward: the reference's rearrange_outputs
// (DynEnv/models/models.py:252-274, catAndPad :147-180) and autograd's derivative of it (a slice per embedding row, nothing summed).
// ONE column walk behind twelve kernels: default mode (counts + base) / fixed-shape mode (counts + rows), forward / backward, and three
// relations between a 16-byte unit of the padded tensor and an embedding row - a copy, float32 -> bf16, float32 -> fp16
// (include/dynenv.h, dynenv_arrange_{,fixed_}pad{,_backward}{,_as}).  Included directly behind arranger_kernels.hip, in front of the
// host code: everything a RoboCup step launches lies in front of arr_count_kernel and does not move (rc_layout_pad, robocup_kernels.hip).
//
// The walk (K5 forward, K5' backward).  One thread per 16-BYTE unit column (t, p, f) of padded[t][:][p][:] - blockIdx.y is the time
// step - walking down its player's slots j = 0 .. maxCount-1 (round 1-4: one thread per slot, 3.8-4.4 TB/s; this form 5.0-5.7 TB/s):
// the counts and row starts of the player are read once (not once per slot), the index arithmetic is one add per slot, and four
// independent 16-byte loads are in flight per thread before their stores.  A wave writes 1 KB contiguous per slot in the forward and
// reads 1 KB per slot in the backward; the other side walks the player's consecutive embedding rows.  HBM-bound: the padded tensor is
// written once and every embedding read once, no pre-zeroing; in the backward every row of every non-NULL g_i is written exactly once
// (each row owns one slot; in the fixed mode the rows behind the kept ones get +0.0 - the block ran on those zero rows and its output
// was discarded), a NULL g_i is stepped over unread, padding slots of the gradient are never read: no atomics, no second pass.
//   forward   padded[t][j][p][f] = unit of e_i[row0_i(t,p) + k][f],  j = sum_{i'<i} c_i' + k,  zeros behind the last object
//   backward  g_i[row0_i(t,p) + k][f] = unit of grad[t][j][p][f]
//   row0_i(t,p) = base_i(t,p) (default mode) or tp * rows[i] (fixed mode)
//
// What a unit is (the Unit policy of the two bodies):
//   ArrCopy       one 16-byte piece of the row per unit: float32 to float32 with F/4 units per row, or embeddings ALREADY in a 16-bit
//                 padded tensor's type with F/8 (a bit copy, zeros included, +0.0 being all-zero bits in every type).
//   ArrNarrow<CV> two float4 pieces of a float32 row per unit of 8 16-bit elements: the forward narrows, the backward widens and stores
//                 two float4s (of units the lanes of a row exchanged first: arrd_widen_st).
// Conversion contract.  float32 -> 16 bit is IEEE round to nearest, ties to even: overflow to infinity, fp16 subnormal results, underflow
// to a signed zero, +-0 and +-inf unchanged; a NaN stays a NaN (its payload is the hardware's).  Written as plain casts of two-element
// vectors, so the compiler picks the packed convert (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 on gfx950).  16 bit -> float32 is exact for every
// bit pattern: a shift for bf16, a cast for fp16 (subnormals included - the unit is built with denormals on, the compiler's default).
//
// Which loads and stores are non-temporal, and why (4096 environments, F = 128 throughout).  Each switch rebuilds the other form for an A/B.
//   Forward stores: non-temporal (the padded tensor is written once and not read here) - worth 15-25 % where most slots are padding
//     zeros, nothing where most carry an embedding.
//   Forward loads of the embeddings, ARR_PAD_NT_LOAD = 0: non-temporal loads gain 5-10 % on dense inputs and lose 17 % on sparse ones in
//     the default mode.  Fixed mode, A/B of libraries, tools/fixed_arranger_time.py, medians of 5 x 40 calls of gather + pad + backward,
//     in us for Driving Full / Driving Partial at M = 96 and at M = 35 / RoboCup Full; the product library before and after the
//     variants: 722-729 / 808-820, 615-618 / 827-837; non-temporal loads: 711 / 844, 645 / 818: 2 % gained on the two dense cases, 3-4 %
//     lost on the sparse one, the same signs: not used.
//   Backward loads and stores, ARR_BWD_NT_LOAD = 1 and ARR_BWD_NT_STORE = 1 (the gradient is read once and every row written once).
//     Default mode, four builds taking turns, three runs each, medians in ms for Driving Full (77 % of the slots carry an object) /
//     RoboCup (100 %) / Driving Partial (19 %):  plain 0.286-0.304 / 0.376-0.377 / 0.052-0.053;  loads only 0.270-0.299 / 0.373 / 0.047;
//     stores only 0.286-0.290 / 0.361-0.364 / 0.0426-0.0429;  both 0.278-0.279 / 0.349-0.350 / 0.048.  Stores alone never lose and are
//     the best form of the sparse case (-18 %); both gain 7 % on the two dense cases, where the time is, and still 8 % on the sparse one.
//     Fixed mode (the A/B above), plain loads of the gradient: 749 / 848, 641 / 860: 3-4 % slower everywhere, in a run whose
//     default-mode legs were 0.5-10 % slower too; no case in which the plain load wins.
//     Not measured: what the rows' next reader - the embedding block's own backward - pays or saves; at these sizes, 130 MB to 1 GB of
//     rows, they do not stay in L2 either way.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "mma_tiles.h"

#ifndef ARR_PAD_NT_LOAD
#define ARR_PAD_NT_LOAD 0
#endif
#ifndef ARR_BWD_NT_LOAD
#define ARR_BWD_NT_LOAD 1
#endif
#ifndef ARR_BWD_NT_STORE
#define ARR_BWD_NT_STORE 1
#endif
#ifndef ARRD_BWD_EXCHANGE
#define ARRD_BWD_EXCHANGE 1
#endif

// ARR_BLOCK and arr_f4 are arranger_kernels.hip's.
struct ArrFixedRows { int rows[DYNENV_ARR_MAX_TYPES]; };   // rows[i] of the fixed mode, by value

// (NT a template argument, not a function's: two loads that differ only in the hint are merged, hint lost, before the call is inlined)
template <bool NT, class V> __device__ __forceinline__ V arr_ld(const V* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, class V> __device__ __forceinline__ void arr_st(V* p, V v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// The widening backward writes 32 bytes per unit it reads.  Stored by the thread that read the unit - two 16-byte stores 16 bytes apart -
// every store instruction of a wave covers every other 16 bytes of 2 KB: half lines, which non-temporal stores do not merge (measured,
// 4096 environments, F = 128: 3.4 TB/s and 1.3 x the float32 backward's TIME on the dense configurations).  So the lanes of a GROUP - the
// G consecutive lanes that share a row, G the largest power of two that divides F/8, at most 64 - exchange their units first
// (ds_bpermute: the LDS crossbar, no memory): lane g of the group stores float4 g of the group's 2 G float4s with the first instruction
// and float4 G + g with the second, so each instruction writes 16 G contiguous bytes per group (F = 128: 256 bytes, two whole lines).
// A group shares its player, hence its counts and its control flow: the lanes a lane reads from are active whenever it is.
// ARRD_BWD_EXCHANGE = 0 rebuilds the direct form (G = 1) for an A/B.
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
  arr_st<ARR_BWD_NT_STORE>(reinterpret_cast<arr_f4*>(p), w);
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

// The Unit policies.  PIECES: 16-byte pieces of an embedding row per unit;  load: the unit from its pieces at src (forward);
// store / zero: the unit, or +0.0, to its pieces at dst (backward);  Lane: what a lane keeps for its stores.
struct ArrCopy {
  static constexpr int PIECES = 1;
  struct Lane {};
  static __device__ __forceinline__ Lane lane(int) { return Lane(); }
  static __device__ __forceinline__ arr_u4 load(const arr_u4* src) { return arr_ld<ARR_PAD_NT_LOAD>(src); }
  static __device__ __forceinline__ void store(arr_u4* dst, arr_u4 w, const Lane&) { arr_st<ARR_BWD_NT_STORE>(dst, w); }
  static __device__ __forceinline__ void zero(arr_u4* dst, const Lane& L) { const arr_u4 z = {0u, 0u, 0u, 0u}; store(dst, z, L); }
};
template <class CV>
struct ArrNarrow {
  static constexpr int PIECES = 2;
  typedef ArrdLane Lane;
  static __device__ __forceinline__ Lane lane(int G) { return arrd_lane(G); }
  static __device__ __forceinline__ arr_u4 load(const arr_u4* src) {
    const arr_f4 *q = reinterpret_cast<const arr_f4*>(src), a = arr_ld<ARR_PAD_NT_LOAD>(q), b = arr_ld<ARR_PAD_NT_LOAD>(q + 1);
    const arr_u4 w = {CV::pack(a.x, a.y), CV::pack(a.z, a.w), CV::pack(b.x, b.y), CV::pack(b.z, b.w)};
    return w;
  }
  static __device__ __forceinline__ void store(arr_u4* dst, arr_u4 w, const Lane& L) { arrd_widen_st<CV>(reinterpret_cast<float*>(dst), w, L); }
  static __device__ __forceinline__ void zero(arr_u4* dst, const Lane& L) {
    const arr_f2 z = {0.f, 0.f};
    arrd_st_f4(reinterpret_cast<float*>(dst) + L.offA, z, z);
    arrd_st_f4(reinterpret_cast<float*>(dst) + L.offB, z, z);
  }
};

// The count of type i kept by this player, clamped so that every access stays in bounds whatever the counts hold: to the slots left, to
// rows[i] in the fixed mode, and to zero from below.
template <bool FIXED>
__device__ __forceinline__ int arr_cols_count(const int32_t* __restrict__ counts, const ArrFixedRows& rw, int i, int TP, int tp, int left) {
  int c = counts[(size_t)i * TP + tp];
  if (FIXED) c = c > rw.rows[i] ? rw.rows[i] : c;
  c = c > left ? left : c;
  return c < 0 ? 0 : c;
}

// The two bodies.  The types loop is unrolled over DYNENV_ARR_MAX_TYPES in all twelve kernels (rolled over the types of the call, the
// narrowing backward loses 0.6-1 % on Driving Full and 2.6-3 % on the sparse Driving Partial; profiles/HISTORY.md has both forms' figures).
template <class Unit, bool FIXED>
__device__ __forceinline__ void arr_pad_cols_body(const void* e0, const void* e1, const void* e2, const void* e3,
                                                  const int32_t* __restrict__ counts, const int32_t* __restrict__ base, const ArrFixedRows& rw,
                                                  int nTypes, int T, int P, int maxCount, int units, arr_u4* __restrict__ padded) {
  const unsigned x = blockIdx.x * ARR_BLOCK + threadIdx.x;
  if (x >= (unsigned)P * (unsigned)units) return;
  const int p = (int)(x / (unsigned)units), f = (int)(x % (unsigned)units);
  const int t = (int)blockIdx.y, TP = T * P, tp = t * P + p;
  const size_t stride = (size_t)P * units;               // units between consecutive slots of one column
  const size_t row = (size_t)units * Unit::PIECES;       // pieces of an embedding row
  arr_u4* out = padded + (size_t)t * maxCount * stride + x;
  const arr_u4 zero = {0u, 0u, 0u, 0u};
  int j = 0;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= nTypes || j >= maxCount) break;
    const int c = arr_cols_count<FIXED>(counts, rw, i, TP, tp, maxCount - j);
    const void* e = i == 0 ? e0 : i == 1 ? e1 : i == 2 ? e2 : e3;
    if (e) {
      const size_t row0 = FIXED ? (size_t)tp * rw.rows[i] : (size_t)base[(size_t)i * TP + tp];
      const arr_u4* src = static_cast<const arr_u4*>(e) + row0 * row + Unit::PIECES * f;
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        const arr_u4 v0 = Unit::load(src + (size_t)(k + 0) * row), v1 = Unit::load(src + (size_t)(k + 1) * row),
                     v2 = Unit::load(src + (size_t)(k + 2) * row), v3 = Unit::load(src + (size_t)(k + 3) * row);
        arr_st<true>(out, v0); arr_st<true>(out + stride, v1); arr_st<true>(out + 2 * stride, v2); arr_st<true>(out + 3 * stride, v3);
        out += 4 * stride;
      }
      for (; k < c; ++k) { arr_st<true>(out, Unit::load(src + (size_t)k * row)); out += stride; }
    } else {
      for (int k = 0; k < c; ++k) { arr_st<true>(out, zero); out += stride; }
    }
    j += c;
  }
  for (; j < maxCount; ++j) { arr_st<true>(out, zero); out += stride; }
}

template <class Unit, bool FIXED>
__device__ __forceinline__ void arr_unpad_cols_body(const arr_u4* __restrict__ grad, const int32_t* __restrict__ counts, const int32_t* __restrict__ base,
                                                    const ArrFixedRows& rw, int nTypes, int T, int P, int maxCount, int units, int G,
                                                    void* __restrict__ g0, void* __restrict__ g1, void* __restrict__ g2, void* __restrict__ g3) {
  const unsigned x = blockIdx.x * ARR_BLOCK + threadIdx.x;
  if (x >= (unsigned)P * (unsigned)units) return;
  const int p = (int)(x / (unsigned)units), f = (int)(x % (unsigned)units);
  const int t = (int)blockIdx.y, TP = T * P, tp = t * P + p;
  const size_t stride = (size_t)P * units;               // units between consecutive slots of one column
  const size_t row = (size_t)units * Unit::PIECES;       // pieces of an embedding row
  const arr_u4* in = grad + (size_t)t * maxCount * stride + x;
  const typename Unit::Lane L = Unit::lane(G);
  int j = 0;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= nTypes) break;
    if (!FIXED && j >= maxCount) break;   // (the fixed mode goes on: the later types' rows are still to be zeroed)
    const int n = FIXED ? rw.rows[i] : 0;
    const int c = arr_cols_count<FIXED>(counts, rw, i, TP, tp, maxCount - j);
    void* g = i == 0 ? g0 : i == 1 ? g1 : i == 2 ? g2 : g3;
    if (g && (FIXED || c > 0)) {
      const size_t row0 = FIXED ? (size_t)tp * n : (size_t)base[(size_t)i * TP + tp];
      arr_u4* dst = static_cast<arr_u4*>(g) + row0 * row + Unit::PIECES * f;
      const arr_u4* src = in;
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        const arr_u4 v0 = arr_ld<ARR_BWD_NT_LOAD>(src), v1 = arr_ld<ARR_BWD_NT_LOAD>(src + stride),
                     v2 = arr_ld<ARR_BWD_NT_LOAD>(src + 2 * stride), v3 = arr_ld<ARR_BWD_NT_LOAD>(src + 3 * stride);
        Unit::store(dst + (size_t)(k + 0) * row, v0, L); Unit::store(dst + (size_t)(k + 1) * row, v1, L);
        Unit::store(dst + (size_t)(k + 2) * row, v2, L); Unit::store(dst + (size_t)(k + 3) * row, v3, L);
        src += 4 * stride;
      }
      for (; k < c; ++k) { Unit::store(dst + (size_t)k * row, arr_ld<ARR_BWD_NT_LOAD>(src), L); src += stride; }
      if (FIXED)
        for (; k < n; ++k) Unit::zero(dst + (size_t)k * row, L);
    }
    in += (size_t)c * stride;
    j += c;
  }
}

// The twelve kernels.  One signature per direction: the default mode reads `base` and leaves `rw` alone, the fixed mode the other way
// round; `units` is the 16-byte units of a padded row (F/4 or F/8), G the exchange group of ArrNarrow's backward (ArrCopy ignores it).
#define ARR_COLS_KERNEL(DIR, MODE, SUFFIX, UNIT, FIXED)                                                                                    \
  extern "C" __global__ void __launch_bounds__(ARR_BLOCK)                                                                                  \
  MODE##_##DIR##_cols##SUFFIX##kernel(ARR_COLS_ARGS_##DIR) {                                                                               \
    arr_##DIR##_cols_body<UNIT, FIXED>(ARR_COLS_PASS_##DIR);                                                                               \
  }
#define ARR_COLS_ARGS_pad                                                                                                                  \
  const void* __restrict__ e0, const void* __restrict__ e1, const void* __restrict__ e2, const void* __restrict__ e3,                      \
  const int32_t* __restrict__ counts, const int32_t* __restrict__ base, ArrFixedRows rw, int nTypes, int T, int P, int maxCount, int units, \
  arr_u4* __restrict__ padded
#define ARR_COLS_PASS_pad e0, e1, e2, e3, counts, base, rw, nTypes, T, P, maxCount, units, padded
#define ARR_COLS_ARGS_unpad                                                                                                                \
  const arr_u4* __restrict__ grad, const int32_t* __restrict__ counts, const int32_t* __restrict__ base, ArrFixedRows rw, int nTypes,      \
  int T, int P, int maxCount, int units, int G, void* __restrict__ g0, void* __restrict__ g1, void* __restrict__ g2, void* __restrict__ g3
#define ARR_COLS_PASS_unpad grad, counts, base, rw, nTypes, T, P, maxCount, units, G, g0, g1, g2, g3
#define ARR_COLS_KERNELS(SUFFIX, UNIT)                                                                                                     \
  ARR_COLS_KERNEL(pad, arr, SUFFIX, UNIT, false) ARR_COLS_KERNEL(unpad, arr, SUFFIX, UNIT, false)                                          \
  ARR_COLS_KERNEL(pad, arrf, SUFFIX, UNIT, true) ARR_COLS_KERNEL(unpad, arrf, SUFFIX, UNIT, true)
ARR_COLS_KERNELS(_, ArrCopy)
ARR_COLS_KERNELS(_bf16_, ArrNarrow<ArrBf16>)
ARR_COLS_KERNELS(_f16_, ArrNarrow<ArrF16>)
