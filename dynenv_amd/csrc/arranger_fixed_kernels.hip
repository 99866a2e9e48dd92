// arranger_fixed_kernels.hip — the arranger at FIXED capacities (include/dynenv.h, dynenv_arrange_fixed_*): the same ragged -> padded
// layout as arranger_kernels.hip (the reference's InOutArranger, DynEnv/models/models.py:219-274), but every shape is the caller's:
// rows[i] rows of type i per (t, p) in inputs[i] and in the embeddings, maxCount = M slots in the padded tensor.  The start of a
// player's rows is arithmetic (tp * rows[i]), so there is no prefix scan, no totals and nothing the host has to wait for: launches
// only, capturable.  Included at the very END of dynenv_capi.hip (next to env_rows_kernels.hip): no kernel a step launches moves
// (rc_layout_pad, robocup_kernels.hip).
//   c_i(t,p) = clamp(count, 0, cap_i)                                  (arr_count: the default mode's count)
//   k_i(t,p) = min(c_i, rows[i], M - sum_{i'<i} k_i')                  kept; earlier types win; c_i - k_i is dropped AND reported
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"

// ArrFixed { ArrTypes ty; int rows[4]; int maxCount; } and ArrFixedRows { int rows[4]; } are declared at the top of dynenv_capi.hip, in
// front of the host code that fills them; ArrTypes, arr_count, ARR_ST and arr_bwd_ld / arr_bwd_st are arranger_kernels.hip's.

// the kept counts of one player's types 0 .. upTo-1 (upTo <= ty.n); returns their sum.  drop[i] = c_i - k_i where drop != nullptr.
__device__ __forceinline__ int arrf_kept(const ArrFixed& fx, int upTo, const float* __restrict__ row, const int32_t* __restrict__ count_env, int e,
                                         int* kept, int* drop) {
  int sum = 0;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= upTo) { kept[i] = 0; if (drop) drop[i] = 0; continue; }
    const int c = arr_count(fx.ty, i, row, count_env, e);
    int k = c < fx.rows[i] ? c : fx.rows[i];
    const int room = fx.maxCount - sum;
    k = k < room ? k : room;
    kept[i] = k;
    if (drop) drop[i] = c - k;
    sum += k;
  }
  return sum;
}

// KF1: one thread per (t, p, j), j < jSpan = max(M, 1): the mask byte of slot j; the thread j == 0 also writes the player's kept counts
// and objCounts and adds what was dropped to `dropped` (int32 [n]; the sum does not depend on the order of the adds).
extern "C" __global__ void __launch_bounds__(ARR_BLOCK)
arrf_plan_kernel(const float* __restrict__ obs, int E, int T, int A, int D, ArrFixed fx, const int32_t* __restrict__ count_env, int jSpan,
                 int32_t* __restrict__ counts, int32_t* __restrict__ obj_counts, uint8_t* __restrict__ mask, int32_t* __restrict__ dropped) {
  const int P = E * A, TP = T * P;
  const long long gid = (long long)blockIdx.x * ARR_BLOCK + threadIdx.x;
  const int tp = (int)(gid / jSpan), j = (int)(gid % jSpan);
  if (tp >= TP) return;
  const int t = tp / P, p = tp % P, e = p / A, a = p % A;
  const float* row = obs + (((size_t)e * T + t) * A + a) * D;
  int kept[DYNENV_ARR_MAX_TYPES], drop[DYNENV_ARR_MAX_TYPES];
  const int sum = arrf_kept(fx, fx.ty.n, row, count_env, e, kept, drop);
  if (mask && j < fx.maxCount) mask[(size_t)tp * fx.maxCount + j] = (uint8_t)(j >= sum);
  if (j != 0) return;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= fx.ty.n) break;
    counts[(size_t)i * TP + tp] = kept[i];
    if (dropped && drop[i] > 0) atomicAdd(dropped + i, drop[i]);
  }
  obj_counts[tp] = sum;
}

// KF2: one thread per float of inputs[i] (blockIdx.y = i): the destination [T][P][rows_i][feat_i] is written linearly; the source is
// the contiguous cap_i * feat_i block of the player's observation row for a kept row r < k_i, and +0.0 behind it - the unused capacity
// of an observation row is never read.  Each thread recomputes its player's kept counts up to its own type.
extern "C" __global__ void __launch_bounds__(ARR_BLOCK)
arrf_gather_kernel(const float* __restrict__ obs, int E, int T, int A, int D, ArrFixed fx, const int32_t* __restrict__ count_env,
                   float* in0, float* in1, float* in2, float* in3) {
  const int i = (int)blockIdx.y;
  float* in = i == 0 ? in0 : i == 1 ? in1 : i == 2 ? in2 : in3;
  if (!in) return;
  const dynenv_arr_type_t d = fx.ty.t[i];
  const long long perPlayer = (long long)fx.rows[i] * d.feat;   // floats of one (t, p)
  const int P = E * A, TP = T * P;
  const long long gid = (long long)blockIdx.x * ARR_BLOCK + threadIdx.x;
  if (perPlayer <= 0 || gid >= perPlayer * TP) return;
  const int tp = (int)(gid / perPlayer), w = (int)(gid % perPlayer), r = w / d.feat;
  const int t = tp / P, p = tp % P, e = p / A, a = p % A;
  const float* row = obs + (((size_t)e * T + t) * A + a) * D;
  int kept[DYNENV_ARR_MAX_TYPES];
  arrf_kept(fx, i + 1, row, count_env, e, kept, nullptr);
  const int k = i == 0 ? kept[0] : i == 1 ? kept[1] : i == 2 ? kept[2] : kept[3];
  in[gid] = r < k ? row[d.offset + w] : 0.0f;
}

// KF3: the padded tensor [T][M][P][F] in one pass, the thread-to-data map of arr_pad_cols_kernel (K5): one thread per float4 column
// (t, p, f) walks down its player's M slots; the rows of type i start at tp * rows[i] of emb_i.  Plain loads, non-temporal stores (what
// K5 settled on).  The counts are clamped to 0 .. rows[i] and to the slots left, so reads and writes stay in bounds whatever they hold.
// The loads, decided as K5 / K5' were: by an A/B of libraries built with the other value of the define, tools/fixed_arranger_time.py at
// 4096 environments, F = 128, medians of 5 x 40 calls of gather + pad + backward, in us for Driving Full / Driving Partial at M = 96 and
// at M = 35 / RoboCup Full; the product library before and after the variants: 722-729 / 808-820, 615-618 / 827-837.
//   non-temporal loads of the embeddings in KF3: 711 / 844, 645 / 818: 2 % gained on the two dense cases, 3-4 % lost on the sparse one,
//     the signs K5 found: not used.
//   plain loads of the gradient in KF3': 749 / 848, 641 / 860: 3-4 % slower everywhere, in a run whose default-mode legs were 0.5-10 %
//     slower too; no case in which the plain load wins: non-temporal, as in K5'.
#ifndef ARRF_PAD_NT_LOAD
#define ARRF_PAD_NT_LOAD 0
#endif
#ifndef ARRF_BWD_NT_LOAD
#define ARRF_BWD_NT_LOAD 1
#endif
__device__ __forceinline__ float4 arrf_ld(const float4* p, bool nt) {
  if (!nt) return *p;
  const arr_f4 w = __builtin_nontemporal_load(reinterpret_cast<const arr_f4*>(p));
  return make_float4(w.x, w.y, w.z, w.w);
}
#define ARRF_PAD_LD(p) arrf_ld((p), ARRF_PAD_NT_LOAD)
#define ARRF_BWD_LD(p) arrf_ld((p), ARRF_BWD_NT_LOAD)
extern "C" __global__ void __launch_bounds__(ARR_BLOCK)
arrf_pad_cols_kernel(const float* __restrict__ e0, const float* __restrict__ e1, const float* __restrict__ e2, const float* __restrict__ e3,
                     const int32_t* __restrict__ counts, ArrFixedRows rw, int nTypes, int T, int P, int maxCount, int F4,
                     float4* __restrict__ padded) {
  const unsigned x = blockIdx.x * ARR_BLOCK + threadIdx.x;
  if (x >= (unsigned)P * (unsigned)F4) return;
  const int f = (int)(x % (unsigned)F4), p = (int)(x / (unsigned)F4);
  const int t = (int)blockIdx.y, TP = T * P, tp = t * P + p;
  const size_t stride = (size_t)P * F4;  // float4s between consecutive slots of one column
  float4* out = padded + (size_t)t * maxCount * stride + x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  int j = 0;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= nTypes || j >= maxCount) break;
    int c = counts[(size_t)i * TP + tp];
    c = c > rw.rows[i] ? rw.rows[i] : c;
    c = c > maxCount - j ? maxCount - j : c;
    c = c < 0 ? 0 : c;
    const float* e = i == 0 ? e0 : i == 1 ? e1 : i == 2 ? e2 : e3;
    if (e) {
      const float4* src = reinterpret_cast<const float4*>(e) + (size_t)tp * rw.rows[i] * F4 + f;
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        const float4 v0 = ARRF_PAD_LD(src + (size_t)(k + 0) * F4), v1 = ARRF_PAD_LD(src + (size_t)(k + 1) * F4),
                     v2 = ARRF_PAD_LD(src + (size_t)(k + 2) * F4), v3 = ARRF_PAD_LD(src + (size_t)(k + 3) * F4);
        ARR_ST(out, v0); ARR_ST(out + stride, v1); ARR_ST(out + 2 * stride, v2); ARR_ST(out + 3 * stride, v3);
        out += 4 * stride;
      }
      for (; k < c; ++k) { ARR_ST(out, ARRF_PAD_LD(src + (size_t)k * F4)); out += stride; }
    } else {
      for (int k = 0; k < c; ++k) { ARR_ST(out, zero); out += stride; }
    }
    j += c;
  }
  for (; j < maxCount; ++j) { ARR_ST(out, zero); out += stride; }
}

// KF3': the backward of KF3, the map of arr_unpad_cols_kernel (K5'): g_i[tp * rows[i] + r][f] = grad[t][j][p][f] for r < k_i, and +0.0
// for the rows k_i .. rows[i]-1 (the block ran on those zero rows and its output was discarded).  Every row of every non-NULL g_i is
// written exactly once; a NULL g_i is stepped over unread; padding slots of the gradient are never read.  Non-temporal loads and
// stores (what K5' settled on), four independent 16-byte accesses in flight in both loops.
extern "C" __global__ void __launch_bounds__(ARR_BLOCK)
arrf_unpad_cols_kernel(const float4* __restrict__ grad, const int32_t* __restrict__ counts, ArrFixedRows rw, int nTypes, int T, int P,
                       int maxCount, int F4, float* __restrict__ g0, float* __restrict__ g1, float* __restrict__ g2, float* __restrict__ g3) {
  const unsigned x = blockIdx.x * ARR_BLOCK + threadIdx.x;
  if (x >= (unsigned)P * (unsigned)F4) return;
  const int f = (int)(x % (unsigned)F4), p = (int)(x / (unsigned)F4);
  const int t = (int)blockIdx.y, TP = T * P, tp = t * P + p;
  const size_t stride = (size_t)P * F4;  // float4s between consecutive slots of one column
  const float4* in = grad + (size_t)t * maxCount * stride + x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  int j = 0;
#pragma unroll
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (i >= nTypes) break;   // (no early exit at j == maxCount: the later types' rows are still to be zeroed)
    const int n = rw.rows[i];
    int c = counts[(size_t)i * TP + tp];
    c = c > n ? n : c;
    c = c > maxCount - j ? maxCount - j : c;
    c = c < 0 ? 0 : c;
    float* g = i == 0 ? g0 : i == 1 ? g1 : i == 2 ? g2 : g3;
    if (g) {
      float4* dst = reinterpret_cast<float4*>(g) + (size_t)tp * n * F4 + f;
      const float4* src = in;
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        const float4 v0 = ARRF_BWD_LD(src), v1 = ARRF_BWD_LD(src + stride), v2 = ARRF_BWD_LD(src + 2 * stride), v3 = ARRF_BWD_LD(src + 3 * stride);
        arr_bwd_st(dst + (size_t)(k + 0) * F4, v0); arr_bwd_st(dst + (size_t)(k + 1) * F4, v1);
        arr_bwd_st(dst + (size_t)(k + 2) * F4, v2); arr_bwd_st(dst + (size_t)(k + 3) * F4, v3);
        src += 4 * stride;
      }
      for (; k < c; ++k) { arr_bwd_st(dst + (size_t)k * F4, ARRF_BWD_LD(src)); src += stride; }
      for (; k + 4 <= n; k += 4) {
        arr_bwd_st(dst + (size_t)(k + 0) * F4, zero); arr_bwd_st(dst + (size_t)(k + 1) * F4, zero);
        arr_bwd_st(dst + (size_t)(k + 2) * F4, zero); arr_bwd_st(dst + (size_t)(k + 3) * F4, zero);
      }
      for (; k < n; ++k) arr_bwd_st(dst + (size_t)k * F4, zero);
    }
    in += (size_t)c * stride;
    j += c;
  }
}
