// arranger_fixed_kernels.hip — the arranger at FIXED capacities (include/dynenv.h, dynenv_arrange_fixed_*): the same ragged -> padded
// layout as arranger_kernels.hip (the reference's InOutArranger, DynEnv/models/models.py:219-274), but every shape is the caller's:
// rows[i] rows of type i per (t, p) in inputs[i] and in the embeddings, maxCount = M slots in the padded tensor.  The start of a
// player's rows is arithmetic (tp * rows[i]), so there is no prefix scan, no totals and nothing the host has to wait for: launches
// only, capturable.  This file: the plan and the gather (KF1, KF2); the padded tensor and its backward (KF3, KF3') are the fixed-mode
// kernels of arranger_cols_kernels.hip.  Included at the very END of dynenv_capi.hip (next to env_rows_kernels.hip): no kernel a step
// launches moves (rc_layout_pad, robocup_kernels.hip).
//   c_i(t,p) = clamp(count, 0, cap_i)                                  (arr_count: the default mode's count)
//   k_i(t,p) = min(c_i, rows[i], M - sum_{i'<i} k_i')                  kept; earlier types win; c_i - k_i is dropped AND reported
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"

// ArrFixed { ArrTypes ty; int rows[4]; int maxCount; } is declared at the top of dynenv_capi.hip, in front of the host code that fills
// it; ArrTypes and arr_count are arranger_kernels.hip's.

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
