// arranger_embed_kernels.hip — the reference's whole InputLayer (DynEnv/models/models.py:278-307) in one pass where no gradient is wanted:
// rearrange_inputs -> one EmbedBlock per object type (models.py:99-124) -> rearrange_outputs, from the observation row straight to the
// slot of the padded tensor (include/dynenv.h, dynenv_arrange_embed_pad).  Neither inputs[i], nor an activation, nor the embeddings
// exist in memory: the kernel reads obs and counts and writes every element of padded[T][maxCount][P][F] exactly once.  Included at the
// very END of dynenv_capi.hip, behind arranger_fixed_kernels.hip: no kernel a step launches moves (rc_layout_pad, robocup_kernels.hip).
// This file also holds the entry point's host code (everything it calls is defined above it in the unit).
//
//   EmbedBlock:  h = LayerNorm_{F/2}(LeakyReLU(W1 x)),  y = LayerNorm_F(LeakyReLU(W2 h)),  W1 [F/2][feat], W2 [F][F/2], no bias
//   slot j = sum_{i'<i} k_i'(t,p) + r, r < k_i(t,p), holds y of obs[e][t][a][offset_i + r*feat_i ..];  +0.0 behind the last object
//   k_i = clamp(counts[i][t][p], 0, min(cap_i, slots left))   (arr_cols_count's clamps, and the capacity: the row is read here)
//
// Work.  blockIdx.y is the object type, blockIdx.x a run of ARE_PLAYERS consecutive (t, p): one type per workgroup keeps the LDS image
// of the weights at w2 + w1 + the LayerNorm vectors (37.5 KB at F = 128).  The workgroup scans the kept counts of its run (one thread per
// player), which COMPACTS the live rows: object m of the run belongs to the player found by bisection of the scan, so a sparse batch
// (Driving Partial fills 19 % of the slots) forms full tiles.  A wave takes tiles of 64 objects, ONE OBJECT PER LANE - the product is
// computed transposed, features down the registers, objects across the lanes - so both LayerNorms are in-lane sums and every sum has
// one fixed order: an object's result depends on its features and its type, not on its lane, its slot or the batch.
//   layer 1   h[c] = fma chain over q < feat of w1t[q][c] * x[q]                 weights: broadcast ds_read_b128 (4 per instruction)
//   layer 2   y[f] = fma chain over k = 0 .. F/2-1 of w2t[k][f] * h[k]           8 k per trip of a rolled loop; h is shifted down by 8
//                                                                                registers per trip, so every register index is static
//   LayerNorm mean = sum / n, var = sum (x - mean)^2 / n (biased, two passes), (x - mean) * (1 / sqrt(var + eps)) * w + b
// float32 throughout (the unit is built with -ffp-contract=off: every fma is written).  The store goes through LDS: the lanes of a wave
// stage ARE_STAGE rows at a time and the wave writes them back with 16 bytes per lane, so that each store instruction covers whole
// contiguous padded rows (two rows of 512 bytes at F = 128 float32); the 16-bit conversion (round to nearest even: ArrBf16 / ArrF16 of
// mma_tiles.h) is applied to the float32 result before it is staged.  The workgroups of type 0 also write the +0.0 behind
// each player's last object, rows of consecutive players side by side.  A type whose weights are NULL writes +0.0 into its slots.
#include <hip/hip_runtime.h>
#include "dynenv.h"
#include "mma_tiles.h"

#define ARE_PLAYERS ARR_BLOCK   // (t, p) per workgroup: one thread each in the scan
#define ARE_STAGE 8             // rows a wave stages per round of the store
#define ARE_MAX_FEAT 16
#ifndef ARE_MIN_WAVES
// Waves per SIMD the kernels are compiled for.  2: at most 256 registers, which F = 128 exceeds by 43-65 spilled to scratch (15 accesses
// per trip of layer 2's loop); 1: 256 VGPRs + 35-42 AGPRs, no scratch - and 20-24 % slower on dense batches at 4096 environments
// (profiles/HISTORY.md has the A/B).  F = 64 fits either way (172-182 VGPRs).
#define ARE_MIN_WAVES 2
#endif

// ARR_BLOCK, ArrTypes, arr_f4 and arr_block_scan are arranger_kernels.hip's; arr_st is arranger_cols_kernels.hip's.
struct AreBlocks {   // dynenv_embed_block_t per type, by value
  const float* w1[DYNENV_ARR_MAX_TYPES];
  const float* ln1w[DYNENV_ARR_MAX_TYPES];
  const float* ln1b[DYNENV_ARR_MAX_TYPES];
  const float* w2[DYNENV_ARR_MAX_TYPES];
  const float* ln2w[DYNENV_ARR_MAX_TYPES];
  const float* ln2b[DYNENV_ARR_MAX_TYPES];
};

// LayerNorm of v[0 .. N-1] in place, then nothing else: w and b are LDS vectors read at static offsets (broadcast)
template <int N>
__device__ __forceinline__ void are_layer_norm(float (&v)[N], const float* w, const float* b, float eps) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < N; ++c) s += v[c];
  const float mean = s * (1.0f / N);
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < N; ++c) { const float d = v[c] - mean; q = fmaf(d, d, q); }
  const float rstd = 1.0f / sqrtf(q * (1.0f / N) + eps);
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = fmaf((v[c] - mean) * rstd, w[c], b[c]);
}

template <int F, class CV /* void: float32 */>
__device__ __forceinline__ void are_embed_pad_body(const float* __restrict__ obs, int E, int T, int A, int D, const ArrTypes& ty,
                                                   const int32_t* __restrict__ counts, int maxCount, const AreBlocks& bl, float slope,
                                                   float eps, arr_u4* __restrict__ padded) {
  constexpr bool WIDE = __is_same(CV, void);
  constexpr int H = F / 2;
  constexpr int RP = WIDE ? F / 4 : F / 8;   // 16-byte pieces of a padded row
  constexpr int SROW = RP + 1;               // ... of a staged row: one piece of padding, so that the 8 writers of a round hit 8 bank groups
  constexpr int RPI = 64 / RP;               // rows one store instruction of a wave covers
  __shared__ arr_f4 w2t[H * F / 4];                 // [k][f]
  __shared__ arr_f4 w1t[ARE_MAX_FEAT * H / 4];      // [q][c]
  __shared__ float lnv[2 * H + 2 * F];              // ln1_w, ln1_b, ln2_w, ln2_b
  __shared__ arr_u4 stage[ARR_BLOCK / 64][ARE_STAGE * SROW];
  __shared__ int start[ARE_PLAYERS], before[ARE_PLAYERS], total[ARE_PLAYERS];
  __shared__ int waveTot[ARR_BLOCK / 64];

  const int i = (int)blockIdx.y, P = E * A, TP = T * P;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tp0 = (int)blockIdx.x * ARE_PLAYERS;
  const dynenv_arr_type_t d = ty.t[i];
  const bool hasW = bl.w1[i] != nullptr;

  // the kept counts of this thread's player: k of the workgroup's type, the slots in front of it, and the player's objects in all
  int k = 0;
  {
    const int tp = tp0 + tid;
    int bef = 0, left = maxCount;
    if (tp < TP) {
#pragma unroll
      for (int ii = 0; ii < DYNENV_ARR_MAX_TYPES; ++ii) {
        if (ii >= ty.n) break;
        int c = counts[(size_t)ii * TP + tp];
        c = c > ty.t[ii].cap ? ty.t[ii].cap : c;
        c = c > left ? left : c;
        c = c < 0 ? 0 : c;
        if (ii == i) { k = c; bef = maxCount - left; }
        left -= c;
      }
    }
    before[tid] = bef;
    total[tid] = tp < TP ? maxCount - left : maxCount;   // (a player past the end has no padding to write)
  }
  int nLive;
  const int incl = arr_block_scan(k, waveTot, nLive);
  start[tid] = incl - k;

  if (nLive > 0 && hasW) {   // the type's weights, transposed so that one ds_read_b128 holds four outputs of one input
    float* w2s = reinterpret_cast<float*>(w2t);
    float* w1s = reinterpret_cast<float*>(w1t);
    const float* __restrict__ w2 = bl.w2[i];
    const float* __restrict__ w1 = bl.w1[i];
    for (int g = tid; g < F * H; g += ARR_BLOCK) w2s[(g % H) * F + g / H] = w2[g];
    for (int g = tid; g < H * d.feat; g += ARR_BLOCK) w1s[(g % d.feat) * H + g / d.feat] = w1[g];
    for (int g = tid; g < H; g += ARR_BLOCK) { lnv[g] = bl.ln1w[i][g]; lnv[H + g] = bl.ln1b[i][g]; }
    for (int g = tid; g < F; g += ARR_BLOCK) { lnv[2 * H + g] = bl.ln2w[i][g]; lnv[2 * H + F + g] = bl.ln2b[i][g]; }
  }
  __syncthreads();

  // every wave runs the same number of trips (the barriers of the store are the workgroup's); a wave past the end only takes part in them
#pragma unroll 1
  for (int m0 = 0; m0 < nLive; m0 += ARR_BLOCK) {
    const int m = m0 + tid;
    const bool waveLive = m0 + wave * 64 < nLive;
    int dstRow = -1;   // this lane's row of the padded tensor viewed as [T*maxCount*P] rows; -1: none
    float y[F];
    if (waveLive) {
      float x[ARE_MAX_FEAT];
#pragma unroll
      for (int q = 0; q < ARE_MAX_FEAT; ++q) x[q] = 0.f;
      if (m < nLive) {
        int lo = 0, hi = ARE_PLAYERS;   // the last player whose scan is <= m (players without objects in front of it share its scan)
#pragma unroll
        for (int s = 0; s < 8; ++s) { const int mid = (lo + hi) >> 1; if (start[mid] <= m) lo = mid; else hi = mid; }
        const int r = m - start[lo], tp = tp0 + lo, t = tp / P, p = tp % P, e = p / A, a = p % A;
        dstRow = (t * maxCount + before[lo] + r) * P + p;
        if (hasW) {
          const float* src = obs + (((size_t)e * T + t) * A + a) * D + d.offset + r * d.feat;
#pragma unroll
          for (int q = 0; q < ARE_MAX_FEAT; ++q)
            if (q < d.feat) x[q] = src[q];
        }
      }
      if (hasW) {
        float h[H];
#pragma unroll
        for (int c = 0; c < H; ++c) h[c] = 0.f;
#pragma unroll
        for (int q = 0; q < ARE_MAX_FEAT; ++q) {
          if (q < d.feat) {   // (uniform)
#pragma unroll
            for (int c4 = 0; c4 < H / 4; ++c4) {
              const arr_f4 w = w1t[q * (H / 4) + c4];
              h[4 * c4 + 0] = fmaf(w.x, x[q], h[4 * c4 + 0]); h[4 * c4 + 1] = fmaf(w.y, x[q], h[4 * c4 + 1]);
              h[4 * c4 + 2] = fmaf(w.z, x[q], h[4 * c4 + 2]); h[4 * c4 + 3] = fmaf(w.w, x[q], h[4 * c4 + 3]);
            }
          }
        }
#pragma unroll
        for (int c = 0; c < H; ++c) h[c] = h[c] > 0.f ? h[c] : h[c] * slope;
        are_layer_norm<H>(h, lnv, lnv + H, eps);
#pragma unroll
        for (int f = 0; f < F; ++f) y[f] = 0.f;
#pragma unroll 1
        for (int g = 0; g < H / 8; ++g) {
          const arr_f4* wrow = w2t + g * 8 * (F / 4);
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) {
#pragma unroll
            for (int f4 = 0; f4 < F / 4; ++f4) {
              const arr_f4 w = wrow[kk * (F / 4) + f4];
              y[4 * f4 + 0] = fmaf(w.x, h[kk], y[4 * f4 + 0]); y[4 * f4 + 1] = fmaf(w.y, h[kk], y[4 * f4 + 1]);
              y[4 * f4 + 2] = fmaf(w.z, h[kk], y[4 * f4 + 2]); y[4 * f4 + 3] = fmaf(w.w, h[kk], y[4 * f4 + 3]);
            }
          }
#pragma unroll
          for (int c = 0; c + 8 < H; ++c) h[c] = h[c + 8];
        }
#pragma unroll
        for (int f = 0; f < F; ++f) y[f] = y[f] > 0.f ? y[f] : y[f] * slope;
        are_layer_norm<F>(y, lnv + 2 * H, lnv + 2 * H + F, eps);
      } else {
#pragma unroll
        for (int f = 0; f < F; ++f) y[f] = 0.f;
      }
    } else {
#pragma unroll
      for (int f = 0; f < F; ++f) y[f] = 0.f;
    }

    // the store: ARE_STAGE lanes at a time put their rows into the wave's stage, then the wave writes them, 16 bytes per lane
    arr_u4* st = stage[wave];
#pragma unroll 1
    for (int rr = 0; rr < 64 / ARE_STAGE; ++rr) {
      if ((lane >> 3) == rr) {
        arr_u4* mine = st + (lane & 7) * SROW;
#pragma unroll
        for (int pc = 0; pc < RP; ++pc) {
          arr_u4 v;
          if constexpr (WIDE) {
            v.x = __float_as_uint(y[4 * pc]); v.y = __float_as_uint(y[4 * pc + 1]); v.z = __float_as_uint(y[4 * pc + 2]); v.w = __float_as_uint(y[4 * pc + 3]);
          } else {
            v.x = CV::pack(y[8 * pc], y[8 * pc + 1]); v.y = CV::pack(y[8 * pc + 2], y[8 * pc + 3]);
            v.z = CV::pack(y[8 * pc + 4], y[8 * pc + 5]); v.w = CV::pack(y[8 * pc + 6], y[8 * pc + 7]);
          }
          mine[pc] = v;
        }
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < ARE_STAGE / RPI; ++it) {
        const int row = it * RPI + lane / RP, pc = lane % RP;
        const int dst = __shfl(dstRow, rr * ARE_STAGE + row, 64);
        if (dst >= 0) arr_st<true>(padded + (size_t)dst * RP + pc, st[row * SROW + pc]);
      }
      __syncthreads();
    }
  }

  // the padding: +0.0 in every slot behind a player's last object, written by the workgroups of type 0; consecutive players are
  // consecutive rows of padded[t][j], so the rows a store instruction covers lie side by side wherever neighbours are padding too
  if (i != 0) return;
  const arr_u4 zero = {0u, 0u, 0u, 0u};
  const int sub = tid / RP, pc = tid % RP;   // ARR_BLOCK / RP rows per trip
#pragma unroll 1
  for (int q = sub; q < maxCount * ARE_PLAYERS; q += ARR_BLOCK / RP) {
    const int j = q / ARE_PLAYERS, pl = q % ARE_PLAYERS;
    if (j < total[pl]) continue;
    const int tp = tp0 + pl, t = tp / P, p = tp % P;
    arr_st<true>(padded + ((size_t)(t * maxCount + j) * P + p) * RP + pc, zero);
  }
}

#define ARE_KERNEL(NAME, F, CV)                                                                                                          \
  extern "C" __global__ void __launch_bounds__(ARR_BLOCK, ARE_MIN_WAVES)                                                                \
  NAME(const float* __restrict__ obs, int E, int T, int A, int D, ArrTypes ty, const int32_t* __restrict__ counts, int maxCount,         \
       AreBlocks bl, float slope, float eps, arr_u4* __restrict__ padded) {                                                             \
    are_embed_pad_body<F, CV>(obs, E, T, A, D, ty, counts, maxCount, bl, slope, eps, padded);                                            \
  }
ARE_KERNEL(are_embed_pad_64_kernel, 64, void)
ARE_KERNEL(are_embed_pad_64_bf16_kernel, 64, ArrBf16)
ARE_KERNEL(are_embed_pad_64_f16_kernel, 64, ArrF16)
ARE_KERNEL(are_embed_pad_128_kernel, 128, void)
ARE_KERNEL(are_embed_pad_128_bf16_kernel, 128, ArrBf16)
ARE_KERNEL(are_embed_pad_128_f16_kernel, 128, ArrF16)

// ---- the entry point.  Argument errors first, then what the kernels do not take, both before a device is looked for; launches only:
// nothing is synchronised, allocated or copied, so the call may be captured (pointers and sizes are frozen, contents read at replay).
extern "C" int dynenv_arrange_embed_pad(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types,
                                        int32_t n_types, const int32_t* counts_dev, int32_t max_count, const dynenv_embed_block_t* blocks,
                                        int32_t F, float slope, float eps, void* padded_dev, int32_t padded_dtype, void* stream) {
  if (!obs_dev || !counts_dev || !blocks || !padded_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (E < 1 || T < 1 || A < 1 || D < 1 || (int64_t)E * T * A > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "arranger: bad shape");
  ArrTypes ty;
  if (int rc = arr_types(types, n_types, D, ty)) return rc;
  if (padded_dtype < DYNENV_ARR_F32 || padded_dtype > DYNENV_ARR_F16) return fail(DYNENV_ERR_ARG, "arranger: unknown dtype (DYNENV_ARR_F32, _BF16 or _F16)");
  if (max_count < 0) return fail(DYNENV_ERR_ARG, "arranger: max_count < 0");
  if ((uintptr_t)padded_dev % 16) return fail(DYNENV_ERR_ARG, "arranger: buffers must be 16-byte aligned");
  // a row of the padded tensor viewed as [T * max_count * P] rows is an int in the kernel, and so is max_count * ARE_PLAYERS
  if ((int64_t)T * max_count * ((int64_t)E * A) > 0x7fffffffLL || max_count >= 1 << 23) return fail(DYNENV_ERR_ARG, "arranger: padded tensor too large for one launch");
  AreBlocks bl;
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    const dynenv_embed_block_t b = i < n_types ? blocks[i] : dynenv_embed_block_t();
    const int have = (b.w1 != nullptr) + (b.ln1_w != nullptr) + (b.ln1_b != nullptr) + (b.w2 != nullptr) + (b.ln2_w != nullptr) + (b.ln2_b != nullptr);
    if (have != 0 && have != 6) return fail(DYNENV_ERR_ARG, "arranger: an embedding block has all six of its pointers or none");
    bl.w1[i] = b.w1; bl.ln1w[i] = b.ln1_w; bl.ln1b[i] = b.ln1_b; bl.w2[i] = b.w2; bl.ln2w[i] = b.ln2_w; bl.ln2b[i] = b.ln2_b;
  }
  if (F != 64 && F != 128) return fail(DYNENV_ERR_UNSUPPORTED, "arranger: the fused embedding takes F = 64 or 128");
  for (int i = 0; i < n_types; ++i)
    if (types[i].feat > ARE_MAX_FEAT) return fail(DYNENV_ERR_UNSUPPORTED, "arranger: the fused embedding takes object types of 1..16 features");
  if (int rc = have_device()) return rc;
  if (max_count == 0) return DYNENV_OK;
  static decltype(&are_embed_pad_64_kernel) const kernels[2][3] = {
      {are_embed_pad_64_kernel, are_embed_pad_64_bf16_kernel, are_embed_pad_64_f16_kernel},
      {are_embed_pad_128_kernel, are_embed_pad_128_bf16_kernel, are_embed_pad_128_f16_kernel}};
  const int64_t TP = (int64_t)E * T * A;
  const dim3 grid((unsigned)((TP + ARE_PLAYERS - 1) / ARE_PLAYERS), (unsigned)n_types);
  hipLaunchKernelGGL(kernels[F == 128][padded_dtype], grid, dim3(ARR_BLOCK), 0, (hipStream_t)stream, obs_dev, E, T, A, D, ty, counts_dev,
                     max_count, bl, slope, eps, static_cast<arr_u4*>(padded_dev));
  return launched();
}
