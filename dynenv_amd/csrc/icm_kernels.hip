// icm_kernels.hip — the reference's curiosity module where no gradient is wanted: ICMDynamics.forward (DynEnv/models/icm.py:207-240) -
// the forward net on cat(f_t, one_hot(a_t)) and the inverse net (an ActorLayer) on cat(f_t, f_{t+1}) - and the per-row terms of
// ICMNet._calc_loss (icm.py:77-109) in ONE launch over a stored rollout, then the masked means in a second, small one (include/dynenv.h,
// dynenv_icm_losses).  Neither the one-hot (icm.py:167-179: a Python loop with one host read per action), the two cats, the hidden
// layer, the prediction nor the logits exist in memory.  Included at the very END of dynenv_capi.hip, behind rollout_kernels.hip: no
// kernel a step launches moves.  This file also holds the entry point's host code.
//
// Per row (t, p):
//   hid  = leaky(f_t W1[:, :K]^T + b1 + sum_g W1_act[start_g + a_g]; slope)     (the one-hot's product is a gather, added in group order)
//   pred = hid W2^T + b2;   curiosity[t][p] = (sum_k (pred_k - f_{t+1,k})^2) / K
//   l    = cat(f_t, f_{t+1}) W_inv^T + b_inv;   inverse_ce[t][g][p] = logsumexp(l_g) - l_g[a_g]
//
// Work.  One workgroup of four waves owns ICM_ROWS = 64 players - four strips of 16, policy_kernels.hip's shape - and walks t = 0 .. T-1:
// the tile features[t + 1][64 players] is read from memory once, rounded into LDS, and serves as `next` of step t and as `cur` of step
// t + 1 (two LDS tiles that swap roles).  The products are the tile toolkit's (mma_tiles.h; DESIGN.md, "The tile toolkit"): a lane's
// accumulator holds four consecutive outputs of one row; a wave computes its output tiles for ALL FOUR strips, so every weight fragment
// it fetches (16 contiguous bytes per lane, from L2) feeds four MFMAs and the workgroup streams the weights once per 64 players and step.
//   phase 0: features[t + 1] of the 64 players rounded into LDS (t = 0: features[0] too); the rows' action indices into LDS
//   phase 1: the ICM_HID / 16 = 10 tiles of the hidden layer and the two of the logits, dealt round robin (tile = wave + 4 j; the
//            logits' tiles 10 and 11 are the third of waves 2 and 3 and run over cat(cur, next)); the gather, the LeakyReLU; the hidden
//            layer rounded into LDS, the logits into LDS as float32
//   phase 2: the K / 16 tiles of the prediction from the hidden layer in LDS; the error against f_{t+1} in FLOAT32 - re-read from
//            memory in the accumulator's layout (the tile was fetched a moment ago: L2), not from the rounded LDS copy; thread (row r,
//            wave q) takes the groups g = q, q + 4 of row r: max-subtracted logsumexp
//   phase 3: the four waves' parts of a row's squared error added in wave order
// Every sum has one fixed order and an MFMA's columns do not mix: a row's result depends on features[t][p], features[t + 1][p],
// actions[t][:, p] and the weights alone.  Rows at or behind P in the last workgroup are +0.0 in LDS and are never stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "mma_tiles.h"

#define ICM_BLOCK 256
#define ICM_WAVES (ICM_BLOCK / 64)
#define ICM_STRIPS 4
#define ICM_ROWS (16 * ICM_STRIPS)
#define ICM_HID DYNENV_ICM_HIDDEN_PAD   // 160: the forward net's 140 hidden units padded to the k step of the second product
#define ICM_LS 33                       // floats per LDS row of the 32 logits: a lane per row reads without bank conflicts
#define ICM_RED_BLOCK 1024

struct IcmArgs {   // dynenv_icm_t by value, the buffers and the sizes
  const float *features, *actions;
  const atp_h *w1, *w2, *winv;
  const float *w1_act, *b1, *b2, *binv;
  unsigned long long group_off;   // 8 bits per group: the first logit of group g
  unsigned group_n;               // 4 bits per group: n_g - 1
  int T, P, G, AD;
  float slope;
  float *curiosity, *ce;
  int* status;
};

template <int K, class CV>
__device__ __forceinline__ void icm_load_tile(atp_h* xb, const float* src, int row0, int P, int tid) {
  constexpr int XS = K + 8;
  const atp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < ICM_ROWS * (K / 4); i += ICM_BLOCK) {
    const int r = i / (K / 4), col = 4 * (i % (K / 4)), p = row0 + r;
    atp_st4<CV>(xb + r * XS + col, p < P ? mt_ldf4(src + (size_t)p * K + col) : zero4);
  }
}

template <int K, class CV>
__device__ __forceinline__ void icm_body(const IcmArgs& a) {
  constexpr int XS = K + 8, HS = ICM_HID + 8;                     // elements per LDS row: 16 bytes of padding
  constexpr int KS = K / 32, HT = ICM_HID / 16, HKS = ICM_HID / 32;   // k steps over a feature, hidden tiles, k steps over the hidden layer
  constexpr int TPW = (HT + 2) / ICM_WAVES;                       // 3: tiles per wave in phase 1
  constexpr int OT = K / 16, OPW = OT / ICM_WAVES;                // tiles of the prediction, per wave
  static_assert((HT + 2) % ICM_WAVES == 0 && OT % ICM_WAVES == 0 && HT == 10, "the deal of the tiles");
  __shared__ __attribute__((aligned(16))) atp_h xb[2][ICM_ROWS * XS];
  __shared__ __attribute__((aligned(16))) atp_h hb[ICM_ROWS * HS];
  __shared__ float lg[ICM_ROWS * ICM_LS];
  __shared__ float part[ICM_WAVES * ICM_ROWS];
  __shared__ int acts[ICM_ROWS * 8];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int row0 = (int)blockIdx.x * ICM_ROWS, P = a.P, G = a.G;
  const atp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bool inv_wave = wave >= 2;   // tiles 10 and 11, the logits, are the third tile of waves 2 and 3

  icm_load_tile<K, CV>(xb[0], a.features, row0, P, tid);
  for (int t = 0; t < a.T; ++t) {
    const atp_h *cur = xb[t & 1], *nxt = xb[(t + 1) & 1];
    const float* next32 = a.features + (size_t)(t + 1) * P * K;
    // ---- phase 0: the next tile; acts[r][g] = start_g + a_g, the row of W1_act and the logit of the action taken
    icm_load_tile<K, CV>(xb[(t + 1) & 1], next32, row0, P, tid);
    bool clamped = false;
    for (int i = tid; i < ICM_ROWS * G; i += ICM_BLOCK) {
      const int g = i / ICM_ROWS, r = i % ICM_ROWS, p = row0 + r;
      const MtGroup gr = mt_group(a.group_off, a.group_n, g);
      const int off = gr.off, n = gr.n;
      acts[r * 8 + g] = off + (p < P ? mt_stored_action(a.actions[((size_t)t * a.AD + g) * P + p], n - 1, clamped) : 0);
    }
    if (clamped && a.status) atomicOr(a.status, 1);
    __syncthreads();

    // ---- phase 1: this wave's three tiles for all 64 rows
    {
      atp_f4 y[TPW][ICM_STRIPS];
      const atp_h* wrow[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const int tile = wave + ICM_WAVES * j;
        atp_f4 b;
        if (tile < HT) {
          b = mt_ldf4(a.b1 + 16 * tile + 4 * lq);
          wrow[j] = a.w1 + (size_t)(16 * tile + lr) * K;
        } else {
          b = mt_ldf4(a.binv + 16 * (tile - HT) + 4 * lq);
          wrow[j] = a.winv + (size_t)(16 * (tile - HT) + lr) * (2 * K);
        }
#pragma unroll
        for (int s = 0; s < ICM_STRIPS; ++s) y[j][s] = b;
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        arr_u4 xf[ICM_STRIPS];
#pragma unroll
        for (int s = 0; s < ICM_STRIPS; ++s) xf[s] = atp_ld16(cur + (16 * s + lr) * XS + 32 * ks + 8 * lq);
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          const arr_u4 w = atp_ld16(wrow[j] + 32 * ks + 8 * lq);
#pragma unroll
          for (int s = 0; s < ICM_STRIPS; ++s) y[j][s] = AtpMma<CV>::mma(w, xf[s], y[j][s]);
        }
      }
      if (inv_wave) {   // the second half of cat(cur, next)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const arr_u4 w = atp_ld16(wrow[TPW - 1] + K + 32 * ks + 8 * lq);
#pragma unroll
          for (int s = 0; s < ICM_STRIPS; ++s)
            y[TPW - 1][s] = AtpMma<CV>::mma(w, atp_ld16(nxt + (16 * s + lr) * XS + 32 * ks + 8 * lq), y[TPW - 1][s]);
        }
      }
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const int tile = wave + ICM_WAVES * j;
        if (tile < HT) {
#pragma unroll
          for (int s = 0; s < ICM_STRIPS; ++s) {
            const int r = 16 * s + lr;
            atp_f4 v = y[j][s];
            for (int g = 0; g < G; ++g) v += mt_ldf4(a.w1_act + (size_t)acts[r * 8 + g] * ICM_HID + 16 * tile + 4 * lq);
            atp_st4<CV>(hb + r * HS + 16 * tile + 4 * lq, mt_leaky4(v, a.slope));
          }
        } else {
#pragma unroll
          for (int s = 0; s < ICM_STRIPS; ++s) mt_st_f4(lg + (16 * s + lr) * ICM_LS + 16 * (tile - HT) + 4 * lq, y[j][s]);
        }
      }
    }
    __syncthreads();

    // ---- phase 2: the prediction and its squared error against the float32 f_{t+1}
    {
      atp_f4 z[OPW][ICM_STRIPS];
      const atp_h* wrow[OPW];
#pragma unroll
      for (int j = 0; j < OPW; ++j) {
        const int tile = wave + ICM_WAVES * j;
        const atp_f4 b = mt_ldf4(a.b2 + 16 * tile + 4 * lq);
        wrow[j] = a.w2 + (size_t)(16 * tile + lr) * ICM_HID;
#pragma unroll
        for (int s = 0; s < ICM_STRIPS; ++s) z[j][s] = b;
      }
#pragma unroll
      for (int ks = 0; ks < HKS; ++ks) {
        arr_u4 hf[ICM_STRIPS];
#pragma unroll
        for (int s = 0; s < ICM_STRIPS; ++s) hf[s] = atp_ld16(hb + (16 * s + lr) * HS + 32 * ks + 8 * lq);
#pragma unroll
        for (int j = 0; j < OPW; ++j) {
          const arr_u4 w = atp_ld16(wrow[j] + 32 * ks + 8 * lq);
#pragma unroll
          for (int s = 0; s < ICM_STRIPS; ++s) z[j][s] = AtpMma<CV>::mma(w, hf[s], z[j][s]);
        }
      }
#pragma unroll
      for (int s = 0; s < ICM_STRIPS; ++s) {
        const int p = row0 + 16 * s + lr;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < OPW; ++j) {
          const atp_f4 d = z[j][s] - (p < P ? mt_ldf4(next32 + (size_t)p * K + 16 * (wave + ICM_WAVES * j) + 4 * lq) : zero4);
          v += atp_sum4(d * d);
        }
        v = atp_row_sum(v);
        if (lq == 0) part[wave * ICM_ROWS + 16 * s + lr] = v;
      }
    }
    // row r's groups g = q, q + 4, by thread (r, q); q is the wave, so a group's size is uniform
    {
      const int r = lane, p = row0 + r;
      const float* L = lg + r * ICM_LS;
      for (int g = wave; g < G; g += ICM_WAVES) {
        const MtGroup gr = mt_group(a.group_off, a.group_n, g);
        const int off = gr.off, n = gr.n;
        float m = L[off];
        for (int j = 1; j < n; ++j) m = fmaxf(m, L[off + j]);
        float sum = 0.f;
        for (int j = 0; j < n; ++j) sum += expf(L[off + j] - m);
        if (p < P) a.ce[((size_t)t * G + g) * P + p] = (m + logf(sum)) - L[acts[r * 8 + g]];
      }
    }
    __syncthreads();

    // ---- phase 3
    if (tid < ICM_ROWS && row0 + tid < P) {
      a.curiosity[(size_t)t * P + row0 + tid] = mt_wave_sum4(part + tid, ICM_ROWS) * (1.0f / K);
    }
    // (no barrier here: what the next step writes first - the tile `cur`, acts - was last read before the barrier above; part, hb and lg
    // are written behind the next step's first barrier)
  }
}

#define ICM_KERNEL(NAME, K, CV) \
  extern "C" __global__ void __launch_bounds__(ICM_BLOCK) NAME(IcmArgs a) { icm_body<K, CV>(a); }
ICM_KERNEL(icm_64_bf16_kernel, 64, ArrBf16)
ICM_KERNEL(icm_64_f16_kernel, 64, ArrF16)
ICM_KERNEL(icm_128_bf16_kernel, 128, ArrBf16)
ICM_KERNEL(icm_128_f16_kernel, 128, ArrF16)
ICM_KERNEL(icm_256_bf16_kernel, 256, ArrBf16)
ICM_KERNEL(icm_256_f16_kernel, 256, ArrF16)

// The masked means: one workgroup, double accumulators.  Thread i takes, for t = 0 .. T-1, the players 4 i .. 4 i + 3, then those 4096
// further on, and so on (a P that is no multiple of 4: the players i, i + 1024, ...); per player the groups' cross-entropies are added
// in group order, a finished player counts as +0; then the 1024 partial sums are added pairwise in a fixed tree; one rounding to float32
// at the end.  G is a template argument so that all 2 + G loads of an iteration are issued before the first is used.
template <int G>
__device__ __forceinline__ void icm_reduce_body(const float* __restrict__ curiosity, const float* __restrict__ ce, const unsigned char* __restrict__ finished,
                                                int T, int P, float* __restrict__ losses) {
  __shared__ double sc[ICM_RED_BLOCK], si[ICM_RED_BLOCK];
  __shared__ int sn[ICM_RED_BLOCK];
  const int tid = (int)threadIdx.x;
  double c = 0.0, s = 0.0;
  int n = 0;
  if ((P & 3) == 0) {   // (the buffers are 16-byte aligned: so is every row of them)
    const int P4 = P >> 2;
    for (int t = 0; t < T; ++t) {
      const atp_f4* c4 = reinterpret_cast<const atp_f4*>(curiosity + (size_t)t * P);
      const unsigned* m4 = finished ? reinterpret_cast<const unsigned*>(finished + (size_t)t * P) : nullptr;
#pragma unroll 2
      for (int i = tid; i < P4; i += ICM_RED_BLOCK) {
        const atp_f4 cv = c4[i];
        const unsigned m = m4 ? m4[i] : 0u;
        atp_f4 e[G];
#pragma unroll
        for (int g = 0; g < G; ++g) e[g] = reinterpret_cast<const atp_f4*>(ce + ((size_t)t * G + g) * P)[i];
        double is[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < G; ++g) { is[0] += (double)e[g].x; is[1] += (double)e[g].y; is[2] += (double)e[g].z; is[3] += (double)e[g].w; }
        const bool on[4] = {(m & 0xffu) == 0, (m & 0xff00u) == 0, (m & 0xff0000u) == 0, (m & 0xff000000u) == 0};
        const float cf[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          n += on[k] ? 1 : 0;
          c += on[k] ? (double)cf[k] : 0.0;
          s += on[k] ? is[k] : 0.0;
        }
      }
    }
  } else {
    for (int t = 0; t < T; ++t) {
      const size_t row = (size_t)t * P;
#pragma unroll 4
      for (int p = tid; p < P; p += ICM_RED_BLOCK) {
        const bool on = !finished || finished[row + p] == 0;
        const float cv = curiosity[row + p];
        double is = 0.0;
#pragma unroll
        for (int g = 0; g < G; ++g) is += (double)ce[((size_t)t * G + g) * P + p];
        n += on ? 1 : 0;
        c += on ? (double)cv : 0.0;
        s += on ? is : 0.0;
      }
    }
  }
  sc[tid] = c; si[tid] = s; sn[tid] = n;
  __syncthreads();
  for (int h = ICM_RED_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) { sc[tid] += sc[tid + h]; si[tid] += si[tid + h]; sn[tid] += sn[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    const int cnt = sn[0];
    losses[0] = cnt ? (float)(sc[0] / (double)cnt) : 0.0f;
    losses[1] = cnt ? (float)(si[0] / ((double)cnt * (double)G)) : 0.0f;
    losses[2] = (float)cnt;
  }
}

#define ICM_REDUCE(G)                                                                                                                         \
  extern "C" __global__ void __launch_bounds__(ICM_RED_BLOCK) icm_reduce_##G##_kernel(const float* curiosity, const float* ce, const unsigned char* finished, \
                                                                                      int T, int P, float* losses) {                        \
    icm_reduce_body<G>(curiosity, ce, finished, T, P, losses);                                                                                \
  }
ICM_REDUCE(1) ICM_REDUCE(2) ICM_REDUCE(3) ICM_REDUCE(4) ICM_REDUCE(5) ICM_REDUCE(6) ICM_REDUCE(7) ICM_REDUCE(8)

// ---- the entry point.  Argument errors first, then what the kernel does not take, both before a device is looked for; the two launches
// and nothing else: nothing is synchronised, allocated or copied, so the call may be captured.
extern "C" int dynenv_icm_losses(const float* features_dev, const float* actions_dev, const uint8_t* finished_dev, int32_t T, int32_t P, int32_t K,
                                 int32_t action_cols, const int32_t* nvec, int32_t G, int32_t w_dtype, const dynenv_icm_t* w, float slope,
                                 float* curiosity_dev, float* inverse_ce_dev, float* losses_dev, int32_t* status_dev, void* stream) {
  if (!features_dev || !actions_dev || !nvec || !w || !curiosity_dev || !inverse_ce_dev) return fail(DYNENV_ERR_ARG, "icm losses: null argument");
  if (!w->fwd_w1 || !w->fwd_w1_act || !w->fwd_b1 || !w->fwd_w2 || !w->fwd_b2 || !w->inv_w || !w->inv_b)
    return fail(DYNENV_ERR_ARG, "icm losses: the forward and the inverse net have all seven of their pointers");
  if (T < 1 || P < 1 || K < 1) return fail(DYNENV_ERR_ARG, "icm losses: bad shape");
  if (G < 1 || G > DYNENV_POLICY_MAX_GROUPS) return fail(DYNENV_ERR_ARG, "icm losses: G is 1..8");
  ModelGroups gr;
  if (int rc = model_groups("icm losses", nvec, G, action_cols, gr)) return rc;
  if (int rc = model_operand_dtype("icm losses", w_dtype)) return rc;
  if (int rc = model_aligned("icm losses", {features_dev, actions_dev, finished_dev, curiosity_dev, inverse_ce_dev, w->fwd_w1, w->fwd_w1_act, w->fwd_b1,
                                            w->fwd_w2, w->fwd_b2, w->inv_w, w->inv_b}, 16))
    return rc;
  if ((uintptr_t)losses_dev % 4 || (uintptr_t)status_dev % 4) return fail(DYNENV_ERR_ARG, "icm losses: losses_dev and status_dev are 4-byte aligned");
  if (((int64_t)T + 1) * P > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "icm losses: (T + 1) * P too large for one launch");
  if (int rc = model_operand_16bit("icm losses", w_dtype, "layer")) return rc;
  if (K != 64 && K != 128 && K != 256) return fail(DYNENV_ERR_UNSUPPORTED, "icm losses: the fused layer takes K = 64, 128 or 256");
  if (int rc = have_device()) return rc;
  IcmArgs k;
  k.features = features_dev; k.actions = actions_dev;
  k.w1 = static_cast<const atp_h*>(w->fwd_w1); k.w2 = static_cast<const atp_h*>(w->fwd_w2); k.winv = static_cast<const atp_h*>(w->inv_w);
  k.w1_act = w->fwd_w1_act; k.b1 = w->fwd_b1; k.b2 = w->fwd_b2; k.binv = w->inv_b;
  k.group_off = gr.off; k.group_n = gr.n;
  k.T = T; k.P = P; k.G = G; k.AD = action_cols; k.slope = slope;
  k.curiosity = curiosity_dev; k.ce = inverse_ce_dev; k.status = status_dev;
  static decltype(&icm_64_bf16_kernel) const kernels[3][2] = {{icm_64_bf16_kernel, icm_64_f16_kernel}, {icm_128_bf16_kernel, icm_128_f16_kernel},
                                                               {icm_256_bf16_kernel, icm_256_f16_kernel}};
  hipLaunchKernelGGL(kernels[K == 64 ? 0 : K == 128 ? 1 : 2][w_dtype == DYNENV_ARR_F16], dim3((unsigned)((P + ICM_ROWS - 1) / ICM_ROWS)), dim3(ICM_BLOCK), 0,
                     (hipStream_t)stream, k);
  static decltype(&icm_reduce_1_kernel) const reduce[8] = {icm_reduce_1_kernel, icm_reduce_2_kernel, icm_reduce_3_kernel, icm_reduce_4_kernel,
                                                           icm_reduce_5_kernel, icm_reduce_6_kernel, icm_reduce_7_kernel, icm_reduce_8_kernel};
  if (losses_dev)
    hipLaunchKernelGGL(reduce[G - 1], dim3(1), dim3(ICM_RED_BLOCK), 0, (hipStream_t)stream, (const float*)curiosity_dev, (const float*)inverse_ce_dev,
                       (const unsigned char*)finished_dev, (int)T, (int)P, losses_dev);
  return launched();
}
