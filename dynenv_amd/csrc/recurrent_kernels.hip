// recurrent_kernels.hip — the back half of the reference's DynEnvFeatureExtractor.forward (DynEnv/models/models.py:584-594, 610-616;
// LSTMLayer: models.py:16-95) in one launch where no gradient is wanted: TransformNet (Linear, LeakyReLU, LayerNorm) over
// cat(feat, ext), the LSTM cell on the persistent h and c with a per-environment reset folded in, and the closing LayerNorm `bn`
// (include/dynenv.h, dynenv_recurrent_head).  The [P][4F] gate pre-activations never exist in memory.  Included at the very END of
// dynenv_capi.hip, behind attention_kernels.hip: no kernel a step launches moves.  This file also holds the entry point's host code.
//
// Per row p (environment p / A):
//   x = feat (X == 0)   or   LayerNorm(leaky(cat(feat, ext) W_tr^T + b_tr))
//   h, c = +0.0 WITHOUT being read where reset_env[p / A] != 0, else read
//   g = x W_ih^T + b_ih + h W_hh^T + b_hh;  c' = sigmoid(g_f) c + sigmoid(g_i) tanh(g_g);  h' = sigmoid(g_o) tanh(c');  out = LayerNorm(h')
//
// Work.  One workgroup of four waves per RH_ROWS = 64 rows = four strips of 16.  The products are the tile toolkit's (mma_tiles.h;
// DESIGN.md, "The tile toolkit"): the weight rows, fetched from global memory (L2), are the A operand, and a lane's accumulator holds
// four consecutive features of one row.  WEIGHT SHARING: a wave owns a quarter of the feature tiles (F / 64 tiles of 16 features) and
// ALL FOUR strips of the workgroup: every weight fragment it fetches feeds four MFMAs, one per strip, whose B operands (the 64 rows' x and h, 16 bit wide) it holds in
// registers.  A workgroup therefore streams the weights once per 64 rows, and no weight element is fetched by two waves of it.  For one
// feature tile the wave holds the four gates i, f, g, o of those features of all 64 rows (16 accumulators), so the cell is evaluated in
// place; c of those features was loaded before anything was written.
//   phase 0: feat (and ext, +0 up to KP), and h unless reset, rounded into LDS row-major; this wave's part of c into registers
//   phase 1 (X > 0): the transform; LayerNorm; x rounded into LDS
//   phase 2: the gates, the cell, h' and c' stored; LayerNorm; out stored
// A LayerNorm needs sums over a row whose features lie in four waves: each wave leaves its part of every row's sum in LDS and every
// wave adds the four parts in wave order - one fixed order, so a row's result depends on the row, its mask byte and the weights alone,
// not on p, on P or on its neighbours (an MFMA's columns do not mix).  Rows at or behind P in the last workgroup are +0.0 in LDS and
// are never stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "mma_tiles.h"

#define RH_BLOCK 256
#define RH_WAVES (RH_BLOCK / 64)
#define RH_STRIPS 4
#define RH_ROWS (16 * RH_STRIPS)

struct RhW {   // dynenv_rhead_t by value
  const atp_h *tr_w, *w_ih, *w_hh;
  const float *tr_b, *tr_ln_w, *tr_ln_b, *b_ih, *b_hh, *ln_w, *ln_b;
};

// torch's LayerNorm (biased variance, two passes) of the rows whose features y[tile][strip] are spread over the four waves; part: [2][RH_WAVES][RH_ROWS]
template <int F, int TPW>
__device__ __forceinline__ void rh_layer_norm(atp_f4 (&y)[TPW][RH_STRIPS], float* part, const float* lnw, const float* lnb, float eps, int wave,
                                              int ft0, int lr, int lq) {
  float mean[RH_STRIPS], rstd[RH_STRIPS];
#pragma unroll
  for (int s = 0; s < RH_STRIPS; ++s) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t) v += atp_sum4(y[t][s]);
    v = atp_row_sum(v);
    if (lq == 0) part[wave * RH_ROWS + 16 * s + lr] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < RH_STRIPS; ++s) {
    const float* q = part + 16 * s + lr;
    mean[s] = mt_wave_sum4(q, RH_ROWS) * (1.0f / F);
  }
  float* part2 = part + RH_WAVES * RH_ROWS;
#pragma unroll
  for (int s = 0; s < RH_STRIPS; ++s) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t) { const atp_f4 d = y[t][s] - mean[s]; v += atp_sum4(d * d); }
    v = atp_row_sum(v);
    if (lq == 0) part2[wave * RH_ROWS + 16 * s + lr] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < RH_STRIPS; ++s) {
    const float* q = part2 + 16 * s + lr;
    rstd[s] = 1.0f / sqrtf(mt_wave_sum4(q, RH_ROWS) * (1.0f / F) + eps);
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const atp_f4 g = mt_ldf4(lnw + 16 * (ft0 + t) + 4 * lq), b = mt_ldf4(lnb + 16 * (ft0 + t) + 4 * lq);
#pragma unroll
    for (int s = 0; s < RH_STRIPS; ++s) y[t][s] = (y[t][s] - mean[s]) * rstd[s] * g + b;
  }
}

template <int F, class CV, bool TR>
__device__ __forceinline__ void rh_body(const float* __restrict__ feat, const float* __restrict__ ext, int A, int X, int P, const RhW& w, float slope,
                                        float tr_eps, float ln_eps, const uint8_t* __restrict__ reset_env, float* h_io, float* c_io,
                                        float* __restrict__ out) {
  constexpr int FT = F / 16, KS = F / 32, TPW = FT / RH_WAVES;   // feature tiles, k steps of F, tiles per wave
  constexpr int XS = F + 8;                                      // elements per LDS row of x and h: 16 bytes of padding (attention_kernels.hip)
  constexpr int KP = F + 32, CS = KP + 8;                        // the transform's padded input width (X in 1..32) and its LDS row
  static_assert(TPW >= 1 && TPW * RH_WAVES == FT, "a whole number of feature tiles per wave");
  __shared__ __attribute__((aligned(16))) atp_h xb[RH_ROWS * XS];
  __shared__ __attribute__((aligned(16))) atp_h hb[RH_ROWS * XS];
  __shared__ __attribute__((aligned(16))) atp_h cb[TR ? RH_ROWS * CS : 8];
  __shared__ float part[2 * RH_WAVES * RH_ROWS];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int row0 = (int)blockIdx.x * RH_ROWS, ft0 = wave * TPW;
  const atp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- phase 0: the inputs, rounded, into LDS; nothing of a row is written before the first barrier below
  for (int i = tid; i < RH_ROWS * (F / 4); i += RH_BLOCK) {
    const int r = i / (F / 4), q = i % (F / 4), p = row0 + r;
    atp_f4 v = zero4, hv = zero4;
    if (p < P) {
      v = mt_ldf4(feat + (size_t)p * F + 4 * q);
      if (!(reset_env && reset_env[p / A])) hv = mt_ldf4(h_io + (size_t)p * F + 4 * q);
    }
    atp_st4<CV>((TR ? cb + r * CS : xb + r * XS) + 4 * q, v);
    atp_st4<CV>(hb + r * XS + 4 * q, hv);
  }
  if constexpr (TR) {
    for (int i = tid; i < RH_ROWS * 32; i += RH_BLOCK) {   // the columns F .. KP - 1: ext, then +0
      const int r = i >> 5, j = i & 31, p = row0 + r;
      const float v = (p < P && j < X) ? ext[(size_t)p * X + j] : 0.f;
      cb[r * CS + F + j] = (atp_h)(CV::pack(v, 0.f) & 0xffffu);
    }
  }
  atp_f4 cell[TPW][RH_STRIPS];   // c of this wave's features, then c'
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int s = 0; s < RH_STRIPS; ++s) {
      const int p = row0 + 16 * s + lr;
      cell[t][s] = zero4;
      if (p < P && !(reset_env && reset_env[p / A])) cell[t][s] = mt_ldf4(c_io + (size_t)p * F + 16 * (ft0 + t) + 4 * lq);
    }
  __syncthreads();

  // ---- phase 1: x = LayerNorm(leaky(cat W_tr^T + b_tr)), rounded into xb
  if constexpr (TR) {
    constexpr int KT = KP / 32;
    arr_u4 cf[RH_STRIPS][KT];
#pragma unroll
    for (int s = 0; s < RH_STRIPS; ++s)
#pragma unroll
      for (int ks = 0; ks < KT; ++ks) cf[s][ks] = atp_ld16(cb + (16 * s + lr) * CS + 32 * ks + 8 * lq);
    atp_f4 y[TPW][RH_STRIPS];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const atp_f4 b = mt_ldf4(w.tr_b + 16 * (ft0 + t) + 4 * lq);
#pragma unroll
      for (int s = 0; s < RH_STRIPS; ++s) y[t][s] = b;
#pragma unroll
      for (int ks = 0; ks < KT; ++ks) {
        const arr_u4 a = atp_ld16(w.tr_w + (size_t)(16 * (ft0 + t) + lr) * KP + 32 * ks + 8 * lq);
#pragma unroll
        for (int s = 0; s < RH_STRIPS; ++s) y[t][s] = AtpMma<CV>::mma(a, cf[s][ks], y[t][s]);
      }
#pragma unroll
      for (int s = 0; s < RH_STRIPS; ++s) y[t][s] = mt_leaky4(y[t][s], slope);
    }
    rh_layer_norm<F, TPW>(y, part, w.tr_ln_w, w.tr_ln_b, tr_eps, wave, ft0, lr, lq);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int s = 0; s < RH_STRIPS; ++s) atp_st4<CV>(xb + (16 * s + lr) * XS + 16 * (ft0 + t) + 4 * lq, y[t][s]);
    __syncthreads();
  }

  // ---- phase 2: the gates of this wave's features for all 64 rows, the cell, LayerNorm
  arr_u4 xf[RH_STRIPS][KS], hf[RH_STRIPS][KS];
#pragma unroll
  for (int s = 0; s < RH_STRIPS; ++s)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      xf[s][ks] = atp_ld16(xb + (16 * s + lr) * XS + 32 * ks + 8 * lq);
      hf[s][ks] = atp_ld16(hb + (16 * s + lr) * XS + 32 * ks + 8 * lq);
    }
  atp_f4 hn[TPW][RH_STRIPS];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int f = 16 * (ft0 + t);
    atp_f4 g[4][RH_STRIPS];   // torch's gate order: i, f, g, o
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const atp_f4 b = mt_ldf4(w.b_ih + k * F + f + 4 * lq) + mt_ldf4(w.b_hh + k * F + f + 4 * lq);
#pragma unroll
      for (int s = 0; s < RH_STRIPS; ++s) g[k][s] = b;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const arr_u4 a = atp_ld16(w.w_ih + (size_t)(k * F + f + lr) * F + 32 * ks + 8 * lq);
#pragma unroll
        for (int s = 0; s < RH_STRIPS; ++s) g[k][s] = AtpMma<CV>::mma(a, xf[s][ks], g[k][s]);
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const arr_u4 a = atp_ld16(w.w_hh + (size_t)(k * F + f + lr) * F + 32 * ks + 8 * lq);
#pragma unroll
        for (int s = 0; s < RH_STRIPS; ++s) g[k][s] = AtpMma<CV>::mma(a, hf[s][ks], g[k][s]);
      }
    }
#pragma unroll
    for (int s = 0; s < RH_STRIPS; ++s) {
      atp_f4 c = cell[t][s], h;
      c.x = mt_sigmoid(g[1][s].x) * c.x + mt_sigmoid(g[0][s].x) * tanhf(g[2][s].x);
      c.y = mt_sigmoid(g[1][s].y) * c.y + mt_sigmoid(g[0][s].y) * tanhf(g[2][s].y);
      c.z = mt_sigmoid(g[1][s].z) * c.z + mt_sigmoid(g[0][s].z) * tanhf(g[2][s].z);
      c.w = mt_sigmoid(g[1][s].w) * c.w + mt_sigmoid(g[0][s].w) * tanhf(g[2][s].w);
      h.x = mt_sigmoid(g[3][s].x) * tanhf(c.x); h.y = mt_sigmoid(g[3][s].y) * tanhf(c.y);
      h.z = mt_sigmoid(g[3][s].z) * tanhf(c.z); h.w = mt_sigmoid(g[3][s].w) * tanhf(c.w);
      hn[t][s] = h;
      const int p = row0 + 16 * s + lr;
      if (p < P) {
        *reinterpret_cast<atp_f4*>(c_io + (size_t)p * F + f + 4 * lq) = c;
        *reinterpret_cast<atp_f4*>(h_io + (size_t)p * F + f + 4 * lq) = h;
      }
    }
  }
  rh_layer_norm<F, TPW>(hn, part, w.ln_w, w.ln_b, ln_eps, wave, ft0, lr, lq);
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int s = 0; s < RH_STRIPS; ++s) {
      const int p = row0 + 16 * s + lr;
      if (p < P) *reinterpret_cast<atp_f4*>(out + (size_t)p * F + 16 * (ft0 + t) + 4 * lq) = hn[t][s];
    }
}

#define RH_KERNEL(NAME, F, CV, TR)                                                                                                       \
  extern "C" __global__ void __launch_bounds__(RH_BLOCK)                                                                                 \
  NAME(const float* __restrict__ feat, const float* __restrict__ ext, int A, int X, int P, RhW w, float slope, float tr_eps, float ln_eps, \
       const uint8_t* __restrict__ reset_env, float* h_io, float* c_io, float* __restrict__ out) {                                       \
    rh_body<F, CV, TR>(feat, ext, A, X, P, w, slope, tr_eps, ln_eps, reset_env, h_io, c_io, out);                                          \
  }
RH_KERNEL(rh_64_bf16_kernel, 64, ArrBf16, false)
RH_KERNEL(rh_64_bf16_tr_kernel, 64, ArrBf16, true)
RH_KERNEL(rh_64_f16_kernel, 64, ArrF16, false)
RH_KERNEL(rh_64_f16_tr_kernel, 64, ArrF16, true)
RH_KERNEL(rh_128_bf16_kernel, 128, ArrBf16, false)
RH_KERNEL(rh_128_bf16_tr_kernel, 128, ArrBf16, true)
RH_KERNEL(rh_128_f16_kernel, 128, ArrF16, false)
RH_KERNEL(rh_128_f16_tr_kernel, 128, ArrF16, true)

// ---- the entry point.  Argument errors first, then what the kernel does not take, both before a device is looked for; one launch and
// nothing else: nothing is synchronised, allocated or copied, so the call may be captured.
extern "C" int dynenv_recurrent_head(const float* feat_dev, const float* ext_dev, int32_t E, int32_t A, int32_t F, int32_t X, int32_t w_dtype,
                                     const dynenv_rhead_t* w, float slope, float tr_eps, float ln_eps, const uint8_t* reset_env_dev,
                                     float* h_dev, float* c_dev, float* out_dev, void* stream) {
  if (!feat_dev || !w || !h_dev || !c_dev || !out_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (!w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh || !w->ln_w || !w->ln_b)
    return fail(DYNENV_ERR_ARG, "recurrent head: the cell and the closing LayerNorm have all six of their pointers");
  if (E < 1 || A < 1 || F < 1 || X < 0) return fail(DYNENV_ERR_ARG, "recurrent head: bad shape");
  if ((X > 0) != (ext_dev != nullptr)) return fail(DYNENV_ERR_ARG, "recurrent head: ext_dev is NULL exactly when X == 0");
  if (X > 0 && (!w->tr_w || !w->tr_b || !w->tr_ln_w || !w->tr_ln_b))
    return fail(DYNENV_ERR_ARG, "recurrent head: X > 0 takes the four pointers of the transform");
  if (int rc = model_operand_dtype("recurrent head", w_dtype)) return rc;
  if (int rc = model_aligned("recurrent head", {feat_dev, h_dev, c_dev, out_dev, w->w_ih, w->w_hh, w->b_ih, w->b_hh, w->ln_w, w->ln_b}, 16)) return rc;
  if (X > 0)
    if (int rc = model_aligned("recurrent head", {w->tr_w, w->tr_b, w->tr_ln_w, w->tr_ln_b}, 16)) return rc;
  if ((int64_t)E * A > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "recurrent head: E * A too large for one launch");
  if (int rc = model_operand_16bit("recurrent head", w_dtype, "layer")) return rc;
  if (F != 64 && F != 128) return fail(DYNENV_ERR_UNSUPPORTED, "recurrent head: the fused layer takes F = 64 or 128");
  if (X > 32) return fail(DYNENV_ERR_UNSUPPORTED, "recurrent head: the fused layer takes X <= 32");
  if (int rc = have_device()) return rc;
  RhW k;
  k.tr_w = static_cast<const atp_h*>(w->tr_w); k.w_ih = static_cast<const atp_h*>(w->w_ih); k.w_hh = static_cast<const atp_h*>(w->w_hh);
  k.tr_b = w->tr_b; k.tr_ln_w = w->tr_ln_w; k.tr_ln_b = w->tr_ln_b; k.b_ih = w->b_ih; k.b_hh = w->b_hh; k.ln_w = w->ln_w; k.ln_b = w->ln_b;
  static decltype(&rh_64_bf16_kernel) const kernels[2][2][2] = {{{rh_64_bf16_kernel, rh_64_bf16_tr_kernel}, {rh_64_f16_kernel, rh_64_f16_tr_kernel}},
                                                                {{rh_128_bf16_kernel, rh_128_bf16_tr_kernel}, {rh_128_f16_kernel, rh_128_f16_tr_kernel}}};
  const int P = E * A;
  hipLaunchKernelGGL(kernels[F == 128][w_dtype == DYNENV_ARR_F16][X > 0], dim3((unsigned)((P + RH_ROWS - 1) / RH_ROWS)), dim3(RH_BLOCK), 0,
                     (hipStream_t)stream, feat_dev, ext_dev, A, X, P, k, slope, tr_eps, ln_eps, reset_env_dev, h_dev, c_dev, out_dev);
  return launched();
}
