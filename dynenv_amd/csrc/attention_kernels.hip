// attention_kernels.hip — the reference's RecurrentTemporalAttention (DynEnv/models/models.py:311-386) over the padded tensor in one
// launch where no gradient is wanted: from padded[T][M][P][F] (bf16 / fp16) and the object counts to the pooled feature out[P][F]
// (include/dynenv.h, dynenv_attend_pool).  Neither q, k, v, the probabilities nor an attention output exist in memory.  Included at the
// very END of dynenv_capi.hip, behind arranger_embed_kernels.hip: no kernel a step launches moves.  This file also holds the entry
// point's host code.
//
// Per player p (c_t its count at time t clamped to 0..M, n = max_t c_t, X_t its slots with +0.0 from c_t on, NEVER read there):
//   mha(w; Qin, KVin, k):  q = Qin Wq^T + bq;  K = KVin[:k] Wk^T + bk and the row bias_k;  V likewise with bias_v;
//                          softmax(q K^T / sqrt(F)) over the k + 1 keys;  (probs V) Wo^T + bo
//   att_t = mha(objAtt; X_t[:n], X_t, c_t);   fin = att_0, k = c_0;   t = 1..T-1: fin = LayerNorm(mha(tempAtt; att_t, fin, k)), k = max(k, c_t)
//   out[p] = sum_{r<n} sigmoid(fin_r conf_w + conf_b) fin_r / n      (+0.0 where n == 0)
//
// Work.  One workgroup of four waves per player; everything a player needs lies in LDS, 16 bit wide: the query input (X_t, overwritten
// strip by strip with att_t), fin, and the K and V^T of the attention at hand.  A product is __builtin_amdgcn_mfma_f32_16x16x32_{bf16,f16}
// with float32 accumulators, ALWAYS in the orientation D^T = W X^T: the weight rows (or key rows) are the A operand, 16 rows of the
// player the B operand, so that a lane's accumulator holds FOUR CONSECUTIVE FEATURES of ONE player row (column lane & 15, features
// 16 tile + 4 (lane >> 4) + reg).  Both operands are then 16 contiguous bytes per lane (k = 32 step + 8 (lane >> 4) + j for A and B
// alike, so the order of k inside a step cancels), a result is stored as one packed 8-byte piece of a row-major row - the layout the
// next product reads - and every sum over a row (softmax, LayerNorm, the confidence) is an in-lane sum over tiles and registers plus
// two exchanges (lanes ^ 16, ^ 32).  Only V^T = X Wv^T takes the other orientation (keys down the registers), for the same store.
//   phase 1 (the workgroup): K and V^T of the key rows, 16 keys and half of the features per unit, units dealt to the waves; the keys
//                            behind the last tile inside a k step (32) of probs V meet probabilities of zero and stay what they were: finite
//   phase 2 (a wave per strip of 16 query rows): q -> scores -> softmax -> probs V -> out projection (-> LayerNorm) in the wave's own
//                            LDS buffer, then the 16 rows of the result into the player's buffer; strips n / 16 .. are never computed
// The bias key is kept OUT of the tiles: its score is the dot product of the rounded q with bias_k and its share of the result
// prob * bias_v, both float32 from 16-bit values, so 16 keys are one tile and not two.  Weights are fetched as operands from global
// memory (every workgroup reads the same 128 KB per attention at F = 128: they live in L2).  The pooled mean of the last result is
// taken from the float32 accumulators; the waves' partial sums are added in wave order, so a player's result depends on its slots and
// counts alone - not on p, on M (the row capacity NT only sizes the buffers) or on the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "mma_tiles.h"

#define ATP_BLOCK 256
#define ATP_WAVES (ATP_BLOCK / 64)

struct AtpMha {   // dynenv_mha_t by value
  const atp_h *in_w, *out_w, *bias_k, *bias_v;
  const float *in_b, *out_b;
};

// the lanes of a wave hand rows to each other through the wave's LDS buffer: LDS operations of one wave complete in order, the fence
// keeps the compiler from moving an access across the hand-over
__device__ __forceinline__ void atp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// phase 1: kb[key][:] = src[key] Wk^T + bk and vt[:][key] = src[key] Wv^T + bv for the keys 0 .. 16 * ceil(c / 16) - 1; a unit is 16 keys, K or V,
// and one half of the features, so that few keys still occupy the four waves
template <int F, class CV, int XS, int VS>
__device__ __forceinline__ void atp_keys_values(const AtpMha& w, const atp_h* src, int c, atp_h* kb, atp_h* vt, int wave, int lr, int lq) {
  constexpr int HT = F / 32;   // feature tiles of a half
  const int units = 4 * ((c + 15) >> 4);
#pragma unroll 1
  for (int u = wave; u < units; u += ATP_WAVES) {
    const int kt = u >> 2, ft0 = (u & 1) * HT;
    arr_u4 xf[F / 32];
#pragma unroll
    for (int ks = 0; ks < F / 32; ++ks) xf[ks] = atp_ld16(src + (16 * kt + lr) * XS + 32 * ks + 8 * lq);
    if (!(u & 2)) {
      const atp_h* wk = w.in_w + (size_t)F * F;
#pragma unroll
      for (int ft = ft0; ft < ft0 + HT; ++ft) {
        atp_f4 acc = *reinterpret_cast<const atp_f4*>(w.in_b + F + 16 * ft + 4 * lq);
#pragma unroll
        for (int ks = 0; ks < F / 32; ++ks) acc = AtpMma<CV>::mma(atp_ld16(wk + (16 * ft + lr) * F + 32 * ks + 8 * lq), xf[ks], acc);
        atp_st4<CV>(kb + (16 * kt + lr) * XS + 16 * ft + 4 * lq, acc);
      }
    } else {
      const atp_h* wv = w.in_w + (size_t)2 * F * F;
#pragma unroll
      for (int ft = ft0; ft < ft0 + HT; ++ft) {
        const float b = w.in_b[2 * F + 16 * ft + lr];
        atp_f4 acc = {b, b, b, b};
#pragma unroll
        for (int ks = 0; ks < F / 32; ++ks) acc = AtpMma<CV>::mma(xf[ks], atp_ld16(wv + (16 * ft + lr) * F + 32 * ks + 8 * lq), acc);
        atp_st4<CV>(vt + (16 * ft + lr) * VS + 16 * kt + 4 * lq, acc);
      }
    }
  }
}

// phase 2: strip s of 16 query rows of qin, by one wave: dst[16 s ..][:] = mha(w; qin rows, the keys of phase 1, c) (LN: LayerNorm of it);
// LAST: the strip's share of sum_r conf_r fin_r is added to pooled[tile] (held by the lanes with lane & 15 == 0)
template <int F, class CV, int NT, int XS, int VS, int WS, bool LN>
__device__ __forceinline__ void atp_strip(const AtpMha& w, const atp_h* qin, int s, int c, const atp_h* kb, const atp_h* vt, atp_h* wb, atp_h* dst,
                                          const float* lnw, const float* lnb, float eps, bool last, int n, const float* confw, float confb,
                                          atp_f4 (&pooled)[F / 16], int lr, int lq) {
  constexpr int FT = F / 16, KS = F / 32;
  const float scale = F == 64 ? 0.125f : 0.08838834764831845f;   // 1 / sqrt(F)
  atp_h* mine = wb + lr * WS;   // the row of the wave's buffer this lane's player row lives in
  arr_u4 xf[KS];

  // q = Qin Wq^T + bq, rounded, into the buffer; the bias key's score from the rounded values
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = atp_ld16(qin + (16 * s + lr) * XS + 32 * ks + 8 * lq);
  float sb = 0.f;
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) {
    atp_f4 acc = *reinterpret_cast<const atp_f4*>(w.in_b + 16 * ft + 4 * lq);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = AtpMma<CV>::mma(atp_ld16(w.in_w + (16 * ft + lr) * F + 32 * ks + 8 * lq), xf[ks], acc);
    atp_st4<CV>(mine + 16 * ft + 4 * lq, acc);
    sb += atp_sum4(atp_round4<CV>(acc) * atp_ld4<CV>(w.bias_k + 16 * ft + 4 * lq));
  }
  sb = atp_row_sum(sb) * scale;
  atp_wave_sync();

  // scores^T = K q^T: keys down the registers (16 tile + 4 (lane >> 4) + reg), this lane's player row across them
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = atp_ld16(mine + 32 * ks + 8 * lq);
  const int kt16 = (c + 15) >> 4, kt32 = (c + 31) >> 5;
  atp_f4 sc[NT];
  float m = sb;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    const atp_f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    sc[kt] = ninf;
    if (kt < kt16) {
      atp_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = AtpMma<CV>::mma(atp_ld16(kb + (16 * kt + lr) * XS + 32 * ks + 8 * lq), xf[ks], acc);
      const int key = 16 * kt + 4 * lq;
      sc[kt].x = key + 0 < c ? acc.x * scale : -INFINITY;
      sc[kt].y = key + 1 < c ? acc.y * scale : -INFINITY;
      sc[kt].z = key + 2 < c ? acc.z * scale : -INFINITY;
      sc[kt].w = key + 3 < c ? acc.w * scale : -INFINITY;
      m = fmaxf(m, fmaxf(fmaxf(sc[kt].x, sc[kt].y), fmaxf(sc[kt].z, sc[kt].w)));
    }
  }
  m = atp_row_max(m);   // (finite: the bias key is never masked)
  float den = 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    if (kt < kt16) {
      sc[kt].x = expf(sc[kt].x - m); sc[kt].y = expf(sc[kt].y - m); sc[kt].z = expf(sc[kt].z - m); sc[kt].w = expf(sc[kt].w - m);
      den += atp_sum4(sc[kt]);
    }
  }
  const float eb = expf(sb - m);
  const float inv = 1.0f / (atp_row_sum(den) + eb);
  atp_wave_sync();   // (every lane has its q fragments)
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    if (kt < 2 * kt32) {   // a whole k step of probs V: zeros behind the last tile of keys
      const atp_f4 zero = {0.f, 0.f, 0.f, 0.f};
      atp_st4<CV>(mine + 16 * kt + 4 * lq, kt < kt16 ? sc[kt] * inv : zero);
    }
  }
  const arr_f2 pb2 = CV::widen(CV::pack(eb * inv, 0.f));
  const float pb = pb2.x;   // the bias key's probability, rounded like the others
  atp_wave_sync();

  // (probs V)^T = V^T probs^T, and the bias key's share; rounded into the buffer
  arr_u4 pf[NT / 2];
#pragma unroll
  for (int kk = 0; kk < NT / 2; ++kk)
    if (kk < kt32) pf[kk] = atp_ld16(mine + 32 * kk + 8 * lq);
  atp_wave_sync();   // (every lane has its probabilities)
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) {
    atp_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NT / 2; ++kk)
      if (kk < kt32) acc = AtpMma<CV>::mma(atp_ld16(vt + (16 * ft + lr) * VS + 32 * kk + 8 * lq), pf[kk], acc);
    const atp_f4 bv = atp_ld4<CV>(w.bias_v + 16 * ft + 4 * lq);
    acc.x = fmaf(pb, bv.x, acc.x); acc.y = fmaf(pb, bv.y, acc.y); acc.z = fmaf(pb, bv.z, acc.z); acc.w = fmaf(pb, bv.w, acc.w);
    atp_st4<CV>(mine + 16 * ft + 4 * lq, acc);
  }
  atp_wave_sync();

  // the out projection, all of the row in registers; LayerNorm; the 16 rows of the result
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = atp_ld16(mine + 32 * ks + 8 * lq);
  atp_f4 y[FT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) {
    atp_f4 acc = *reinterpret_cast<const atp_f4*>(w.out_b + 16 * ft + 4 * lq);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = AtpMma<CV>::mma(atp_ld16(w.out_w + (16 * ft + lr) * F + 32 * ks + 8 * lq), xf[ks], acc);
    y[ft] = acc;
  }
  if constexpr (LN) {   // torch's: biased variance, two passes, (x - mean) / sqrt(var + eps) * w + b
    float sum = 0.f;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) sum += atp_sum4(y[ft]);
    const float mean = atp_row_sum(sum) * (1.0f / F);
    float q = 0.f;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) { const atp_f4 d = y[ft] - mean; q += atp_sum4(d * d); }
    const float rstd = 1.0f / sqrtf(atp_row_sum(q) * (1.0f / F) + eps);
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) {
      const atp_f4 g = *reinterpret_cast<const atp_f4*>(lnw + 16 * ft + 4 * lq), b = *reinterpret_cast<const atp_f4*>(lnb + 16 * ft + 4 * lq);
      y[ft] = (y[ft] - mean) * rstd * g + b;
    }
  }
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) atp_st4<CV>(dst + (16 * s + lr) * XS + 16 * ft + 4 * lq, y[ft]);

  if (last) {   // conf_r = sigmoid(fin_r conf_w + conf_b); the strip's sum over its rows r < n of conf_r fin_r
    float d = 0.f;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) d += atp_sum4(y[ft] * *reinterpret_cast<const atp_f4*>(confw + 16 * ft + 4 * lq));
    d = atp_row_sum(d) + confb;
    const float conf = 16 * s + lr < n ? 1.0f / (1.0f + expf(-d)) : 0.f;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) {
      atp_f4 v = y[ft] * conf;
#pragma unroll
      for (int sh = 1; sh < 16; sh <<= 1) {
        v.x += __shfl_xor(v.x, sh, 64); v.y += __shfl_xor(v.y, sh, 64); v.z += __shfl_xor(v.z, sh, 64); v.w += __shfl_xor(v.w, sh, 64);
      }
      pooled[ft] += v;
    }
  }
}

template <int F, class CV, int NT>
__device__ __forceinline__ void atp_body(const atp_h* __restrict__ padded, const int32_t* __restrict__ counts, int T, int M, int P, const AtpMha& oa,
                                         const AtpMha& ta, const float* __restrict__ lnw, const float* __restrict__ lnb, float eps,
                                         const float* __restrict__ confw, const float* __restrict__ confb, float* __restrict__ out) {
  constexpr int R = 16 * NT;                  // row capacity (a multiple of 32: the k step of probs V)
  constexpr int XS = F + 8;                   // elements per row of xa, fin and kb: 16 bytes of padding, so that 16 rows hit 64 banks
  constexpr int VS = R + 8;                   // ... of vt [F][keys]
  constexpr int WS = (F > R ? F : R) + 8;     // ... of a wave's buffer [16][features or keys]
  static_assert(NT % 2 == 0, "whole k steps");
  __shared__ __attribute__((aligned(16))) atp_h xa[R * XS];    // X_t, then att_t
  __shared__ __attribute__((aligned(16))) atp_h fin[R * XS];
  __shared__ __attribute__((aligned(16))) atp_h kb[R * XS];    // K [key][feature]
  __shared__ __attribute__((aligned(16))) atp_h vt[F * VS];    // V^T [feature][key]
  __shared__ __attribute__((aligned(16))) atp_h wbuf[ATP_WAVES][16 * WS];
  __shared__ float part[ATP_WAVES][F];

  const int p = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  int n = 0;
  for (int t = 0; t < T; ++t) {
    int c = counts[(size_t)t * P + p];
    c = c > M ? M : c;
    n = c > n ? c : n;
  }
  if (n <= 0) {
    for (int f = tid; f < F; f += ATP_BLOCK) out[(size_t)p * F + f] = 0.f;
    return;
  }
  const int nt = (n + 15) >> 4;   // strips of query rows
  {   // the keys behind the last tile inside a k step of probs V meet probabilities of zero: finite from the start (zeros, later the keys of
      // an earlier result).  Every row of xa, fin and kb that is read has been written: X_t and the strips cover whole tiles.
    const arr_u4 zero = {0u, 0u, 0u, 0u};
    for (int i = tid; i < F * VS / 8; i += ATP_BLOCK) reinterpret_cast<arr_u4*>(vt)[i] = zero;
  }
  atp_f4 pooled[F / 16];
#pragma unroll
  for (int ft = 0; ft < F / 16; ++ft) { const atp_f4 zero = {0.f, 0.f, 0.f, 0.f}; pooled[ft] = zero; }
  const float cb = confb[0];
  int k = 0;   // the temporal attention's keys: max of the counts so far
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    int c = counts[(size_t)t * P + p];
    c = c > M ? M : (c < 0 ? 0 : c);
    // X_t: the c live slots, +0.0 up to the end of the last strip (att_{t-1} lay there); nothing behind c is read
    for (int i = tid; i < 16 * nt * (F / 8); i += ATP_BLOCK) {
      const int j = i / (F / 8), pc = i % (F / 8);
      arr_u4 v = {0u, 0u, 0u, 0u};
      if (j < c) v = atp_ld16(padded + (((size_t)t * M + j) * P + p) * F + 8 * pc);
      *reinterpret_cast<arr_u4*>(xa + j * XS + 8 * pc) = v;
    }
    __syncthreads();
    atp_keys_values<F, CV, XS, VS>(oa, xa, c, kb, vt, wave, lr, lq);
    __syncthreads();
#pragma unroll 1
    for (int s = wave; s < nt; s += ATP_WAVES)
      atp_strip<F, CV, NT, XS, VS, WS, false>(oa, xa, s, c, kb, vt, wbuf[wave], t == 0 ? fin : xa, lnw, lnb, eps, T == 1, n, confw, cb, pooled, lr, lq);
    __syncthreads();
    if (t > 0) {
      atp_keys_values<F, CV, XS, VS>(ta, fin, k, kb, vt, wave, lr, lq);
      __syncthreads();
#pragma unroll 1
      for (int s = wave; s < nt; s += ATP_WAVES)
        atp_strip<F, CV, NT, XS, VS, WS, true>(ta, xa, s, k, kb, vt, wbuf[wave], fin, lnw, lnb, eps, t == T - 1, n, confw, cb, pooled, lr, lq);
      __syncthreads();
    }
    k = c > k ? c : k;
  }
  if (lr == 0) {
#pragma unroll
    for (int ft = 0; ft < F / 16; ++ft) *reinterpret_cast<atp_f4*>(&part[wave][16 * ft + 4 * lq]) = pooled[ft];
  }
  __syncthreads();
  for (int f = tid; f < F; f += ATP_BLOCK) out[(size_t)p * F + f] = mt_wave_sum4(&part[0][f], F) / (float)n;
}

#define ATP_KERNEL(NAME, F, CV, NT)                                                                                                      \
  extern "C" __global__ void __launch_bounds__(ATP_BLOCK, (F) == 64 && (NT) <= 4 ? 2 : 1)                                                                              \
  NAME(const atp_h* __restrict__ padded, const int32_t* __restrict__ counts, int T, int M, int P, AtpMha oa, AtpMha ta,                   \
       const float* __restrict__ lnw, const float* __restrict__ lnb, float eps, const float* __restrict__ confw,                          \
       const float* __restrict__ confb, float* __restrict__ out) {                                                                       \
    atp_body<F, CV, NT>(padded, counts, T, M, P, oa, ta, lnw, lnb, eps, confw, confb, out);                                               \
  }
// the row capacity (16 NT rows: 32, 64, 128) only sizes the LDS image - a smaller one leaves room for a second workgroup on the CU
ATP_KERNEL(atp_64_bf16_2_kernel, 64, ArrBf16, 2)
ATP_KERNEL(atp_64_bf16_4_kernel, 64, ArrBf16, 4)
ATP_KERNEL(atp_64_bf16_8_kernel, 64, ArrBf16, 8)
ATP_KERNEL(atp_64_f16_2_kernel, 64, ArrF16, 2)
ATP_KERNEL(atp_64_f16_4_kernel, 64, ArrF16, 4)
ATP_KERNEL(atp_64_f16_8_kernel, 64, ArrF16, 8)
ATP_KERNEL(atp_128_bf16_2_kernel, 128, ArrBf16, 2)
ATP_KERNEL(atp_128_bf16_4_kernel, 128, ArrBf16, 4)
ATP_KERNEL(atp_128_bf16_8_kernel, 128, ArrBf16, 8)
ATP_KERNEL(atp_128_f16_2_kernel, 128, ArrF16, 2)
ATP_KERNEL(atp_128_f16_4_kernel, 128, ArrF16, 4)
ATP_KERNEL(atp_128_f16_8_kernel, 128, ArrF16, 8)

// ---- the entry point.  Argument errors first, then what the kernel does not take, both before a device is looked for; one launch and
// nothing else: nothing is synchronised, allocated or copied, so the call may be captured.
static bool atp_mha_complete(const dynenv_mha_t* m) { return m && m->in_w && m->out_w && m->bias_k && m->bias_v && m->in_b && m->out_b; }
static AtpMha atp_mha(const dynenv_mha_t* m) {
  AtpMha a;
  a.in_w = static_cast<const atp_h*>(m->in_w); a.out_w = static_cast<const atp_h*>(m->out_w);
  a.bias_k = static_cast<const atp_h*>(m->bias_k); a.bias_v = static_cast<const atp_h*>(m->bias_v);
  a.in_b = m->in_b; a.out_b = m->out_b;
  return a;
}

extern "C" int dynenv_attend_pool(const void* padded_dev, int32_t padded_dtype, const int32_t* obj_counts_dev, int32_t T, int32_t M, int32_t P,
                                  int32_t F, const dynenv_mha_t* obj_att, const dynenv_mha_t* temp_att, const float* ln_w_dev,
                                  const float* ln_b_dev, float ln_eps, const float* conf_w_dev, const float* conf_b_dev, float* out_dev,
                                  void* stream) {
  if (!obj_counts_dev || !ln_w_dev || !ln_b_dev || !conf_w_dev || !conf_b_dev || !out_dev || (!padded_dev && M != 0))
    return fail(DYNENV_ERR_ARG, "null argument");
  if (!atp_mha_complete(obj_att) || !atp_mha_complete(temp_att)) return fail(DYNENV_ERR_ARG, "attention: an attention has all six of its pointers");
  if (T < 1 || P < 1 || F < 1 || M < 0) return fail(DYNENV_ERR_ARG, "attention: bad shape");
  if (padded_dtype < DYNENV_ARR_F32 || padded_dtype > DYNENV_ARR_F16) return fail(DYNENV_ERR_ARG, "attention: unknown dtype (DYNENV_ARR_BF16 or _F16)");
  if (int rc = model_aligned("attention", {padded_dev, out_dev, ln_w_dev, ln_b_dev, conf_w_dev, obj_att->in_w, obj_att->out_w, obj_att->in_b, obj_att->out_b,
                                           temp_att->in_w, temp_att->out_w, temp_att->in_b, temp_att->out_b}, 16))
    return rc;
  const void* aligned8[] = {obj_att->bias_k, obj_att->bias_v, temp_att->bias_k, temp_att->bias_v};
  for (const void* q : aligned8)
    if ((uintptr_t)q % 8) return fail(DYNENV_ERR_ARG, "attention: bias_k and bias_v must be 8-byte aligned");
  if ((int64_t)T * P > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "attention: T * P too large for one launch");
  if (padded_dtype == DYNENV_ARR_F32) return fail(DYNENV_ERR_UNSUPPORTED, "attention: the fused layer takes a bf16 or fp16 padded tensor");
  if (F != 64 && F != 128) return fail(DYNENV_ERR_UNSUPPORTED, "attention: the fused layer takes F = 64 or 128");
  if (M > 128) return fail(DYNENV_ERR_UNSUPPORTED, "attention: the fused layer takes M <= 128");
  if (int rc = have_device()) return rc;
  static decltype(&atp_64_bf16_2_kernel) const kernels[2][2][3] = {
      {{atp_64_bf16_2_kernel, atp_64_bf16_4_kernel, atp_64_bf16_8_kernel}, {atp_64_f16_2_kernel, atp_64_f16_4_kernel, atp_64_f16_8_kernel}},
      {{atp_128_bf16_2_kernel, atp_128_bf16_4_kernel, atp_128_bf16_8_kernel}, {atp_128_f16_2_kernel, atp_128_f16_4_kernel, atp_128_f16_8_kernel}}};
  hipLaunchKernelGGL(kernels[F == 128][padded_dtype == DYNENV_ARR_F16][(M > 32) + (M > 64)], dim3((unsigned)P), dim3(ATP_BLOCK), 0, (hipStream_t)stream,
                     static_cast<const atp_h*>(padded_dev), obj_counts_dev, T, M, P, atp_mha(obj_att), atp_mha(temp_att), ln_w_dev, ln_b_dev,
                     ln_eps, conf_w_dev, conf_b_dev, out_dev);
  return launched();
}
