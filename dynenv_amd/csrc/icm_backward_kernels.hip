// icm_backward_kernels.hip — the backward of the curiosity losses of icm_kernels.hip (include/dynenv.h, dynenv_icm_backward): the
// gradients of forward_mean and inverse_mean (ICMNet._calc_loss, DynEnv/models/icm.py:77-109, through ICMDynamics.forward, icm.py:207-240)
// with respect to every packed operand of dynenv_icm_t and to the features, in ONE launch over the stored rollout plus a small second
// one.  NOTHING is saved by the forward: a row's hidden layer, prediction and logits are recomputed from the features, and neither
// they, the one-hot, the two cats nor a gradient of any of them exists in memory.  Included at the very END of dynenv_capi.hip, behind
// icm_kernels.hip: no existing kernel moves.  This file also holds the entry point's host code.
//
// Per ACTIVE row (t, p) (not finished; an inactive row's deltas are zeroed), with alpha = 2 s_f / (n K), beta = s_i / (n G):
//   e  = pred - f_{t+1};   dh = (W2^T e) * leaky'(h_pre);   q = cat_g(softmax(l_g) - onehot(a_g))
//   dW2 += e h^T, db2 += e;  dW1[:, :K] += dh f^T, db1 += dh, dW1_act[start_g + a_g] += dh;  dW_inv += q cat(f, f')^T, db_inv += q
//   dfeatures[t][p] += alpha W1[:, :K]^T dh + beta W_inv[:, :K]^T q;   dfeatures[t+1][p] += -alpha e + beta W_inv[:, K:]^T q
// The products run on the UNSCALED e, dh and q, rounded to w_dtype; alpha and beta are applied in float32 behind them: nothing that
// carries 1 / n, s_f or s_i is ever rounded to 16 bits (alpha is about 1e-8 at the workload's size: below fp16's subnormals).
//
// Work.  A capped, persistent grid: workgroup b of four waves takes the blocks b, b + grid, ... of ICB_ROWS = 32 players - two strips of
// 16 - and walks t = 0 .. T-1 for each, as the forward kernel does.  16x16x32 MFMAs with float32 accumulators.  Every tile that a
// product contracts over lives in LDS twice, rounded to w_dtype: row-major (the contraction runs over its columns: the recomputed
// forward and the transposed products) and transposed (the contraction runs over the 32 ROWS: the weight gradients, one MFMA per
// 16 x 16 tile and step).  Per step:
//   phase 0: features[t + 1] of the block into LDS, both ways (t = 0: features[0] too); action indices and the rows' mask
//   phase 1: hidden layer and logits as in the forward kernel (tile = wave + 4 j); a lane keeps the sign of its h_pre as a bit mask:
//            the SAME lane holds the same units of dh in phase 3; the one-hot, transposed, into LDS (an operand of the scatter-add
//            dW1_act = onehot^T dh, which so runs on the matrix units in one fixed order)
//   phase 2: the prediction, e in float32 against the float32 f_{t+1}; thread (row, group): the softmax and q
//   phase 2b / 3: dW2 += h^T e;  dh^T = W2T e^T, masked;  then dh replaces h in LDS
//   phase 4: u = W1T dh^T, v = W_invT[:K] q^T, v' = W_invT[K:] q^T in the accumulator layout of phase 2, so that the lane that held e holds
//            the same elements: dfeatures[t] = (alpha u + beta v) + carry is stored ONCE, and carry = beta v' - alpha e stays in
//            registers for step t + 1 (stored as dfeatures[T] behind the last step)
//   phase 5: dW1 += f^T dh,  dW_inv += cat(f, f')^T q,  dW1_act += dh^T onehot
// The weight gradients stay in registers across all the blocks a workgroup walks (at K = 128: 212 float32 per lane, one wave per SIMD)
// and go to the workgroup's slice of the workspace once; icm_bwd_reduce_kernel adds the slices in workgroup order and applies alpha and
// beta.  No floating-point atomic; every sum has one fixed order.  An MFMA's columns do not mix: a row of dfeatures depends on its
// player's features and actions, the weights, n and upstream alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "mma_tiles.h"

#define ICB_BLOCK 256
#define ICB_WAVES (ICB_BLOCK / 64)
#define ICB_STRIPS 2
#define ICB_ROWS (16 * ICB_STRIPS)   // 32: one k step of a weight-gradient product
#define ICB_RS (ICB_ROWS + 8)        // elements per LDS row of a transposed tile: 16 bytes of padding
#define ICB_QS 40                    // ... of the row-major q tile (32 logits)
#define ICB_HID DYNENV_ICM_HIDDEN_PAD
#define ICB_LS 33                    // floats per LDS row of the 32 logits
#define ICB_MAX_GRID DYNENV_ICM_BWD_MAX_WORKGROUPS
#define ICB_RED_BLOCK 256

// a workgroup's slice of the workspace, float32, in the layouts of dynenv_icm_grad_t one behind the other (d_fwd_w1_act with all 32 rows)
__host__ __device__ constexpr int icb_off_w1(int) { return 0; }
__host__ __device__ constexpr int icb_off_act(int K) { return ICB_HID * K; }
__host__ __device__ constexpr int icb_off_b1(int K) { return icb_off_act(K) + 32 * ICB_HID; }
__host__ __device__ constexpr int icb_off_w2(int K) { return icb_off_b1(K) + ICB_HID; }
__host__ __device__ constexpr int icb_off_b2(int K) { return icb_off_w2(K) + K * ICB_HID; }
__host__ __device__ constexpr int icb_off_iw(int K) { return icb_off_b2(K) + K; }
__host__ __device__ constexpr int icb_off_ib(int K) { return icb_off_iw(K) + 32 * 2 * K; }
__host__ __device__ constexpr int icb_part(int K) { return icb_off_ib(K) + 32; }   // 385 K + 5312

struct IcbArgs {
  const float *features, *actions;
  const unsigned char* finished;
  const atp_h *w1, *w2, *winv, *w2t, *w1t, *winvt;
  const float *w1_act, *b1, *b2, *binv;
  const float *count, *upstream;
  unsigned long long group_off;   // 8 bits per group: the first logit of group g
  unsigned group_n;               // 4 bits per group: n_g - 1
  int T, P, G, AD, nblocks;
  float slope;
  float *dfeat, *part;
  int* status;
};

// alpha = 2 s_f / (n K) and beta = s_i / (n G), +0 where n == 0: the same expressions in both kernels
__device__ __forceinline__ void icb_scales(const float* count, const float* upstream, int K, int G, float& alpha, float& beta) {
  const float n = count[2];
  alpha = n > 0.f ? (2.0f * upstream[0]) / (n * (float)K) : 0.f;
  beta = n > 0.f ? upstream[1] / (n * (float)G) : 0.f;
}

template <int K, class CV>
__device__ __forceinline__ void icb_load_tile(atp_h* xb, atp_h* xt, const float* src, int row0, int P, int tid) {
  constexpr int XS = K + 8;
  const atp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < ICB_ROWS * (K / 4); i += ICB_BLOCK) {
    const int r = i / (K / 4), col = 4 * (i % (K / 4)), p = row0 + r;
    mt_st4_both<CV, ICB_RS>(xb + r * XS + col, xt + col * ICB_RS, r, p < P ? mt_ldf4(src + (size_t)p * K + col) : zero4);
  }
}

template <int K, class CV>
__device__ __forceinline__ void icb_body(const IcbArgs& a) {
  constexpr int XS = K + 8, HS = ICB_HID + 8, RS = ICB_RS, QS = ICB_QS, S = ICB_STRIPS;
  constexpr int KS = K / 32, HT = ICB_HID / 16, HKS = ICB_HID / 32;
  constexpr int TPW = (HT + 2) / ICB_WAVES;                  // 3: tiles per wave in phases 1 and 3
  constexpr int OT = K / 16, OPW = OT / ICB_WAVES;           // tiles of a feature row, per wave
  constexpr int CPW = 2 * OT / ICB_WAVES;                    // tiles of cat(f, f'), per wave
  constexpr int APW = 2 * HT / ICB_WAVES;                    // 5: tiles of dW1_act, per wave
  static_assert((HT + 2) % ICB_WAVES == 0 && OT % ICB_WAVES == 0 && HT == 10 && ICB_ROWS == 32, "the deal of the tiles");
  __shared__ __attribute__((aligned(16))) atp_h xb[2][ICB_ROWS * XS];   // f_t / f_{t+1}, row-major: swap roles
  __shared__ __attribute__((aligned(16))) atp_h xt[2][K * RS];          // ... transposed
  __shared__ __attribute__((aligned(16))) atp_h hb[ICB_ROWS * HS];      // h, then dh
  __shared__ __attribute__((aligned(16))) atp_h ht[ICB_HID * RS];       // ... transposed
  __shared__ __attribute__((aligned(16))) atp_h eb[ICB_ROWS * XS];
  __shared__ __attribute__((aligned(16))) atp_h et[K * RS];
  __shared__ __attribute__((aligned(16))) atp_h qb[ICB_ROWS * QS];
  __shared__ __attribute__((aligned(16))) atp_h qt[32 * RS];
  __shared__ __attribute__((aligned(16))) atp_h ot[32 * RS];            // the one-hot, transposed
  __shared__ float lg[ICB_ROWS * ICB_LS];                               // the logits, then q in float32
  __shared__ int acts[ICB_ROWS * 8];
  __shared__ int on[ICB_ROWS];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int P = a.P, G = a.G;
  const atp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bool inv_wave = wave >= 2;   // tiles 10 and 11, the logits, are the third tile of waves 2 and 3
  const atp_h one = mt_h<CV>(1.0f);
  float alpha, beta;
  icb_scales(a.count, a.upstream, K, G, alpha, beta);

  for (int i = tid; i < ICB_ROWS * QS; i += ICB_BLOCK) qb[i] = 0;   // the logits from N on stay +0
  for (int i = tid; i < 32 * RS; i += ICB_BLOCK) qt[i] = 0;

  atp_f4 gW2[OPW][HT], gW1[OPW][HT], gWi[CPW][2], gWa[APW], db2[OPW], db1[TPW];
  float dbi = 0.f;
#pragma unroll
  for (int j = 0; j < OPW; ++j) {
    db2[j] = zero4;
#pragma unroll
    for (int h = 0; h < HT; ++h) { gW2[j][h] = zero4; gW1[j][h] = zero4; }
  }
#pragma unroll
  for (int j = 0; j < CPW; ++j) { gWi[j][0] = zero4; gWi[j][1] = zero4; }
#pragma unroll
  for (int j = 0; j < APW; ++j) gWa[j] = zero4;
#pragma unroll
  for (int j = 0; j < TPW; ++j) db1[j] = zero4;

  for (int blk = (int)blockIdx.x; blk < a.nblocks; blk += (int)gridDim.x) {
    const int row0 = blk * ICB_ROWS;
    atp_f4 carry[OPW][S];
#pragma unroll
    for (int j = 0; j < OPW; ++j)
#pragma unroll
      for (int s = 0; s < S; ++s) carry[j][s] = zero4;
    icb_load_tile<K, CV>(xb[0], xt[0], a.features, row0, P, tid);
    for (int t = 0; t < a.T; ++t) {
      const int ci = t & 1, ni = (t + 1) & 1;
      const atp_h *cur = xb[ci], *nxt = xb[ni];
      const float* next32 = a.features + (size_t)(t + 1) * P * K;
      // ---- phase 0
      icb_load_tile<K, CV>(xb[ni], xt[ni], next32, row0, P, tid);
      bool clamped = false;
      for (int i = tid; i < ICB_ROWS * G; i += ICB_BLOCK) {
        const int g = i / ICB_ROWS, r = i % ICB_ROWS, p = row0 + r;
        const MtGroup gr = mt_group(a.group_off, a.group_n, g);
        const int off = gr.off, n = gr.n;
        acts[r * 8 + g] = off + (p < P ? mt_stored_action(a.actions[((size_t)t * a.AD + g) * P + p], n - 1, clamped) : 0);
      }
      if (clamped && a.status) atomicOr(a.status, 1);
      if (tid < ICB_ROWS) {
        const int p = row0 + tid;
        on[tid] = p < P && !(a.finished && a.finished[(size_t)t * P + p]) ? 1 : 0;
      }
      __syncthreads();

      // ---- phase 1: the hidden layer and the logits; the one-hot
      unsigned pos = 0;   // bit (j S + s) 4 + i: h_pre > 0
      {
        const int r = tid & 31, n0 = 4 * (tid >> 5);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          bool hit = false;
          for (int g = 0; g < G; ++g) hit |= acts[r * 8 + g] == n0 + i;
          ot[(n0 + i) * RS + r] = hit ? one : (atp_h)0;
        }
        atp_f4 y[TPW][S];
        const atp_h* wrow[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          const int tile = wave + ICB_WAVES * j;
          atp_f4 b;
          if (tile < HT) {
            b = mt_ldf4(a.b1 + 16 * tile + 4 * lq);
            wrow[j] = a.w1 + (size_t)(16 * tile + lr) * K;
          } else {
            b = mt_ldf4(a.binv + 16 * (tile - HT) + 4 * lq);
            wrow[j] = a.winv + (size_t)(16 * (tile - HT) + lr) * (2 * K);
          }
#pragma unroll
          for (int s = 0; s < S; ++s) y[j][s] = b;
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          arr_u4 xf[S];
#pragma unroll
          for (int s = 0; s < S; ++s) xf[s] = atp_ld16(cur + (16 * s + lr) * XS + 32 * ks + 8 * lq);
#pragma unroll
          for (int j = 0; j < TPW; ++j) {
            const arr_u4 w = atp_ld16(wrow[j] + 32 * ks + 8 * lq);
#pragma unroll
            for (int s = 0; s < S; ++s) y[j][s] = AtpMma<CV>::mma(w, xf[s], y[j][s]);
          }
        }
        if (inv_wave) {   // the second half of cat(cur, next)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const arr_u4 w = atp_ld16(wrow[TPW - 1] + K + 32 * ks + 8 * lq);
#pragma unroll
            for (int s = 0; s < S; ++s)
              y[TPW - 1][s] = AtpMma<CV>::mma(w, atp_ld16(nxt + (16 * s + lr) * XS + 32 * ks + 8 * lq), y[TPW - 1][s]);
          }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          const int tile = wave + ICB_WAVES * j;
          if (tile < HT) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
              const int r = 16 * s + lr;
              atp_f4 v = y[j][s];
              for (int g = 0; g < G; ++g) v += mt_ldf4(a.w1_act + (size_t)acts[r * 8 + g] * ICB_HID + 16 * tile + 4 * lq);
              pos |= mt_pos4(v) << (4 * (j * S + s));
              mt_st4_both<CV, ICB_RS>(hb + r * HS + 16 * tile + 4 * lq, ht + (16 * tile + 4 * lq) * RS, r, mt_leaky4(v, a.slope));
            }
          } else {
#pragma unroll
            for (int s = 0; s < S; ++s) mt_st_f4(lg + (16 * s + lr) * ICB_LS + 16 * (tile - HT) + 4 * lq, y[j][s]);
          }
        }
      }
      __syncthreads();

      // ---- phase 2: e = pred - f_{t+1} in float32, zeroed for an inactive row; q by thread (row, group)
      atp_f4 carryn[OPW][S];   // -alpha e
      {
        atp_f4 z[OPW][S];
        const atp_h* wrow[OPW];
#pragma unroll
        for (int j = 0; j < OPW; ++j) {
          const int tile = wave + ICB_WAVES * j;
          const atp_f4 b = mt_ldf4(a.b2 + 16 * tile + 4 * lq);
          wrow[j] = a.w2 + (size_t)(16 * tile + lr) * ICB_HID;
#pragma unroll
          for (int s = 0; s < S; ++s) z[j][s] = b;
        }
#pragma unroll
        for (int ks = 0; ks < HKS; ++ks) {
          arr_u4 hf[S];
#pragma unroll
          for (int s = 0; s < S; ++s) hf[s] = atp_ld16(hb + (16 * s + lr) * HS + 32 * ks + 8 * lq);
#pragma unroll
          for (int j = 0; j < OPW; ++j) {
            const arr_u4 w = atp_ld16(wrow[j] + 32 * ks + 8 * lq);
#pragma unroll
            for (int s = 0; s < S; ++s) z[j][s] = AtpMma<CV>::mma(w, hf[s], z[j][s]);
          }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int r = 16 * s + lr, p = row0 + r;
          const bool live = on[r] != 0;   // (implies p < P)
#pragma unroll
          for (int j = 0; j < OPW; ++j) {
            const int col = 16 * (wave + ICB_WAVES * j) + 4 * lq;
            const atp_f4 e = live ? z[j][s] - mt_ldf4(next32 + (size_t)p * K + col) : zero4;
            db2[j] += e;
            carryn[j][s] = zero4 - alpha * e;
            mt_st4_both<CV, ICB_RS>(eb + r * XS + col, et + col * RS, r, e);
          }
        }
      }
      {
        const int r = tid & 31, g = tid >> 5;
        if (g < G) {
          float* L = lg + r * ICB_LS;
          const MtGroup gr = mt_group(a.group_off, a.group_n, g);
          const int off = gr.off, n = gr.n;
          const int taken = acts[r * 8 + g];
          const bool live = on[r] != 0;
          float m = L[off];
          for (int j = 1; j < n; ++j) m = fmaxf(m, L[off + j]);
          float sum = 0.f;
          for (int j = 0; j < n; ++j) sum += expf(L[off + j] - m);
          for (int j = 0; j < n; ++j) {
            const float sm = expf(L[off + j] - m) / sum;   // a group of one action: exp(0) / 1 - 1 = 0
            const float q = live ? sm - (off + j == taken ? 1.0f : 0.0f) : 0.0f;
            L[off + j] = q;
            const atp_h q16 = mt_h<CV>(q);
            qb[r * QS + off + j] = q16;
            qt[(off + j) * RS + r] = q16;
          }
        }
      }
      __syncthreads();

      // ---- phase 2b: db_inv in row order; dW2 += h^T e (D[hidden][k])
      if (tid < 32) {
        for (int r = 0; r < ICB_ROWS; ++r) dbi += lg[r * ICB_LS + tid];
      }
      {
        arr_u4 ef[OPW];
#pragma unroll
        for (int j = 0; j < OPW; ++j) ef[j] = atp_ld16(et + (16 * (wave + ICB_WAVES * j) + lr) * RS + 8 * lq);
#pragma unroll
        for (int h = 0; h < HT; ++h) {
          const arr_u4 hf = atp_ld16(ht + (16 * h + lr) * RS + 8 * lq);
#pragma unroll
          for (int j = 0; j < OPW; ++j) gW2[j][h] = AtpMma<CV>::mma(hf, ef[j], gW2[j][h]);
        }
      }
      // ---- phase 3: dh^T = W2T e^T, times leaky'(h_pre) by the lane that computed h_pre
      atp_f4 d[TPW][S];
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const int tile = wave + ICB_WAVES * j;
#pragma unroll
        for (int s = 0; s < S; ++s) d[j][s] = zero4;
        if (tile < HT) {
          const atp_h* wrow = a.w2t + (size_t)(16 * tile + lr) * K;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const arr_u4 w = atp_ld16(wrow + 32 * ks + 8 * lq);
#pragma unroll
            for (int s = 0; s < S; ++s) d[j][s] = AtpMma<CV>::mma(w, atp_ld16(eb + (16 * s + lr) * XS + 32 * ks + 8 * lq), d[j][s]);
          }
#pragma unroll
          for (int s = 0; s < S; ++s) {
            d[j][s] = mt_leaky_grad4(d[j][s], pos >> (4 * (j * S + s)), a.slope);
            db1[j] += d[j][s];
          }
        }
      }
      __syncthreads();   // h has been read by everybody
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const int tile = wave + ICB_WAVES * j;
        if (tile < HT) {
#pragma unroll
          for (int s = 0; s < S; ++s) mt_st4_both<CV, ICB_RS>(hb + (16 * s + lr) * HS + 16 * tile + 4 * lq, ht + (16 * tile + 4 * lq) * RS, 16 * s + lr, d[j][s]);
        }
      }
      __syncthreads();

      // ---- phase 4: dfeatures[t], stored once; the carry for t + 1
#pragma unroll
      for (int j = 0; j < OPW; ++j) {
        const int kt = wave + ICB_WAVES * j;
        atp_f4 u[S], v[S], v2[S];
#pragma unroll
        for (int s = 0; s < S; ++s) { u[s] = zero4; v[s] = zero4; v2[s] = zero4; }
        const atp_h* wrow = a.w1t + (size_t)(16 * kt + lr) * ICB_HID;
#pragma unroll
        for (int ks = 0; ks < HKS; ++ks) {
          const arr_u4 w = atp_ld16(wrow + 32 * ks + 8 * lq);
#pragma unroll
          for (int s = 0; s < S; ++s) u[s] = AtpMma<CV>::mma(w, atp_ld16(hb + (16 * s + lr) * HS + 32 * ks + 8 * lq), u[s]);
        }
        const arr_u4 wa = atp_ld16(a.winvt + (size_t)(16 * kt + lr) * 32 + 8 * lq), wb = atp_ld16(a.winvt + (size_t)(K + 16 * kt + lr) * 32 + 8 * lq);
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const arr_u4 qf = atp_ld16(qb + (16 * s + lr) * QS + 8 * lq);
          v[s] = AtpMma<CV>::mma(wa, qf, v[s]);
          v2[s] = AtpMma<CV>::mma(wb, qf, v2[s]);
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int p = row0 + 16 * s + lr;
          const atp_f4 out = ((alpha * u[s] + beta * v[s]) + carry[j][s]) + zero4;   // (+ 0: no -0 leaves)
          if (a.dfeat && p < P) *reinterpret_cast<atp_f4*>(a.dfeat + ((size_t)t * P + p) * K + 16 * kt + 4 * lq) = out;
          carry[j][s] = beta * v2[s] + carryn[j][s];
        }
      }
      // ---- phase 5: dW1 += f^T dh (D[k][hidden]); dW_inv += cat(f, f')^T q (D[column][logit]); dW1_act += dh^T onehot (D[hidden][action row])
      {
        arr_u4 ff[OPW];
#pragma unroll
        for (int j = 0; j < OPW; ++j) ff[j] = atp_ld16(xt[ci] + (16 * (wave + ICB_WAVES * j) + lr) * RS + 8 * lq);
#pragma unroll
        for (int h = 0; h < HT; ++h) {
          const arr_u4 df = atp_ld16(ht + (16 * h + lr) * RS + 8 * lq);
#pragma unroll
          for (int j = 0; j < OPW; ++j) gW1[j][h] = AtpMma<CV>::mma(ff[j], df, gW1[j][h]);
        }
        const arr_u4 q0 = atp_ld16(qt + lr * RS + 8 * lq), q1 = atp_ld16(qt + (16 + lr) * RS + 8 * lq);
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
          const int ct = wave + ICB_WAVES * j;
          const atp_h* src = ct < OT ? xt[ci] + (16 * ct + lr) * RS : xt[ni] + (16 * (ct - OT) + lr) * RS;
          const arr_u4 xf = atp_ld16(src + 8 * lq);
          gWi[j][0] = AtpMma<CV>::mma(xf, q0, gWi[j][0]);
          gWi[j][1] = AtpMma<CV>::mma(xf, q1, gWi[j][1]);
        }
#pragma unroll
        for (int j = 0; j < APW; ++j) {
          const int id = wave + ICB_WAVES * j, h = id % HT, at = id / HT;
          gWa[j] = AtpMma<CV>::mma(atp_ld16(ht + (16 * h + lr) * RS + 8 * lq), atp_ld16(ot + (16 * at + lr) * RS + 8 * lq), gWa[j]);
        }
      }
      __syncthreads();   // the next step's phase 0 overwrites the tile that was `cur`
    }
    if (a.dfeat) {
#pragma unroll
      for (int j = 0; j < OPW; ++j)
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int p = row0 + 16 * s + lr;
          if (p < P) *reinterpret_cast<atp_f4*>(a.dfeat + ((size_t)a.T * P + p) * K + 16 * (wave + ICB_WAVES * j) + 4 * lq) = carry[j][s] + zero4;
        }
    }
  }

  // ---- this workgroup's slice: every element stored once
  float* part = a.part + (size_t)blockIdx.x * icb_part(K);
#pragma unroll
  for (int j = 0; j < OPW; ++j) {
    const int kt = wave + ICB_WAVES * j;
#pragma unroll
    for (int h = 0; h < HT; ++h) {
      *reinterpret_cast<atp_f4*>(part + icb_off_w1(K) + (16 * h + lr) * K + 16 * kt + 4 * lq) = gW1[j][h];
      *reinterpret_cast<atp_f4*>(part + icb_off_w2(K) + (16 * kt + lr) * ICB_HID + 16 * h + 4 * lq) = gW2[j][h];
    }
    const atp_f4 b = mt_sum16(db2[j]);
    if (lr == 0) *reinterpret_cast<atp_f4*>(part + icb_off_b2(K) + 16 * kt + 4 * lq) = b;
  }
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    const int ct = wave + ICB_WAVES * j;
    *reinterpret_cast<atp_f4*>(part + icb_off_iw(K) + lr * (2 * K) + 16 * ct + 4 * lq) = gWi[j][0];
    *reinterpret_cast<atp_f4*>(part + icb_off_iw(K) + (16 + lr) * (2 * K) + 16 * ct + 4 * lq) = gWi[j][1];
  }
#pragma unroll
  for (int j = 0; j < APW; ++j) {
    const int id = wave + ICB_WAVES * j, h = id % HT, at = id / HT;
    *reinterpret_cast<atp_f4*>(part + icb_off_act(K) + (16 * at + lr) * ICB_HID + 16 * h + 4 * lq) = gWa[j];
  }
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int tile = wave + ICB_WAVES * j;
    const atp_f4 b = mt_sum16(db1[j]);
    if (tile < HT && lr == 0) *reinterpret_cast<atp_f4*>(part + icb_off_b1(K) + 16 * tile + 4 * lq) = b;
  }
  if (tid < 32) part[icb_off_ib(K) + tid] = dbi;
}

#define ICB_KERNEL(NAME, K, CV) \
  extern "C" __global__ void __launch_bounds__(ICB_BLOCK) NAME(IcbArgs a) { icb_body<K, CV>(a); }
ICB_KERNEL(icm_bwd_64_bf16_kernel, 64, ArrBf16)
ICB_KERNEL(icm_bwd_64_f16_kernel, 64, ArrF16)
ICB_KERNEL(icm_bwd_128_bf16_kernel, 128, ArrBf16)
ICB_KERNEL(icm_bwd_128_f16_kernel, 128, ArrF16)

// The second launch: element i of the slices added in workgroup order, times alpha (the forward net's) or beta (the inverse net's), into
// its place in dynenv_icm_grad_t; the rows of d_fwd_w1_act from N on are not stored (the buffer has N).
struct IcbGrad { float *w1, *act, *b1, *w2, *b2, *iw, *ib; };
extern "C" __global__ void __launch_bounds__(ICB_RED_BLOCK) icm_bwd_reduce_kernel(const float* __restrict__ part, int slices, int K, int G, int N,
                                                                                   const float* __restrict__ count, const float* __restrict__ upstream, IcbGrad o) {
  const int i = (int)(blockIdx.x * ICB_RED_BLOCK + threadIdx.x), n = icb_part(K);
  if (i >= n) return;
  float alpha, beta;
  icb_scales(count, upstream, K, G, alpha, beta);
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < slices; ++b) s += part[(size_t)b * n + i];
  const float fwd = alpha * s + 0.f, inv = beta * s + 0.f;   // (+ 0: no -0 leaves)
  if (i < icb_off_act(K)) o.w1[i] = fwd;
  else if (i < icb_off_b1(K)) { if (i - icb_off_act(K) < N * ICB_HID) o.act[i - icb_off_act(K)] = fwd; }
  else if (i < icb_off_w2(K)) o.b1[i - icb_off_b1(K)] = fwd;
  else if (i < icb_off_b2(K)) o.w2[i - icb_off_w2(K)] = fwd;
  else if (i < icb_off_iw(K)) o.b2[i - icb_off_b2(K)] = fwd;
  else if (i < icb_off_ib(K)) o.iw[i - icb_off_iw(K)] = inv;
  else o.ib[i - icb_off_ib(K)] = inv;
}

// ---- the entry points.  Argument errors first, then what the kernel does not take, both before a device is looked for.
static int icb_groups(int32_t P) {
  const int64_t blocks = ((int64_t)P + ICB_ROWS - 1) / ICB_ROWS;
  return (int)(blocks < ICB_MAX_GRID ? blocks : ICB_MAX_GRID);
}

extern "C" int dynenv_icm_backward_workspace(int32_t P, int32_t K, uint64_t* bytes) {
  if (!bytes) return fail(DYNENV_ERR_ARG, "icm backward workspace: null argument");
  if (P < 1 || K < 1) return fail(DYNENV_ERR_ARG, "icm backward workspace: bad shape");
  if (K != 64 && K != 128) return fail(DYNENV_ERR_UNSUPPORTED, "icm backward workspace: the fused backward takes K = 64 or 128");
  *bytes = (uint64_t)icb_groups(P) * (uint64_t)icb_part(K) * 4u;
  return DYNENV_OK;
}

extern "C" int dynenv_icm_backward(const float* features_dev, const float* actions_dev, const uint8_t* finished_dev, int32_t T, int32_t P, int32_t K,
                                   int32_t action_cols, const int32_t* nvec, int32_t G, int32_t w_dtype, const dynenv_icm_t* w, float slope,
                                   const float* count_dev, const float* upstream_dev, const dynenv_icm_bwd_t* wt, const dynenv_icm_grad_t* grad,
                                   float* d_features_dev, void* workspace_dev, uint64_t workspace_bytes, int32_t* status_dev, void* stream) {
  if (!features_dev || !actions_dev || !nvec || !w || !count_dev || !upstream_dev || !wt || !grad || !workspace_dev)
    return fail(DYNENV_ERR_ARG, "icm backward: null argument");
  if (!w->fwd_w1 || !w->fwd_w1_act || !w->fwd_b1 || !w->fwd_w2 || !w->fwd_b2 || !w->inv_w || !w->inv_b)
    return fail(DYNENV_ERR_ARG, "icm backward: the forward and the inverse net have all seven of their pointers");
  if (!wt->fwd_w2_t || !wt->fwd_w1_t || !wt->inv_w_t) return fail(DYNENV_ERR_ARG, "icm backward: the three transposed copies have their pointers");
  if (!grad->d_fwd_w1 || !grad->d_fwd_w1_act || !grad->d_fwd_b1 || !grad->d_fwd_w2 || !grad->d_fwd_b2 || !grad->d_inv_w || !grad->d_inv_b)
    return fail(DYNENV_ERR_ARG, "icm backward: the seven gradients have their pointers");
  if (T < 1 || P < 1 || K < 1) return fail(DYNENV_ERR_ARG, "icm backward: bad shape");
  if (G < 1 || G > DYNENV_POLICY_MAX_GROUPS) return fail(DYNENV_ERR_ARG, "icm backward: G is 1..8");
  ModelGroups gr;
  if (int rc = model_groups("icm backward", nvec, G, action_cols, gr)) return rc;
  if (int rc = model_operand_dtype("icm backward", w_dtype)) return rc;
  if (int rc = model_aligned("icm backward", {features_dev, actions_dev, finished_dev, d_features_dev, workspace_dev, w->fwd_w1, w->fwd_w1_act, w->fwd_b1,
                                              w->fwd_w2, w->fwd_b2, w->inv_w, w->inv_b, wt->fwd_w2_t, wt->fwd_w1_t, wt->inv_w_t, grad->d_fwd_w1,
                                              grad->d_fwd_w1_act, grad->d_fwd_b1, grad->d_fwd_w2, grad->d_fwd_b2, grad->d_inv_w, grad->d_inv_b}, 16))
    return rc;
  if ((uintptr_t)count_dev % 4 || (uintptr_t)upstream_dev % 4 || (uintptr_t)status_dev % 4)
    return fail(DYNENV_ERR_ARG, "icm backward: count_dev, upstream_dev and status_dev are 4-byte aligned");
  if (((int64_t)T + 1) * P > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "icm backward: (T + 1) * P too large for one launch");
  if ((K == 64 || K == 128) && workspace_bytes < (uint64_t)icb_groups(P) * (uint64_t)icb_part(K) * 4u)
    return fail(DYNENV_ERR_ARG, "icm backward: the workspace is smaller than dynenv_icm_backward_workspace asks for");
  if (int rc = model_operand_16bit("icm backward", w_dtype, "backward")) return rc;
  if (K != 64 && K != 128) return fail(DYNENV_ERR_UNSUPPORTED, "icm backward: the fused backward takes K = 64 or 128");
  if (int rc = have_device()) return rc;
  IcbArgs k;
  k.features = features_dev; k.actions = actions_dev; k.finished = finished_dev;
  k.w1 = static_cast<const atp_h*>(w->fwd_w1); k.w2 = static_cast<const atp_h*>(w->fwd_w2); k.winv = static_cast<const atp_h*>(w->inv_w);
  k.w2t = static_cast<const atp_h*>(wt->fwd_w2_t); k.w1t = static_cast<const atp_h*>(wt->fwd_w1_t); k.winvt = static_cast<const atp_h*>(wt->inv_w_t);
  k.w1_act = w->fwd_w1_act; k.b1 = w->fwd_b1; k.b2 = w->fwd_b2; k.binv = w->inv_b;
  k.count = count_dev; k.upstream = upstream_dev;
  k.group_off = gr.off; k.group_n = gr.n;
  k.T = T; k.P = P; k.G = G; k.AD = action_cols; k.nblocks = (P + ICB_ROWS - 1) / ICB_ROWS; k.slope = slope;
  k.dfeat = d_features_dev; k.part = static_cast<float*>(workspace_dev); k.status = status_dev;
  const int groups = icb_groups(P);
  static decltype(&icm_bwd_64_bf16_kernel) const kernels[2][2] = {{icm_bwd_64_bf16_kernel, icm_bwd_64_f16_kernel}, {icm_bwd_128_bf16_kernel, icm_bwd_128_f16_kernel}};
  hipLaunchKernelGGL(kernels[K == 128][w_dtype == DYNENV_ARR_F16], dim3((unsigned)groups), dim3(ICB_BLOCK), 0, (hipStream_t)stream, k);
  IcbGrad o = {grad->d_fwd_w1, grad->d_fwd_w1_act, grad->d_fwd_b1, grad->d_fwd_w2, grad->d_fwd_b2, grad->d_inv_w, grad->d_inv_b};
  hipLaunchKernelGGL(icm_bwd_reduce_kernel, dim3((unsigned)((icb_part(K) + ICB_RED_BLOCK - 1) / ICB_RED_BLOCK)), dim3(ICB_RED_BLOCK), 0, (hipStream_t)stream,
                     (const float*)workspace_dev, groups, (int)K, (int)G, gr.N, count_dev, upstream_dev, o);
  return launched();
}
