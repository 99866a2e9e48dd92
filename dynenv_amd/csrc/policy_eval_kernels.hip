// policy_eval_kernels.hip — the policy head over a STORED rollout, with its backward (include/dynenv.h, dynenv_policy_eval,
// dynenv_policy_eval_backward): log_prob of the stored actions, the probabilities and the critic's value for every row (t, p) of
// features [T][P][K], and the gradients of those three with respect to the eight packed operands of dynenv_policy_t and to the features.
// The loss between the two stays torch's.  Included at the very END of dynenv_capi.hip, behind icm_backward_kernels.hip: no existing
// kernel moves.  This file also holds the entry points' host code.
//
// The forward IS policy_kernels.hip's kernel body (ph_body with EVAL): the same device function, so a row has the bits dynenv_policy_head
// gave it when it drew that action.  The backward saves nothing: per block of PH_ROWS = 64 rows it runs ph_forward again, then
//   phase B1: thread (row, wave q) takes the groups q, q + 4: softmax, the stored action, and
//             dl_g = d_logp_g [not clamped] (onehot(a_g) - probs_g) + probs_g (d_probs_g - <d_probs_g, probs_g>)  in float32, into LDS
//             as float32 (the bias gradient) and, rounded to bf16, row-major and transposed
//   phase B2: the critic, on the lanes that hold the hidden layer: with c = w2 * ln_w, xh = (h - mean) rstd,
//             dh_pre = d_value * (rstd (c - mean(c) - xh mean(c xh))) * leaky'(h_pre)  - the bracket does not carry the upstream -
//             and the float32 sums d_b1, d_ln_w, d_ln_b, d_w2, d_b2; dh_pre rounded to bf16 into LDS, both ways
//   phase B3: d_features = dl W_actor + dh_pre W1 in the accumulator layout D^T = W^T X^T (the transposed copies of dynenv_policy_bwd_t
//             are the A operands): a lane holds four consecutive columns of one row and stores them once
//   phase B4: d_actor_w += dl^T x and d_critic_w1 += dh_pre^T x, contracted over the 64 rows: two k steps per 16 x 16 tile
// on a capped, persistent grid as icm_backward_kernels.hip's: workgroup b takes the blocks b, b + grid, ...; the weight gradients stay in
// registers across them ((32 + K / 2) K / 256 float32 per lane) and go to the workgroup's slice of the workspace once;
// pe_bwd_reduce_kernel adds the slices in workgroup order.  No floating-point atomic; every sum has one fixed order.
// What carries an upstream gradient - dl, dh_pre - is bf16 whatever w_dtype is (float16's range does not hold 1 / (T P G)); the operand
// beside it in a product - the transposed weights, the transposed rows - is bf16 too.  With w_dtype float16, whose 11 significant bits
// one bf16 does not hold, every one of these operands is a PAIR of bf16 - the rounding, and the rounding of what it left: 16 bits - and
// a product is three MFMAs (hi hi, hi lo, lo hi).  Rounding to bf16 and float32 accumulation commute with a power of two: scaling the
// three upstream tensors by one scales every output by it exactly.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "mma_tiles.h"

#define PE_QS 40   // elements per LDS row of the row-major dl tile (32 logits): 16 bytes of padding
#define PE_MAX_GRID DYNENV_POLICY_EVAL_MAX_WORKGROUPS
#define PE_RED_BLOCK 256

// a workgroup's slice of the workspace, float32, in the layouts of dynenv_policy_grad_t one behind the other (d_critic_b2 padded to four)
__host__ __device__ constexpr int pe_off_aw(int) { return 0; }
__host__ __device__ constexpr int pe_off_w1(int K) { return 32 * K; }
__host__ __device__ constexpr int pe_off_ab(int K) { return pe_off_w1(K) + (K / 2) * K; }
__host__ __device__ constexpr int pe_off_b1(int K) { return pe_off_ab(K) + 32; }
__host__ __device__ constexpr int pe_off_lnw(int K) { return pe_off_b1(K) + K / 2; }
__host__ __device__ constexpr int pe_off_lnb(int K) { return pe_off_lnw(K) + K / 2; }
__host__ __device__ constexpr int pe_off_w2(int K) { return pe_off_lnb(K) + K / 2; }
__host__ __device__ constexpr int pe_off_b2(int K) { return pe_off_w2(K) + K / 2; }
__host__ __device__ constexpr int pe_part(int K) { return pe_off_b2(K) + 4; }   // K K / 2 + 34 K + 36

struct PeArgs {
  PhArgs f;   // the forward's: P = T * ev_P rows, no outputs
  const float *d_logp, *d_probs, *d_value;
  const atp_h *actor_wt, *w1t, *actor_wtl, *w1tl;
  float *dfeat, *part;
  int nblocks;
};

// the operands that carry an upstream gradient, and those beside them, are bf16: mt_split and mt_mma_split (mma_tiles.h)
template <class CV> struct PeSplit { static constexpr bool on = false; };
template <> struct PeSplit<ArrF16> { static constexpr bool on = true; };   // w_dtype float16: every bf16 operand of the backward's products is a pair

template <int K, class CV>
__device__ __forceinline__ void pe_bwd_body(const PeArgs& a) {
  constexpr int H = PhShape<K>::H, CT = PhShape<K>::CT, TPW = PhShape<K>::TPW, XS = PhShape<K>::XS;
  constexpr int HS = H + 8, HKS = H / 32, OT = K / 16, OPW = OT / PH_WAVES, S = PH_STRIPS, TS = PH_TS, RKS = PH_ROWS / 32;
  constexpr bool SP = PeSplit<CV>::on;
  constexpr int LO = SP ? 1 : 0;   // the second halves of the pairs exist with float16 only
  static_assert(OT % PH_WAVES == 0 && CT <= PH_WAVES && TPW * S * 4 <= 32, "the deal of the tiles; the sign mask");
  __shared__ __attribute__((aligned(16))) atp_h xb[PH_ROWS * XS];    // the rows, w_dtype, row-major: the forward's operand
  __shared__ __attribute__((aligned(16))) atp_h xt[K * TS];          // ... bf16, transposed
  __shared__ __attribute__((aligned(16))) atp_h dhb[PH_ROWS * HS];   // dh_pre, bf16, row-major
  __shared__ __attribute__((aligned(16))) atp_h dht[H * TS];         // ... transposed
  __shared__ __attribute__((aligned(16))) atp_h dlb[PH_ROWS * PE_QS];
  __shared__ __attribute__((aligned(16))) atp_h dlt[32 * TS];
  __shared__ __attribute__((aligned(16))) atp_h xtl[LO * K * TS + 8], dhbl[LO * PH_ROWS * HS + 8], dhtl[LO * H * TS + 8], dlbl[LO * PH_ROWS * PE_QS + 8],
      dltl[LO * 32 * TS + 8];                                        // the pairs' second halves
  __shared__ float lg[PH_ROWS * PH_LS];                              // the logits, the probabilities, then dl in float32
  __shared__ float dp[PH_ROWS * PH_LS];                              // d_probs of the block
  __shared__ float part[3 * PH_WAVES * PH_ROWS];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int R = a.f.P, G = a.f.G, N = a.f.N;
  const atp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

  atp_f4 gA[OPW][2], gC[OPW][CT], db1 = zero4, dlnw = zero4, dlnb = zero4, dw2 = zero4;
  float db2 = 0.f, dab = 0.f;
#pragma unroll
  for (int j = 0; j < OPW; ++j) {
    gA[j][0] = zero4; gA[j][1] = zero4;
#pragma unroll
    for (int c = 0; c < CT; ++c) gC[j][c] = zero4;
  }
  // the critic tile of this wave (CT <= 4: at most one, t = 0) and its float32 operands
  const bool critic = wave < CT;
  atp_f4 lnw4 = zero4, lnb4 = zero4, w24 = zero4;
  if (critic) {
    lnw4 = mt_ldf4(a.f.ln_w + 16 * wave + 4 * lq); lnb4 = mt_ldf4(a.f.ln_b + 16 * wave + 4 * lq); w24 = mt_ldf4(a.f.w2 + 16 * wave + 4 * lq);
  }
  const atp_f4 c4 = w24 * lnw4;

  for (int blk = (int)blockIdx.x; blk < a.nblocks; blk += (int)gridDim.x) {
    const int row0 = blk * PH_ROWS, rows = min(PH_ROWS, R - row0);
    if (a.d_probs)
      for (int i = tid; i < rows * N; i += PH_BLOCK) dp[(i / N) * PH_LS + i % N] = a.d_probs[(size_t)row0 * N + i];
    atp_f4 y[TPW][S];
    float mean[S], rstd[S];
    unsigned pos = 0;
    ph_forward<K, CV, true>(a.f, row0, xb, xt, SP ? xtl : nullptr, lg, part, y, mean, rstd, pos);

    // ---- phase B1: dl by thread (row, group)
    {
      const int r = lane, q = wave, p = row0 + r;
      float* L = lg + r * PH_LS;
      const float* D = dp + r * PH_LS;
      bool clamped = false;
      for (int g = q; g < G; g += PH_WAVES) {
        const MtGroup gr = mt_group(a.f.group_off, a.f.group_n, g);
        const int off = gr.off, n = gr.n;
        ph_softmax(L, off, n);
        int act = 0;
        float up = 0.f;
        bool live = false;
        if (p < R) {
          act = ph_stored_action(a.f, p, g, n - 1, clamped);
          const int t = p / a.f.ev_P;
          up = a.d_logp[((size_t)t * G + g) * a.f.ev_P + (p - t * a.f.ev_P)];
          const float eps32 = 1.1920928955078125e-07f, pa = L[off + act];
          live = pa >= eps32 && pa <= 1.0f - eps32;   // the clamp's gradient: 0 where it binds
        }
        float dot = 0.f;
        if (a.d_probs && p < R)
          for (int j = 0; j < n; ++j) dot += D[off + j] * L[off + j];
        for (int j = 0; j < n; ++j) {
          const float pj = L[off + j];
          const float t1 = live ? up * ((j == act ? 1.0f : 0.0f) - pj) : 0.f;   // a group of one action: 1 - exp(0) / 1 = 0
          const float t2 = a.d_probs && p < R ? pj * (D[off + j] - dot) : 0.f;
          const float dl = t1 + t2;
          L[off + j] = dl;
          unsigned hi16, lo16;
          mt_split(dl, 0.f, hi16, lo16);
          dlb[r * PE_QS + off + j] = (atp_h)(hi16 & 0xffffu);
          dlt[(off + j) * TS + r] = (atp_h)(hi16 & 0xffffu);
          if constexpr (SP) {
            dlbl[r * PE_QS + off + j] = (atp_h)(lo16 & 0xffffu);
            dltl[(off + j) * TS + r] = (atp_h)(lo16 & 0xffffu);
          }
        }
      }
      for (int c = N + q; c < 32; c += PH_WAVES) {   // the padding of the actor's rows
        L[c] = 0.f;
        dlb[r * PE_QS + c] = 0;
        dlt[c * TS + r] = 0;
        if constexpr (SP) {
          dlbl[r * PE_QS + c] = 0;
          dltl[c * TS + r] = 0;
        }
      }
      if (clamped && a.f.status) atomicOr(a.f.status, 1);
    }

    // ---- phase B2: the critic's backward on the lanes that hold its hidden layer
    float dv[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int p = row0 + 16 * s + lr;
      dv[s] = p < R ? a.d_value[p] : 0.f;
    }
    atp_f4 xh[S];
    float* part2 = part + PH_WAVES * PH_ROWS;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      xh[s] = (y[0][s] - mean[s]) * rstd[s];
      float s1 = 0.f, s2 = 0.f;
      if (critic) { s1 = atp_sum4(c4); s2 = atp_sum4(c4 * xh[s]); }
      s1 = atp_row_sum(s1); s2 = atp_row_sum(s2);
      if (lq == 0) { part[wave * PH_ROWS + 16 * s + lr] = s1; part2[wave * PH_ROWS + 16 * s + lr] = s2; }
    }
    __syncthreads();   // (dl is complete too)
    if (critic) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const float m1 = mt_wave_sum4(part + 16 * s + lr, PH_ROWS) * (1.0f / H), m2 = mt_wave_sum4(part2 + 16 * s + lr, PH_ROWS) * (1.0f / H);
        const atp_f4 u = rstd[s] * ((c4 - m1) - xh[s] * m2);
        const atp_f4 d = mt_leaky_grad4(dv[s] * u, pos >> (4 * s), a.f.slope);
        db1 += d;
        dlnw += dv[s] * (w24 * xh[s]);
        dlnb += dv[s] * w24;
        dw2 += dv[s] * (xh[s] * lnw4 + lnb4);
        const int r = 16 * s + lr;
        unsigned lo, hi, llo, lhi;
        mt_split(d.x, d.y, lo, llo);
        mt_split(d.z, d.w, hi, lhi);
        mt_st_both<TS>(dhb + r * HS + 16 * wave + 4 * lq, dht + (16 * wave + 4 * lq) * TS, r, lo, hi);
        if constexpr (SP) mt_st_both<TS>(dhbl + r * HS + 16 * wave + 4 * lq, dhtl + (16 * wave + 4 * lq) * TS, r, llo, lhi);
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) db2 += dv[s];
    if (tid < 32)
      for (int r = 0; r < PH_ROWS; ++r) dab += lg[r * PH_LS + tid];   // d_actor_b in row order
    __syncthreads();

    // ---- phase B3: d_features, stored once
#pragma unroll
    for (int j = 0; j < OPW; ++j) {
      const int kt = wave + PH_WAVES * j;
      const arr_u4 wa = atp_ld16(a.actor_wt + (size_t)(16 * kt + lr) * 32 + 8 * lq);
      arr_u4 wal = wa, w1f[HKS], w1l[HKS];
      if constexpr (SP) wal = atp_ld16(a.actor_wtl + (size_t)(16 * kt + lr) * 32 + 8 * lq);
#pragma unroll
      for (int ks = 0; ks < HKS; ++ks) {
        w1f[ks] = atp_ld16(a.w1t + (size_t)(16 * kt + lr) * H + 32 * ks + 8 * lq);
        w1l[ks] = w1f[ks];
        if constexpr (SP) w1l[ks] = atp_ld16(a.w1tl + (size_t)(16 * kt + lr) * H + 32 * ks + 8 * lq);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int at = (16 * s + lr) * PE_QS + 8 * lq;
        atp_f4 acc = mt_mma_split<SP>(wa, wal, atp_ld16(dlb + at), atp_ld16(dlbl + LO * at), zero4);
#pragma unroll
        for (int ks = 0; ks < HKS; ++ks) {
          const int ah = (16 * s + lr) * HS + 32 * ks + 8 * lq;
          acc = mt_mma_split<SP>(w1f[ks], w1l[ks], atp_ld16(dhb + ah), atp_ld16(dhbl + LO * ah), acc);
        }
        const int p = row0 + 16 * s + lr;
        if (a.dfeat && p < R) *reinterpret_cast<atp_f4*>(a.dfeat + (size_t)p * K + 16 * kt + 4 * lq) = acc + zero4;   // (+ 0: no -0 leaves)
      }
    }
    // ---- phase B4: d_actor_w += dl^T x (D[k][logit]), d_critic_w1 += dh_pre^T x (D[k][hidden])
#pragma unroll
    for (int ks = 0; ks < RKS; ++ks) {
      arr_u4 xf[OPW], xl[OPW];
#pragma unroll
      for (int j = 0; j < OPW; ++j) {
        const int at = (16 * (wave + PH_WAVES * j) + lr) * TS + 32 * ks + 8 * lq;
        xf[j] = atp_ld16(xt + at);
        xl[j] = atp_ld16(xtl + LO * at);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int at = (16 * h + lr) * TS + 32 * ks + 8 * lq;
        const arr_u4 df = atp_ld16(dlt + at), dl2 = atp_ld16(dltl + LO * at);
#pragma unroll
        for (int j = 0; j < OPW; ++j) gA[j][h] = mt_mma_split<SP>(xf[j], xl[j], df, dl2, gA[j][h]);
      }
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int at = (16 * c + lr) * TS + 32 * ks + 8 * lq;
        const arr_u4 df = atp_ld16(dht + at), dh2 = atp_ld16(dhtl + LO * at);
#pragma unroll
        for (int j = 0; j < OPW; ++j) gC[j][c] = mt_mma_split<SP>(xf[j], xl[j], df, dh2, gC[j][c]);
      }
    }
    __syncthreads();   // the next block's phase 0 overwrites the tiles
  }

  // ---- this workgroup's slice: every element stored once
  float* out = a.part + (size_t)blockIdx.x * pe_part(K);
#pragma unroll
  for (int j = 0; j < OPW; ++j) {
    const int kt = wave + PH_WAVES * j;
#pragma unroll
    for (int h = 0; h < 2; ++h) *reinterpret_cast<atp_f4*>(out + pe_off_aw(K) + (16 * h + lr) * K + 16 * kt + 4 * lq) = gA[j][h];
#pragma unroll
    for (int c = 0; c < CT; ++c) *reinterpret_cast<atp_f4*>(out + pe_off_w1(K) + (16 * c + lr) * K + 16 * kt + 4 * lq) = gC[j][c];
  }
  {
    const atp_f4 s1 = mt_sum16(db1), s2 = mt_sum16(dlnw), s3 = mt_sum16(dlnb), s4 = mt_sum16(dw2);
    if (critic && lr == 0) {
      *reinterpret_cast<atp_f4*>(out + pe_off_b1(K) + 16 * wave + 4 * lq) = s1;
      *reinterpret_cast<atp_f4*>(out + pe_off_lnw(K) + 16 * wave + 4 * lq) = s2;
      *reinterpret_cast<atp_f4*>(out + pe_off_lnb(K) + 16 * wave + 4 * lq) = s3;
      *reinterpret_cast<atp_f4*>(out + pe_off_w2(K) + 16 * wave + 4 * lq) = s4;
    }
    const float v = mt_sum16(db2);
    if (tid < 4) out[pe_off_b2(K) + tid] = tid == 0 ? v : 0.f;
  }
  if (tid < 32) out[pe_off_ab(K) + tid] = dab;
}

#define PE_BWD_KERNEL(NAME, K, CV) \
  extern "C" __global__ void __launch_bounds__(PH_BLOCK) NAME(PeArgs a) { pe_bwd_body<K, CV>(a); }
PE_BWD_KERNEL(pe_bwd_64_bf16_kernel, 64, ArrBf16)
PE_BWD_KERNEL(pe_bwd_64_f16_kernel, 64, ArrF16)
PE_BWD_KERNEL(pe_bwd_128_bf16_kernel, 128, ArrBf16)
PE_BWD_KERNEL(pe_bwd_128_f16_kernel, 128, ArrF16)

#define PE_FWD_KERNEL(NAME, K, CV) \
  extern "C" __global__ void __launch_bounds__(PH_BLOCK) NAME(PhArgs a) { ph_body<K, CV, true>(a); }
PE_FWD_KERNEL(pe_fwd_64_bf16_kernel, 64, ArrBf16)
PE_FWD_KERNEL(pe_fwd_64_f16_kernel, 64, ArrF16)
PE_FWD_KERNEL(pe_fwd_128_bf16_kernel, 128, ArrBf16)
PE_FWD_KERNEL(pe_fwd_128_f16_kernel, 128, ArrF16)

// The second launch: element i of the slices added in workgroup order into its place in dynenv_policy_grad_t.
struct PeGrad { float *aw, *w1, *ab, *b1, *lnw, *lnb, *w2, *b2; };
extern "C" __global__ void __launch_bounds__(PE_RED_BLOCK) pe_bwd_reduce_kernel(const float* __restrict__ part, int slices, int K, PeGrad o) {
  const int i = (int)(blockIdx.x * PE_RED_BLOCK + threadIdx.x), n = pe_part(K);
  if (i >= n) return;
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < slices; ++b) s += part[(size_t)b * n + i];
  s += 0.f;   // (no -0 leaves)
  if (i < pe_off_w1(K)) o.aw[i] = s;
  else if (i < pe_off_ab(K)) o.w1[i - pe_off_w1(K)] = s;
  else if (i < pe_off_b1(K)) o.ab[i - pe_off_ab(K)] = s;
  else if (i < pe_off_lnw(K)) o.b1[i - pe_off_b1(K)] = s;
  else if (i < pe_off_lnb(K)) o.lnw[i - pe_off_lnw(K)] = s;
  else if (i < pe_off_w2(K)) o.lnb[i - pe_off_lnb(K)] = s;
  else if (i < pe_off_b2(K)) o.w2[i - pe_off_w2(K)] = s;
  else if (i == pe_off_b2(K)) o.b2[0] = s;
}

// ---- the entry points.  Argument errors first, then what the kernels do not take, both before a device is looked for.
static int pe_groups(int64_t rows) {
  const int64_t blocks = (rows + PH_ROWS - 1) / PH_ROWS;
  return (int)(blocks < PE_MAX_GRID ? blocks : PE_MAX_GRID);
}

// what the three entry points check alike -> 0, or the error; fills the forward's arguments
static int pe_common(const char* who, const float* features_dev, const float* actions_dev, int32_t T, int32_t P, int32_t K, int32_t w_dtype,
                     const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t action_cols, float slope, float ln_eps, int32_t* status_dev, PhArgs& k) {
  auto say = [&](int rc, const char* what) { return fail(rc, std::string(who) + ": " + what); };
  if (!features_dev || !actions_dev || !w || !nvec) return say(DYNENV_ERR_ARG, "null argument");
  if (!w->actor_w || !w->actor_b || !w->critic_w1 || !w->critic_b1 || !w->critic_ln_w || !w->critic_ln_b || !w->critic_w2 || !w->critic_b2)
    return say(DYNENV_ERR_ARG, "the actor and the critic have all eight of their pointers");
  if (T < 1 || P < 1 || K < 1) return say(DYNENV_ERR_ARG, "bad shape");
  if (G < 1 || G > DYNENV_POLICY_MAX_GROUPS) return say(DYNENV_ERR_ARG, "G is 1..8");
  ModelGroups gr;
  if (int rc = model_groups(who, nvec, G, action_cols, gr)) return rc;
  if (int rc = model_operand_dtype(who, w_dtype)) return rc;
  if (int rc = model_aligned(who, {features_dev, actions_dev, w->actor_w, w->actor_b, w->critic_w1, w->critic_b1, w->critic_ln_w, w->critic_ln_b, w->critic_w2}, 16))
    return rc;
  if ((uintptr_t)w->critic_b2 % 4 || (uintptr_t)status_dev % 4) return say(DYNENV_ERR_ARG, "critic_b2 and status_dev are 4-byte aligned");
  if ((int64_t)T * P > (int64_t)1 << 30) return say(DYNENV_ERR_ARG, "T * P too large for one launch");
  k = PhArgs{};
  k.feat0 = features_dev; k.feat1 = nullptr;
  k.actor_w = static_cast<const atp_h*>(w->actor_w); k.w1 = static_cast<const atp_h*>(w->critic_w1);
  k.actor_b = w->actor_b; k.b1 = w->critic_b1; k.ln_w = w->critic_ln_w; k.ln_b = w->critic_ln_b; k.w2 = w->critic_w2; k.b2 = w->critic_b2;
  k.group_off = gr.off; k.group_n = gr.n;
  k.P = T * P; k.G = G; k.N = gr.N; k.C = 0; k.AD = action_cols;
  k.slope = slope; k.eps = ln_eps;
  k.ev_actions = actions_dev; k.ev_P = P; k.status = status_dev;
  return 0;
}

extern "C" int dynenv_policy_eval(const float* features_dev, const float* actions_dev, int32_t T, int32_t P, int32_t K, int32_t w_dtype,
                                  const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t action_cols, float slope, float ln_eps,
                                  float* logp_dev, float* probs_dev, float* value_dev, int32_t* status_dev, void* stream) {
  PhArgs k;
  if (!logp_dev || !value_dev) return fail(DYNENV_ERR_ARG, "policy eval: null argument");
  if (int rc = pe_common("policy eval", features_dev, actions_dev, T, P, K, w_dtype, w, nvec, G, action_cols, slope, ln_eps, status_dev, k)) return rc;
  if (int rc = model_aligned("policy eval", {logp_dev, probs_dev, value_dev}, 16)) return rc;
  if (int rc = model_operand_16bit("policy eval", w_dtype, "layer")) return rc;
  if (K != 64 && K != 128) return fail(DYNENV_ERR_UNSUPPORTED, "policy eval: the fused layer takes K = 64 or 128");
  if (int rc = have_device()) return rc;
  k.logp = logp_dev; k.probs = probs_dev; k.value = value_dev;
  static decltype(&pe_fwd_64_bf16_kernel) const kernels[2][2] = {{pe_fwd_64_bf16_kernel, pe_fwd_64_f16_kernel}, {pe_fwd_128_bf16_kernel, pe_fwd_128_f16_kernel}};
  hipLaunchKernelGGL(kernels[K == 128][w_dtype == DYNENV_ARR_F16], dim3((unsigned)((k.P + PH_ROWS - 1) / PH_ROWS)), dim3(PH_BLOCK), 0, (hipStream_t)stream, k);
  return launched();
}

extern "C" int dynenv_policy_eval_backward_workspace(int32_t rows, int32_t K, uint64_t* bytes) {
  if (!bytes) return fail(DYNENV_ERR_ARG, "policy eval backward workspace: null argument");
  if (rows < 1 || K < 1) return fail(DYNENV_ERR_ARG, "policy eval backward workspace: bad shape");
  if (rows > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "policy eval backward workspace: more than 2^30 rows");
  if (K != 64 && K != 128) return fail(DYNENV_ERR_UNSUPPORTED, "policy eval backward workspace: the fused backward takes K = 64 or 128");
  *bytes = (uint64_t)pe_groups(rows) * (uint64_t)pe_part(K) * 4u;
  return DYNENV_OK;
}

extern "C" int dynenv_policy_eval_backward(const float* features_dev, const float* actions_dev, int32_t T, int32_t P, int32_t K, int32_t w_dtype,
                                           const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t action_cols, float slope, float ln_eps,
                                           const float* d_logp_dev, const float* d_probs_dev, const float* d_value_dev, const dynenv_policy_bwd_t* wt,
                                           const dynenv_policy_grad_t* grad, float* d_features_dev, void* workspace_dev, uint64_t workspace_bytes,
                                           int32_t* status_dev, void* stream) {
  PeArgs k;
  if (!d_logp_dev || !d_value_dev || !wt || !grad || !workspace_dev) return fail(DYNENV_ERR_ARG, "policy eval backward: null argument");
  if (int rc = pe_common("policy eval backward", features_dev, actions_dev, T, P, K, w_dtype, w, nvec, G, action_cols, slope, ln_eps, status_dev, k.f)) return rc;
  if (!wt->actor_w_t || !wt->critic_w1_t) return fail(DYNENV_ERR_ARG, "policy eval backward: the two transposed copies have their pointers");
  if (w_dtype == DYNENV_ARR_F16 && (!wt->actor_w_t_lo || !wt->critic_w1_t_lo))
    return fail(DYNENV_ERR_ARG, "policy eval backward: float16 takes the second halves of the two transposed copies");
  if (!grad->d_actor_w || !grad->d_actor_b || !grad->d_critic_w1 || !grad->d_critic_b1 || !grad->d_critic_ln_w || !grad->d_critic_ln_b || !grad->d_critic_w2 ||
      !grad->d_critic_b2)
    return fail(DYNENV_ERR_ARG, "policy eval backward: the eight gradients have their pointers");
  if (int rc = model_aligned("policy eval backward", {d_logp_dev, d_probs_dev, d_value_dev, d_features_dev, workspace_dev, wt->actor_w_t, wt->critic_w1_t,
                                                      wt->actor_w_t_lo, wt->critic_w1_t_lo, grad->d_actor_w, grad->d_actor_b, grad->d_critic_w1,
                                                      grad->d_critic_b1, grad->d_critic_ln_w, grad->d_critic_ln_b, grad->d_critic_w2}, 16))
    return rc;
  if ((uintptr_t)grad->d_critic_b2 % 4) return fail(DYNENV_ERR_ARG, "policy eval backward: d_critic_b2 is 4-byte aligned");
  const int groups = pe_groups((int64_t)T * P);
  if ((K == 64 || K == 128) && workspace_bytes < (uint64_t)groups * (uint64_t)pe_part(K) * 4u)
    return fail(DYNENV_ERR_ARG, "policy eval backward: the workspace is smaller than dynenv_policy_eval_backward_workspace asks for");
  if (int rc = model_operand_16bit("policy eval backward", w_dtype, "backward")) return rc;
  if (K != 64 && K != 128) return fail(DYNENV_ERR_UNSUPPORTED, "policy eval backward: the fused backward takes K = 64 or 128");
  if (int rc = have_device()) return rc;
  k.d_logp = d_logp_dev; k.d_probs = d_probs_dev; k.d_value = d_value_dev;
  k.actor_wt = static_cast<const atp_h*>(wt->actor_w_t); k.w1t = static_cast<const atp_h*>(wt->critic_w1_t);
  k.actor_wtl = static_cast<const atp_h*>(wt->actor_w_t_lo); k.w1tl = static_cast<const atp_h*>(wt->critic_w1_t_lo);
  k.dfeat = d_features_dev; k.part = static_cast<float*>(workspace_dev);
  k.nblocks = (k.f.P + PH_ROWS - 1) / PH_ROWS;
  static decltype(&pe_bwd_64_bf16_kernel) const kernels[2][2] = {{pe_bwd_64_bf16_kernel, pe_bwd_64_f16_kernel}, {pe_bwd_128_bf16_kernel, pe_bwd_128_f16_kernel}};
  hipLaunchKernelGGL(kernels[K == 128][w_dtype == DYNENV_ARR_F16], dim3((unsigned)groups), dim3(PH_BLOCK), 0, (hipStream_t)stream, k);
  PeGrad o = {grad->d_actor_w, grad->d_critic_w1, grad->d_actor_b, grad->d_critic_b1, grad->d_critic_ln_w, grad->d_critic_ln_b, grad->d_critic_w2, grad->d_critic_b2};
  hipLaunchKernelGGL(pe_bwd_reduce_kernel, dim3((unsigned)((pe_part(K) + PE_RED_BLOCK - 1) / PE_RED_BLOCK)), dim3(PE_RED_BLOCK), 0, (hipStream_t)stream,
                     (const float*)workspace_dev, groups, (int)K, o);
  return launched();
}
