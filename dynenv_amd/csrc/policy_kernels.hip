// policy_kernels.hip — the reference's policy head in one launch where no gradient is wanted: ActorLayer and CriticLayer
// (DynEnv/models/actor_critic.py:161-242) on cat(features[0:2]) (actor_critic.py:88, never materialised), the softmax and the draw of
// _calc_log_probs per discrete action group (actor_critic.py:125-140), and transformActions (DynEnv/utils/utils.py:20-39) of the drawn
// actions (include/dynenv.h, dynenv_policy_head).  The logits never exist in memory.  Included at the very END of dynenv_capi.hip,
// behind recurrent_kernels.hip: no kernel a step launches moves.  This file also holds the entry point's host code.
//
// Per row p:
//   l = cat(feat0, feat1) W_actor^T + b            (32 rows: the N logits of the G groups, the C outputs of the Box block, +0)
//   probs_g = softmax(l_g);  cont = (sigmoid(l) - 0.5) * scale + mean
//   value = LayerNorm(leaky(cat W1^T + b1)) . w2 + b2
//   u_g from Philox4x32-10 keyed by (seed; row_base + p, draw, purpose + g / 4);  action_g = #{j < n_g - 1: c_j <= u_g c_{n-1}}
//
// Work.  One workgroup of four waves per PH_ROWS = 64 rows = four strips of 16, recurrent_kernels.hip's shape, on the tile toolkit
// (mma_tiles.h; DESIGN.md, "The tile toolkit"): a lane's accumulator holds four consecutive outputs of one row.  The
// output tiles of 16 - K / 32 of the critic's Layer1, then the two of the actor - are dealt to the waves round robin (tile = wave +
// 4 t); a wave computes its tiles for ALL FOUR strips, so every weight fragment it fetches (16 contiguous bytes per lane, from L2)
// feeds four MFMAs and the workgroup streams the weights once per 64 rows.  The B operands come from the 64 rows in LDS, 16 bit wide.
//   phase 0: cat(feat0, feat1) rounded into LDS row-major
//   phase 1: the products; the actor's 32 outputs of every row into LDS (float32); the critic's LayerNorm and its dot product with
//            Layer2.weight, the four waves' parts of every row's sums added in wave order
//   phase 2: thread (row r, wave q) takes the groups g = q, q + 4 of row r: softmax in place in LDS, the cumulative sum, the draw,
//            log_prob; and the Box output c = q
//   phase 3: probs, actions and next_ext leave LDS as contiguous pieces of the 64 rows
// Every sum has one fixed order and an MFMA's columns do not mix: a row's result depends on the row, the weights and its stream alone.
// Rows at or behind P in the last workgroup are +0.0 in LDS and are never stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "dynenv_math.h"
#include "mma_tiles.h"

#define PH_BLOCK 256
#define PH_WAVES (PH_BLOCK / 64)
#define PH_STRIPS 4
#define PH_ROWS (16 * PH_STRIPS)
#define PH_LS 33   // floats per LDS row of the 32 actor outputs: a lane per row reads without bank conflicts

struct PhArgs {   // dynenv_policy_t by value, the outputs and the sizes
  const float *feat0, *feat1;
  const atp_h *actor_w, *w1;
  const float *actor_b, *cont_scale, *cont_mean, *b1, *ln_w, *ln_b, *w2, *b2;
  const unsigned long long* draw;
  unsigned long long seed, row_base;
  unsigned long long group_off;   // 8 bits per group: the first logit of group g
  unsigned group_n;               // 4 bits per group: n_g - 1
  int P, G, N, C, AD, discrete_turn;
  float slope, eps;
  int* actions;
  double* cont;
  float *probs, *logp, *value, *next_ext;
  // dynenv_policy_eval (policy_eval_kernels.hip): the stored actions [T][AD][ev_P] stand where the draw stood, P = T * ev_P rows
  const float* ev_actions;
  int ev_P;
  int* status;
};

#define PH_TS (PH_ROWS + 8)   // elements per LDS row of the transposed copy of the 64 rows: 16 bytes of padding
template <int K> struct PhShape {   // critic tiles, all tiles, tiles per wave, k steps; elements per LDS row: 16 bytes of padding
  static constexpr int H = K / 2, CT = H / 16, T = CT + 2, TPW = (T + PH_WAVES - 1) / PH_WAVES, KS = K / 32, XS = K + 8;
};

// Phases 0 and 1 of the rows row0 .. row0 + 63: what dynenv_policy_head, dynenv_policy_eval and the recomputation of
// dynenv_policy_eval_backward share, so that the three give a row the same bits.  Leaves the logits in lg, the critic's hidden layer
// behind its LeakyReLU in y (the tiles wave + 4 t below CT), its LayerNorm's mean and 1 / std per strip, and the four waves' parts of
// every row's dot product with Layer2.weight in part + 2 * PH_WAVES * PH_ROWS, behind a barrier.  With TR the rows also go into xt,
// transposed and rounded to bf16 (the operand of the weight gradients; xtl, unless NULL, takes the bf16 rounding of what that rounding
// left), and bit 4 (t PH_STRIPS + s) + i of pos says h_pre > 0.
template <int K, class CV, bool TR>
__device__ __forceinline__ void ph_forward(const PhArgs& a, int row0, atp_h* xb, atp_h* xt, atp_h* xtl, float* lg, float* part,
                                           atp_f4 (&y)[PhShape<K>::TPW][PH_STRIPS], float (&mean)[PH_STRIPS], float (&rstd)[PH_STRIPS], unsigned& pos) {
  constexpr int H = PhShape<K>::H, CT = PhShape<K>::CT, T = PhShape<K>::T, TPW = PhShape<K>::TPW, KS = PhShape<K>::KS, XS = PhShape<K>::XS;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int P = a.P;
  const int F = a.feat1 ? H : K;
  const atp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- phase 0: cat(feat0, feat1), rounded, into LDS
  for (int i = tid; i < PH_ROWS * (K / 4); i += PH_BLOCK) {
    const int r = i / (K / 4), col = 4 * (i % (K / 4)), p = row0 + r;
    atp_f4 v = zero4;
    if (p < P) v = col < F ? mt_ldf4(a.feat0 + (size_t)p * F + col) : mt_ldf4(a.feat1 + (size_t)p * F + (col - F));
    atp_st4<CV>(xb + r * XS + col, v);
    if constexpr (TR) {
      const unsigned lo = ArrBf16::pack(v.x, v.y), hi = ArrBf16::pack(v.z, v.w);
      mt_st_tr<PH_TS>(xt + col * PH_TS + r, lo, hi);
      if (xtl) {   // what the rounding to bf16 left, rounded to bf16: xt + xtl holds 16 significant bits of the row (mt_split's arithmetic,
                   // written out: with two calls of it the float16 backward kernels are scheduled differently)
        const arr_f2 w0 = ArrBf16::widen(lo), w1 = ArrBf16::widen(hi);
        const unsigned l0 = ArrBf16::pack(v.x - w0.x, v.y - w0.y), l1 = ArrBf16::pack(v.z - w1.x, v.w - w1.y);
        mt_st_tr<PH_TS>(xtl + col * PH_TS + r, l0, l1);
      }
    }
  }
  __syncthreads();

  // ---- phase 1: this wave's tiles for all 64 rows
  const atp_h* wrow[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wave + PH_WAVES * t;
    atp_f4 b = zero4;
    wrow[t] = a.w1;
    if (tile < CT) {
      b = mt_ldf4(a.b1 + 16 * tile + 4 * lq);
      wrow[t] = a.w1 + (size_t)(16 * tile + lr) * K;
    } else if (tile < T) {
      b = mt_ldf4(a.actor_b + 16 * (tile - CT) + 4 * lq);
      wrow[t] = a.actor_w + (size_t)(16 * (tile - CT) + lr) * K;
    }
#pragma unroll
    for (int s = 0; s < PH_STRIPS; ++s) y[t][s] = b;
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    arr_u4 xf[PH_STRIPS];
#pragma unroll
    for (int s = 0; s < PH_STRIPS; ++s) xf[s] = atp_ld16(xb + (16 * s + lr) * XS + 32 * ks + 8 * lq);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
      if (wave + PH_WAVES * t < T) {
        const arr_u4 w = atp_ld16(wrow[t] + 32 * ks + 8 * lq);
#pragma unroll
        for (int s = 0; s < PH_STRIPS; ++s) y[t][s] = AtpMma<CV>::mma(w, xf[s], y[t][s]);
      }
  }
  // the actor's outputs into LDS; the critic's LeakyReLU
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wave + PH_WAVES * t;
    if (tile < CT) {
#pragma unroll
      for (int s = 0; s < PH_STRIPS; ++s) {
        if constexpr (TR) pos |= mt_pos4(y[t][s]) << (4 * (t * PH_STRIPS + s));
        y[t][s] = mt_leaky4(y[t][s], a.slope);
      }
    } else if (tile < T) {
#pragma unroll
      for (int s = 0; s < PH_STRIPS; ++s) mt_st_f4(lg + (16 * s + lr) * PH_LS + 16 * (tile - CT) + 4 * lq, y[t][s]);
    }
  }
  // torch's LayerNorm (biased variance, two passes) over the H critic features of a row, which lie in up to four waves, and the dot
  // product with Layer2.weight: a wave without a critic tile adds +0
#pragma unroll
  for (int s = 0; s < PH_STRIPS; ++s) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
      if (wave + PH_WAVES * t < CT) v += atp_sum4(y[t][s]);
    v = atp_row_sum(v);
    if (lq == 0) part[wave * PH_ROWS + 16 * s + lr] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < PH_STRIPS; ++s) {
    const float* q = part + 16 * s + lr;
    mean[s] = mt_wave_sum4(q, PH_ROWS) * (1.0f / H);
  }
  float* part2 = part + PH_WAVES * PH_ROWS;
#pragma unroll
  for (int s = 0; s < PH_STRIPS; ++s) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
      if (wave + PH_WAVES * t < CT) { const atp_f4 d = y[t][s] - mean[s]; v += atp_sum4(d * d); }
    v = atp_row_sum(v);
    if (lq == 0) part2[wave * PH_ROWS + 16 * s + lr] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < PH_STRIPS; ++s) {
    const float* q = part2 + 16 * s + lr;
    rstd[s] = 1.0f / sqrtf(mt_wave_sum4(q, PH_ROWS) * (1.0f / H) + a.eps);
  }
  float* part3 = part + 2 * PH_WAVES * PH_ROWS;
  {
    float dot[PH_STRIPS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tile = wave + PH_WAVES * t;
      if (tile < CT) {
        const atp_f4 g = mt_ldf4(a.ln_w + 16 * tile + 4 * lq), b = mt_ldf4(a.ln_b + 16 * tile + 4 * lq), w2 = mt_ldf4(a.w2 + 16 * tile + 4 * lq);
#pragma unroll
        for (int s = 0; s < PH_STRIPS; ++s) dot[s] += atp_sum4(((y[t][s] - mean[s]) * rstd[s] * g + b) * w2);
      }
    }
#pragma unroll
    for (int s = 0; s < PH_STRIPS; ++s) {
      const float v = atp_row_sum(dot[s]);
      if (lq == 0) part3[wave * PH_ROWS + 16 * s + lr] = v;
    }
  }
  __syncthreads();   // (the actor's outputs in lg are complete too)
}

// softmax of the n logits at L[off ..], in place -> c_{n-1}: the probabilities added left to right
__device__ __forceinline__ float ph_softmax(float* L, int off, int n) {
  float m = L[off];
  for (int j = 1; j < n; ++j) m = fmaxf(m, L[off + j]);
  float sum = 0.f;
  for (int j = 0; j < n; ++j) {
    const float e = expf(L[off + j] - m);
    L[off + j] = e;
    sum += e;
  }
  float last = 0.f;
  for (int j = 0; j < n; ++j) {
    const float pj = L[off + j] / sum;
    L[off + j] = pj;
    last += pj;
  }
  return last;
}

// the stored action of group g (n_g - 1 = last) for row p = t ev_P + pp
__device__ __forceinline__ int ph_stored_action(const PhArgs& a, int p, int g, int last, bool& clamped) {
  const int t = p / a.ev_P, pp = p - t * a.ev_P;
  return mt_stored_action(a.ev_actions[((size_t)t * a.AD + g) * a.ev_P + pp], last, clamped);
}

// EVAL: dynenv_policy_eval - the stored action in place of the draw, log_probs in the storage's layout [T][G][ev_P], probs optional,
// no actions, cont or next_ext.
template <int K, class CV, bool EVAL>
__device__ __forceinline__ void ph_body(const PhArgs& a) {
  constexpr int TPW = PhShape<K>::TPW, XS = PhShape<K>::XS;
  __shared__ __attribute__((aligned(16))) atp_h xb[PH_ROWS * XS];
  __shared__ float lg[PH_ROWS * PH_LS];
  __shared__ float part[3 * PH_WAVES * PH_ROWS];
  __shared__ int acts[PH_ROWS * 8];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = (int)blockIdx.x * PH_ROWS, P = a.P;
  atp_f4 y[TPW][PH_STRIPS];
  float mean[PH_STRIPS], rstd[PH_STRIPS];
  unsigned pos = 0;
  ph_forward<K, CV, false>(a, row0, xb, nullptr, nullptr, lg, part, y, mean, rstd, pos);
  if (tid < PH_ROWS && row0 + tid < P) {
    const float* q = part + 2 * PH_WAVES * PH_ROWS + tid;
    a.value[row0 + tid] = mt_wave_sum4(q, PH_ROWS) + a.b2[0];
  }

  // ---- phase 2: row r's groups g = q, q + 4 and its Box output c = q, by thread (r, q); q is the wave, so a group's size is uniform
  {
    const int r = lane, q = wave, p = row0 + r;
    float* L = lg + r * PH_LS;
    const unsigned long long draw = !EVAL && a.draw ? a.draw[0] : 0ull, row = a.row_base + (unsigned long long)p;
    bool clamped = false;
    for (int g = q; g < a.G; g += PH_WAVES) {
      const MtGroup gr = mt_group(a.group_off, a.group_n, g);
      const int off = gr.off, n = gr.n;
      const float last = ph_softmax(L, off, n);   // c_{n-1}
      int act = 0;
      if constexpr (EVAL) {
        if (p < P) act = ph_stored_action(a, p, g, n - 1, clamped);
      } else {
        const dm_u32x4 w = dm_philox((uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)row, (uint32_t)draw, (uint32_t)(draw >> 32),
                                     DYNENV_POLICY_RNG_PURPOSE + (uint32_t)(g >> 2));
        const uint32_t word = q == 0 ? w.v[0] : q == 1 ? w.v[1] : q == 2 ? w.v[2] : w.v[3];
        const float u = (float)(word >> 8) * 5.9604644775390625e-08f;   // 2^-24: exact
        const float t = u * last;
        float c = 0.f;
        for (int j = 0; j + 1 < n; ++j) {
          c += L[off + j];
          act += c <= t ? 1 : 0;
        }
        acts[r * 8 + g] = act;
      }
      if (p < P) {
        const float eps32 = 1.1920928955078125e-07f;
        const float pa = fminf(fmaxf(L[off + act], eps32), 1.0f - eps32);
        size_t at = (size_t)p * a.G + g;
        if constexpr (EVAL) {
          const int t = p / a.ev_P;
          at = ((size_t)t * a.G + g) * a.ev_P + (p - t * a.ev_P);
        }
        a.logp[at] = (float)log((double)pa);   // the float32 nearest to the logarithm: a host reproduces it bit for bit
      }
    }
    if (EVAL && clamped && a.status) atomicOr(a.status, 1);
    if (!EVAL && q < a.C && p < P) {
      const float v = (mt_sigmoid(L[a.N + q]) - 0.5f) * a.cont_scale[q] + a.cont_mean[q];
      a.cont[(size_t)p * a.C + q] = (double)v;
    }
  }
  __syncthreads();

  // ---- phase 3: the 64 rows' probs, actions and next_ext are contiguous in memory
  const int rows = min(PH_ROWS, P - row0);
  if (!EVAL || a.probs)
    for (int i = tid; i < rows * a.N; i += PH_BLOCK) a.probs[(size_t)row0 * a.N + i] = lg[(i / a.N) * PH_LS + i % a.N];
  if (EVAL) return;
  const int AD = a.AD;
  for (int i = tid; i < rows * AD; i += PH_BLOCK) {
    const int r = i / AD, k = i % AD;
    const int v = k < a.G ? acts[r * 8 + k] : 0;
    a.actions[(size_t)row0 * AD + i] = v;
    if (a.next_ext) {   // utils.py:20-39, as its in-place assignments run
      int e = v;
      if (AD == 4) {
        const int a0 = acts[r * 8];
        if (k == 0) e = v < 3 ? 0 : v == 3 ? 1 : v == 4 ? -1 : v;
        else if (k == 1) e = v == 2 ? -1 : v;
        else if (k == 2) e = (a0 == 1 || a0 == 2) ? -1 : 0;   // sides: 2 -> 1, then every 1 -> -1
        else if (a.discrete_turn) e = v - 3;
      } else if (k < 2) {
        e = v - 1;
      }
      a.next_ext[(size_t)row0 * AD + i] = (float)e;
    }
  }
}

#define PH_KERNEL(NAME, K, CV) \
  extern "C" __global__ void __launch_bounds__(PH_BLOCK) NAME(PhArgs a) { ph_body<K, CV, false>(a); }
PH_KERNEL(ph_64_bf16_kernel, 64, ArrBf16)
PH_KERNEL(ph_64_f16_kernel, 64, ArrF16)
PH_KERNEL(ph_128_bf16_kernel, 128, ArrBf16)
PH_KERNEL(ph_128_f16_kernel, 128, ArrF16)
PH_KERNEL(ph_256_bf16_kernel, 256, ArrBf16)
PH_KERNEL(ph_256_f16_kernel, 256, ArrF16)

// ---- the entry point.  Argument errors first, then what the kernel does not take, both before a device is looked for; one launch and
// nothing else: nothing is synchronised, allocated or copied, so the call may be captured.
extern "C" int dynenv_policy_head(const float* feat0_dev, const float* feat1_dev, int32_t E, int32_t A, int32_t F, int32_t w_dtype,
                                  const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t C, int32_t action_cols, uint64_t seed,
                                  const uint64_t* draw_dev, uint64_t row_base, float slope, float ln_eps, int32_t discrete_turn,
                                  int32_t* actions_dev, double* cont_dev, float* probs_dev, float* logp_dev, float* value_dev,
                                  float* next_ext_dev, void* stream) {
  if (!feat0_dev || !w || !nvec || !actions_dev || !probs_dev || !logp_dev || !value_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (!w->actor_w || !w->actor_b || !w->critic_w1 || !w->critic_b1 || !w->critic_ln_w || !w->critic_ln_b || !w->critic_w2 || !w->critic_b2)
    return fail(DYNENV_ERR_ARG, "policy head: the actor and the critic have all eight of their pointers");
  if (E < 1 || A < 1 || F < 1) return fail(DYNENV_ERR_ARG, "policy head: bad shape");
  if (G < 1 || G > DYNENV_POLICY_MAX_GROUPS || C < 0 || C > DYNENV_POLICY_MAX_CONT) return fail(DYNENV_ERR_ARG, "policy head: G is 1..8 and C 0..4");
  ModelGroups gr;
  if (int rc = model_groups("policy head", nvec, G, action_cols, gr, C)) return rc;
  if ((C > 0) != (cont_dev != nullptr)) return fail(DYNENV_ERR_ARG, "policy head: cont_dev is NULL exactly when C == 0");
  if (C > 0 && (!w->cont_scale || !w->cont_mean)) return fail(DYNENV_ERR_ARG, "policy head: C > 0 takes cont_scale and cont_mean");
  if (int rc = model_operand_dtype("policy head", w_dtype)) return rc;
  if (int rc = model_aligned("policy head", {feat0_dev, feat1_dev, w->actor_w, w->actor_b, w->critic_w1, w->critic_b1, w->critic_ln_w, w->critic_ln_b,
                                             w->critic_w2, actions_dev, cont_dev, probs_dev, logp_dev, value_dev, next_ext_dev}, 16))
    return rc;
  if ((uintptr_t)w->critic_b2 % 4 || (uintptr_t)w->cont_scale % 4 || (uintptr_t)w->cont_mean % 4 || (uintptr_t)draw_dev % 8)
    return fail(DYNENV_ERR_ARG, "policy head: critic_b2, cont_scale and cont_mean are 4-byte, draw_dev 8-byte aligned");
  if ((int64_t)E * A > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "policy head: E * A too large for one launch");
  if (int rc = model_operand_16bit("policy head", w_dtype, "layer")) return rc;
  if (F != 64 && F != 128) return fail(DYNENV_ERR_UNSUPPORTED, "policy head: the fused layer takes F = 64 or 128");
  if (int rc = have_device()) return rc;
  PhArgs k;
  k.feat0 = feat0_dev; k.feat1 = feat1_dev;
  k.actor_w = static_cast<const atp_h*>(w->actor_w); k.w1 = static_cast<const atp_h*>(w->critic_w1);
  k.actor_b = w->actor_b; k.cont_scale = w->cont_scale; k.cont_mean = w->cont_mean; k.b1 = w->critic_b1; k.ln_w = w->critic_ln_w;
  k.ln_b = w->critic_ln_b; k.w2 = w->critic_w2; k.b2 = w->critic_b2;
  k.draw = reinterpret_cast<const unsigned long long*>(draw_dev); k.seed = seed; k.row_base = row_base; k.group_off = gr.off; k.group_n = gr.n;
  k.P = E * A; k.G = G; k.N = gr.N; k.C = C; k.AD = action_cols; k.discrete_turn = discrete_turn != 0;
  k.slope = slope; k.eps = ln_eps;
  k.actions = actions_dev; k.cont = cont_dev; k.probs = probs_dev; k.logp = logp_dev; k.value = value_dev; k.next_ext = next_ext_dev;
  k.ev_actions = nullptr; k.ev_P = 0; k.status = nullptr;
  static decltype(&ph_64_bf16_kernel) const kernels[3][2] = {{ph_64_bf16_kernel, ph_64_f16_kernel}, {ph_128_bf16_kernel, ph_128_f16_kernel},
                                                              {ph_256_bf16_kernel, ph_256_f16_kernel}};
  const int Kc = feat1_dev ? 2 * F : F;
  hipLaunchKernelGGL(kernels[Kc == 64 ? 0 : Kc == 128 ? 1 : 2][w_dtype == DYNENV_ARR_F16], dim3((unsigned)((k.P + PH_ROWS - 1) / PH_ROWS)), dim3(PH_BLOCK), 0,
                     (hipStream_t)stream, k);
  return launched();
}
