// rollout_kernels.hip — the reference's rollout storage behind the policy head (include/dynenv.h, dynenv_rollout_insert and
// dynenv_rollout_returns): RolloutStorage.insert (DynEnv/models/storage.py:134-166, called at DynEnv/models/train.py:277) as ONE launch
// that reads its row from a device cursor, and _discount_rewards (storage.py:168-209) as one launch instead of 2 T + 2.  Included at the
// very END of dynenv_capi.hip, behind policy_kernels.hip: no kernel a step launches moves.  This file also holds the entry points' host code.
//
// The insert.  Workgroups of 256 threads; row t = cursor[0] is read by every thread (one word, the same for all: a scalar load).  Row t
// of the features is P * K / 4 pieces of 16 bytes, and workgroup b copies the CHUNK of RI_CHUNK = 1024 pieces from 1024 b on - a thread
// four of them, 256 apart, all four loads issued before the first store; cat(feat0, feat1) is formed by the choice of the source row and
// never exists in memory (one feature: the source is the same flat piece, no division).  This is nearly all of the launch's bytes.
// Workgroup b also takes the ROW GROUP of the RI_ROWS = 64 players from 64 b on, for everything else of row t:
//   rewards, finished, values:     one thread per player
//   actions, log_probs(_old):      [AD or G][P] - thread i takes (column i / rows, player i % rows): the stores are coalesced, the
//                                  loads stay inside the row group's rows * AD contiguous words
//   probs:                         rows * N contiguous floats
//   dones:                         the environments [64 b, 64 b + 64) below E; E <= P, so every environment has exactly one workgroup
// The grid is the larger of the two counts (with row_features_only: the chunks); a workgroup past the end of either does nothing there.
// Every output element of row t is written exactly once, by one thread; no atomics, no LDS, no scratch.  A cursor outside the admitted
// rows (0..T-1; 0..T with row_features_only) writes nothing but status[0] = 1: a plain store from thread 0 of workgroup 0.
//
// The returns.  One lane owns one player and walks t = T-1 .. 0: at every t the lanes of a wave read and write 64 consecutive floats
// of rewards, values, returns and advantages.  float32 throughout; the build has contraction off, so every multiply and add below
// is rounded on its own, in the order the header states.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dynenv.h"
#include "mma_tiles.h"

#define RI_BLOCK 256
#define RI_ROWS 64
#define RI_PER 4
#define RI_CHUNK (RI_BLOCK * RI_PER)
#define RR_BLOCK 256

struct RiArgs {
  const int* cursor;
  int* status;
  int T, E, P, F, K, G, AD, N, features_only;
  const double* rewards_in;
  const unsigned char *finished_in, *dones_in;
  const float *feat0, *feat1, *logp_in, *logp_old_in, *value_in, *probs_in;
  const int* actions_in;
  float *rewards, *features, *actions, *logp, *logp_old, *values, *dones, *probs;
  unsigned char* finished;
};

extern "C" __global__ void __launch_bounds__(RI_BLOCK) rollout_insert_kernel(RiArgs a) {
  const int tid = (int)threadIdx.x, t = a.cursor[0];
  if (t < 0 || t >= a.T + (a.features_only ? 1 : 0)) {
    if (blockIdx.x == 0 && tid == 0) a.status[0] = 1;
    return;
  }
  const int P = a.P;
  if (a.feat0) {
    // chunk blockIdx.x of row t: RI_CHUNK 16-byte pieces, RI_PER to a thread, all of a thread's loads issued before its first store
    const unsigned K4 = (unsigned)a.K >> 2, F = (unsigned)a.F, total = (unsigned)P * K4;
    atp_f4* dst = reinterpret_cast<atp_f4*>(a.features + (size_t)t * P * a.K);
    const unsigned i0 = blockIdx.x * RI_CHUNK + (unsigned)tid;
    atp_f4 v[RI_PER];
#pragma unroll
    for (int j = 0; j < RI_PER; ++j) {
      const unsigned i = i0 + j * RI_BLOCK;
      if (i < total) {
        if (a.feat1) {
          const unsigned r = i / K4, col = 4 * (i - r * K4);
          v[j] = col < F ? mt_ldf4(a.feat0 + (size_t)r * F + col) : mt_ldf4(a.feat1 + (size_t)r * F + (col - F));
        } else {
          v[j] = mt_ldf4(a.feat0 + 4 * (size_t)i);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < RI_PER; ++j) {
      const unsigned i = i0 + j * RI_BLOCK;
      if (i < total) dst[i] = v[j];
    }
  }
  if (a.features_only) return;
  const int p0 = (int)blockIdx.x * RI_ROWS, rows = min(RI_ROWS, P - p0);
  if (rows <= 0) return;   // (a workgroup that only had a chunk of the features)
  const size_t row = (size_t)t * P + p0;
  if (tid < rows) {
    if (a.rewards_in) a.rewards[row + tid] = (float)a.rewards_in[p0 + tid];   // one rounding to nearest
    if (a.finished_in) a.finished[row + tid] = a.finished_in[p0 + tid] ? 1 : 0;
    if (a.value_in) a.values[row + tid] = a.value_in[p0 + tid];
  }
  if (a.actions_in) {
    const int AD = a.AD;
    for (int i = tid; i < rows * AD; i += RI_BLOCK) {
      const int k = i / rows, r = i - k * rows;
      a.actions[((size_t)t * AD + k) * P + p0 + r] = (float)a.actions_in[(size_t)(p0 + r) * AD + k];
    }
  }
  if (a.logp_in || a.logp_old_in) {
    const int G = a.G;
    for (int i = tid; i < rows * G; i += RI_BLOCK) {
      const int g = i / rows, r = i - g * rows;
      const size_t o = ((size_t)t * G + g) * P + p0 + r, s = (size_t)(p0 + r) * G + g;
      if (a.logp_in) a.logp[o] = a.logp_in[s];
      if (a.logp_old_in) a.logp_old[o] = a.logp_old_in[s];
    }
  }
  if (a.probs_in) {
    const int N = a.N;
    for (int i = tid; i < rows * N; i += RI_BLOCK) a.probs[row * N + i] = a.probs_in[(size_t)p0 * N + i];
  }
  if (a.dones_in && tid < RI_ROWS && p0 + tid < a.E) a.dones[(size_t)t * a.E + p0 + tid] = a.dones_in[p0 + tid] ? 1.0f : 0.0f;
}

struct RrArgs {
  const float *rewards, *values, *dones, *final_value;
  float *returns, *advantages;
  int T, E, A, P, mode;
  float gamma, lambda;
};

extern "C" __global__ void __launch_bounds__(RR_BLOCK) rollout_returns_kernel(RrArgs a) {
  const int p = (int)(blockIdx.x * RR_BLOCK + threadIdx.x), P = a.P;
  if (p >= P) return;
  const int env = p / a.A;
  const float gamma = a.gamma, fin = a.final_value[p];
  if (a.mode == DYNENV_RETURNS_GAE) {
    const float gl = gamma * a.lambda;
    float adv = 0.0f, next = fin;
    for (int t = a.T - 1; t >= 0; --t) {
      const size_t i = (size_t)t * P + p;
      const float nd = 1.0f - a.dones[(size_t)t * a.E + env], v = a.values[i];
      const float delta = (a.rewards[i] + (gamma * next) * nd) - v;
      adv = delta + (gl * adv) * nd;
      a.returns[i] = adv + v;
      if (a.advantages) a.advantages[i] = adv;
      next = v;
    }
    return;
  }
  float R = fin;
  for (int t = a.T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * P + p;
    float g = gamma * R;
    if (a.mode == DYNENV_RETURNS_DONES) g = g * (1.0f - a.dones[(size_t)t * a.E + env]);
    R = a.rewards[i] + g;
    a.returns[i] = R;
    if (a.advantages) a.advantages[i] = R - a.values[i];
  }
}

// ---- the entry points.  Argument errors first, then what the kernels do not take, both before a device is looked for; one launch and
// nothing else: nothing is synchronised, allocated or copied, so the calls may be captured.
extern "C" int dynenv_rollout_insert(const int32_t* cursor_dev, int32_t T, int32_t E, int32_t A, int32_t F, int32_t G, int32_t action_cols, int32_t N,
                                     int32_t row_features_only, const double* rewards_in_dev, const uint8_t* finished_in_dev, const float* feat0_dev,
                                     const float* feat1_dev, const int32_t* actions_in_dev, const float* logp_in_dev, const float* logp_old_in_dev,
                                     const float* value_in_dev, const uint8_t* dones_in_dev, const float* probs_in_dev, float* rewards_dev,
                                     uint8_t* finished_dev, float* features_dev, float* actions_dev, float* logp_dev, float* logp_old_dev,
                                     float* values_dev, float* dones_dev, float* probs_dev, int32_t* status_dev, void* stream) {
  if (!cursor_dev || !status_dev) return fail(DYNENV_ERR_ARG, "rollout insert: null cursor_dev or status_dev");
  if (T < 1 || E < 1 || A < 1 || F < 1 || G < 1 || action_cols < 1 || N < 0) return fail(DYNENV_ERR_ARG, "rollout insert: bad shape");
  if (T > (1 << 24) || (int64_t)E * A > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "rollout insert: T above 2^24 or E * A above 2^30");
  if (feat1_dev && !feat0_dev) return fail(DYNENV_ERR_ARG, "rollout insert: feat1_dev without feat0_dev");
  if ((int64_t)E * A * F * (feat1_dev ? 2 : 1) > (int64_t)1 << 32) return fail(DYNENV_ERR_ARG, "rollout insert: a row of features above 2^32 elements");
  if (row_features_only && !feat0_dev) return fail(DYNENV_ERR_ARG, "rollout insert: row_features_only takes feat0_dev");
  if (probs_in_dev && N < 1) return fail(DYNENV_ERR_ARG, "rollout insert: probs_in_dev with N == 0");
  const void* pairs[][2] = {{rewards_in_dev, rewards_dev}, {finished_in_dev, finished_dev}, {feat0_dev, features_dev}, {actions_in_dev, actions_dev},
                            {logp_in_dev, logp_dev}, {logp_old_in_dev, logp_old_dev}, {value_in_dev, values_dev}, {dones_in_dev, dones_dev},
                            {probs_in_dev, probs_dev}};
  for (auto& q : pairs)
    if (q[0] && !q[1]) return fail(DYNENV_ERR_ARG, "rollout insert: an input without its buffer");
  if ((uintptr_t)feat0_dev % 16 || (uintptr_t)feat1_dev % 16 || (uintptr_t)features_dev % 16)
    return fail(DYNENV_ERR_ARG, "rollout insert: feat0_dev, feat1_dev and features_dev must be 16-byte aligned");
  const void* words[] = {cursor_dev, status_dev, actions_in_dev, logp_in_dev, logp_old_in_dev, value_in_dev, probs_in_dev, rewards_dev, actions_dev,
                         logp_dev, logp_old_dev, values_dev, dones_dev, probs_dev};
  for (const void* q : words)
    if ((uintptr_t)q % 4) return fail(DYNENV_ERR_ARG, "rollout insert: 32-bit buffers must be 4-byte aligned");
  if ((uintptr_t)rewards_in_dev % 8) return fail(DYNENV_ERR_ARG, "rollout insert: rewards_in_dev must be 8-byte aligned");
  if (F % 4) return fail(DYNENV_ERR_UNSUPPORTED, "rollout insert: the fused insert takes F a multiple of 4");
  if (G > 8 || action_cols > 8 || N > 32) return fail(DYNENV_ERR_UNSUPPORTED, "rollout insert: the fused insert takes G <= 8, action_cols <= 8 and N <= 32");
  if (int rc = have_device()) return rc;
  RiArgs k;
  k.cursor = cursor_dev; k.status = status_dev;
  k.T = T; k.E = E; k.P = E * A; k.F = F; k.K = feat1_dev ? 2 * F : F; k.G = G; k.AD = action_cols; k.N = N; k.features_only = row_features_only != 0;
  k.rewards_in = rewards_in_dev; k.finished_in = finished_in_dev; k.dones_in = dones_in_dev;
  k.feat0 = feat0_dev; k.feat1 = feat1_dev; k.logp_in = logp_in_dev; k.logp_old_in = logp_old_in_dev; k.value_in = value_in_dev; k.probs_in = probs_in_dev;
  k.actions_in = actions_in_dev;
  k.rewards = rewards_dev; k.features = features_dev; k.actions = actions_dev; k.logp = logp_dev; k.logp_old = logp_old_dev; k.values = values_dev;
  k.dones = dones_dev; k.probs = probs_dev; k.finished = finished_dev;
  const int64_t groups = (k.P + RI_ROWS - 1) / RI_ROWS, chunks = feat0_dev ? ((int64_t)k.P * (k.K / 4) + RI_CHUNK - 1) / RI_CHUNK : 0;
  hipLaunchKernelGGL(rollout_insert_kernel, dim3((unsigned)(row_features_only ? chunks : chunks > groups ? chunks : groups)), dim3(RI_BLOCK), 0,
                     (hipStream_t)stream, k);
  return launched();
}

extern "C" int dynenv_rollout_returns(const float* rewards_dev, const float* values_dev, const float* dones_dev, const float* final_value_dev, int32_t T,
                                      int32_t E, int32_t A, int32_t mode, float gamma, float gae_lambda, float* returns_dev, float* advantages_dev,
                                      void* stream) {
  if (!rewards_dev || !final_value_dev || !returns_dev) return fail(DYNENV_ERR_ARG, "rollout returns: null rewards_dev, final_value_dev or returns_dev");
  if (mode < DYNENV_RETURNS_REFERENCE || mode > DYNENV_RETURNS_GAE) return fail(DYNENV_ERR_ARG, "rollout returns: mode is 0 (reference), 1 (dones) or 2 (GAE)");
  if (mode != DYNENV_RETURNS_REFERENCE && !dones_dev) return fail(DYNENV_ERR_ARG, "rollout returns: modes 1 and 2 take dones_dev");
  if ((mode == DYNENV_RETURNS_GAE || advantages_dev) && !values_dev) return fail(DYNENV_ERR_ARG, "rollout returns: GAE and advantages_dev take values_dev");
  if (T < 1 || E < 1 || A < 1) return fail(DYNENV_ERR_ARG, "rollout returns: bad shape");
  if (T > (1 << 24) || (int64_t)E * A > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "rollout returns: T above 2^24 or E * A above 2^30");
  if (int rc = model_aligned("rollout returns", {rewards_dev, values_dev, dones_dev, final_value_dev, returns_dev, advantages_dev}, 4)) return rc;
  if (int rc = have_device()) return rc;
  RrArgs k;
  k.rewards = rewards_dev; k.values = values_dev; k.dones = dones_dev; k.final_value = final_value_dev; k.returns = returns_dev; k.advantages = advantages_dev;
  k.T = T; k.E = E; k.A = A; k.P = E * A; k.mode = mode; k.gamma = gamma; k.lambda = gae_lambda;
  hipLaunchKernelGGL(rollout_returns_kernel, dim3((unsigned)((k.P + RR_BLOCK - 1) / RR_BLOCK)), dim3(RR_BLOCK), 0, (hipStream_t)stream, k);
  return launched();
}
