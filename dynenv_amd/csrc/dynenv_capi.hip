// dynenv_capi.hip — the C ABI of include/dynenv.h on top of the gfx950 kernels.  This unit: the RoboCup and arranger kernels, the
// RoboCup handle (robocup_host.hip) and the entry points, which check their arguments, select the handle's device and call through the
// handle (dynenv_host.h), plus the arranger, the transport and the checkpoint.  driving_tu.hip: the Driving kernels and their handle.
// There is NO CPU fallback: without a usable HIP device every entry point fails with DYNENV_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <cmath>

#include "driving_host.h"   /* the Driving kernels and their host code are a translation unit of their own: driving_tu.hip */
#include "robocup_kernels.hip"
#include "arranger_kernels.hip"
#include "arranger_cols_kernels.hip"
#include "dynenv_host.h"
#include "robocup_host.hip"
#include "dynenv_math_probe.h"   /* (inline device code and two sizes: nothing is emitted here) */

// the kernels of env_rows_kernels.hip, which this unit includes last (behind everything the step launches run)
extern "C" __global__ void env_rows_save_kernel(EnvRowTable T, const int* __restrict__ idx, unsigned char* __restrict__ blobs);
extern "C" __global__ void env_rows_load_kernel(EnvRowTable T, const int* __restrict__ idx, const unsigned char* __restrict__ blobs, int* __restrict__ status);
// ... and the plan and gather of arranger_fixed_kernels.hip, with the struct they take by value
struct ArrFixed { ArrTypes ty; int rows[DYNENV_ARR_MAX_TYPES]; int maxCount; };
extern "C" __global__ void arrf_plan_kernel(const float* __restrict__ obs, int E, int T, int A, int D, ArrFixed fx, const int32_t* __restrict__ count_env, int jSpan,
                                            int32_t* __restrict__ counts, int32_t* __restrict__ obj_counts, uint8_t* __restrict__ mask, int32_t* __restrict__ dropped);
extern "C" __global__ void arrf_gather_kernel(const float* __restrict__ obs, int E, int T, int A, int D, ArrFixed fx, const int32_t* __restrict__ count_env,
                                              float* in0, float* in1, float* in2, float* in3);
// ... and this unit's math probe (include/dynenv_math_probe.h), the last kernel of the unit
extern "C" __global__ void rc_math_probe_kernel(const double* in, int n, double* out);

static thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int have_device(int* ndev, const char* msg) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(DYNENV_ERR_NO_DEVICE, msg);
  if (ndev) *ndev = n;
  return DYNENV_OK;
}

// dynenv_reset / dynenv_step / dynenv_full_obs: the Driving Full writer stores float4 where the row layout allows it, so an observation
// buffer is 16-byte aligned (NULL, where NULL is allowed, passes).  An argument check like the NULL checks: before a device is looked
// for, before the handle is dereferenced, nothing launched.
static int obs_aligned(const float* p, const char* name) {
  if ((uintptr_t)p % 16) return fail(DYNENV_ERR_ARG, std::string(name) + " must be 16-byte aligned (the observation writers store float4)");
  return DYNENV_OK;
}

extern "C" {

int dynenv_abi_version(void) { return DYNENV_ABI_VERSION; }
const char* dynenv_last_error(void) { return g_err.c_str(); }

int dynenv_create(const dynenv_cfg_t* cfg, dynenv_t** out) {
  if (!cfg || !out) return fail(DYNENV_ERR_ARG, "null argument");
  if (cfg->abi_version != DYNENV_ABI_VERSION) return fail(DYNENV_ERR_ARG, "ABI version mismatch");
  if (cfg->num_envs <= 0 || cfg->n_players <= 0) return fail(DYNENV_ERR_ARG, "num_envs and n_players must be > 0");
  if (cfg->noise_magnitude < 0 || cfg->noise_magnitude > 5)
    return fail(DYNENV_ERR_ARG, "Error: The noise magnitude must be between 0 and 5!");  // environment_base.py:162-164
  int ndev = 0;
  if (int rc = have_device(&ndev)) return rc;
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(DYNENV_ERR_ARG, "device_id out of range");
  DeviceGuard guard_(cfg->device_id);  // (the __constant__ tables are uploaded to this device below)
  if (!guard_.ok) return fail(DYNENV_ERR_HIP, "hipSetDevice failed");
  if (cfg->env_type != DYNENV_DRIVE && cfg->env_type != DYNENV_ROBO_CUP) return fail(DYNENV_ERR_ARG, "unknown env_type");
  const int32_t known = DYNENV_FLAG_RANDOM_INIT | DYNENV_FLAG_DETERMINISTIC_TURN | DYNENV_FLAG_CAN_FALL | DYNENV_FLAG_USE_OBS_REWARDS |
                        DYNENV_FLAG_ALLOW_HEAD_TURN;
  if (cfg->flags & ~known) return fail(DYNENV_ERR_UNSUPPORTED, "unknown bits in dynenv_cfg.flags");
  if (cfg->env_type == DYNENV_DRIVE && cfg->flags != 0)
    return fail(DYNENV_ERR_UNSUPPORTED, "dynenv_cfg.flags are RoboCup's class switches; DrivingEnvironment has none (continuous actions are broken in the reference, DrivingEnvironment.py:360-368)");
  if (cfg->obs_type != DYNENV_OBS_FULL && cfg->obs_type != DYNENV_OBS_PARTIAL)
    return fail(DYNENV_ERR_UNSUPPORTED, "Image observations are out of scope");
  dynenv* h = cfg->env_type == DYNENV_ROBO_CUP ? new RcHandle() : drv_new_handle();
  h->cfg = *cfg;
  int rc = h->init();
  if (!rc) rc = h->rows_finish();
  if (!rc) rc = h->alloc(&h->stage, h->state_bytes / 8 + 1, SCRATCH);  // (scratch: the checkpoint is `allocs`, in init()'s order)
  if (rc) { dynenv_destroy(h); return rc; }
  *out = h;
  return DYNENV_OK;
}

void dynenv_destroy(dynenv_t* h) {
  if (!h) return;
  DeviceGuard guard_(h->cfg.device_id);
  delete h;
}

int dynenv_layout(const dynenv_t* h, dynenv_layout_t* L) {
  if (!h || !L) return fail(DYNENV_ERR_ARG, "null argument");
  memset(L, 0, sizeof(*L));
  L->num_envs = h->cfg.num_envs; L->n_agents = h->A; L->n_time_steps = h->T; L->obs_dim = h->obs_dim;
  L->action_dim = h->action_dim;
  h->layout(*L);
  return DYNENV_OK;
}

// The seed is a by-value kernel argument: a launch that was captured keeps the one it was captured with at every replay, whatever the
// handle holds by then, while the eager launches of the same handle would follow the new one.  Never silently.
static int frozen_seed(const char* who) {
  return fail(DYNENV_ERR_UNSUPPORTED, std::string(who) + ": a step or masked reset of this handle has been captured into a graph, and a captured "
              "step replays with the seed it was captured with: the handle keeps that seed for good - create a new handle for another seed");
}

int dynenv_seed(dynenv_t* h, uint64_t seed) {
  if (!h) return fail(DYNENV_ERR_ARG, "null handle");
  if (h->captured && seed != h->cfg.seed) return frozen_seed("dynenv_seed");
  h->set_seed(seed);
  return DYNENV_OK;
}

int dynenv_reset(dynenv_t* h, float* obs_dev, void* stream) {
  if (!h) return fail(DYNENV_ERR_ARG, "null handle");
  if (int rc = obs_aligned(obs_dev, "obs_dev")) return rc;
  ON_DEVICE(h);
  return h->reset_masked(nullptr, obs_dev, (hipStream_t)stream);
}

int dynenv_reset_masked(dynenv_t* h, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!h || !mask_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (int rc = obs_aligned(obs_dev, "obs_dev")) return rc;
  ON_DEVICE(h);
  return h->reset_masked(mask_dev, obs_dev, (hipStream_t)stream);
}

int dynenv_full_obs_dim(const dynenv_t* h) { return h ? h->full_dim : fail(DYNENV_ERR_ARG, "null handle"); }
int dynenv_full_obs(dynenv_t* h, float* full_dev, void* stream) {
  if (!h || !full_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (int rc = obs_aligned(full_dev, "full_dev")) return rc;
  ON_DEVICE(h);
  return h->full_obs(full_dev, (hipStream_t)stream);
}

int dynenv_global_state_dim(const dynenv_t* h) { return h ? h->global_dim : fail(DYNENV_ERR_ARG, "null handle"); }
int dynenv_global_state(dynenv_t* h, float* state_dev, void* stream) {
  if (!h || !state_dev) return fail(DYNENV_ERR_ARG, "null argument");
  ON_DEVICE(h);
  return h->global_state(state_dev, (hipStream_t)stream);
}

// the one step: dynenv_step / dynenv_step_head are dynenv_step_masked without a mask (every environment)
static int step_any(dynenv_t* h, const uint8_t* mask_dev, const int32_t* actions_dev, const double* head_dev, float* obs_dev, double* rewards_dev,
                    uint8_t* dones_dev, void* stream) {
  if (!h || !actions_dev || !rewards_dev || !dones_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (int rc = obs_aligned(obs_dev, "obs_dev")) return rc;
  if (head_dev && !(h->cfg.flags & DYNENV_FLAG_ALLOW_HEAD_TURN))  // (RoboCup's switch: a Driving handle has no flags, dynenv_create)
    return fail(DYNENV_ERR_ARG, "the continuous head channel exists for RoboCup with DYNENV_FLAG_ALLOW_HEAD_TURN only");
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  // measurement hook (dynenv_set_step_events): the step's dominant kernel bracketed by events on the launch stream - ev_begin and
  // ev_main are recorded by the handle's step around that kernel (step_begin / step_main_done), ev_end here, behind its last launch
  struct StepEvents {
    dynenv* h; hipStream_t st;
    ~StepEvents() { if (h->ev_end) (void)hipEventRecord(h->ev_end, st); }
  } sev{h, st};
  return h->step(mask_dev, (const int*)actions_dev, head_dev, obs_dev, rewards_dev, dones_dev, st);
}

int dynenv_step(dynenv_t* h, const int32_t* actions_dev, float* obs_dev, double* rewards_dev, uint8_t* dones_dev,
                void* stream) {
  return step_any(h, nullptr, actions_dev, nullptr, obs_dev, rewards_dev, dones_dev, stream);
}

int dynenv_step_head(dynenv_t* h, const int32_t* actions_dev, const double* head_dev, float* obs_dev, double* rewards_dev,
                     uint8_t* dones_dev, void* stream) {
  return step_any(h, nullptr, actions_dev, head_dev, obs_dev, rewards_dev, dones_dev, stream);
}

int dynenv_step_masked(dynenv_t* h, const uint8_t* mask_dev, const int32_t* actions_dev, const double* head_dev, float* obs_dev,
                       double* rewards_dev, uint8_t* dones_dev, void* stream) {
  if (!h || !mask_dev) return fail(DYNENV_ERR_ARG, "null argument");
  return step_any(h, mask_dev, actions_dev, head_dev, obs_dev, rewards_dev, dones_dev, stream);
}

int dynenv_set_step_events(dynenv_t* h, void* ev_begin, void* ev_main_done, void* ev_end) {
  if (!h) return fail(DYNENV_ERR_ARG, "null handle");
  h->ev_begin = (hipEvent_t)ev_begin; h->ev_main = (hipEvent_t)ev_main_done; h->ev_end = (hipEvent_t)ev_end;
  return DYNENV_OK;
}

int dynenv_counts(dynenv_t* h, int32_t* counts_dev, void* stream) {
  if (!h || !counts_dev) return fail(DYNENV_ERR_ARG, "null argument");
  ON_DEVICE(h);
  return h->counts(counts_dev, (hipStream_t)stream);
}

int dynenv_episode_stats(dynenv_t* h, double* ep_r, double* ep_pos_r, double* ep_obs_r, int32_t* goals, void* stream) {
  if (!h) return fail(DYNENV_ERR_ARG, "null handle");
  ON_DEVICE(h);
  return h->episode_stats(ep_r, ep_pos_r, ep_obs_r, goals, (hipStream_t)stream);
}

size_t dynenv_state_size(const dynenv_t* h) { return h ? h->state_bytes : sizeof(dynenv_driving_state_t); }

int dynenv_sync(dynenv_t* h, void* stream) {
  if (!h) return fail(DYNENV_ERR_ARG, "null handle");
  ON_DEVICE(h);
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  return DYNENV_OK;
}

// error flags raised by the kernels (bit0: contact cache overflow), OR-ed over all envs
int dynenv_error_flags(dynenv_t* h, int32_t* out) {
  if (!h || !out) return fail(DYNENV_ERR_ARG, "null argument");
  ON_DEVICE(h);
  HIP_OK(hipDeviceSynchronize());
  std::vector<int> w((size_t)h->cfg.num_envs * h->rows.errStride);
  HIP_OK(hipMemcpy(w.data(), h->rows.err, w.size() * sizeof(int), hipMemcpyDeviceToHost));
  int fl = 0;
  for (size_t e = 0; e < (size_t)h->cfg.num_envs; ++e) fl |= w[e * h->rows.errStride + h->rows.errIndex];
  *out = fl;
  return DYNENV_OK;
}

// diagnostics of the Driving step (the handle's debug_counters / debug_placement say what they report)
int dynenv_debug_counters(dynenv_t* h, int64_t* out16) {
  if (!h || !out16) return fail(DYNENV_ERR_ARG, "null argument");
  ON_DEVICE(h);
  return h->debug_counters(out16);
}
int dynenv_debug_placement(dynenv_t* h, uint32_t* out, int32_t n) {
  if (!h || !out || n < 0) return fail(DYNENV_ERR_ARG, "bad argument");
  ON_DEVICE(h);
  return h->debug_placement(out, n);
}

// ONE environment through host memory, synchronously: the state kernels for one blob in the handle's staging area, on the null stream
int dynenv_get_state(dynenv_t* h, int32_t env, void* blob, size_t nbytes) {
  if (!h || !blob) return fail(DYNENV_ERR_ARG, "null argument");
  if (env < 0 || env >= h->cfg.num_envs || nbytes < h->state_bytes) return fail(DYNENV_ERR_ARG, "bad env index / size");
  ON_DEVICE(h);
  HIP_OK(hipDeviceSynchronize());
  if (int rc = h->get_states(nullptr, env, 1, h->stage, nullptr)) return rc;
  HIP_OK(hipMemcpy(blob, h->stage, h->state_bytes, hipMemcpyDeviceToHost));
  return DYNENV_OK;
}
// A blob that does not fit is an error of this call, whose caller is told: nothing is written and no error bit is raised.
int dynenv_set_state(dynenv_t* h, int32_t env, const void* blob, size_t nbytes) {
  if (!h || !blob) return fail(DYNENV_ERR_ARG, "null argument");
  if (env < 0 || env >= h->cfg.num_envs || nbytes < h->state_bytes) return fail(DYNENV_ERR_ARG, "bad env index / size");
  ON_DEVICE(h);
  HIP_OK(hipDeviceSynchronize());
  int32_t* status_dev = (int32_t*)(h->stage + h->state_bytes / 8);
  int32_t status = -1;
  HIP_OK(hipMemcpy(h->stage, blob, h->state_bytes, hipMemcpyHostToDevice));
  if (int rc = h->set_states(nullptr, env, 1, h->stage, status_dev, false, nullptr)) return rc;
  HIP_OK(hipMemcpy(&status, status_dev, sizeof(status), hipMemcpyDeviceToHost));
  if (status != 0) return fail(DYNENV_ERR_ARG, "state blob does not match this handle's layout");
  return DYNENV_OK;
}

// the batched, device-side forms: ordered on `stream`, no host synchronisation, no allocation, no host copy
// (what: "the" canonical blobs, 8-byte aligned; "the exact" blobs, 16-byte aligned)
static int blobs_args(const dynenv_t* h, const int32_t* idx, int32_t n, const void* blobs, unsigned align, const char* what) {
  if (!h || (!blobs && n > 0)) return fail(DYNENV_ERR_ARG, "null argument");
  if (n < 0) return fail(DYNENV_ERR_ARG, "negative blob count");
  if (!idx && n > h->cfg.num_envs) return fail(DYNENV_ERR_ARG, "more blobs than environments and no index list");
  if ((uintptr_t)blobs % align) return fail(DYNENV_ERR_ARG, std::string(what) + " blobs must be " + std::to_string(align) + "-byte aligned");
  return DYNENV_OK;
}
int dynenv_get_states(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, void* blobs_dev, void* stream) {
  if (int rc = blobs_args(h, env_idx_dev, n, blobs_dev, 8, "the")) return rc;
  if (n == 0) return DYNENV_OK;
  ON_DEVICE(h);
  return h->get_states(env_idx_dev, 0, n, blobs_dev, (hipStream_t)stream);
}
int dynenv_set_states(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, const void* blobs_dev, int32_t* status_dev, void* stream) {
  if (int rc = blobs_args(h, env_idx_dev, n, blobs_dev, 8, "the")) return rc;
  if (n == 0) return DYNENV_OK;
  ON_DEVICE(h);
  return h->set_states(env_idx_dev, 0, n, blobs_dev, status_dev, true, (hipStream_t)stream);
}

// exact save / restore of chosen environments: every row of the handle's row table (dynenv_host.h), one launch each way of the two
// kernels both handles share (env_rows_kernels.hip); the rules of dynenv_get_states / dynenv_set_states, 16-byte aligned blobs
size_t dynenv_exact_size(const dynenv_t* h) { return h ? h->rows.blobBytes : 0; }
int dynenv_get_exact(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, void* blobs_dev, void* stream) {
  if (int rc = blobs_args(h, env_idx_dev, n, blobs_dev, 16, "the exact")) return rc;
  if (n == 0) return DYNENV_OK;
  ON_DEVICE(h);
  hipLaunchKernelGGL(env_rows_save_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, h->rows, (const int*)env_idx_dev, (unsigned char*)blobs_dev);
  return launched();
}
int dynenv_set_exact(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, const void* blobs_dev, int32_t* status_dev, void* stream) {
  if (int rc = blobs_args(h, env_idx_dev, n, blobs_dev, 16, "the exact")) return rc;
  if (n == 0) return DYNENV_OK;
  ON_DEVICE(h);
  hipLaunchKernelGGL(env_rows_load_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, h->rows, (const int*)env_idx_dev, (const unsigned char*)blobs_dev,
                     (int*)status_dev);
  return launched();
}

int dynenv_error_flags_env(dynenv_t* h, int32_t* flags_dev, void* stream) {
  if (!h || !flags_dev) return fail(DYNENV_ERR_ARG, "null argument");
  ON_DEVICE(h);
  return h->error_flags_env(flags_dev, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// ragged -> padded arranger (arranger_kernels.hip); replaces InOutArranger (reference models/models.py:208-274)
// ------------------------------------------------------------------------------------------------
static int arr_types(const dynenv_arr_type_t* types, int32_t n_types, int32_t D, ArrTypes& out) {
  if (!types || n_types < 1 || n_types > DYNENV_ARR_MAX_TYPES) return fail(DYNENV_ERR_ARG, "arranger: 1..4 object types");
  out.n = n_types;
  for (int i = 0; i < n_types; ++i) {
    const dynenv_arr_type_t& t = types[i];
    if (t.feat < 1 || t.cap < 0 || t.offset < 0 || t.offset + t.feat * t.cap > D) return fail(DYNENV_ERR_ARG, "arranger: block outside the observation row");
    if (t.count_mode == DYNENV_ARR_COUNT_ROW && (t.count_index < 0 || t.count_index >= D)) return fail(DYNENV_ERR_ARG, "arranger: count_index outside the observation row");
    if (t.count_mode < 0 || t.count_mode > DYNENV_ARR_COUNT_ROW) return fail(DYNENV_ERR_ARG, "arranger: unknown count_mode");
    out.t[i] = t;
  }
  return DYNENV_OK;
}

int64_t dynenv_arrange_scratch_ints(int32_t E, int32_t T, int32_t A, int32_t n_types) {
  const int64_t TP = (int64_t)E * T * A, nBlocks = (TP + ARR_BLOCK - 1) / ARR_BLOCK;
  return (n_types + 1) * nBlocks + 2 * (DYNENV_ARR_MAX_TYPES + 1) /* int64 results */;
}

int dynenv_arrange_plan(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types,
                        int32_t n_types, const int32_t* count_env_dev, int32_t* counts_dev, int32_t* obj_counts_dev,
                        int32_t* base_dev, int32_t* scratch_dev, dynenv_arr_plan_t* plan_host, void* stream) {
  if (int rc = have_device()) return rc;
  if (!obs_dev || !counts_dev || !obj_counts_dev || !base_dev || !scratch_dev || !plan_host) return fail(DYNENV_ERR_ARG, "null argument");
  if (E < 1 || T < 1 || A < 1 || D < 1 || (int64_t)E * T * A > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "arranger: bad shape");
  ArrTypes ty;
  if (int rc = arr_types(types, n_types, D, ty)) return rc;
  for (int i = 0; i < n_types; ++i)
    if (types[i].count_mode == DYNENV_ARR_COUNT_ENV && !count_env_dev) return fail(DYNENV_ERR_ARG, "arranger: count_env_dev missing");
  hipStream_t st = (hipStream_t)stream;
  const int TP = E * T * A, nBlocks = (TP + ARR_BLOCK - 1) / ARR_BLOCK;
  int32_t* blockTot = scratch_dev;
  // int64 results live behind the block totals, 8-byte aligned
  size_t off = (size_t)(n_types + 1) * nBlocks;
  off = (off + 1) & ~(size_t)1;
  int64_t* result = reinterpret_cast<int64_t*>(scratch_dev + off);
  hipLaunchKernelGGL(arr_count_kernel, dim3(nBlocks), dim3(ARR_BLOCK), 0, st, obs_dev, E, T, A, D, ty, count_env_dev, counts_dev,
                     obj_counts_dev, base_dev, blockTot);
  hipLaunchKernelGGL(arr_scan_blocks_kernel, dim3(1), dim3(ARR_BLOCK), 0, st, blockTot, nBlocks, n_types, result);
  hipLaunchKernelGGL(arr_add_offsets_kernel, dim3(nBlocks), dim3(ARR_BLOCK), 0, st, base_dev, blockTot, TP, nBlocks, n_types);
  HIP_OK(hipGetLastError());
  int64_t res[DYNENV_ARR_MAX_TYPES + 1];
  HIP_OK(hipMemcpyAsync(res, result, sizeof(int64_t) * (n_types + 1), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  plan_host->n_types = n_types; plan_host->n_time = T; plan_host->n_players = E * A; plan_host->max_count = (int32_t)res[n_types];
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) plan_host->total[i] = i < n_types ? res[i] : 0;
  return DYNENV_OK;
}

int dynenv_arrange_gather(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types,
                          int32_t n_types, const int32_t* counts_dev, const int32_t* base_dev, int32_t max_count,
                          float* const* inputs_dev, int32_t* const* slot_dev, uint8_t* mask_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (!obs_dev || !counts_dev || !base_dev) return fail(DYNENV_ERR_ARG, "null argument");
  ArrTypes ty;
  if (int rc = arr_types(types, n_types, D, ty)) return rc;
  int capSum = 0;
  for (int i = 0; i < n_types; ++i) capSum += types[i].cap;
  const int jSpan = capSum > max_count ? capSum : (max_count > 0 ? max_count : 1);
  const long long total = (long long)E * T * A * jSpan;
  float* in[DYNENV_ARR_MAX_TYPES] = {nullptr, nullptr, nullptr, nullptr};
  int32_t* sl[DYNENV_ARR_MAX_TYPES] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < n_types; ++i) { if (inputs_dev) in[i] = inputs_dev[i]; if (slot_dev) sl[i] = slot_dev[i]; }
  hipLaunchKernelGGL(arr_gather_kernel, dim3((unsigned)((total + ARR_BLOCK - 1) / ARR_BLOCK)), dim3(ARR_BLOCK), 0, (hipStream_t)stream,
                     obs_dev, E, T, A, D, ty, counts_dev, base_dev, max_count, jSpan, in[0], in[1], in[2], in[3], sl[0], sl[1], sl[2], sl[3], mask_dev);
  return launched();
}

int dynenv_arrange_scatter(const float* emb_dev, const int32_t* slot_dev, int64_t N, int32_t F, float* padded_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (N == 0) return DYNENV_OK;
  if (!emb_dev || !slot_dev || !padded_dev || N < 0 || F < 1) return fail(DYNENV_ERR_ARG, "bad argument");
  const long long total = (long long)N * F;
  hipLaunchKernelGGL(arr_scatter_kernel, dim3((unsigned)((total + ARR_BLOCK - 1) / ARR_BLOCK)), dim3(ARR_BLOCK), 0, (hipStream_t)stream,
                     emb_dev, slot_dev, (long long)N, F, padded_dev);
  return launched();
}

// ---- the padded tensor in one pass and its backward (arranger_cols_kernels.hip): eight entry points, one launcher.
// What the checked entry points share: every argument error, before a device is looked for.  `third` is base_dev (default mode,
// rw == nullptr) or rows (fixed mode).
static int arr_as_args(const void* big, const void* const* per_type, const int32_t* counts_dev, const void* third, int32_t n_types, int32_t T,
                       int32_t P, int32_t max_count, int32_t F, int32_t emb_dtype, int32_t padded_dtype, ArrFixedRows* rw) {
  if (!big || !per_type || !counts_dev || !third) return fail(DYNENV_ERR_ARG, "null argument");
  if (emb_dtype < DYNENV_ARR_F32 || emb_dtype > DYNENV_ARR_F16 || padded_dtype < DYNENV_ARR_F32 || padded_dtype > DYNENV_ARR_F16)
    return fail(DYNENV_ERR_ARG, "arranger: unknown dtype (DYNENV_ARR_F32, _BF16 or _F16)");
  const int u = padded_dtype == DYNENV_ARR_F32 ? 4 : 8;
  if (n_types < 1 || n_types > DYNENV_ARR_MAX_TYPES || T < 1 || P < 1 || max_count < 0 || F < u || (F & (u - 1)))
    return fail(DYNENV_ERR_ARG, u == 8 ? "arranger: bad shape (F must be a multiple of 8 for a 16-bit padded tensor)" : "arranger: bad shape (F must be a multiple of 4)");
  if ((long long)P * (F / u) > 0x7fffffffLL || T > 65535 || (rw && (int64_t)T * P > (int64_t)1 << 30))
    return fail(DYNENV_ERR_ARG, "arranger: padded tensor too large for one launch");
  if ((uintptr_t)big % 16) return fail(DYNENV_ERR_ARG, "arranger: buffers must be 16-byte aligned");
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) {
    if (rw) {
      rw->rows[i] = i < n_types ? ((const int32_t*)third)[i] : 0;
      if (rw->rows[i] < 0) return fail(DYNENV_ERR_ARG, "arranger: rows[i] < 0");
    }
    if (i < n_types && (uintptr_t)per_type[i] % 16) return fail(DYNENV_ERR_ARG, "arranger: buffers must be 16-byte aligned");
  }
  const bool ok = emb_dtype == padded_dtype || emb_dtype == DYNENV_ARR_F32;
  if (!ok) return fail(DYNENV_ERR_UNSUPPORTED, "arranger: embeddings are float32 or of the padded tensor's own dtype");
  return DYNENV_OK;
}
// The launch behind the eight, arguments already checked and a device found: forward (big = the padded tensor, per_type = the
// embeddings) or backward (big = its gradient, per_type = the embeddings' gradients), default mode (base, rw == nullptr) or fixed mode
// (rw).  Embeddings of the padded tensor's own dtype are a copy of 16-byte units - 4 float32 or 8 16-bit elements - else float32 is
// narrowed to / widened from bf16 or fp16.  max_count == 0 launches nothing.
static int arr_cols_launch(bool backward, const void* big, const void* const* per_type, const int32_t* counts_dev, const int32_t* base_dev,
                           const ArrFixedRows* rw, int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, int32_t emb_dtype,
                           int32_t padded_dtype, void* stream) {
  static decltype(&arr_pad_cols_kernel) const pad[2][3] = {{arr_pad_cols_kernel, arr_pad_cols_bf16_kernel, arr_pad_cols_f16_kernel},
                                                           {arrf_pad_cols_kernel, arrf_pad_cols_bf16_kernel, arrf_pad_cols_f16_kernel}};
  static decltype(&arr_unpad_cols_kernel) const unpad[2][3] = {{arr_unpad_cols_kernel, arr_unpad_cols_bf16_kernel, arr_unpad_cols_f16_kernel},
                                                               {arrf_unpad_cols_kernel, arrf_unpad_cols_bf16_kernel, arrf_unpad_cols_f16_kernel}};
  if (max_count == 0) return DYNENV_OK;
  const int unit = emb_dtype == padded_dtype ? 0 : padded_dtype == DYNENV_ARR_BF16 ? 1 : 2;
  const int units = F / (padded_dtype == DYNENV_ARR_F32 ? 4 : 8);   // 16-byte units of a padded row
  // the lanes that exchange their units in the widening backward (arrd_widen_st): the largest power of two that divides F / 8, at most a wave
  int G = 1;
  while (unit && G < 64 && units % (2 * G) == 0) G *= 2;
  const void* q[DYNENV_ARR_MAX_TYPES] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < n_types; ++i) q[i] = per_type[i];
  const dim3 grid((unsigned)(((long long)P * units + ARR_BLOCK - 1) / ARR_BLOCK), (unsigned)T);
  const ArrFixedRows rows = rw ? *rw : ArrFixedRows();
  if (backward)
    hipLaunchKernelGGL(unpad[rw != nullptr][unit], grid, dim3(ARR_BLOCK), 0, (hipStream_t)stream, static_cast<const arr_u4*>(big), counts_dev, base_dev,
                       rows, n_types, T, P, max_count, units, G, const_cast<void*>(q[0]), const_cast<void*>(q[1]), const_cast<void*>(q[2]),
                       const_cast<void*>(q[3]));
  else
    hipLaunchKernelGGL(pad[rw != nullptr][unit], grid, dim3(ARR_BLOCK), 0, (hipStream_t)stream, q[0], q[1], q[2], q[3], counts_dev, base_dev, rows, n_types,
                       T, P, max_count, units, static_cast<arr_u4*>(const_cast<void*>(big)));
  return launched();
}

// (device first, and no alignment check here or in the backward: the Python side routes misaligned buffers to the scatter kernels)
int dynenv_arrange_pad(const float* const* emb_dev, const int32_t* counts_dev, const int32_t* base_dev, int32_t n_types,
                       int32_t T, int32_t P, int32_t max_count, int32_t F, float* padded_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (!emb_dev || !counts_dev || !base_dev || !padded_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (n_types < 1 || n_types > DYNENV_ARR_MAX_TYPES || T < 1 || P < 1 || max_count < 0 || F < 4 || (F & 3)) return fail(DYNENV_ERR_ARG, "arranger: bad shape (F must be a multiple of 4)");
  if (max_count == 0) return DYNENV_OK;
  if ((long long)P * (F / 4) > 0x7fffffffLL || T > 65535) return fail(DYNENV_ERR_ARG, "arranger: padded tensor too large for one launch");
  return arr_cols_launch(false, padded_dev, (const void* const*)emb_dev, counts_dev, base_dev, nullptr, n_types, T, P, max_count, F, DYNENV_ARR_F32,
                         DYNENV_ARR_F32, stream);
}

// the backward of the two calls above.  Argument errors come before a device is looked for (as in dynenv_reset_masked): they are
// the same with and without a GPU.
int dynenv_arrange_pad_backward(const float* grad_padded_dev, const int32_t* counts_dev, const int32_t* base_dev, int32_t n_types,
                                int32_t T, int32_t P, int32_t max_count, int32_t F, float* const* grad_emb_dev, void* stream) {
  if (!grad_padded_dev || !counts_dev || !base_dev || !grad_emb_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (n_types < 1 || n_types > DYNENV_ARR_MAX_TYPES || T < 1 || P < 1 || max_count < 0 || F < 4 || (F & 3)) return fail(DYNENV_ERR_ARG, "arranger: bad shape (F must be a multiple of 4)");
  if ((long long)P * (F / 4) > 0x7fffffffLL || T > 65535) return fail(DYNENV_ERR_ARG, "arranger: padded tensor too large for one launch");
  if (int rc = have_device()) return rc;
  return arr_cols_launch(true, grad_padded_dev, (const void* const*)grad_emb_dev, counts_dev, base_dev, nullptr, n_types, T, P, max_count, F,
                         DYNENV_ARR_F32, DYNENV_ARR_F32, stream);
}

int dynenv_arrange_scatter_backward(const float* grad_padded_dev, const int32_t* slot_dev, int64_t N, int32_t F, float* grad_emb_dev, void* stream) {
  if (N < 0 || F < 1) return fail(DYNENV_ERR_ARG, "bad argument");
  if (N > 0 && (!grad_padded_dev || !slot_dev || !grad_emb_dev)) return fail(DYNENV_ERR_ARG, "null argument");
  const long long nBlocks = (N > 0x7fffffffffffffffLL / F) ? -1 : ((long long)N * F + ARR_BLOCK - 1) / ARR_BLOCK;
  if (nBlocks < 0 || nBlocks > 0x7fffffffLL) return fail(DYNENV_ERR_ARG, "arranger: too many rows for one launch");
  if (int rc = have_device()) return rc;
  if (N == 0) return DYNENV_OK;
  hipLaunchKernelGGL(arr_unscatter_kernel, dim3((unsigned)nBlocks), dim3(ARR_BLOCK), 0, (hipStream_t)stream,
                     grad_padded_dev, slot_dev, (long long)N, F, grad_emb_dev);
  return launched();
}

// ---- the arranger at fixed capacities (arranger_fixed_kernels.hip): launches only - nothing synchronised, allocated or copied to the
// host, so every call may be captured.  Argument errors come before a device is looked for.
int dynenv_arrange_fixed_gather(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types,
                                int32_t n_types, const int32_t* count_env_dev, const int32_t* rows, int32_t max_count, int32_t* counts_dev,
                                int32_t* obj_counts_dev, float* const* inputs_dev, uint8_t* mask_dev, int32_t* dropped_dev, void* stream) {
  if (!obs_dev || !rows || !counts_dev || !obj_counts_dev) return fail(DYNENV_ERR_ARG, "null argument");
  if (E < 1 || T < 1 || A < 1 || D < 1 || (int64_t)E * T * A > (int64_t)1 << 30) return fail(DYNENV_ERR_ARG, "arranger: bad shape");
  if (max_count < 0) return fail(DYNENV_ERR_ARG, "arranger: max_count < 0");
  ArrFixed fx;
  if (int rc = arr_types(types, n_types, D, fx.ty)) return rc;
  const long long TP = (long long)E * T * A;
  long long gatherBlocks = 0;
  float* in[DYNENV_ARR_MAX_TYPES] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < DYNENV_ARR_MAX_TYPES; ++i) fx.rows[i] = 0;
  for (int i = 0; i < n_types; ++i) {
    if (types[i].count_mode == DYNENV_ARR_COUNT_ENV && !count_env_dev) return fail(DYNENV_ERR_ARG, "arranger: count_env_dev missing");
    if (rows[i] < 0 || rows[i] > types[i].cap) return fail(DYNENV_ERR_ARG, "arranger: rows[i] outside 0..cap");
    fx.rows[i] = rows[i];
    if (inputs_dev && rows[i] > 0) in[i] = inputs_dev[i];
    const long long b = in[i] ? (TP * rows[i] * types[i].feat + ARR_BLOCK - 1) / ARR_BLOCK : 0;
    gatherBlocks = b > gatherBlocks ? b : gatherBlocks;
  }
  fx.maxCount = max_count;
  const int jSpan = max_count > 0 ? max_count : 1;
  const long long planBlocks = (TP * jSpan + ARR_BLOCK - 1) / ARR_BLOCK;
  if (planBlocks > 0x7fffffffLL || gatherBlocks > 0x7fffffffLL) return fail(DYNENV_ERR_ARG, "arranger: too many rows for one launch");
  if (int rc = have_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(arrf_plan_kernel, dim3((unsigned)planBlocks), dim3(ARR_BLOCK), 0, st, obs_dev, E, T, A, D, fx, count_env_dev, jSpan,
                     counts_dev, obj_counts_dev, max_count > 0 ? mask_dev : (uint8_t*)nullptr, dropped_dev);
  if (gatherBlocks > 0)
    hipLaunchKernelGGL(arrf_gather_kernel, dim3((unsigned)gatherBlocks, (unsigned)n_types), dim3(ARR_BLOCK), 0, st, obs_dev, E, T, A, D, fx,
                       count_env_dev, in[0], in[1], in[2], in[3]);
  return launched();
}

// the float32 calls are the _as calls with float32 twice
int dynenv_arrange_fixed_pad(const float* const* emb_dev, const int32_t* counts_dev, const int32_t* rows, int32_t n_types, int32_t T,
                             int32_t P, int32_t max_count, int32_t F, float* padded_dev, void* stream) {
  return dynenv_arrange_fixed_pad_as((const void* const*)emb_dev, DYNENV_ARR_F32, counts_dev, rows, n_types, T, P, max_count, F, padded_dev, DYNENV_ARR_F32, stream);
}

int dynenv_arrange_fixed_pad_backward(const float* grad_padded_dev, const int32_t* counts_dev, const int32_t* rows, int32_t n_types, int32_t T,
                                      int32_t P, int32_t max_count, int32_t F, float* const* grad_emb_dev, void* stream) {
  return dynenv_arrange_fixed_pad_backward_as(grad_padded_dev, DYNENV_ARR_F32, counts_dev, rows, n_types, T, P, max_count, F, (void* const*)grad_emb_dev,
                                              DYNENV_ARR_F32, stream);
}

// ---- dynenv_arrange_pad / _pad_backward / _fixed_pad / _fixed_pad_backward with a dtype for the per-type buffers and one for the
// padded tensor
int dynenv_arrange_pad_as(const void* const* emb_dev, int32_t emb_dtype, const int32_t* counts_dev, const int32_t* base_dev, int32_t n_types,
                          int32_t T, int32_t P, int32_t max_count, int32_t F, void* padded_dev, int32_t padded_dtype, void* stream) {
  if (int rc = arr_as_args(padded_dev, emb_dev, counts_dev, base_dev, n_types, T, P, max_count, F, emb_dtype, padded_dtype, nullptr)) return rc;
  if (int rc = have_device()) return rc;
  return arr_cols_launch(false, padded_dev, emb_dev, counts_dev, base_dev, nullptr, n_types, T, P, max_count, F, emb_dtype, padded_dtype, stream);
}

int dynenv_arrange_pad_backward_as(const void* grad_padded_dev, int32_t padded_dtype, const int32_t* counts_dev, const int32_t* base_dev,
                                   int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* const* grad_emb_dev,
                                   int32_t emb_dtype, void* stream) {
  if (int rc = arr_as_args(grad_padded_dev, (const void* const*)grad_emb_dev, counts_dev, base_dev, n_types, T, P, max_count, F, emb_dtype, padded_dtype, nullptr)) return rc;
  if (int rc = have_device()) return rc;
  return arr_cols_launch(true, grad_padded_dev, (const void* const*)grad_emb_dev, counts_dev, base_dev, nullptr, n_types, T, P, max_count, F, emb_dtype,
                         padded_dtype, stream);
}

int dynenv_arrange_fixed_pad_as(const void* const* emb_dev, int32_t emb_dtype, const int32_t* counts_dev, const int32_t* rows, int32_t n_types,
                                int32_t T, int32_t P, int32_t max_count, int32_t F, void* padded_dev, int32_t padded_dtype, void* stream) {
  ArrFixedRows rw;
  if (int rc = arr_as_args(padded_dev, emb_dev, counts_dev, rows, n_types, T, P, max_count, F, emb_dtype, padded_dtype, &rw)) return rc;
  if (int rc = have_device()) return rc;
  return arr_cols_launch(false, padded_dev, emb_dev, counts_dev, nullptr, &rw, n_types, T, P, max_count, F, emb_dtype, padded_dtype, stream);
}

int dynenv_arrange_fixed_pad_backward_as(const void* grad_padded_dev, int32_t padded_dtype, const int32_t* counts_dev, const int32_t* rows,
                                         int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* const* grad_emb_dev,
                                         int32_t emb_dtype, void* stream) {
  ArrFixedRows rw;
  if (int rc = arr_as_args(grad_padded_dev, (const void* const*)grad_emb_dev, counts_dev, rows, n_types, T, P, max_count, F, emb_dtype, padded_dtype, &rw)) return rc;
  if (int rc = have_device()) return rc;
  return arr_cols_launch(true, grad_padded_dev, (const void* const*)grad_emb_dev, counts_dev, nullptr, &rw, n_types, T, P, max_count, F, emb_dtype,
                         padded_dtype, stream);
}

int dynenv_obs_pack(const float* obs_dev, int64_t n_env_time, int32_t A, int32_t D, int32_t split, float* packed_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (!obs_dev || !packed_dev || n_env_time < 0 || A < 1 || D < 1 || split < 0 || split > D) return fail(DYNENV_ERR_ARG, "bad argument");
  const long long total = (long long)n_env_time * ((long long)A * split + (D - split));
  if (total == 0) return DYNENV_OK;
  hipLaunchKernelGGL(obs_pack_kernel, dim3((unsigned)((total + ARR_BLOCK - 1) / ARR_BLOCK)), dim3(ARR_BLOCK), 0, (hipStream_t)stream,
                     obs_dev, (long long)n_env_time, A, D, split, packed_dev);
  return launched();
}
int dynenv_obs_unpack(const float* packed_dev, int64_t n_env_time, int32_t A, int32_t D, int32_t split, float* obs_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (!obs_dev || !packed_dev || n_env_time < 0 || A < 1 || D < 1 || split < 0 || split > D) return fail(DYNENV_ERR_ARG, "bad argument");
  const long long total = (long long)n_env_time * A * D;
  if (total == 0) return DYNENV_OK;
  hipLaunchKernelGGL(obs_unpack_kernel, dim3((unsigned)((total + ARR_BLOCK - 1) / ARR_BLOCK)), dim3(ARR_BLOCK), 0, (hipStream_t)stream,
                     packed_dev, (long long)n_env_time, A, D, split, obs_dev, 0ll);
  return launched();
}
int dynenv_obs_unpack_ranks(const float* packed_dev, int64_t src_stride_floats, int32_t n_ranks, int64_t n_env_time, int32_t A,
                            int32_t D, int32_t split, float* obs_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (!obs_dev || !packed_dev || n_env_time < 0 || A < 1 || D < 1 || split < 0 || split > D || n_ranks < 1 || n_ranks > 65535 || src_stride_floats < 0)
    return fail(DYNENV_ERR_ARG, "bad argument");
  const long long total = (long long)n_env_time * A * D;
  if (total == 0) return DYNENV_OK;
  hipLaunchKernelGGL(obs_unpack_kernel, dim3((unsigned)((total + ARR_BLOCK - 1) / ARR_BLOCK), (unsigned)n_ranks), dim3(ARR_BLOCK), 0,
                     (hipStream_t)stream, packed_dev, (long long)n_env_time, A, D, split, obs_dev, (long long)src_stride_floats);
  return launched();
}

int dynenv_obs_pack_peers(const float* obs_dev, int64_t n_env_time, int32_t A, int32_t D, float* packed_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (!obs_dev || !packed_dev || n_env_time < 0 || A < 1 || D < PEER_SELF + (A - 1) * PEER_COLS) return fail(DYNENV_ERR_ARG, "bad argument");
  const long long total = (long long)n_env_time * (A * PEER_SELF + (D - PEER_SELF - (A - 1) * PEER_COLS));
  if (total == 0) return DYNENV_OK;
  hipLaunchKernelGGL(obs_pack_peers_kernel, dim3((unsigned)((total + ARR_BLOCK - 1) / ARR_BLOCK)), dim3(ARR_BLOCK), 0, (hipStream_t)stream,
                     obs_dev, (long long)n_env_time, A, D, packed_dev);
  return launched();
}
int dynenv_obs_unpack_peers_ranks(const float* packed_dev, int64_t src_stride_floats, int32_t n_ranks, int64_t n_env_time, int32_t A,
                                  int32_t D, float* obs_dev, void* stream) {
  if (int rc = have_device()) return rc;
  if (!obs_dev || !packed_dev || n_env_time < 0 || A < 1 || D < PEER_SELF + (A - 1) * PEER_COLS || n_ranks < 1 || n_ranks > 65535 ||
      src_stride_floats < 0)
    return fail(DYNENV_ERR_ARG, "bad argument");
  const long long total = (long long)n_env_time * A * D;
  if (total == 0) return DYNENV_OK;
  const bool vec = (D % 4) == 0 && ((uintptr_t)obs_dev % 16) == 0;
  if (vec && A <= PEER_ROWS_MAXA && D - (PEER_SELF + (A - 1) * PEER_COLS) <= 160) {
    // row job (see obs_unpack_peers_rows_kernel)
    int rowsPerBlock = (int)((n_env_time * (long long)n_ranks + 4095) / 4096);  // ~4096 blocks: the chip several times over
    if (rowsPerBlock < 1) rowsPerBlock = 1;
    if (rowsPerBlock > 32) rowsPerBlock = 32;
    const dim3 rgrid((unsigned)((n_env_time + rowsPerBlock - 1) / rowsPerBlock), (unsigned)n_ranks);
    hipLaunchKernelGGL(obs_unpack_peers_rows_kernel, rgrid, dim3(ARR_BLOCK), 0, (hipStream_t)stream, packed_dev, (long long)n_env_time, A, D,
                       obs_dev, (long long)src_stride_floats, rowsPerBlock);
    return launched();
  }
  const long long threads = vec ? total / 4 : total;
  const dim3 grid((unsigned)((threads + ARR_BLOCK - 1) / ARR_BLOCK), (unsigned)n_ranks);
  if (vec)
    hipLaunchKernelGGL(obs_unpack_peers4_kernel, grid, dim3(ARR_BLOCK), 0, (hipStream_t)stream, packed_dev, (long long)n_env_time, A, D,
                       obs_dev, (long long)src_stride_floats);
  else
    hipLaunchKernelGGL(obs_unpack_peers1_kernel, grid, dim3(ARR_BLOCK), 0, (hipStream_t)stream, packed_dev, (long long)n_env_time, A, D,
                       obs_dev, (long long)src_stride_floats);
  return launched();
}

// ------------------------------------------------------------------------------------------------
// exact checkpoint: every device array of the handle, bit for bit
// ------------------------------------------------------------------------------------------------
struct CkptHeader {
  char magic[8];  // "DYNCKPT2"
  int32_t abi_version, n_arrays;
  dynenv_cfg_t cfg;
  uint64_t payload_bytes;
};
static size_t ckpt_payload(const dynenv* h) {
  size_t n = 0;
  for (size_t b : h->alloc_bytes) n += b;
  return n;
}
size_t dynenv_checkpoint_size(const dynenv_t* h) { return h ? sizeof(CkptHeader) + ckpt_payload(h) : 0; }

int dynenv_checkpoint_save(dynenv_t* h, void* buf_host, size_t nbytes) {
  if (!h || !buf_host) return fail(DYNENV_ERR_ARG, "null argument");
  if (nbytes < dynenv_checkpoint_size(h)) return fail(DYNENV_ERR_ARG, "checkpoint buffer too small");
  ON_DEVICE(h);
  HIP_OK(hipDeviceSynchronize());
  CkptHeader hd;
  memset(&hd, 0, sizeof(hd));
  memcpy(hd.magic, "DYNCKPT2", 8);
  hd.abi_version = DYNENV_ABI_VERSION; hd.n_arrays = (int32_t)h->allocs.size(); hd.cfg = h->cfg;
  hd.payload_bytes = ckpt_payload(h);
  char* out = (char*)buf_host;
  memcpy(out, &hd, sizeof(hd));
  out += sizeof(hd);
  for (size_t i = 0; i < h->allocs.size(); ++i) {
    HIP_OK(hipMemcpy(out, h->allocs[i], h->alloc_bytes[i], hipMemcpyDeviceToHost));
    out += h->alloc_bytes[i];
  }
  return DYNENV_OK;
}

int dynenv_checkpoint_load(dynenv_t* h, const void* buf_host, size_t nbytes) {
  if (!h || !buf_host) return fail(DYNENV_ERR_ARG, "null argument");
  ON_DEVICE(h);
  if (nbytes < sizeof(CkptHeader)) return fail(DYNENV_ERR_ARG, "not a checkpoint");
  CkptHeader hd;
  memcpy(&hd, buf_host, sizeof(hd));
  // (ABI 3 changed no array and no layout: checkpoints written by an ABI 2 library load)
  if (memcmp(hd.magic, "DYNCKPT2", 8) != 0 || (hd.abi_version != DYNENV_ABI_VERSION && hd.abi_version != 2)) return fail(DYNENV_ERR_ARG, "not a checkpoint of this ABI version");
  const dynenv_cfg_t& a = hd.cfg; const dynenv_cfg_t& b = h->cfg;
  if (a.env_type != b.env_type || a.num_envs != b.num_envs || a.n_players != b.n_players || a.obs_type != b.obs_type ||
      a.noise_type != b.noise_type || a.noise_magnitude != b.noise_magnitude || a.env_id_offset != b.env_id_offset || a.flags != b.flags)
    return fail(DYNENV_ERR_ARG, "checkpoint was taken from a differently configured handle");
  if (hd.n_arrays != (int32_t)h->allocs.size() || hd.payload_bytes != ckpt_payload(h) || nbytes < sizeof(hd) + hd.payload_bytes)
    return fail(DYNENV_ERR_ARG, "checkpoint layout does not match this build");
  if (h->captured && a.seed != b.seed) return frozen_seed("dynenv_checkpoint_load (the checkpoint was taken under another seed)");  // (nothing copied yet)
  HIP_OK(hipDeviceSynchronize());
  const char* in = (const char*)buf_host + sizeof(hd);
  // ABI 2 kept "an invalid action was seen" and, for Partial observations, "rows beyond the layout's capacity were dropped" in ONE bit
  // (1) of the per-environment error word, which is part of the checkpointed array; ABI 3 gave the second its own bit 3.  A set bit 1
  // of an ABI 2 blob of a Partial handle may mean either: it is loaded as both (nothing that was reported goes unreported).
  for (size_t i = 0; i < h->allocs.size(); ++i) {
    if (hd.abi_version == 2 && b.obs_type == DYNENV_OBS_PARTIAL && h->allocs[i] == (const void*)h->rows.err) {
      const size_t errStride = (size_t)h->rows.errStride, errWord = (size_t)h->rows.errIndex;
      std::vector<int> w(h->alloc_bytes[i] / sizeof(int));
      memcpy(w.data(), in, w.size() * sizeof(int));
      for (size_t e = 0; (e + 1) * errStride <= w.size(); ++e) if (w[e * errStride + errWord] & 2) w[e * errStride + errWord] |= 8;
      HIP_OK(hipMemcpy(h->allocs[i], w.data(), h->alloc_bytes[i], hipMemcpyHostToDevice));
    } else {
      HIP_OK(hipMemcpy(h->allocs[i], in, h->alloc_bytes[i], hipMemcpyHostToDevice));
    }
    in += h->alloc_bytes[i];
  }
  h->set_seed(a.seed);
  return h->checkpoint_loaded();
}

// diagnostics: one row of every routine of include/dynenv_math.h per input row (include/dynenv_math_probe.h), computed by the kernel of
// the unit asked for - this one (-O3) or the Driving unit (-Os): each carries its own compiled copy of the header and of dev_common.h's
// out-of-line wrappers.  Host buffers on both sides, the null stream, everything freed on every way out.
int dynenv_math_probe(int32_t unit, const double* in_host, int32_t n, double* out_host, int32_t device_id) {
  if (!in_host || !out_host) return fail(DYNENV_ERR_ARG, "null argument");
  if (n < 0) return fail(DYNENV_ERR_ARG, "negative row count");
  if (unit != DYNENV_MATH_UNIT_ROBOCUP && unit != DYNENV_MATH_UNIT_DRIVING) return fail(DYNENV_ERR_ARG, "unknown unit");
  if (n == 0) return DYNENV_OK;
  int ndev = 0;
  if (int rc = have_device(&ndev, "no HIP device visible")) return rc;
  if (device_id < 0 || device_id >= ndev) return fail(DYNENV_ERR_ARG, "device_id out of range");
  DeviceGuard guard_(device_id);
  if (!guard_.ok) return fail(DYNENV_ERR_HIP, "hipSetDevice failed");
  struct Bufs {
    double *in = nullptr, *out = nullptr;
    ~Bufs() { (void)hipFree(in); (void)hipFree(out); }
  } d;
  const size_t inBytes = sizeof(double) * DM_PROBE_NIN * (size_t)n, outBytes = sizeof(double) * DM_PROBE_NOUT * (size_t)n;
  HIP_OK(hipMalloc((void**)&d.in, inBytes));
  HIP_OK(hipMalloc((void**)&d.out, outBytes));
  HIP_OK(hipMemcpy(d.in, in_host, inBytes, hipMemcpyHostToDevice));
  if (unit == DYNENV_MATH_UNIT_DRIVING) {
    if (int rc = drv_math_probe_launch(d.in, n, d.out)) return rc;
  } else {
    hipLaunchKernelGGL(rc_math_probe_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, (const double*)d.in, (int)n, d.out);
    if (int rc = launched()) return rc;
  }
  HIP_OK(hipMemcpy(out_host, d.out, outBytes, hipMemcpyDeviceToHost));  // (waits for the kernel: the null stream)
  return DYNENV_OK;
}

}  // extern "C"

// device code only, behind everything above: no kernel a step launches moves (rc_layout_pad, robocup_kernels.hip)
#include "robocup_reset.hip"
#include "env_rows_kernels.hip"
#include "arranger_fixed_kernels.hip"
#include "arranger_embed_kernels.hip"   /* (with its entry point: dynenv_arrange_embed_pad) */
#include "attention_kernels.hip"        /* (with its entry point: dynenv_attend_pool) */
#include "recurrent_kernels.hip"        /* (with its entry point: dynenv_recurrent_head) */
#include "policy_kernels.hip"           /* (with its entry point: dynenv_policy_head) */
#include "rollout_kernels.hip"          /* (with its entry points: dynenv_rollout_insert, dynenv_rollout_returns) */
#include "icm_kernels.hip"              /* (with its entry point: dynenv_icm_losses) */
#include "icm_backward_kernels.hip"     /* (with its entry points: dynenv_icm_backward, dynenv_icm_backward_workspace) */
#include "policy_eval_kernels.hip"      /* (with its entry points: dynenv_policy_eval, dynenv_policy_eval_backward, dynenv_policy_eval_backward_workspace) */
// this unit's math probe: every routine of include/dynenv_math.h as compiled here (-O3), the row of include/dynenv_math_probe.h
extern "C" __global__ void __launch_bounds__(64) rc_math_probe_kernel(const double* in, int n, double* out) { dm_probe_wave(in, n, out); }
