// dynenv_host.h - the handle behind include/dynenv.h's dynenv_t: the part every environment type shares and the interface the entry
// points of dynenv_capi.hip call through, plus the host helpers both implementations use (robocup_host.hip in the dynenv_capi.hip
// unit, driving_tu.hip).  Host code only does allocation, constant upload and launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "dynenv.h"

#define HOST_LOCAL __attribute__((visibility("hidden"))) /* shared by the two units, not part of the library's ABI */
HOST_LOCAL int fail(int code, const std::string& msg);   // sets the calling thread's dynenv_last_error(), returns code (dynenv_capi.hip)
// the one "is there a device" test: DYNENV_OK, or DYNENV_ERR_NO_DEVICE with `msg`
HOST_LOCAL int have_device(int* ndev = nullptr, const char* msg = "no HIP device visible: libdynenv_hip has no CPU fallback");

// Every entry point runs on the handle's device and leaves the calling thread's current device as it found it (a process may
// hold handles on several devices next to torch's own current device).
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (prev >= 0) { int cur = -1; if (hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); } }
};
#define ON_DEVICE(h) DeviceGuard guard_((h)->cfg.device_id); if (!guard_.ok) return fail(DYNENV_ERR_HIP, "hipSetDevice failed")
#define HIP_OK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess)                                                                              \
      return fail(DYNENV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                 \
  } while (0)
static inline int launched() { HIP_OK(hipGetLastError()); return DYNENV_OK; }  // behind an entry point's (last) kernel launch

// The argument checks the model kernels' entry points share; `who` opens the message ("policy head: ...").  Each entry point calls them
// in its own order: argument errors, then what the kernel does not take, then the device.
// The discrete action groups of nvec[0 .. G-1] (G checked by the caller), packed as the kernels take them (mt_group, mma_tiles.h); C: the
// outputs that share the 32 rows with the N logits (the policy head's Box block), -1 where the call has none and its message names N alone.
struct ModelGroups {
  unsigned long long off = 0;   // 8 bits per group: the first logit of group g
  unsigned n = 0;               // 4 bits per group: n_g - 1
  int N = 0;
};
static inline int model_groups(const char* who, const int32_t* nvec, int G, int action_cols, ModelGroups& out, int C = -1) {
  out = ModelGroups();
  for (int g = 0; g < G; ++g) {
    if (nvec[g] < 1 || nvec[g] > 16) return fail(DYNENV_ERR_ARG, std::string(who) + ": a group has 1..16 actions");
    out.off |= (unsigned long long)out.N << (8 * g);
    out.n |= (unsigned)(nvec[g] - 1) << (4 * g);
    out.N += nvec[g];
  }
  if (out.N + (C < 0 ? 0 : C) > DYNENV_POLICY_ROWS) return fail(DYNENV_ERR_ARG, std::string(who) + (C < 0 ? ": N is at most 32" : ": N + C is at most 32"));
  if (action_cols < G || action_cols > 8) return fail(DYNENV_ERR_ARG, std::string(who) + ": action_cols is G..8");
  return DYNENV_OK;
}
static inline int model_aligned(const char* who, std::initializer_list<const void*> ptrs, unsigned bytes) {   // (NULL passes)
  for (const void* q : ptrs)
    if ((uintptr_t)q % bytes) return fail(DYNENV_ERR_ARG, std::string(who) + ": buffers must be " + std::to_string(bytes) + "-byte aligned");
  return DYNENV_OK;
}
// the operands' type: an argument error unless it is one of the three, ...
static inline int model_operand_dtype(const char* who, int32_t w_dtype) {
  if (w_dtype < DYNENV_ARR_F32 || w_dtype > DYNENV_ARR_F16) return fail(DYNENV_ERR_ARG, std::string(who) + ": unknown dtype (DYNENV_ARR_BF16 or _F16)");
  return DYNENV_OK;
}
// ... and, behind the argument errors, unsupported where it is float32; `fused`: "layer" or "backward"
static inline int model_operand_16bit(const char* who, int32_t w_dtype, const char* fused) {
  if (w_dtype == DYNENV_ARR_F32) return fail(DYNENV_ERR_UNSUPPORTED, std::string(who) + ": the fused " + fused + " takes bf16 or fp16 operands");
  return DYNENV_OK;
}

// One description of a handle's per-environment rows: every checkpointed array of the shape [fields][E][row], in allocation order
// (alloc_rows below).  env_rows_save_kernel / env_rows_load_kernel (env_rows_kernels.hip, in the dynenv_capi.hip unit) take it by value
// and copy an environment's rows to / from an exact blob: a 16-byte header (the layout tag, then zeros), then every array's rows
// field-major at blobOff, each array's part padded with zero words to a multiple of 16 bytes.  A "unit" is one access of 1 << wlog
// bytes: 16 or 8 where the row's size allows (bases come from hipMalloc, blobs are 16-byte aligned and each part starts 16-byte
// aligned), else 4.
#define ENV_ROWS_MAX 16
struct EnvRowArr {
  char* base;
  unsigned long long fieldStride;   // bytes between two fields = E * rowBytes
  uint32_t rowBytes, blobOff;       // bytes of one environment's row of one field; where the array's rows start in the blob
  uint32_t unitsPerRow, units;      // units of one row, and of all `fields` rows
  uint16_t fields, elemBytes;
  uint8_t wlog, trips, padWords, next;  // trips = wave iterations = ceil(units / 64); padWords = zero words behind the rows (the kernel takes them from padAt); next array of this wlog (n: none)
};
struct EnvRowTable {
  int n, E;
  int errStride, errIndex;          // the environment's error word: err[e * errStride + errIndex]
  int* err;
  unsigned long long tag;           // layout tag: never 0, so a zero-filled buffer is no blob
  uint32_t blobBytes;               // dynenv_exact_size
  int first[3];                     // first array whose wlog is 4, 3, 2 (n: none)
  int nPad;                         // the zero words behind the arrays' parts, all of them: lane l < nPad writes the word at byte padAt[l]
  uint32_t padAt[3 * ENV_ROWS_MAX];
  EnvRowArr arr[ENV_ROWS_MAX];
};

struct HOST_LOCAL dynenv {
  dynenv_cfg_t cfg;
  int A = 0, obs_dim = 0, T = 0, action_dim = 0;
  int full_dim = 0, global_dim = 0;  // widths of the rows dynenv_full_obs / dynenv_global_state write (0: there is no such row)
  size_t state_bytes = 0;            // size of the canonical per-environment blob of dynenv_get_state / dynenv_set_state
  std::vector<void*> allocs;
  std::vector<size_t> alloc_bytes;  // checkpoint = these arrays, in allocation order
  std::vector<void*> scratch;       // scheduling scratch (SIMD-isolation lists), `stage`: NOT simulation state, never checkpointed
  // the per-environment arrays among `allocs` (alloc_rows), completed by rows_finish(), and - set by init() - where the kernels keep the
  // per-environment error word: rows.err[env * rows.errStride + rows.errIndex] (rows.err is one of `allocs`)
  EnvRowTable rows = {};
  // where dynenv_get_state / dynenv_set_state keep their one blob on the device: state_bytes, then the status word (dynenv_create;
  // a handle is used by one thread at a time: dynenv.h)
  unsigned long long* stage = nullptr;
  hipEvent_t ev_begin = nullptr, ev_main = nullptr, ev_end = nullptr;  // dynenv_set_step_events (caller-owned)
  // set by the first step or masked reset issued on a capturing stream, for the rest of the handle's life: the seed is a by-value
  // kernel argument, so a replay draws from the seed of the capture whatever the handle holds by then - from here on dynenv_seed and
  // dynenv_checkpoint_load refuse any other seed (dynenv_capi.hip)
  bool captured = false;
  void note_capture(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!captured && hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) captured = true;
  }

  virtual ~dynenv() {  // (on the handle's device: dynenv_destroy)
    for (void* p : allocs) (void)hipFree(p);
    for (void* p : scratch) (void)hipFree(p);
  }
  // what dynenv_create, after checking cfg, leaves to the environment: the sizes above, allocations (their ORDER is the checkpoint format), constants
  virtual int init() = 0;
  virtual void layout(dynenv_layout_t& L) const = 0;  // the block table and steps_per_episode
  virtual void set_seed(uint64_t seed) = 0;
  // the reset: every environment (mask == nullptr: dynenv_reset) or exactly the environments e with mask[e] != 0 (device uint8 [E]); one
  // wave per environment, nothing but launches on `st` (capturable behind a captured step); the scheduler's scratch is not touched
  virtual int reset_masked(const uint8_t* mask, float* obs, hipStream_t st) = 0;
  // the step of every environment (mask == nullptr: dynenv_step / dynenv_step_head) or of exactly the environments e with mask[e] != 0
  // (device uint8 [E], read by the step kernel: dynenv_step_masked), the others left byte for byte as they are;
  // records ev_begin in front of the step's dominant kernel and ev_main right behind it (step_begin / step_main_done)
  virtual int step(const uint8_t* mask, const int* actions, const double* head, float* obs, double* rewards, uint8_t* dones, hipStream_t st) = 0;
  virtual int full_obs(float* full, hipStream_t st) = 0;
  virtual int global_state(float* state, hipStream_t st) = 0;
  virtual int counts(int32_t* out, hipStream_t st) = 0;
  virtual int episode_stats(double* ep_r, double* ep_pos_r, double* ep_obs_r, int32_t* goals, hipStream_t st) = 0;
  // state transfer: n blobs state_bytes apart in device memory, one launch on `st`, no host synchronisation, allocation or copy.
  // idx (device; nullptr: environments first..first + n - 1) and n are checked by the entry point as far as the host can see them; the
  // kernels skip an index outside [0, E).  status (may be nullptr): int32 [n] = 0 written, 1 blob rejected, 2 index out of range;
  // raise: a rejected blob also raises error bit 6 on its environment.  dynenv_get_state / dynenv_set_state are these for n = 1.
  virtual int get_states(const int32_t* idx, int32_t first, int32_t n, void* blobs, hipStream_t st) = 0;
  virtual int set_states(const int32_t* idx, int32_t first, int32_t n, const void* blobs, int32_t* status, bool raise, hipStream_t st) = 0;
  virtual int error_flags_env(int32_t* flags, hipStream_t st) = 0;  // int32 [E]: every environment's error word
  virtual int debug_counters(int64_t* out16) = 0;
  virtual int debug_placement(uint32_t*, int32_t) { return 0; }  // (Driving's SIMD isolation only: 0 words recorded)
  virtual int checkpoint_loaded() { return DYNENV_OK; }      // behind dynenv_checkpoint_load's copies

  int step_begin(hipStream_t st) { if (ev_begin) HIP_OK(hipEventRecord(ev_begin, st)); return 0; }
  void step_main_done(hipStream_t st) { if (ev_main) (void)hipEventRecord(ev_main, st); }

  // zeroed device memory: part of the checkpoint, or (scratch) not part of the simulation state - never saved / restored
  template <typename X>
  int alloc(X** out, size_t count, bool is_scratch = false) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, count * sizeof(X)));
    HIP_OK(hipMemset(p, 0, count * sizeof(X)));
    if (is_scratch) scratch.push_back(p);
    else { allocs.push_back(p); alloc_bytes.push_back(count * sizeof(X)); }
    *out = (X*)p;
    return 0;
  }
  // a checkpointed array of the shape [fields][E][rowElems]: alloc() of that many elements, and one entry of the row table
  template <typename X>
  int alloc_rows(X** out, size_t fields, size_t rowElems) {
    const size_t E = (size_t)cfg.num_envs;
    if (rows.n >= ENV_ROWS_MAX || fields > 0xFFFF || sizeof(X) > 0xFFFF || rowElems * sizeof(X) % 4 || rowElems * sizeof(X) > 0x7FFFFFFF)
      return fail(DYNENV_ERR_HIP, "internal: a per-environment array does not fit the row table");
    if (int rc = alloc(out, fields * E * rowElems)) return rc;
    EnvRowArr& a = rows.arr[rows.n++];
    a.base = (char*)*out; a.rowBytes = (uint32_t)(rowElems * sizeof(X)); a.fieldStride = (unsigned long long)E * a.rowBytes;
    a.fields = (uint16_t)fields; a.elemBytes = (uint16_t)sizeof(X);
    return 0;
  }
  // behind init(): access widths, blob offsets and the layout tag - a function of the configuration's env_type, n_players, obs_type and
  // flags and of every array's shape, NOT of num_envs, env_id_offset, seed or noise: a blob fits any handle of the same configuration
  int rows_finish() {
    unsigned long long tag = 0xcbf29ce484222325ull;  // FNV-1a over 32-bit words
    auto mix = [&tag](uint32_t w) { for (int k = 0; k < 4; ++k) { tag ^= (w >> (8 * k)) & 0xFF; tag *= 0x100000001b3ull; } };
    mix(0x58455644u /* "DVEX" */); mix((uint32_t)cfg.env_type); mix((uint32_t)cfg.n_players); mix((uint32_t)cfg.obs_type); mix((uint32_t)cfg.flags);
    size_t off = 16;
    rows.nPad = 0;
    for (int i = 0; i < rows.n; ++i) {
      EnvRowArr& a = rows.arr[i];
      a.wlog = a.rowBytes % 16 == 0 ? 4 : a.rowBytes % 8 == 0 ? 3 : 2;
      a.unitsPerRow = a.rowBytes >> a.wlog; a.units = a.unitsPerRow * a.fields;
      const size_t bytes = (size_t)a.rowBytes * a.fields, trips = (a.units + 63) / 64;
      if (trips > 0xFF || off + bytes + 16 > 0x7FFFFFFF) return fail(DYNENV_ERR_HIP, "internal: a per-environment array does not fit the row table");
      a.trips = (uint8_t)trips; a.blobOff = (uint32_t)off; a.padWords = (uint8_t)((16 - bytes % 16) % 16 / 4);
      for (int k = 0; k < a.padWords; ++k) rows.padAt[rows.nPad++] = (uint32_t)(off + bytes) + 4 * k;
      off += bytes + 4 * a.padWords;
      mix(a.fields); mix(a.rowBytes); mix(a.elemBytes);
    }
    for (int w = 0; w < 3; ++w) {  // the arrays of one access width, chained in table order
      int prev = -1;
      rows.first[w] = rows.n;
      for (int i = 0; i < rows.n; ++i) {
        if (rows.arr[i].wlog != 4 - w) continue;
        if (prev < 0) rows.first[w] = i; else rows.arr[prev].next = (uint8_t)i;
        rows.arr[i].next = (uint8_t)rows.n;
        prev = i;
      }
    }
    rows.E = cfg.num_envs;
    rows.tag = tag ? tag : 1; rows.blobBytes = (uint32_t)off;
    return 0;
  }
};
enum { SCRATCH = 1 };

// blocks of an observation row, one behind the other unless `off` says where: fills L's table (if given), returns the summed width
static inline int row_blocks(dynenv_layout_t* L, int n, const int* rows, const int* feat, const int* off = nullptr) {
  int w = 0;
  for (int i = 0; i < n; ++i) {
    if (L) { L->n_blocks = n; L->block_offset[i] = off ? off[i] : w; L->block_rows[i] = rows[i]; L->block_feat[i] = feat[i]; }
    w += rows[i] * feat[i];
  }
  return w;
}

// -DDRV_PROFILE builds: a profile symbol of N counters, `cols` per row -> <name>.txt in the directory DYNENV_PROFILE_DIR names (the profile
// tools set it: tools/contact_profile.py, robocup_profile.py, vision_profile.py; unset: the current directory), a blank behind every
// counter of a row (a single column: none), one row per line
template <size_t N>
static int prof_dump(const unsigned long long (&sym)[N], const char* name, size_t cols) {
  std::vector<unsigned long long> d(N);
  HIP_OK(hipMemcpyFromSymbol(d.data(), HIP_SYMBOL(sym), N * sizeof(unsigned long long)));
  const char* dir = getenv("DYNENV_PROFILE_DIR");
  FILE* f = fopen((std::string(dir ? dir : ".") + "/" + name + ".txt").c_str(), "w");
  if (!f) return fail(DYNENV_ERR_ARG, std::string("cannot write the profile dump ") + name + ".txt");
  for (size_t k = 0; k < N; ++k) fprintf(f, cols == 1 ? "%llu\n" : ((k + 1) % cols ? "%llu " : "%llu \n"), d[k]);
  fclose(f);
  return 0;
}
