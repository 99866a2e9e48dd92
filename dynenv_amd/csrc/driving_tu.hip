// driving_tu.hip - the Driving translation unit: the kernels of driving_kernels.hip / driving_partial.hip and the Driving handle, i.e.
// all of their host code (constants, allocation, the isolation scheduler, launches, diagnostics).
// Compiled with -Os (dynenv_amd/build.py; driving_host.h says why), linked with dynenv_capi.hip.
#include <hip/hip_runtime.h>

#include "driving_kernels.hip"
#include "driving_partial.hip"
#include "driving_reset.hip"
#include "dynenv_host.h"

#define ISO_PROBE_EVERY 64     /* steps between two looks at the device's validation counter (an asynchronous 4-byte copy) */
#define ISO_PAUSE_STEPS 2048   /* steps without isolation after a probe window in which more than half of the launches did not validate */

// ---------------------------------------------------------------------------------------------- constants
static void road_init_host(DrvRoad& r, int nLanes, double width, V2 p0, V2 p1) {  // Road.py:11-33
  V2 d = vsub(p1, p0);
  r.nLanes = nLanes; r.width = width; r.p0 = p0; r.p1 = p1; r.followDist = 90.0;
  r.length = vlen(d);
  r.dir = v2(d.x / r.length, d.y / r.length);
  r.normal = vrot_angle(r.dir, DM_PI / 2.0);
  r.dirAngle = dm_atan2(r.dir.y, r.dir.x);
  r.cosDir0 = dm_cos(r.dirAngle - 0.0);
  double k = (double)(nLanes + 1) * width;
  r.walk[0][0] = vadd(p0, vmul(r.normal, k)); r.walk[0][1] = vadd(p1, vmul(r.normal, k));
  r.walk[1][0] = vsub(p0, vmul(r.normal, k)); r.walk[1][1] = vsub(p1, vmul(r.normal, k));
}

static double moment_for_box(double m, double hx, double hy) {  // cpMomentForPoly on Car.points (Car.py:21-23)
  V2 verts[4] = {v2(hx, hy), v2(-hx, hy), v2(-hx, -hy), v2(hx, -hy)};
  double sum1 = 0.0, sum2 = 0.0;
  for (int i = 0; i < 4; ++i) {
    V2 a1 = verts[i], a2 = verts[(i + 1) % 4];
    double a = vcross(a2, a1);
    double b = vdot(a1, a1) + vdot(a1, a2) + vdot(a2, a2);
    sum1 += a * b; sum2 += a;
  }
  return (m * sum1) / (6.0 * sum2);
}

static void build_consts(DrvConst& c) {
  memset(&c, 0, sizeof(c));
  road_init_host(c.roads[0], 2, 35.0, v2(875.0, 0.0), v2(875.0, 1000.0));  // DrivingEnvironment.py:110-115
  road_init_host(c.roads[1], 1, 35.0, v2(0.0, 500.0), v2(1750.0, 500.0));
  // lane rows of getFullState (:689-695) incl. the negative-index quirk `Lanes[i - nLanes]`
  int row = 0;
  for (int r = 0; r < 2; ++r) {
    const DrvRoad& l = c.roads[r];
    int n = l.nLanes, cnt = 2 * n + 1;
    for (int i = -n; i <= n; ++i) {
      int idx = ((i - n) % cnt + cnt) % cnt;
      double s = (double)(idx - n) * l.width;
      V2 a = vadd(l.p0, vmul(l.normal, s)), b = vadd(l.p1, vmul(l.normal, s));
      c.laneRows[row * 5 + 0] = (float)normalize_obs(a.x, STD_NORM_X, 0.0);
      c.laneRows[row * 5 + 1] = (float)normalize_obs(a.y, STD_NORM_Y, 0.0);
      c.laneRows[row * 5 + 2] = (float)normalize_obs(b.x, STD_NORM_X, 0.0);
      c.laneRows[row * 5 + 3] = (float)normalize_obs(b.y, STD_NORM_Y, 0.0);
      c.laneRows[row * 5 + 4] = (float)((i == n || i == -n) ? 1 : (i == 0 ? -1 : 0));
      ++row;
    }
  }
  const double masses[4] = {1200, 1800, 3500, 5000}, widths[4] = {5, 6, 7, 8}, lengths[4] = {10, 15, 20, 25},
               powers[4] = {3, 4, 3, 4};  // Car.py:9-12
  for (int t = 0; t < 4; ++t) {
    c.carMass[t] = masses[t]; c.carHx[t] = lengths[t]; c.carHy[t] = widths[t]; c.carPower[t] = powers[t];
    c.carInertia[t] = moment_for_box(masses[t], lengths[t], widths[t]);
  }
  c.pedMass = 90.0;  // Pedestrian.py:11-14
  c.pedInertia = 90.0 * (0.5 * (0.0 * 0.0 + DRV_PED_R * DRV_PED_R) + 0.0);
}

// the device code spells the road constants as literals (RoadK<R>): they must equal the computed ones bit for bit
template <int R>
static bool road_literals_ok(const DrvRoad& r) {
  return r.p0.x == RoadK<R>::p0x && r.p0.y == RoadK<R>::p0y && r.dir.x == RoadK<R>::dirx && r.dir.y == RoadK<R>::diry &&
         (double)r.nLanes * r.width + 5.0 == RoadK<R>::lat && r.length == RoadK<R>::length &&
         r.dirAngle == RoadK<R>::dirAngle && r.cosDir0 == RoadK<R>::cosDir0 && r.normal.x == RoadK<R>::nx &&
         r.normal.y == RoadK<R>::ny;
}

// ... and so are the car-type constants (CarK)
static bool car_literals_ok(const DrvConst& c) {
  const double m[4] = {CarK::carMass0, CarK::carMass1, CarK::carMass2, CarK::carMass3}, hx[4] = {CarK::carHx0, CarK::carHx1, CarK::carHx2, CarK::carHx3};
  const double hy[4] = {CarK::carHy0, CarK::carHy1, CarK::carHy2, CarK::carHy3}, pw[4] = {CarK::carPower0, CarK::carPower1, CarK::carPower2, CarK::carPower3};
  const double in[4] = {CarK::carInertia0, CarK::carInertia1, CarK::carInertia2, CarK::carInertia3};
  for (int t = 0; t < 4; ++t)
    if (c.carMass[t] != m[t] || c.carHx[t] != hx[t] || c.carHy[t] != hy[t] || c.carPower[t] != pw[t] || c.carInertia[t] != in[t]) return false;
  return c.pedMass == CarK::pedMass && c.pedInertia == CarK::pedInertia;
}
static bool drv_literals_ok(const DrvConst& c) { return road_literals_ok<0>(c.roads[0]) && road_literals_ok<1>(c.roads[1]) && car_literals_ok(c); }

// ---------------------------------------------------------------------------------------------- the handle
// the Full row: self 9 | the other cars (A - 1) x 7 | obstacles x 4 | pedestrians x 2 | lane rows x 5; returns its width
static int drv_full_row(int A, dynenv_layout_t* L = nullptr) {
  const int rows[5] = {1, A - 1, DRV_MAXO, DRV_MAXP, DRV_LANE_ROWS}, feat[5] = {9, 7, 4, 2, 5};
  return row_blocks(L, 5, rows, feat);
}

struct HOST_LOCAL DrvHandle final : dynenv {
  DrvState S;
  bool partial = false;
  // SIMD isolation, host side: iso_cfg = the mode the handle was created with (S.iso_on may be 0 while isolation is paused);
  // iso_seen = pinned word the device's count of launches whose placement did not validate is copied into now and then
  int iso_cfg = 0, iso_last_invalid = 0, iso_pauses = 0;
  long long steps = 0, iso_paused_until = 0;
  int* iso_seen = nullptr;

  ~DrvHandle() override { if (iso_seen) (void)hipHostFree(iso_seen); }

  // the SIMD-isolation scheduler starts from scratch: empty lists, placement "not validated yet", no environment "done"
  int iso_clear(bool async, hipStream_t st) {  // async: stream-ordered
    auto set = [=](void* p, int v, size_t n) { return async ? hipMemsetAsync(p, v, n, st) : hipMemset(p, v, n); };
    S.tick = 0;
    HIP_OK(set(S.iso, 0, sizeof(int) * DRV_ISO_WORDS));
    HIP_OK(set(S.iso_done, 0xFF, sizeof(int) * (size_t)S.E));
    HIP_OK(set(S.iso_hw, 0xFF, sizeof(unsigned) * 2 * 4 * DRV_ISO_GROUPS));
    return 0;
  }
  // ... at creation and behind a checkpoint load, where both deferred-observation lists are emptied as well
  int iso_reset() {
    if (iso_clear(false, nullptr)) return DYNENV_ERR_HIP;
    HIP_OK(hipMemset(S.pvq, 0, sizeof(int) * DRV_PVQ_IDS));
    S.pv_par = 0;
    return 0;
  }

  int init() override {
    A = cfg.n_players > DRV_MAXA ? DRV_MAXA : cfg.n_players;  // environment_base.py:57
    partial = cfg.obs_type == DYNENV_OBS_PARTIAL;
    full_dim = drv_full_row(A); global_dim = 0; state_bytes = sizeof(dynenv_driving_state_t);
    obs_dim = partial ? PV_DIM : full_dim; T = 1; action_dim = 2;
    memset(&S, 0, sizeof(S));
    const size_t E = (size_t)cfg.num_envs;
    S.E = (int)E; S.A = A; S.obs_dim = full_dim; S.seed = cfg.seed; S.env_id_offset = cfg.env_id_offset;
    int rc = 0;
    // (every checkpointed array is per-environment, [fields][E][row]: the row table of dynenv_get_exact / dynenv_set_exact)
    rc |= alloc_rows(&S.body, BF_COUNT, DRV_NB);
    rc |= alloc_rows(&S.carx, CF_COUNT, 16);
    rc |= alloc_rows(&S.flags, 1, DRV_NB);
    rc |= alloc_rows(&S.aux, 1, DRV_NB);
    rc |= alloc_rows(&S.obst, 2, DRV_MAXO);
    rc |= alloc_rows(&S.envi, 1, EI_COUNT);
    rc |= alloc_rows(&S.epr, 2, 16);
    rc |= alloc_rows(&S.s_pair, 1, DRV_NS);
    rc |= alloc_rows(&S.s_meta, 1, DRV_NS);
    rc |= alloc_rows(&S.s_hash, 2, DRV_NS);
    rc |= alloc_rows(&S.s_imp, 4, DRV_NS);
    rc |= alloc_rows(&S.lastcand, 1, 64);
    rc |= alloc(&S.iso, DRV_ISO_WORDS, SCRATCH);
    rc |= alloc(&S.iso_done, E, SCRATCH);
    rc |= alloc(&S.iso_hw, 2 * 4 * DRV_ISO_GROUPS, SCRATCH);
    rc |= alloc(&S.pvq, DRV_PVQ_WORDS((size_t)S.E), SCRATCH);
    if (rc) return DYNENV_ERR_HIP;
    rows.err = S.envi; rows.errStride = EI_COUNT; rows.errIndex = EI_ERR;
    {
      // The slowest environments of the previous step get a SIMD to themselves (drv_iso_assign): only where the block -> SIMD
      // pattern it relies on was measured - 4096 environments = one residency round of a 256-CU device, four waves per SIMD.
      hipDeviceProp_t prop;
      S.iso_on = 0;
      if (hipGetDeviceProperties(&prop, cfg.device_id) == hipSuccess)
      {
        const bool dev256 = prop.multiProcessorCount * 4 == DRV_ISO_GROUPS, off = getenv("DYNENV_NO_ISOLATION") != nullptr;
        // 1: isolation - one residency round, Full observations (Partial: the fused observation makes the displaced environments
        //    too long for the second round: +1.4 %);  2: more environments than fit at once - the slow ones simply start first;
        // 3: Partial observations - nothing is rescheduled, the step's slowest environment is timed all the same: an environment on
        //    the contact path runs as many of its own vision passes as fit before that one is done (drv_step_body)
        // (round 5: mode 1 for every E in (DRV_ISO_MIN_E, 4096], not for E == 4096 alone - the launch is 4096 regular blocks + spares
        //  whatever E is, and the blocks without an environment end at once; below DRV_ISO_MIN_E a SIMD holds two waves or fewer)
        const int isoMinE = getenv("DYNENV_ISO_MIN_E") ? atoi(getenv("DYNENV_ISO_MIN_E")) : DRV_ISO_MIN_E;
        S.iso_on = off || !dev256 ? 0 : ((int)E > isoMinE && E <= 4 * DRV_ISO_GROUPS ? (partial ? 0 : 1) : (E > 4 * DRV_ISO_GROUPS ? 2 : 0));
        if (!off && S.iso_on == 0 && partial) S.iso_on = 3;
      }
      if (iso_reset()) return DYNENV_ERR_HIP;
      iso_cfg = S.iso_on;
      if (S.iso_on == 1) {
        if (hipHostMalloc((void**)&iso_seen, sizeof(int), hipHostMallocDefault) != hipSuccess) return fail(DYNENV_ERR_HIP, "hipHostMalloc");
        *iso_seen = 0;
      }
    }
    DrvConst c;
    build_consts(c);
    if (!drv_literals_ok(c)) return fail(DYNENV_ERR_HIP, "internal: RoadK / CarK literals differ from the computed constants");
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(C), &c, sizeof(c));
    if (e != hipSuccess) return fail(DYNENV_ERR_HIP, hipGetErrorString(e));
    return DYNENV_OK;
  }

  void layout(dynenv_layout_t& L) const override {
    L.steps_per_episode = DRV_MAX_TIME / 10;
    if (!partial) { drv_full_row(A, &L); return; }
    // ((cars, obstacles, pedestrians), (self, lanes)) of getAgentVision + the 4 row counts
    const int off[6] = {0, PV_OFF_CARS, PV_OFF_OBST, PV_OFF_PEDS, PV_OFF_LANES, PV_DIM - 4};
    const int rows[6] = {1, PV_CAP_CARS, PV_CAP_OBST, PV_CAP_PEDS, PV_CAP_LANES, 1}, feat[6] = {9, 7, 6, 2, 4, 4};
    row_blocks(&L, 6, rows, feat, off);
  }

  void set_seed(uint64_t seed) override { cfg.seed = seed; S.seed = seed; }

  int reset_masked(const uint8_t* mask, float* obs, hipStream_t st) override {
    note_capture(st);
    hipLaunchKernelGGL(drv_reset_masked_kernel, dim3(S.E), dim3(64), 0, st, S, mask);
    if (obs && partial)
      hipLaunchKernelGGL(drv_partial_obs_kernel, dim3(S.E), dim3(64), 0, st, S, mask, (int)cfg.noise_type, cfg.noise_magnitude, obs);
    else if (obs)
      hipLaunchKernelGGL(drv_obs_kernel, dim3(S.E), dim3(64), 0, st, S, mask, obs);
    return launched();
  }

  int full_obs(float* full, hipStream_t st) override {
    hipLaunchKernelGGL(drv_obs_kernel, dim3(S.E), dim3(64), 0, st, S, (const uint8_t*)nullptr, full);
    return launched();
  }
  int global_state(float*, hipStream_t) override {
    return fail(DYNENV_ERR_UNSUPPORTED, "Driving: getFullState(None) is made of columns of dynenv_full_obs (every car's own self block); no separate emit");
  }

  int step(const uint8_t* mask, const int* actions, const double* head, float* obs, double* rewards, uint8_t* dones, hipStream_t st) override {
    if (head) return fail(DYNENV_ERR_ARG, "the continuous head channel exists for RoboCup with DYNENV_FLAG_ALLOW_HEAD_TURN only");
    // Partial: getAgentVision for every agent (DrivingEnvironment.py:294) is fused into the step kernel - each wave writes its
    // environment's observation as soon as its step is done, which fills the launch's tail
    // (with isolation on, 3 x DRV_ISO_MAX spare blocks behind the E regular ones: the environments displaced from a slow
    //  environment's SIMD run there - or nothing, and the block ends at once)
    // A device this handle does not have to itself (another handle stepping on another stream, another kernel): the placement
    // does not validate, isolation holds off on the device - and what is left of it (the spare blocks, the placement record, the
    // per-environment report) still costs 0.5-0.9 % of a step.  So the host looks at the device's count of
    // launches that did not validate every ISO_PROBE_EVERY steps - an asynchronous 4-byte copy, read one window later, never
    // waited for - and when more than half of a window's launches did not validate it drops to the plain launch (mode 0: exactly
    // what DYNENV_NO_ISOLATION=1 gives) for ISO_PAUSE_STEPS steps, then starts isolation over.  Scheduling only, as ever.
    // A step that is being CAPTURED into a hipGraph will be replayed with frozen kernel arguments, and none of the host logic below
    // runs at replay: from the first captured step on, for good, the handle keeps tick / pv_par in two device words that a one-thread
    // kernel advances in front of every step (eager steps included: ~2 us each), the isolation pause logic is off (the device-side
    // validation still holds isolation off on a shared device), and a paused isolation stays paused.
    if (!S.tick_src) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) { S.tick_src = 1; captured = true; }  // (the one query serves both)
    }
    if (S.tick_src) hipLaunchKernelGGL(drv_tick_advance_kernel, dim3(1), dim3(64), 0, st, S, (partial && obs) ? 1 : 0);
    if (step_begin(st)) return DYNENV_ERR_HIP;  // (behind the advance kernel: the event window is the step kernel's own duration)
    if (iso_cfg == 1 && !S.tick_src) {
      steps += 1;
      if (S.iso_on == 0 && steps >= iso_paused_until) {
        if (iso_clear(true, st)) return DYNENV_ERR_HIP;  // (resuming isolation between two steps)
        S.iso_on = 1; iso_last_invalid = 0; *iso_seen = 0;
      } else if (S.iso_on == 1 && steps % ISO_PROBE_EVERY == 0) {
        const int seen = *(volatile int*)iso_seen;  // the copy issued one window ago (stale at worst)
        if (seen - iso_last_invalid > ISO_PROBE_EVERY / 2) {
          S.iso_on = 0; iso_paused_until = steps + ISO_PAUSE_STEPS; iso_pauses += 1;
        } else {
          iso_last_invalid = seen;
          HIP_OK(hipMemcpyAsync(iso_seen, S.iso + DRV_ISOW_INVALID, sizeof(int), hipMemcpyDeviceToHost, st));
        }
      }
    }
    const unsigned stepGrid = S.iso_on == 1 ? 4u * DRV_ISO_GROUPS + 3u * DRV_ISO_MAX + 1u /* one residency round + spares + the placement validator */ : (unsigned)S.E;
    if (!S.tick_src) S.tick = (S.tick + 1) % DRV_TICK_WRAP;
    if (partial && obs)
    {
      if (!S.tick_src) S.pv_par ^= 1;
      hipLaunchKernelGGL(drv_step_partial_kernel, dim3(stepGrid), dim3(64), 0, st, S, mask, actions, rewards, dones, obs,
                         (int)cfg.noise_type, (double)cfg.noise_magnitude);
      step_main_done(st);
      // one block per (listed environment, agent) in turn, over a grid that fits the device at once: the step launch left a list
      const long long items = (long long)S.E * S.A;
      hipLaunchKernelGGL(drv_partial_obs_deferred_kernel, dim3((unsigned)(items < 4096 ? items : 4096)), dim3(64), 0, st, S,
                         (int)cfg.noise_type, (double)cfg.noise_magnitude, obs);
    }
    else {
      hipLaunchKernelGGL(drv_step_kernel, dim3(stepGrid), dim3(64), 0, st, S, mask, actions, partial ? (float*)nullptr : obs, rewards, dones);
      step_main_done(st);
    }
    return launched();
  }

  int counts(int32_t* out, hipStream_t st) override {
    hipLaunchKernelGGL(drv_counts_kernel, dim3((S.E + 63) / 64), dim3(64), 0, st, S, (int*)out);
    return launched();
  }
  int episode_stats(double* ep_r, double* ep_pos_r, double* ep_obs_r, int32_t* goals, hipStream_t st) override {
    hipLaunchKernelGGL(drv_stats_kernel, dim3((S.E + 63) / 64), dim3(64), 0, st, S, ep_r, ep_pos_r, ep_obs_r, (int*)goals);
    return launched();
  }

  // diagnostics: per-path substep counts since the last reset, summed over envs: out8 = {fast, quiescent, contact,
  // slot-sum, contact-because-candidates-changed, -because-a-body-moved, -because-an-arbiter-was-not-inert,
  // steady replays, 0...}
  int debug_counters(int64_t* out4) override {
    HIP_OK(hipDeviceSynchronize());
    std::vector<int> envi((size_t)S.E * EI_COUNT);
    HIP_OK(hipMemcpy(envi.data(), S.envi, envi.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) out4[k] = 0;
    for (int e = 0; e < S.E; ++e)
      for (int k = 0; k < 10; ++k) out4[k] += envi[(size_t)e * EI_COUNT + EI_N_FAST + k];
    {  // SIMD isolation: how many environments the next step isolates, placeholders that gave up waiting (should stay 0)
      int iso[DRV_ISO_HDR];
      HIP_OK(hipMemcpy(iso, S.iso, sizeof(iso), hipMemcpyDeviceToHost));
      const int nxt = ((S.tick_src ? iso[DRV_ISOW_TICK] : S.tick) + 1) % 3, k = iso[DRV_ISOW_LEN + nxt];
      const int cap = S.iso_on == 1 ? DRV_ISO_MAX : DRV_ISO_LIST;
      out4[10] = S.iso_on ? (k < cap ? k : cap) : -1; out4[11] = iso[DRV_ISOW_GAVE_UP];
      // out[12]: scheduling mode (0 off, 1 SIMD isolation, 2 slow environments first, 3 timing only: Partial); out[13]: 1 = the next step found the block ->
      // SIMD placement validated (mode 1 only; 0 = isolation is holding off); out[14]: launches whose placement did not validate
      out4[12] = iso_cfg; out4[13] = S.iso_on == 1 ? iso[DRV_ISOW_VALID + nxt] : (iso_cfg == 1 ? 0 : -1); out4[14] = iso[DRV_ISOW_INVALID];
      out4[15] = iso_pauses;  // times the host dropped to the plain launch because the placement kept failing to validate
    }
#ifdef DRV_PROFILE
    if (prof_dump(g_dbgr, "dbgr", 1) || prof_dump(g_dbgw, "dbgw", 12) || prof_dump(g_dbgp, "dbgp", 8) || prof_dump(g_dbgs, "dbgs", 8) ||
        prof_dump(g_pvprof, "dbgv", 16) || prof_dump(g_dbgl, "dbgl", 8))
      return DYNENV_ERR_HIP;
#endif
    return DYNENV_OK;
  }

  // diagnostics: where the blocks of the last Driving step ran (XCC << 16 | HW_ID bits: SE 15:13, SH 12, CU 11:8, SIMD 5:4), one
  // word per regular block; only recorded by handles in isolation mode 1.  Returns the number of words written (<= n), < 0 on error.
  int debug_placement(uint32_t* out, int32_t n) override {
    if (S.iso_on != 1) return 0;
    HIP_OK(hipDeviceSynchronize());
    const int m = n < 4 * DRV_ISO_GROUPS ? n : 4 * DRV_ISO_GROUPS;
    int tick = S.tick;
    if (S.tick_src) HIP_OK(hipMemcpy(&tick, S.iso + DRV_ISOW_TICK, sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out, S.iso_hw + (size_t)(tick & 1) * (4 * DRV_ISO_GROUPS), sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    return m;
  }

  // one wave per blob (drv_get_states_kernel / drv_set_states_kernel)
  int get_states(const int32_t* idx, int32_t first, int32_t n, void* blobs, hipStream_t st) override {
    hipLaunchKernelGGL(drv_get_states_kernel, dim3(n), dim3(64), 0, st, S, (const int*)idx, (int)first, (unsigned long long*)blobs);
    return launched();
  }
  int set_states(const int32_t* idx, int32_t first, int32_t n, const void* blobs, int32_t* status, bool raise, hipStream_t st) override {
    hipLaunchKernelGGL(drv_set_states_kernel, dim3(n), dim3(64), 0, st, S, (const int*)idx, (int)first, (const unsigned long long*)blobs, (int*)status,
                       raise ? 1 : 0);
    return launched();
  }
  int error_flags_env(int32_t* flags, hipStream_t st) override {
    hipLaunchKernelGGL(drv_error_flags_env_kernel, dim3((S.E + 63) / 64), dim3(64), 0, st, S, (int*)flags);
    return launched();
  }

  // the scheduler's lists describe the timing of the steps this handle ran, not the state just restored: start them over
  // (a list that keeps ids from before the restore could be appended to without having been cleared - ADVICE r3)
  int checkpoint_loaded() override {
    if (iso_reset()) return DYNENV_ERR_HIP;
    S.iso_on = iso_cfg; iso_last_invalid = 0; iso_paused_until = 0; steps = 0;
    if (iso_seen) *iso_seen = 0;
    return DYNENV_OK;
  }
};

dynenv* drv_new_handle() { return new DrvHandle(); }

// the deterministic math header's device self-test lives here because its kernel does (driving_kernels.hip)
extern "C" int dynenv_math_selftest(const double* x, const double* y, int32_t n, double* out, int32_t device_id) {
  if (int rc = have_device(nullptr, "no HIP device visible")) return rc;
  HIP_OK(hipSetDevice(device_id));
  double *dx = nullptr, *dy = nullptr, *dout = nullptr;
  HIP_OK(hipMalloc((void**)&dx, sizeof(double) * n));
  HIP_OK(hipMalloc((void**)&dy, sizeof(double) * n));
  HIP_OK(hipMalloc((void**)&dout, sizeof(double) * n * 5));
  HIP_OK(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dy, y, sizeof(double) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(math_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, dout);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpy(out, dout, sizeof(double) * n * 5, hipMemcpyDeviceToHost));
  hipFree(dx); hipFree(dy); hipFree(dout);
  return DYNENV_OK;
}

// dynenv_math_probe, this unit's half: every routine of include/dynenv_math.h as compiled HERE (-Os, this unit's own copies of the
// out-of-line wrappers of dev_common.h).  The row is include/dynenv_math_probe.h's, shared with the dynenv_capi.hip unit and the oracle.
// Behind everything else in the unit: no other kernel moves.
#include "dynenv_math_probe.h"
extern "C" __global__ void __launch_bounds__(64) drv_math_probe_kernel(const double* in, int n, double* out) { dm_probe_wave(in, n, out); }
int drv_math_probe_launch(const double* in_dev, int n, double* out_dev) {
  hipLaunchKernelGGL(drv_math_probe_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in_dev, n, out_dev);
  return launched();
}
