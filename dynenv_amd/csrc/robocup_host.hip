// robocup_host.hip - the RoboCup handle: all host code of the RoboCup kernels (constant and scene tables, the pair table, launches,
// profile dumps).  Included by dynenv_capi.hip behind robocup_kernels.hip: it stays part of that translation unit, whose code
// layout the RoboCup launch time is sensitive to (RC_LAYOUT_PAD_WORDS, tools/rc_layout_sweep.py).
static double moment_for_segment_host(double m, V2 a, V2 b, double r) {  // cpMomentForSegment
  V2 offset = vlerp(a, b, 0.5);
  V2 d = vsub(b, a);
  double length = dm_sqrt(vdot(d, d)) + 2.0 * r;
  return m * ((length * length + 4.0 * r * r) / 12.0 + vlensq(offset));
}

// the Full row: ball 4 | self 8 | the other robots (R - 1) x 6 - ((ball, robots), (self,)) of RoboCupEnvironment.py:440-443; returns its width
static int rc_full_row(int R, dynenv_layout_t* L = nullptr) {
  const int rows[3] = {1, 1, R - 1}, feat[3] = {4, 8, 6};
  return row_blocks(L, 3, rows, feat);
}

// the kernels of robocup_reset.hip, which dynenv_capi.hip includes last (behind everything the step launches run)
extern "C" __global__ void rc_reset_masked_kernel(RcState S, const uint8_t* __restrict__ mask);
extern "C" __global__ void rc_obs_kernel(RcState S, const uint8_t* __restrict__ mask, float* __restrict__ obs, int fullOnce);
extern "C" __global__ void rc_partial_obs_kernel(RcState S, const uint8_t* __restrict__ mask, float* __restrict__ obs);

struct HOST_LOCAL RcHandle final : dynenv {
  RcState R;

  int init() override {
    memset(&R, 0, sizeof(R));
    const size_t E = (size_t)cfg.num_envs;
    R.E = (int)E; R.n = cfg.n_players > 5 ? 5 : cfg.n_players; R.R = 2 * R.n;  // environment_base.py:57, maxPlayers = 5
    R.obs_type = cfg.obs_type; R.noise_type = cfg.noise_type; R.noise_magn = cfg.noise_magnitude;
    R.obs_dim = cfg.obs_type == DYNENV_OBS_PARTIAL ? RCP_DIM : rc_full_row(R.R);
    R.seed = cfg.seed; R.env_id_offset = cfg.env_id_offset; R.flags = cfg.flags;
    A = R.R; obs_dim = R.obs_dim; T = 5; action_dim = 4;
    full_dim = rc_full_row(R.R); global_dim = R.R * 6 + 3; state_bytes = sizeof(dynenv_robocup_state_t);
    int rc = 0;
    // (per-environment arrays, [fields][E][row]: the row table of dynenv_get_exact / dynenv_set_exact)
    rc |= alloc_rows(&R.body, RB_COUNT + 4, RC_NB);
    rc |= alloc_rows(&R.rob, RR_COUNT, 16);
    rc |= alloc_rows(&R.robi, RI_COUNT, 16);
    rc |= alloc_rows(&R.envi, 1, RE_COUNT);
    rc |= alloc_rows(&R.envd, 1, RD_COUNT);
    rc |= alloc_rows(&R.epr, 2, 16);
    rc |= alloc_rows(&R.epo, 1, 16);
    rc |= alloc_rows(&R.snap, 1, 5);
    rc |= alloc_rows(&R.prew0, 1, 16);
    // (per-step scratch of the Partial observation - who deferred what, the seen counts in transit, the scheduling forecast: rebuilt
    //  by every step, never part of a checkpoint, whose bytes stay a function of the simulation state alone)
    rc |= alloc(&R.seenPart, (size_t)E * 5 * 10 * RCP_SEEN_STRIDE, SCRATCH);
    rc |= alloc(&R.deferList, (size_t)E + 1 + 8, SCRATCH);
    rc |= alloc_rows(&R.s_pair, 1, RC_NS);
    rc |= alloc_rows(&R.s_meta, 1, RC_NS);
    rc |= alloc_rows(&R.s_hash, 2, RC_NS);
    rc |= alloc_rows(&R.s_imp, 4, RC_NS);
    uint64_t* pairTab = nullptr;
    rc |= alloc(&pairTab, 64 * 2);  // (constant, not per-environment: checkpointed, but no row of the table)
    if (rc) return DYNENV_ERR_HIP;
    R.pairTab = pairTab;
    rows.err = R.envi; rows.errStride = RE_COUNT; rows.errIndex = RE_ERR;
    RcConst c;
    memset(&c, 0, sizeof(c));
    c.footInertia = moment_for_segment_host(4000.0, v2(-10.0, 10.0), v2(10.0, 10.0), 7.5);  // Robot.py:34
    c.ballInertia = 10.0 * (0.5 * (0.0 * 0.0 + 10.0 * 10.0) + 0.0);                          // Ball.py:9
    {  // cpPivotJoint preStep with r1 = r2 = 0 (k_tensor + inverse), cpRotaryLimitJoint iSum: same operations, same order
      const double ma = 1.0 / ROBOT_MASS, mb = 1.0 / ROBOT_MASS, ia = 1.0 / c.footInertia, ib = 1.0 / c.footInertia;
      const double pr1x = 0.0, pr1y = 0.0, pr2x = 0.0, pr2y = 0.0;
      const double m_sum = ma + mb;
      double k11 = m_sum, k12 = 0.0, k21 = 0.0, k22 = m_sum;
      { const double r1xsq = pr1x * pr1x * ia, r1ysq = pr1y * pr1y * ia, r1nxy = -pr1x * pr1y * ia; k11 += r1ysq; k12 += r1nxy; k21 += r1nxy; k22 += r1xsq; }
      { const double r2xsq = pr2x * pr2x * ib, r2ysq = pr2y * pr2y * ib, r2nxy = -pr2x * pr2y * ib; k11 += r2ysq; k12 += r2nxy; k21 += r2nxy; k22 += r2xsq; }
      const double det = k11 * k22 - k12 * k21;
      const double det_inv = 1.0 / det;
      c.jkk0 = k22 * det_inv; c.jkk1 = -k12 * det_inv; c.jkk2 = -k21 * det_inv; c.jkk3 = k11 * det_inv;
      c.jiSum = 1.0 / (ia + ib);
      c.footMinv = ma; c.footIinv = ia; c.ballIinv = 1.0 / c.ballInertia;
    }
    {  // the Partial-observation scene by vision lane (same expressions as oracle/robocup_partial.c rcp_scene)
      const double W = RC_W, H = RC_H, s = RC_SIDE, pl = 60.0, pw = 110.0, cr = 75.0, pd = 130.0, gw = 80.0;
      int i = 33;
#define LN(ax, ay, bx, by, tx, ty) do { c.visPx[i] = ax; c.visPy[i] = ay; c.visQx[i] = bx; c.visQy[i] = by; c.visT0[i] = tx; c.visT1[i] = ty; ++i; } while (0)
      LN(s, s, s, H - s, 1, 0); LN(W - s, s, W - s, H - s, -1, 0); LN(s, s, W - s, s, 0, 1); LN(s, H - s, W - s, H - s, 0, -1);
      LN(W / 2, s, W / 2, H - s, 0, 0);
      LN(s, H / 2 - pw, s + pl, H / 2 - pw, 1, 0.37); LN(s, H / 2 + pw, s + pl, H / 2 + pw, 1, -0.37);
      LN(s + pl, H / 2 - pw, s + pl, H / 2 + pw, 0.87, 0);
      LN(W - s - pl, H / 2 - pw, W - s, H / 2 - pw, -1, 0.37); LN(W - s - pl, H / 2 + pw, W - s, H / 2 + pw, -1, -0.37);
      LN(W - s - pl, H / 2 - pw, W - s - pl, H / 2 + pw, -0.87, 0);
#undef LN
#define PT(k, x, y, tx, ty) do { c.visPx[k] = x; c.visPy[k] = y; c.visT0[k] = tx; c.visT1[k] = ty; } while (0)
      PT(10, s, H / 2 + gw, 1, -0.27); PT(11, s, H / 2 - gw, 1, 0.27); PT(12, W - s, H / 2 + gw, -1, -0.27); PT(13, W - s, H / 2 - gw, -1, 0.27);
      PT(14, 520.0, 370.0, 0, 0); PT(15, s + pd, 370.0, 1, 0); PT(16, W - (s + pd), 370.0, -1, 0);
      i = 17;
#define FC(x, y, tx, ty) do { PT(i, x, y, tx, ty); ++i; } while (0)
      FC(s, s, 1, 1); FC(s, H - s, 1, -1); FC(W - s, s, -1, 1); FC(W - s, H - s, -1, -1);
      FC(W / 2, s, 0, 1); FC(W / 2, H - s, 0, -1);
      FC(W / 2, H / 2 - cr * 2, 0, 0.5); FC(W / 2, H / 2 + cr * 2, 0, -0.5);
      FC(s, H / 2 - pw, 1, 0.37); FC(s, H / 2 + pw, 1, -0.37); FC(s + pl, H / 2 - pw, 0.87, 0.37); FC(s + pl, H / 2 + pw, 0.87, -0.37);
      FC(W - s, H / 2 - pw, -1, 0.37); FC(W - s, H / 2 + pw, -1, -0.37); FC(W - s - pl, H / 2 - pw, -0.87, 0.37); FC(W - s - pl, H / 2 + pw, -0.87, -0.37);
#undef FC
#undef PT
    }
    int p = 0;
    for (int i = 0; i <= RC_BALL; ++i)
      for (int j = i + 1; j < RC_POST + 4; ++j) c.pairs[p++] = (uint16_t)((i << 8) | j);
    for (; p < RC_NPAIR_ROUNDS * 64; ++p) c.pairs[p] = 0xFFFF;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(RC), &c, sizeof(c));
    if (e != hipSuccess) return fail(DYNENV_ERR_HIP, hipGetErrorString(e));
    {  // the pairs of each lane (lane l tests pairs l, 64 + l, ...), packed, without those of feet this handle's robots do not have
      static_assert(RC_NPAIR_ROUNDS == 5, "pairTab packs four rounds into the first word and the fifth into the second");
      uint64_t tab[64][2];
      for (int lane = 0; lane < 64; ++lane) {
        uint64_t lo = 0ull, hi = 0ull, feet = 0ull;
        for (int t = 0; t < RC_NPAIR_ROUNDS; ++t) {
          const int pr = c.pairs[t * 64 + lane], i = pr >> 8, j = pr & 0xFF;
          bool ok = pr != 0xFFFF;
          if (ok && i < RC_BALL) ok = i < 2 * R.R;  // feet 2r, 2r + 1 of robot r < R.R
          if (ok && j < RC_BALL) ok = j < 2 * R.R;
          const uint64_t v = (uint64_t)(ok ? pr : 0xFFFF);
          if (t < 4) lo |= v << (16 * t); else hi |= v;
          if (ok && j < RC_BALL && j == i + 1 && !(i & 1)) feet |= 1ull << t;
        }
        tab[lane][0] = lo; tab[lane][1] = hi | (feet << 32);
      }
      e = hipMemcpy(pairTab, tab, sizeof(tab), hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(DYNENV_ERR_HIP, hipGetErrorString(e));
    }
    return 0;
  }

  void layout(dynenv_layout_t& L) const override {
    L.steps_per_episode = RC_MAX_TIME / 50;
    if (R.obs_type != DYNENV_OBS_PARTIAL) { rc_full_row(R.R, &L); return; }
    // ((balls, robots), (goals, crosses, line crosses, lines), (numLandMarks, robotsSeen, ballsSeen)) of getAgentVision;
    // block 6 = the tail: 6 list lengths, numLandMarks, ballsSeen, robotsSeen[9]
    const int off[7] = {RCP_OFF_BALL, RCP_OFF_ROB, RCP_OFF_GOAL, RCP_OFF_CROSS, RCP_OFF_FCROSS, RCP_OFF_LINE, RCP_OFF_TAIL};
    const int rows[7] = {RCP_CAP_BALL, RCP_CAP_ROB, RCP_CAP_GOAL, RCP_CAP_CROSS, RCP_CAP_FCROSS, RCP_CAP_LINE, 1};
    const int feat[7] = {5, 7, 6, 6, 8, 5, 17};
    row_blocks(&L, 7, rows, feat, off);
  }

  void set_seed(uint64_t seed) override { cfg.seed = seed; R.seed = seed; }

  int reset_masked(const uint8_t* mask, float* obs, hipStream_t st) override {
    note_capture(st);
    hipLaunchKernelGGL(rc_reset_masked_kernel, dim3(R.E), dim3(64), 0, st, R, mask);
    if (obs) {
      hipLaunchKernelGGL(rc_obs_kernel, dim3(R.E), dim3(64), 0, st, R, mask, obs, 0);
      if (R.obs_type == DYNENV_OBS_PARTIAL)
        hipLaunchKernelGGL(rc_partial_obs_kernel, dim3(R.E), dim3(64), 0, st, R, mask, obs);
    }
    return launched();
  }

  int full_obs(float* full, hipStream_t st) override {
    hipLaunchKernelGGL(rc_obs_kernel, dim3(R.E), dim3(64), 0, st, R, (const uint8_t*)nullptr, full, 1);
    return launched();
  }
  int global_state(float* state, hipStream_t st) override {
    hipLaunchKernelGGL(rc_global_state_kernel, dim3((R.E + 3) / 4), dim3(64), 0, st, R, state);
    return launched();
  }

  int step(const uint8_t* mask, const int* actions, const double* head, float* obs, double* rewards, uint8_t* dones, hipStream_t st) override {
    note_capture(st);  // (R.seed is frozen into a captured launch: dynenv_host.h)
    if (R.obs_type == DYNENV_OBS_PARTIAL && obs) {  // getAgentVision at the five snapshots + processSeens fused into the launch
      HIP_OK(hipMemsetAsync(R.deferList, 0, sizeof(int), st));
      if (step_begin(st)) return DYNENV_ERR_HIP;
      hipLaunchKernelGGL(rc_step_partial_kernel, dim3(R.E), dim3(64), 0, st, R, mask, actions, head, obs, rewards, dones);
      step_main_done(st);
      const int nb = R.E < RC_DEFER_BLOCKS ? R.E : RC_DEFER_BLOCKS;  // the deferred environments are few: blocks stride over their list
      hipLaunchKernelGGL(rc_partial_obs_deferred_kernel, dim3(nb, 5, R.R), dim3(64), 0, st, R, obs);
      hipLaunchKernelGGL(rc_partial_finalize_kernel, dim3(nb), dim3(64), 0, st, R, rewards);
    }
    else if (R.obs_type == DYNENV_OBS_PARTIAL)
      return fail(DYNENV_ERR_ARG, "RoboCup Partial: the observation buffer is required (the processSeens rewards come out of the same pass)");
    else {
      if (step_begin(st)) return DYNENV_ERR_HIP;
      hipLaunchKernelGGL(rc_step_kernel, dim3(R.E), dim3(64), 0, st, R, mask, actions, head, obs, rewards, dones);
      step_main_done(st);
    }
    return launched();
  }

  int counts(int32_t* out, hipStream_t st) override { HIP_OK(hipMemsetAsync(out, 0, sizeof(int32_t) * 2 * R.E, st)); return DYNENV_OK; }
  int episode_stats(double* ep_r, double* ep_pos_r, double* ep_obs_r, int32_t* goals, hipStream_t st) override {
    hipLaunchKernelGGL(rc_stats_kernel, dim3((R.E + 63) / 64), dim3(64), 0, st, R, ep_r, ep_pos_r, ep_obs_r, (int*)goals);
    return launched();
  }

  int debug_counters(int64_t* out16) override {  // (the counters are Driving's; -DDRV_PROFILE builds dump the stage profiles here)
    for (int k = 0; k < 16; ++k) out16[k] = 0;
#ifdef DRV_PROFILE
    HIP_OK(hipDeviceSynchronize());
    if (prof_dump(g_rcprof, "rcprof", 12) || prof_dump(g_rcprof2, "rcprof2", 8) || prof_dump(g_rcprof3, "rcprof3", 8) || prof_dump(g_rcprof4, "rcprof4", 8))
      return DYNENV_ERR_HIP;
#endif
    return DYNENV_OK;
  }

  // one wave per blob (rc_get_states_kernel / rc_set_states_kernel)
  int get_states(const int32_t* idx, int32_t first, int32_t n, void* blobs, hipStream_t st) override {
    hipLaunchKernelGGL(rc_get_states_kernel, dim3(n), dim3(64), 0, st, R, (const int*)idx, (int)first, (unsigned long long*)blobs);
    return launched();
  }
  int set_states(const int32_t* idx, int32_t first, int32_t n, const void* blobs, int32_t* status, bool raise, hipStream_t st) override {
    hipLaunchKernelGGL(rc_set_states_kernel, dim3(n), dim3(64), 0, st, R, (const int*)idx, (int)first, (const unsigned long long*)blobs, (int*)status,
                       raise ? 1 : 0);
    return launched();
  }
  int error_flags_env(int32_t* flags, hipStream_t st) override {
    hipLaunchKernelGGL(rc_error_flags_env_kernel, dim3((R.E + 63) / 64), dim3(64), 0, st, R, (int*)flags);
    return launched();
  }
};
