// robocup_reset.hip - the RoboCup reset (dynenv_reset, dynenv_reset_masked) and the stand-alone observation kernels: what runs when no
// step does.  Included at the very END of dynenv_capi.hip, behind everything the step launches run (rc_layout_pad in
// robocup_kernels.hip pins their addresses).
//
// rc_reset_masked_kernel: one wave per environment (grid E).  mask == nullptr resets every environment, otherwise exactly those whose
// byte is set (a wave whose byte is 0 ends at once).  RoboCupEnvironment.__init__ + _setup_scene (:73-99, :239-336), both randomInit
// modes: the 24 + 7 + 8 draws of DM_RNG_ROBO_RESET are made on lanes 0..23, 24..30 and 32..39 in one Philox evaluation of the wave, the
// three short Fisher-Yates loops (perm8 of randomInit, the two team permutations) are serial and run wave-uniformly on tables in LDS,
// lane s < 10 evaluates spot s, and every access to the field-major arrays is one whole row of the environment per instruction, as
// in rc_set_states_kernel.
// A reset WRITES: the body rows (shape cache included), the robot, robot-int and the three episode-reward rows whole, the contact
// cache's pair and meta words (every slot free), the int row (ball owner, the next episode, the constraints in add order, everything
// else - error word, cache occupancy, scores - 0) and the double row.
// It LEAVES ALONE: the contact cache's hashes and impulses, the Partial snapshots (rc_obs_kernel below writes them) and
// prew0.
DE_DEV double rc_cell_x(int i) {  // xL of randomInit's field cells
  return i == 0 ? RC_SIDE + 10.0 : i == 1 ? RC_SIDE + 50.0 : i == 2 ? RC_SIDE + 250.0 : i == 3 ? RC_SIDE + 450.0 : i == 4 ? RC_SIDE + 650.0 :
         i == 5 ? RC_SIDE + 850.0 : RC_SIDE + 890.0;
}
DE_DEV double rc_cell_y(int j) { return j == 0 ? RC_SIDE + 20.0 : j == 1 ? RC_SIDE + 300.0 : RC_SIDE + 580.0; }  // yL

extern "C" __global__ void __launch_bounds__(64)
rc_reset_masked_kernel(RcState S, const uint8_t* __restrict__ mask) {
  __shared__ double rnd[24], spx[10], spy[10];
  __shared__ int perm8[8], perm[2][8];
  const int e = blockIdx.x, lane = threadIdx.x, R = S.R, n = S.n;
  if (mask && uniform_i(mask[e]) == 0) return;
  const size_t E = (size_t)S.E, row = (size_t)e * RC_NB, r16 = (size_t)e * 16;
  const uint32_t ep = (uint32_t)uniform_i(S.envi[(size_t)e * RE_COUNT + RE_EPISODE]);
  const uint32_t genv = (uint32_t)(S.env_id_offset + e);
  const bool randomInit = (S.flags & DYNENV_FLAG_RANDOM_INIT) != 0, detTurn = (S.flags & DYNENV_FLAG_DETERMINISTIC_TURN) != 0;
  // lane i < 24: rnd[i]; lane 24 + i: perm8's draw i < 7 (entity 48 + i); lane 32 + 4 t + i: team t's draw i < 4 (entity 32 + 8 t + i)
  const int pt = (lane - 32) >> 2, pi = (lane - 32) & 3;
  const uint32_t ent = (uint32_t)(lane < 24 ? lane : lane < 32 ? 48 + (lane - 24) : 32 + pt * 8 + pi);
  const uint32_t u0 = dm_env_rng(S.seed, genv, ep, DM_RNG_ROBO_RESET, ent, 0).v[0];
  const int swapWith = lane < 32 ? (lane - 24) + dm_randint(u0, 0, lane < 31 ? 7 - (lane - 24) : 0) : pi + dm_randint(u0, 0, 4 - pi);
  if (lane < 24) rnd[lane] = dm_unit(u0);
  if (lane < 8) { perm8[lane] = lane; perm[0][lane] = lane; perm[1][lane] = lane; }
  __syncthreads();
  if (randomInit)
    for (int i = 0; i < 7; ++i) {
      const int j = __builtin_amdgcn_readlane(swapWith, 24 + i);
      if (lane == 0) { const int tmp = perm8[i]; perm8[i] = perm8[j]; perm8[j] = tmp; }
    }
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 4; ++i) {
      const int j = __builtin_amdgcn_readlane(swapWith, 32 + 4 * t + i);
      if (lane == 0) { const int tmp = perm[t][i]; perm[t][i] = perm[t][j]; perm[t][j] = tmp; }
    }
  __syncthreads();
  // spots[team][slot] = spot 5 team + slot (_create_robot_spots :275-293, randomInit :241-272), one per lane
  const double centX = RC_W / 2.0;
  if (lane < 10) {
    V2 p;
    if (randomInit) {
      // one random spot in each of 10 field cells; the goal-side cells go to the two teams, perm8 deals the 8 middle ones
      const int k = lane == 0 ? 0 : lane == 5 ? 9 : perm8[lane < 5 ? lane - 1 : lane - 2] + 1;
      const bool edge = k == 0 || k == 9;
      const int i = k == 0 ? 0 : k == 9 ? 5 : 1 + ((k - 1) >> 1), j = (k - 1) & 1;
      const double yBeg = edge ? rc_cell_y(0) : rc_cell_y(j), yEnd = edge ? rc_cell_y(2) : rc_cell_y(j + 1);
      const double x = rc_cell_x(i) + rnd[2 * k] * (rc_cell_x(i + 1) - rc_cell_x(i));
      const double y = yBeg + rnd[2 * k + 1] * (yEnd - yBeg);
      p = v2(x, y);
    } else {
      switch (lane) {
        case 0: p = v2(centX - (5.0 * 2.0 + ROBOT_TOTAL_RADIUS) - rnd[0] * 50.0, RC_H / 2.0 + (rnd[1] - 0.5) * 25.0); break;
        case 1: p = v2(centX - (ROBOT_TOTAL_RADIUS + 5.0 * 2.0) - rnd[2] * 50.0, RC_SIDE + 600.0 / 4.0 + (rnd[3] - 0.5) * 50.0); break;
        case 2: p = v2(centX - (ROBOT_TOTAL_RADIUS + 5.0 * 2.0) - rnd[4] * 50.0, RC_SIDE + 3.0 * 600.0 / 4.0 + (rnd[5] - 0.5) * 50.0); break;
        case 3: p = v2(centX - (900.0 / 4.0) - (rnd[6] - 0.5) * 50.0, RC_SIDE + 600.0 / 2.0 + (rnd[7] - 0.5) * 50.0); break;
        case 4: p = v2(RC_SIDE + 20.0, RC_H / 2.0 + (rnd[8] - 0.5) * 50.0); break;
        case 5: p = v2(centX + (75.0 * 2.0 + ROBOT_TOTAL_RADIUS + 5.0 / 2.0) + rnd[9] * 50.0, RC_H / 2.0 + (rnd[10] - 0.5) * 50.0); break;
        case 6: p = v2(centX + (ROBOT_TOTAL_RADIUS + 5.0 / 2.0 + 75.0) + rnd[11] * 50.0, RC_SIDE + 600.0 / 4.0 + (rnd[12] - 0.5) * 50.0); break;
        case 7: p = v2(centX + (ROBOT_TOTAL_RADIUS + 5.0 / 2.0 + 75.0) + rnd[13] * 50.0, RC_SIDE + 3.0 * 600.0 / 4.0 + (rnd[14] - 0.5) * 50.0); break;
        case 8: p = v2(centX + (RC_SIDE + 900.0 / 4.0) + rnd[15] * 50.0, RC_SIDE + 600.0 / 2.0 + (rnd[16] - 0.5) * 50.0); break;
        default: p = v2(RC_W - (RC_SIDE + 20.0), RC_H / 2.0 + (rnd[17] - 0.5) * 50.0); break;
      }
    }
    spx[lane] = p.x; spy[lane] = p.y;
  }
  __syncthreads();
  V2 ballPos = v2(520.0, 370.0);  // W // 2, H // 2
  int owned = 1;
  if (randomInit) {  // _create_ball :325-331
    ballPos = v2(rnd[20] * 900.0 + RC_SIDE, rnd[21] * 600.0 + RC_SIDE);
    owned = rnd[22] > 0.4 ? 1 : 0;
    if (owned != 0 && rnd[23] > 0.5) owned *= -1;
  }
  if (lane < RC_NB) {  // lane = body slot: feet 2 id, 2 id + 1 of robot id, the ball; the shape cache rows RB_COUNT..+3 = (x, y, cos, sin)
    double b[RB_COUNT + 4];
#pragma unroll
    for (int f = 0; f < RB_COUNT + 4; ++f) b[f] = (f == RB_COUNT + 2) ? 1.0 : 0.0;
    if (lane < 2 * R) {
      const int id = lane >> 1, team = id < n ? 1 : -1;
      const int s = id < n ? perm[0][id] : 5 + perm[1][id - n];
      const V2 pos = v2(spx[s], spy[s]);
      const double angle = team > 0 ? 0.0 : DM_PI;
      double sn, cs;
      dm_sincos(angle, &sn, &cs);
      b[RB_PX] = pos.x; b[RB_PY] = pos.y; b[RB_ANG] = angle;
      b[RB_COUNT + 0] = pos.x; b[RB_COUNT + 1] = pos.y; b[RB_COUNT + 2] = cs; b[RB_COUNT + 3] = sn;
    } else if (lane == RC_BALL) {
      b[RB_PX] = ballPos.x; b[RB_PY] = ballPos.y; b[RB_COUNT + 0] = ballPos.x; b[RB_COUNT + 1] = ballPos.y;
    }
#pragma unroll
    for (int f = 0; f < RB_COUNT + 4; ++f) S.body[(size_t)f * E * RC_NB + row + lane] = b[f];
  }
  if (lane < 16) {  // lane = robot
    double rr[RR_COUNT];
#pragma unroll
    for (int f = 0; f < RR_COUNT; ++f) rr[f] = 0.0;
    int fl = 0;
    if (lane < R) {
      const int team = lane < n ? 1 : -1;
      const int s = lane < n ? perm[0][lane] : 5 + perm[1][lane - n];
      const V2 pos = v2(spx[s], spy[s]);
      rr[RR_PREVX] = (pos.x + pos.x) / 2.0; rr[RR_PREVY] = (pos.y + pos.y) / 2.0;  // prevPos = getPos() = (p + p) / 2
      if (detTurn) rr[RR_HEAD] = (double)team * ROBOT_HEAD_MAX;  // :317-319
      fl = team > 0 ? RF_TEAMPOS : 0;
    }
#pragma unroll
    for (int f = 0; f < RR_COUNT; ++f) S.rob[(size_t)f * E * 16 + r16 + lane] = rr[f];
#pragma unroll
    for (int f = 0; f < RI_COUNT; ++f) S.robi[(size_t)f * E * 16 + r16 + lane] = f == RI_FLAGS ? fl : 0;
    S.epr[r16 + lane] = 0.0; S.epr[E * 16 + r16 + lane] = 0.0; S.epo[r16 + lane] = 0.0;
  }
  if (lane < RC_NS) { S.s_pair[(size_t)e * RC_NS + lane] = 0xFFFF; S.s_meta[(size_t)e * RC_NS + lane] = 0; }
  if (lane < RE_COUNT) {  // the joints in add order: joint, rotJoint per robot (:321-323); error word, cache occupancy, scores at 0
    const int k = lane - RE_CORDER;
    S.envi[(size_t)e * RE_COUNT + lane] = lane == RE_OWNED ? owned : lane == RE_EPISODE ? (int)(ep + 1) : lane == RE_NCON ? 2 * R :
                                          (k >= 0 && k < 2 * R) ? k : 0;
  }
  if (lane < RD_COUNT)
    S.envd[(size_t)e * RD_COUNT + lane] = lane == RD_FREECNT ? 9999.0 : (lane == RD_PT0 || lane == RD_PT1) ? 20000.0 :
                                          lane == RD_BPREVX ? ballPos.x : lane == RD_BPREVY ? ballPos.y : 0.0;
}

// The stand-alone observation kernels, one wave per environment (grid E), mask as above.
// fullOnce = 0: the observation tensor after a reset (nTimeSteps rows per environment, the configured observation type);
// fullOnce = 1: ONE noise-free Full observation of the current state [E, A, 66], whatever the observation type - what
// info['Full State'] / info['Recon States'] are made of (RoboCupEnvironment.py:511-512), dynenv_full_obs
extern "C" __global__ void __launch_bounds__(64)
rc_obs_kernel(RcState S, const uint8_t* __restrict__ mask, float* __restrict__ obs, int fullOnce) {
  RcLds& L = g_R;
  const int e = blockIdx.x, lane = threadIdx.x;
  if (mask && uniform_i(mask[e]) == 0) return;
  rc_load_env(S, L, e, lane, 0ull);
  __syncthreads();
  if (fullOnce) {
    rc_write_obs_ool(lane, S.R, 4 + 8 + (S.R - 1) * 6, obs + (size_t)e * S.R * (4 + 8 + (S.R - 1) * 6));
    return;
  }
  if (S.obs_type == DYNENV_OBS_PARTIAL) {
    // environment_base.py:217-222: nTimeSteps separate getAgentVision calls on the initial state, each with fresh noise
    // (draw keys: time word = t); rc_partial_obs_kernel follows on the same stream
    for (int t = 0; t < 5; ++t) {
      RvSnap& sn = S.snap[(size_t)e * 5 + t];
      if (lane < 21) { sn.px[lane] = L.px[lane]; sn.py[lane] = L.py[lane]; }
      if (lane < 20) sn.ang[lane] = L.ang[lane];
      if (lane < 10) { sn.head[lane] = L.head[lane]; sn.rflags[lane] = L.rflags[lane]; }
      if (lane == 0) { sn.owned = L.envi[RE_OWNED]; sn.close0 = L.envi[RE_CLOSE0]; sn.close1 = L.envi[RE_CLOSE1]; sn.tkey = t; }
    }
    return;
  }
  for (int t = 0; t < 5; ++t)  // environment_base.py:217-222: nTimeSteps copies of the initial observation
    rc_write_obs_ool(lane, S.R, S.obs_dim, obs + ((size_t)e * 5 + t) * S.R * S.obs_dim);
}

// Partial: the rows of the five snapshots rc_obs_kernel left; no processSeens rewards behind a reset (rewards == nullptr)
extern "C" __global__ void __launch_bounds__(64, 4)
rc_partial_obs_kernel(RcState S, const uint8_t* __restrict__ mask, float* __restrict__ obs) {
  if (mask && uniform_i(mask[blockIdx.x]) == 0) return;
  rv_env(S, g_V, blockIdx.x, threadIdx.x, obs, nullptr);
}
