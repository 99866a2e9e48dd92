// driving_reset.hip - the Driving reset (dynenv_reset, dynenv_reset_masked) and the stand-alone observation kernels: what runs when no
// step does.  Included at the END of the device code of driving_tu.hip, so everything a step launches stays in front of it (the unit's
// addresses are not pinned: DESIGN.md 4).
//
// drv_reset_masked_kernel: one wave per environment (grid E).  mask == nullptr resets every environment, otherwise exactly those whose
// byte is set (a wave whose byte is 0 ends at once).  Lane = object, as in the step kernel: cars 0..9, pedestrians 10..29, obstacle
// candidates 30..49; every lane makes its own dm_env_rng draws (purpose, entity, counter), and every access to the field-major arrays
// is one whole row of the environment per instruction, as in drv_set_states_kernel.
// A reset WRITES: the body, flag, aux, car and episode-reward rows whole (scene re-randomisation, environment_base.py:205-211 ->
// DrivingEnvironment._setup_scene :58-115, :527-584), the obstacles it keeps, the contact cache's pair and meta words (every slot
// free), lastcand (-1) and the int row - time 0, the next episode, the new counts, everything else 0.
// It LEAVES ALONE: the obstacle slots behind the new count, envi[EI_DEFER_OBS] (scheduling scratch of the Partial step) and the contact
// cache's hashes and impulses.
DE_DEV void road_get_spot(const DrvRoad& r, int lane, int spot, V2& pos, double& angle) {  // Road.py:100-114
  int end = lane >= r.nLanes ? 1 : 0;
  V2 p = end ? r.p1 : r.p0;
  V2 spotDir = vmul(end ? vneg(r.dir) : r.dir, r.followDist);
  V2 laneDir = vmul(end ? r.normal : vneg(r.normal), r.width);
  double l = (double)(end ? lane - r.nLanes : lane) + 0.5;
  pos = vadd(vadd(p, vmul(laneDir, l)), vmul(spotDir, (double)spot));
  angle = dm_atan2(spotDir.y, spotDir.x);
}
DE_DEV V2 road_get_walk_spot(const DrvRoad& r, int side, double length, double width) {  // Road.py:117-123
  V2 w0 = r.walk[side][0], w1 = r.walk[side][1];
  V2 center = vadd(w0, vmul(vsub(w1, w0), length));
  double f = width * r.width;
  V2 off = vmul(vmul(r.normal, f), side ? 1.0 : -1.0);
  return vadd(center, off);
}

extern "C" __global__ void __launch_bounds__(64)
drv_reset_masked_kernel(DrvState S, const uint8_t* __restrict__ mask) {
  __shared__ int spots[32];
  const int e = blockIdx.x, lane = threadIdx.x, A = S.A;
  if (mask && uniform_i(mask[e]) == 0) return;
  const size_t E = (size_t)S.E, row = (size_t)e * DRV_NB;
  const uint32_t ep = (uint32_t)uniform_i(S.envi[(size_t)e * EI_COUNT + EI_EPISODE]);
  const uint32_t genv = (uint32_t)(S.env_id_offset + e);
  const dm_u32x4 uc = dm_env_rng(S.seed, genv, ep, DM_RNG_RESET_COUNTS, 0, 0);
  const int nPed = dm_randint(uc.v[0], 10, 20), nObstRaw = dm_randint(uc.v[1], 10, 20);
  const bool isCar = lane < A, isPed = lane >= DRV_SLOT_PED && lane < DRV_SLOT_PED + nPed;
  const bool isObst = lane >= DRV_SLOT_OBST && lane < DRV_SLOT_OBST + nObstRaw;
  // every lane's own draws, two Philox evaluations for the whole wave: a = the car's (road, end, team, type), the pedestrian's or
  // the obstacle's (road, side, length, width); b = the car's Fisher-Yates draw, the pedestrian's speed
  const uint32_t ent = (uint32_t)(isCar ? lane : (lane < DRV_SLOT_OBST ? lane - DRV_SLOT_PED : lane - DRV_SLOT_OBST));
  const dm_u32x4 a = dm_env_rng(S.seed, genv, ep, isCar ? DM_RNG_RESET_AGENT : (lane < DRV_SLOT_OBST ? DM_RNG_RESET_PED : DM_RNG_RESET_OBST), ent, 0);
  const dm_u32x4 b = dm_env_rng(S.seed, genv, ep, isCar ? DM_RNG_RESET_PERM : DM_RNG_RESET_PED, ent, isCar ? 0u : 1u);
  // spots = permutation(30)[:A]: the partial Fisher-Yates is serial in i, so it runs wave-uniformly on a table in LDS; lane i made draw i
  const int swapWith = lane + dm_randint(b.v[0], 0, isCar ? 29 - lane : 0);
  if (lane < 32) spots[lane] = lane;
  __syncthreads();
  for (int i = 0; i < A; ++i) {
    const int j = __builtin_amdgcn_readlane(swapWith, i);
    if (lane == 0) { const int t = spots[i]; spots[i] = spots[j]; spots[j] = t; }
  }
  __syncthreads();
  double bf[BF_COUNT], cx[CF_COUNT];
#pragma unroll
  for (int f = 0; f < BF_COUNT; ++f) bf[f] = 0.0;
#pragma unroll
  for (int f = 0; f < CF_COUNT; ++f) cx[f] = 0.0;
  int fl = 0;
  if (isCar) {
    const int roadSel = dm_randint(a.v[0], 0, 1), endSel = dm_randint(a.v[1], 0, 1);
    const int team = dm_randint(a.v[2], 0, 2), type = dm_randint(a.v[3], 0, 3);
    const V2 goal = endSel ? C.roads[roadSel].p1 : C.roads[roadSel].p0;
    int spotID = spots[lane];
    const int roadID = spotID < 20 ? 0 : 1;
    spotID -= roadID ? 20 : 0;
    const int laneID = spotID / 5, spot = spotID % 5;
    V2 pos; double angle;
    road_get_spot(C.roads[roadID], laneID, spot, pos, angle);
    const V2 dir = vrot_angle(v2(1.0, 0.0), angle);
    bf[BF_PX] = pos.x; bf[BF_PY] = pos.y; bf[BF_ANG] = angle;
    cx[CF_DIRX] = dir.x; cx[CF_DIRY] = dir.y; cx[CF_PREVX] = pos.x; cx[CF_PREVY] = pos.y; cx[CF_GOALX] = goal.x; cx[CF_GOALY] = goal.y;
    fl = CARF_PACK(type, team, 0, 0, 0, LP_OffRoad);
  }
  bool keep = false;
  V2 w = v2(0.0, 0.0);
  if (isPed || isObst) {  // pedestrians and obstacle candidates are placed by the same walk-spot draw
    const int road = dm_randint(a.v[0], 0, 1), side = dm_randint(a.v[1], 0, 1);
    const double len = dm_unit(a.v[2]), wid = dm_unit(a.v[3]) / 2.0 + 0.25;
    w = road_get_walk_spot(C.roads[road], side, len, wid);
    if (isPed) {
      bf[BF_PX] = w.x; bf[BF_PY] = w.y;
      fl = PEDF_PACK(road, side, 0, 0, 0, dm_randint(b.v[0], 3, 6));
    } else {
      keep = drv_is_off_road(w);
    }
  }
  // the obstacles drv_is_off_road keeps, compacted in ascending candidate order; the slots behind the new count keep what they held
  const uint64_t kept = wave_ballot(keep);
  const int nObst = __popcll(kept);
  if (keep) {
    const int at = __popcll(kept & lanemask_lt());
    S.obst[(size_t)e * DRV_MAXO + at] = w.x;
    S.obst[E * DRV_MAXO + (size_t)e * DRV_MAXO + at] = w.y;
  }
  if (lane < DRV_NB) {
#pragma unroll
    for (int f = 0; f < BF_COUNT; ++f) S.body[(size_t)f * E * DRV_NB + row + lane] = bf[f];
    S.flags[row + lane] = fl; S.aux[row + lane] = 0;
  }
  if (lane < 16) {
#pragma unroll
    for (int f = 0; f < CF_COUNT; ++f) S.carx[(size_t)f * E * 16 + (size_t)e * 16 + lane] = cx[f];
    S.epr[(size_t)e * 16 + lane] = 0.0;
    S.epr[E * 16 + (size_t)e * 16 + lane] = 0.0;
  }
  if (lane < DRV_NS) { S.s_pair[(size_t)e * DRV_NS + lane] = 0xFFFF; S.s_meta[(size_t)e * DRV_NS + lane] = 0; }
  // the int row: time 0, the next episode, the new counts; cache occupancy, error word, shortcut bits and the diagnostics at 0
  // (EI_DEFER_OBS is scheduling scratch of the Partial step and keeps its value)
  static_assert(EI_DEFER_OBS == EI_COUNT - 1, "the words a reset writes are the row without its last one");
  if (lane < EI_DEFER_OBS)
    S.envi[(size_t)e * EI_COUNT + lane] = lane == EI_NPED ? nPed : lane == EI_NOBST ? nObst : lane == EI_EPISODE ? (int)(ep + 1) : 0;
  S.lastcand[(size_t)e * 64 + lane] = -1;  // quiescent shortcut state unknown
}

// The stand-alone observation kernels, one wave per environment (grid E), mask as above: the first observation behind a reset, and
// dynenv_full_obs (drv_obs_kernel, every environment).  The step kernels write their own.
extern "C" __global__ void __launch_bounds__(64) drv_obs_kernel(DrvState S, const uint8_t* __restrict__ mask, float* __restrict__ obs) {
  DrvLds& L = g_L;
  const int e = blockIdx.x, lane = threadIdx.x, A = S.A;
  if (mask && uniform_i(mask[e]) == 0) return;
  const int* envi = S.envi + (size_t)e * EI_COUNT;
  const int nPed = uniform_i(envi[EI_NPED]), nObst = uniform_i(envi[EI_NOBST]);
  load_env(S, L, e, lane, A, nPed, nObst, 0ull);
  write_full_obs_ool(lane, A, nPed, nObst, S.obs_dim, obs + (size_t)e * A * S.obs_dim);
}

extern "C" __global__ void __launch_bounds__(64, 4)  // 128 VGPRs: all 4096 environments resident in one pass
drv_partial_obs_kernel(DrvState S, const uint8_t* __restrict__ mask, int noiseType, double magn, float* __restrict__ obs) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (mask && uniform_i(mask[e]) == 0) return;
  const int* envi = S.envi + (size_t)e * EI_COUNT;
  const int nPed = uniform_i(envi[EI_NPED]), nObst = uniform_i(envi[EI_NOBST]), elapsed = uniform_i(envi[EI_ELAPSED]);
  const uint32_t episode = (uint32_t)uniform_i(envi[EI_EPISODE]);
  const PvIn in = pv_load_inputs(S, e, lane, nPed, nObst);
  pv_env(S, g_P, e, lane, nPed, nObst, elapsed, episode, in, noiseType, magn, obs, 0, S.A);
}
