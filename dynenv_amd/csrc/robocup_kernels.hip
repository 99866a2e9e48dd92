// robocup_kernels.hip — hand-written gfx950 kernels for the batched DynEnv RoboCup step (Full observations).
//
// Replaces RoboCupEnvironment.step (reference RoboCupEnvironment.py:446-524) for E environments at once: 50 physics
// substeps {processAction, tick per robot, isBallOutOfField | pymunk Space.step with 2 joints per robot and capsule /
// circle contacts | callbacks} and the 5 Full-observation snapshots, fused in ONE launch; one wavefront per
// environment (lane roles in robocup_dev.h).  Mirrors oracle/robocup.c + oracle/cp_lite.c operation by operation
// (fp64, FMA contraction off) so results are bit-identical to the CPU oracle.
#include "robocup_dev.h"
// Where the RoboCup code starts in the code object.  rc_step_kernel and the out-of-line functions it calls are ~110 KB of
// instructions, more than the 64 KB instruction cache, and the launch's time moves by ~1 % with their addresses: the same
// instructions ran 1.418 ms per step in one build and 1.430 in the next, in which only code in FRONT of them had grown (three same-box
// A/Bs; padding them back to the old addresses modulo 32 KB recovered it).  This function pins the phase: it pads to a 32 KB boundary
// and on to the offset the 1.418 ms build happened to have, so edits elsewhere (the Driving code in front, the vision code - which
// is emitted behind the step kernels for the same reason, see the end of this file) no longer move RoboCup's time.
#ifndef RC_LAYOUT_PAD_WORDS
#define RC_LAYOUT_PAD_WORDS 6103
#endif
extern "C" __device__ __attribute__((used, noinline)) void rc_layout_pad() { asm volatile(".p2align 15\n.fill %0, 4, 0xbf800000" ::"i"(RC_LAYOUT_PAD_WORDS)); }

__constant__ RcConst RC;

// The per-substep stages are out-of-line functions (DE_OOL: no callee-saved registers, dev_common.h).  Measured on MI355X (4096
// envs, round 1): both out of line 3.93 ms/step, physics inlined 4.29, both inlined 4.45 -> out of line wins (smaller live ranges
// beat the call overhead)
#ifndef RC_WAVES_PER_SIMD
#define RC_WAVES_PER_SIMD 4
#endif
// The COMMON part of a substep (game logic, position update, broadphase,
// the quiet substep's joints) is an out-of-line function of its own, rc_common_substep - 102 VGPRs, no call inside, nothing
// saved, nothing spilled - instead of living inline in a kernel whose register allocation it shared with everything else
// (round 1: 87 spilled VGPRs, ~50 scratch instructions per substep and wave, 2.1 GB of HBM traffic per launch; 0.11 GB now).
// The one call the common part could make (the sequential game logic) is made by the kernel.
#define RC_COMMON_SINCOS(x) dev_sincos_inl(x)


#define ROBOT_VELOCITY 50.0
#define ROBOT_MASS 4000.0
#define ROBOT_HEAD_MAX (2.0 * DM_PI / 3.0)
#define ROBOT_TOTAL_RADIUS 17.5
#define FOOT_RADIUS 7.5
#define BALL_R 10.0 /* Circle(body, radius*2) with radius = 5 (Ball.py:8-16) */
#define POST_R 10.0 /* Goalpost.py:5-13 */
#define RC_TIME 10.0

struct RcMailbox {
  double p1x[RC_NS][2], p1y[RC_NS][2], p2x[RC_NS][2], p2y[RC_NS][2], nx[RC_NS], ny[RC_NS];
  int hash[RC_NS][2], count[RC_NS], flag[RC_NS];
};
struct RcArbShare {  // what an arbiter's slot lane hands to its bias lane (slot + 16) after the prestep
  double d[RC_NS][14];  // n, r1[0], r1[1], r2[0], r2[1], nMass[0..1], bias[0..1]
  int code[RC_NS];      // bodyA | bodyB << 8 | count << 16 | level << 24
};
struct RcObsStage {
  float rx[RC_MAXR], ry[RC_MAXR], rcs[RC_MAXR], rsn[RC_MAXR], hc[RC_MAXR], hs[RC_MAXR], ahc[RC_MAXR], ahs[RC_MAXR];
  float team[RC_MAXR], down[RC_MAXR];
  float bx, by;
};
struct RcPrefilter {
  float4 box[RC_NB];  // (centre x, centre y, half width + 1, half height + 1) of a body's box in fp32: ONE 16-byte LDS read per body of a pair
};
struct __align__(16) RcLds {
  // bodies: feet 0..19, ball 20 (home location of the state); posts 21..24 are constants
  double px[RC_NB], py[RC_NB], vx[RC_NB], vy[RC_NB], ang[RC_NB], w[RC_NB], vbx[RC_NB], vby[RC_NB], wb[RC_NB];
  double fx[RC_NB], fy[RC_NB], tq[RC_NB];
  // shape cache as of the last position integration (what pymunk's spatial queries and the narrowphase see)
  double cpx[RC_NB], cpy[RC_NB], crc[RC_NB], crs[RC_NB];
  double rotAng[RC_BALL];  // the angle (crc, crs) are the cosine and sine of; NaN at kernel entry (the angle is not part of the saved state)
  double aabb[21][4];
  // robots
  double head[16], headmov[16], prevx[16], prevy[16], initx[16], inity[16], penalT[16], fallT[16], moveT[16];
  double jx[16], jy[16], jrot[16];
  double rrew[16], rposrew[16];
  double envd[RD_COUNT], teamRew[2];
  int rflags[16], touchc[16], fallc[16];
  int envi[RE_COUNT];
  int s_pair[RC_NS], s_meta[RC_NS], s_hash0[RC_NS], s_hash1[RC_NS];
  double s_jn0[RC_NS], s_jt0[RC_NS], s_jn1[RC_NS], s_jt1[RC_NS];
  unsigned short candList[128];  // compacted broadphase candidates (pair codes) in canonical order
  // What rc_physics derives from the STRUCTURE of the contact set alone is kept from call to call within a launch (as in the Driving
  // contact path): the candidate list while every lane's candidate mask is the one it was built from, the level schedule while the
  // active-arbiter mask is the previous evaluation's.
  unsigned char lastCand[64];    // the candidate masks candList was built from (0xFF: none)
  unsigned char sLevel[RC_NS];   // level of slot s in the cached schedule
  int candN;                     // entries of candList (-1: not valid)
  int sMaxLevel;                 // maxLevel of the cached schedule
  unsigned long long sActive;    // the active mask it belongs to: the previous evaluation's (every evaluation records its own)
  union {
    RcMailbox mb;
    RcArbShare sh;
    RcObsStage ob;
    RcPrefilter pf;
  } u;
};
// the LDS tile of a wave's environment
static_assert(sizeof(RcLds) <= 10240, "16 one-wave workgroups per CU - one residency round of 4096 environments on 256 CUs - need <= 160 KB / 16 of LDS each");
__shared__ RcLds g_R;

// One environment per wave is the only layout: the whole wave serves it, and its tile is g_R.
// (The measured alternatives - two environments per wave, one lane per robot - are in profiles/r02_robocup_variants_final.txt.)
static_assert(RC_NPAIR_ROUNDS <= 8, "a lane's pair codes are two words of four rounds each");
#define RC_MY_PAIR(t) ((int)((((t) < 4 ? pairLo : pairHi) >> (16 * ((t)&3))) & 0xFFFFull))

DE_DEV double rc_minv(int b) { return b == RC_BALL ? 1.0 / 10.0 : (b < RC_BALL ? 1.0 / ROBOT_MASS : 0.0); }
DE_DEV double rc_iinv(int b) { return b == RC_BALL ? RC.ballIinv : (b < RC_BALL ? RC.footIinv : 0.0); }  // host-side 1.0 / inertia
DE_DEV V2 post_pos(int idx) {  // RoboCupEnvironment.py:295-302
  int k = idx - RC_POST;
  return v2((k & 2) ? RC_W - RC_SIDE : RC_SIDE, (k & 1) ? RC_H / 2.0 - 80.0 : RC_H / 2.0 + 80.0);
}
DE_DEV V2 robot_pos(const RcLds& L, int r) {  // Robot.getPos
  return v2((L.px[2 * r] + L.px[2 * r + 1]) / 2.0, (L.py[2 * r] + L.py[2 * r + 1]) / 2.0);
}
DE_DEV double robot_angle(const RcLds& L, int r) { return (L.ang[2 * r] + L.ang[2 * r + 1]) / 2.0; }
DE_DEV int robot_team(const RcLds& L, int r) { return (L.rflags[r] & RF_TEAMPOS) ? 1 : -1; }

// cutils.py:102-140 apply_friction incl. the embedded Body.update_velocity (forces from fall() are consumed here)
DE_DEV void rc_velocity_update(RcLds& L, int b) {
  double vx = L.vx[b], vy = L.vy[b], w = L.w[b];
  const double minv = rc_minv(b), iinv = rc_iinv(b);
  vx = vx * 1.0 + (0.0 + L.fx[b] * minv) * DE_DT;
  vy = vy * 1.0 + (0.0 + L.fy[b] * minv) * DE_DT;
  w = w * 1.0 + L.tq[b] * iinv * DE_DT;
  L.fx[b] = 0.0; L.fy[b] = 0.0; L.tq[b] = 0.0;
  const double m = b == RC_BALL ? 10.0 : ROBOT_MASS;
  const double friction = b == RC_BALL ? 2.8e-2 : 1e-3, rotFriction = b == RC_BALL ? 1e-3 : 1e-2;
  const double spin = b == RC_BALL ? 5e-2 : 0.0;
  const double factor = friction * m, rotFactor = rotFriction * m;
  double x = vx, y = vy;
  const double length = 1.0 / (dm_abs(x) + dm_abs(y) + 1e-5);
  double theta = w;
  double a0 = x * factor * length;
  double a1 = y * factor * length;
  a0 += a1 * spin * theta;
  a1 -= a0 * spin * theta;
  if (dm_abs(x) < factor) x = 0.0; else x -= a0;
  if (dm_abs(y) < factor) y = 0.0; else y -= a1;
  if (dm_abs(theta) < rotFactor) theta = 0.0; else theta -= (theta > 0.0 ? rotFactor : -rotFactor);
  L.vx[b] = x; L.vy[b] = y; L.w[b] = theta;
}

// ------------------------------------------------------------------------------------------------
// scalar game logic (lane 0): mirrors oracle/robocup.c
// ------------------------------------------------------------------------------------------------
struct RcCtx {
  uint64_t seed;
  uint32_t genv, episode;
  int n, R, canFall, allowHead, detTurn;
};

// The context is the same in every lane; an out-of-line function receives it in vector registers (the calling convention has no
// uniform arguments) and says so here, first thing: its fields then live in scalar registers instead of nine VGPRs that would be
// spilled across the solver.
DE_DEV RcCtx rc_ctx_uniform(const RcCtx& v) {
  RcCtx c;
  c.seed = uniform_u64(v.seed); c.genv = (uint32_t)uniform_i((int)v.genv); c.episode = (uint32_t)uniform_i((int)v.episode);
  c.n = uniform_i(v.n); c.R = uniform_i(v.R); c.canFall = uniform_i(v.canFall); c.allowHead = uniform_i(v.allowHead); c.detTurn = uniform_i(v.detTurn);
  return c;
}
DE_DEV dm_u32x4 rc_rng(const RcCtx& c, const RcLds& L, uint32_t entity) {
  return dm_env_rng(c.seed, c.genv, c.episode, DM_RNG_ROBO_STEP, entity, (uint32_t)L.envi[RE_ELAPSED]);
}
DE_DEV bool in_last_kicked(const RcLds& L, int id) {
  for (int i = 0; i < L.envi[RE_NLK]; ++i) if (L.envi[RE_LK0 + i] == id) return true;
  return false;
}
DE_DEV void push_last_kicked(RcLds& L, int id) {
  int n = L.envi[RE_NLK] < 4 ? L.envi[RE_NLK] : 3;
  for (int i = n; i > 0; --i) L.envi[RE_LK0 + i] = L.envi[RE_LK0 + i - 1];
  L.envi[RE_LK0] = id;
  L.envi[RE_NLK] = n + 1;
}
// constraint array bookkeeping (cpArrayDeleteObj swaps the last element into the hole; add appends)
// derived from the constraint list: bit r = robot r's pivot (id 2r) precedes its rotary limit (id 2r+1).  Recomputed
// whenever the list changes (rare: kicks, penalties) instead of searching the list in every substep.
DE_DEV void refresh_pivot_first(RcLds& L) {
  const int n = L.envi[RE_NCON];
  int mask = 0;
  for (int r = 0; r < 10; ++r) {  // DYNENV_MAX_ROBOTS
    int posP = -1, posR = -1;
    for (int i = 0; i < n; ++i) {
      const int cid = L.envi[RE_CORDER + i];
      if (cid == 2 * r) posP = i;
      if (cid == 2 * r + 1) posR = i;
    }
    if (posP < posR) mask |= 1 << r;
  }
  L.envi[RE_PIVFIRST] = mask;
}
DE_DEV void con_remove(RcLds& L, int cid) {
  int n = L.envi[RE_NCON];
  for (int i = 0; i < n; ++i) {
    if (L.envi[RE_CORDER + i] == cid) { L.envi[RE_CORDER + i] = L.envi[RE_CORDER + n - 1]; L.envi[RE_NCON] = n - 1; break; }
  }
  refresh_pivot_first(L);
}
DE_DEV void con_add(RcLds& L, int cid) { L.envi[RE_CORDER + L.envi[RE_NCON]] = cid; L.envi[RE_NCON] += 1; refresh_pivot_first(L); }

DE_DEV void set_body_angle(RcLds& L, int b, double a) { L.ang[b] = a; }

DE_DEV void free_penalty_spot(const RcCtx& c, const RcLds& L, int r, V2& spot, double& angle) {  // :792-821
  const double y = L.py[RC_BALL];
  const bool lower = !(y > RC_H / 2.0);
  const int team = robot_team(L, r);
  int sel = 0;
  angle = (y < RC_H / 2.0) ? -DM_PI / 2.0 : DM_PI / 2.0;
  for (int k = 0; k < 7; ++k) {
    const double sx = team > 0 ? RC_SIDE + (double)(k + 1) * ROBOT_TOTAL_RADIUS * 3.0 : RC_W - RC_SIDE - (double)(k + 1) * ROBOT_TOTAL_RADIUS * 3.0;
    const double sy = lower ? RC_H - RC_SIDE : RC_SIDE;
    bool available = true;
    for (int j = 0; j < c.R; ++j) {
      if (j == r) continue;
      V2 p = robot_pos(L, j);
      if (vlen(v2(sx - p.x, sy - p.y)) < ROBOT_TOTAL_RADIUS * 3.0) { available = false; break; }
    }
    if (available) { sel = k; break; }
  }
  spot.x = team > 0 ? RC_SIDE + (double)(sel + 1) * ROBOT_TOTAL_RADIUS * 3.0 : RC_W - RC_SIDE - (double)(sel + 1) * ROBOT_TOTAL_RADIUS * 3.0;
  spot.y = lower ? RC_H - RC_SIDE : RC_SIDE;
}

DE_OOL void rc_penalize(const RcCtx c_, int r) {  // :824-859
  const RcCtx c = rc_ctx_uniform(c_);
  RcLds& L = g_R;
  const int teamIdx = robot_team(L, r) > 0 ? 0 : 1;
  int f = L.rflags[r];
  f |= RF_PENAL;
  L.penalT[r] = L.envd[RD_PT0 + teamIdx];
  L.rrew[r] -= L.envd[RD_PT0 + teamIdx] / 2000.0;
  L.envd[RD_PT0 + teamIdx] += 10000.0;
  V2 pos; double angle;
  free_penalty_spot(c, L, r, pos, angle);
  for (int k = 0; k < 2; ++k) {
    const int b = 2 * r + k;
    L.px[b] = pos.x; L.py[b] = pos.y; set_body_angle(L, b, angle);
    L.vx[b] = 0.0; L.vy[b] = 0.0; L.w[b] = 0.0;
  }
  if ((f & RF_KICK) && (f & RF_JREM)) {
    f &= ~RF_KICK;
    con_add(L, 2 * r);
    f &= ~RF_JREM;
  }
  L.rflags[r] = f;
}

// surface distance of cached shape `s` to p (cpSpacePointQuery in cp_lite.c)
DE_DEV double shape_point_dist(const RcLds& L, int s, V2 p) {
  if (s == RC_BALL) { V2 d = vsub(p, v2(L.cpx[s], L.cpy[s])); return dm_sqrt(vdot(d, d)) - BALL_R; }
  if (s > RC_BALL) { V2 d = vsub(p, post_pos(s)); return dm_sqrt(vdot(d, d)) - POST_R; }
  const double ly = (s & 1) ? -10.0 : 10.0;
  const double c = L.crc[s], sn = L.crs[s];
  const V2 ta = v2(c * -10.0 - sn * ly + L.cpx[s], sn * -10.0 + c * ly + L.cpy[s]);
  const V2 tb = v2(c * 10.0 - sn * ly + L.cpx[s], sn * 10.0 + c * ly + L.cpy[s]);
  const V2 seg = vsub(tb, ta);
  const double t = fclamp01_cp(vdot(seg, vsub(p, ta)) / vlensq(seg));
  const V2 closest = vadd(ta, vmul(seg, t));
  const V2 d = vsub(p, closest);
  return dm_sqrt(vdot(d, d)) - FOOT_RADIUS;
}

DE_OOL void rc_fall(const RcCtx c_, int r, int punish) {  // :735-791
  const RcCtx c = rc_ctx_uniform(c_);
  RcLds& L = g_R;
  const V2 pos = robot_pos(L, r);
  if (punish) L.rrew[r] -= 2.0;
  for (int s = 0; s <= RC_BALL; ++s) {  // canonical slot order; goalposts are static (forces never integrated)
    if (s < RC_BALL && s >= 2 * c.R) continue;
    if (s == 2 * r || s == 2 * r + 1) continue;
    if (!(shape_point_dist(L, s, pos) < 40.0)) continue;
    const double m = s == RC_BALL ? 10.0 : ROBOT_MASS;
    const double force = ROBOT_VELOCITY * ROBOT_MASS * m / 50.0;
    V2 dp = vsub(pos, v2(L.px[s], L.py[s]));
    const double len = vlen(dp);
    dp = v2(-dp.x * force / len, -dp.y * force / len);
    const V2 rr = vsub(pos, v2(L.px[s], L.py[s]));  // cpBodyApplyForceAtWorldPoint
    L.fx[s] = L.fx[s] + dp.x; L.fy[s] = L.fy[s] + dp.y;
    L.tq[s] += vcross(rr, dp);
    if (s == RC_BALL) {
      if (L.envi[RE_NLK] && !in_last_kicked(L, r)) push_last_kicked(L, r);
      if (L.envi[RE_OWNED] != 0) { L.envd[RD_GRACE] = 0.0; L.envd[RD_FREECNT] = 0.0; L.envi[RE_OWNED] = 0; }
    }
  }
  L.rflags[r] |= RF_FALLEN;
  L.fallc[r] += 1;
  L.fallT[r] = 4000.0;
  if (L.fallc[r] > 2) rc_penalize(c, r);
}

DE_DEV void rc_process_action(const RcCtx& c, RcLds& L, int r, const int* action, const double* headAct) {  // :527-581
  const int move = action[0], turn = action[1], kick = action[2];
  double head = (double)action[3];  // a float with allowHeadTurn (Box(-3, 3), :339-342), an int otherwise: exact either way
  const dm_u32x4 u = rc_rng(c, L, (uint32_t)r);
  if (c.allowHead && headAct) head = headAct[r];
  if (c.detTurn) head = (double)(-3 * robot_team(L, r));  // :529-530
  if (!c.allowHead) head -= 3.0;
  // the reference raises on a malformed action (:543-550); here the robot keeps still and the environment's error flag (bit 1,
  // dynenv_error_flags) records it - never an out-of-range index below
  if (move < 0 || move > 4 || turn < 0 || turn > 2 || kick < 0 || kick > 2 || !(dm_abs(head) <= 6.0)) { L.envi[RE_ERR] |= 2; return; }
  const int f0 = L.rflags[r];
  const bool canMove = !(f0 & (RF_PENAL | RF_KICK | RF_FALLEN));
  if (move > 0 && canMove) {
    const double rr = c.canFall ? dm_unit(u.v[0]) : 0.0;
    if (rr > 0.999) { rc_fall(c, r, 0); return; }
    if (!(L.rflags[r] & (RF_KICK | RF_PENAL | RF_FALLEN))) {  // Robot.step :103-119
      L.moveT[r] = 500.0;
      const int dir = move - 1;
      V2 vel = v2(0.0, 0.0);
      bool has = true;
      if (dir == 0) vel = v2(0.0, 2.0 * ROBOT_VELOCITY);
      else if (dir == 1) vel = v2(0.0, -2.0 * ROBOT_VELOCITY);
      else if (dir == 2) vel = v2(2.5 * ROBOT_VELOCITY, 0.0);
      else if (dir == 3) vel = v2(-2.0 * ROBOT_VELOCITY, 0.0);
      else has = false;
      if (has) {
        const DevSC sc = dev_sincos(L.ang[2 * r]);
        L.vx[2 * r] = vel.x * sc.c - vel.y * sc.s;
        L.vy[2 * r] = vel.x * sc.s + vel.y * sc.c;
      }
    }
  }
  if (turn > 0 && canMove) {
    const double rr = c.canFall ? dm_unit(u.v[1]) : 0.0;
    if (rr > 0.999) { rc_fall(c, r, 0); return; }
    if (!(L.rflags[r] & (RF_KICK | RF_PENAL | RF_FALLEN))) {  // Robot.turn :122-125
      L.moveT[r] = 500.0;
      L.w[2 * r] += (turn - 1) ? 20.0 : -20.0;
    }
  }
  if (head != 0.0) { L.headmov[r] = head * DM_PI / 720.0; L.moveT[r] = 500.0; }  // Robot.turnHead :136-138
  if (kick > 0 && move == 0 && turn == 0 && canMove) {
    const double rr = c.canFall ? dm_unit(u.v[2]) : 0.0;
    if (rr > 0.99) { rc_fall(c, r, 0); return; }
    int f = L.rflags[r];
    if (!(f & (RF_KICK | RF_PENAL | RF_FALLEN))) {  // Robot.kick :128-133
      const int foot = kick - 1;
      f = foot ? (f | RF_FOOT) : (f & ~RF_FOOT);
      L.initx[r] = L.px[2 * r + foot]; L.inity[r] = L.py[2 * r + foot];
      f |= RF_KICK;
      L.moveT[r] = 1000.0;
      L.rflags[r] = f;
    }
  }
}

// The reference's tick, every branch: used by the sequential form (rc_game_serial).  The common substep runs the event-free
// subset one robot per lane on registers (rc_game_logic_batched below).
DE_DEV void rc_tick(const RcCtx& c, RcLds& L, int r) {  // :862-1007
  const double time = RC_TIME;
  if (L.moveT[r] > 0.0) {
    L.moveT[r] -= time;
    if (L.headmov[r] != 0.0) {
      double h = L.head[r] + L.headmov[r];
      L.head[r] = dm_max(-ROBOT_HEAD_MAX, dm_min(ROBOT_HEAD_MAX, h));
    }
    int f = L.rflags[r];
    if (f & RF_KICK) {
      const int fb = 2 * r + ((f & RF_FOOT) ? 1 : 0);
      const double mt = L.moveT[r];
      if (mt + time > 500.0 && mt <= 500.0) {
        if (!(f & RF_JREM)) { con_remove(L, 2 * r); f |= RF_JREM; }
        const DevSC sc = dev_sincos(L.ang[fb]);
        const double vxl = ROBOT_VELOCITY * 3.0;
        L.vx[fb] = vxl * sc.c - 0.0 * sc.s; L.vy[fb] = vxl * sc.s + 0.0 * sc.c;
      }
      if (mt + time > 400.0 && mt <= 400.0) {
        const DevSC sc = dev_sincos(L.ang[fb]);
        const double vxl = ROBOT_VELOCITY * 2.5;
        L.vx[fb] = -(vxl * sc.c - 0.0 * sc.s); L.vy[fb] = -(vxl * sc.s + 0.0 * sc.c);
      } else if (mt <= 300.0) {
        L.vx[fb] = 0.0; L.vy[fb] = 0.0;
        f &= ~RF_KICK;
        L.px[fb] = L.initx[r]; L.py[fb] = L.inity[r];
        if (f & RF_JREM) { con_add(L, 2 * r); f &= ~RF_JREM; }
      }
      L.rflags[r] = f;
    }
    if (L.moveT[r] <= 0.0) {
      L.moveT[r] = 0.0; L.headmov[r] = 0.0;
      L.vx[2 * r] = 0.0; L.vy[2 * r] = 0.0; L.w[2 * r] = 0.0;
      L.vx[2 * r + 1] = 0.0; L.vy[2 * r + 1] = 0.0; L.w[2 * r + 1] = 0.0;
    }
  }
  if (L.rflags[r] & RF_FALLEN) {
    L.fallT[r] -= time;
    if (L.fallT[r] < 0.0) {
      const dm_u32x4 u = rc_rng(c, L, (uint32_t)r | (1u << 8));
      const double rr = dm_unit(u.v[0]);
      if (rr > 0.9 && !(L.rflags[r] & RF_PENAL) && c.canFall) { rc_fall(c, r, 0); return; }
      L.rflags[r] &= ~RF_FALLEN;
      L.fallc[r] = 0;
    }
  }
  if (L.rflags[r] & RF_PENAL) {
    L.penalT[r] -= time;
    if (L.penalT[r] <= 0.0) {
      L.penalT[r] = 0.0;
      L.rflags[r] &= ~(RF_PENAL | RF_FALLEN);
      L.fallc[r] = 0;
      V2 p; double angle;
      free_penalty_spot(c, L, r, p, angle);
      for (int k = 0; k < 2; ++k) { L.px[2 * r + k] = p.x; L.py[2 * r + k] = p.y; set_body_angle(L, 2 * r + k, angle); }
    }
  } else {
    const int teamIdx = robot_team(L, r) > 0 ? 0 : 1;
    const V2 p = robot_pos(L, r);
    const double robX = teamIdx ? RC_W - p.x : p.x;
    const double penX = RC_SIDE + 60.0 + 5.0 / 2.0;
    const int bit = 1 << r;
    const bool isDef = (L.envi[RE_DEF0 + teamIdx] & bit) != 0;
    if (robX < penX && p.y > (RC_H / 2.0 - 110.0) && p.y < (RC_H / 2.0 + 110.0)) {
      if (!isDef) {
        if (__popc(L.envi[RE_DEF0 + teamIdx]) >= 2) rc_penalize(c, r);
        else L.envi[RE_DEF0 + teamIdx] |= bit;
      }
    } else if (isDef) {
      L.envi[RE_DEF0 + teamIdx] &= ~bit;
    }
  }
  const V2 pos = robot_pos(L, r);
  if (pos.y < 0.0 || pos.x < 0.0 || pos.y > RC_H || pos.x > RC_W) rc_penalize(c, r);
  if (pos.x != L.prevx[r] || pos.y != L.prevy[r]) {
    if ((r == L.envi[RE_CLOSE0] || r == L.envi[RE_CLOSE1]) && !(L.rflags[r] & RF_PENAL)) {
      const V2 ballPos = v2(L.px[RC_BALL], L.py[RC_BALL]);
      const double diff = vlen(vsub(pos, ballPos)) - vlen(vsub(v2(L.prevx[r], L.prevy[r]), ballPos));
      L.rrew[r] -= diff * 0.05;
      L.rposrew[r] += dm_max(0.0, -diff * 0.05);
    }
    L.prevx[r] = pos.x; L.prevy[r] = pos.y;
  }
}

// ------------------------------------------------------------------------------------------------
// The lane-parallel game logic of the common substep on REGISTERS: one batch of LDS loads, then
//   (1) would robot r's tick touch anything another robot's tick reads or writes?  Events: the kick taking the pivot joint out of
//       / back into the constraint list (and the foot snapping back), a getting-up roll, the end of a penalty, entering or leaving
//       the defender set, leaving the field.  Conservative; evaluated without side effects from the state before the tick.  With
//       an event in any lane the function returns false with NOTHING stored and the kernel runs the sequential form (rc_game_serial).
//   (2) the event-free tick (rc_tick with the branches only an event reaches removed), one robot per lane: without an event a tick
//       reads shared state only and writes its own robot's fields, so the ticks of all robots commute;
//   (3) isBallOutOfField + ballFreeKickProcess (:600-732) by the whole wave: the scalar decisions are computed redundantly by every
//       lane and written by lane 0, the per-robot reward terms run one robot per lane, the two "closest robot" searches replay the
//       reference's ascending strict-< loop over the per-lane distances.
// On loaded values because a lone wave cannot hide an LDS round trip (~110 cycles): the plain form made some forty of them per
// substep, one after the other.
// ------------------------------------------------------------------------------------------------
// min over the 16 lanes of a DPP row, in every lane of the row: four rotate-and-min steps (row_ror 8, 4, 2, 1), no LDS, no loop.
// v_min_f64 ignores a NaN operand, like the `qi < d0` scan this replaces.
template <int ROT>
DE_DEV double rc_row_ror(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x120 + ROT, 0xF, 0xF, false);  // DPP row_ror:ROT
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x120 + ROT, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
DE_DEV double rc_row_min(double x) {
  x = __builtin_fmin(x, rc_row_ror<8>(x));
  x = __builtin_fmin(x, rc_row_ror<4>(x));
  x = __builtin_fmin(x, rc_row_ror<2>(x));
  x = __builtin_fmin(x, rc_row_ror<1>(x));
  return x;
}
#ifdef DRV_PROFILE
__device__ unsigned long long g_rcprof4[4096 * 8];  // stages of the batched game logic: loads + events | tick | ball | closest robots | lane-0 stores; [5..7] the general solve: level passes | joint phases | number of level passes + (number of joint phases << 32)
#define RC_PROF_G(...) __VA_ARGS__
#else
#define RC_PROF_G(...)
#endif
DE_DEV bool rc_game_logic_batched(const RcCtx& c, RcLds& L, int lane, bool withTick) {
RC_PROF_G(const unsigned long long G0 = __builtin_amdgcn_s_memtime(); unsigned long long G1 = G0, G2 = G0;)
  const int R = c.R, n = c.n;
  const bool isRobot = lane < R;
  const int r = isRobot ? lane : 0;
  const double time = RC_TIME;
  // ---- loads ----
  double moveT = L.moveT[r], headmov = L.headmov[r], head = L.head[r], fallT = L.fallT[r], penalT = L.penalT[r];
  const int f = L.rflags[r];
  const double pxa = L.px[2 * r], pxb = L.px[2 * r + 1], pya = L.py[2 * r], pyb = L.py[2 * r + 1];
  double prevx = L.prevx[r], prevy = L.prevy[r];
  double rrew = L.rrew[r], rposrew = L.rposrew[r];
  const int close0 = L.envi[RE_CLOSE0], close1 = L.envi[RE_CLOSE1], def0 = L.envi[RE_DEF0], def1 = L.envi[RE_DEF1];
  const int nlk = L.envi[RE_NLK], lk0 = L.envi[RE_LK0], lk1 = L.envi[RE_LK0 + 1], lk2 = L.envi[RE_LK0 + 2], lk3 = L.envi[RE_LK0 + 3];
  const V2 bpos = v2(L.px[RC_BALL], L.py[RC_BALL]);
  const double bprevx = L.envd[RD_BPREVX];
  // (lane 0's end-of-logic updates read these)
  double grace = L.envd[RD_GRACE], freecnt = L.envd[RD_FREECNT];
  int owned = L.envi[RE_OWNED];
  const int g_goal0 = L.envi[RE_GOAL0], g_goal1 = L.envi[RE_GOAL1];
  const double g_tr0 = L.teamRew[0], g_tr1 = L.teamRew[1];
  const V2 rpos = v2((pxa + pxb) / 2.0, (pya + pyb) / 2.0);  // Robot.getPos (robot_pos)
  if (withTick) {
    // ---- (1) events ----
    bool ev = false;
    if (isRobot) {
      if (moveT > 0.0 && (f & RF_KICK)) {
        const double mt = moveT - time;
        if ((mt + time > 500.0 && mt <= 500.0 && !(f & RF_JREM)) || mt <= 300.0) ev = true;
      }
      if ((f & RF_FALLEN) && fallT - time < 0.0) ev = true;
      if (f & RF_PENAL) {
        if (penalT - time <= 0.0) ev = true;
      } else {
        const int teamIdx = (f & RF_TEAMPOS) ? 0 : 1;
        const double robX = teamIdx ? RC_W - rpos.x : rpos.x;
        const double penX = RC_SIDE + 60.0 + 5.0 / 2.0;
        const bool isDef = ((teamIdx ? def1 : def0) & (1 << r)) != 0;
        const bool inArea = robX < penX && rpos.y > (RC_H / 2.0 - 110.0) && rpos.y < (RC_H / 2.0 + 110.0);
        if (inArea != isDef) ev = true;
      }
      if (rpos.y < 0.0 || rpos.x < 0.0 || rpos.y > RC_H || rpos.x > RC_W) ev = true;
    }
    if (wave_ballot(ev) != 0ull) return false;
RC_PROF_G(G1 = __builtin_amdgcn_s_memtime();)
    // ---- (2) the event-free tick (:862-1007) ----
    if (isRobot) {
      if (moveT > 0.0) {
        moveT -= time;
        if (headmov != 0.0) {
          const double h = head + headmov;
          head = dm_max(-ROBOT_HEAD_MAX, dm_min(ROBOT_HEAD_MAX, h));
          L.head[r] = head;
        }
        if (f & RF_KICK) {
          const int fb = 2 * r + ((f & RF_FOOT) ? 1 : 0);
          const double mt = moveT;
          if (mt + time > 500.0 && mt <= 500.0) {
            const DevSC sc = RC_COMMON_SINCOS(L.ang[fb]);
            const double vxl = ROBOT_VELOCITY * 3.0;
            L.vx[fb] = vxl * sc.c - 0.0 * sc.s; L.vy[fb] = vxl * sc.s + 0.0 * sc.c;
          }
          if (mt + time > 400.0 && mt <= 400.0) {
            const DevSC sc = RC_COMMON_SINCOS(L.ang[fb]);
            const double vxl = ROBOT_VELOCITY * 2.5;
            L.vx[fb] = -(vxl * sc.c - 0.0 * sc.s); L.vy[fb] = -(vxl * sc.s + 0.0 * sc.c);
          }
        }
        if (moveT <= 0.0) {
          moveT = 0.0;
          L.headmov[r] = 0.0;
          L.vx[2 * r] = 0.0; L.vy[2 * r] = 0.0; L.w[2 * r] = 0.0;
          L.vx[2 * r + 1] = 0.0; L.vy[2 * r + 1] = 0.0; L.w[2 * r + 1] = 0.0;
        }
        L.moveT[r] = moveT;
      }
      if (f & RF_FALLEN) L.fallT[r] = fallT - time;
      if (f & RF_PENAL) L.penalT[r] = penalT - time;
      if (rpos.x != prevx || rpos.y != prevy) {
        if ((r == close0 || r == close1) && !(f & RF_PENAL)) {
          const double diff = vlen(vsub(rpos, bpos)) - vlen(vsub(v2(prevx, prevy), bpos));
          rrew -= diff * 0.05;
          rposrew += dm_max(0.0, -diff * 0.05);
        }
        prevx = rpos.x; prevy = rpos.y;
        L.prevx[r] = prevx; L.prevy[r] = prevy;
      }
    }
  }
RC_PROF_G(G2 = __builtin_amdgcn_s_memtime(); if (!withTick) G1 = G2;)
  // ---- (3) the ball (:622-732) ----
  bool finished = false, moved = false;
  int team = 0;
  const V2 pos = bpos;
  double cr0 = 0.0, cr1 = 0.0;
  double x = pos.x, y = pos.y;
  int goal0 = 0, goal1 = 0;
  const double outMin = RC_SIDE - 5.0, outMaxX = RC_W - RC_SIDE + 5.0, outMaxY = RC_H - RC_SIDE + 5.0;
  if (pos.y < outMin || pos.x < outMin || pos.y > outMaxY || pos.x > outMaxX) {
    moved = true;
    x = RC_W / 2.0; y = RC_H / 2.0;
    team = nlk ? robot_team(L, lk0) : 1;
    if (pos.y < outMin || pos.y > outMaxY) {
      x = team < 0 ? pos.x + 50.0 : pos.x - 50.0;
      y = pos.y < outMin ? outMin + 5.0 : outMaxY - 5.0;
    } else {
      if (pos.y < RC_H / 2.0 + 80.0 && pos.y > RC_H / 2.0 - 80.0) {
        finished = true;
        if (pos.x < outMin) { cr0 += -25.0; cr1 += 25.0; goal1 = 1; }
        else { cr0 += 25.0; cr1 += -25.0; goal0 = 1; }
      } else {
        if (pos.x < outMin) {
          if (team < 0) x = RC_SIDE + 60.0;
          else { x = RC_SIDE; y = pos.y < RC_H / 2.0 ? RC_SIDE : RC_H - RC_SIDE; }
        } else {
          if (team > 0) x = RC_W - (RC_SIDE + 60.0);
          else { x = RC_W - RC_SIDE; y = pos.y < RC_H / 2.0 ? RC_SIDE : RC_H - RC_SIDE; }
        }
      }
    }
  }
  if (!finished) {
    const double dx = x - bprevx;
    const double d = dx == 0.0 ? dx : dx / 20.0;  // +-0 / 20 is that same zero: a resting ball skips the division
    cr0 += d;
    cr1 -= d;
  }
  bool inLk = false;
  const bool anyTeamTerm = !(cr0 == 0.0 && cr1 == 0.0);
  if (anyTeamTerm && isRobot) {
    double disc = 1.0;
    for (int i = 0; i < nlk; ++i) {
      const int lki = i == 0 ? lk0 : i == 1 ? lk1 : i == 2 ? lk2 : lk3;
      if (lki == lane) {
        inLk = true;
        const double rew = (lane < n ? cr0 : cr1) * disc;
        rrew += rew;
        rposrew += dm_max(0.0, rew);
      }
      disc *= 0.5;
    }
    const bool cond1 = (lane == close0 || lane == close1);
    const bool cond2 = vlen(vsub(rpos, pos)) < 150.0;
    if ((cond1 || cond2) && !inLk) rrew += dm_min(0.0, (lane < n ? cr0 : cr1) * 0.5);
  }
  if (isRobot) { L.rrew[r] = rrew; L.rposrew[r] = rposrew; }
RC_PROF_G(const unsigned long long G3 = __builtin_amdgcn_s_memtime();)
  // closest robot of each team to the (possibly reset) ball
  double q = INFINITY;
  if (isRobot) {
    const V2 d = vsub(v2(x, y), rpos);
    q = d.x * d.x + d.y * d.y;
  }
  // The reference scans each team in ascending order with a strict `<` from +inf: the FIRST robot at the smallest distance wins, a NaN
  // never does, and with no finite distance at all the answer is robot 0.  The same without a loop: the team's minimum by four DPP
  // rotate-and-min steps over the row (robots sit on lanes 0 .. 2n-1 <= 9 of row 0), then the lowest lane that holds it.
  int best0 = 0, best1 = 0;
  {
    const bool t0 = lane < n, t1 = lane >= n && lane < 2 * n;
    const double m0 = rc_row_min(t0 ? q : INFINITY), m1 = rc_row_min(t1 ? q : INFINITY);
    const uint64_t w0 = wave_ballot(t0 && q == m0 && q < INFINITY), w1 = wave_ballot(t1 && q == m1 && q < INFINITY);
    best0 = w0 ? (int)__builtin_ctzll(w0) : 0;
    best1 = w1 ? (int)__builtin_ctzll(w1) - n : 0;
  }
RC_PROF_G(const unsigned long long G4 = __builtin_amdgcn_s_memtime();)
  __syncthreads();  // every lane has read the shared scalars it needs
  if (lane == 0) {
    if (moved) { L.px[RC_BALL] = x; L.py[RC_BALL] = y; L.vx[RC_BALL] = 0.0; L.vy[RC_BALL] = 0.0; L.w[RC_BALL] = 0.0; }
    L.envi[RE_GOAL0] = g_goal0 + goal0; L.envi[RE_GOAL1] = g_goal1 + goal1;
    {  // ballFreeKickProcess(-team) :600-619
      const int tm = -team;
      if (tm == 0) {
        if (grace > 0.0) {
          grace -= RC_TIME;
          if (grace < 0.0) { grace = 0.0; freecnt = 9999.0; }
        } else if (freecnt > 0.0) {
          freecnt -= RC_TIME;
          if (freecnt < 0.0) { freecnt = 0.0; owned = 0; }
        }
      } else {
        owned = tm; grace = 14999.0; freecnt = 0.0;
      }
      L.envd[RD_GRACE] = grace; L.envd[RD_FREECNT] = freecnt; L.envi[RE_OWNED] = owned;
    }
    L.envd[RD_BPREVX] = x; L.envd[RD_BPREVY] = y;
    L.teamRew[0] = g_tr0 + cr0 * 0.1;
    L.teamRew[1] = g_tr1 + cr1 * 0.1;
    L.envi[RE_CLOSE0] = best0;
    L.envi[RE_CLOSE1] = n + best1;
  }
RC_PROF_G(if (lane == 0 && c.genv < 4096u) { unsigned long long* d = g_rcprof4 + c.genv * 8; const unsigned long long G5 = __builtin_amdgcn_s_memtime(); d[0] += G1 - G0; d[1] += G2 - G1; d[2] += G3 - G2; d[3] += G4 - G3; d[4] += G5 - G4; })
  return true;
}

// The sequential form of the robots' game logic - for robot in agents: [processAction]; tick - for the first substep and for
// substeps with a cross-robot event; out of line, called by lane 0 from the kernel.  (The ball's part follows in
// rc_game_logic_batched, which the common substep then runs without its tick.)
DE_OOL void rc_game_serial(RcCtx c_, int it, const int* __restrict__ actions, const double* __restrict__ headAct) {
  const RcCtx c = rc_ctx_uniform(c_);
  RcLds& L = g_R;
  for (int r = 0; r < c.R; ++r) {
    if (it == 0) {
      int act[4] = {actions[4 * r], actions[4 * r + 1], actions[4 * r + 2], actions[4 * r + 3]};
      rc_process_action(c, L, r, act, headAct);
    }
    rc_tick(c, L, r);
  }
}
// ------------------------------------------------------------------------------------------------
// collision callbacks (lane 0), RoboCupEnvironment.py:1010-1146
// ------------------------------------------------------------------------------------------------
DE_DEV bool rc_cb_begin(const RcCtx& c, RcLds& L, int i, int j) {  // pair (i < j), returns "keep"
  if (j < RC_BALL) {  // robotPushingDet: shapes in collision order (a = lower slot)
    const int r1 = i >> 1, r2 = j >> 1;
    const double v1x = L.vx[i], v1y = L.vy[i], v2x = L.vx[j], v2y = L.vy[j];
    const V2 p1 = robot_pos(L, r1), p2 = robot_pos(L, r2);
    const V2 dp = vsub(p1, p2);
    const double adp = dev_atan2(dp.y, dp.x);
    const bool push1 = vlen(v2(v1x, v1y)) > 1.0 && dev_cos(adp - dev_atan2(v1y, v1x)) < -0.4;
    const bool push2 = vlen(v2(v2x, v2y)) > 1.0 && dev_cos(adp - dev_atan2(v2y, v2x)) > 0.4;
    L.rflags[r1] = push1 ? (L.rflags[r1] | RF_PUSH) : (L.rflags[r1] & ~RF_PUSH);
    L.rflags[r2] = push2 ? (L.rflags[r2] | RF_PUSH) : (L.rflags[r2] & ~RF_PUSH);
    L.rflags[r1] |= RF_TOUCH; L.rflags[r2] |= RF_TOUCH;
    L.touchc[r1] = 0; L.touchc[r2] = 0;
    return true;
  }
  if (j == RC_BALL) {  // ballCollision (foot i, ball)
    const int r = i >> 1;
    if (L.envi[RE_OWNED] != 0) {
      if (robot_team(L, r) != L.envi[RE_OWNED] && !(L.rflags[r] & RF_PENAL) && c.canFall) rc_penalize(c, r);
      else { L.envi[RE_OWNED] = 0; L.envd[RD_GRACE] = 0.0; L.envd[RD_FREECNT] = 0.0; }
    }
    push_last_kicked(L, r);
    return true;
  }
  return true;  // foot-goalpost and ball-goalpost: default begin
}

// `rr > base ** n` (the fall dice of the collision callbacks) without the power in the common case: (1 - x)^n >= 1 - n x
// (Bernoulli), `xOver` is a little more than 1 - base and dm_powi's rounding error (~n 2^-53 relative) is far inside the
// margin, so a die at or below the bound cannot exceed the threshold; every other die is compared with the exact power.
DE_DEV bool rc_dice_exceeds(double rr, double base, double xOver, int n) {
  if (rr <= 1.0 - (double)n * xOver - 1e-6) return false;
  return rr > dm_powi(base, n);
}
// The dice of the post_solve handlers (robotCollision / goalpostCollision) of pair (i, j): two uniforms in [0, 1), a pure
// function of the pair and the time.  Every active arbiter's lane draws its own (one instance of the Philox code for all of
// them) before the handlers run one after the other on lane 0.
DE_DEV void rc_post_solve_dice(const RcCtx& c, const RcLds& L, int i, int j, double& d0, double& d1) {
  const uint32_t key = (uint32_t)(i * 32 + j);
  const dm_u32x4 u = rc_rng(c, L, key | ((j < RC_BALL ? 2u : 3u) << 16));
  d0 = dm_unit(u.v[0]); d1 = dm_unit(u.v[1]);
}
DE_DEV void rc_cb_post_solve(const RcCtx& c, RcLds& L, int i, int j, double dice0, double dice1) {
  if (!c.canFall) return;
  if (j < RC_BALL) {  // robotCollision :1039-1088
    const int r1 = i >> 1, r2 = j >> 1;
    if (r1 == r2) return;
    // both robots' flags and counters in one LDS round trip; rc_fall(r) / rc_penalize(r) only ever change robot r's own
    const int f1 = L.rflags[r1], f2 = L.rflags[r2];
    int t1 = L.touchc[r1], t2 = L.touchc[r2];
    if (!(f1 & (RF_FALLEN | RF_PENAL))) t1 += 1;
    if (!(f2 & (RF_FALLEN | RF_PENAL))) t2 += 1;
    L.touchc[r1] = t1; L.touchc[r2] = t2;
    const bool p1 = f1 & RF_PUSH, p2 = f2 & RF_PUSH;
    if (!(f1 & RF_FALLEN) && rc_dice_exceeds(dice0, p1 ? 0.99995 : 0.9999, p1 ? 5.0001e-5 : 1.0001e-4, t1)) {
      rc_fall(c, r1, p1 ? 1 : 0);
      L.touchc[r1] = 0;
    }
    if (!(f2 & RF_FALLEN) && rc_dice_exceeds(dice1, p2 ? 0.99995 : 0.9999, p2 ? 5.0001e-5 : 1.0001e-4, t2)) {
      rc_fall(c, r2, p2 ? 1 : 0);
      L.touchc[r2] = 0;
    }
    if (p1 != p2) {  // (the pushing bits are not touched by a fall; the fallen bits are: read them again)
      const bool diffTeam = robot_team(L, r1) != robot_team(L, r2);
      if (p1 && (L.rflags[r2] & RF_FALLEN) && diffTeam) { rc_penalize(c, r1); L.touchc[r1] = 0; }
      else if (p2 && (L.rflags[r1] & RF_FALLEN) && diffTeam) { rc_penalize(c, r2); L.touchc[r2] = 0; }
    }
  } else if (j > RC_BALL && i < RC_BALL) {  // goalpostCollision :1106-1125
    const int r = i >> 1;
    int f = L.rflags[r], t = L.touchc[r];
    if (f & RF_FALLEN) { L.touchc[r] = 0; return; }
    if (!(f & RF_TOUCH)) { L.rflags[r] = f | RF_TOUCH; t = 0; }
    t += 1;
    L.touchc[r] = t;
    if (rc_dice_exceeds(dice0, 0.9998, 2.0001e-4, t)) rc_fall(c, r, 1);
  }
}

DE_DEV void rc_cb_separate(RcLds& L, int i, int j) {  // :1091-1103 (Robot-Robot and Robot-Goalpost handlers only)
  if (i < RC_BALL && j != RC_BALL) {
    const int r1 = i >> 1;
    L.rflags[r1] &= ~(RF_TOUCH | RF_PUSH); L.touchc[r1] = 0;
    if (j < RC_BALL) { const int r2 = j >> 1; L.rflags[r2] &= ~(RF_TOUCH | RF_PUSH); L.touchc[r2] = 0; }
  }
}

// ------------------------------------------------------------------------------------------------
// narrowphase (mirrors oracle/cp_lite.c: circle_to_circle, circle_to_segment, segment_to_segment + ContactPoints)
// ------------------------------------------------------------------------------------------------
struct RcContacts {
  int count;
  V2 n, p1[2], p2[2];
  int hash[2];
  bool degenerate;  // capsule cores touched or crossed: the normal is shape 1's own, not a contact normal (error bit 4)
};
struct SegW {
  V2 ta, tb, tn;
};
DE_DEV void seg_world(const RcLds& L, int s, SegW& o) {
  const double ly = (s & 1) ? -10.0 : 10.0;
  const double c = L.crc[s], sn = L.crs[s], x = L.cpx[s], y = L.cpy[s];
  o.ta = v2(c * -10.0 - sn * ly + x, sn * -10.0 + c * ly + y);
  o.tb = v2(c * 10.0 - sn * ly + x, sn * 10.0 + c * ly + y);
  o.tn = v2(c * 0.0 - sn * -1.0, sn * 0.0 + c * -1.0);  // local normal (0,-1)
}
struct RcEdge {
  V2 ap, bp, n;
  int ah, bh;
};
DE_DEV RcEdge support_edge_segment(const SegW& s, int slot, V2 n) {
  RcEdge e;
  const int h = slot * 4;
  if (vdot(s.tn, n) > 0.0) { e.ap = s.ta; e.ah = h + 0; e.bp = s.tb; e.bh = h + 1; e.n = s.tn; }
  else { e.ap = s.tb; e.ah = h + 1; e.bp = s.ta; e.bh = h + 0; e.n = vneg(s.tn); }
  return e;
}
DE_DEV int rc_hash_pair(int a, int b) { return 1 + ((a << 8) | b); }
DE_DEV void rc_contact_points(const RcEdge& e1, const RcEdge& e2, double r1, double r2, V2 n, RcContacts& out) {
  const double d_e1_a = vcross(e1.ap, n), d_e1_b = vcross(e1.bp, n);
  const double d_e2_a = vcross(e2.ap, n), d_e2_b = vcross(e2.bp, n);
  const double e1_denom = 1.0 / (d_e1_b - d_e1_a + DE_DBL_MIN);
  const double e2_denom = 1.0 / (d_e2_b - d_e2_a + DE_DBL_MIN);
  out.n = n;
  out.count = 0;
  {
    V2 p1 = vadd(vmul(n, r1), vlerp(e1.ap, e1.bp, fclamp01_cp((d_e2_b - d_e1_a) * e1_denom)));
    V2 p2 = vadd(vmul(n, -r2), vlerp(e2.ap, e2.bp, fclamp01_cp((d_e1_a - d_e2_a) * e2_denom)));
    double dist = vdot(vsub(p2, p1), n);
    if (dist <= 0.0) { out.p1[0] = p1; out.p2[0] = p2; out.hash[0] = rc_hash_pair(e1.ah, e2.bh); out.count = 1; }
  }
  {
    V2 p1 = vadd(vmul(n, r1), vlerp(e1.ap, e1.bp, fclamp01_cp((d_e2_a - d_e1_a) * e1_denom)));
    V2 p2 = vadd(vmul(n, -r2), vlerp(e2.ap, e2.bp, fclamp01_cp((d_e1_b - d_e2_a) * e2_denom)));
    double dist = vdot(vsub(p2, p1), n);
    if (dist <= 0.0) {
      int h = rc_hash_pair(e1.bh, e2.ah);
      if (out.count == 0) { out.p1[0] = p1; out.p2[0] = p2; out.hash[0] = h; }
      else { out.p1[1] = p1; out.p2[1] = p2; out.hash[1] = h; }
      out.count += 1;
    }
  }
}
DE_DEV void closest_seg_seg(V2 p1, V2 q1, V2 p2, V2 q2, V2& c1, V2& c2) {
  const V2 d1 = vsub(q1, p1), d2 = vsub(q2, p2), r = vsub(p1, p2);
  const double a = vdot(d1, d1), e = vdot(d2, d2), f = vdot(d2, r);
  const double c = vdot(d1, r), b = vdot(d1, d2);
  const double denom = a * e - b * b;
  double s, t;
  if (denom != 0.0) s = fclamp01_cp((b * f - c * e) / denom); else s = 0.0;
  t = (b * s + f) / e;
  if (t < 0.0) { t = 0.0; s = fclamp01_cp(-c / a); }
  else if (t > 1.0) { t = 1.0; s = fclamp01_cp((b - c) / a); }
  c1 = vadd(p1, vmul(d1, s));
  c2 = vadd(p2, vmul(d2, t));
}
DE_DEV bool capsules_far_apart(const SegW& s1, const SegW& s2) {
  const double M = FOOT_RADIUS + FOOT_RADIUS + 1e-3;
  const double da = vdot(vsub(s2.ta, s1.ta), s1.tn), db = vdot(vsub(s2.tb, s1.ta), s1.tn);
  return (da > M && db > M) || (da < -M && db < -M);
}
DE_DEV bool feet_far_apart(const RcLds& L, int r) {
  SegW s1, s2;
  seg_world(L, 2 * r, s1);
  seg_world(L, 2 * r + 1, s2);
  return capsules_far_apart(s1, s2);
}
DE_DEV void rc_narrowphase(const RcLds& L, int i, int j, RcContacts& out) {  // pair i < j in canonical slot order
  out.count = 0;
  out.degenerate = false;
  if (j < RC_BALL) {  // capsule - capsule
    SegW s1, s2;
    seg_world(L, i, s1);
    seg_world(L, j, s2);
    // Separating-axis early out along s1's normal: if both ends of s2 lie on one side of s1's line, further away than the
    // two radii plus a margin far above any rounding of the exact test below, the closest points are further apart than
    // that as well and the pair cannot touch.  This is what the two feet of one robot (a candidate pair in every substep:
    // parallel capsules 20 apart) look like; it spares them the closest-point computation with its four divisions.
    if (capsules_far_apart(s1, s2)) return;
    V2 a, b;
    closest_seg_seg(s1.ta, s1.tb, s2.ta, s2.tb, a, b);
    const V2 delta = vsub(b, a);
    const double dsq = vlensq(delta), mind = FOOT_RADIUS + FOOT_RADIUS;
    if (dsq > mind * mind) return;
    const double d = dm_sqrt(dsq);
    V2 n = (d != 0.0) ? vmul(delta, 1.0 / d) : s1.tn;
    if (dsq < 1e-12) {
      // Cores that touch or CROSS (oracle/cp_lite.c cores_crossing_normal, operation for operation): Chipmunk's EPA answers with the inward
      // normal of the edge of the Minkowski difference closest to the origin = the smallest of the four "one end point back onto the
      // other core's line" translations.  Reached in play by the two feet of one robot that has been knocked about.
      const V2 dA = vsub(s1.tb, s1.ta), dB = vsub(s2.tb, s2.ta);
      const V2 uA = vmul(dA, 1.0 / dm_sqrt(vlensq(dA))), uB = vmul(dB, 1.0 / dm_sqrt(vlensq(dB)));
      const double s0 = vcross(uA, vsub(s2.ta, s1.ta)), s1_ = vcross(uA, vsub(s2.tb, s1.ta));
      const double t0 = vcross(uB, vsub(s1.ta, s2.ta)), t1 = vcross(uB, vsub(s1.tb, s2.ta));
      const bool crossing = s0 * s1_ <= 0.0 && t0 * t1 <= 0.0;
      bool exact0 = false;
      if (crossing) {
        double best = dm_abs(s0);
        n = s0 > 0.0 ? vneg(vperp(uA)) : vperp(uA);
        if (dm_abs(s1_) < best) { best = dm_abs(s1_); n = s1_ > 0.0 ? vneg(vperp(uA)) : vperp(uA); }
        if (dm_abs(t0) < best) { best = dm_abs(t0); n = t0 > 0.0 ? vperp(uB) : vneg(vperp(uB)); }
        if (dm_abs(t1) < best) { best = dm_abs(t1); n = t1 > 0.0 ? vperp(uB) : vneg(vperp(uB)); }
        exact0 = best == 0.0;
      }
      out.degenerate = exact0 || (!crossing && d == 0.0);  // the normal's sign is a convention there: reported, error bit 4
    }
    rc_contact_points(support_edge_segment(s1, i, n), support_edge_segment(s2, j, vneg(n)), FOOT_RADIUS, FOOT_RADIUS, n, out);
  } else if (i < RC_BALL) {  // circle (ball or goalpost) = shape a, capsule foot i = shape b
    const V2 center = v2(L.cpx[j], L.cpy[j]);  // (the ball's shape cache or a goalpost's constant slot)
    const double cr = 10.0;
    SegW s;
    seg_world(L, i, s);
    const V2 seg_delta = vsub(s.tb, s.ta);
    const double closest_t = fclamp01_cp(vdot(seg_delta, vsub(center, s.ta)) / vlensq(seg_delta));
    const V2 closest = vadd(s.ta, vmul(seg_delta, closest_t));
    const double mindist = cr + FOOT_RADIUS;
    const V2 delta = vsub(closest, center);
    const double distsq = vlensq(delta);
    if (distsq < mindist * mindist) {
      const double dist = dm_sqrt(distsq);
      const V2 n = (dist != 0.0) ? vmul(delta, 1.0 / dist) : s.tn;
      out.n = n; out.p1[0] = vadd(center, vmul(n, cr)); out.p2[0] = vadd(closest, vmul(n, -FOOT_RADIUS));
      out.hash[0] = 0; out.count = 1;
    }
  } else {  // ball - goalpost: circle_to_circle (a = ball)
    const V2 c1 = v2(L.cpx[RC_BALL], L.cpy[RC_BALL]), c2 = v2(L.cpx[j], L.cpy[j]);
    const double mindist = BALL_R + POST_R;
    const V2 delta = vsub(c2, c1);
    const double distsq = vlensq(delta);
    if (distsq < mindist * mindist) {
      const double dist = dm_sqrt(distsq);
      const V2 n = (dist != 0.0) ? vmul(delta, 1.0 / dist) : v2(1.0, 0.0);
      out.n = n; out.p1[0] = vadd(c1, vmul(n, BALL_R)); out.p2[0] = vadd(c2, vmul(n, -POST_R));
      out.hash[0] = 0; out.count = 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// body table for the solver
// ------------------------------------------------------------------------------------------------
struct RBody {
  V2 p, v, vb;
  double w, wb, minv, iinv;
};
DE_DEV void rbody_load(const RcLds& L, int idx, RBody& b) {  // (a goalpost's slot holds its position and zero velocities: rc_load_env)
  b.p = v2(L.px[idx], L.py[idx]); b.v = v2(L.vx[idx], L.vy[idx]); b.w = L.w[idx];
  b.vb = v2(L.vbx[idx], L.vby[idx]); b.wb = L.wb[idx]; b.minv = rc_minv(idx); b.iinv = rc_iinv(idx);
}
// The arbiter solver's arithmetic with its multiply-adds FUSED: the dms_* functions of include/dynenv_math.h, the same ones
// oracle/cp_lite.c calls (k_scalar_body_f, relative_velocity_f, apply_impulse_f ...).  (vrotate_f / vdot_f: driving_kernels.hip)
DE_DEV double rk_scalar_body(const RBody& b, V2 r, V2 n) { return dms_k_scalar(b.minv, b.iinv, r.x, r.y, n.x, n.y); }
DE_DEV V2 rrelative_velocity(const RBody& a, const RBody& b, V2 r1, V2 r2) {
  V2 v1 = v2(dms_point_vx(a.v.x, r1.y, a.w), dms_point_vy(a.v.y, r1.x, a.w));
  V2 v2s = v2(dms_point_vx(b.v.x, r2.y, b.w), dms_point_vy(b.v.y, r2.x, b.w));
  return vsub(v2s, v1);
}
DE_DEV void rapply_impulse(RBody& b, V2 j, V2 r) {
  b.v = v2(dm_fma(j.x, b.minv, b.v.x), dm_fma(j.y, b.minv, b.v.y));
  b.w = dm_fma(b.iinv, dms_cross(r.x, r.y, j.x, j.y), b.w);
}
// arbiter material: e = e_a * e_b, u = u_a * u_b in narrowphase order (a = circle / lower slot)
DE_DEV void pair_material(int i, int j, double& e, double& u) {
  if (j < RC_BALL) { e = 0.3 * 0.3; u = 2.5 * 2.5; }
  else if (i < RC_BALL && j == RC_BALL) { e = 0.98 * 0.3; u = 3.0 * 2.5; }
  else if (i < RC_BALL) { e = 0.95 * 0.3; u = 0.0 * 2.5; }
  else { e = 0.98 * 0.95; u = 3.0 * 0.0; }
}

// ------------------------------------------------------------------------------------------------
// Space.step(0.01) after the position update: contacts + joints + velocity update + solver + post-solve callbacks.
// Out of line (large register footprint).  `cand`: my broadphase candidates; returns updated occupancy / error bit.
// ------------------------------------------------------------------------------------------------
// the two constraints of one robot (pivot + rotary limit between its feet), cpPivotJoint.c / cpRotaryLimitJoint.c
struct RcJoint {
  bool hasPivot, pivotFirst;
  double kk0, kk1, kk2, kk3, pbx, pby, iSum, rbias, m, i;
};
struct RcFeet {
  double vx0, vy0, w0, vx1, vy1, w1;
};
DE_DEV bool is_negzero(double x) { return __double_as_longlong(x) == (long long)0x8000000000000000ull; }
DE_DEV bool is_finite(double x) { return __builtin_fabs(x) < INFINITY; }
// precondition of the <CLEAN = true> joint arithmetic
DE_DEV bool feet_clean(const RcFeet& f) {
  return !(is_negzero(f.vx0) || is_negzero(f.vy0) || is_negzero(f.w0) || is_negzero(f.vx1) || is_negzero(f.vy1) || is_negzero(f.w1)) &&
         is_finite(f.w0) && is_finite(f.w1);
}
// ord 0 / 1: first / second constraint in the space's constraint order.
// CLEAN: the caller has checked that none of the six foot velocities is -0 and that both angular velocities are finite.
// The pivot's anchors are the body origins (r1 = r2 = 0), so cpPivotJoint's "v + perp(r) * w" adds (+-0, +-0) to each
// velocity and its angular impulse "i_inv * cross(r, j)" adds +-0 to each w.  x + (+-0) is x bit for bit unless x is -0,
// and a sum or difference is -0 only if both operands are zeros, so "no -0" survives every update in here: the 18 fp64
// operations that only produce those zeros are dropped (the caller verifies afterwards that no impulse became inf/NaN,
// the one case in which 0 * j would not have been a zero, and otherwise redoes the solve with CLEAN = false).
template <bool CLEAN>
DE_DEV void pivot_warm_start(const RcJoint& J, RcFeet& f, double jx, double jy) {
  if (J.hasPivot) {
    const V2 j = vmul(v2(jx, jy), 1.0);
    f.vx0 = dm_fma(-j.x, J.m, f.vx0); f.vy0 = dm_fma(-j.y, J.m, f.vy0);
    if (!CLEAN) f.w0 = dm_fma(J.i, dms_cross(0.0, 0.0, -j.x, -j.y), f.w0);
    f.vx1 = dm_fma(j.x, J.m, f.vx1); f.vy1 = dm_fma(j.y, J.m, f.vy1);
    if (!CLEAN) f.w1 = dm_fma(J.i, dms_cross(0.0, 0.0, j.x, j.y), f.w1);
  }
}
DE_DEV void rotary_warm_start(const RcJoint& J, RcFeet& f, double jr) {
  const double j = jr * 1.0;
  f.w0 = dm_fma(-j, J.i, f.w0);
  f.w1 = dm_fma(j, J.i, f.w1);
}
template <bool CLEAN>
DE_DEV void pivot_iterate(const RcJoint& J, RcFeet& f, double& jx, double& jy) {
  if (J.hasPivot) {
    // relative_velocity with r1 = r2 = 0
    const V2 v1s = CLEAN ? v2(f.vx0, f.vy0) : v2(dms_point_vx(f.vx0, 0.0, f.w0), dms_point_vy(f.vy0, 0.0, f.w0));
    const V2 v2s = CLEAN ? v2(f.vx1, f.vy1) : v2(dms_point_vx(f.vx1, 0.0, f.w1), dms_point_vy(f.vy1, 0.0, f.w1));
    const V2 vr = vsub(v2s, v1s);
    const V2 d = vsub(v2(J.pbx, J.pby), vr);
    V2 j = v2(dm_fma(d.x, J.kk0, d.y * J.kk1), dm_fma(d.x, J.kk2, d.y * J.kk3));
    const V2 jOld = v2(jx, jy);
    jx = jx + j.x; jy = jy + j.y;
    j = vsub(v2(jx, jy), jOld);
    f.vx0 = dm_fma(-j.x, J.m, f.vx0); f.vy0 = dm_fma(-j.y, J.m, f.vy0);
    if (!CLEAN) f.w0 = dm_fma(J.i, dms_cross(0.0, 0.0, -j.x, -j.y), f.w0);
    f.vx1 = dm_fma(j.x, J.m, f.vx1); f.vy1 = dm_fma(j.y, J.m, f.vy1);
    if (!CLEAN) f.w1 = dm_fma(J.i, dms_cross(0.0, 0.0, j.x, j.y), f.w1);
  }
}
DE_DEV void rotary_iterate(const RcJoint& J, RcFeet& f, double& jr) {
  if (J.rbias != 0.0) {
    const double wr = f.w1 - f.w0;
    const double jOld = jr;
    const double s = dm_fma(-(J.rbias + wr), J.iSum, jOld);
    if (J.rbias < 0.0) jr = fmax_cp(s, 0.0); else jr = fmin_cp(s, 0.0);
    const double j = jr - jOld;
    f.w0 = dm_fma(-j, J.i, f.w0);
    f.w1 = dm_fma(j, J.i, f.w1);
  }
}
// general path: both constraints of this robot in the space's constraint order.  The pivot block is issued once for all
// lanes, between the rotary block of the rotary-first robots and that of the pivot-first ones.
DE_DEV void joints_warm_start_ordered(const RcJoint& J, RcFeet& f, double jx, double jy, double jr) {
  if (!J.pivotFirst) rotary_warm_start(J, f, jr);
  pivot_warm_start<false>(J, f, jx, jy);
  if (J.pivotFirst) rotary_warm_start(J, f, jr);
}
DE_DEV void joints_iterate_ordered(const RcJoint& J, RcFeet& f, double& jx, double& jy, double& jr) {
  if (!J.pivotFirst) rotary_iterate(J, f, jr);
  pivot_iterate<false>(J, f, jx, jy);
  if (J.pivotFirst) rotary_iterate(J, f, jr);
}

DE_DEV void joint_prestep(const RcLds& L, int lane, RcJoint& J, double& jx, double& jy, double& jr) {
  const int la = 2 * lane, lb = 2 * lane + 1;
  J.hasPivot = !(L.rflags[lane] & RF_JREM);
  J.pivotFirst = (L.envi[RE_PIVFIRST] >> lane) & 1;
  jx = L.jx[lane]; jy = L.jy[lane]; jr = L.jrot[lane];
  J.m = RC.footMinv; J.i = RC.footIinv;  // both feet: same mass and inertia
  J.kk0 = J.kk1 = J.kk2 = J.kk3 = 0.0; J.pbx = J.pby = 0.0;
  if (J.hasPivot) {
    // anchors are the body origins (PivotJoint(a, b, pos) with both bodies at pos): r1 = r2 = 0, so K^-1 is the
    // per-build constant RC.jkk* (dynenv_capi.hip computes it with cpPivotJoint's own operation order)
    J.kk0 = RC.jkk0; J.kk1 = RC.jkk1; J.kk2 = RC.jkk2; J.kk3 = RC.jkk3;
    const V2 pr1 = v2(0.0, 0.0), pr2 = v2(0.0, 0.0);
    const V2 delta = vsub(vadd(v2(L.px[lb], L.py[lb]), pr2), vadd(v2(L.px[la], L.py[la]), pr1));
    J.pbx = delta.x * (-DE_PIVOT_BIAS_COEF / DE_DT); J.pby = delta.y * (-DE_PIVOT_BIAS_COEF / DE_DT);
  }
  {
    const double dist = L.ang[lb] - L.ang[la];
    double pdist = 0.0;
    if (dist > 0.0) pdist = 0.0 - dist; else if (dist < 0.0) pdist = 0.0 - dist;
    J.iSum = RC.jiSum;
    J.rbias = -DE_JOINT_BIAS_COEF * pdist / DE_DT;
    if (J.rbias == 0.0) jr = 0.0;
  }
}

// The common substep: no active arbiter.  Joints couple only the two feet of one robot, so each robot lane is independent
// of every other lane: prestep, warm start and all 10 iterations run on registers (same arithmetic as the general path
// in rc_physics, no LDS round trips, no barriers).  Out of line so that it gets its own small register allocation
// instead of sharing rc_physics' (whose arbiter state pushed the joint constants to scratch inside the iteration loop).
// Warm start + 10 iterations of one robot's two constraints, in registers.  A robot runs (pivot, rotary) or (rotary, pivot)
// per iteration depending on where its pivot sits in the constraint list (it moves to the end when a kick re-adds it).
// Lanes of both kinds share one instruction stream: the rotary-first lanes take their first rotary pass up front, then
// every lane alternates pivot, rotary - each lane still sees exactly its own sequence (R P R P ... R P resp. P R ... P R),
// and each block is issued once per iteration instead of once per order.
template <bool CLEAN>
DE_DEV void joints_solve(const RcJoint& J, RcFeet& f, double& jx, double& jy, double& jr) {
  if constexpr (CLEAN) {
    // CLEAN: the pivot reads and writes (vx, vy) only, the rotary limit w only (pivot_warm_start's comment): two independent chains of a
    // warm start + ten iterations each, the same in either constraint order - no `pivotFirst` bookkeeping, no branch per order.
    // Fixed-point exit: an iteration that leaves the three accumulated impulses where they were has applied impulses of +-0 to
    // velocities none of which is -0: it changed nothing, and every later one - a function of the same state - changes nothing either.
    // All robots of the wave must have got there: the lanes share the loop.  A walking robot's pivot is solved exactly by its first
    // pass up to rounding; the second or third pass adds zero.
    rotary_warm_start(J, f, jr);
    pivot_warm_start<true>(J, f, jx, jy);
#pragma unroll 1
    for (int iter = 0; iter < 10; ++iter) {
      const double jx0 = jx, jy0 = jy, jr0 = jr;
      pivot_iterate<true>(J, f, jx, jy);
      rotary_iterate(J, f, jr);
      if (__ballot(!(jx == jx0 && jy == jy0 && jr == jr0)) == 0ull) break;
    }
    return;
  }
  const bool pf = J.pivotFirst;
  if (!pf) rotary_warm_start(J, f, jr);
  pivot_warm_start<CLEAN>(J, f, jx, jy);
  if (pf) rotary_warm_start(J, f, jr);
  if (!pf) rotary_iterate(J, f, jr);
  // CLEAN: fixed-point exit.  An iteration (pivot, rotary) that leaves the three accumulated impulses where they were has applied
  // impulses jNew - jOld = 0 to the feet: x + (+-0) is x bit for bit since no velocity is -0 (the CLEAN invariant), so the
  // iteration changed nothing - and every later one, a function of the same state, changes nothing either (also the last one
  // of a rotary-first robot, which lacks its rotary half).  All robots of the wave must have got there: the lanes share the loop.
  // A walking robot's pivot is solved exactly by its first pass up to rounding; the second or third pass adds zero.
#pragma unroll 1
  for (int iter = 0; iter < 10; ++iter) {
    const double jx0 = jx, jy0 = jy, jr0 = jr;
    pivot_iterate<CLEAN>(J, f, jx, jy);
    if (pf || iter < 9) rotary_iterate(J, f, jr);
    if (CLEAN && __ballot(!(jx == jx0 && jy == jy0 && jr == jr0)) == 0ull) break;
  }
}
DE_DEV void rc_joints_only_inl(int lane, int R) {
  RcLds& L = g_R;
  if (lane < R) {
    const int la = 2 * lane, lb = 2 * lane + 1;
    RcJoint J;
    double jx, jy, jr;
    joint_prestep(L, lane, J, jx, jy, jr);
    RcFeet f;
    f.vx0 = L.vx[la]; f.vy0 = L.vy[la]; f.w0 = L.w[la]; f.vx1 = L.vx[lb]; f.vy1 = L.vy[lb]; f.w1 = L.w[lb];
    // fast path (see joint_iterate): no -0 among the velocities, finite w, finite accumulated impulses
    bool clean = feet_clean(f) && is_finite(jx) && is_finite(jy);
    if (clean) {
      joints_solve<true>(J, f, jx, jy, jr);
      // every pivot impulse that was applied is a difference of finite jx / jy values iff these stayed finite
      clean = is_finite(jx) && is_finite(jy) && is_finite(f.vx0) && is_finite(f.vy0) && is_finite(f.vx1) && is_finite(f.vy1) &&
              is_finite(f.w0) && is_finite(f.w1);
      if (!clean) {  // never seen; redo from the unchanged LDS state with the reference's full arithmetic
        joint_prestep(L, lane, J, jx, jy, jr);
        f.vx0 = L.vx[la]; f.vy0 = L.vy[la]; f.w0 = L.w[la]; f.vx1 = L.vx[lb]; f.vy1 = L.vy[lb]; f.w1 = L.w[lb];
      }
    }
    if (!clean) joints_solve<false>(J, f, jx, jy, jr);
    L.vx[la] = f.vx0; L.vy[la] = f.vy0; L.w[la] = f.w0; L.vx[lb] = f.vx1; L.vy[lb] = f.vy1; L.w[lb] = f.w1;
    L.jx[lane] = jx; L.jy[lane] = jy; L.jrot[lane] = jr;
  }
}

// out of line where it runs inside the general path's caller (its own small register allocation)
DE_OOL void rc_joints_only_ool(int lane, int R) { rc_joints_only_inl(lane, R); }

#ifdef DRV_PROFILE
#define RC_PROF(...) __VA_ARGS__
#else
#define RC_PROF(...)
#endif
RC_PROF(__device__ unsigned long long g_rcprof[4096 * 12];)
RC_PROF(__device__ unsigned long long g_rcprof2[4096 * 8];)  // stages of "contacts + prestep", summed over the step's rc_physics calls
RC_PROF(__device__ unsigned long long g_rcprof3[4096 * 8];)  // stages of the common part: game logic | position + shape cache | broadphase | quiet test | velocity | quiet joints | quiet substeps | calls
struct RcStepRet {
  uint64_t occ;
  int err;
};

DE_DEV RcStepRet rc_physics_inl(RcCtx c, int lane, int cand, uint64_t pairLo, uint64_t pairHi, uint64_t occ) {
  // The two impulse chains of an arbiter's contact - velocity (normal + tangent) and position correction (bias) -
  // read and write disjoint body fields (v, w against v_bias, w_bias) and run the same instruction sequence up to the
  // impulse vector; a lone wave pays per instruction, not per lane, so the bias chain runs on lane slot + 16 beside
  // the velocity chain on lane slot.
  RcLds& L = g_R;
  RcMailbox& M = L.u.mb;
  int err = 0;
  bool biasLane = false;
  const bool anyContactWork = wave_ballot(cand != 0) != 0ull || occ != 0ull;
RC_PROF(const unsigned long long T0 = __builtin_amdgcn_s_memtime(); unsigned long long C0 = T0, C1 = T0, C2 = T0, C3 = T0, C4 = T0;)
  // --- contact detection / cache -------------------------------------------------------------------------
  bool touched = false, slotOcc = false, freeMe = false, active = false;
  int bodyA = 0, bodyB = 0, a_pair = 0xFFFF, a_state = ARB_FIRST_, a_count = 0, a_age = 0, rank = 0, nTouched = 0;
  int arank = 0, nActive = 0;  // canonical order among the active arbiters (cached with the levels)
  int myLevel = 0, maxLevel = -1;
  double jn[2] = {0.0, 0.0}, jt[2] = {0.0, 0.0};
  double nMass[2] = {0.0, 0.0}, tMass[2] = {0.0, 0.0}, bias[2] = {0.0, 0.0}, bounce[2] = {0.0, 0.0};
  double arb_e = 0.0, arb_u = 0.0;
  V2 n = v2(0.0, 0.0), r1[2], r2[2];
  r1[0] = r1[1] = r2[0] = r2[1] = v2(0.0, 0.0);
  uint64_t touchedMask = 0ull, activeMask = 0ull;
  if (anyContactWork) {
    // Compact the candidates of all rounds into one dense list in canonical order (round-major, lane-minor = pair index
    // order), so that the narrowphase runs once over up to 64 pairs instead of once per round that holds a candidate
    // (the two feet of one robot are a candidate pair in every substep).  candList is a member of its own, kept from call to call
    // within a launch: it stays valid while every lane's candidate mask is the one it was built from (lastCand / candN).
    unsigned short* cl = L.candList;
    int nCand = 0;
    const int prevCand = (int)L.lastCand[lane], savedN = uniform_i(L.candN);
    int spair = lane < RC_NS ? L.s_pair[lane] : -1;  // the slots' pairs for the slot search (one load, then v_readlane per occupied slot)
    if (lane < RC_NS) M.flag[lane] = 0;
    if (savedN >= 0 && wave_ballot(prevCand != (cand & 0xFF)) == 0ull) nCand = savedN;  // same masks as when the list was built: it is still there
    else {
    // (straight-line over the five rounds: five ballots, v_mbcnt, masked stores - no loop-carried wait, no branch per round)
#pragma unroll
    for (int t = 0; t < RC_NPAIR_ROUNDS; ++t) {
      const bool cbit = (cand >> t) & 1;
      const uint64_t m = wave_ballot(cbit);
      if (cbit) {
        const int idx = nCand + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (idx < 128) cl[idx] = (unsigned short)RC_MY_PAIR(t); else err |= 1;  // overflow is reported through RE_ERR
      }
      nCand += __popcll(m);
    }
    L.lastCand[lane] = (unsigned char)(cand & 0xFF);
    if (lane == 0) L.candN = nCand <= 128 ? nCand : -1;  // (an overflow is reported by every build)
    if (nCand > 128) nCand = 128;
    }
    __syncthreads();
RC_PROF(C0 = __builtin_amdgcn_s_memtime();)
#pragma unroll 1
    for (int pass = 0; pass * DE_WAVE < nCand; ++pass) {
      const int pr = pass * DE_WAVE + lane < nCand ? (int)cl[pass * DE_WAVE + lane] : 0xFFFF;
      const bool isCand = pr != 0xFFFF;
      RcContacts ct;
      ct.count = 0; ct.degenerate = false;
      if (isCand) rc_narrowphase(L, pr >> 8, pr & 0xFF, ct);
      const bool touch = isCand && ct.count > 0;
      if (wave_ballot(touch) == 0ull) continue;
      if (ct.degenerate) err |= 16;  // (a degenerate pair always has contacts: the check sits behind the early continue)
      int slot = -1;
      for (uint64_t mm = occ; mm; mm &= mm - 1) {
        int sidx = __builtin_ctzll(mm);
        if (bcast_i(spair, sidx) == pr) slot = sidx;
      }
      if (!touch) slot = -1;
      const bool needNew = touch && slot < 0;
      const uint64_t newMask = wave_ballot(needNew);
      if (newMask) {
        const uint64_t slotBits = (1ull << RC_NS) - 1ull;
        int rk = __popcll(newMask & lanemask_lt());
        uint64_t fm = (~occ) & slotBits;
        if (needNew) {
          for (int r = 0; r < rk; ++r) fm &= fm - 1;
          if (fm) { slot = __builtin_ctzll(fm); L.s_pair[slot] = pr; }
          else err |= 1;
        }
        int cnt = __popcll(newMask);
        uint64_t fm2 = (~occ) & slotBits;
        for (int r = 0; r < cnt && fm2; ++r) { occ |= (fm2 & (~fm2 + 1)); fm2 &= fm2 - 1; }
        spair = lane < RC_NS ? L.s_pair[lane] : -1;  // (slots were handed out: a later pass must see their pairs)
      }
      if (touch && slot >= 0) {
        M.flag[slot] = needNew ? 3 : 1;
        M.count[slot] = ct.count;
        M.nx[slot] = ct.n.x; M.ny[slot] = ct.n.y;
        M.p1x[slot][0] = ct.p1[0].x; M.p1y[slot][0] = ct.p1[0].y; M.p2x[slot][0] = ct.p2[0].x; M.p2y[slot][0] = ct.p2[0].y;
        M.hash[slot][0] = ct.hash[0];
        if (ct.count > 1) {
          M.p1x[slot][1] = ct.p1[1].x; M.p1y[slot][1] = ct.p1[1].y; M.p2x[slot][1] = ct.p2[1].x; M.p2y[slot][1] = ct.p2[1].y;
          M.hash[slot][1] = ct.hash[1];
        }
      }
      __syncthreads();
    }
    __syncthreads();
RC_PROF(C1 = __builtin_amdgcn_s_memtime();)
    // the cached schedule's key and values: loads issued here, used at the levels below
    const unsigned long long c_active = L.sActive;
    const int c_maxLevel = L.sMaxLevel;
    const int c_level = lane < RC_NS ? (int)L.sLevel[lane] : 0;
    // slot lanes: load the cached arbiter, match hashes (cpArbiterUpdate without the r1/r2 part, see below)
    slotOcc = lane < RC_NS && ((occ >> lane) & 1ull);
    int cnt = 0;
    if (slotOcc) {
      const int flag = M.flag[lane];
      touched = flag != 0;
      a_pair = L.s_pair[lane];
      const int meta = L.s_meta[lane];
      a_state = meta & 0xFF; a_count = (meta >> 8) & 0xFF; a_age = (meta >> 16) & 0xFF;
      if (flag & 2) { a_state = ARB_FIRST_; a_count = 0; a_age = 0; }
      if (touched) {
        const int i = a_pair >> 8, j = a_pair & 0xFF;
        if (j < RC_BALL) { bodyA = i; bodyB = j; }       // capsule-capsule: a = lower slot
        else if (i < RC_BALL) { bodyA = j; bodyB = i; }  // circle (ball/post) is shape a, the foot shape b
        else { bodyA = i; bodyB = j; }                   // ball - post
        pair_material(i, j, arb_e, arb_u);
        cnt = M.count[lane];
        const int h0 = M.hash[lane][0], h1 = cnt > 1 ? M.hash[lane][1] : 0;
        const int oh0 = L.s_hash0[lane], oh1 = L.s_hash1[lane];
        if (a_count > 0 && h0 == oh0) { jn[0] = L.s_jn0[lane]; jt[0] = L.s_jt0[lane]; }
        if (a_count > 1 && h0 == oh1) { jn[0] = L.s_jn1[lane]; jt[0] = L.s_jt1[lane]; }
        if (cnt > 1) {
          if (a_count > 0 && h1 == oh0) { jn[1] = L.s_jn0[lane]; jt[1] = L.s_jt0[lane]; }
          if (a_count > 1 && h1 == oh1) { jn[1] = L.s_jn1[lane]; jt[1] = L.s_jt1[lane]; }
        }
        n = v2(M.nx[lane], M.ny[lane]);
        a_count = cnt;
        L.s_hash0[lane] = h0; L.s_hash1[lane] = h1;
        if (a_state == ARB_CACHED_) a_state = ARB_FIRST_;
        a_age = 0;
      }
    }
RC_PROF(C2 = __builtin_amdgcn_s_memtime();)
    touchedMask = wave_ballot(touched);
    nTouched = __popcll(touchedMask);
    // (the rank - canonical order among the touched arbiters - is needed by the begin callbacks and by a level computation; a call
    //  without a first contact whose active set is the previous evaluation's needs neither)
    if (wave_ballot(touched && a_state == ARB_FIRST_) != 0ull) {
      for (uint64_t mm = touchedMask; mm; mm &= mm - 1) {
        int b = __builtin_ctzll(mm);
        int pk = bcast_i(a_pair, b);
        rank += (pk < a_pair) ? 1 : 0;
      }
    }
    // canonical order: r1/r2 relative to the bodies' CURRENT positions (an earlier begin callback may have teleported
    // a robot: ballCollision -> penalize), then the begin callback of first contacts (scalar, lane 0)
    // (no first contact among the touched arbiters - the usual case - means no begin callback, nothing moves a body in between,
    //  and every touched lane takes its r1 / r2 at once instead of one lane after the other with an LDS round trip each)
    const bool anyFirst = wave_ballot(touched && a_state == ARB_FIRST_) != 0ull;
    for (int k = 0; k < (anyFirst ? nTouched : (nTouched ? 1 : 0)); ++k) {
      const uint64_t who = wave_ballot(touched && rank == k);
      const int b = __builtin_ctzll(who);
      if (anyFirst ? lane == b : touched) {
        const V2 pa = v2(L.px[bodyA], L.py[bodyA]), pb = v2(L.px[bodyB], L.py[bodyB]);
        r1[0] = vsub(v2(M.p1x[lane][0], M.p1y[lane][0]), pa);
        r2[0] = vsub(v2(M.p2x[lane][0], M.p2y[lane][0]), pb);
        if (a_count > 1) {
          r1[1] = vsub(v2(M.p1x[lane][1], M.p1y[lane][1]), pa);
          r2[1] = vsub(v2(M.p2x[lane][1], M.p2y[lane][1]), pb);
        }
      }
      if (!anyFirst) break;
      const int st = bcast_i(a_state, b);
      if (st != ARB_FIRST_) continue;
      const int pk = bcast_i(a_pair, b);
      if (lane == 0) rc_cb_begin(c, L, pk >> 8, pk & 0xFF);  // every RoboCup begin handler returns True
      __syncthreads();
    }
    // separate callbacks + expiry of untouched slots, canonical order over ALL occupied slots
    if (slotOcc && !touched) {
      a_age += 1;
      if (a_age >= 3) freeMe = true;
    }
    {
      const bool sepMe = slotOcc && !touched && a_state != ARB_CACHED_;
      const uint64_t sepMask = wave_ballot(sepMe);
      if (sepMask) {
        int srank = 0;
        for (uint64_t mm = sepMask; mm; mm &= mm - 1) {
          int b = __builtin_ctzll(mm);
          int pk = bcast_i(a_pair, b);
          srank += (pk < a_pair) ? 1 : 0;
        }
        const int ns = __popcll(sepMask);
        for (int k = 0; k < ns; ++k) {
          const uint64_t who = wave_ballot(sepMe && srank == k);
          const int b = __builtin_ctzll(who);
          const int pk = bcast_i(a_pair, b);
          if (lane == 0) rc_cb_separate(L, pk >> 8, pk & 0xFF);
          __syncthreads();
        }
      }
      if (sepMe) a_state = ARB_CACHED_;
    }
RC_PROF(C3 = __builtin_amdgcn_s_memtime();)
    // levels of the active arbiters
    active = touched && a_state != ARB_IGNORE_;
    activeMask = wave_ballot(active);
    // The schedule is a function of the active arbiters' pairs alone.  sActive is the active mask of the PREVIOUS evaluation (every
    // one records its own; slots only change in evaluations).  An arbiter active in two consecutive evaluations was touched in both,
    // so its slot was neither freed nor handed out again in between: same mask, same pairs, same schedule.
    const bool lvHit = uniform_u64(c_active) == activeMask;
    nActive = __popcll(activeMask);
    if (!lvHit && lane == 0) L.sActive = activeMask;
    if (lvHit) { myLevel = c_level & 15; arank = c_level >> 4; maxLevel = uniform_i(c_maxLevel); }
    else {
    for (uint64_t mm = activeMask; mm; mm &= mm - 1) {  // canonical order among the ACTIVE arbiters (ascending pair id)
      int b = __builtin_ctzll(mm);
      int pk = bcast_i(a_pair, b);
      arank += (pk < a_pair) ? 1 : 0;
    }
    int blvl = 0;
    for (int k = 0; k < nActive; ++k) {
      const uint64_t who = wave_ballot(active && arank == k);
      const int b = __builtin_ctzll(who);
      const int ba = bcast_i(bodyA, b), bb2 = bcast_i(bodyB, b);
      const int la = ba <= RC_BALL ? bcast_i(blvl, ba) : 0;
      const int lb = bb2 <= RC_BALL ? bcast_i(blvl, bb2) : 0;
      const int lv = la > lb ? la : lb;
      if (lane == b) myLevel = lv;
      if (lane == ba || lane == bb2) blvl = lv + 1;
      maxLevel = lv > maxLevel ? lv : maxLevel;
    }
    if (lane < RC_NS) L.sLevel[lane] = (unsigned char)(myLevel | (arank << 4));  // (RC_NS = 16 slots: both fit four bits)
    if (lane == 0) L.sMaxLevel = maxLevel;
    }
RC_PROF(C4 = __builtin_amdgcn_s_memtime();)
    // arbiter prestep
    if (active) {
      RBody a, b;
      rbody_load(L, bodyA, a);
      rbody_load(L, bodyB, b);
      const V2 body_delta = vsub(b.p, a.p);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (q < a_count) {
          nMass[q] = 1.0 / (rk_scalar_body(a, r1[q], n) + rk_scalar_body(b, r2[q], n));
          tMass[q] = 1.0 / (rk_scalar_body(a, r1[q], vperp(n)) + rk_scalar_body(b, r2[q], vperp(n)));
          const double dist = vdot_f(vadd(vsub(r2[q], r1[q]), body_delta), n);
          bias[q] = -DE_CONTACT_BIAS_COEF * fmin_cp(0.0, dist + DE_COLLISION_SLOP) / DE_DT;
          bounce[q] = vdot_f(rrelative_velocity(a, b, r1[q], r2[q]), n) * arb_e;
        }
      }
    }
    if (activeMask != 0ull) {  // hand every active arbiter's bias chain to lane slot + 16
      RcArbShare& H = L.u.sh;  // overlays the mailbox, which nobody reads any more
      __syncthreads();
      if (active) {
        H.code[lane] = bodyA | (bodyB << 8) | (a_count << 16) | (myLevel << 24);
        double* d = H.d[lane];
        d[0] = n.x; d[1] = n.y; d[2] = r1[0].x; d[3] = r1[0].y; d[4] = r1[1].x; d[5] = r1[1].y;
        d[6] = r2[0].x; d[7] = r2[0].y; d[8] = r2[1].x; d[9] = r2[1].y;
        d[10] = nMass[0]; d[11] = nMass[1]; d[12] = bias[0]; d[13] = bias[1];
      }
      __syncthreads();
      static_assert(RC_NS == 16, "the bias lanes are the 16 lanes above the slot lanes, below the joint lanes");
      const int sl = lane - 16;
      if (sl >= 0 && sl < RC_NS && ((activeMask >> sl) & 1ull)) {
        biasLane = true;
        const int code = H.code[sl];
        bodyA = code & 0xFF; bodyB = (code >> 8) & 0xFF; a_count = (code >> 16) & 0xFF; myLevel = (code >> 24) & 0xFF;
        const double* d = H.d[sl];
        n = v2(d[0], d[1]); r1[0] = v2(d[2], d[3]); r1[1] = v2(d[4], d[5]); r2[0] = v2(d[6], d[7]); r2[1] = v2(d[8], d[9]);
        nMass[0] = d[10]; nMass[1] = d[11];
        // the bias chain in the velocity chain's form: jbn = (bias - vbn) nMass = -((-bias) + vbn) nMass (the two can only
        // differ in the sign of a zero jbn, which jBias = max(jBias + jbn, 0) with jBias >= +0 absorbs); no tangent part.
        // The accumulated bias impulse jBias, zero at the prestep, lives in this lane's jn.
        bounce[0] = -d[12]; bounce[1] = -d[13];
        jn[0] = jn[1] = jt[0] = jt[1] = 0.0; tMass[0] = tMass[1] = 0.0; arb_u = 0.0;
      }
    }
  }
RC_PROF(const unsigned long long T1 = __builtin_amdgcn_s_memtime();)
  // --- joints: prestep (cpPivotJoint / cpRotaryLimitJoint preStep), one robot per lane ------------------------
  const bool jointsOnly = activeMask == 0ull;  // then rc_joints_only_ool() below does prestep + solve out of line
  // General path: robot r's joints live on lane 32 + r.  Those lanes are never slot lanes (RC_NS <= 32), so the joint's
  // state OVERLAYS the registers that hold arbiter state on the slot lanes (jn/jt <-> accumulated joint impulses,
  // nMass/tMass <-> pivot K^-1, bias <-> pivot bias, bounce <-> iSum / rotary bias).  Holding both sets at once pushed
  // the joint constants to scratch inside the iteration loop.
  static_assert(RC_NS <= RC_JOINT_LANE0 && RC_JOINT_LANE0 + RC_MAXR <= DE_WAVE, "joint lanes must not be slot lanes");
  const int rl = lane - RC_JOINT_LANE0;
  const bool isRobot = rl >= 0 && rl < c.R && !jointsOnly;
  bool hasPivot = false, pivotFirst = true;
  if (isRobot) {
    RcJoint Jp;
    joint_prestep(L, rl, Jp, jn[0], jn[1], jt[0]);
    hasPivot = Jp.hasPivot; pivotFirst = Jp.pivotFirst;
    nMass[0] = Jp.kk0; nMass[1] = Jp.kk1; tMass[0] = Jp.kk2; tMass[1] = Jp.kk3; bias[0] = Jp.pbx; bias[1] = Jp.pby;
    bounce[0] = Jp.iSum; bounce[1] = Jp.rbias;
  }
#define RC_JOINT_VIEW(J)                                                                                       \
  RcJoint J;                                                                                                   \
  J.hasPivot = hasPivot; J.pivotFirst = pivotFirst; J.kk0 = nMass[0]; J.kk1 = nMass[1]; J.kk2 = tMass[0];      \
  J.kk3 = tMass[1]; J.pbx = bias[0]; J.pby = bias[1]; J.iSum = bounce[0]; J.rbias = bounce[1];                 \
  J.m = RC.footMinv; J.i = RC.footIinv;
  __syncthreads();
RC_PROF(const unsigned long long T2 = __builtin_amdgcn_s_memtime();)
  // --- velocity update ------------------------------------------------------------------------------------
  if (lane <= RC_BALL && (lane == RC_BALL || lane < 2 * c.R)) rc_velocity_update(L, lane);
  __syncthreads();
RC_PROF(const unsigned long long T3 = __builtin_amdgcn_s_memtime(); unsigned long long T4 = T3;)
  const int la = 2 * rl, lb = 2 * rl + 1;
  if (jointsOnly) {
RC_PROF(T4 = __builtin_amdgcn_s_memtime();)
    rc_joints_only_ool(lane, c.R);
  } else {
    // --- warm start: arbiters (level by level), then joints -------------------------------------------------
    bool jointsDirty = false;
    {
      // (only v and w change; a goalpost reads its zeros and writes to the scratch slot, as in the iterations below)
      const int nLvW = uniform_i(maxLevel) + 1;
      const int wa = bodyA <= RC_BALL ? bodyA : RC_NB - 1, wb_ = bodyB <= RC_BALL ? bodyB : RC_NB - 1;
      for (int lv = 0; lv < nLvW; ++lv) {
        if (active && myLevel == lv && a_state != ARB_FIRST_) {
          RBody a, b;
          a.v = v2(L.vx[bodyA], L.vy[bodyA]); a.w = L.w[bodyA]; a.minv = rc_minv(bodyA); a.iinv = rc_iinv(bodyA);
          b.v = v2(L.vx[bodyB], L.vy[bodyB]); b.w = L.w[bodyB]; b.minv = rc_minv(bodyB); b.iinv = rc_iinv(bodyB);
          {
            V2 j = vrotate_f(n, v2(jn[0], jt[0]));
            j = vmul(j, 1.0);
            rapply_impulse(a, vneg(j), r1[0]);
            rapply_impulse(b, j, r2[0]);
          }
          if (a_count > 1) {
            V2 j = vrotate_f(n, v2(jn[1], jt[1]));
            j = vmul(j, 1.0);
            rapply_impulse(a, vneg(j), r1[1]);
            rapply_impulse(b, j, r2[1]);
          }
          L.vx[wa] = a.v.x; L.vy[wa] = a.v.y; L.w[wa] = a.w;
          L.vx[wb_] = b.v.x; L.vy[wb_] = b.v.y; L.w[wb_] = b.w;
        }
        __syncthreads();
      }
    }
    if (isRobot) {  // both constraints of a robot in one LDS round trip: nobody else touches its feet in between
      RC_JOINT_VIEW(J)
      RcFeet f;
      f.vx0 = L.vx[la]; f.vy0 = L.vy[la]; f.w0 = L.w[la]; f.vx1 = L.vx[lb]; f.vy1 = L.vy[lb]; f.w1 = L.w[lb];
      joints_warm_start_ordered(J, f, jn[0], jn[1], jt[0]);
      L.vx[la] = f.vx0; L.vy[la] = f.vy0; L.w[la] = f.w0; L.vx[lb] = f.vx1; L.vy[lb] = f.vy1; L.w[lb] = f.w1;
      jointsDirty = !(feet_clean(f) && is_finite(jn[0]) && is_finite(jn[1]));
    }
    __syncthreads();
RC_PROF(T4 = __builtin_amdgcn_s_memtime();)
    // --- 10 iterations: all arbiters (canonical order via levels), then all constraints ----------------------
    RBody a, b;
    // velocity lanes (the slot lanes) work on (v, w), bias lanes on (v_bias, w_bias): same code, other fields
    double* const fX = biasLane ? L.vbx : L.vx;
    double* const fY = biasLane ? L.vby : L.vy;
    double* const fW = biasLane ? L.wb : L.w;
    const bool solveMe = active || biasLane;
    const bool aDyn = bodyA <= RC_BALL, bDyn = bodyB <= RC_BALL;
    a.minv = rc_minv(bodyA); a.iinv = rc_iinv(bodyA); b.minv = rc_minv(bodyB); b.iinv = rc_iinv(bodyB);  // (0 for a goalpost)
    a.v = b.v = v2(0.0, 0.0); a.w = b.w = 0.0;
    {
      // A static partner (a goalpost) reads the zeros of its own, never written LDS slot and writes to a scratch slot nobody reads:
      // no branch around the loads and stores.  (Its velocity is +0 after every finite impulse - x * 0 + 0 - so reloading the zeros
      // is what keeping it in registers was.)
      const bool cleanAll = wave_ballot(jointsDirty) == 0ull;
      bool notFinite = false;
      const int nLv = uniform_i(maxLevel) + 1;
      const int sa = aDyn ? bodyA : RC_NB - 1, sb = bDyn ? bodyB : RC_NB - 1;
      const bool two = a_count > 1;
#define RC_CONTACT_PASS(q)                                                                     \
      {                                                                                      \
        const V2 vr = rrelative_velocity(a, b, r1[q], r2[q]);                                \
        const double vrn = vdot_f(vr, n);                                                    \
        const double vrt = vdot_f(vr, vperp(n));                                             \
        const double jnOld = jn[q];                                                          \
        jn[q] = dms_acc_clamp0(-(bounce[q] + vrn), nMass[q], jnOld);                         \
        const double jtMax = arb_u * jn[q];                                                  \
        const double jtOld = jt[q];                                                          \
        jt[q] = fclamp_cp(dm_fma(-vrt, tMass[q], jtOld), -jtMax, jtMax);                     \
        const double dj = jn[q] - jnOld;                                                     \
        const V2 jr = vrotate_f(n, v2(dj, jt[q] - jtOld));                                   \
        const V2 jl = vmul(n, dj);                                                           \
        const V2 jj = biasLane ? jl : jr;                                                    \
        rapply_impulse(a, vneg(jj), r1[q]);                                                  \
        rapply_impulse(b, jj, r2[q]);                                                        \
      }
RC_PROF(unsigned long long nNoop = 0ull, tLv = 0ull, tJt = 0ull;)
      for (int iter = 0; iter < 10; ++iter) {
RC_PROF(const double pj0 = jn[0], pj1 = jn[1], pj2 = jt[0], pj3 = jt[1]; const unsigned long long S0 = __builtin_amdgcn_s_memtime();)
        for (int lv = 0; lv < nLv; ++lv) {
          if (solveMe && myLevel == lv) {
            a.v = v2(fX[bodyA], fY[bodyA]); a.w = fW[bodyA];
            b.v = v2(fX[bodyB], fY[bodyB]); b.w = fW[bodyB];
            RC_CONTACT_PASS(0)
            if (two) RC_CONTACT_PASS(1)
            fX[sa] = a.v.x; fY[sa] = a.v.y; fW[sa] = a.w;
            fX[sb] = b.v.x; fY[sb] = b.v.y; fW[sb] = b.w;
          }
          __syncthreads();
        }
RC_PROF(const unsigned long long S1 = __builtin_amdgcn_s_memtime();)
        if (isRobot) {
          RC_JOINT_VIEW(J)
          RcFeet f;
          f.vx0 = L.vx[la]; f.vy0 = L.vy[la]; f.w0 = L.w[la]; f.vx1 = L.vx[lb]; f.vy1 = L.vy[lb]; f.w1 = L.w[lb];
          if (cleanAll) {
            // CLEAN arithmetic (pivot_warm_start's comment): no foot velocity is -0 - checked after the warm start, and an accumulation
            // v = fma(x, y, v) cannot produce a -0 from a v that is not one, so the arbiters' impulses keep it so - hence the pivot
            // reads and writes (vx, vy) only, the rotary limit w only: the two are independent and their order is immaterial.
            pivot_iterate<true>(J, f, jn[0], jn[1]);
            rotary_iterate(J, f, jt[0]);
            if (iter == 9) notFinite = !(is_finite(jn[0]) && is_finite(jn[1]) && is_finite(f.vx0) && is_finite(f.vy0) && is_finite(f.vx1) &&
                                         is_finite(f.vy1) && is_finite(f.w0) && is_finite(f.w1));
          } else
          joints_iterate_ordered(J, f, jn[0], jn[1], jt[0]);
          L.vx[la] = f.vx0; L.vy[la] = f.vy0; L.w[la] = f.w0; L.vx[lb] = f.vx1; L.vy[lb] = f.vy1; L.w[lb] = f.w1;
        }
        __syncthreads();
RC_PROF(tLv += S1 - S0; tJt += __builtin_amdgcn_s_memtime() - S1;)
RC_PROF(if (wave_ballot((solveMe || isRobot) && !(pj0 == jn[0] && pj1 == jn[1] && pj2 == jt[0] && (isRobot || pj3 == jt[1]))) == 0ull) nNoop += 1ull;)
      }
RC_PROF(if (lane == 0 && c.genv < 4096u) { g_rcprof2[c.genv * 8 + 7] += nNoop; g_rcprof4[c.genv * 8 + 5] += tLv; g_rcprof4[c.genv * 8 + 6] += tJt; g_rcprof4[c.genv * 8 + 7] += (unsigned long long)(10 * nLv) + (10ull << 32); })
      // Non-finite values persist through accumulations: finite feet velocities and pivot impulses at the end mean they were finite
      // all along, i.e. every product the CLEAN arithmetic dropped was a zero.  Otherwise (an overflowing state: never seen) this
      // substep's joints are not the reference's: reported, error bit 5.
      if (wave_ballot(notFinite) != 0ull) err |= 32;
#undef RC_CONTACT_PASS
    }
  }
RC_PROF(const unsigned long long T5 = __builtin_amdgcn_s_memtime();)
  if (isRobot) { L.jx[rl] = jn[0]; L.jy[rl] = jn[1]; L.jrot[rl] = jt[0]; }
#undef RC_JOINT_VIEW
  // --- post-solve callbacks of the active arbiters, canonical order (scalar, lane 0) -------------------------
  if (anyContactWork) {
    double dice0 = 0.0, dice1 = 0.0;
    if (active && c.canFall) rc_post_solve_dice(c, L, a_pair >> 8, a_pair & 0xFF, dice0, dice1);
    for (int k = 0; k < nActive; ++k) {
      const uint64_t who = wave_ballot(active && arank == k);
      const int b = __builtin_ctzll(who);
      const int pk = bcast_i(a_pair, b);
      const double d0 = bcast_d(dice0, b), d1 = bcast_d(dice1, b);
      if (lane == 0) rc_cb_post_solve(c, L, pk >> 8, pk & 0xFF, d0, d1);
      __syncthreads();
    }
    if (active && a_state == ARB_FIRST_) a_state = ARB_NORMAL_;
    if (slotOcc) {
      if (freeMe) L.s_pair[lane] = 0xFFFF;
      L.s_meta[lane] = a_state | (a_count << 8) | (a_age << 16);
      if (touched) { L.s_jn0[lane] = jn[0]; L.s_jt0[lane] = jt[0]; L.s_jn1[lane] = jn[1]; L.s_jt1[lane] = jt[1]; }
    }
    occ &= ~wave_ballot(freeMe);
  }
  __syncthreads();
RC_PROF(if (lane == 0 && c.genv < 4096u) { unsigned long long* d = g_rcprof + c.genv * 12;  /* (profile runs: env_id_offset 0) */ const unsigned long long T6 = __builtin_amdgcn_s_memtime(); d[3] += T1 - T0; d[4] += T2 - T1; d[5] += T3 - T2; d[6] += T4 - T3; d[7] += T5 - T4; d[8] += T6 - T5; d[9] += (unsigned long long)nTouched; d[10] += (unsigned long long)(maxLevel + 1);
  if (anyContactWork) { unsigned long long* q = g_rcprof2 + c.genv * 8; q[0] += C0 - T0; q[1] += C1 - C0; q[2] += C2 - C1; q[3] += C3 - C2; q[4] += C4 - C3; q[5] += T1 - C4; q[6] += 1ull; } })
  RcStepRet ret;
  ret.occ = occ; ret.err = err;
  return ret;
}

DE_OOL RcStepRet rc_physics_ool(RcCtx c_, int lane, int cand, uint64_t pairLo, uint64_t pairHi, uint64_t occ) {
  const RcCtx c = rc_ctx_uniform(c_);
  return rc_physics_inl(c, lane, cand, pairLo, pairHi, occ);
}

// ------------------------------------------------------------------------------------------------
// HBM <-> LDS
// ------------------------------------------------------------------------------------------------
DE_DEV void rc_load_env(const RcState& S, RcLds& L, int e, int lane, uint64_t occ) {
  const size_t E = (size_t)S.E;
  if (lane < RC_NB) {
    const bool used = lane == RC_BALL || lane < 2 * S.R;
    const double* b = S.body + (size_t)e * RC_NB + lane;
    L.px[lane] = used ? b[RB_PX * E * RC_NB] : 0.0; L.py[lane] = used ? b[RB_PY * E * RC_NB] : 0.0;
    L.vx[lane] = used ? b[RB_VX * E * RC_NB] : 0.0; L.vy[lane] = used ? b[RB_VY * E * RC_NB] : 0.0;
    L.ang[lane] = used ? b[RB_ANG * E * RC_NB] : 0.0; L.w[lane] = used ? b[RB_W * E * RC_NB] : 0.0;
    L.vbx[lane] = used ? b[RB_VBX * E * RC_NB] : 0.0; L.vby[lane] = used ? b[RB_VBY * E * RC_NB] : 0.0;
    L.wb[lane] = used ? b[RB_WB * E * RC_NB] : 0.0;
    L.fx[lane] = used ? b[RB_FX * E * RC_NB] : 0.0; L.fy[lane] = used ? b[RB_FY * E * RC_NB] : 0.0;
    L.tq[lane] = used ? b[RB_TQ * E * RC_NB] : 0.0;
    // shape cache (position / rotation at the last integration) is stored in the 4 spare body fields
    L.cpx[lane] = used ? b[(RB_COUNT + 0) * E * RC_NB] : 0.0; L.cpy[lane] = used ? b[(RB_COUNT + 1) * E * RC_NB] : 0.0;
    L.crc[lane] = used ? b[(RB_COUNT + 2) * E * RC_NB] : 1.0; L.crs[lane] = used ? b[(RB_COUNT + 3) * E * RC_NB] : 0.0;
    if (lane < RC_BALL) L.rotAng[lane] = __builtin_nan("");
    // the goalposts (static bodies 21..24) live in the same arrays - their positions, zero velocities, never written - so that a
    // contact's bodies are read without a branch on "is it a post" (rbody_load, the narrowphase, the broadphase)
    if (lane >= RC_POST && lane < RC_POST + 4) {
      const V2 pp = post_pos(lane);
      L.px[lane] = pp.x; L.py[lane] = pp.y; L.cpx[lane] = pp.x; L.cpy[lane] = pp.y;
    }
  }
  if (lane < 16) {
    const bool used = lane < S.R;
    const double* r = S.rob + (size_t)e * 16 + lane;
    L.head[lane] = used ? r[RR_HEAD * E * 16] : 0.0; L.headmov[lane] = used ? r[RR_HEADMOV * E * 16] : 0.0;
    L.prevx[lane] = used ? r[RR_PREVX * E * 16] : 0.0; L.prevy[lane] = used ? r[RR_PREVY * E * 16] : 0.0;
    L.initx[lane] = used ? r[RR_INITX * E * 16] : 0.0; L.inity[lane] = used ? r[RR_INITY * E * 16] : 0.0;
    L.penalT[lane] = used ? r[RR_PENALT * E * 16] : 0.0; L.fallT[lane] = used ? r[RR_FALLT * E * 16] : 0.0;
    L.moveT[lane] = used ? r[RR_MOVET * E * 16] : 0.0;
    L.jx[lane] = used ? r[RR_JX * E * 16] : 0.0; L.jy[lane] = used ? r[RR_JY * E * 16] : 0.0; L.jrot[lane] = used ? r[RR_JROT * E * 16] : 0.0;
    const int* ri = S.robi + (size_t)e * 16 + lane;
    L.rflags[lane] = used ? ri[RI_FLAGS * E * 16] : 0; L.touchc[lane] = used ? ri[RI_TOUCHC * E * 16] : 0;
    L.fallc[lane] = used ? ri[RI_FALLC * E * 16] : 0;
    L.rrew[lane] = 0.0; L.rposrew[lane] = 0.0;
  }
  for (int k = lane; k < RE_COUNT; k += DE_WAVE) L.envi[k] = S.envi[(size_t)e * RE_COUNT + k];
  if (lane < RD_COUNT) L.envd[lane] = S.envd[(size_t)e * RD_COUNT + lane];
  if (lane < 2) L.teamRew[lane] = 0.0;
  if (lane < RC_NS) {
    const bool on = (occ >> lane) & 1ull;
    size_t o = (size_t)e * RC_NS + lane;
    L.s_pair[lane] = on ? S.s_pair[o] : 0xFFFF;
    L.s_meta[lane] = on ? S.s_meta[o] : 0;
    L.s_hash0[lane] = on ? (int)S.s_hash[o] : 0; L.s_hash1[lane] = on ? (int)S.s_hash[E * RC_NS + o] : 0;
    L.s_jn0[lane] = on ? S.s_imp[o] : 0.0; L.s_jt0[lane] = on ? S.s_imp[E * RC_NS + o] : 0.0;
    L.s_jn1[lane] = on ? S.s_imp[2 * E * RC_NS + o] : 0.0; L.s_jt1[lane] = on ? S.s_imp[3 * E * RC_NS + o] : 0.0;
  }
}

DE_DEV void rc_store_env(const RcState& S, const RcLds& L, int e, int lane, uint64_t occ) {
  const size_t E = (size_t)S.E;
  if (lane == RC_BALL || lane < 2 * S.R) {
    double* b = S.body + (size_t)e * RC_NB + lane;
    b[RB_PX * E * RC_NB] = L.px[lane]; b[RB_PY * E * RC_NB] = L.py[lane]; b[RB_VX * E * RC_NB] = L.vx[lane];
    b[RB_VY * E * RC_NB] = L.vy[lane]; b[RB_ANG * E * RC_NB] = L.ang[lane]; b[RB_W * E * RC_NB] = L.w[lane];
    b[RB_VBX * E * RC_NB] = L.vbx[lane]; b[RB_VBY * E * RC_NB] = L.vby[lane]; b[RB_WB * E * RC_NB] = L.wb[lane];
    b[RB_FX * E * RC_NB] = L.fx[lane]; b[RB_FY * E * RC_NB] = L.fy[lane]; b[RB_TQ * E * RC_NB] = L.tq[lane];
    b[(RB_COUNT + 0) * E * RC_NB] = L.cpx[lane]; b[(RB_COUNT + 1) * E * RC_NB] = L.cpy[lane];
    b[(RB_COUNT + 2) * E * RC_NB] = L.crc[lane]; b[(RB_COUNT + 3) * E * RC_NB] = L.crs[lane];
  }
  if (lane < S.R) {
    double* r = S.rob + (size_t)e * 16 + lane;
    r[RR_HEAD * E * 16] = L.head[lane]; r[RR_HEADMOV * E * 16] = L.headmov[lane];
    r[RR_PREVX * E * 16] = L.prevx[lane]; r[RR_PREVY * E * 16] = L.prevy[lane];
    r[RR_INITX * E * 16] = L.initx[lane]; r[RR_INITY * E * 16] = L.inity[lane];
    r[RR_PENALT * E * 16] = L.penalT[lane]; r[RR_FALLT * E * 16] = L.fallT[lane]; r[RR_MOVET * E * 16] = L.moveT[lane];
    r[RR_JX * E * 16] = L.jx[lane]; r[RR_JY * E * 16] = L.jy[lane]; r[RR_JROT * E * 16] = L.jrot[lane];
    int* ri = S.robi + (size_t)e * 16 + lane;
    ri[RI_FLAGS * E * 16] = L.rflags[lane]; ri[RI_TOUCHC * E * 16] = L.touchc[lane]; ri[RI_FALLC * E * 16] = L.fallc[lane];
  }
  for (int k = lane; k < RE_COUNT; k += DE_WAVE) S.envi[(size_t)e * RE_COUNT + k] = L.envi[k];
  if (lane < RD_COUNT) S.envd[(size_t)e * RD_COUNT + lane] = L.envd[lane];
  if (lane < RC_NS && ((occ >> lane) & 1ull)) {
    size_t o = (size_t)e * RC_NS + lane;
    S.s_pair[o] = L.s_pair[lane]; S.s_meta[o] = L.s_meta[lane];
    S.s_hash[o] = (uint32_t)L.s_hash0[lane]; S.s_hash[E * RC_NS + o] = (uint32_t)L.s_hash1[lane];
    S.s_imp[o] = L.s_jn0[lane]; S.s_imp[E * RC_NS + o] = L.s_jt0[lane];
    S.s_imp[2 * E * RC_NS + o] = L.s_jn1[lane]; S.s_imp[3 * E * RC_NS + o] = L.s_jt1[lane];
  }
}

// ------------------------------------------------------------------------------------------------
// Full observation of one snapshot (RoboCupEnvironment.getFullState/get_full_obs :1149-1189, :440-443)
// row per agent: [ball 4 | self 8 | other robots (R-1) x 6]
// ------------------------------------------------------------------------------------------------
#define RC_STD_NORM (2.0 / RC_W)
DE_DEV double norm_after_scale(double pt, double nf, double mean) { return (pt - mean) * nf; }  // x team applied as a sign

// out of line with inline trigonometry (a leaf, its own register allocation: no spill reloads between its stores)
DE_OOL void rc_write_obs_ool(int lane, int R, int obs_dim, float* __restrict__ out) {
  RcLds& L = g_R;
  constexpr int W = 64;
  RcObsStage& O = L.u.ob;
  __syncthreads();
  if (lane < R) {
    const V2 p = robot_pos(L, lane);
    const double ang = robot_angle(L, lane);
    const int f = L.rflags[lane];
    O.rx[lane] = (float)norm_after_scale(p.x, RC_STD_NORM, RC_W / 2.0);
    O.ry[lane] = (float)norm_after_scale(p.y, RC_STD_NORM, RC_H / 2.0);
    const DevSC a = dev_sincos_inl(ang);
    O.rcs[lane] = (float)a.c; O.rsn[lane] = (float)a.s;
    const DevSC ah = dev_sincos_inl(ang + L.head[lane]);
    O.ahc[lane] = (float)ah.c; O.ahs[lane] = (float)ah.s;
    const DevSC h = dev_sincos_inl(L.head[lane]);
    O.hc[lane] = (float)h.c; O.hs[lane] = (float)h.s;
    O.team[lane] = (f & RF_TEAMPOS) ? 1.0f : -1.0f;
    O.down[lane] = (f & (RF_FALLEN | RF_PENAL)) ? 1.0f : 0.0f;
  }
  if (lane == W - 1) {
    O.bx = (float)norm_after_scale(L.px[RC_BALL], RC_STD_NORM, RC_W / 2.0);
    O.by = (float)norm_after_scale(L.py[RC_BALL], RC_STD_NORM, RC_H / 2.0);
  }
  __syncthreads();
  const float owned = (float)L.envi[RE_OWNED];
  const int c0 = L.envi[RE_CLOSE0], c1 = L.envi[RE_CLOSE1];
  for (int idx = lane; idx < R * obs_dim; idx += W) {
    const int a = idx / obs_dim, ff = idx - a * obs_dim;
    const float team = O.team[a];
    float x;
    if (ff == 0) x = O.bx * team;
    else if (ff == 1) x = O.by * team;
    // ballOwned * team is an INT product in the reference (RoboCupEnvironment.py:1149-1189): a free ball reads +0.0f for either team,
    // where the float product 0.0f * -1.0f is -0.0f; adding +0.0f turns that -0.0f into +0.0f and changes no other value
    else if (ff == 2) x = owned * team + 0.0f;
    else if (ff == 3) x = (a == c0 || a == c1) ? 1.0f : 0.0f;
    else if (ff == 4) x = O.rx[a] * team;
    else if (ff == 5) x = O.ry[a] * team;
    else if (ff == 6) x = O.ahc[a];
    else if (ff == 7) x = O.ahs[a];
    else if (ff == 8) x = O.hc[a];
    else if (ff == 9) x = O.hs[a];
    else if (ff == 10) x = team;
    else if (ff == 11) x = O.down[a];
    else {
      int k = (ff - 12) / 6, q = (ff - 12) - k * 6;
      k += (k >= a);
      x = q == 0 ? O.rx[k] * team : q == 1 ? O.ry[k] * team : q == 2 ? O.rcs[k] : q == 3 ? O.rsn[k] : q == 4 ? O.team[k] * team : O.down[k];
    }
    out[idx] = x;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// THE RoboCup step kernel
// ------------------------------------------------------------------------------------------------
#include "robocup_partial.hip"

#ifndef RC_PV_DEADLINE_PCT
#define RC_PV_DEADLINE_PCT 98 /* fused vision passes start until this many percent of the forecast of the launch's slowest environment (round 6 sweep: 85 +5 %, 90 +2 %, 95 0, 98 -0.5 %, 100 -0.3 %, 105 +1 %, 115 +7.5 %) */
#endif
#define RC_SCHED_MIN 1800000    /* cycles from which an environment may be the step's slowest (a light one needs 1.4 M) */
#ifndef RC_DEFER_MIN_GENERAL
#define RC_DEFER_MIN_GENERAL 15 /* rc_physics substeps (of 50) from which an environment defers its Partial observation */
#endif
struct RcCommonRet {
  uint64_t pairLo, pairHi;  // this lane's pair codes, for rc_physics (S.pairTab)
  int cand, bits;           // bits: 1 quiet
};
DE_OOL RcCommonRet rc_common_substep(RcCtx c_, int serial_, int lane, const uint64_t* __restrict__ pairTab, uint64_t occ_) {
  const RcCtx c = rc_ctx_uniform(c_);
  RcLds& L = g_R;
  const bool serial = uniform_i(serial_) != 0;  // the sequential game logic has run already: no tick here
  const int R = c.R;
  const uint64_t occ = uniform_u64(occ_);
  const bool isBody = lane == RC_BALL || lane < 2 * R;
  // my pairs: loaded here, first used by the broadphase - the latency is hidden behind the game logic and the position update.
  // They are NOT kept in registers across substeps: whatever the kernel holds across the call of rc_physics (128 VGPRs) is
  // spilled around it, 4 bytes x 64 lanes a register and call - that was most of this kernel's HBM writes.
  const uint64_t pairLo = pairTab[2 * lane], pairHiFeet = pairTab[2 * lane + 1];
  const uint64_t pairHi = pairHiFeet & 0xFFFFull;
  const int feetPairs = (int)(pairHiFeet >> 32);  // bit t: my pair of round t is the two feet of one robot
RC_PROF(const unsigned long long P0 = __builtin_amdgcn_s_memtime();)
    // ---- game logic: tick per robot (one robot per lane, unless the sequential form has run), then the ball (:465-475) ----
    if (!rc_game_logic_batched(c, L, lane, !serial)) {
      RcCommonRet ret;  // a robot's tick has a cross-robot event: nothing has been changed, the kernel runs the sequential form
      ret.pairLo = 0ull; ret.pairHi = 0ull; ret.cand = 0; ret.bits = 4;
      return ret;
    }
    __syncthreads();
RC_PROF(const unsigned long long P1 = __builtin_amdgcn_s_memtime();)
    // ---- cpBodyUpdatePosition + shape cache + AABB ------------------------------------------------------
    if (isBody) {
      const double npx = L.px[lane] + (L.vx[lane] + L.vbx[lane]) * DE_DT;
      const double npy = L.py[lane] + (L.vy[lane] + L.vby[lane]) * DE_DT;
      const double nang = L.ang[lane] + (L.w[lane] + L.wb[lane]) * DE_DT;
      L.px[lane] = npx; L.py[lane] = npy; L.ang[lane] = nang;
      L.vbx[lane] = 0.0; L.vby[lane] = 0.0; L.wb[lane] = 0.0;
      float fcx, fcy, fhx, fhy;
      double al, ab, ar, at;
      if (lane != RC_BALL) {
        if (!(nang == L.rotAng[lane])) {  // the shape cache's rotation is that of another angle (or, NaN, of an earlier launch)
          const DevSC sc = RC_COMMON_SINCOS(nang);
          L.crc[lane] = sc.c; L.crs[lane] = sc.s; L.rotAng[lane] = nang;
        }
        L.cpx[lane] = npx; L.cpy[lane] = npy;
        SegW s;
        seg_world(L, lane, s);
        double l, r, b, t;
        if (s.ta.x < s.tb.x) { l = s.ta.x; r = s.tb.x; } else { l = s.tb.x; r = s.ta.x; }
        if (s.ta.y < s.tb.y) { b = s.ta.y; t = s.tb.y; } else { b = s.tb.y; t = s.ta.y; }
        al = l - FOOT_RADIUS; ab = b - FOOT_RADIUS; ar = r + FOOT_RADIUS; at = t + FOOT_RADIUS;
      } else {
        L.cpx[lane] = npx; L.cpy[lane] = npy;
        al = npx - BALL_R; ab = npy - BALL_R; ar = npx + BALL_R; at = npy + BALL_R;
      }
      L.aabb[lane][0] = al; L.aabb[lane][1] = ab; L.aabb[lane][2] = ar; L.aabb[lane][3] = at;  // (kept in registers for the prefilter: no read-back)
      fcx = (float)(0.5 * (al + ar)); fcy = (float)(0.5 * (ab + at));
      fhx = (float)(0.5 * (ar - al)) + 1.0f; fhy = (float)(0.5 * (at - ab)) + 1.0f;
      L.u.pf.box[lane] = make_float4(fcx, fcy, fhx, fhy);
    } else if (lane >= RC_POST && lane < RC_POST + 4) {  // the goalposts' entries (the table shares its LDS with the mailbox: rewritten every substep)
      const V2 pc = post_pos(lane);
      L.u.pf.box[lane] = make_float4((float)pc.x, (float)pc.y, 11.0f, 11.0f);
    }
    __syncthreads();
RC_PROF(const unsigned long long P2 = __builtin_amdgcn_s_memtime();)
    // ---- broadphase ---------------------------------------------------------------------------------------
    // The two feet of one robot overlap in every substep: they are candidates without a test (a candidate whose boxes
    // do not overlap is harmless - shapes that touch have overlapping boxes, so the narrowphase finds nothing), which
    // keeps the double-precision box test below for the rare real prefilter hits.
    int cand = feetPairs, pre = 0;
#pragma unroll
    for (int t = 0; t < RC_NPAIR_ROUNDS; ++t) {  // the fp32 prefilter of all my pairs first: their LDS reads are in flight together
      const int pr = RC_MY_PAIR(t);
      if (pr != 0xFFFF && !((feetPairs >> t) & 1)) {
        const int i = pr >> 8, j = pr & 0xFF;
        const float4 bi = L.u.pf.box[i], bj = L.u.pf.box[j];
        const float dx = bi.x - bj.x, dy = bi.y - bj.y;
        if (__builtin_fabsf(dx) <= bi.z + bj.z && __builtin_fabsf(dy) <= bi.w + bj.w) pre |= 1 << t;
      }
    }
#pragma unroll 1
    for (int mm = pre; mm; mm &= mm - 1) {  // the exact test (cpBBIntersects) of the pairs that passed (rare)
      const int t = __builtin_ctz(mm);
      const int pr = RC_MY_PAIR(t);
      const int i = pr >> 8, j = pr & 0xFF;
      const double al = L.aabb[i][0], ab = L.aabb[i][1], ar = L.aabb[i][2], at = L.aabb[i][3];
      double bl, bb, br, bt;
      if (j <= RC_BALL) { bl = L.aabb[j][0]; bb = L.aabb[j][1]; br = L.aabb[j][2]; bt = L.aabb[j][3]; }
      else { const V2 pc = post_pos(j); bl = pc.x - POST_R; bb = pc.y - POST_R; br = pc.x + POST_R; bt = pc.y + POST_R; }
      if (al <= br && bl <= ar && ab <= bt && bb <= at) cand |= (1 << t);
    }
    __syncthreads();
    // ---- contacts, joints, velocity update, solver, post-solve callbacks -----------------------------------------
    // The common substep never enters rc_physics: no cached arbiter, the only candidates are the robots' own feet pairs, and
    // the narrowphase's separating-axis early out rejects every one of them.  What rc_physics does then is exactly this:
    // velocity update, then every robot's joints (prestep, warm start, 10 iterations) in registers.
RC_PROF(const unsigned long long P3 = __builtin_amdgcn_s_memtime(); unsigned long long P4 = P3, P5 = P3, P6 = P3;)
    bool quiet = occ == 0ull && wave_ballot((cand & ~feetPairs) != 0) == 0ull;
    if (quiet) {
      const bool far = lane < R ? feet_far_apart(L, lane) : true;
      quiet = wave_ballot(!far) == 0ull;
    }
RC_PROF(P4 = P5 = P6 = __builtin_amdgcn_s_memtime();)
    if (quiet) {
      if (isBody) rc_velocity_update(L, lane);
      __syncthreads();
RC_PROF(P5 = __builtin_amdgcn_s_memtime();)
      rc_joints_only_inl(lane, R);
      __syncthreads();
RC_PROF(P6 = __builtin_amdgcn_s_memtime();)
    }
RC_PROF(if (lane == 0 && c.genv < 4096u) { unsigned long long* d = g_rcprof3 + c.genv * 8; d[0] += P1 - P0; d[1] += P2 - P1; d[2] += P3 - P2; d[3] += P4 - P3; d[4] += P5 - P4; d[5] += P6 - P5; d[6] += quiet ? 1ull : 0ull; d[7] += 1ull; })
  RcCommonRet ret;
  ret.pairLo = pairLo; ret.pairHi = pairHi; ret.cand = cand; ret.bits = quiet ? 1 : 0;
  return ret;
}
// mask (device uint8 [E], dynenv_step_masked; nullptr: every environment): the wave of an environment whose byte is 0 ends at once - it
// reads no action and writes no byte of the environment's state, of its output rows or of deferList's entries.  The one thing a block
// does for the LAUNCH, environment 0's rotation of the forecast words, does not depend on the mask.
template <bool PARTIAL>
DE_DEV void rc_step_body(const RcState& S, const uint8_t* __restrict__ mask, const int e, const int* __restrict__ actions,
                         const double* __restrict__ headActions, float* __restrict__ obs, double* __restrict__ rewards, uint8_t* __restrict__ dones) {
  static_assert(RC_NS <= 16, "sLevel packs level and rank into four bits each");
  int lane = (int)threadIdx.x;
  const int R = S.R;
  if (e < 0 || e >= S.E) return;  // (a block beyond the batch has no environment: its wave ends here)
  if (mask && uniform_i(mask[e]) == 0) {
    if (PARTIAL && e == 0 && lane == 0) { int* sc = S.deferList + S.E + 1; sc[0] = sc[1]; sc[1] = 0; }  // (as below)
    return;
  }
  RcLds& L = g_R;
  uint64_t occ = (uint64_t)(uint32_t)uniform_i(S.envi[(size_t)e * RE_COUNT + RE_OCC]);
  // Environments with live contacts are the long ones and the launch ends with the slowest: their waves get issue priority
  // over the lighter waves they share a SIMD with, from the first instruction on.
  if (occ != 0ull) __builtin_amdgcn_s_setprio(3);
  else if (PARTIAL) __builtin_amdgcn_s_setprio(1);
  unsigned long long schedT0 = 0ull;
  if constexpr (PARTIAL) schedT0 = __builtin_amdgcn_s_memtime();
  // the forecast for this step = the slowest environment of the previous one (0: none was slow); block 0 is among the first to start,
  // everybody else reads the word when its physics is done - a million cycles later
  if (PARTIAL && e == 0 && lane == 0) { int* sc = S.deferList + S.E + 1; sc[0] = sc[1]; sc[1] = 0; }
  rc_load_env(S, L, e, lane, occ);
  L.lastCand[lane & 63] = 0xFF;  // rc_physics' call-to-call caches start empty
  if (lane == 0) { L.candN = -1; L.sActive = ~0ull; L.sMaxLevel = -1; }
  RcCtx c;
  c.seed = S.seed; c.genv = (uint32_t)(S.env_id_offset + e); c.n = S.n; c.R = R;
  c.canFall = (S.flags & DYNENV_FLAG_CAN_FALL) != 0; c.allowHead = (S.flags & DYNENV_FLAG_ALLOW_HEAD_TURN) != 0;
  c.detTurn = (S.flags & DYNENV_FLAG_DETERMINISTIC_TURN) != 0;
  __syncthreads();
  c.episode = (uint32_t)uniform_i(L.envi[RE_EPISODE]);  // (an LDS read is a vector value until told otherwise: it would be spilled around every call)
  if (lane == 0) refresh_pivot_first(L);
  __syncthreads();
  const bool partial = PARTIAL;
  const bool isBody = lane == RC_BALL || lane < 2 * R;
  const int* myActions = actions + (size_t)e * R * 4;
  const double* myHead = headActions ? headActions + (size_t)e * R : nullptr;
  int snap = 0, nGeneral = 0;  // substeps that went through rc_physics

RC_PROF(if (lane < 8 && e < 4096) { g_rcprof2[e * 8 + lane] = 0ull; g_rcprof3[e * 8 + lane] = 0ull; g_rcprof4[e * 8 + lane] = 0ull; })
RC_PROF(if (lane < 12 && e < 4096) g_rcprof[e * 12 + lane] = 0ull; const unsigned long long K0 = __builtin_amdgcn_s_memtime(); unsigned long long tG = 0, tP = 0, tB = 0;)
  for (int it = 0; it < 50; ++it) {
    lane = fresh_lane();  // per substep: nothing derived from the lane id is hoisted out of the loop, and the id itself is not kept across the calls
RC_PROF(const unsigned long long A0 = __builtin_amdgcn_s_memtime();)
    // the game logic's sequential form (first substep: processAction; later: a cross-robot event) is the only call of the common
    // part: it is made from here, the outermost frame, so that rc_common_substep itself contains no call at all
    // (the first substep is always sequential: processAction; later ones when the common part's lane-parallel tick reports an
    //  event - it then returns without having changed anything and is called again after the sequential form)
    bool serial = it == 0;
    if (serial) {
      if (lane == 0) rc_game_serial(c, it, myActions, myHead);
RC_PROF(tG += 1;)  // (profile build: "game logic" = substeps with the sequential form, "position" = cycles of the whole common part)
    }
    RcCommonRet cr = rc_common_substep(c, serial ? 1 : 0, lane, S.pairTab, occ);
    if (uniform_i(cr.bits & 4) != 0) {
      lane = fresh_lane();
      if (lane == 0) rc_game_serial(c, it, myActions, myHead);
RC_PROF(tG += 1;)
      lane = fresh_lane();
      cr = rc_common_substep(c, 1, lane, S.pairTab, occ);
    }
    const int cand = cr.cand;
    const bool quiet = uniform_i(cr.bits & 1) != 0;
RC_PROF(tP += __builtin_amdgcn_s_memtime() - A0;)
    if (quiet) {
    } else {
      __builtin_amdgcn_s_setprio(3);  // an environment with contact work is on the launch's critical path: issue it first
      ++nGeneral;
      const RcStepRet sr = rc_physics_ool(c, fresh_lane(), cand, cr.pairLo, cr.pairHi, occ);
      occ = uniform_u64(sr.occ);
      lane = fresh_lane();
      {  // a full slot table / candidate list (bit 0), a capsule pair on the fallback normal (bit 4): reported, never silent
        const int eb = (wave_ballot((sr.err & 1) != 0) != 0ull ? 1 : 0) | (wave_ballot((sr.err & 16) != 0) != 0ull ? 16 : 0) | (wave_ballot((sr.err & 32) != 0) != 0ull ? 32 : 0);
        if (eb != 0 && lane == 0) L.envi[RE_ERR] |= eb;
      }
    }
    lane = fresh_lane();
    if (lane == 0) L.envi[RE_ELAPSED] += 1;
    __syncthreads();
    if (it % 10 == 9) {
      if (partial) {  // export what getAgentVision reads of this snapshot; rc_partial_obs_kernel turns it into rows
        RvSnap& sn = S.snap[(size_t)e * 5 + snap];
        if (lane < 21) { sn.px[lane] = L.px[lane]; sn.py[lane] = L.py[lane]; }
        if (lane < 20) sn.ang[lane] = L.ang[lane];
        if (lane < 10) { sn.head[lane] = L.head[lane]; sn.rflags[lane] = L.rflags[lane]; }
        if (lane == 0) { sn.owned = L.envi[RE_OWNED]; sn.close0 = L.envi[RE_CLOSE0]; sn.close1 = L.envi[RE_CLOSE1]; sn.tkey = L.envi[RE_ELAPSED]; }
      } else if (obs) rc_write_obs_ool(lane, R, S.obs_dim, obs + ((size_t)e * 5 + snap) * R * S.obs_dim);
      ++snap;
    }
  }
RC_PROF(if (lane == 0 && e < 4096) { unsigned long long* d = g_rcprof + e * 12; d[0] = tG; d[1] = tP; d[2] = tB; d[11] = __builtin_amdgcn_s_memtime() - K0; })
  // ---- end of env step :497-524 ------------------------------------------------------------------------------
  if (lane < R) {
    const double tr = lane < S.n ? L.teamRew[0] : L.teamRew[1];
    double rew = L.rrew[lane] + tr;
    double prew = L.rposrew[lane] + dm_max(0.0, tr);
    if (partial) {
      // the observation reward (processSeens) is added by rc_partial_obs_kernel, which then updates the episode sums in
      // the reference's order: episodeRewards += (robot + team + obs)
      S.prew0[(size_t)e * 16 + lane] = prew;
    } else {
      rew += 0.0;   // obsRewards are zero for Full observations (processSeens returns early)
      prew += 0.0;
      double* er = S.epr + (size_t)e * 16 + lane;
      double* ep = S.epr + (size_t)S.E * 16 + (size_t)e * 16 + lane;
      *er = *er + rew;
      *ep = *ep + prew;
    }
    rewards[(size_t)e * R + lane] = rew;
  }
  __syncthreads();
  // Partial: an environment that spent much of the step in rc_physics is among the last to finish and leaves its vision
  // to the deferred launch (five waves per environment) instead of appending 50 agent passes to the critical path
  // Partial: with a forecast of when the launch will end (the slowest environment of the previous step, RcState.deferList) every
  // environment runs its vision passes - 5 R of them, in (snapshot, agent) order - until then and leaves the rest to the deferred
  // launch: the SIMDs whose four waves are all light have the most vision to do and finish about when the slowest environment
  // does; an environment that spent the step in rc_physics gets to fewer of its passes.  Without a forecast (no environment has
  // been slow yet) the old rule: all or, from RC_DEFER_MIN_GENERAL substeps of contact work, nothing.
  int budget = 0, ownPasses = 5 * R;
  if (PARTIAL && obs) {
    int* sc = S.deferList + S.E + 1;
    const int slowest = uniform_i(__atomic_load_n(sc, __ATOMIC_RELAXED));
    const int cycles = (int)(__builtin_amdgcn_s_memtime() - schedT0);
    if (slowest > 0) { budget = (slowest / 100) * RC_PV_DEADLINE_PCT - cycles; if (budget <= 0) ownPasses = 0; }
    else if (nGeneral >= RC_DEFER_MIN_GENERAL) ownPasses = 0;
    // (only an environment slower than everything so far touches the shared word: thousands of atomics on one address serialise)
    if (lane == 0 && cycles > RC_SCHED_MIN && cycles > __atomic_load_n(sc + 1, __ATOMIC_RELAXED)) atomicMax(sc + 1, cycles);
  }
  if (lane == 0) {
    dones[e] = (uint8_t)(L.envi[RE_ELAPSED] >= RC_MAX_TIME);
    L.envi[RE_OCC] = (int)(uint32_t)occ;
  }
  __syncthreads();
  rc_store_env(S, L, e, lane, occ);
  if constexpr (PARTIAL) {
    if (obs) {
      if (ownPasses > 0) {  // getAgentVision at the five snapshots (+ processSeens if it gets through all of them)
        __builtin_amdgcn_s_setprio(0);  // vision is nobody's critical path: behind every neighbour's physics (priority >= 1)
        ownPasses = rc_partial_obs_fused(S.seed, S.env_id_offset, S.envi, S.n, S.R, S.noise_type, S.noise_magn, S.snap, S.flags, S.prew0, S.epr, S.E, S.epo, e, obs,
                                         rewards, S.seenPart, budget);
      }
      if (ownPasses < 5 * R && (int)threadIdx.x == 0) S.deferList[1 + atomicAdd(&S.deferList[0], 1)] = e | (ownPasses << 20);
    }
  }
}
// Full observations: one environment per wave at four waves per SIMD (128 VGPRs, the general path out of line)
extern "C" __global__ void __launch_bounds__(64, RC_WAVES_PER_SIMD)
rc_step_kernel(RcState S, const uint8_t* __restrict__ mask, const int* __restrict__ actions, const double* __restrict__ headActions,
               float* __restrict__ obs, double* __restrict__ rewards, uint8_t* __restrict__ dones) {
  rc_step_body<false>(S, mask, (int)blockIdx.x, actions, headActions, obs, rewards, dones);
}
extern "C" __global__ void __launch_bounds__(64, RC_WAVES_PER_SIMD)
rc_step_partial_kernel(RcState S, const uint8_t* __restrict__ mask, const int* __restrict__ actions, const double* __restrict__ headActions,
                       float* __restrict__ obs, double* __restrict__ rewards, uint8_t* __restrict__ dones) {
  rc_step_body<true>(S, mask, (int)blockIdx.x, actions, headActions, obs, rewards, dones);
}

// getFullState(agent=None) (RoboCupEnvironment.py:1149-1161), what step() stores as info['Full State'] (:511): per environment
// robots [R][6] = (normalize(x, standardNorm, 0), normalize(y, ...), cos a, sin a, team, fallen | penalized) in FIELD coordinates
// (no team flip, a different normalisation from the per-agent rows: ((pt * nf) - 0) * 2, cutils.py:318-323), then the ball
// (normalize(bx), normalize(by), ballOwned): out float32 [E][R * 6 + 3].  One thread per (environment, robot) + one for the ball.
extern "C" __global__ void __launch_bounds__(64) rc_global_state_kernel(RcState S, float* __restrict__ out) {
  const int e = blockIdx.x * 4 + (threadIdx.x >> 4), r = threadIdx.x & 15, R = S.R;
  if (e >= S.E || r > R) return;
  const size_t E = (size_t)S.E;
  float* o = out + (size_t)e * (R * 6 + 3);
  const double* px = S.body + ((size_t)RB_PX * E + e) * RC_NB;
  const double* py = S.body + ((size_t)RB_PY * E + e) * RC_NB;
  if (r == R) {
    o[R * 6 + 0] = (float)(((px[RC_BALL] * RC_STD_NORM) - 0.0) * 2.0);
    o[R * 6 + 1] = (float)(((py[RC_BALL] * RC_STD_NORM) - 0.0) * 2.0);
    o[R * 6 + 2] = (float)S.envi[(size_t)e * RE_COUNT + RE_OWNED];
    return;
  }
  const double* ang = S.body + ((size_t)RB_ANG * E + e) * RC_NB;
  const double x = (px[2 * r] + px[2 * r + 1]) / 2.0, y = (py[2 * r] + py[2 * r + 1]) / 2.0;  // Robot.getPos
  const DevSC a = dev_sincos((ang[2 * r] + ang[2 * r + 1]) / 2.0);                             // Robot.getAngle
  const int f = S.robi[((size_t)RI_FLAGS * E + e) * 16 + r];
  o[r * 6 + 0] = (float)(((x * RC_STD_NORM) - 0.0) * 2.0);
  o[r * 6 + 1] = (float)(((y * RC_STD_NORM) - 0.0) * 2.0);
  o[r * 6 + 2] = (float)a.c;
  o[r * 6 + 3] = (float)a.s;
  o[r * 6 + 4] = (f & RF_TEAMPOS) ? 1.0f : -1.0f;
  o[r * 6 + 5] = (f & (RF_FALLEN | RF_PENAL)) ? 1.0f : 0.0f;
}

extern "C" __global__ void rc_stats_kernel(RcState S, double* ep_r, double* ep_pos_r, double* ep_obs_r, int* goals) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S.E) return;
  for (int a = 0; a < S.R; ++a) {
    if (ep_r) ep_r[(size_t)e * S.R + a] = S.epr[(size_t)e * 16 + a];
    if (ep_pos_r) ep_pos_r[(size_t)e * S.R + a] = S.epr[(size_t)S.E * 16 + (size_t)e * 16 + a];
    if (ep_obs_r) ep_obs_r[(size_t)e * S.R + a] = S.epo[(size_t)e * 16 + a];
  }
  if (goals) { goals[2 * e] = S.envi[(size_t)e * RE_COUNT + RE_GOAL0]; goals[2 * e + 1] = S.envi[(size_t)e * RE_COUNT + RE_GOAL1]; }
}

#define RC_PARTIAL_FUNCTIONS
#include "robocup_partial.hip"

// ------------------------------------------------------------------------------------------------
// batched state transfer (dynenv_get_states / dynenv_set_states / dynenv_error_flags_env), behind everything the step launches run so
// that the step code keeps its addresses (rc_layout_pad above).  One wave per listed environment (grid n), lane = body slot (feet 2r,
// 2r + 1 of robot r, the ball at RC_BALL) or robot.  The blob (2552 bytes: 8-byte aligned, not 16) travels between HBM and an LDS tile
// as contiguous 8-byte words across the wave; the lanes read / write their robot's struct in LDS, and every access to the field-major
// arrays is one whole row of the environment per instruction.  dynenv_get_state / dynenv_set_state are these kernels for one blob
// (idx == nullptr, first = the environment) through a staging area in device memory.
// ------------------------------------------------------------------------------------------------
#define RC_BLOB_WORDS ((int)(sizeof(dynenv_robocup_state_t) / 8))
static_assert(sizeof(dynenv_robocup_state_t) % 8 == 0, "the blob moves as 8-byte words");
static_assert(RE_COUNT <= 64 && RD_COUNT <= 64, "an environment's int / double row is one access of the wave");
union RcBlobTile {
  dynenv_robocup_state_t st;
  unsigned long long q[RC_BLOB_WORDS];
};
// the twelve doubles a robot's struct starts with: left foot px py vx vy angle w, right foot the same
DE_DEV double* rc_blob_foot(dynenv_robot_state_t& r, int side) { return reinterpret_cast<double*>(&r) + 6 * side; }
static_assert(offsetof(dynenv_robot_state_t, rpx) == 6 * sizeof(double) && offsetof(dynenv_robot_state_t, head_angle) == 12 * sizeof(double), "foot blocks");

// idx == nullptr: environments first..first + n - 1.  An index outside [0, E) leaves its blob untouched.
extern "C" __global__ void __launch_bounds__(64)
rc_get_states_kernel(RcState S, const int* __restrict__ idx, int first, unsigned long long* __restrict__ blobs) {
  __shared__ RcBlobTile T;
  __shared__ int envi[64];
  __shared__ double envd[RD_COUNT];
  const int lane = threadIdx.x, k = blockIdx.x, R = S.R;
  const int e = idx ? uniform_i(idx[k]) : first + k;
  if (e < 0 || e >= S.E) return;
  const size_t E = (size_t)S.E, row = (size_t)e * RC_NB, r16 = (size_t)e * 16;
  for (int q = lane; q < RC_BLOB_WORDS; q += 64) T.q[q] = 0ull;  // the pads and the slots of robots this handle does not have read 0
  envi[lane] = lane < RE_COUNT ? S.envi[(size_t)e * RE_COUNT + lane] : 0;
  if (lane < RD_COUNT) envd[lane] = S.envd[(size_t)e * RD_COUNT + lane];
  double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rr[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, er = 0.0, epos = 0.0;
  int ri[RI_COUNT] = {0, 0, 0};
  if (lane < RC_NB) {
#pragma unroll
    for (int f = 0; f < 6; ++f) b[f] = S.body[(size_t)f * E * RC_NB + row + lane];  // RB_PX .. RB_W
  }
  if (lane < 16) {
#pragma unroll
    for (int f = 0; f < 9; ++f) rr[f] = S.rob[(size_t)f * E * 16 + r16 + lane];  // RR_HEAD .. RR_MOVET
#pragma unroll
    for (int f = 0; f < RI_COUNT; ++f) ri[f] = S.robi[(size_t)f * E * 16 + r16 + lane];
    er = S.epr[r16 + lane]; epos = S.epr[E * 16 + r16 + lane];
  }
  __syncthreads();
  if (lane < 2 * R) {
    double* d = rc_blob_foot(T.st.robots[lane >> 1], lane & 1);
    d[0] = b[RB_PX]; d[1] = b[RB_PY]; d[2] = b[RB_VX]; d[3] = b[RB_VY]; d[4] = b[RB_ANG]; d[5] = b[RB_W];
  }
  if (lane == RC_BALL) { T.st.bpx = b[RB_PX]; T.st.bpy = b[RB_PY]; T.st.bvx = b[RB_VX]; T.st.bvy = b[RB_VY]; T.st.bw = b[RB_W]; }
  if (lane < R) {
    dynenv_robot_state_t& s = T.st.robots[lane];
    const int f = ri[RI_FLAGS];
    s.head_angle = rr[RR_HEAD]; s.head_moving = rr[RR_HEADMOV]; s.prevx = rr[RR_PREVX]; s.prevy = rr[RR_PREVY];
    s.initx = rr[RR_INITX]; s.inity = rr[RR_INITY]; s.penal_time = rr[RR_PENALT]; s.fall_time = rr[RR_FALLT]; s.move_time = rr[RR_MOVET];
    s.team = (f & RF_TEAMPOS) ? 1 : -1; s.penalized = !!(f & RF_PENAL); s.touching = !!(f & RF_TOUCH); s.might_push = !!(f & RF_PUSH);
    s.fallen = !!(f & RF_FALLEN); s.kicking = !!(f & RF_KICK); s.foot = !!(f & RF_FOOT); s.joint_removed = !!(f & RF_JREM);
    s.touch_cntr = ri[RI_TOUCHC]; s.fall_cntr = ri[RI_FALLC];
  }
  if (lane < DYNENV_MAX_ROBOTS) { T.st.episode_r[lane] = er; T.st.episode_pos_r[lane] = epos; }
  if (lane < 2) {  // the defenders are a set on the device: reported as an ascending id list
    int n = 0;
    for (int i = 0; i < DYNENV_MAX_ROBOTS; ++i) if (envi[RE_DEF0 + lane] & (1 << i)) T.st.defenders[lane][n++] = i;
    T.st.n_def[lane] = n;
    T.st.penal_times[lane] = envd[RD_PT0 + lane];
    T.st.goals[lane] = envi[RE_GOAL0 + lane]; T.st.closest[lane] = envi[RE_CLOSE0 + lane];
  }
  if (lane < 4) T.st.last_kicked[lane] = lane < envi[RE_NLK] ? envi[RE_LK0 + lane] : 0;
  if (lane == 0) {
    T.st.elapsed = envi[RE_ELAPSED]; T.st.n_robots = R; T.st.ball_owned = envi[RE_OWNED]; T.st.n_last_kicked = envi[RE_NLK];
    T.st.episode = envi[RE_EPISODE];
    T.st.ball_free_cntr = envd[RD_FREECNT]; T.st.grace_period = envd[RD_GRACE]; T.st.bprevx = envd[RD_BPREVX]; T.st.bprevy = envd[RD_BPREVY];
  }
  __syncthreads();
  unsigned long long* out = blobs + (size_t)k * RC_BLOB_WORDS;
  for (int q = lane; q < RC_BLOB_WORDS; q += 64) out[q] = T.q[q];
}

// status (may be nullptr): 0 written, 1 blob rejected (nothing of the environment touched but, if `raise`, error bit 6 raised on it: the
// batched call has nobody to return an error to, the synchronous one has), 2 index outside [0, E).  This is THE test of a blob's fit.
extern "C" __global__ void __launch_bounds__(64)
rc_set_states_kernel(RcState S, const int* __restrict__ idx, int first, const unsigned long long* __restrict__ blobs, int* __restrict__ status,
                      int raise) {
  __shared__ RcBlobTile T;
  __shared__ int envi[64];
  const int lane = threadIdx.x, k = blockIdx.x, R = S.R;
  const int e = idx ? uniform_i(idx[k]) : first + k;
  if (e < 0 || e >= S.E) { if (status && lane == 0) status[k] = 2; return; }
  const size_t E = (size_t)S.E, row = (size_t)e * RC_NB, r16 = (size_t)e * 16;
  const unsigned long long* in = blobs + (size_t)k * RC_BLOB_WORDS;
  for (int q = lane; q < RC_BLOB_WORDS; q += 64) T.q[q] = in[q];
  envi[lane] = 0;
  __syncthreads();
  {
    const int nd0 = uniform_i(T.st.n_def[0]), nd1 = uniform_i(T.st.n_def[1]);
    bool bad = uniform_i(T.st.n_robots) != R || nd0 < 0 || nd0 > DYNENV_MAX_ROBOTS || nd1 < 0 || nd1 > DYNENV_MAX_ROBOTS;
    bool badId = false;
    if (lane < 2 * DYNENV_MAX_ROBOTS) {
      const int t = lane / DYNENV_MAX_ROBOTS, i = lane - t * DYNENV_MAX_ROBOTS, id = T.st.defenders[t][i];
      badId = i < (t ? nd1 : nd0) && (id < 0 || id >= DYNENV_MAX_ROBOTS);
    }
    if (bad || wave_ballot(badId) != 0ull) {
      if (lane == 0) { if (raise) atomicOr(&S.envi[(size_t)e * RE_COUNT + RE_ERR], 64); if (status) status[k] = 1; }
      return;
    }
  }
  if (lane < RC_NB) {
    double b[RB_COUNT + 4];
#pragma unroll
    for (int f = 0; f < RB_COUNT + 4; ++f) b[f] = 0.0;  // velocity biases, forces and torque (a pending fall force) start over at 0
    if (lane < 2 * R) {
      const double* d = rc_blob_foot(T.st.robots[lane >> 1], lane & 1);
      b[RB_PX] = d[0]; b[RB_PY] = d[1]; b[RB_VX] = d[2]; b[RB_VY] = d[3]; b[RB_ANG] = d[4]; b[RB_W] = d[5];
      const DevSC sc = dev_sincos_inl(b[RB_ANG]);  // shape cache = geometry at cpSpaceAddShape time
      b[RB_COUNT + 0] = b[RB_PX]; b[RB_COUNT + 1] = b[RB_PY]; b[RB_COUNT + 2] = sc.c; b[RB_COUNT + 3] = sc.s;
    } else if (lane == RC_BALL) {
      b[RB_PX] = T.st.bpx; b[RB_PY] = T.st.bpy; b[RB_VX] = T.st.bvx; b[RB_VY] = T.st.bvy; b[RB_W] = T.st.bw;
      b[RB_COUNT + 0] = T.st.bpx; b[RB_COUNT + 1] = T.st.bpy; b[RB_COUNT + 2] = 1.0;
    }
#pragma unroll
    for (int f = 0; f < RB_COUNT + 4; ++f) S.body[(size_t)f * E * RC_NB + row + lane] = b[f];
  }
  bool jrem = false;
  if (lane < 16) {
    double rr[RR_COUNT];
#pragma unroll
    for (int f = 0; f < RR_COUNT; ++f) rr[f] = 0.0;  // RR_JX, RR_JY, RR_JROT: the joints' accumulated impulses start over at 0
    int ri[RI_COUNT] = {0, 0, 0};
    if (lane < R) {
      const dynenv_robot_state_t& s = T.st.robots[lane];
      rr[RR_HEAD] = s.head_angle; rr[RR_HEADMOV] = s.head_moving; rr[RR_PREVX] = s.prevx; rr[RR_PREVY] = s.prevy;
      rr[RR_INITX] = s.initx; rr[RR_INITY] = s.inity; rr[RR_PENALT] = s.penal_time; rr[RR_FALLT] = s.fall_time; rr[RR_MOVET] = s.move_time;
      ri[RI_FLAGS] = (s.team > 0 ? RF_TEAMPOS : 0) | (s.penalized ? RF_PENAL : 0) | (s.touching ? RF_TOUCH : 0) | (s.might_push ? RF_PUSH : 0) |
                     (s.fallen ? RF_FALLEN : 0) | (s.kicking ? RF_KICK : 0) | (s.foot ? RF_FOOT : 0) | (s.joint_removed ? RF_JREM : 0);
      ri[RI_TOUCHC] = s.touch_cntr; ri[RI_FALLC] = s.fall_cntr;
      jrem = s.joint_removed != 0;
    }
#pragma unroll
    for (int f = 0; f < RR_COUNT; ++f) S.rob[(size_t)f * E * 16 + r16 + lane] = rr[f];
#pragma unroll
    for (int f = 0; f < RI_COUNT; ++f) S.robi[(size_t)f * E * 16 + r16 + lane] = ri[f];
    S.epr[r16 + lane] = lane < DYNENV_MAX_ROBOTS ? T.st.episode_r[lane] : 0.0;
    S.epr[E * 16 + r16 + lane] = lane < DYNENV_MAX_ROBOTS ? T.st.episode_pos_r[lane] : 0.0;
  }
  // the environment's int row, built in LDS.  Constraint order: robot r's pivot joint (2r; absent once removed) then its rotary limit
  // (2r + 1), robots in id order - the entries in front of robot r are 2r minus the removed joints below it
  const uint64_t jremMask = wave_ballot(jrem);
  if (lane < R) {
    int at = RE_CORDER + 2 * lane - __popcll(jremMask & lanemask_lt());
    if (!jrem) envi[at++] = 2 * lane;
    envi[at] = 2 * lane + 1;
  }
  if (lane < 2) {
    int m = 0;
    for (int i = 0; i < T.st.n_def[lane]; ++i) m |= 1 << T.st.defenders[lane][i];
    envi[RE_DEF0 + lane] = m; envi[RE_GOAL0 + lane] = T.st.goals[lane]; envi[RE_CLOSE0 + lane] = T.st.closest[lane];
  }
  if (lane < 4) envi[RE_LK0 + lane] = T.st.last_kicked[lane];
  if (lane == 0) {
    envi[RE_ELAPSED] = T.st.elapsed; envi[RE_OWNED] = T.st.ball_owned; envi[RE_NLK] = T.st.n_last_kicked;
    envi[RE_NCON] = 2 * R - __popcll(jremMask); envi[RE_EPISODE] = T.st.episode;  // RE_OCC, RE_ERR, RE_PIVFIRST: 0
  }
  __syncthreads();
  if (lane < RE_COUNT) S.envi[(size_t)e * RE_COUNT + lane] = envi[lane];
  if (lane < RD_COUNT) {
    const double v = lane == RD_FREECNT ? T.st.ball_free_cntr : lane == RD_GRACE ? T.st.grace_period : lane == RD_PT0 ? T.st.penal_times[0] :
                     lane == RD_PT1 ? T.st.penal_times[1] : lane == RD_BPREVX ? T.st.bprevx : lane == RD_BPREVY ? T.st.bprevy : 0.0;
    S.envd[(size_t)e * RD_COUNT + lane] = v;
  }
  if (status && lane == 0) status[k] = 0;
}

extern "C" __global__ void rc_error_flags_env_kernel(RcState S, int* __restrict__ flags) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < S.E) flags[e] = S.envi[(size_t)e * RE_COUNT + RE_ERR];
}
