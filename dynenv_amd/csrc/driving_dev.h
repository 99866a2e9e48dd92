// driving_dev.h — device-side data layout of the batched Driving environment (HBM SoA + LDS tile).
//
// Mapping: ONE WAVEFRONT (64 lanes) PER ENVIRONMENT.  Lane l doubles as
//   * object l of the scene: cars 0..9, pedestrians 10..29 (dynamic bodies, state in the LDS tile), obstacles 30..49,
//     buildings 50..53 - for integration and for the broadphase (bit i of lane j's mask = canonical pair (car i, j))
//   * one quarter of a candidate pair in the narrowphase (four lanes per pair)
//   * the owner of contact-cache slot l    (l < DRV_NS persistent arbiters)
// HBM layout is field-major with the 32 body slots of one env contiguous (`field[e][32]`), so a wave's load of one
// field is a single 256-byte coalesced segment.
#pragma once
#include "dev_common.h"

#define DRV_MAXA 10
#define DRV_MAXP 20
#define DRV_MAXO 20
#define DRV_NB 32          /* dynamic body slots per env (30 used) */
#define DRV_NS 24          /* persistent arbiter (contact cache) slots per env (LDS budget: 16 envs per CU) */
#define DRV_SLOT_PED 10
#define DRV_SLOT_OBST 30
#define DRV_SLOT_BLD 50
#define DRV_W 1700.0
#define DRV_H 1000.0
#define DRV_MAX_TIME 6000
#define DRV_TIME_DIFF 10
#define DRV_LANE_ROWS 8
// the scene's fixed geometry (DrivingEnvironment.py:101-106, Obstacle / Pedestrian shapes): building k of 4 by its centre, the half
// extents of a building's and of an obstacle's box, a pedestrian's radius
#define DRV_BLD_CX(k) (((k) & 2) ? 1385.0 : 365.0)
#define DRV_BLD_CY(k) (((k) & 1) ? 800.0 : 200.0)
#define DRV_BLD_HX 400.0
#define DRV_BLD_HY 225.0
#define DRV_OBST_H 10.0
#define DRV_PED_R 5.0
// cutils.py:318-323 normalize and the Full observation's factors (DrivingEnvironment.py:121-124)
#define STD_NORM_X (0.5 / (DRV_W + 100.0))
#define STD_NORM_Y (0.5 / (DRV_H + 100.0))
#define STD_NORM_W (1.0 / 15.0)
#define STD_NORM_H (1.0 / 25.0)
DE_HD double normalize_obs(double pt, double nf, double mean) { return ((pt * nf) - mean) * 2.0 * 1.0; }

// body f64 fields
enum { BF_PX = 0, BF_PY, BF_VX, BF_VY, BF_ANG, BF_W, BF_VBX, BF_VBY, BF_WB, BF_COUNT };
// car f64 fields
enum { CF_DIRX = 0, CF_DIRY, CF_PREVX, CF_PREVY, CF_GOALX, CF_GOALY, CF_COUNT };
// env int fields
enum { EI_ELAPSED = 0, EI_ALLFIN, EI_NPED, EI_NOBST, EI_EPISODE, EI_OCC, EI_ERR, EI_SHORTCUT,
       EI_N_FAST, EI_N_QUIET, EI_N_CONTACT, EI_N_SLOTS, /* diagnostics: substeps per path, sum of live slots */
       EI_N_WHY_CAND, EI_N_WHY_MOVING, EI_N_WHY_INERT, EI_N_STEADY, EI_N_LIGHT, /* why the quiescent shortcut was not taken */
       EI_N_SPLIT, /* contact-path substeps whose sweeps ran in drv_solve_general_split (general multi-level solves) */
       EI_DEFER_OBS, /* Partial: first agent whose observation is left to drv_partial_obs_deferred_kernel (A = none) */
       EI_COUNT };
// envi[EI_SHORTCUT]: what the step's shortcuts carry from launch to launch - every cached arbiter was inert / steady when the contact
// path last ran, and L.vb* hold the bias velocities of a solve the next position update has to see
enum { SC_INERT = 1, SC_STEADY = 2, SC_VB_VALID = 4 };
// (envi[EI_ERR] holds the DYNENV_ERRBIT_* of include/dynenv.h)
// arbiter states (Chipmunk cpArbiterState)
enum { ARB_FIRST = 0, ARB_NORMAL = 1, ARB_IGNORE = 2, ARB_CACHED = 3 };
// The two packed words of a contact-cache slot.  Both start with the slot record: state[0:8) count[8:16) age[16:24).
//   s_meta (persisted):  record | steady[24] inert[25] - how the slot came out of its last evaluation
//   pk (what the contact path hands the solve functions, who write s_meta from it):
//                        record | touched[24] freeMe[25] hashSame[26] prevInert[27] skipped[28] slotOcc[29] active[30]
enum { SLOT_COUNT_SH = 8, SLOT_AGE_SH = 16, SLOT_REC_BITS = 24,
       META_STEADY_SH = SLOT_REC_BITS, META_INERT_SH,
       PK_TOUCHED_SH = SLOT_REC_BITS, PK_FREE_SH, PK_HASH_SAME_SH, PK_PREV_INERT_SH, PK_SKIPPED_SH, PK_OCC_SH, PK_ACTIVE_SH };
#define SLOT_STATE(w) ((w)&0xFF)
#define SLOT_COUNT(w) (((w) >> SLOT_COUNT_SH) & 0xFF)
#define SLOT_AGE(w) (((w) >> SLOT_AGE_SH) & 0xFF)
#define SLOT_BIT(w, sh) (((w) >> (sh)) & 1)
DE_HD constexpr int slot_rec(int state, int count, int age) { return state | (count << SLOT_COUNT_SH) | (age << SLOT_AGE_SH); }
DE_HD constexpr int meta_pack(int state, int count, int age, bool steady, bool inert) {
  return slot_rec(state, count, age) | (steady ? (1 << META_STEADY_SH) : 0) | (inert ? (1 << META_INERT_SH) : 0);
}
DE_HD constexpr int pk_pack(int state, int count, int age, bool touched, bool freeMe, bool hashSame, bool prevInert, bool skipped, bool slotOcc,
                            bool active) {
  return slot_rec(state & 0xFF, count & 0xFF, age & 0xFF) | (touched ? 1 << PK_TOUCHED_SH : 0) | (freeMe ? 1 << PK_FREE_SH : 0) |
         (hashSame ? 1 << PK_HASH_SAME_SH : 0) | (prevInert ? 1 << PK_PREV_INERT_SH : 0) | (skipped ? 1 << PK_SKIPPED_SH : 0) |
         (slotOcc ? 1 << PK_OCC_SH : 0) | (active ? 1 << PK_ACTIVE_SH : 0);
}
static_assert((pk_pack(0xA1, 0xB2, 0xC3, true, true, true, true, true, true, true) & ((1 << SLOT_REC_BITS) - 1)) == meta_pack(0xA1, 0xB2, 0xC3, false, false) &&
              PK_ACTIVE_SH == 30, "the low 24 bits of pk are s_meta's state, count and age; pk ends below the sign bit");
// LanePosition (cutils.py:143-148)
enum { LP_AtGoal = 0, LP_InRightLane = 1, LP_InOpposingLane = 2, LP_OverRoad = 3, LP_OffRoad = 4 };

// car flag word:  type[0:2) team[2:4) finished[4] crashed[5] fric[6] lanepos[8:11)
// ped flag word:  road[0] side[1] dead[2] crossing[3] begin[4] speed[8:12)
#define CARF_TYPE(f) ((f)&3)
#define CARF_TEAM(f) (((f) >> 2) & 3)
#define CARF_FIN(f) (((f) >> 4) & 1)
#define CARF_CRASHED(f) (((f) >> 5) & 1)
#define CARF_FRIC(f) (((f) >> 6) & 1)
#define CARF_LP(f) (((f) >> 8) & 7)
#define CARF_SET_LP(f, lp) (((f) & ~(7 << 8)) | ((lp) << 8))
#define CARF_FIN_BIT (1 << 4)
#define CARF_CRASHED_BIT (1 << 5)
#define CARF_FRIC_BIT (1 << 6)
#define CARF_CRASH_BITS (CARF_FIN_BIT | CARF_CRASHED_BIT | CARF_FRIC_BIT) /* Car.crash(): finished, crashed, friction_car_crashed */
#define PEDF_ROAD(f) ((f)&1)
#define PEDF_SIDE(f) (((f) >> 1) & 1)
#define PEDF_DEAD(f) (((f) >> 2) & 1)
#define PEDF_CROSSING(f) (((f) >> 3) & 1)
#define PEDF_BEGIN(f) (((f) >> 4) & 1)
#define PEDF_SPEED(f) (((f) >> 8) & 15)
#define PEDF_DEAD_BIT (1 << 2)
#define CARF_PACK(type, team, fin, crashed, fric, lp) \
  ((type) | ((team) << 2) | ((fin) << 4) | ((crashed) << 5) | ((fric) << 6) | ((lp) << 8))
#define PEDF_PACK(road, side, dead, crossing, begin, speed) \
  ((road) | ((side) << 1) | ((dead) << 2) | ((crossing) << 3) | ((begin) << 4) | ((speed) << 8))

struct DrvRoad {
  int nLanes;
  double width, length, dirAngle, followDist;
  double cosDir0; /* dm_cos(dirAngle - 0.0): the pedestrian / obstacle road test always passes angle 0 */
  V2 p0, p1, dir, normal;
  V2 walk[2][2];
};

struct DrvConst {
  DrvRoad roads[2];
  float laneRows[DRV_LANE_ROWS * 5];
  double carMass[4], carInertia[4], carHx[4], carHy[4], carPower[4];
  double pedMass, pedInertia;
  double turnCos[2], turnSin[2]; /* cos/sin(-/+ 2*pi/180) */
};

// per-lane inputs of the Partial observation of one environment (lane = body slot / obstacle / car index)
struct PvIn {
  double px, py, ang; /* body slot `lane` (< 32), 0 for unused slots */
  double ox, oy;      /* obstacle `lane` (< nObst) */
  double gx, gy;      /* goal of car `lane` (< A) */
  int flags;          /* flag word of body slot `lane` */
};

struct DrvState {
  int E, A, obs_dim, pad0;
  uint64_t seed;
  int env_id_offset, pad1;
  double* body;   /* [BF_COUNT][E][32] */
  double* carx;   /* [CF_COUNT][E][16] */
  int* flags;     /* [E][32] */
  int* aux;       /* [E][32]  ped `moving` (ms) */
  double* obst;   /* [2][E][20] */
  int* envi;      /* [E][EI_COUNT] */
  double* epr;    /* [2][E][16] episode_r, episode_pos_r */
  int* s_pair;    /* [E][NS]  pair id (i<<8|j) */
  int* s_meta;    /* [E][NS]  state | count<<8 | age<<16 */
  uint32_t* s_hash; /* [2][E][NS] */
  double* s_imp;  /* [4][E][NS] jn0 jt0 jn1 jt1 */
  int* lastcand;  /* [E][64] per-lane candidate mask of the last substep (-1 = unknown); with envi[EI_SHORTCUT] (SC_*) the shortcut state */
  /* SIMD isolation of the slow environments (scheduling only - which block steps which environment; see drv_iso_assign): the header
     words DRV_ISOW_* below, then three lists of ids used in rotation (step t reads list t % 3, fills (t + 1) % 3, clears (t + 2) % 3);
     a step's "placement validated" word is written by the launch before the one that reads it.  iso_done[e] = tick of e's last
     finished step; iso_hw[t & 1][b] = hardware id (XCC | SE | SH | CU | SIMD) block b of step t ran on.  None of this is simulation
     state: it is allocated outside the checkpointed arrays and starts over at dynenv_checkpoint_load. */
  int* iso;
  int* iso_done;
  unsigned* iso_hw;
  /* Partial observation: the environments whose agent passes the step launch left to the deferred one (scheduling scratch as
     well; DRV_PVQ_* below), one list per parity p = pv_par: the host flips it every step, and the deferred launch of a step clears
     the other parity's length for the next one. */
  int* pvq;
  int pv_par;
  int tick, iso_on;  /* iso_on: 0 off, 1 isolation (E = one residency round), 2 slow environments first (E larger) */
  int tick_src;      /* 0: `tick` / `pv_par` above, advanced by the host per launch; 1: the device words DRV_ISOW_TICK / DRV_ISOW_PV_PAR, advanced by
                        drv_tick_advance_kernel in front of every step - set for good once a step has been captured into a hipGraph */
};
#ifndef DRV_ISO_MAX
#define DRV_ISO_MAX 192  /* at most this many environments get a SIMD of their own (iso_on = 1).  The list fills in FINISHING order: a cap
                            below the number of listed environments drops the slowest of them (round 6: 64 -> 192 with the threshold at
                            75 % instead of 80 %: -0.6 %; 40: +2.2 %; 256 at 65 %: +2 %) */
#endif
#ifndef DRV_ISO_MIN_E
#define DRV_ISO_MIN_E 3072 /* isolation (mode 1) for DRV_ISO_MIN_E < E <= 4096: measured -6.5 % at 4095, -6 % at 4000, -4 % at 3584, -0.8 % at 3072, +0.8 % at 2048 (HISTORY "Round 5") */
#endif
#define DRV_ISO_LIST 256 /* capacity of a list; iso_on = 2 (more environments than fit at once) starts up to this many slow ones first */
#define DRV_ISO_HDR 16    /* header words of DrvState.iso in front of the three lists */
#define DRV_ISO_WORDS (DRV_ISO_HDR + 3 * DRV_ISO_LIST)
// the header words (x3: one per list)
enum { DRV_ISOW_LEN = 0,      /* x3  list lengths */
       DRV_ISOW_SLOWEST = 3,  /* x3  cycles of the slowest environment */
       DRV_ISOW_GAVE_UP = 7,  /*     placeholders that gave up waiting */
       DRV_ISOW_VALID = 8,    /* x3  1: the block -> SIMD placement isolation relies on was observed */
       DRV_ISOW_INVALID = 11, /*     launches in which it was not */
       DRV_ISOW_COOL = 12,    /*     cool-down counter of the validation */
       DRV_ISOW_TICK = 13,    /*     tick and ... */
       DRV_ISOW_PV_PAR = 14   /*     ... pv_par on the device (tick_src = 1) */ };
static_assert(DRV_ISOW_LEN + 3 <= DRV_ISOW_SLOWEST && DRV_ISOW_SLOWEST + 3 <= DRV_ISOW_GAVE_UP && DRV_ISOW_GAVE_UP < DRV_ISOW_VALID &&
              DRV_ISOW_VALID + 3 <= DRV_ISOW_INVALID && DRV_ISOW_INVALID < DRV_ISOW_COOL && DRV_ISOW_COOL < DRV_ISOW_TICK &&
              DRV_ISOW_TICK < DRV_ISOW_PV_PAR && DRV_ISOW_PV_PAR < DRV_ISO_HDR, "the header words are distinct and in front of the lists");
#define DRV_TICK_WRAP (3 * (1 << 28)) /* tick wraps at a multiple of 3: the three lists keep rotating in order */
// DrvState.pvq: the length word of parity p (a cache line apart), the ids of its list, the words in all
#define DRV_PVQ_LEN(p) (16 * (p))
#define DRV_PVQ_IDS 32
#define DRV_PVQ_LIST(p, E) (DRV_PVQ_IDS + (p) * (E))
#define DRV_PVQ_WORDS(E) (DRV_PVQ_IDS + 2 * (E))
#define DRV_ISO_COOLDOWN 64 /* validated launches isolation stays off for after one that did not validate */
#define DRV_ISO_G0 256     /* first SIMD group isolation uses: groups 256..511 are the ones whose four blocks always share a SIMD */
#define DRV_ISO_GSPAN 256  /* ... and how many of them the device-side validation checks (DRV_ISO_MAX <= GSPAN) */
#define DRV_ISO_GROUPS 1024 /* SIMDs of an MI355X: blocks b, b + 1024, b + 2048, b + 3072 of a launch share one (measured) */
