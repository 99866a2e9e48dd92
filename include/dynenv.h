/* dynenv.h — C ABI of the MI355X-native batched DynEnv step() (libdynenv_hip.so).
 *
 * Drop-in boundary for the reference's hot path.  Each entry point names the reference interface it replaces
 * (paths relative to the reference repo root):
 *
 *   dynenv_create        <- DynEnv/__init__.py:6-25 make_dyn_env(...) building num_envs DrivingEnvironment /
 *                           RoboCupEnvironment objects (DrivingEnvironment.py:20-56, RoboCupEnvironment.py:23-71)
 *   dynenv_reset         <- DynEnv/utils/subproc_vec_env.py:118-122 SubprocVecEnv.reset ->
 *                           DynEnv/environment_base.py:205-224 EnvironmentBase.reset
 *   dynenv_reset_masked  <- the same EnvironmentBase.reset (environment_base.py:205-224), for chosen environments: what a
 *                           SubprocVecEnv worker does when ITS environment is done (subproc_vec_env.py:19-22)
 *   dynenv_step_masked   <- a SubprocVecEnv worker that is sent nothing does nothing: the step for chosen environments
 *   dynenv_step          <- DynEnv/utils/subproc_vec_env.py:102-111 step_async/step_wait ->
 *                           DynEnv/DrivingEnvironment.py:248-322 / DynEnv/RoboCupEnvironment.py:446-524 step
 *   dynenv_episode_stats <- info['episode_r'|'episode_p_r'|'episode_o_r'|'episode_g'] (DrivingEnvironment.py:310-316,
 *                           RoboCupEnvironment.py:516-521)
 *   dynenv_seed          <- DynEnv/environment_base.py:190-193 set_random_seed
 *   dynenv_get/set_state <- (no reference equivalent; SURVEY §5 "checkpoint/resume" + parity tests)
 *   dynenv_get/set_exact <- (no reference equivalent: exact save / restore of chosen environments on the device, for lookahead)
 *   dynenv_destroy       <- SubprocVecEnv.close (subproc_vec_env.py:124-133)
 *
 * All functions return 0 on success, <0 on error (dynenv_last_error() gives the text).  Pointers named *_dev are
 * DEVICE pointers (HBM) owned by the caller; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * No torch types cross this boundary.  A handle is single-threaded; distinct handles are independent (dynenv_last_error() is
 * per calling thread).
 * There is NO CPU fallback: every entry fails with DYNENV_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef DYNENV_H
#define DYNENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYNENV_ABI_VERSION 3 /* 2: dynenv_debug_counters writes 16 words; checkpoints hold simulation state only.  3: dynenv_error_flags - Partial-observation rows dropped moved from bit 1 to its own bit 3; dynenv_step may be stream-captured */

/* DynEnvType / ObservationType / NoiseType values are the reference's (cutils.py:10-51) */
#define DYNENV_ROBO_CUP 0
#define DYNENV_DRIVE 1
#define DYNENV_OBS_FULL 0
#define DYNENV_OBS_PARTIAL 1
#define DYNENV_NOISE_RANDOM 0
#define DYNENV_NOISE_REALISTIC 1

#define DYNENV_OK 0
#define DYNENV_ERR_ARG (-1)
#define DYNENV_ERR_NO_DEVICE (-2)
#define DYNENV_ERR_HIP (-3)
#define DYNENV_ERR_UNSUPPORTED (-4)
#define DYNENV_ERR_ACTION (-5) /* reference raises on malformed actions, DrivingEnvironment.py:262-263,365-368 */

/* RoboCup class-level switches (RoboCupEnvironment.py:18-21): randomInit (:241, :326 random robot spots, ball position and
 * ownership), deterministicTurn (:317 head starts at team * headMaxAngle, :529 the head action is forced to -3 * team),
 * canFall, useObsRewards; and the constructor's allowHeadTurn (:24, :339, :539).  All five are implemented. */
#define DYNENV_FLAG_RANDOM_INIT 1
#define DYNENV_FLAG_DETERMINISTIC_TURN 2
#define DYNENV_FLAG_CAN_FALL 4
#define DYNENV_FLAG_USE_OBS_REWARDS 8
#define DYNENV_FLAG_ALLOW_HEAD_TURN 16

#define DYNENV_MAX_CARS 10
#define DYNENV_MAX_PEDS 20
#define DYNENV_MAX_OBST 20
#define DYNENV_DRIVE_LANES 8

typedef struct dynenv_cfg {
  int32_t abi_version;    /* DYNENV_ABI_VERSION */
  int32_t env_type;       /* DYNENV_DRIVE | DYNENV_ROBO_CUP */
  int32_t num_envs;       /* environments owned by THIS handle (this GPU's shard) */
  int32_t n_players;      /* nPlayers: cars (Driving, <=10) or robots per team (RoboCup, <=5) */
  int32_t obs_type;       /* DYNENV_OBS_* */
  int32_t noise_type;     /* DYNENV_NOISE_* */
  double noise_magnitude; /* 0..5 */
  uint64_t seed;
  int32_t env_id_offset;  /* global id of local env 0: RNG streams are keyed by global id => shard-count invariant */
  int32_t flags;          /* DYNENV_FLAG_* */
  int32_t device_id;      /* HIP device ordinal */
  int32_t reserved;
} dynenv_cfg_t;

/* dense, padded observation layout of one (env, time step, agent) row; all float32 */
typedef struct dynenv_layout {
  int32_t num_envs, n_agents, n_time_steps, obs_dim;
  int32_t action_dim;       /* 2 Driving, 4 RoboCup */
  int32_t n_blocks;         /* number of row blocks below */
  int32_t block_offset[8];  /* float offset inside the obs row */
  int32_t block_rows[8];    /* row capacity */
  int32_t block_feat[8];    /* features per row */
  int32_t steps_per_episode;
  int32_t reserved;
} dynenv_layout_t;

/* Driving layout block ids: mirrors ((cars, obstacles, pedestrians), (self, lanes)) of DrivingEnvironment.py:121-124 */
#define DYNENV_DRV_BLOCK_SELF 0
#define DYNENV_DRV_BLOCK_CARS 1
#define DYNENV_DRV_BLOCK_OBST 2
#define DYNENV_DRV_BLOCK_PEDS 3
#define DYNENV_DRV_BLOCK_LANES 4

/* ---- canonical per-env state blob (checkpoint / parity tests).  set_state clears the contact cache. ---- */
typedef struct dynenv_car_state {
  double px, py, vx, vy, angle, w;
  double dirx, diry, prevx, prevy, goalx, goaly;
  int32_t type, team, finished, crashed, lane_pos, fric; /* fric: 0 friction_car, 1 friction_car_crashed */
  int32_t pad[2];
} dynenv_car_state_t;

typedef struct dynenv_ped_state {
  double px, py, vx, vy;
  int32_t road, side, dead, moving, speed, crossing, begin_crossing, pad;
} dynenv_ped_state_t;

typedef struct dynenv_driving_state {
  int32_t elapsed, all_finished, n_cars, n_peds, n_obst, episode;
  int32_t pad[2];
  double episode_r[DYNENV_MAX_CARS], episode_pos_r[DYNENV_MAX_CARS];
  dynenv_car_state_t cars[DYNENV_MAX_CARS];
  dynenv_ped_state_t peds[DYNENV_MAX_PEDS];
  double obst_x[DYNENV_MAX_OBST], obst_y[DYNENV_MAX_OBST];
} dynenv_driving_state_t;

/* RoboCup blob.  set_state clears the contact cache, the joints' accumulated impulses and pending fall forces. */
#define DYNENV_MAX_ROBOTS 10
typedef struct dynenv_robot_state {
  double lpx, lpy, lvx, lvy, la, lw; /* left foot body */
  double rpx, rpy, rvx, rvy, ra, rw; /* right foot body */
  double head_angle, head_moving, prevx, prevy, initx, inity, penal_time, fall_time, move_time;
  int32_t team, penalized, touching, touch_cntr, might_push, fallen, fall_cntr, kicking, foot, joint_removed;
  int32_t pad[2];
} dynenv_robot_state_t;

typedef struct dynenv_robocup_state {
  int32_t elapsed, n_robots, ball_owned, n_last_kicked;
  int32_t last_kicked[4], goals[2], closest[2], n_def[2], defenders[2][DYNENV_MAX_ROBOTS];
  int32_t episode, pad;
  double ball_free_cntr, grace_period, penal_times[2];
  double bpx, bpy, bvx, bvy, bw, bprevx, bprevy;
  double episode_r[DYNENV_MAX_ROBOTS], episode_pos_r[DYNENV_MAX_ROBOTS];
  dynenv_robot_state_t robots[DYNENV_MAX_ROBOTS];
} dynenv_robocup_state_t;

typedef struct dynenv dynenv_t;

int dynenv_abi_version(void);
const char* dynenv_last_error(void);

int dynenv_create(const dynenv_cfg_t* cfg, dynenv_t** out);
void dynenv_destroy(dynenv_t* h);
int dynenv_layout(const dynenv_t* h, dynenv_layout_t* out);

/* set_random_seed for every environment of the handle: all 64 bits of `seed` key every draw from now on (include/dynenv_math.h
 * dm_env_rng: seed, global id, episode counter, purpose, entity, time).  Host state only: nothing is launched, copied or synchronised.
 *   Before a reset: the reset draws its scene from (seed, global id, episode) - the handle is then what a handle created with `seed`
 *   and brought to the same episode counters would be.
 *   Mid-episode: no byte of any environment's state changes (the seed is in no state blob); the step-time draws of the running
 *   episode - pedestrian moves, RoboCup's dice and kicks, observation noise - come from the new seed from the next step on.
 *   Checkpoints: dynenv_checkpoint_save stores the handle's current seed, dynenv_checkpoint_load adopts the checkpoint's, whatever
 *   dynenv_seed set before; a dynenv_seed after a load holds until the next load.
 *   After a capture: the seed travels as a by-value kernel argument, so a dynenv_step / dynenv_step_masked / dynenv_reset_masked that
 *   was captured into a hipGraph replays with the seed it was captured with.  From the first such call issued on a capturing stream,
 *   for the rest of the handle's life, a `seed` other than the handle's returns DYNENV_ERR_UNSUPPORTED and changes nothing (the
 *   handle's own seed again is accepted): create a new handle for another seed. */
int dynenv_seed(dynenv_t* h, uint64_t seed);

/* (Re)build every environment's scene and write the first observation(s): obs_dev float32 [E, T, A, obs_dim].  The launches of
 * dynenv_reset_masked without a mask.
 * Alignment: obs_dev must be 16-byte aligned here, in dynenv_reset_masked and in every step call (the observation writers store
 * float4 where the row layout allows it); a non-NULL obs_dev that is not returns DYNENV_ERR_ARG before a device is looked for, and
 * nothing is launched.  The other buffers of these calls need their element's natural alignment only. */
int dynenv_reset(dynenv_t* h, float* obs_dev, void* stream);

/* Reset exactly the environments e with mask_dev[e] != 0 (uint8 [E]; the dones_dev of the step before it is a valid mask).
 * obs_dev as for dynenv_reset: float32 [E, T, A, obs_dim], or NULL.
 *   A LISTED environment ends up as dynenv_reset would leave it, starting from the same per-environment episode counter - byte for
 *   byte, in every device array of the handle: its episode counter goes up by one, its elapsed time becomes 0 and its scene is redrawn
 *   from (seed, global id, episode); its accumulators are zeroed, its contact-cache slots freed, its shortcut state and its error word
 *   cleared; RoboCup: the joints' order, the per-environment constants and the shape cache are rewritten.  obs_dev[e] gets the first
 *   observation: T copies for Full, T separate noisy draws (time word t) for Partial.
 *   An UNLISTED environment: no byte of its state and no byte of obs_dev[e] changes.
 * Ordered on `stream`; no host synchronisation, no allocation, no host copy: capturable into a hipGraph behind a captured dynenv_step.
 * One wave per environment, the launches of dynenv_reset; the scheduler's scratch (timing only) is not touched.
 * Errors: NULL handle or mask -> DYNENV_ERR_ARG. */
int dynenv_reset_masked(dynenv_t* h, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* One environment step for all E environments (10 / 50 physics substeps fused in one launch).
 *   actions_dev  int32 [E, A, action_dim]      obs_dev float32 [E, T, A, obs_dim]
 *   rewards_dev  float64 [E, A]                dones_dev uint8 [E]
 * Does NOT auto-reset: the host mirror calls dynenv_reset after a terminal step (SubprocVecEnv semantics).
 * obs_dev may be NULL (no observation written) except for RoboCup with Partial observations, whose rewards contain the
 * observation reward of processSeens (RoboCupEnvironment.py:497-524) and come out of the same pass: DYNENV_ERR_ARG then.
 * Alignment: a non-NULL obs_dev must be 16-byte aligned (dynenv_step, dynenv_step_head, dynenv_step_masked alike), else
 * DYNENV_ERR_ARG: checked with the other arguments, before a device is looked for; no state changes and nothing is launched.
 * May be captured into a hipGraph (stream capture) and replayed: per-step scheduling counters move to the device on the first
 * captured call, for the rest of the handle's life (INTEGRATION.md "Scheduling, checkpoints and graphs"). */
int dynenv_step(dynenv_t* h, const int32_t* actions_dev, float* obs_dev, double* rewards_dev, uint8_t* dones_dev,
                void* stream);

/* The noise-free Full observation of the CURRENT state, whatever the handle's observation type: full_dev float32
 * [E, A, dynenv_full_obs_dim(h)] in the Full layout (Driving: self 9 | cars (A-1) x 7 | obstacles 20 x 4 | pedestrians 20 x 2 |
 * lanes 8 x 5; RoboCup: ball 4 | self 8 | robots (A-1) x 6).  This is what the reference puts into info['Full State'] /
 * info['Recon States'] after every step in every observation mode (getFullState, DrivingEnvironment.py:306-307,
 * RoboCupEnvironment.py:511-512) and what a caller needs after dynenv_set_state / dynenv_checkpoint_load.
 * Alignment: full_dev must be 16-byte aligned, as obs_dev in dynenv_reset; DYNENV_ERR_ARG otherwise, nothing launched. */
int dynenv_full_obs_dim(const dynenv_t* h);
int dynenv_full_obs(dynenv_t* h, float* full_dev, void* stream);

/* RoboCup's info['Full State'] = getFullState(agent=None) of the CURRENT state (RoboCupEnvironment.py:511, :1149-1161), which is
 * NOT a per-agent row of dynenv_full_obs: robots float32 [A][6] = (normalize(x, standardNorm, 0), normalize(y, standardNorm, 0),
 * cos a, sin a, team, fallen | penalized) in field coordinates (no team flip; normalize = cutils.py:318-323), then the ball
 * [3] = (normalize(bx), normalize(by), ballOwned): state_dev float32 [E, dynenv_global_state_dim(h)] with dim = 6 A + 3.
 * The reference's trainer reads the robots' last column from it (models/train.py:272).  Driving: dim 0 and
 * DYNENV_ERR_UNSUPPORTED - its getFullState(None) (DrivingEnvironment.py:697-711) is columns {0..5, 8} of every car's own self
 * block in dynenv_full_obs plus the shared obstacle / pedestrian / lane blocks, bit for bit. */
int dynenv_global_state_dim(const dynenv_t* h);
int dynenv_global_state(dynenv_t* h, float* state_dev, void* stream);

/* dynenv_step with the reference's continuous head action: RoboCup built with allowHeadTurn (make_dyn_env's
 * use_continuous_actions, DynEnv/__init__.py:11) takes Tuple((MultiDiscrete([5, 3, 3]), Box(-3, 3, (1,))))
 * (RoboCupEnvironment.py:339-342); head_dev float64 [E, A] carries the Box channel (turnHead(head), Robot.py:136-138),
 * actions_dev[..., 3] is ignored then.  head_dev == NULL: the discrete head action of actions_dev[..., 3] (what dynenv_step
 * does).  DYNENV_ERR_ARG unless the handle is RoboCup with DYNENV_FLAG_ALLOW_HEAD_TURN. */
int dynenv_step_head(dynenv_t* h, const int32_t* actions_dev, const double* head_dev, float* obs_dev, double* rewards_dev,
                     uint8_t* dones_dev, void* stream);

/* One environment step for exactly the environments e with mask_dev[e] != 0 (uint8 [E]); the others stand still.  The buffers are
 * dynenv_step's; head_dev may be NULL, and non-NULL is allowed under dynenv_step_head's rule only; RoboCup with Partial observations
 * needs obs_dev, as in dynenv_step.
 *   A LISTED environment gets exactly what dynenv_step / dynenv_step_head would have done to it - byte for byte, in every device
 *   array of the handle and in obs_dev[e], rewards_dev[e], dones_dev[e] - however many calls it sat out before: everything it draws is
 *   keyed by its own elapsed time and episode counter.
 *   An UNLISTED environment: no byte of its state changes - bodies, contact cache (warm-start impulses), shortcut state, call-to-call
 *   caches, episode accumulators, diagnostic counters, error word - and no byte of obs_dev[e], rewards_dev[e], dones_dev[e]: those rows
 *   keep whatever the buffers held (a caller that sums rewards masks them).  Its rows of actions_dev / head_dev are not read.
 * Ordered on `stream`; no host synchronisation, no allocation, no host copy.  Capturable into a hipGraph like dynenv_step; the mask is
 * read by the kernel, so a replay uses what mask_dev holds THEN.  The launches of dynenv_step; the scheduler's scratch (timing
 * only) sees the listed environments alone.
 * Errors: NULL handle or mask -> DYNENV_ERR_ARG (before a device is looked for); then dynenv_step_head's. */
int dynenv_step_masked(dynenv_t* h, const uint8_t* mask_dev, const int32_t* actions_dev, const double* head_dev,
                       float* obs_dev, double* rewards_dev, uint8_t* dones_dev, void* stream);

/* Measurement hook (bench.py's roofline leg): three caller-owned hipEvent_t (as void*; NULL = none, all NULL = off) that every
 * following dynenv_step / dynenv_step_head / dynenv_step_masked records on ITS launch stream - before the step's dominant kernel (drv_step_kernel,
 * rc_step_kernel, drv_step_partial_kernel, rc_step_partial_kernel), right after it, and after the step's last kernel (the
 * deferred-observation / finalize launches of the Partial paths).  hipEventElapsedTime(begin, main_done) is that kernel's own
 * launch duration.  The events are overwritten by the next step: synchronise on ev_end before stepping again. */
int dynenv_set_step_events(dynenv_t* h, void* ev_begin, void* ev_main_done, void* ev_end);

/* Per-env object counts of the current episode: int32 [E, 2] = (n_obstacles, n_pedestrians) (Driving). */
int dynenv_counts(dynenv_t* h, int32_t* counts_dev, void* stream);

/* Episode accumulators: ep_r, ep_pos_r, ep_obs_r float64 [E, A]; goals int32 [E, 2]. Any pointer may be NULL. */
int dynenv_episode_stats(dynenv_t* h, double* ep_r_dev, double* ep_pos_r_dev, double* ep_obs_r_dev,
                         int32_t* goals_dev, void* stream);

/* Copy one environment's canonical state blob to / from HOST memory (synchronous; test + checkpoint path): the device is synchronised,
 * then ONE launch of the kernels behind dynenv_get_states / dynenv_set_states and one copy between host memory and a staging area of
 * the handle (device memory that is no part of a checkpoint).  dynenv_set_state of a blob that does not fit the handle (the list at
 * dynenv_set_states) returns DYNENV_ERR_ARG, writes nothing and - unlike the batched call, which has no caller to tell - raises no
 * error bit. */
size_t dynenv_state_size(const dynenv_t* h);
int dynenv_get_state(dynenv_t* h, int32_t env_idx, void* host_blob, size_t nbytes);
int dynenv_set_state(dynenv_t* h, int32_t env_idx, const void* host_blob, size_t nbytes);

/* The same for MANY environments in one launch, device memory on both sides: blobs_dev holds n canonical blobs dynenv_state_size(h)
 * bytes apart, 8-byte aligned (no more: the RoboCup blob is 2552 bytes); env_idx_dev int32 [n] names the environment of each blob,
 * NULL = environments 0..n-1.  Ordered on `stream`: no host synchronisation, no allocation, no host copy.
 *   dynenv_get_states  writes, per listed environment, exactly the bytes dynenv_get_state writes (pads and unused car / pedestrian /
 *                      obstacle / robot slots zeroed, RoboCup defenders as an ascending id list).  An index outside [0, E) leaves its
 *                      blob untouched.
 *   dynenv_set_states  leaves every device array of the handle in exactly the bytes dynenv_set_state produces for a valid blob (whole
 *                      field rows rewritten, contact cache and the environment's error word cleared).  A blob that does not fit -
 *                      Driving: n_cars != A, n_peds / n_obst outside 0..20; RoboCup: n_robots != R, an n_def[t] outside 0..10, a
 *                      listed defender id outside 0..9 - leaves its environment untouched and raises error bit 6 on it.
 *                      status_dev (may be NULL) int32 [n]: 0 written, 1 blob rejected, 2 index outside [0, E) (entry skipped).
 *                      The same index twice in one call is a caller error: that environment's state is unspecified then. */
int dynenv_get_states(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, void* blobs_dev, void* stream);
int dynenv_set_states(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, const void* blobs_dev, int32_t* status_dev, void* stream);

/* ---- exact save / restore of CHOSEN environments on the device (no reference equivalent; the reference has no state transfer at all).
 * The canonical blob above drops the contact cache, so an environment in contact that is set and replayed is not the run it was saved
 * from; dynenv_checkpoint_save is exact but goes through host memory, for the whole handle, and synchronises.  An EXACT BLOB is every
 * simulation-state row of one environment bit for bit - bodies, contact cache (pair / meta / hash tables, warm-start impulses), shortcut
 * state and call-to-call caches, joints' accumulated impulses and pending forces, episode accumulators and counter, elapsed time,
 * diagnostic counters, the error word - i.e. the environment's part of every checkpointed per-environment array; the scheduler's
 * scratch (timing only) is no part of it.  Since every random draw is keyed by (seed, global id, episode, purpose, entity, time) and
 * episode and time are in those rows, dynenv_set_exact + the same actions reproduces the run from dynenv_get_exact bit for bit.
 *   The blob: a 16-byte header (a 64-bit layout tag, then zeros), then the rows.  dynenv_exact_size(h) bytes, a multiple of 16 (0 for
 *   a NULL handle).  The format is opaque: valid for the same library build and the same configuration.  The tag is a hash of env_type,
 *   n_players, obs_type, flags and the shape of every per-environment array - NOT of num_envs, env_id_offset, seed or noise settings: a
 *   blob may go into another environment index and into another handle of the same configuration with another batch size (it then
 *   draws from that environment's own random streams).
 * blobs_dev holds n blobs dynenv_exact_size(h) apart, 16-byte aligned; env_idx_dev int32 [n] names the environment of each, NULL =
 * environments 0..n-1.  Both calls are ONE launch ordered on `stream` - no host synchronisation, no allocation, no host copy - and may
 * be captured into a hipGraph: pointers and n are frozen, indices and blob contents are read at replay (an index of -1 switches a slot
 * off).
 *   dynenv_get_exact  writes every byte of the blob of each listed environment; an index outside [0, E) leaves its blob untouched.
 *   dynenv_set_exact  a blob with this handle's tag: every per-environment row of the destination ends up with exactly the saved bytes
 *                     (error word, diagnostic counters and Driving Partial's deferred-observation word included); nothing else changes.
 *                     What stands behind a valid tag is trusted, as dynenv_checkpoint_load trusts its buffer.  Any other tag (a buffer
 *                     nobody wrote, a blob of another configuration): the environment is untouched and error bit 6 is raised on it.
 *                     status_dev (may be NULL) int32 [n]: 0 written, 1 blob rejected, 2 index outside [0, E) (entry skipped).
 *                     The same index twice in one call is a caller error: that environment's state is unspecified then.
 * Errors: NULL handle, n < 0, NULL blobs_dev with n > 0, blobs_dev not 16-byte aligned, more blobs than environments without an index
 * list -> DYNENV_ERR_ARG (before a device is looked for); n == 0 -> DYNENV_OK, nothing launched. */
size_t dynenv_exact_size(const dynenv_t* h);
int dynenv_get_exact(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, void* blobs_dev, void* stream);
int dynenv_set_exact(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, const void* blobs_dev, int32_t* status_dev, void* stream);

int dynenv_sync(dynenv_t* h, void* stream);

/* OR over all environments of the kernels' error flags (bit 0: contact cache or candidate list overflow - an environment had
 * more arbiters at once than its slot table holds (24 Driving, 16 RoboCup) or more than 128 candidate pairs in a substep - and a pair was
 * DROPPED: the reference has no such cap, so from that substep on the environment is not the reference's; sticky until the next reset /
 * set_state of it; the host mirror's step() raises on it; bit 1: an action
 * outside the action space was seen - the reference raises there, DrivingEnvironment.py:365-368 / RoboCupEnvironment.py:543-550;
 * here that agent's action is ignored for the step and the flag stays up until the next reset; bit 3: a Partial observation
 * list had more rows than its capacity in the layout and the rows beyond it were DROPPED - the reference's lists have no cap
 * (DrivingEnvironment.py:816-890); SURVEY Appendix E's worst case is above the Driving capacities (24 cars / 32 obstacles / 40
 * pedestrians / 16 lanes), astronomically unlikely, and no longer silent: the host mirror's step() raises on it; bit 2: Driving Partial, the list of environments left to the deferred
 * observation launch is full - it is cleared between steps by launches that alternate a parity; a guard that no supported use
 * reaches: a captured dynenv_step keeps that parity on the device); bit 4 (value 16): RoboCup, the CORES of two
 * capsules (feet, Robot.py:38-52) were exactly collinear or exactly touching.  Cores that CROSS - the two feet of one robot that
 * has been knocked about get there in play - take the normal Chipmunk's EPA gives (the minimum-translation axis of the two cores;
 * DESIGN.md 2b); in this measure-zero case even that normal's SIGN is a convention, and from that substep on the environment may
 * not be what pymunk would have computed.  A dynenv_set_state blob can put two feet on one line.  Sticky until the next reset /
 * set_state; the host mirror's step() raises on it; bit 5 (value 32):
 * RoboCup, a foot velocity or a joint impulse left the finite range during a solve (never seen): the joints' arithmetic drops
 * products that are zeros for finite operands only, so that substep is not the reference's - reported like bit 4.
 * bit 6 (value 64): a blob given to dynenv_set_states did not fit the handle's layout, or a blob given to dynenv_set_exact did not
 * carry the handle's layout tag, and was NOT written; sticky on that environment until the next reset or the next valid set_state /
 * set_states / set_exact of it (a valid exact blob brings its own error word, saved with the rest); the host mirror's step() raises on it.
 * Synchronises the device. */
#define DYNENV_ERRBIT_OVERFLOW 1      /* bit 0: a contact or a candidate pair was dropped */
#define DYNENV_ERRBIT_ACTION 2        /* bit 1: an action outside the action space */
#define DYNENV_ERRBIT_DEFER_LIST 4    /* bit 2: Driving Partial, the deferred-observation list was full */
#define DYNENV_ERRBIT_ROWS_DROPPED 8  /* bit 3: Partial observation rows beyond a list's capacity */
#define DYNENV_ERRBIT_DEGENERATE 16   /* bit 4: RoboCup, capsule cores collinear or touching */
#define DYNENV_ERRBIT_NONFINITE 32    /* bit 5: RoboCup, a non-finite velocity or impulse in a solve */
#define DYNENV_ERRBIT_BLOB 64         /* bit 6: a state blob that did not fit was not written */
int dynenv_error_flags(dynenv_t* h, int32_t* out);
/* The per-environment error words themselves (the bits above): flags_dev int32 [E], ordered on `stream`, no synchronisation - to
 * name the environment a sticky bit belongs to and repair only that one. */
int dynenv_error_flags_env(dynenv_t* h, int32_t* flags_dev, void* stream);

/* Diagnostics (Driving), summed over environments since the last reset: out16 = {substeps on the no-contact fast path,
 * on the quiescent shortcut, on the full contact path, sum of live contact-cache slots, contact-path substeps caused by
 * a changed candidate set / a moving body / a non-inert arbiter, substeps served by a steady replay, by the light mode,
 * contact-path substeps whose sweeps ran as split-lane general multi-level solves, the number of environments the next step
 * gives a SIMD of their own (-1: isolation off for this handle), isolation placeholders that gave up waiting (stays 0),
 * the handle's scheduling mode (0 none, 1 SIMD isolation, 2 slow environments first, 3 timing only: Partial observations), whether the block -> SIMD placement
 * isolation relies on validated for the next step (mode 1; it is re-checked on the device every launch and isolation holds
 * off while it does not validate), launches whose placement did not validate (since isolation was last started), the number
 * of times the host paused isolation - plain launches for 2048 steps - because more than half of the launches of a 64-step
 * window did not validate: a device shared with another handle or kernel}.
 * Synchronises the device. */
int dynenv_debug_counters(dynenv_t* h, int64_t* out16);
/* Diagnostics: where the regular blocks of the last Driving step ran - out[b] = XCC id << 16 | HW_ID bits (SE 15:13, SH 12,
 * CU 11:8, SIMD 5:4) of block b; recorded only by handles in scheduling mode 1 (it is what the self-validation of the SIMD
 * isolation reads).  Returns the number of words written (0: not recorded), < 0 on error.  Synchronises the device. */
int dynenv_debug_placement(dynenv_t* h, uint32_t* out, int32_t n);

/* ---- de-duplicated transport format for the multi-GPU all-gather.  Where every agent row of an (env, time) ends in the
 * same tail (Driving Full: obstacles, pedestrians, lane rows = 160 of 232 floats), the packed form holds the A prefixes
 * of `split` floats followed by the tail once: A*split + (D - split) floats instead of A*D.  n_env_time = E*T rows of
 * [A][D].  unpack(pack(x)) == x bit for bit when the tails are identical (they are written from one LDS copy). ---- */
int dynenv_obs_pack(const float* obs_dev, int64_t n_env_time, int32_t A, int32_t D, int32_t split, float* packed_dev, void* stream);
int dynenv_obs_unpack(const float* packed_dev, int64_t n_env_time, int32_t A, int32_t D, int32_t split, float* obs_dev, void* stream);
/* the gathered buffer of an all-gather: n_ranks packed blocks `src_stride_floats` apart -> obs_dev [n_ranks][n_env_time][A][D], one launch */
int dynenv_obs_unpack_ranks(const float* packed_dev, int64_t src_stride_floats, int32_t n_ranks, int64_t n_env_time, int32_t A,
                            int32_t D, int32_t split, float* obs_dev, void* stream);
/* Peer-compacted transport format of a Driving Full observation (reference: DrivingEnvironment.getFullState,
 * DrivingEnvironment.py:686-747).  Agent a's row is [self 9 | the other A-1 cars x 7 | tail]; the 7 floats of car c are
 * columns {0..5, 8} of c's own self block, so per (env, time) the A self blocks plus the tail once carry everything:
 * 9A + (D - 9 - 7(A-1)) floats instead of A*D.  unpack_peers_ranks expands n_ranks gathered blocks (src_stride_floats
 * apart) into the dense [n_ranks][n_env_time][A][D] tensor, bit for bit. */
int dynenv_obs_pack_peers(const float* obs_dev, int64_t n_env_time, int32_t A, int32_t D, float* packed_dev, void* stream);
int dynenv_obs_unpack_peers_ranks(const float* packed_dev, int64_t src_stride_floats, int32_t n_ranks, int64_t n_env_time,
                                  int32_t A, int32_t D, float* obs_dev, void* stream);

/* ---- exact checkpoint (the reference has none).  Unlike the canonical per-env blob of
 * dynenv_get_state (which drops the contact cache), a checkpoint is every device array of the handle bit for bit -
 * bodies, contact cache, shortcut state, episode counters, seed - so that load + the same actions reproduces the run
 * exactly from the middle of an episode.  Host buffers; the handle must have the configuration the checkpoint was taken
 * with (env type, sizes, observation/noise type, flags, env_id_offset).  The seed need not match: a load adopts the checkpoint's
 * seed - except on a handle of which a step or masked reset has been captured into a hipGraph (see dynenv_seed: a replay keeps the
 * captured seed), where a checkpoint taken under another seed returns DYNENV_ERR_UNSUPPORTED before anything is copied. ---- */
size_t dynenv_checkpoint_size(const dynenv_t* h);
int dynenv_checkpoint_save(dynenv_t* h, void* buf_host, size_t nbytes);
int dynenv_checkpoint_load(dynenv_t* h, const void* buf_host, size_t nbytes);

/* ---- ragged -> padded arranger.  Replaces InOutArranger.rearrange_inputs / rearrange_outputs of the
 * reference's input layer (DynEnv/models/models.py:219-250, :252-274) on the dense observation tensor this library
 * writes.  Pure functions of device buffers on the current HIP device (no handle).  A "group" is the list of object
 * types the reference passes as one element of obs[..., 0] / obs[..., 1], e.g. Driving movable = (cars, obstacles,
 * pedestrians).  P = E*A players, player index p = e*A + a (models.py:222-223).                                   ---- */
#define DYNENV_ARR_MAX_TYPES 4
#define DYNENV_ARR_COUNT_CONST 0 /* every (env, time, agent) row holds `count_value` objects of the type */
#define DYNENV_ARR_COUNT_ENV 1   /* count = count_env[env * count_stride + count_index]   (dynenv_counts() layout) */
#define DYNENV_ARR_COUNT_ROW 2   /* count = (int) obs_row[count_index]   (Driving Partial keeps list lengths in the row tail) */
/* In every mode the count used is clamp(count, 0, cap): a negative count is 0 objects, a count above the row capacity is
 * `cap` objects (the rows past cap do not exist).  COUNT_ROW converts the float with a C cast, i.e. truncates toward zero
 * (2.9 -> 2, -0.5 -> 0) before the clamp. */
typedef struct dynenv_arr_type {
  int32_t offset, feat, cap; /* block inside an observation row: float offset, features per object, row capacity */
  int32_t count_mode, count_value, count_index, count_stride, reserved;
} dynenv_arr_type_t;
typedef struct dynenv_arr_plan {
  int32_t n_types, n_time, n_players, max_count; /* max_count = max over (time, player) of the summed counts (:233) */
  int64_t total[DYNENV_ARR_MAX_TYPES];           /* N_i = number of objects of type i over all (time, player) */
} dynenv_arr_plan_t;

/* ints of scratch dynenv_arrange_plan needs for E*T*A rows and n_types types */
int64_t dynenv_arrange_scratch_ints(int32_t E, int32_t T, int32_t A, int32_t n_types);
/* Phase 1 (rearrange_inputs :226-236): counts [n_types][T][P], obj_counts [T][P], base [n_types][T][P] = exclusive prefix
 * sums in (time, player) order (where the objects of (t, p) start inside inputs[i]).  Synchronises the stream and fills
 * *plan_host (the reference's `.item()` on maxCount is the same host round trip). */
int dynenv_arrange_plan(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types,
                        int32_t n_types, const int32_t* count_env_dev, int32_t* counts_dev, int32_t* obj_counts_dev,
                        int32_t* base_dev, int32_t* scratch_dev, dynenv_arr_plan_t* plan_host, void* stream);
/* Phase 2 (rearrange_inputs :238-245 + the index arithmetic of rearrange_outputs :259-268): inputs_dev[i] float32
 * [N_i][feat_i] in (time, player, object) order; slot_dev[i] int32 [N_i] = destination row of each object in the padded
 * tensor [T][max_count][P][F] viewed as [T*max_count*P][F]; mask_dev uint8 [T][P][max_count], 1 = padding (createMask).
 * Any of the pointers may be NULL to skip that output. */
int dynenv_arrange_gather(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types,
                          int32_t n_types, const int32_t* counts_dev, const int32_t* base_dev, int32_t max_count,
                          float* const* inputs_dev, int32_t* const* slot_dev, uint8_t* mask_dev, void* stream);
/* Phase 3 (rearrange_outputs :257-268, catAndPad): padded[slot[n]][:] = emb[n][:] for the N embeddings of one type;
 * padded_dev float32 [T][max_count][P][F] must have been zeroed by the caller (the padding). */
int dynenv_arrange_scatter(const float* emb_dev, const int32_t* slot_dev, int64_t N, int32_t F, float* padded_dev, void* stream);
/* Phase 3, fused (preferred): writes EVERY element of padded_dev float32 [T][max_count][P][F] in one pass - the
 * embedding of the object that owns the slot, or zero - so no pre-zeroing and no second pass per type.  emb_dev[i] is
 * float32 [N_i][F] (NULL for a type without objects); F must be a multiple of 4 and the buffers 16-byte aligned. */
int dynenv_arrange_pad(const float* const* emb_dev, const int32_t* counts_dev, const int32_t* base_dev, int32_t n_types,
                       int32_t T, int32_t P, int32_t max_count, int32_t F, float* padded_dev, void* stream);
/* Backward of phase 3.  The reference's rearrange_outputs (models.py:250-274) is out[range] -> torch.cat -> F.pad ->
 * torch.stack, so autograd's derivative of catAndPad (:147-166) hands every embedding row the upstream gradient's row at
 * that object's slot: nothing is summed, no row is used twice, padding slots have no gradient.
 * Fused (preferred), the mirror of dynenv_arrange_pad: grad_emb_dev[i][base[i][t][p] + k][:] = grad_padded_dev[t][j][p][:]
 * for k < counts[i][t][p], j running over the player's slots in type order.  grad_padded_dev is float32
 * [T][max_count][P][F], contiguous; grad_emb_dev[i] is float32 [N_i][F], every row of which is written exactly once (no
 * pre-zeroing), or NULL: no gradient wanted for type i, its slots are stepped over and not read.  F must be a multiple of
 * 4 and all buffers 16-byte aligned.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL grad_padded_dev, counts_dev, base_dev or
 * grad_emb_dev; n_types outside 1..DYNENV_ARR_MAX_TYPES; T < 1, P < 1, max_count < 0; F < 4 or F & 3; P * F / 4 >= 2^31 or
 * T > 65535 (the launch limits of dynenv_arrange_pad).  max_count == 0 launches nothing and returns DYNENV_OK. */
int dynenv_arrange_pad_backward(const float* grad_padded_dev, const int32_t* counts_dev, const int32_t* base_dev,
                                int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F,
                                float* const* grad_emb_dev, void* stream);
/* Backward of dynenv_arrange_scatter, one type per call, any F and any alignment:
 * grad_emb_dev[n][:] = grad_padded_dev[slot_dev[n]][:] for the N embeddings of the type (slot_dev as dynenv_arrange_gather
 * wrote it).  Errors, DYNENV_ERR_ARG, before a device is looked for: N < 0, F < 1, a NULL pointer with N > 0, N * F beyond
 * one launch (2^31 blocks of 256).  N == 0 launches nothing and returns DYNENV_OK. */
int dynenv_arrange_scatter_backward(const float* grad_padded_dev, const int32_t* slot_dev, int64_t N, int32_t F,
                                    float* grad_emb_dev, void* stream);

/* ---- the arranger at FIXED capacities: the same layout with every shape chosen by the caller, so that nothing is copied to the
 * host and nothing waited for.  All three calls are launches only, ordered on `stream`: no synchronisation, no allocation, no
 * host copy.  They may be captured into a hipGraph: pointers and sizes (rows, max_count, the types) are frozen into the graph,
 * buffer contents are read at replay.  The caller chooses rows[i] in 0..types[i].cap, the rows of type i kept per (time, player)
 * (a HOST array [n_types]), and max_count = M >= 0, the slots of the padded tensor.  With c_i(t,p) = clamp(count, 0, cap_i), the
 * count of the calls above, the KEPT count is k_i(t,p) = min(c_i, rows[i], M - sum_{i'<i} k_i'): earlier types win.  Rows beyond
 * a capacity are dropped and reported, never silently (as error bit 3): sum_{t,p}(c_i - k_i) is ADDED to dropped_dev[i].
 * tp = t*P + p.  Whenever nothing is dropped (rows[i] >= c_i everywhere, M >= the batch's maxCount) the kept rows, the leading
 * maxCount slots of the padded tensor and of the mask, and the kept rows of the gradients are bit for bit those of
 * dynenv_arrange_plan / _gather / _pad / _pad_backward; behind maxCount the padded tensor is zero and the mask 1.
 *
 * dynenv_arrange_fixed_gather (rearrange_inputs, models.py:219-250; the mask: createMask :166-180), at most two launches:
 *   counts_dev int32 [n_types][T][P] = k_i;  obj_counts_dev int32 [T][P] = sum_i k_i;
 *   inputs_dev[i] float32 [T][P][rows[i]][feat_i] (the array or an entry may be NULL): row r < k_i holds the object's features,
 *     row r >= k_i holds +0.0 exactly - the unused capacity of an observation row is never read;
 *   mask_dev uint8 [T][P][M] (may be NULL): 1 where j >= obj_counts[t][p];
 *   dropped_dev int32 [n_types] (may be NULL): sticky, added to with atomics; the caller zeroes it.
 *   max_count == 0 still writes the counts (all zero), dropped and the zeroed inputs.
 *   Errors, DYNENV_ERR_ARG, before a device is looked for: a NULL obs_dev, types, rows, counts_dev or obj_counts_dev; n_types
 *   outside 1..DYNENV_ARR_MAX_TYPES; a type outside the observation row; rows[i] outside 0..cap_i; max_count < 0; count_env_dev
 *   NULL with a DYNENV_ARR_COUNT_ENV type; E, T, A or D < 1; more than 2^31 blocks of 256 threads in a launch. */
int dynenv_arrange_fixed_gather(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D,
                                const dynenv_arr_type_t* types, int32_t n_types, const int32_t* count_env_dev,
                                const int32_t* rows /* host [n_types] */, int32_t max_count, int32_t* counts_dev,
                                int32_t* obj_counts_dev, float* const* inputs_dev, uint8_t* mask_dev, int32_t* dropped_dev,
                                void* stream);
/* dynenv_arrange_fixed_pad (rearrange_outputs, models.py:252-274, catAndPad :147-180), one launch: padded_dev float32
 * [T][M][P][F]; slot j = sum_{i'<i} k_i' + r with r < k_i gets emb_dev[i][tp*rows[i] + r][:], emb_dev[i] being float32
 * [T*P*rows[i]][F]; a NULL emb_dev[i] writes zeros in its slots; slots j >= obj_counts get +0.0.  EVERY element is written: no
 * pre-zeroing.  counts_dev is what dynenv_arrange_fixed_gather wrote (k_i); it is clamped to 0..rows[i] and to the slots left,
 * so reads and writes stay in bounds whatever it holds.
 * Errors, DYNENV_ERR_ARG, before a device is looked for: a NULL emb_dev, counts_dev, rows or padded_dev; n_types outside
 * 1..DYNENV_ARR_MAX_TYPES; rows[i] < 0; T < 1, P < 1, max_count < 0; F < 4 or F & 3; padded_dev or an emb_dev[i] not 16-byte
 * aligned; T > 65535, P * F / 4 >= 2^31 or T * P > 2^30.  max_count == 0 launches nothing and returns DYNENV_OK. */
int dynenv_arrange_fixed_pad(const float* const* emb_dev, const int32_t* counts_dev, const int32_t* rows, int32_t n_types,
                             int32_t T, int32_t P, int32_t max_count, int32_t F, float* padded_dev, void* stream);
/* Backward of dynenv_arrange_fixed_pad (autograd's derivative of catAndPad, models.py:147-180, as dynenv_arrange_pad_backward),
 * one launch: grad_emb_dev[i][tp*rows[i] + r][:] = grad_padded_dev[t][j][p][:] for r < k_i and +0.0 for r >= k_i - the
 * embedding block ran on the zero rows too and their output was discarded, so their gradient is zero.  Every row of every
 * non-NULL grad_emb_dev[i] (float32 [T*P*rows[i]][F]) is written exactly once; a NULL entry (no gradient wanted) is stepped
 * over unread; padding slots of grad_padded_dev are never read.  Errors and max_count == 0 as dynenv_arrange_fixed_pad (with
 * max_count == 0 nothing is written: every gradient row is zero and the caller's to fill). */
int dynenv_arrange_fixed_pad_backward(const float* grad_padded_dev, const int32_t* counts_dev, const int32_t* rows,
                                      int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F,
                                      float* const* grad_emb_dev, void* stream);

/* ---- the padded tensor in a 16-BIT type.  A network under torch.autocast reads the padded tensor in bf16 (or fp16): the four calls
 * below are dynenv_arrange_pad / _pad_backward / _fixed_pad / _fixed_pad_backward with an element type for the per-type buffers
 * (emb_dtype) and one for the padded tensor or its gradient (padded_dtype).  Layout, slots, counts, NULL entries and clamping are
 * those of the call each mirrors, element for element; only the element types differ.  Supported pairs (emb_dtype, padded_dtype):
 *   (F32, BF16), (F32, F16)    the forward converts, the backward widens to float32 rows;
 *   (BF16, BF16), (F16, F16)   a bit copy both ways;
 *   (F32, F32)                 forwarded to the call it mirrors;
 *   anything else              DYNENV_ERR_UNSUPPORTED.
 * Conversion contract, the same on every path: float32 -> 16 bit is IEEE round to nearest, ties to even - overflow to infinity, fp16
 * subnormal results, underflow to a signed zero, +-0 and +-inf unchanged - so it is bit for bit what torch's CPU `.to(dtype)` gives for
 * every non-NaN input; a NaN stays a NaN, its payload is not part of the contract.  16 bit -> float32 is exact for every bit pattern,
 * fp16 subnormals included.  Padding is +0.0 (all-zero bits).
 * With a 16-bit padded tensor F must be a multiple of 8 (a 16-byte unit of the padded tensor is 8 elements) and EVERY buffer 16-byte
 * aligned; there is no per-row fallback.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL padded / grad_padded, counts_dev, base_dev / rows or
 * per-type pointer array; n_types outside 1..DYNENV_ARR_MAX_TYPES; T < 1, P < 1, max_count < 0; rows[i] < 0 (fixed mode); a dtype
 * outside 0..2; F < 8 or F & 7 with a 16-bit padded tensor (F < 4 or F & 3 with a float32 one); T > 65535, P * F / 8 (or / 4) >= 2^31,
 * and in the fixed mode T * P > 2^30 (the launch limits); the padded tensor or a per-type buffer not 16-byte aligned.  Then an
 * unsupported pair: DYNENV_ERR_UNSUPPORTED, also before the device.  max_count == 0 launches nothing and returns DYNENV_OK. */
#define DYNENV_ARR_F32 0
#define DYNENV_ARR_BF16 1
#define DYNENV_ARR_F16 2
/* dynenv_arrange_pad in these types (rearrange_outputs, models.py:252-274, catAndPad :147-180), one launch: padded_dev
 * [T][max_count][P][F] of padded_dtype, EVERY element written - the embedding of the object that owns the slot, converted by the
 * contract above, or +0.0; emb_dev[i] is [N_i][F] of emb_dtype (NULL for a type without objects: zeros in its slots).  Errors: the
 * list above (DYNENV_ERR_ARG, then DYNENV_ERR_UNSUPPORTED, before a device is looked for). */
int dynenv_arrange_pad_as(const void* const* emb_dev, int32_t emb_dtype, const int32_t* counts_dev, const int32_t* base_dev,
                          int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* padded_dev,
                          int32_t padded_dtype, void* stream);
/* dynenv_arrange_pad_backward in these types (autograd's derivative of catAndPad, models.py:147-180), one launch:
 * grad_emb_dev[i][base[i][t][p] + k][:] = grad_padded_dev[t][j][p][:], widened exactly to float32 or bit-copied; grad_padded_dev is
 * [T][max_count][P][F] of padded_dtype, grad_emb_dev[i] [N_i][F] of emb_dtype.  Every row of every non-NULL grad_emb_dev[i] is written
 * exactly once; a NULL entry is stepped over; padding slots are never read.  Errors: the list above (DYNENV_ERR_ARG, then
 * DYNENV_ERR_UNSUPPORTED, before a device is looked for). */
int dynenv_arrange_pad_backward_as(const void* grad_padded_dev, int32_t padded_dtype, const int32_t* counts_dev,
                                   const int32_t* base_dev, int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F,
                                   void* const* grad_emb_dev, int32_t emb_dtype, void* stream);
/* dynenv_arrange_fixed_pad in these types (rearrange_outputs, models.py:252-274, catAndPad :147-180), one launch, capturable:
 * padded_dev [T][M][P][F] of padded_dtype, every element written; emb_dev[i] is [T*P*rows[i]][F] of emb_dtype, a NULL entry writes
 * zeros in its slots; the conversion is the contract above.  Errors: the list above (DYNENV_ERR_ARG, then DYNENV_ERR_UNSUPPORTED,
 * before a device is looked for); every buffer 16-byte aligned. */
int dynenv_arrange_fixed_pad_as(const void* const* emb_dev, int32_t emb_dtype, const int32_t* counts_dev, const int32_t* rows,
                                int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* padded_dev,
                                int32_t padded_dtype, void* stream);
/* dynenv_arrange_fixed_pad_backward in these types (models.py:147-180), one launch, capturable: grad_emb_dev[i][tp*rows[i] + r][:] =
 * grad_padded_dev[t][j][p][:] for r < k_i, widened exactly or bit-copied, and +0.0 in the rows behind the kept ones.  Every row of
 * every non-NULL grad_emb_dev[i] ([T*P*rows[i]][F] of emb_dtype) is written exactly once; a NULL entry is stepped over; padding
 * slots of grad_padded_dev are never read.  Errors: the list above (DYNENV_ERR_ARG, then DYNENV_ERR_UNSUPPORTED, before a device is
 * looked for). */
int dynenv_arrange_fixed_pad_backward_as(const void* grad_padded_dev, int32_t padded_dtype, const int32_t* counts_dev,
                                         const int32_t* rows, int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F,
                                         void* const* grad_emb_dev, int32_t emb_dtype, void* stream);

/* ---- embed and pad in ONE pass, where no gradient is wanted: the reference's whole InputLayer (models.py:278-307) - rearrange_inputs,
 * one EmbedBlock per object type (models.py:99-124), rearrange_outputs - from the observation row straight to the padded tensor.
 * Neither inputs[i], nor an activation, nor the embeddings exist in memory.  One EmbedBlock, float32, in torch's layouts:
 *   h = LayerNorm(LeakyReLU(w1 x)),  y = LayerNorm(LeakyReLU(w2 h)):  Linear(feat -> F/2, no bias), LeakyReLU(slope), LayerNorm(F/2),
 *   Linear(F/2 -> F, no bias), LeakyReLU(slope), LayerNorm(F);  LayerNorm as torch defines it: biased variance,
 *   (x - mean) / sqrt(var + eps) * w + b. */
typedef struct dynenv_embed_block {
  const float *w1;            /* [F/2][feat]  Layer1.weight */
  const float *ln1_w, *ln1_b; /* [F/2]        bn1 */
  const float *w2;            /* [F][F/2]     Layer2.weight */
  const float *ln2_w, *ln2_b; /* [F]          bn2 */
} dynenv_embed_block_t;
/* dynenv_arrange_embed_pad, one launch, capturable (launches only: nothing is synchronised or allocated; pointers and sizes are frozen
 * by a capture, contents are read at replay): padded_dev [T][max_count][P][F] of padded_dtype (DYNENV_ARR_F32 / _BF16 / _F16), P = E*A,
 * p = e*A + a.  Slot j = sum_{i'<i} k_i' + r, r < k_i, holds block_i(obs[e][t][a][offset_i + r*feat_i .. + feat_i]); every slot behind
 * the player's last object holds +0.0; EVERY element is written exactly once - no pre-zeroing, no second pass.  counts_dev int32
 * [n_types][T][P] is what dynenv_arrange_plan or dynenv_arrange_fixed_gather wrote; the kernel clamps each count to 0..cap_i and to the
 * slots left (k_i), so reads and writes stay in bounds whatever the buffer holds.  Neither `base` nor `rows` is needed - the call reads
 * the observation row itself - so it serves the default and the fixed-shape mode.  blocks is a HOST array of n_types entries of device
 * pointers; an entry has all six pointers or none: a type all of whose counts are zero may leave them NULL (a type with objects and
 * NULL weights gets +0.0 in its slots, as a NULL embedding does in dynenv_arrange_pad_as).
 * Arithmetic: float32 throughout, every sum in one fixed order: an object's result depends on its features and its type alone - not
 * on its slot, its lane or the batch around it - and the same call twice gives the same bits.  A 16-bit padded tensor is the float32
 * result converted at the store by the contract above (round to nearest, ties to even).
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL obs_dev, types, counts_dev, blocks or padded_dev; E, T, A or
 * D < 1; n_types outside 1..DYNENV_ARR_MAX_TYPES; a type outside the observation row; a dtype outside 0..2; max_count < 0; padded_dev
 * not 16-byte aligned; T * max_count * P >= 2^31, max_count >= 2^23 or E * T * A > 2^30 (the launch limits); a block with some but not all of its pointers.
 * Then what the kernels do not take: F other than 64 or 128, or a feat_i above 16: DYNENV_ERR_UNSUPPORTED, also before the device.
 * max_count == 0 launches nothing and returns DYNENV_OK. */
int dynenv_arrange_embed_pad(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types,
                             int32_t n_types, const int32_t* counts_dev, int32_t max_count, const dynenv_embed_block_t* blocks,
                             int32_t F, float slope, float eps, void* padded_dev, int32_t padded_dtype, void* stream);

/* ---- attention over the padded tensor in ONE launch, where no gradient is wanted: the reference's RecurrentTemporalAttention
 * (models.py:311-386), from the 16-bit padded tensor and the object counts to the pooled feature of every player.  Neither q, k, v,
 * the probabilities nor an attention output exist in memory.  One nn.MultiheadAttention(F, 1, add_bias_kv=True), in torch's layouts:
 * the four matrices and the two bias rows in the padded tensor's 16-bit type (the operands of the matrix units), the two bias vectors
 * float32. */
typedef struct dynenv_mha {
  const void *in_w;            /* [3F][F]  in_proj_weight: Wq, Wk, Wv     (padded_dtype) */
  const void *out_w;           /* [F][F]   out_proj.weight                (padded_dtype) */
  const void *bias_k, *bias_v; /* [F]      bias_k, bias_v                 (padded_dtype) */
  const float *in_b;           /* [3F]     in_proj_bias: bq, bk, bv */
  const float *out_b;          /* [F]      out_proj.bias */
} dynenv_mha_t;
/* dynenv_attend_pool, one launch, capturable (a launch and nothing else: nothing is synchronised, allocated or copied; pointers and
 * sizes are frozen by a capture, contents are read at replay): out_dev float32 [P][F], EVERY element written exactly once.
 * padded_dev is [T][M][P][F] of padded_dtype (DYNENV_ARR_BF16 / _F16), obj_counts_dev int32 [T][P] (what dynenv_arrange_plan or
 * dynenv_arrange_fixed_gather wrote); obj_att and temp_att are HOST structs of device pointers, ln_w_dev / ln_b_dev [F] and ln_eps the
 * LayerNorm `bn`, conf_w_dev [F] and conf_b_dev [1] the Linear of `confLayer`, all float32 on the device.  For player p, with c_t its
 * count at time t clamped to 0..M, n = max_t c_t and X_t its M slots at time t, every slot at or behind c_t taken as +0.0 WITHOUT
 * being read (the masks of the arranger are prefixes: True from the count on):
 *   mha(w; Qin, KVin, k):  q = Qin Wq^T + bq;  K = KVin[:k] Wk^T + bk with the row bias_k appended, V likewise with bias_v;
 *                          softmax(q K^T / sqrt(F)) over the k + 1 keys (the bias key is never masked: a row of probabilities always
 *                          exists);  the result is (probs V) Wo^T + bo
 *   att_t = mha(obj_att; X_t[:n], X_t, c_t) for every t - the query rows between c_t and n are zero rows, q = bq, and they count;
 *   fin = att_0, k = c_0;  for t = 1..T-1: fin = LayerNorm(mha(temp_att; att_t, fin, k)), then k = max(k, c_t) (models.py:362-363:
 *   the temporal keys take the mask from before the update);
 *   out[p] = sum_{r < n} sigmoid(fin_r . conf_w + conf_b) fin_r / n, and +0.0 where n == 0.  Rows at or behind n are never computed.
 * M == 0 writes +0.0 everywhere and returns DYNENV_OK (the reference returns the sum over an empty axis, models.py:376-377);
 * padded_dev may then be NULL.
 * Arithmetic: every matrix product takes 16-bit operands (padded_dtype) on the matrix units and accumulates in float32; biases,
 * softmax, LayerNorm, the sigmoid and the pooled mean are float32 - what torch.autocast does to the reference's layer, with one
 * rounding fewer where a product feeds the next from registers.  Every sum has one fixed order: a player's result depends on its own
 * slots and counts alone - not on p, on M or on the batch - and the same call twice gives the same bits.  Inputs that are not finite
 * are outside the contract.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL obj_counts_dev, obj_att, temp_att, ln_w_dev, ln_b_dev,
 * conf_w_dev, conf_b_dev or out_dev, a NULL padded_dev with M > 0, an attention with fewer than its six pointers; T, P or F < 1,
 * M < 0; a dtype outside 0..2; padded_dev, out_dev or a weight, LayerNorm or conf_w buffer not 16-byte aligned (bias_k, bias_v: 8-byte);
 * T * P > 2^30 (the launch limit).  Then what the kernel does not take: DYNENV_ARR_F32, an F other than 64 or 128, M > 128:
 * DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_attend_pool(const void* padded_dev, int32_t padded_dtype, const int32_t* obj_counts_dev, int32_t T, int32_t M, int32_t P,
                       int32_t F, const dynenv_mha_t* obj_att, const dynenv_mha_t* temp_att, const float* ln_w_dev,
                       const float* ln_b_dev, float ln_eps, const float* conf_w_dev, const float* conf_b_dev, float* out_dev,
                       void* stream);

/* ---- the recurrent head in ONE launch, where no gradient is wanted: the back half of the reference's DynEnvFeatureExtractor.forward
 * (models.py:584-594, 610-616) - TransformNet = Sequential(Linear(F + X, F), LeakyReLU, LayerNorm(F)), the nn.LSTMCell(F, F) of
 * LSTMLayer (models.py:16-95) on its persistent h and c, and the closing LayerNorm `bn` - with a per-environment reset of the state
 * folded in.  The [P][4F] gate pre-activations never exist in memory.  A HOST struct of device pointers, in torch's layouts: the
 * three matrices in the 16-bit type w_dtype (the operands of the matrix units), everything else float32. */
typedef struct dynenv_rhead {
  const void  *tr_w;                        /* [F][KP] TransformNet.0.weight in the 16-bit type, KP = F + X rounded up to a multiple of 32, columns from F + X on +0; unused when X == 0 */
  const float *tr_b, *tr_ln_w, *tr_ln_b;    /* [F] TransformNet.0.bias, TransformNet.2.weight / .bias; unused when X == 0 */
  const void  *w_ih, *w_hh;                 /* [4F][F] LSTM.cell.weight_ih / weight_hh, torch's gate order i, f, g, o (16-bit type) */
  const float *b_ih, *b_hh;                 /* [4F] */
  const float *ln_w, *ln_b;                 /* [F] the closing bn */
} dynenv_rhead_t;
/* dynenv_recurrent_head, one launch, capturable (a launch and nothing else: nothing is synchronised, allocated or copied; pointers
 * and sizes are frozen by a capture, contents are read at replay).  P = E * A rows; row p belongs to environment p / A (the
 * arranger's player order, and that of the reference's commented-out reset, models.py:45).  feat_dev [P][F] float32 (what
 * dynenv_attend_pool wrote); ext_dev [P][X] float32, the reference's `position`, NULL exactly when X == 0; h_dev and c_dev [P][F]
 * float32, read and written IN PLACE; out_dev [P][F] float32.  reset_env_dev is NULL or uint8 [E] - the dones_dev of a step is a
 * valid mask, as for dynenv_reset_masked.  Per row, all non-matrix arithmetic in float32:
 *   x = feat when X == 0 (the reference skips TransformNet when position is None, models.py:611-612; w->tr_* are then unused and may
 *       be NULL), else x = LayerNorm(leaky(cat(feat, ext) W_tr^T + b_tr; slope); tr_ln, tr_eps);
 *   where reset_env_dev != NULL and reset_env_dev[p / A] != 0, h and c are taken as +0.0 WITHOUT being read (they may hold anything,
 *       NaN included); otherwise they are read;
 *   g = x W_ih^T + b_ih + h W_hh^T + b_hh;  c' = sigmoid(g_f) c + sigmoid(g_i) tanh(g_g);  h' = sigmoid(g_o) tanh(c');
 *   out = LayerNorm(h'; ln, ln_eps).
 * h', c' and out are each written exactly once, every element of the P rows; a row's h and c are read completely before any byte of
 * that row is written.
 * Arithmetic: the three matrix products take 16-bit operands of w_dtype (DYNENV_ARR_BF16 / _F16) on the matrix units and accumulate
 * in float32; cat(feat, ext), x and h are rounded to w_dtype only as operands: the state in memory stays float32, and
 * c is never rounded.  Every sum has one fixed order: a row's result depends on that row, its environment's mask byte and the
 * weights alone - not on p, on P or on the other rows - and the same call twice gives the same bits.  Inputs that are not finite
 * are outside the contract, except the never-read state of a reset environment.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL feat_dev, w, h_dev, c_dev, out_dev, or one of w's
 * pointers of the cell and the closing LayerNorm (with X > 0: of the transform too); ext_dev NULL with X > 0 or non-NULL with
 * X == 0; E, A or F < 1; X < 0; a dtype outside 0..2; feat_dev, h_dev, c_dev, out_dev or a weight buffer not 16-byte aligned;
 * E * A > 2^30 (the launch limit).  Then what the kernel does not take: DYNENV_ARR_F32, an F other than 64 or 128, X > 32:
 * DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_recurrent_head(const float* feat_dev, const float* ext_dev, int32_t E, int32_t A, int32_t F, int32_t X, int32_t w_dtype,
                          const dynenv_rhead_t* w, float slope, float tr_eps, float ln_eps, const uint8_t* reset_env_dev,
                          float* h_dev, float* c_dev, float* out_dev, void* stream);

/* ---- the policy head in ONE launch, where no gradient is wanted: the reference's ActorLayer and CriticLayer
 * (DynEnv/models/actor_critic.py:161-242) on cat(features[0:2], dim=1) (actor_critic.py:88), the softmax and the draw of
 * _calc_log_probs for every discrete action group (actor_critic.py:125-140, the rollout of DynEnv/models/train.py:251-266), and
 * transformActions (DynEnv/utils/utils.py:20-39) of the drawn actions.  Neither the concatenated feature nor the logits exist in
 * memory.  A HOST struct of device pointers, in torch's layouts: the two matrices in the 16-bit type w_dtype (the operands of the
 * matrix units), everything else float32. */
#define DYNENV_POLICY_ROWS 32         /* the rows of the actor's matrix: N + C of them are used */
#define DYNENV_POLICY_MAX_GROUPS 8    /* G: the discrete action groups */
#define DYNENV_POLICY_MAX_CONT 4      /* C: the outputs of a Box block */
#define DYNENV_POLICY_RNG_PURPOSE 16u /* counter word 3 of the draw is this + g / 4; the step kernels' purposes (dynenv_math.h) are 1..9 */
typedef struct dynenv_policy {
  const void  *actor_w;                                /* [32][K] every actor.blocks.*.Layer*.weight in the order of ActorLayer.forward's flattened list: the N = sum n_g logits of the G groups, then the C outputs of the Box block; rows from N + C on +0 (16-bit type) */
  const float *actor_b;                                /* [32] the biases in the same order, +0 from N + C on */
  const float *cont_scale, *cont_mean;                 /* [C] ActorBlock.scale / .means; unused when C == 0 */
  const void  *critic_w1;                              /* [K/2][K] critic.blocks.Layer1.weight (16-bit type) */
  const float *critic_b1, *critic_ln_w, *critic_ln_b;  /* [K/2] Layer1.bias, bn.weight / .bias */
  const float *critic_w2, *critic_b2;                  /* [K/2] Layer2.weight, [1] Layer2.bias */
} dynenv_policy_t;
/* dynenv_policy_head, one launch, capturable (a launch and nothing else: nothing is synchronised, allocated or copied; pointers
 * and sizes are frozen by a capture, contents are read at replay).  P = E * A rows; row p belongs to environment p / A.  feat0_dev
 * [P][F] float32 and feat1_dev NULL or [P][F] float32: the input of a row is cat(feat0, feat1) of width K = F or 2F.  nvec is a
 * HOST array of the G group sizes n_g, N = sum n_g; C the width of the Box block; action_cols = AD the width of an action row, G <=
 * AD <= 8.  Per row p, all non-matrix arithmetic in float32 (actor_critic.py:204-213, 230-242):
 *   l = cat(feat0, feat1) W_actor^T + b;  probs_g = softmax(l_g) for every group;  cont = (sigmoid(l) - 0.5) * scale + mean for the
 *       Box block's outputs;
 *   value = LayerNorm(leaky(cat(feat0, feat1) W1^T + b1; slope); bn, ln_eps) . w2 + b2;
 *   the draw: w = dm_philox(lo32(seed), hi32(seed), lo32(row_base + p), lo32(draw), hi32(draw), DYNENV_POLICY_RNG_PURPOSE + g / 4)
 *       (include/dynenv_math.h: Philox4x32-10, the first two words the key), draw = draw_dev[0], or 0 where draw_dev is NULL (const
 *       uint64 [1] on the device: read at replay); the word of group g is w.v[g % 4] and u = (float)(word >> 8) * 2^-24, which is exact;
 *   the sample, in float32: c_j = c_{j-1} + probs_g[j] summed left to right, t = u * c_{n-1} (one rounding), action_g = the number
 *       of j in 0..n_g-2 with c_j <= t: an action of probability 0 is never drawn and the result is always inside the group;
 *   logp_g = log(clamp(probs_g[action_g], eps32, 1 - eps32)), eps32 = 2^-23, what Categorical(probs).log_prob computes - evaluated in
 *       double and rounded once, so it is the float32 nearest to the logarithm and a host reproduces it bit for bit;
 *   next_ext = transformActions(actions, discrete_turn) as float32 - the reference's function as its in-place assignments run, not a
 *       tidied one: with AD == 4 column 0 maps 0, 1, 2 -> 0, 3 -> 1, 4 -> -1, column 1 maps 2 -> -1, column 2 is the `sides` of column
 *       0 and maps BOTH 1 and 2 to -1 (2 -> 1, then every 1 -> -1) and the rest to 0, column 3 is lowered by 3 where discrete_turn !=
 *       0; with any other AD columns 0 and 1 are lowered by 1.
 * Outputs, EVERY element of each written exactly once: actions_dev int32 [P][AD] - [E][A][AD], what dynenv_step reads - with columns
 * G..AD-1 written 0 (RoboCup with allowHeadTurn: [5, 3, 3] and one Box output, AD = 4; dynenv_step_head ignores column 3); cont_dev
 * double [P][C], NULL exactly when C == 0 (with C == 1 the head_dev of dynenv_step_head); probs_dev float32 [P][N]; logp_dev float32
 * [P][G]; value_dev float32 [P]; next_ext_dev NULL or float32 [P][AD].
 * Arithmetic: the two matrix products take 16-bit operands of w_dtype (DYNENV_ARR_BF16 / _F16) on the matrix units and accumulate in
 * float32; biases, softmax, sigmoid, LayerNorm and the cumulative sums are float32.  Every sum has one fixed order: a row's result
 * depends on that row, the weights and (seed, draw, row_base + p) alone - not on p's place in the launch, on P or on the other rows
 * (shards of a batch pass their first row as row_base) - and the same call twice gives the same bits.  Inputs that are not finite
 * are outside the contract.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL feat0_dev, w, nvec, actions_dev, probs_dev, logp_dev or
 * value_dev, or one of w's eight pointers of the actor and the critic (with C > 0: cont_scale and cont_mean too); cont_dev NULL with
 * C > 0 or non-NULL with C == 0; E, A or F < 1; G outside 1..8, an n_g outside 1..16, C outside 0..4, N + C > 32, AD outside G..8; a
 * dtype outside 0..2; feat0_dev, feat1_dev, an output or a weight buffer not 16-byte aligned (critic_b2, cont_scale, cont_mean:
 * 4-byte; draw_dev: 8-byte); E * A > 2^30 (the launch limit).  Then what the kernel does not take: DYNENV_ARR_F32, an F other than
 * 64 or 128: DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_policy_head(const float* feat0_dev, const float* feat1_dev, int32_t E, int32_t A, int32_t F, int32_t w_dtype,
                       const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t C, int32_t action_cols, uint64_t seed,
                       const uint64_t* draw_dev, uint64_t row_base, float slope, float ln_eps, int32_t discrete_turn,
                       int32_t* actions_dev, double* cont_dev, float* probs_dev, float* logp_dev, float* value_dev,
                       float* next_ext_dev, void* stream);

/* ---- the rollout storage behind the policy head: the reference's RolloutStorage (DynEnv/models/storage.py) on the device.  The
 * buffers are those of reset_buffers (storage.py:76-111), all float32 but `finished`, P = E * A players, K = F or 2 F:
 *   rewards [T][P], finished uint8 [T][P] (agentFinished: a torch.bool tensor's storage), features [T+1][P][K], actions [T][AD][P],
 *   log_probs and log_probs_old [T][G][P], values [T][P], dones [T][E], and - not the reference's, which keeps a Python list - probs
 *   [T][P][N]. */
#define DYNENV_RETURNS_REFERENCE 0 /* _discount_rewards as it runs (storage.py:168-209): dones are NOT looked at */
#define DYNENV_RETURNS_DONES 1     /* the chain is cut where an episode ended */
#define DYNENV_RETURNS_GAE 2       /* generalised advantage estimation, the reference's "todo: add GAE" (storage.py:203) */
/* dynenv_rollout_insert, one launch, capturable (a launch and nothing else: nothing is synchronised, allocated or copied; pointers
 * and sizes are frozen by a capture, contents are read at replay): RolloutStorage.insert (storage.py:134-166, called at
 * DynEnv/models/train.py:277) at row t = cursor_dev[0], an int32 [1] on the device that is read at replay.  The kernel does not
 * advance the cursor.  Inputs -> row t of their buffer:
 *   rewards_in_dev  double [E][A], the step's       -> rewards[t][p]        rounded once to nearest (storage.py:158)
 *   finished_in_dev uint8 [P], 0 / nonzero          -> finished[t][p]       0 or 1 (storage.py:159)
 *   feat0_dev, feat1_dev float32 [P][F]             -> features[t][p][0:K]  side by side, K = F without feat1_dev, else 2 F: the
 *                                                                           reference's cat is never materialised (storage.py:160)
 *   actions_in_dev  int32 [P][AD], the policy's     -> actions[t][k][p]     transposed, as float32: torch.stack(action, dim=0) (storage.py:161)
 *   logp_in_dev     float32 [P][G]                  -> log_probs[t][g][p]   transposed (storage.py:162)
 *   logp_old_in_dev float32 [P][G]                  -> log_probs_old[t][g][p]   (storage.py:163-164)
 *   value_in_dev    float32 [P]                     -> values[t][p]         (storage.py:165)
 *   dones_in_dev    uint8 [E], the step's           -> dones[t][e]          0.0 or 1.0 (storage.py:166)
 *   probs_in_dev    float32 [P][N]                  -> probs[t][p][0:N]     (train.py:257)
 * Every input pointer may be NULL: its buffer is then not touched (and may be NULL too).  An input that is given writes EVERY element
 * of row t of its buffer exactly once and no other row; no arithmetic but the conversions above, so a row is the same bits whoever
 * computes it.  row_features_only != 0 writes features[t] alone - the reference's features[step + 1].copy_(final_features)
 * (train.py:290) - and admits t = T; otherwise t is 0..T-1.  A cursor outside the admitted rows writes NOTHING and sets status_dev[0]
 * (int32 [1]) to 1; the kernel never clears it.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL cursor_dev or status_dev; T, E, A, F, G or action_cols
 * < 1, N < 0, T > 2^24, E * A > 2^30, E * A * K > 2^32; feat1_dev without feat0_dev; row_features_only without feat0_dev; probs_in_dev with N == 0; an
 * input whose buffer is NULL; feat0_dev, feat1_dev or features_dev not 16-byte aligned, rewards_in_dev not 8-byte, any other 32-bit
 * buffer not 4-byte aligned.  Then what the kernel does not take: F not a multiple of 4 (so K is one), G > 8, action_cols > 8, N > 32
 * (dynenv_policy_head's limits): DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_rollout_insert(const int32_t* cursor_dev, int32_t T, int32_t E, int32_t A, int32_t F, int32_t G, int32_t action_cols, int32_t N,
                          int32_t row_features_only, const double* rewards_in_dev, const uint8_t* finished_in_dev, const float* feat0_dev,
                          const float* feat1_dev, const int32_t* actions_in_dev, const float* logp_in_dev, const float* logp_old_in_dev,
                          const float* value_in_dev, const uint8_t* dones_in_dev, const float* probs_in_dev, float* rewards_dev,
                          uint8_t* finished_dev, float* features_dev, float* actions_dev, float* logp_dev, float* logp_old_dev,
                          float* values_dev, float* dones_dev, float* probs_dev, int32_t* status_dev, void* stream);
/* dynenv_rollout_returns, one launch, capturable: _discount_rewards (storage.py:168-209) over rewards_dev [T][P], values_dev [T][P],
 * dones_dev [T][E] and final_value_dev [P] into returns_dev [T][P] and, unless NULL, advantages_dev [T][P]; player p belongs to
 * environment p / A.  float32 throughout; every multiply and every add is rounded on its own (no fused multiply-add), in exactly
 * this order of operations, t = T-1 .. 0, with g = gamma and nd = 1 - dones[t][p / A]:
 *   mode 0, DYNENV_RETURNS_REFERENCE:  R = final_value;  R = rewards[t] + g * R;  returns[t] = R.  Dones are NOT looked at - the
 *           reference's dones4players is all zeros (storage.py:195) - and dones_dev may be NULL.
 *   mode 1, DYNENV_RETURNS_DONES:      R = final_value;  R = rewards[t] + (g * R) * nd;  returns[t] = R.
 *   mode 2, DYNENV_RETURNS_GAE:        adv = 0;  next = t == T-1 ? final_value : values[t+1];
 *           delta = (rewards[t] + (g * next) * nd) - values[t];  adv = delta + ((g * lambda) * adv) * nd;  returns[t] = adv + values[t];
 *           advantages[t] = adv.
 *   In modes 0 and 1 advantages[t] = returns[t] - values[t].
 * Every element of returns_dev (and advantages_dev) is written exactly once.  Inputs that are not finite are outside the contract.
 * Errors, DYNENV_ERR_ARG, before a device is looked for: a NULL rewards_dev, final_value_dev or returns_dev; a mode outside 0..2;
 * dones_dev NULL in modes 1 and 2; values_dev NULL in mode 2 or with advantages_dev; T, E or A < 1, T > 2^24, E * A > 2^30; a buffer
 * not 4-byte aligned. */
int dynenv_rollout_returns(const float* rewards_dev, const float* values_dev, const float* dones_dev, const float* final_value_dev, int32_t T,
                           int32_t E, int32_t A, int32_t mode, float gamma, float gae_lambda, float* returns_dev, float* advantages_dev,
                           void* stream);

/* ---- the curiosity module over a stored rollout, where no gradient is wanted: the reference's ICMNet (DynEnv/models/icm.py) - the
 * forward net of ICMDynamics on cat(f_t, one_hot(a_t)) (icm.py:112-146, 218-226), its inverse net, an ActorLayer, on cat(f_t, f_{t+1})
 * (icm.py:228-238), and the terms of _calc_loss (icm.py:77-109) - on the buffers of the rollout storage above.  Neither the one-hot
 * (icm.py:167-179: a Python loop with one host read per action), the two cats, the hidden layer, the prediction nor the logits exist
 * in memory.  A HOST struct of device pointers: the three matrices in the 16-bit type w_dtype (the operands of the matrix units),
 * everything else float32.  H = 140 is the forward net's hidden width (icm.py:124), H' = 160 its padded size: the rows of fwd_w1 and
 * the columns of fwd_w2 from H on are +0, as are fwd_b1 and the columns of fwd_w1_act from H on; N = sum n_g. */
#define DYNENV_ICM_HIDDEN 140     /* H: ForwardNet.fc_hidden */
#define DYNENV_ICM_HIDDEN_PAD 160 /* H': H rounded up to the 32 elements of a k step of the second product */
typedef struct dynenv_icm {
  const void  *fwd_w1;     /* [160][K] the first K columns of pred_net.fwd_net.fc1.weight, rows from 140 on +0 (16-bit type) */
  const float *fwd_w1_act; /* [N][160] the N one-hot columns of fc1.weight, transposed: row start_g + a is what action a of group g adds; columns from 140 on +0 */
  const float *fwd_b1;     /* [160] fc1.bias, +0 from 140 on */
  const void  *fwd_w2;     /* [K][160] pred_net.fwd_net.fc2.weight, columns from 140 on +0 (16-bit type) */
  const float *fwd_b2;     /* [K] fc2.bias */
  const void  *inv_w;      /* [32][2K] every pred_net.inv_net.blocks.*.Layer.*.weight in the order of ActorLayer.forward's flattened list; rows from N on +0, as in dynenv_policy_t's actor_w (16-bit type) */
  const float *inv_b;      /* [32] the biases in the same order, +0 from N on */
} dynenv_icm_t;
/* dynenv_icm_losses, two launches, capturable (launches and nothing else: nothing is synchronised, allocated or copied; pointers and
 * sizes are frozen by a capture, contents are read at replay).  features_dev float32 [T+1][P][K], actions_dev float32 [T][AD][P] and
 * finished_dev uint8 [T][P] are the storage's buffers (finished_dev NULL: nobody finished); nvec is a HOST array of the G group sizes
 * n_g, start_g = n_0 + .. + n_{g-1}; action_cols = AD, G <= AD <= 8: only the action columns 0..G-1 are read.  An action value is
 * rounded to the nearest integer and clamped into 0..n_g-1 for addressing; a value that had to be clamped ORs bit 0 into status_dev[0]
 * (int32 [1], or NULL), which the kernel never clears - the reference raises an IndexError there.  Per row (t, p), all non-matrix
 * arithmetic in float32, f_t = features[t][p]:
 *   hid  = leaky(f_t W1[:, :K]^T + b1 + sum_g W1_act[start_g + a_g]; slope)   - the one-hot's product is a gather, added in group order
 *   pred = hid W2^T + b2;   curiosity[t][p] = (sum_k (pred_k - f_{t+1,k})^2) / K   - the error against the float32 f_{t+1}
 *   l    = cat(f_t, f_{t+1}) W_inv^T + b_inv;   inverse_ce[t][g][p] = logsumexp(l_g) - l_g[a_g]   - max-subtracted: (m + log(sum_j
 *          exp(l_j - m))) - l_a, which is exactly 0 for a group of one action
 * curiosity_dev float32 [T][P] is F.mse_loss(pred, next, reduction="none").mean(-1), the intrinsic-reward signal of the ICM paper;
 * inverse_ce_dev float32 [T][G][P] is F.cross_entropy(..., reduction="none") per group, in log_probs' layout.  EVERY element of both is
 * written exactly once, finished rows included: the mask belongs to the losses.
 * losses_dev float32 [3] or NULL: when given, a second launch reduces the two under the mask = !finished, n = the number of its true
 * entries, into { sum_mask curiosity / n,  (sum_g sum_mask inverse_ce_g) / (n G),  (float) n } - ICMNet._calc_loss's forward and
 * inverse losses (icm.py:91, 98-100) before their coefficients, which are the caller's business.  It accumulates in double, in one fixed
 * order, and rounds once; the first two are +0 where n == 0 (the reference's early return, icm.py:80-86).
 * Arithmetic: the three matrix products take 16-bit operands of w_dtype (DYNENV_ARR_BF16 / _F16) on the matrix units and accumulate
 * in float32 - the hidden layer is rounded to w_dtype between the two products of the forward net; biases, the gather, the LeakyReLU,
 * the squared error and the logsumexp are float32.  Every sum has one fixed order: a row's result depends on features[t][p],
 * features[t+1][p], actions[t][:, p] and the weights alone - not on its place in the launch, on T, on P or on its neighbours - and
 * the same call twice gives the same bits.  Inputs that are not finite are outside the contract.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL features_dev, actions_dev, nvec, w, curiosity_dev or
 * inverse_ce_dev, or one of w's seven pointers; T, P or K < 1; G outside 1..8, an n_g outside 1..16, N > 32, AD outside G..8; a dtype
 * outside 0..2; features_dev, actions_dev, finished_dev, an output or a weight buffer not 16-byte aligned (losses_dev, status_dev:
 * 4-byte); (T + 1) * P > 2^30 (the launch limit).  Then what the kernel does not take: DYNENV_ARR_F32, a K other than 64, 128 or
 * 256: DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_icm_losses(const float* features_dev, const float* actions_dev, const uint8_t* finished_dev, int32_t T, int32_t P, int32_t K,
                      int32_t action_cols, const int32_t* nvec, int32_t G, int32_t w_dtype, const dynenv_icm_t* w, float slope,
                      float* curiosity_dev, float* inverse_ce_dev, float* losses_dev, int32_t* status_dev, void* stream);

/* ---- the backward of those two losses: the gradients of forward_mean and inverse_mean (losses_dev[0] and [1] above; ICMNet._calc_loss,
 * icm.py:77-109, through ICMDynamics.forward, icm.py:207-240) with respect to the seven packed operands of dynenv_icm_t and to the
 * features.  The forward saves NOTHING for it: the backward recomputes the hidden layer, the prediction and the logits per row from
 * the features, and neither they, the one-hot, the two cats nor a gradient of any of them exists in memory.
 * dynenv_icm_bwd_t: a second HOST struct of device pointers, the transposed copies in w_dtype that the three transposed products read
 * (an operand of the matrix units is contiguous along the contraction); the caller keeps them in step with dynenv_icm_t. */
typedef struct dynenv_icm_bwd {
  const void *fwd_w2_t; /* [160][K] fwd_w2 transposed, rows from 140 on +0: dh = W2^T e contracts over the K outputs (16-bit type) */
  const void *fwd_w1_t; /* [K][160] fwd_w1 transposed, columns from 140 on +0: dfeatures[t] takes W1[:, :K]^T dh, contracted over the hidden units (16-bit type) */
  const void *inv_w_t;  /* [2K][32] inv_w transposed, columns from N on +0: rows 0..K-1 give dfeatures[t], rows K..2K-1 dfeatures[t+1], contracted over the logits (16-bit type) */
} dynenv_icm_bwd_t;
/* dynenv_icm_grad_t: a HOST struct of float32 device pointers, the outputs, in the layouts of the forward's packed operands. */
typedef struct dynenv_icm_grad {
  float *d_fwd_w1;     /* [160][K]; rows from 140 on +0 */
  float *d_fwd_w1_act; /* [N][160]; columns from 140 on +0 */
  float *d_fwd_b1;     /* [160]; +0 from 140 on */
  float *d_fwd_w2;     /* [K][160]; columns from 140 on +0 */
  float *d_fwd_b2;     /* [K] */
  float *d_inv_w;      /* [32][2K]; rows from N on +0 */
  float *d_inv_b;      /* [32]; +0 from N on */
} dynenv_icm_grad_t;
/* The most workgroups the row kernel runs: the grid is persistent and capped, a workgroup keeps its partial weight gradients in
 * registers across the blocks of 32 players it walks and writes ONE slice of the workspace. */
#define DYNENV_ICM_BWD_MAX_WORKGROUPS 256
/* dynenv_icm_backward_workspace: host only, touches no device.  *bytes = min(ceil(P / 32), 256) * (385 K + 5312) * 4: at most
 * 256 * (385 K + 5312) * 4 bytes whatever P and T are - 30 670 848 at K = 64 and 55 902 208 at K = 128.  DYNENV_ERR_ARG: bytes NULL,
 * P or K < 1; DYNENV_ERR_UNSUPPORTED: a K other than 64 or 128. */
int dynenv_icm_backward_workspace(int32_t P, int32_t K, uint64_t* bytes);
/* dynenv_icm_backward, two launches, capturable (launches and nothing else: nothing is synchronised, allocated or copied; pointers and
 * sizes are frozen by a capture, contents are read at replay).  features_dev .. slope are dynenv_icm_losses' arguments, unchanged, and w
 * is the forward's struct.  count_dev is the forward's losses_dev: n is read from its element 2 on the device.  upstream_dev float32
 * [2] = { s_f, s_i } = { dL/dforward_mean, dL/dinverse_mean } on the device.  With alpha = 2 s_f / (n K), beta = s_i / (n G), per
 * ACTIVE row (t, p) (finished[t][p] == 0), in the notation of dynenv_icm_losses, f = features[t][p], f' = features[t+1][p],
 * e = pred - f':
 *   dh = (W2^T e) * leaky'(h_pre), leaky' = 1 where h_pre > 0 and slope elsewhere (h_pre == 0 included: torch's LeakyReLU backward)
 *   q  = cat_g(softmax(l_g) - onehot(a_g)), exactly 0 for a group of one action
 *   d_fwd_w2 = alpha sum e h^T,  d_fwd_b2 = alpha sum e,  d_fwd_w1 = alpha sum dh f^T,  d_fwd_b1 = alpha sum dh,
 *   d_fwd_w1_act[start_g + a_g] += alpha dh for every g,  d_inv_w = beta sum q cat(f, f')^T,  d_inv_b = beta sum q
 *   d_features[t][p] += alpha W1[:, :K]^T dh + beta W_inv[:, :K]^T q;   d_features[t+1][p] += -alpha e + beta W_inv[:, K:]^T q
 * the sums over the active rows only; an inactive row contributes nothing; with n == 0 every gradient is +0.
 * Outputs: EVERY element of the seven buffers of grad is written exactly once per call and nothing is accumulated into; the padding
 * is zero.  d_features_dev float32 [T+1][P][K], or NULL where the features want no gradient (the seven are then the same bits): every
 * element is written exactly once, a (t, p) that no active row touches is +0.  A clamped action ORs bit 0 into status_dev[0] (or NULL)
 * and takes the nearest action's gradients.
 * workspace_dev: workspace_bytes >= what dynenv_icm_backward_workspace(P, K) gives, 16-byte aligned, contents irrelevant before and
 * after the call.
 * Arithmetic: the three recomputed products, the three transposed ones and the four weight-gradient products (the scatter-add into
 * d_fwd_w1_act is the product onehot^T dh) take 16-bit operands of w_dtype on the matrix units and accumulate in float32; biases, the
 * gather, the LeakyReLU and its derivative, the softmax, e, the bias gradients and -alpha e are float32.  NO quantity that carries
 * 1 / n, s_f or s_i is ever rounded to 16 bits: the products run on the unscaled e, dh and q, and alpha and beta are applied in float32
 * behind them - scaling upstream by a power of two scales every output by it exactly.  Every sum has one fixed order and there is no
 * floating-point atomic: the same call twice gives the same bits.  A row of d_features depends on that player's features and
 * actions, the weights, n and upstream alone - not on P, on its place in the launch or on its neighbours.  The weight gradients are
 * added per workgroup, then over the workgroups' slices in workgroup order by the second launch: their summation order depends on P
 * (through the grid) and on nothing else.  Inputs that are not finite are outside the contract.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL features_dev, actions_dev, nvec, w, count_dev,
 * upstream_dev, wt, grad or workspace_dev, or one of the 7 + 3 + 7 pointers in the structs; T, P or K < 1; G outside 1..8, an n_g
 * outside 1..16, N > 32, AD outside G..8; a dtype outside 0..2; a buffer not 16-byte aligned (count_dev, upstream_dev, status_dev:
 * 4-byte); (T + 1) * P > 2^30; a workspace that is too small.  Then what the kernel does not take: DYNENV_ARR_F32, a K other than 64
 * or 128 (at K = 256 the weight gradients' accumulators, 384 float32 per lane, do not fit the register file beside the working set):
 * DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_icm_backward(const float* features_dev, const float* actions_dev, const uint8_t* finished_dev, int32_t T, int32_t P, int32_t K,
                        int32_t action_cols, const int32_t* nvec, int32_t G, int32_t w_dtype, const dynenv_icm_t* w, float slope,
                        const float* count_dev, const float* upstream_dev, const dynenv_icm_bwd_t* wt, const dynenv_icm_grad_t* grad,
                        float* d_features_dev, void* workspace_dev, uint64_t workspace_bytes, int32_t* status_dev, void* stream);

/* ---- the policy head over a STORED rollout, with its backward: what trains the actor and the critic from a rollout that was collected
 * without a gradient (a replayed graph).  The loss between the two calls is the caller's: A2CNet's a2c_loss in torch
 * (DynEnv/models/storage.py:211-262) on the three tensors dynenv_policy_eval returns.
 * dynenv_policy_eval, one launch, capturable (a launch and nothing else).  features_dev float32 [T][P][K] - the storage's
 * features[0..T-1] - and actions_dev float32 [T][AD][P] are the storage's buffers; w, nvec, G, w_dtype, slope and ln_eps are
 * dynenv_policy_head's, action_cols = AD, G <= AD <= 8; there is no Box block (C = 0): actor_w and actor_b are +0 from row N on.  Per
 * row (t, p) the statement is dynenv_policy_head's with the stored action in place of the draw, f = features[t][p]:
 *   l = f W_actor^T + b;  probs_g = softmax(l_g);  a_g = actions[t][g][p], rounded to the nearest integer and clamped into 0..n_g-1 - a
 *       value that had to be clamped ORs bit 0 into status_dev[0] (int32 [1], or NULL), which the kernel never clears (dynenv_icm_losses'
 *       convention);
 *   logp_g = log(clamp(probs_g[a_g], eps32, 1 - eps32)), evaluated in double and rounded once;
 *   value = LayerNorm(leaky(f W1^T + b1; slope); bn, ln_eps) . w2 + b2.
 * Outputs in the storage's layouts, EVERY element written exactly once: logp_dev float32 [T][G][P], probs_dev float32 [T][P][N] or NULL
 * (not written, the others' bits unchanged), value_dev float32 [T][P].
 * Arithmetic and order of sums: dynenv_policy_head's, by the SAME device function - for the action that dynenv_policy_head drew from
 * the same feature row and weights, logp, probs and value are the bits that entry point produced.  A row's result depends on that row,
 * its actions and the weights alone; the same call twice gives the same bits.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: a NULL features_dev, actions_dev, w, nvec, logp_dev or value_dev,
 * or one of w's eight pointers of the actor and the critic; T, P or K < 1; G outside 1..8, an n_g outside 1..16, N > 32, AD outside
 * G..8; a dtype outside 0..2; a buffer not 16-byte aligned (critic_b2, status_dev: 4-byte); T * P > 2^30 (the launch limit).  Then what
 * the kernel does not take: DYNENV_ARR_F32, a K other than 64 or 128: DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_policy_eval(const float* features_dev, const float* actions_dev, int32_t T, int32_t P, int32_t K, int32_t w_dtype,
                       const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t action_cols, float slope, float ln_eps,
                       float* logp_dev, float* probs_dev, float* value_dev, int32_t* status_dev, void* stream);
/* dynenv_policy_bwd_t: a second HOST struct of device pointers, the transposed copies that the two transposed products of the backward
 * read (an operand of the matrix units is contiguous along the contraction); the caller keeps them in step with dynenv_policy_t.
 * ALWAYS bf16, whatever w_dtype is: the operand beside them carries the upstream gradient and is bf16 (below). */
typedef struct dynenv_policy_bwd {
  const void *actor_w_t;   /* [K][32] actor_w transposed, columns from N on +0: d_features takes dl W_actor, contracted over the logits (bf16) */
  const void *critic_w1_t; /* [K][K/2] critic_w1 transposed: d_features takes dh_pre W1, contracted over the hidden units (bf16) */
  const void *actor_w_t_lo, *critic_w1_t_lo; /* the second halves of the two, read with w_dtype float16 only (else they may be NULL): bf16(w - bf16(w)) of the float32 weight w, in the same layouts */
} dynenv_policy_bwd_t;
/* dynenv_policy_grad_t: a HOST struct of float32 device pointers, the outputs, in the layouts of the forward's packed operands. */
typedef struct dynenv_policy_grad {
  float *d_actor_w;                       /* [32][K]; rows from N on +0 */
  float *d_actor_b;                       /* [32]; +0 from N on */
  float *d_critic_w1;                     /* [K/2][K] */
  float *d_critic_b1, *d_critic_ln_w, *d_critic_ln_b; /* [K/2] */
  float *d_critic_w2, *d_critic_b2;       /* [K/2], [1] */
} dynenv_policy_grad_t;
/* The backward walks blocks of DYNENV_POLICY_EVAL_ROWS rows of the T * P on a persistent grid of at most
 * DYNENV_POLICY_EVAL_MAX_WORKGROUPS workgroups: workgroup b takes the blocks b, b + grid, ..., keeps its partial weight gradients in
 * registers and writes ONE slice of the workspace. */
#define DYNENV_POLICY_EVAL_ROWS 64
#define DYNENV_POLICY_EVAL_MAX_WORKGROUPS 256
/* dynenv_policy_eval_backward_workspace: host only, touches no device.  rows = T * P.  *bytes = min(ceil(rows / 64), 256) *
 * (K K / 2 + 34 K + 36) * 4: at most 4 362 240 at K = 64 and 12 881 920 at K = 128.  DYNENV_ERR_ARG: bytes NULL, rows or K < 1, rows >
 * 2^30; DYNENV_ERR_UNSUPPORTED: a K other than 64 or 128. */
int dynenv_policy_eval_backward_workspace(int32_t rows, int32_t K, uint64_t* bytes);
/* dynenv_policy_eval_backward, two launches, capturable (launches and nothing else: nothing is synchronised, allocated or copied).
 * features_dev .. ln_eps are dynenv_policy_eval's arguments, unchanged.  Upstream: d_logp_dev float32 [T][G][P], d_probs_dev float32
 * [T][P][N] or NULL (= all zeros, the same bits), d_value_dev float32 [T][P].  The forward saved NOTHING: a row's logits, probabilities
 * and hidden layer are recomputed by dynenv_policy_eval's device function.  Per row, with onehot(a_g) the stored action's and
 * eps32 <= probs_g[a_g] <= 1 - eps32 meaning "not clamped" (the clamp's gradient is 0 where it binds):
 *   dl_g = d_logp_g [not clamped] (onehot(a_g) - probs_g) + probs_g (d_probs_g - <d_probs_g, probs_g>)   - exactly 0 for a group of one action
 *   with h_pre = f W1^T + b1, h = leaky(h_pre), xh = (h - mean) rstd, y = xh ln_w + ln_b, c = w2 * ln_w (elementwise), m(.) the mean over K/2:
 *   dh_pre = d_value (rstd (c - m(c) - xh m(c xh))) leaky'(h_pre), leaky' = 1 where h_pre > 0 and slope elsewhere (h_pre == 0 included:
 *       torch's LeakyReLU backward)
 *   d_actor_w = sum dl^T f,  d_actor_b = sum dl,  d_critic_w1 = sum dh_pre^T f,  d_critic_b1 = sum dh_pre,  d_critic_ln_w = sum d_value w2 xh,
 *   d_critic_ln_b = sum d_value w2,  d_critic_w2 = sum d_value y,  d_critic_b2 = sum d_value       - the sums over all T * P rows
 *   d_features[t][p] = dl W_actor + dh_pre W1
 * Outputs: EVERY element of the eight buffers of grad is written exactly once per call and nothing is accumulated into; the rows of
 * d_actor_w and d_actor_b from N on are +0.  d_features_dev float32 [T][P][K], or NULL where the features want no gradient (the eight
 * are then the same bits): every element written exactly once.  Zero upstream gives +0 everywhere.  A clamped action ORs bit 0 into
 * status_dev[0] (or NULL) and takes the nearest action's gradients.
 * workspace_dev: workspace_bytes >= what dynenv_policy_eval_backward_workspace(T * P, K) gives, 16-byte aligned, contents irrelevant
 * before and after the call.
 * Arithmetic: the two recomputed products take 16-bit operands of w_dtype on the matrix units and accumulate in float32, as the
 * forward does.  The four products of the backward - dl W_actor, dh_pre W1, dl^T f, dh_pre^T f - run on the matrix units with float32
 * accumulation too, but a quantity that carries an upstream gradient (dl, dh_pre) is NEVER float16: the loss hands over values of order
 * 1 / (T P G), which float16's range does not hold.  THE CHOICE: dl and dh_pre are rounded to bf16 whatever w_dtype is, and the operand
 * beside them - the transposed weights of dynenv_policy_bwd_t, the feature rows - is bf16 too (with w_dtype float16 the recomputed
 * forward alone uses float16).  One bf16 holds 8 significant bits, float16 holds 11: with w_dtype float16 every one of these operands
 * is a PAIR of bf16, v = hi + lo with hi = bf16(v) and lo = bf16(v - hi) of the float32 v - 16 significant bits in bf16's range - and
 * a product A B is the three products hi hi + hi lo + lo hi, accumulated in float32 in that order.  Everything else - softmax, dl, the LayerNorm's backward, the five bias-like sums - is float32.  Rounding
 * to bf16 and float32 accumulation commute with a power of two: scaling all three upstream tensors by one scales every output by it
 * exactly (while nothing underflows).  Every sum has one fixed order and there is no floating-point atomic: the same call twice gives
 * the same bits.  A row of d_features depends on that row, its actions, the weights and its upstream alone.  The weight gradients are
 * added per workgroup - over the blocks it walks, in order - then over the workgroups' slices in workgroup order by the second launch:
 * their order depends on T * P (through the grid) and on nothing else.  Inputs that are not finite are outside the contract.
 * Errors, DYNENV_ERR_ARG, all reported before a device is looked for: dynenv_policy_eval's for the shared arguments; a NULL d_logp_dev,
 * d_value_dev, wt, grad or workspace_dev, or one of the 2 + 8 pointers in the two structs (with float16: 4 + 8); a buffer not 16-byte aligned (d_critic_b2:
 * 4-byte); a workspace that is too small.  Then what the kernel does not take: DYNENV_ARR_F32, a K other than 64 or 128 (K = 256: the
 * module takes its torch route): DYNENV_ERR_UNSUPPORTED, also before the device. */
int dynenv_policy_eval_backward(const float* features_dev, const float* actions_dev, int32_t T, int32_t P, int32_t K, int32_t w_dtype,
                                const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t action_cols, float slope, float ln_eps,
                                const float* d_logp_dev, const float* d_probs_dev, const float* d_value_dev, const dynenv_policy_bwd_t* wt,
                                const dynenv_policy_grad_t* grad, float* d_features_dev, void* workspace_dev, uint64_t workspace_bytes,
                                int32_t* status_dev, void* stream);


/* Device self-test of the deterministic math header: evaluates sincos/atan2/sqrt/div on n host-provided doubles and
 * returns the raw results so tests can compare them bit-for-bit with the host evaluation. out: [n,5]. */
int dynenv_math_selftest(const double* x_host, const double* y_host, int32_t n, double* out_host, int32_t device_id);

/* Device probe of the deterministic math header, routine by routine and build by build.  The library is two translation units with
 * their own optimisation level and their own compiled copy of include/dynenv_math.h: `unit` names the one whose kernel runs.
 * in_host: [n, 4] doubles (a, b, c, d); out_host: [n, 29] doubles, the columns of include/dynenv_math_probe.h (DM_PROBE_NIN,
 * DM_PROBE_NOUT) - every sincos and atan2 variant of the kernels, atan, sqrt, /, rint, fma, the solver's fused forms, powi, Philox,
 * dm_unit, dm_randint.  Host buffers on both sides, one synchronous call, like dynenv_math_selftest.  NULL buffers, n < 0 or an unknown
 * unit are DYNENV_ERR_ARG before a device is looked for; n == 0 is DYNENV_OK; no visible device is DYNENV_ERR_NO_DEVICE. */
#define DYNENV_MATH_UNIT_ROBOCUP 0 /* the unit of the C ABI, the RoboCup and the arranger kernels */
#define DYNENV_MATH_UNIT_DRIVING 1 /* the unit of the Driving kernels */
int dynenv_math_probe(int32_t unit, const double* in_host, int32_t n, double* out_host, int32_t device_id);

#ifdef __cplusplus
}
#endif
#endif /* DYNENV_H */
