"""Host-side mirror of the reference's vectorised environment for the batched HIP step().

`BatchedDynEnv` exposes the surface callers of `make_dyn_env` rely on (DynEnv/utils/base_vec_env.py:57-233 VecEnv,
DynEnv/utils/subproc_vec_env.py:75-172 SubprocVecEnv): `reset`, `step_async`, `step_wait`, `step`, `close`,
`get_attr`, `set_attr`, `env_method`, `seed`, `num_envs`, `observation_space`, `action_space` — but all `num_envs`
environments live on one MI355X and one call into libdynenv_hip.so steps them together.

Two ways to consume a step:
  * fast path  `step_flat(actions)` -> (obs[E,T,A,D] f32, rewards[E,A] f64, dones[E] u8) torch tensors in HBM;
  * compat path `step(actions)` -> the reference's ragged object array obs[E,T,A,3], np rewards/dones, info dicts
    (materialised on the host from the dense tensors, only when a legacy consumer asks).

PyTorch is used for device memory and streams only.  There is no CPU fallback: constructing an env without a GPU,
or without the built library, raises.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Tuple as TTuple

import numpy as np

from . import _capi
from . import spaces as sp
from .compat import CompatBuilder, LazyInfo, LazyInfos, LazyObsArray
from .enums import DynEnvType, NoiseType, ObservationType
from .obs_layout import row_groups


@dataclass
class StateSpaceDescriptor:  # environment_base.py:18-21
    numItemsPerGridCell: int
    space: object


@dataclass
class PredictionDescriptor:  # environment_base.py:24-31
    numContinuous: int = None
    numBinary: int = 0
    contIdx: List[int] = None
    binaryIdx: List[int] = None
    posIdx: List[int] = (0, 1)
    categoricIdx: int = None


@dataclass
class RecoDescriptor:  # environment_base.py:34-38
    featureGridSize: TTuple[int, int]
    fullStateSpace: List[StateSpaceDescriptor]
    targetDefs: List[PredictionDescriptor]


def _driving_spaces(obs_type):
    """DrivingEnvironment._create_observation_space / _setup_action_space / _setup_reconstruction_info
    (DrivingEnvironment.py:129-232); mean = 5.0 always (quirk C1, :235)."""
    mean = 5.0
    pos_xy = sp.Box(-mean * 2, +mean * 2, shape=(2,))
    width_height = sp.Box(-10, 10, shape=(2,))
    orientation = sp.Box(-1, 1, shape=(2,))
    typ = sp.Box(-1, 1, shape=(1,))
    self_space = sp.Dict([("position", pos_xy), ("orientation", orientation), ("width_height", width_height),
                          ("goal_position", pos_xy), ("finished", sp.MultiBinary(1))])
    car_space = sp.Dict([("position", pos_xy), ("orientation", orientation), ("width_height", width_height),
                         ("finished", sp.MultiBinary(1))])
    pedestrian_space = sp.Dict([("position", pos_xy)])
    if obs_type == ObservationType.FULL:
        lane_space = sp.Dict([("points", sp.Box(-mean * 2, mean * 2, shape=(4,))), ("type", typ)])
        obstacle_space = sp.Dict([("position", pos_xy), ("width_height", width_height)])
    else:
        lane_space = sp.Dict([("signed_distance", sp.Box(-mean * 2, mean * 2, shape=(1,))),
                              ("orientation", orientation), ("type", typ)])
        obstacle_space = sp.Dict([("position", pos_xy), ("orientation", orientation), ("width_height", width_height)])
    observation_space = sp.Tuple([sp.Tuple([car_space, obstacle_space, pedestrian_space]),
                                  sp.Tuple([self_space, lane_space])])
    action_space = sp.Tuple((sp.MultiDiscrete([3, 3]),))
    size = sp.Box(-10, 10, shape=(2,))
    conf = sp.MultiBinary(1)
    self_state = StateSpaceDescriptor(1, sp.Dict([("position", pos_xy), ("orientation", orientation), ("size", size),
                                                  ("confidence", conf)]))
    car_state = StateSpaceDescriptor(4, sp.Dict([("position", pos_xy), ("orientation", orientation), ("size", size),
                                                 ("confidence", conf)]))
    obstacle_state = StateSpaceDescriptor(4, sp.Dict([("position", pos_xy), ("size", size), ("confidence", conf)]))
    ped_state = StateSpaceDescriptor(6, sp.Dict([("position", pos_xy), ("confidence", conf)]))
    reco = RecoDescriptor(featureGridSize=(10, 17),
                          fullStateSpace=[self_state, car_state, obstacle_state, ped_state],
                          targetDefs=[PredictionDescriptor(numContinuous=4, contIdx=[2, 3, 4, 5]),
                                      PredictionDescriptor(numContinuous=4, contIdx=[2, 3, 4, 5]),
                                      PredictionDescriptor(numContinuous=2, contIdx=[2, 3]),
                                      PredictionDescriptor(numContinuous=0)])
    return observation_space, action_space, reco


def _robocup_spaces(obs_type, allow_head_turn):
    """RoboCupEnvironment._create_observation_space / _setup_action_space / _setup_reconstruction_info
    (RoboCupEnvironment.py:101-132,338-430), Full observation; mean = 2.0 always (quirk C1, :67)."""
    mean = 2.0
    pos_xy = sp.Box(-mean * 2, +mean * 2, shape=(2,))
    team = sp.Box(-1, 1, shape=(1,))
    self_space = sp.Dict([("position", pos_xy), ("orientation", sp.Box(-1, 1, shape=(4,))), ("team", team),
                          ("penalized or penalized", sp.MultiBinary(1))])
    ball_space = sp.Dict([("position", pos_xy), ("team", team), ("closest", sp.MultiBinary(1))])
    robot_space = sp.Dict([("position", pos_xy), ("orientation", sp.Box(-1, 1, shape=(2,))), ("team", team),
                           ("penalized or penalized", sp.MultiBinary(1))])
    observation_space = sp.Tuple([sp.Tuple([ball_space, robot_space]), sp.Tuple([self_space, ])])
    if obs_type == ObservationType.PARTIAL:  # RoboCupEnvironment.py:346-430, the `else` branch of _create_observation_space
        rad = sp.Box(-mean * 2, +mean * 2, shape=(1,))
        pos_radial = sp.Box(-1, +1, shape=(3,))
        typ = sp.Box(-1, +1, shape=(2,))
        line_space = sp.Dict([("position", pos_radial), ("type", typ)])
        cross_space = goalpost_space = sp.Dict([("position", pos_radial), ("radius", rad), ("type", typ)])
        field_cross_space = sp.Dict([("position", pos_radial), ("radius", rad), ("type", typ), ("angle", sp.Box(-1, +1, shape=(2,)))])
        p_robot = sp.Dict([("position", pos_xy), ("radius", rad), ("orientation", sp.Box(-1, 1, shape=(2,))), ("team", team),
                           ("penalized or penalized", sp.MultiBinary(1))])
        p_ball = sp.Dict([("position", pos_xy), ("radius", rad), ("team", team), ("closest", sp.MultiBinary(1))])
        observation_space = sp.Tuple([sp.Tuple([p_ball, p_robot]),
                                      sp.Tuple([goalpost_space, cross_space, field_cross_space, line_space])])
    if allow_head_turn:
        action_space = sp.Tuple((sp.MultiDiscrete([5, 3, 3]), sp.Box(low=-3, high=3, shape=(1,))))
    else:
        action_space = sp.Tuple((sp.MultiDiscrete([5, 3, 3, 7]),))
    position_xy = sp.Box(-2, +2, shape=(2,))
    conf = sp.MultiBinary(1)
    ball_state = StateSpaceDescriptor(1, sp.Dict([("position", position_xy), ("team", sp.Box(-1, 1, shape=(1,))),
                                                  ("confidence", conf)]))
    robot_state = StateSpaceDescriptor(4, sp.Dict([("position", position_xy),
                                                   ("orientation", sp.Box(-1.0, +1.0, shape=(2,))),
                                                   ("team", sp.Box(-1, 1, shape=(1,))), ("active", sp.MultiBinary(1)),
                                                   ("confidence", conf)]))
    reco = RecoDescriptor(featureGridSize=(1, 1), fullStateSpace=[ball_state, robot_state],
                          targetDefs=[PredictionDescriptor(numContinuous=1, contIdx=[2, ]),
                                      PredictionDescriptor(numContinuous=3, numBinary=1, contIdx=[2, 3, 4], binaryIdx=[5, ])])
    return observation_space, action_space, reco


def reset_mask(envs, num_envs, device=None, what="reset_envs"):
    """The argument of BatchedDynEnv.reset_envs (or of step_flat(active=...): `what` names the caller in the error messages) -> a contiguous
    uint8 [num_envs] mask tensor (on `device`, if given).
      * a bool tensor or numpy array, wherever it lives, and a uint8 tensor ON THE DEVICE - `dones` - are the mask itself: [num_envs],
        taken as it is (bool is viewed as uint8: no copy, nothing is read);
      * a list / numpy array / host tensor of integer ids - uint8 included: on the host small integers are ids, never a mask - is
        built into a mask here and uploaded with one copy; an id may be listed more than once, an id outside [0, num_envs) raises.
    Anything else (a float, ids on the device - checking them would mean reading them back -, more than one dimension, another
    length) raises DynEnvError: before anything is launched."""
    import torch
    if isinstance(envs, torch.Tensor) and (envs.dtype == torch.bool or (envs.dtype == torch.uint8 and envs.device.type != "cpu")):
        m = envs
    elif isinstance(envs, torch.Tensor):
        if envs.device.type != "cpu":
            raise _capi.DynEnvError("%s: a device tensor must be a bool / uint8 mask [%d], not %s ids (they would have to be read back "
                                    "to be checked; `mask[ids] = 1` is one line)" % (what, num_envs, envs.dtype))
        m = envs.numpy()
    else:
        m = np.asarray(envs)
    if not isinstance(m, torch.Tensor):
        if m.dtype == np.bool_:
            m = torch.as_tensor(np.ascontiguousarray(m))
        else:
            if m.size and m.dtype.kind not in "iu":
                raise _capi.DynEnvError("%s: environment ids must be integers, got %s" % (what, m.dtype))
            if m.ndim > 1:
                raise _capi.DynEnvError("%s: expected a list of environment ids, got shape %s" % (what, m.shape))
            ids = m.reshape(-1).astype(np.int64)
            if ids.size and (ids.min() < 0 or ids.max() >= num_envs):
                raise _capi.DynEnvError("%s: environment id %d outside [0, %d)" % (what, int(ids.min() if ids.min() < 0 else ids.max()), num_envs))
            host = np.zeros((num_envs,), np.uint8)
            host[ids] = 1
            m = torch.as_tensor(host)
    if m.dim() != 1 or m.shape[0] != num_envs:
        raise _capi.DynEnvError("%s: the mask must be [%d], got shape %s" % (what, num_envs, tuple(m.shape)))
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if device is not None and m.device != torch.device(device):
        m = m.to(device)
    return m if m.is_contiguous() else m.contiguous()


# The error bits of include/dynenv.h that the compat step raises on - never silently -: (bit, the handles it is looked at on, message % the first
# environment that carries it).
#   0: the reference's arbiter set has no cap; the contact tables have (DRV_NS / RC_NS slots, 128 candidate pairs a substep), and a pair
#      beyond them was dropped: not the reference's state any more
#   3: the reference's observation lists have no cap (DrivingEnvironment.py:816-890); the dense layout has, and rows beyond it were dropped
#   4: two capsule cores exactly collinear / exactly touching: the sign of the contact normal is a convention there (Robot.py:38-52) -
#      possibly not pymunk's trajectory from here on
#   6: a blob that did not fit the handle was refused by set_states / set_exact: that environment still holds its OLD state
_STEP_ERRORS = (
    (1, "any",
     "contact cache or candidate list overflow: a colliding pair was dropped (error bit 0): the state is not the "
     "reference's any more; reset() or set_state() clears it; first in environment %d"),
    (8, "partial",
     "Partial observation: a list had more rows than the dense layout's capacity; rows were dropped (error bit 3), "
     "first in environment %d"),
    (32, "robocup",
     "RoboCup: a velocity or joint impulse left the finite range (error bit 5): the state is not the reference's any more; "
     "first in environment %d"),
    (16, "robocup",
     "RoboCup: the cores of two feet are exactly collinear / touching: the contact normal's sign is a convention "
     "(error bit 4); reset() or set_state() clears it; first in environment %d (set_states() repairs that one alone)"),
    (_capi.ERR_BAD_BLOB, "any",
     "set_states / set_exact: a blob did not fit this handle and was not written (error bit 6): environment %d still holds its "
     "earlier state; a valid set_states() / set_exact() of it or reset() clears the bit"),
)


@dataclass(frozen=True)
class _BlobKind:
    """What tells the canonical state blobs (get_states / set_states) from the exact ones (get_exact / set_exact)"""
    name: str      # dynenv_get_<name> / dynenv_set_<name>, and the name in the messages
    size: str      # the property that holds a blob's bytes
    align: int     # the address a blob buffer is held to HERE: a misaligned device tensor is cloned, a misaligned `out` refused
    structs: bool  # set_*: structured arrays and ctypes structs are accepted next to uint8 arrays


_STATES = _BlobKind("states", "state_size", 1, True)   # (the C side asks for 8 bytes and says so itself)
_EXACT = _BlobKind("exact", "exact_size", 16, False)


class BatchedDynEnv(object):
    """All `num_envs` environments of one GPU shard behind the reference's VecEnv surface.

    `episodes` says who decides that an episode is over:
      * "lockstep" (the default): the whole batch is at one position of its fixed-length episode, the host counts the steps, and
        step_flat(auto_reset=True) resets all environments together at the episode's end (SubprocVecEnv semantics);
      * "per_env": every environment keeps its own time on the device.  step_flat(auto_reset=True) is the step followed by
        reset_envs(dones) on the same stream: `dones` is the step's, and the rows of `obs` of the environments that finished already
        hold their next episode's first observation.  Nothing is decided on the host, so the call may be captured into a graph, and
        set_state / set_states / restore / fork / reset_envs may put environments at different times.  `keep_terminal_obs=True` copies
        `obs` into the persistent tensor `terminal_obs` before that reset (a 38 MB copy per step at 4096 x 10 Driving Full); `track_episode_stats=True`
        refreshes `last_episode_stats` (r, p, o, g) for the environments that just finished (one episode_stats() call per step, into persistent tensors:
        both options work inside a captured step).
        The compat step() / step_wait() raise: the reference's object-array protocol is lock-step by construction."""

    metadata = {"render.modes": []}

    def __init__(self, env_type, num_envs, num_players, observationType=ObservationType.FULL,
                 noiseType=NoiseType.REALISTIC, noiseMagnitude=0, use_continuous_actions=False, seed=42,
                 device=None, env_id_offset=0, flags=None, out_buffers=None, eager_compat=False, episodes="lockstep",
                 keep_terminal_obs=False, track_episode_stats=False):
        import torch  # device memory + streams only
        if not torch.cuda.is_available():
            raise _capi.DynEnvError("dynenv_amd needs an MI355X (HIP device); there is no CPU fallback")
        if episodes not in ("lockstep", "per_env"):
            raise _capi.DynEnvError("episodes must be 'lockstep' or 'per_env', got %r" % (episodes,))
        self._torch = torch
        self._lib = _capi.load()
        self.episodes = episodes
        self.per_env = episodes == "per_env"
        self.keep_terminal_obs, self.track_episode_stats = bool(keep_terminal_obs), bool(track_episode_stats)
        self.last_episode_stats = None
        self._stats_now = None
        env_type = DynEnvType(env_type)
        if env_type == DynEnvType.DRIVE and use_continuous_actions:
            # reference quirk C4: the continuous-action branch of DrivingEnvironment.processAction is broken
            raise NotImplementedError("continuous actions are broken in the reference Driving env (acc/steer unbound)")
        if observationType == ObservationType.IMAGE:
            raise NotImplementedError("Image observations are out of scope (SURVEY.md §2)")
        if flags is None:  # the reference's defaults; an explicit value (0 included: canFall = useObsRewards = False) is taken as is
            flags = 0
            if env_type == DynEnvType.ROBO_CUP:
                # class-level switches of the reference (RoboCupEnvironment.py:18-21): canFall=True, useObsRewards=True,
                # randomInit=False, deterministicTurn=False; make_dyn_env passes allowHeadTurn=use_continuous_actions
                # (DynEnv/__init__.py:9-11)
                flags = _capi.FLAG_CAN_FALL | _capi.FLAG_USE_OBS_REWARDS
                if use_continuous_actions:
                    flags |= _capi.FLAG_ALLOW_HEAD_TURN
        self.flags = int(flags)
        self.eager_compat = bool(eager_compat)  # step()/reset() return the eager object ndarray / tuple of dicts instead of the lazy forms
        self.env_type = env_type
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.cfg = _capi.Cfg(_capi.DYNENV_ABI_VERSION, int(env_type), int(num_envs), int(num_players),
                             int(observationType), int(noiseType), float(noiseMagnitude), int(seed),
                             int(env_id_offset), int(flags), self.device.index or 0, 0)
        self._h = C.c_void_p()
        _capi.check(self._lib.dynenv_create(C.byref(self.cfg), C.byref(self._h)), "dynenv_create")
        self.layout = _capi.Layout()
        _capi.check(self._lib.dynenv_layout(self._h, C.byref(self.layout)), "dynenv_layout")
        L = self.layout
        self.num_envs, self.n_agents, self.n_time_steps = L.num_envs, L.n_agents, L.n_time_steps
        self.obs_dim, self.action_dim, self.steps_per_episode = L.obs_dim, L.action_dim, L.steps_per_episode
        self.observationType, self.noiseType, self.noiseMagnitude = observationType, noiseType, noiseMagnitude
        if env_type == DynEnvType.DRIVE:
            self.observation_space, self.action_space, self.recoDescriptor = _driving_spaces(observationType)
            self.stepNum = 6000 / 10.0  # DrivingEnvironment.py:49
        else:
            self.observation_space, self.action_space, self.recoDescriptor = _robocup_spaces(
                observationType, bool(flags & _capi.FLAG_ALLOW_HEAD_TURN))
            self.stepNum = 12000 / 10.0 / 5  # RoboCupEnvironment.py:61
        E, T, A, D = self.num_envs, self.n_time_steps, self.n_agents, self.obs_dim
        if out_buffers is None:
            self.obs = torch.zeros((E, T, A, D), dtype=torch.float32, device=self.device)
            self.rewards = torch.zeros((E, A), dtype=torch.float64, device=self.device)
            self.dones = torch.zeros((E,), dtype=torch.uint8, device=self.device)
        else:  # e.g. views into a packed all-gather slab (dynenv_amd.distributed)
            self.obs, self.rewards, self.dones = out_buffers
        self.allow_head_turn = env_type == DynEnvType.ROBO_CUP and bool(self.flags & _capi.FLAG_ALLOW_HEAD_TURN)
        self.full_obs_dim = int(self._lib.dynenv_full_obs_dim(self._h))
        self._builder = CompatBuilder(row_groups(self.layout, env_type, observationType))
        self._counts_np = None
        self.terminal_obs = None
        if self.per_env:
            # persistent buffers, written in place by every step: a captured step refreshes THESE tensors at every replay
            if self.keep_terminal_obs:
                self.terminal_obs = torch.zeros_like(self.obs)
            if self.track_episode_stats:
                mk = lambda n, dt: torch.zeros((E, n), dtype=dt, device=self.device)
                self.last_episode_stats = (mk(A, torch.float64), mk(A, torch.float64), mk(A, torch.float64), mk(2, torch.int32))
                self._stats_now = tuple(torch.zeros_like(x) for x in self.last_episode_stats)
        self._episode_step = 0
        self._needs_reset = True
        self._pending = None
        self.closed = False

    def use_buffers(self, obs, rewards, dones):
        """Switch the output buffers of the next reset/step (ping-pong slabs of dynenv_amd.distributed.StepGather)."""
        assert tuple(obs.shape) == tuple(self.obs.shape) and obs.dtype == self.obs.dtype and obs.is_contiguous()
        self.obs, self.rewards, self.dones = obs, rewards, dones

    # ------------------------------------------------------------------ fast path
    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def reset_flat(self):
        _capi.check(self._lib.dynenv_reset(self._h, _capi.ptr(self.obs), self._stream()), "dynenv_reset")
        self._episode_step = 0
        self._needs_reset = False
        self._counts_np = None  # the scene (obstacle / pedestrian counts) changed
        return self.obs

    def reset_envs(self, envs):
        """Reset exactly the listed environments on the device (dynenv_reset_masked: one wave per environment, on torch's current stream,
        nothing waited for) and write their first observation into their rows of `self.obs`; every other environment and its rows stay
        as they are.  `envs`: a bool / uint8 [num_envs] device tensor - `self.dones`, say -, used as it is, or a list / numpy array / host
        tensor of environment ids (reset_mask).  A listed environment ends up exactly as reset_flat() would leave it: next episode,
        time 0, a fresh scene, contact cache, shortcut state and error word cleared.  With episodes="lockstep" the host's position in
        the episode stays where it is: `dones` of an environment reset on its own then comes from its own time on the device."""
        mask = reset_mask(envs, self.num_envs, self.device)
        _capi.check(self._lib.dynenv_reset_masked(self._h, _capi.ptr(mask), _capi.ptr(self.obs), self._stream()),
                    "dynenv_reset_masked")
        self._counts_np = None  # the scenes (obstacle / pedestrian counts) changed
        return self.obs

    def _stage_actions(self, actions):
        """-> (int32 [E, A, action_dim] on the device, float64 [E, A] head channel or None).  With allowHeadTurn the 4th action is
        the reference's continuous head turn (Box(-3, 3), RoboCupEnvironment.py:339-342): any float in the 4th column (or a
        (discrete [E, A, 3], head [E, A]) pair) travels as float64 and is not truncated."""
        torch = self._torch
        head = None
        if self.allow_head_turn:
            if isinstance(actions, (tuple, list)) and len(actions) == 2:
                disc, hd = actions
                disc = torch.as_tensor(np.asarray(disc) if not isinstance(disc, torch.Tensor) else disc)
                hd = torch.as_tensor(np.asarray(hd, dtype=np.float64) if not isinstance(hd, torch.Tensor) else hd)
                actions = torch.cat([disc.to(torch.float64), hd.to(torch.float64).reshape(disc.shape[0], disc.shape[1], 1)], -1)
            a_f = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(actions, dtype=np.float64))
            if a_f.dim() == 3 and a_f.shape[-1] == 4:
                head = a_f[..., 3].to(device=self.device, dtype=torch.float64).contiguous()
                a = a_f.to(device=self.device).to(torch.int32).contiguous()
                a[..., 3] = 0
            else:
                a = a_f.to(device=self.device).to(torch.int32).contiguous()
        elif isinstance(actions, torch.Tensor):
            a = actions
            if a.device != self.device or a.dtype != torch.int32 or not a.is_contiguous():
                a = a.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            a = torch.as_tensor(np.ascontiguousarray(actions, dtype=np.int32)).to(self.device)
        if tuple(a.shape) != (self.num_envs, self.n_agents, self.action_dim):
            # DrivingEnvironment.py:262-263
            raise Exception("Error: There must be %d actions for every %s" %
                            (self.action_dim, "car" if self.env_type == DynEnvType.DRIVE else "robot"))
        return a, head

    def step_flat(self, actions, auto_reset=True, validate=False, active=None):
        """One env step of every environment: ONE kernel launch on torch's current stream.  Nothing is waited for and no flag is
        read here: a consumer of Partial observations that wants to know whether a list ever outgrew the layout's capacity (rows
        dropped; astronomically unlikely, include/dynenv.h error bit 3) calls error_flags() at its own pace; step() does, and raises.

        `active` (episodes="per_env" only): step exactly the listed environments and hold the others still (dynenv_step_masked) - a
        bool / uint8 [num_envs] device tensor, used as it is (nothing is read on the host: a captured call reads the tensor's contents
        at every replay), or a list / numpy array / host tensor of environment ids (reset_mask).  A listed environment gets exactly the
        step it would have got; of an unlisted one no byte of state changes, and its rows of the returned `obs`, `rewards` and `dones`
        are STALE: they keep what the tensors held before the call - usually that environment's last own step.  A caller that sums
        `rewards` masks them (`rew * active.unsqueeze(1)`); its rows of `actions` are not read.  With auto_reset=True the environments
        reset are `dones & active` (a stale `dones` byte resets nothing), and last_episode_stats / terminal_obs follow the same mask.
        validate=True looks at the listed rows only."""
        if self._needs_reset:
            raise _capi.DynEnvError("call reset() before step()")
        torch = self._torch
        if active is not None and not self.per_env:
            # dones and the auto-reset of a lock-step handle follow ONE host-side position in the episode: a partial step would make it meaningless
            raise _capi.DynEnvError("step_flat(active=...) needs a handle with episodes='per_env' (every environment keeps its own time)")
        if auto_reset and not self.per_env and torch.cuda.is_current_stream_capturing():
            # the host's position in the episode does not advance at replay: a reset decided now would be frozen into the graph (or never come)
            raise _capi.DynEnvError("step_flat(auto_reset=True) inside a stream capture: capture with auto_reset=False and reset between replays")
        mask = reset_mask(active, self.num_envs, self.device, what="step_flat") if active is not None else None
        a, head = self._stage_actions(actions)
        listed = (lambda bad: bad) if mask is None else (lambda bad: bad & mask.bool().reshape((-1,) + (1,) * (bad.dim() - 1)))
        if validate and self.env_type == DynEnvType.DRIVE:
            if bool(listed((a < 0) | (a > 2)).any()):  # DrivingEnvironment.py:365-368
                raise Exception("Error: Acceleration must be between +/-3")
        if validate and self.env_type == DynEnvType.ROBO_CUP:  # RoboCupEnvironment.py:543-550
            hi = torch.tensor([4, 2, 2], device=a.device, dtype=a.dtype)
            if bool(listed((a[..., :3] < 0) | (a[..., :3] > hi)).any()):
                raise Exception("Error: Robot movement must be categorical in the range [0-4]")
            bad_head = listed(head.abs() > 6).any() if head is not None else listed((a[..., 3] < 0) | (a[..., 3] > 6)).any()
            if bool(bad_head):
                raise Exception("Error: Head turn must be between +/-6")
        if mask is not None:
            # (the casts spelled out in this method alone: the per-step path pays for no helper call)
            _capi.check(self._lib.dynenv_step_masked(self._h, C.c_void_p(mask.data_ptr()), C.c_void_p(a.data_ptr()),
                                                     C.c_void_p(head.data_ptr()) if head is not None else None,
                                                     C.c_void_p(self.obs.data_ptr()), C.c_void_p(self.rewards.data_ptr()),
                                                     C.c_void_p(self.dones.data_ptr()), self._stream()), "dynenv_step_masked")
        elif head is not None:
            _capi.check(self._lib.dynenv_step_head(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(head.data_ptr()),
                                                   C.c_void_p(self.obs.data_ptr()), C.c_void_p(self.rewards.data_ptr()),
                                                   C.c_void_p(self.dones.data_ptr()), self._stream()), "dynenv_step_head")
        else:
            _capi.check(self._lib.dynenv_step(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(self.obs.data_ptr()),
                                              C.c_void_p(self.rewards.data_ptr()), C.c_void_p(self.dones.data_ptr()),
                                              self._stream()), "dynenv_step")
        if self.per_env:
            # every environment ends on its own: the device's `dones` is the mask, no host counter is read or kept
            if auto_reset:
                # (with `active`: an unlisted environment's dones byte is stale, so the finished AND listed ones - one op, nothing read)
                ended = self.dones if mask is None else torch.logical_and(self.dones, mask)
                if self.keep_terminal_obs:
                    if mask is None:
                        self.terminal_obs.copy_(self.obs)
                    else:
                        torch.where(mask.bool().reshape(-1, 1, 1, 1), self.obs, self.terminal_obs, out=self.terminal_obs)
                if self.track_episode_stats:
                    self.episode_stats(out=self._stats_now)
                    done = ended.bool().unsqueeze(1)
                    for last, now in zip(self.last_episode_stats, self._stats_now):
                        torch.where(done, now, last, out=last)
                self.reset_envs(ended)
            return self.obs, self.rewards, self.dones
        self._episode_step += 1
        self.last_done = self._episode_step >= self.steps_per_episode  # fixed-length episodes
        if self.last_done and auto_reset:
            # SubprocVecEnv worker semantics (subproc_vec_env.py:19-22): keep the terminal observation, return the reset one
            self.terminal_obs = self.obs.clone()
            self._episode_stats = self.episode_stats()
            self.reset_flat()
        return self.obs, self.rewards, self.dones

    def episode_stats(self, out=None):
        """(r, p, o [E, A] float64, g [E, 2] int32) of the running episodes; `out`: four such tensors to write into instead of new ones"""
        torch = self._torch
        E, A = self.num_envs, self.n_agents
        if out is not None:
            r, p, o, g = out
        else:
            r = torch.empty((E, A), dtype=torch.float64, device=self.device)
            p = torch.empty_like(r)
            o = torch.empty_like(r)
            g = torch.empty((E, 2), dtype=torch.int32, device=self.device)
        _capi.check(self._lib.dynenv_episode_stats(self._h, _capi.ptr(r), _capi.ptr(p),
                                                   _capi.ptr(o), _capi.ptr(g), self._stream()),
                    "dynenv_episode_stats")
        return r, p, o, g

    def counts(self):
        c = self._torch.empty((self.num_envs, 2), dtype=self._torch.int32, device=self.device)
        _capi.check(self._lib.dynenv_counts(self._h, _capi.ptr(c), self._stream()), "dynenv_counts")
        return c

    def error_flags(self):
        f = C.c_int32(0)
        _capi.check(self._lib.dynenv_error_flags(self._h, C.byref(f)), "dynenv_error_flags")
        return f.value

    def debug_counters(self):
        out = (C.c_int64 * 16)()
        _capi.check(self._lib.dynenv_debug_counters(self._h, out), "dynenv_debug_counters")
        return dict(fast=out[0], quiescent=out[1], contact=out[2], slot_sum=out[3], why_cand=out[4], why_moving=out[5],
                    why_inert=out[6], steady=out[7], light=out[8], split=out[9], isolated_next=out[10], isolation_timeouts=out[11],
                    isolation_mode=out[12], placement_validated=out[13], placement_invalid_launches=out[14], isolation_pauses=out[15])

    def debug_placement(self):
        """uint32 [4096]: XCC << 16 | SE, SH, CU, SIMD bits of HW_ID of every regular block of the last step (mode 1 handles), else empty"""
        out = np.zeros((4096,), np.uint32)
        n = self._lib.dynenv_debug_placement(self._h, C.c_void_p(out.ctypes.data), out.size)
        if n < 0:
            _capi.check(n, "dynenv_debug_placement")
        return out[:n]

    def get_state(self, env=0):
        st = _capi.DrivingState() if self.env_type == DynEnvType.DRIVE else _capi.RoboCupState()
        _capi.check(self._lib.dynenv_get_state(self._h, env, C.byref(st), C.sizeof(st)), "dynenv_get_state")
        return st

    def _substeps(self):
        return 50 if self.env_type == DynEnvType.ROBO_CUP else 10

    def set_state(self, env, st):
        """Episodes are lock-step: `dones` and the auto-reset follow ONE host-side position in the episode, and that
        position follows the blob's `elapsed` - like restore() - so a blob with an edited `elapsed` moves host and device together.
        (Blobs that put different environments at different times make `dones` meaningless; the device keeps stepping them.)"""
        _capi.check(self._lib.dynenv_set_state(self._h, env, C.byref(st), C.sizeof(st)), "dynenv_set_state")
        self._counts_np = None  # the scene (obstacle / pedestrian counts) may have changed
        if self.per_env:  # no host-side position: the environment's own `elapsed` is all there is
            self._needs_reset = False
            return
        step = int(st.elapsed) // self._substeps()
        if not self._needs_reset and step != self._episode_step and self.num_envs > 1 and not getattr(self, "_set_state_moved", False):
            # ONE blob with another `elapsed` than the batch's moves the host's episode position - and with it `dones` and the auto-reset of
            # ALL environments; the device keeps per-environment times.  Legitimate when every environment is being set (the tests do);
            # said once so that a scene written into one environment does not silently shift the others' episode end.
            import warnings
            warnings.warn("set_state: the blob's elapsed (%d) puts the batch's episode position at step %d (was %d): dones / auto-reset of every "
                          "environment follow it" % (int(st.elapsed), step, self._episode_step), stacklevel=2)
            self._set_state_moved = True
        self._needs_reset = False
        self._episode_step = step

    # ------------------------------------------------------------------ batched, device-side state transfer
    @property
    def state_size(self):
        """bytes of one canonical state blob (_capi.state_dtype(self.env_type).itemsize)"""
        return int(self._lib.dynenv_state_size(self._h))

    def _env_ids(self, env_ids, unique=False):
        """-> (int32 [n] tensor on the device or None = environments 0..n-1, n).  A list / numpy array / host tensor is uploaded with one
        copy and, with `unique`, checked for duplicates first; ids that already live on the device are taken as they are (nothing is
        read back: an id outside [0, E) is skipped by the kernels, dynenv_set_states reports it in its status)."""
        torch = self._torch
        if env_ids is None:
            return None, self.num_envs
        if isinstance(env_ids, torch.Tensor) and env_ids.device.type != "cpu":
            ids = env_ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            return ids, int(ids.numel())
        host = np.asarray(env_ids.numpy() if isinstance(env_ids, torch.Tensor) else env_ids).reshape(-1).astype(np.int64)
        if unique and np.unique(host).size != host.size:
            raise _capi.DynEnvError("set_states / set_exact: an environment id is listed twice (its state would be unspecified)")
        if host.size and (host.min() < -2 ** 31 or host.max() >= 2 ** 31):
            raise _capi.DynEnvError("environment ids must fit int32")
        return torch.as_tensor(host.astype(np.int32)).to(self.device), int(host.size)

    def _get_blobs(self, kind, env_ids, out):
        """get_states / get_exact: one launch that writes the `kind` blobs of `env_ids` into `out` (None: a new tensor)"""
        torch = self._torch
        ids, n = self._env_ids(env_ids)
        size = getattr(self, kind.size)
        if out is None:
            out = torch.empty((n, size), dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or out.device != self.device or tuple(out.shape) != (n, size) or not out.is_contiguous()
              or out.data_ptr() % kind.align):
            raise _capi.DynEnvError("get_%s: out must be a contiguous, %d-byte aligned uint8 [%d, %d] tensor on %s"
                                    % (kind.name, kind.align, n, size, self.device))
        fn = "dynenv_get_" + kind.name
        _capi.check(getattr(self._lib, fn)(self._h, _capi.ptr(ids if n else None), n, _capi.ptr(out if n else None), self._stream()), fn)
        return out

    def _set_blobs(self, kind, env_ids, blobs, episode_step):
        """set_states / set_exact: one launch that writes blobs[k] into environment env_ids[k]; -> the int32 [n] status tensor"""
        torch = self._torch
        what = "set_" + kind.name
        if self._needs_reset and episode_step is None and not self.per_env:
            raise _capi.DynEnvError("%s before the first reset(): pass episode_step (the batch's position in its lock-step episode)" % what)
        ids, n = self._env_ids(env_ids, unique=True)
        size = getattr(self, kind.size)
        if isinstance(blobs, torch.Tensor):
            b = blobs
            if b.dtype != torch.uint8:
                raise _capi.DynEnvError("%s: blobs must be uint8 [n, %d]" % (what, size))
            if b.device != self.device or not b.is_contiguous():
                b = b.to(self.device).contiguous()
            if b.data_ptr() % kind.align:  # (a view into a larger tensor: a copy starts at an allocation)
                b = b.clone()
        elif kind.structs and not (isinstance(blobs, np.ndarray) and blobs.dtype == np.uint8):
            b = torch.as_tensor(np.ascontiguousarray(_capi.states_as_blobs(blobs))).to(self.device)
        else:
            b = torch.as_tensor(np.ascontiguousarray(blobs, dtype=np.uint8)).to(self.device)
        if b.dim() != 2 or b.shape[1] != size:
            raise _capi.DynEnvError("%s: blobs must be uint8 [n, %d], got shape %s" % (what, size, tuple(b.shape)))
        if ids is None:
            n = int(b.shape[0])  # environments 0..n-1
            if n > self.num_envs:
                raise _capi.DynEnvError("%s: %d blobs for %d environments" % (what, n, self.num_envs))
        elif int(b.shape[0]) != n:
            raise _capi.DynEnvError("%s: %d environment ids but %d blobs" % (what, n, int(b.shape[0])))
        status = torch.empty((n,), dtype=torch.int32, device=self.device)
        fn = "dynenv_" + what
        _capi.check(getattr(self._lib, fn)(self._h, _capi.ptr(ids if n else None), n, _capi.ptr(b if n else None),
                                           _capi.ptr(status if n else None), self._stream()), fn)
        self._counts_np = None  # the scenes (obstacle / pedestrian counts) may have changed
        if episode_step is not None:
            self._episode_step = int(episode_step)
            self._needs_reset = False
        elif self.per_env:
            self._needs_reset = False
        return status

    def get_states(self, env_ids=None):
        """The canonical state blobs of `env_ids` (a list, a numpy array or a device tensor; None = all environments, in order) as a
        torch.uint8 [n, state_size] tensor on the device: ONE launch on torch's current stream, nothing is waited for and nothing
        touches the host.  Row k holds exactly the bytes get_state(env_ids[k]) returns; `_capi.blobs_as_states(t.cpu().numpy(),
        env_type)` views them as a numpy structured array.  An id outside [0, num_envs) leaves its row as allocated (unspecified)."""
        return self._get_blobs(_STATES, env_ids, None)

    def set_states(self, env_ids, blobs, episode_step=None):
        """Write blobs[k] into environment env_ids[k] (None = environments 0..n-1), all in ONE launch on torch's current stream.  `blobs`
        is a uint8 [n, state_size] device tensor (used in place) or a numpy array - uint8 [n, state_size] or a structured array of
        `_capi.state_dtype` - uploaded with one copy.  Each environment ends up exactly as set_state() leaves it: whole field rows
        rewritten, contact cache and error word cleared.  Returns the per-blob status as an int32 [n] device tensor (not read here):
        0 written, 1 blob rejected - it does not fit this handle; the environment is untouched and carries error bit 6 until it is
        reset or validly set, step() raises on it -, 2 id outside [0, num_envs).

        Episodes are lock-step: `dones` and the auto-reset follow ONE host-side position in the episode.  Unlike set_state,
        which moves that position to the blob's `elapsed`, this call reads nothing back and leaves it where it is unless `episode_step`
        says where the batch now stands; blobs whose `elapsed` differs from it keep their own time on the device, and `dones` is not
        meaningful for them.  On a handle that was never reset there is no position to keep: pass `episode_step` then.
        Duplicate ids in one call are an error (raised when the ids live on the host, unspecified state otherwise)."""
        return self._set_blobs(_STATES, env_ids, blobs, episode_step)

    def fork(self, src_ids, dst_ids, exact=False):
        """Copy the state of environment src_ids[k] over environment dst_ids[k] - set_states(dst_ids, get_states(src_ids)): two launches,
        no host copy.  One source may be listed many times (branch one state into many environments), a destination once.  Like
        set_state, the copy drops the contact cache (warm-started impulses), so source and copy are the same canonical state, not the
        same checkpoint.  A forked environment keeps its OWN random stream: draws are keyed by the environment's global id, the
        episode counter and the time inside the episode, and the id is the destination's - so the copy's later random events
        (pedestrian starts, observation noise, ...) are its own, not a replay of the source's.  Returns set_states' status tensor.

        exact=True: the copy goes through get_exact / set_exact instead and carries EVERY row of the source - the contact cache with its
        warm-start impulses, the shortcut state and call-to-call caches, the diagnostic counters and the error word (a source with a
        sticky error bit hands it on; nothing is cleared) - so source and copy are the same checkpoint.  The copy still draws from the
        destination's own random streams.  Returns set_exact's status tensor."""
        if exact:
            return self.set_exact(dst_ids, self.get_exact(src_ids))
        return self.set_states(dst_ids, self.get_states(src_ids))

    # ------------------------------------------------------------------ exact, device-side save and restore
    @property
    def exact_size(self):
        """bytes of one exact blob (a multiple of 16)"""
        return int(self._lib.dynenv_exact_size(self._h))

    def get_exact(self, env_ids=None, out=None):
        """The exact blobs of `env_ids` (a list, a numpy array or a device tensor; None = all environments, in order) as a torch.uint8
        [n, exact_size] tensor on the device: ONE launch on torch's current stream, nothing is waited for and nothing touches the
        host; capturable.  An exact blob is every simulation-state row of the environment, bit for bit - what checkpoint() keeps of it,
        contact cache, shortcut state, counters and error word included - behind a 16-byte header; its format is opaque and valid for
        this library build and this configuration (environment type, players, observation type, flags; NOT num_envs, env_id_offset,
        seed or noise: a blob fits another environment and another handle of the same configuration).  set_exact() of it followed by
        the same actions reproduces the run bit for bit, random draws included (they are keyed by the environment's id, episode
        counter and time, and the last two travel in the blob).  `out`: a contiguous uint8 [n, exact_size] device tensor to write into;
        the row of an id outside [0, num_envs) is left as it is."""
        return self._get_blobs(_EXACT, env_ids, out)

    def set_exact(self, env_ids, blobs, episode_step=None):
        """Write exact blob blobs[k] (get_exact) into environment env_ids[k] (None = environments 0..n-1), all in ONE launch on torch's
        current stream; capturable when `env_ids` and `blobs` are device tensors (their contents are read at replay; an id of -1
        switches its slot off).  `blobs` is a uint8 [n, exact_size] device tensor (used in place) or a numpy array (one upload).  Every
        row of a listed environment ends up with exactly the saved bytes - error word and diagnostic counters included - and nothing
        else changes.  Returns the per-blob status as an int32 [n] device tensor (not read here): 0 written, 1 the blob does not carry
        this configuration's layout tag (a buffer nobody wrote, a blob of another configuration) - the environment is untouched and
        carries error bit 6 until it is reset or validly set, step() raises on it -, 2 id outside [0, num_envs).

        Lock-step handles: the host's position in the episode stays where it is unless `episode_step` says where the batch now stands
        (set_states' rule; a roll-back of k steps of the whole batch passes the position it saved at); on a handle that was never reset
        pass `episode_step`.  Duplicate ids in one call are an error (raised when the ids live on the host)."""
        return self._set_blobs(_EXACT, env_ids, blobs, episode_step)

    def error_flags_per_env(self):
        """Every environment's error word (the bits of include/dynenv.h's dynenv_error_flags) as an int32 [num_envs] device tensor: one
        launch, nothing waited for.  Its OR over the environments is error_flags()."""
        f = self._torch.empty((self.num_envs,), dtype=self._torch.int32, device=self.device)
        _capi.check(self._lib.dynenv_error_flags_env(self._h, _capi.ptr(f), self._stream()), "dynenv_error_flags_env")
        return f

    def _first_env_with(self, bit):
        """lowest id of an environment whose error word has `bit` (the compat step names it so that the caller can repair that one)"""
        hit = np.nonzero(self.error_flags_per_env().cpu().numpy() & bit)[0]
        return int(hit[0]) if hit.size else -1

    # ------------------------------------------------------------------ exact checkpoint
    def checkpoint(self):
        """Every device array of the handle, bit for bit, as a numpy uint8 array (contact cache, shortcut state, episode
        counters and seed included): restore() + the same actions reproduces the run exactly, mid-episode too."""
        n = int(self._lib.dynenv_checkpoint_size(self._h))
        buf = np.empty((n,), np.uint8)
        _capi.check(self._lib.dynenv_checkpoint_save(self._h, C.c_void_p(buf.ctypes.data), n), "dynenv_checkpoint_save")
        return buf

    def restore(self, buf):
        """Load a checkpoint() of a handle with this configuration: every device array, and the checkpoint's seed - whatever seed this
        handle was created with or given by seed() since.  After a step_flat() / reset_envs() of this handle has been captured into a
        graph, a checkpoint taken under another seed raises DynEnvError and nothing is copied (a replay would keep drawing from the
        captured seed): restore it into a new handle."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        _capi.check(self._lib.dynenv_checkpoint_load(self._h, C.c_void_p(buf.ctypes.data), buf.size), "dynenv_checkpoint_load")
        self._needs_reset = False
        self._counts_np = None
        if self.per_env:
            return
        # the host's position in the (lock-step, fixed-length) episode follows the restored device state: auto-reset and
        # `dones` are driven by it
        self._episode_step = int(self.get_state(0).elapsed) // self._substeps()

    def full_state_obs(self):
        """The noise-free Full observation of the current state, [E, A, full_obs_dim] float32 on the device, whatever the
        observation type (getFullState: what info['Full State'] / info['Recon States'] are made of)."""
        out = self._torch.empty((self.num_envs, self.n_agents, self.full_obs_dim), dtype=self._torch.float32, device=self.device)
        _capi.check(self._lib.dynenv_full_obs(self._h, _capi.ptr(out), self._stream()), "dynenv_full_obs")
        return out

    def global_state(self):
        """RoboCup: getFullState(agent=None) of the current state for every environment, float32 [E, 6 A + 3] on the device -
        robots [A, 6] = (x, y, cos, sin, team, fallen | penalized) in field coordinates, then the ball (x, y, ballOwned) - the
        content of info['Full State'] (RoboCupEnvironment.py:511, :1149-1161)."""
        if self.env_type != DynEnvType.ROBO_CUP:
            raise NotImplementedError("Driving's getFullState(None) is made of columns of full_state_obs()")
        out = self._torch.empty((self.num_envs, 6 * self.n_agents + 3), dtype=self._torch.float32, device=self.device)
        _capi.check(self._lib.dynenv_global_state(self._h, _capi.ptr(out), self._stream()), "dynenv_global_state")
        return out

    def agent_finished(self, out=None):
        """bool [E, A] on the device, with no host read: whether each agent is out of the game in the current state - what the
        reference's rollout reads as `agent[-1] for agent in info['Full State'][0]` (DynEnv/models/train.py:272) from the compat step().
        Driving: column 8 (`finished`) of the noise-free Full rows - the step's last snapshot in `self.obs` with Full observations,
        full_state_obs() otherwise; RoboCup: column 5 of each robot's six in global_state() (fallen | penalized).  `out`: a bool [E, A]
        tensor to write into (a recorded step refreshes it at every replay)."""
        torch = self._torch
        if self.env_type == DynEnvType.ROBO_CUP:
            col = self.global_state()[:, :6 * self.n_agents].view(self.num_envs, self.n_agents, 6)[:, :, 5]
        elif self.observationType == ObservationType.FULL:
            col = self.obs[:, -1, :, 8]
        else:
            col = self.full_state_obs()[:, :, 8]
        return torch.ne(col, 0, out=out) if out is not None else torch.ne(col, 0)

    def refresh_obs(self):
        """Re-emit the observation of the current state into `self.obs` (after set_state / restore).  Full observations only:
        a Partial observation is a noisy draw keyed by the step that produced it."""
        if self.observationType != ObservationType.FULL:
            raise NotImplementedError("refresh_obs re-emits Full observations; use full_state_obs() for the true state")
        full = self.full_state_obs()
        self.obs.copy_(full.unsqueeze(1).expand(-1, self.n_time_steps, -1, -1))
        return self.obs

    # ------------------------------------------------------------------ reference-compatible (legacy) path
    def _host_counts(self):
        """(n_obstacles, n_pedestrians) per environment on the host: they change at a reset only, so one copy per episode."""
        if self._counts_np is None:
            self._counts_np = self.counts().cpu().numpy()
        return self._counts_np

    def _snapshot(self):
        """self.obs as the compat containers keep it (self.obs is rewritten by the next step): a clone in HBM that is copied to the
        host when somebody looks at an element, or - eager_compat - the host copy now."""
        return self.obs.cpu().numpy() if self.eager_compat else self.obs.clone()

    def _compat(self, dense, counts):
        return self._builder.array(dense, counts) if self.eager_compat else LazyObsArray(self._builder, dense, counts)

    def _compat_obs(self, obs_t, counts):
        """dense [E,T,A,D] (numpy or device tensor) -> the eager object ndarray [E,T,A,3]: the name earlier callers know, kept over
        the one builder."""
        return self._builder.array(obs_t, counts)

    def _full_states(self, full_np, counts, e, glob_np=None):
        """info['Full State'] / info['Recon States'] (DrivingEnvironment.py:306-307, RoboCupEnvironment.py:511-512) of env e from
        the noise-free Full rows [E, A, full_obs_dim] of the state after the step (whatever the observation type) and, for
        RoboCup, the rows of dynenv_global_state [E, 6 A + 3]."""
        A = self.n_agents
        if self.env_type == DynEnvType.ROBO_CUP:
            recon = []  # getFullState(agent) = [ball, self, robots] (:1164-1188)
            for a in range(A):
                r = full_np[e, a]
                recon.append([r[0:4].reshape(1, 4).copy(), r[4:12].reshape(1, 8).copy(),
                              r[12:12 + (A - 1) * 6].reshape(A - 1, 6).copy()])
            g = glob_np[e]  # getFullState(None) = [robots [A, 6], ball [3]] (:1149-1161)
            return [g[:6 * A].reshape(A, 6).copy(), g[6 * A:6 * A + 3].copy()], recon
        n_obst, n_ped = int(counts[e, 0]), int(counts[e, 1])
        o1 = 9 + (A - 1) * 7
        o2, o3 = o1 + 80, o1 + 120
        recon = []
        for a in range(A):
            r = full_np[e, a]
            recon.append([r[0:9].reshape(1, 9).copy(), r[9:o1].reshape(A - 1, 7).copy(),
                          r[o1:o1 + n_obst * 4].reshape(n_obst, 4).copy(),
                          r[o2:o2 + n_ped * 2].reshape(n_ped, 2).copy(),
                          r[o3:o3 + 40].reshape(8, 5).copy()])
        # complete state: every car row = own [x,y,cos,sin,w,h] + finished
        cars = np.stack([np.concatenate([recon[a][0][0, :6], recon[a][0][0, 8:9]]) for a in range(A)]).astype(np.float32)
        full = [cars, recon[0][2], recon[0][3], recon[0][4]]
        return full, recon

    def reset(self):
        self.reset_flat()
        return self._compat(self._snapshot(), self._host_counts())

    def step_async(self, actions):
        self._pending = actions

    def step_wait(self):
        if self.per_env:
            raise _capi.DynEnvError("step() / step_wait() return the reference's lock-step object arrays (SURVEY F6): with episodes='per_env' "
                                    "use step_flat()")
        actions, self._pending = self._pending, None
        counts = self._host_counts()
        self.step_flat(actions if self.allow_head_turn else np.asarray(actions), auto_reset=False, validate=True)
        # the state behind info['Full State'] / info['Recon States']: with Full observations it is the step's last snapshot; with
        # Partial ones a noise-free Full row is emitted now (one short launch) and copied to the host only if somebody asks
        full_dev = self.full_state_obs() if self.observationType != ObservationType.FULL else None
        glob_dev = self.global_state() if self.env_type == DynEnvType.ROBO_CUP else None  # 252 B per environment, one short launch
        rewards = self.rewards.cpu().numpy().copy()
        robocup, partial = self.env_type == DynEnvType.ROBO_CUP, self.observationType == ObservationType.PARTIAL
        flags = self.error_flags()  # ONE read per step: it is a device synchronisation and a copy of the flags
        applies = {"any": True, "robocup": robocup, "partial": partial}
        for bit, where, message in _STEP_ERRORS:  # in this order: the first bit set is the one reported
            if flags & bit and applies[where]:
                raise _capi.DynEnvError(message % self._first_env_with(bit))
        done = bool(self.last_done)
        dones = np.full((self.num_envs,), done, dtype=bool)
        # The step's observations stay in HBM (a snapshot: self.obs is rewritten by the next step) until somebody looks at them:
        # ONE device->host copy then serves obs and infos alike.  (A fresh 38 MB host buffer per step costs ~20 ms of page
        # faults at 4096 envs - more than the step.)
        dense = self._snapshot()
        step_obs = self._compat(dense, counts)
        cache = {}

        def full_np():
            if "full" not in cache:
                cache["full"] = full_dev.cpu().numpy() if full_dev is not None else (dense if self.eager_compat else step_obs._dense)[:, -1]
            return cache["full"]

        def glob_np():
            if glob_dev is None:
                return None
            if "glob" not in cache:
                cache["glob"] = glob_dev.cpu().numpy()
            return cache["glob"]
        stats = term = None
        if done:
            stats = [x.cpu().numpy() for x in self.episode_stats()]
            term = np.asarray(step_obs)  # every element: the bulk builder on the step's host copy

        def make_info(e):
            eager = {}
            if done:
                eager["episode_r"] = stats[0][e].copy()
                eager["episode_p_r"] = stats[1][e].copy()
                eager["episode_o_r"] = stats[2][e].copy() if self.env_type == DynEnvType.ROBO_CUP else [0, ] * self.n_agents
                eager["episode_g"] = [int(stats[3][e, 0]), int(stats[3][e, 1])]
                eager["terminal_observation"] = [list(term[e, t]) for t in range(self.n_time_steps)]
            return LazyInfo(lambda: self._full_states(full_np(), counts, e, glob_np()), eager)
        infos = LazyInfos(self.num_envs, make_info)
        if self.eager_compat:
            infos = tuple(infos)
        if done:
            self.terminal_obs = self.obs.clone()
            return self.reset(), rewards, dones, infos  # SubprocVecEnv worker semantics (subproc_vec_env.py:19-22)
        return step_obs, rewards, dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def seed(self, seed=None):
        """Working replacement for SubprocVecEnv.seed (which calls a non-existent env.seed, quirk C5); env_method("set_random_seed", s)
        is this call.  Every environment draws from `seed` from now on (dynenv_seed): the next reset's scene, and - mid-episode - the
        step-time draws of the running one (pedestrian moves, dice, observation noise).  No state blob changes; a later checkpoint()
        carries the new seed, restore() brings back the checkpoint's.
        Once a step_flat() / reset_envs() of this handle has been captured into a graph the seed is frozen: a replay draws from the seed
        it was captured with.  seed() with any other value raises DynEnvError then and changes nothing; make a new handle."""
        _capi.check(self._lib.dynenv_seed(self._h, int(seed if seed is not None else 0)), "dynenv_seed")
        return [seed] * self.num_envs

    def _get_indices(self, indices):
        if indices is None:
            return list(range(self.num_envs))
        if isinstance(indices, int):
            return [indices]
        return list(indices)

    def get_attr(self, attr_name, indices=None):
        idx = self._get_indices(indices)
        if not hasattr(self, attr_name):
            raise AttributeError(attr_name)
        return [getattr(self, attr_name) for _ in idx]

    def set_attr(self, attr_name, value, indices=None):
        setattr(self, attr_name, value)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        idx = self._get_indices(indices)
        if method_name == "get_agent_locs":
            o = self.full_state_obs().cpu().numpy()  # getFullState(agent): the true state, whatever the observation type
            if self.env_type == DynEnvType.ROBO_CUP:  # RoboCupEnvironment.py:434-435: self rows [:, 0:6]
                return [[o[e, a, 4:10].reshape(1, 6).copy() for a in range(self.n_agents)] for e in idx]
            # DrivingEnvironment.py:126-127: self rows [x, y, cos, sin] per agent
            return [[o[e, a, 0:4].reshape(1, 4).copy() for a in range(self.n_agents)] for e in idx]
        if method_name == "set_random_seed":
            return self.seed(*method_args)
        raise NotImplementedError(method_name)

    def render(self, *a, **k):
        return None

    def get_images(self, *a, **k):
        """base_vec_env.py:174-178: the rendered frames of the sub-environments.  Rendering (pygame) is outside the step path."""
        raise NotImplementedError("rendering is not part of the batched step path (SURVEY.md section 2: out of scope)")

    @property
    def unwrapped(self):  # base_vec_env.py:203-208
        return self

    def close(self):
        if not self.closed and self._h:
            self._lib.dynenv_destroy(self._h)
            self._h = None
            self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_dyn_env(env, num_envs, num_players, render, observationType, noiseType, noiseMagnitude,
                 use_continuous_actions, **kwargs):
    """Drop-in for DynEnv.make_dyn_env (DynEnv/__init__.py:6-25): returns (vec_env, name)."""
    if render:
        raise NotImplementedError("rendering (pygame/cv2) is out of scope; use render=False")
    if env is DynEnvType.ROBO_CUP or env == DynEnvType.ROBO_CUP:
        name = "RoboCup"
    elif env is DynEnvType.DRIVE or env == DynEnvType.DRIVE:
        name = "Driving"
    else:
        raise ValueError
    venv = BatchedDynEnv(DynEnvType(env), num_envs, num_players, observationType, noiseType, noiseMagnitude,
                         use_continuous_actions, **kwargs)
    return venv, name
