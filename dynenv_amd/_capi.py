"""ctypes binding of include/dynenv.h (libdynenv_hip.so).  No fallback: a missing library or GPU raises."""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DYNENV_HIP_LIB", os.path.join(PKG, "libdynenv_hip.so"))  # override: A/B builds only

DYNENV_ABI_VERSION = 3
ERR_NO_DEVICE = -2


class DynEnvError(RuntimeError):
    pass


class Cfg(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("env_type", C.c_int32), ("num_envs", C.c_int32),
                ("n_players", C.c_int32), ("obs_type", C.c_int32), ("noise_type", C.c_int32),
                ("noise_magnitude", C.c_double), ("seed", C.c_uint64), ("env_id_offset", C.c_int32),
                ("flags", C.c_int32), ("device_id", C.c_int32), ("reserved", C.c_int32)]


class Layout(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("n_agents", C.c_int32), ("n_time_steps", C.c_int32),
                ("obs_dim", C.c_int32), ("action_dim", C.c_int32), ("n_blocks", C.c_int32),
                ("block_offset", C.c_int32 * 8), ("block_rows", C.c_int32 * 8), ("block_feat", C.c_int32 * 8),
                ("steps_per_episode", C.c_int32), ("reserved", C.c_int32)]


CAR_F = ("px", "py", "vx", "vy", "angle", "w", "dirx", "diry", "prevx", "prevy", "goalx", "goaly")
CAR_I = ("type", "team", "finished", "crashed", "lane_pos", "fric")
PED_F = ("px", "py", "vx", "vy")
PED_I = ("road", "side", "dead", "moving", "speed", "crossing", "begin_crossing")


class CarState(C.Structure):
    _fields_ = [(n, C.c_double) for n in CAR_F] + [(n, C.c_int32) for n in CAR_I] + [("pad", C.c_int32 * 2)]


class PedState(C.Structure):
    _fields_ = [(n, C.c_double) for n in PED_F] + [(n, C.c_int32) for n in PED_I] + [("pad", C.c_int32)]


class DrivingState(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("elapsed", "all_finished", "n_cars", "n_peds", "n_obst", "episode")] + \
               [("pad", C.c_int32 * 2), ("episode_r", C.c_double * 10), ("episode_pos_r", C.c_double * 10),
                ("cars", CarState * 10), ("peds", PedState * 20), ("obst_x", C.c_double * 20),
                ("obst_y", C.c_double * 20)]


ROBOT_F = ("lpx", "lpy", "lvx", "lvy", "la", "lw", "rpx", "rpy", "rvx", "rvy", "ra", "rw", "head_angle", "head_moving",
           "prevx", "prevy", "initx", "inity", "penal_time", "fall_time", "move_time")
ROBOT_I = ("team", "penalized", "touching", "touch_cntr", "might_push", "fallen", "fall_cntr", "kicking", "foot",
           "joint_removed")


class RobotState(C.Structure):
    _fields_ = [(n, C.c_double) for n in ROBOT_F] + [(n, C.c_int32) for n in ROBOT_I] + [("pad", C.c_int32 * 2)]


class RoboCupState(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("elapsed", "n_robots", "ball_owned", "n_last_kicked")] + \
               [("last_kicked", C.c_int32 * 4), ("goals", C.c_int32 * 2), ("closest", C.c_int32 * 2),
                ("n_def", C.c_int32 * 2), ("defenders", (C.c_int32 * 10) * 2), ("episode", C.c_int32),
                ("pad", C.c_int32), ("ball_free_cntr", C.c_double), ("grace_period", C.c_double),
                ("penal_times", C.c_double * 2)] + \
               [(n, C.c_double) for n in ("bpx", "bpy", "bvx", "bvy", "bw", "bprevx", "bprevy")] + \
               [("episode_r", C.c_double * 10), ("episode_pos_r", C.c_double * 10), ("robots", RobotState * 10)]


FLAG_RANDOM_INIT, FLAG_DETERMINISTIC_TURN, FLAG_CAN_FALL, FLAG_USE_OBS_REWARDS, FLAG_ALLOW_HEAD_TURN = 1, 2, 4, 8, 16

ARR_MAX_TYPES = 4
ARR_COUNT_CONST, ARR_COUNT_ENV, ARR_COUNT_ROW = 0, 1, 2
ARR_F32, ARR_BF16, ARR_F16 = 0, 1, 2  # DYNENV_ARR_F32 / _BF16 / _F16: the element types of dynenv_arrange_*_as
ERR_UNSUPPORTED = -4
RETURNS_REFERENCE, RETURNS_DONES, RETURNS_GAE = 0, 1, 2  # DYNENV_RETURNS_*: the modes of dynenv_rollout_returns


class ArrType(C.Structure):  # dynenv_arr_type_t
    _fields_ = [("offset", C.c_int32), ("feat", C.c_int32), ("cap", C.c_int32), ("count_mode", C.c_int32),
                ("count_value", C.c_int32), ("count_index", C.c_int32), ("count_stride", C.c_int32),
                ("reserved", C.c_int32)]


class ArrPlan(C.Structure):  # dynenv_arr_plan_t
    _fields_ = [("n_types", C.c_int32), ("n_time", C.c_int32), ("n_players", C.c_int32), ("max_count", C.c_int32),
                ("total", C.c_int64 * ARR_MAX_TYPES)]


class EmbedBlock(C.Structure):  # dynenv_embed_block_t: device pointers of one EmbedBlock's six float32 parameters
    _fields_ = [(n, C.c_void_p) for n in ("w1", "ln1_w", "ln1_b", "w2", "ln2_w", "ln2_b")]


class Mha(C.Structure):  # dynenv_mha_t: device pointers of one nn.MultiheadAttention(F, 1, add_bias_kv=True); the first four 16 bit, the last two float32
    _fields_ = [(n, C.c_void_p) for n in ("in_w", "out_w", "bias_k", "bias_v", "in_b", "out_b")]


class Rhead(C.Structure):  # dynenv_rhead_t: device pointers of the recurrent head; tr_w, w_ih and w_hh 16 bit, the rest float32
    _fields_ = [(n, C.c_void_p) for n in ("tr_w", "tr_b", "tr_ln_w", "tr_ln_b", "w_ih", "w_hh", "b_ih", "b_hh", "ln_w", "ln_b")]


class Policy(C.Structure):  # dynenv_policy_t: device pointers of the policy head; actor_w and critic_w1 16 bit, the rest float32
    _fields_ = [(n, C.c_void_p) for n in ("actor_w", "actor_b", "cont_scale", "cont_mean", "critic_w1", "critic_b1", "critic_ln_w", "critic_ln_b",
                                          "critic_w2", "critic_b2")]


class PolicyBwd(C.Structure):  # dynenv_policy_bwd_t: the transposed bf16 copies the products of dynenv_policy_eval_backward read
    _fields_ = [(n, C.c_void_p) for n in ("actor_w_t", "critic_w1_t", "actor_w_t_lo", "critic_w1_t_lo")]


class PolicyGrad(C.Structure):  # dynenv_policy_grad_t: float32 device pointers of the eight gradients, in the packed operands' layouts
    _fields_ = [(n, C.c_void_p) for n in ("d_actor_w", "d_actor_b", "d_critic_w1", "d_critic_b1", "d_critic_ln_w", "d_critic_ln_b", "d_critic_w2",
                                          "d_critic_b2")]


class IcmBwd(C.Structure):  # dynenv_icm_bwd_t: the transposed 16-bit copies the backward's products read
    _fields_ = [(n, C.c_void_p) for n in ("fwd_w2_t", "fwd_w1_t", "inv_w_t")]


class IcmGrad(C.Structure):  # dynenv_icm_grad_t: float32 device pointers of the seven gradients, in the packed operands' layouts
    _fields_ = [(n, C.c_void_p) for n in ("d_fwd_w1", "d_fwd_w1_act", "d_fwd_b1", "d_fwd_w2", "d_fwd_b2", "d_inv_w", "d_inv_b")]


class Icm(C.Structure):  # dynenv_icm_t: device pointers of the curiosity module; fwd_w1, fwd_w2 and inv_w 16 bit, the rest float32
    _fields_ = [(n, C.c_void_p) for n in ("fwd_w1", "fwd_w1_act", "fwd_b1", "fwd_w2", "fwd_b2", "inv_w", "inv_b")]


vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t

# THE binding of include/dynenv.h: name -> (restype, argtypes), in the header's order of growth.  load() sets exactly these, so an entry
# point cannot be exported without its argument types (a missing list would truncate pointers to int); tests/test_host_and_abi.py
# holds every line against the header's prototype.
SIGNATURES = {
    "dynenv_abi_version": (C.c_int, []),
    "dynenv_last_error": (C.c_char_p, []),
    "dynenv_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(vp)]),
    "dynenv_destroy": (None, [vp]),
    "dynenv_layout": (C.c_int, [vp, C.POINTER(Layout)]),
    "dynenv_seed": (C.c_int, [vp, C.c_uint64]),
    "dynenv_reset": (C.c_int, [vp, vp, vp]),
    "dynenv_step": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "dynenv_counts": (C.c_int, [vp, vp, vp]),
    "dynenv_episode_stats": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "dynenv_state_size": (sz, [vp]),
    "dynenv_get_state": (C.c_int, [vp, i32, vp, sz]),
    "dynenv_set_state": (C.c_int, [vp, i32, vp, sz]),
    "dynenv_sync": (C.c_int, [vp, vp]),
    "dynenv_math_selftest": (C.c_int, [vp, vp, i32, vp, i32]),
    "dynenv_error_flags": (C.c_int, [vp, C.POINTER(i32)]),
    "dynenv_debug_counters": (C.c_int, [vp, C.POINTER(i64)]),
    "dynenv_debug_placement": (C.c_int, [vp, vp, i32]),
    "dynenv_arrange_scratch_ints": (i64, [i32, i32, i32, i32]),
    "dynenv_arrange_plan": (C.c_int, [vp, i32, i32, i32, i32, C.POINTER(ArrType), i32, vp, vp, vp, vp, vp, C.POINTER(ArrPlan), vp]),
    "dynenv_arrange_gather": (C.c_int, [vp, i32, i32, i32, i32, C.POINTER(ArrType), i32, vp, vp, i32, C.POINTER(vp), C.POINTER(vp), vp, vp]),
    "dynenv_arrange_scatter": (C.c_int, [vp, vp, i64, i32, vp, vp]),
    "dynenv_arrange_pad": (C.c_int, [C.POINTER(vp), vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "dynenv_arrange_pad_backward": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp), vp]),
    "dynenv_arrange_scatter_backward": (C.c_int, [vp, vp, i64, i32, vp, vp]),
    "dynenv_checkpoint_size": (sz, [vp]),
    "dynenv_checkpoint_save": (C.c_int, [vp, vp, sz]),
    "dynenv_checkpoint_load": (C.c_int, [vp, vp, sz]),
    "dynenv_obs_pack": (C.c_int, [vp, i64, i32, i32, i32, vp, vp]),
    "dynenv_obs_unpack": (C.c_int, [vp, i64, i32, i32, i32, vp, vp]),
    "dynenv_obs_unpack_ranks": (C.c_int, [vp, i64, i32, i64, i32, i32, i32, vp, vp]),
    "dynenv_obs_pack_peers": (C.c_int, [vp, i64, i32, i32, vp, vp]),
    "dynenv_obs_unpack_peers_ranks": (C.c_int, [vp, i64, i32, i64, i32, i32, vp, vp]),
    "dynenv_step_head": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
    "dynenv_full_obs": (C.c_int, [vp, vp, vp]),
    "dynenv_full_obs_dim": (C.c_int, [vp]),
    "dynenv_global_state": (C.c_int, [vp, vp, vp]),
    "dynenv_global_state_dim": (C.c_int, [vp]),
    "dynenv_set_step_events": (C.c_int, [vp, vp, vp, vp]),
    "dynenv_get_states": (C.c_int, [vp, vp, i32, vp, vp]),
    "dynenv_set_states": (C.c_int, [vp, vp, i32, vp, vp, vp]),
    "dynenv_error_flags_env": (C.c_int, [vp, vp, vp]),
    "dynenv_reset_masked": (C.c_int, [vp, vp, vp, vp]),
    "dynenv_step_masked": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "dynenv_exact_size": (sz, [vp]),
    "dynenv_get_exact": (C.c_int, [vp, vp, i32, vp, vp]),
    "dynenv_set_exact": (C.c_int, [vp, vp, i32, vp, vp, vp]),
    "dynenv_arrange_fixed_gather": (C.c_int, [vp, i32, i32, i32, i32, C.POINTER(ArrType), i32, vp, C.POINTER(i32), i32, vp, vp, C.POINTER(vp), vp, vp, vp]),
    "dynenv_arrange_fixed_pad": (C.c_int, [C.POINTER(vp), vp, C.POINTER(i32), i32, i32, i32, i32, i32, vp, vp]),
    "dynenv_arrange_fixed_pad_backward": (C.c_int, [vp, vp, C.POINTER(i32), i32, i32, i32, i32, i32, C.POINTER(vp), vp]),
    "dynenv_math_probe": (C.c_int, [i32, vp, i32, vp, i32]),
    "dynenv_arrange_pad_as": (C.c_int, [C.POINTER(vp), i32, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp]),
    "dynenv_arrange_pad_backward_as": (C.c_int, [vp, i32, vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp), i32, vp]),
    "dynenv_arrange_fixed_pad_as": (C.c_int, [C.POINTER(vp), i32, vp, C.POINTER(i32), i32, i32, i32, i32, i32, vp, i32, vp]),
    "dynenv_arrange_fixed_pad_backward_as": (C.c_int, [vp, i32, vp, C.POINTER(i32), i32, i32, i32, i32, i32, C.POINTER(vp), i32, vp]),
    "dynenv_arrange_embed_pad": (C.c_int, [vp, i32, i32, i32, i32, C.POINTER(ArrType), i32, vp, i32, C.POINTER(EmbedBlock), i32, C.c_float, C.c_float,
                                           vp, i32, vp]),
    "dynenv_attend_pool": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, C.POINTER(Mha), C.POINTER(Mha), vp, vp, C.c_float, vp, vp, vp, vp]),
    # (the two of the rollout storage and the curiosity module's stand in front of the two heads: tests/test_policy_host.py pins the last
    # two names of the table)
    "dynenv_rollout_insert": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                        vp, vp]),
    "dynenv_rollout_returns": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, vp, vp, vp]),
    "dynenv_icm_losses": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, C.POINTER(i32), i32, i32, C.POINTER(Icm), C.c_float, vp, vp, vp, vp, vp]),
    "dynenv_icm_backward_workspace": (C.c_int, [i32, i32, C.POINTER(C.c_uint64)]),
    "dynenv_icm_backward": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, C.POINTER(i32), i32, i32, C.POINTER(Icm), C.c_float, vp, vp, C.POINTER(IcmBwd),
                                      C.POINTER(IcmGrad), vp, vp, C.c_uint64, vp, vp]),
    "dynenv_policy_eval": (C.c_int, [vp, vp, i32, i32, i32, i32, C.POINTER(Policy), C.POINTER(i32), i32, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
    "dynenv_policy_eval_backward_workspace": (C.c_int, [i32, i32, C.POINTER(C.c_uint64)]),
    "dynenv_policy_eval_backward": (C.c_int, [vp, vp, i32, i32, i32, i32, C.POINTER(Policy), C.POINTER(i32), i32, i32, C.c_float, C.c_float, vp, vp, vp,
                                              C.POINTER(PolicyBwd), C.POINTER(PolicyGrad), vp, vp, C.c_uint64, vp, vp]),
    "dynenv_recurrent_head": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, C.POINTER(Rhead), C.c_float, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
    "dynenv_policy_head": (C.c_int, [vp, vp, i32, i32, i32, i32, C.POINTER(Policy), C.POINTER(i32), i32, i32, i32, C.c_uint64, vp, C.c_uint64,
                                     C.c_float, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp]),
}
EXPORTS = list(SIGNATURES)

ERR_BAD_BLOB = 64  # error bit 6: a blob given to dynenv_set_states / dynenv_set_exact did not fit the handle and was not written
SET_WRITTEN, SET_REJECTED, SET_BAD_INDEX = 0, 1, 2  # the per-blob status of dynenv_set_states and dynenv_set_exact


def state_struct(env_type):
    """The ctypes struct of an environment type's canonical state blob (DynEnvType or its int: 0 RoboCup, 1 Driving)."""
    return DrivingState if int(env_type) == 1 else RoboCupState


def state_dtype(env_type):
    """The numpy structured dtype of the blob - np.dtype of the ctypes struct, so offsets, pads and the item size are the C compiler's:
    fields are edited with numpy (`blobs["cars"]["px"][:, 0] += 1`) instead of ctypes."""
    import numpy as np
    return np.dtype(state_struct(env_type))


def blobs_as_states(blobs, env_type):
    """uint8 [n, state_size] (or one blob [state_size]) -> structured array [n] (or [1]) of state_dtype(env_type): a view of the same
    memory when `blobs` is C-contiguous, so edits land in it."""
    import numpy as np
    dt = state_dtype(env_type)
    b = np.ascontiguousarray(blobs, dtype=np.uint8)
    if b.ndim not in (1, 2) or b.shape[-1] != dt.itemsize:
        raise ValueError("expected uint8 [n, %d], got %s" % (dt.itemsize, (b.shape,)))
    return b.reshape(-1, dt.itemsize).view(dt).reshape(-1)


def states_as_blobs(states):
    """structured array [n] of a state_dtype (or a ctypes DrivingState / RoboCupState, or a list of them) -> uint8 [n, state_size]: a
    view for a contiguous structured array, a copy for ctypes structs."""
    import numpy as np
    if isinstance(states, C.Structure):
        states = [states]
    if isinstance(states, (list, tuple)):
        return np.stack([np.frombuffer(bytes(s), dtype=np.uint8) for s in states]) if len(states) else np.zeros((0, 0), np.uint8)
    a = np.ascontiguousarray(states)
    return a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)

_lib = None


def load():
    """Load the HIP library; raises if it has not been built (there is no Python/CPU substitute)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DynEnvError("libdynenv_hip.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(dynenv_amd has no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        if not hasattr(lib, name):
            raise DynEnvError("libdynenv_hip.so does not export " + name)
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        if restype is not C.c_int:  # (ctypes' default, and faster left unset: ~50 ns a call, which step_flat's host cost shows)
            fn.restype = restype
    if lib.dynenv_abi_version() != DYNENV_ABI_VERSION:
        raise DynEnvError("ABI version mismatch between dynenv_amd and libdynenv_hip.so")
    _lib = lib
    return lib


def ptr(t):
    """c_void_p of a tensor's data; None (an optional argument left out) stays None, the C side's NULL"""
    return None if t is None else C.c_void_p(t.data_ptr())


def check(rc, what):
    if rc != 0:
        msg = load().dynenv_last_error().decode("utf-8", "replace")
        raise DynEnvError("%s failed (%d): %s" % (what, rc, msg))
