"""What the tests of the per-environment device calls share - the batched state transfer, the masked reset, the masked step, the
exact save / restore, the RNG key tests and tests/golden/gen_state_digests.py: ONE table of configurations, the handles and oracles
made from it, the random actions, the bit views everything is compared through, the situations with live contacts ("piles"), the
staggered batch, and the checkpoint comparison that leaves Driving Partial's timing word out.  A helper module: no test in here.

The oracle has no per-environment reset or step and gets none.  Its environments are independent, though: OracleEnv(num_envs=1,
env_id_offset=e, seed=...) IS environment e of a batch (env_oracle), and resetting that object k times puts it into episode k."""
import collections
import warnings

import numpy as np

import capacity_scenes as cs
import oracle_lib as ol

# env_type: the oracle's (0 RoboCup, 1 Driving); highs: the actions' exclusive upper bounds; partial: Partial observations with
# Realistic noise of magnitude 3; steps: how long a step test of the RNG key tests runs
Cfg = collections.namedtuple("Cfg", "env_type players highs partial flags steps")
_DRV, _RC, _DEF = (3, 3), (5, 3, 3, 7), ol.ROBOCUP_DEFAULT_FLAGS
# (name, the RNG key tests' name for it, record).  robocup5_random (randomInit + deterministicTurn: the other half of
# rc_reset_masked_kernel) and rc5r (randomInit alone) are two configurations.
_TABLE = (
    ("driving10", "drv10", Cfg(1, 10, _DRV, False, 0, 12)),
    ("driving2", "drv2", Cfg(1, 2, _DRV, False, 0, 12)),
    ("robocup5", "rc5", Cfg(0, 5, _RC, False, _DEF, 40)),
    ("robocup1", None, Cfg(0, 1, _RC, False, _DEF, 40)),
    ("driving_partial", "drvp", Cfg(1, 10, _DRV, True, 0, 12)),
    ("robocup_partial", "rcp", Cfg(0, 5, _RC, True, _DEF, 12)),
    ("robocup5_random", None, Cfg(0, 5, _RC, False, _DEF | ol.FLAG_RANDOM_INIT | ol.FLAG_DETERMINISTIC_TURN, 40)),
    (None, "rc5r", Cfg(0, 5, _RC, False, _DEF | ol.FLAG_RANDOM_INIT, 40)),
)
CFGS = {name: c for long, short, c in _TABLE for name in (long, short) if name}   # every name, long or short -> its record
NAMES = tuple(long for long, _, _ in _TABLE if long)   # the configurations of the masked reset, the masked step and the exact transfer


def cfg_of(cfg):
    """a configuration's record: `cfg` is a name of the table or - for a test module that has configurations of its own - the record"""
    return cfg if isinstance(cfg, Cfg) else CFGS[cfg]


def select(*names):
    """name -> record of the listed configurations, in that order: the table a test module parametrizes over"""
    return {n: CFGS[n] for n in names}


def driving(cfg):
    return cfg_of(cfg).env_type == 1


def agents(cfg):
    return cfg_of(cfg).players * (1 if driving(cfg) else 2)


def sub(cfg):   # `elapsed` per step, and the episode's length in it
    return (10, 6000) if driving(cfg) else (50, 12000)


PILE_CFGS = [c for c in NAMES if agents(c) == 10]   # the ten agents the pile scenes need
# name: (E, the listed set M): E = 70 with every third environment plus 63 and 64 (both sides of a 64 boundary)
SHAPES = {"E1": (1, [0]), "E5": (5, [3, 0, 4]), "E70": (70, sorted(set(range(0, 70, 3)) | {63, 64}))}
CASES = [(c, s) for c in NAMES for s in SHAPES]
HISTORY = 40   # steps every handle runs before anything is read or written: mid-episode, contacts cached, pedestrians under way
SEED = 31
SENTINEL = 0x5EA71E55   # the int32 pattern obs is pre-filled with where no byte of it may change


# ------------------------------------------------------------------------------------------------ handles, oracles, actions
def make(cfg, E, seed=SEED, off=0, **kw):
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    c = cfg_of(cfg)
    if c.partial:
        kw.update(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=3)
    return BatchedDynEnv(DynEnvType.DRIVE if c.env_type == 1 else DynEnvType.ROBO_CUP, E, c.players, seed=seed, env_id_offset=off, flags=c.flags, **kw)


def oracle(cfg, E, seed=SEED, off=0, **kw):
    """the oracle of a batch of E environments (kw: threads)"""
    c = cfg_of(cfg)
    if c.partial:
        kw.update(obs_type=1, noise_type=1, noise_magnitude=3.0)
    return ol.OracleEnv(env_type=c.env_type, num_envs=E, n_players=c.players, seed=seed, env_id_offset=off, flags=c.flags, **kw)


def env_oracle(cfg, e, seed=SEED):
    """environment e of a batch, as an oracle of its own"""
    return oracle(cfg, 1, seed, off=e)


def pile_envs(cfg, E):
    return list(range(min(2, E))) if cfg in PILE_CFGS else []


def _idle(cfg, a, envs):
    """the environments that hold a pile take no action"""
    for e in envs:
        if driving(cfg):
            a[e] = 1
        else:
            a[e] = 0
            a[e, :, 3] = 3
    return a


def actions(cfg, E, A, steps, seed, idle=()):
    """[steps] of int32 [E, A, K], uniformly random in the action space; the environments in `idle` take no action"""
    rng = np.random.default_rng(seed)
    return [_idle(cfg, np.stack([rng.integers(0, h, (E, A)) for h in cfg_of(cfg).highs], -1).astype(np.int32), idle) for _ in range(steps)]


def step(env, a, **kw):
    import torch
    return env.step_flat(torch.tensor(a, device="cuda"), **kw)


# ------------------------------------------------------------------------------------------------ bit views
def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def bits32(x):
    """float32 values (a tensor or an array) as their int32 bit patterns"""
    return np.ascontiguousarray(_host(x), dtype=np.float32).view(np.int32)


def bits64(x):
    """float64 values (a tensor or an array) as their int64 bit patterns"""
    return np.ascontiguousarray(_host(x), dtype=np.float64).view(np.int64)


def same_f32(a, b):
    return np.array_equal(bits32(a), bits32(b))


def same_f64(a, b):
    return np.array_equal(bits64(a), bits64(b))


# ------------------------------------------------------------------------------------------------ situations
def write_pile(cfg, st, step):
    (cs.drv_full_coupled if driving(cfg) else cs.rc_chain)(st)
    st.elapsed = step * sub(cfg)[0]
    return st


def situation(cfg, E, **kw):
    """a handle HISTORY + 2 steps into its first episode whose pile environments hold live contacts (the same for the same arguments):
    capacity_scenes.drv_full_coupled / rc_chain written into environments 0 and 1 of the configurations that have the ten agents the
    scenes need, and stepped twice"""
    env = make(cfg, E, **kw)
    env.reset_flat()
    piles = pile_envs(cfg, E)
    blank = {e: env.get_state(e) for e in piles}
    for a in actions(cfg, E, env.n_agents, HISTORY, 5):
        step(env, a, auto_reset=False)
    for e in piles:
        env.set_state(e, write_pile(cfg, blank[e], HISTORY))
    for a in actions(cfg, E, env.n_agents, 2, 6, idle=piles):
        step(env, a, auto_reset=False)
    return env


def staggered(cfg, E, **kw):
    """a per_env handle whose environment e ends after 1 + e % 4 steps: blobs from step HISTORY with `elapsed` edited, written with ONE
    set_states that needs no episode_step and warns about nothing.  -> (handle, the blobs as uint8 [E, state_size])"""
    from dynenv_amd import _capi
    env = make(cfg, E, episodes="per_env", **kw)
    env.reset_flat()
    for a in actions(cfg, E, env.n_agents, HISTORY, 5):
        step(env, a, auto_reset=False)
    blobs = env.get_states().cpu().numpy()
    view = _capi.blobs_as_states(blobs, env.env_type)
    per_step, end = sub(cfg)
    for e in range(E):
        view["elapsed"][e] = end - (1 + e % 4) * per_step
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert env.set_states(None, blobs).cpu().tolist() == [0] * E
    return env, blobs


# ------------------------------------------------------------------------------------------------ the batched state transfer's handles
# name: (E, listed environments; None = all of them, in order): E = 5 with a permuted subset, E = 70 with every environment (more than
# one 64-wide block of the per-environment kernels; the random resets give the environments differing pedestrian and obstacle counts)
STATE_SHAPES = {"E1": (1, [0]), "E5_subset": (5, [3, 0, 4]), "E70_all": (70, None)}
STATE_CASES = [(c, s) for c in NAMES[:6] for s in STATE_SHAPES]
DONOR_SEED = 977


def started(cfg, E, seed, act_seed=5):
    """a handle HISTORY steps into its first episode (the same history for the same arguments)"""
    env = make(cfg, E, seed)
    env.reset_flat()
    for a in actions(cfg, E, env.n_agents, HISTORY, act_seed):
        step(env, a, auto_reset=False)
    return env


def donor_blobs(cfg, E, ids):
    """mid-episode states of a third run, read one by one with get_state: (ctypes structs, uint8 [n, state_size]); blob k
    comes from environment (3 k + 1) % E of the donor, so that a batched write that ignored its index list would not pass"""
    donor = started(cfg, E, DONOR_SEED, act_seed=9)
    sts = [donor.get_state((3 * k + 1) % E) for k in range(len(ids))]
    donor.close()
    return sts, np.stack([np.frombuffer(bytes(s), np.uint8) for s in sts])


def listed_ids(E, listed):
    return list(range(E)) if listed is None else list(listed)


# ------------------------------------------------------------------------------------------------ checkpoints
# Driving's checkpointed arrays in allocation order (csrc/driving_tu.hip: init), as (fields, slots per environment, bytes per element);
# envi is the sixth: EI_COUNT = 19 ints an environment, EI_DEFER_OBS the last of them (csrc/driving_dev.h)
DRV_NB, DRV_EI_COUNT, DRV_EI_DEFER_OBS, CKPT_HEADER = 32, 19, 18, 80
DRV_ARRAYS = (("body", 9, DRV_NB, 8), ("carx", 6, 16, 8), ("flags", 1, DRV_NB, 4), ("aux", 1, DRV_NB, 4), ("obst", 2, 20, 8),
              ("envi", 1, DRV_EI_COUNT, 4), ("epr", 2, 16, 8), ("s_pair", 1, cs.DRV_NS, 4), ("s_meta", 1, cs.DRV_NS, 4),
              ("s_hash", 2, cs.DRV_NS, 4), ("s_imp", 4, cs.DRV_NS, 8), ("lastcand", 1, 64, 4))
RC_PAIRTAB_BYTES = 64 * 2 * 8   # RoboCup's constant pair table: the last array of its checkpoint, no row of any environment


def ckpt(env):
    """checkpoint() - every device array of the handle that is simulation state - as uint8.  For Driving PARTIAL handles one word of it
    is not state and is left out: envi[EI_DEFER_OBS] says how many of the agents' Partial observations the STEP launch got done before
    its forecast end and how many it left to the deferred launch.  It is scheduling scratch that lives in a checkpointed row, depends
    on timing once an environment is on the contact path - the piles are - and is neither read nor written by either reset.  Every
    other configuration is compared whole."""
    from dynenv_amd import ObservationType
    c = env.checkpoint().copy()
    if int(env.env_type) == 1 and env.observationType == ObservationType.PARTIAL:
        E = env.num_envs
        size = {name: f * n * b * E for name, f, n, b in DRV_ARRAYS}
        assert c.size == CKPT_HEADER + sum(size.values()), "the checkpoint's layout changed: find envi again"
        off = CKPT_HEADER + sum(size[name] for name, _, _, _ in DRV_ARRAYS[:5])
        c[off:off + size["envi"]].view(np.int32).reshape(E, DRV_EI_COUNT)[:, DRV_EI_DEFER_OBS] = 0
    return c


def ckpt_diff(a, b):
    ca, cb = ckpt(a), ckpt(b)
    diff = np.nonzero(ca != cb)[0]
    return "" if diff.size == 0 else "checkpoints differ in %d bytes, first at offset %d of %d" % (diff.size, diff[0], ca.size)
