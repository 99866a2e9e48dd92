"""What tests/test_rng_key_oracle.py (CPU) and tests/test_gpu_rng_key.py (-m gpu) share on top of tests/per_env_common.py: the key tuples,
the six configurations they run in, an independent Philox4x32-10 with the key derivation of include/dynenv_math.h's dm_env_rng, blob helpers and the twin experiment.
No test in here.

Every random draw of both environments is dm_env_rng(seed, genv, episode, purpose, entity, t)
  = philox4x32-10(key = (seed_lo, seed_hi ^ (genv * 0x9E3779B1 + 0x7F4A7C15)), counter = (episode, purpose, entity, t)),
and the oracle calls the same function as the kernels: the two can only disagree in the WORDS they hand to it.  The key tuples put
every one of those words where a 32-bit habit would break it: a seed with a high word, a global id with bit 16 / bit 30 set, an
episode counter past 16 and 24 bits and at the top of int32.

The twin experiment is what keeps all of that from being vacuous: two simulators that get the SAME bodies (set_state of one blob) and
differ in ONE key word must part ways - else a test that runs "at a key" would pass whatever the kernel did with that word."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import per_env_common as pc
from per_env_common import bits32, bits64, driving  # noqa: F401  (the tests of both files reach them as rk.*)

E = 32
M32 = 0xFFFFFFFF

# name: (seed, env_id_offset, episode written into every blob before the reset or None)
KEYS = {
    "K1": (42 + 2 ** 32, 0, None),
    "K2": (2 ** 64 - 1, 0, None),
    "K3": (0x8000000080000000, 65520, None),     # the batch straddles global ids 65535 | 65536
    "K4": (0, 2 ** 31 - E, None),                # the last global id is 2^31 - 1: the largest for which env_id_offset + e is defined
    "K5": (42, 0, 65535),                        # the reset draws at episode 65535, the steps at 65536
    "K6": (2 ** 33 + 7, 0, 2 ** 24),
    "K7": (42, 0, 2 ** 31 - 2),                  # the reset makes the counter 2^31 - 1; nothing lets it pass that
}
HIGH_WORD_KEYS = [k for k, v in KEYS.items() if v[0] >> 32]

CFGS = pc.select("drv10", "drv2", "drvp", "rc5", "rc5r", "rcp")   # (tests/per_env_common.py's records under their short names)


def steps_of(cfg):
    return CFGS[cfg].steps


# ------------------------------------------------------------------------------------------------ Philox4x32-10, from its definition
def philox4x32_10(key, ctr):
    """Random123's philox4x32-10 on Python integers: ten rounds of two 32 x 32 -> 64 multiplies (M0 = 0xD2511F53 on counter word 0,
    M1 = 0xCD9E8D57 on word 2), out = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), the key bumped by the Weyl constants 0x9E3779B9 /
    0xBB67AE85 between rounds (not after the last)."""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return (c0, c1, c2, c3)


def env_rng(seed, genv, episode, purpose, entity, t):
    """dm_env_rng's key derivation, restated"""
    key = (seed & M32, ((seed >> 32) & M32) ^ ((genv * 0x9E3779B1 + 0x7F4A7C15) & M32))
    return philox4x32_10(key, (episode & M32, purpose & M32, entity & M32, t & M32))


def oracle_env_rng(seed, genv, episode, purpose, entity, t):
    out = np.zeros(4, np.uint32)
    ol.lib().oracle_env_rng(seed, genv, episode, purpose, entity, t, out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------------------------------------ simulators and blobs
def oracle(cfg, num_envs=E, seed=42, env_id_offset=0, threads=8):
    return pc.oracle(cfg, num_envs, seed, env_id_offset, threads=threads)


def actions(cfg, num_envs, steps, seed):
    """[steps] of int32 [num_envs, A, K], uniformly random in the action space"""
    return pc.actions(cfg, num_envs, pc.agents(cfg), steps, seed)


def as_states(blobs, cfg):
    """uint8 [n, state_size] -> numpy structured array [n] over the same memory (dynenv_amd._capi.blobs_as_states; loads no library)"""
    from dynenv_amd import _capi
    return _capi.blobs_as_states(blobs, CFGS[cfg][0])


def oracle_blobs(ora, cfg):
    """every environment's state blob as the device reports it: uint8 [E, state_size]; RoboCup's defender lists ascending (they are a
    set; dynenv_get_states writes them in that order, the oracle in the order they joined)"""
    rows = np.stack([np.frombuffer(bytes(ora.get_state(e)), np.uint8) for e in range(ora.E)]).copy()
    if not driving(cfg):
        v = as_states(rows, cfg)
        for e in range(ora.E):
            for t in range(2):
                k = int(v["n_def"][e, t])
                v["defenders"][e, t, :k] = np.sort(v["defenders"][e, t, :k])
    return rows


def set_oracle_blobs(ora, cfg, blobs):
    st = ol.DrivingState if driving(cfg) else ol.RoboCupState
    for e in range(ora.E):
        ora.set_state(e, st.from_buffer_copy(np.ascontiguousarray(blobs[e]).tobytes()))


def blob_diff(a, b, cfg):
    """"" if the two uint8 [n, state_size] arrays hold the same bytes, else the fields and environments that differ"""
    if np.array_equal(a, b):
        return ""
    va, vb = as_states(a, cfg), as_states(b, cfg)
    bad = []
    for name in va.dtype.names:
        x, y = np.ascontiguousarray(va[name]).reshape(len(va), -1), np.ascontiguousarray(vb[name]).reshape(len(vb), -1)
        rows = np.nonzero((x.view(np.uint8).reshape(len(va), -1) != y.view(np.uint8).reshape(len(vb), -1)).any(1))[0]
        if rows.size:
            bad.append("%s (environments %s)" % (name, rows[:6].tolist()))
    return "state blobs differ in " + ", ".join(bad)


# ------------------------------------------------------------------------------------------------ the twin experiment
TWIN_SEED, TWIN_OFFSET = 42, 0
TWIN_WORDS = ("high", "episode", "genv")   # the one key word a twin differs in: seed + 2^32, episode + 1, global id + 1
DRIVING_TWIN_STEPS, ROBOCUP_TWIN_STEPS, ROBOCUP_TWIN_MIN = 5, 40, 8


def twin_key(word):
    """(seed, env_id_offset, added to every blob's episode) of the twin that differs from (TWIN_SEED, TWIN_OFFSET, + 0) in `word`"""
    assert word in TWIN_WORDS
    return (TWIN_SEED + (2 ** 32 if word == "high" else 0), TWIN_OFFSET + (1 if word == "genv" else 0), 1 if word == "episode" else 0)


def twin_blobs(cfg, num_envs=E):
    """the bodies both twins start from: the reset scenes of the base key, uint8 [num_envs, state_size]"""
    base = oracle(cfg, num_envs, TWIN_SEED, TWIN_OFFSET)
    base.reset()
    rows = oracle_blobs(base, cfg)
    base.close()
    return rows


def bump_episode(blobs, cfg, by):
    out = blobs.copy()
    as_states(out, cfg)["episode"] += by
    return out


def first_divergence(step_a, step_b, acts):
    """step_x(a) -> that simulator's observations after one step with actions a, as a numpy array [E, ...].  Returns int [E]: the
    number of steps after which environment e's observations first differed in any bit, 0 if they never did."""
    first = None
    for s, a in enumerate(acts):
        oa, ob = bits32(step_a(a)), bits32(step_b(a))
        differ = (oa.reshape(oa.shape[0], -1) != ob.reshape(ob.shape[0], -1)).any(1)
        if first is None:
            first = np.zeros(differ.shape, np.int64)
        first[(first == 0) & differ] = s + 1
    return first


def oracle_twins(cfg, word, steps, num_envs=E):
    """the experiment on two oracles -> first_divergence"""
    blobs = twin_blobs(cfg, num_envs)
    seed, off, ep = twin_key(word)
    a, b = oracle(cfg, num_envs, TWIN_SEED, TWIN_OFFSET), oracle(cfg, num_envs, seed, off)
    a.reset()
    b.reset()
    set_oracle_blobs(a, cfg, blobs)
    set_oracle_blobs(b, cfg, bump_episode(blobs, cfg, ep))
    first = first_divergence(lambda x: a.step(x)[0], lambda x: b.step(x)[0], actions(cfg, num_envs, steps, 17))
    a.close()
    b.close()
    return first


def twins_diverge_enough(cfg, first):
    """the condition of the issue, the same on the oracle twins (CPU) and on the device twins (GPU): Driving - all environments within
    5 steps; RoboCup - at least 8 of 32 within 40 steps.  -> "" or what is missing"""
    if driving(cfg):
        n = int(((first > 0) & (first <= DRIVING_TWIN_STEPS)).sum())
        return "" if n == len(first) else "only %d of %d environments diverged within %d steps" % (n, len(first), DRIVING_TWIN_STEPS)
    n = int(((first > 0) & (first <= ROBOCUP_TWIN_STEPS)).sum())
    return "" if n >= ROBOCUP_TWIN_MIN else "only %d of %d environments diverged within %d steps" % (n, len(first), ROBOCUP_TWIN_STEPS)
