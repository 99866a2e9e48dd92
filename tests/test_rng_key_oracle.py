"""The random streams' key on the CPU: the derivation itself, the oracle's re-seeding, and that every key word matters.  No GPU.

The kernels are "bit-identical to the oracle", and both call dm_env_rng (include/dynenv_math.h): a change to the key derivation would
move every stream on both sides at once and no parity test would see it.  So the derivation is pinned here against a Philox4x32-10
written out in tests/rng_key_common.py from its definition, itself checked first against the Random123 known answers.
oracle_seed (the oracle's set_random_seed, what tests/test_gpu_rng_key.py holds dynenv_seed against) is checked against a fresh
oracle.  The twin experiment shows that the inputs of the GPU tests are not vacuous: one changed key word changes what comes out."""
import numpy as np
import pytest

import oracle_lib as ol
import rng_key_common as rk


@pytest.fixture(scope="module", autouse=True)
def _built(oracle_built):
    return oracle_built


# the Random123 kat_vectors for philox4x32-10 (the three of tests/test_detmath.py): (key, counter, output)
KATS = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
PURPOSES = range(1, 10)   # DM_RNG_RESET_AGENT .. DM_RNG_OBS_NOISE


def test_the_python_philox_passes_the_known_answers():
    for key, ctr, want in KATS:
        assert rk.philox4x32_10(key, ctr) == want


def _key_inputs():
    """(seed, genv, episode) of every key tuple of the GPU tests - the first, the last and the environments either side of a 2^16
    boundary of each batch; the episode the reset draws at and the one the steps draw at - and four hundred random ones"""
    out = []
    for seed, off, ep in rk.KEYS.values():
        envs = sorted({0, 1, rk.E - 1} | {e for e in range(rk.E) if (off + e) & 0xFFFF in (0xFFFF, 0)})
        for e in envs:
            for episode in ((0, 1) if ep is None else (ep, ep + 1)):
                out.append((seed, off + e, episode))
    for word in rk.TWIN_WORDS:
        seed, off, ep = rk.twin_key(word)
        out.append((seed, off, 1 + ep))
    rng = np.random.default_rng(2026)
    for _ in range(400):
        out.append((int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))))
    return out


def test_key_derivation_is_philox_of_the_documented_key():
    """dm_env_rng(seed, genv, episode, purpose, entity, t) = philox4x32-10(key = (seed_lo, seed_hi ^ (genv * 0x9E3779B1 + 0x7F4A7C15)),
    counter = (episode, purpose, entity, t)), with the formula applied here and the Philox of rng_key_common: every purpose at the
    keys the GPU tests run at, random purposes / entities / times on top."""
    rng = np.random.default_rng(7)
    n = 0
    for seed, genv, episode in _key_inputs():
        draws = [(p, int(rng.integers(0, 64)), int(rng.integers(0, 12000))) for p in PURPOSES]
        draws.append(tuple(int(v) for v in rng.integers(0, 2 ** 32, 3)))
        draws.append((9, 0xFFFFFFFF, 0xFFFFFFFF))
        for purpose, entity, t in draws:
            got = rk.oracle_env_rng(seed, genv, episode, purpose, entity, t)
            key = (seed & 0xFFFFFFFF, (seed >> 32) ^ ((genv * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF))
            want = rk.philox4x32_10(key, (episode, purpose, entity, t))
            assert got == want, "seed %#x genv %d episode %d purpose %d entity %d t %d" % (seed, genv, episode, purpose, entity, t)
            n += 1
    assert n == 11 * len(_key_inputs()) and len(_key_inputs()) > 400 + 3 * 2 * len(rk.KEYS)
    # ... and every word of the tuple reaches the output: flipping any one bit of seed (each half), genv or episode changes the block
    base = (rk.KEYS["K3"][0], 65535, 65535, 6, 3, 40)
    b0 = rk.oracle_env_rng(*base)
    for word, width in ((0, 64), (1, 32), (2, 32)):
        for bit in range(width):
            other = list(base)
            other[word] ^= 1 << bit
            assert rk.oracle_env_rng(*other) != b0, (word, bit)


S1, S2 = 0x0123456700000007, 0xFEDCBA9876543210   # both with a high word


@pytest.mark.parametrize("cfg", sorted(rk.CFGS))
def test_oracle_seed_then_reset_is_a_fresh_oracle(cfg):
    """OracleEnv(s1), seed(s2), reset() = OracleEnv(s2), reset(): observations, counts, every blob - and after two steps still"""
    n = 6
    a, b = rk.oracle(cfg, n, S1, 3), rk.oracle(cfg, n, S2, 3)
    a.seed(S2)
    assert np.array_equal(rk.bits32(a.reset()), rk.bits32(b.reset()))
    assert np.array_equal(a.counts(), b.counts())
    assert rk.blob_diff(rk.oracle_blobs(a, cfg), rk.oracle_blobs(b, cfg), cfg) == ""
    other = rk.oracle(cfg, n, S1, 3)
    assert not np.array_equal(rk.bits32(other.reset()), rk.bits32(b.obs)), "s1 and s2 must not draw the same scenes"
    for act in rk.actions(cfg, n, 2, 3):
        oa, ra, da = a.step(act)
        ob, rb, db = b.step(act)
        assert np.array_equal(rk.bits32(oa), rk.bits32(ob)) and np.array_equal(rk.bits64(ra), rk.bits64(rb)) and np.array_equal(da, db)
    assert rk.blob_diff(rk.oracle_blobs(a, cfg), rk.oracle_blobs(b, cfg), cfg) == ""


@pytest.mark.parametrize("cfg", sorted(rk.CFGS))
def test_oracle_seed_mid_episode_changes_no_blob(cfg):
    n = 6
    a = rk.oracle(cfg, n, S1, 3)
    a.reset()
    for act in rk.actions(cfg, n, 3, 4):
        a.step(act)
    before = rk.oracle_blobs(a, cfg)
    counts, stats = a.counts(), [x.copy() for x in a.episode_stats()]
    a.seed(S2)
    assert rk.blob_diff(rk.oracle_blobs(a, cfg), before, cfg) == ""
    assert np.array_equal(a.counts(), counts) and all(np.array_equal(x, y) for x, y in zip(a.episode_stats(), stats))


@pytest.mark.parametrize("word", rk.TWIN_WORDS)
@pytest.mark.parametrize("cfg", ["drv10", "drv2", "drvp"])
def test_one_key_word_moves_every_driving_environment_within_five_steps(cfg, word):
    """the twin experiment (rng_key_common): same bodies, one key word changed - all 32 of 32 environments differ within 5 steps"""
    first = rk.oracle_twins(cfg, word, rk.DRIVING_TWIN_STEPS)
    print("%s, %s: environments diverged by step 1..%d: %s" % (cfg, word, rk.DRIVING_TWIN_STEPS, [int((first == s).sum()) for s in range(1, 6)]))
    assert rk.twins_diverge_enough(cfg, first) == ""


@pytest.mark.parametrize("word", rk.TWIN_WORDS)
@pytest.mark.parametrize("cfg", ["rc5", "rc5r"])
def test_one_key_word_moves_a_quarter_of_the_robocup_environments_within_forty_steps(cfg, word):
    """... at least 8 of 32 RoboCup environments (5 a side) within 40 steps: its step-time draws are dice that most steps do not roll"""
    first = rk.oracle_twins(cfg, word, rk.ROBOCUP_TWIN_STEPS)
    print("%s, %s: %d of %d environments diverged by step 5, %d by step 40" % (cfg, word, int(((first > 0) & (first <= 5)).sum()), len(first),
                                                                             int((first > 0).sum())))
    assert rk.twins_diverge_enough(cfg, first) == ""


@pytest.mark.parametrize("key", sorted(rk.KEYS))
def test_every_key_tuple_changes_the_reset_scene(key):
    """the key tuples are not vacuous at the reset either: against the plain key (42, 0, no episode written) every one of them draws
    other scenes, in Driving, RoboCup and RoboCup with RANDOM_INIT, and the oracle runs them finite and without complaint"""
    seed, off, ep = rk.KEYS[key]
    for cfg in ("drv10", "rc5", "rc5r"):
        plain, at = rk.oracle(cfg, 4, 42, 0), rk.oracle(cfg, 4, seed, off)
        plain.reset()
        at.reset()
        if ep is not None:
            rk.set_oracle_blobs(at, cfg, rk.bump_episode(rk.oracle_blobs(at, cfg), cfg, ep - 1))
            assert [at.get_state(e).episode for e in range(4)] == [ep] * 4
        plain.reset()
        at.reset()   # (both twice: the second reset is the one that draws at the written episode)
        assert [at.get_state(e).episode for e in range(4)] == [(2 if ep is None else ep + 1)] * 4
        assert not np.array_equal(rk.bits32(plain.obs), rk.bits32(at.obs)), cfg
        assert np.isfinite(at.obs).all() and at.overflow() == 0
