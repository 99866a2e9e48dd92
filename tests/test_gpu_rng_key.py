"""Every word of the random streams' key, and re-seeding, on the device (-m gpu).  Everything is compared bit for bit.

dm_env_rng(seed, genv, episode, purpose, entity, t) is one function on both sides (tests/test_rng_key_oracle.py pins it), so the
kernels can only differ from the oracle in the words they hand to it.  The key tuples of tests/rng_key_common.py put those words where
a 32-bit habit breaks them - the seed's high word (carried as a kernel argument, passed through uniform_u64, split into two ints and
glued together again in drv_light_substep), a global id with bit 16 / bit 30 set, an episode counter past 16 and 24 bits and at the
top of int32 - in six configurations: Driving Full with 10 and 2 cars, Driving Partial, RoboCup Full 5 a side with the default flags
and with RANDOM_INIT, RoboCup Partial (Partial: Realistic noise of magnitude 3).  32 environments, 12 steps (RoboCup Full: 40).

  1 + 2  reset, then steps, at every key tuple in every configuration                       test_reset_then_steps_at_every_key
  3      who computes a Driving Partial vision pass (fused / deferred launch)               test_both_vision_launches_draw_from_the_whole_seed
  4      the high word matters: device twins part ways like the oracle's                    test_the_high_word_of_the_seed_matters
  5      shard invariance at global ids up to 2^31 - 1                                      test_shard_invariance_at_the_largest_global_ids
  6      re-seeding: before a reset, mid-episode, through env_method, across a restore      test_reseed_*, test_restore_brings_back_*
  7      re-seeding a handle whose step was captured is refused, loudly                     test_captured_*"""
import numpy as np
import pytest

import capacity_scenes as cs
import oracle_lib as ol
import per_env_common as pc
import rng_key_common as rk
from capacity_scenes import resting_chain_scene as _resting_chain_scene

pytestmark = pytest.mark.gpu

E = rk.E
S1, S2 = 0x0123456700000007, 0xFEDCBA9876543210   # the re-seeding tests' seeds: both carry a high word (6e)


@pytest.fixture(scope="module", autouse=True)
def gpu(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import dynenv_amd
    return dynenv_amd


def _make(cfg, num_envs=E, seed=42, off=0, **kw):
    return pc.make(cfg, num_envs, seed, off, **kw)


def _t(a):
    import torch
    return torch.tensor(a, device="cuda")


def _step(env, a):
    o, r, d = env.step_flat(_t(a), auto_reset=False)
    return o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()


def _blobs(env):
    return env.get_states().cpu().numpy()


def _same_step(got, want, what):
    (og, rg, dg), (oc, rc, dc) = got, want
    assert np.array_equal(dg, dc), what + ": dones"
    assert np.array_equal(rk.bits64(rg), rk.bits64(rc)), what + ": rewards"
    bad = np.argwhere(rk.bits32(og) != rk.bits32(oc))
    assert len(bad) == 0, "%s: observations, first at (env, t, agent, column) = %s" % (what, bad[0])


def _same_stats(env, ora, what):
    g = [x.cpu().numpy() for x in env.episode_stats()]
    o = ora.episode_stats()
    for k in range(3):
        assert np.array_equal(rk.bits64(g[k]), rk.bits64(o[k])), "%s: episode_stats()[%d]" % (what, k)
    assert np.array_equal(g[3], o[3]), what + ": episode_stats()[3]"


def _clean(env, ora, what):
    assert env.error_flags() == 0 and ora.overflow() == 0 and ora.degenerate() == 0, what
    if rk.driving(what.split()[0]):
        assert ora.l.oracle_obs_overflow(ora.h) == 0, what


def _at_key(cfg, key):
    """a handle and an oracle at the key tuple, in front of the reset the tuple is about: created with its seed and env_id_offset; an
    episode tuple resets both once to have blobs, writes the episode into every blob - set_states on the device, set_state on the
    oracle - and reads it back"""
    seed, off, ep = rk.KEYS[key]
    env, ora = _make(cfg, seed=seed, off=off), rk.oracle(cfg, E, seed, off)
    if ep is not None:
        env.reset_flat()
        ora.reset()
        blobs = rk.oracle_blobs(ora, cfg)
        assert rk.blob_diff(_blobs(env), blobs, cfg) == ""
        rk.as_states(blobs, cfg)["episode"][:] = ep
        assert env.set_states(None, blobs, episode_step=0).cpu().tolist() == [0] * E
        rk.set_oracle_blobs(ora, cfg, blobs)
        assert rk.as_states(_blobs(env), cfg)["episode"].tolist() == [ep] * E == [ora.get_state(e).episode for e in range(E)]
    return env, ora


# ------------------------------------------------------------------------------------------------ resting piles (Driving, ten cars)
PILE_ENVS = (1, 9, 17, 30)


def _light_scene(st):
    """a crashed car whose face is 0.099 deep in an obstacle - inside the collision slop of 0.1: a resting arbiter that holds its slot
    and moves nothing - and a live pedestrian drifting through a corner of the car's box without ever touching it (its centre stays
    5.4 or more from the box's corner, its radius is 5; `moving` is set far ahead, so it never draws): a candidate pair with a moving
    body next to a steady one, which the contact path tests alone - its light mode, 118 of the 120 substeps of 12 steps"""
    st.n_peds, st.n_obst = 1, 1
    cs._place_crashed_car(st.cars[0], 0, 300.0, cs.CY, 0.0)
    st.obst_x[0], st.obst_y[0] = 300.0 + 10.0 + 10.0 - 0.099, cs.CY
    p = st.peds[0]
    p.px, p.py, p.vx, p.vy = 300.0 - 14.0, cs.CY + 9.0, 0.3, 0.0
    p.road, p.side, p.dead, p.moving, p.speed, p.crossing, p.begin_crossing = 1, 0, 0, 100000, 4, 0, 0
    cs._park(st, range(1, 10))


def _write_piles(cfg, env, ora):
    """resting piles in PILE_ENVS of a ten-car Driving pair (the blobs keep their episode counter and elapsed = 0)"""
    scenes = (lambda st: cs.drv_chain10(st, 5, mixed=True), cs.drv_full_coupled, lambda st: _resting_chain_scene(st, np.random.default_rng(3)),
              _light_scene)
    for e, scene in zip(PILE_ENVS, scenes):
        st = ora.get_state(e)
        scene(st)
        env.set_state(e, st)
        ora.set_state(e, st)


def _idle_piles(cfg, acts):
    for a in acts:
        a[list(PILE_ENVS)] = 1   # coast
    return acts


# ------------------------------------------------------------------------------------------------ 1 + 2
@pytest.mark.parametrize("cfg", sorted(rk.CFGS))
@pytest.mark.parametrize("key", sorted(rk.KEYS))
def test_reset_then_steps_at_every_key(key, cfg):
    """1. the reset at the key: observations (Partial: the T separate noisy draws), counts() and all E state blobs are the oracle's; an
    episode tuple's counter reads back as value + 1 on both sides.
    2. then the steps: observations, rewards and dones at every step; at the end all state blobs and episode_stats(), error_flags() == 0
    and no oracle overflow.  The ten-car Driving configurations hold resting piles in four environments (written after the reset), and
    with a seed that has a high word Driving Full must have run contact-path and light-mode substeps (debug_counters)."""
    what = "%s %s" % (cfg, key)
    seed, off, ep = rk.KEYS[key]
    env, ora = _at_key(cfg, key)
    og, oc = env.reset_flat().cpu().numpy(), ora.reset()
    assert np.array_equal(rk.bits32(og), rk.bits32(oc)), what + ": reset observations"
    assert np.array_equal(env.counts().cpu().numpy(), ora.counts()), what + ": counts()"
    assert rk.blob_diff(_blobs(env), rk.oracle_blobs(ora, cfg), cfg) == "", what + " after the reset"
    want_ep = 1 if ep is None else ep + 1
    assert rk.as_states(_blobs(env), cfg)["episode"].tolist() == [want_ep] * E == [ora.get_state(e).episode for e in range(E)]
    piles = cfg in ("drv10", "drvp")
    acts = rk.actions(cfg, E, rk.steps_of(cfg), 23)
    if piles:
        _write_piles(cfg, env, ora)
        _idle_piles(cfg, acts)
    for s, a in enumerate(acts):
        _same_step(_step(env, a), ora.step(a), "%s step %d" % (what, s))
    assert rk.blob_diff(_blobs(env), rk.oracle_blobs(ora, cfg), cfg) == "", what + " after the steps"
    _same_stats(env, ora, what)
    _clean(env, ora, what)
    if cfg == "drv10" and key in rk.HIGH_WORD_KEYS:
        dc = env.debug_counters()
        print(what, dc)
        assert dc["contact"] > 0 and dc["light"] > 0, dc
    env.close()
    ora.close()


# ------------------------------------------------------------------------------------------------ 3
DRV_ENVI_OFFSET_ARRAYS = 5   # pc.DRV_ARRAYS: envi is the sixth checkpointed array


def _defer_obs(env):
    """envi[EI_DEFER_OBS] of every environment of a Driving handle, out of its checkpoint: the first agent whose vision pass the step
    launch left to drv_partial_obs_deferred_kernel (0: all of them, A: none)"""
    c = env.checkpoint()
    n = env.num_envs
    size = {name: f * k * b * n for name, f, k, b in pc.DRV_ARRAYS}
    assert c.size == pc.CKPT_HEADER + sum(size.values()), "the checkpoint's layout changed: find envi again"
    off = pc.CKPT_HEADER + sum(size[name] for name, _, _, _ in pc.DRV_ARRAYS[:DRV_ENVI_OFFSET_ARRAYS])
    return c[off:off + size["envi"]].view(np.int32).reshape(n, pc.DRV_EI_COUNT)[:, pc.DRV_EI_DEFER_OBS].copy()


@pytest.mark.parametrize("key", ["K2", "K3"])
def test_both_vision_launches_draw_from_the_whole_seed(key, monkeypatch):
    """3. Driving Partial at a seed with a high word, on a handle created under DYNENV_NO_ISOLATION=1: without a forecast the static
    rule decides who computes an environment's ten vision passes - five or more contact-path substeps in the step leave all ten to
    drv_partial_obs_deferred_kernel, which gets the seed as an argument of its own; anything less and the step kernel runs them fused.
    The pile environments are on the contact path from the first substep, the others touch nothing.
    How the test knows both ran: the step kernel leaves "first agent not done here" in envi[EI_DEFER_OBS], a checkpointed word; it is
    read after every step and must be 0 (all ten deferred) for a pile environment and 10 (all ten fused) for an undisturbed one, in every
    step - while every observation row equals the oracle's."""
    cfg = "drvp"
    seed, off, _ = rk.KEYS[key]
    monkeypatch.setenv("DYNENV_NO_ISOLATION", "1")
    env = _make(cfg, seed=seed, off=off)
    monkeypatch.delenv("DYNENV_NO_ISOLATION")
    assert env.debug_counters()["isolation_mode"] == 0
    ora = rk.oracle(cfg, E, seed, off)
    assert np.array_equal(rk.bits32(env.reset_flat().cpu().numpy()), rk.bits32(ora.reset()))
    _write_piles(cfg, env, ora)
    deferred_all, fused_all = np.zeros(E, np.int64), np.zeros(E, np.int64)
    steps = 6
    for s, a in enumerate(_idle_piles(cfg, rk.actions(cfg, E, steps, 29))):
        _same_step(_step(env, a), ora.step(a), "%s %s step %d" % (cfg, key, s))
        d = _defer_obs(env)
        deferred_all += d == 0
        fused_all += d == env.n_agents
    print("steps with all ten passes deferred:", deferred_all.tolist(), "fused:", fused_all.tolist())
    piles = list(PILE_ENVS[:3])   # the chains and the coupled groups: ten contact-path substeps a step
    assert (deferred_all[piles] == steps).all(), "the piles' passes were not left to the deferred launch: %s" % deferred_all[piles]
    rest = [e for e in range(E) if e not in PILE_ENVS]
    assert (fused_all[rest] > 0).all() and fused_all[rest].sum() >= (steps - 1) * len(rest), "the undisturbed environments did not run fused: %s" % fused_all[rest]
    assert rk.blob_diff(_blobs(env), rk.oracle_blobs(ora, cfg), cfg) == ""
    _clean(env, ora, cfg + " " + key)
    env.close()
    ora.close()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cfg", ["drv10", "drv2", "rc5"])
def test_the_high_word_of_the_seed_matters(cfg):
    """4. two handles with seeds 42 and 42 + 2^32: their reset scenes differ; given the same blobs (set_states) they part ways - every
    Driving environment within 5 steps, at least 8 of 32 RoboCup environments within 40: the condition the oracle twins meet on the
    CPU (tests/test_rng_key_oracle.py).  And since both sides are bit-identical to the oracle, every environment parts ways at the very
    step at which the oracle twins do."""
    seed, off, _ = rk.twin_key("high")
    a, b = _make(cfg, seed=rk.TWIN_SEED, off=rk.TWIN_OFFSET), _make(cfg, seed=seed, off=off)
    assert not np.array_equal(rk.bits32(a.reset_flat().cpu().numpy()), rk.bits32(b.reset_flat().cpu().numpy())), "the reset scenes"
    assert not np.array_equal(_blobs(a), _blobs(b))
    blobs = rk.twin_blobs(cfg)
    for x in (a, b):
        assert x.set_states(None, blobs, episode_step=0).cpu().tolist() == [0] * E
    assert np.array_equal(_blobs(a), blobs) and np.array_equal(_blobs(b), blobs)
    steps = rk.DRIVING_TWIN_STEPS if rk.driving(cfg) else rk.ROBOCUP_TWIN_STEPS
    first = rk.first_divergence(lambda x: _step(a, x)[0], lambda x: _step(b, x)[0], rk.actions(cfg, E, steps, 17))
    print(cfg, "first divergence per environment:", first.tolist())
    assert rk.twins_diverge_enough(cfg, first) == ""
    assert np.array_equal(first, rk.oracle_twins(cfg, "high", steps)), "the device twins do not part ways where the oracle twins do"
    assert a.error_flags() == 0 and b.error_flags() == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("cfg", ["drv10", "drvp", "rc5r", "rcp"])
def test_shard_invariance_at_the_largest_global_ids(cfg):
    """5. environment k of a handle at env_id_offset = 2^31 - E is environment 0 of a one-environment handle at 2^31 - E + k: after
    the reset and after 5 steps, observations, rewards, dones and the state blob"""
    seed, off = 2 ** 33 + 7, 2 ** 31 - E
    ks = (0, 13, E - 1)
    batch = _make(cfg, seed=seed, off=off)
    ones = [_make(cfg, 1, seed=seed, off=off + k) for k in ks]
    ob = batch.reset_flat().cpu().numpy()
    for k, one in zip(ks, ones):
        assert np.array_equal(rk.bits32(one.reset_flat().cpu().numpy()[0]), rk.bits32(ob[k])), "reset observation of environment %d" % k
        assert np.array_equal(_blobs(one)[0], _blobs(batch)[k]), "reset state of environment %d" % k
    assert not np.array_equal(ob[ks[0]], ob[ks[1]])
    for s, a in enumerate(rk.actions(cfg, E, 5, 31)):
        got = _step(batch, a)
        for k, one in zip(ks, ones):
            _same_step(_step(one, a[k:k + 1]), tuple(x[k:k + 1] for x in got), "environment %d step %d" % (k, s))
    bb = _blobs(batch)
    for k, one in zip(ks, ones):
        assert np.array_equal(_blobs(one)[0], bb[k]), "state of environment %d after the steps" % k
        assert one.error_flags() == 0
        one.close()
    assert batch.error_flags() == 0
    batch.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("cfg", ["drv10", "drvp", "rc5r", "rcp"])
def test_reseed_then_reset_is_a_fresh_handle(cfg):
    """6a. created with s1, seed(s2), reset = created with s2, reset = the oracle of s2: observations, counts, blobs, and the two
    handles' checkpoints byte for byte (pc.ckpt: whole, but for Driving Partial's scheduling word EI_DEFER_OBS)"""
    a, b, ora = _make(cfg, seed=S1, off=5), _make(cfg, seed=S2, off=5), rk.oracle(cfg, E, S2, 5)
    assert a.seed(S2) == [S2] * E
    oa, ob, oc = a.reset_flat().cpu().numpy(), b.reset_flat().cpu().numpy(), ora.reset()
    assert np.array_equal(rk.bits32(oa), rk.bits32(ob)) and np.array_equal(rk.bits32(oa), rk.bits32(oc))
    assert np.array_equal(a.counts().cpu().numpy(), ora.counts())
    assert rk.blob_diff(_blobs(a), rk.oracle_blobs(ora, cfg), cfg) == ""
    assert pc.ckpt_diff(a, b) == ""
    for s, act in enumerate(rk.actions(cfg, E, 3, 37)):
        got = _step(a, act)
        _same_step(got, _step(b, act), "re-seeded against fresh, step %d" % s)
        _same_step(got, ora.step(act), "re-seeded against the oracle, step %d" % s)
    assert pc.ckpt_diff(a, b) == ""
    for x in (a, b):
        assert x.error_flags() == 0
        x.close()


@pytest.mark.parametrize("cfg", ["drv10", "drvp", "rc5", "rcp"])
def test_reseed_mid_episode_changes_the_draws_and_no_state(cfg):
    """6b. four steps under s1, then seed(s2) on the handle and on the oracle: no state blob changes, and the steps after it are the
    oracle's - the rest of the episode draws from s2 at the same (global id, episode, time)"""
    env, ora = _make(cfg, seed=S1), rk.oracle(cfg, E, S1)
    assert np.array_equal(rk.bits32(env.reset_flat().cpu().numpy()), rk.bits32(ora.reset()))
    acts = rk.actions(cfg, E, 12, 41)
    for s, a in enumerate(acts[:4]):
        _same_step(_step(env, a), ora.step(a), "%s under s1, step %d" % (cfg, s))
    before = _blobs(env)
    ck = pc.ckpt(env)
    assert env.seed(S2) == [S2] * E
    ora.seed(S2)
    assert np.array_equal(_blobs(env), before) and rk.blob_diff(rk.oracle_blobs(ora, cfg), before, cfg) == ""
    after = pc.ckpt(env)
    assert np.array_equal(after[pc.CKPT_HEADER:], ck[pc.CKPT_HEADER:]), "seed() changed a device array"
    assert not np.array_equal(after[:pc.CKPT_HEADER], ck[:pc.CKPT_HEADER]), "a checkpoint taken after seed() carries the new seed"
    for s, a in enumerate(acts[4:]):
        _same_step(_step(env, a), ora.step(a), "%s under s2, step %d" % (cfg, 4 + s))
    assert rk.blob_diff(_blobs(env), rk.oracle_blobs(ora, cfg), cfg) == ""
    _same_stats(env, ora, cfg)
    _clean(env, ora, cfg + " re-seeded")
    env.close()
    ora.close()


def test_reseed_through_env_method_is_the_same_call():
    """6c. env_method("set_random_seed", s) and seed(s) are one call, and both return [s] * num_envs"""
    cfg = "drv2"
    a, b, c = _make(cfg, seed=S1), _make(cfg, seed=S1), _make(cfg, seed=S2)
    assert a.seed(S2) == [S2] * E and b.env_method("set_random_seed", S2) == [S2] * E
    oa, ob, oc = (x.reset_flat().cpu().numpy() for x in (a, b, c))
    assert np.array_equal(rk.bits32(oa), rk.bits32(ob)) and np.array_equal(rk.bits32(oa), rk.bits32(oc))
    assert pc.ckpt_diff(a, b) == "" and pc.ckpt_diff(a, c) == ""
    for x in (a, b, c):
        x.close()


@pytest.mark.parametrize("cfg", ["drv10", "drvp", "rc5"])
def test_restore_brings_back_the_seed_of_the_checkpoint(cfg):
    """6d. checkpoint under s1, seed(s2), three steps, restore(): the continuation is that of a twin that stayed with s1 throughout and
    never took the detour.  (A third handle takes the detour's three steps under s1: in Driving, where every step draws, the re-seeded
    handle's must differ from them - the detour really ran under another seed.)"""
    a, twin, detour = _make(cfg, seed=S1), _make(cfg, seed=S1), _make(cfg, seed=S1)
    for x in (a, twin, detour):
        x.reset_flat()
    acts = rk.actions(cfg, E, 11, 43)
    for act in acts[:3]:
        got = _step(a, act)
        _same_step(got, _step(twin, act), "before the checkpoint")
        _same_step(got, _step(detour, act), "before the checkpoint")
    ck = a.checkpoint()
    assert a.seed(S2) == [S2] * E
    strayed = False
    for act in acts[3:6]:
        strayed = strayed or not np.array_equal(rk.bits32(_step(a, act)[0]), rk.bits32(_step(detour, act)[0]))
    assert strayed or not rk.driving(cfg), "the steps under s2 should have differed from the same steps under s1"
    a.restore(ck)
    for s, act in enumerate(acts[6:]):
        _same_step(_step(a, act), _step(twin, act), "after the restore, step %d" % s)
    assert pc.ckpt_diff(a, twin) == ""
    for x in (a, twin, detour):
        assert x.error_flags() == 0
        x.close()


# ------------------------------------------------------------------------------------------------ 7
def _refuses_another_seed(graphed, other_ckpt):
    """after a capture: seed(other) and restore() of a checkpoint taken under another seed raise and leave every byte of the handle as
    it was (the whole checkpoint, header - the seed - included); the handle's own seed again is accepted"""
    from dynenv_amd import _capi
    before = graphed.checkpoint().tobytes()
    with pytest.raises(_capi.DynEnvError, match="captured"):
        graphed.seed(S2)
    with pytest.raises(_capi.DynEnvError, match="captured"):
        graphed.env_method("set_random_seed", S2)
    with pytest.raises(_capi.DynEnvError, match="captured"):
        graphed.restore(other_ckpt)
    assert graphed.checkpoint().tobytes() == before, "a refused call changed the handle"
    assert graphed.seed(S1) == [S1] * graphed.num_envs
    assert graphed.checkpoint().tobytes() == before


def _other_checkpoint(make):
    other = make(S2)
    other.reset_flat()
    ck = other.checkpoint()
    other.close()
    return ck


def _same_tensors(eager, graphed, what):
    import torch
    assert torch.equal(eager.dones, graphed.dones), (what, "dones")
    assert torch.equal(eager.rewards.view(torch.int64), graphed.rewards.view(torch.int64)), (what, "rewards")
    assert torch.equal(eager.obs.view(torch.int32), graphed.obs.view(torch.int32)), (what, "observations")


@pytest.mark.parametrize("cfg", ["drv10", "rc5"])
def test_captured_step_keeps_its_seed_and_says_so(cfg):
    """7. one captured step (the seed is a by-value kernel argument: a replay draws from the seed of the capture): from the capture on
    another seed is refused, by seed() and by restore(), before anything is written; replays go on equal to an eager twin"""
    import torch
    eager, graphed = _make(cfg, seed=S1), _make(cfg, seed=S1)
    other_ckpt = _other_checkpoint(lambda s: _make(cfg, seed=s))
    eager.reset_flat()
    graphed.reset_flat()
    acts = rk.actions(cfg, E, 8, 47)
    for a in acts[:2]:
        eager.step_flat(_t(a), auto_reset=False)
        graphed.step_flat(_t(a), auto_reset=False)
    assert graphed.seed(S1) == [S1] * E   # (free before the capture: a no-op here)
    static_a = _t(acts[2])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_flat(static_a, auto_reset=False)
    _refuses_another_seed(graphed, other_ckpt)
    for r, a in enumerate(acts[2:]):
        static_a.copy_(_t(a))
        g.replay()
        eager.step_flat(_t(a), auto_reset=False)
        _same_tensors(eager, graphed, "replay %d" % r)
    assert torch.equal(eager.get_states(), graphed.get_states())
    assert eager.error_flags() == 0 and graphed.error_flags() == 0
    eager.close()
    graphed.close()


def test_captured_step_with_auto_reset_keeps_its_seed_and_says_so():
    """7. ... and step_flat(auto_reset=True) of a per-environment handle - the step and the masked reset behind it in one graph, 32
    environments whose episodes end one to four steps from here: the resets inside the replays draw their scenes from the captured
    seed, like the eager twin's"""
    import torch
    cfg = "driving10"
    eager, _ = pc.staggered(cfg, E, seed=S1)
    graphed, _ = pc.staggered(cfg, E, seed=S1)
    other_ckpt = _other_checkpoint(lambda s: pc.make(cfg, E, seed=s))
    static_a = torch.zeros((E, eager.n_agents, eager.action_dim), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_flat(static_a, auto_reset=True)
    _refuses_another_seed(graphed, other_ckpt)
    n_done = 0
    for r, a in enumerate(pc.actions(cfg, E, eager.n_agents, 6, 13)):
        static_a.copy_(_t(a))
        g.replay()
        eager.step_flat(static_a.clone(), auto_reset=True)
        _same_tensors(eager, graphed, "replay %d" % r)
        n_done += int(graphed.dones.sum())
    assert n_done == E, "every environment ended - and was reset inside a replay - once"
    assert torch.equal(eager.get_states(), graphed.get_states())
    assert eager.error_flags() == 0 and graphed.error_flags() == 0
    eager.close()
    graphed.close()


def test_captured_masked_reset_alone_freezes_the_seed_too():
    """7. the masked reset draws whole scenes from the seed: capturing it alone (RoboCup, no step captured) is enough to refuse another"""
    import torch
    cfg = "rc5r"
    eager, graphed = _make(cfg, seed=S1, episodes="per_env"), _make(cfg, seed=S1, episodes="per_env")
    other_ckpt = _other_checkpoint(lambda s: _make(cfg, seed=s, episodes="per_env"))
    eager.reset_flat()
    graphed.reset_flat()
    mask = torch.zeros((E,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.reset_envs(mask)
    _refuses_another_seed(graphed, other_ckpt)
    for r, listed in enumerate(([0, 5, 31], [5], list(range(E)))):
        mask.zero_()
        mask[listed] = 1
        g.replay()
        eager.reset_envs(listed)
        assert torch.equal(eager.obs.view(torch.int32), graphed.obs.view(torch.int32)), r
        assert torch.equal(eager.get_states(), graphed.get_states()), r
    assert pc.ckpt_diff(eager, graphed) == ""
    eager.close()
    graphed.close()
