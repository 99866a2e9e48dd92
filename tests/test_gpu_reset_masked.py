"""Per-environment reset on the device (dynenv_reset_masked; BatchedDynEnv.reset_envs, episodes="per_env").  -m gpu.

The oracle has no per-environment reset and gets none.  Its environments are independent, though: OracleEnv(num_envs=1,
env_id_offset=e, seed=...) IS environment e of a batch, and resetting that object k times puts it into episode k.  The tests use one
such object per environment ("per-env oracles").  Every comparison is bit for bit: int views of the tensors, or checkpoint() bytes.

Configurations: those of tests/test_gpu_state_batch.py plus robocup5_random (randomInit + deterministicTurn: the other half of
rc_reset_masked_kernel).  dynenv_reset is the same kernels with no mask; tests/test_gpu_state_digests.py pins what they write.  Shapes: E = 1, E = 5 with the listed set {3, 0, 4}, E = 70 with every third environment plus 63 and 64 (both
sides of a 64 boundary).  "Pile" environments: capacity_scenes.drv_full_coupled / rc_chain written into environments 0 and 1 of the
configurations that have the ten agents the scenes need, and stepped twice: they hold live contacts when they are reset."""
import numpy as np
import pytest

import oracle_lib as ol
from per_env_common import (CASES, HISTORY, NAMES, PILE_CFGS, SENTINEL, SHAPES, actions as _actions, bits32 as _i32, bits64 as _i64,
                            ckpt as _ckpt, ckpt_diff as _ckpt_diff, driving as _driving, env_oracle as _oracle, make as _make,
                            pile_envs as _pile_envs, same_f32 as _same_f32, same_f64 as _same_f64, select, situation as _situation,
                            staggered as _staggered, step as _step, sub as _sub, write_pile as _write_pile)

pytestmark = pytest.mark.gpu

CFGS = select(*NAMES)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cfg,shape", CASES)
def test_all_listed_equals_the_whole_batch_reset(cfg, shape):
    """1. two handles in the same situation: A does reset_flat(), B reset_envs(every environment).  Every device array of the handle and
    the observation are the same bytes - twice in a row, which takes both through two episode counters."""
    import torch
    E, _ = SHAPES[shape]
    a, b = _situation(cfg, E), _situation(cfg, E)
    assert _ckpt_diff(a, b) == "", "same configuration, same history"
    ep0 = a.get_state(E - 1).episode
    for rnd, everyone in enumerate((torch.ones((E,), dtype=torch.uint8, device="cuda"), list(range(E)))):
        before = _ckpt(b).tobytes()
        oa = a.reset_flat()
        b.obs.view(torch.int32).fill_(SENTINEL)
        ob = b.reset_envs(everyone)
        assert _ckpt(b).tobytes() != before
        assert _ckpt_diff(a, b) == "", "round %d" % rnd
        assert np.array_equal(_i32(oa), _i32(ob)), "observations, round %d" % rnd
        assert a.get_state(E - 1).episode == b.get_state(E - 1).episode == ep0 + rnd + 1
    assert a.error_flags() == b.error_flags() == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("cfg,shape", CASES)
def test_a_subset_then_its_complement(cfg, shape):
    """2. reset_envs(M) changes the environments of M and nothing else - not a byte of the others' observation rows, not their state,
    and (five further steps against a twin that was never reset) not their contact caches; M and then its complement, each once,
    is the whole-batch reset; an empty mask changes nothing."""
    import torch
    E, M = SHAPES[shape]
    rest = [e for e in range(E) if e not in M]
    piles = _pile_envs(cfg, E)
    a, b, c = _situation(cfg, E), _situation(cfg, E), _situation(cfg, E)
    start, start_state = b.checkpoint(), _ckpt(b).tobytes()
    # an empty mask
    b.obs.view(torch.int32).fill_(SENTINEL)
    b.reset_envs([])
    b.reset_envs(torch.zeros((E,), dtype=torch.bool, device="cuda"))
    assert _ckpt(b).tobytes() == start_state and b.checkpoint().tobytes() == start.tobytes(), "an empty mask must not change a byte of the handle"
    assert bool((b.obs.view(torch.int32) == SENTINEL).all()), "... nor of obs"
    # M
    mask = torch.zeros((E,), dtype=torch.bool, device="cuda")
    mask[M] = True
    b.reset_envs(M if E <= 5 else mask)
    ob = _i32(b.obs)
    assert (ob[rest] == SENTINEL).all(), "observation rows of unlisted environments were written"
    for e in M:
        assert not (ob[e] == SENTINEL).any(), "environment %d: part of its observation was not written" % e
    if rest:
        assert torch.equal(b.get_states(rest), c.get_states(rest)), "the state of an unlisted environment changed"
    assert not torch.equal(b.get_states(M), c.get_states(M))
    sub = _sub(cfg)[0]
    for e in M:
        st = b.get_state(e)
        assert st.elapsed == 0 and st.episode == c.get_state(e).episode + 1
    for s, act in enumerate(_actions(cfg, E, b.n_agents, 5, 7, idle=piles)):
        ob_, rb, db = _step(b, act, auto_reset=False)
        oc, rc, dc = _step(c, act, auto_reset=False)
        if rest:
            assert np.array_equal(_i32(ob_)[rest], _i32(oc)[rest]), "observations of the unlisted environments, step %d" % s
            assert np.array_equal(_i64(rb)[rest], _i64(rc)[rest]), "rewards of the unlisted environments, step %d" % s
    if rest:
        assert torch.equal(b.get_states(rest), c.get_states(rest))
        assert b.get_state(rest[0]).elapsed == (HISTORY + 2 + 5) * sub
    # M, then the complement, from the situation as it was: the whole-batch reset
    b.restore(start)
    b.obs.view(torch.int32).fill_(SENTINEL)
    b.reset_envs(mask)
    b.reset_envs(~mask)
    oa = a.reset_flat()
    assert _ckpt_diff(a, b) == ""
    assert np.array_equal(_i32(oa), _i32(b.obs))
    for x in (a, b, c):
        x.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("cfg", PILE_CFGS)
def test_live_contacts_at_the_moment_of_reset(cfg, oracle_built):
    """3. environments 0 and 1 hold a pile with live contacts (asserted on the per-env oracles) when they are reset: ten steps of their
    next episode are the oracle's, and their error word is 0.  A contact-cache slot that was not freed or a stale shortcut row would
    show here; random play does not get there."""
    E, piles = 5, [0, 1]
    env = _make(cfg, E)
    env.reset_flat()
    ora = {e: _oracle(cfg, e) for e in piles}
    A = env.n_agents
    for a in _actions(cfg, E, A, HISTORY, 5):
        _step(env, a, auto_reset=False)
    for e in piles:
        ora[e].reset()
        st = _write_pile(cfg, ora[e].get_state(0), HISTORY)
        env.set_state(e, st)
        ora[e].set_state(0, st)

    def both(act, what):
        og, rg, dg = _step(env, act, auto_reset=False)
        og, rg, dg = og.cpu().numpy(), rg.cpu().numpy(), dg.cpu().numpy()
        for e in piles:
            oc, rc, dc = ora[e].step(act[e:e + 1])
            assert _same_f32(og[e], oc[0]), "%s: observations of environment %d" % (what, e)
            assert _same_f64(rg[e], rc[0]) and dg[e] == dc[0], "%s: rewards / dones of environment %d" % (what, e)
    for s, act in enumerate(_actions(cfg, E, A, 2, 6, idle=piles)):
        both(act, "pile step %d" % s)
    for e in piles:
        assert ora[e].active_contacts(0) > 0, "environment %d holds no live contact before the reset" % e
        assert ora[e].overflow() == 0
    obs = env.reset_envs(piles).cpu().numpy()
    for e in piles:
        assert _same_f32(obs[e], ora[e].reset()[0]), "the reset observation of environment %d" % e
    for s, act in enumerate(_actions(cfg, E, A, 10, 8)):
        both(act, "step %d of the next episode" % s)
    assert env.error_flags_per_env().cpu().numpy()[piles].tolist() == [0, 0]
    env.close()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cfg", ["driving10", "robocup5"])
def test_reset_clears_the_error_word_of_the_listed_environment_only(cfg):
    """4. error bit 1 on environment 2 (an action outside the action space), bit 6 on environment 3 (a refused blob): reset_envs([2])
    clears the one and leaves the other"""
    from dynenv_amd import _capi
    E = 5
    env = _make(cfg, E)
    env.reset_flat()
    act = _actions(cfg, E, env.n_agents, 1, 3)[0]
    act[2, 0, 0] = 9
    _step(env, act, auto_reset=False)
    bad = _capi.blobs_as_states(env.get_states([3]).cpu().numpy(), env.env_type)
    bad["n_cars" if _driving(cfg) else "n_robots"][0] += 1
    assert env.set_states([3], bad).cpu().tolist() == [1]
    assert env.error_flags_per_env().cpu().tolist() == [0, 0, 2, 64, 0]
    env.reset_envs([2])
    assert env.error_flags_per_env().cpu().tolist() == [0, 0, 0, 64, 0]
    assert env.error_flags() == 64
    env.reset_envs([3])
    assert env.error_flags() == 0
    env.close()


# ------------------------------------------------------------------------------------------------ 5
def _soak_sets(E, seed):
    """step -> environments reset before it.  Half of the environments are never listed; of the others one is listed at 3, 10 and 11
    (three times, and at two steps in a row), the rest at random, and all of them at 25."""
    rng = np.random.default_rng(seed)
    pool = [int(e) for e in rng.permutation(E)[:E // 2]]
    sets = {s: sorted(set([pool[0]] + [e for e in pool if rng.random() < 0.4])) for s in (3, 10, 11)}
    sets[25] = sorted(pool)
    return sets, pool


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_staggered_soak_against_per_env_oracles(cfg, oracle_built):
    """5. thirty steps with reset_envs at steps 3, 10, 11 and 25 against per-env oracles reset at the same moments: observations (the
    reset ones included), rewards and dones at every step, counts() after every reset"""
    E = 5 if CFGS[cfg][3] else 70
    sets, pool = _soak_sets(E, 77)
    times = {e: sum(e in v for v in sets.values()) for e in range(E)}
    assert sum(t > 0 for t in times.values()) * 3 >= E and sum(t == 0 for t in times.values()) * 3 >= E
    assert max(times.values()) >= 3 and set(sets[10]) & set(sets[11])
    env = _make(cfg, E)
    ora = [_oracle(cfg, e) for e in range(E)]
    og = env.reset_flat().cpu().numpy()
    for e in range(E):
        assert _same_f32(og[e], ora[e].reset()[0]), "first observation of environment %d" % e
    for s, act in enumerate(_actions(cfg, E, env.n_agents, 30, 9)):
        if s in sets:
            og = env.reset_envs(sets[s]).cpu().numpy()
            for e in sets[s]:
                assert _same_f32(og[e], ora[e].reset()[0]), "reset observation of environment %d before step %d" % (e, s)
            assert np.array_equal(env.counts().cpu().numpy(), np.concatenate([o.counts() for o in ora])), "counts after the reset before step %d" % s
        og, rg, dg = _step(env, act, auto_reset=False)
        og, rg, dg = og.cpu().numpy(), rg.cpu().numpy(), dg.cpu().numpy()
        for e in range(E):
            oc, rc, dc = ora[e].step(act[e:e + 1])
            assert _same_f32(og[e], oc[0]), "observations of environment %d, step %d" % (e, s)
            assert _same_f64(rg[e], rc[0]) and dg[e] == dc[0], "rewards / dones of environment %d, step %d" % (e, s)
    assert env.error_flags() == 0
    for e in range(E):
        assert env.get_state(e).episode == 1 + times[e] and env.get_state(e).elapsed == ora[e].get_state(0).elapsed
    env.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("cfg,E", [("driving10", 8), ("robocup5", 6)])
def test_natural_ends_per_env(cfg, E, oracle_built):
    """6. episodes="per_env": step_flat(auto_reset=True) returns the step's dones with the finished environments' rows of obs already
    holding their next episode's first observation; terminal_obs and last_episode_stats hold what the finished environments ended
    with.  An oracle is reset when its own done comes up.  No host-side position is consulted."""
    env, blobs = _staggered(cfg, E, keep_terminal_obs=True, track_episode_stats=True)
    ost = ol.DrivingState if _driving(cfg) else ol.RoboCupState
    ora = [_oracle(cfg, e) for e in range(E)]
    for e in range(E):
        ora[e].reset()
        ora[e].set_state(0, ost.from_buffer_copy(blobs[e].tobytes()))
    env._episode_step = 12345   # (nothing may depend on it)
    ended, last_stats = set(), {}
    for s, act in enumerate(_actions(cfg, E, env.n_agents, 8, 11)):
        og, rg, dg = _step(env, act, auto_reset=True)
        og, rg, dg = og.cpu().numpy(), rg.cpu().numpy(), dg.cpu().numpy()
        term = env.terminal_obs.cpu().numpy()
        stats = [x.cpu().numpy() for x in env.last_episode_stats]
        want_done = [e for e in range(E) if s + 1 == 1 + e % 4]
        assert sorted(np.nonzero(dg)[0].tolist()) == want_done, "step %d" % s
        if s < 4:
            assert 0 < len(want_done) < E, "the episodes must end apart"
        for e in range(E):
            oc, rc, dc = ora[e].step(act[e:e + 1])
            oc = oc.copy()
            assert dg[e] == dc[0] and _same_f64(rg[e], rc[0]), "dones / rewards of environment %d, step %d" % (e, s)
            assert _same_f32(term[e], oc[0]), "terminal_obs is the step's own observation (environment %d, step %d)" % (e, s)
            if dc[0]:
                last_stats[e] = [x[0].copy() for x in ora[e].episode_stats()]
                ended.add(e)
                oc = ora[e].reset()
            assert _same_f32(og[e], oc[0]), "observations of environment %d, step %d" % (e, s)
        for e in range(E):   # the rows of the environments that did not finish in this step keep their last value
            for k in range(4):
                want = last_stats[e][k] if e in ended else np.zeros_like(stats[k][e])
                assert np.array_equal(stats[k][e], want), "last_episode_stats[%d] of environment %d, step %d" % (k, e, s)
    assert ended == set(range(E))
    assert env._episode_step == 12345 and env.error_flags() == 0
    with pytest.raises(Exception, match="per_env"):
        env.step(_actions(cfg, E, env.n_agents, 1, 3)[0])
    env.close()


# ------------------------------------------------------------------------------------------------ 7
def test_a_captured_step_with_auto_reset_replays_like_eager_steps():
    """7. Driving Full, E = 5, per_env: ONE step_flat(auto_reset=True) - the step and the masked reset behind it, nothing decided on the
    host - captured with torch.cuda.graph and replayed 12 times across the staggered ends of test 6, against an eager handle; with
    keep_terminal_obs and track_episode_stats on, whose persistent tensors every replay refreshes"""
    import torch
    cfg, E = "driving10", 5
    eager, _ = _staggered(cfg, E, keep_terminal_obs=True, track_episode_stats=True)
    graphed, _ = _staggered(cfg, E, keep_terminal_obs=True, track_episode_stats=True)
    kept = (graphed.terminal_obs, graphed.last_episode_stats)   # persistent tensors: the replays must refresh these very objects
    assert torch.equal(eager.get_states(), graphed.get_states())
    static_a = torch.zeros((E, eager.n_agents, eager.action_dim), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_flat(static_a, auto_reset=True)
    # (the capture itself executed nothing)
    n_done = 0
    for r, act in enumerate(_actions(cfg, E, eager.n_agents, 12, 13)):
        static_a.copy_(torch.tensor(act, device="cuda"))
        g.replay()
        o, rw, d = eager.step_flat(static_a.clone(), auto_reset=True)
        assert torch.equal(d, graphed.dones), (r, "dones")
        assert torch.equal(rw.view(torch.int64), graphed.rewards.view(torch.int64)), (r, "rewards")
        assert torch.equal(o.view(torch.int32), graphed.obs.view(torch.int32)), (r, "observations")
        assert graphed.terminal_obs is kept[0] and graphed.last_episode_stats is kept[1]
        assert torch.equal(eager.terminal_obs.view(torch.int32), kept[0].view(torch.int32)), (r, "terminal_obs")
        assert not torch.equal(kept[0], graphed.obs) or int(d.sum()) == 0, (r, "terminal_obs is the observation before the reset")
        for k in range(4):
            assert torch.equal(eager.last_episode_stats[k], kept[1][k]), (r, "last_episode_stats", k)
        n_done += int(d.sum())
    assert n_done == E, "every environment ended once during the replays"
    assert torch.equal(eager.get_states(), graphed.get_states())
    assert eager.error_flags() == 0 and graphed.error_flags() == 0
    eager.close()
    graphed.close()


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("cfg", ["driving10", "robocup5"])
def test_lockstep_default_is_untouched(cfg):
    """8. a default-mode handle over an episode end: terminal_obs set, the whole batch reset, the host's position back at 0"""
    import torch
    from dynenv_amd import _capi
    E = 3
    env = _make(cfg, E)
    assert env.episodes == "lockstep" and not env.per_env
    env.reset_flat()
    sub, end = _sub(cfg)
    blobs = env.get_states().cpu().numpy()
    _capi.blobs_as_states(blobs, env.env_type)["elapsed"][:] = end - 2 * sub
    env.set_states(None, blobs, episode_step=env.steps_per_episode - 2)
    acts = _actions(cfg, E, env.n_agents, 2, 3)
    o, r, d = _step(env, acts[0], auto_reset=True)
    assert not env.last_done and env.terminal_obs is None and d.cpu().tolist() == [0] * E
    o, r, d = _step(env, acts[1], auto_reset=True)
    assert env.last_done and d.cpu().tolist() == [1] * E
    assert env.terminal_obs is not None and not torch.equal(env.terminal_obs, env.obs)
    assert env._episode_step == 0
    for e in range(E):
        st = env.get_state(e)
        assert st.elapsed == 0 and st.episode == 2
    with pytest.raises(_capi.DynEnvError, match="episodes"):
        _make(cfg, E, episodes="sometimes")
    env.close()
    # ... and the reference's object-array protocol is lock-step by construction: the compat step() of a per_env handle raises
    per = _make(cfg, E, episodes="per_env")
    per.reset()
    with pytest.raises(_capi.DynEnvError, match="per_env"):
        per.step(acts[0])
    with pytest.raises(_capi.DynEnvError, match="per_env"):
        per.step_wait()
    per.close()
