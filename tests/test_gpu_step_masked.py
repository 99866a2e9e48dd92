"""Stepping chosen environments on the device (dynenv_step_masked; BatchedDynEnv.step_flat(active=...), episodes="per_env").  -m gpu.

A listed environment gets exactly the step it would have got, an unlisted one keeps every byte of its state and of its output rows.
Every comparison is bit for bit: int views of the tensors, or checkpoint() bytes.  The oracle needs nothing new: OracleEnv(num_envs=1,
env_id_offset=e) IS environment e of a batch ("per-env oracles", tests/test_gpu_reset_masked.py) and is stepped exactly when e is
listed.  Configurations, shapes and pile environments are that file's (tests/per_env_common.py; the sentinels and the soak's masks: tests/step_masked_common.py)."""
import numpy as np
import pytest

import oracle_lib as ol
import per_env_common as pc
import step_masked_common as sm

pytestmark = pytest.mark.gpu


def _per_env_situation(cfg, E, **kw):
    return pc.situation(cfg, E, episodes="per_env", **kw)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cfg,shape", pc.CASES)
def test_all_listed_equals_the_plain_step(cfg, shape):
    """1. two handles in the same situation, piles with live contacts included, take three steps: A behind a mask of ones, B without
    a mask.  Checkpoints, observations, rewards and dones are the same bytes after each."""
    import torch
    E, _ = pc.SHAPES[shape]
    a, b = _per_env_situation(cfg, E), _per_env_situation(cfg, E)
    assert pc.ckpt_diff(a, b) == "", "same configuration, same history"
    ones = torch.ones((E,), dtype=torch.bool, device="cuda")
    for s, act in enumerate(pc.actions(cfg, E, a.n_agents, 3, 7, idle=pc.pile_envs(cfg, E))):
        before = pc.ckpt(a).tobytes()
        pc.step(a, act, auto_reset=False, active=ones if s != 1 else list(range(E)))
        pc.step(b, act, auto_reset=False)
        assert pc.ckpt(a).tobytes() != before
        assert pc.ckpt_diff(a, b) == "", "step %d" % s
        assert sm.same_outputs(sm.outputs(a), sm.outputs(b)) == "", "step %d" % s
    assert a.error_flags() == b.error_flags() == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("cfg,shape", pc.CASES)
def test_a_subset_then_its_complement_is_one_plain_step(cfg, shape):
    """2. step(M) changes the environments of M and nothing else - not a byte of the others' rows of obs / rewards / dones, not their
    state; M and then its complement with the same actions is one plain step of a twin, in every byte of the checkpoint and of the
    outputs; an empty mask changes no byte at all."""
    E, M = pc.SHAPES[shape]
    rest = [e for e in range(E) if e not in M]
    a, b = _per_env_situation(cfg, E), _per_env_situation(cfg, E)
    act = pc.actions(cfg, E, a.n_agents, 1, 7, idle=pc.pile_envs(cfg, E))[0]
    sm.fill_sentinels(a)
    sm.fill_sentinels(b)
    start = b.checkpoint().tobytes()
    # an empty mask, as ids and as a device tensor
    pc.step(b, act, auto_reset=False, active=[])
    pc.step(b, act, auto_reset=False, active=sm.mask_tensor(E, []))
    assert b.checkpoint().tobytes() == start, "an empty mask must not change a byte of the handle"
    assert sm.rows_are_sentinel(sm.outputs(b), list(range(E))), "... nor of the outputs"
    # M
    states = b.get_states().cpu().numpy()
    mask = sm.mask_tensor(E, M)
    pc.step(b, act, auto_reset=False, active=M if E <= 5 else mask)
    mid = sm.outputs(b)
    now = b.get_states().cpu().numpy()
    if rest:
        assert sm.rows_are_sentinel(mid, rest), "output rows of unlisted environments were written"
        assert np.array_equal(now[rest], states[rest]), "the state of an unlisted environment changed"
    for e in M:
        assert not np.array_equal(now[e], states[e]), "listed environment %d did not move" % e
        assert mid[2][e] in (0, 1) and not (mid[1][e] == sm.REW_SENTINEL).any(), "rewards / dones of listed environment %d" % e
    # ... then the complement: one plain step of the twin
    pc.step(b, act, auto_reset=False, active=~mask)
    pc.step(a, act, auto_reset=False)
    assert pc.ckpt_diff(a, b) == ""
    assert sm.same_outputs(sm.outputs(a), sm.outputs(b)) == ""
    if rest:
        assert sm.same_outputs(mid, sm.outputs(b), rows=M) == "", "the second call wrote rows of the first call's environments"
    assert a.error_flags() == b.error_flags() == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("cfg", pc.PILE_CFGS)
def test_frozen_in_the_middle_of_a_pile_then_resumed(cfg, oracle_built):
    """3. environments 0 and 1 hold a pile with live contacts (asserted on the per-env oracles at each freeze).  0 is left out at steps
    3 and 4 while 1 keeps going, 1 at step 7: every listed step is the oracle's next step, which takes the contact cache, the
    shortcut state and the call-to-call caches to have stayed as they were - what get_states / set_states around a step cannot do."""
    E, piles = 5, [0, 1]
    frozen = {3: [0], 4: [0], 7: [1]}
    env = pc.make(cfg, E, episodes="per_env")
    env.reset_flat()
    ora = {e: pc.env_oracle(cfg, e) for e in piles}
    A = env.n_agents
    for a in pc.actions(cfg, E, A, pc.HISTORY, 5):
        pc.step(env, a, auto_reset=False)
    for e in piles:
        ora[e].reset()
        st = pc.write_pile(cfg, ora[e].get_state(0), pc.HISTORY)
        env.set_state(e, st)
        ora[e].set_state(0, st)
    prev = sm.outputs(env)
    for s, act in enumerate(pc.actions(cfg, E, A, 12, 6, idle=piles)):
        out = frozen.get(s, [])
        for e in out:
            assert ora[e].active_contacts(0) > 0, "environment %d holds no live contact when it is frozen at step %d" % (e, s)
        listed = [e for e in range(E) if e not in out]
        og, rg, dg = pc.step(env, act, auto_reset=False, active=listed)
        og, rg, dg = og.cpu().numpy(), rg.cpu().numpy(), dg.cpu().numpy()
        for e in piles:
            if e in out:
                continue
            oc, rc, dc = ora[e].step(act[e:e + 1])
            assert pc.same_f32(og[e], oc[0]), "observations of environment %d, step %d" % (e, s)
            assert pc.same_f64(rg[e], rc[0]) and dg[e] == dc[0], "rewards / dones of environment %d, step %d" % (e, s)
        now = sm.outputs(env)
        if out:
            assert sm.same_outputs(prev, now, rows=out) == "", "output rows of the frozen environment changed at step %d" % s
        prev = now
    for e in piles:
        assert ora[e].overflow() == 0
        assert env.get_state(e).elapsed == ora[e].get_state(0).elapsed == (pc.HISTORY + 12 - (2 if e == 0 else 1)) * pc.sub(cfg)[0]
    assert env.error_flags_per_env().cpu().tolist() == [0] * E
    env.close()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cfg", sorted(pc.NAMES))
def test_soak_with_random_masks_against_per_env_oracles(cfg, oracle_built):
    """4. thirty steps, a seeded random mask of density one half per step (environment 0 always listed, 1 never, 2 every other step):
    the listed rows are the oracle's at every step, the unlisted rows the previous step's bytes, and at the end every environment's
    elapsed time is its own count of listed steps.  The Partial configurations are where a draw keyed by anything but the
    environment's own time would show."""
    E, steps = (5 if pc.CFGS[cfg][3] else 70), 30
    masks, times = sm.soak_masks(E, steps, sm.soak_seed(E, steps))
    assert times[0] == steps and times[1] == 0 and times[2] == steps // 2
    assert all(0 < t < steps for t in times[2:]), "every other environment is listed at least once and frozen at least once"
    assert abs(sum(times) / (E * steps) - 0.5) < 0.15
    env = pc.make(cfg, E, episodes="per_env")
    ora = [pc.env_oracle(cfg, e) for e in range(E)]
    og = env.reset_flat().cpu().numpy()
    for e in range(E):
        assert pc.same_f32(og[e], ora[e].reset()[0]), "first observation of environment %d" % e
    prev = sm.outputs(env)
    for s, act in enumerate(pc.actions(cfg, E, env.n_agents, steps, 9)):
        listed = masks[s]
        rest = [e for e in range(E) if e not in listed]
        og, rg, dg = pc.step(env, act, auto_reset=False, active=listed if s % 2 else sm.mask_tensor(E, listed))
        og, rg, dg = og.cpu().numpy(), rg.cpu().numpy(), dg.cpu().numpy()
        for e in listed:
            oc, rc, dc = ora[e].step(act[e:e + 1])
            assert pc.same_f32(og[e], oc[0]), "observations of environment %d, step %d" % (e, s)
            assert pc.same_f64(rg[e], rc[0]) and dg[e] == dc[0], "rewards / dones of environment %d, step %d" % (e, s)
        now = sm.outputs(env)
        assert sm.same_outputs(prev, now, rows=rest) == "", "output rows of unlisted environments changed at step %d" % s
        prev = now
    assert env.error_flags() == 0
    for e in range(E):
        assert env.get_state(e).elapsed == times[e] * pc.sub(cfg)[0], "environment %d" % e
    env.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("cfg,E", [("driving10", 8), ("robocup5", 6)])
def test_one_episode_each(cfg, E, oracle_built):
    """5. the evaluation loop: a staggered handle (environment e ends after 1 + e % 4 steps) is stepped with active=alive,
    auto_reset=False, until nobody is alive, and twice more.  Every environment stops exactly at its own end: its elapsed time and
    episode_stats() stay the oracle's values at its done, its dones byte stays 1."""
    import torch
    env, blobs = pc.staggered(cfg, E)
    ost = ol.DrivingState if pc.driving(cfg) else ol.RoboCupState
    ora = [pc.env_oracle(cfg, e) for e in range(E)]
    for e in range(E):
        ora[e].reset()
        ora[e].set_state(0, ost.from_buffer_copy(blobs[e].tobytes()))
    alive = torch.ones((E,), dtype=torch.bool, device="cuda")
    end_stats, live, n = {}, set(range(E)), 0
    acts = pc.actions(cfg, E, env.n_agents, 6, 11)
    while bool(alive.any()):
        obs, rew, done = env.step_flat(torch.tensor(acts[n], device="cuda"), auto_reset=False, active=alive)
        dg, rg = done.cpu().numpy(), rew.cpu().numpy()
        for e in sorted(live):
            oc, rc, dc = ora[e].step(acts[n][e:e + 1])
            assert dg[e] == dc[0] == (n + 1 == 1 + e % 4) and pc.same_f64(rg[e], rc[0]), "environment %d, step %d" % (e, n)
            if dc[0]:
                end_stats[e] = [x[0].copy() for x in ora[e].episode_stats()]
                live.discard(e)
        alive &= ~done.bool()
        n += 1
        assert sorted(np.nonzero(alive.cpu().numpy())[0].tolist()) == sorted(live)
    assert n == 4 and not live
    for extra in range(2):   # nobody is listed: nothing moves
        env.step_flat(torch.tensor(acts[n + extra], device="cuda"), auto_reset=False, active=alive)
    assert env.dones.cpu().tolist() == [1] * E
    stats = [x.cpu().numpy() for x in env.episode_stats()]
    for e in range(E):
        st = env.get_state(e)
        assert st.elapsed == pc.sub(cfg)[1] == ora[e].get_state(0).elapsed and st.episode == 1, "environment %d ran past its end" % e
        for k in range(4):
            assert np.array_equal(stats[k][e], end_stats[e][k]), "episode_stats[%d] of environment %d" % (k, e)
    assert env.error_flags() == 0
    env.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("cfg,E", [("driving10", 8), ("robocup5", 6)])
def test_auto_reset_with_active_resets_dones_and_active(cfg, E):
    """6. auto_reset=True with `active`: a finished, listed environment is reset once; a finished, unlisted one, whose dones byte is
    stale, is not - by episode counters; last_episode_stats rows change only for dones & active.  A twin that never resets says what
    the rows of the environments that just finished must hold."""
    env, _ = pc.staggered(cfg, E, track_episode_stats=True)
    twin, _ = pc.staggered(cfg, E)
    acts = pc.actions(cfg, E, env.n_agents, 3, 11)
    episodes = lambda h: [h.get_state(e).episode for e in range(E)]
    assert episodes(env) == [1] * E
    # step 0, nobody is reset: environments 0 and 4 finish
    pc.step(env, acts[0], auto_reset=False)
    pc.step(twin, acts[0], auto_reset=False)
    assert env.dones.cpu().tolist() == [int(e % 4 == 0) for e in range(E)] and episodes(env) == [1] * E
    want = [1] * E
    rows = [x.cpu().numpy().copy() for x in env.last_episode_stats]
    assert all(not r.any() for r in rows)
    listed = list(range(1, E))   # environment 0 stays out: finished, its dones byte 1 from step 0 on
    for s in (1, 2):
        _, _, done = pc.step(env, acts[s], auto_reset=True, active=listed)
        pc.step(twin, acts[s], auto_reset=False, active=listed)
        dg = done.cpu().numpy()
        assert dg[0] == 1, "the stale byte of the unlisted environment"
        ended = [e for e in listed if dg[e]]
        assert ended == [e for e in listed if s + 1 == 1 + e % 4 or (s == 1 and e == 4)], "step %d" % s   # (4 finished at step 0 and steps past its end)
        for e in ended:
            want[e] += 1
        assert episodes(env) == want, "step %d: exactly the finished and listed environments are reset, once" % s
        assert env.get_state(0).elapsed == pc.sub(cfg)[1], "the unlisted, finished environment was touched"
        now = [x.cpu().numpy().copy() for x in env.last_episode_stats]
        tw = [x.cpu().numpy() for x in twin.episode_stats()]
        others = [e for e in range(E) if e not in ended]
        for k in range(4):
            assert np.array_equal(now[k][others], rows[k][others]), "last_episode_stats[%d] changed outside dones & active, step %d" % (k, s)
            fresh = [e for e in ended if want[e] == 2 and not (s == 1 and e == 4)]   # (the twin's 4 took the same steps only up to step 0)
            assert np.array_equal(now[k][fresh], tw[k][fresh]), "last_episode_stats[%d] of the environments that finished at step %d" % (k, s)
        rows = now
    assert want[0] == 1 and want[4] == 2 and sum(want) == E + len([e for e in range(1, E) if e % 4 in (0, 1, 2)])
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("cfg", ["driving10", "driving_partial"])
def test_a_captured_masked_step_reads_its_mask_at_replay(cfg):
    """7. ONE step_flat(static_a, auto_reset=False, active=static_mask) captured with torch.cuda.graph and replayed 8 times, the mask's
    contents rewritten between the replays (everyone and nobody among them), against an eager handle.  Driving Partial: the deferred
    list's parity lives in device words after a capture and must alternate as the eager host's does."""
    import torch
    E = 5
    eager, graphed = _per_env_situation(cfg, E), _per_env_situation(cfg, E)
    assert pc.ckpt_diff(eager, graphed) == ""
    eager.obs.copy_(graphed.obs)   # (the rows of environments that sit a replay out are compared too: start from the same bytes)
    static_a = torch.zeros((E, eager.n_agents, eager.action_dim), dtype=torch.int32, device="cuda")
    static_mask = torch.zeros((E,), dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_flat(static_a, auto_reset=False, active=static_mask)
    masks = [[0, 2, 4], [1, 3], [], [0, 1, 2, 3, 4], [4], [0, 1], [2, 3, 4], [1]]
    for r, act in enumerate(pc.actions(cfg, E, eager.n_agents, 8, 13, idle=pc.pile_envs(cfg, E))):
        static_a.copy_(torch.tensor(act, device="cuda"))
        static_mask.copy_(sm.mask_tensor(E, masks[r]))
        g.replay()
        eager.step_flat(static_a.clone(), auto_reset=False, active=static_mask.clone())
        assert sm.same_outputs(sm.outputs(eager), sm.outputs(graphed)) == "", "replay %d" % r
        assert pc.ckpt_diff(eager, graphed) == "", "replay %d" % r
    want = [sum(e in m for m in masks) for e in range(E)]
    assert [graphed.get_state(e).elapsed for e in range(E)] == [(pc.HISTORY + 2 + w) * pc.sub(cfg)[0] for w in want]
    assert eager.error_flags() == 0 and graphed.error_flags() == 0
    eager.close()
    graphed.close()


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("cfg,E", [("driving10", 4096), ("driving10", 4100), ("driving_partial", 4096)])
def test_scheduling_shapes(cfg, E):
    """8. the launches that reschedule environments (isolation mode 1 at 4096, mode 2 at 4100, mode 3 for Partial), with piles in a
    handful of environments so that there are slow ones: four plain steps, then six steps where B takes "M_t, then its complement"
    and A one plain step.  Outputs and checkpoints are equal after every step and no placeholder gave up waiting.  B launches twice
    as often as A: nothing may depend on the launch count.  (Whether isolation engaged is not asserted: the placement may not
    validate on a shared device.)"""
    import torch
    piles = [5, 300, 1030, 2049, 4000]
    a, b = pc.make(cfg, E, episodes="per_env"), pc.make(cfg, E, episodes="per_env")
    for h in (a, b):
        h.reset_flat()
        for e in piles:
            h.set_state(e, pc.write_pile(cfg, h.get_state(e), 0))
    same = lambda: torch.equal(a.obs.view(torch.int32), b.obs.view(torch.int32)) and torch.equal(a.rewards.view(torch.int64), b.rewards.view(torch.int64)) \
        and torch.equal(a.dones, b.dones)
    ids = torch.arange(E, device="cuda")
    for s, act in enumerate(pc.actions(cfg, E, a.n_agents, 10, 17, idle=piles)):
        act = torch.tensor(act, device="cuda")
        a.step_flat(act, auto_reset=False)
        if s < 4:
            b.step_flat(act, auto_reset=False)
        else:
            m = (ids + s) % 2 == 0 if s % 3 else (ids // 7 + s) % 3 == 0   # (odd and even piles: each is among the frozen in the first call on some steps)
            b.step_flat(act, auto_reset=False, active=m)
            b.step_flat(act, auto_reset=False, active=~m)
        assert same(), "outputs, step %d" % s
        assert pc.ckpt_diff(a, b) == "", "step %d" % s
    for h in (a, b):
        assert h.debug_counters()["isolation_timeouts"] == 0
        assert h.error_flags() == 0
    assert a.debug_counters()["contact"] > 0, "the piles are on the contact path"
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("cfg", ["driving10", "robocup5"])
def test_error_words_of_unlisted_environments(cfg):
    """9. an action outside the action space in an unlisted row raises no bit 1 (the row is not read) and nothing under validate=True;
    the sticky bits of an unlisted environment survive; a listed environment that carries bit 6 keeps it"""
    from dynenv_amd import _capi
    E = 5
    env = pc.make(cfg, E, episodes="per_env")
    env.reset_flat()
    good = pc.actions(cfg, E, env.n_agents, 1, 3)[0]
    bad = good.copy()
    bad[2, 0, 0] = 9
    flags = lambda: env.error_flags_per_env().cpu().tolist()
    pc.step(env, bad, auto_reset=False, active=[0, 1, 3, 4])
    assert flags() == [0] * E, "the action row of an unlisted environment was read"
    pc.step(env, bad, auto_reset=False, validate=True, active=[0, 1, 3, 4])   # validate=True looks at the listed rows only ...
    before = env.get_states().cpu().numpy()
    with pytest.raises(Exception, match="Error: "):                           # ... and raises the reference's error for one of those
        pc.step(env, bad, auto_reset=False, validate=True, active=sm.mask_tensor(E, [2, 3]))
    assert np.array_equal(env.get_states().cpu().numpy(), before) and flags() == [0] * E, "raised before anything was launched"
    pc.step(env, bad, auto_reset=False, active=[2, 3])
    assert flags() == [0, 0, 2, 0, 0]
    pc.step(env, good, auto_reset=False, active=[0, 1, 3, 4])
    assert flags() == [0, 0, 2, 0, 0], "a sticky bit of an unlisted environment survives"
    blob = _capi.blobs_as_states(env.get_states([3]).cpu().numpy(), env.env_type)
    blob["n_cars" if pc.driving(cfg) else "n_robots"][0] += 1
    assert env.set_states([3], blob).cpu().tolist() == [1]
    assert flags() == [0, 0, 2, 64, 0]
    pc.step(env, good, auto_reset=False, active=[3])
    pc.step(env, good, auto_reset=False, active=[0])
    assert flags() == [0, 0, 2, 64, 0], "a listed environment keeps bit 6, an unlisted one too"
    assert env.error_flags() == 66
    env.close()


def test_active_needs_a_per_env_handle():
    """a lock-step handle's dones and auto-reset follow one host-side position that a partial step would make meaningless"""
    from dynenv_amd import _capi
    env = pc.make("driving2", 3)
    env.reset_flat()
    act = pc.actions("driving2", 3, env.n_agents, 1, 3)[0]
    with pytest.raises(_capi.DynEnvError, match="per_env"):
        pc.step(env, act, auto_reset=False, active=[0])
    pc.step(env, act, auto_reset=False)
    assert env.get_state(0).elapsed == 10
    env.close()
