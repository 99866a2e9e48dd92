"""The frame of the Driving substep loop: bookkeeping read off the next substep's batch, no-solve substeps finished inside
drv_light_substep (-m gpu, plus one CPU test of the scenes' preconditions on the oracle).

drv_light_substep reports whether every car was finished and not crashed in the flags it loaded at its ENTRY - the state at the end of
the previous substep, that substep's callbacks included - and the kernel applies that with the previous substep's elapsed time; a
substep that solves nothing (fast, quiescent, steady replay) ends inside the function with the velocity update on the registers it
holds.  What can go wrong: the team reward and all_finished one substep early or late (at either end of the step: the entry of
substep 0 is ignored, the tenth substep is read after the loop), taken from the flags in front of a callback, or the fused velocity
update on a stale velocity, flag or mass (tick's out-of-bounds zeroing, a car that tick has just crashed, the pedestrian's FSM).

One handle of 16 ten-car environments and one of 4 three-car environments, 12 steps, every step bit for bit against the oracle
(observations, rewards, dones, state blobs), Full and Partial + Realistic noise 3.  Every car that plays no part is finished and NOT
crashed, so that "all finished" hangs on the scene's cars alone.  `runner`: an unfinished car on the horizontal road's axis that
leaves the road's left end (x < -10, less than 100 from its goal at (0, 500)) and finishes in the tick of a chosen substep.

  goal_sub0 / _mid / _sub9   the last unfinished car finishes in substep 0, 5, 9 of step 0: finishedAt = 1, 6, 10
  crash_same        a finished car slides into another finished one; the `begin` callback crashes both in substep 5, the substep in
                    whose tick the runner finishes: all_finished must stay 0 (flags after the callback)
  crash_after       the same with the slider one substep later: all_finished = 1, finishedAt = 6, then the crash
  all_done_set / all_done_unset   every car finished before the step, all_finished 1 / 0 in the blob (0: substep 0 sets it)
  friction          no candidate pair (fast path, fused velocity update): a crashed car sliding (friction bit), a finished car that
                    crosses x = -50 within the step and is zeroed by tick's out-of-bounds rule, a dead pedestrian sliding, a live one
                    walking, an unfinished car that leaves the road and is crashed by tick while it moves
  quiescent         kat_scenes_r4.k3_scene: a car at rest inside a standing pedestrian, the pair ignored - every arbiter inert
  steady_pile       the recorded pile of tests/test_gpu_verdict_batch.py: steady replay
  face_on, pileup, head_on, chain   contact substeps between fast ones: vbValid true at a substep's entry after a solve, false after
                    a fast substep, in one step (face_on: the cars meet in step 0 and part again)
  three cars        the second handle: goal_mid and crash_same with n_players = 3

The path counters of debug_counters() are sums over the handle.  Per step they must add up to 10 substeps per environment, and there
is a step in which every path - fast, contact, steady replay, quiescent - ran.  (ONE environment cannot go through all four and back
to fast in the ten substeps of a step: the steady and inert verdicts come from the contact path alone, a slot needs three calls of it
to be steady and three more without a touch to expire.)

step_flat(active=...): a per-environment handle with the same scenes, one step with every other environment frozen.
"""
import math
import os

import numpy as np
import pytest

import capacity_scenes as cs
import oracle_lib as ol
import player_count_scenes as pcs
from capacity_scenes import _dead_ped
from kat_scenes_r4 import CY, _arrival_x, _place_crashed_car, k3_scene
from parity_common import _assert_state_equal, _scenario

SEED = 61
STEPS = 12
E, E3 = 16, 4
PART = dict(obs_type=1, noise_type=1, noise_magnitude=3.0)
STEADY_ENV, QUIET_ENV, FRICTION_ENV = 14, 9, 8
RUN_X = {0: -10.5, 5: -8.9, 9: -7.9}   # runner's x -> the substep of step 0 in whose tick it finishes (speed 30, coasting = braking)
_PILE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drv_steady_pile.npz"))


def _done_car(c, x, y, vx=0.0):
    """finished and not crashed: takes no action, slides under the crashed cars' friction, counts as done"""
    _place_crashed_car(c, 0, x, y, vx)
    c.crashed = 0


def _begin(st, n=10):
    st.n_peds = st.n_obst = 0
    st.elapsed = st.all_finished = 0
    for k in range(n):
        _done_car(st.cars[k], 60.0 + 40.0 * k, 560.0)


def _runner(c, x, v=30.0):
    _place_crashed_car(c, 0, x, 500.0, -v)
    c.angle, c.dirx, c.diry = math.pi, -1.0, 0.0
    c.finished = c.crashed = c.fric = 0
    c.lane_pos = 1
    c.goalx, c.goaly = 0.0, 500.0


def goal(sub):
    def scene(st, n=10):
        _begin(st, n)
        _runner(st.cars[0], RUN_X[sub])
    return scene


def crash(arrive):
    """car 2 slides into car 1's rear face (x = 290) in the position update of substep `arrive`; the runner finishes in substep 5"""
    def scene(st, n=10):
        _begin(st, n)
        _runner(st.cars[0], RUN_X[5])
        _done_car(st.cars[1], 300.0, CY)
        _done_car(st.cars[2], _arrival_x(0, 30.0, arrive, 290.0), CY, 30.0)
    return scene


def all_done(flag):
    def scene(st, n=10):
        _begin(st, n)
        st.all_finished = flag
    return scene


def friction(st):
    _begin(st)
    _place_crashed_car(st.cars[0], 0, 300.0, CY, 30.0)           # crashed, sliding
    _done_car(st.cars[1], -49.8, CY, -30.0)                      # crosses x = -50 in the step
    c = st.cars[2]                                               # unfinished, off every road, moving: tick crashes it in substep 0
    _place_crashed_car(c, 1, 500.0, CY, 20.0)
    c.finished = c.crashed = c.fric = 0
    st.n_peds = 2
    _dead_ped(st.peds[0], 600.0, CY, 20.0)
    p = st.peds[1]                                               # alive, walking along the horizontal road's walkway
    p.px, p.py, p.vx, p.vy = 1200.0, 440.0, 4.0, 0.0
    p.road, p.side, p.dead, p.moving, p.speed, p.crossing, p.begin_crossing = 1, 0, 0, 100000, 4, 0, 0


def face_on(st, n=10):
    _begin(st, n)
    _done_car(st.cars[0], 300.0, CY, 30.0)
    _done_car(st.cars[1], 324.0, CY + 2.0, -30.0)


SCENES = {1: goal(0), 2: goal(5), 3: goal(9), 4: crash(5), 5: crash(6), 6: all_done(1), 7: all_done(0), FRICTION_ENV: friction,
          10: face_on, 11: lambda st: cs.drv_chain10(st, seed=5, mixed=True)}
SCENARIOS = {12: "pileup", 15: "head_on"}


def _scenes():
    """environment -> state blob; environments 0 and 13 keep their reset state and play randomly"""
    ref = ol.OracleEnv(num_envs=1, n_players=10, seed=SEED)
    ref.reset()
    out = {}
    for e, scene in SCENES.items():
        st = ref.get_state(0)
        scene(st)
        st.elapsed = 0
        out[e] = st
    ref.close()
    for e, kind in SCENARIOS.items():
        out[e] = _scenario(kind)
        out[e].elapsed = 0
    out[QUIET_ENV] = k3_scene("with")
    out[QUIET_ENV].elapsed = 0
    pile = ol.DrivingState.from_buffer_copy(_PILE["blob"].tobytes())
    pile.elapsed = 0
    out[STEADY_ENV] = pile
    return out


def _scenes3():
    """the three-car handle: goal_mid and crash_same; environments 0 and 3 play randomly"""
    ref = ol.OracleEnv(num_envs=1, n_players=3, seed=SEED)
    ref.reset()
    out = {}
    for e, scene in ((1, goal(5)), (2, crash(5))):
        st = ref.get_state(0)
        scene(st, 3)
        st.n_cars, st.elapsed = 3, 0
        out[e] = st
    ref.close()
    return out


def _actions(rng, n_env, A, scenes, step, ten):
    a = rng.integers(0, 3, size=(n_env, A, 2)).astype(np.int32)
    for e in scenes:
        a[e] = 1                         # coast
    if ten:
        a[15, :2, 0] = 2                 # head_on: under power
        a[STEADY_ENV] = _PILE["actions"][step]
    return a


def _finished_at(reward_of_a_done_car):
    """a car that was finished before the step earns the team reward alone: (6000 - finishedAt) / 100"""
    return int(round(6000 - 100.0 * reward_of_a_done_car))


def test_scenes_reach_what_they_are_for(oracle_built):
    """CPU: what the oracle can tell of the scenes"""
    scenes = _scenes()
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4)
    ora.reset()
    for e, st in scenes.items():
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    _, r, _ = ora.step(_actions(rng, E, 10, scenes, 0, True))
    r = r.copy()
    after = {e: ora.get_state(e) for e in scenes}
    # the runner finishes in substep 0, 5, 9: finishedAt is the elapsed time at that substep's end
    for e, sub in ((1, 0), (2, 5), (3, 9)):
        assert after[e].all_finished == 1 and after[e].cars[0].finished == 1 and after[e].cars[0].crashed == 0, e
        assert _finished_at(r[e, 9]) == sub + 1, (e, r[e, 9])
    # the crash in the runner's substep: never all finished; one substep later: all finished at 6, and the cars crashed all the same
    s4, s5 = after[4], after[5]
    assert s4.all_finished == 0 and s4.cars[0].finished == 1 and s4.cars[0].crashed == 0 and s4.cars[1].crashed == 1 and s4.cars[2].crashed == 1
    assert r[4, 9] == 0.0
    assert s5.all_finished == 1 and _finished_at(r[5, 9]) == 6 and s5.cars[1].crashed == 1 and s5.cars[2].crashed == 1
    # all done before the step
    assert after[6].all_finished == 1 and not r[6].any()
    assert after[7].all_finished == 1 and _finished_at(r[7, 9]) == 1
    # friction: nothing touches; who slows down, who is zeroed, who is crashed by tick
    f0, f1 = scenes[FRICTION_ENV], after[FRICTION_ENV]
    assert ora.peak_arbiters(FRICTION_ENV) == 0
    assert 0.0 < f1.cars[0].vx < 30.0
    assert f1.cars[1].px <= -50.0 and f1.cars[1].vx == 0.0 and f0.cars[1].px > -50.0
    assert f1.cars[2].crashed == 1 and f1.cars[2].fric == 1 and 0.0 < f1.cars[2].vx < 20.0
    assert f1.peds[0].dead == 1 and 0.0 <= f1.peds[0].vx < 20.0 and f1.peds[0].px > 600.0
    assert f1.peds[1].dead == 0 and f1.peds[1].vx == 4.0 and f1.peds[1].px > 1200.0
    # the quiescent pair: an arbiter that is never solved, car and pedestrian at rest
    q = after[QUIET_ENV]
    assert ora.peak_arbiters(QUIET_ENV) == 1 and q.cars[0].vx == 0.0 and q.cars[0].crashed == 0 and q.peds[0].dead == 0
    # contacts where they are meant to be
    assert ora.peak_arbiters(10) >= 1 and ora.active_contacts(STEADY_ENV) >= 1
    for s in range(1, STEPS):
        ora.step(_actions(rng, E, 10, scenes, s, True))
    for e in (11, 12, 15):
        assert ora.peak_arbiters(e) >= 1, e
    assert ora.overflow() == 0 and ora.degenerate() == 0
    ora.close()
    # the three-car handle
    scenes3 = _scenes3()
    ora = ol.OracleEnv(num_envs=E3, n_players=3, seed=SEED, threads=2)
    ora.reset()
    for e, st in scenes3.items():
        ora.set_state(e, st)
    _, r, _ = ora.step(_actions(rng, E3, 3, scenes3, 0, False))
    assert ora.get_state(1).all_finished == 1 and _finished_at(r[1, 2]) == 6
    assert ora.get_state(2).all_finished == 0 and ora.get_state(2).cars[1].crashed == 1
    ora.close()


@pytest.fixture(scope="module")
def gpu(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import dynenv_amd
    return dynenv_amd


PATHS = ("fast", "quiescent", "contact", "steady")


def _compare(env, ora, og, rg, dg, oc, rc, dc, rows, msg):
    np.testing.assert_array_equal(dg.cpu().numpy()[rows], dc[rows], err_msg=msg + " dones")
    np.testing.assert_array_equal(rg.cpu().numpy()[rows], rc[rows], err_msg=msg + " rewards")
    np.testing.assert_array_equal(og.cpu().numpy()[rows], oc[rows], err_msg=msg + " observations")
    blobs = env.get_states().cpu().numpy()
    for e in rows:
        _assert_state_equal(ol.DrivingState.from_buffer_copy(blobs[e].tobytes()), ora.get_state(e), msg + " env %d" % e)
    return blobs


def _run(gpu, n_env, A, scenes, partial, ten):
    kw = dict(observationType=gpu.ObservationType.PARTIAL, noiseType=gpu.NoiseType.REALISTIC, noiseMagnitude=3) if partial else {}
    env = gpu.BatchedDynEnv(gpu.DynEnvType.DRIVE, n_env, A, seed=SEED, **kw)
    ora = ol.OracleEnv(num_envs=n_env, n_players=A, seed=SEED, threads=4, **(PART if partial else {}))
    np.testing.assert_array_equal(env.reset_flat().cpu().numpy(), ora.reset())
    for e, st in scenes.items():
        env.set_state(e, st)
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    rows = list(range(n_env))
    last = env.debug_counters()
    every_path = []
    for s in range(STEPS):
        a = _actions(rng, n_env, A, scenes, s, ten)
        og, rg, dg = env.step_flat(a, auto_reset=False)
        oc, rc, dc = ora.step(a)
        _compare(env, ora, og, rg, dg, oc, rc, dc, rows, "%d cars, step %d" % (A, s))
        assert env.error_flags_per_env().cpu().numpy().tolist() == [0] * n_env, s
        now = env.debug_counters()
        took = {k: now[k] - last[k] for k in PATHS}
        last = now
        print("step %d paths %s" % (s, took))
        assert sum(took.values()) == 10 * n_env, (s, took)
        every_path.append(all(took[k] > 0 for k in PATHS))
    assert env.error_flags() == 0 and ora.overflow() == 0 and ora.degenerate() == 0
    if ten:
        assert any(every_path), "no step in which the fast, quiescent, contact and steady-replay paths all ran"
    env.close()
    ora.close()


@pytest.mark.gpu
def test_substep_frame_full(gpu):
    _run(gpu, E, 10, _scenes(), partial=False, ten=True)
    _run(gpu, E3, 3, _scenes3(), partial=False, ten=False)


@pytest.mark.gpu
def test_substep_frame_partial(gpu):
    """drv_step_partial_kernel shares the step's body"""
    _run(gpu, E, 10, _scenes(), partial=True, ten=True)
    _run(gpu, E3, 3, _scenes3(), partial=True, ten=False)


@pytest.mark.gpu
def test_substep_frame_half_frozen(gpu):
    """step_flat(active=...), one step: the odd environments step (two runners, the crash one substep later, all done with the flag
    unset, the quiescent pair, the chain, head_on), the even ones keep every field of their state"""
    scenes = _scenes()
    env = gpu.BatchedDynEnv(gpu.DynEnvType.DRIVE, E, 10, seed=SEED, episodes="per_env")
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4)
    held = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4)   # never stepped: what a frozen environment must still hold
    np.testing.assert_array_equal(env.reset_flat().cpu().numpy(), ora.reset())
    held.reset()
    for e, st in scenes.items():
        env.set_state(e, st)
        ora.set_state(e, st)
        held.set_state(e, st)
    rng = np.random.default_rng(SEED)
    a = _actions(rng, E, 10, scenes, 0, True)
    odd, even = list(range(1, E, 2)), list(range(0, E, 2))
    og, rg, dg = env.step_flat(a, auto_reset=False, active=odd)
    oc, rc, dc = ora.step(a)
    blobs = _compare(env, ora, og, rg, dg, oc, rc, dc, odd, "half frozen")
    for e in even:
        _assert_state_equal(ol.DrivingState.from_buffer_copy(blobs[e].tobytes()), held.get_state(e), "frozen env %d" % e)
    assert env.error_flags() == 0
    env.close()
    ora.close()
    held.close()
