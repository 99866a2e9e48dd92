"""The call paths of a Driving contact substep (-m gpu, plus one CPU test of the scenes' preconditions).

A contact substep ends in one of four solves: single-level bias-only, single-level general (drv_prestep_solve), multi-level bias-only
(drv_prestep_solve_multi, sweeps inside) and general multi-level, where drv_prestep_solve_multi hands its values back to the kernel,
which calls drv_solve_general_split and then drv_split_verdicts.  Everything a slot needs travels through argument and return
registers from one function to the next: a value dropped or mis-routed on the way shows in the slot record (the state blob) at once
and in the observations a step later.  One handle of 16 environments, 24 steps, holds scenes for all four:

  drv_passes         isolated arbiters: four cars resting 0.5 deep in an obstacle each (single-level, bias-only), two cars sliding
                     into an obstacle a few steps later (single-level, general)
  drv_full_coupled   five groups of two cars and obstacles, everything at rest 0.5 deep: arbiters share bodies, only bias moves
  drv_chain10 mixed  ten moving cars and three pedestrians in one row: thirteen levels deep, general - the split path
  pile-up            three cars driven into each other (tests/parity_common.py): the split path while they collide, other solves once
                     they have come apart or to rest - both within one step

The oracle solves every contact graph with the same sequential sweep, so it cannot tell the four apart; what it can tell -
how many arbiters are solved, whether they share bodies (by construction of the scenes), whether anything moves - is checked
on the CPU below.  On the GPU the per-environment diagnostic counters tell which environment took the split path in which step."""
import ctypes as C

import numpy as np
import pytest

import capacity_scenes as cs
import oracle_lib as ol
from parity_common import _assert_state_equal, _scenario

SEED = 21
STEPS = 24
EI_N_FAST, N_COUNTERS = 8, 10   # driving_dev.h: EI_N_FAST .. EI_N_SPLIT, ten consecutive words of an environment's int row
FAST, QUIET, CONTACT, SLOTS, WHY_CAND, WHY_MOVING, WHY_INERT, STEADY, LIGHT, SPLIT = range(10)
PART = dict(obs_type=1, noise_type=1, noise_magnitude=3.0)


def _scenes():
    """environment -> state blob; the environments in between keep their reset state and play randomly"""
    ref = ol.OracleEnv(num_envs=1, n_players=10, seed=SEED)
    ref.reset()

    def blob(scene, **kw):
        st = ref.get_state(0)
        scene(st, **kw)
        st.elapsed = 0
        return st
    pile = _scenario("pileup")
    pile.elapsed = 0
    return {1: blob(cs.drv_chain10, seed=5, mixed=True), 2: blob(cs.drv_full_coupled), 4: blob(cs.drv_passes), 7: pile,
            9: blob(cs.drv_chain10, seed=6, mixed=True), 12: pile, 14: blob(cs.drv_full_coupled)}


def _actions(rng, E, scenes, step):
    a = rng.integers(0, 3, size=(E, 10, 2)).astype(np.int32)
    for e, st in scenes.items():
        a[e] = 1                      # coast
        if st.n_peds == 2 and st.n_obst == 2 and step >= 10:
            a[e, 0, 0] = 2            # the pile-up: car 0 accelerates into what it rests against (as in test_collision_scenarios)
    return a


def test_scenes_reach_what_they_are_for(oracle_built):
    """CPU: the oracle's view of the four scenes over the 24 steps of the GPU test"""
    E = 16
    scenes = _scenes()
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4)
    ora.reset()
    for e, st in scenes.items():
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    act = {e: [] for e in scenes}
    moving = {e: [] for e in scenes}
    for s in range(STEPS):
        ora.step(_actions(rng, E, scenes, s))
        for e in scenes:
            act[e].append(ora.active_contacts(e))
            d = ol.state_to_dict(ora.get_state(e))
            moving[e].append(bool(np.any(d["cars_f"][:, 2:4] != 0.0)))   # vx, vy of the cars
    assert ora.overflow() == 0 and ora.degenerate() == 0
    # drv_passes: isolated arbiters (no two share a car), four at rest from the start, six once cars 0 and 9 have arrived
    assert act[4][0] == 4 and max(act[4]) == 6 and ora.peak_arbiters(4) == 6, act[4]
    # drv_full_coupled: 24 arbiters over ten cars (they share bodies; some let go and touch again as the bias pushes them apart) and no
    # car ever has a velocity: bias only
    assert act[2][0] == cs.DRV_NS and min(act[2]) >= 15 and not any(moving[2]), (act[2], moving[2])
    # the chains: at least ten arbiters deep while the row is moving
    for e in (1, 9):
        assert max(act[e]) >= 10 and moving[e][0], act[e]
    # the pile-up: three cars, one arbiter first, then two that share the middle car, moving; at rest before the end
    assert 1 in act[7] and max(act[7]) == 2 and moving[7][0] and not moving[7][-1], (act[7], moving[7])
    ora.close()


@pytest.fixture(scope="module")
def gpu(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import dynenv_amd
    return dynenv_amd


def _counters(env, E):
    """every environment's ten diagnostic counters, out of the handle's checkpoint (driving_tu.hip: the payload is the device arrays
    body, carx, flags, aux, obst, envi, ... in allocation order, each [planes][E][row]; envi's row length follows from the size)"""
    ck = env.checkpoint()
    header = C.sizeof(ol.Cfg) + 24
    payload = len(ck) - header
    assert int(np.frombuffer(ck[header - 8:header].tobytes(), np.uint64)[0]) == payload
    before = E * (9 * 32 * 8 + 6 * 16 * 8 + 32 * 4 + 32 * 4 + 2 * 20 * 8)
    after = E * (2 * 16 * 8 + 24 * 4 + 24 * 4 + 2 * 24 * 4 + 4 * 24 * 8 + 64 * 4)
    row = (payload - before - after) // E
    assert row > 0 and row % 4 == 0 and before + after + E * row == payload
    envi = np.frombuffer(ck[header + before:header + before + E * row].tobytes(), np.int32).reshape(E, row // 4)
    return envi[:, EI_N_FAST:EI_N_FAST + N_COUNTERS].astype(np.int64)


def _run(gpu, E, steps, scenes, partial):
    kw = dict(observationType=gpu.ObservationType.PARTIAL, noiseType=gpu.NoiseType.REALISTIC, noiseMagnitude=3) if partial else {}
    env = gpu.BatchedDynEnv(gpu.DynEnvType.DRIVE, E, 10, seed=SEED, **kw)
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4, **(PART if partial else {}))
    np.testing.assert_array_equal(env.reset_flat().cpu().numpy(), ora.reset())
    for e, st in scenes.items():
        env.set_state(e, st)
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    per_step = []
    prev = _counters(env, E)
    for s in range(steps):
        a = _actions(rng, E, scenes, s)
        og, rg, dg = env.step_flat(a, auto_reset=False)
        oc, rc, dc = ora.step(a)
        msg = "step %d" % s
        np.testing.assert_array_equal(dg.cpu().numpy(), dc, err_msg=msg + " dones")
        np.testing.assert_array_equal(rg.cpu().numpy(), rc, err_msg=msg + " rewards")
        np.testing.assert_array_equal(og.cpu().numpy(), oc, err_msg=msg + " observations")
        rows = env.get_states().cpu().numpy()
        for e in range(E):
            _assert_state_equal(ol.DrivingState.from_buffer_copy(rows[e].tobytes()), ora.get_state(e), msg + " env %d" % e)
        assert env.error_flags_per_env().cpu().numpy().tolist() == [0] * E, msg
        now = _counters(env, E)
        per_step.append(now - prev)
        prev = now
    assert env.error_flags() == 0 and ora.overflow() == 0 and ora.degenerate() == 0
    total = np.sum(per_step, axis=0)
    dc_ = env.debug_counters()
    # the checkpoint's rows are what dynenv_debug_counters sums
    names = ["fast", "quiescent", "contact", "slot_sum", "why_cand", "why_moving", "why_inert", "steady", "light", "split"]
    assert [int(total[:, k].sum()) for k in range(N_COUNTERS)] == [dc_[n] for n in names], (total.sum(0), dc_)
    env.close()
    ora.close()
    return np.array(per_step), dc_


def _check_counters(per_step, dc, E, steps, split_envs):
    # the packed counters still add up: every substep of every environment took exactly one of the four paths
    paths = per_step[:, :, FAST] + per_step[:, :, QUIET] + per_step[:, :, CONTACT] + per_step[:, :, STEADY]
    assert (paths == 10).all(), paths
    assert dc["fast"] + dc["quiescent"] + dc["contact"] + dc["steady"] == 10 * steps * E, dc
    assert (per_step[:, :, SLOTS] <= 10 * cs.DRV_NS).all() and (per_step[:, :, LIGHT:] <= 10).all()
    assert dc["split"] > 0, "no general multi-level solve: the call path kernel -> sweeps -> verdicts never ran"
    for e in split_envs:
        assert per_step[:, e, SPLIT].sum() > 0, "environment %d never took the split path: %s" % (e, per_step[:, e, SPLIT])


@pytest.mark.gpu
def test_all_solver_call_paths_full(gpu):
    E = 16
    scenes = _scenes()
    per_step, dc = _run(gpu, E, STEPS, scenes, partial=False)
    _check_counters(per_step, dc, E, STEPS, split_envs=(1, 7, 9, 12))
    # the split path and another solve in the same step of one environment: full-path substeps (contact path, no light-mode replay)
    # of which some, not all, ran the split sweeps
    full = per_step[:, :, CONTACT] - per_step[:, :, LIGHT]
    mixed = (per_step[:, :, SPLIT] > 0) & (per_step[:, :, SPLIT] < full)
    assert mixed.any(), "no environment mixed the split path with another solve within one step: split %s full-path %s" % (
        per_step[:, :, SPLIT].T.tolist(), full.T.tolist())
    # the environments without a split: coupled groups at rest (multi-level, bias only) and isolated arbiters stay off that path
    for e in (2, 4, 14):
        assert per_step[:, e, SPLIT].sum() == 0 and per_step[:, e, CONTACT].sum() > 0, (e, per_step[:, e].tolist())


@pytest.mark.gpu
def test_all_solver_call_paths_partial(gpu):
    """drv_step_partial_kernel shares the step's body"""
    E, steps = 8, 6
    scenes = {e: st for e, st in _scenes().items() if e < E}
    per_step, dc = _run(gpu, E, steps, scenes, partial=True)
    _check_counters(per_step, dc, E, steps, split_envs=(1, 7))
