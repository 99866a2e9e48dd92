"""The capacity scenes (tests/capacity_scenes.py), proven on the oracle alone: each scene reaches what it is for, so the GPU tests
(tests/test_gpu_contact_capacity.py) start from established preconditions instead of assumed ones.

  * the load counter itself (OracleEnv.peak_arbiters: cleared by reset and set_state, leaves pairs out that the kernels never see);
  * Driving: peaks of exactly 24 and 25 arbiters, isolated and coupled; chains ten arbiters deep in a permuted canonical order;
    60 candidates in 4 passes with first contacts in passes 0, 1, 2 of one substep and later first contacts in front of and behind
    cached pairs; exactly 128 and 129 candidates with the touching pair at the list's very end;
  * RoboCup: peaks of exactly 16 and 17 without a degenerate capsule pair; a chain of nine arbiters through ten robots' joints;
  * a record of how far random play stays from the tables' capacities (printed: pytest -s).

NOT built: a RoboCup scene with more than 64 candidates (two narrowphase passes of 64) and at most 16 arbiters.  The candidate rule
(robocup_kernels.hip, "broadphase") is: the ten pairs (left foot, right foot) of one robot always, every other pair when the boxes
intersect.  Ten feet pairs and at most 16 touching pairs leave 39 pairs to find whose boxes intersect while the shapes stay apart;
the box of an axis-parallel capsule has slack at its four corners only, and in the arrangements of rotated robots tried here the
feet that came near enough for their boxes to intersect touched.  It is not shown to be impossible, it was not found: the second
RoboCup pass stays without a test.
"""
import numpy as np
import pytest

import capacity_scenes as cs
import oracle_lib as ol


COAST = np.ones((1, 10, 2), np.int32)
RC_IDLE = np.zeros((1, 10, 4), np.int32)
RC_IDLE[..., 3] = 3   # head action 3 = no head turn; nobody walks, turns or kicks


def _drv(scene, **kw):
    ora = ol.OracleEnv(num_envs=1, n_players=10, seed=3)
    ora.reset()
    st = ora.get_state(0)
    ret = scene(st, **kw)
    ora.set_state(0, st)
    return ora, st, ret


def _rc(scene, flags=8, **kw):
    ora = ol.OracleEnv(env_type=0, num_envs=1, n_players=5, seed=3, flags=flags)
    ora.reset()
    st = ora.get_state(0)
    scene(st, **kw)
    ora.set_state(0, st)
    return ora, st


# ------------------------------------------------------------------------------------------------ the counter
def test_peak_counter_is_cleared_by_reset_and_set_state(oracle_built):
    ora, st, _ = _drv(cs.drv_full)
    assert ora.peak_arbiters(0) == 0, "set_state clears it"
    ora.step(COAST)
    assert ora.peak_arbiters(0) == 24
    ora.set_state(0, ora.get_state(0))
    assert ora.peak_arbiters(0) == 0
    ora.step(COAST)
    assert ora.peak_arbiters(0) == 24
    ora.reset()
    assert ora.peak_arbiters(0) == 0


def test_peak_counter_leaves_out_the_pairs_the_kernels_never_enumerate(oracle_built):
    """pedestrian-pedestrian and pedestrian-static pairs get an arbiter in the reference (its `begin` always rejects); the kernels collide
    car pairs only, so those hold no slot and are not counted"""
    ora, st, _ = _drv(cs.drv_full)
    st = ora.get_state(0)
    st.n_peds = 8
    for k in range(4, 8):   # four coincident dead pedestrians inside obstacle 0, away from car 0's box: 6 + 4 arbiters of the reference
        cs._dead_ped(st.peds[k], st.obst_x[0] - 4.0, st.obst_y[0] + 4.0)
    assert len(cs.drv_candidates(st)) == 24, "no car pair was added"
    ora.set_state(0, st)
    ora.step(COAST)
    assert ora.peak_arbiters(0) == 24 and ora.overflow() == 0


# ------------------------------------------------------------------------------------------------ Driving: 24 and 25
@pytest.mark.parametrize("scene,want", [(cs.drv_full, 24), (cs.drv_over, 25), (cs.drv_full_coupled, 24), (cs.drv_over_coupled, 25)])
def test_driving_table_scenes_peak_at_and_one_past_capacity(oracle_built, scene, want):
    ora, st, _ = _drv(scene)
    assert len(cs.drv_candidates(st)) == want, "every candidate of these scenes touches"
    for s in range(12):
        ora.step(COAST)
        if s == 0:
            assert ora.peak_arbiters(0) == want, "the table is at its peak from the first step on"
    assert ora.peak_arbiters(0) == want and ora.overflow() == 0
    if scene in (cs.drv_full, cs.drv_over):   # 20 solved (car | obstacle), the pedestrians' pairs rejected by pedHit yet counted
        assert ora.active_contacts(0) == 20
        assert all(st.peds[k].dead for k in range(st.n_peds))


def test_driving_coupled_table_holds_coupled_arbiters(oracle_built):
    ora, st, _ = _drv(cs.drv_full_coupled)
    ora.step(COAST)
    assert ora.active_contacts(0) == 24, "all 24 are solved, in five groups that share bodies"
    pairs = cs.drv_candidates(st)
    assert sum(1 for i, j in pairs if j < 10) == 5
    for i in range(10):
        assert sum(1 for a, b in pairs if i in (a, b)) == (3 if i < 9 else 2), "car %d: its neighbour, the obstacle at its end, one on top (not car 9)" % i


# ------------------------------------------------------------------------------------------------ Driving: chains
@pytest.mark.parametrize("seed,mixed", [(1, False), (2, False), (3, False), (4, False), (5, True), (6, True)])
def test_driving_chain_is_ten_arbiters_deep(oracle_built, seed, mixed):
    ora, st, order = _drv(cs.drv_chain10, seed=seed, mixed=mixed)
    assert sorted(order) == list(range(10)) and order != sorted(order), "canonical order must differ from the spatial order"
    xs = [st.cars[k].px for k in order]
    assert xs == sorted(xs), "`order` is the spatial order"
    if mixed:
        assert st.n_peds == 3 and len(set(st.cars[k].type for k in range(10))) > 1
    deep = 0
    for s in range(8):
        ora.step(COAST)
        deep = max(deep, ora.active_contacts(0))
    assert deep >= 10 + (3 if mixed else 0), deep
    assert ora.peak_arbiters(0) == 10 + (3 if mixed else 0) and ora.overflow() == 0
    g = ora.get_state(0)
    assert all(g.peds[k].dead for k in range(g.n_peds))


# ------------------------------------------------------------------------------------------------ Driving: passes
def _peak_after_one_step(st):
    ora = ol.OracleEnv(num_envs=1, n_players=10, seed=3)
    ora.reset()
    ora.set_state(0, st)
    ora.step(COAST)
    return ora.peak_arbiters(0)


def test_driving_passes_scene(oracle_built):
    ora, st, _ = _drv(cs.drv_passes)
    cand = cs.drv_candidates(st)
    assert len(cand) == 60 > 2 * cs.DRV_PASS
    own = [(k, 30 + o) for o, k in enumerate((1, 2, 3, 4))]   # each car's own obstacle
    # which pairs touch, shown by taking obstacles away (far off, into a building): exactly the four own pairs
    assert _peak_after_one_step(st) == 4

    def without(obstacles):
        ora2, st2, _ = _drv(cs.drv_passes)
        for o in obstacles:
            st2.obst_x[o], st2.obst_y[o] = 1300.0, 800.0
        return st2
    assert _peak_after_one_step(without(range(4, 20))) == 4, "the stack's 56 pairs never touch"
    assert _peak_after_one_step(without(range(0, 4))) == 0
    for o in range(4):
        assert _peak_after_one_step(without([o])) == 3
    passes = [cand.index(p) // cs.DRV_PASS for p in own]
    assert passes == [0, 0, 1, 2], "first contacts in passes 0, 1 and 2 of the first substep: %s" % passes
    # later: car 0 reaches obstacle 18 (its pair is the list's first), then car 9 obstacle 19 (the list's last)
    peaks, lists = [], []
    for s in range(8):
        ora.step(COAST)
        peaks.append(ora.peak_arbiters(0))
        lists.append(cs.drv_candidates(ora.get_state(0)))
    assert peaks[0] == 4 and peaks[-1] == 6 and ora.overflow() == 0
    s0 = peaks.index(5)
    s9 = peaks.index(6)
    assert 0 < s0 < s9, "car 0 arrives first, in a later step than the first; car 9 after it: %s" % peaks
    assert lists[s0][0] == (0, 48) and lists[s0].index((0, 48)) // cs.DRV_PASS == 0
    assert [lists[s0].index(p) // cs.DRV_PASS for p in own] == [0, 1, 1, 2], "cached pairs are re-touched in later passes than the new one"
    assert lists[s9][-1] == (9, 49) and len(lists[s9]) == 62 and (len(lists[s9]) - 1) // cs.DRV_PASS == 3, "a first contact in the last pass"
    assert max(peaks) <= cs.DRV_NS


@pytest.mark.parametrize("over,want", [(False, 128), (True, 129)])
def test_driving_candidate_list_scenes(oracle_built, over, want):
    ora, st, _ = _drv(cs.drv_clist, over=over)
    cand = cs.drv_candidates(st)
    assert len(cand) == want
    assert cand[-1] == (8, 49), "the list's last pair is car 8 | its own obstacle: the one that touches"
    assert cand.index((8, 49)) == want - 1 and cand.index((1, 48)) == (19 if over else 18)   # behind car 0's pairs and car 1's 16 with stack A
    if over:
        assert cand[0] == (0, 9)
    for s in range(10):
        ora.step(COAST)
        assert cs.drv_candidates(ora.get_state(0)) == cand, "the candidate set must not change while the scene runs (step %d)" % s
    assert ora.peak_arbiters(0) == 2 <= cs.DRV_NS and ora.active_contacts(0) == 2 and ora.overflow() == 0


# ------------------------------------------------------------------------------------------------ RoboCup
@pytest.mark.parametrize("flags", [8, ol.ROBOCUP_DEFAULT_FLAGS])
@pytest.mark.parametrize("scene,want", [(cs.rc_full, 16), (cs.rc_over, 17)])
def test_robocup_table_scenes_peak_at_and_one_past_capacity(oracle_built, scene, want, flags):
    ora, st = _rc(scene, flags=flags)
    for s in range(8):
        ora.step(RC_IDLE)
        if s == 0:
            assert ora.peak_arbiters(0) == want
    assert ora.peak_arbiters(0) == want and ora.degenerate() == 0 and ora.overflow() == 0
    if flags == 8:   # nobody falls: everything rests
        assert ora.active_contacts(0) == want


def test_robocup_chain_is_nine_arbiters_through_the_joints(oracle_built):
    ora, st = _rc(cs.rc_chain)
    deep = 0
    for s in range(8):
        ora.step(RC_IDLE)
        deep = max(deep, ora.active_contacts(0))
    assert deep >= 9 and ora.peak_arbiters(0) == 9 and ora.degenerate() == 0 and ora.overflow() == 0
    g = ora.get_state(0)
    assert g.robots[9].lpy > st.robots[9].lpy + 0.5, "the push on robot 0 has reached the far end of the column"


# ------------------------------------------------------------------------------------------------ headroom (a record, not a gate)
def test_random_play_stays_inside_the_tables(oracle_built):
    """How full the tables get in random play: 512 Driving environments x one 600-step episode with 10 cars, 256 RoboCup environments
    x one 240-step episode with 5 robots a team, seed 42.  Recorded in profiles/HISTORY.md: Driving peaks at 5 of 24, RoboCup at 4 of 16."""
    E = 512
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=42, threads=8)
    ora.reset()
    rng = np.random.default_rng(42)
    for s in range(600):
        ora.step_noobs(rng.integers(0, 3, size=(E, 10, 2)).astype(np.int32))
    drv = np.bincount([ora.peak_arbiters(e) for e in range(E)])
    print("\nDriving: environments by peak arbiter count (0, 1, ...):", drv.tolist())
    assert len(drv) - 1 <= cs.DRV_NS and ora.overflow() == 0
    E = 256
    ora = ol.OracleEnv(env_type=0, num_envs=E, n_players=5, seed=42, flags=ol.ROBOCUP_DEFAULT_FLAGS, threads=8)
    ora.reset()
    for s in range(240):
        a = np.stack([rng.integers(0, 5, (E, 10)), rng.integers(0, 3, (E, 10)), rng.integers(0, 3, (E, 10)), rng.integers(0, 7, (E, 10))], -1)
        ora.step_noobs(a.astype(np.int32))
    rc = np.bincount([ora.peak_arbiters(e) for e in range(E)])
    print("RoboCup: environments by peak arbiter count (0, 1, ...):", rc.tolist())
    assert len(rc) - 1 <= cs.RC_NS and ora.overflow() == 0
