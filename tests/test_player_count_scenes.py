"""The player-count scenes (tests/player_count_scenes.py), proven on the oracle alone: every batch the GPU tests run
(tests/test_gpu_player_counts.py: the same seeds, sizes, step counts and actions) reaches the contact path at its player count, so
those tests start from established preconditions instead of assumed ones.  Conditions on the INPUTS: a later change to a scene or a
seed that breaks one fails here, on a machine without a GPU.

  * the chain in environment 0 holds exactly A arbiters after every one of the 12 steps, at every A in 1..10, Full and Partial; the
    mixed chain in environment 4 peaks at one arbiter a car and one more a wedged pedestrian and never holds fewer than A;
  * the truncated scenario in environment 1 has contacts after at least 11 (pileup, A >= 3, peak 2) / 10 (obstacle) of the 12 steps;
  * RoboCup's column holds 2 n - 1 arbiters after every one of the 8 steps with the fall dice off, and peaks there with them on;
  * the rolling ball pays robot n - the first lane past the team split - its team's negative reward in at least 4 of the 8 steps;
  * random play from a random start has contacts of its own at n = 3 and 4;
  * nothing overflows, no capsule pair is degenerate."""
import numpy as np
import pytest

import capacity_scenes as cs
import oracle_lib as ol
import player_count_scenes as ps


def _run(family, players):
    """the batch's oracle over the tour -> (batch, active contacts [steps][E])"""
    c = ps.cfg(family, players)
    b = ps.OracleBatch(c, ps.seed_of(family, players))
    active = []
    for a in b.actions():
        b.ora.step(a)
        active.append([b.ora.active_contacts(e) for e in range(ps.E)])
    assert len(active) == ps.tour_steps(c)
    assert b.ora.overflow() == 0 and b.ora.degenerate() == 0
    return b, np.array(active)


@pytest.mark.parametrize("seed,mixed", [(1, False), (4, False), (5, True), (6, True)])
def test_the_chain_at_ten_cars_is_the_capacity_scene(seed, mixed):
    a, b = ol.DrivingState(), ol.DrivingState()
    a.n_cars = b.n_cars = 10
    assert cs.drv_chain10(a, seed, mixed) == ps.drv_chain(b, 10, seed, mixed)
    assert bytes(a) == bytes(b)


@pytest.mark.parametrize("A", range(1, 11))
def test_chain_order_and_types(A):
    st = ol.DrivingState()
    order = ps.drv_chain(st, A, 300 + A)
    assert sorted(order) == list(range(A)) and st.n_cars == A and st.n_peds == 0 and st.n_obst == 1
    xs = [st.cars[k].px for k in order]
    assert xs == sorted(xs), "`order` is the spatial order"
    assert [st.cars[k].vx for k in order] == [40.0] + [3.0] * (A - 1)
    st = ol.DrivingState()
    ps.drv_chain(st, A, 1300 + A, mixed=True)
    assert st.n_peds == min(3, A - 1, 8)
    if A >= 4:
        assert len(set(st.cars[k].type for k in range(A))) > 1


@pytest.mark.parametrize("family,players", [(f, n) for f, n in ps.TOUR + ps.CLAMPED if ps.FAMILIES[f].env_type == 1])
def test_driving_batches_reach_the_contact_path(oracle_built, family, players):
    b, active = _run(family, players)
    A = b.A
    assert A == min(players, 10)
    assert (active[:, ps.CHAIN_ENV] == A).all(), "the chain: A arbiters after every step: %s" % active[:, ps.CHAIN_ENV]
    assert b.ora.peak_arbiters(ps.CHAIN_ENV) == A == ps.chain_arbiters(b.blobs[ps.CHAIN_ENV])
    want = ps.chain_arbiters(b.blobs[ps.CHAIN2_ENV])
    assert want == A + min(3, A - 1)
    assert b.ora.peak_arbiters(ps.CHAIN2_ENV) == want and (active[:, ps.CHAIN2_ENV] >= A).all(), active[:, ps.CHAIN2_ENV]
    touched = int((active[:, ps.SCENARIO_ENV] > 0).sum())
    if ps.scenario_kind(A) == "pileup":
        assert touched >= 11 and b.ora.peak_arbiters(ps.SCENARIO_ENV) == 2, active[:, ps.SCENARIO_ENV]
    else:
        assert touched >= 10 and b.ora.peak_arbiters(ps.SCENARIO_ENV) == 1, active[:, ps.SCENARIO_ENV]
    g = b.ora.get_state(ps.CHAIN2_ENV)
    assert all(g.peds[k].dead for k in range(g.n_peds))


@pytest.mark.parametrize("kind,A", [("pileup", 3), ("pileup", 7), ("obstacle", 1), ("obstacle", 2), ("building", 1), ("building", 6)])
def test_scenarios_at_their_full_length(oracle_built, kind, A):
    """25 steps as in test_collision_scenarios: contacts after 24 (pileup, peak 2), 23 (obstacle) and 22 (building) of them"""
    ora = ol.OracleEnv(num_envs=1, n_players=A, seed=3)
    ora.reset()
    ora.set_state(0, ps.drv_scenario(kind, A))
    acts = np.ones((1, A, 2), np.int32)
    touched = 0
    for s in range(25):
        if s == ps.ACCELERATE_FROM:
            acts[:, 0, 0] = 2
        ora.step(acts)
        touched += ora.active_contacts(0) > 0
    assert touched == {"pileup": 24, "obstacle": 23, "building": 22}[kind]
    assert ora.peak_arbiters(0) == (2 if kind == "pileup" else 1) and ora.overflow() == 0


@pytest.mark.parametrize("family,players", [(f, n) for f, n in ps.TOUR + ps.CLAMPED if ps.FAMILIES[f].env_type == 0])
def test_robocup_batches_reach_the_contact_path(oracle_built, family, players):
    b, active = _run(family, players)
    R = b.A
    assert R == 2 * min(players, 5)
    for e in (ps.CHAIN_ENV, ps.CHAIN2_ENV):
        assert b.ora.peak_arbiters(e) == R - 1, "the column: 2 n - 1 arbiters at its peak (environment %d)" % e
        if family == "rc_resting":   # nobody falls: everything rests
            assert (active[:, e] == R - 1).all(), active[:, e]
    others = [e for e in range(ps.E) if e not in (ps.CHAIN_ENV, ps.BALL_ENV, ps.CHAIN2_ENV)]
    if (family, players) in ps.RANDOM_PLAY_CONTACTS:
        assert (active[:, others] > 0).any(), "random play from a random start has no contact of its own"


@pytest.mark.parametrize("family,players", [(f, n) for f, n in ps.TOUR + ps.CLAMPED if ps.FAMILIES[f].env_type == 0])
def test_the_rolling_ball_pays_team_rewards_next_to_the_second_teams_first_robot(oracle_built, family, players):
    """in at least 4 of the 8 steps the ball has moved in x (both teams' reward terms are nonzero) while robot n - the first lane past
    the team split - stands within 150 of it and is not among the last kickers: it is paid the negative half of ITS team's term"""
    c = ps.cfg(family, players)
    b = ps.OracleBatch(c, ps.seed_of(family, players))
    n = b.A // 2
    paid = 0
    for a in b.actions():
        before = b.ora.get_state(ps.BALL_ENV)
        b.ora.step(a)
        st = b.ora.get_state(ps.BALL_ENV)
        x, y = ps.robot_pos(st.robots[n])
        near = np.hypot(x - st.bpx, y - st.bpy) < 150.0
        kicked = n in list(st.last_kicked)[:st.n_last_kicked]
        paid += bool(st.bpx != before.bpx and near and not kicked and list(st.goals) == list(before.goals))
    assert paid >= 4, paid
