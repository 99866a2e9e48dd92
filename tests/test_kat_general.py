"""Differential tests of the oracle's `Space.step` (oracle/cp_lite.c - PARITY UNPINNED against pymunk, which this pipeline cannot
run) against tests/kat_general.py, a second restatement written from Chipmunk 7's published algorithm by ANOTHER ROUTE (GJK / EPA
closest features -> ContactPoints instead of SAT; feature-tuple contact ids; dict arbiter cache; unfused arithmetic; libm sin / cos).
CPU suite; tests/test_gpu_kat_general.py runs the same scenes through `dynenv_set_state` on the HIP path.

  (a) narrowphase: 10^5 random configurations per shape pair (rotated box-box incl. near-parallel faces and corner-corner,
      box-circle, capsule-capsule incl. parallel feet, capsule-circle, circle-circle): contact count, order, normal, both points
      and the contact ids to 1e-9; every disagreement must fall into one of the catalogued classes below;
  (b) 2000 random Driving scenes x 30 substeps and 500 RoboCup scenes x 50 substeps, full kinematic state to 1e-9, with the same
      rule: a scene above 1e-9 must be explained by a measured property of the scene (capsule cores crossing; ill-conditioning:
      a 1e-15 relative nudge of the inputs moves the independent restatement itself by more than the deviation / 1000);
  (c) KATs: re-contact inside collision_persistence with a third body (K5), handler argument order (K6), and the two plausible
      wrong readings of the re-contact rule shown to be caught by (b)'s population.
"""
import math

import numpy as np
import pytest

import kat_fuzz as kf
import kat_general as kg
import kat_worlds as kw
import oracle_lib as ol
from kat_scenes_common import _feet_scene, driving_scenes, events, k5_check, k6_check, robocup_scenes, run_driving_on, run_robocup_on, tally

# classes of narrowphase disagreement that are properties of the configuration, not of either implementation
EXPLAINED = {
    "contact at a threshold (|gap| < 1e-9): count differs",
    "two axes of equal depth (tie)",
    "capsule cores cross",
    "nearly parallel capsules (|sin| < 1e-6): normals differ by less than the misalignment",
    "circle centre on the polygon's boundary (|d| < 1e-6)",
}
N_PAIR = 100000


@pytest.fixture(scope="module", autouse=True)
def _built(oracle_built):
    return oracle_built


def test_constants_and_moments_agree_with_the_oracle():
    l = ol.lib()
    l.oracle_bias_coef.restype = __import__("ctypes").c_double
    assert abs(l.oracle_bias_coef(0) - (1.0 - kg.COLLISION_BIAS ** kg.DT)) < 1e-17
    assert abs(l.oracle_bias_coef(1) - (1.0 - 0.1 ** kg.DT)) < 1e-17
    for t in range(4):
        m, hx, hy = kg.CAR_M[t], kg.CAR_HX[t], kg.CAR_HY[t]
        assert abs(l.oracle_moment_for_box(m, hx, hy) / kg.moment_for_box(m, hx, hy) - 1.0) < 1e-15
    assert abs(l.oracle_moment_for_circle(10.0, 0.0, 10.0) - kg.moment_for_circle(10.0, 0.0, 10.0)) < 1e-12
    for yo in (10.0, -10.0):
        assert abs(l.oracle_moment_for_segment(4000.0, -10.0, yo, 10.0, yo, 7.5) / kg.moment_for_segment(4000.0, -10.0, yo, 10.0, yo, 7.5) - 1.0) < 1e-15


@pytest.mark.parametrize("pair", kf.PAIRS)
def test_narrowphase_fuzz_gjk_epa_against_the_oracle(pair):
    A, B = kf.generate(pair, N_PAIR, 20261004)
    res = kf.compare(pair, A, B, kf.oracle_collide(A, B))
    assert res["colliding"] > 0.4 * N_PAIR, "the generator must produce contacts"
    unexplained = {c: n for c, n in res["classes"].items() if c not in EXPLAINED}
    assert not unexplained, (unexplained, {c: res["examples"][c] for c in unexplained})
    assert res["agree"] + sum(res["classes"].values()) == N_PAIR
    assert res["agree"] >= 0.99 * N_PAIR, res["classes"]
    if pair in ("box_circle", "capsule_circle", "circle_circle"):
        assert res["agree"] == N_PAIR, res["classes"]


@pytest.mark.parametrize("pair", ("box_box", "box_circle", "capsule_capsule"))
def test_narrowphase_fuzz_with_gjk_warm_started_like_chipmunk(pair):
    """Chipmunk starts GJK from the closest features of the pair's previous call (the collision id); the answer must not depend on it"""
    A, B = kf.generate(pair, 20000, 7)
    res = kf.compare(pair, A, B, kf.oracle_collide(A, B), warm=True)
    unexplained = {c: n for c, n in res["classes"].items() if c not in EXPLAINED}
    assert not unexplained, (unexplained, {c: res["examples"][c] for c in unexplained})
    assert res["agree"] >= 0.99 * 20000


# ------------------------------------------------------------------------------------------------ scenes


def test_driving_scenes_full_state_against_the_oracle():
    n = 2000
    scenes = driving_scenes(n, 7)
    ora = ol.OracleEnv(env_type=1, num_envs=n, n_players=10, seed=5, threads=8)
    ora.reset()
    acts = np.ones((n, 10, 2), np.int32)
    dev = run_driving_on(ora.set_state, lambda: ora.step(acts), ora.get_state, scenes, ora.get_state(0))
    assert ora.overflow() == 0
    classes = tally(scenes, dev, kw.driving_expected, 2)
    assert "UNEXPLAINED" not in classes, classes["UNEXPLAINED"]
    assert len(classes["agree"]) >= 0.995 * n, {k: len(v) for k, v in classes.items()}
    # what the population exercised: first touches, separations, re-touches inside collision_persistence, EPA on rotated boxes
    assert events(scenes, "begin") > 3 * n and events(scenes, "separate") > n and events(scenes, "retouch") > 300
    assert sum(w.stats.get("epa_calls", 0) for _, _, w in scenes) > 20 * n


def test_robocup_scenes_full_state_against_the_oracle():
    n = 500
    scenes = robocup_scenes(n, 11)
    ora = ol.OracleEnv(env_type=0, num_envs=n, n_players=5, seed=3, flags=ol.FLAG_USE_OBS_REWARDS, threads=8)   # canFall off
    ora.reset()
    a = np.zeros((n, 10, 4), np.int32)
    a[..., 3] = 3                                              # head action 3 = none
    dev = run_robocup_on(ora.set_state, lambda: ora.step(a), ora.get_state, scenes, ora.get_state(0))
    assert ora.overflow() == 0
    classes = tally(scenes, dev, lambda sc: kw.robocup_expected(sc), 0)
    assert "UNEXPLAINED" not in classes, classes["UNEXPLAINED"]
    assert len(classes["agree"]) >= 0.96 * n, {k: len(v) for k, v in classes.items()}
    assert events(scenes, "begin") > 2 * n and events(scenes, "separate") > n and events(scenes, "retouch") > 100
    # error bit 4 stays down (the population's one "capsule cores cross" scene is kat_general's EPA answering -20 for the two exactly
    # parallel feet of ONE robot, 20 px apart - a degenerate Minkowski difference; the cores do not touch)
    assert ora.degenerate() == 0


def test_crossed_capsule_cores_get_chipmunks_normal_and_degenerate_ones_are_reported():
    """VERDICT r5 item 5, and what it turned up: a foot laid ACROSS another foot has no closest-point normal (the crossing point is computed
    twice: d = 0 or rounding noise).  Chipmunk's EPA gives the minimum-translation axis there; so do the oracle and the kernels since
    round 6 (oracle/cp_lite.c cores_crossing_normal) - the capsule-capsule fuzz has no "cores cross" class any more - and what is left
    for error bit 4 is the measure-zero case in which even that normal's sign is a convention: cores exactly collinear / exactly touching.
    Sticky until reset / set_state."""
    import math
    ora = ol.OracleEnv(env_type=0, num_envs=4, n_players=5, seed=3, flags=ol.FLAG_USE_OBS_REWARDS, threads=1)
    ora.reset()
    a = np.zeros((4, 10, 4), np.int32)
    a[..., 3] = 3
    # 1: B turned by 90 degrees, its left core (the vertical segment x = Bx - 10, By - 10 .. By + 10) crossing A's left core (y = Ay + 10) 1 px
    #    from B's lower end: the minimum translation pushes B up by ~1 px, and after the step B has moved UP, not sideways
    ora.set_state(1, _feet_scene(ora, 1, math.pi / 2, 10.0, 19.0))
    # 2: B beside A, same angle, B's right core 1e-3 px above A's left core (capsules 15 px deep): close, not crossing, nothing to report
    ora.set_state(2, _feet_scene(ora, 2, 0.0, 0.0, 20.0 + 1e-3))
    # 3: B's right core exactly ON A's left core (collinear, overlapping): every candidate distance is 0 - reported
    ora.set_state(3, _feet_scene(ora, 3, 0.0, 5.0, 20.0))
    y0 = ora.get_state(1).robots[5].lpy
    l = ol.lib()
    l.oracle_cp_cores_cross.restype = C_long = __import__("ctypes").c_long
    before = l.oracle_cp_cores_cross()
    ora.step(a)
    assert l.oracle_cp_cores_cross() > before
    assert [ora.degenerate_env(i) for i in range(4)] == [0, 0, 0, 16]
    assert ora.get_state(1).robots[5].lpy > y0 + 0.01, "the crossing foot is pushed back along the minimum-translation axis (up)"
    assert ora.degenerate() == 16
    ora.set_state(3, ora.get_state(0))
    assert ora.degenerate() == 0


def test_scene_outcomes_do_not_depend_on_the_gjk_warm_start():
    """Chipmunk starts a pair's GJK from the closest features of its previous step (the collision id cached in the BB-tree pair);
    kat_general does the same by default.  Started cold in every step the scenes must come out the same (to 1e-9, ill-conditioned
    scenes aside): the cache is an accelerator, not a semantic."""
    scenes = driving_scenes(300, 5)
    dev = np.array([kw.deviation(list(exp[2]), list(kw.driving_expected(sc, warm_gjk=False)[0][2])) for sc, exp, _ in scenes])
    assert (dev <= 1e-9).mean() >= 0.99 and np.median(dev) < 1e-12, (np.sort(dev)[-5:],)
    scenes = robocup_scenes(100, 5)
    dev = np.array([kw.deviation(list(exp[0]), list(kw.robocup_expected(sc, warm_gjk=False)[0][0])) for sc, exp, _ in scenes])
    assert (dev <= 1e-9).mean() >= 0.95 and np.median(dev) < 1e-12, (np.sort(dev)[-5:],)


def test_capsule_cores_cross_rarely_in_play_and_never_degenerately():
    """Round 5 claimed that capsule cores never cross in play - its counter waited for a closest distance of exactly 0, and a crossing comes
    out as ~1e-15.  They do (the two feet of a robot that has been knocked about: 1 environment in 4096 per episode); since round 6 those
    calls take Chipmunk's minimum-translation normal.  What stays impossible in play is the DEGENERATE case (error bit 4)."""
    import ctypes as C
    l = ol.lib()
    l.oracle_cp_cores_cross.restype = C.c_long
    before = l.oracle_cp_cores_cross()
    E = 256
    env = ol.OracleEnv(env_type=0, num_envs=E, n_players=5, seed=42, flags=ol.ROBOCUP_DEFAULT_FLAGS, threads=8)
    env.reset()
    rng = np.random.default_rng(0)
    contacts = 0
    for s in range(240):
        env.step_noobs(np.stack([rng.integers(0, k, (E, 10)) for k in (5, 3, 3, 7)], -1).astype(np.int32))
        contacts += sum(env.active_contacts(e) for e in range(0, E, 16))
    assert contacts > 50, "the episode must contain contacts"
    assert l.oracle_cp_cores_cross() - before < 200 and env.degenerate() == 0


def test_wrong_readings_of_the_recontact_rule_would_be_caught():
    """Chipmunk keeps a separated pair's arbiter - contacts and accumulated impulses included - for collision_persistence = 3 steps.
    On a re-touch inside that window `begin` fires again, the old impulses ARE carried over by contact id, and
    cpArbiterApplyCachedImpulse is skipped (the arbiter is in its first-contact state).  Two plausible wrong readings - forget the
    impulses at `separate`; apply them on the re-touch - move the outcome of every scene whose re-touching contact still carried an
    impulse (a pair usually parts BECAUSE its impulse has gone to zero; with a third body pushing it does not) far beyond the 1e-9 at
    which the oracle agrees with the right reading (test_driving_scenes_...; K5 freezes one such scene)."""
    scenes = [s for s in driving_scenes(600, 33) if any(ev[1] == "retouch" for ev in s[2].log)]
    assert len(scenes) > 50
    for variant in (dict(drop_cache_on_separate=True), dict(apply_cached_on_retouch=True)):
        moved = sum(kw.deviation(list(exp[2]), list(kw.driving_expected(sc, **variant)[0][2])) > 1e-6 for sc, exp, _ in scenes)
        assert moved >= 5, (variant, moved, len(scenes))


def test_k5_recontact_inside_the_persistence_window_with_a_third_body():
    ora = ol.OracleEnv(env_type=1, num_envs=1, n_players=10, seed=5)
    ora.reset()
    acts = np.ones((1, 10, 2), np.int32)
    k5_check(ora.set_state, lambda: ora.step(acts), ora.get_state, ora.get_state(0))


def test_k6_handler_argument_order_the_car_comes_first():
    ora = ol.OracleEnv(env_type=1, num_envs=1, n_players=10, seed=5)
    ora.reset()
    acts = np.ones((1, 10, 2), np.int32)
    k6_check(ora.set_state, lambda: ora.step(acts), ora.get_state, ora.get_state(0))
