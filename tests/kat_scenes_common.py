"""The differential scenes of tests/test_kat_general.py (the oracle), tests/test_gpu_kat_general.py (the HIP path) and
tools/kat_general_fuzz.py: the random scene populations, running them on a simulator given as (set, step, get), the classification of a
deviation, and the K5 / K6 checks.  A helper module: no test in here."""
import math

import numpy as np

import kat_general as kg
import kat_worlds as kw
import oracle_lib as ol


def _nudged(scene, rng, eps=1e-15):
    """the scene with every VELOCITY changed by a relative 1e-15 (one rounding error).  Positions and angles stay: exact zeros in them
    are structural (two feet created at one point with one angle keep the rotary limit joint inactive, quirk C14)"""
    def f(t, lo):
        return tuple(v * (1.0 + eps * rng.uniform(-1.0, 1.0)) if k >= lo else v for k, v in enumerate(t))
    if "cars" in scene:
        return dict(cars=[f(c, 4) for c in scene["cars"]], peds=[f(p, 2) for p in scene["peds"]], obst=scene["obst"])
    return dict(robots=[(f(L, 3), f(R, 3), t) for L, R, t in scene["robots"]], ball=f(scene["ball"], 2))


def classify(scene, dev, world, expected_fn, last):
    """a scene's deviation (oracle or HIP against kat_general) -> 'agree' | a catalogued class | 'UNEXPLAINED'"""
    if dev <= 1e-9:
        return "agree"
    if world.stats.get("cores_cross", 0):
        return "capsule cores cross"
    e1 = expected_fn(scene)[0]
    e2 = expected_fn(_nudged(scene, np.random.default_rng(1)))[0]
    own = kw.deviation(list(e1[last]), list(e2[last]))
    return "ill-conditioned scene" if dev <= 1e3 * own else "UNEXPLAINED"


def driving_scenes(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        sc = kw.driving_scene(rng)
        exp, world, ok = kw.driving_expected(sc)
        if ok:
            out.append((sc, exp, world))
    return out


def robocup_scenes(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        sc = kw.robocup_scene(rng)
        if not kw.valid_robocup_start(sc):
            continue
        exp, world, ok = kw.robocup_expected(sc)
        if ok:
            out.append((sc, exp, world))
    return out


def run_driving_on(sim_set, sim_step, sim_get, scenes, template):
    """set every scene on environment i, three env steps, -> deviations [n] from kat_general (largest over the three read-backs)"""
    for i, (sc, _, _) in enumerate(scenes):
        sim_set(i, kw.driving_state(template, sc))
    dev = np.zeros(len(scenes))
    for s in range(3):
        sim_step()
        for i, (_, exp, _) in enumerate(scenes):
            dev[i] = max(dev[i], kw.deviation(list(kw.driving_readback(sim_get(i))), list(exp[s])))
    return dev


def run_robocup_on(sim_set, sim_step, sim_get, scenes, template):
    for i, (sc, _, _) in enumerate(scenes):
        sim_set(i, kw.robocup_state(template, sc))
    sim_step()
    return np.array([kw.deviation(list(kw.robocup_readback(sim_get(i))), list(exp[0])) for i, (_, exp, _) in enumerate(scenes)])


def tally(scenes, dev, expected_fn, last):
    classes = {}
    for (sc, _, world), d in zip(scenes, dev):
        c = classify(sc, d, world, expected_fn, last)
        classes.setdefault(c, []).append(float(d))
    return classes


def events(scenes, what):
    return sum(sum(1 for ev in w.log if ev[1] == what) for _, _, w in scenes)


def _feet_scene(ora, env_idx, b_angle, dx, dy):
    """robot 5's feet at robot 0's left-foot position + (dx, dy), turned to b_angle; robot 0 at angle 0 -> the state blob"""
    st = ora.get_state(env_idx)
    A, B = st.robots[0], st.robots[5]
    for f in ("l", "r"):
        setattr(A, f + "a", 0.0)
        setattr(B, f + "a", b_angle)
        setattr(B, f + "px", A.lpx + dx)
        setattr(B, f + "py", A.lpy + dy)
    return st


def k5_check(sim_set, sim_step, sim_get, template):
    exp, world, ok = kw.driving_expected(K5_SCENE)
    assert ok and world.log == K5_LOG, world.log
    sim_set(0, kw.driving_state(template, K5_SCENE))
    for s in range(3):
        sim_step()
        assert kw.deviation(list(kw.driving_readback(sim_get(0))), list(exp[s])) < 1e-10, s
    got = kw.driving_readback(sim_get(0))
    for variant in (dict(drop_cache_on_separate=True), dict(apply_cached_on_retouch=True)):
        wrong = kw.driving_expected(K5_SCENE, **variant)[0][2]
        assert kw.deviation(list(got), list(wrong)) > 1e-3, (variant, "would have gone unnoticed")


def k6_scene(template):
    """K6: a crashed car (type 0) slides at 30 px/s into a LIVE pedestrian standing on the walkway strip.  Chipmunk orders an arbiter's
    shapes by shape type (circle before polygon: the pedestrian first) and swaps them for the callback when the first shape's
    collision type is not the handler's first declared type - `arbiter.shapes[0]` is the CAR in pedHit (handler (Car, Pedestrian),
    DrivingEnvironment.py:69,643-644).  Read the other way round, pedHit would take the pedestrian's velocity (0) for the car's, return
    False, and the pair would be ignored: the pedestrian would stay alive and unmoved."""
    st = ol.DrivingState.from_buffer_copy(template)
    st.elapsed, st.all_finished, st.n_peds, st.n_obst = 0, 0, 1, 0
    for k, y in zip(range(st.n_cars), (60.0, 135.0, 210.0, 285.0, 360.0, 640.0, 715.0, 790.0, 865.0, 940.0)):   # parked on the vertical road
        c = st.cars[k]
        c.px, c.py, c.vx, c.vy, c.angle, c.w = 892.5, y, 0.0, 0.0, math.pi / 2, 0.0
        c.dirx, c.diry, c.prevx, c.prevy = 0.0, 1.0, c.px, c.py
        c.type, c.finished, c.crashed, c.fric, c.lane_pos = 0, 1, 1, 1, 4
    c = st.cars[0]
    c.px, c.py, c.vx, c.vy, c.angle, c.dirx, c.diry = 300.0, 445.0, 30.0, 0.0, 0.0, 1.0, 0.0
    c.prevx, c.prevy = c.px, c.py
    p = st.peds[0]
    p.px, p.py, p.vx, p.vy = 316.0, 446.0, 0.0, 0.0            # the car's front face (x = 310) reaches the circle (r = 5) in 4 substeps
    p.road, p.side, p.dead, p.moving, p.speed, p.crossing, p.begin_crossing = 1, 0, 0, 100000, 4, 0, 0
    return st


def k6_check(sim_set, sim_step, sim_get, template):
    sim_set(0, k6_scene(template))
    sim_step()
    g = sim_get(0)
    car, ped = g.cars[0], g.peds[0]
    assert ped.dead == 1 and ped.moving == 0, "pedHit must have been handed the car first"
    assert ped.vx > 1.0 and car.vx < 29.0 and car.crashed == 1 and car.type == 0, (ped.vx, car.vx)
    # the same collision in the independent restatement (the pedestrian's velocity is zeroed by die() at `begin`, then the solve)
    w = kg.DrivingWorld([(0, 300.0, 445.0, 0.0, 30.0, 0.0, 0.0)], [(316.0, 446.0, 0.0, 0.0)], [])
    w.peds[0].fric = None                                      # alive until the hit (cpBodyUpdateVelocity: nothing); die() installs the friction
    for _ in range(10):
        w.step()
    assert w.peds[0].fric == kg.FRIC_PED_DEAD
    np.testing.assert_allclose([car.px, car.vx, car.w, ped.px, ped.py, ped.vx, ped.vy],
                               [w.cars[0].px, w.cars[0].vx, w.cars[0].w, w.peds[0].px, w.peds[0].py, w.peds[0].vx, w.peds[0].vy], rtol=1e-11, atol=1e-11)

# K5: frozen from the fuzz population (driving_scene(default_rng(33)), scene 31): cars 0 and 1 touch in substep 10, car 2 hits car 0
# in substep 12, cars 0 | 1 part in substep 14 and touch again in substep 15 - inside the persistence window, with a third body.
K5_SCENE = {'cars': [(1, 1544.4120503260542, 470.4683168673731, 1.5093479788450166, 101.24452194237047, 27.335516176848227, 1.6293065599236982),
                     (0, 1569.443454243659, 485.0360461127719, 0.9842063131329395, -0.0, 0.0, 0.0),
                     (1, 1519.1451356605219, 488.99995923270654, 3.135232723450839, 119.09322118218591, -23.052525498809487, 0.0),
                     (1, 1596.7966454338477, 493.53427924740305, -2.2774933724830184, -156.75509115512293, 7.916301057588406, 1.369630347824736),
                     (0, 892.5, 60.0, 1.5707963267948966, 0.0, 0.0, 0.0), (2, 892.5, 135.0, 1.5707963267948966, 0.0, 0.0, 0.0),
                     (1, 892.5, 210.0, 1.5707963267948966, 0.0, 0.0, 0.0), (2, 892.5, 285.0, 1.5707963267948966, 0.0, 0.0, 0.0),
                     (2, 892.5, 360.0, 1.5707963267948966, 0.0, 0.0, 0.0), (3, 892.5, 640.0, 1.5707963267948966, 0.0, 0.0, 0.0)],
            'peds': [(1493.3940026554483, 459.99519469552894, 9.321199999357635, 10.489392815254257)],
            'obst': [(1610.436704345423, 458.56864823223157)]}
K5_LOG = [(5, 'begin', 1, 3), (10, 'begin', 0, 1), (12, 'begin', 0, 2), (14, 'separate', 0, 1), (15, 'retouch', 0, 1), (15, 'begin', 0, 1),
          (28, 'separate', 0, 2)]
