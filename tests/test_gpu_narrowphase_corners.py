"""The pair tests of the Driving narrowphase on cached car corners, ContactPoints shared by a quad's lanes (-m gpu, plus one CPU test
of the scenes' preconditions on the oracle).

The position update of a substep stores the four world corners of every car it moved (or turned) in the LDS tile; the pair tests of
the contact path read them instead of transforming (+-hx, +-hy) again, a static box's corner is one add per component, and the two
candidate contacts of ContactPoints are evaluated on lanes 0 and 1 of the pair's quad and assembled on lane 0.  What can go wrong: a
corner that is stale (a frozen car keeps the corners of an earlier substep; a car that steers in place has no velocity), read from
the wrong row (the per-car arrays have exactly ten rows now) or overwritten (the mailbox of an earlier pass of sixteen pairs), and
the two candidates in the wrong order or with the other's contact id.  All of it changes a contact point or an id, i.e. the state
blob within a step.

One handle of 16 ten-car environments and one of 4 three-car environments, 12 steps, every step bit for bit against the oracle
(observations, rewards, dones, state blobs), Full and Partial + Realistic noise 3 (both step kernels inline the narrowphase):

  face_on           two cars slide into each other face on face: two contacts, both cars moving
  corner_a / _b     a turned car and a straight one slide into each other, corner into face: one contact; the turned car is the
                    lower index (shape a) in one, the higher (shape b) in the other, and the contact at either end of the face
  frozen_hit / _t   a car slides into one that has been at rest - frozen - since the first substep (straight / turned by 0.3)
  steer_in_place    a car at rest, not crashed, 0.2 above a resting car's face, steers by 2 degrees at substep 0: only the turn
                    brings its corner into the face.  (The contact crashes it, so it steers once.)
  statics           a turned car slides into an obstacle, another one into a building's face: the static corner as one add
  chain             capacity_scenes.drv_chain10, mixed: car-car, car-pedestrian and car-obstacle pairs in one pass, all moving
  drv_passes        four passes of sixteen, slots handed out in three of them: cached corners survive the mailbox writes
  drv_clist         the full list of 128 candidates
  oblique, head_on, pileup, building (parity_common._scenario): cars under power, 1 or 2 contacts, chained arbiters
  steady_pile       the recorded pile of tests/test_gpu_verdict_batch.py: bias velocities turn cars by sub-ulp amounts in every substep
  three cars        the second handle (n_players = 3): the pile-up and face_on - the car rows of a lane that is no car are clamped

The CPU test checks on the oracle that each scene reaches its situation, and that ContactPoints comes out all three ways somewhere:
both candidates, the first alone, the second alone.  It reads that off the oracle's own narrowphase (oracle_cp_collide_batch) on a
pair's geometry at the end of a step - the geometry the step's last substep tested, positions change only in a substep's update:
with one contact, its id on shape a is the start of a's support edge for the first candidate and the end of it for the second.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import capacity_scenes as cs
import oracle_lib as ol
import player_count_scenes as pcs
from capacity_scenes import CAR_HX, CAR_HY, _park, _turn
from kat_scenes_r4 import CY, _place_crashed_car
from parity_common import _assert_state_equal, _scenario

SEED = 57
STEPS = 12
E, E3 = 16, 4
PART = dict(obs_type=1, noise_type=1, noise_magnitude=3.0)
X0 = 300.0
STEER_ENV, STEADY_ENV = 6, 14
_PILE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drv_steady_pile.npz"))


def _begin(st, used, n_obst=0):
    st.n_peds, st.n_obst = 0, n_obst
    _park(st, [k for k in range(10) if k not in used])


def _car(st, k, x, y=CY, vx=0.0, vy=0.0, angle=0.0, t=0):
    _place_crashed_car(st.cars[k], t, x, y, vx)
    st.cars[k].vy = vy
    if angle != 0.0:
        _turn(st.cars[k], angle)


def _ext(angle, t=0):
    """half the width of a car's bounding box"""
    return abs(math.cos(angle)) * CAR_HX[t] + abs(math.sin(angle)) * CAR_HY[t]


def face_on(st):
    _begin(st, (0, 1))
    _car(st, 0, X0, vx=30.0)
    _car(st, 1, X0 + 20.0 + 4.0, CY + 2.0, vx=-30.0)


def corner_a(st, ang=0.6):
    _begin(st, (0, 1))
    _car(st, 0, X0, vx=30.0, angle=ang)
    _car(st, 1, X0 + _ext(ang) + 10.0 + 4.0, CY + 1.0, vx=-30.0)


def corner_b(st, ang=-0.6):
    _begin(st, (0, 1))
    _car(st, 0, X0, vx=30.0)
    _car(st, 1, X0 + _ext(ang) + 10.0 + 4.0, CY - 1.0, vx=-30.0, angle=ang)


def frozen_hit(st, ang=0.0, gap=4.0):
    _begin(st, (0, 1))
    _car(st, 0, X0, vx=30.0)
    _car(st, 1, X0 + 10.0 + gap + _ext(ang), CY + 1.5, angle=ang)


def frozen_hit_turned(st):
    frozen_hit(st, ang=0.3, gap=6.0)


def steer_in_place(st):
    """car 0 rests; car 1, a car like any other at rest (not crashed: it takes its action), lies 0.2 above car 0's upper face"""
    _begin(st, (0, 1))
    _car(st, 0, X0)
    _car(st, 1, X0, CY + 2.0 * CAR_HY[0] + 0.2)
    c = st.cars[1]
    c.finished, c.crashed, c.fric, c.lane_pos = 0, 0, 0, 1


def statics(st):
    _begin(st, (0, 1), n_obst=1)
    _car(st, 0, X0, vx=30.0, angle=0.5)
    st.obst_x[0], st.obst_y[0] = X0 + _ext(0.5) + 10.0 + 4.0, CY + 2.0
    _car(st, 1, X0 + 200.0, 425.0 + CAR_HY[0] + 3.0, vy=-30.0)      # the building's face is y = 425


SCENES = {1: face_on, 2: corner_a, 3: corner_b, 4: frozen_hit, 5: frozen_hit_turned, STEER_ENV: steer_in_place, 8: statics,
          9: lambda st: cs.drv_chain10(st, seed=5, mixed=True), 10: cs.drv_passes, 11: cs.drv_clist}
SCENARIOS = {7: "oblique", 12: "pileup", 13: "building", 15: "head_on"}
CAR_CAR = (1, 2, 3, 4, 5, STEER_ENV, 7, 12, 15)   # environments whose cars 0..2 meet each other


def _scenes():
    """environment -> state blob; environment 0 keeps its reset state and plays randomly"""
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
    pile = ol.DrivingState.from_buffer_copy(_PILE["blob"].tobytes())
    pile.elapsed = 0
    out[STEADY_ENV] = pile
    return out


def _scenes3():
    """the three-car handle: the pile-up and face_on; environments 0 and 3 play randomly"""
    ref = ol.OracleEnv(num_envs=1, n_players=3, seed=SEED)
    ref.reset()
    st = ref.get_state(0)
    face_on(st)
    st.n_cars, st.elapsed = 3, 0
    ref.close()
    pile = pcs.drv_scenario("pileup", 3)
    pile.elapsed = 0
    return {1: pile, 2: st}


def _actions(rng, n_env, A, scenes, step, ten):
    a = rng.integers(0, 3, size=(n_env, A, 2)).astype(np.int32)
    for e in scenes:
        a[e] = 1                         # coast
    if ten:
        a[STEER_ENV, 1, 1] = 2           # car 1 steers
        a[7, :2, 0] = a[15, :2, 0] = 2   # oblique, head_on: under power (coasting cars brake and never meet)
        a[STEADY_ENV] = _PILE["actions"][step]
    return a


def _outcome(ci, cj):
    """ContactPoints of car i (shape a) against car j on the oracle: None (apart), "both", "first" or "second\""""
    desc = np.zeros((2, 9))
    for d, c in zip(desc, (ci, cj)):
        d[:6] = 2.0, c.px, c.py, c.angle, CAR_HX[c.type], CAR_HY[c.type]
    out = np.zeros(15)
    ol.lib().oracle_cp_collide_batch(1, desc[0].ctypes.data_as(C.c_void_p), desc[1].ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if out[1] == 0:
        return None
    if out[1] == 2:
        return "both"
    assert out[2] == 0.0                 # two boxes are never swapped
    # a's support edge: the edge whose normal points most along n; edge k runs from corner k - 1 to corner k (box_world's order)
    c, s = math.cos(ci.angle), math.sin(ci.angle)
    dots = [(c * nx - s * ny) * out[3] + (s * nx + c * ny) * out[4] for nx, ny in ((-1.0, 0.0), (0.0, -1.0), (1.0, 0.0), (0.0, 1.0))]
    k = int(np.argmax(dots))
    if sorted(dots)[-1] - sorted(dots)[-2] < 1e-6:
        return "tie"                     # n half way between two faces of a: not classified
    ida = (int(out[9]) - 1) >> 8         # slot of shape a is 0: its contact id is the corner
    assert ida in ((k + 3) & 3, k), (ida, k)
    return "first" if ida == ((k + 3) & 3) else "second"


def test_scenes_reach_what_they_are_for(oracle_built):
    """CPU: what the oracle can tell of the scenes over the 12 steps of the GPU test"""
    scenes = _scenes()
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4)
    ora.reset()
    for e, st in scenes.items():
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    act = {e: [] for e in scenes}
    cars = {e: [] for e in scenes}       # per step: the state's cars
    outcomes = {e: [] for e in CAR_CAR}
    for s in range(STEPS):
        ora.step(_actions(rng, E, 10, scenes, s, True))
        for e in scenes:
            act[e].append(ora.active_contacts(e))
            st = ora.get_state(e)
            cars[e].append(st.cars)
            if e in CAR_CAR:
                outcomes[e].append([_outcome(st.cars[i], st.cars[j]) for i, j in ((0, 1), (0, 2), (1, 2))])
    assert ora.overflow() == 0 and ora.degenerate() == 0
    seen = {e: set(x for o in outcomes[e] for x in o) for e in CAR_CAR}
    print("ContactPoints outcomes by environment:", seen)
    moving = lambda c: c.vx != 0.0 or c.vy != 0.0 or c.w != 0.0
    # face on face: two contacts while both cars move; corner into face: one, and both ways round
    first = next(s for s in range(STEPS) if act[1][s])
    assert outcomes[1][first][0] == "both" and moving(cars[1][first][0]) and moving(cars[1][first][1]), outcomes[1]
    for e in (2, 3):
        first = next(s for s in range(STEPS) if act[e][s])
        assert outcomes[e][first][0] in ("first", "second") and moving(cars[e][first][0]) and moving(cars[e][first][1]), outcomes[e]
    everything = set().union(*seen.values())
    assert {"both", "first", "second"} <= everything, seen
    # a frozen car is hit: at rest, where it was put, through at least the first step; then a contact, and it moves
    for e in (4, 5):
        x1 = scenes[e].cars[1].px
        first = next(s for s in range(STEPS) if act[e][s])
        assert first >= 1 and all(not moving(cars[e][s][1]) and cars[e][s][1].px == x1 for s in range(first)), (e, first)
        assert moving(cars[e][first][1]) or moving(cars[e][first + 1][1]), e
    # steering in place: the turn alone makes the contact, in the first step, and the contact crashes the car
    c1 = cars[STEER_ENV][0][1]
    # (the turn is 2 degrees = 0.0349; the contact it makes turns the car back a little within the same step)
    assert act[STEER_ENV][0] >= 1 and c1.crashed == 1 and 0.03 < c1.angle < 0.035, (act[STEER_ENV], c1.angle)
    assert _outcome(scenes[STEER_ENV].cars[0], scenes[STEER_ENV].cars[1]) is None, "it touched before it turned"
    # statics: the obstacle and the building are both hit (two arbiters at once at some step)
    assert max(act[8]) == 2, act[8]
    # the chain: car-car, car-pedestrian and car-obstacle arbiters together; the capacity scenes as tests/test_capacity_scenes.py pins them
    assert max(act[9]) >= 10 and scenes[9].n_peds == 3, act[9]
    assert len(cs.drv_candidates(scenes[10])) == 60 and act[10][0] == 4 and max(act[10]) == 6, act[10]
    assert len(cs.drv_candidates(scenes[11])) == cs.CLIST and act[11][0] == 2, act[11]
    for e in SCENARIOS:   # (oblique and head_on bounce apart within a step: no contact is left at the end of one)
        assert ora.peak_arbiters(e) >= 1, e
    assert max(act[12]) == 2
    assert min(act[STEADY_ENV]) >= 1
    ora.close()
    # the three-car handle
    scenes3 = _scenes3()
    ora = ol.OracleEnv(num_envs=E3, n_players=3, seed=SEED, threads=2)
    ora.reset()
    for e, st in scenes3.items():
        ora.set_state(e, st)
    peak = {e: 0 for e in scenes3}
    for s in range(STEPS):
        ora.step(_actions(rng, E3, 3, scenes3, s, False))
        for e in scenes3:
            peak[e] = max(peak[e], ora.active_contacts(e))
    assert peak[1] == 2 and peak[2] == 1 and ora.overflow() == 0, peak
    ora.close()


@pytest.fixture(scope="module")
def gpu(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import dynenv_amd
    return dynenv_amd


def _run(gpu, n_env, A, scenes, partial, ten):
    kw = dict(observationType=gpu.ObservationType.PARTIAL, noiseType=gpu.NoiseType.REALISTIC, noiseMagnitude=3) if partial else {}
    env = gpu.BatchedDynEnv(gpu.DynEnvType.DRIVE, n_env, A, seed=SEED, **kw)
    ora = ol.OracleEnv(num_envs=n_env, n_players=A, seed=SEED, threads=4, **(PART if partial else {}))
    np.testing.assert_array_equal(env.reset_flat().cpu().numpy(), ora.reset())
    for e, st in scenes.items():
        env.set_state(e, st)
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    touched = 0
    for s in range(STEPS):
        a = _actions(rng, n_env, A, scenes, s, ten)
        og, rg, dg = env.step_flat(a, auto_reset=False)
        oc, rc, dc = ora.step(a)
        msg = "%d cars, step %d" % (A, s)
        np.testing.assert_array_equal(dg.cpu().numpy(), dc, err_msg=msg + " dones")
        np.testing.assert_array_equal(rg.cpu().numpy(), rc, err_msg=msg + " rewards")
        np.testing.assert_array_equal(og.cpu().numpy(), oc, err_msg=msg + " observations")
        rows = env.get_states().cpu().numpy()
        for e in range(n_env):
            _assert_state_equal(ol.DrivingState.from_buffer_copy(rows[e].tobytes()), ora.get_state(e), msg + " env %d" % e)
        assert env.error_flags_per_env().cpu().numpy().tolist() == [0] * n_env, msg
        touched += sum(ora.active_contacts(e) for e in scenes)
    assert env.error_flags() == 0 and ora.overflow() == 0 and ora.degenerate() == 0
    assert touched > 0 and env.debug_counters()["contact"] > 0
    env.close()
    ora.close()


@pytest.mark.gpu
def test_narrowphase_corners_full(gpu):
    _run(gpu, E, 10, _scenes(), partial=False, ten=True)
    _run(gpu, E3, 3, _scenes3(), partial=False, ten=False)


@pytest.mark.gpu
def test_narrowphase_corners_partial(gpu):
    """drv_step_partial_kernel shares the step's body"""
    _run(gpu, E, 10, _scenes(), partial=True, ten=True)
    _run(gpu, E3, 3, _scenes3(), partial=True, ten=False)
