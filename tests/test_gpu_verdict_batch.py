"""The steady verdict of a Driving contact slot with its LDS operands loaded in one batch (-m gpu, plus one CPU test of the scenes'
preconditions on the oracle).

drv_slot_verdicts decides `steady` from ten words: the slot's four stored impulses against the solve's (jn0, jt0, jn1, jt1), then three
velocity words of body i and of body j (vx, vy, w; a static j has none).  They used to be tested one behind the other, each load issued
after the comparison before it; now all ten are loaded first (a lane without a slot reads slot 0, a static partner and a free slot's
pair 0xFFFF read the all-zero body slot) and the comparisons are joined without short circuit.  The same was done to what a slot
lane reads of the mailbox and the slot record in cpArbiterUpdate, and to the two `still` words of the clean-slot test.  A wrong clamp, a
word compared against the wrong operand or a static partner that no longer counts as at rest changes when a pile is taken for steady,
i.e. which substeps are replayed instead of solved: it shows in the state blob within a step.

One handle of 16 environments, 12 steps, bit for bit against the oracle after every step, Full and Partial + Realistic noise 3 (the
Partial kernel inlines the same contact path).  The scenes, by what ends the verdict (all crashed cars on the free strip, which take
no action and slide; contacts 0.05 deep are inside the collision slop: no bias, nothing moves unless something arrives):

  rest_static       a car at rest in an obstacle: passes every test, j static (its three tests skipped before, read as +0 now)
  rest_pair         two cars at rest in each other: passes every test, j dynamic
  push_face         a car at rest, face in an obstacle, is hit from behind: two contacts, jn0 and jn1 leave their stored values
  push_corner       the same with a corner in the obstacle: ONE contact, jn0 alone can differ (jn1 is 0 on both sides)
  hit_j / hit_i     two cars at rest in each other along x; a third car arrives ALONG y on the higher-index (j) / lower-index (i) car,
                    centred: the normal of the resting pair is x, a y velocity does not load it (no friction: jt is +0 always), so the
                    pair's impulses stay what they were while one of its bodies moves in vy - and, the two contacts of the hit being
                    solved one after the other, by a last-bit w
  hit_offcentre     the same 4 px off the centre: vy and w
  stacked_hit       the resting pair stacked along y, the third car arrives along x: the moving body moves in vx
  slide_off         a car slides along an obstacle's face and off its end: the slot goes untouched, is cached and then freed (pair
                    0xFFFF, later a lane whose slot is not occupied) while a resting contact elsewhere keeps the contact path running
  ignored           a dead pedestrian inside a car at rest: pedHit rejects the pair, the slot is ARB_IGNORE, beside a resting contact
  deep_rest         a car 0.5 deep in an obstacle: the bias pushes it out, step after step
  steady_pile       a recorded one (tests/golden/drv_steady_pile.npz: the state blob of an environment of a random-play run three
                    steps before its pile came to rest, and its ten cars' actions of the twelve steps after): a crashed car whose
                    contact comes out of every solve as it went in without being inert, beside nine cars that drive on.  From the
                    fourth step on every substep is a steady replay - the only scene here whose `steady` counter rises: a pile
                    at rest inside the collision slop is inert and takes the quiescent shortcut instead, and nothing hand-placed
                    stays bit for bit what it was while a bias or a stored impulse is at work

What cannot be reached: jt0 or jt1 differing.  No Driving shape sets a friction, so arb.u = +0 and every tangent impulse is clamped
to +0 in every solve (arb_apply_impulse); the stored jt and the solve's are both +0 in every state a step can produce, and a state
blob carries no impulses.  Nor can a body of a pair that was at rest when prestepped move in w alone or in vx alone to the last bit:
what moves it is a contact impulse of a third body, solved contact by contact.  The scenes above are the nearest a step can get;
the CPU test below checks on the oracle which bodies move and which do not.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle_lib as ol
from capacity_scenes import CAR_HX, CAR_HY, S2, _dead_ped, _park, _turn
from kat_scenes_r4 import CY, _place_crashed_car
from parity_common import _assert_state_equal

SEED = 33
STEPS = 12
E = 16
EI_N_FAST, N_COUNTERS = 8, 10   # driving_dev.h: EI_N_FAST .. EI_N_SPLIT, ten consecutive words of an environment's int row
FAST, QUIET, CONTACT, SLOTS, WHY_CAND, WHY_MOVING, WHY_INERT, STEADY, LIGHT, SPLIT = range(10)
PART = dict(obs_type=1, noise_type=1, noise_magnitude=3.0)
IN = 0.05            # depth of a contact inside the collision slop (0.1)
X0 = 300.0


def _begin(st, used, n_obst, n_peds=0):
    st.n_peds, st.n_obst = n_peds, n_obst
    _park(st, [k for k in range(10) if k not in used])


def _obst(st, k, x, y=CY):
    st.obst_x[k], st.obst_y[k] = x, y


def _car(st, k, x, y=CY, vx=0.0, vy=0.0, angle=0.0):
    _place_crashed_car(st.cars[k], 0, x, y, vx)
    st.cars[k].vy = vy
    if angle != 0.0:
        _turn(st.cars[k], angle)


def rest_static(st):
    _begin(st, (0,), 1)
    _car(st, 0, X0)
    _obst(st, 0, X0 + 20.0 - IN)


def rest_pair(st):
    _begin(st, (0, 1), 0)
    _car(st, 0, X0)
    _car(st, 1, X0 + 20.0 - IN)


def push_face(st):
    _begin(st, (0, 1), 1)
    _car(st, 0, X0)
    _obst(st, 0, X0 + 20.0 - IN)
    _car(st, 1, X0 - 20.0 - 6.0, vx=30.0)      # 6 px behind car 0's back face: there within the first step


def push_corner(st):
    """car 0 at 45 degrees: its rightmost corner, ((hx + hy), (hx - hy)) / sqrt 2 from the centre, in the obstacle's left face; car 1
    arrives on the leftmost corner"""
    _begin(st, (0, 1), 1)
    cx, cyo = (CAR_HX[0] + CAR_HY[0]) * S2, (CAR_HX[0] - CAR_HY[0]) * S2
    _car(st, 0, X0, angle=math.pi / 4)
    _obst(st, 0, X0 + cx + 10.0 - IN, CY + cyo)
    _car(st, 1, X0 - cx - 10.0 - 6.0, CY - cyo, vx=30.0)


def _pair_x(st):
    _car(st, 0, X0)
    _car(st, 1, X0 + 20.0 - IN)


def hit_j(st, off=0.0):
    """car 2 stands on end (its long axis along y) above car 1 and comes down on the middle of its upper face"""
    _begin(st, (0, 1, 2), 0)
    _pair_x(st)
    _car(st, 2, st.cars[1].px + off, CY + CAR_HY[0] + CAR_HX[0] + 6.0, vy=-30.0, angle=math.pi / 2)


def hit_i(st):
    _begin(st, (0, 1, 2), 0)
    _pair_x(st)
    _car(st, 2, st.cars[0].px, CY + CAR_HY[0] + CAR_HX[0] + 6.0, vy=-30.0, angle=math.pi / 2)


def hit_offcentre(st):
    hit_j(st, off=4.0)


def stacked_hit(st):
    """cars 0 and 1 one above the other (the pair's normal is y); car 2 arrives along x on the middle of car 1's back face.  Car 0
    stands 12 px further on, so that car 2, whose lower edge is 0.05 below car 0's upper face, stops short of it."""
    _begin(st, (0, 1, 2), 0)
    _car(st, 0, X0 + 12.0, CY)
    _car(st, 1, X0, CY + 2.0 * CAR_HY[0] - IN)
    _car(st, 2, X0 - 20.0 - 6.0, st.cars[1].py, vx=30.0)


def slide_off(st):
    _begin(st, (0, 1), 2)
    _car(st, 0, X0, CY + 10.0, vy=30.0)         # its right face on obstacle 0's left face, 5 px from the end of it, moving along it
    _obst(st, 0, X0 + 20.0 - IN)
    _car(st, 1, X0 + 300.0)
    _obst(st, 1, X0 + 300.0 + 20.0 - IN)


def ignored(st):
    _begin(st, (0,), 1, n_peds=1)
    _car(st, 0, X0)
    _obst(st, 0, X0 + 20.0 - IN)
    _dead_ped(st.peds[0], X0 - 4.0, CY + CAR_HY[0] + 5.0 - 0.5)


def deep_rest(st):
    _begin(st, (0,), 1)
    _car(st, 0, X0)
    _obst(st, 0, X0 + 20.0 - 0.5)


STEADY_ENV = 14       # the recorded pile
_PILE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drv_steady_pile.npz"))

SCENES = {1: rest_static, 2: rest_pair, 3: push_face, 4: push_corner, 5: hit_j, 6: hit_i, 7: hit_offcentre, 9: stacked_hit,
          10: slide_off, 12: ignored, 13: deep_rest, 15: rest_pair}


def _scenes():
    """environment -> state blob; the environments in between keep their reset state and play randomly"""
    ref = ol.OracleEnv(num_envs=1, n_players=10, seed=SEED)
    ref.reset()
    out = {}
    for e, scene in SCENES.items():
        st = ref.get_state(0)
        scene(st)
        st.elapsed = 0
        out[e] = st
    ref.close()
    pile = ol.DrivingState.from_buffer_copy(_PILE["blob"].tobytes())
    pile.elapsed = 0
    out[STEADY_ENV] = pile
    return out


def _actions(rng, scenes, step):
    a = rng.integers(0, 3, size=(E, 10, 2)).astype(np.int32)
    for e in scenes:
        a[e] = 1   # coast (crashed cars ignore it)
    a[STEADY_ENV] = _PILE["actions"][step]
    return a


def test_scenes_reach_what_they_are_for(oracle_built):
    """CPU: what the oracle can tell of the scenes over the 12 steps of the GPU test - how many arbiters are solved, which cars move"""
    scenes = _scenes()
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4)
    ora.reset()
    for e, st in scenes.items():
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    act = {e: [] for e in scenes}
    vel = {e: [] for e in scenes}   # per step: cars' (vx, vy, w)
    for s in range(STEPS):
        ora.step(_actions(rng, scenes, s))
        for e in scenes:
            act[e].append(ora.active_contacts(e))
            d = ol.state_to_dict(ora.get_state(e))
            vel[e].append(d["cars_f"][:, [2, 3, 5]].copy())
    assert ora.overflow() == 0 and ora.degenerate() == 0
    still = lambda e: all(not v.any() for v in vel[e])
    # the resting scenes: one solved arbiter throughout, no car ever has a velocity; the ignored pair holds a slot but is not solved
    for e in (1, 2, 15, 13):
        assert act[e] == [1] * STEPS and still(e), (e, act[e])
    assert act[12] == [1] * STEPS and still(12) and ora.peak_arbiters(12) == 2, (act[12], ora.peak_arbiters(12))
    # the pushes: the resting arbiter first, then two that share car 0; car 0 at rest before the hit (car 1 alone moves at first)
    for e in (3, 4):
        assert max(act[e]) == 2 and ora.peak_arbiters(e) == 2, (e, act[e])
        assert vel[e][0][1].any(), e
    # the hits along y: three cars, two arbiters sharing the car that is hit; the hit car moves in y (no friction: the resting pair's
    # normal is x, so its impulses are not loaded by it)
    for e, hit, other in ((5, 1, 0), (6, 0, 1), (7, 1, 0)):
        assert max(act[e]) == 2 and ora.peak_arbiters(e) == 2, (e, act[e])
        first = next(s for s in range(STEPS) if vel[e][s][hit, 1] != 0.0)
        assert vel[e][first][hit, 1] < 0.0, (e, vel[e][first])
        if e != 7:   # (centred: the pair's other car gets no y velocity from it; off the centre the hit car turns and takes it along)
            assert vel[e][first][other, 1] == 0.0, (e, vel[e][first])
    assert any(v[1, 2] != 0.0 for v in vel[7]), "the off-centre hit never turned car 1"
    # stacked: the hit car moves in x
    first = next(s for s in range(STEPS) if vel[9][s][1, 0] != 0.0)
    assert vel[9][first][1, 0] > 0.0 and max(act[9]) == 2
    # slide_off: two arbiters while car 0 is on the face, one once it has left it
    assert act[10][0] == 2 and act[10][-1] == 1 and ora.peak_arbiters(10) == 2, act[10]
    # the recorded pile: a solved arbiter in every step, the crashed car (9) at rest from the fourth step on, other cars driving
    e = STEADY_ENV
    assert min(act[e]) >= 1 and not any(v[9].any() for v in vel[e][3:]) and all(v[:9].any() for v in vel[e]), (act[e], [v[9].tolist() for v in vel[e]])
    ora.close()


@pytest.fixture(scope="module")
def gpu(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import dynenv_amd
    return dynenv_amd


def _counters(env):
    """every environment's ten diagnostic counters, out of the handle's checkpoint (as tests/test_gpu_contact_call_paths.py reads them)"""
    ck = env.checkpoint()
    header = C.sizeof(ol.Cfg) + 24
    payload = len(ck) - header
    before = E * (9 * 32 * 8 + 6 * 16 * 8 + 32 * 4 + 32 * 4 + 2 * 20 * 8)
    after = E * (2 * 16 * 8 + 24 * 4 + 24 * 4 + 2 * 24 * 4 + 4 * 24 * 8 + 64 * 4)
    row = (payload - before - after) // E
    assert row > 0 and row % 4 == 0 and before + after + E * row == payload
    envi = np.frombuffer(ck[header + before:header + before + E * row].tobytes(), np.int32).reshape(E, row // 4)
    return envi[:, EI_N_FAST:EI_N_FAST + N_COUNTERS].astype(np.int64)


def _run(gpu, partial):
    scenes = _scenes()
    kw = dict(observationType=gpu.ObservationType.PARTIAL, noiseType=gpu.NoiseType.REALISTIC, noiseMagnitude=3) if partial else {}
    env = gpu.BatchedDynEnv(gpu.DynEnvType.DRIVE, E, 10, seed=SEED, **kw)
    ora = ol.OracleEnv(num_envs=E, n_players=10, seed=SEED, threads=4, **(PART if partial else {}))
    np.testing.assert_array_equal(env.reset_flat().cpu().numpy(), ora.reset())
    for e, st in scenes.items():
        env.set_state(e, st)
        ora.set_state(e, st)
    rng = np.random.default_rng(SEED)
    start = _counters(env)
    for s in range(STEPS):
        a = _actions(rng, scenes, s)
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
    assert env.error_flags() == 0 and ora.overflow() == 0 and ora.degenerate() == 0
    total = _counters(env) - start
    env.close()
    ora.close()
    return total


def _check(total):
    print("per-environment counters [fast quiet contact slots why_cand why_moving why_inert steady light split]:")
    for e in sorted(SCENES):
        print("  env %2d %-14s %s" % (e, SCENES[e].__name__, total[e].tolist()))
    paths = total[:, FAST] + total[:, QUIET] + total[:, CONTACT] + total[:, STEADY]
    assert (paths == 10 * STEPS).all(), paths
    # where the pile comes to rest without being inert the verdict is `steady` and the substeps after it are replayed
    print("  env %2d %-14s %s" % (STEADY_ENV, "steady_pile", total[STEADY_ENV].tolist()))
    assert total[STEADY_ENV, STEADY] >= 10 * (STEPS - 4), "the recorded pile was not replayed as steady: %s" % total[STEADY_ENV].tolist()
    # the hand-placed piles at rest are inert: quiescent, not steady (and deep_rest is pushed by its bias in every substep)
    for e in (1, 2, 15, 12):
        assert total[e, QUIET] > 10 * (STEPS - 2) and total[e, STEADY] == 0, (e, total[e].tolist())
    assert total[13, CONTACT] == 10 * STEPS, total[13].tolist()
    # every scene ran the contact path, and none a general multi-level solve it is not built for
    for e in SCENES:
        assert total[e, CONTACT] > 0, (e, total[e].tolist())


@pytest.mark.gpu
def test_verdict_batch_full(gpu):
    _check(_run(gpu, partial=False))


@pytest.mark.gpu
def test_verdict_batch_partial(gpu):
    """drv_step_partial_kernel shares the step's body"""
    _check(_run(gpu, partial=True))
