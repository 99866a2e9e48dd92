"""Contact scenes that exist at EVERY player count the C ABI accepts - Driving with 1..10 cars, RoboCup with 1..5 robots a team -
and the batch the player-count tests run them in, written once and run twice: on the oracle alone (tests/test_player_count_scenes.py,
CPU - it pins what each scene reaches) and on the HIP path against the oracle (tests/test_gpu_player_counts.py, -m gpu).

Random play does not reach the contact solver at small player counts within a test's few steps; the scenes of
tests/capacity_scenes.py need ten cars or ten robots.  These are the same constructions for A cars / R = 2 n robots:

  drv_chain(st, A, seed, mixed)   capacity_scenes.drv_chain10 for A cars (identical to it at A = 10)
  drv_scenario(kind, A)           parity_common._scenario with n_cars = A: only cars 0..2 play a part
  rc_column(st, R)                capacity_scenes.rc_chain for R robots
  rc_rolling_ball(st)             the ball rolls past the second team's first robot: the team rewards are paid

The batch (OracleBatch / scene_blobs / tour_actions): about six environments; the chain or column in environment 0, a truncated scenario in
environment 1 (Driving), the rolling ball in environment 2 (RoboCup, under random actions), a second chain or column in environment 4,
the others at their reset state under random actions.
A helper module: no test in here."""
import collections

import numpy as np

import oracle_lib as ol
import per_env_common as pc
from capacity_scenes import CAR_HX, CY, RC_X0, _dead_ped, _place_crashed_car, _place_robot
from parity_common import _scenario

E = 6                              # environments of every batch
CHAIN_ENV, SCENARIO_ENV, BALL_ENV, CHAIN2_ENV = 0, 1, 2, 4   # (the scenario: Driving; the rolling ball: RoboCup)
DRV_STEPS, RC_STEPS = 12, 8        # steps of a tour
ACCELERATE_FROM = 10               # the scenario's car 0 accelerates into what it rests against from this step on (test_collision_scenarios)
_DRV, _RC, _DEF = (3, 3), (5, 3, 3, 7), ol.ROBOCUP_DEFAULT_FLAGS


# ------------------------------------------------------------------------------------------------ scenes
def drv_chain(st, A, seed, mixed=False):
    """capacity_scenes.drv_chain10 for A cars: all A cars in one row, faces 0.05 deep in each other (inside the collision slop), an
    obstacle at the far end; the row drifts at 3 px/s and the first car arrives at 40: one connected contact graph of A arbiters
    (A - 1 car-car + 1 car-obstacle), A levels deep in spatial order, while the canonical pair order is a permutation of it (seed).
    A = 1 is one car at 40 px/s against the obstacle.
    mixed: car types are mixed and a dead pedestrian is wedged into up to three of the gaps (2 arbiters in place of 1); every car
    moves faster than 1 px/s at the first touch, so pedHit accepts the pairs and they are solved.
    The draws are drv_chain10's, so at A = 10 the scene is that one, byte for byte.  -> the spatial order"""
    assert 1 <= A <= 10
    rng = np.random.default_rng(seed)
    order = [int(k) for k in rng.permutation(A)]
    types = [int(t) for t in rng.integers(0, 4, A)] if mixed else [0] * A
    gaps = np.arange(1, min(A, 9))   # gap g lies between the cars at g - 1 and g (A = 10: gaps 1..8, like drv_chain10)
    wedged = set(int(g) for g in rng.choice(gaps, min(3, len(gaps)), replace=False)) if mixed and len(gaps) else set()
    st.n_cars, st.n_peds, st.n_obst = A, 0, 1
    x, prev_hx = 200.0, None
    for pos, k in enumerate(order):
        hx = CAR_HX[types[pos]]
        if prev_hx is not None:
            if pos in wedged:
                _dead_ped(st.peds[st.n_peds], x + prev_hx + 5.0 - 0.05, CY, 3.0)
                st.n_peds += 1
                x += prev_hx + 10.0 + hx - 0.1
            else:
                x += prev_hx + hx - 0.05
        _place_crashed_car(st.cars[k], types[pos], x, CY, 40.0 if pos == 0 else 3.0)
        prev_hx = hx
    st.obst_x[0], st.obst_y[0] = x + prev_hx + 10.0 - 0.05, CY
    return order


def chain_arbiters(st):
    """what a drv_chain blob holds once everything touches: one arbiter per car (its right-hand neighbour or the obstacle) and one more
    per wedged pedestrian"""
    return st.n_cars + st.n_peds


def drv_scenario(kind, A):
    """parity_common._scenario (its geometry is not repeated here) for a handle with A cars: cars 0..2 act, the rest are parked; the
    cars from A on do not exist.  "pileup" needs A >= 3, "obstacle" and "building" A >= 1."""
    assert A >= (3 if kind == "pileup" else 1)
    st = _scenario(kind)
    st.n_cars = A
    return st


def scenario_kind(A):
    return "pileup" if A >= 3 else "obstacle"


def rc_column(st, R, x0=RC_X0, push=60.0):
    """capacity_scenes.rc_chain for R robots: one column 34 apart (robot k above robot k - 1), the lowest pushed upwards at `push`
    px/s: R - 1 foot-foot arbiters, chained through the robots' joints between their two feet.  The ball is parked."""
    assert 2 <= R <= 10 and st.n_robots == R
    for k in range(R):
        _place_robot(st.robots[k], x0, 100.0 + 34.0 * k, 0.0, push if k == 0 else 0.0)
    st.bpx, st.bpy = 520.0, 600.0
    st.bvx = st.bvy = st.bw = 0.0
    st.bprevx, st.bprevy = st.bpx, st.bpy


RC_W, RC_H = 1040.0, 740.0


def robot_pos(r):
    return 0.5 * (r.lpx + r.rpx), 0.5 * (r.lpy + r.rpy)


def rc_rolling_ball(st):
    """the ball rolls past the first robot of the second team (robot n, the first lane on the far side of the kernels' `lane < n` team
    split), 60 beside it, at 60 px/s along x towards the field's middle; everything else stays as the reset left it.  A ball that
    moves in x is what pays the team rewards (+-dx / 20), and a robot within 150 of it that did not kick it gets the negative half
    of its own team's: at rest - the tour's random play does not move the ball in eight steps - both teams' terms are zero and the
    team a robot is counted to is never looked at."""
    x, y = robot_pos(st.robots[st.n_robots // 2])
    st.bpx, st.bpy = x, y + (60.0 if y < RC_H / 2 else -60.0)
    st.bvx, st.bvy, st.bw = (60.0 if x < RC_W / 2 else -60.0), 0.0, 0.0
    st.bprevx, st.bprevy = st.bpx, st.bpy


# ------------------------------------------------------------------------------------------------ the cases
# name -> (per_env_common.Cfg without its player count, the player counts).  Partial: Realistic noise of magnitude 3 (per_env_common.make).
Family = collections.namedtuple("Family", "env_type highs partial flags counts")
FAMILIES = {
    "drv_full": Family(1, _DRV, False, 0, range(1, 11)),
    "drv_partial": Family(1, _DRV, True, 0, range(1, 11)),
    "rc_resting": Family(0, _RC, False, ol.FLAG_USE_OBS_REWARDS, range(1, 6)),   # no fall dice: every arbiter rests
    "rc_default": Family(0, _RC, False, _DEF, range(1, 6)),                        # the robots knock each other over
    "rc_random_init": Family(0, _RC, False, _DEF | ol.FLAG_RANDOM_INIT, range(1, 6)),
    "rc_partial": Family(0, _RC, True, _DEF, range(1, 6)),
}
TOUR = [(f, n) for f in FAMILIES for n in FAMILIES[f].counts]
# more players than there are: both sides clamp to 10 cars / 5 robots a team (environment_base.py:57)
CLAMPED = [("drv_full", 12), ("rc_default", 7)]
# the per-environment calls: the counts between those tests/per_env_common.py's table has (10 / 2 cars, 5 / 1 robots a team)
PER_ENV = [("drv_full", 3), ("drv_full", 7), ("rc_default", 3), ("rc_default", 4)]
# random play that has contacts of its own, at team sizes where the default start has none: the cases in which an environment outside
# the scenes has an active contact after at least one of the tour's steps (test_player_count_scenes pins it on the oracle)
RANDOM_PLAY_CONTACTS = {("rc_random_init", 3), ("rc_random_init", 4)}


def cfg(family, players):
    f = FAMILIES[family]
    return pc.Cfg(f.env_type, players, f.highs, f.partial, f.flags, DRV_STEPS if f.env_type == 1 else RC_STEPS)


def seed_of(family, players):
    """the handle's and the oracle's seed: one per case"""
    return 300 + 20 * sorted(FAMILIES).index(family) + players


def tour_steps(c):
    return DRV_STEPS if pc.driving(c) else RC_STEPS


# ------------------------------------------------------------------------------------------------ the batch
def scene_blobs(c, blank, seed):
    """{environment: state blob} of the scenes of a batch; blank(e) is a fresh copy of environment e's reset state (it has the handle's
    own player count - after clamping - and `elapsed` 0)"""
    out = {}
    if pc.driving(c):
        st = blank(CHAIN_ENV)
        A = st.n_cars
        drv_chain(st, A, seed)
        out[CHAIN_ENV] = st
        st = drv_scenario(scenario_kind(A), A)
        out[SCENARIO_ENV] = st
        st = blank(CHAIN2_ENV)
        drv_chain(st, A, seed + 1000, mixed=True)
        out[CHAIN2_ENV] = st
    else:
        st = blank(CHAIN_ENV)
        rc_column(st, st.n_robots)
        out[CHAIN_ENV] = st
        st = blank(CHAIN2_ENV)
        rc_column(st, st.n_robots, x0=RC_X0 + 300.0, push=45.0)
        out[CHAIN2_ENV] = st
        st = blank(BALL_ENV)
        rc_rolling_ball(st)
        out[BALL_ENV] = st
    for st in out.values():
        assert st.elapsed == 0
    return out


def tour_actions(c, A, steps, seed, first=0):
    """[steps] of int32 [E, A, K]: random everywhere but in the scene environments, which take no action (Driving: coast; RoboCup:
    nobody walks, turns or kicks, no head turn) - only car 0 of the scenario accelerates from step ACCELERATE_FROM on.  `first`: the
    number of the first of these steps in the tour."""
    scenes = (CHAIN_ENV, SCENARIO_ENV, CHAIN2_ENV) if pc.driving(c) else (CHAIN_ENV, CHAIN2_ENV)
    acts = pc.actions(c, E, A, steps, seed, idle=scenes)
    if pc.driving(c):
        for s, a in enumerate(acts):
            if first + s >= ACCELERATE_FROM:
                a[SCENARIO_ENV, 0, 0] = 2
    return acts


def blob_class(c):
    return ol.DrivingState if pc.driving(c) else ol.RoboCupState


def copy_blob(st):
    return type(st).from_buffer_copy(bytes(st))


class OracleBatch:
    """the oracle's side of a batch: E environments at their reset state with the scenes written in"""

    def __init__(self, c, seed, **kw):
        self.c, self.seed = c, seed
        self.ora = pc.oracle(c, E, seed, **kw)
        self.ora.reset()
        self.A = self.ora.A
        self.blobs = scene_blobs(c, lambda e: copy_blob(self.ora.get_state(e)), seed)
        for e, st in self.blobs.items():
            self.ora.set_state(e, st)

    def actions(self, steps=None, first=0):
        return tour_actions(self.c, self.A, tour_steps(self.c) if steps is None else steps, self.seed + 7 + first, first)
