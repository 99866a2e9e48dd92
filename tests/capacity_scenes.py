"""Scenes at the capacity of the contact paths' fixed tables, written once and run twice: on the oracle alone
(tests/test_capacity_scenes.py, CPU - it proves that each scene reaches what it is for) and on the HIP path against the oracle
(tests/test_gpu_contact_capacity.py, -m gpu).  Every function edits a state blob (ol.DrivingState / ol.RoboCupState) in place.

The tables: an environment's arbiters live in DRV_NS = 24 (Driving) / RC_NS = 16 (RoboCup) slots, one per lane; a substep's
candidate pairs go into a list of 128 and through the narrowphase in passes of 16 (Driving) / 64 (RoboCup).  The oracle has no such
limits, so at or below them both sides must agree bit for bit, and one above them the kernels drop a pair and raise error bit 0.
The load is what OracleEnv.peak_arbiters counts.

Driving geometry used throughout: the buildings leave the strips 425 < y < 575 and 765 < x < 985 free; a crashed + finished car
takes no action and just slides; a DEAD pedestrian is a free circle of radius 5; a car slower than 1 px/s that touches a pedestrian
has the pair rejected by pedHit - the arbiter exists (it holds a slot) but is never solved; obstacles are static 20 x 20 boxes and
may coincide (static pairs do not exist).  A car at 45 degrees leaves two corner triangles of its bounding box free: what sits there
is a candidate pair that never touches.
"""
import math

import numpy as np

from kat_scenes_r4 import CY, _place_crashed_car

DRV_NS, RC_NS, CLIST, DRV_PASS, RC_PASS = 24, 16, 128, 16, 64
CAR_HX, CAR_HY = (10.0, 15.0, 20.0, 25.0), (5.0, 6.0, 7.0, 8.0)
BUILDINGS = ((365.0, 200.0), (365.0, 800.0), (1385.0, 200.0), (1385.0, 800.0))
S2 = math.sqrt(0.5)


# ------------------------------------------------------------------------------------------------ Driving helpers
def _dead_ped(p, x, y, vx=0.0):
    p.px, p.py, p.vx, p.vy = x, y, vx, 0.0
    p.road, p.side, p.dead, p.moving, p.speed, p.crossing, p.begin_crossing = 1, 0, 1, 0, 4, 0, 0


def _turn(c, angle):
    c.angle, c.dirx, c.diry = angle, math.cos(angle), math.sin(angle)


def _park(st, ks, x0=60.0, y=560.0, dx=40.0):
    """cars that play no part: crashed type-0 cars in a row along the lower edge of the free strip, touching nothing"""
    for n, k in enumerate(ks):
        _place_crashed_car(st.cars[k], 0, x0 + dx * n, y, 0.0)


def drv_boxes(st):
    """the broadphase's boxes (l, b, r, t) by slot: cars 0..9 (rotated box min / max), pedestrians 10..29 (+-5), obstacles 30..49 (+-10),
    buildings 50..53 (400 x 225 half extents); None for a slot without an object"""
    bx = [None] * 54
    for i in range(st.n_cars):
        c = st.cars[i]
        hx, hy = CAR_HX[c.type], CAR_HY[c.type]
        ex = abs(math.cos(c.angle)) * hx + abs(math.sin(c.angle)) * hy
        ey = abs(math.sin(c.angle)) * hx + abs(math.cos(c.angle)) * hy
        bx[i] = (c.px - ex, c.py - ey, c.px + ex, c.py + ey)
    for k in range(st.n_peds):
        p = st.peds[k]
        bx[10 + k] = (p.px - 5.0, p.py - 5.0, p.px + 5.0, p.py + 5.0)
    for k in range(st.n_obst):
        bx[30 + k] = (st.obst_x[k] - 10.0, st.obst_y[k] - 10.0, st.obst_x[k] + 10.0, st.obst_y[k] + 10.0)
    for k, (x, y) in enumerate(BUILDINGS):
        bx[50 + k] = (x - 400.0, y - 225.0, x + 400.0, y + 225.0)
    return bx


def drv_candidates(st):
    """the substep's candidate list in the kernels' order: canonical pairs (car i, slot j > i) whose boxes intersect (cpBBIntersects),
    i ascending, then j ascending.  Pair k of the list goes through the narrowphase in pass k // 16."""
    bx = drv_boxes(st)
    out = []
    for i in range(st.n_cars):
        a = bx[i]
        for j in range(i + 1, 54):
            b = bx[j]
            if b is not None and a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]:
                out.append((i, j))
    return out


# ------------------------------------------------------------------------------------------------ Driving: the slot table
def drv_full(st, extra=0):
    """24 (+ extra) isolated arbiters: ten crashed type-0 cars 150 apart on the walkway strip, each 0.5 deep in an obstacle on either
    side (20 arbiters that are solved), and a dead pedestrian 0.5 deep in the upper face of the first 4 (+ extra) cars: rejected by
    pedHit, never solved, yet each holds a slot.  All from the first substep on, none ever expires."""
    assert 0 <= extra <= 6
    st.n_peds, st.n_obst = 4 + extra, 20
    for k in range(10):
        x = 100.0 + 150.0 * k
        _place_crashed_car(st.cars[k], 0, x, CY, 0.0)
        st.obst_x[2 * k], st.obst_y[2 * k] = x - 19.5, CY
        st.obst_x[2 * k + 1], st.obst_y[2 * k + 1] = x + 19.5, CY
    for k in range(st.n_peds):
        _dead_ped(st.peds[k], st.cars[k].px - 4.0, CY + 9.5)


def drv_over(st):
    """drv_full and one arbiter more than the table holds: 25"""
    drv_full(st, extra=1)


def drv_full_coupled(st, extra=0):
    """24 (+ extra <= 1) arbiters in five coupled groups: the cars stand in pairs, 0.5 deep in each other and in an obstacle at either
    end (obstacle | car | car | obstacle: 3 arbiters that share bodies), and an obstacle lies 0.5 deep on the upper face of the first
    9 (+ extra) cars: every group is one connected contact graph of 4 or 5 arbiters over 2 dynamic bodies.  The car indices of a pair
    are far apart, so the groups interleave in canonical order."""
    assert 0 <= extra <= 1
    st.n_peds, st.n_obst = 0, 19 + extra
    for g in range(5):
        x = 120.0 + 300.0 * g
        a, b = g, 9 - g
        _place_crashed_car(st.cars[a], 0, x, CY, 0.0)
        _place_crashed_car(st.cars[b], 0, x + 19.5, CY, 0.0)
        st.obst_x[2 * g], st.obst_y[2 * g] = x - 19.5, CY
        st.obst_x[2 * g + 1], st.obst_y[2 * g + 1] = x + 39.0, CY
    for n in range(9 + extra):   # on top of car n: x overlap with its own car only (the neighbour's face starts 9.5 further on)
        c = st.cars[n]
        left = n < 5             # cars 0..4 are the left car of their pair
        st.obst_x[10 + n], st.obst_y[10 + n] = c.px + (-10.5 if left else 10.5), CY + 14.5


def drv_over_coupled(st):
    drv_full_coupled(st, extra=1)


# ------------------------------------------------------------------------------------------------ Driving: deep chains
def drv_chain10(st, seed, mixed=False):
    """All ten cars in one row, faces 0.05 deep in each other (inside the collision slop), an obstacle at the far end; the whole row
    drifts at 3 px/s and the first car arrives at 40: one connected contact graph of 10 arbiters (9 car-car + 1 car-obstacle), ten
    levels deep in spatial order, while the canonical pair order is a random permutation of it (seed).
    mixed: car types are mixed and a dead pedestrian is wedged into three of the gaps (2 arbiters in place of 1; the circle is
    shape a of its pairs, the car of a car-car pair's, so both orders occur along the chain).  Every car moves faster than 1 px/s at
    the first touch, so pedHit accepts the pairs and they are solved."""
    rng = np.random.default_rng(seed)
    order = [int(k) for k in rng.permutation(10)]
    types = [int(t) for t in rng.integers(0, 4, 10)] if mixed else [0] * 10
    wedged = set(int(g) for g in rng.choice(np.arange(1, 9), 3, replace=False)) if mixed else set()
    st.n_peds, st.n_obst = 0, 1
    x, prev_hx = 200.0, None
    for pos, k in enumerate(order):
        hx = CAR_HX[types[pos]]
        if prev_hx is not None:
            if pos in wedged:   # gap `pos` (between the cars at pos - 1 and pos) holds a pedestrian
                _dead_ped(st.peds[st.n_peds], x + prev_hx + 5.0 - 0.05, CY, 3.0)
                st.n_peds += 1
                x += prev_hx + 10.0 + hx - 0.1
            else:
                x += prev_hx + hx - 0.05
        _place_crashed_car(st.cars[k], types[pos], x, CY, 40.0 if pos == 0 else 3.0)
        prev_hx = hx
    st.obst_x[0], st.obst_y[0] = x + prev_hx + 10.0 - 0.05, CY
    return order


# ------------------------------------------------------------------------------------------------ Driving: candidate list and passes
R3 = (CAR_HX[3] + CAR_HY[3]) * S2   # half the bounding box of a type-3 car (50 x 16) at 45 degrees: 23.33


def resting_chain_scene(st, rng):
    """2..4 crashed cars in a row (random types, lateral offsets, overlaps above and below the collision slop), optionally a dead
    pedestrian wedged in and an obstacle at the end: resting contacts that share bodies - the two- and three-level solves a launch's
    slowest environments run (drv_solve_bias_multi / drv_solve_general_split), in every arrangement of who is shape a and shape b."""
    n = int(rng.integers(2, 5))
    st.n_peds, st.n_obst = 0, 0
    x, cy = 300.0 + float(rng.uniform(0, 50)), CY
    order = list(rng.permutation(n))         # which car index stands where: canonical pair order != spatial order
    prev_hx = None
    for pos, k in enumerate(order):
        t = int(rng.integers(0, 4))
        hx = [10.0, 15.0, 20.0, 25.0][t]
        if prev_hx is not None:
            x += prev_hx + hx - float(rng.choice([0.03, 0.5, 1.5, 3.0]))
        _place_crashed_car(st.cars[k], t, x, cy + float(rng.uniform(-3.0, 3.0)), float(rng.choice([0.0, 0.0, 0.0, 2.0])) if pos == 0 else 0.0)
        prev_hx = hx
    for k in range(n, st.n_cars):
        _place_crashed_car(st.cars[k], 0, 1500.0, 480.0 + 45.0 * k, 0.0)
    if rng.random() < 0.6:
        st.n_obst = 1
        st.obst_x[0], st.obst_y[0] = x + prev_hx + 10.0 - float(rng.choice([0.03, 0.8, 2.0])), cy + float(rng.uniform(-6.0, 6.0))
    if rng.random() < 0.3:   # a dead pedestrian (a circle, dynamic, shape a of its pair) leaning on the first car
        st.n_peds = 1
        p = st.peds[0]
        c = st.cars[order[0]]
        p.px, p.py, p.vx, p.vy = c.px - [10.0, 15.0, 20.0, 25.0][c.type] - 5.0 + float(rng.choice([0.05, 0.7])), c.py, 0.0, 0.0
        p.road, p.side, p.dead, p.moving, p.speed, p.crossing, p.begin_crossing = 1, 0, 1, 0, 4, 0, 0


def _cars_around_stack(st, ks, sx, sy, d=8.0):
    """four type-3 cars at +-45 degrees around the point (sx, sy): the bounding box of each overlaps a 20 x 20 box centred there by d
    in x and y, at a corner its own rotated box leaves free (the nearest the box comes is 25 - d * sqrt 2 from that corner, d < 17).
    With d = 8 a pedestrian (radius 5) at the centre lies in all four bounding boxes too, and the cars' boxes stay 4 apart."""
    off = R3 + 10.0 - d
    for k, (ux, uy) in zip(ks, ((-1, 1), (1, -1), (1, 1), (-1, -1))):
        _place_crashed_car(st.cars[k], 3, sx + ux * off, sy + uy * off, 0.0)
        _turn(st.cars[k], math.pi / 4 if ux != uy else -math.pi / 4)


def drv_passes(st):
    """60 candidates in 4 passes of 16, 4 to 6 arbiters.  Cars 1..4 stand around a stack of 14 coincident obstacles (4 x 14 pairs that
    never touch) and each is 0.5 deep in an obstacle of its own with a LOWER index than the stack's, so the list reads
    [car 1: touch, 14 x no][car 2: touch, 14 x no][car 3: ...][car 4: ...]: the touching pairs sit at 0, 15, 30, 45 - first contacts in
    passes 0, 0, 1 and 2 of the first substep, which hands out slots in three consecutive passes.  Car 0 (its pairs come first) slides
    into obstacle 18 and car 9 (its pairs come last) into obstacle 19 a few steps later: a first contact in pass 0 while the four cached
    pairs are re-touched in passes 0..2 behind it, and one in the last pass behind them."""
    st.n_peds, st.n_obst = 0, 20
    sx, sy = 500.0, 500.0
    _cars_around_stack(st, (1, 2, 3, 4), sx, sy)
    for o in range(4, 18):
        st.obst_x[o], st.obst_y[o] = sx, sy
    # the corner of a car's rotated box that points away from the stack in x: (+-R3, +-(25 - 8) sqrt 1/2) from its centre
    for o, k in enumerate((1, 2, 3, 4)):
        c = st.cars[k]
        ox = 1.0 if c.px > sx else -1.0
        oy = ox if c.angle > 0 else -ox
        st.obst_x[o], st.obst_y[o] = c.px + ox * (R3 + 10.0 - 0.5), c.py + oy * (CAR_HX[3] - CAR_HY[3]) * S2
    _place_crashed_car(st.cars[0], 0, 180.0, CY, 30.0)
    st.obst_x[18], st.obst_y[18] = 180.0 + 10.0 + 6.0 + 10.0, CY     # 6 px ahead of car 0's face
    _place_crashed_car(st.cars[9], 0, 1180.0, CY, 30.0)
    st.obst_x[19], st.obst_y[19] = 1180.0 + 10.0 + 7.4 + 10.0, CY    # 7.4 px ahead of car 9's face (a crashed car at 30 px/s slides 7.65)
    _park(st, (5, 6, 7, 8))


def drv_clist(st, over=False):
    """128 candidates (over: 129), 2 arbiters.  Cars 1..4 stand around stack A (9 coincident obstacles + 7 coincident dead
    pedestrians: 16 pairs per car that never touch), cars 5..8 around stack B (9 + 6: 15 per car); car 1 and car 8 are each 0.5 deep in
    an obstacle of their own (obstacles 18, 19: the HIGHEST indices, so pair (8, obstacle 19) is the very last of the list); car 0 has
    two coincident dead pedestrians in one free corner of its box.  64 + 1 + 60 + 1 + 2 = 128: the list is full to its last entry, and that entry
    touches.  over: car 9 stands where its box overlaps car 0's without touching: pair (0, 9) is candidate 0, everything moves up by
    one, and the touching pair (8, obstacle 19) is the 129th - the one that is dropped."""
    st.n_peds, st.n_obst = 15, 20
    ax, bx, sy = 400.0, 1200.0, 500.0
    _cars_around_stack(st, (1, 2, 3, 4), ax, sy)
    _cars_around_stack(st, (5, 6, 7, 8), bx, sy)
    for o in range(9):
        st.obst_x[o], st.obst_y[o] = ax, sy
        st.obst_x[9 + o], st.obst_y[9 + o] = bx, sy
    for p in range(7):
        _dead_ped(st.peds[p], ax, sy)
    for p in range(6):
        _dead_ped(st.peds[7 + p], bx, sy)
    for o, k in ((18, 1), (19, 8)):
        c = st.cars[k]
        sx = ax if k == 1 else bx
        ox = 1.0 if c.px > sx else -1.0
        oy = ox if c.angle > 0 else -ox
        st.obst_x[o], st.obst_y[o] = c.px + ox * (R3 + 10.0 - 0.5), c.py + oy * (CAR_HX[3] - CAR_HY[3]) * S2
    # car 0: type 3 at 45 degrees on its own; two coincident pedestrians in one free corner of its box (1 inside it in x and y, 23 from
    # the rotated box; the corner away from car 9)
    _place_crashed_car(st.cars[0], 3, 800.0, 500.0, 0.0)
    _turn(st.cars[0], math.pi / 4)
    _dead_ped(st.peds[13], 800.0 - R3 + 1.0, 500.0 + R3 - 1.0)
    _dead_ped(st.peds[14], 800.0 - R3 + 1.0, 500.0 + R3 - 1.0)
    # car 9: parallel to car 0; 30 to the right its box overlaps car 0's (46.7 wide) while the rotated boxes are 30 sqrt 1/2 = 21.2 > 16 apart
    _place_crashed_car(st.cars[9], 3, 830.0 if over else 940.0, 500.0, 0.0)
    _turn(st.cars[9], math.pi / 4)


# ------------------------------------------------------------------------------------------------ RoboCup
def _place_robot(r, x, y, vx=0.0, vy=0.0):
    """both feet at the robot's position, angle 0: the left foot's capsule runs from (x - 10, y + 10) to (x + 10, y + 10), the right
    foot's 20 below it, radius 7.5 - the robot covers x +- 17.5, y +- 17.5"""
    r.lpx = r.rpx = x; r.lpy = r.rpy = y; r.lvx = r.rvx = vx; r.lvy = r.rvy = vy
    r.la = r.ra = 0.0; r.lw = r.rw = 0.0
    r.prevx, r.prevy = x, y


RC_X0, RC_Y0 = 200.0, 150.0


def rc_full(st, ball=False):
    """16 arbiters (ball: 17).  Ten robots on a 2 x 5 grid, rows 34 apart: a robot's left foot is 1 deep in the right foot of the robot
    above it (8 arbiters).  In four rows the columns are 34 apart: both feet touch their neighbour's end caps (2 arbiters a row); in
    the fifth the two robots stand 13 further out each (60 apart: no contact there, and their feet still overlap the next row's in x).
    The right column stands 0.3 higher, so the cores of two feet in a row are not collinear (error bit 4 stays down).
    With the fall dice on (FLAG_CAN_FALL) the robots knock each other over within a few steps and the arbiters go; without, all 16 rest.
    ball: beside the outer cap of the lowest left robot's right foot, 0.5 deep."""
    for k in range(10):
        col, row = k % 2, k // 2
        out = 13.0 if row == 4 else 0.0
        _place_robot(st.robots[k], RC_X0 + (34.0 + out if col else -out), RC_Y0 + 34.0 * row + (0.3 if col else 0.0))
    if ball:
        r = st.robots[0]
        st.bpx, st.bpy = r.rpx - 10.0 - 7.5 - 5.0 + 0.5, r.rpy - 10.0
    else:
        st.bpx, st.bpy = 520.0, 600.0
    st.bvx = st.bvy = st.bw = 0.0
    st.bprevx, st.bprevy = st.bpx, st.bpy


def rc_over(st):
    rc_full(st, ball=True)


def rc_chain(st):
    """one column of ten robots 34 apart (robot k above robot k - 1), the lowest pushed upwards at 60 px/s: nine foot-foot arbiters,
    chained through the nine robots' joints between their two feet"""
    for k in range(10):
        _place_robot(st.robots[k], RC_X0, 100.0 + 34.0 * k, 0.0, 60.0 if k == 0 else 0.0)
    st.bpx, st.bpy = 520.0, 600.0
    st.bvx = st.bvy = st.bw = 0.0
    st.bprevx, st.bprevy = st.bpx, st.bpy
