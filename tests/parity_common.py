"""What the GPU parity, contact-capacity, contact-call-path and verdict-batch tests share: the state comparison against the oracle, field by
field, the Driving collision scenarios and RoboCup's random actions.  A helper module: no test in here."""
import numpy as np

import oracle_lib as ol


def _assert_state_equal(sg, so, msg=""):
    dg, do = ol.state_to_dict(sg), ol.state_to_dict(so)
    for k in do:
        np.testing.assert_array_equal(dg[k], do[k], err_msg="%s field %s" % (msg, k))


def _scenario(kind):
    """Hand-built collision scenes (set_state on both sides): analytically meaningful contact cases."""
    st = ol.DrivingState()
    st.n_cars, st.n_peds, st.n_obst, st.episode = 10, 2, 2, 1
    for i in range(10):  # park the unused cars far apart on the vertical road's right lane
        c = st.cars[i]
        c.px, c.py, c.angle = 892.5, 40.0 + 95.0 * i, np.pi / 2
        c.dirx, c.diry = 6.123233995736766e-17, 1.0
        c.prevx, c.prevy, c.goalx, c.goaly = c.px, c.py, 875.0, 1000.0
        c.type, c.lane_pos = i % 4, 4
    for k in range(2):
        p = st.peds[k]
        p.px, p.py, p.road, p.side, p.speed, p.moving = 700.0 + 30 * k, 440.0, 1, 0, 4, 100000
    st.obst_x[0], st.obst_y[0] = 200.0, 440.0
    st.obst_x[1], st.obst_y[1] = 1500.0, 560.0
    a, b = st.cars[0], st.cars[1]
    if kind == "head_on":  # two cars on the horizontal road driving into each other
        a.px, a.py, a.angle, a.vx, a.vy = 400.0, 517.5, 0.0, 60.0, 0.0
        a.dirx, a.diry = 1.0, 0.0
        b.px, b.py, b.angle, b.vx, b.vy = 480.0, 517.5, -np.pi, -45.0, 0.0
        b.dirx, b.diry = -1.0, -1.2246467991473532e-16
    elif kind == "oblique":  # rotated box hits a moving box off-centre -> spin + 1 or 2 contact points
        a.px, a.py, a.angle, a.vx, a.vy = 400.0, 510.0, 0.3, 50.0, 10.0
        a.dirx, a.diry = np.cos(0.3), np.sin(0.3)
        b.px, b.py, b.angle, b.vx, b.vy = 455.0, 530.0, 2.0, -30.0, -5.0
        b.dirx, b.diry = np.cos(2.0), np.sin(2.0)
    elif kind == "obstacle":  # car slides into a static obstacle box and comes to rest against it
        a.px, a.py, a.angle, a.vx, a.vy = 160.0, 442.0, 0.0, 90.0, 0.0
        a.dirx, a.diry = 1.0, 0.0
    elif kind == "building":  # car leaves the road into a building wall (rests there => persistent contacts)
        a.px, a.py, a.angle, a.vx, a.vy = 500.0, 440.0, -np.pi / 2 + 0.2, 5.0, -40.0
        a.dirx, a.diry = np.cos(a.angle), np.sin(a.angle)
    elif kind == "ped_fast":  # fast car kills a pedestrian (pedHit returns True: solved) and crashes
        a.px, a.py, a.angle, a.vx, a.vy = 660.0, 482.5, 0.0, 55.0, 0.0
        a.dirx, a.diry = 1.0, 0.0
        st.peds[0].py = 484.0
    elif kind == "ped_slow":  # slow car touches a pedestrian: pedHit returns False -> ignored until separation
        a.px, a.py, a.angle, a.vx, a.vy = 683.0, 482.5, 0.0, 0.9, 0.0
        a.dirx, a.diry = 1.0, 0.0
        st.peds[0].py = 484.0
        st.peds[0].vx = -1.0
    elif kind == "pileup":  # three cars in a row + the building: chained arbiters share bodies (multi-level solve)
        a.px, a.py, a.angle, a.vx, a.vy = 300.0, 480.0, 0.0, 70.0, -8.0
        a.dirx, a.diry = 1.0, 0.0
        b.px, b.py, b.angle, b.vx, b.vy = 345.0, 478.0, 0.1, 0.0, 0.0
        b.dirx, b.diry = np.cos(0.1), np.sin(0.1)
        c = st.cars[2]
        c.px, c.py, c.angle, c.vx, c.vy = 388.0, 474.0, -0.4, -70.0, -3.0
        c.dirx, c.diry = np.cos(-0.4), np.sin(-0.4)
    for c in (st.cars[0], st.cars[1], st.cars[2]):
        c.prevx, c.prevy = c.px, c.py
    return st


def _assert_rc_state_equal(sg, so, msg=""):
    dg, do = ol.rc_state_to_dict(sg), ol.rc_state_to_dict(so)
    for k in do:
        if k == "scalars":  # defenders are a set on the device (reported ascending); compare everything else exactly
            continue
        np.testing.assert_array_equal(dg[k], do[k], err_msg="%s field %s" % (msg, k))
    assert [sg.elapsed, sg.ball_owned, sg.n_last_kicked, sg.episode] == [so.elapsed, so.ball_owned, so.n_last_kicked, so.episode], msg
    assert list(sg.last_kicked)[:sg.n_last_kicked] == list(so.last_kicked)[:so.n_last_kicked], msg
    assert list(sg.goals) == list(so.goals) and list(sg.closest) == list(so.closest), msg
    for t in range(2):
        assert sorted(list(sg.defenders[t])[:sg.n_def[t]]) == sorted(list(so.defenders[t])[:so.n_def[t]]), msg + " defenders"


def _rc_actions(rng, E, A):
    return np.stack([rng.integers(0, 5, (E, A)), rng.integers(0, 3, (E, A)), rng.integers(0, 3, (E, A)),
                     rng.integers(0, 7, (E, A))], -1).astype(np.int32)
