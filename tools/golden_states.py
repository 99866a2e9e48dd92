"""Oracle state blobs from the arrays of a recorded fixture (tests/golden/*.npz): what tools/pymunk_crosscheck.py and the golden tests
(tests/golden_common.py) both start a trajectory from.  It lives with the tools: the crosscheck is a tool that the suite runs, and besides this it needs only
tests/oracle_lib.py, whose structs these are, and the fixture generators."""
import oracle_lib as ol


def _state_from_npz(z, tag, which, key):
    cf, ci = z["%s_%s_cars_f" % (tag, which)], z["%s_%s_cars_i" % (tag, which)]
    pf, pi = z["%s_%s_peds_f" % (tag, which)], z["%s_%s_peds_i" % (tag, which)]
    ob, sc = z["%s_%s_obst" % (tag, which)], z["%s_%s_scalars" % (tag, which)]
    st = ol.DrivingState()
    st.elapsed, st.all_finished = int(sc[0]), int(sc[1])
    st.n_cars, st.n_peds, st.n_obst, st.episode = len(cf), len(pf), len(ob), int(key[2])
    for i in range(len(cf)):
        for n, v in zip(ol.CAR_F, cf[i]):
            setattr(st.cars[i], n, float(v))
        for n, v in zip(ol.CAR_I, ci[i]):
            setattr(st.cars[i], n, int(v))
    for i in range(len(pf)):
        for n, v in zip(ol.PED_F, pf[i]):
            setattr(st.peds[i], n, float(v))
        for n, v in zip(ol.PED_I, pi[i]):
            setattr(st.peds[i], n, int(v))
    for i in range(len(ob)):
        st.obst_x[i], st.obst_y[i] = float(ob[i][0]), float(ob[i][1])
    er, epr = z["%s_%s_episode_r" % (tag, which)], z["%s_%s_episode_pos_r" % (tag, which)]
    for i in range(len(er)):
        st.episode_r[i], st.episode_pos_r[i] = float(er[i]), float(epr[i])
    return st


def _to_state(rf, ri, sc, fl, episode):
    st = ol.RoboCupState()
    n = int(sc[1])
    st.elapsed, st.n_robots, st.ball_owned, st.n_last_kicked = int(sc[0]), n, int(sc[2]), int(sc[3])
    for i in range(4):
        st.last_kicked[i] = int(sc[4 + i])
    st.goals[0], st.goals[1], st.closest[0], st.closest[1] = int(sc[8]), int(sc[9]), int(sc[10]), int(sc[11])
    st.n_def[0], st.n_def[1] = int(sc[12]), int(sc[13])
    for i in range(10):
        st.defenders[0][i] = int(sc[14 + i])
        st.defenders[1][i] = int(sc[24 + i])
    st.episode = episode
    st.ball_free_cntr, st.grace_period, st.penal_times[0], st.penal_times[1] = fl[0], fl[1], fl[2], fl[3]
    st.bpx, st.bpy, st.bvx, st.bvy, st.bw, st.bprevx, st.bprevy = fl[4:11]
    for i in range(n):
        for k, v in zip(ol.ROBOT_F, rf[i]):
            setattr(st.robots[i], k, float(v))
        for k, v in zip(ol.ROBOT_I, ri[i]):
            setattr(st.robots[i], k, int(v))
    return st
