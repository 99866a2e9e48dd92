"""What the tests against the reference's recorded vectors (tests/golden/*.npz) and the tools that replay such trajectories share: state
blobs from a fixture's arrays, the state comparisons, and the trajectory checks with their tags.  A helper module: no test in here."""
import os
import sys

import numpy as np

import oracle_lib as ol

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from golden_states import _state_from_npz, _to_state  # noqa: E402, F401  (the tests take them from here)

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check(st, rf, ri, sc, fl, msg, skip_def_order=False):
    n = int(sc[1])
    got_f = np.array([[getattr(st.robots[i], k) for k in ol.ROBOT_F] for i in range(n)])
    got_i = np.array([[getattr(st.robots[i], k) for k in ol.ROBOT_I] for i in range(n)])
    np.testing.assert_allclose(got_f, rf[:n], rtol=RT, atol=AT, err_msg=msg + " robot floats")
    np.testing.assert_array_equal(got_i, ri[:n], err_msg=msg + " robot ints")
    assert [st.elapsed, st.ball_owned, st.n_last_kicked] == [int(sc[0]), int(sc[2]), int(sc[3])], msg
    assert list(st.last_kicked)[:st.n_last_kicked] == [int(x) for x in sc[4:4 + int(sc[3])]], msg + " lastKicked"
    assert [st.goals[0], st.goals[1], st.closest[0], st.closest[1]] == [int(x) for x in sc[8:12]], msg + " goals/closest"
    assert [st.n_def[0], st.n_def[1]] == [int(sc[12]), int(sc[13])], msg + " defenders"
    assert list(st.defenders[0])[:st.n_def[0]] == [int(x) for x in sc[14:14 + st.n_def[0]]], msg
    assert list(st.defenders[1])[:st.n_def[1]] == [int(x) for x in sc[24:24 + st.n_def[1]]], msg
    got_fl = [st.ball_free_cntr, st.grace_period, st.penal_times[0], st.penal_times[1], st.bpx, st.bpy, st.bvx, st.bvy,
              st.bw, st.bprevx, st.bprevy]
    np.testing.assert_allclose(got_fl, fl, rtol=RT, atol=AT, err_msg=msg + " env floats")

TAGS = list("abcdefghijklmn")   # k: one whole episode, terminal step included; l, m: every car reaches its goal (allFinished, team reward); n: all but one


def _close(got, want, tol, msg):
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.size == 0 or float(err.max()) <= tol, "%s: deviation %.3e at %s" % (msg, err.max(), np.unravel_index(err.argmax(), err.shape))


def check_trajectory(z, tag, make_env):
    """make_env(n_players, seed, env_id_offset) -> (set_state(st), step(actions [A, 2]) -> (obs [A, D], rewards [A], done), get_state())"""
    key = z["%s_key" % tag]
    st0 = _state_from_npz(z, tag, "init", key)
    made = make_env(st0.n_cars, int(key[0]), int(key[1]))
    set_state, step, get_state = made[:3]
    set_state(st0)
    acts, marks = z["%s_actions" % tag], list(z["%s_state_steps" % tag])
    every = int(z["%s_obs_every" % tag][0]) if "%s_obs_every" % tag in z else 1   # (the whole-episode fixture keeps every 10th observation)
    n_obs = 0
    for s in range(len(acts)):
        o, r, d = step(acts[s].astype(np.int32))
        _close(r, z["%s_rewards" % tag][s], 1e-9, "%s: rewards of step %d" % (tag, s))
        assert int(d) == int(z["%s_dones" % tag][s])
        if s % every == every - 1 or s == len(acts) - 1:
            np.testing.assert_allclose(o, z["%s_obs" % tag][n_obs], rtol=0, atol=2e-6, err_msg="%s: observation of step %d" % (tag, s))
            n_obs += 1
        if int(d):   # the terminal step: info['episode_r'], ['episode_p_r'], ['episode_o_r'], ['episode_g'] (DrivingEnvironment.py:309-316)
            assert s == len(acts) - 1 == 599 and len(made) == 4
            er, ep, eo, g = made[3]()
            want = z["%s_episode_info" % tag]
            _close(er, want[0], 1e-9, tag + ": episode_r"); _close(ep, want[1], 1e-9, tag + ": episode_p_r"); _close(eo, want[2], 0.0, tag + ": episode_o_r")
            np.testing.assert_array_equal(np.asarray(g, float), z["%s_episode_goals" % tag])
        if s in marks:
            k = marks.index(s)
            got = ol.state_to_dict(get_state())
            _close(got["cars_f"], z["%s_states_cars_f" % tag][k], 1e-9, "%s: cars after step %d" % (tag, s))
            _close(got["peds_f"], z["%s_states_peds_f" % tag][k], 1e-9, "%s: pedestrians after step %d" % (tag, s))
            np.testing.assert_array_equal(got["cars_i"], z["%s_states_cars_i" % tag][k], err_msg="%s: car flags after step %d" % (tag, s))
            np.testing.assert_array_equal(got["peds_i"], z["%s_states_peds_i" % tag][k], err_msg="%s: pedestrian flags after step %d" % (tag, s))
            _close(got["episode_r"], z["%s_states_episode_r" % tag][k], 1e-9, "%s: episode rewards after step %d" % (tag, s))
            _close(got["episode_pos_r"], z["%s_states_episode_pos_r" % tag][k], 1e-9, "%s: positive episode rewards after step %d" % (tag, s))
            if "%s_states_scalars" % tag in z:   # elapsed, allFinished
                np.testing.assert_array_equal(got["scalars"][:2], z["%s_states_scalars" % tag][k], err_msg="%s: elapsed / allFinished after step %d" % (tag, s))
RC_TAGS = list("abcdefghijklmn")   # l: the last ten steps of an episode, terminal step included; m: two penalties expire; n: a walking robot trips
RC_MIN_STEPS = {"a": 30, "b": 40, "c": 50, "d": 30, "e": 12, "f": 20, "g": 25, "h": 40, "i": 30, "j": 60, "k": 15, "l": 10, "m": 6, "n": 5}   # steps of each trajectory that are well-conditioned (and checked)


def _rc_check_state(st, rf, ri, sc, fl, msg, tol=1e-9):
    n = int(sc[1])
    got_f = np.array([[getattr(st.robots[i], k) for k in ol.ROBOT_F] for i in range(n)])
    got_i = np.array([[getattr(st.robots[i], k) for k in ol.ROBOT_I] for i in range(n)])
    _close(got_f, rf[:n], tol, msg + ": robot floats")
    np.testing.assert_array_equal(got_i, ri[:n], err_msg=msg + ": robot flags")
    assert [st.elapsed, st.ball_owned, st.n_last_kicked] == [int(sc[0]), int(sc[2]), int(sc[3])], msg
    assert list(st.last_kicked)[:st.n_last_kicked] == [int(x) for x in sc[4:4 + int(sc[3])]], msg + ": lastKicked"
    assert [st.goals[0], st.goals[1], st.closest[0], st.closest[1]] == [int(x) for x in sc[8:12]], msg + ": goals / closest"
    assert [st.n_def[0], st.n_def[1]] == [int(sc[12]), int(sc[13])], msg + ": defenders"
    _close([st.ball_free_cntr, st.grace_period, st.penal_times[0], st.penal_times[1], st.bpx, st.bpy, st.bvx, st.bvy, st.bw, st.bprevx,
            st.bprevy], fl, tol, msg + ": ball / timers")
RCP_TAIL = 793 - 17   # oracle/robocup_partial.h: the row's last 17 entries are list lengths and the seen tuple (exact)
RCP_OFF_LINE = 32 * 5 + 20 * 7 + 16 * 6 + 16 * 6 + 28 * 8   # oracle/robocup_partial.h: the line block [12][5] of a Partial row


def _own_line_excused(got, want, tol):
    """A penalized robot stands exactly ON its side line (its penalty spot), so that line passes through the robot's own position and
    cutils.isLineInArea (:751-828) returns either nothing or a zero-length line AT the robot - which of the two is decided by the last
    bit of libm's sin / cos of the field-of-view edges (the oracle's are within 2 ulp of glibc's, tests/test_detmath.py, not identical).
    True if two rows differ by exactly that: one more line on one side, that line degenerate (normalized distance -1), everything else equal."""
    gt, wt = got[RCP_TAIL:], want[RCP_TAIL:]
    d = gt - wt
    if not (abs(d[5]) == 1 and d[6] == d[5] and not np.delete(d, [5, 6]).any()):
        return False
    lng, sht = (got, want) if d[5] > 0 else (want, got)
    nl = int(lng[RCP_TAIL + 5])
    a, b = lng[RCP_OFF_LINE:RCP_OFF_LINE + 5 * nl].reshape(nl, 5), sht[RCP_OFF_LINE:RCP_OFF_LINE + 5 * (nl - 1)].reshape(nl - 1, 5)
    for j in range(nl):
        if a[j][0] < -0.999 and np.allclose(np.delete(a, j, 0), b, rtol=2e-6, atol=max(2e-6, 10 * tol)):
            return np.allclose(got[:RCP_OFF_LINE], want[:RCP_OFF_LINE], rtol=2e-6, atol=max(2e-6, 10 * tol))
    return False


def check_robocup_trajectory(z, tag, make_env, partial=False, own_line_slack=None):
    """make_env(n, seed, offset, flags[, noise magnitude]) -> (set_state(st), step(actions [R, 4]) -> (obs [5, R, D], rewards [R], done), get_state())
    own_line_slack (a list, Partial only; tools/reference_step_fuzz.py): rows that differ by `_own_line_excused` are appended to it as (step, snapshot,
    robot) instead of failing; such a robot's rewards (processSeens: 0.0025 x the mean landmark count of the five snapshots) get 0.0026 of slack"""
    n, can_fall, seed, genv, episode, _, _ = [int(x) for x in z[tag + "_meta"]]
    flags = (ol.FLAG_CAN_FALL if can_fall else 0) | ol.FLAG_USE_OBS_REWARDS
    set_state, step, get_state = make_env(n, seed, genv, flags, float(z[tag + "_noise"][1])) if partial else make_env(n, seed, genv, flags)
    set_state(_to_state(z[tag + "_b_rf"], z[tag + "_b_ri"], z[tag + "_b_sc"], z[tag + "_b_fl"], episode))
    acts, marks, R = z[tag + "_actions"], list(z[tag + "_state_steps"]), 2 * n
    # The fixture carries its own conditioning: per window of steps (up to each recorded state), how far a twin of the reference run had
    # drifted whose velocities got a relative 1e-15 nudge before every physics substep.  RoboCup's contact phases amplify rounding by orders
    # of magnitude now and then (nearly parallel feet, duplicate end-cap contacts under friction 6.25; profiles/r05_kat_general_fuzz.txt):
    # the tolerance of a window is 1e-9 or 1000 x the twin's largest drift in it, and where the twin is off by more than 1e-6 the
    # trajectory pins nothing any more: the check ends.
    cond = list(z[tag + "_conditioning"])
    checked = 0
    mine = []    # this trajectory's excused rows
    for s in range(len(acts)):
        k = min(i for i, m in enumerate(marks) if m >= s)
        if cond[k] > 1e-6:
            break
        tol = max(1e-9, 1e3 * cond[k])
        o, r, d = step(acts[s].astype(np.int32))
        want = z[tag + "_obs"][s][:, :R, :o.shape[-1]]
        if partial and own_line_slack is not None:
            o, want, r = np.array(o), np.array(want), np.array(r)
            for t in range(o.shape[0]):
                for a in range(R):
                    if not np.array_equal(o[t, a, RCP_TAIL:], want[t, a, RCP_TAIL:]) and _own_line_excused(o[t, a], want[t, a], tol):
                        own_line_slack.append((s, t, a)); mine.append((s, t, a))
                        o[t, a] = want[t, a]
            slack = sorted(set(a for (s_, _, a) in mine))          # (episode sums carry a deviation on)
            for a in slack:
                if abs(r[a] - z[tag + "_rewards"][s][a]) <= 0.0026:
                    r[a] = z[tag + "_rewards"][s][a]
        _close(r, z[tag + "_rewards"][s], tol, "%s: rewards of step %d" % (tag, s))
        assert int(d) == int(z[tag + "_dones"][s])
        if partial:   # list lengths and the seen tuple exact, rows to float32 accuracy (as tests/test_oracle_golden_robocup_partial.py)
            np.testing.assert_array_equal(o[..., RCP_TAIL:], want[..., RCP_TAIL:], err_msg="%s: list lengths / seen tuple of step %d" % (tag, s))
            np.testing.assert_allclose(o[..., :RCP_TAIL], want[..., :RCP_TAIL], rtol=2e-6, atol=max(2e-6, 10 * tol), err_msg="%s: Partial observation of step %d" % (tag, s))
        else:
            np.testing.assert_allclose(o, want, rtol=0, atol=max(2e-6, 10 * tol), err_msg="%s: observation (5 snapshots) of step %d" % (tag, s))
        if s in marks:
            st = get_state()
            _rc_check_state(st, z[tag + "_states_rf"][k], z[tag + "_states_ri"][k], z[tag + "_states_sc"][k], z[tag + "_states_fl"][k],
                            "%s: state after step %d" % (tag, s), tol)
            # episodeRewards / episodePosRewards (info['episode_r'] / ['episode_p_r'] of the terminal step, RoboCupEnvironment.py:516-521)
            if not mine:
                _close(list(st.episode_r)[:R] + list(st.episode_pos_r)[:R], z[tag + "_episode"][s], max(tol, 1e-9) * (s + 1), "%s: episode sums after step %d" % (tag, s))
        checked = s + 1
    return checked
P_TAGS = ["a", "b", "c", "d"]   # d: pedestrians within 20 px of an obstacle's centre: the `Nearby` noise multiplier (cutils.py:514-515) on 36 rows


def check_partial_trajectory(z, tag, make_env):
    """make_env(n_players, seed, offset, noise_magnitude) -> (set_state, step(actions [A, 2]) -> (obs [A, 517], rewards [A], done), get_state)"""
    key = z["%s_key" % tag]
    n_players, _, magn = z["%s_cfg" % tag]
    st0 = _state_from_npz(z, tag, "init", key)
    set_state, step, get_state = make_env(int(n_players), int(key[0]), int(key[1]), float(magn))
    set_state(st0)
    acts = z["%s_actions" % tag]
    rows = np.zeros(4)
    for s in range(len(acts)):
        o, r, d = step(acts[s].astype(np.int32))
        _close(r, z["%s_rewards" % tag][s], 1e-9, "%s: rewards of step %d" % (tag, s))
        assert int(d) == int(z["%s_dones" % tag][s])
        want = z["%s_obs" % tag][s]
        np.testing.assert_array_equal(o[:, -4:], want[:, -4:], err_msg="%s: row counts of step %d" % (tag, s))
        np.testing.assert_allclose(o, want, rtol=0, atol=3e-5, err_msg="%s: Partial observation of step %d" % (tag, s))   # (the tolerance of test_oracle_golden_partial.py)
        rows += o[:, -4:].sum(0)
    got = ol.state_to_dict(get_state())
    _close(got["cars_f"], z["%s_final_cars_f" % tag], 1e-9, tag + ": final cars")
    _close(got["peds_f"], z["%s_final_peds_f" % tag], 1e-9, tag + ": final pedestrians")
    np.testing.assert_array_equal(got["cars_i"], z["%s_final_cars_i" % tag])
    np.testing.assert_array_equal(got["peds_i"], z["%s_final_peds_i" % tag])
    return rows
RCP_TAGS = ["a", "b", "c"]
RCP_MIN_STEPS = {"a": 20, "b": 20, "c": 25}

RT, AT = 1e-11, 1e-10
