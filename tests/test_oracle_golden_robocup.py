"""The RoboCup oracle (oracle/robocup.c) against fixtures computed by the reference's own Python
(tests/golden/gen_golden_robocup.py): processAction, tick, isBallOutOfField/ballFreeKickProcess, penalize/
getFreePenaltySpot, the begin callbacks, Full-observation formatting and the kick-off spot formulas."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from golden_common import _check, _to_state

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def z(oracle_built):
    return np.load(os.path.join(G, "robocup_unit.npz"))


def _run(z, tag, call, flags=0):
    key = [int(x) for x in z["key"]]
    env = ol.OracleEnv(env_type=0, num_envs=1, n_players=5, seed=key[0], env_id_offset=key[1], flags=flags)
    env.reset()
    n = len(z[tag + "_rew"])
    for t in range(n):
        st = _to_state(z[tag + "_b_rf"][t], z[tag + "_b_ri"][t], z[tag + "_b_sc"][t], z[tag + "_b_fl"][t], key[2])
        env.set_state(0, st)
        rew = np.zeros(22)
        ret = call(env, z[tag + "_extra"][t], rew)
        got = env.get_state(0)
        _check(got, z[tag + "_a_rf"][t], z[tag + "_a_ri"][t], z[tag + "_a_sc"][t], z[tag + "_a_fl"][t], "%s trial %d" % (tag, t))
        np.testing.assert_allclose(rew, z[tag + "_rew"][t], rtol=1e-10, atol=1e-12, err_msg="%s trial %d rewards" % (tag, t))
        yield t, ret, z[tag + "_extra"][t], env


def test_process_action(z):
    def call(env, extra, rew):
        act = np.array(extra[:4], np.int32)
        env.l.oracle_rc_process_action(env.h, 0, int(extra[4]), act.ctypes.data_as(C.c_void_p), rew.ctypes.data_as(C.c_void_p))
    for _ in _run(z, "pa", call):
        pass


def test_tick_all_branches(z):
    def call(env, extra, rew):
        env.l.oracle_rc_tick(env.h, 0, int(extra[0]), rew.ctypes.data_as(C.c_void_p))
        return env.l.oracle_rc_joint_count(env.h, 0)
    for t, joints, extra, env in _run(z, "tick", call):
        assert joints - 10 == int(extra[2]), "trial %d: pivot joints in space after tick (kick FSM add/remove)" % t


def test_ball_out_of_field_and_free_kick(z):
    def call(env, extra, rew):
        return env.l.oracle_rc_ball(env.h, 0, rew.ctypes.data_as(C.c_void_p))
    for t, fin, extra, env in _run(z, "ball", call):
        assert fin == int(extra[0]), "trial %d finished flag" % t


def test_penalize_and_free_spot(z):
    def call(env, extra, rew):
        env.l.oracle_rc_penalize(env.h, 0, int(extra[0]), rew.ctypes.data_as(C.c_void_p))
        return env.l.oracle_rc_joint_count(env.h, 0)
    for t, joints, extra, env in _run(z, "pen", call):
        assert joints - 10 == int(extra[2]), "trial %d joints" % t


@pytest.mark.parametrize("can_fall", [0, 1])
def test_begin_callbacks(z, can_fall):
    key = [int(x) for x in z["key"]]
    flags = ol.FLAG_CAN_FALL if can_fall else 0
    env = ol.OracleEnv(env_type=0, num_envs=1, n_players=5, seed=key[0], env_id_offset=key[1], flags=flags)
    env.reset()
    n = len(z["cb_rew"])
    done = 0
    for t in range(n):
        extra = z["cb_extra"][t]
        if int(extra[3]) != can_fall:
            continue
        st = _to_state(z["cb_b_rf"][t], z["cb_b_ri"][t], z["cb_b_sc"][t], z["cb_b_fl"][t], key[2])
        env.set_state(0, st)
        rew = np.zeros(22)
        ret = env.l.oracle_rc_begin(env.h, 0, int(extra[0]), int(extra[1]), rew.ctypes.data_as(C.c_void_p))
        assert ret == int(extra[2])
        _check(env.get_state(0), z["cb_a_rf"][t], z["cb_a_ri"][t], z["cb_a_sc"][t], z["cb_a_fl"][t], "cb trial %d" % t)
        np.testing.assert_allclose(rew, z["cb_rew"][t], rtol=1e-10, atol=1e-12)
        done += 1
    assert done > 20


def test_full_observation_formatting(z):
    key = [int(x) for x in z["key"]]
    for t in range(len(z["obs_flat"])):
        n = int(z["obs_extra"][t][0])
        env = ol.OracleEnv(env_type=0, num_envs=1, n_players=n, seed=1, flags=0)
        env.reset()
        st = _to_state(z["obs_b_rf"][t], z["obs_b_ri"][t], z["obs_b_sc"][t], z["obs_b_fl"][t], key[2])
        env.set_state(0, st)
        # a zero-length "step" is not available; use reset-free path: write obs through a dedicated hook
        out = np.zeros((2 * n, env.D), np.float32)
        env.l.oracle_rc_obs(env.h, 0, out.ctypes.data_as(C.c_void_p))
        np.testing.assert_allclose(out, z["obs_flat"][t][:2 * n, :env.D], rtol=0, atol=2e-6, err_msg="trial %d" % t)


def test_kickoff_spots(z):
    l = ol.lib()
    for row in z["spots"]:
        draws, exp = row[:18].copy(), row[18:].reshape(2, 5, 2)
        out = np.zeros((2, 5, 2))
        l.oracle_rc_spots(draws.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        np.testing.assert_allclose(out, exp, rtol=1e-14, atol=1e-12)
