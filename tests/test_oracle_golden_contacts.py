"""The oracle against trajectories of the reference's OWN `DrivingEnvironment.step()` WITH collisions (tests/golden/gen_golden_contacts.py:
the reference's Python - processAction, tick, move, carCrash / pedHit / carHit, the friction velocity functions, rewards, getFullState -
on a functional pymunk facade over tests/kat_general.py, the independent GJK / EPA restatement of Chipmunk).  Unlike the free-flight
fixtures these contain crashes, pushes, resting contacts and a killed pedestrian: they pin the COMPOSITION of callbacks and physics inside
a step.  Tolerances: rewards / states 1e-9 (relative to max(1, |value|)), observations 2e-6 (float32), flags and dones exact."""
import os

import numpy as np
import pytest

import oracle_lib as ol
from golden_common import (P_TAGS, RC_MIN_STEPS, RC_TAGS, RCP_MIN_STEPS, RCP_TAGS, TAGS, check_partial_trajectory,
                           check_robocup_trajectory, check_trajectory)

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_fixtures_contain_what_they_are_for():
    z = np.load(os.path.join(G, "driving_contacts.npz"))
    crashed = sum(int(z["%s_states_cars_i" % t][-1][:, 3].sum()) for t in TAGS)      # CAR_I: type team finished crashed lane_pos fric
    dead = sum(int(z["%s_states_peds_i" % t][-1][:, 2].sum()) for t in TAGS)         # PED_I: road side dead ...
    begins = sum(int(z["%s_begins_per_step" % t].sum()) for t in TAGS)
    assert crashed >= 15 and dead >= 2 and begins >= 30, (crashed, dead, begins)
    # l, m: all three cars finished without a crash, allFinished set, and the step in which the last one arrived carries the team reward
    # (maxTime - elapsed) / 100 ~ 59 for every car (DrivingEnvironment.py:281-285, :301); n: one car short, no such step
    for t in "lm":
        assert z[t + "_states_scalars"][-1][1] == 1 and z[t + "_states_cars_i"][-1][:, 2].all() and not z[t + "_states_cars_i"][-1][:, 3].any()
        assert (z[t + "_rewards"] > 50).all(1).sum() == 1 and (z[t + "_rewards"].sum(0) > 115).all(), "one step with the team reward for everybody, on top of each car's own arrival reward"
    assert z["n_states_scalars"][-1][1] == 0 and not (z["n_rewards"] > 50).all(1).any()


@pytest.mark.parametrize("tag", TAGS)
def test_reference_step_with_collisions_against_the_oracle(oracle_built, tag):
    z = np.load(os.path.join(G, "driving_contacts.npz"))

    def make_env(n_players, seed, offset):
        env = ol.OracleEnv(num_envs=1, n_players=n_players, seed=seed, env_id_offset=offset)
        env.reset()

        def step(a):
            o, r, d = env.step(a[None])
            return o[0, 0], r[0], d[0]

        def stats():
            r, p, o, g = env.episode_stats()
            return r[0], p[0], o[0], g[0]
        return (lambda st: env.set_state(0, st)), step, (lambda: env.get_state(0)), stats
    check_trajectory(z, tag, make_env)


# ------------------------------------------------------------------------------------------------ RoboCup


def test_the_robocup_fixtures_contain_what_they_are_for():
    z = np.load(os.path.join(G, "robocup_contacts.npz"))
    assert list(z["l_dones"]) == [0] * 9 + [1] and int(z["l_states_sc"][-1][0]) == 12000, "fixture l ends with the episode's terminal step"
    # ROBOT_I[1] = penalized, [5] = fallen.  m: robots 1 and 7 start penalized and are back in play at the first recorded state (tick's
    # un-penalize branch, RoboCupEnvironment.py:948-968); n: robot 7 falls in a step without any robot-robot touch (processAction :556-560)
    assert z["m_b_ri"][[1, 7], 1].all() and not z["m_states_ri"][0][:, 1].any()
    assert z["n_states_ri"][-1][7, 5] == 1 and z["n_begins"][0] == 0
    begins = sum(z[t + "_begins"] for t in RC_TAGS)     # robot-robot, robot-ball, robot-post, ball-post, own feet
    assert begins[0] >= 30 and begins[1] >= 6 and begins[2] >= 5 and begins[3] >= 1, begins
    kicking = sum(int(z[t + "_states_ri"][:, :, 7].sum()) for t in RC_TAGS)          # ROBOT_I[7] = kicking (pivot joint removed mid-kick)
    assert kicking >= 100, kicking
    fallen = sum(int(z[t + "_states_ri"][:, :, 5].max(0).sum()) for t in RC_TAGS)   # ROBOT_I[5] = fallen
    assert fallen >= 2, fallen


@pytest.mark.parametrize("tag", RC_TAGS)
def test_reference_robocup_step_with_collisions_against_the_oracle(oracle_built, tag):
    z = np.load(os.path.join(G, "robocup_contacts.npz"))

    def make_env(n, seed, offset, flags):
        env = ol.OracleEnv(env_type=0, num_envs=1, n_players=n, seed=seed, env_id_offset=offset, flags=flags)
        env.reset()

        def step(a):
            o, r, d = env.step(a[None])
            return o[0], r[0], d[0]
        return (lambda st: env.set_state(0, st)), step, (lambda: env.get_state(0))
    assert check_robocup_trajectory(z, tag, make_env) >= RC_MIN_STEPS[tag]


# ------------------------------------------------------------------------------------------------ Driving, Partial observations (configs[3])


@pytest.mark.parametrize("tag", P_TAGS)
def test_reference_step_with_partial_observations_and_collisions_against_the_oracle(oracle_built, tag):
    """BASELINE configs[3] as the reference runs it: `step()` with ObservationType.PARTIAL, NoiseType.REALISTIC, noiseMagnitude 3 -
    getAgentVision of every agent inside the step, on top of physics with crashes"""
    z = np.load(os.path.join(G, "driving_partial_contacts.npz"))

    def make_env(n_players, seed, offset, magn):
        env = ol.OracleEnv(env_type=1, num_envs=1, n_players=n_players, obs_type=1, noise_type=1, noise_magnitude=magn, seed=seed, env_id_offset=offset)
        env.reset()

        def step(a):
            o, r, d = env.step(a[None])
            return o[0, 0], r[0], d[0]
        return (lambda st: env.set_state(0, st)), step, (lambda: env.get_state(0))
    rows = check_partial_trajectory(z, tag, make_env)
    assert (rows > 50).all(), rows      # cars, obstacles, pedestrians, lanes seen over the trajectory
    assert tag != "d" or int(z["d_nearby_rows"][0]) >= 30


@pytest.mark.parametrize("tag", RCP_TAGS)
def test_reference_robocup_step_with_partial_observations_against_the_oracle(oracle_built, tag):
    """SURVEY section 8 a17 / f3 as the reference runs it: `RoboCupEnvironment.step()` with ObservationType.PARTIAL + Realistic noise 3 -
    getAgentVision of every agent at the five snapshots inside the step, processSeens' observation rewards folded into the step's rewards"""
    z = np.load(os.path.join(G, "robocup_partial_contacts.npz"))

    def make_env(n, seed, offset, flags, magn):
        env = ol.OracleEnv(env_type=0, num_envs=1, n_players=n, obs_type=1, noise_type=1, noise_magnitude=magn, seed=seed, env_id_offset=offset, flags=flags)
        env.reset()

        def step(a):
            o, r, d = env.step(a[None])
            return o[0], r[0], d[0]
        return (lambda st: env.set_state(0, st)), step, (lambda: env.get_state(0))
    assert check_robocup_trajectory(z, tag, make_env, partial=True) >= RCP_MIN_STEPS[tag]
