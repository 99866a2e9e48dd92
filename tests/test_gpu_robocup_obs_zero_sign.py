"""The sign of zero in RoboCup's Full observation (-m gpu).  Column 2 of an agent's row is ballOwned * team, an INT product in the
reference (RoboCupEnvironment.py:1149-1189) and in the oracle: a free ball reads +0.0f for either team.  A float product gives -0.0f for
team -1, which a float comparison cannot see (-0.0 == 0.0): this test compares int32 views, for the reset observation (dynenv_reset,
randomInit: the ball starts free in two environments of five) and for dynenv_step."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu


def test_a_free_ball_reads_plus_zero_for_both_teams(oracle_built):
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType
    E, n, steps = 70, 5, 12
    flags = ol.ROBOCUP_DEFAULT_FLAGS | ol.FLAG_RANDOM_INIT
    env = BatchedDynEnv(DynEnvType.ROBO_CUP, E, n, seed=31, flags=flags)
    ora = ol.OracleEnv(env_type=0, num_envs=E, n_players=n, seed=31, flags=flags, threads=8)
    og, oc = env.reset_flat().cpu().numpy(), ora.reset()
    free = [e for e in range(E) if ora.get_state(e).ball_owned == 0]
    assert len(free) >= E // 5, "randomInit should leave the ball free in about 40 % of the environments"
    assert (oc[free][:, :, n:, 2].view(np.int32) == 0).all(), "the oracle writes +0.0f for team -1 and a free ball"
    assert np.array_equal(og.view(np.int32), oc.view(np.int32)), "reset observation"
    rng = np.random.default_rng(5)
    seen_free = 0
    for s in range(steps):
        a = np.stack([rng.integers(0, h, (E, 2 * n)) for h in (5, 3, 3, 7)], -1).astype(np.int32)
        og, rg, dg = env.step_flat(torch.tensor(a, device="cuda"), auto_reset=False)
        oc, rc, dc = ora.step(a)
        seen_free += sum(ora.get_state(e).ball_owned == 0 for e in range(E))
        assert np.array_equal(og.cpu().numpy().view(np.int32), oc.view(np.int32)), "observations, step %d" % s
        assert np.array_equal(rg.cpu().numpy().view(np.int64), rc.view(np.int64)), "rewards, step %d" % s
    assert seen_free > 0
    assert env.error_flags() == 0
    env.close()
    ora.close()
