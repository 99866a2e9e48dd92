"""The one description of the observation row (dynenv_amd.obs_layout.row_groups) on the oracle's layouts - the same dense layout as
the library's: the arranger types made from it are the ones groups_for spelled out by hand before, and the description is
consistent in itself."""
import types

import numpy as np
import pytest

DRIVING_PARTIAL = ([(9, 7, 24, 2, 0, 513, 0), (177, 6, 32, 2, 0, 514, 0), (369, 2, 40, 2, 0, 515, 0)],
                   [(0, 9, 1, 0, 1, 0, 0), (449, 4, 16, 2, 0, 516, 0)])
ROBOCUP_PARTIAL = ([(0, 5, 32, 2, 0, 776, 0), (160, 7, 20, 2, 0, 777, 0)],
                   [(300, 6, 16, 2, 0, 778, 0), (396, 6, 16, 2, 0, 779, 0), (492, 8, 28, 2, 0, 780, 0), (716, 5, 12, 2, 0, 781, 0)])
# (env_type, partial, players) -> (n_agents, obs_dim, movable, static); a type is (offset, feat, cap, count_mode, count_value,
# count_index, count_stride).  Written down from groups_for as it was when it listed the four layouts by hand.
GROUPS = {
    (1, 0, 1): (1, 169, [(9, 7, 0, 0, 0, 0, 0), (9, 4, 20, 1, 0, 0, 2), (89, 2, 20, 1, 0, 1, 2)],
                [(0, 9, 1, 0, 1, 0, 0), (129, 5, 8, 0, 8, 0, 0)]),
    (1, 0, 2): (2, 176, [(9, 7, 1, 0, 1, 0, 0), (16, 4, 20, 1, 0, 0, 2), (96, 2, 20, 1, 0, 1, 2)],
                [(0, 9, 1, 0, 1, 0, 0), (136, 5, 8, 0, 8, 0, 0)]),
    (1, 0, 5): (5, 197, [(9, 7, 4, 0, 4, 0, 0), (37, 4, 20, 1, 0, 0, 2), (117, 2, 20, 1, 0, 1, 2)],
                [(0, 9, 1, 0, 1, 0, 0), (157, 5, 8, 0, 8, 0, 0)]),
    (1, 0, 10): (10, 232, [(9, 7, 9, 0, 9, 0, 0), (72, 4, 20, 1, 0, 0, 2), (152, 2, 20, 1, 0, 1, 2)],
                 [(0, 9, 1, 0, 1, 0, 0), (192, 5, 8, 0, 8, 0, 0)]),
    (1, 1, 1): (1, 517) + DRIVING_PARTIAL,
    (1, 1, 2): (2, 517) + DRIVING_PARTIAL,
    (1, 1, 5): (5, 517) + DRIVING_PARTIAL,
    (1, 1, 10): (10, 517) + DRIVING_PARTIAL,
    (0, 0, 1): (2, 18, [(0, 4, 1, 0, 1, 0, 0), (12, 6, 1, 0, 1, 0, 0)], [(4, 8, 1, 0, 1, 0, 0)]),
    (0, 0, 2): (4, 30, [(0, 4, 1, 0, 1, 0, 0), (12, 6, 3, 0, 3, 0, 0)], [(4, 8, 1, 0, 1, 0, 0)]),
    (0, 0, 5): (10, 66, [(0, 4, 1, 0, 1, 0, 0), (12, 6, 9, 0, 9, 0, 0)], [(4, 8, 1, 0, 1, 0, 0)]),
    (0, 0, 10): (10, 66, [(0, 4, 1, 0, 1, 0, 0), (12, 6, 9, 0, 9, 0, 0)], [(4, 8, 1, 0, 1, 0, 0)]),  # 5 per team at the most
    (0, 1, 1): (2, 793) + ROBOCUP_PARTIAL,
    (0, 1, 2): (4, 793) + ROBOCUP_PARTIAL,
    (0, 1, 5): (10, 793) + ROBOCUP_PARTIAL,
    (0, 1, 10): (10, 793) + ROBOCUP_PARTIAL,
}


def _oracle(ol, env_type, partial, players):
    kw = dict(obs_type=1, noise_type=1, noise_magnitude=3.0) if partial else {}
    return ol.OracleEnv(env_type=env_type, num_envs=2, n_players=players, seed=3,
                        flags=ol.ROBOCUP_DEFAULT_FLAGS if env_type == 0 else 0, **kw)


@pytest.mark.parametrize("env_type,partial,players", sorted(GROUPS))
def test_groups_for_gives_the_arranger_types_it_always_gave(oracle_built, env_type, partial, players):
    from dynenv_amd import DynEnvType, ObservationType, groups_for
    ora = _oracle(oracle_built, env_type, partial, players)

    env = types.SimpleNamespace(layout=ora.layout, n_agents=ora.A, obs_dim=ora.D, env_type=DynEnvType(env_type),
                                observationType=ObservationType(partial))  # what groups_for reads of a BatchedDynEnv
    n_agents, obs_dim, movable, static = GROUPS[(env_type, partial, players)]
    assert (ora.A, ora.D) == (n_agents, obs_dim)
    got = groups_for(env)
    assert sorted(got) == ["movable", "static"]
    fields = lambda t: (t.offset, t.feat, t.cap, t.count_mode, t.count_value, t.count_index, t.count_stride)
    assert [fields(t) for t in got["movable"]] == movable and [fields(t) for t in got["static"]] == static
    assert all(t.reserved == 0 for g in got.values() for t in g)


@pytest.mark.parametrize("env_type,partial,players", sorted(GROUPS))
def test_row_description_is_consistent(oracle_built, env_type, partial, players):
    """the blocks the description names lie inside the row and do not overlap; a count kept in the row (and the 'seen' triple of
    RoboCup Partial) lies inside the row and outside every data block; capacities hold the constant counts"""
    from dynenv_amd import _capi
    from dynenv_amd.obs_layout import row_groups
    ora = _oracle(oracle_built, env_type, partial, players)
    D = ora.D
    g = row_groups(ora.layout, env_type, partial)
    assert sorted(g) == ["movable", "seen", "static"]
    blocks = g["movable"] + g["static"]
    used = np.zeros(D, np.int32)
    for off, feat, cap, mode, value, index, stride in blocks:
        assert feat > 0 and cap >= 0 and 0 <= off and off + cap * feat <= D
        used[off:off + cap * feat] += 1
        assert mode in (_capi.ARR_COUNT_CONST, _capi.ARR_COUNT_ENV, _capi.ARR_COUNT_ROW)
        if mode == _capi.ARR_COUNT_CONST:
            assert 0 <= value <= cap
        if mode == _capi.ARR_COUNT_ENV:
            assert 0 <= index < stride == 2   # dynenv_counts: (obstacles, pedestrians) per environment
    assert used.max() <= 1, "blocks overlap"
    in_row = [index for _, _, _, mode, _, index, _ in blocks if mode == _capi.ARR_COUNT_ROW]
    assert (g["seen"] is not None) == (env_type == 0 and bool(partial))
    if g["seen"] is not None:
        landmarks, balls, lo, n = g["seen"]
        assert n == ora.A - 1
        in_row += [landmarks, balls] + list(range(lo, lo + n))
    assert len(set(in_row)) == len(in_row), "two values in one float of the row"
    for index in in_row:
        assert 0 <= index < D and used[index] == 0, index
