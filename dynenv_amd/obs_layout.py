"""The one description of the dense observation row: which blocks of `dynenv_layout()` make up obs[..., 0] (movable objects)
and obs[..., 1] (self / static rows) of the reference's observation, in which order, and where each block's row count lives
(DrivingEnvironment.py:121-124, :977; RoboCupEnvironment.py:440-443 and getAgentVision).  Offsets, capacities and feature widths
are the layout's; the arranger's types (arranger.groups_for) and the compat builders (compat.CompatBuilder) are made from this.
Plain data: no device, no handle."""
from ._capi import ARR_COUNT_CONST, ARR_COUNT_ENV, ARR_COUNT_ROW
from .enums import DynEnvType, ObservationType


def row_groups(layout, env_type, observation_type):
    """-> {"movable": [type...], "static": [type...], "seen": None or (numLandMarks index, ballsSeen index, robotsSeen offset,
    robotsSeen length)} with type = (offset, feat, cap, count_mode, count_value, count_index, count_stride), the leading fields of
    dynenv_arr_type_t.  How many of a block's `cap` rows are filled: always count_value (ARR_COUNT_CONST), column count_index of the
    per-environment counts [E, count_stride] of dynenv_counts (ARR_COUNT_ENV), or float count_index of the row (ARR_COUNT_ROW).
    "seen" is where the third element of a RoboCup Partial observation lives; the other three layouts have (1, 1, 1) there."""
    off, cap, feat = list(layout.block_offset), list(layout.block_rows), list(layout.block_feat)

    def const(k):
        return (off[k], feat[k], cap[k], ARR_COUNT_CONST, cap[k], 0, 0)

    def per_env(k, column):
        return (off[k], feat[k], cap[k], ARR_COUNT_ENV, 0, column, 2)

    def per_row(k, index):
        return (off[k], feat[k], cap[k], ARR_COUNT_ROW, 0, index, 0)

    robocup, partial = env_type == DynEnvType.ROBO_CUP, observation_type == ObservationType.PARTIAL
    seen = None
    if robocup and partial:
        # blocks: balls, robots | goals, crosses, line crosses, lines | tail = 6 list lengths, numLandMarks, ballsSeen, robotsSeen[A - 1]
        t = off[6]
        movable, static = [per_row(k, t + k) for k in (0, 1)], [per_row(k, t + k) for k in (2, 3, 4, 5)]
        seen = (t + 6, t + 7, t + 8, layout.n_agents - 1)
    elif robocup:  # blocks: ball, self, the other robots
        movable, static = [const(0), const(2)], [const(1)]
    elif partial:  # blocks: self, cars, obstacles, pedestrians, lanes, tail = the 4 list lengths
        t = off[5]
        movable, static = [per_row(1, t), per_row(2, t + 1), per_row(3, t + 2)], [const(0), per_row(4, t + 3)]
    else:  # blocks: self, the other cars, obstacles and pedestrians of the environment, lanes
        movable, static = [const(1), per_env(2, 0), per_env(3, 1)], [const(0), const(4)]
    return {"movable": movable, "static": static, "seen": seen}
