"""The independent reference of the compat observation array: the plain triple loop over (env, time, agent) that the product
used to carry as `BatchedDynEnv._compat_obs`, kept word for word with its hand-written feature widths and offsets.  The
product builds the same array from one description of the row (dynenv_amd.obs_layout); this module must never import that
description or anything derived from it - the arranger tests check the arranger kernels, whose types come from the same
description, against what this loop builds."""
import numpy as np

from dynenv_amd.enums import DynEnvType, ObservationType


def compat_obs(layout, env_type, observation_type, n_agents, dense, counts):
    """dense [E,T,A,D] (numpy) -> object ndarray [E,T,A,3] of ((cars, obstacles, peds), (self, lanes), (1,1,1)) for Driving,
    ((ball, robots), (self,), (1,1,1)) for RoboCup Full, ((balls, robots), (goals, crosses, line crosses, lines),
    (numLandMarks, robotsSeen, ballsSeen)) for RoboCup Partial.  `counts`: int [E, 2] (obstacles, pedestrians) of Driving Full."""
    assert isinstance(dense, np.ndarray), "copy a device tensor to the host first"
    o = dense
    E, T, A, D = o.shape
    assert A == n_agents
    L = layout
    off, rows, feat = list(L.block_offset), list(L.block_rows), list(L.block_feat)
    out = np.empty((E, T, A, 3), dtype=object)
    if env_type == DynEnvType.ROBO_CUP and observation_type == ObservationType.PARTIAL:
        # getAgentVision: ((balls, robots), (goals, crosses, line crosses, lines), (numLandMarks, robotsSeen, ballsSeen))
        tail = off[6]
        for e in range(E):
            for t in range(T):
                for a in range(A):
                    r = o[e, t, a]
                    n = [int(x) for x in r[tail:tail + 6]]
                    lists = [r[off[k]:off[k] + n[k] * feat[k]].reshape(n[k], feat[k]) for k in range(6)]
                    out[e, t, a, 0] = [lists[0], lists[1]]
                    out[e, t, a, 1] = [lists[2], lists[3], lists[4], lists[5]]
                    out[e, t, a, 2] = (int(r[tail + 6]), r[tail + 8:tail + 8 + (A - 1)].astype("uint8"), bool(r[tail + 7]))
        return out
    ones = (1, 1, 1)
    if env_type == DynEnvType.ROBO_CUP:  # ((ball, robots), (self,), (1,1,1)) RoboCupEnvironment.py:440-443
        ball = o[..., 0:4].reshape(E, T, A, 1, 4)
        selfr = o[..., 4:12].reshape(E, T, A, 1, 8)
        robs = o[..., 12:12 + (A - 1) * 6].reshape(E, T, A, A - 1, 6)
        for e in range(E):
            for t in range(T):
                for a in range(A):
                    out[e, t, a, 0] = [ball[e, t, a], robs[e, t, a]]
                    out[e, t, a, 1] = [selfr[e, t, a], ]
                    out[e, t, a, 2] = ones
        return out
    if observation_type == ObservationType.PARTIAL:  # ragged rows of getAgentVision, lengths in the last 4 floats
        cars = o[..., off[1]:off[1] + rows[1] * 7].reshape(E, T, A, rows[1], 7)
        obst = o[..., off[2]:off[2] + rows[2] * 6].reshape(E, T, A, rows[2], 6)
        peds = o[..., off[3]:off[3] + rows[3] * 2].reshape(E, T, A, rows[3], 2)
        lanes = o[..., off[4]:off[4] + rows[4] * 4].reshape(E, T, A, rows[4], 4)
        selfr = o[..., 0:9].reshape(E, T, A, 1, 9)
        n = o[..., D - 4:].astype(np.int64)
        for e in range(E):
            for t in range(T):
                for a in range(A):
                    nc, no, npd, nl = n[e, t, a]
                    out[e, t, a, 0] = [cars[e, t, a, :nc], obst[e, t, a, :no], peds[e, t, a, :npd]]
                    out[e, t, a, 1] = [selfr[e, t, a], lanes[e, t, a, :nl]]
                    out[e, t, a, 2] = ones
        return out
    selfr = o[..., off[0]:off[0] + 9].reshape(E, T, A, 1, 9)
    cars = o[..., off[1]:off[1] + rows[1] * 7].reshape(E, T, A, rows[1], 7)
    obst = o[..., off[2]:off[2] + rows[2] * 4].reshape(E, T, A, rows[2], 4)
    peds = o[..., off[3]:off[3] + rows[3] * 2].reshape(E, T, A, rows[3], 2)
    lanes = o[..., off[4]:off[4] + rows[4] * 5].reshape(E, T, A, rows[4], 5)
    for e in range(E):
        n_obst, n_ped = int(counts[e, 0]), int(counts[e, 1])
        for t in range(T):
            for a in range(A):
                out[e, t, a, 0] = [cars[e, t, a], obst[e, t, a, :n_obst], peds[e, t, a, :n_ped]]
                out[e, t, a, 1] = [selfr[e, t, a], lanes[e, t, a]]
                out[e, t, a, 2] = ones
    return out


def compat_obs_of(env, dense, counts=None):
    """`compat_obs` for a BatchedDynEnv handle; `dense` may be a device tensor (copied to the host here)."""
    if not isinstance(dense, np.ndarray):
        dense = dense.detach().cpu().numpy()
    if counts is not None and not isinstance(counts, np.ndarray):
        counts = counts.cpu().numpy()
    return compat_obs(env.layout, env.env_type, env.observationType, env.n_agents, dense, counts)
