"""numpy float64 statement of the fused embed-and-pad contract (include/dynenv.h, dynenv_arrange_embed_pad): the reference's EmbedBlock
(DynEnv/models/models.py:99-124) as arithmetic, and the padded tensor of its whole InputLayer (:278-307) built on arranger_ref.py
(default mode) and arranger_fixed_ref.py (fixed-shape mode).  A helper module: no test in here.

    block(x)  = LN_F(lrelu(LN_{F/2}(lrelu(x W1^T)) W2^T)),  lrelu(v) = v if v > 0 else slope * v,
    LN(v)     = (v - mean) / sqrt(var + eps) * w + b with the biased variance, as torch defines LayerNorm
    padded    = float64 [T, M, P, F]: slot before_i(t, p) + r, r < kept_i(t, p), holds block_i(row r of type i's block of obs[e, t, a]);
                +0.0 elsewhere.  kept / before are the plan's (arranger_ref.plan or arranger_fixed_ref.plan).
Held to a torch float64 twin, and to the reference's own EmbedBlock where it is present, by tests/test_arranger_embed_ref.py."""
import numpy as np

import arranger_fixed_ref as FR
import arranger_ref as R

PARAMS = ("Layer1.weight", "bn1.weight", "bn1.bias", "Layer2.weight", "bn2.weight", "bn2.bias")   # the reference's names, the C struct's order


def layer_norm(v, w, b, eps):
    mean = v.mean(-1, keepdims=True)
    var = ((v - mean) ** 2).mean(-1, keepdims=True)
    return (v - mean) / np.sqrt(var + eps) * w + b


def block(x, p, slope=0.1, eps=1e-5):
    """x [N, feat], p = the six arrays of PARAMS in that order -> float64 [N, F]"""
    w1, g1, b1, w2, g2, b2 = [np.asarray(a, np.float64) for a in p]
    h = np.asarray(x, np.float64) @ w1.T
    h = layer_norm(np.where(h > 0, h, slope * h), g1, b1, eps)
    y = h @ w2.T
    return layer_norm(np.where(y > 0, y, slope * y), g2, b2, eps)


def make_params(rng, feats, F):
    """per type the six float32 arrays: torch's default Linear init (uniform in +-1/sqrt(fan_in)), LayerNorm weights in [0.5, 1.5] and
    biases in [-0.5, 0.5]"""
    out = []
    for f in feats:
        u = lambda shape, lo, hi: rng.uniform(lo, hi, shape).astype(np.float32)
        out.append([u((F // 2, f), -f ** -0.5, f ** -0.5), u((F // 2,), 0.5, 1.5), u((F // 2,), -0.5, 0.5),
                    u((F, F // 2), -(F // 2) ** -0.5, (F // 2) ** -0.5), u((F,), 0.5, 1.5), u((F,), -0.5, 0.5)])
    return out


def padded_from_plan(obs, types, kept, before, M, params, F, slope=0.1, eps=1e-5):
    """kept, before int [n, T, P] -> float64 [T, M, P, F]; params[i] None: +0.0 in the type's slots"""
    E, T, A, _ = obs.shape
    P, TP = E * A, T * E * A
    out = np.zeros((T, int(M), P, F), np.float64)
    for i, ty in enumerate(types):
        f, cap = int(ty.feat), int(ty.cap)
        if cap == 0 or params[i] is None:
            continue
        blk = obs[..., int(ty.offset):int(ty.offset) + cap * f].reshape(E, T, A, cap, f).transpose(1, 0, 2, 3, 4).reshape(TP, cap, f)
        tp, r = np.nonzero(np.arange(cap)[None, :] < kept[i].reshape(TP)[:, None])
        if tp.size:
            out[tp // P, before[i].reshape(TP)[tp] + r, tp % P] = block(blk[tp, r], params[i], slope, eps)
    return out


def padded_default(obs, types, params, F, count_env=None, M=None):
    """the default mode: M = the batch's largest object count unless given (M above it: zero slots behind; below it: the counts are
    clamped to the slots left, earlier types winning, as the kernels clamp them).  -> (padded, plan)"""
    pl = R.plan(obs, types, count_env)
    if M is None or M >= pl["max_count"]:
        before = np.cumsum(pl["counts"], axis=0) - pl["counts"]
        return padded_from_plan(obs, types, pl["counts"], before, pl["max_count"] if M is None else M, params, F), pl
    fp = FR.plan_from_counts(pl["counts"], [int(t.cap) for t in types], M)
    return padded_from_plan(obs, types, fp["counts"], fp["before"], M, params, F), pl


def padded_fixed(obs, types, rows, M, params, F, count_env=None):
    """the fixed-shape mode -> (padded, plan of arranger_fixed_ref: counts = kept, dropped, obj_counts)"""
    pl = FR.plan(obs, types, rows, M, count_env)
    return padded_from_plan(obs, types, pl["counts"], pl["before"], M, params, F), pl
