"""numpy statement of the FIXED-shape arranger contract (include/dynenv.h, dynenv_arrange_fixed_*), built on arranger_ref.py (type_counts,
make_dense, Ty).  A helper module: no test in here.

The caller fixes rows[i] in 0..cap_i (rows of type i kept per (time, player)) and M >= 0 (slots of the padded tensor).  With
c_i(t, p) = arranger_ref.type_counts (the default mode's clamped count), p = e*A + a, tp = t*P + p:
    k_i(t, p)    = min(c_i, rows[i], M - sum_{i' < i} k_i')          kept; earlier types win
    dropped[i]   = sum_{t, p} (c_i - k_i)
    inputs[i]    = float32 [T*P*rows[i], feat_i]: row tp*rows[i] + r is the object's features for r < k_i, +0.0 behind
    mask         = uint8 [T, P, M], 1 where j >= sum_i k_i
    padded       = float32 [T, M, P, F]: slot j = sum_{i' < i} k_i' + r (r < k_i) holds emb_i[tp*rows[i] + r], +0.0 elsewhere
    grad_emb_i   = float32 [T*P*rows[i], F]: row tp*rows[i] + r is grad[t, j, p] for r < k_i, +0.0 behind
Held to arranger_ref / arranger_grad_ref, to the reference's recorded vectors and to a longhand loop by tests/test_arranger_fixed_ref.py."""
import numpy as np

import arranger_ref as R


def plan(obs, types, rows, M, count_env=None):
    """-> dict(c int64 [n, T, P] (clamped counts), counts [n, T, P] (kept), obj_counts [T, P], before [n, T, P] (kept of the earlier
    types), dropped int64 [n])"""
    c = np.stack([R.type_counts(obs, ty, count_env) for ty in types])
    return plan_from_counts(c, rows, M)


def plan_from_counts(c, rows, M):
    """the same from the clamped counts c [n, T, P] alone"""
    c = np.asarray(c, np.int64)
    k = np.zeros_like(c)
    before = np.zeros_like(c)
    total = np.zeros(c.shape[1:], np.int64)
    for i in range(c.shape[0]):
        before[i] = total
        k[i] = np.minimum(np.minimum(c[i], int(rows[i])), int(M) - total)
        total = total + k[i]
    return dict(c=c, counts=k, obj_counts=total, before=before, dropped=(c - k).reshape(c.shape[0], -1).sum(1))


def _kept(pl, i, rows):
    """(tp, r) of every kept row of type i, in (tp, r) order"""
    k = pl["counts"][i].reshape(-1)
    take = np.arange(int(rows[i]))[None, :] < k[:, None]
    return np.nonzero(take)


def gather(obs, types, rows, M, pl):
    """-> (inputs [n] float32 [T*P*rows_i, feat_i], mask uint8 [T, P, M])"""
    E, T, A, _ = obs.shape
    TP = T * E * A
    inputs = []
    for i, ty in enumerate(types):
        f, cap, n = int(ty.feat), int(ty.cap), int(rows[i])
        blk = obs[..., int(ty.offset):int(ty.offset) + cap * f].reshape(E, T, A, cap, f).transpose(1, 0, 2, 3, 4).reshape(TP, cap, f)[:, :n]
        take = np.arange(n)[None, :] < pl["counts"][i].reshape(TP)[:, None]
        inputs.append(np.where(take[:, :, None], blk, np.float32(0)).astype(np.float32).reshape(TP * n, f))
    mask = (np.arange(int(M))[None, None, :] >= pl["obj_counts"][:, :, None]).astype(np.uint8)
    return inputs, mask


def pad(embs, rows, M, pl, F):
    """padded float32 [T, M, P, F]; embs[i] float32 [T*P*rows_i, F] or None (zeros in its slots)"""
    n, T, P = pl["counts"].shape
    out = np.zeros((T, int(M), P, F), np.float32)
    for i in range(n):
        if embs[i] is None:
            continue
        tp, r = _kept(pl, i, rows)
        out[tp // P, pl["before"][i].reshape(-1)[tp] + r, tp % P] = embs[i][tp * int(rows[i]) + r]
    return out


def unpad(grad, rows, pl):
    """grad [T, M, P, F] -> per type float32 [T*P*rows_i, F], zero in the rows that were not kept"""
    n, T, P = pl["counts"].shape
    F = grad.shape[-1]
    out = []
    for i in range(n):
        g = np.zeros((T * P * int(rows[i]), F), np.float32)
        tp, r = _kept(pl, i, rows)
        g[tp * int(rows[i]) + r] = grad[tp // P, pl["before"][i].reshape(-1)[tp] + r, tp % P]
        out.append(g)
    return out


def kept_rows(x, rows_i, k):
    """the kept rows of a capacity tensor x [T*P*rows_i, W], compacted in (t, p, r) order - the default mode's layout; k: kept [T, P]"""
    take = np.arange(int(rows_i))[None, :] < np.asarray(k).reshape(-1)[:, None]
    return x.reshape(take.shape[0], int(rows_i), x.shape[1])[take]
