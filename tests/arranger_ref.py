"""Vectorised numpy reference of the GPU arranger contract (include/dynenv.h, dynenv_arrange_*) over the DENSE observation tensor
obs [E, T, A, D].  No per-player Python loops, so it keeps up with production sizes (T*E*A ~ 1e5 players x time steps).

It restates what the kernels must compute, not how: per object type i (an object with the attributes of dynenv_arr_type_t:
offset, feat, cap, count_mode, count_value, count_index, count_stride)
    count_i(t, p)  = clamp(c, 0, cap_i),  c = count_value | count_env[e * count_stride + count_index] | trunc(obs[e, t, a, count_index])
    inputs[i]      = the first count_i rows of type i's block in every (t, p), in (t, p, k) order, p = e*A + a
    slots[i]       = (t * maxCount + sum_{i' < i} count_i'(t, p) + k) * P + p
    mask           = [T, P, maxCount] uint8, 1 where j >= objCounts(t, p)
    padded         = [T, maxCount, P, F], the embedding of the object that owns the slot, zero elsewhere.
Held to oracle/arranger.py (the reference's own InOutArranger, restated) by tests/test_arranger_ref.py."""
import numpy as np

COUNT_CONST, COUNT_ENV, COUNT_ROW = 0, 1, 2


def type_counts(obs, ty, count_env=None):
    """int64 [T, P] counts of one object type, clamped to [0, cap]"""
    E, T, A, _ = obs.shape
    if ty.count_mode == COUNT_CONST:
        c = np.full((T, E * A), int(ty.count_value), np.int64)
    elif ty.count_mode == COUNT_ENV:
        ce = np.asarray(count_env).reshape(-1).astype(np.int64)
        per_env = ce[np.arange(E) * int(ty.count_stride) + int(ty.count_index)]
        c = np.broadcast_to(np.repeat(per_env, A)[None, :], (T, E * A)).copy()
    elif ty.count_mode == COUNT_ROW:
        # (int) of a float: truncation toward zero
        c = np.trunc(obs[:, :, :, int(ty.count_index)].astype(np.float64)).astype(np.int64).transpose(1, 0, 2).reshape(T, E * A)
    else:
        raise ValueError("unknown count_mode %r" % ty.count_mode)
    return np.clip(c, 0, int(ty.cap))


def plan(obs, types, count_env=None):
    """-> dict(counts int64 [n, T, P], obj_counts [T, P], max_count, base [n, T, P] (exclusive prefix in (t, p) order), total [n])"""
    counts = np.stack([type_counts(obs, ty, count_env) for ty in types])
    obj_counts = counts.sum(0)
    flat = counts.reshape(len(types), -1)
    base = (np.cumsum(flat, axis=1) - flat).reshape(counts.shape)
    return dict(counts=counts, obj_counts=obj_counts, max_count=int(obj_counts.max()), base=base, total=flat.sum(1))


def gather(obs, types, pl):
    """-> (inputs [n] float32 [N_i, feat_i], slots [n] int64 [N_i], mask uint8 [T, P, maxCount])"""
    E, T, A, _ = obs.shape
    P, TP, M = E * A, T * E * A, pl["max_count"]
    counts = pl["counts"].reshape(len(types), TP)
    before = np.cumsum(counts, axis=0) - counts        # objects of the earlier types of the same (t, p)
    inputs, slots = [], []
    for i, ty in enumerate(types):
        f, cap, c = int(ty.feat), int(ty.cap), counts[i]
        if cap == 0:
            inputs.append(np.zeros((0, f), np.float32))
            slots.append(np.zeros((0,), np.int64))
            continue
        blk = obs[..., int(ty.offset):int(ty.offset) + cap * f].reshape(E, T, A, cap, f).transpose(1, 0, 2, 3, 4).reshape(TP, cap, f)
        take = np.arange(cap)[None, :] < c[:, None]
        inputs.append(np.ascontiguousarray(blk[take]))
        tp = np.repeat(np.arange(TP, dtype=np.int64), c)
        k = np.arange(tp.size, dtype=np.int64) - np.repeat(pl["base"].reshape(len(types), TP)[i], c)
        t, p = tp // P, tp % P
        slots.append((t * M + before[i][tp] + k) * P + p)
    mask = (np.arange(M)[None, None, :] >= pl["obj_counts"][:, :, None]).astype(np.uint8)
    return inputs, slots, mask


def pad(embs, slots, T, max_count, P, F):
    """padded [T, maxCount, P, F] float32: embs[i][n] at row slots[i][n] of the [T*maxCount*P, F] view, zeros elsewhere
    (embs[i] None: a type without objects)"""
    out = np.zeros((T * max_count * P, F), np.float32)
    for e, s in zip(embs, slots):
        if e is not None and len(s):
            out[s] = e
    return out.reshape(T, max_count, P, F)


# ---- synthetic inputs shared by the CPU cross-check and the GPU shape tests ----
class Ty(object):
    """an object type with the fields of dynenv_arr_type_t"""
    _fields = ("offset", "feat", "cap", "count_mode", "count_value", "count_index", "count_stride")

    def __init__(self, offset, feat, cap, count_mode=COUNT_CONST, count_value=0, count_index=0, count_stride=0):
        self.offset, self.feat, self.cap, self.count_mode = offset, feat, cap, count_mode
        self.count_value, self.count_index, self.count_stride = count_value, count_index, count_stride

    def astuple(self):
        return tuple(int(getattr(self, f)) for f in self._fields)


JUNK = np.float32(-12345.5)  # unused capacity: a read of it shows up in the output


def make_dense(rng, E, T, A, specs, lead=0, trail=0):
    """A dense [E, T, A, D] float32 observation and its types.  specs: (feat, cap, mode, lo, hi) per type; the raw count of
    every (e, t, a) (mode ROW), e (mode ENV) or the type (mode CONST) is drawn from [lo, hi], which may reach below 0 and above
    cap.  Layout: `lead` junk floats, the blocks of cap * feat floats, one count column per type (ROW: the raw count plus a
    fraction away from zero, so that only truncation recovers it), `trail` junk floats.  Valid rows hold random normals,
    everything else JUNK.  Returns (obs, types, count_env int32 [E, n])."""
    n = len(specs)
    offs = lead + np.concatenate([[0], np.cumsum([f * c for f, c, *_ in specs])]).astype(int)
    cnt_col = int(offs[-1])
    D = cnt_col + n + trail
    obs = np.full((E, T, A, D), JUNK, np.float32)
    count_env = rng.integers(-2, 3, (E, n)).astype(np.int32)
    types = []
    for i, (f, cap, mode, lo, hi) in enumerate(specs):
        if mode == COUNT_CONST:
            v = int(rng.integers(lo, hi + 1))
            raw = np.full((E, T, A), v, np.int64)
            types.append(Ty(int(offs[i]), f, cap, COUNT_CONST, count_value=v))
        elif mode == COUNT_ENV:
            count_env[:, i] = rng.integers(lo, hi + 1, E)
            raw = np.broadcast_to(count_env[:, i].astype(np.int64)[:, None, None], (E, T, A))
            types.append(Ty(int(offs[i]), f, cap, COUNT_ENV, count_index=i, count_stride=n))
        else:
            raw = rng.integers(lo, hi + 1, (E, T, A))
            frac = rng.random((E, T, A)).astype(np.float32) * np.float32(0.96)
            obs[..., cnt_col + i] = raw.astype(np.float32) + np.where(raw < 0, -frac, frac)
            types.append(Ty(int(offs[i]), f, cap, COUNT_ROW, count_index=cnt_col + i))
        if cap:
            c = np.clip(raw, 0, cap)
            blk = rng.standard_normal((E, T, A, cap, f)).astype(np.float32)
            blk[np.arange(cap)[None, None, None, :] >= c[..., None]] = JUNK
            obs[..., int(offs[i]):int(offs[i + 1])] = blk.reshape(E, T, A, cap * f)
    return obs, types, count_env
