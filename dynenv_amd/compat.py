"""The reference-compatible (legacy) forms of a step's results, built on the host from the dense tensors: the ragged object
array obs[E, T, A, 3] (`CompatBuilder`, over the row description of obs_layout.row_groups), and the lazy containers that put off
that work - and the device->host copy behind it - until a consumer looks (`LazyObsArray`, `LazyInfos`, `LazyInfo`)."""
import gc
import itertools

import numpy as np

from ._capi import ARR_COUNT_CONST, ARR_COUNT_ENV


def _to_host(t):
    """Device tensor -> numpy through a PINNED staging tensor: torch's caching host allocator hands the block of the previous
    step back (no 38 MB of fresh page faults per step, ~20 ms at 4096 envs) and the copy runs at PCIe speed.  The numpy array
    keeps the tensor alive; every step gets its own block, as the reference returns fresh arrays."""
    import torch
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    return h.numpy()


class CompatBuilder(object):
    """Builds elements of the reference's observation array from dense rows: element [e, t, a] is [movable-object arrays,
    static / self arrays, seen info] - Driving ((cars, obstacles, peds), (self, lanes), (1, 1, 1)), RoboCup ((ball, robots), (self,),
    (1, 1, 1)), RoboCup Partial ((balls, robots), (goals, crosses, line crosses, lines), (numLandMarks, robotsSeen, ballsSeen)).
    The arrays are views into the dense host copy `o` [E, T, A, D]; `counts` [E, 2] are the per-environment row counts."""

    def __init__(self, groups):
        self.movable, self.static, self.seen = groups["movable"], groups["static"], groups["seen"]

    def element(self, o, counts, e, t, a):
        """One element [e, t, a] (the same views / values `array` assembles for the whole batch)."""
        r = o[e, t, a]

        def rows(ty):
            off, feat, cap, mode, value, index, stride = ty
            n = value if mode == ARR_COUNT_CONST else int(counts[e, index]) if mode == ARR_COUNT_ENV else int(r[index])
            return r[off:off + n * feat].reshape(n, feat)
        seen = (1, 1, 1)
        if self.seen is not None:
            landmarks, balls, lo, n = self.seen
            seen = (int(r[landmarks]), r[lo:lo + n].astype("uint8"), bool(r[balls]))
        return [[rows(ty) for ty in self.movable], [rows(ty) for ty in self.static], seen]

    def array(self, o, counts):
        """The whole object ndarray [E, T, A, 3] without a Python-level loop over (env, time, agent): the per-agent arrays of a type
        are made by iterating the type's block once in C (`np.fromiter(iter(block), object)`: one view per row), ragged blocks grouped
        by their row count, and the reference's nested lists by `zip`.  ~1 us per agent (five ndarray objects and two lists per
        agent remain - the reference's format)."""
        if not isinstance(o, np.ndarray):
            o = _to_host(o.detach())
        gc_was_on = gc.isenabled()
        gc.disable()  # ~8 N container objects are about to be allocated: every 700th would trigger a collection pass over them
        try:
            return self._array(o, counts)
        finally:
            if gc_was_on:
                gc.enable()

    def _array(self, o, counts):
        E, T, A, D = o.shape
        N = E * T * A
        flat = o.reshape(N, D)

        def views(ty):
            off, feat, cap, mode, value, index, stride = ty
            block = flat[:, off:off + cap * feat].reshape(N, cap, feat)
            if mode == ARR_COUNT_CONST:
                return np.fromiter(iter(block[:, :value]), dtype=object, count=N)
            if mode == ARR_COUNT_ENV:
                lens = np.repeat(np.asarray(counts)[:, index].astype(np.int64), T * A)
            else:
                lens = flat[:, index].astype(np.int64)
            res = np.empty(N, dtype=object)
            for n in np.unique(lens):
                pos = np.nonzero(lens == n)[0]
                res[pos] = np.fromiter(iter(block[pos, :int(n)]), dtype=object, count=len(pos))
            return res

        def lists(types):
            return np.fromiter(map(list, zip(*[views(ty) for ty in types])), dtype=object, count=N)
        out = np.empty((N, 3), dtype=object)
        out[:, 0] = lists(self.movable)
        out[:, 1] = lists(self.static)
        if self.seen is None:
            out[:, 2] = np.fromiter(itertools.repeat((1, 1, 1), N), dtype=object, count=N)
        else:
            landmarks, balls, lo, n = self.seen
            robots = np.fromiter(iter(flat[:, lo:lo + n].astype("uint8")), dtype=object, count=N)
            out[:, 2] = np.fromiter(zip(flat[:, landmarks].astype(np.int64).tolist(), robots, (flat[:, balls] != 0).tolist()),
                                    dtype=object, count=N)
        return out.reshape(E, T, A, 3)


class LazyInfo(dict):
    """The per-environment `info` dict of the reference (subproc_vec_env.py:17-23, DrivingEnvironment.py:306-316) whose two
    expensive entries - 'Full State' and 'Recon States', lists of per-agent arrays - are built from the step's single
    host copy of the observations only when somebody reads them.  Everything else of the dict protocol
    behaves as if they had been there all along."""
    LAZY = ("Full State", "Recon States")

    def __init__(self, make, eager=None):
        dict.__init__(self, eager or {})
        self._make = make

    def _materialise(self):
        if self._make is not None:
            full, recon = self._make()
            self._make = None
            dict.__setitem__(self, "Full State", full)
            dict.__setitem__(self, "Recon States", recon)

    def __missing__(self, key):
        if key in self.LAZY and self._make is not None:
            self._materialise()
            return dict.__getitem__(self, key)
        raise KeyError(key)

    def get(self, key, default=None):
        if key in self.LAZY:
            self._materialise()
        return dict.get(self, key, default)

    def __contains__(self, key):
        return key in self.LAZY or dict.__contains__(self, key)

    def __iter__(self):
        self._materialise()
        return dict.__iter__(self)

    def __len__(self):
        self._materialise()
        return dict.__len__(self)

    def keys(self):
        self._materialise()
        return dict.keys(self)

    def items(self):
        self._materialise()
        return dict.items(self)

    def values(self):
        self._materialise()
        return dict.values(self)

    def __repr__(self):
        self._materialise()
        return dict.__repr__(self)


class LazyObsArray(object):
    """The reference's observation `np.ndarray(dtype=object)` of shape [E, T, A, 3] (subproc_vec_env.py:201 over
    DrivingEnvironment.py:123 / RoboCupEnvironment.py:442) without the E*T*A Python objects: it keeps the step's dense host
    copy [E, T, A, D] and builds an element - `(movable-object arrays, static/self arrays, seen info)` - when it is indexed.
    Indexing follows numpy's basic rules (ints, slices, Ellipsis); a sub-array is again lazy (`obs[..., :-1]`,
    `obs[..., -1]` as models/train.py:67-68 does); `np.asarray(obs)` / `obs.materialize()` gives the reference's eager object array."""
    dtype = np.dtype(object)

    def __init__(self, builder, dense, counts, sel=None, box=None):
        # `builder`: what makes one element / the whole array from the dense copy (CompatBuilder's `element` and `array`);
        # `dense`: the step's observations [E, T, A, D] - a numpy array, or a device tensor (a snapshot the step made in HBM)
        # that is copied to the host the first time an element is looked at; `box` shares that copy among sub-arrays
        self._builder, self._counts = builder, counts
        self._box = box if box is not None else [dense]
        E, T, A, _ = dense.shape
        self._sel = sel if sel is not None else (range(E), range(T), range(A), range(3))  # per axis: range (kept) or int (dropped)

    @property
    def _dense(self):
        d = self._box[0]
        if not isinstance(d, np.ndarray):
            d = self._box[0] = _to_host(d)
        return d

    @property
    def shape(self):
        return tuple(len(s) for s in self._sel if not isinstance(s, int))

    @property
    def ndim(self):
        return len(self.shape)

    def __len__(self):
        sh = self.shape
        if not sh:
            raise TypeError("len() of unsized object")
        return sh[0]

    def _element(self, e, t, a, k):
        return self._builder.element(self._dense, self._counts, e, t, a)[k]

    def __getitem__(self, idx):
        if not isinstance(idx, tuple):
            idx = (idx,)
        kept = [i for i, s in enumerate(self._sel) if not isinstance(s, int)]
        if any(i is Ellipsis for i in idx):
            p = [i for i, x in enumerate(idx) if x is Ellipsis][0]
            idx = idx[:p] + (slice(None),) * (len(kept) - (len(idx) - 1)) + idx[p + 1:]
        if len(idx) > len(kept):
            raise IndexError("too many indices for array")
        idx = idx + (slice(None),) * (len(kept) - len(idx))
        sel = list(self._sel)
        for ax, i in zip(kept, idx):
            r = sel[ax]
            if isinstance(i, slice):
                sel[ax] = r[i]
            else:
                sel[ax] = r[int(i)]   # IndexError like numpy when out of range
        if all(isinstance(x, int) for x in sel):
            return self._element(*sel)
        return LazyObsArray(self._builder, self._box[0], self._counts, tuple(sel), self._box)

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def materialize(self):
        """The eager object ndarray of this (sub-)array, element for element what the reference returns."""
        E, T, A, _ = self._dense.shape
        if all(isinstance(x, range) and x == range(n) for x, n in zip(self._sel, (E, T, A, 3))):
            return self._builder.array(self._dense, self._counts)  # the whole array: the bulk builder
        axes = [([s] if isinstance(s, int) else list(s)) for s in self._sel]
        out = np.empty(tuple(len(a) for a in axes), dtype=object)
        for ie, e in enumerate(axes[0]):
            for it, t in enumerate(axes[1]):
                for ia, a in enumerate(axes[2]):
                    el = self._builder.element(self._dense, self._counts, e, t, a)
                    for ik, k in enumerate(axes[3]):
                        out[ie, it, ia, ik] = el[k]
        return out.reshape(self.shape)

    def __array__(self, dtype=None, copy=None):
        return self.materialize()

    def tolist(self):
        return self.materialize().tolist()

    def __repr__(self):
        return "LazyObsArray(shape=%r, dtype=object)" % (self.shape,)


class LazyInfos(object):
    """The per-environment `info` dicts of one step as a read-only sequence (the reference returns a tuple of dicts,
    subproc_vec_env.py:109-111): a dict is built when it is asked for and kept, so a consumer that never looks at
    `info` pays nothing for 4096 of them."""

    def __init__(self, n, make):
        self._n, self._make, self._cache = n, make, {}

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return tuple(self[k] for k in range(*i.indices(self._n)))
        i = int(i)
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        d = self._cache.get(i)
        if d is None:
            d = self._cache[i] = self._make(i)
        return d

    def __iter__(self):
        return (self[i] for i in range(self._n))
