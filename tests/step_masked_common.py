"""What only the masked step's tests need on top of tests/per_env_common.py (tests/test_gpu_step_masked.py; the exact transfer's tests
freeze environments with them too): the sentinels every output tensor is pre-filled with, the output triples as bit patterns, and the
random masks of the soak.  No test in here."""
import numpy as np

from per_env_common import SENTINEL, bits32, bits64

OBS_SENTINEL = SENTINEL               # int32 pattern of an observation word nobody wrote
REW_SENTINEL = 0x5EA71E555EA71E55     # int64 pattern of a reward nobody wrote
DONE_SENTINEL = 0xA5                  # a dones byte nobody wrote


def fill_sentinels(env):
    import torch
    env.obs.view(torch.int32).fill_(OBS_SENTINEL)
    env.rewards.view(torch.int64).fill_(REW_SENTINEL)
    env.dones.fill_(DONE_SENTINEL)


def outputs(env):
    """(obs as int32, rewards as int64, dones) on the host: bit patterns"""
    return bits32(env.obs), bits64(env.rewards), env.dones.cpu().numpy().copy()


def rows_are_sentinel(out, rows):
    o, r, d = out
    return bool((o[rows] == OBS_SENTINEL).all() and (r[rows] == REW_SENTINEL).all() and (d[rows] == DONE_SENTINEL).all())


def same_outputs(x, y, rows=None):
    """"" if the two (obs, rewards, dones) triples hold the same bits (in `rows`), else which of them differs"""
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    bad = [n for n, a, b in zip(("observations", "rewards", "dones"), x, y) if not np.array_equal(sel(a), sel(b))]
    return " and ".join(bad)


def mask_tensor(E, listed):
    import torch
    m = torch.zeros((E,), dtype=torch.bool, device="cuda")
    if len(listed):
        m[list(listed)] = True
    return m


def soak_masks(E, steps, seed):
    """step -> sorted listed environments: environment 0 always, 1 never, 2 (if there is one) at the even steps, the others with
    probability one half.  -> (masks, how often each environment is listed)"""
    rng = np.random.default_rng(seed)
    masks = []
    for s in range(steps):
        m = rng.random(E) < 0.5
        m[0] = True
        if E > 1:
            m[1] = False
        if E > 2:
            m[2] = s % 2 == 0
        masks.append([int(e) for e in np.nonzero(m)[0]])
    return masks, [sum(e in m for m in masks) for e in range(E)]


def soak_seed(E, steps):
    """the first seed with which every environment but 0 and 1 is listed at least once and frozen at least once (found on the host)"""
    for seed in range(100, 200):
        _, times = soak_masks(E, steps, seed)
        if all(0 < t < steps for t in times[2:]):
            return seed
    raise AssertionError("no seed in [100, 200) gives every environment both a listed and a frozen step")
