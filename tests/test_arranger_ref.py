"""The vectorised arranger reference (tests/arranger_ref.py, what the GPU shape tests compare the kernels with) against the
arranger oracle (oracle/arranger.py, pinned to the reference's own InOutArranger by tests/golden/arranger.npz), and the
transport's numpy index maps (dynenv_amd.distributed.pack_* / unpack_*) against their own inverses.  CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import arranger as oa  # noqa: E402
import arranger_ref as R  # noqa: E402
from dynenv_amd.distributed import PEER_COL_MAP, PEER_COLS, PEER_SELF, pack_peers_np, pack_tail_np, unpack_peers_np, unpack_tail_np  # noqa: E402


def _count_slow(obs_row, ty, count_env, e):
    """the contract of include/dynenv.h for one row, element by element"""
    if ty.count_mode == R.COUNT_CONST:
        c = ty.count_value
    elif ty.count_mode == R.COUNT_ENV:
        c = int(count_env.reshape(-1)[e * ty.count_stride + ty.count_index])
    else:
        c = int(float(obs_row[ty.count_index]))  # Python int(): truncation toward zero, as the C cast
    return min(max(c, 0), ty.cap)


def _ragged(obs, types, count_env):
    E, T, A, _ = obs.shape
    return [[[[obs[e, t, a, ty.offset:ty.offset + _count_slow(obs[e, t, a], ty, count_env, e) * ty.feat].reshape(-1, ty.feat)
               for ty in types] for a in range(A)] for t in range(T)] for e in range(E)]


def _random_specs(rng, k):
    n = 1 + k % 4                                   # 1-4 types, every count mode
    specs = []
    for i in range(n):
        cap = int(rng.choice([0, 1, 2, 3, 5, 9]))   # cap = 0: a type that never has a row
        mode = int((k // 4 + i) % 3)
        lo, hi = (-3, cap + 3) if rng.random() < 0.7 else (0, 0)  # below zero, above cap; or all empty
        specs.append((int(rng.integers(1, 6)), cap, mode, lo, hi))
    return specs


@pytest.mark.parametrize("seed", range(6))
def test_arranger_ref_matches_oracle_on_random_batches(seed):
    """50 random dense batches per seed (300 in all): counts, objCounts, maxCount, inputs per type, padded tensor and masks of
    tests/arranger_ref.py == oracle/arranger.py on the ragged form of the same observation"""
    rng = np.random.default_rng(100 + seed)
    seen = set()
    for k in range(50):
        E, T, A = int(rng.integers(1, 5)), int(rng.choice([1, 2, 5])), int(rng.integers(1, 7))
        specs = _random_specs(rng, 50 * seed + k)
        obs, types, count_env = R.make_dense(rng, E, T, A, specs, lead=int(rng.integers(0, 3)), trail=int(rng.integers(0, 3)))
        pl = R.plan(obs, types, count_env)
        inputs, slots, mask = R.gather(obs, types, pl)
        x = _ragged(obs, types, count_env)
        o_in, (o_counts, o_max, o_obj) = oa.rearrange_inputs(x, len(types), E * A, T)
        assert pl["max_count"] == o_max
        assert np.array_equal(pl["counts"], o_counts) and np.array_equal(pl["obj_counts"], o_obj)
        assert np.array_equal(pl["total"], o_counts.reshape(len(types), -1).sum(1))
        for i, ty in enumerate(types):
            assert np.array_equal(inputs[i], np.asarray(o_in[i], np.float32).reshape(-1, ty.feat)), (k, i)
            assert not np.any(inputs[i] == R.JUNK)
        F = int(rng.choice([1, 4, 6]))
        embs = [rng.standard_normal((len(s), F)).astype(np.float32) if len(s) else None for s in slots]
        if o_max == 0:
            assert mask.shape == (T, E * A, 0)
            continue
        o_pad, o_masks = oa.rearrange_outputs(embs, (o_counts, o_max, o_obj))
        assert np.array_equal(R.pad(embs, slots, T, o_max, E * A, F), o_pad), k
        assert np.array_equal(mask.astype(bool), np.stack(o_masks))
        seen |= {(ty.count_mode, ty.cap == 0, int(c.max()) == 0) for ty, c in zip(types, pl["counts"])}
        seen.add(("types", len(types)))
    assert {(m, False, False) for m in range(3)} <= seen and {("types", n) for n in range(1, 5)} <= seen
    assert any(s[1] for s in seen if s[0] != "types") and any(s[2] and not s[1] for s in seen if s[0] != "types")


def test_arranger_ref_truncates_and_clamps_row_counts():
    """COUNT_ROW: (int) truncates toward zero (2.9 -> 2, -0.5 -> 0), then [0, cap]"""
    obs = np.zeros((1, 1, 6, 4), np.float32)
    obs[0, 0, :, 3] = [2.9, -0.5, -3.2, 7.99, 3.0, 0.99]
    ty = R.Ty(0, 1, 3, R.COUNT_ROW, count_index=3)
    assert R.type_counts(obs, ty).tolist() == [[2, 0, 0, 3, 3, 0]]


def test_arranger_ref_slots_and_padding_by_hand():
    """two players, two types; player 0: 2 + 1 objects, player 1: 0 + 2 -> maxCount 3"""
    obs = np.zeros((1, 1, 2, 8), np.float32)
    obs[0, 0, 0, :3] = [10, 11, 99]
    obs[0, 0, 0, 3:5] = [20, 99]
    obs[0, 0, 1, 3:5] = [21, 22]
    obs[0, 0, :, 6] = [2, 0]
    obs[0, 0, :, 7] = [1, 2]
    types = [R.Ty(0, 1, 3, R.COUNT_ROW, count_index=6), R.Ty(3, 1, 2, R.COUNT_ROW, count_index=7)]
    pl = R.plan(obs, types)
    inputs, slots, mask = R.gather(obs, types, pl)
    assert pl["max_count"] == 3 and inputs[0].ravel().tolist() == [10, 11] and inputs[1].ravel().tolist() == [20, 21, 22]
    # slot = (t * maxCount + j) * P + p
    assert slots[0].tolist() == [0, 2] and slots[1].tolist() == [4, 1, 3]
    assert mask.tolist() == [[[0, 0, 0], [0, 0, 1]]]
    padded = R.pad(inputs, slots, 1, 3, 2, 1)
    assert padded[0, :, :, 0].tolist() == [[10, 21], [11, 22], [20, 0]]


# ---- transport index maps ----
def _shared_tail(rng, n, a, d, split):
    x = rng.standard_normal((n, a, d)).astype(np.float32)
    x[:, :, split:] = x[:, :1, split:]
    return x


@pytest.mark.parametrize("n, a, d, split", [(7, 3, 11, 0), (7, 3, 11, 11), (5, 1, 9, 4), (4, 10, 232, 72), (3, 4, 6, 6), (2, 1, 1, 0)])
def test_tail_pack_is_inverted_by_unpack(n, a, d, split):
    """unpack(pack(x)) == x where the tails are shared, pack(unpack(p)) == p for any p; split 0 (all tail), split D (no tail), A = 1"""
    rng = np.random.default_rng(n * 1000 + a * 10 + d)
    x = _shared_tail(rng, n, a, d, split)
    p = pack_tail_np(x, split)
    assert p.shape == (n, a * split + d - split)
    assert np.array_equal(unpack_tail_np(p, a, d, split), x)
    q = rng.standard_normal(p.shape).astype(np.float32)
    assert np.array_equal(pack_tail_np(unpack_tail_np(q, a, d, split), split), q)


def _peer_consistent(rng, n, a, tail):
    cars_end = PEER_SELF + (a - 1) * PEER_COLS
    selfb = rng.standard_normal((n, a, PEER_SELF)).astype(np.float32)
    t = rng.standard_normal((n, tail)).astype(np.float32)
    x = np.empty((n, a, cars_end + tail), np.float32)
    for i in range(a):
        x[:, i, :PEER_SELF] = selfb[:, i]
        others = [c for c in range(a) if c != i]
        for q, c in enumerate(others):
            x[:, i, PEER_SELF + q * PEER_COLS:PEER_SELF + (q + 1) * PEER_COLS] = selfb[:, c][:, list(PEER_COL_MAP)]
        x[:, i, cars_end:] = t
    return x


@pytest.mark.parametrize("a, tail", [(1, 0), (1, 5), (2, 0), (10, 160), (16, 160), (17, 3)])
def test_peer_pack_is_inverted_by_unpack(a, tail):
    """unpack_peers(pack_peers(x)) == x for a peer-consistent x (every car's columns in another row are its own self columns),
    pack_peers(unpack_peers(p)) == p for any p; A = 1 (no other car), tail 0"""
    rng = np.random.default_rng(a * 100 + tail)
    n = 5
    x = _peer_consistent(rng, n, a, tail)
    d = x.shape[2]
    p = pack_peers_np(x)
    assert p.shape == (n, a * PEER_SELF + tail)
    assert np.array_equal(unpack_peers_np(p, a, d), x)
    q = rng.standard_normal(p.shape).astype(np.float32)
    assert np.array_equal(pack_peers_np(unpack_peers_np(q, a, d)), q)
