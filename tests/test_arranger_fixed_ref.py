"""The numpy statement of the fixed-shape arranger (tests/arranger_fixed_ref.py), no device:
  - where nothing is dropped it IS the default mode (arranger_ref.plan / gather / pad, arranger_grad_ref.unpad) in the leading maxCount
    slots, zero / 1 behind them - on random dense batches and on every recorded case of the reference's own InOutArranger
    (tests/golden/arranger.npz, arranger_grad.npz);
  - the drop rule against a per-player loop written out longhand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_ref as R  # noqa: E402
import arranger_grad_ref as GR  # noqa: E402
import arranger_fixed_ref as FR  # noqa: E402
from arranger_golden import CASES, G, ragged_from_golden  # noqa: E402
from test_gpu_arranger import dense_from_ragged  # noqa: E402  (the dense row the GPU golden test packs the recorded ragged input into)

SPECS = [(3, 5, R.COUNT_ROW, -2, 7), (2, 7, R.COUNT_ENV, -1, 9), (4, 1, R.COUNT_CONST, 1, 1), (2, 0, R.COUNT_CONST, 3, 3)]
JUNK = np.float32(-777.25)   # in the capacity rows of an embedding that no object owns: must not reach the padded tensor


def _cap_embeddings(rng, pl, rows, F):
    """random embeddings at capacity [T*P*rows_i, F] with JUNK in the rows that are not kept, and their kept rows compacted"""
    n, T, P = pl["counts"].shape
    cap, compact = [], []
    for i in range(n):
        e = np.full((T * P * rows[i], F), JUNK, np.float32)
        tp, r = FR._kept(pl, i, rows)
        e[tp * rows[i] + r] = rng.standard_normal((len(tp), F)).astype(np.float32)
        cap.append(e)
        compact.append(FR.kept_rows(e, rows[i], pl["counts"][i]))
    return cap, compact


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("seed, extra", [(0, 0), (1, 3), (2, 0), (3, 1)])
def test_without_drops_it_is_the_default_mode(seed, extra):
    """rows = caps, M = the batch's maxCount + extra: leading slots bit for bit, zero / 1 behind, gradients of the kept rows"""
    rng = np.random.default_rng(seed)
    E, T, A, F = 5 + seed, 1 + seed % 3, 2, 8
    obs, types, ce = R.make_dense(rng, E, T, A, SPECS, lead=seed, trail=1)
    dpl = R.plan(obs, types, ce)
    d_inputs, d_slots, d_mask = R.gather(obs, types, dpl)
    rows = [int(t.cap) for t in types]
    M0 = dpl["max_count"]
    M = M0 + extra
    P = E * A
    pl = FR.plan(obs, types, rows, M, ce)
    assert np.array_equal(pl["counts"], dpl["counts"]) and np.array_equal(pl["obj_counts"], dpl["obj_counts"])
    assert not pl["dropped"].any()
    inputs, mask = FR.gather(obs, types, rows, M, pl)
    for i in range(len(types)):
        assert inputs[i].shape == (T * P * rows[i], types[i].feat)
        assert _same_bits(FR.kept_rows(inputs[i], rows[i], pl["counts"][i]), d_inputs[i]), "kept rows of type %d" % i
        assert not (inputs[i] == R.JUNK).any(), "unused capacity of an observation row was read"
        rest = np.ones(len(inputs[i]), bool)
        tp, r = FR._kept(pl, i, rows)
        rest[tp * rows[i] + r] = False
        assert not inputs[i][rest].view(np.uint32).any(), "+0.0 exactly behind the kept rows"
    assert _same_bits(np.ascontiguousarray(mask[..., :M0]), d_mask) and (mask[..., M0:] == 1).all()
    cap, compact = _cap_embeddings(rng, pl, rows, F)
    padded = FR.pad(cap, rows, M, pl, F)
    assert _same_bits(np.ascontiguousarray(padded[:, :M0]), R.pad(compact, d_slots, T, M0, P, F))
    assert not padded[:, M0:].view(np.uint32).any()
    # backward: NaN in every slot behind maxCount and in every padding slot must not be read
    up = rng.standard_normal((T, M, P, F)).astype(np.float32)
    up[mask.transpose(0, 2, 1).astype(bool)] = np.nan
    grads = FR.unpad(up, rows, pl)
    d_grads = GR.unpad(np.ascontiguousarray(up[:, :M0]), d_slots)
    for i in range(len(types)):
        assert np.isfinite(grads[i]).all()
        assert _same_bits(FR.kept_rows(grads[i], rows[i], pl["counts"][i]), d_grads[i]), "gradient of type %d" % i
        assert int(np.count_nonzero(grads[i].view(np.uint32).any(axis=1))) <= int(pl["counts"][i].sum())
    # a type whose embedding is None leaves zeros in its slots
    none0 = FR.pad([None] + cap[1:], rows, M, pl, F)
    own0 = (np.arange(M)[None, :, None] < pl["counts"][0][:, None, :])
    assert not none0[own0].view(np.uint32).any() and _same_bits(none0[~own0], padded[~own0])


@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("name", CASES)
def test_reference_vectors_forward(name, extra):
    """tests/golden/arranger.npz: with rows = caps and M >= the case's maxCount the fixed statement reproduces the reference's inputs,
    padded tensor and masks in the leading slots"""
    x, (E, T, A, nT) = ragged_from_golden(name)
    feats = [int(f) for f in G[name + "/feats"]]
    caps = [int(G[name + "/x_counts"][..., i].max()) + 1 for i in range(nT)]
    o, offs, D = dense_from_ragged(x, feats, caps)
    types = [R.Ty(int(offs[i]), feats[i], caps[i], R.COUNT_ROW, count_index=D - nT + i) for i in range(nT)]
    M0 = int(G[name + "/maxCount"])
    M, P = M0 + extra, E * A
    pl = FR.plan(o, types, caps, M)
    assert np.array_equal(pl["counts"], G[name + "/counts"]) and np.array_equal(pl["obj_counts"], G[name + "/objCounts"])
    assert not pl["dropped"].any()
    inputs, mask = FR.gather(o, types, caps, M, pl)
    embs = []
    for i in range(nT):
        kept = FR.kept_rows(inputs[i], caps[i], pl["counts"][i])
        assert np.array_equal(kept, G["%s/inputs%d" % (name, i)]), "inputs of type %d" % i
        # the generator's linear "embedding", applied to the capacity rows (a zero row maps to zero: replaced by JUNK, it must not be used)
        e = (inputs[i] @ G["%s/W%d" % (name, i)]).astype(np.float32)
        tp, r = FR._kept(pl, i, caps)
        rest = np.ones(len(e), bool)
        rest[tp * caps[i] + r] = False
        e[rest] = JUNK
        embs.append(e)
    want = G[name + "/padded"]
    padded = FR.pad(embs, caps, M, pl, want.shape[-1])
    assert np.array_equal(padded[:, :M0], want) and not padded[:, M0:].view(np.uint32).any()
    assert np.array_equal(mask.astype(bool)[..., :M0], G[name + "/masks"].astype(bool)) and (mask[..., M0:] == 1).all()


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("name", GR.CASES)
def test_reference_vectors_backward(name, extra):
    """tests/golden/arranger_grad.npz: the recorded embeddings at capacity give the recorded padded tensor, the recorded upstream
    gradient (NaN appended behind maxCount) gives the recorded gradients in the kept rows and zero in the others"""
    c = GR.golden_case(name)
    counts, T, P, F, M0 = c["plan"]["counts"], c["T"], c["P"], c["F"], c["plan"]["max_count"]
    rows = [int(counts[i].max()) for i in range(c["nT"])]
    M = M0 + extra
    pl = FR.plan_from_counts(counts, rows, M)
    assert np.array_equal(pl["counts"], counts) and not pl["dropped"].any()
    cap = []
    for i in range(c["nT"]):
        e = np.full((T * P * rows[i], F), JUNK, np.float32)
        tp, r = FR._kept(pl, i, rows)
        if c["has_emb"][i]:
            e[tp * rows[i] + r] = c["embs"][i]
        else:
            assert len(tp) == 0
        cap.append(e)
    padded = FR.pad(cap, rows, M, pl, F)
    assert padded[:, :M0].tobytes() == c["padded"].tobytes() and not padded[:, M0:].view(np.uint32).any()
    up = np.concatenate([c["G"], np.full((T, extra, P, F), np.nan, np.float32)], axis=1)
    grads = FR.unpad(up, rows, pl)
    for i in range(c["nT"]):
        kept = FR.kept_rows(grads[i], rows[i], counts[i])
        if c["has_emb"][i]:
            assert kept.tobytes() == c["grads"][i].tobytes(), "gradient of type %d" % i
        tp, r = FR._kept(pl, i, rows)
        rest = np.ones(len(grads[i]), bool)
        rest[tp * rows[i] + r] = False
        assert not grads[i][rest].view(np.uint32).any()


# ---- the drop rule, longhand ----
def _longhand(c, rows, M):
    """per (t, p), type after type: what is kept, what is dropped"""
    n, T, P = c.shape
    k = np.zeros_like(c)
    dropped = [0] * n
    for t in range(T):
        for p in range(P):
            used = 0
            for i in range(n):
                keep = int(c[i, t, p])
                if keep > rows[i]:
                    keep = rows[i]
                if keep > M - used:
                    keep = M - used
                k[i, t, p] = keep
                used += keep
                dropped[i] += int(c[i, t, p]) - keep
    return k, dropped


@pytest.mark.parametrize("what, rows, M", [
    ("rows below the counts", [2, 3, 1, 0], 13),
    ("M below the sum: earlier types win", [5, 7, 1, 0], 5),
    ("both", [3, 4, 0, 0], 4),
    ("M = 1", [5, 7, 1, 0], 1),
    ("M = 0", [5, 7, 1, 0], 0),
    ("rows all zero", [0, 0, 0, 0], 5),
])
def test_the_drop_rule(what, rows, M):
    rng = np.random.default_rng(11)
    E, T, A, F = 7, 2, 3, 4
    obs, types, ce = R.make_dense(rng, E, T, A, SPECS)
    P = E * A
    pl = FR.plan(obs, types, rows, M, ce)
    c = np.stack([R.type_counts(obs, ty, ce) for ty in types])
    k, dropped = _longhand(c, rows, M)
    assert np.array_equal(pl["counts"], k), what
    assert list(pl["dropped"]) == dropped, what
    assert np.array_equal(pl["obj_counts"], k.sum(0)) and int(pl["obj_counts"].max(initial=0)) <= M
    if what != "rows all zero" and M:
        assert sum(dropped) > 0, "the case drops something"
    if what.startswith("M below"):
        # a player whose first type alone fills M keeps nothing of the later ones
        full = k[0] == M
        assert full.any() and not k[1:, full].any()
    inputs, mask = FR.gather(obs, types, rows, M, pl)
    cap, _ = _cap_embeddings(rng, pl, rows, F)
    padded = FR.pad(cap, rows, M, pl, F)
    up = rng.standard_normal((T, M, P, F)).astype(np.float32)
    grads = FR.unpad(up, rows, pl)
    assert mask.shape == (T, P, M) and padded.shape == (T, M, P, F)
    for t in range(T):
        for p in range(P):
            j = 0
            e, a = divmod(p, A)
            for i, ty in enumerate(types):
                for r in range(rows[i]):
                    n = (t * P + p) * rows[i] + r
                    if r < k[i, t, p]:
                        src = obs[e, t, a, ty.offset + r * ty.feat: ty.offset + (r + 1) * ty.feat]
                        assert np.array_equal(inputs[i][n], src)
                        assert np.array_equal(padded[t, j, p], cap[i][n]) and np.array_equal(grads[i][n], up[t, j, p])
                        assert mask[t, p, j] == 0
                        j += 1
                    else:
                        assert not inputs[i][n].view(np.uint32).any() and not grads[i][n].view(np.uint32).any()
            assert j == pl["obj_counts"][t, p]
            assert (mask[t, p, j:] == 1).all() and not padded[t, j:, p].view(np.uint32).any()
