"""numpy restatement of the arranger's BACKWARD and the reference's recorded gradients (tests/golden/arranger_grad.npz, written by
tests/golden/gen_golden_arranger_grad.py from autograd through the reference's InOutArranger.rearrange_outputs).  A helper module:
no test in here.

The forward (arranger_ref.pad) places embedding row n of type i at row slots[i][n] of the padded tensor viewed as [T*maxCount*P, F]
and zeros elsewhere; every slot is owned by at most one row.  Its adjoint therefore reads, for every embedding row, the upstream
gradient's row at that slot: nothing is summed, padding slots are not read."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "arranger_grad.npz")

G = np.load(GOLDEN)
CASES = sorted({k.split("/")[0] for k in G.files})


def unpad(grad, slots):
    """grad [T, maxCount, P, F] -> per type float32 [N_i, F]: row slots[i][n] of the [T*maxCount*P, F] view"""
    F = grad.shape[-1]
    flat = np.ascontiguousarray(grad, np.float32).reshape(-1, F)
    return [flat[np.asarray(s, np.int64)] if len(s) else np.zeros((0, F), np.float32) for s in slots]


def plan_from_counts(counts):
    """counts [n, T, P] -> the dict arranger_ref.plan returns (counts, obj_counts, max_count, base, total), its arithmetic"""
    counts = np.asarray(counts, np.int64)
    obj_counts = counts.sum(0)
    flat = counts.reshape(counts.shape[0], -1)
    base = (np.cumsum(flat, axis=1) - flat).reshape(counts.shape)
    return dict(counts=counts, obj_counts=obj_counts, max_count=int(obj_counts.max()), base=base, total=flat.sum(1))


def slots_from_plan(pl):
    """the slots arranger_ref.gather computes, from the plan alone: (t * maxCount + sum_{i' < i} count_i'(t, p) + k) * P + p"""
    n, T, P = pl["counts"].shape
    TP, M = T * P, pl["max_count"]
    counts = pl["counts"].reshape(n, TP)
    before = np.cumsum(counts, axis=0) - counts
    slots = []
    for i in range(n):
        c = counts[i]
        tp = np.repeat(np.arange(TP, dtype=np.int64), c)
        k = np.arange(tp.size, dtype=np.int64) - np.repeat(pl["base"].reshape(n, TP)[i], c)
        t, p = tp // P, tp % P
        slots.append((t * M + before[i][tp] + k) * P + p)
    return slots


def golden_case(name):
    """-> dict(E, T, A, nT, F, P, plan, slots, has_emb, embs, grads, G, padded) of one recorded case; embs[i] / grads[i] are None where
    the reference was given None (a type without objects)"""
    E, T, A, nT, F = (int(v) for v in G[name + "/shape"])
    pl = plan_from_counts(G[name + "/counts"])
    assert pl["max_count"] == int(G[name + "/maxCount"])
    has = [bool(h) for h in G[name + "/has_emb"]]
    embs = [G["%s/emb%d" % (name, i)] if has[i] else None for i in range(nT)]
    grads = [G["%s/grad%d" % (name, i)] if has[i] else None for i in range(nT)]
    return dict(E=E, T=T, A=A, nT=nT, F=F, P=E * A, plan=pl, slots=slots_from_plan(pl), has_emb=has, embs=embs, grads=grads,
                G=G[name + "/G"], padded=G[name + "/padded"])
