"""The backward of the curiosity losses as a numpy float64 statement (a helper module: no tests in it): the formulas of
dynenv_icm_backward (include/dynenv.h) over icm_ref's rows and indices - the gradients of s_f * forward_mean + s_i * inverse_mean with
respect to every pred_net parameter and to the features - and their packing into the seven layouts of dynenv_icm_grad_t."""
import collections

import numpy as np

import icm_ref as IR

HIDDEN, HIDDEN_PAD, ROWS = IR.HIDDEN, 160, 32
FWD = "pred_net.fwd_net."
INV = "pred_net.inv_net.blocks.0.Layer.%d"


def names(groups):
    """the parameters the backward covers, in state_dict order"""
    out = [FWD + "fc1.weight", FWD + "fc1.bias", FWD + "fc2.weight", FWD + "fc2.bias"]
    for g in range(len(groups)):
        out += [INV % g + ".weight", INV % g + ".bias"]
    return out


def grads(features, actions, finished, pr, groups, s_f=1.0, s_i=1.0, slope=IR.SLOPE):
    """-> OrderedDict name -> gradient (every name of names(groups), then "features"), float64; finished None: nobody finished"""
    f = features.astype(np.float64)
    T, P, K = f.shape[0] - 1, f.shape[1], f.shape[2]
    G = len(groups)
    w = {k: v.astype(np.float64) for k, v in pr.items()}
    cur, nxt = f[:-1], f[1:]
    idx, _ = IR.indices(actions, groups)
    oh = IR.one_hot(idx, groups)
    mask = np.ones((T, P), bool) if finished is None else ~np.asarray(finished, bool)
    n = int(mask.sum())
    out = collections.OrderedDict((k, np.zeros(w[k].shape)) for k in names(groups))
    out["features"] = np.zeros(f.shape)
    if n == 0:
        return out
    alpha, beta = 2.0 * s_f / (n * K), s_i / (n * G)
    W1, W2 = w[FWD + "fc1.weight"], w[FWD + "fc2.weight"]
    x = np.concatenate([cur, oh], 2)
    h_pre = x @ W1.T + w[FWD + "fc1.bias"]
    h = np.where(h_pre > 0, h_pre, h_pre * slope)
    pred = h @ W2.T + w[FWD + "fc2.bias"]
    m = mask[..., None]
    e = np.where(m, pred - nxt, 0.0)
    if slope == IR.SLOPE:   # (icm_ref.rows is the same forward)
        assert np.allclose((pred - nxt) ** 2, IR.rows(features, actions, pr, groups)[2], rtol=1e-12, atol=1e-300)
    dh = (e @ W2) * np.where(h_pre > 0, 1.0, slope)
    out[FWD + "fc2.weight"] = alpha * np.einsum("tpk,tph->kh", e, h)
    out[FWD + "fc2.bias"] = alpha * e.sum((0, 1))
    out[FWD + "fc1.weight"] = alpha * np.einsum("tph,tpc->hc", dh, x)   # (the one-hot columns: the scatter-add)
    out[FWD + "fc1.bias"] = alpha * dh.sum((0, 1))
    xx = np.concatenate([cur, nxt], 2)
    dcat = np.zeros((T, P, 2 * K))
    for g in range(G):
        name = INV % g
        l = xx @ w[name + ".weight"].T + w[name + ".bias"]
        q = IR._softmax(l)
        np.put_along_axis(q, idx[:, g][..., None], np.take_along_axis(q, idx[:, g][..., None], 2) - 1.0, axis=2)
        q = np.where(m, q, 0.0)
        if groups[g] == 1:
            assert not q.any()
        out[name + ".weight"] = beta * np.einsum("tpn,tpc->nc", q, xx)
        out[name + ".bias"] = beta * q.sum((0, 1))
        dcat += beta * (q @ w[name + ".weight"])
    df = out["features"]
    df[:-1] += alpha * (dh @ W1[:, :K]) + dcat[..., :K]
    df[1:] += -alpha * e + dcat[..., K:]
    return out


def pack(g, K, groups):
    """the gradients in the layouts of dynenv_icm_grad_t -> dict(w1 [160][K], act [N][160], b1 [160], w2 [K][160], b2 [K], inv_w [32][2K],
    inv_b [32]), the padding zero"""
    N, G = sum(groups), len(groups)
    out = dict(w1=np.zeros((HIDDEN_PAD, K)), act=np.zeros((N, HIDDEN_PAD)), b1=np.zeros(HIDDEN_PAD), w2=np.zeros((K, HIDDEN_PAD)), b2=g[FWD + "fc2.bias"].copy(),
               inv_w=np.zeros((ROWS, 2 * K)), inv_b=np.zeros(ROWS))
    out["w1"][:HIDDEN] = g[FWD + "fc1.weight"][:, :K]
    out["act"][:, :HIDDEN] = g[FWD + "fc1.weight"][:, K:].T
    out["b1"][:HIDDEN] = g[FWD + "fc1.bias"]
    out["w2"][:, :HIDDEN] = g[FWD + "fc2.weight"]
    out["inv_w"][:N] = np.concatenate([g[INV % i + ".weight"] for i in range(G)])
    out["inv_b"][:N] = np.concatenate([g[INV % i + ".bias"] for i in range(G)])
    return out


PACKED = ("w1", "act", "b1", "w2", "b2", "inv_w", "inv_b")
