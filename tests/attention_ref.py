"""The numpy float64 statement of the attention layer (include/dynenv.h, dynenv_attend_pool; the reference's RecurrentTemporalAttention,
DynEnv/models/models.py:311-386) that the tests compare against, and the parameters and counts they share.  A helper module: no tests.

For player p: c_t its count at time t clamped to 0..M, n = max_t c_t, X_t its slots with every slot at or behind c_t taken as zero.
  mha(w; Qin, KVin, k): q = Qin Wq^T + bq; K = KVin[:k] Wk^T + bk and the row bias_k; V likewise with bias_v;
                        softmax(q K^T / sqrt(F)) over the k + 1 keys; (probs V) Wo^T + bo
  att_t = mha(objAtt; X_t[:n], X_t, c_t); fin = att_0, k = c_0; t = 1..T-1: fin = LayerNorm(mha(tempAtt; att_t, fin, k)), k = max(k, c_t)
  out[p] = sum_{r<n} sigmoid(fin_r conf_w + conf_b) fin_r / n, zero where n == 0"""
import numpy as np

MHA = ("in_proj_weight", "in_proj_bias", "bias_k", "bias_v", "out_proj.weight", "out_proj.bias")
NAMES = tuple("%s.%s" % (a, k) for a in ("objAtt", "tempAtt") for k in MHA) + ("bn.weight", "bn.bias", "confLayer.0.weight", "confLayer.0.bias")
EPS = 1e-5
TILE_EDGES = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)


def make_params(F, seed=0):
    """{name: float32 array} of a RecurrentTemporalAttention(F): torch's default initialisation, then EVERY bias uniform in +-0.5 and
    bn.weight in [0.5, 1.5] (torch starts the attention biases at zero, and with zero biases a spuriously included zero key is
    nearly invisible)"""
    import torch
    from dynenv_amd import GpuTemporalAttention
    gen = torch.Generator().manual_seed(1000 + seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    layer = GpuTemporalAttention(F)
    torch.random.set_rng_state(state)
    with torch.no_grad():
        for k, p in layer.named_parameters():
            if k == "bn.weight":
                p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
            elif "bias" in k:
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)
    return {k: v.detach().numpy().copy() for k, v in layer.state_dict().items()}


def load(layer, params, dtype=None):
    """the parameters into a GpuTemporalAttention (or the reference's class), strict"""
    import torch
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return layer if dtype is None else layer.to(dtype)


def make_counts(T, M, P):
    """int32 [T, P]: the first players of time 0 take the tile edges that fit, M - 1 and M; then a player with no object at any time, one
    with none at time 0 only, one with objects at time 0 only, and (T > 1) one falling from M to 1 and one rising from 1 to M; the rest
    (and the other times of the first players) at random"""
    rng = np.random.default_rng(100 * T + M)
    edges = sorted(set(e for e in TILE_EDGES + (M - 1, M) if 0 <= e <= M))
    special = 3 + (2 if T > 1 else 0)
    assert P >= special + 1, "room for the required players"
    counts = rng.integers(0, M + 1, (T, P)).astype(np.int32)
    lead = min(len(edges), P - special)
    if lead < len(edges):   # what does not fit is dropped from the middle: 0, 1 and the last ones stay
        edges = edges[:lead // 2] + edges[len(edges) - (lead - lead // 2):]
    counts[0, :lead] = edges
    q = lead
    counts[:, q] = 0
    counts[0, q + 1] = 0
    counts[1:, q + 1] = np.maximum(counts[1:, q + 1], 1)
    counts[0, q + 2] = M
    counts[1:, q + 2] = 0
    if T > 1:
        counts[:, q + 3] = np.round(np.linspace(M, 1, T)).astype(np.int32)
        counts[:, q + 4] = np.round(np.linspace(1, M, T)).astype(np.int32)
    return counts


def masks_of(counts, M):
    """bool [T, P, M]: the arranger's masks, True from the count on"""
    return np.arange(M)[None, None, :] >= counts[:, :, None]


def layer_norm(x, w, b):
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + EPS) * w + b


def mha(pr, which, q_in, kv_in, k):
    g = lambda name: np.asarray(pr["%s.%s" % (which, name)], np.float64)  # noqa: E731
    F = q_in.shape[1]
    w, b = g("in_proj_weight"), g("in_proj_bias")
    q = q_in @ w[:F].T + b[:F]
    K = np.concatenate([kv_in[:k] @ w[F:2 * F].T + b[F:2 * F], g("bias_k").reshape(1, F)])
    V = np.concatenate([kv_in[:k] @ w[2 * F:].T + b[2 * F:], g("bias_v").reshape(1, F)])
    s = q @ K.T / np.sqrt(F)
    e = np.exp(s - s.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)) @ V @ g("out_proj.weight").T + g("out_proj.bias")


def attend_pool(padded, counts, pr):
    """padded [T, M, P, F] (any float type; slots at or behind a count are not looked at), counts [T, P] -> float64 [P, F]"""
    T, M, P, F = padded.shape
    out = np.zeros((P, F))
    cw, cb = np.asarray(pr["confLayer.0.weight"], np.float64).reshape(F), float(np.asarray(pr["confLayer.0.bias"]).reshape(()))
    lw, lb = np.asarray(pr["bn.weight"], np.float64), np.asarray(pr["bn.bias"], np.float64)
    for p in range(P):
        c = np.clip(counts[:, p], 0, M)
        n = int(c.max())
        if n == 0:
            continue
        X = np.zeros((T, n, F))
        for t in range(T):
            X[t, :c[t]] = padded[t, :c[t], p].astype(np.float64)
        fin, k = mha(pr, "objAtt", X[0], X[0], c[0]), c[0]
        for t in range(1, T):
            att = mha(pr, "objAtt", X[t], X[t], c[t])
            fin = layer_norm(mha(pr, "tempAtt", att, fin, k), lw, lb)
            k = max(k, c[t])
        conf = 1.0 / (1.0 + np.exp(-(fin @ cw + cb)))
        out[p] = (conf[:, None] * fin).sum(0) / n
    return out
