"""The numpy float64 statement of the policy head over a stored rollout and of its backward (include/dynenv.h, dynenv_policy_eval and
dynenv_policy_eval_backward) that the tests compare against, built on policy_ref.py's head and log_probs, and the case maker.  A helper
module: no tests.

Forward, per row (t, p): policy_ref.head's probs and value on features[t][p]; logp_g = log(clamp(probs_g[a_g], eps32, 1 - eps32)) with
a_g = actions[t][g][p] rounded and clamped into the group.
Backward, for the upstream (d_logp [T, G, P], d_probs [T, P, N], d_value [T, P]):
  dl_g = d_logp_g [eps32 <= probs_g[a_g] <= 1 - eps32] (onehot(a_g) - probs_g) + probs_g (d_probs_g - <d_probs_g, probs_g>)
  h_pre = f W1^T + b1, h = leaky(h_pre), xh = (h - mean) rstd, y = xh ln_w + ln_b, c = w2 ln_w:
  dh_pre = d_value rstd (c - mean(c) - xh mean(c xh)) leaky'(h_pre)      (leaky' = slope at h_pre <= 0)
  the eight sums over the rows and d_features = dl W_actor + dh_pre W1, in the packed layouts (32 actor rows, the padding 0)."""
import numpy as np

import policy_ref as PR

ROWS, MAX_WORKGROUPS = 64, 256   # DYNENV_POLICY_EVAL_ROWS, DYNENV_POLICY_EVAL_MAX_WORKGROUPS
PACKED = ("aw", "ab", "w1", "b1", "lnw", "lnb", "w2", "b2")
CRITIC = {"w1": "critic.blocks.Layer1.weight", "b1": "critic.blocks.Layer1.bias", "lnw": "critic.blocks.bn.weight", "lnb": "critic.blocks.bn.bias",
          "w2": "critic.blocks.Layer2.weight", "b2": "critic.blocks.Layer2.bias"}


def part(K):
    """float32 per workgroup slice of the backward's workspace (include/dynenv.h)"""
    return K * K // 2 + 34 * K + 36


def make_case(T, P, K, groups, AD, seed=0):
    """features float32 [T, P, K], actions float32 [T, AD, P] inside the groups (the columns behind G are 0), and the three upstream
    tensors, of order 1"""
    rng = np.random.default_rng(seed)
    G, N = len(groups), sum(groups)
    actions = np.zeros((T, AD, P), np.float32)
    for g, n in enumerate(groups):
        actions[:, g] = rng.integers(0, n, size=(T, P))
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    return dict(features=f32(T, P, K), actions=actions, d_logp=f32(T, G, P), d_probs=f32(T, P, N), d_value=f32(T, P))


def indices(actions, groups):
    """actions [T, AD, P] -> (int64 [T, G, P] inside the groups, whether a value had to be clamped)"""
    G = len(groups)
    v = np.rint(np.asarray(actions, np.float64)[:, :G])
    last = np.asarray(groups, np.float64).reshape(1, G, 1) - 1
    return np.clip(v, 0, last).astype(np.int64), bool(((v < 0) | (v > last)).any())


def critic(x, params, slope):
    """x [R, K] -> dict of the critic's intermediates, float64"""
    g = lambda k: np.asarray(params[CRITIC[k]], np.float64)  # noqa: E731
    pre = x @ g("w1").T + g("b1")
    h = np.where(pre > 0, pre, slope * pre)
    mean = h.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((h - mean) ** 2).mean(-1, keepdims=True) + PR.EPS)
    xh = (h - mean) * rstd
    y = xh * g("lnw") + g("lnb")
    return dict(pre=pre, rstd=rstd, xh=xh, y=y, value=y @ g("w2")[0] + g("b2")[0])


def forward(features, actions, params, groups, slope=PR.SLOPE):
    """-> float64 (log_probs [T, G, P], probs [T, P, N], values [T, P]) in the storage's layouts"""
    T, P, K = features.shape
    x = np.asarray(features, np.float64).reshape(T * P, K)
    probs, _, value = PR.head(x, params, groups)
    mine = critic(x, params, slope)["value"]
    if slope == PR.SLOPE:
        assert np.allclose(mine, value, rtol=1e-12, atol=1e-12)
    idx, _ = indices(actions, groups)
    acts = idx.transpose(0, 2, 1).reshape(T * P, len(groups))
    logp = PR.log_probs(probs, groups, acts)
    return logp.reshape(T, P, -1).transpose(0, 2, 1), probs.reshape(T, P, -1), mine.reshape(T, P)


def backward(features, actions, params, groups, d_logp, d_probs, d_value, slope=PR.SLOPE):
    """-> dict of float64 arrays: the eight gradients in the packed layouts (PACKED) and "dfeat" [T, P, K]"""
    T, P, K = features.shape
    G, N, R = len(groups), sum(groups), T * P
    x = np.asarray(features, np.float64).reshape(R, K)
    probs, _, _ = PR.head(x, params, groups)
    idx, _ = indices(actions, groups)
    acts = idx.transpose(0, 2, 1).reshape(R, G)
    up = np.asarray(d_logp, np.float64).transpose(0, 2, 1).reshape(R, G)
    dp = np.zeros((R, N)) if d_probs is None else np.asarray(d_probs, np.float64).reshape(R, N)
    dv = np.asarray(d_value, np.float64).reshape(R, 1)
    dl, off = np.zeros((R, 32)), 0
    for g, n in enumerate(groups):
        p = probs[:, off:off + n]
        pa = p[np.arange(R), acts[:, g]]
        live = ((pa >= PR.EPS32) & (pa <= 1 - PR.EPS32)).astype(np.float64)
        onehot = np.zeros((R, n))
        onehot[np.arange(R), acts[:, g]] = 1.0
        d = dp[:, off:off + n]
        dl[:, off:off + n] = (up[:, g] * live)[:, None] * (onehot - p) + p * (d - (d * p).sum(1, keepdims=True))
        off += n
    w, _ = PR.actor_rows(params)
    wa = np.zeros((32, K))
    wa[:N] = w[:N]
    c = critic(x, params, slope)
    g = lambda k: np.asarray(params[CRITIC[k]], np.float64)  # noqa: E731
    cc = g("w2")[0] * g("lnw")
    u = c["rstd"] * (cc - cc.mean() - c["xh"] * (cc * c["xh"]).mean(-1, keepdims=True))
    dh = dv * u * np.where(c["pre"] > 0, 1.0, slope)
    return dict(aw=dl.T @ x, ab=dl.sum(0), w1=dh.T @ x, b1=dh.sum(0), lnw=(dv * g("w2")[0] * c["xh"]).sum(0), lnb=(dv * g("w2")[0]).sum(0) + 0 * g("lnb"),
                w2=(dv * c["y"]).sum(0), b2=dv.sum(0), dfeat=(dl @ wa + dh @ g("w1")).reshape(T, P, K))


def names(groups):
    """the parameters dynenv_policy_eval_backward gives a gradient, in the module's names"""
    return ["actor.blocks.0.Layer.%d.%s" % (g, k) for g in range(len(groups)) for k in ("weight", "bias")] + list(CRITIC.values())


def by_name(packed, groups):
    """the packed gradients -> {parameter name: array in the parameter's shape}"""
    out, off = {}, 0
    for g, n in enumerate(groups):
        out["actor.blocks.0.Layer.%d.weight" % g] = packed["aw"][off:off + n]
        out["actor.blocks.0.Layer.%d.bias" % g] = packed["ab"][off:off + n]
        off += n
    for k, name in CRITIC.items():
        out[name] = packed[k].reshape(1, -1) if k == "w2" else packed[k]
    return out


def pack(named, K, groups):
    """{parameter name: gradient} -> the packed layouts (32 actor rows, the padding 0)"""
    N = sum(groups)
    aw, ab = np.zeros((32, K)), np.zeros(32)
    aw[:N] = np.concatenate([named["actor.blocks.0.Layer.%d.weight" % g] for g in range(len(groups))])
    ab[:N] = np.concatenate([named["actor.blocks.0.Layer.%d.bias" % g] for g in range(len(groups))])
    out = dict(aw=aw, ab=ab)
    for k, name in CRITIC.items():
        out[k] = np.asarray(named[name], np.float64).reshape(-1) if k in ("w2", "b2") else np.asarray(named[name], np.float64)
    return out
