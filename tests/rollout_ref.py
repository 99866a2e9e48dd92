"""The rollout storage as numpy statements (a helper module: no tests in it): the insert as pure indexing plus astype, the three modes of
the returns on np.float32 scalars in the order include/dynenv.h states, a2c_loss and its PPO branch (DynEnv/models/storage.py:211-290) in
float64 - and the case maker and the loader of the reference's own class that the tests and tests/golden/gen_golden_rollout_storage.py share."""
import ast
import collections
import itertools
import json
import os

import numpy as np

REF_DIR = os.environ.get("DYNENV_REFERENCE", "/root/reference")
REF_STORAGE = os.path.join(REF_DIR, "DynEnv", "models", "storage.py")
REF_LOSSES = os.path.join(REF_DIR, "DynEnv", "models", "loss_descriptors.py")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_storage.json")

BUFFERS = ("rewards", "agentFinished", "features", "actions", "log_probs", "log_probs_old", "values", "dones", "probs")


# ---- the insert
def make_buffers(T, E, A, K, G, AD, N, ppo=True, fill=None):
    """the buffers of reset_buffers (storage.py:76-111) and probs [T][P][N]; `fill`: a function (name, shape, dtype) -> array, else zeros"""
    P = E * A
    shapes = dict(rewards=(T, P), agentFinished=(T, P), features=(T + 1, P, K), actions=(T, AD, P), log_probs=(T, G, P), log_probs_old=(T, G, P),
                  values=(T, P), dones=(T, E), probs=(T, P, N))
    out = {}
    for k, shape in shapes.items():
        if (k == "log_probs_old" and not ppo) or (k == "probs" and not N):
            continue
        dt = np.uint8 if k == "agentFinished" else np.float32
        out[k] = np.zeros(shape, dt) if fill is None else fill(k, shape, dt)
    return out


def insert_row(bufs, t, rewards=None, finished=None, feat0=None, feat1=None, actions=None, log_probs=None, value=None, dones=None, probs=None,
               log_probs_old=None, features_only=False):
    """storage.py:158-166 at row t, in place: indexing and astype only.  None leaves its buffer alone."""
    if feat0 is not None:
        bufs["features"][t] = feat0 if feat1 is None else np.concatenate([feat0, feat1], axis=1)
    if features_only:
        return
    if rewards is not None:
        bufs["rewards"][t] = rewards.reshape(-1).astype(np.float32)
    if finished is not None:
        bufs["agentFinished"][t] = (finished.reshape(-1) != 0).astype(np.uint8)
    if actions is not None:
        bufs["actions"][t] = actions.T.astype(np.float32)
    if log_probs is not None:
        bufs["log_probs"][t] = log_probs.T
    if log_probs_old is not None:
        bufs["log_probs_old"][t] = log_probs_old.T
    if value is not None:
        bufs["values"][t] = value.reshape(-1)
    if dones is not None:
        bufs["dones"][t] = (dones != 0).astype(np.float32)
    if probs is not None:
        bufs["probs"][t] = probs


def make_step(rng, E, A, F, two, G, AD, N):
    """one step's results as a step and GpuPolicyHead.act leave them; G < AD leaves zero columns"""
    P = E * A
    actions = np.zeros((P, AD), np.int32)
    actions[:, :G] = rng.integers(0, 7, (P, G))
    return dict(rewards=rng.standard_normal((E, A)) * 3.0,   # float64: most are not float32 values, so the rounding is visible
                finished=(rng.random((E, A)) < 0.3).astype(np.uint8) * rng.integers(1, 255, (E, A)).astype(np.uint8),
                feat0=rng.standard_normal((P, F)).astype(np.float32), feat1=rng.standard_normal((P, F)).astype(np.float32) if two else None,
                actions=actions, log_probs=-rng.random((P, G)).astype(np.float32), log_probs_old=-rng.random((P, G)).astype(np.float32),
                value=rng.standard_normal(P).astype(np.float32), dones=(rng.random(E) < 0.4).astype(np.uint8),
                probs=rng.random((P, N)).astype(np.float32) if N else None)


# ---- the returns, on np.float32 scalars
def returns(rewards, values, dones, final_value, A, discount=0.99, mode="reference", gae_lambda=0.95):
    """-> (returns, advantages) float32 [T, P], every multiply and add rounded to float32 on its own, in the header's order"""
    f = np.float32
    T, P = rewards.shape
    g, lam = f(discount), f(gae_lambda)
    ret, adv_out = np.zeros((T, P), f), np.zeros((T, P), f)
    for p in range(P):
        e = p // A
        if mode == "gae":
            gl = f(g * lam)
            adv, nxt = f(0), f(final_value[p])
            for t in reversed(range(T)):
                nd = f(f(1) - f(dones[t, e]))
                v = f(values[t, p])
                delta = f(f(f(rewards[t, p]) + f(f(g * nxt) * nd)) - v)
                adv = f(delta + f(f(gl * adv) * nd))
                ret[t, p] = f(adv + v)
                adv_out[t, p] = adv
                nxt = v
            continue
        R = f(final_value[p])
        for t in reversed(range(T)):
            x = f(g * R)
            if mode == "dones":
                x = f(x * f(f(1) - f(dones[t, e])))
            R = f(f(rewards[t, p]) + x)
            ret[t, p] = R
            adv_out[t, p] = f(R - f(values[t, p]))
    return ret, adv_out


# ---- the loss, float64, with a first-order bound of a float32 evaluation's distance from it
Loss = collections.namedtuple("Loss", ["loss", "policy", "value", "entropy", "temp_entropy", "bound"])
U = 2.0 ** -24   # the unit roundoff of float32


def mean_bound(x, ops):
    """a float32 mean of x.size terms, each formed by `ops` float32 operations from exact inputs, summed in ANY order, lies within
    (x.size + ops) * U * mean|term| of the exact mean, to first order: (x.size - 1) additions and the division by the count, each of
    relative error U on a partial sum that mean|term| * size bounds, plus ops * U on every term"""
    return (x.size + ops) * U * float(np.abs(x).mean())


def _entropy(p, eps_in):
    """Categorical(probs=p).entropy() over the last axis - p / p.sum(), logits = log(clamp(p, eps32, 1 - eps32)), -sum p * logits -
    and its float32 bound where every p carries a relative error eps_in: the normalised p_j one of e = 2 eps_in + (n + 1) U (the sum of n
    terms and the division), its logarithm an absolute one of e + 2 U |log p_j| (the rounding of log, two units), the product one more
    U, the sum of the n products n U of their magnitudes: sum_j p_j e (|log p_j| + 1) + (3 + n) U sum_j p_j |log p_j|"""
    n = p.shape[-1]
    p = p / p.sum(-1, keepdims=True)
    eps = float(np.finfo(np.float32).eps)
    lg = np.log(np.clip(p, eps, 1 - eps))
    e = 2 * eps_in + (n + 1) * U
    return -(p * lg).sum(-1), (p * e * (np.abs(lg) + 1)).sum(-1) + (3 + n) * U * (p * np.abs(lg)).sum(-1)


def a2c_loss(returns_, advantages, values, log_probs, probs, groups, value_coeff, entropy_coeff, use_full_entropy=False, log_probs_old=None,
             ppo_clip=0.2, delta=1e-8):
    """storage.py:211-290 in float64 on float32 inputs: returns_ [T, P] from returns(), advantages the policy term's weight, log_probs
    [T, G, P], probs [T, P, N] split by `groups`; log_probs_old switches to the PPO branch as it runs (`+ delta` outside the exp, the
    minimum with its sign).  `bound`: a dict, per field, of the first-order distance of a float32 evaluation of the same statements
    (tests/test_rollout_ref.py states the derivation)."""
    d = np.float64
    ret, adv, values, lp = returns_.astype(d), advantages.astype(d), values.astype(d), log_probs.astype(d)
    T, G, P = lp.shape
    if log_probs_old is None:
        per_group = [-lp[:, g] * adv for g in range(G)]   # one product per term
        means = np.array([x.mean() for x in per_group])
        policy = means.mean()
        b_policy = float(np.mean([mean_bound(x, 1) for x in per_group])) + mean_bound(means, 0)
    else:
        # a term: the difference (1), exp (2 units, and the difference's rounding scaled by |x| <= 1: 1), + delta (1), the clamp's bounds
        # rounded to float32 (1), the product (1)
        r = np.exp(lp - log_probs_old.astype(d)).transpose(1, 0, 2) + delta
        rc = np.clip(r, 1 - ppo_clip, 1 + ppo_clip)
        x = np.minimum(r * adv, rc * adv)
        policy, b_policy = x.mean(), mean_bound(x, 7)
    x = (ret - values) ** 2   # the difference (counted twice by the square) and the square
    value = value_coeff * x.mean()
    b_value = value_coeff * mean_bound(x, 3) + U * abs(value)
    blocks = np.split(probs.astype(d), np.cumsum(groups)[:-1], axis=2)

    def outer(pairs):
        h = np.concatenate([np.ravel(a) for a, _ in pairs])
        hb = np.concatenate([np.ravel(b) for _, b in pairs])
        return h.mean(), float(hb.mean()) + mean_bound(h, 0)
    temp, b_temp = outer([_entropy(b.mean(0), (T + 0) * U) for b in blocks])      # a mean of T positive terms: relative T U
    batch, b_batch = outer([_entropy(b.mean(1), (P + 0) * U) for b in blocks])
    full, b_full = outer([_entropy(b, 0.0) for b in blocks])
    ent, b_ent = (full, b_full) if use_full_entropy else (batch, b_batch)
    entropy, temp_entropy = -entropy_coeff * ent, entropy_coeff * temp
    b_entropy, b_temp = entropy_coeff * b_ent + U * abs(entropy), entropy_coeff * b_temp + U * abs(temp_entropy)
    loss = policy + value + entropy + temp_entropy
    b_loss = b_policy + b_value + b_entropy + b_temp + 4 * U * (abs(policy) + abs(value) + abs(entropy) + abs(temp_entropy))
    return Loss(loss, policy, value, entropy, temp_entropy, dict(loss=b_loss, policy=b_policy, value=b_value, entropy=b_entropy, temp_entropy=b_temp))


# ---- the cases of the golden file and the reference's own class
def golden_case(T, E, A, groups, F, seed):
    """the inputs of one case: T steps as the reference's insert takes them, and final_value"""
    rng = np.random.default_rng(seed)
    P, G, N = E * A, len(groups), sum(groups)
    steps = []
    for _ in range(T):
        s = make_step(rng, E, A, F, False, G, G, N)
        parts = [rng.random((P, n)).astype(np.float32) + np.float32(0.05) for n in groups]
        s["probs"] = np.concatenate([(p / p.sum(1, keepdims=True)).astype(np.float32) for p in parts], axis=1)
        s["rewards"] = s["rewards"].astype(np.float32).astype(np.float64)
        steps.append(s)
    return steps, rng.standard_normal(P).astype(np.float32)


def reference_class():
    """RolloutStorage compiled out of the reference's file with ast (the package around it does not import), with the reference's own
    A2CLosses compiled the same way"""
    import torch
    from torch.distributions import Categorical
    ns = dict(torch=torch)
    tree = ast.parse(open(REF_LOSSES).read())
    keep = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom)) or (isinstance(n, ast.ClassDef) and n.name in ("LossLogger", "A2CLosses"))]
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_LOSSES, "exec"), ns)
    ns.update(itertools=itertools, deque=collections.deque, np=np, Categorical=Categorical)
    tree = ast.parse(open(REF_STORAGE).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("sliceable_deque", "RolloutStorage")]
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_STORAGE, "exec"), ns)
    return ns["RolloutStorage"]


def reference_filled(cls, steps, E, A, groups, F, use_ppo, use_full_entropy):
    """the reference's storage after its own insert of every step -> (storage, action_probs: its list over time of lists over groups)"""
    import torch
    T, G = len(steps), len(groups)
    st = cls(T, E, A, G, 1, feature_size=F, is_cuda=False, use_full_entropy=use_full_entropy, use_ppo=use_ppo)
    action_probs = []
    for t, s in enumerate(steps):
        col = lambda x: [torch.from_numpy(np.ascontiguousarray(x[:, g])) for g in range(G)]
        st.insert(t, s["rewards"].astype(np.float32), torch.from_numpy(s["finished"]), None, col(s["actions"].astype(np.float32)), col(s["log_probs"]),
                  torch.from_numpy(s["value"]).view(-1, 1), s["dones"].tolist(), torch.from_numpy(s["feat0"]), None, None, None, None,
                  col(s["log_probs_old"]) if use_ppo else None)
        action_probs.append([torch.from_numpy(b.copy()) for b in np.split(s["probs"], np.cumsum(groups)[:-1], axis=1)])
    return st, action_probs


def bits(x):
    """float32 array -> its words as a list of ints (JSON keeps them exactly)"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32).reshape(-1).tolist()


def from_bits(words, shape):
    return np.array(words, np.uint32).view(np.float32).reshape(shape)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
