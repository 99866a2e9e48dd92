"""The curiosity module as numpy float64 statements (a helper module: no tests in it): the per-row terms of dynenv_icm_losses
(include/dynenv.h) and the losses of ICMNet.forward + _calc_loss (DynEnv/models/icm.py:53-109) as they run - and the parameter and case
makers, the loader of the reference's own ICMNet and the loader of the fixture that the tests and tests/golden/gen_golden_icm.py share."""
import ast
import collections
import contextlib
import enum
import json
import os

import numpy as np

REF_DIR = os.environ.get("DYNENV_REFERENCE", "/root/reference")
REF_ICM = os.path.join(REF_DIR, "DynEnv", "models", "icm.py")
REF_ACTOR = os.path.join(REF_DIR, "DynEnv", "models", "actor_critic.py")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icm.json")

HIDDEN, SLOPE = 140, 0.1   # ForwardNet.fc_hidden and its LeakyReLU (icm.py:124, 131)
U = 2.0 ** -24             # the unit roundoff of float32


def have_reference():
    return os.path.exists(REF_ICM) and os.path.exists(REF_ACTOR)


# ---- parameters and cases
def param_shapes(K, groups, rollout, loss_attn=False):
    """name -> shape of ICMNet.state_dict() for one MultiDiscrete member of `groups`, built from the constructor's arguments"""
    N = sum(groups)
    out = collections.OrderedDict()

    def linear(name, rows, cols):
        out[name + ".weight"], out[name + ".bias"] = (rows, cols), (rows,)

    def forward_net(name):
        linear(name + ".fc1", HIDDEN, K + N)
        linear(name + ".fc2", K, HIDDEN)
    forward_net("pred_net.fwd_net")
    for g, n in enumerate(groups):
        linear("pred_net.inv_net.blocks.0.Layer.%d" % g, n, 2 * K)
    if loss_attn:
        linear("loss_attn.attention", K, K)
    linear("loss_long_horizon_curiosity.attention.attention", K, K)
    for t in range(rollout):
        forward_net("long_horizon_fwd_net.fwd_nets.%d" % t)
    return out


def make_params(K, groups, rollout, loss_attn=False, seed=0):
    """float32 parameters: weights uniform in +-1 / sqrt(fan_in), every bias in +-0.5 (a missing bias moves a term visibly)"""
    rng = np.random.default_rng(seed)
    pr = collections.OrderedDict()
    for name, shape in param_shapes(K, groups, rollout, loss_attn).items():
        scale = 0.5 if name.endswith(".bias") else 1.0 / np.sqrt(shape[1])
        pr[name] = (rng.uniform(-1.0, 1.0, shape) * scale).astype(np.float32)
    return pr


def make_case(T, P, K, groups, AD=None, seed=0, mask="random"):
    """standard-normal features [T + 1, P, K], uniform actions [T, AD, P] as float32 (the columns behind G hold 7: they are never read)
    and agent_finished bool [T, P]: about 30 % finished ("random"), all finished ("all"), exactly one active ("one") or nobody ("none")"""
    rng = np.random.default_rng(seed)
    G = len(groups)
    AD = G if AD is None else AD
    features = rng.standard_normal((T + 1, P, K)).astype(np.float32)
    actions = np.full((T, AD, P), 7.0, np.float32)
    for g, n in enumerate(groups):
        actions[:, g] = rng.integers(0, n, (T, P))
    finished = rng.random((T, P)) < 0.3
    if mask == "all":
        finished[:] = True
    elif mask == "one":
        finished[:] = True
        finished[rng.integers(0, T), rng.integers(0, P)] = False
    elif mask == "none":
        finished[:] = False
    return dict(features=features, actions=actions, finished=finished)


# ---- the statements, float64
def _linear(x, pr, name):
    return x @ pr[name + ".weight"].astype(np.float64).T + pr[name + ".bias"].astype(np.float64)


def _forward_net(x, pr, name):
    h = _linear(x, pr, name + ".fc1")
    return _linear(np.where(h > 0, h, h * SLOPE), pr, name + ".fc2")


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def indices(actions, groups):
    """[T, AD, P] -> int [T, G, P] rounded and clamped into the groups, and whether anything had to be clamped"""
    G = len(groups)
    v = np.rint(actions[:, :G].astype(np.float64))
    last = np.asarray(groups, np.float64).reshape(1, G, 1) - 1
    ok = (v >= 0) & (v <= last)
    return np.where(ok, v, np.where(v > last, last, 0)).astype(np.int64), bool((~ok).any())


def one_hot(idx, groups):
    T, G, P = idx.shape
    out = np.zeros((T, P, sum(groups)))
    starts = np.cumsum((0,) + tuple(groups[:-1]))
    for g in range(G):
        np.put_along_axis(out, (idx[:, g] + starts[g])[..., None], 1.0, axis=2)
    return out


def rows(features, actions, pr, groups):
    """-> (curiosity [T, P], inverse_ce [T, G, P], se [T, P, K]): the header's per-row terms"""
    f = features.astype(np.float64)
    cur, nxt = f[:-1], f[1:]
    idx, _ = indices(actions, groups)
    pred = _forward_net(np.concatenate([cur, one_hot(idx, groups)], 2), pr, "pred_net.fwd_net")
    se = (pred - nxt) ** 2
    x = np.concatenate([cur, nxt], 2)
    ce = []
    for g in range(len(groups)):
        l = _linear(x, pr, "pred_net.inv_net.blocks.0.Layer.%d" % g)
        m = l.max(-1)
        ce.append(m + np.log(np.exp(l - m[..., None]).sum(-1)) - np.take_along_axis(l, idx[:, g][..., None], 2)[..., 0])
    return se.mean(-1), np.stack(ce, 1), se


def losses(features, actions, finished, pr, groups, forward_coeff=1e-2, icm_beta=1e-2, long_horizon_coeff=0.0, loss_attn=False):
    """ICMNet.forward + _calc_loss as they run -> dict(forward, inverse, long_horizon_forward, loss, n); the long-horizon term is always
    evaluated here (the module's long_horizon=True)"""
    T = features.shape[0] - 1
    K = features.shape[2]
    cur_err, ce, se = rows(features, actions, pr, groups)
    mask = ~np.asarray(finished, bool)
    n = int(mask.sum())
    if n == 0:
        return dict(forward=0.0, inverse=0.0, long_horizon_forward=0.0, loss=0.0, n=0)
    nxt = features[1:].astype(np.float64)
    if loss_attn:   # icm.py:93: not masked
        fwd = (se * _softmax(_linear(nxt, pr, "loss_attn.attention"))).mean()
    else:
        fwd = se[mask].sum() / (n * K)
    inv = float(np.mean([ce[:, g][mask].sum() / n for g in range(len(groups))]))
    idx, _ = indices(actions, groups)
    oh = one_hot(idx, groups)
    pred, lh, weight = features[0].astype(np.float64), 0.0, 1.0
    for t in range(T):
        pred = _forward_net(np.concatenate([pred, oh[t]], 1), pr, "long_horizon_fwd_net.fwd_nets.%d" % t)
        step = (pred - nxt[t]) ** 2
        lh += (weight * step).mean()
        weight = step * _softmax(_linear(step, pr, "loss_long_horizon_curiosity.attention.attention"))
    out = dict(forward=forward_coeff * fwd, inverse=icm_beta * inv, long_horizon_forward=long_horizon_coeff * lh, n=n)
    out["loss"] = out["forward"] + out["inverse"]
    return out


# ---- the module under test and the reference's own class
def load(module, pr):
    """pr into a GpuICM (or the reference's ICMNet) with strict=True, in the module's dtype"""
    import torch
    dt = next(module.parameters()).dtype
    module.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)).to(dt) for k, v in pr.items()}, strict=True)
    return module


class _StubLosses(object):
    """ICMLosses without the .item() calls of prepare_losses (loss_descriptors.py:49-55): the fields stay tensors"""

    def __init__(self, forward, inverse, long_horizon_forward):
        self.forward, self.inverse, self.long_horizon_forward = forward, inverse, long_horizon_forward

    def prepare_losses(self):
        self.loss = self.inverse.sum() + self.forward.sum()


def reference_classes():
    """ICMNet and what it needs compiled out of the reference's files with ast (the package around them does not import: gym): its own
    ActorLayer from actor_critic.py; stubs for gym's MultiDiscrete and Box, the two enums, flatten and ICMLosses"""
    import torch

    class MultiDiscrete(object):
        def __init__(self, nvec):
            self.nvec = np.asarray(nvec, np.int64)
            self.shape = self.nvec.shape

    class Box(object):
        pass

    class AttentionType(enum.Enum):
        SINGLE_ATTENTION = 0
        DOUBLE_ATTENTION = 1

    class AttentionTarget(enum.Enum):
        NONE = 0
        ICM = 1
        A2C = 2
        ICM_LOSS = 3
    ns = dict(torch=torch, nn=torch.nn, F=torch.nn.functional, np=np, MultiDiscrete=MultiDiscrete, Box=Box, AttentionType=AttentionType,
              AttentionTarget=AttentionTarget, ICMLosses=_StubLosses, flatten=lambda l: [item for sub in l for item in sub])
    for path, names in ((REF_ACTOR, ("ActorLayer", "ActorBlock")), (REF_ICM, None)):
        tree = ast.parse(open(path).read())
        keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and (names is None or n.name in names)]
        exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


@contextlib.contextmanager
def default_dtype(dtype):
    """the reference creates its accumulators and its one-hot with torch's default dtype: float64 means float64 there too"""
    import torch
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def reference_net(ns, K, groups, T, P, pr, forward_coeff, icm_beta, long_horizon_coeff, loss_attn, dtype):
    """the reference's ICMNet with `pr` loaded; K = feat_size * 2"""
    target = ns["AttentionTarget"].ICM_LOSS if loss_attn else ns["AttentionTarget"].NONE
    with default_dtype(dtype):
        net = ns["ICMNet"](1, P, [ns["MultiDiscrete"](groups)], target, ns["AttentionType"].SINGLE_ATTENTION, K // 2, forward_coeff, long_horizon_coeff,
                           icm_beta, 1, T)
    return load(net.to(dtype), pr)


# ---- the fixture
GOLDEN_CASES = [dict(T=3, P=6, K=16, groups=(3, 3), mask=m, loss_attn=a, seed=s) for s, (m, a) in
                enumerate((("random", False), ("all", False), ("one", False), ("random", True), ("one", True)))] + \
               [dict(T=3, P=6, K=16, groups=(5, 3, 3), mask=m, loss_attn=a, seed=10 + s) for s, (m, a) in
                enumerate((("random", False), ("none", True), ("all", True)))]
GOLDEN_COEFFS = dict(forward_coeff=0.2, icm_beta=0.8, long_horizon_coeff=0.5)


def golden_inputs(c):
    """the parameters and the case of one entry of GOLDEN_CASES"""
    pr = make_params(c["K"], c["groups"], c["T"], c["loss_attn"], seed=100 + c["seed"])
    return pr, make_case(c["T"], c["P"], c["K"], c["groups"], seed=c["seed"], mask=c["mask"])


def bits(x):
    """float32 array -> its words as a list of ints (JSON keeps them exactly)"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32).reshape(-1).tolist()


def from_bits(words, shape=()):
    return np.array(words, np.uint32).view(np.float32).reshape(shape)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
