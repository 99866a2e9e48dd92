"""tests/policy_ref.py - the numpy float64 statement the GPU tests of the fused policy head compare against - held to the torch route of
GpuPolicyHead in float64 on the CPU; that route's draw held to the statement's inverse CDF on the route's own float32 probabilities bit
for bit; the draw counter; and, where the reference is on this machine, forward bit for bit against the reference's own ActorLayer and
CriticLayer (DynEnv/models/actor_critic.py:161-242) with its state_dict() loaded strict=True, and transform_actions against the
reference's transformActions.  tests/golden/transform_actions.json holds that function's results for every action tuple of both
environments.  No GPU."""
import ast
import itertools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as PR  # noqa: E402

REF_AC = "/root/reference/DynEnv/models/actor_critic.py"
REF_UTILS = "/root/reference/DynEnv/utils/utils.py"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transform_actions.json")
# (K, nvec, C): Driving; RoboCup; RoboCup with allowHeadTurn; the cap on a group; eight groups with one of a single action
SPACES = [(64, (3, 3), 0), (128, (5, 3, 3, 7), 0), (256, (5, 3, 3), 1), (128, (16, 16), 0), (64, (2, 2, 1, 2, 2, 2, 2, 2), 0)]
P = 37
SEED, DRAW = 2 ** 40 + 5, 2 ** 33 + 7   # both with a high word


def _feature(K, seed=0):
    return np.random.default_rng(seed + K).standard_normal((P, K))


def _head(K, nvec, C, pr, dtype=None, seed=SEED, draw=DRAW):
    from dynenv_amd import GpuPolicyHead
    layer = PR.load(GpuPolicyHead(K, PR.space(nvec, C), seed=seed), pr, dtype)
    layer.reseed(seed, draw)
    return layer


@pytest.mark.parametrize("case", SPACES, ids=str)
def test_statement_is_the_torch_route_in_float64(case):
    import torch
    K, nvec, C = case
    G = len(nvec)
    pr = PR.make_params(K, nvec, C, seed=K)
    x = _feature(K)
    probs, cont, value = PR.head(x, pr, nvec, C)
    layer = _head(K, nvec, C, pr, torch.float64)
    assert layer.last_route is None
    with torch.no_grad():
        out = layer.act(torch.from_numpy(x))
    assert layer.last_route.startswith("torch (fallback: "), "a CPU call reports a fallback"
    got = torch.cat(out.probs, 1).numpy()
    assert got.dtype == np.float64 and got.shape == (P, sum(nvec)) and np.abs(got - probs).max() < 1e-12
    assert tuple(out.value.shape) == (P, 1) and np.abs(out.value.numpy()[:, 0] - value).max() < 1e-12
    assert out.actions.dtype == torch.int32 and tuple(out.actions.shape) == (P, G + C) and not out.actions[:, G:].any()
    acts = out.actions.numpy()[:, :G]
    assert (acts >= 0).all() and (acts < np.array(nvec)).all()
    want_lp = PR.log_probs(probs, nvec, acts, eps=float(np.finfo(np.float64).eps))
    assert tuple(out.log_probs.shape) == (P, G) and np.abs(out.log_probs.numpy() - want_lp).max() < 1e-12
    if C:
        assert out.head.dtype == torch.float64 and tuple(out.head.shape) == (P,) and np.abs(out.head.numpy() - cont[:, 0]).max() < 1e-12
        assert np.abs(cont).max() < PR.HIGH and np.abs(cont).max() > 0.1
    else:
        assert out.head is None
    assert np.array_equal(out.next_ext.numpy(), PR.transform_table(out.actions.numpy(), False).astype(np.float32))
    # forward: the logits whose softmax those probabilities are, and the same value; differentiable
    layer.reseed(SEED, DRAW)
    again = layer.act(torch.from_numpy(x))
    assert layer.last_route == "torch" and again.log_probs.grad_fn is not None and again.value.grad_fn is not None
    assert torch.equal(again.actions, out.actions) and torch.equal(again.log_probs.detach(), out.log_probs)
    policies, v = layer(torch.from_numpy(x))
    assert len(policies) == G + (1 if C else 0) and torch.equal(v.detach(), out.value)
    assert all(torch.equal(torch.softmax(l, -1).detach(), p) for l, p in zip(policies, out.probs))


@pytest.mark.parametrize("case", SPACES, ids=str)
def test_the_torch_route_draws_the_statements_inverse_cdf_of_its_own_float32_probabilities(case):
    import torch
    K, nvec, C = case
    G = len(nvec)
    pr = PR.make_params(K, nvec, C, seed=K + 1)
    x = torch.from_numpy(_feature(K, 1).astype(np.float32))
    layer = _head(K, nvec, C, pr).requires_grad_(False)
    for call, row_base in enumerate((0, 0, 2 ** 32 - 5, 2 ** 63 + 11)):   # the counter runs on; a row_base across 2^32 and one with the top bit
        out = layer.act(x, row_base=row_base)
        probs = torch.cat(out.probs, 1).numpy()
        assert probs.dtype == np.float32
        want = PR.draw_actions(probs, nvec, SEED, DRAW + call, row_base)
        assert np.array_equal(out.actions.numpy()[:, :G], want), (call, row_base)
        lp = np.log(np.clip(np.take_along_axis(probs, np.cumsum((0,) + nvec[:-1])[None, :] + want, 1), np.float32(PR.EPS32), np.float32(1 - PR.EPS32)))
        assert np.abs(out.log_probs.numpy() - lp).max() <= 2 * PR.EPS32 * np.abs(lp).max()
    # a probability of zero is never drawn, a single action always: the statement on made-up probabilities
    u = np.array([0.0, 0.25, 0.5, 1 - 2.0 ** -24])
    assert PR.inverse_cdf(np.array([[0, 0.5, 0, 0.5]] * 4, np.float32), u).tolist() == [1, 1, 3, 3]
    assert PR.inverse_cdf(np.array([[0.5, 0.5, 0, 0]] * 4, np.float32), u).tolist() == [0, 0, 1, 1]
    assert PR.inverse_cdf(np.ones((4, 1), np.float32), u).tolist() == [0, 0, 0, 0]
    from dynenv_amd.policy import sample_inverse_cdf
    for pr_ in ([0, 0.5, 0, 0.5], [0.5, 0.5, 0, 0], [1.0], [0.1, 0.2, 0.3, 0.4]):
        t = torch.tensor([pr_] * 4, dtype=torch.float32)
        assert sample_inverse_cdf(t, torch.from_numpy(u).float()).tolist() == PR.inverse_cdf(t.numpy(), u).tolist()


def test_the_draw_is_the_philox_of_the_statement_and_the_counter_advances():
    import torch
    from dynenv_amd.policy import RNG_PURPOSE, draw_uniform
    assert RNG_PURPOSE == PR.PURPOSE
    for seed, draw, row_base, G in ((0, 0, 0, 1), (SEED, DRAW, 2 ** 32 - 3, 8), (2 ** 64 - 1, 2 ** 64 - 1, 7, 5)):
        signed = draw - 2 ** 64 if draw >> 63 else draw
        got = draw_uniform(seed, torch.tensor([signed], dtype=torch.int64), row_base, 9, G, "cpu")
        want = PR.uniform(seed, draw, row_base, 9, G)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().astype(np.float64), want) and want.min() >= 0 and want.max() < 1
    K, nvec, C = 64, (5, 3, 3, 7), 0
    pr = PR.make_params(K, nvec, C)
    x = torch.from_numpy(_feature(K, 2).astype(np.float32))
    layer = _head(K, nvec, C, pr).requires_grad_(False)
    assert layer.draw.dtype == torch.int64 and int(layer.draw) == DRAW
    first = layer.act(x).actions.clone()
    assert int(layer.draw) == DRAW + 1
    second = layer.act(x).actions.clone()
    assert int(layer.draw) == DRAW + 2 and not torch.equal(first, second), "another draw gives other actions"
    layer.reseed(SEED, DRAW)
    assert torch.equal(layer.act(x).actions, first), "the same (seed, draw) gives the same actions"
    layer.reseed(SEED, DRAW)
    assert not torch.equal(layer.act(x, row_base=1000).actions, first), "another row_base gives other actions"
    layer.reseed(SEED, DRAW)
    shifted = layer.act(x[1:], row_base=1).actions
    assert torch.equal(shifted, first[1:]), "a row keeps its stream: row_base + p"
    layer.reseed(SEED + 1, DRAW)
    assert not torch.equal(layer.act(x).actions, first), "another seed gives other actions"
    layer.reseed(SEED, 2 ** 64 - 1)
    layer.act(x)
    assert int(layer.draw) == 0, "the counter is a 64-bit word"
    out = torch.zeros((P, 4), dtype=torch.int32)
    layer.reseed(SEED, DRAW)
    res = layer.act(x, out_actions=out)
    assert torch.equal(out, first) and res.actions.data_ptr() == out.data_ptr(), "out_actions is written in place"


def test_names_shapes_and_routes(monkeypatch):
    import torch
    import dynenv_amd
    from dynenv_amd import GpuPolicyHead
    assert "GpuPolicyHead" in dynenv_amd.__all__
    K = 128
    layer = GpuPolicyHead(K, PR.space((5, 3, 3), 1))
    want = {"actor.blocks.0.Layer.0.weight": (5, K), "actor.blocks.0.Layer.0.bias": (5,), "actor.blocks.0.Layer.1.weight": (3, K),
            "actor.blocks.0.Layer.1.bias": (3,), "actor.blocks.0.Layer.2.weight": (3, K), "actor.blocks.0.Layer.2.bias": (3,),
            "actor.blocks.1.Layer.weight": (1, K), "actor.blocks.1.Layer.bias": (1,), "critic.blocks.Layer1.weight": (K // 2, K),
            "critic.blocks.Layer1.bias": (K // 2,), "critic.blocks.Layer2.weight": (1, K // 2), "critic.blocks.Layer2.bias": (1,),
            "critic.blocks.bn.weight": (K // 2,), "critic.blocks.bn.bias": (K // 2,)}
    assert [(k, tuple(v.shape)) for k, v in layer.state_dict().items()] == list(want.items())
    assert layer.critic.blocks.relu.negative_slope == PR.SLOPE and layer.critic.blocks.bn.eps == PR.EPS
    assert layer.action_cols == 4 and layer.nvec == [5, 3, 3] and layer.n_cont == 1
    pr = PR.make_params(K, (5, 3, 3), 1)
    assert tuple(pr) == tuple(want) and all(np.abs(v).max() > 0.1 for k, v in pr.items() if "bias" in k)
    x = torch.zeros(4, K)
    layer.act(x)
    assert layer.last_route == "torch"
    layer.requires_grad_(False)
    layer.act(x)
    assert layer.last_route.startswith("torch (fallback: features that are not on the device")
    monkeypatch.setenv("DYNENV_POLICY_FUSED", "0")
    layer.act(x)
    assert layer.last_route == "torch (fallback: DYNENV_POLICY_FUSED=0)"
    monkeypatch.delenv("DYNENV_POLICY_FUSED")
    other = GpuPolicyHead(96, PR.space((3, 3))).requires_grad_(False)
    other.act(torch.zeros(4, 96))
    assert other.last_route.startswith("torch (fallback: F = 96")
    wide = GpuPolicyHead(64, PR.space((17, 3))).requires_grad_(False)
    out = wide.act(torch.zeros(4, 64))
    assert wide.last_route.startswith("torch (fallback: an action space beyond") and tuple(out.probs[0].shape) == (4, 17)
    with torch.no_grad():
        layer.requires_grad_(True)
        layer.act(x)
        assert layer.last_route.startswith("torch (fallback: ")


def _golden():
    return json.load(open(GOLDEN))


def test_transform_actions_against_the_recorded_results_of_the_reference():
    import torch
    from dynenv_amd.policy import transform_actions
    gold = _golden()
    assert len(gold["driving"]["actions"]) == 9 and len(gold["robocup"]["actions"]) == 315
    for name, g in gold.items():
        acts = np.array(g["actions"], np.int64)
        assert acts.tolist() == [list(t) for t in itertools.product(*[range(n) for n in g["nvec"]])], "every tuple of the space"
        for turn in (False, True):
            want = np.array(g["true" if turn else "false"], np.int64)
            for dt in (torch.int64, torch.int32):
                got = transform_actions(torch.from_numpy(acts).to(dt), turn)
                assert got.dtype == dt and np.array_equal(got.numpy(), want), (name, turn)
            assert np.array_equal(PR.transform_table(acts, turn), want), (name, turn)
            assert np.array_equal(acts, np.array(g["actions"])), "the argument is not written to"
    rc = gold["robocup"]
    sides = {a[0]: t[2] for a, t in zip(rc["actions"], rc["false"])}
    assert sides == {0: 0, 1: -1, 2: -1, 3: 0, 4: 0}, "the reference's sides column maps both 1 and 2 to -1"


def _compiled(path, names, kind, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, kind) and n.name in names]
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


@pytest.mark.skipif(not os.path.exists(REF_UTILS), reason="the reference is not on this machine")
def test_the_recorded_results_and_transform_actions_are_the_references_function():
    import torch
    from dynenv_amd.policy import transform_actions
    ref = _compiled(REF_UTILS, {"transformActions"}, ast.FunctionDef, dict(torch=torch))["transformActions"]
    for name, g in _golden().items():
        acts = torch.tensor(g["actions"], dtype=torch.int64)
        for turn in (False, True):
            assert ref(acts, turn).tolist() == g["true" if turn else "false"], (name, turn)
    rng = np.random.default_rng(0)
    for width, hi in ((2, 3), (3, 5), (4, 16), (5, 4), (8, 2)):   # widths and values beyond the two environments'
        acts = torch.from_numpy(rng.integers(0, hi, (200, width)))
        for turn in (False, True):
            assert torch.equal(transform_actions(acts, turn), ref(acts, turn)), (width, turn)


def _reference_classes():
    """the reference's classes as its own file defines them, compiled from it (the package around it needs gym), with this package's
    spaces.Box for gym's"""
    import torch
    from dynenv_amd import spaces
    ns = dict(torch=torch, nn=torch.nn, F=torch.nn.functional, Box=spaces.Box, flatten=lambda l: list(itertools.chain.from_iterable(l)))
    return _compiled(REF_AC, {"ActorLayer", "ActorBlock", "CriticLayer", "CriticBlock"}, ast.ClassDef, ns)


@pytest.mark.skipif(not os.path.exists(REF_AC), reason="the reference is not on this machine")
@pytest.mark.parametrize("case", SPACES[:4], ids=str)
def test_forward_is_the_reference_actor_and_critic_bit_for_bit(case):
    import torch
    from dynenv_amd import GpuPolicyHead
    K, nvec, C = case
    ns = _reference_classes()
    torch.manual_seed(K)
    sp = PR.space(nvec, C)
    ref = torch.nn.ModuleDict({"actor": ns["ActorLayer"](K, sp.spaces), "critic": ns["CriticLayer"](K)})
    ours = GpuPolicyHead(K, sp)
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ours.state_dict().items()]
    sd = dict(ref.state_dict(), **{k: torch.from_numpy(v) for k, v in PR.make_params(K, nvec, C, seed=3).items()})
    ref.load_state_dict(sd, strict=True)
    ours.load_state_dict(ref.state_dict(), strict=True)
    for dtype in (torch.float32, torch.float64):
        ref, ours = ref.to(dtype), ours.to(dtype)
        x = torch.from_numpy(_feature(K, 4)).to(dtype)
        with torch.no_grad():
            want_p, want_v = ref["actor"](x), ref["critic"](x)
            got_p, got_v = ours(x)
        G = len(nvec)
        assert torch.equal(got_v, want_v) and got_v.dtype == dtype
        assert len(got_p) == G + (1 if C else 0) and all(torch.equal(a, b) for a, b in zip(got_p[:G], want_p[:G]))
        if C:   # the reference's flatten iterates over the Box block's [P, C] output: its rows follow the G logit tensors
            assert len(want_p) == G + P and torch.equal(got_p[G], torch.stack(want_p[G:]))
