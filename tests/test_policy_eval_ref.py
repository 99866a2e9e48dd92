"""tests/policy_eval_ref.py - the numpy float64 statement of the policy head over a stored rollout and of its backward, which the GPU
tests of dynenv_policy_eval / dynenv_policy_eval_backward compare against - held to float64 autograd of GpuPolicyHead.evaluate's torch
route on the CPU; that route held to the reference's own ActorLayer and CriticLayer with Categorical(probs).log_prob on given actions,
where the reference is on this machine; the clamp's zero gradient; a group of one action.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_eval_ref as ER  # noqa: E402
import policy_ref as PR  # noqa: E402

# (T, P, K, groups, AD): the GPU tests' small cases and K = 256, which only the torch route takes
CASES = [(1, 1, 64, (3, 3), 2), (2, 17, 128, (5, 3, 3, 7), 4), (3, 9, 128, (5, 3, 3), 4), (1, 43, 64, (2, 2, 1, 2, 2, 2, 2, 2), 8), (2, 5, 256, (16, 16), 2)]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _head(K, groups, pr, slope=0.1, dtype=None, **kw):
    from dynenv_amd import GpuPolicyHead
    m = PR.load(GpuPolicyHead(K, PR.space(groups), **kw), pr, dtype)
    m.critic.blocks.relu.negative_slope = slope
    return m


def _autograd(m, c, with_probs=True):
    """sum of the three outputs against the case's upstream, backward -> (PolicyEval, {name: float64 gradient}, with "features")"""
    dt = next(m.parameters()).dtype
    f = _t(c["features"]).to(dt).requires_grad_(True)
    ev = m.evaluate(f, _t(c["actions"]).to(dt))
    assert m.last_eval_route == "torch"
    loss = (ev.log_probs * _t(c["d_logp"]).to(dt)).sum() + (ev.values * _t(c["d_value"]).to(dt)).sum()
    if with_probs:
        loss = loss + (ev.probs * _t(c["d_probs"]).to(dt)).sum()
    loss.backward()
    got = {k: p.grad.double().numpy() for k, p in m.named_parameters()}
    got["features"] = f.grad.double().numpy()
    return ev, got


@pytest.mark.parametrize("slope", [0.1, 1.0])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_statements_are_float64_autograd_of_the_torch_route(case, slope):
    T, P, K, groups, AD = case
    pr = PR.make_params(K, groups, seed=P)
    c = ER.make_case(T, P, K, groups, AD, seed=K + P)
    ev, got = _autograd(_head(K, groups, pr, slope, dtype=__import__("torch").float64), c)
    logp, probs, values = ER.forward(c["features"], c["actions"], pr, groups, slope)
    for name, a, b in (("log_probs", ev.log_probs, logp), ("probs", ev.probs, probs), ("values", ev.values, values)):
        assert tuple(a.shape) == b.shape and np.allclose(a.detach().numpy(), b, rtol=1e-10, atol=1e-12), name
    want = ER.backward(c["features"], c["actions"], pr, groups, c["d_logp"], c["d_probs"], c["d_value"], slope)
    named = ER.by_name(want, groups)
    assert sorted(named) == sorted(ER.names(groups)) == sorted(k for k in got if k != "features")
    for k, v in named.items():
        assert got[k].shape == v.shape and np.allclose(got[k], v, rtol=1e-9, atol=1e-11), k
    assert np.allclose(got["features"], want["dfeat"], rtol=1e-9, atol=1e-11)
    N = sum(groups)
    assert not want["aw"][N:].any() and not want["ab"][N:].any(), "the padding of the actor's rows"
    back = ER.pack(named, K, groups)
    assert all(np.array_equal(back[k], want[k]) for k in ER.PACKED), "pack inverts by_name"
    # d_probs None is d_probs of zeros
    none = ER.backward(c["features"], c["actions"], pr, groups, c["d_logp"], None, c["d_value"], slope)
    _, got0 = _autograd(_head(K, groups, pr, slope, dtype=__import__("torch").float64), c, with_probs=False)
    assert all(np.allclose(got0[k], v, rtol=1e-9, atol=1e-11) for k, v in ER.by_name(none, groups).items())


def test_a_group_of_one_action_gives_exactly_zero():
    T, P, K, groups, AD = CASES[3]
    pr = PR.make_params(K, groups, seed=P)
    c = ER.make_case(T, P, K, groups, AD, seed=5)
    want = ER.backward(c["features"], c["actions"], pr, groups, c["d_logp"], c["d_probs"], c["d_value"])
    at = sum(groups[:2])
    assert groups[2] == 1 and not want["aw"][at].any() and want["ab"][at] == 0.0
    _, got = _autograd(_head(K, groups, pr), c)
    assert not got["actor.blocks.0.Layer.2.weight"].any() and not got["actor.blocks.0.Layer.2.bias"].any()
    assert got["actor.blocks.0.Layer.1.weight"].any()


def test_the_clamp_has_no_gradient_where_it_binds():
    """a probability forced beyond 1 - eps32: log_prob is log(1 - eps32) and d_logp goes nowhere"""
    import torch
    T, P, K, groups, AD = 1, 6, 64, (3, 3), 2
    pr = PR.make_params(K, groups, seed=1)
    pr["actor.blocks.0.Layer.0.bias"] = np.array([40.0, 0.0, 0.0], np.float32)
    c = ER.make_case(T, P, K, groups, AD, seed=2)
    c["actions"][:, 0] = 0
    c["d_probs"][:] = 0
    c["d_value"][:] = 0
    logp, probs, _ = ER.forward(c["features"], c["actions"], pr, groups)
    assert (probs[:, :, 0] > 1 - PR.EPS32).all() and np.allclose(logp[:, 0], np.log(1 - PR.EPS32), rtol=0, atol=1e-15)
    want = ER.backward(c["features"], c["actions"], pr, groups, c["d_logp"], c["d_probs"], c["d_value"])
    assert not want["aw"][:3].any() and not want["ab"][:3].any() and want["aw"][3:6].any()
    ev, got = _autograd(_head(K, groups, pr), c)
    assert torch.equal(ev.log_probs[:, 0], torch.full((T, P), float(np.log(np.float32(1) - np.float32(PR.EPS32))), dtype=torch.float32))
    assert not got["actor.blocks.0.Layer.0.weight"].any() and not got["actor.blocks.0.Layer.0.bias"].any()
    assert got["actor.blocks.0.Layer.1.weight"].any()
    # an action on the other side of the clamp: a probability below eps32
    c["actions"][:, 0] = 1
    want = ER.backward(c["features"], c["actions"], pr, groups, c["d_logp"], c["d_probs"], c["d_value"])
    assert not want["aw"][:3].any()
    _, got = _autograd(_head(K, groups, pr), c)
    assert not got["actor.blocks.0.Layer.0.weight"].any()


def test_an_action_outside_its_group_is_clamped_and_sets_the_status_bit():
    import torch
    T, P, K, groups, AD = 2, 5, 64, (3, 3), 2
    pr = PR.make_params(K, groups, seed=1)
    c = ER.make_case(T, P, K, groups, AD, seed=3)
    m = _head(K, groups, pr)
    with torch.no_grad():
        inside = m.evaluate(_t(c["features"]), _t(c["actions"]))
    assert int(m.eval_status) == 0 and m.last_eval_route.startswith("torch (fallback: features that are not on the device")
    bad = c["actions"].copy()
    bad[1, 0, 2], bad[0, 1, 4] = 7.0, -2.0
    near = c["actions"].copy()
    near[1, 0, 2], near[0, 1, 4] = 2.0, 0.0
    with torch.no_grad():
        got, want = m.evaluate(_t(c["features"]), _t(bad)), _head(K, groups, pr).evaluate(_t(c["features"]), _t(near))
    assert int(m.eval_status) == 1 and torch.equal(got.log_probs, want.log_probs) and torch.equal(got.probs, inside.probs)
    assert ER.indices(bad, groups)[1] and not ER.indices(near, groups)[1] and np.array_equal(ER.indices(bad, groups)[0], ER.indices(near, groups)[0])


from test_policy_ref import REF_AC, _reference_classes  # noqa: E402  (the loader of the reference's classes, and where they live)


@pytest.mark.skipif(not os.path.exists(REF_AC), reason="the reference is not on this machine")
@pytest.mark.parametrize("case", CASES[:4], ids=str)
def test_the_torch_route_is_the_reference_actor_critic_and_categorical_log_prob(case):
    import torch
    from torch.distributions import Categorical
    T, P, K, groups, AD = case
    ns = _reference_classes()
    pr = PR.make_params(K, groups, seed=P)
    ref = PR.load(torch.nn.ModuleDict({"actor": ns["ActorLayer"](K, PR.space(groups).spaces), "critic": ns["CriticLayer"](K)}), pr)
    m = _head(K, groups, pr)
    c = ER.make_case(T, P, K, groups, AD, seed=K)
    f, a = _t(c["features"]), _t(c["actions"])
    with torch.no_grad():
        ev = m.evaluate(f, a)
        policies, value = ref["actor"](f), ref["critic"](f)   # (on the same [T, P, K] tensor: the same matrix products)
        probs = [torch.softmax(l, dim=-1) for l in policies]
        assert torch.equal(ev.values, value.squeeze(-1))
        assert torch.equal(ev.probs, torch.cat(probs, dim=2))
        for g, p in enumerate(probs):
            # Categorical divides its probs by their sum first, which is 1 to within n_g roundings: 16 * 2^-24 < 1e-6 in the logarithm
            assert torch.allclose(ev.log_probs[:, g], Categorical(p).log_prob(a[:, g].long()), rtol=0, atol=1e-6), g
