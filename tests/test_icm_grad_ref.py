"""The float64 statement of the curiosity losses' backward (tests/icm_grad_ref.py) against torch float64 autograd through GpuICM's torch
route - every pred_net parameter and the features, at the shapes of test_gpu_icm_backward.py, with a random mask, without a mask and
with nobody active - and, where the reference is present, against the reference's own ICMNet.  Required: relative 1e-10 of each
tensor's largest entry."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icm_grad_ref as GR  # noqa: E402
import icm_ref as IR  # noqa: E402

CASES = [(1, 1, 64, (3, 3), 2), (2, 17, 128, (5, 3, 3, 7), 4), (6, 65, 128, (5, 3, 3), 4), (1, 43, 64, (2, 2, 1, 2, 2, 2, 2, 2), 8), (3, 130, 256, (16, 16), 2)]
COEFFS = dict(forward_coeff=0.2, icm_beta=0.8)
REL = 1e-10


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _autograd(module, features, actions, finished):
    """loss.backward() through `module` in float64 -> dict name -> gradient (None kept), with "features" """
    import torch
    f = _t(features, torch.float64).requires_grad_(True)
    with IR.default_dtype(torch.float64):
        out = module(f, _t(actions, torch.float64), None if finished is None else _t(finished))
    out.loss.backward()
    got = {k: (None if p.grad is None else p.grad.numpy()) for k, p in module.named_parameters()}
    got["features"] = f.grad.numpy()
    return got


def _compare(want, got, what):
    for k, w in want.items():
        scale = np.abs(w).max()
        err = np.abs(got[k] - w).max()
        assert err <= REL * scale, (what, k, err, scale)
    for k, g in got.items():
        if k not in want:
            assert g is None or not g.any(), (what, k)


@pytest.mark.parametrize("slope", [0.1, 1.0])
@pytest.mark.parametrize("mask", ["random", "none", "null", "all", "one"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_statement_equals_float64_autograd_through_the_torch_route(case, mask, slope):
    from dynenv_amd import GpuICM
    T, P, K, groups, AD = case
    pr = IR.make_params(K, groups, T, seed=P + K)
    c = IR.make_case(T, P, K, groups, AD=AD, seed=7 * P + K, mask="none" if mask == "null" else mask)
    finished = None if mask == "null" else c["finished"]
    m = IR.load(GpuICM(K, groups, T, **COEFFS).double(), pr)
    for net in [m.pred_net.fwd_net] + list(m.long_horizon_fwd_net.fwd_nets):
        net.relu.negative_slope = slope
    got = _autograd(m, c["features"], c["actions"], finished)
    assert m.last_route == "torch"
    want = GR.grads(c["features"], c["actions"], finished, pr, groups, s_f=COEFFS["forward_coeff"], s_i=COEFFS["icm_beta"], slope=slope)
    assert list(want) == GR.names(groups) + ["features"]
    _compare(want, got, (case, mask, slope))
    n = T * P if finished is None else int((~finished).sum())
    if n == 0:
        assert all(not g.any() for g in want.values())
    else:
        single = [GR.INV % g for g, size in enumerate(groups) if size == 1]
        for k, w in want.items():   # a gradient that is all zero checks nothing: only a single action's Linear has one
            assert bool(w.any()) != any(k.startswith(s + ".") for s in single), k
    packed = GR.pack(want, K, groups)
    assert list(packed) == list(GR.PACKED) and not packed["w1"][GR.HIDDEN:].any() and not packed["inv_w"][sum(groups):].any()


@pytest.mark.parametrize("case", CASES[:3], ids=str)
def test_statement_equals_the_reference_icmnet(case):
    """(where the reference is present; elsewhere there is nothing to hold the statement to)"""
    import torch
    if not IR.have_reference():
        return
    T, P, K, groups, AD = case
    pr = IR.make_params(K, groups, T, seed=P + K)
    c = IR.make_case(T, P, K, groups, seed=7 * P + K)   # (the reference reads every action column: AD = G)
    ns = IR.reference_classes()
    ref = IR.reference_net(ns, K, groups, T, P, pr, COEFFS["forward_coeff"], COEFFS["icm_beta"], 0.5, False, torch.float64)
    got = _autograd(ref, c["features"], c["actions"], c["finished"])
    want = GR.grads(c["features"], c["actions"], c["finished"], pr, groups, s_f=COEFFS["forward_coeff"], s_i=COEFFS["icm_beta"])
    _compare(want, got, case)
