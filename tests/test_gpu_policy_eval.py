"""The policy head over a stored rollout on the device, with its backward (csrc/policy_eval_kernels.hip through dynenv_policy_eval,
dynenv_policy_eval_backward and GpuPolicyHead.evaluate) against the numpy float64 statement tests/policy_eval_ref.py.  -m gpu.

Accuracy, the project's rule (test_gpu_icm_backward.py), per output tensor - the three outputs of the forward, the eight packed gradients
and d_features at the C ABI, every actor.* and critic.* parameter and `features` through the module: err_fused = max |x - g64| <=
4 * err_cpu_autocast.  g64 is the float64 statement (held to float64 autograd of the module's torch route by test_policy_eval_ref.py);
err_cpu_autocast is the same distance for the module's torch route run here on the CPU under torch.autocast("cpu", dtype), computed at
run time, independent of the code under test and of the device.  Every run prints both.  Every case runs with slope 0.1 and with slope
1.0: a 16-bit rounding of h_pre near zero flips LeakyReLU's derivative, in the yardstick as in the kernel; at slope 1 there is no kink
and Layer1's gradient is held to the tight yardstick too.
Exact checks take no tolerance: guard bands, every element written, the padding, repeatability, the bits of dynenv_policy_head, locality
of a row, exact scaling by 2^-12, zero upstream, NULL arguments, the clamp's status bit, a captured forward + backward.

The backward's tiling: a workgroup walks blocks of 64 rows of the T * P, the grid is capped at 256 workgroups.  CASES (T, P, K, groups,
AD): a single row; K = 128 with four groups; a block boundary plus one row (6 * 65 = 390 = 6 * 64 + 6 rows, blocks that straddle t);
eight groups, one of a single action; and 64 * 256 + 1 rows: workgroup 0 walks one block more than the rest, its last block of one row."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_eval_ref as ER  # noqa: E402
import policy_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 64, (3, 3), 2), (2, 17, 128, (5, 3, 3, 7), 4), (6, 65, 128, (5, 3, 3), 4), (1, 43, 64, (2, 2, 1, 2, 2, 2, 2, 2), 8),
         (1, ER.ROWS * ER.MAX_WORKGROUPS + 1, 64, (3, 3), 2)]
KINDS = ["bf16", "f16"]
SLOPES = [0.1, 1.0]
CODE = {"bf16": 1, "f16": 2}
FACTOR = 4.0
FWD = ("logp", "probs", "value")
OUT = ER.PACKED + ("dfeat",)
SHAPES = lambda T, P, K, G, N: dict(aw=(32, K), ab=(32,), w1=(K // 2, K), b1=(K // 2,), lnw=(K // 2,), lnb=(K // 2,), w2=(K // 2,), b2=(1,),  # noqa: E731
                                    dfeat=(T, P, K), logp=(T, G, P), probs=(T, P, N), value=(T, P), status=(1,))


def _tdtype(kind):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _module(K, groups, pr, kind="bf16", slope=0.1, **kw):
    from dynenv_amd import GpuPolicyHead
    m = PR.load(GpuPolicyHead(K, PR.space(groups), operand_dtype=_tdtype(kind), **kw), pr)
    m.critic.blocks.relu.negative_slope = slope
    return m


@functools.lru_cache(maxsize=None)
def _inputs(case):
    T, P, K, groups, AD = case
    return dict(ER.make_case(T, P, K, groups, AD, seed=31 * P + K + len(groups)), pr=PR.make_params(K, groups, seed=P + K))


@functools.lru_cache(maxsize=None)
def _g64(case, slope):
    """the float64 statement: the forward's three outputs and the backward's nine (computed once, never written to)"""
    T, P, K, groups, AD = case
    c = _inputs(case)
    logp, probs, value = ER.forward(c["features"], c["actions"], c["pr"], groups, slope)
    return dict(ER.backward(c["features"], c["actions"], c["pr"], groups, c["d_logp"], c["d_probs"], c["d_value"], slope), logp=logp, probs=probs, value=value)


def _torch_route(m, c, autocast=None):
    """evaluate + the case's upstream + backward through the torch route on m's device -> dict in the packed layouts, with the forward's"""
    import contextlib
    import torch
    dev = next(m.parameters()).device
    f = _t(c["features"]).to(dev).requires_grad_(True)
    ctx = torch.autocast(dev.type, dtype=autocast) if autocast is not None else contextlib.nullcontext()
    with ctx:
        ev = m.evaluate(f, _t(c["actions"]).to(dev))
    loss = (ev.log_probs.float() * _t(c["d_logp"]).to(dev)).sum() + (ev.probs.float() * _t(c["d_probs"]).to(dev)).sum() + \
        (ev.values.float() * _t(c["d_value"]).to(dev)).sum()
    loss.backward()
    named = {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()}
    K, groups = m.feature_size, tuple(m.nvec)
    return dict(ER.pack(named, K, groups), dfeat=f.grad.double().cpu().numpy(), logp=ev.log_probs.detach().double().cpu().numpy(),
                probs=ev.probs.detach().double().cpu().numpy(), value=ev.values.detach().double().cpu().numpy(), **named)


@functools.lru_cache(maxsize=None)
def _err_cpu(case, kind, slope):
    T, P, K, groups, AD = case
    c = _inputs(case)
    got = _torch_route(_module(K, groups, c["pr"], kind, slope), c, autocast=_tdtype(kind))
    want = _g64(case, slope)
    want = dict(want, **ER.by_name(want, groups))
    return {k: float(np.abs(got[k] - want[k]).max()) for k in want}


def _judge(what, got, case, kind, slope, keys):
    """print both errors of every tensor, then the rule"""
    groups = case[3]
    want, cpu = _g64(case, slope), _err_cpu(case, kind, slope)
    want = dict(want, **ER.by_name(want, groups), features=want["dfeat"])
    cpu = dict(cpu, features=cpu["dfeat"])
    bad = []
    for k in keys:
        err, scale = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()), float(np.abs(want[k]).max())
        print("%s %s slope %g %s %s: max %.3g err_fused %.3g | err_cpu_autocast %.3g" % (case, kind, slope, what, k, scale, err, cpu[k]))
        if not err <= FACTOR * cpu[k]:
            bad.append((k, err, cpu[k]))
    assert not bad, bad


def _dev_weights(pr, K, groups, kind):
    """the packed operands of dynenv_policy_t and the two transposed bf16 copies of dynenv_policy_bwd_t, on the device"""
    import torch
    from dynenv_amd import _capi
    N, dt = sum(groups), _tdtype(kind)
    w, b = PR.actor_rows(pr)
    aw, ab = np.zeros((32, K), np.float32), np.zeros(32, np.float32)
    aw[:N], ab[:N] = w[:N], b[:N]
    t = dict(aw=_t(aw).cuda().to(dt), ab=_t(ab).cuda(), w1=_t(pr[ER.CRITIC["w1"]]).cuda().to(dt))
    for k, w in (("aw_t", _t(aw).cuda().t().contiguous()), ("w1_t", _t(pr[ER.CRITIC["w1"]]).cuda().t().contiguous())):
        t[k] = w.to(torch.bfloat16)
        t[k + "_lo"] = (w - t[k].float()).to(torch.bfloat16)   # (the pairs' second halves: read with float16 only)
    for k in ("b1", "lnw", "lnb", "w2", "b2"):
        t[k] = _t(np.asarray(pr[ER.CRITIC[k]], np.float32).reshape(-1)).cuda()
    s = _capi.Policy()
    s.actor_w, s.actor_b, s.critic_w1, s.critic_b1 = (t[k].data_ptr() for k in ("aw", "ab", "w1", "b1"))
    s.critic_ln_w, s.critic_ln_b, s.critic_w2, s.critic_b2 = (t[k].data_ptr() for k in ("lnw", "lnb", "w2", "b2"))
    wt = _capi.PolicyBwd()
    wt.actor_w_t, wt.critic_w1_t, wt.actor_w_t_lo, wt.critic_w1_t_lo = (t[k].data_ptr() for k in ("aw_t", "w1_t", "aw_t_lo", "w1_t_lo"))
    return t, s, wt


class Call(object):
    """the arguments of one dynenv_policy_eval and one dynenv_policy_eval_backward call on the device, every output between guard bands
    and prefilled with a NaN pattern: forward() and backward() launch and nothing else; collect() synchronises, checks the bands and
    that every element was written -> dict of host arrays"""

    def __init__(self, case, kind, c, weights, slope=0.1, want_dfeat=True, want_dprobs=True, want_probs=True, scale=1.0):
        import torch
        from dynenv_amd import _capi
        from test_gpu_arranger_dtype import Guarded
        T, P, K, groups, AD = case
        self.case, self.kind, self.slope, self.weights = case, kind, slope, weights
        self.want = dict(dfeat=want_dfeat, probs=want_probs)
        self.want_dprobs = want_dprobs
        self.f, self.a = _t(np.asarray(c["features"], np.float32)).cuda(), _t(np.asarray(c["actions"], np.float32)).cuda()
        self.up = {k: _t(np.asarray(c[k], np.float32) * np.float32(scale)).cuda() for k in ("d_logp", "d_probs", "d_value")}
        self.shapes = SHAPES(T, P, K, len(groups), sum(groups))
        self.bufs = {k: Guarded(int(np.prod(s)), 4) for k, s in self.shapes.items()}
        self.bufs["status"].payload.zero_()   # (the kernels OR into it)
        need = C.c_uint64(0)
        assert _capi.load().dynenv_policy_eval_backward_workspace(T * P, K, C.byref(need)) == 0
        self.ws, self.ws_bytes = Guarded(need.value // 4, 4), need.value
        self.grad = _capi.PolicyGrad()
        for name, k in zip(("d_actor_w", "d_actor_b", "d_critic_w1", "d_critic_b1", "d_critic_ln_w", "d_critic_ln_b", "d_critic_w2", "d_critic_b2"), ER.PACKED):
            setattr(self.grad, name, self.bufs[k].ptr())
        self.ran = set()

    def _head(self):
        import torch
        T, P, K, groups, AD = self.case
        G, vp = len(groups), C.c_void_p
        _, w, _ = self.weights
        return (vp(self.f.data_ptr()), vp(self.a.data_ptr()), T, P, K, CODE[self.kind], C.byref(w), (C.c_int32 * G)(*groups), G, AD, self.slope, PR.EPS), \
            vp(torch.cuda.current_stream().cuda_stream)

    def forward(self):
        from dynenv_amd import _capi
        lib, vp = _capi.load(), C.c_void_p
        head, stream = self._head()
        rc = lib.dynenv_policy_eval(*head, vp(self.bufs["logp"].ptr()), vp(self.bufs["probs"].ptr()) if self.want["probs"] else None, vp(self.bufs["value"].ptr()),
                                    vp(self.bufs["status"].ptr()), stream)
        assert rc == 0, lib.dynenv_last_error()
        self.ran |= set(FWD)
        return self

    def backward(self):
        from dynenv_amd import _capi
        lib, vp = _capi.load(), C.c_void_p
        head, stream = self._head()
        _, _, wt = self.weights
        rc = lib.dynenv_policy_eval_backward(*head, vp(self.up["d_logp"].data_ptr()), vp(self.up["d_probs"].data_ptr()) if self.want_dprobs else None,
                                             vp(self.up["d_value"].data_ptr()), C.byref(wt), C.byref(self.grad), vp(self.bufs["dfeat"].ptr()) if self.want["dfeat"] else None,
                                             vp(self.ws.ptr()), self.ws_bytes, vp(self.bufs["status"].ptr()), stream)
        assert rc == 0, lib.dynenv_last_error()
        self.ran |= set(OUT)
        return self

    def collect(self):
        import torch
        torch.cuda.synchronize()
        if "aw" in self.ran:
            self.ws.check("workspace", True)   # (its bands; every slice is written whole)
        out = {}
        for k, b in self.bufs.items():
            written = k == "status" or (k in self.ran and self.want.get(k, True))
            pay = b.check(k, written).copy()
            if written:
                out[k] = pay.reshape(self.shapes[k])
        out["status"] = out["status"].view(np.int32)
        return out


def _run(case, kind, c, weights, forward=False, **kw):
    call = Call(case, kind, c, weights, **kw)
    if forward:
        call.forward()
    return call.backward().collect()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(a, b, keys):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _plus_zero(x):
    return not _bits(x).any()


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_c_abi_accuracy_every_element_written_and_the_padding(case, kind, slope):
    c = _inputs(case)
    T, P, K, groups, AD = case
    N = sum(groups)
    out = _run(case, kind, c, _dev_weights(c["pr"], K, groups, kind), forward=True, slope=slope)
    assert all(np.isfinite(out[k]).all() for k in OUT + FWD) and out["status"][0] == 0
    _judge("C ABI", out, case, kind, slope, FWD + OUT)
    assert _plus_zero(out["aw"][N:]) and _plus_zero(out["ab"][N:]), "the padding of the actor's gradients is +0"
    start = 0
    for n in groups:
        if n == 1:
            assert _plus_zero(out["aw"][start]) and _plus_zero(out["ab"][start:start + 1]), "a single action's Linear has the gradient 0"
        start += n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_has_the_bits_of_the_policy_head_for_the_actions_it_drew(case, kind):
    """dynenv_policy_head on the T * P rows, then dynenv_policy_eval on the actions it drew: log_probs, probs and value bit for bit"""
    import torch
    T, P, K, groups, AD = case
    c = _inputs(case)
    m = _module(K, groups, c["pr"], kind).cuda().requires_grad_(False)
    m.reseed(5, 7)
    f = _t(c["features"]).cuda()
    act = m.act(f.view(T * P, K))
    assert m.last_route == "fused" and AD >= len(groups)
    stored = torch.zeros((T, AD, P), dtype=torch.float32, device="cuda")
    stored[:, :len(groups)] = act.actions.view(T, P, -1)[:, :, :len(groups)].permute(0, 2, 1).float()
    ev = m.evaluate(f, stored)
    assert m.last_eval_route == "fused" and int(m.eval_status) == 0
    bits = lambda x: x.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(ev.values), bits(act.value.view(T, P)))
    assert torch.equal(bits(ev.probs), bits(torch.cat(act.probs, dim=1).view(T, P, -1)))
    assert torch.equal(bits(ev.log_probs), bits(act.log_probs.view(T, P, -1).permute(0, 2, 1)))
    # the C ABI with the same weights, probs_dev NULL: the other two unchanged
    c2 = dict(c, actions=stored.cpu().numpy())
    weights = _dev_weights(c["pr"], K, groups, kind)
    full, bare = Call(case, kind, c2, weights).forward().collect(), Call(case, kind, c2, weights, want_probs=False).forward().collect()
    assert _same(full, bare, ("logp", "value", "status")) and "probs" not in bare
    assert np.array_equal(_bits(full["logp"]), _bits(ev.log_probs.cpu().numpy())) and np.array_equal(_bits(full["probs"]), _bits(ev.probs.cpu().numpy()))


EXACT = [(CASES[1], "bf16"), (CASES[2], "f16"), (CASES[3], "bf16"), (CASES[4], "f16")]


@pytest.mark.parametrize("case, kind", EXACT, ids=str)
def test_exact_properties(case, kind):
    c = _inputs(case)
    T, P, K, groups, AD = case
    weights = _dev_weights(c["pr"], K, groups, kind)
    run = functools.partial(_run, case, kind, weights=weights)
    base = run(c)
    assert _same(base, run(c), OUT + ("status",)), "two calls give the same bits"
    assert _same(base, run(c, want_dfeat=False), ER.PACKED + ("status",)), "d_features_dev NULL leaves the weight gradients alone"
    # d_probs_dev NULL is d_probs of zeros
    zeros = dict(c, d_probs=np.zeros_like(c["d_probs"]))
    assert _same(run(zeros), run(c, want_dprobs=False), OUT + ("status",))
    # scaling: every output by exactly 2^-12
    small = run(c, scale=2.0 ** -12)
    for k in OUT:
        assert np.array_equal(_bits(small[k]), _bits(base[k] * np.float32(2.0 ** -12))), k
    # zero upstream: +0 everywhere
    nothing = run(c, scale=0.0)
    assert all(_plus_zero(nothing[k]) for k in OUT)
    # locality: another row's feature and upstream changed, this row's d_features unchanged
    if T * P > 1:
        other = {k: v.copy() for k, v in c.items() if k != "pr"}
        t1, p1 = T - 1, P // 2
        keep = np.ones((T, P), bool)
        keep[t1, p1] = False
        rng = np.random.default_rng(2)
        other["features"][t1, p1] = rng.standard_normal(K)
        other["d_logp"][t1, :, p1] += 1.0
        other["d_value"][t1, p1] -= 2.0
        other["d_probs"][t1, p1] += 0.5
        moved = run(other)
        assert np.array_equal(_bits(moved["dfeat"][keep]), _bits(base["dfeat"][keep])) and not np.array_equal(moved["dfeat"][t1, p1], base["dfeat"][t1, p1])
        assert not _same(moved, base, ("aw", "w1"))
    # a clamped action sets bit 0 and takes the nearest action's gradients
    bad, near = c["actions"].copy(), c["actions"].copy()
    bad[0, 0, 0], near[0, 0, 0] = groups[0] + 3.0, groups[0] - 1.0
    bad[T - 1, len(groups) - 1, P - 1], near[T - 1, len(groups) - 1, P - 1] = -1.0, 0.0
    clamped, nearest = run(dict(c, actions=bad), forward=True), run(dict(c, actions=near), forward=True)
    assert clamped["status"][0] == 1 and nearest["status"][0] == 0 and _same(clamped, nearest, OUT + FWD)


def test_a_captured_forward_and_backward_replayed_on_new_contents_equal_eager_calls():
    import torch
    case, kind = CASES[2], "bf16"
    T, P, K, groups, AD = case
    c = _inputs(case)
    weights = _dev_weights(c["pr"], K, groups, kind)
    call = Call(case, kind, c, weights)
    call.forward().backward()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.forward().backward()
    other = ER.make_case(T, P, K, groups, AD, seed=77)
    call.f.copy_(_t(other["features"]).cuda())
    call.a.copy_(_t(other["actions"]).cuda())
    for k, v in call.up.items():
        v.copy_(_t(other[k]).cuda())
    graph.replay()
    replayed = call.collect()
    eager = _run(case, kind, other, weights, forward=True)
    assert _same(replayed, eager, OUT + FWD + ("status",))
    assert not _same(_run(case, kind, c, weights), eager, ("dfeat",)), "the second contents are others"


# ---- the module
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("kind", KINDS)
def test_module_routes_forward_bits_and_gradients(kind, slope):
    import torch
    T, P, K, groups, AD = case = CASES[2]
    c = _inputs(case)
    m = _module(K, groups, c["pr"], kind, slope, fused_backward=True).cuda()
    f, a = _t(c["features"]).cuda().requires_grad_(True), _t(c["actions"]).cuda()
    with torch.no_grad():
        plain = m.evaluate(f, a)
    assert m.last_eval_route == "fused"
    ev = m.evaluate(f, a)
    assert m.last_eval_route == "fused (backward)" and int(m.eval_status) == 0
    for k in ("log_probs", "probs", "values"):
        assert getattr(ev, k).grad_fn is not None and torch.equal(getattr(ev, k).detach().view(torch.int32), getattr(plain, k).view(torch.int32)), k
    up = {k: _t(c[k]).cuda() for k in ("d_logp", "d_probs", "d_value")}
    ((ev.log_probs * up["d_logp"]).sum() + (ev.probs * up["d_probs"]).sum() + (ev.values * up["d_value"]).sum()).backward()
    got = {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    got["features"] = f.grad.double().cpu().numpy()
    names = ER.names(groups)
    assert sorted(k for k in got if k != "features") == sorted(names), "exactly the discrete groups and the critic receive a gradient"
    _judge("module", got, case, kind, slope, names + ["features"])
    # the torch route on the device, float32, under the same rule (it is the route the fused one stands in for)
    twin = _module(K, groups, c["pr"], kind, slope).cuda()
    ref = _torch_route(twin, c)
    assert twin.last_eval_route == "torch"
    _judge("torch route on the device", dict(ref, features=ref["dfeat"]), case, kind, slope, names + ["features"])
    # features that want no gradient and probs that nobody asked for: the parameters' gradients of log_probs and values are the same bits
    m2 = _module(K, groups, c["pr"], kind, slope, fused_backward=True).cuda()
    m3 = _module(K, groups, c["pr"], kind, slope, fused_backward=True).cuda()
    grads = []
    for mod, feat, want_probs in ((m2, f.detach(), True), (m3, f.detach().clone().requires_grad_(True), False)):
        e = mod.evaluate(feat, a, want_probs=want_probs)
        assert mod.last_eval_route == "fused (backward)" and (e.probs is None) == (not want_probs)
        ((e.log_probs * up["d_logp"]).sum() + (e.values * up["d_value"]).sum()).backward()
        grads.append([p.grad for p in mod._eval_params()])
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*grads))


def test_module_default_is_the_torch_route_and_every_fallback_is_named(monkeypatch):
    import torch
    from dynenv_amd import GpuPolicyHead
    T, P, K, groups, AD = 2, 9, 64, (3, 3), 2
    pr = PR.make_params(K, groups, seed=1)
    c = ER.make_case(T, P, K, groups, AD, seed=2)
    f, a = _t(c["features"]).cuda(), _t(c["actions"]).cuda()
    m = _module(K, groups, pr).cuda()
    assert m.fused_backward is False and m.evaluate(f, a).values.grad_fn is not None and m.last_eval_route == "torch"
    on = _module(K, groups, pr, fused_backward=True).cuda()
    assert on.evaluate(f, a).values.grad_fn is not None and on.last_eval_route == "fused (backward)"
    with torch.no_grad():
        on.evaluate(f, a)
    assert on.last_eval_route == "fused"

    def falls_back(mod, why, *args):
        ev = mod.evaluate(*args)
        assert mod.last_eval_route.startswith("torch (fallback: " + why), mod.last_eval_route
        loss = ev.log_probs.sum() + ev.values.sum() + (ev.probs ** 2).sum()
        assert bool(torch.isfinite(loss)) and loss.grad_fn is not None
        loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in mod._eval_params())
    monkeypatch.setenv("DYNENV_POLICY_FUSED", "0")
    falls_back(on, "DYNENV_POLICY_FUSED=0", f, a)
    monkeypatch.delenv("DYNENV_POLICY_FUSED")
    falls_back(GpuPolicyHead(256, PR.space(groups), fused_backward=True, device="cuda"), "K = 256", torch.randn((T, P, 256), device="cuda"), a)
    falls_back(GpuPolicyHead(96, PR.space(groups), fused_backward=True, device="cuda"), "K = 96", torch.randn((T, P, 96), device="cuda"), a)
    box = GpuPolicyHead(K, PR.space(groups, 1), fused_backward=True, device="cuda")
    a4 = torch.zeros((T, 3, P), device="cuda")
    falls_back(box, "a Box block", f, a4)
    assert all(p.grad is None for p in box.actor.blocks[-1].parameters()), "the Box block's parameters get no gradient"
    falls_back(_module(K, groups, pr, fused_backward=True), "features that are not on the device", f.cpu(), a.cpu())
    with torch.no_grad():
        box.evaluate(f, a4)
    assert box.last_eval_route == "torch (fallback: a Box block)"


def test_a_graph_collected_rollout_trains_the_actor_and_the_critic():
    """Driving, 4 environments, T = 3, graph=True: collect() leaves buffers without a history; evaluate + a2c_loss(evaluation=) + backward"""
    import torch
    from dynenv_amd import GpuRollout
    from test_gpu_rollout import _stack
    E, F, T = 4, 64, 3
    envs, nets, pols, sts = _stack(E, F, T)
    st, pol = sts[0], pols[0]
    pol.requires_grad_(True)
    pol.fused_backward = True
    ro = GpuRollout(envs[0], nets[0], pol, st, graph=True)
    final_value = ro.collect()
    assert ro.graph is not None and st.log_probs.grad_fn is None and st.values.grad_fn is None
    ev = pol.evaluate(st.features[:-1], st.actions)
    assert pol.last_eval_route == "fused (backward)" and int(pol.eval_status) == 0
    bits = lambda x: x.detach().contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(ev.values), bits(st.values)) and torch.equal(bits(ev.log_probs), bits(st.log_probs)) and torch.equal(bits(ev.probs), bits(st.probs))
    st.a2c_loss(final_value, evaluation=ev).loss.backward()
    got = {}
    for k, p in pol.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        got[k] = p.grad.double().cpu().numpy()
    assert any(g.any() for g in got.values())
    # the torch route's gradients of the same loss, float32 on the device, and the CPU autocast yardstick against float64
    def grads(mod, dev, dtype=torch.float32, autocast=None):
        import contextlib
        mod = mod.to(dev).to(dtype)
        mod.fused_backward = False
        mod.zero_grad(set_to_none=True)
        ctx = torch.autocast("cpu", dtype=autocast) if autocast is not None else contextlib.nullcontext()
        with ctx:
            e = mod.evaluate(st.features[:-1].to(dev).to(dtype), st.actions.to(dev).to(dtype))
        e = type(e)(e.log_probs.to(dtype), e.probs.to(dtype), e.values.to(dtype))
        twin = type(st)(T, E, st.num_players, st.action_cols, st.groups, F, n_probs=st.n_probs, device=dev)
        for name, b in st.buffers().items():
            getattr(twin, name).copy_(b)
        twin.rewards, twin.values, twin.dones = twin.rewards.to(dtype), twin.values.to(dtype), twin.dones.to(dtype)
        twin.a2c_loss(final_value.to(dev).to(dtype), evaluation=e).loss.backward()
        return {k: p.grad.double().cpu().numpy() for k, p in mod.named_parameters()}
    def clone():
        from dynenv_amd import GpuPolicyHead
        twin = GpuPolicyHead(F, envs[0].action_space)
        twin.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()}, strict=True)
        return twin
    on_device = grads(clone(), "cuda")
    g64 = grads(clone(), "cpu", torch.float64)
    cast = grads(clone(), "cpu", autocast=torch.bfloat16)
    bad = []
    for k in got:
        err, err_t, cpu = (float(np.abs(x[k] - g64[k]).max()) for x in (got, on_device, cast))
        print("rollout %s: max %.3g err_fused %.3g err_torch_device %.3g | err_cpu_autocast %.3g" % (k, float(np.abs(g64[k]).max()), err, err_t, cpu))
        if not err <= FACTOR * cpu:
            bad.append((k, err, cpu))
    assert not bad, bad
    for e in envs:
        e.close()
