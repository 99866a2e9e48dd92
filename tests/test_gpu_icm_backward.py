"""The fused backward of the curiosity losses on the device (csrc/icm_backward_kernels.hip through dynenv_icm_backward and
GpuICM(fused_backward=True)) against float64 autograd on the CPU.  -m gpu.

Accuracy, the project's rule (test_gpu_icm.py), per gradient tensor - the seven packed tensors and d_features at the C ABI, every
pred_net parameter and `features` through the module: err_fused = max |x - g64| <= 4 * err_cpu_autocast.  g64 is the autograd of the
module's float64 twin on the CPU (held to the numpy statement tests/icm_grad_ref.py by test_icm_grad_ref.py); err_cpu_autocast is the
same distance for the module's torch route run here on the CPU under torch.autocast("cpu", dtype), computed at run time, independent of
the code under test and of the device.  Every run prints both.  Every case runs with slope 0.1 and with slope 1.0: a 16-bit rounding of
h_pre near zero flips LeakyReLU's derivative for a whole row of fc1.weight's gradient, in the yardstick as in the kernel; at slope 1
there is no kink and fc1's gradient is held to the tight yardstick too.  A single action's Linear: the yardstick's error is 0, so the
rule demands exactly 0.
Exact checks take no tolerance: guard bands, every element written, repeatability, masks, linearity and exact scaling in upstream,
locality of d_features, the clamp, a captured call.

The kernel's tiling: a workgroup walks blocks of 32 players, the grid is capped at 256 workgroups (DYNENV_ICM_BWD_MAX_WORKGROUPS).
CASES (T, P, K, groups, AD): test_gpu_icm.py's with K <= 128 (K = 256 is not taken: DYNENV_ERR_UNSUPPORTED, the module names the
fallback), and P = 64 * 256 + 1 at T = 1, K = 64: workgroup 0 walks three blocks, the last of one player."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icm_grad_ref as GR  # noqa: E402
import icm_ref as IR  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 256
CASES = [(1, 1, 64, (3, 3), 2), (2, 17, 128, (5, 3, 3, 7), 4), (6, 65, 128, (5, 3, 3), 4), (1, 43, 64, (2, 2, 1, 2, 2, 2, 2, 2), 8), (1, 64 * CAP + 1, 64, (3, 3), 2)]
KINDS = ["bf16", "f16"]
SLOPES = [0.1, 1.0]
CODE = {"bf16": 1, "f16": 2}
FACTOR = 4.0
COEFFS = dict(forward_coeff=0.2, icm_beta=0.8)
UPSTREAM = (COEFFS["forward_coeff"], COEFFS["icm_beta"])   # what autograd hands the kernel for `loss`: one reference serves both levels
OUT = GR.PACKED + ("dfeat",)


def _tdtype(kind):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _set_slope(m, slope):
    for net in [m.pred_net.fwd_net] + list(m.long_horizon_fwd_net.fwd_nets):
        net.relu.negative_slope = slope
    return m


def _module(K, groups, T, pr, kind="bf16", slope=0.1, **kw):
    from dynenv_amd import GpuICM
    return _set_slope(IR.load(GpuICM(K, groups, T, w_dtype=_tdtype(kind), **dict(COEFFS, **kw)), pr), slope)


def _cpu_grads(m, c, autocast=None):
    """loss.backward() on the CPU through the torch route -> dict name -> float64 array, with "features" """
    import contextlib
    import torch
    dt = next(m.parameters()).dtype
    f = _t(c["features"]).to(dt).requires_grad_(True)
    ctx = torch.autocast("cpu", dtype=autocast) if autocast is not None else contextlib.nullcontext()
    with ctx:
        out = m(f, _t(c["actions"]).to(dt), _t(c["finished"]))
    assert m.last_route == "torch"
    out.loss.backward()
    got = {k: p.grad.double().numpy() for k, p in m.named_parameters() if k.startswith("pred_net.")}
    got["features"] = f.grad.double().numpy()
    return got


def _with_packed(g, K, groups):
    return dict(GR.pack(g, K, groups), dfeat=g["features"], **g)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    T, P, K, groups, AD = case
    pr = IR.make_params(K, groups, T, seed=P + K)
    return dict(IR.make_case(T, P, K, groups, AD=AD, seed=31 * P + K + len(groups)), case=case, pr=pr)


@functools.lru_cache(maxsize=None)
def _g64(case, slope):
    """the float64 twin's autograd, by parameter name and in the packed layouts (computed once, never written to)"""
    T, P, K, groups, AD = case
    c = _inputs(case)
    return _with_packed(_cpu_grads(_module(K, groups, T, c["pr"], slope=slope).double(), c), K, groups)


@functools.lru_cache(maxsize=None)
def _err_cpu(case, kind, slope):
    T, P, K, groups, AD = case
    c = _inputs(case)
    got = _with_packed(_cpu_grads(_module(K, groups, T, c["pr"], kind, slope), c, autocast=_tdtype(kind)), K, groups)
    want = _g64(case, slope)
    return {k: float(np.abs(got[k] - want[k]).max()) for k in want}


def _judge(what, got, case, kind, slope, keys):
    """print both errors of every tensor, then the rule"""
    want, cpu = _g64(case, slope), _err_cpu(case, kind, slope)
    bad = []
    for k in keys:
        err, scale = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()), float(np.abs(want[k]).max())
        print("%s %s slope %g %s %s: max %.3g err_fused %.3g | err_cpu_autocast %.3g" % (case, kind, slope, what, k, scale, err, cpu[k]))
        if not err <= FACTOR * cpu[k]:
            bad.append((k, err, cpu[k]))
    assert not bad, bad


def _dev_weights(pr, K, groups, kind):
    """test_gpu_icm.py's packed operands and the three transposed copies of dynenv_icm_bwd_t"""
    from dynenv_amd import _capi
    from test_gpu_icm import _dev_weights as forward_weights
    t, w = forward_weights(pr, K, groups, kind)
    t.update(w2_t=t["w2"].t().contiguous(), w1_t=t["w1"].t().contiguous(), iw_t=t["iw"].t().contiguous())
    wt = _capi.IcmBwd()
    wt.fwd_w2_t, wt.fwd_w1_t, wt.inv_w_t = (t[k].data_ptr() for k in ("w2_t", "w1_t", "iw_t"))
    return t, w, wt


class Call(object):
    """the arguments of one dynenv_icm_backward call on the device, every output between guard bands of NaN: launch() launches and
    nothing else; collect() synchronises, checks the bands and that every element was written -> dict of host arrays"""

    def __init__(self, case, kind, features, actions, finished, weights, upstream=UPSTREAM, slope=0.1, want_dfeat=True, count=None):
        import torch
        from dynenv_amd import _capi
        from test_gpu_arranger_dtype import Guarded
        _, _, K, groups, _ = case
        self.K, self.groups, self.kind, self.slope, self.weights, self.want_dfeat = K, groups, kind, slope, weights, want_dfeat
        self.T, self.P, self.AD, N = features.shape[0] - 1, features.shape[1], actions.shape[1], sum(groups)
        self.f, self.a = _t(np.asarray(features, np.float32)).cuda(), _t(np.asarray(actions, np.float32)).cuda()
        self.fin = None if finished is None else _t(np.asarray(finished, np.uint8)).cuda()
        n = self.T * self.P if finished is None else int((~np.asarray(finished, bool)).sum())
        self.count = torch.tensor([0.5, 0.25, float(n) if count is None else count], dtype=torch.float32, device="cuda")
        self.up = torch.tensor(upstream, dtype=torch.float32, device="cuda")
        sizes = dict(w1=160 * K, act=N * 160, b1=160, w2=K * 160, b2=K, inv_w=32 * 2 * K, inv_b=32, dfeat=(self.T + 1) * self.P * K, status=1)
        self.shapes = dict(w1=(160, K), act=(N, 160), w2=(K, 160), inv_w=(32, 2 * K), dfeat=(self.T + 1, self.P, K))
        self.bufs = {k: Guarded(v, 4) for k, v in sizes.items()}
        self.bufs["status"].payload.zero_()   # (the kernel ORs into it)
        need = C.c_uint64(0)
        assert _capi.load().dynenv_icm_backward_workspace(self.P, K, C.byref(need)) == 0
        self.ws = Guarded(need.value // 4, 4)
        self.ws_bytes = need.value
        self.grad = _capi.IcmGrad()
        for name, k in zip(("d_fwd_w1", "d_fwd_w1_act", "d_fwd_b1", "d_fwd_w2", "d_fwd_b2", "d_inv_w", "d_inv_b"), GR.PACKED):
            setattr(self.grad, name, self.bufs[k].ptr())

    def launch(self):
        import torch
        from dynenv_amd import _capi
        lib, vp, G = _capi.load(), C.c_void_p, len(self.groups)
        _, w, wt = self.weights
        rc = lib.dynenv_icm_backward(vp(self.f.data_ptr()), vp(self.a.data_ptr()), None if self.fin is None else vp(self.fin.data_ptr()), self.T, self.P, self.K,
                                     self.AD, (C.c_int32 * G)(*self.groups), G, CODE[self.kind], C.byref(w), self.slope, vp(self.count.data_ptr()),
                                     vp(self.up.data_ptr()), C.byref(wt), C.byref(self.grad), vp(self.bufs["dfeat"].ptr()) if self.want_dfeat else None,
                                     vp(self.ws.ptr()), self.ws_bytes, vp(self.bufs["status"].ptr()), vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.dynenv_last_error()
        return self

    def collect(self):
        import torch
        torch.cuda.synchronize()
        self.ws.check("workspace", True)   # (its bands; every slice is written whole)
        out = {k: b.check(k, self.want_dfeat or k != "dfeat").copy() for k, b in self.bufs.items()}
        for k, shape in self.shapes.items():
            if k != "dfeat" or self.want_dfeat:
                out[k] = out[k].reshape(shape)
        out["status"] = out["status"].view(np.int32)
        return out


def _bwd(case, kind, features, actions, finished, weights, **kw):
    return Call(case, kind, features, actions, finished, weights, **kw).launch().collect()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(a, b, keys=OUT + ("status",)):
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
    out = _bwd(case, kind, c["features"], c["actions"], c["finished"], _dev_weights(c["pr"], K, groups, kind), slope=slope)
    assert all(np.isfinite(out[k]).all() for k in OUT) and out["status"][0] == 0
    _judge("C ABI", out, case, kind, slope, OUT)
    for k, pad in (("w1", out["w1"][GR.HIDDEN:]), ("act", out["act"][:, GR.HIDDEN:]), ("b1", out["b1"][GR.HIDDEN:]), ("w2", out["w2"][:, GR.HIDDEN:]),
                   ("inv_w", out["inv_w"][N:]), ("inv_b", out["inv_b"][N:])):
        assert _plus_zero(pad), "the padding of %s is +0" % k
    start = 0
    for n in groups:
        if n == 1:
            assert _plus_zero(out["inv_w"][start]) and _plus_zero(out["inv_b"][start:start + 1]), "a single action's Linear has the gradient 0"
        start += n


EXACT = [(CASES[1], "bf16"), (CASES[2], "f16"), (CASES[3], "bf16"), (CASES[4], "f16")]


@pytest.mark.parametrize("case, kind", EXACT, ids=str)
def test_exact_properties(case, kind):
    c = _inputs(case)
    T, P, K, groups, AD = case
    G = len(groups)
    weights = _dev_weights(c["pr"], K, groups, kind)
    f, a, fin = c["features"], c["actions"], c["finished"]
    run = functools.partial(_bwd, case, kind, weights=weights)
    base = run(f, a, fin)
    assert _same(base, run(f, a, fin)), "two calls give the same bits"
    # masks: NULL is all-zero; d_features NULL leaves the seven alone; everybody finished; exactly one active row
    none = run(f, a, None)
    assert _same(none, run(f, a, np.zeros((T, P), bool)))
    assert _same(base, run(f, a, fin, want_dfeat=False), keys=GR.PACKED + ("status",)), "d_features_dev NULL leaves the weight gradients alone"
    nobody = run(f, a, np.ones((T, P), bool))
    assert all(_plus_zero(nobody[k]) for k in OUT), "n == 0: every output is +0"
    one = np.ones((T, P), bool)
    t1, p1 = T - 1, P // 2
    one[t1, p1] = False
    alone = run(f, a, one)
    touched = np.zeros((T + 1, P), bool)
    touched[t1, p1] = touched[t1 + 1, p1] = True
    assert _plus_zero(alone["dfeat"][~touched]) and alone["dfeat"][touched].all(), "one active row touches its two feature rows"
    idx, _ = IR.indices(a, groups)
    rows = np.zeros(sum(groups), bool)
    rows[[int(sum(groups[:g]) + idx[t1, g, p1]) for g in range(G)]] = True
    assert _plus_zero(alone["act"][~rows]) and alone["act"][rows][:, :GR.HIDDEN].any(axis=1).all(), "... and its G action rows"
    # linearity in upstream
    s_f, s_i = UPSTREAM
    only_f, only_i = run(f, a, fin, upstream=(s_f, 0.0)), run(f, a, fin, upstream=(0.0, s_i))
    assert _plus_zero(only_f["inv_w"]) and _plus_zero(only_f["inv_b"])
    assert all(_plus_zero(only_i[k]) for k in ("w1", "act", "b1", "w2", "b2"))
    assert _same(only_f, base, keys=("w1", "act", "b1", "w2", "b2")) and _same(only_i, base, keys=("inv_w", "inv_b"))
    both = dict(dfeat=only_f["dfeat"].astype(np.float64) + only_i["dfeat"].astype(np.float64))
    _judge("sum of the two halves", both, case, kind, 0.1, ("dfeat",))
    # locality of d_features: the players in another order (same mask, same count); the batch around a player replaced
    perm = np.random.default_rng(1).permutation(P)
    moved = run(f[:, perm], a[:, :, perm], fin[:, perm])
    assert np.array_equal(_bits(moved["dfeat"]), _bits(base["dfeat"][:, perm])), "a row of d_features depends on its place"
    rng = np.random.default_rng(2)
    for keep in sorted({0, P // 2, P - 1}):
        of, oa = rng.standard_normal(f.shape).astype(np.float32), a.copy()
        for g, n in enumerate(groups):
            oa[:, g] = rng.integers(0, n, (T, P))
        of[:, keep], oa[:, :, keep] = f[:, keep], a[:, :, keep]
        got = run(of, oa, fin)
        assert np.array_equal(_bits(got["dfeat"][:, keep]), _bits(base["dfeat"][:, keep])), "player %d depends on the batch" % keep
    # a clamped action: the status bit and the nearest action's gradients
    bad, ok = a.copy(), a.copy()
    bad[0, G - 1, P - 1], ok[0, G - 1, P - 1] = 40.0, groups[-1] - 1
    live = fin.copy()
    live[0, P - 1] = False   # (the row counts)
    clamped = run(f, bad, live)
    assert clamped["status"][0] == 1 and _same(clamped, run(f, ok, live), keys=OUT)


@pytest.mark.parametrize("kind", KINDS)
def test_upstream_scaled_by_a_power_of_two_scales_every_output_exactly(kind):
    """a scale that leaked into a 16-bit rounding would underflow in fp16 (alpha * 2^-20 is about 1e-9 here) or round differently"""
    case = CASES[2]
    c = _inputs(case)
    T, P, K, groups, AD = case
    weights = _dev_weights(c["pr"], K, groups, kind)
    base = _bwd(case, kind, c["features"], c["actions"], c["finished"], weights)
    small = _bwd(case, kind, c["features"], c["actions"], c["finished"], weights, upstream=tuple(u * 2.0 ** -20 for u in UPSTREAM))
    for k in OUT:
        want = np.ldexp(base[k], -20)
        assert want.dtype == np.float32 and np.abs(want[want != 0]).min() > 1e-37, "no subnormal in the comparison"
        assert np.array_equal(_bits(small[k]), _bits(want)), k


def test_a_captured_call_replayed_on_new_contents_equals_an_eager_call():
    import torch
    case, kind = CASES[2], "bf16"
    c = _inputs(case)
    T, P, K, groups, AD = case
    weights = _dev_weights(c["pr"], K, groups, kind)
    call = Call(case, kind, c["features"], c["actions"], c["finished"], weights)
    call.launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.launch()
    other = IR.make_case(T, P, K, groups, AD=AD, seed=77)
    call.f.copy_(_t(other["features"]).cuda())
    call.a.copy_(_t(other["actions"]).cuda())
    call.fin.copy_(_t(other["finished"].astype(np.uint8)).cuda())
    call.count[2] = float((~other["finished"]).sum())
    call.up.mul_(-0.5)
    graph.replay()
    replayed = call.collect()
    eager = _bwd(case, kind, other["features"], other["actions"], other["finished"], weights, upstream=tuple(-0.5 * u for u in UPSTREAM))
    assert _same(replayed, eager)
    first = _bwd(case, kind, c["features"], c["actions"], c["finished"], weights)
    assert not _same(first, eager, keys=("dfeat",)), "the second contents are others"


# ---- the module
def _named_grads(m, f):
    got = {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    got["features"] = None if f.grad is None else f.grad.double().cpu().numpy()
    return got


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("kind", KINDS)
def test_module_route_loss_bits_and_gradients(kind, slope):
    import torch
    T, P, K, groups, AD = case = CASES[2]
    c = _inputs(case)
    m = _module(K, groups, T, c["pr"], kind, slope, fused_backward=True).cuda()
    a, fin = _t(c["actions"]).cuda(), _t(c["finished"]).cuda()
    f = _t(c["features"]).cuda().requires_grad_(True)
    with torch.no_grad():
        plain = m(f, a, fin)
    assert m.last_route == "fused"
    out = m(f, a, fin)
    assert m.last_route == "fused (backward)" and int(m.status) == 0
    for k in ("loss", "forward", "inverse"):
        assert getattr(out, k).grad_fn is not None and torch.equal(getattr(out, k).detach().view(torch.int32), getattr(plain, k).view(torch.int32)), k
    assert out.long_horizon_forward.grad_fn is None and float(out.long_horizon_forward) == 0.0
    out.loss.backward()
    got = _named_grads(m, f)
    want = _g64(case, slope)
    names = GR.names(groups)
    assert sorted(k for k in got if k != "features") == sorted(names), "exactly pred_net.* receives a gradient"
    for k in names:
        assert got[k].shape == want[k].shape, k
    _judge("module", got, case, kind, slope, names + ["features"])
    # features that want no gradient: the parameters' are the same bits
    m2 = _module(K, groups, T, c["pr"], kind, slope, fused_backward=True).cuda()
    f2 = _t(c["features"]).cuda()
    m2(f2, a, fin).loss.backward()
    assert m2.last_route == "fused (backward)" and f2.grad is None
    for (k, p), q in zip(m.named_parameters(), m2.parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32))), k
    # a second backward accumulates into .grad as autograd does; the long-horizon term stays torch, detached
    lh = m2(f2, a, fin, long_horizon=True)
    assert m2.last_route == "fused (backward)" and lh.long_horizon_forward.grad_fn is None
    lh.loss.backward()
    w = m2.pred_net.fwd_net.fc2.weight
    assert torch.equal(w.grad, 2 * m.pred_net.fwd_net.fc2.weight.grad)


def test_module_default_is_the_torch_route_and_every_fallback_is_named(monkeypatch):
    import torch
    from dynenv_amd import GpuICM
    T, P, K, groups = 2, 9, 64, (3, 3)
    pr = IR.make_params(K, groups, T, seed=1)
    case = IR.make_case(T, P, K, groups, seed=2)
    f, a, fin = _t(case["features"]).cuda(), _t(case["actions"]).cuda(), _t(case["finished"]).cuda()
    m = _module(K, groups, T, pr).cuda()
    assert m.fused_backward is False and m(f, a, fin).loss.grad_fn is not None and m.last_route == "torch"
    on = _module(K, groups, T, pr, fused_backward=True).cuda()
    assert on(f, a, fin).loss.grad_fn is not None and on.last_route == "fused (backward)"
    with torch.no_grad():
        on(f, a, fin)
    assert on.last_route == "fused", "without gradients the route is today's"

    def falls_back(mod, why, *args):
        out = mod(*args)
        assert mod.last_route.startswith("torch (fallback: " + why), mod.last_route
        assert bool(torch.isfinite(out.loss)) and out.loss.grad_fn is not None
        out.loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in mod.pred_net.parameters())
    monkeypatch.setenv("DYNENV_ICM_FUSED", "0")
    falls_back(on, "DYNENV_ICM_FUSED=0", f, a, fin)
    monkeypatch.delenv("DYNENV_ICM_FUSED")
    falls_back(GpuICM(K, groups, T, loss_attention=True, fused_backward=True, device="cuda"), "loss_attention=True", f, a, fin)
    falls_back(GpuICM(96, groups, T, fused_backward=True, device="cuda"), "K = 96", torch.randn((T + 1, P, 96), device="cuda"), a, fin)
    falls_back(GpuICM(256, groups, T, fused_backward=True, device="cuda"), "K = 256: the fused backward takes 64 or 128", torch.randn((T + 1, P, 256), device="cuda"),
               a, fin)
    falls_back(GpuICM(K, groups, T, fused_backward=True, device="cuda").double(), "features that is not torch.float32", f.double(), a.double(), fin)
    falls_back(_module(K, groups, T, pr, fused_backward=True), "features that are not on the device", f.cpu(), a.cpu(), fin.cpu())


def test_training_ten_adam_steps_lowers_both_losses_like_the_float32_torch_route():
    import torch
    T, P, K, groups, AD = case = CASES[2]
    c = _inputs(case)
    a, fin, f = _t(c["actions"]).cuda(), _t(c["finished"]).cuda(), _t(c["features"]).cuda()
    fused = _module(K, groups, T, c["pr"], fused_backward=True).cuda()
    twin = _module(K, groups, T, c["pr"]).cuda()
    curves = {}
    for name, m, route in (("fused", fused, "fused (backward)"), ("twin", twin, "torch")):
        opt = torch.optim.Adam(m.pred_net.parameters(), lr=1e-3)
        hist, where = [], None
        for step in range(11):
            out = m(f, a, fin)
            assert m.last_route == route
            hist.append((float(out.forward.detach()) / COEFFS["forward_coeff"], float(out.inverse.detach()) / COEFFS["icm_beta"]))
            if step == 0 and m is fused:
                where = {k: v.data_ptr() for k, v in m._packed.items() if torch.is_tensor(v)}
                assert {"w1", "w2", "inv_w", "w2_t", "w1_t", "inv_w_t"} <= set(where)
            if step < 10:
                opt.zero_grad(set_to_none=True)
                out.loss.backward()
                opt.step()
        if m is fused:
            assert where == {k: v.data_ptr() for k, v in m._packed.items() if torch.is_tensor(v)}, "the packed operands sit at their original addresses"
        curves[name] = np.array(hist)
        print("%s: forward %.4f -> %.4f, inverse %.4f -> %.4f" % ((name,) + tuple(np.array(hist)[[0, -1]].T.reshape(-1))))
    drop = {k: v[0] - v[-1] for k, v in curves.items()}
    assert (drop["twin"] > 0).all(), "the float32 torch route learns on this data"
    assert (drop["fused"] >= 0.5 * drop["twin"]).all(), (drop, "each loss falls by at least half of what the float32 twin's falls")


def test_on_a_collected_rollout_the_storage_own_buffers_train_the_module():
    """Driving, 8 environments, T = 3: GpuRollout.collect() from no autograd graph, then loss.backward() on the storage's buffers"""
    import torch
    from dynenv_amd import GpuICM, GpuRollout
    from test_gpu_rollout import _stack
    E, F, T = 8, 64, 3
    envs, nets, pols, sts = _stack(E, F, T)
    st = sts[0]
    ro = GpuRollout(envs[0], nets[0], pols[0], st)
    torch.manual_seed(3)
    icm = GpuICM(st.feature_size, pols[0].nvec, T, device="cuda", fused_backward=True)
    ro.collect()
    out = icm(st.features, st.actions, st.agentFinished)
    assert icm.last_route == "fused (backward)" and not st.features.requires_grad
    out.loss.backward()
    assert int(icm.status) == 0
    for k, p in icm.named_parameters():
        if k.startswith("pred_net."):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), k
        else:
            assert p.grad is None, k
    for e in envs:
        e.close()
