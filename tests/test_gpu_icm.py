"""The fused curiosity module on the device (csrc/icm_kernels.hip through dynenv_icm_losses and GpuICM) against the numpy float64 statement
tests/icm_ref.py.  -m gpu.

Accuracy, the project's rule (test_gpu_policy.py): err_fused = max |x - ref64| for x = curiosity and inverse_ce; err_cpu_autocast the same
distances for the module's torch route run here on the CPU under torch.autocast("cpu", dtype) on the same inputs, computed at run time,
independent of the code under test and of the device.  Required, for both: err_fused <= 4 * err_cpu_autocast (room for another
accumulation order and for where the 16-bit roundings fall; a missing bias, a wrong group offset, an unread f_{t+1} or a dropped one-hot
column moves a term by 0.1 to 1).  Every run prints both errors; measured figures: profiles/HISTORY.md, the section of this kernel.
Inputs: standard-normal features; icm_ref.make_params (every bias in +-0.5); uniform actions; about 30 % finished.
Exact checks take no tolerance: guard bands, every element written, repeatability, independence of p, of P, of T and of the other rows,
a NULL mask an all-zero one, a NULL losses_dev the same rows.  The reduction: within one float32 ulp of the float64 sums of the kernel's
own returned rows under the mask, the count exact.

The kernel's tiling: a workgroup of 64 players in four strips of 16 walks t = 0 .. T-1; one kernel per K = 64, 128, 256.
CASES (T, P, K, groups, AD) - the issue's, unchanged but for the action columns, which it leaves open:
  one row, one step, K = 64 | one row past a strip, K = 128, four groups | one row past a workgroup at the reference's T = 6, K = 128,
  RoboCup's groups with an unread fourth action column | P = 130, no multiple of 16, three workgroups, K = 256, the cap on a group |
  eight groups with one of a single action, whose cross-entropy is exactly 0, K = 64."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icm_ref as IR  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 64, (3, 3), 2), (2, 17, 128, (5, 3, 3, 7), 4), (6, 65, 128, (5, 3, 3), 4), (3, 130, 256, (16, 16), 2), (1, 43, 64, (2, 2, 1, 2, 2, 2, 2, 2), 8)]
KINDS = ["bf16", "f16"]
CODE = {"bf16": 1, "f16": 2}
FACTOR = 4.0
COEFFS = dict(forward_coeff=0.2, icm_beta=0.8)


def _tdtype(kind):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _module(K, groups, T, pr, kind="bf16", **kw):
    from dynenv_amd import GpuICM
    return IR.load(GpuICM(K, groups, T, w_dtype=_tdtype(kind), **dict(COEFFS, **kw)), pr)


def _autocast_rows(m, features, actions, device, kind):
    """the torch route's rows under autocast -> (curiosity, inverse_ce) float64 on the host"""
    import torch
    with torch.no_grad(), torch.autocast(device, dtype=_tdtype(kind)):
        se, ce, _ = m._rows_torch(_t(features).to(device), m._indices(_t(actions).to(device)))
    return se.mean(-1).double().cpu().numpy(), torch.stack(ce, 1).double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """inputs, parameters, the float64 statement and the CPU autocast error of one case, computed once and shared (nothing in it is
    written to afterwards)"""
    T, P, K, groups, AD = case
    pr = IR.make_params(K, groups, T, seed=P + K)
    c = dict(IR.make_case(T, P, K, groups, AD=AD, seed=31 * P + K + len(groups) + (kind == "f16")), case=case, kind=kind, pr=pr)
    cur, ce, _ = IR.rows(c["features"], c["actions"], pr, groups)
    c["ref"] = (cur, ce)
    got = _autocast_rows(_module(K, groups, T, pr, kind), c["features"], c["actions"], "cpu", kind)
    c["err_cpu"] = np.array([np.abs(got[0] - cur).max(), np.abs(got[1] - ce).max()])
    return c


def _errors(c, cur, ce):
    return np.array([np.abs(np.asarray(cur, np.float64) - c["ref"][0]).max(), np.abs(np.asarray(ce, np.float64) - c["ref"][1]).max()])


def _fmt(err):
    return "curiosity %.3g inverse_ce %.3g" % tuple(err)


def _dev_weights(pr, K, groups, kind):
    """the device tensors of dynenv_icm_t, packed here from the parameters, and the host struct over them"""
    import torch
    from dynenv_amd import _capi
    dt, N, H, HP = _tdtype(kind), sum(groups), IR.HIDDEN, 160
    w1 = torch.from_numpy(pr["pred_net.fwd_net.fc1.weight"]).cuda()
    t = dict(w1=torch.zeros((HP, K), dtype=dt, device="cuda"), act=torch.zeros((N, HP), device="cuda"), b1=torch.zeros(HP, device="cuda"),
             w2=torch.zeros((K, HP), dtype=dt, device="cuda"), b2=torch.from_numpy(pr["pred_net.fwd_net.fc2.bias"]).cuda(),
             iw=torch.zeros((32, 2 * K), dtype=dt, device="cuda"), ib=torch.zeros(32, device="cuda"))
    t["w1"][:H] = w1[:, :K]
    t["act"][:, :H] = w1[:, K:].t()
    t["b1"][:H] = torch.from_numpy(pr["pred_net.fwd_net.fc1.bias"]).cuda()
    t["w2"][:, :H] = torch.from_numpy(pr["pred_net.fwd_net.fc2.weight"]).cuda()
    t["iw"][:N] = torch.cat([torch.from_numpy(pr["pred_net.inv_net.blocks.0.Layer.%d.weight" % g]) for g in range(len(groups))]).cuda()
    t["ib"][:N] = torch.cat([torch.from_numpy(pr["pred_net.inv_net.blocks.0.Layer.%d.bias" % g]) for g in range(len(groups))]).cuda()
    w = _capi.Icm()
    w.fwd_w1, w.fwd_w1_act, w.fwd_b1, w.fwd_w2, w.fwd_b2, w.inv_w, w.inv_b = (t[k].data_ptr() for k in ("w1", "act", "b1", "w2", "b2", "iw", "ib"))
    return t, w


def _icm(c, features, actions, finished, weights, want_losses=True):
    """dynenv_icm_losses with every output between guard bands -> dict of host arrays; finished None: a NULL mask"""
    import torch
    from dynenv_amd import _capi
    from test_gpu_arranger_dtype import Guarded
    lib = _capi.load()
    _, _, K, groups, _ = c["case"]
    T, P, AD, G = features.shape[0] - 1, features.shape[1], actions.shape[1], len(groups)
    keep, w = weights
    f, a = _t(np.asarray(features, np.float32)).cuda(), _t(np.asarray(actions, np.float32)).cuda()
    fin = None if finished is None else _t(np.asarray(finished, np.uint8)).cuda()
    bufs = dict(curiosity=Guarded(T * P, 4), ce=Guarded(T * G * P, 4), losses=Guarded(3, 4), status=Guarded(1, 4))
    bufs["status"].payload.zero_()   # (the kernel ORs into it)
    vp = C.c_void_p
    rc = lib.dynenv_icm_losses(vp(f.data_ptr()), vp(a.data_ptr()), None if fin is None else vp(fin.data_ptr()), T, P, K, AD, (C.c_int32 * G)(*groups), G,
                               CODE[c["kind"]], C.byref(w), IR.SLOPE, vp(bufs["curiosity"].ptr()), vp(bufs["ce"].ptr()),
                               vp(bufs["losses"].ptr()) if want_losses else None, vp(bufs["status"].ptr()), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dynenv_last_error()
    torch.cuda.synchronize()
    out = {k: b.check(k, want_losses or k != "losses").copy() for k, b in bufs.items()}
    out["curiosity"], out["ce"] = out["curiosity"].reshape(T, P), out["ce"].reshape(T, G, P)
    out["status"] = out["status"].view(np.int32)
    return out


def _same(a, b, keys=("curiosity", "ce", "losses", "status")):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


def _ulp_close(got, want64):
    """a float32 within one ulp of the float64 `want64`"""
    near = np.float32(want64)
    return got == near or got == np.nextafter(near, np.float32(np.inf)) or got == np.nextafter(near, np.float32(-np.inf))


def _check_reduction(out, finished, G):
    mask = np.ones(out["curiosity"].shape, bool) if finished is None else ~np.asarray(finished, bool)
    n = int(mask.sum())
    got = out["losses"]
    assert got[2] == n
    if n == 0:
        assert not got[:2].any() and not np.signbit(got[:2]).any(), "+0, +0, 0"
        return
    assert _ulp_close(got[0], out["curiosity"].astype(np.float64)[mask].sum() / n)
    assert _ulp_close(got[1], sum(out["ce"][:, g].astype(np.float64)[mask].sum() for g in range(G)) / (n * G))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_c_abi_accuracy_every_element_written_and_the_reduction(case, kind):
    c = _case(case, kind)
    T, P, K, groups, AD = case
    out = _icm(c, c["features"], c["actions"], c["finished"], _dev_weights(c["pr"], K, groups, kind))
    err = _errors(c, out["curiosity"], out["ce"])
    print("%s %s: err_fused %s | err_cpu_autocast %s (C ABI)" % (case, kind, _fmt(err), _fmt(c["err_cpu"])))
    assert np.isfinite(out["curiosity"]).all() and np.isfinite(out["ce"]).all() and (out["curiosity"] > 0).all()
    assert (err <= FACTOR * c["err_cpu"]).all()
    assert out["status"][0] == 0
    for g, n in enumerate(groups):
        if n == 1:
            assert not out["ce"][:, g].any(), "a single action's cross-entropy is exactly 0"
    _check_reduction(out, c["finished"], len(groups))


EXACT = [(CASES[1], "bf16"), (CASES[2], "f16"), (CASES[3], "bf16"), (CASES[4], "f16")]


@pytest.mark.parametrize("case, kind", EXACT, ids=str)
def test_exact_properties(case, kind):
    c = _case(case, kind)
    T, P, K, groups, AD = case
    G = len(groups)
    weights = _dev_weights(c["pr"], K, groups, kind)
    f, a, fin = c["features"], c["actions"], c["finished"]
    base = _icm(c, f, a, fin, weights)
    assert _same(base, _icm(c, f, a, fin, weights)), "two calls give the same bits"
    rows = ("curiosity", "ce")
    assert _same(base, _icm(c, f, a, fin, weights, want_losses=False), keys=rows), "losses_dev NULL leaves the rows alone"
    # a NULL mask is an all-zero mask; all finished; exactly one active row
    none = _icm(c, f, a, None, weights)
    assert _same(none, _icm(c, f, a, np.zeros((T, P), bool), weights)) and _same(none, base, keys=rows)
    _check_reduction(none, None, G)
    everyone = np.ones((T, P), bool)
    _check_reduction(_icm(c, f, a, everyone, weights), everyone, G)
    one = everyone.copy()
    one[T - 1, P // 2] = False
    alone = _icm(c, f, a, one, weights)
    _check_reduction(alone, one, G)
    assert alone["losses"][0] == base["curiosity"][T - 1, P // 2], "exactly one active row gives that row's terms"
    # the players in another order: a row moves with its player
    perm = np.random.default_rng(1).permutation(P)
    moved = _icm(c, f[:, perm], a[:, :, perm], fin[:, perm], weights)
    assert np.array_equal(moved["curiosity"].view(np.uint32), base["curiosity"][:, perm].view(np.uint32)), "a row's result depends on its index"
    assert np.array_equal(moved["ce"].view(np.uint32), base["ce"][:, :, perm].view(np.uint32))
    # T changes: the first step alone, and the rollout without its first step
    first = _icm(c, f[:2], a[:1], fin[:1], weights)
    assert all(np.array_equal(first[k].view(np.uint32), base[k][:1].view(np.uint32)) for k in rows), "a row depends on T"
    if T > 1:
        rest = _icm(c, f[1:], a[1:], fin[1:], weights)
        assert all(np.array_equal(rest[k].view(np.uint32), base[k][1:].view(np.uint32)) for k in rows), "a row depends on its t"
    # the batch around a player changes; the batch shrinks to the players from `keep` on, and to that player alone
    rng = np.random.default_rng(2)
    for keep in sorted({0, P // 2, P - 1}):
        of, oa = rng.standard_normal(f.shape).astype(np.float32), a.copy()
        for g, n in enumerate(groups):
            oa[:, g] = rng.integers(0, n, (T, P))
        of[:, keep], oa[:, :, keep] = f[:, keep], a[:, :, keep]
        got = _icm(c, of, oa, fin, weights)
        assert np.array_equal(got["curiosity"][:, keep].view(np.uint32), base["curiosity"][:, keep].view(np.uint32)), "player %d depends on the batch" % keep
        assert np.array_equal(got["ce"][:, :, keep].view(np.uint32), base["ce"][:, :, keep].view(np.uint32)), "player %d depends on the batch" % keep
        for sl in (slice(keep, None), slice(keep, keep + 1)):
            part = _icm(c, f[:, sl], a[:, :, sl], fin[:, sl], weights)
            assert np.array_equal(part["curiosity"].view(np.uint32), base["curiosity"][:, sl].view(np.uint32)), "player %d on depends on P or on p" % keep
            assert np.array_equal(part["ce"].view(np.uint32), base["ce"][:, :, sl].view(np.uint32)), "player %d on depends on P or on p" % keep
    # a clamped action: the status bit, the nearest action's result, no other row
    bad = a.copy()
    bad[0, G - 1, P - 1] = 40.0
    ok = a.copy()
    ok[0, G - 1, P - 1] = groups[-1] - 1
    clamped = _icm(c, f, bad, fin, weights)
    assert clamped["status"][0] == 1 and _same(clamped, _icm(c, f, ok, fin, weights), keys=rows + ("losses",))
    keep = np.ones((T, P), bool)
    keep[0, P - 1] = False
    assert np.array_equal(clamped["curiosity"][keep].view(np.uint32), base["curiosity"][keep].view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
def test_module_takes_the_fused_route_and_its_losses_follow_the_accuracy_rule(kind):
    """the scalars under the same rule: |fused - ref64| <= 4 * |cpu autocast - ref64| for `forward` and `inverse`"""
    import torch
    T, P, K, groups, AD = case = CASES[2]
    c = _case(case, kind)
    want = IR.losses(c["features"], c["actions"], c["finished"], c["pr"], groups, **COEFFS)
    m = _module(K, groups, T, c["pr"], kind).cuda()
    f, a, fin = _t(c["features"]).cuda(), _t(c["actions"]).cuda(), _t(c["finished"]).cuda()
    with torch.no_grad():
        got = m(f, a, fin)
    assert m.last_route == "fused" and got.loss.grad_fn is None and got.loss.is_cuda and got.loss.dim() == 0
    assert float(got.long_horizon_forward) == 0.0 and float(got.loss) == float(got.inverse + got.forward) and int(m.status) == 0
    cur, ce = m.rows(f, a)
    assert m.last_route == "fused" and tuple(cur.shape) == (T, P) and tuple(ce.shape) == (T, len(groups), P)
    err = _errors(c, cur.cpu().numpy(), ce.cpu().numpy())
    assert (err <= FACTOR * c["err_cpu"]).all()
    cpu = _module(K, groups, T, c["pr"], kind).requires_grad_(False)
    with torch.autocast("cpu", dtype=_tdtype(kind)):
        ref = cpu._forward_torch(_t(c["features"]), _t(c["actions"]), _t(c["finished"]), False)
    for k in ("forward", "inverse"):
        e_fused, e_cpu = abs(float(getattr(got, k)) - want[k]), abs(float(getattr(ref, k)) - want[k])
        print("%s %s %s: exact %.9e err_fused %.3g | err_cpu_autocast %.3g" % (case, kind, k, want[k], e_fused, e_cpu))
        assert e_fused <= FACTOR * e_cpu, k
    # the packed weights follow the parameters: in place, at the same addresses
    before = m._packed["w1"].data_ptr()
    with torch.no_grad():
        m.pred_net.fwd_net.fc2.bias.add_(1.0)
        moved = m(f, a, fin)
    assert m.last_route == "fused" and m._packed["w1"].data_ptr() == before and float(moved.forward) > float(got.forward)
    assert torch.equal(moved.inverse, got.inverse)
    # with gradients enabled and parameters that want one: the torch route, differentiable; under no_grad the fused one again
    out = m(f, a, fin)
    assert m.last_route == "torch" and out.loss.grad_fn is not None
    m.requires_grad_(False)
    assert m(f, a, fin).loss.grad_fn is None and m.last_route == "fused"
    assert m(f.clone().requires_grad_(True), a, fin).loss.grad_fn is not None and m.last_route == "torch"


def test_module_names_every_fallback(monkeypatch):
    import torch
    T, P, K, groups = 2, 9, 64, (3, 3)
    pr = IR.make_params(K, groups, T, seed=1)
    case = IR.make_case(T, P, K, groups, seed=2)
    f, a, fin = _t(case["features"]).cuda(), _t(case["actions"]).cuda(), _t(case["finished"]).cuda()
    m = _module(K, groups, T, pr).cuda().requires_grad_(False)
    base = m(f, a, fin)
    assert m.last_route == "fused"

    def falls_back(mod, why, *args):
        with torch.no_grad():
            out = mod(*args)
        assert mod.last_route.startswith("torch (fallback: " + why), mod.last_route
        assert bool(torch.isfinite(out.loss)) and out.loss.grad_fn is None
        return out
    monkeypatch.setenv("DYNENV_ICM_FUSED", "0")
    plain = falls_back(m, "DYNENV_ICM_FUSED=0", f, a, fin)
    monkeypatch.delenv("DYNENV_ICM_FUSED")
    assert abs(float(plain.loss) - float(base.loss)) < 0.02 * abs(float(plain.loss)), "the routes differ by the operands' rounding only"
    from dynenv_amd import GpuICM
    falls_back(GpuICM(K, groups, T, loss_attention=True, device="cuda").requires_grad_(False), "loss_attention=True", f, a, fin)
    falls_back(GpuICM(96, groups, T, device="cuda").requires_grad_(False), "K = 96", torch.randn((T + 1, P, 96), device="cuda"), a, fin)
    wide = torch.zeros((T, 3, P), device="cuda")
    falls_back(GpuICM(K, (16, 16, 4), T, device="cuda").requires_grad_(False), "an action space beyond", f, wide, fin)
    falls_back(GpuICM(K, (2,) * 9, T, device="cuda").requires_grad_(False), "an action space beyond", f, torch.zeros((T, 9, P), device="cuda"), fin)
    falls_back(_module(K, groups, T, pr).requires_grad_(False), "features that are not on the device", f.cpu(), a.cpu(), fin.cpu())
    falls_back(m, "features that is not torch.float32, contiguous", f.transpose(0, 1).contiguous().transpose(0, 1), a, fin)
    falls_back(m, "actions that is not torch.float32", f, a.double(), fin)
    falls_back(m, "agent_finished that is not torch.bool / torch.uint8", f, a, fin.float())
    falls_back(GpuICM(K, groups, T, device="cuda").double().requires_grad_(False), "features that is not torch.float32", f.double(), a.double(), fin)
    assert m(f, a, fin.to(torch.uint8)).loss.item() == base.loss.item() and m.last_route == "fused"
    assert torch.isfinite(m(f, a, None).loss) and m.last_route == "fused"


def test_torch_route_gradients_against_a_float64_cpu_twin():
    """float32 on the device against float64 on the CPU: the gradients of `loss` with respect to every pred_net parameter and to the
    features agree to 1e-3 of the largest gradient entry of each (test_gpu_recurrent.py's bound)"""
    import torch
    T, P, K, groups = 3, 12, 128, (5, 3, 3, 7)
    pr = IR.make_params(K, groups, T, seed=9)
    case = IR.make_case(T, P, K, groups, seed=4)
    dev = _module(K, groups, T, pr).cuda()
    twin = _module(K, groups, T, pr).double()
    fd = _t(case["features"]).cuda().requires_grad_(True)
    f64 = _t(case["features"]).double().requires_grad_(True)
    out = dev(fd, _t(case["actions"]).cuda(), _t(case["finished"]).cuda())
    assert dev.last_route == "torch"
    out.loss.backward()
    out64 = twin(f64, _t(case["actions"]).double(), _t(case["finished"]))
    out64.loss.backward()
    assert abs(float(out.loss.detach()) - float(out64.loss.detach())) <= 1e-5 * abs(float(out64.loss.detach()))
    pairs = [(k, p.grad, q.grad) for (k, p), q in zip(dev.named_parameters(), twin.parameters())] + [("features", fd.grad, f64.grad)]
    for k, g, g64 in pairs:
        if not k.startswith("pred_net.") and k != "features":
            assert g is None and g64 is None, k
            continue
        scale = float(g64.abs().max())
        err = float((g.double().cpu() - g64).abs().max())
        print("grad %s: max %.3g err %.3g" % (k, scale, err))
        assert scale > 0 and err <= 1e-3 * scale, k


def test_end_to_end_on_a_collected_rollout_eagerly_and_from_a_graph():
    """Driving, 8 environments, T = 3: GpuRollout.collect(), then icm(storage.features, storage.actions, storage.agentFinished) under
    no_grad takes the fused route on the storage's own buffers; the same call recorded with torch.cuda.graph - a capture fails at the
    first host read - and replayed after a second collect() equals an eager call on the second rollout bit for bit"""
    import torch
    from dynenv_amd import GpuICM, GpuRollout
    from test_gpu_rollout import _stack
    E, F, T = 8, 64, 3
    envs, nets, pols, sts = _stack(E, F, T)
    st = sts[0]
    ro = GpuRollout(envs[0], nets[0], pols[0], st)
    torch.manual_seed(3)
    icm = GpuICM(st.feature_size, pols[0].nvec, T, device="cuda")
    ro.collect()
    with torch.no_grad():
        first = icm(st.features, st.actions, st.agentFinished)
        assert icm.last_route == "fused" and bool(torch.isfinite(first.loss)) and float(first.loss) > 0 and int(icm.status) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            recorded = icm(st.features, st.actions, st.agentFinished)
        assert icm.last_route == "fused"
        st.after_update()
        ro.collect()
        graph.replay()
        eager = icm(st.features, st.actions, st.agentFinished)
        cur, ce = icm.rows(st.features, st.actions)
    for k in ("loss", "inverse", "forward"):
        assert torch.equal(getattr(recorded, k).view(torch.int32), getattr(eager, k).view(torch.int32)), k
    assert not torch.equal(eager.loss, first.loss), "the second rollout is another one"
    assert tuple(cur.shape) == (T, E * envs[0].n_agents) and bool(torch.isfinite(cur).all()) and bool(torch.isfinite(ce).all())
    for e in envs:
        e.close()
