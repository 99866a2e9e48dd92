"""The fused policy head on the device (csrc/policy_kernels.hip through dynenv_policy_head and GpuPolicyHead) against the numpy float64
statement tests/policy_ref.py.  -m gpu.

Accuracy: err_fused = max |x - ref64| for x = probs, value, cont and log_probs, the last evaluated in the float64 statement AT THE
ACTIONS THE KERNEL DREW; err_cpu_autocast the same distances for the module's torch route run here on the CPU under
torch.autocast("cpu", dtype) on the same inputs (log_probs at that route's own actions), computed at run time, independent of the code
under test and of the device.  Required, for each of the four: err_fused <= 4 * err_cpu_autocast (the embed, attention and recurrent
kernels' factor: room for another accumulation order and for where the 16-bit roundings fall; a missing bias, a wrong group offset or
an unused feat1 moves a probability by 0.1 to 1).  Every run prints both errors; measured figures: profiles/HISTORY.md, the section of
this kernel.  Inputs: standard-normal features; policy_ref.make_params (every bias in +-0.5).
Exact checks take no tolerance: the drawn actions are the host's inverse CDF of the kernel's own returned probabilities with the host's
Philox u, next_ext the table of those actions, log_probs the float32 nearest to the log of the returned probability, the columns behind
G zero, guard bands, every element written, repeatability, independence of p, of P and of the other rows, a NULL counter a zero one.

The kernel's tiling: a workgroup of 64 rows in four strips of 16; one kernel per K = 64, 128, 256 (1, 2 and 3 output tiles per wave).
CASES (P, F, feat1, nvec, C, AD):
  one row, K = 64, Driving's space | one row past a strip, K = 128, RoboCup's space | one row past a workgroup, K = 128 from two features,
  RoboCup with allowHeadTurn (Box output, AD = 4: a zero column) | P = 130, no multiple of 16, three workgroups, K = 256, the cap on a
  group | eight groups with one of a single action, K = 64 from one feature | four Box outputs and AD = 7 behind two groups, K = 128 |
  K = 256 with the Box output."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(1, 64, False, (3, 3), 0, 2), (17, 128, False, (5, 3, 3, 7), 0, 4), (65, 64, True, (5, 3, 3), 1, 4), (130, 128, True, (16, 16), 0, 2),
         (43, 64, False, (2, 2, 1, 2, 2, 2, 2, 2), 0, 8), (33, 128, False, (4, 6), 4, 7), (77, 128, True, (5, 3, 3), 1, 4)]
KINDS = ["bf16", "f16"]
CODE = {"bf16": 1, "f16": 2}
FACTOR = 4.0
SEED, DRAW, ROW_BASE = 2 ** 40 + 5, 2 ** 33 + 7, 2 ** 32 - 20   # each with a high word or a carry into one
NAMES = ("probs", "value", "cont", "log_probs")


def _tdtype(kind):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _fmt(err):
    return " ".join("%s %.3g" % (n, e) for n, e in zip(NAMES, err))


def _errors(ref, nvec, probs, value, cont, logp, actions):
    """the four distances to the float64 statement; log_probs at `actions`"""
    p64, c64, v64 = ref
    G = len(nvec)
    want_lp = PR.log_probs(p64, nvec, np.asarray(actions)[:, :G])
    return np.array([np.abs(np.asarray(probs, np.float64) - p64).max(), np.abs(np.asarray(value, np.float64).reshape(-1) - v64).max(),
                     np.abs(np.asarray(cont, np.float64).reshape(c64.shape) - c64).max() if c64.size else 0.0,
                     np.abs(np.asarray(logp, np.float64) - want_lp).max()])


def _module_errors(layer, ref, nvec, feat0, feat1, device, autocast_kind):
    """one act() of `layer` on `device` (under autocast: its torch route) -> the four distances"""
    import torch
    layer.reseed(SEED, DRAW)
    args = (_t(feat0).to(device), None if feat1 is None else _t(feat1).to(device))
    with torch.no_grad():
        if autocast_kind is None:
            out = layer.act(*args, row_base=ROW_BASE)
        else:
            with torch.autocast(device, dtype=_tdtype(autocast_kind)):
                out = layer._act_torch(*args, None, ROW_BASE)
    cont = np.zeros((feat0.shape[0], 0)) if out.head is None else out.head.double().cpu().numpy()
    return _errors(ref, nvec, torch.cat(out.probs, 1).double().cpu().numpy(), out.value.double().cpu().numpy(), cont,
                   out.log_probs.double().cpu().numpy(), out.actions.cpu().numpy()), out


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """inputs, parameters, the float64 statement and the CPU autocast error of one case, computed once and shared (nothing in it is
    written to afterwards)"""
    from dynenv_amd import GpuPolicyHead
    P, F, two, nvec, Cn, AD = case
    K = 2 * F if two else F
    rng = np.random.default_rng(31 * P + F + len(nvec) + (kind == "f16"))
    feat0 = rng.standard_normal((P, F)).astype(np.float32)
    feat1 = rng.standard_normal((P, F)).astype(np.float32) if two else None
    x = feat0 if feat1 is None else np.concatenate([feat0, feat1], 1)
    pr = PR.make_params(K, nvec, Cn, seed=P + K)
    ref = PR.head(x, pr, nvec, Cn)
    c = dict(case=case, kind=kind, K=K, feat0=feat0, feat1=feat1, x=x, pr=pr, ref=ref)
    cpu = PR.load(GpuPolicyHead(K, PR.space(nvec, Cn), operand_dtype=_tdtype(kind)), pr).requires_grad_(False)
    c["err_cpu"] = _module_errors(cpu, ref, nvec, feat0, feat1, "cpu", kind)[0]
    return c


def _dev_weights(pr, K, nvec, Cn, kind):
    """the device tensors of dynenv_policy_t and the host struct over them"""
    import torch
    from dynenv_amd import _capi
    dt = _tdtype(kind)
    w64, b64 = PR.actor_rows(pr)
    n = w64.shape[0]
    aw = torch.zeros((32, K), dtype=dt, device="cuda")
    aw[:n] = torch.from_numpy(w64.astype(np.float32)).cuda()
    ab = torch.zeros((32,), dtype=torch.float32, device="cuda")
    ab[:n] = torch.from_numpy(b64.astype(np.float32)).cuda()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in pr.items() if k.startswith("critic.")}
    keep = [aw, ab, t, t["critic.blocks.Layer1.weight"].to(dt), torch.full((max(Cn, 1),), (PR.HIGH - PR.LOW) * 0.5, device="cuda"),
            torch.full((max(Cn, 1),), (PR.HIGH + PR.LOW) * 0.5, device="cuda")]
    w = _capi.Policy()
    w.actor_w, w.actor_b, w.critic_w1 = aw.data_ptr(), ab.data_ptr(), keep[3].data_ptr()
    w.critic_b1, w.critic_ln_w, w.critic_ln_b = (t["critic.blocks." + k].data_ptr() for k in ("Layer1.bias", "bn.weight", "bn.bias"))
    w.critic_w2, w.critic_b2 = t["critic.blocks.Layer2.weight"].data_ptr(), t["critic.blocks.Layer2.bias"].data_ptr()
    if Cn:
        w.cont_scale, w.cont_mean = keep[4].data_ptr(), keep[5].data_ptr()
    return keep, w


def _policy(c, feat0, feat1, weights, seed=SEED, draw=DRAW, row_base=ROW_BASE, turn=0, want_ext=True):
    """dynenv_policy_head with every output between guard bands -> dict of host arrays; draw None: a NULL counter"""
    import torch
    from dynenv_amd import _capi
    from test_gpu_arranger_dtype import Guarded
    lib = _capi.load()
    _, F, _, nvec, Cn, AD = c["case"]
    P, G, N = feat0.shape[0], len(nvec), sum(nvec)
    keep, w = weights
    f0 = _t(np.asarray(feat0, np.float32)).cuda()
    f1 = None if feat1 is None else _t(np.asarray(feat1, np.float32)).cuda()
    dd = None if draw is None else torch.tensor([draw - 2 ** 64 if draw >> 63 else draw], dtype=torch.int64, device="cuda")
    sizes = dict(actions=(P * AD, 4), cont=(P * Cn, 8), probs=(P * N, 4), logp=(P * G, 4), value=(P, 4), next_ext=(P * AD, 4))
    bufs = {k: Guarded(*v) for k, v in sizes.items()}
    vp = C.c_void_p
    ptr = lambda k: vp(bufs[k].ptr()) if bufs[k].ptr() is not None else None  # noqa: E731
    rc = lib.dynenv_policy_head(vp(f0.data_ptr()), None if f1 is None else vp(f1.data_ptr()), P, 1, F, CODE[c["kind"]], C.byref(w), (C.c_int32 * G)(*nvec),
                                G, Cn, AD, seed, None if dd is None else vp(dd.data_ptr()), row_base, PR.SLOPE, PR.EPS, turn, ptr("actions"), ptr("cont"),
                                ptr("probs"), ptr("logp"), ptr("value"), ptr("next_ext") if want_ext else None, vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dynenv_last_error()
    torch.cuda.synchronize()
    out = {k: b.check(k, want_ext or k != "next_ext").copy() for k, b in bufs.items()}
    out["actions"] = out["actions"].view(np.int32).reshape(P, AD)
    out["cont"] = out["cont"].view(np.float64).reshape(P, Cn)
    out["probs"], out["logp"], out["next_ext"] = out["probs"].reshape(P, N), out["logp"].reshape(P, G), out["next_ext"].reshape(P, AD)
    return out


def _same(a, b, keys=("actions", "cont", "probs", "logp", "value", "next_ext"), rows=None):
    pick = (lambda v: v) if rows is None else (lambda v: v[rows])
    return all(np.array_equal(pick(a[k]).view(np.uint8), pick(b[k]).view(np.uint8)) for k in keys)


def _exact(c, out, seed, draw, row_base, turn=0):
    """what holds of every call without a tolerance"""
    _, _, _, nvec, Cn, AD = c["case"]
    G = len(nvec)
    probs = out["probs"]
    assert np.isfinite(probs).all() and np.isfinite(out["value"]).all() and np.isfinite(out["cont"]).all()
    want = PR.draw_actions(probs, nvec, seed, draw, row_base)
    assert np.array_equal(out["actions"][:, :G], want), "the actions are not the inverse CDF of the returned probabilities"
    assert not out["actions"][:, G:].any(), "the columns behind G are 0"
    assert np.array_equal(out["next_ext"], PR.transform_table(out["actions"], turn).astype(np.float32))
    off = np.cumsum((0,) + tuple(nvec[:-1]))
    pa = np.take_along_axis(probs, off[None, :] + want, 1)
    lp = np.log(np.clip(pa, np.float32(PR.EPS32), np.float32(1) - np.float32(PR.EPS32)).astype(np.float64)).astype(np.float32)
    assert np.array_equal(out["logp"].view(np.uint32), lp.view(np.uint32)), "log_probs is the float32 log of the returned probability"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_c_abi_accuracy_the_exact_draw_and_every_element_written_and_nothing_else(case, kind):
    c = _case(case, kind)
    P, F, two, nvec, Cn, AD = case
    out = _policy(c, c["feat0"], c["feat1"], _dev_weights(c["pr"], c["K"], nvec, Cn, kind))
    err = _errors(c["ref"], nvec, out["probs"], out["value"], out["cont"], out["logp"], out["actions"])
    print("%s %s: err_fused %s | err_cpu_autocast %s (C ABI)" % (case, kind, _fmt(err), _fmt(c["err_cpu"])))
    assert (err <= FACTOR * c["err_cpu"]).all()
    _exact(c, out, SEED, DRAW, ROW_BASE)
    assert np.abs(out["probs"].reshape(P, -1)[:, :nvec[0]].sum(1) - 1).max() < 1e-6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_module_accuracy_against_float64_within_the_cpu_autocast_error(case, kind):
    from dynenv_amd import GpuPolicyHead
    c = _case(case, kind)
    P, F, two, nvec, Cn, AD = case
    layer = PR.load(GpuPolicyHead(c["K"], PR.space(nvec, Cn), operand_dtype=_tdtype(kind)), c["pr"]).cuda().requires_grad_(False)
    err, out = _module_errors(layer, c["ref"], nvec, c["feat0"], c["feat1"], "cuda", None)
    assert layer.last_route == "fused", layer.last_route
    err_dev, _ = _module_errors(layer, c["ref"], nvec, c["feat0"], c["feat1"], "cuda", kind)
    print("%s %s: err_fused %s | err_cpu_autocast %s | err_device_autocast %s" % (case, kind, _fmt(err), _fmt(c["err_cpu"]), _fmt(err_dev)))
    assert (err <= FACTOR * c["err_cpu"]).all()
    assert tuple(out.actions.shape) == (P, len(nvec) + Cn) and tuple(out.value.shape) == (P, 1) and tuple(out.next_ext.shape) == (P, len(nvec) + Cn)
    if Cn == 1:
        assert tuple(out.head.shape) == (P,) and out.head.dtype.is_floating_point and out.head.element_size() == 8


EXACT = [(CASES[1], "bf16"), (CASES[2], "f16"), (CASES[3], "bf16"), (CASES[4], "f16"), (CASES[5], "bf16"), (CASES[6], "f16")]


@pytest.mark.parametrize("case, kind", EXACT, ids=str)
def test_exact_properties(case, kind):
    c = _case(case, kind)
    P, F, two, nvec, Cn, AD = case
    weights = _dev_weights(c["pr"], c["K"], nvec, Cn, kind)
    f0, f1 = c["feat0"], c["feat1"]
    sub = lambda a, idx: None if a is None else a[idx]  # noqa: E731
    base = _policy(c, f0, f1, weights)
    assert _same(base, _policy(c, f0, f1, weights)), "two calls give the same bits"
    # a NULL counter is a zero counter; another counter, seed or row_base draws otherwise from the same probabilities
    zero = _policy(c, f0, f1, weights, draw=0)
    assert _same(zero, _policy(c, f0, f1, weights, draw=None))
    _exact(c, zero, SEED, 0, ROW_BASE)
    for kw in (dict(draw=DRAW + 1), dict(draw=DRAW + 2 ** 32), dict(seed=SEED + 1), dict(seed=SEED + 2 ** 32), dict(row_base=ROW_BASE + 1),
               dict(row_base=ROW_BASE + 2 ** 32 + 1)):
        other = _policy(c, f0, f1, weights, **kw)
        _exact(c, other, kw.get("seed", SEED), kw.get("draw", DRAW), kw.get("row_base", ROW_BASE))
        assert _same(other, base, keys=("probs", "value", "cont")) and (P < 17 or not np.array_equal(other["actions"], base["actions"])), kw
    assert _same(_policy(c, f0, f1, weights, row_base=ROW_BASE + 2 ** 32), base), "the stream takes the low word of row_base + p"
    # discrete_turn, and next_ext left out
    turn = _policy(c, f0, f1, weights, turn=1)
    _exact(c, turn, SEED, DRAW, ROW_BASE, turn=1)
    assert _same(turn, base, keys=("actions", "cont", "probs", "logp", "value"))
    assert _same(_policy(c, f0, f1, weights, want_ext=False), base, keys=("actions", "cont", "probs", "logp", "value"))
    # the rows in another order: what is not drawn moves with its row, and the draw is that of the row's new stream
    perm = np.random.default_rng(1).permutation(P)
    moved = _policy(c, f0[perm], sub(f1, perm), weights)
    assert all(np.array_equal(moved[k].view(np.uint8), base[k][perm].view(np.uint8)) for k in ("probs", "value", "cont")), "a row's result depends on its index"
    _exact(c, moved, SEED, DRAW, ROW_BASE)
    # the batch around a row changes; the batch shrinks to the rows from `keep` on, and to that row alone, each keeping its stream
    rng = np.random.default_rng(2)
    for keep in sorted({0, P // 2, P - 1}):
        other = [rng.standard_normal(a.shape).astype(np.float32) if a is not None else None for a in (f0, f1)]
        for o, a in zip(other, (f0, f1)):
            if a is not None:
                o[keep] = a[keep]
        got = _policy(c, other[0], other[1], weights)
        assert _same(got, base, rows=slice(keep, keep + 1)), "row %d depends on the batch" % keep
        tail = _policy(c, f0[keep:], sub(f1, slice(keep, None)), weights, row_base=ROW_BASE + keep)
        assert all(np.array_equal(tail[k].view(np.uint8), base[k][keep:].view(np.uint8)) for k in tail), "row %d on depends on P or on p" % keep
        alone = _policy(c, f0[keep:keep + 1], sub(f1, slice(keep, keep + 1)), weights, row_base=ROW_BASE + keep)
        assert all(np.array_equal(alone[k].view(np.uint8), base[k][keep:keep + 1].view(np.uint8)) for k in alone), "row %d depends on P" % keep


def test_probabilities_of_zero_are_never_drawn_and_a_single_action_always():
    """an actor whose bias puts -200 on every second action of a group: softmax gives exactly 0 there in float32, and no row draws one"""
    c = dict(_case(CASES[3], "bf16"))
    P, F, two, nvec, Cn, AD = c["case"]
    pr = {k: v.copy() for k, v in c["pr"].items()}
    for g in range(2):
        pr["actor.blocks.0.Layer.%d.bias" % g][1::2] = -200.0
    c["pr"] = pr
    out = _policy(c, c["feat0"], c["feat1"], _dev_weights(pr, c["K"], nvec, Cn, "bf16"))
    assert (out["probs"][:, 1::2] == 0).all() and (out["actions"] % 2 == 0).all() and len(np.unique(out["actions"])) > 4
    _exact(c, out, SEED, DRAW, ROW_BASE)


def test_module_routes_fallbacks_the_counter_and_out_actions(monkeypatch):
    import torch
    from dynenv_amd import GpuPolicyHead
    K, nvec, Cn = 128, (5, 3, 3), 1
    P = 21
    pr = PR.make_params(K, nvec, Cn, seed=1)
    layer = PR.load(GpuPolicyHead(K, PR.space(nvec, Cn), seed=SEED), pr).cuda().requires_grad_(False)
    assert layer.last_route is None and layer.draw.is_cuda and int(layer.draw) == 0
    g = torch.Generator().manual_seed(0)
    feat = torch.randn((P, K), generator=g).cuda()
    out = layer.act(feat)
    assert layer.last_route == "fused" and out.log_probs.grad_fn is None and out.actions.dtype == torch.int32 and int(layer.draw) == 1
    probs = torch.cat(out.probs, 1).cpu().numpy()
    assert np.array_equal(out.actions.cpu().numpy()[:, :3], PR.draw_actions(probs, nvec, SEED, 0, 0)) and not out.actions[:, 3].any()
    assert out.head.dtype == torch.float64 and float(out.head.abs().max()) < PR.HIGH
    halves = layer.act(feat[:, :64].contiguous(), feat[:, 64:].contiguous())   # the same feature in two pieces
    assert layer.last_route == "fused" and int(layer.draw) == 2
    layer.reseed(SEED, 0)
    again = layer.act(feat[:, :64].contiguous(), feat[:, 64:].contiguous())
    for a, b in zip((out.actions, out.head, out.log_probs, out.value, out.next_ext) + tuple(out.probs),
                    (again.actions, again.head, again.log_probs, again.value, again.next_ext) + tuple(again.probs)):
        assert torch.equal(a, b), "cat(feat0, feat1) is never materialised, and is the same feature"
    assert not torch.equal(halves.actions, again.actions), "the counter advanced between the calls"
    # out_actions: written in place, in the step's layout
    static = torch.full((7, 3, 4), -1, dtype=torch.int32, device="cuda")
    layer.reseed(SEED, 0)
    res = layer.act(feat, out_actions=static)
    assert layer.last_route == "fused" and res.actions.data_ptr() == static.data_ptr() and torch.equal(static.view(P, 4), out.actions)
    # the torch route with the same draw: the same actions wherever its own float32 probabilities lead to them
    layer.requires_grad_(True)
    layer.reseed(SEED, 0)
    static.fill_(-1)
    t = layer.act(feat, out_actions=static)
    assert layer.last_route == "torch" and t.log_probs.grad_fn is not None and t.value.grad_fn is not None and int(layer.draw) == 1
    tp = torch.cat(t.probs, 1).detach().cpu().numpy()
    assert np.array_equal(static.view(P, 4).cpu().numpy()[:, :3], PR.draw_actions(tp, nvec, SEED, 0, 0)) and not static[..., 3].any()
    # (the routes differ by the rounding of the operands to bf16, 2^-9 relative: a logit moves by about 0.01, a probability by less, and
    # the head by 3 * 0.25 of it; a wrong draw or another feature would move them by 0.1 to 1)
    assert float(np.abs(tp - probs).max()) < 0.02 and float((t.head - out.head).abs().max()) < 0.05
    assert torch.equal(t.next_ext, _t(PR.transform_table(static.view(P, 4).cpu().numpy()).astype(np.float32)).cuda())
    layer.requires_grad_(False)

    def falls_back(lay, why, *args, **kw):
        with torch.no_grad():
            o = lay.act(*args, **kw)
        assert lay.last_route.startswith("torch (fallback: " + why), lay.last_route
        assert bool(torch.isfinite(o.value).all())
    monkeypatch.setenv("DYNENV_POLICY_FUSED", "0")
    falls_back(layer, "DYNENV_POLICY_FUSED=0", feat)
    monkeypatch.delenv("DYNENV_POLICY_FUSED")
    falls_back(GpuPolicyHead(96, PR.space(nvec), device="cuda").requires_grad_(False), "F = 96", feat[:, :96].contiguous())
    falls_back(GpuPolicyHead(64, PR.space((17, 3)), device="cuda").requires_grad_(False), "an action space beyond", feat[:, :64].contiguous())
    falls_back(GpuPolicyHead(K, PR.space(nvec, Cn)).requires_grad_(False), "features that are not on the device", feat.cpu())
    falls_back(layer, "features that are not float32, contiguous", feat.t().contiguous().t())
    falls_back(layer, "an out_actions that is not int32", feat, out_actions=torch.zeros((P, 4), dtype=torch.int64, device="cuda"))
    dbl = GpuPolicyHead(K, PR.space(nvec, Cn), device="cuda").double().requires_grad_(False)
    falls_back(dbl, "features that are not float32", feat.double())
    odd = PR.load(GpuPolicyHead(K, PR.space(nvec, Cn)), pr).cuda().requires_grad_(False)
    odd.critic.blocks.bn.weight.data = torch.ones(K, device="cuda")[::2]   # (not contiguous)
    falls_back(odd, "parameters that are not float32, contiguous", feat)
    with torch.no_grad():
        layer.requires_grad_(True)
        assert layer.act(feat).log_probs.grad_fn is None and layer.last_route == "fused"


def test_torch_route_gradients_against_a_float64_cpu_twin():
    """float32 on the device against float64 on the CPU: the same actions, and the parameters' gradients of sum(log_probs * W) +
    sum(value * V) agree to 1e-3 of the largest gradient entry of the parameter (test_gpu_recurrent.py's bound)"""
    import torch
    from dynenv_amd import GpuPolicyHead
    K, nvec, Cn, P = 128, (5, 3, 3, 7), 0, 12
    rng = np.random.default_rng(4)
    f0, f1 = rng.standard_normal((P, 64)).astype(np.float32), rng.standard_normal((P, 64)).astype(np.float32)
    W, V = torch.from_numpy(rng.standard_normal((P, 4))), torch.from_numpy(rng.standard_normal((P, 1)))
    pr = PR.make_params(K, nvec, Cn, seed=9)
    dev = PR.load(GpuPolicyHead(K, PR.space(nvec, Cn), seed=SEED), pr).cuda()
    twin = PR.load(GpuPolicyHead(K, PR.space(nvec, Cn), seed=SEED), pr).double()
    out = dev.act(_t(f0).cuda(), _t(f1).cuda(), row_base=5)
    assert dev.last_route == "torch"
    ((out.log_probs * W.float().cuda()).sum() + (out.value * V.float().cuda()).sum()).backward()
    out64 = twin.act(_t(f0).double(), _t(f1).double(), row_base=5)
    ((out64.log_probs * W).sum() + (out64.value * V).sum()).backward()
    assert torch.equal(out.actions.cpu(), out64.actions), "float32 and float64 probabilities led to other actions"
    assert np.array_equal(out.actions.cpu().numpy(), PR.draw_actions(torch.cat(out.probs, 1).detach().cpu().numpy(), nvec, SEED, 0, 5))
    assert float((out.log_probs.detach().double().cpu() - out64.log_probs.detach()).abs().max()) <= 1e-4
    for (k, p), q in zip(dev.named_parameters(), twin.parameters()):
        scale = float(q.grad.abs().max())
        err = float((p.grad.double().cpu() - q.grad).abs().max())
        print("grad %s: max %.3g err %.3g" % (k, scale, err))
        assert scale > 0 and err <= 1e-3 * scale, k


def _driving(E, seed=11):
    from dynenv_amd import BatchedDynEnv, DynEnvType
    return BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed)


def test_the_closed_loop_in_one_captured_graph():
    """step -> extractor -> action -> step with no host in it: step_flat(static_actions, auto_reset=False) + counts() +
    GpuFeatureExtractor(fixed=True, bfloat16, extended_feature_cnt=2) + GpuPolicyHead.act(feature, out_actions=static_actions), next_ext
    copied into the extractor's static position tensor, recorded once with torch.cuda.graph on one stream - a capture fails at the first
    synchronisation or host copy - and replayed four times with no host input in between; every replay bit for bit against an eagerly
    stepped twin whose counter starts at the same value"""
    import torch
    from dynenv_amd import GpuFeatureExtractor, GpuPolicyHead, groups_for
    E, F, X = 16, 64, 2
    env, twin = _driving(E), _driving(E)
    env.reset_flat()
    twin.reset_flat()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    P = E * A
    assert env.action_dim == X
    types = groups_for(env)["movable"]
    torch.manual_seed(9)
    kw = dict(extended_feature_cnt=X, fixed=True, padded_dtype=torch.bfloat16)
    nets = [GpuFeatureExtractor(types, F, E, A, T, D, **kw).requires_grad_(False) for _ in range(2)]
    pols = [GpuPolicyHead(F, env.action_space, seed=SEED, device="cuda").requires_grad_(False) for _ in range(2)]
    with torch.no_grad():
        for m in (nets[0], pols[0]):
            for k, p in m.named_parameters():
                if "bias" in k:
                    p.uniform_(-0.5, 0.5)
    nets[1].load_state_dict(nets[0].state_dict(), strict=True)
    pols[1].load_state_dict(pols[0].state_dict(), strict=True)
    acts = [torch.zeros((E, A, X), dtype=torch.int32, device="cuda") for _ in range(2)]
    exts = [torch.zeros((P, X), device="cuda") for _ in range(2)]

    def loop(e, net, pol, a, ext):
        obs, _, _ = e.step_flat(a, auto_reset=False)
        feature = net(obs, ext, e.counts())
        out = pol.act(feature, out_actions=a)
        ext.copy_(out.next_ext)
        return out
    # one eager call of the two layers first: the kernels' code objects are loaded outside the recording
    pols[0].act(nets[0](env.obs, exts[0], env.counts()))
    nets[0].reset()
    for pol in pols:
        pol.reseed(SEED, DRAW)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = loop(env, nets[0], pols[0], acts[0], exts[0])
    assert nets[0].last_route == ("fused", "fused", "fused") and pols[0].last_route == "fused"
    nets[0].reset()
    pols[0].reseed(SEED, DRAW)   # (whatever the recording itself did to the counter is gone)
    acts[0].zero_()
    exts[0].zero_()
    previous = None
    for r in range(4):
        graph.replay()
        want = loop(twin, nets[1], pols[1], acts[1], exts[1])
        assert nets[1].last_route == ("fused", "fused", "fused") and pols[1].last_route == "fused"
        assert torch.equal(env.obs.view(torch.int32), twin.obs.view(torch.int32)), "replay %d: obs" % r
        assert torch.equal(acts[0], acts[1]) and torch.equal(exts[0], exts[1]), "replay %d: actions" % r
        assert torch.equal(nets[0].h.view(torch.int32), nets[1].h.view(torch.int32)) and torch.equal(nets[0].c.view(torch.int32), nets[1].c.view(torch.int32))
        assert torch.equal(out.log_probs.view(torch.int32), want.log_probs.view(torch.int32)) and torch.equal(out.value.view(torch.int32), want.value.view(torch.int32))
        assert int(pols[0].draw) == int(pols[1].draw) == DRAW + r + 1, "the counter advances inside the graph"
        assert int(acts[0].min()) >= 0 and int(acts[0].max()) <= 2 and torch.equal(exts[0], acts[0].view(P, X).float() - 1)
        assert previous is None or not torch.equal(previous, acts[0]), "the actions change between replays"
        previous = acts[0].clone()
    assert env.error_flags() == 0 and twin.error_flags() == 0   # (bit 1 would be an action outside the space)
    env.close()
    twin.close()


def test_robocup_with_a_head_turn_steps_eagerly_on_the_policys_actions():
    """RoboCup with allowHeadTurn: [5, 3, 3] and the Box output; the discrete columns and `head` through step_flat((disc, head))"""
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuPolicyHead
    E, K = 8, 128
    env = BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, use_continuous_actions=True, seed=5)
    assert env.allow_head_turn and env.action_dim == 4
    A = env.n_agents
    P = E * A
    env.reset_flat()
    torch.manual_seed(3)
    pol = GpuPolicyHead(K, env.action_space, seed=SEED, device="cuda").requires_grad_(False)
    assert pol.nvec == [5, 3, 3] and pol.n_cont == 1 and pol.action_cols == 4
    lo, hi = float(env.action_space.spaces[1].low.min()), float(env.action_space.spaces[1].high.max())
    before = env.obs.clone()
    for s in range(3):
        out = pol.act(torch.randn((P, K), device="cuda"))
        assert pol.last_route == "fused"
        assert float(out.head.min()) > lo and float(out.head.max()) < hi and float(out.head.abs().max()) > 0.01
        acts = out.actions.cpu().numpy()
        assert np.array_equal(acts[:, :3], PR.draw_actions(torch.cat(out.probs, 1).cpu().numpy(), (5, 3, 3), SEED, s, 0)) and not acts[:, 3].any()
        assert np.array_equal(out.next_ext.cpu().numpy(), PR.transform_table(acts).astype(np.float32))
        env.step_flat((out.actions.view(E, A, 4)[..., :3], out.head.view(E, A)), auto_reset=False, validate=True)
    assert env.error_flags() == 0 and not torch.equal(before, env.obs)
    env.close()


def test_two_features_from_two_extractors_of_a_real_handle():
    """Driving, E = 4, F = 64, bf16: the movable and the static group's extractors give features[0:2]; act(feat0, feat1) on them, fused,
    against the float64 statement on the same two features within the CPU autocast error, three steps on the drawn actions"""
    import torch
    from dynenv_amd import GpuFeatureExtractor, GpuPolicyHead, groups_for
    E, F = 4, 64
    env = _driving(E)
    env.reset_flat()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    P = E * A
    torch.manual_seed(7)
    nets = [GpuFeatureExtractor(types, F, E, A, T, D, padded_dtype=torch.bfloat16).requires_grad_(False) for types in groups_for(env).values()]
    nvec = (3, 3)
    pr = PR.make_params(2 * F, nvec, 0, seed=2)
    pol = PR.load(GpuPolicyHead(2 * F, env.action_space, seed=SEED), pr).cuda().requires_grad_(False)
    cpu = PR.load(GpuPolicyHead(2 * F, env.action_space, seed=SEED), pr).requires_grad_(False)
    acts = torch.ones((E, A, 2), dtype=torch.int32, device="cuda")
    for s in range(3):
        obs, _, _ = env.step_flat(acts, auto_reset=False)
        ce = env.counts()
        feats = [net(obs, None, ce) for net in nets]
        pol.reseed(SEED, DRAW + s)
        out = pol.act(feats[0], feats[1], out_actions=acts)
        assert pol.last_route == "fused"
        f0, f1 = (f.cpu().numpy() for f in feats)
        assert np.abs(f0).max() > 0.01 and np.abs(f1).max() > 0.01 and not np.array_equal(f0, f1)
        ref = PR.head(np.concatenate([f0, f1], 1), pr, nvec)
        probs = torch.cat(out.probs, 1).cpu().numpy()
        err = _errors(ref, nvec, probs, out.value.cpu().numpy(), np.zeros((P, 0)), out.log_probs.cpu().numpy(), out.actions.cpu().numpy())
        cpu.reseed(SEED, DRAW + s)
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            o = cpu._act_torch(_t(f0), _t(f1), None, 0)
        err_cpu = _errors(ref, nvec, torch.cat(o.probs, 1).double().numpy(), o.value.double().numpy(), np.zeros((P, 0)), o.log_probs.double().numpy(),
                          o.actions.numpy())
        print("step %d: err_fused %s | err_cpu_autocast %s" % (s, _fmt(err), _fmt(err_cpu)))
        assert (err <= FACTOR * err_cpu).all()
        assert np.array_equal(acts.view(P, 2).cpu().numpy(), PR.draw_actions(probs, nvec, SEED, DRAW + s, 0))
    assert env.error_flags() == 0
    env.close()
