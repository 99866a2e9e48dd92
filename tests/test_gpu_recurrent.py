"""The fused recurrent head on the device (csrc/recurrent_kernels.hip through dynenv_recurrent_head, GpuRecurrentHead and
GpuFeatureExtractor) against the numpy float64 statement tests/recurrent_ref.py.  -m gpu.

Accuracy, over 3 chained calls so that h is fed back, with a reset mask at call 2: err_fused = the max over the calls of |out - ref64|,
and likewise for h and c; err_cpu_autocast the same three distances for the module's torch route run here on the CPU under
torch.autocast("cpu", dtype) on the same inputs - the reference's own arithmetic at the same operand width, computed at run time,
independent of the code under test and of the device.  Required, for each of out, h and c: err_fused <= 4 * err_cpu_autocast (the
embed and the attention kernels' factor: room for another accumulation order and for where the 16-bit roundings fall; a wrong gate
order, a missing bias or an unused h moves a LayerNormed output by 0.1 to 1).  fp16 is the sharp test, bf16 the one users run.  Every
run prints the errors and those of the torch route under autocast on the device; measured figures: profiles/HISTORY.md, the section of
this kernel.  Inputs: standard-normal features and positions; recurrent_ref.make_params (every bias in +-0.5).
Exact checks take no tolerance: guard bands, every element written, repeatability, independence of p, of P and of the other rows, a
reset environment's state never read, unlisted environments untouched by the mask."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recurrent_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
# (E, A, F, X): one row; one row past a strip; P = 130; P = 129 and X no multiple of 8; the cap on X; one row past a workgroup's 64 rows
SHAPES = [(1, 1, 64, 0), (6, 3, 128, 6), (13, 10, 64, 4), (43, 3, 128, 13), (9, 5, 64, 32), (5, 13, 128, 0)]
KINDS = ["bf16", "f16"]
CODE = {"bf16": 1, "f16": 2}
FACTOR = 4.0
STEPS = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_extractor_state_dict.json")


def _tdtype(kind):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _chain_errors(run, c):
    """the max over the calls of |x - ref64| for x = out, h, c; run(step) -> (h, c, out) as arrays after that call"""
    err = np.zeros(3)
    for s in range(STEPS):
        got = run(s)
        err = np.maximum(err, [float(np.abs(np.asarray(g, np.float64) - w).max()) for g, w in zip((got[2], got[0], got[1]), (c["ref"][s][2], c["ref"][s][0], c["ref"][s][1]))])
    return err


def _module_chain(c, device, autocast):
    """the three calls through a GpuRecurrentHead's torch route on `device` under autocast (or whichever route forward takes when
    autocast is None) -> errors (out, h, c)"""
    import torch
    from dynenv_amd import GpuRecurrentHead
    E, A, F, X = c["shape"]
    layer = RR.load(GpuRecurrentHead(F, A, E, X, operand_dtype=_tdtype(c["kind"])), c["pr"]).to(device).requires_grad_(False)

    def run(s):
        args = (_t(c["feats"][s]).to(device), None if not X else _t(c["exts"][s]).to(device), None if c["masks"][s] is None else _t(c["masks"][s]).to(device))
        with torch.no_grad():
            if autocast is None:
                out = layer(*args)
            else:
                with torch.autocast(device, dtype=_tdtype(c["kind"])):
                    out = layer._forward_torch(*args)
        return layer.h.double().cpu().numpy(), layer.c.double().cpu().numpy(), out.double().cpu().numpy()
    return _chain_errors(run, c), layer


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """one chain per shape and type, computed once and shared (nothing in it is written to afterwards)"""
    E, A, F, X = shape
    P = E * A
    rng = np.random.default_rng(17 * E + A + F + X + (kind == "f16"))
    feats = rng.standard_normal((STEPS, P, F)).astype(np.float32)
    exts = rng.standard_normal((STEPS, P, X)).astype(np.float32) if X else [None] * STEPS
    masks = [None] * STEPS
    masks[1] = (np.arange(E) % 3 == 0).astype(np.uint8)   # the mask at call 2 (environment 0 always listed)
    pr = RR.make_params(F, X, seed=E + X)
    ref, h, cc = [], np.zeros((P, F)), np.zeros((P, F))
    for s in range(STEPS):
        h, cc, out = RR.head_step(feats[s], exts[s], h, cc, masks[s], A, pr)
        ref.append((h, cc, out))
    c = dict(shape=shape, kind=kind, P=P, feats=feats, exts=exts, masks=masks, pr=pr, ref=ref)
    c["err_cpu"] = _module_chain(c, "cpu", True)[0]
    return c


def _dev_weights(pr, F, X, kind):
    """the device tensors of dynenv_rhead_t and the host struct over them"""
    import torch
    from dynenv_amd import _capi
    dt = _tdtype(kind)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in pr.items()}
    keep = [t, t["LSTM.cell.weight_ih"].to(dt), t["LSTM.cell.weight_hh"].to(dt)]
    w = _capi.Rhead()
    if X:
        KP = (F + X + 31) // 32 * 32
        tr = torch.zeros((F, KP), dtype=dt, device="cuda")
        tr[:, :F + X] = t["TransformNet.0.weight"]
        keep.append(tr)
        w.tr_w, w.tr_b, w.tr_ln_w, w.tr_ln_b = tr.data_ptr(), t["TransformNet.0.bias"].data_ptr(), t["TransformNet.2.weight"].data_ptr(), t["TransformNet.2.bias"].data_ptr()
    w.w_ih, w.w_hh = keep[1].data_ptr(), keep[2].data_ptr()
    w.b_ih, w.b_hh = t["LSTM.cell.bias_ih"].data_ptr(), t["LSTM.cell.bias_hh"].data_ptr()
    w.ln_w, w.ln_b = t["bn.weight"].data_ptr(), t["bn.bias"].data_ptr()
    return keep, w


def _head(pr, kind, A, feat, ext, h, c, mask, weights=None):
    """dynenv_recurrent_head with h, c and out between guard bands; h / c None: the state is left as sentinels (a reset environment's is
    never read).  Returns (h', c', out) as host arrays [P, F]"""
    import torch
    from dynenv_amd import _capi
    from test_gpu_arranger_dtype import Guarded
    lib = _capi.load()
    P, F = feat.shape
    X = 0 if ext is None else ext.shape[1]
    assert P % A == 0
    keep, w = weights if weights is not None else _dev_weights(pr, F, X, kind)
    fd = _t(np.asarray(feat, np.float32)).cuda()
    ed = None if ext is None else _t(np.asarray(ext, np.float32)).cuda()
    md = None if mask is None else _t(np.asarray(mask, np.uint8)).cuda()
    bufs = [Guarded(P * F, 4) for _ in range(3)]
    for b, v in zip(bufs, (h, c)):
        if v is not None:
            b.payload.view(torch.float32).copy_(_t(np.asarray(v, np.float32)).reshape(-1))
    vp = C.c_void_p
    rc = lib.dynenv_recurrent_head(vp(fd.data_ptr()), None if ed is None else vp(ed.data_ptr()), P // A, A, F, X, CODE[kind], C.byref(w), RR.SLOPE,
                                   RR.EPS, RR.EPS, None if md is None else vp(md.data_ptr()), vp(bufs[0].ptr()), vp(bufs[1].ptr()), vp(bufs[2].ptr()),
                                   vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dynenv_last_error()
    torch.cuda.synchronize()
    return tuple(b.check(n, True).reshape(P, F).copy() for b, n in zip(bufs, ("h", "c", "out")))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fmt(err):
    return " ".join("%.3g" % e for e in err)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_c_abi_accuracy_and_every_element_written_and_nothing_else(shape, kind):
    c = _case(shape, kind)
    E, A, F, X = shape
    state = [np.zeros((c["P"], F), np.float32)] * 2

    def run(s):
        got = _head(c["pr"], kind, A, c["feats"][s], c["exts"][s], state[0], state[1], c["masks"][s])
        state[0], state[1] = got[0], got[1]
        assert all(np.isfinite(g).all() for g in got)
        return got
    err = _chain_errors(run, c)
    print("%s %s (out, h, c): err_fused %s err_cpu_autocast %s (C ABI)" % (shape, kind, _fmt(err), _fmt(c["err_cpu"])))
    assert (err <= FACTOR * c["err_cpu"]).all()
    # every environment reset, the state left as it was allocated (sentinels): all of h, c and out written, and the values of a zero state
    every = _head(c["pr"], kind, A, c["feats"][0], c["exts"][0], None, None, np.ones(E, np.uint8))
    zero = np.zeros((c["P"], F), np.float32)
    assert _same(every, _head(c["pr"], kind, A, c["feats"][0], c["exts"][0], zero, zero, None))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_module_accuracy_against_float64_within_the_cpu_autocast_error(shape, kind):
    c = _case(shape, kind)
    err, layer = _module_chain(c, "cuda", None)
    assert layer.last_route == "fused"
    err_dev = _module_chain(c, "cuda", True)[0]
    print("%s %s (out, h, c): err_fused %s err_cpu_autocast %s err_device_autocast %s" % (shape, kind, _fmt(err), _fmt(c["err_cpu"]), _fmt(err_dev)))
    assert (err <= FACTOR * c["err_cpu"]).all()


EXACT = [((6, 3, 128, 6), "bf16"), ((13, 10, 64, 4), "f16"), ((43, 3, 128, 13), "f16"), ((5, 13, 128, 0), "bf16"), ((9, 5, 64, 32), "bf16")]


@pytest.mark.parametrize("shape, kind", EXACT, ids=str)
def test_exact_properties(shape, kind):
    c = _case(shape, kind)
    E, A, F, X = shape
    P, pr = c["P"], c["pr"]
    feat, ext = c["feats"][2], c["exts"][2]
    h0, c0 = (np.asarray(a, np.float32) for a in c["ref"][1][:2])   # a live state
    weights = _dev_weights(pr, F, X, kind)
    call = lambda f, e, h, cc, m, a=A: _head(pr, kind, a, f, e, h, cc, m, weights)  # noqa: E731
    base = call(feat, ext, h0, c0, None)
    assert _same(base, call(feat, ext, h0, c0, None)), "two calls from the same state give the same bits"
    assert _same(base, call(feat, ext, h0, c0, np.zeros(E, np.uint8))), "a NULL mask is an all-zero mask"
    sub = lambda a, idx: None if a is None else a[idx]  # noqa: E731
    # the rows in another order (no mask: a row's environment plays no part)
    perm = np.random.default_rng(1).permutation(P)
    moved = call(feat[perm], sub(ext, perm), h0[perm], c0[perm], None)
    assert _same(moved, [b[perm] for b in base]), "a row's result depends on its index"
    # the batch around a row changes, and shrinks to that row's environment alone
    rng = np.random.default_rng(2)
    for keep in sorted({0, P // 2, P - 1}):
        other = [rng.standard_normal(a.shape).astype(np.float32) if a is not None else None for a in (feat, ext, h0, c0)]
        for o, a in zip(other, (feat, ext, h0, c0)):
            if a is not None:
                o[keep] = a[keep]
        got = call(*other, None)
        assert _same([g[keep] for g in got], [b[keep] for b in base]), "row %d depends on the batch" % keep
        rows = np.arange(keep // A * A, keep // A * A + A)
        alone = call(feat[rows], sub(ext, rows), h0[rows], c0[rows], None)
        assert _same(alone, [b[rows] for b in base]), "row %d depends on P" % keep
    # a mask: the listed environments' rows are a call without a mask on zeroed h and c - also with NaN there beforehand, never read -
    # and the other rows are untouched by it
    mask = (np.arange(E) % 2 == 0).astype(np.uint8)
    listed = np.repeat(mask.astype(bool), A)
    hz, cz = h0.copy(), c0.copy()
    hz[listed] = 0
    cz[listed] = 0
    want = call(feat, ext, hz, cz, None)
    assert _same([w[~listed] for w in want], [b[~listed] for b in base])
    assert _same(call(feat, ext, h0, c0, mask), want), "a listed environment's rows are those of a zero state"
    hn, cn = h0.copy(), c0.copy()
    hn[listed] = np.nan
    cn[listed] = np.nan
    assert _same(call(feat, ext, hn, cn, mask), want), "the state of a listed environment was read"
    assert _same(call(feat, ext, h0, c0, mask * 255), want), "any non-zero byte lists an environment"
    if X == 0:   # w->tr_* are ignored: NULL (above) or anything else
        keep2, w2 = _dev_weights(pr, F, X, kind)
        w2.tr_w = w2.tr_b = w2.tr_ln_w = w2.tr_ln_b = w2.w_ih + 2
        assert _same(_head(pr, kind, A, feat, None, h0, c0, None, (keep2, w2)), base)
        assert not weights[1].tr_w and not weights[1].tr_b


def test_module_routes_and_fallbacks(monkeypatch):
    import torch
    from dynenv_amd import GpuRecurrentHead
    E, A, F, X = 6, 3, 64, 6
    P = E * A
    pr = RR.make_params(F, X, seed=1)
    layer = RR.load(GpuRecurrentHead(F, A, E, X), pr).cuda().requires_grad_(False)
    assert layer.last_route is None and layer.h.is_cuda
    g = torch.Generator().manual_seed(0)
    feat, pos = torch.randn((P, F), generator=g).cuda(), torch.randn((P, X), generator=g).cuda()
    out = layer(feat, pos)
    assert layer.last_route == "fused" and out.grad_fn is None and out.dtype == torch.float32 and tuple(out.shape) == (P, F)
    ptrs = (layer.h.data_ptr(), layer.c.data_ptr())
    layer(feat)   # position None: the reference skips TransformNet
    assert layer.last_route == "fused" and (layer.h.data_ptr(), layer.c.data_ptr()) == ptrs, "the state's pointers never change"
    layer(feat, pos, torch.zeros(E, dtype=torch.bool, device="cuda"))
    assert layer.last_route == "fused" and (layer.h.data_ptr(), layer.c.data_ptr()) == ptrs

    def falls_back(lay, why, *args):
        with torch.no_grad():
            o = lay(*args)
        assert lay.last_route.startswith("torch (fallback: " + why), lay.last_route
        assert bool(torch.isfinite(o).all())
    monkeypatch.setenv("DYNENV_RHEAD_FUSED", "0")
    falls_back(layer, "DYNENV_RHEAD_FUSED=0", feat, pos)
    monkeypatch.delenv("DYNENV_RHEAD_FUSED")
    falls_back(GpuRecurrentHead(32, A, E, device="cuda").requires_grad_(False), "F = 32", feat[:, :32].contiguous())
    falls_back(GpuRecurrentHead(F, A, E, 33, device="cuda").requires_grad_(False), "X = 33", feat, torch.zeros((P, 33), device="cuda"))
    falls_back(GpuRecurrentHead(F, A, E, 6).requires_grad_(False), "features that are not on the device", feat.cpu(), pos.cpu())
    falls_back(layer, "inputs or a state that are not float32, contiguous", feat.t().contiguous().t(), pos)
    dbl = GpuRecurrentHead(F, A, E, device="cuda").double().requires_grad_(False)
    falls_back(dbl, "inputs or a state that are not float32", feat.double())
    half = RR.load(GpuRecurrentHead(F, A, E, X), pr).cuda().requires_grad_(False)
    half.bn.weight.data = torch.ones(2 * F, device="cuda")[::2]   # (not contiguous)
    falls_back(half, "parameters that are not float32, contiguous", feat)
    layer.reset()
    with torch.no_grad():
        wrong = GpuRecurrentHead(F, A, E, 0, device="cuda").requires_grad_(False)
        try:   # a position where X == 0: the torch route's own error, whatever it is, after the route was named
            wrong(feat, pos)
        except RuntimeError:
            pass
        assert wrong.last_route.startswith("torch (fallback: a position of width 6, not X = 0")
    # gradients wanted: the torch route
    layer.requires_grad_(True)
    out = layer(feat, pos)
    assert layer.last_route == "torch" and out.grad_fn is not None and layer.h.grad_fn is not None
    with torch.no_grad():
        assert layer(feat, pos).grad_fn is None and layer.last_route == "fused" and (layer.h.data_ptr(), layer.c.data_ptr()) == ptrs


def test_the_state_is_carried_between_the_routes_and_reset_envs_is_reset_env():
    """torch route (gradients wanted, float32) -> fused -> torch, against float64; within the CPU autocast error of the whole chain"""
    import torch
    from dynenv_amd import GpuRecurrentHead
    c = _case((13, 10, 64, 4), "bf16")
    E, A, F, X = c["shape"]
    layer = RR.load(GpuRecurrentHead(F, A, E, X), c["pr"]).cuda()
    routes = []
    for s in range(STEPS):
        args = (_t(c["feats"][s]).cuda(), _t(c["exts"][s]).cuda(), None if c["masks"][s] is None else _t(c["masks"][s]).cuda())
        if s == 1:
            with torch.no_grad():
                out = layer(*args)
        else:
            out = layer(*args)
        routes.append(layer.last_route)
        err = [float(np.abs(g.detach().double().cpu().numpy() - w).max()) for g, w in zip((out, layer.h, layer.c), (c["ref"][s][2], c["ref"][s][0], c["ref"][s][1]))]
        print("call %d (%s): err (out, h, c) %s, err_cpu_autocast %s" % (s, layer.last_route, _fmt(err), _fmt(c["err_cpu"])))
        assert (np.array(err) <= FACTOR * c["err_cpu"]).all(), s
    assert routes == ["torch", "fused", "torch"]
    # reset_envs(mask), then forward == forward(reset_env=mask), bit for bit, on both routes' states
    layer.requires_grad_(False)
    twin = RR.load(GpuRecurrentHead(F, A, E, X), c["pr"]).cuda().requires_grad_(False)
    layer.detach()
    twin.set_states(layer.get_states())
    mask = _t(np.arange(E) % 4 == 1).cuda()
    feat, pos = _t(c["feats"][0]).cuda(), _t(c["exts"][0]).cuda()
    before = layer.get_states()
    layer.reset_envs(mask)
    rows = mask.repeat_interleave(A)
    assert not layer.h[rows].any() and not layer.c[rows].any() and torch.equal(layer.h[~rows], before[0][~rows]) and torch.equal(layer.c[~rows], before[1][~rows])
    a, b = layer(feat, pos), twin(feat, pos, mask)
    assert layer.last_route == twin.last_route == "fused"
    for x, y in ((a, b), (layer.h, twin.h), (layer.c, twin.c)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # reset(): every environment, in place
    ptr = layer.h.data_ptr()
    layer.reset(mask)
    assert layer.h.data_ptr() == ptr and not layer.h.any() and not layer.c.any()


def test_torch_route_gradients_against_a_float64_cpu_twin():
    """float32 on the device against float64 on the CPU, two chained calls with a reset mask at the second: the parameters' gradients of
    sum(out * W) agree to 1e-3 of the largest gradient entry of the parameter (the attention test's bound)"""
    import torch
    from dynenv_amd import GpuRecurrentHead
    E, A, F, X = 4, 3, 64, 6
    P = E * A
    rng = np.random.default_rng(4)
    feats, exts = rng.standard_normal((2, P, F)).astype(np.float32), rng.standard_normal((2, P, X)).astype(np.float32)
    W = torch.from_numpy(rng.standard_normal((P, F)))
    mask = torch.tensor([0, 1, 0, 0], dtype=torch.uint8)
    pr = RR.make_params(F, X, seed=9)
    dev = RR.load(GpuRecurrentHead(F, A, E, X), pr).cuda()
    twin = RR.load(GpuRecurrentHead(F, A, E, X), pr).double()
    dev(_t(feats[0]).cuda(), _t(exts[0]).cuda())
    out = dev(_t(feats[1]).cuda(), _t(exts[1]).cuda(), mask.cuda())
    assert dev.last_route == "torch"
    (out * W.float().cuda()).sum().backward()
    twin(_t(feats[0]).double(), _t(exts[0]).double())
    out64 = twin(_t(feats[1]).double(), _t(exts[1]).double(), mask)
    (out64 * W).sum().backward()
    assert float((out.detach().double().cpu() - out64.detach()).abs().max()) <= 1e-4
    for (k, p), q in zip(dev.named_parameters(), twin.parameters()):
        if k.startswith("LSTM.transformer"):
            assert p.grad is None and q.grad is None   # (set_state's layer: no part in forward)
            continue
        scale = float(q.grad.abs().max())
        err = float((p.grad.double().cpu() - q.grad).abs().max())
        print("grad %s: max %.3g err %.3g" % (k, scale, err))
        assert scale > 0 and err <= 1e-3 * scale, k


def test_a_reference_state_dict_loads_strict():
    """the names and shapes of the reference's DynEnvFeatureExtractor.state_dict() (tests/golden, held to the reference by
    test_recurrent_ref.py) into GpuFeatureExtractor, strict=True"""
    import torch
    from dynenv_amd import GpuFeatureExtractor, _capi
    gold = json.load(open(GOLDEN))
    feats = gold["features_per_object_type"]
    types, off = [], 0
    for f in feats:
        types.append(_capi.ArrType(off, f, 2, _capi.ARR_COUNT_CONST, 2, 0, 0, 0))
        off += 2 * f
    net = GpuFeatureExtractor(types, gold["feature_size"], gold["num_envs"], gold["num_players"], gold["num_time"], off,
                              extended_feature_cnt=gold["extended_feature_cnt"])
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(k, list(s)) for k, s in gold["state_dict"]]
    g = torch.Generator().manual_seed(1)
    sd = {k: torch.rand(tuple(s), generator=g) for k, s in gold["state_dict"]}
    net.load_state_dict(sd, strict=True)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in net.state_dict().items())
    assert net.last_route == (None, None, None) and not list(net.buffers())


def _make_env(cfg, E, seed=11):
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    part = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=3)
    if cfg == "driving_full":
        return BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed), [3, 3]
    return BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=seed, **part), [5, 3, 3, 7]


@pytest.mark.parametrize("cfg", ["driving_full", "robocup_partial"])
def test_end_to_end_from_a_real_handle(cfg):
    """a few steps into an episode, both object groups, E = 4, F = 64, bf16, X = 6, two consecutive observations so that the state is fed
    back, the second with a reset mask: GpuFeatureExtractor, all three routes fused, against the float64 chain of the three statements
    (arranger_embed_ref, attention_ref, recurrent_ref).  err_cpu_autocast: the float64 padded tensor rounded to bf16 (what the input
    layer stores; the reference's own blocks under autocast are no more exact), then the attention's and the head's torch routes on
    the CPU under autocast, chained."""
    import torch
    import arranger_embed_ref as ER
    import attention_ref as AR
    from dynenv_amd import GpuFeatureExtractor, GpuRecurrentHead, GpuTemporalAttention, groups_for
    E, F, X = 4, 64, 6
    env, hi = _make_env(cfg, E)
    env.reset_flat()
    rng = np.random.default_rng(3)
    step = lambda: env.step_flat(np.stack([rng.integers(0, k, (E, env.n_agents)) for k in hi], -1).astype(np.int32))[0].contiguous().clone()  # noqa: E731
    for _ in range(3):
        step()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    P = E * A
    seen = []
    for _ in range(2):
        obs = step()
        ce = env.counts()
        seen.append((obs, None if ce is None else ce.clone()))
    positions = [torch.from_numpy(rng.standard_normal((P, X)).astype(np.float32)) for _ in range(2)]
    masks = [None, torch.tensor([0, 1, 0, 1], dtype=torch.uint8)]
    torch.manual_seed(7)
    for name, types in groups_for(env).items():
        net = GpuFeatureExtractor(types, F, E, A, T, D, extended_feature_cnt=X, padded_dtype=torch.bfloat16).requires_grad_(False)
        att_pr, head_pr = AR.make_params(F, seed=len(name)), RR.make_params(F, X, seed=len(name))
        AR.load(net.AttNet, att_pr)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in head_pr.items()}, strict=False)
        for b in net.InNet.blocks:
            for ln in (b.bn1, b.bn2):
                ln.weight.data.uniform_(0.5, 1.5)
        params = [[b.state_dict()[k].cpu().numpy() for k in ER.PARAMS] for b in net.InNet.blocks]
        cpu_att = AR.load(GpuTemporalAttention(F), att_pr)
        cpu_head = RR.load(GpuRecurrentHead(F, A, E, X), head_pr).requires_grad_(False)
        h = c = np.zeros((P, F))
        for s, (obs, ce) in enumerate(seen):
            out = net(obs, positions[s].cuda(), ce, None if masks[s] is None else masks[s].cuda())
            assert net.last_route == ("fused", "fused", "fused"), net.last_route
            padded64, pl = ER.padded_default(obs.cpu().numpy(), list(types), params, F, None if ce is None else ce.cpu().numpy())
            feat64 = AR.attend_pool(padded64, pl["obj_counts"], att_pr)
            h, c, want = RR.head_step(feat64, positions[s].numpy(), h, c, None if masks[s] is None else masks[s].numpy(), A, head_pr)
            with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
                m = [torch.from_numpy(x) for x in AR.masks_of(pl["obj_counts"], padded64.shape[1])]
                feat_cpu = cpu_att._forward_torch((torch.from_numpy(padded64).to(torch.bfloat16), m)).float()
                out_cpu = cpu_head._forward_torch(feat_cpu, positions[s], masks[s])
            err_fused = float(np.abs(out.double().cpu().numpy() - want).max())
            err_cpu = float(np.abs(out_cpu.double().numpy() - want).max())
            print("%s %s call %d M=%d: err_fused %.3g err_cpu_autocast %.3g" % (cfg, name, s, padded64.shape[1], err_fused, err_cpu))
            assert padded64.shape[1] > 0 and err_fused <= FACTOR * err_cpu
    assert env.error_flags() == 0
    env.close()


def test_a_captured_step_with_the_whole_extractor():
    """step_flat(auto_reset=False) + counts() + GpuFeatureExtractor(fixed=True, bfloat16) with a static reset_env tensor recorded once with
    torch.cuda.graph on one stream - a capture fails at the first synchronisation or host copy - and replayed three times with changing
    actions, the mask set for two environments before the second replay; every replay bit for bit against an eagerly stepped twin
    through an eager extractor"""
    import torch
    from dynenv_amd import GpuFeatureExtractor, groups_for
    E, F, X = 16, 64, 6
    env, hi = _make_env("driving_full", E)
    twin, _ = _make_env("driving_full", E)
    env.reset_flat()
    twin.reset_flat()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    types = groups_for(env)["movable"]
    torch.manual_seed(9)
    kw = dict(extended_feature_cnt=X, fixed=True, padded_dtype=torch.bfloat16)
    net = GpuFeatureExtractor(types, F, E, A, T, D, **kw).requires_grad_(False)
    eager = GpuFeatureExtractor(types, F, E, A, T, D, **kw).requires_grad_(False)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.5, 0.5)
    eager.load_state_dict(net.state_dict(), strict=True)
    static_a = torch.zeros((E, A, env.action_dim), dtype=torch.int32, device="cuda")
    static_pos = torch.randn((E * A, X), device="cuda")
    static_mask = torch.zeros((E,), dtype=torch.uint8, device="cuda")
    net(env.obs, static_pos, env.counts(), static_mask)   # one eager call first: the kernels' code objects are loaded outside the recording
    net.reset()
    ptrs = (net.h.data_ptr(), net.c.data_ptr())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obs, _, _ = env.step_flat(static_a, auto_reset=False)
        out = net(obs, static_pos, env.counts(), static_mask)
    assert net.last_route == ("fused", "fused", "fused") and (net.h.data_ptr(), net.c.data_ptr()) == ptrs
    net.reset()   # (in place: whatever the recording itself did to the state is gone, the pointers stay)
    twin.step_flat(static_a.clone(), auto_reset=False)
    rng = np.random.default_rng(2)
    previous = None
    for r in range(3):
        if r:
            act = np.stack([rng.integers(0, k, (E, A)) for k in hi], -1).astype(np.int32)
            static_a.copy_(torch.from_numpy(act).cuda())
            twin.step_flat(static_a.clone(), auto_reset=False)
        if r == 1:
            static_mask[3] = 1
            static_mask[10] = 1
        if r == 2:
            static_mask.zero_()
        graph.replay()
        assert torch.equal(env.obs.view(torch.int32), twin.obs.view(torch.int32)), "replay %d: the twin is elsewhere" % r
        want = eager(twin.obs, static_pos, twin.counts(), static_mask.clone())
        assert eager.last_route == ("fused", "fused", "fused")
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "replay %d" % r
        assert torch.equal(net.h.view(torch.int32), eager.h.view(torch.int32)) and torch.equal(net.c.view(torch.int32), eager.c.view(torch.int32))
        assert bool(out.abs().sum() > 0) and (previous is None or not torch.equal(previous, out.view(torch.int32))), "the observations changed"
        previous = out.view(torch.int32).clone()
    assert env.error_flags() == 0
    env.close()
    twin.close()
