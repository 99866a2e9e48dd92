"""The fused attention on the device (csrc/attention_kernels.hip through dynenv_attend_pool and GpuTemporalAttention) against the numpy
float64 statement tests/attention_ref.py.  -m gpu.

Accuracy: err_fused = max |fused - ref64| over out [P, F]; err_cpu_autocast the same distance for the module's torch route run here on
the CPU under torch.autocast("cpu", dtype) on the same inputs - the reference's own arithmetic at the same operand width, computed at
run time, independent of the code under test and of the device.  Required: err_fused <= 4 * err_cpu_autocast (the embed kernel's factor:
room for another accumulation order and for where the 16-bit roundings fall; a structural mistake - a key too many or too few, no bias
key, no 1 / sqrt(F), the temporal mask from after the update - moves the result by 5e-2 to 2).  fp16 is the sharp test, bf16 the one
users run.  Every run prints both errors and that of the torch route under autocast on the device; measured figures: profiles/HISTORY.md,
the section of this kernel.  Inputs: standard-normal rows rounded to the 16-bit type; attention_ref.make_params (every bias in +-0.5);
counts: attention_ref.make_counts (tile edges, and the players the running key count and the zero query rows decide).
Exact checks take no tolerance: slots behind a count are never read, a player's row of out does not depend on p, on M or on the other
players, two calls give the same bits, n == 0 gives +0.0, guard bands stay."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(1, 49, 20, 128), (1, 96, 20, 64), (5, 10, 12, 128), (3, 72, 18, 64), (5, 1, 6, 64)]   # (T, M, P, F)
KINDS = ["bf16", "f16"]
CODE = {"bf16": 1, "f16": 2}
FACTOR = 4.0


def _tdtype(kind):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _masks(counts, M):
    import torch
    return [torch.from_numpy(m) for m in AR.masks_of(counts, M)]


def _padding_zeroed(padded, counts):
    """the tensor as the arranger writes it: +0.0 in every slot at or behind a count"""
    import torch
    x = padded.clone()
    x[torch.from_numpy(np.transpose(AR.masks_of(counts, padded.shape[1]), (0, 2, 1)))] = 0
    return x


def _autocast_err(padded, counts, pr, ref, device):
    """max |torch route under autocast - ref64|, on `device`"""
    import torch
    from dynenv_amd import GpuTemporalAttention
    T, M, P, F = padded.shape
    layer = AR.load(GpuTemporalAttention(F), pr).to(device)
    masks = [m.to(device) for m in _masks(counts, M)]
    with torch.no_grad(), torch.autocast(device, dtype=padded.dtype):
        got = layer._forward_torch((_padding_zeroed(padded, counts).to(device), masks))
    return float(np.abs(got.double().cpu().numpy() - ref).max())


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """one batch per shape and type, computed once and shared (nothing in it is written to afterwards)"""
    import torch
    T, M, P, F = shape
    rng = np.random.default_rng(31 * T + M + (kind == "f16"))
    counts = AR.make_counts(T, M, P)
    padded = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(_tdtype(kind))   # (live values everywhere: see _padding_zeroed)
    pr = AR.make_params(F, seed=T + M)
    ref = AR.attend_pool(padded.double().numpy(), counts, pr)
    return dict(T=T, M=M, P=P, F=F, kind=kind, counts=counts, padded=padded, pr=pr, ref=ref, err_cpu=_autocast_err(padded, counts, pr, ref, "cpu"))


def _dev_params(pr, kind):
    """the device tensors of dynenv_attend_pool's arguments, and the two host structs over them"""
    import torch
    from dynenv_amd import _capi
    dt = _tdtype(kind)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in pr.items()}
    keep = [t]

    def mha(a):
        w16 = [t[a + ".in_proj_weight"].to(dt), t[a + ".out_proj.weight"].to(dt), t[a + ".bias_k"].to(dt).reshape(-1), t[a + ".bias_v"].to(dt).reshape(-1)]
        keep.append(w16)
        return _capi.Mha(*[x.data_ptr() for x in w16 + [t[a + ".in_proj_bias"], t[a + ".out_proj.bias"]]])
    return keep, t, mha("objAtt"), mha("tempAtt")


def _attend_pool(padded, counts, pr, kind, P=None, F=None):
    """dynenv_attend_pool into a guard-banded out; returns it as a host array [P, F] (padded None: M == 0)"""
    import torch
    from dynenv_amd import _capi
    from test_gpu_arranger_dtype import Guarded
    lib = _capi.load()
    if padded is not None:
        T, M, P, F = padded.shape
        dev = padded.cuda().contiguous()
    else:
        T, M, dev = counts.shape[0], 0, None
    keep, t, obj, tmp = _dev_params(pr, kind)
    cnt = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
    out = Guarded(P * F, 4)
    vp = C.c_void_p
    rc = lib.dynenv_attend_pool(vp(dev.data_ptr()) if dev is not None else None, CODE[kind], vp(cnt.data_ptr()), T, M, P, F, C.byref(obj), C.byref(tmp),
                                vp(t["bn.weight"].data_ptr()), vp(t["bn.bias"].data_ptr()), AR.EPS, vp(t["confLayer.0.weight"].data_ptr()),
                                vp(t["confLayer.0.bias"].data_ptr()), vp(out.ptr()), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dynenv_last_error()
    torch.cuda.synchronize()
    return out.check("out", True).reshape(P, F).copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _module(c, **kw):
    import torch  # noqa: F401
    from dynenv_amd import GpuTemporalAttention
    return AR.load(GpuTemporalAttention(c["F"], **kw), c["pr"]).cuda().requires_grad_(False)


def test_the_counts_hold_the_required_players():
    for T, M, P, F in SHAPES:
        c = AR.make_counts(T, M, P)
        assert c.shape == (T, P) and c.min() >= 0 and c.max() <= M
        edges = [e for e in AR.TILE_EDGES + (M - 1, M) if 0 <= e <= M]
        assert {0, min(1, M), M} <= set(c[0]) and len(set(c[0]) & set(edges)) >= min(len(set(edges)), P - 5)
        assert (c.max(0) == 0).any() and ((c[0] == 0) & ((c[1:] > 0).all(0) if T > 1 else True)).any()
        assert ((c[0] == M) & (c[1:] == 0).all(0)).any()
        if T > 1:
            assert ((c[0] == M) & (c[-1] == 1)).any() and ((c[0] == 1) & (c[-1] == M)).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_c_abi_writes_every_element_of_out_and_nothing_else(shape, kind):
    c = _case(shape, kind)
    got = _attend_pool(c["padded"], c["counts"], c["pr"], kind)
    err = float(np.abs(got - c["ref"]).max())
    print("%s %s: err_fused %.3g err_cpu_autocast %.3g (C ABI)" % (shape, kind, err, c["err_cpu"]))
    assert np.isfinite(got).all() and err <= FACTOR * c["err_cpu"]
    none = c["counts"].max(0) == 0
    assert none.any() and not _bits(got)[none].any(), "n == 0 gives +0.0"
    # M == 0: +0.0 everywhere, whatever the counts say, and no padded tensor is needed
    empty = _attend_pool(None, c["counts"], c["pr"], kind, P=c["P"], F=c["F"])
    assert not _bits(empty).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_accuracy_against_float64_within_the_cpu_autocast_error(shape, kind):
    import torch
    c = _case(shape, kind)
    layer = _module(c)
    counts = torch.from_numpy(c["counts"]).cuda()
    with torch.no_grad():
        out = layer((_padding_zeroed(c["padded"], c["counts"]).cuda(), [m.cuda() for m in _masks(c["counts"], c["M"])]), counts)
    assert layer.last_route == "fused" and out.dtype == torch.float32 and tuple(out.shape) == (c["P"], c["F"])
    err_fused = float(np.abs(out.double().cpu().numpy() - c["ref"]).max())
    err_dev = _autocast_err(c["padded"], c["counts"], c["pr"], c["ref"], "cuda")
    print("%s %s: err_fused %.3g err_cpu_autocast %.3g err_device_autocast %.3g" % (shape, kind, err_fused, c["err_cpu"], err_dev))
    assert err_fused <= FACTOR * c["err_cpu"]


EXACT = [((5, 10, 12, 128), "bf16"), ((3, 72, 18, 64), "f16"), ((1, 49, 20, 128), "f16"), ((5, 1, 6, 64), "bf16")]


@pytest.mark.parametrize("shape, kind", EXACT, ids=str)
def test_exact_properties(shape, kind):
    import torch
    c = _case(shape, kind)
    T, M, P, F = shape
    padded, counts, pr = c["padded"], c["counts"], c["pr"]
    base = _attend_pool(padded, counts, pr, kind)
    assert np.array_equal(_bits(base), _bits(_attend_pool(padded, counts, pr, kind))), "two calls give the same bits"
    behind = torch.from_numpy(np.transpose(AR.masks_of(counts, M), (0, 2, 1)))
    # NaN bit patterns, or zeros, in every slot at or behind a count: the same bits
    for fill in (float("nan"), 0.0):
        x = padded.clone()
        x[behind] = fill
        assert np.array_equal(_bits(_attend_pool(x, counts, pr, kind)), _bits(base)), "a slot behind a count was read (%r)" % fill
    # the players in another order
    perm = np.random.default_rng(1).permutation(P)
    moved = _attend_pool(padded[:, :, perm].contiguous(), counts[:, perm], pr, kind)
    assert np.array_equal(_bits(moved), _bits(base[perm])), "a player's result depends on its index"
    # M grows with zero slots (into the kernel's larger row capacities: 32, 64 and 128 rows)
    for more in (3, 40, 100):
        if M + more > 128:
            continue
        wide = torch.zeros((T, M + more, P, F), dtype=padded.dtype)
        wide[:, :M] = padded
        assert np.array_equal(_bits(_attend_pool(wide, counts, pr, kind)), _bits(base)), "a player's result depends on M (+%d)" % more
    # every other player's data and counts change
    rng = np.random.default_rng(2)
    for keep in (0, P // 2, P - 1):
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(padded.dtype)
        x[:, :, keep] = padded[:, :, keep]
        cnt = rng.integers(0, M + 1, counts.shape).astype(np.int32)
        cnt[:, keep] = counts[:, keep]
        assert np.array_equal(_bits(_attend_pool(x, cnt, pr, kind))[keep], _bits(base)[keep]), "player %d depends on the batch" % keep
    # counts outside 0..M are clamped
    wild = counts.copy()
    wild[counts == M] = M + 1000
    wild[counts == 0] = -5
    assert np.array_equal(_bits(_attend_pool(padded, wild, pr, kind)), _bits(base))


def test_module_routes_and_fallbacks(monkeypatch):
    import torch
    from dynenv_amd import GpuTemporalAttention
    c = _case((3, 72, 18, 64), "bf16")
    T, M, P, F = 3, 72, 18, 64
    x16 = _padding_zeroed(c["padded"], c["counts"]).cuda()
    masks = [m.cuda() for m in _masks(c["counts"], M)]
    counts = torch.from_numpy(c["counts"]).cuda()
    layer = _module(c)
    assert layer.last_route is None
    given = layer((x16, masks), counts)
    assert layer.last_route == "fused" and given.grad_fn is None
    derived = layer((x16, masks))
    assert layer.last_route == "fused" and torch.equal(given.view(torch.int32), derived.view(torch.int32)), "obj_counts given or derived from the masks"

    def falls_back(lay, x, why):
        with torch.no_grad():
            out = lay((x, masks if x.shape[1] == M else [torch.ones((P, x.shape[1]), dtype=torch.bool, device="cuda")] * T))
        assert lay.last_route.startswith("torch (fallback: " + why), lay.last_route
        assert tuple(out.shape) == (P, x.shape[3]) and bool(torch.isfinite(out).all())
        return out
    f32 = falls_back(layer, x16.float(), "a padded tensor of float32")
    assert float((f32 - given).abs().max()) <= FACTOR * c["err_cpu"] + float(np.abs(f32.double().cpu().numpy() - c["ref"]).max())
    monkeypatch.setenv("DYNENV_ATT_FUSED", "0")
    falls_back(layer, x16, "DYNENV_ATT_FUSED=0")
    monkeypatch.delenv("DYNENV_ATT_FUSED")
    falls_back(GpuTemporalAttention(32, device="cuda").requires_grad_(False), x16[..., :32].contiguous(), "F = 32")
    falls_back(layer, torch.zeros((T, 129, P, F), dtype=torch.bfloat16, device="cuda"), "M = 129")
    falls_back(GpuTemporalAttention(F, num_heads=2, device="cuda").requires_grad_(False), x16, "num_heads = 2")
    falls_back(layer, x16.transpose(0, 1).contiguous().transpose(0, 1), "a padded tensor that is not contiguous")
    # the one shape routed by measurement: M = 1 at F = 128; DYNENV_ATT_FUSED=1 takes the kernel there too
    wide = GpuTemporalAttention(128, device="cuda").requires_grad_(False)
    one = torch.randn((T, 1, P, 128), device="cuda").to(torch.bfloat16)
    none = [torch.zeros((P, 1), dtype=torch.bool, device="cuda")] * T
    with torch.no_grad():
        slow = wide((one, none))
        assert wide.last_route.startswith("torch (fallback: M = 1 at F = 128")
        monkeypatch.setenv("DYNENV_ATT_FUSED", "1")
        fast = wide((one, none))
        # (the two routes on one input: bf16 operands against float32, within 4 x the largest bf16 err_cpu_autocast of this file, 1.3e-2)
        assert wide.last_route == "fused" and float((fast - slow).abs().max()) < 0.05
        monkeypatch.delenv("DYNENV_ATT_FUSED")
    # gradients wanted: the torch route, whatever the input's type
    layer.requires_grad_(True)
    out = layer((x16.float(), masks))
    assert layer.last_route == "torch" and out.grad_fn is not None
    with torch.no_grad():
        assert layer((x16, masks)).grad_fn is None and layer.last_route == "fused"
    cpu = GpuTemporalAttention(F)
    assert cpu((torch.zeros((1, 2, 3, F)), [torch.zeros((3, 2), dtype=torch.bool)])).shape == (3, F) and cpu.last_route == "torch"
    with torch.no_grad():
        cpu((torch.zeros((1, 2, 3, F), dtype=torch.bfloat16), [torch.zeros((3, 2), dtype=torch.bool)]))
    assert cpu.last_route.startswith("torch (fallback: a padded tensor that is not on the device")


def test_torch_route_gradients_against_a_float64_cpu_twin():
    """float32 on the device against float64 on the CPU: the parameters' gradients of sum(out * W) agree to 1e-3 of the largest gradient
    entry of the parameter (float32 rounding through a few hundred-term sums is 1e-5 of it; a wrong term is of its order)"""
    import torch
    from dynenv_amd import GpuTemporalAttention
    T, M, P, F = 3, 10, 12, 64
    counts = AR.make_counts(T, M, P)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.standard_normal((T, M, P, F)).astype(np.float32))
    x = _padding_zeroed(x, counts)
    W = torch.from_numpy(rng.standard_normal((P, F)))
    pr = AR.make_params(F, seed=9)
    dev = AR.load(GpuTemporalAttention(F), pr).cuda()
    twin = AR.load(GpuTemporalAttention(F), pr).double()
    out = dev((x.cuda(), [m.cuda() for m in _masks(counts, M)]))
    assert dev.last_route == "torch"
    (out * W.float().cuda()).sum().backward()
    out64 = twin((x.double(), _masks(counts, M)))
    (out64 * W).sum().backward()
    assert float((out.detach().double().cpu() - out64.detach()).abs().max()) <= 1e-4
    for (k, p), q in zip(dev.named_parameters(), twin.parameters()):
        scale = float(q.grad.abs().max())
        err = float((p.grad.double().cpu() - q.grad).abs().max())
        print("grad %s: max %.3g err %.3g" % (k, scale, err))
        assert scale > 0 and err <= 1e-3 * scale, k


def _make_env(cfg, E, seed=11):
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    part = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=3)
    if cfg == "driving_full":
        return BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed), [3, 3]
    if cfg == "driving_partial":
        return BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed, **part), [3, 3]
    if cfg == "robocup_partial":
        return BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=seed, **part), [5, 3, 3, 7]
    return BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=seed), [5, 3, 3, 7]


@pytest.mark.parametrize("cfg", ["driving_full", "driving_partial", "robocup_full", "robocup_partial"])
def test_end_to_end_from_a_real_handle(cfg):
    """a few steps into an episode, both object groups, F = 64, bf16: GpuEmbedInputLayer -> GpuTemporalAttention, the fused route against
    float64 on the real padded tensor, within the CPU autocast error on that tensor"""
    import torch
    from dynenv_amd import GpuEmbedInputLayer, GpuTemporalAttention, groups_for
    E, F = 4, 64
    env, hi = _make_env(cfg, E)
    env.reset_flat()
    rng = np.random.default_rng(3)
    for _ in range(4):
        obs, _, _ = env.step_flat(np.stack([rng.integers(0, k, (E, env.n_agents)) for k in hi], -1).astype(np.int32))
    obs = obs.contiguous()
    ce = env.counts()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    torch.manual_seed(7)
    for name, types in groups_for(env).items():
        layer = GpuEmbedInputLayer(types, F, E, A, T, D, padded_dtype=torch.bfloat16).requires_grad_(False)
        pr = AR.make_params(F, seed=len(name))
        att = AR.load(GpuTemporalAttention(F), pr).cuda().requires_grad_(False)
        padded, masks = layer(obs, ce)
        assert layer.last_route == "fused" and padded.dtype == torch.bfloat16
        out = att((padded, masks), layer.last_obj_counts)
        assert att.last_route == "fused"
        assert torch.equal(out.view(torch.int32), att((padded, masks)).view(torch.int32)), "counts from the masks"
        counts = layer.last_obj_counts.cpu().numpy()
        ref = AR.attend_pool(padded.double().cpu().numpy(), counts, pr)
        err_fused = float(np.abs(out.double().cpu().numpy() - ref).max())
        err_cpu = _autocast_err(padded.cpu(), counts, pr, ref, "cpu")
        err_dev = _autocast_err(padded.cpu(), counts, pr, ref, "cuda")
        print("%s %s M=%d n<=%d: err_fused %.3g err_cpu_autocast %.3g err_device_autocast %.3g" % (cfg, name, padded.shape[1], counts.max(), err_fused,
                                                                                                 err_cpu, err_dev))
        assert padded.shape[1] > 0 and err_fused <= FACTOR * err_cpu
    assert env.error_flags() == 0
    env.close()


def test_a_captured_step_with_the_input_layer_and_the_attention():
    """step_flat(auto_reset=False) + counts() + GpuEmbedInputLayer(fixed=True, bfloat16) + GpuTemporalAttention recorded once with
    torch.cuda.graph on one stream - a capture fails at the first synchronisation or host copy - and replayed on changing observations,
    against an eagerly stepped twin through the eager pair"""
    import torch
    from dynenv_amd import GpuEmbedInputLayer, GpuTemporalAttention, groups_for
    E, F = 16, 64
    env, hi = _make_env("driving_full", E)
    twin, _ = _make_env("driving_full", E)
    env.reset_flat()
    twin.reset_flat()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    types = groups_for(env)["movable"]
    torch.manual_seed(9)
    kw = dict(fixed=True, padded_dtype=torch.bfloat16)
    layer = GpuEmbedInputLayer(types, F, E, A, T, D, **kw).requires_grad_(False)
    eager = GpuEmbedInputLayer(types, F, E, A, T, D, **kw).requires_grad_(False)
    eager.load_state_dict(layer.state_dict(), strict=True)
    pr = AR.make_params(F, seed=2)
    att = AR.load(GpuTemporalAttention(F), pr).cuda().requires_grad_(False)
    eager_att = AR.load(GpuTemporalAttention(F), pr).cuda().requires_grad_(False)
    static_a = torch.zeros((E, A, env.action_dim), dtype=torch.int32, device="cuda")
    att(layer(env.obs, env.counts()), layer.last_obj_counts)   # one eager call first: the kernels' code objects are loaded outside the recording
    att(layer(env.obs, env.counts()))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obs, _, _ = env.step_flat(static_a, auto_reset=False)
        out = att(layer(obs, env.counts()), layer.last_obj_counts)
        out_from_masks = att(layer(obs, env.counts()))
    assert layer.last_route == "fused" and att.last_route == "fused"
    twin.step_flat(static_a.clone(), auto_reset=False)
    rng = np.random.default_rng(2)
    previous = None
    for r in range(3):
        if r:
            act = np.stack([rng.integers(0, k, (E, A)) for k in hi], -1).astype(np.int32)
            static_a.copy_(torch.from_numpy(act).cuda())
            twin.step_flat(static_a.clone(), auto_reset=False)
        graph.replay()
        assert torch.equal(env.obs.view(torch.int32), twin.obs.view(torch.int32)), "replay %d: the twin is elsewhere" % r
        want = eager_att(eager(twin.obs, twin.counts()), eager.last_obj_counts)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "replay %d" % r
        assert torch.equal(out_from_masks.view(torch.int32), want.view(torch.int32)), "replay %d, counts from the masks" % r
        assert bool(out.abs().sum() > 0) and (previous is None or not torch.equal(previous, out.view(torch.int32))), "the observations changed"
        previous = out.view(torch.int32).clone()
    assert env.error_flags() == 0
    env.close()
    twin.close()
