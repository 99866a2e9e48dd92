"""The fused embed-and-pad on the device (csrc/arranger_embed_kernels.hip through dynenv_arrange_embed_pad and GpuEmbedInputLayer) against
the numpy float64 statement tests/arranger_embed_ref.py and against the unfused route of the same module on the same device.  -m gpu.

Accuracy: err_fused = max |fused - ref64| over the whole padded tensor, err_blocks the same for the unfused route; required are
err_fused <= 4 * err_blocks and err_blocks <= 1e-4 (two correct float32 evaluations differ from the truth by amounts of the same order;
the factor leaves room for another summation order and variance formulation; a misplaced row shows as an error of order 1).  Inputs:
features uniform in [-1, 1], torch's default Linear init, LayerNorm weights in [0.5, 1.5] (arranger_embed_ref.make_params).  Measured
on an MI355X (F = 64 / 128, err_fused, err_blocks): see profiles/HISTORY.md, the section of this kernel; every test prints its figures.
Exact checks take no tolerance: padding is +0.0 bit for bit, guard bands stay, 16-bit results are .to(dtype) of the float32 result,
identical rows give identical bits, two calls give the same bits, the two modes agree on the leading slots.

Shapes: E3 T2 A2 with three types, feats (7, 4, 2), caps (3, 2, 4), one count mode each; E5 T2 A3 with cap 5 (more than 64 live rows of a
type: a full tile and a partial one); the static group of RoboCup Partial (four types, caps 16, 16, 28, 12), the fourth without any
object in the batch; the last two hold a (t, p) without objects (the first one's CONST type gives every player two)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_embed_ref as ER  # noqa: E402
import arranger_fixed_ref as FR  # noqa: E402
import arranger_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROW, ENV, CONST = R.COUNT_ROW, R.COUNT_ENV, R.COUNT_CONST
CASES = {   # (E, T, A, specs)
    "three types": (3, 2, 2, [(7, 3, ENV, 0, 4), (4, 2, CONST, 2, 2), (2, 4, ROW, -1, 6)]),
    "tiles": (5, 2, 3, [(5, 5, ROW, 3, 6), (3, 5, ENV, 0, 6)]),
    "robocup partial static": (2, 2, 2, [(6, 16, ROW, 0, 17), (6, 16, ROW, -2, 16), (8, 28, ROW, 0, 29), (5, 12, ROW, -3, 0)]),
}
WIDTHS = [64, 128]
CODE = {"f32": 0, "bf16": 1, "f16": 2}


def _tdtype(kind):
    import torch
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]


@functools.lru_cache(maxsize=None)
def _case(name, F):
    """one synthetic batch per shape and width, computed once and shared (nothing in it is written to afterwards)"""
    E, T, A, specs = CASES[name]
    rng = np.random.default_rng(7 * len(name) + F)
    obs, types, ce = R.make_dense(rng, E, T, A, specs, lead=1, trail=2)
    for ty in types:   # the features the bound was worked out for: uniform in [-1, 1]; the unused capacity stays JUNK
        blk = obs[..., ty.offset:ty.offset + ty.cap * ty.feat]
        live = blk != R.JUNK
        blk[live] = rng.uniform(-1, 1, int(live.sum())).astype(np.float32)
    # a (t, p) without any object: player (e 0, t 0, a 0) - ROW counts in its row, ENV counts of environment 0 - except where a CONST
    # type gives every player its objects ("three types")
    for i, ty in enumerate(types):
        if ty.count_mode == ROW:
            obs[0, 0, 0, ty.count_index] = 0.5
        elif ty.count_mode == ENV:
            ce[0, i] = 0
    params = ER.make_params(rng, [t.feat for t in types], F)
    if name == "tiles" and R.plan(obs, types, ce)["total"][0] % 64 == 0:   # a partial last tile: one more player without objects of type 0
        obs[1, 1, 1, types[0].count_index] = 0.5
    pl = R.plan(obs, types, ce)
    want, _ = ER.padded_default(obs, types, params, F, ce)
    return dict(E=E, T=T, A=A, P=E * A, F=F, n=len(types), obs=obs, types=types, ce=ce, params=params, pl=pl, M=pl["max_count"], want=want)


def _arr_types(types):
    from dynenv_amd import _capi
    return [_capi.ArrType(*(ty.astuple() + (0,))) for ty in types]


def _dev_params(params):
    import torch
    return [[torch.from_numpy(a).cuda() for a in p] if p is not None else None for p in params]


def _embed_pad(c, counts, M, kind="f32", params="own"):
    """dynenv_arrange_embed_pad into a guard-banded buffer; returns the payload as a host array [T, M, P, F] (float32, or uint16 bits)"""
    import torch
    from dynenv_amd import _capi
    from test_gpu_arranger_dtype import Guarded
    lib = _capi.load()
    T, P, F, n = c["T"], c["P"], c["F"], c["n"]
    dev = _dev_params(c["params"] if params == "own" else params)
    blocks = (_capi.EmbedBlock * n)(*[_capi.EmbedBlock(*[t.data_ptr() for t in p]) if p is not None else _capi.EmbedBlock() for p in dev])
    types = (_capi.ArrType * n)(*_arr_types(c["types"]))
    obs = torch.from_numpy(c["obs"]).cuda()
    cnt = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
    size = 4 if kind == "f32" else 2
    out = Guarded(max(T * M * P * F, 8), size)
    vp = C.c_void_p
    rc = lib.dynenv_arrange_embed_pad(vp(obs.data_ptr()), c["E"], T, c["A"], c["obs"].shape[3], types, n, vp(cnt.data_ptr()), M, blocks, F, 0.1, 1e-5,
                                      vp(out.ptr()), CODE[kind], vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dynenv_last_error()
    torch.cuda.synchronize()
    if M == 0:
        out.check("padded (max_count 0)", False)
        return None
    return out.check("padded", True).reshape(T, M, P, F)


def _padding_is_plus_zero(got, obj_counts):
    """every slot at or behind a player's object count holds all-zero bits"""
    M = got.shape[1]
    behind = np.arange(M)[None, :, None] >= np.minimum(obj_counts, M)[:, None, :]
    bits = got.view(np.uint32 if got.dtype == np.float32 else np.uint16)
    assert not bits[behind].any(), "padding is not +0.0"
    return int(behind.sum())


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("name", list(CASES))
def test_c_abi_writes_every_element_once_and_nothing_else(name, F):
    c = _case(name, F)
    pl, M, want = c["pl"], c["M"], c["want"]
    assert (pl["obj_counts"] == 0).any() or name == "three types", "a (t, p) without objects"
    assert name != "robocup partial static" or (pl["total"][3] == 0 and pl["total"][:3].all()), "a type without objects in the batch"
    assert name != "tiles" or (pl["total"][0] > 64 and pl["total"][0] % 64), "more than a tile of live rows and a partial last tile"
    got = _embed_pad(c, pl["counts"], M)
    err = float(np.abs(got - want).max())
    print("%s F=%d: err_fused %.3g (C ABI, M = %d)" % (name, F, err, M))
    assert err <= 1e-4, "an error of order 1 is a misplaced row"
    assert _padding_is_plus_zero(got, pl["obj_counts"]) > 0
    assert np.array_equal(got.view(np.uint32), _embed_pad(c, pl["counts"], M).view(np.uint32)), "two calls give the same bits"
    # M above the batch's maximum: the same leading slots bit for bit, +0.0 behind
    more = _embed_pad(c, pl["counts"], M + 3)
    assert np.array_equal(more[:, :M].view(np.uint32), got.view(np.uint32)) and not more[:, M:].view(np.uint32).any()
    # M below it: the kernel clamps to the slots left, earlier types winning
    less = _embed_pad(c, pl["counts"], M - 2)
    want_less, _ = ER.padded_default(c["obs"], c["types"], c["params"], F, c["ce"], M=M - 2)
    assert np.abs(less - want_less).max() <= 1e-4
    kept = FR.plan_from_counts(pl["counts"], [t.cap for t in c["types"]], M - 2)
    assert kept["dropped"].any()
    _padding_is_plus_zero(less, kept["obj_counts"])
    # max_count == 0 launches nothing
    assert _embed_pad(c, pl["counts"], 0) is None
    # the 16-bit tensors are the float32 result converted, bit for bit
    import torch
    for kind in ("bf16", "f16"):
        bits = _embed_pad(c, pl["counts"], M, kind)
        conv = torch.from_numpy(got).to(_tdtype(kind)).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(bits, conv), kind


@pytest.mark.parametrize("F", WIDTHS)
def test_counts_are_clamped_and_a_null_block_writes_zeros(F):
    c = _case("three types", F)
    caps = np.array([t.cap for t in c["types"]])
    # counts far above the capacities (and below zero for one player): every capacity row is embedded, JUNK included, nothing is read
    # or written out of bounds
    wild = np.full_like(c["pl"]["counts"], 1000)
    wild[:, 0, 0] = -7
    kept = np.broadcast_to(caps[:, None, None], wild.shape).copy()
    kept[:, 0, 0] = 0
    M = int(caps.sum())
    got = _embed_pad(c, wild, M)
    want = ER.padded_from_plan(c["obs"], c["types"], kept, np.cumsum(kept, 0) - kept, M, c["params"], F)
    assert np.abs(got - want).max() <= 1e-4
    assert not got[0, :, 0].view(np.uint32).any()
    # a type WITH objects and NULL weights: +0.0 in its slots, everything else bit for bit as before
    full = _embed_pad(c, c["pl"]["counts"], c["M"])
    holed = _embed_pad(c, c["pl"]["counts"], c["M"], params=[c["params"][0], None, c["params"][2]])
    changed = holed.view(np.uint32) != full.view(np.uint32)
    assert changed.any() and not holed.view(np.uint32)[changed].any()
    want_holed, _ = ER.padded_default(c["obs"], c["types"], [c["params"][0], None, c["params"][2]], F, c["ce"])
    assert np.array_equal(changed.any(-1), (want_holed != c["want"]).any(-1))


@pytest.mark.parametrize("F", WIDTHS)
def test_identical_rows_give_identical_bits(F):
    """every object of a type carries the same features, at different slots, players, times, lanes and waves: one bit pattern per type"""
    c = dict(_case("tiles", F))
    obs = c["obs"].copy()
    rng = np.random.default_rng(F)
    for ty in c["types"]:
        row = rng.uniform(-1, 1, ty.feat).astype(np.float32)
        obs[..., ty.offset:ty.offset + ty.cap * ty.feat] = np.tile(row, ty.cap)
    c["obs"] = obs
    got = _embed_pad(c, c["pl"]["counts"], c["M"])
    pl = c["pl"]
    before = np.cumsum(pl["counts"], 0) - pl["counts"]
    j = np.arange(c["M"])[None, :, None]
    for i in range(c["n"]):
        own = (j >= before[i][:, None, :]) & (j < (before[i] + pl["counts"][i])[:, None, :])
        rows = got[own]
        assert rows.shape[0] == pl["total"][i] > 64 or i
        assert len(np.unique(rows.view(np.uint32), axis=0)) == 1, "type %d: the result depends on where the object sits" % i


def _layer(c, fixed=None, padded_dtype=None):
    import torch
    from dynenv_amd import GpuEmbedInputLayer
    layer = GpuEmbedInputLayer(_arr_types(c["types"]), c["F"], c["E"], c["A"], c["T"], c["obs"].shape[3], fixed=fixed, padded_dtype=padded_dtype)
    state = {"blocks.%d.%s" % (i, k): torch.from_numpy(a) for i, p in enumerate(c["params"]) for k, a in zip(ER.PARAMS, p)}
    layer.load_state_dict(state, strict=True)
    return layer


def _run(layer, c, route):
    import torch
    obs, ce = torch.from_numpy(c["obs"]).cuda(), torch.from_numpy(c["ce"]).cuda()
    with torch.no_grad():
        padded, masks = layer(obs, ce) if route == "fused" else layer._forward_blocks(obs, ce)
    if route == "fused":
        assert layer.last_route == "fused"
    return padded, torch.stack(masks)


MODES = ["default", "fixed above", "fixed below"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("name", list(CASES))
def test_module_against_float64_and_against_its_unfused_route(name, F, mode):
    import torch
    c = _case(name, F)
    caps = [t.cap for t in c["types"]]
    if mode == "default":
        fixed, want, M, dropped = None, c["want"], c["M"], None
        obj = c["pl"]["obj_counts"]
    else:
        M = c["M"] + 3 if mode == "fixed above" else c["M"] - 2
        fixed = dict(max_count=M, rows=caps)
        want, fp = ER.padded_fixed(c["obs"], c["types"], caps, M, c["params"], F, c["ce"])
        obj, dropped = fp["obj_counts"], fp["dropped"]
        assert dropped.any() == (mode == "fixed below")
    fused_layer, blocks_layer = _layer(c, fixed), _layer(c, fixed)
    fused, fmask = _run(fused_layer, c, "fused")
    blocks, bmask = _run(blocks_layer, c, "blocks")
    assert tuple(fused.shape) == tuple(blocks.shape) == (c["T"], M, c["P"], F) and fused.dtype == torch.float32
    got = fused.cpu().numpy()
    err_fused, err_blocks = float(np.abs(got - want).max()), float(np.abs(blocks.cpu().numpy() - want).max())
    print("%s F=%d %s: err_fused %.3g err_blocks %.3g" % (name, F, mode, err_fused, err_blocks))
    assert err_blocks <= 1e-4, "a condition on the inputs"
    assert err_fused <= 4 * err_blocks
    _padding_is_plus_zero(got, obj)
    assert torch.equal(fmask, bmask) and np.array_equal(fmask.cpu().numpy(), np.arange(M)[None, None, :] >= obj[:, :, None])
    assert torch.equal(fused_layer.last_counts, blocks_layer.arranger.rearrange_inputs(torch.from_numpy(c["obs"]).cuda(), torch.from_numpy(c["ce"]).cuda())[1][0])
    if fixed is not None:
        assert np.array_equal(fused_layer.arranger.dropped.cpu().numpy(), dropped)
        assert np.array_equal(blocks_layer.arranger.dropped.cpu().numpy(), 2 * dropped)   # (its forward, and the rearrange_inputs above)
    if mode == "fixed above":   # nothing drops: the two modes agree on the leading slots bit for bit
        dflt, _ = _run(_layer(c), c, "fused")
        assert torch.equal(fused[:, :c["M"]].view(torch.int32), dflt.view(torch.int32)) and not bool(fused[:, c["M"]:].view(torch.int32).any())
    for dt in (torch.bfloat16, torch.float16):   # padded_dtype: the float32 result converted, bit for bit
        p16, m16 = _run(_layer(c, fixed, dt), c, "fused")
        assert p16.dtype == dt and torch.equal(p16.view(torch.int16), fused.to(dt).view(torch.int16)) and torch.equal(m16, fmask)


def test_routes_gradients_and_fallbacks(monkeypatch):
    import torch
    from dynenv_amd import GpuEmbedInputLayer, GpuInputLayer
    c = _case("three types", 64)
    obs, ce = torch.from_numpy(c["obs"]).cuda(), torch.from_numpy(c["ce"]).cuda()
    layer = _layer(c)
    assert layer.last_route is None and sorted(k for k, _ in layer.named_parameters()) == sorted(
        "blocks.%d.%s" % (i, k) for i in range(c["n"]) for k in ER.PARAMS) and not list(layer.buffers())
    with torch.no_grad():
        fused, fmasks = layer(obs, ce)
    assert layer.last_route == "fused" and fused.grad_fn is None
    # gradients wanted: the existing route, and GpuInputLayer's gradients over the same blocks
    W = torch.randn(tuple(fused.shape), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    padded, masks = layer(obs, ce)
    assert layer.last_route == "blocks" and padded.grad_fn is not None
    (padded * W).sum().backward()
    mine = [p.grad.clone() for p in layer.parameters()]
    layer.zero_grad(set_to_none=True)
    twin = GpuInputLayer(layer.blocks, _arr_types(c["types"]), c["E"], c["A"], c["T"], c["obs"].shape[3])
    padded2, masks2 = twin(obs, ce)
    (padded2 * W).sum().backward()
    assert torch.equal(padded, padded2) and all(torch.equal(a, b) for a, b in zip(masks, masks2))
    assert all(torch.equal(g, p.grad) for g, p in zip(mine, layer.parameters())) and all(bool(g.abs().sum() > 0) for g in mine)
    # frozen parameters: nothing to differentiate, gradients enabled or not
    layer.requires_grad_(False)
    again, _ = layer(obs, ce)
    assert layer.last_route == "fused" and torch.equal(again.view(torch.int32), fused.view(torch.int32))
    # what the kernel does not take falls back without raising, and says why
    monkeypatch.setenv("DYNENV_ARR_EMBED_FUSED", "0")
    off, _ = layer(obs, ce)
    assert layer.last_route.startswith("blocks (fallback: DYNENV_ARR_EMBED_FUSED=0") and torch.equal(off, padded.detach())
    monkeypatch.delenv("DYNENV_ARR_EMBED_FUSED")
    narrow = GpuEmbedInputLayer(_arr_types(c["types"]), 32, c["E"], c["A"], c["T"], c["obs"].shape[3])
    with torch.no_grad():
        out, _ = narrow(obs, ce)
    assert narrow.last_route.startswith("blocks (fallback: F = 32") and tuple(out.shape) == (c["T"], c["M"], c["P"], 32)
    layer.blocks[1].double()
    with torch.no_grad():
        assert layer._not_fusable().startswith("parameters that are not float32")
    plain = _layer(c)
    plain.blocks[0].bn2 = torch.nn.LayerNorm(64, elementwise_affine=False).cuda()
    with torch.no_grad():
        out, _ = plain(obs, ce)
    assert plain.last_route.startswith("blocks (fallback: a LayerNorm without affine")
    # autocast: the fused route stays float32 inside (only the store converts)
    auto = _layer(c, None, torch.bfloat16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        p16, _ = auto(obs, ce)
    assert auto.last_route == "fused" and torch.equal(p16.view(torch.int16), fused.to(torch.bfloat16).view(torch.int16))


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
    """a few steps into an episode, both object groups, F = 64: the fused route against float64 and against the unfused route"""
    import torch
    from dynenv_amd import GpuEmbedInputLayer, groups_for
    E, F = 8, 64
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
        layer = GpuEmbedInputLayer(types, F, E, A, T, D)
        for b in layer.blocks:
            for ln in (b.bn1, b.bn2):
                ln.weight.data.uniform_(0.5, 1.5)
        with torch.no_grad():
            fused, fmasks = layer(obs, ce)
            assert layer.last_route == "fused"
            blocks, bmasks = layer._forward_blocks(obs, ce)
        params = [[b.state_dict()[k].cpu().numpy() for k in ER.PARAMS] for b in layer.blocks]
        want, pl = ER.padded_default(obs.cpu().numpy(), list(types), params, F, None if ce is None else ce.cpu().numpy())
        assert tuple(fused.shape) == want.shape and pl["max_count"] > 0
        err_fused, err_blocks = float(np.abs(fused.cpu().numpy() - want).max()), float(np.abs(blocks.cpu().numpy() - want).max())
        print("%s %s: err_fused %.3g err_blocks %.3g, %d objects" % (cfg, name, err_fused, err_blocks, int(pl["total"].sum())))
        assert err_blocks <= 1e-4 and err_fused <= 4 * err_blocks
        _padding_is_plus_zero(fused.cpu().numpy(), pl["obj_counts"])
        assert all(torch.equal(a, b) for a, b in zip(fmasks, bmasks))
    assert env.error_flags() == 0
    env.close()


def test_a_captured_step_with_the_fused_input_layer():
    """step_flat(auto_reset=False) + counts() + GpuEmbedInputLayer(fixed=True) recorded once with torch.cuda.graph - a capture fails at the
    first synchronisation or host copy - and replayed on changing observations, against an eagerly stepped twin through an eager layer"""
    import torch
    from dynenv_amd import GpuEmbedInputLayer, groups_for
    E, F = 16, 64
    env, hi = _make_env("driving_full", E)
    twin, _ = _make_env("driving_full", E)
    env.reset_flat()
    twin.reset_flat()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    types = groups_for(env)["movable"]
    torch.manual_seed(9)
    layer = GpuEmbedInputLayer(types, F, E, A, T, D, fixed=True).requires_grad_(False)
    eager = GpuEmbedInputLayer(types, F, E, A, T, D, fixed=True).requires_grad_(False)
    eager.load_state_dict(layer.state_dict(), strict=True)
    static_a = torch.zeros((E, A, env.action_dim), dtype=torch.int32, device="cuda")
    layer(env.obs, env.counts())   # one eager call first: the kernels' code objects are loaded outside the recording
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obs, _, _ = env.step_flat(static_a, auto_reset=False)
        out = layer(obs, env.counts())
    assert layer.last_route == "fused"
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
        want, want_masks = eager(twin.obs, twin.counts())
        got, got_masks = out
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "replay %d: padded" % r
        assert torch.equal(torch.stack(got_masks), torch.stack(want_masks))
        assert previous is None or not torch.equal(previous, got.view(torch.int32)), "the observations changed between the replays"
        previous = got.view(torch.int32).clone()
        assert not bool(layer.arranger.dropped.any())
    assert env.error_flags() == 0
    env.close()
    twin.close()
