"""The arranger's backward on the GPU (arr_unpad_cols_kernel / arr_unscatter_kernel through the C ABI, and through autograd from
GpuInOutArranger.rearrange_outputs and GpuInputLayer), bit for bit against
  (1) the gradients autograd returned through the reference's own InOutArranger (tests/golden/arranger_grad.npz), and
  (2) the numpy restatement tests/arranger_grad_ref.py: unpad
at the smallest shapes at which these kernels can go wrong: every count residue of the 4-slot unroll, player counts that are no
multiple of a wave with more than one time step, both forward routes, the row-gather fallbacks, a type without a gradient, clamped
counts, guard bands, a plan that a later call must not overwrite, and real ragged observations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_ref as R  # noqa: E402
import arranger_grad_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu
ROW, ENV, CONST = R.COUNT_ROW, R.COUNT_ENV, R.COUNT_CONST


def _arr_types(types):
    from dynenv_amd import _capi
    return [_capi.ArrType(*(ty.astuple() + (0,))) for ty in types]


def _same_bits(got, want, what):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d of %d floats differ, first at %s" % (what, len(bad), got.size, bad[0].tolist()))


def _upstream(G_np, kind):
    """the upstream gradient on the device: as it is, a permuted non-contiguous view, or a contiguous view 4 bytes off alignment"""
    import torch
    if kind == "permuted":
        g = torch.from_numpy(np.ascontiguousarray(G_np.transpose(0, 2, 1, 3))).cuda().permute(0, 2, 1, 3)
        assert not g.is_contiguous()
    elif kind == "misaligned":
        buf = torch.empty((G_np.size + 1,), dtype=torch.float32, device="cuda")
        g = buf[1:].view(G_np.shape)
        g.copy_(torch.from_numpy(G_np))
        assert g.is_contiguous() and g.data_ptr() % 16 == 4
    else:
        g = torch.from_numpy(G_np).cuda()
    assert tuple(g.shape) == G_np.shape
    return g


def check_backward(obs_np, types, ce_np, F, seed=0, upstream="plain", frozen=(), arr_types=None):
    """rearrange_inputs + rearrange_outputs on leaf embeddings that require grad (None for a type without objects; `frozen`: types
    whose embedding does not), backward of a random upstream gradient: the padded tensor == arranger_ref.pad and every .grad == unpad,
    bit for bit.  Returns (plan, the route the backward took)."""
    import torch
    from dynenv_amd import GpuInOutArranger
    E, T, A, D = obs_np.shape
    P = E * A
    arr = GpuInOutArranger(arr_types if arr_types is not None else _arr_types(types), E, A, T, D)
    ce = torch.from_numpy(np.ascontiguousarray(ce_np, np.int32)).cuda() if ce_np is not None else None
    inputs, countArr = arr.rearrange_inputs(torch.from_numpy(obs_np).cuda(), ce)
    pl = R.plan(obs_np, types, ce_np)
    _, r_sl, _ = R.gather(obs_np, types, pl)
    M = pl["max_count"]
    assert countArr[1] == M
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal((len(s), F)).astype(np.float32) if len(s) else None for s in r_sl]
    embs = [torch.from_numpy(h).cuda().requires_grad_(i not in frozen) if h is not None else None for i, h in enumerate(host)]
    padded, _ = arr.rearrange_outputs(embs, countArr)
    assert padded.grad_fn is not None and padded.requires_grad
    _same_bits(padded, R.pad(host, r_sl, T, M, P, F), "padded")
    G_np = rng.standard_normal((T, M, P, F)).astype(np.float32)
    padded.backward(_upstream(G_np, upstream))
    want = GR.unpad(G_np, r_sl)
    for i, e in enumerate(embs):
        if e is None:
            continue
        if i in frozen:
            assert e.grad is None, "type %d does not require grad" % i
        else:
            assert e.grad is not None and e.grad.is_contiguous()
            _same_bits(e.grad, want[i], "gradient of type %d" % i)
    return pl, arr.last_backward


# ---- the reference's recorded gradients ----
def _golden_on_device(c):
    import torch
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    return i32(c["plan"]["counts"]), i32(c["plan"]["base"]), [i32(s) for s in c["slots"]]


@pytest.mark.parametrize("name", GR.CASES)
def test_c_abi_reproduces_the_reference_gradients(name):
    """dynenv_arrange_pad_backward (one call) and dynenv_arrange_scatter_backward (one call per type) on counts / base / slots built on
    the host from the fixture's counts"""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    c = GR.golden_case(name)
    counts, base, slots = _golden_on_device(c)
    T, P, M, F, n = c["T"], c["P"], c["plan"]["max_count"], c["F"], c["nT"]
    assert F % 4 == 0, "every recorded width takes the fused kernel (12 among them)"
    G = torch.from_numpy(c["G"]).cuda()
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    rows = [len(s) for s in c["slots"]]
    outs = [torch.full((r, F), float("nan"), device="cuda") for r in rows]
    ptrs = (vp * n)(*[o.data_ptr() if r else None for o, r in zip(outs, rows)])
    _capi.check(lib.dynenv_arrange_pad_backward(vp(G.data_ptr()), vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, ptrs, st),
                "pad_backward")
    for i in range(n):
        if c["has_emb"][i]:
            _same_bits(outs[i], c["grads"][i], "fused, type %d" % i)
    outs = [torch.full((r, F), float("nan"), device="cuda") for r in rows]
    for i in range(n):
        _capi.check(lib.dynenv_arrange_scatter_backward(vp(G.data_ptr()), _capi.ptr(slots[i]) if rows[i] else None, rows[i], F,
                                                        _capi.ptr(outs[i]) if rows[i] else None, st), "scatter_backward")
        if c["has_emb"][i]:
            _same_bits(outs[i], c["grads"][i], "row gather, type %d" % i)


@pytest.mark.parametrize("upstream", ["plain", "misaligned"])
@pytest.mark.parametrize("name", GR.CASES)
def test_autograd_reproduces_the_reference_gradients(name, upstream):
    """the recorded embeddings through rearrange_outputs and backward of the recorded G: aligned it takes the fused kernel (F = 12
    too), from a view 4 bytes off alignment the row gather"""
    import torch
    from dynenv_amd import GpuInOutArranger, _capi
    from dynenv_amd.arranger import ArrangePlan
    c = GR.golden_case(name)
    counts, base, slots = _golden_on_device(c)
    T, P, M, F, n = c["T"], c["P"], c["plan"]["max_count"], c["F"], c["nT"]
    arr = GpuInOutArranger([_capi.ArrType(0, 1, 0, _capi.ARR_COUNT_CONST, 0, 0, 0, 0)] * n, c["E"], c["A"], T, 1)   # (the plan is given)
    obj = counts.sum(0).to(torch.int32)
    mask = (torch.arange(M, device="cuda")[None, None, :] >= obj[:, :, None]).to(torch.uint8)
    embs = [torch.from_numpy(e).cuda().requires_grad_(True) if e is not None else None for e in c["embs"]]
    padded, _ = arr.rearrange_outputs(embs, ArrangePlan(counts, M, obj, slots, mask, base))
    _same_bits(padded, c["padded"], "padded")
    padded.backward(_upstream(c["G"], upstream))
    assert arr.last_backward == ("fused" if upstream == "plain" else "rows")
    for i in range(n):
        if c["has_emb"][i]:
            _same_bits(embs[i].grad, c["grads"][i], "type %d" % i)


# ---- autograd at the shapes where the kernels can go wrong ----
@pytest.mark.parametrize("F", [4, 8, 128])
def test_backward_count_residues(F, monkeypatch):
    """the fused backward copies 4 slots per step, then the rest: per player and type every count 0-7 and 16+.  F = 4: one wave covers
    64 players; F = 128: a wave sits inside one player."""
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", "0")
    rng = np.random.default_rng(F)
    specs = [(3, 19, ROW, 0, 19), (2, 6, ENV, 0, 6), (1, 2, CONST, 1, 1), (4, 5, ROW, -1, 5)]
    obs, types, ce = R.make_dense(rng, 64, 2, 4, specs)
    pl, route = check_backward(obs, types, ce, F=F, seed=F)
    assert route == "fused"
    seen = set(np.unique(pl["counts"][0]).tolist())
    assert set(range(8)) <= seen and any(c >= 16 for c in seen)


@pytest.mark.parametrize("dense_min", ["0", "2"])   # forward in one pass / zero fill + scatter: the backward is the same
@pytest.mark.parametrize("E, T, A", [(1, 1, 1), (51, 1, 5), (64, 2, 2), (257, 1, 1)])
def test_backward_sizes(E, T, A, dense_min, monkeypatch):
    """P no multiple of 64, T > 1 (blockIdx.y), a last block that is partly live"""
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", dense_min)
    rng = np.random.default_rng(E * 31 + T * 7 + A)
    specs = [(3, 4, ROW, -1, 6), (2, 3, ENV, -1, 4), (5, 2, CONST, 1, 2)]
    obs, types, ce = R.make_dense(rng, E, T, A, specs, lead=1, trail=1)
    pl, route = check_backward(obs, types, ce, F=8, seed=E + T)
    assert pl["max_count"] > 0 and route == "fused"


@pytest.mark.parametrize("F, upstream, route", [(5, "plain", "rows"), (13, "plain", "rows"), (8, "permuted", "fused"),
                                                (8, "misaligned", "rows"), (13, "permuted", "rows")])
def test_backward_fallbacks(F, upstream, route, monkeypatch):
    """odd widths and a gradient off alignment take the row gather; a permuted view is made contiguous first (and is aligned then)"""
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", "0")
    rng = np.random.default_rng(F)
    specs = [(3, 17, ROW, -2, 19), (2, 3, ENV, 0, 3), (5, 1, CONST, 1, 1)]
    obs, types, ce = R.make_dense(rng, 70, 2, 3, specs, lead=2)
    _, took = check_backward(obs, types, ce, F=F, seed=F, upstream=upstream)
    assert took == route


@pytest.mark.parametrize("F, route", [(8, "fused"), (5, "rows")])
def test_a_type_that_needs_no_gradient_gets_none(F, route):
    """outs[1] without requires_grad: its .grad stays None, its NULL destination is accepted, the other types are right"""
    rng = np.random.default_rng(12)
    specs = [(3, 4, ROW, 0, 4), (2, 5, ROW, 1, 5), (2, 3, ENV, 0, 3)]
    obs, types, ce = R.make_dense(rng, 33, 2, 2, specs)
    _, took = check_backward(obs, types, ce, F=F, frozen=(1,))
    assert took == route


@pytest.mark.parametrize("dense_min", ["0", "2"])
def test_backward_with_every_count_clamped_and_a_cap_0_type_as_none(dense_min, monkeypatch):
    """the all_clamped spec of test_arranger_gather_span: counts above cap in all three modes, and a cap-0 type with a positive count,
    which has no objects and is passed as None"""
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", dense_min)
    rng = np.random.default_rng(5)
    specs = [(2, 3, ROW, 4, 9), (3, 2, ENV, 3, 6), (1, 4, CONST, 7, 7), (2, 0, CONST, 5, 5)]
    obs, types, ce = R.make_dense(rng, 300, 2, 3, specs)
    pl, route = check_backward(obs, types, ce, F=8)
    cap_sum = sum(ty.cap for ty in types)
    assert pl["max_count"] == cap_sum and (pl["obj_counts"] == cap_sum).all() and pl["total"][3] == 0 and route == "fused"


def test_c_abi_backward_writes_every_row_and_nothing_else():
    """both entry points with every grad_emb a slice of a larger buffer: sentinel guard bands around it, NaN inside it.  Afterwards the
    bands are intact, no NaN is left and the rows equal unpad (4 types, P = 300 players: a partly live last block, T = 3)"""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(9)
    specs = [(3, 5, ROW, -1, 6), (2, 3, ENV, 0, 4), (1, 2, CONST, 2, 2), (4, 6, ROW, -2, 8)]
    E, T, A, F = 300, 3, 1, 8
    obs_np, types, ce_np = R.make_dense(rng, E, T, A, specs, lead=1)
    pl = R.plan(obs_np, types, ce_np)
    _, r_sl, _ = R.gather(obs_np, types, pl)
    P, M, n = E * A, pl["max_count"], len(types)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    counts, base, slots = i32(pl["counts"]), i32(pl["base"]), [i32(s) for s in r_sl]
    G_np = rng.standard_normal((T, M, P, F)).astype(np.float32)
    G = torch.from_numpy(G_np).cuda()
    want = GR.unpad(G_np, r_sl)
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    GUARD, SENT = 64, 777.25   # guard floats on either side (keeps 16-byte alignment)

    def guarded(rows):
        buf = torch.full((rows * F + 2 * GUARD,), SENT, dtype=torch.float32, device="cuda")
        inner = buf[GUARD:GUARD + rows * F].view(rows, F)
        inner.fill_(float("nan"))
        return buf, inner

    def verify(bufs, what):
        for i, (buf, inner) in enumerate(bufs):
            b = buf.cpu()
            assert bool((b[:GUARD] == SENT).all()) and bool((b[-GUARD:] == SENT).all()), "%s, type %d: guard band overwritten" % (what, i)
            assert not bool(torch.isnan(inner).any()), "%s, type %d: a row was left out" % (what, i)
            _same_bits(inner, want[i], "%s, type %d" % (what, i))

    assert all(len(s) for s in r_sl)
    bufs = [guarded(len(s)) for s in r_sl]
    ptrs = (vp * n)(*[inner.data_ptr() for _, inner in bufs])
    _capi.check(lib.dynenv_arrange_pad_backward(vp(G.data_ptr()), vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, ptrs, st),
                "pad_backward")
    verify(bufs, "fused")
    # a NULL destination: that type is stepped over, the others are as before
    bufs = [guarded(len(s)) for s in r_sl]
    ptrs = (vp * n)(*[None if i == 1 else inner.data_ptr() for i, (_, inner) in enumerate(bufs)])
    _capi.check(lib.dynenv_arrange_pad_backward(vp(G.data_ptr()), vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, ptrs, st),
                "pad_backward")
    assert bool(torch.isnan(bufs[1][1]).all()), "a type without a destination was written"
    bufs[1][1].copy_(torch.from_numpy(want[1]))
    verify(bufs, "fused, type 1 skipped")
    bufs = [guarded(len(s)) for s in r_sl]
    for i, (_, inner) in enumerate(bufs):
        _capi.check(lib.dynenv_arrange_scatter_backward(vp(G.data_ptr()), vp(slots[i].data_ptr()), len(r_sl[i]), F, vp(inner.data_ptr()), st),
                    "scatter_backward")
    verify(bufs, "row gather")
    # nothing to do is no error
    assert lib.dynenv_arrange_pad_backward(vp(G.data_ptr()), vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, 0, F, ptrs, st) == 0
    assert lib.dynenv_arrange_scatter_backward(None, None, 0, F, None, st) == 0


def test_a_plan_outlives_later_calls():
    """one arranger, two rearrange_inputs + rearrange_outputs calls on different observations with different maxCount; backward through
    the FIRST result after the second call gives the first call's gradients, and rearrange_outputs(outs, countArr_first) still builds
    the first padded tensor"""
    import torch
    from dynenv_amd import GpuInOutArranger
    E, T, A, F = 40, 2, 3, 8
    made = []
    for seed, hi in ((1, 3), (2, 6)):
        rng = np.random.default_rng(seed)
        specs = [(3, 6, ROW, 0, hi), (2, 6, ROW, 0, hi), (2, 2, ENV, 0, 2)]
        made.append(R.make_dense(rng, E, T, A, specs))
    D = made[0][0].shape[3]
    arr = GpuInOutArranger(_arr_types(made[0][1]), E, A, T, D)
    runs = []
    for obs_np, types, ce_np in made:
        pl = R.plan(obs_np, types, ce_np)
        _, r_sl, _ = R.gather(obs_np, types, pl)
        inputs, countArr = arr.rearrange_inputs(torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda())
        rng = np.random.default_rng(7)
        host = [rng.standard_normal((len(s), F)).astype(np.float32) for s in r_sl]
        embs = [torch.from_numpy(h).cuda().requires_grad_(True) for h in host]
        padded, _ = arr.rearrange_outputs(embs, countArr)
        runs.append(dict(pl=pl, sl=r_sl, host=host, embs=embs, padded=padded, countArr=countArr))
    a, b = runs
    assert a["pl"]["max_count"] != b["pl"]["max_count"] and not np.array_equal(a["pl"]["counts"], b["pl"]["counts"])
    assert np.array_equal(arr._base.cpu().numpy(), b["pl"]["base"]), "arr._base is the latest plan"
    assert np.array_equal(a["countArr"].base.cpu().numpy(), a["pl"]["base"]) and np.array_equal(a["countArr"][0].cpu().numpy(), a["pl"]["counts"])
    G_np = np.random.default_rng(8).standard_normal(tuple(a["padded"].shape)).astype(np.float32)
    a["padded"].backward(torch.from_numpy(G_np).cuda())
    for i, (e, w) in enumerate(zip(a["embs"], GR.unpad(G_np, a["sl"]))):
        _same_bits(e.grad, w, "first call, type %d" % i)
    want = R.pad(a["host"], a["sl"], T, a["pl"]["max_count"], E * A, F)
    again, _ = arr.rearrange_outputs([e.detach() for e in a["embs"]], a["countArr"])
    _same_bits(again, want, "the first padded tensor, rebuilt after the second call")
    plain, _ = arr.rearrange_outputs([e.detach() for e in a["embs"]], tuple(a["countArr"]))   # (a plain 5-tuple: bases from its own counts)
    _same_bits(plain, want, "the first padded tensor from a plain tuple")


@pytest.mark.parametrize("dense_min", ["0", "2"])
def test_without_a_gradient_wanted_nothing_changes(dense_min, monkeypatch):
    """inputs without requires_grad, and inputs with it under torch.no_grad(): no grad_fn, the padded tensor as ever"""
    import torch
    from dynenv_amd import GpuInOutArranger
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", dense_min)
    rng = np.random.default_rng(21)
    specs = [(3, 4, ROW, -1, 6), (2, 3, ENV, -1, 4), (5, 2, CONST, 1, 2)]
    E, T, A, F = 51, 2, 3, 8
    obs_np, types, ce_np = R.make_dense(rng, E, T, A, specs)
    pl = R.plan(obs_np, types, ce_np)
    _, r_sl, _ = R.gather(obs_np, types, pl)
    arr = GpuInOutArranger(_arr_types(types), E, A, T, obs_np.shape[3])
    _, countArr = arr.rearrange_inputs(torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda())
    host = [rng.standard_normal((len(s), F)).astype(np.float32) for s in r_sl]
    want = R.pad(host, r_sl, T, pl["max_count"], E * A, F)
    padded, _ = arr.rearrange_outputs([torch.from_numpy(h).cuda() for h in host], countArr)
    assert padded.grad_fn is None and not padded.requires_grad
    _same_bits(padded, want, "padded, no requires_grad")
    with torch.no_grad():
        padded, _ = arr.rearrange_outputs([torch.from_numpy(h).cuda().requires_grad_(True) for h in host], countArr)
    assert padded.grad_fn is None and not padded.requires_grad
    _same_bits(padded, want, "padded, under no_grad")


def test_input_layer_trains_its_blocks():
    """GpuInputLayer with nn.Linear(feat_i, 8, bias=False) blocks, loss = (padded * W).sum(): every block's weight.grad equals the one
    obtained by building `padded` with plain torch (zeros().index_copy by slot) from the same blocks - identical grad_emb through the
    same torch ops, so rtol = atol = 0.  The last type has no objects: its block never runs and its weight keeps grad None."""
    import torch
    from dynenv_amd import GpuInputLayer
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    specs = [(3, 4, ROW, 0, 4), (2, 3, ENV, 0, 3), (5, 2, CONST, 1, 2), (4, 3, CONST, 0, 0)]
    E, T, A, F = 24, 2, 3, 8
    obs_np, types, ce_np = R.make_dense(rng, E, T, A, specs)
    obs, ce = torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda()
    blocks = torch.nn.ModuleList([torch.nn.Linear(ty.feat, F, bias=False) for ty in types]).cuda()
    layer = GpuInputLayer(blocks, _arr_types(types), E, A, T, obs_np.shape[3])
    assert layer.blocks is blocks and len(list(layer.parameters())) == 4
    padded, masks = layer(obs, ce)
    M, P = padded.shape[1], E * A
    assert padded.grad_fn is not None and tuple(padded.shape) == (T, M, P, F) and len(masks) == T and masks[0].dtype == torch.bool
    W = torch.randn(padded.shape, device="cuda")
    (padded * W).sum().backward()
    got = [b.weight.grad.clone() if b.weight.grad is not None else None for b in blocks]
    assert all(g is not None for g in got[:3]) and got[3] is None, "the empty type's block gets no gradient"
    # the same network, `padded` assembled by torch
    for b in blocks:
        b.weight.grad = None
    inputs, countArr = layer.arranger.rearrange_inputs(obs, ce)
    assert [int(i.shape[0]) > 0 for i in inputs] == [True, True, True, False]
    flat = torch.zeros((T * M * P, F), device="cuda")
    for b, x, s in zip(blocks, inputs, countArr[3]):
        if x.shape[0]:
            flat = flat.index_copy(0, s.long(), b(x))
    ref = flat.view(T, M, P, F)
    torch.testing.assert_close(padded.detach(), ref.detach(), rtol=0, atol=0)
    (ref * W).sum().backward()
    for i in range(3):
        torch.testing.assert_close(got[i], blocks[i].weight.grad, rtol=0, atol=0)
    assert blocks[3].weight.grad is None


def _real_obs(cfg, E):
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    part = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=5)
    if cfg == "robocup_partial":
        env, hi = BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=11, **part), [5, 3, 3, 7]
    else:
        env, hi = BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=11, **part), [3, 3]
    env.reset_flat()
    rng = np.random.default_rng(2)
    for _ in range(4):
        act = np.stack([rng.integers(0, k, (E, env.n_agents)) for k in hi], -1).astype(np.int32)
        obs, _, _ = env.step_flat(torch.tensor(act, device="cuda"), auto_reset=False)
    return env, obs.contiguous()


@pytest.mark.parametrize("cfg", ["driving_partial", "robocup_partial"])
def test_backward_on_real_ragged_observations(cfg):
    """Driving Partial and RoboCup Partial with Realistic noise, 64 environments after four steps, both groups"""
    from dynenv_amd import DynEnvType, groups_for
    E = 64
    env, obs = _real_obs(cfg, E)
    obs_np = obs.cpu().numpy()
    ce = env.counts().cpu().numpy() if env.env_type == DynEnvType.DRIVE else None
    for gname, grp in groups_for(env).items():
        types = [R.Ty(*[getattr(t, f) for f in R.Ty._fields]) for t in grp]
        pl, route = check_backward(obs_np, types, ce, F=8, arr_types=grp)
        assert route == "fused"
        assert pl["max_count"] > 0 and len(np.unique(pl["counts"])) > 1, (cfg, gname)
    env.close()
