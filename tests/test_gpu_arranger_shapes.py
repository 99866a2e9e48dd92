"""The GPU arranger (arranger_kernels.hip through dynenv_amd.GpuInOutArranger and the C ABI) bit for bit against the vectorised
reference tests/arranger_ref.py at the shapes production runs: the multi-chunk block scan (more than 256 blocks of 256 players),
the fused pad kernel over tens of thousands of players, every count residue of its 4-slot unroll, embedding widths up to 256,
the scatter fallback (odd widths, misaligned embeddings), clamped counts, real observations of 4096 environments, and guard
bands around every output buffer."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROW, ENV, CONST = R.COUNT_ROW, R.COUNT_ENV, R.COUNT_CONST


def _arr_types(types):
    from dynenv_amd import _capi
    return [_capi.ArrType(*(ty.astuple() + (0,))) for ty in types]


def _embs(rng, slots, F, misaligned=False):
    """host embeddings [N_i, F] (None for a type without objects) and their device copies (misaligned: a view at +1 float)"""
    import torch
    host, dev = [], []
    for s in slots:
        if not len(s):
            host.append(None)
            dev.append(None)
            continue
        h = rng.standard_normal((len(s), F)).astype(np.float32)
        if misaligned:
            buf = torch.empty((h.size + 1,), dtype=torch.float32, device="cuda")
            d = buf[1:].view(len(s), F)
            d.copy_(torch.from_numpy(h))
            assert d.is_contiguous() and d.data_ptr() % 16 == 4
        else:
            d = torch.from_numpy(h).cuda()
        host.append(h)
        dev.append(d)
    return host, dev


def check_arranger(obs_np, types, count_env_np, F, seed=0, misaligned=False, arr_types=None):
    """rearrange_inputs + rearrange_outputs on the device == arranger_ref on the host, every output bit for bit.  Returns the plan."""
    import torch
    from dynenv_amd import GpuInOutArranger
    E, T, A, D = obs_np.shape
    P = E * A
    arr = GpuInOutArranger(arr_types if arr_types is not None else _arr_types(types), E, A, T, D)
    obs = torch.from_numpy(obs_np).cuda()
    ce = torch.from_numpy(np.ascontiguousarray(count_env_np, np.int32)).cuda() if count_env_np is not None else None
    inputs, countArr = arr.rearrange_inputs(obs, ce)
    counts, max_count, obj_counts, slots, mask = countArr
    pl = R.plan(obs_np, types, count_env_np)
    r_in, r_sl, r_mask = R.gather(obs_np, types, pl)
    assert max_count == pl["max_count"]
    assert np.array_equal(counts.cpu().numpy(), pl["counts"])
    assert np.array_equal(obj_counts.cpu().numpy(), pl["obj_counts"])
    assert np.array_equal(arr._base.cpu().numpy(), pl["base"])
    for i in range(len(types)):
        assert np.array_equal(inputs[i].cpu().numpy(), r_in[i]), "inputs of type %d" % i
        assert np.array_equal(slots[i].cpu().numpy(), r_sl[i]), "slots of type %d" % i
    assert np.array_equal(mask.cpu().numpy(), r_mask)
    host, dev = _embs(np.random.default_rng(seed), r_sl, F, misaligned)
    padded, masks = arr.rearrange_outputs(dev, countArr)
    want = R.pad(host, r_sl, T, max_count, P, F)
    assert tuple(padded.shape) == want.shape
    got = padded.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("padded: %d of %d floats differ, first at %s" % (len(bad), got.size, bad[0].tolist()))
    assert np.array_equal(torch.stack(masks).cpu().numpy(), r_mask.astype(bool))
    return pl


# (E, T, A): T*E*A = 1, 255, 256, 257, 65536 (exactly 256 scan blocks), 65537 (the first carry of the block scan), 102400
# (RoboCup 4096 x 5 players x 5 time steps), 131075 (more than two scan chunks)
SIZES = [(1, 1, 1), (51, 1, 5), (64, 2, 2), (257, 1, 1), (4096, 4, 4), (65537, 1, 1), (4096, 5, 5), (5243, 5, 5)]


@pytest.mark.parametrize("dense_min", ["0", "2"])   # one pass over the padded tensor / zero fill + scatter
@pytest.mark.parametrize("E, T, A", SIZES)
def test_arranger_sizes(E, T, A, dense_min, monkeypatch):
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", dense_min)
    rng = np.random.default_rng(E * 31 + T * 7 + A)
    specs = [(3, 4, ROW, -1, 6), (2, 3, ENV, -1, 4), (5, 2, CONST, 1, 2)]
    obs, types, ce = R.make_dense(rng, E, T, A, specs, lead=1, trail=1)
    pl = check_arranger(obs, types, ce, F=8, seed=E + T)
    assert pl["max_count"] > 0


@pytest.mark.parametrize("dense_min", ["0", "2"])
@pytest.mark.parametrize("case", ["cap_sum_above_max", "all_clamped"])
def test_arranger_gather_span(case, dense_min, monkeypatch):
    """the gather kernel runs max(capSum, maxCount) threads per player: capSum well above maxCount, and every count clamped
    (counts above cap in all three modes, a cap-0 type with a positive count) so that maxCount == capSum"""
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", dense_min)
    rng = np.random.default_rng(5)
    if case == "cap_sum_above_max":
        specs = [(2, 9, ROW, -2, 2), (3, 7, ENV, 0, 2), (1, 5, CONST, 1, 1)]
    else:
        specs = [(2, 3, ROW, 4, 9), (3, 2, ENV, 3, 6), (1, 4, CONST, 7, 7), (2, 0, CONST, 5, 5)]
    obs, types, ce = R.make_dense(rng, 300, 2, 3, specs)
    pl = check_arranger(obs, types, ce, F=8)
    cap_sum = sum(ty.cap for ty in types)
    if case == "cap_sum_above_max":
        assert pl["max_count"] < cap_sum
    else:
        assert pl["max_count"] == cap_sum and (pl["obj_counts"] == cap_sum).all()


@pytest.mark.parametrize("F", [4, 8, 128, 256])
def test_arranger_pad_kernel_count_residues(F, monkeypatch):
    """the fused pad kernel copies 4 slots per step, then the rest: per player and type every count 0-7 and 16+"""
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", "0")
    rng = np.random.default_rng(F)
    specs = [(3, 19, ROW, 0, 19), (2, 6, ENV, 0, 6), (1, 2, CONST, 1, 1), (4, 5, ROW, -1, 5)]
    obs, types, ce = R.make_dense(rng, 64, 2, 4, specs)
    pl = check_arranger(obs, types, ce, F=F, seed=F)
    seen = set(np.unique(pl["counts"][0]).tolist())
    assert set(range(8)) <= seen and any(c >= 16 for c in seen)


@pytest.mark.parametrize("F, misaligned", [(5, False), (13, False), (8, True)])
def test_arranger_scatter_path(F, misaligned, monkeypatch):
    """zero fill + one scatter per type: an odd width, and a width that is a multiple of 4 on embeddings 4 bytes off alignment"""
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", "0")   # (the pad kernel would be taken if it could)
    rng = np.random.default_rng(F)
    specs = [(3, 17, ROW, -2, 19), (2, 3, ENV, 0, 3), (5, 1, CONST, 1, 1)]
    obs, types, ce = R.make_dense(rng, 700, 2, 3, specs, lead=2)
    check_arranger(obs, types, ce, F=F, seed=F, misaligned=misaligned)


def test_arranger_none_for_a_type_with_objects_is_refused():
    """the reference packs the later types to the left when a type's output is None (models.py:259-266), the kernels would
    leave a gap: refused.  None stays legal for a type without objects (here: cap 0)."""
    import torch
    from dynenv_amd import GpuInOutArranger
    rng = np.random.default_rng(3)
    specs = [(2, 3, ROW, 1, 3), (2, 0, CONST, 0, 0), (2, 2, ENV, 1, 2)]
    obs_np, types, ce_np = R.make_dense(rng, 8, 2, 3, specs)
    E, T, A, D = obs_np.shape
    arr = GpuInOutArranger(_arr_types(types), E, A, T, D)
    inputs, countArr = arr.rearrange_inputs(torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda())
    outs = [torch.ones((int(i.shape[0]), 4), device="cuda") for i in inputs]
    assert outs[0].shape[0] > 0 and outs[1].shape[0] == 0
    with pytest.raises(ValueError):
        arr.rearrange_outputs([None, outs[1], outs[2]], countArr)
    with pytest.raises(ValueError):
        arr.rearrange_outputs(outs[:2], countArr)
    check_arranger(obs_np, types, ce_np, F=4)   # (the cap-0 type gets None there)


def _real_obs(cfg, E):
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    part = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=5)
    if cfg == "robocup_full":
        env, hi = BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=11), [5, 3, 3, 7]
    elif cfg == "robocup_partial":
        env, hi = BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=11, **part), [5, 3, 3, 7]
    else:
        env, hi = BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=11, **part), [3, 3]
    env.reset_flat()
    rng = np.random.default_rng(2)
    for _ in range(4):
        act = np.stack([rng.integers(0, k, (E, env.n_agents)) for k in hi], -1).astype(np.int32)
        obs, _, _ = env.step_flat(torch.tensor(act, device="cuda"), auto_reset=False)
    return env, obs.contiguous()


@pytest.mark.parametrize("dense_min", ["0", "2"])
@pytest.mark.parametrize("cfg", ["robocup_full", "robocup_partial", "driving_partial"])
def test_arranger_on_real_observations_at_production_size(cfg, dense_min, monkeypatch):
    """4096 environments (RoboCup 5 players, Driving 10 agents), both groups, the reference on the same observation tensor"""
    from dynenv_amd import DynEnvType, groups_for
    monkeypatch.setenv("DYNENV_ARR_DENSE_MIN", dense_min)
    E = 4096
    env, obs = _real_obs(cfg, E)
    obs_np = obs.cpu().numpy()
    ce = env.counts().cpu().numpy() if env.env_type == DynEnvType.DRIVE else None
    for gname, grp in groups_for(env).items():
        types = [R.Ty(*[getattr(t, f) for f in R.Ty._fields]) for t in grp]
        pl = check_arranger(obs_np, types, ce, F=8, arr_types=grp)
        assert pl["max_count"] > 0 and int(pl["total"].sum()) > E, (cfg, gname)
    env.close()


def test_arranger_c_abi_writes_nothing_outside_its_outputs():
    """dynenv_arrange_plan / _gather / _pad / _scatter with every output a slice of a larger buffer filled with a sentinel:
    the outputs equal the reference and the sentinels around them survive (4 types, more than 256 scan blocks)"""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(9)
    specs = [(3, 5, ROW, -1, 6), (2, 3, ENV, 0, 4), (1, 2, CONST, 2, 2), (4, 6, ROW, -2, 8)]
    E, T, A = 22000, 3, 1
    obs_np, types, ce_np = R.make_dense(rng, E, T, A, specs, lead=1)
    D, P, n = obs_np.shape[3], E * A, len(types)
    TP = T * P
    pl = R.plan(obs_np, types, ce_np)
    r_in, r_sl, r_mask = R.gather(obs_np, types, pl)
    M = pl["max_count"]
    G = 64   # guard elements on either side (keeps 16-byte alignment)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)

    def guarded(count, dtype, fill):
        buf = torch.full((count + 2 * G,), fill, dtype=dtype, device="cuda")
        return buf, buf[G:G + count]

    def intact(buf, fill, what):
        b = buf.cpu()
        assert bool((b[:G] == fill).all()) and bool((b[-G:] == fill).all()), what + ": guard band overwritten"

    I32S, F32S, U8S = -0x21524111, 777.25, 0xAB
    obs, ce = dev(obs_np), dev(ce_np)
    aty = (_capi.ArrType * n)(*_arr_types(types))
    cb, counts = guarded(n * TP, torch.int32, I32S)
    ob, objc = guarded(TP, torch.int32, I32S)
    bb, base = guarded(n * TP, torch.int32, I32S)
    nscr = int(lib.dynenv_arrange_scratch_ints(E, T, A, n))
    sb, scr = guarded(nscr + 2, torch.int32, I32S)
    plan = _capi.ArrPlan()
    _capi.check(lib.dynenv_arrange_plan(vp(obs.data_ptr()), E, T, A, D, aty, n, vp(ce.data_ptr()), vp(counts.data_ptr()),
                                        vp(objc.data_ptr()), vp(base.data_ptr()), vp(scr.data_ptr()), C.byref(plan), st), "plan")
    assert plan.max_count == M and [plan.total[i] for i in range(n)] == pl["total"].tolist()
    assert np.array_equal(counts.cpu().numpy().reshape(pl["counts"].shape), pl["counts"])
    assert np.array_equal(objc.cpu().numpy().reshape(T, P), pl["obj_counts"])
    assert np.array_equal(base.cpu().numpy().reshape(pl["base"].shape), pl["base"])
    for b, what in ((cb, "counts"), (ob, "obj_counts"), (bb, "base"), (sb, "scratch")):
        intact(b, I32S, what)

    ins = [guarded(int(pl["total"][i]) * types[i].feat, torch.float32, F32S) for i in range(n)]
    sls = [guarded(int(pl["total"][i]), torch.int32, I32S) for i in range(n)]
    mb, mask = guarded(TP * M, torch.uint8, U8S)
    in_ptrs = (vp * n)(*[v.data_ptr() for _, v in ins])
    sl_ptrs = (vp * n)(*[v.data_ptr() for _, v in sls])
    _capi.check(lib.dynenv_arrange_gather(vp(obs.data_ptr()), E, T, A, D, aty, n, vp(counts.data_ptr()), vp(base.data_ptr()), M,
                                          in_ptrs, sl_ptrs, vp(mask.data_ptr()), st), "gather")
    for i in range(n):
        assert np.array_equal(ins[i][1].cpu().numpy().reshape(-1, types[i].feat), r_in[i])
        assert np.array_equal(sls[i][1].cpu().numpy(), r_sl[i])
        intact(ins[i][0], F32S, "inputs %d" % i)
        intact(sls[i][0], I32S, "slots %d" % i)
    assert np.array_equal(mask.cpu().numpy().reshape(T, P, M), r_mask)
    intact(mb, U8S, "mask")

    F = 8
    host = [rng.standard_normal((len(s), F)).astype(np.float32) for s in r_sl]
    embs = [dev(h) for h in host]
    want = R.pad(host, r_sl, T, M, P, F)
    pb, padded = guarded(T * M * P * F, torch.float32, F32S)
    e_ptrs = (vp * n)(*[e.data_ptr() for e in embs])
    _capi.check(lib.dynenv_arrange_pad(e_ptrs, vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, vp(padded.data_ptr()), st), "pad")
    assert np.array_equal(padded.cpu().numpy().reshape(want.shape), want)
    intact(pb, F32S, "padded (pad kernel)")

    pb, padded = guarded(T * M * P * F, torch.float32, F32S)
    padded.zero_()
    for i in range(n):
        _capi.check(lib.dynenv_arrange_scatter(vp(embs[i].data_ptr()), vp(sls[i][1].data_ptr()), len(r_sl[i]), F, vp(padded.data_ptr()), st),
                    "scatter")
    assert np.array_equal(padded.cpu().numpy().reshape(want.shape), want)
    intact(pb, F32S, "padded (scatter)")


@pytest.mark.parametrize("padded_kind", ["f32", "bf16"])
@pytest.mark.parametrize("fixed", [False, True], ids=["default", "fixed"])
def test_counts_the_plan_did_not_make(fixed, padded_kind):
    """The C ABI takes counts_dev from the caller: a negative count, and one beyond rows[i] and beyond the slots left, through the
    pad and pad_backward calls of both modes (arranger_cols_kernels.hip), float32 embeddings, a float32 and a bf16 padded tensor.
    Every kernel keeps c' = max(0, min(c, rows[i] if fixed, slots left)), so with counts = [[-2, 2], [2, 5]] (type x player), M = 3:
        player 0: type 0 keeps 0, type 1 keeps 2      -> slots: type 1's first row, its second row, zeros
        player 1: type 0 keeps 2, type 1 keeps 1 of 5 -> slots: type 0's first row, its second row, type 1's first row
    All values are small integers, exact in bf16.  Every output lies between guard bands that even an unclamped walk stays inside."""
    import torch
    from dynenv_amd import _capi
    from test_gpu_arranger_dtype import Guarded, SENTINEL
    lib = _capi.load()
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    n, T, P, M, F = 2, 1, 2, 3, 8
    counts = torch.tensor([[-2, 2], [2, 5]], dtype=torch.int32).cuda()
    if fixed:
        rows = [2, 3]
        nrows = [T * P * r for r in rows]
        start = [[0, 2], [0, 3]]             # tp * rows[i], type x player
        third = (C.c_int32 * n)(*rows)
        pad_fn, bwd_fn = lib.dynenv_arrange_fixed_pad_as, lib.dynenv_arrange_fixed_pad_backward_as
    else:
        nrows = [2, 5]
        start = [[0, 0], [0, 2]]
        base = torch.tensor(start, dtype=torch.int32).cuda()
        third = vp(base.data_ptr())
        pad_fn, bwd_fn = lib.dynenv_arrange_pad_as, lib.dynenv_arrange_pad_backward_as
    kept = [[0, 2], [2, 1]]                  # c', type x player
    owner = {(0, 0): (1, 0), (1, 0): (1, 1), (0, 1): (0, 0), (1, 1): (0, 1), (2, 1): (1, 0)}   # (slot, player) -> (type, the player's k-th row)
    pc, words = (0, 2) if padded_kind == "f32" else (1, 1)
    to_padded = lambda a: a.view(np.uint32) if words == 2 else (a.view(np.uint32) >> 16).astype(np.uint16)   # exact: small integers

    host = [(1 + 100 * i + np.arange(r * F)).reshape(r, F).astype(np.float32) for i, r in enumerate(nrows)]
    assert host[1].max() < 256
    embs = [torch.from_numpy(h).cuda() for h in host]
    want = np.zeros((T, M, P, F), np.float32)
    for (j, p), (i, k) in owner.items():
        want[0, j, p] = host[i][start[i][p] + k]
    out = Guarded(T * M * P * F, 2 * words)
    e_ptrs = (vp * n)(*[e.data_ptr() for e in embs])
    _capi.check(pad_fn(e_ptrs, 0, vp(counts.data_ptr()), third, n, T, P, M, F, vp(out.ptr()), pc, st), "pad")
    got = out.check("padded", True)          # the bands are intact and every element was written
    assert np.array_equal(got.view(np.uint32 if words == 2 else np.uint16).reshape(T, M, P, F), to_padded(want)), "padded, bit for bit"

    up = (1 + np.arange(T * M * P * F)).reshape(T, M, P, F).astype(np.float32)
    up[0, 2, 0] = np.nan                     # player 0's padding slot
    if words == 2:
        upd = torch.from_numpy(up).cuda()
    else:
        upd = torch.from_numpy((up.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).cuda()
    gs = [Guarded(r * F, 4) for r in nrows]
    g_ptrs = (vp * n)(*[g.ptr() for g in gs])
    _capi.check(bwd_fn(vp(upd.data_ptr()), pc, vp(counts.data_ptr()), third, n, T, P, M, F, g_ptrs, 0, st), "pad_backward")
    unwritten = np.uint32(SENTINEL << 16 | SENTINEL)
    for i, g in enumerate(gs):
        b = g.buf.cpu().numpy().view(np.uint16)
        band = g.G * g.words
        assert (b[:band] == SENTINEL).all() and (b[b.size - band:] == SENTINEL).all(), "grad_emb %d: a guard band was written" % i
        pay = b[band:b.size - band].view(np.uint32).reshape(nrows[i], F)
        expect = np.full((nrows[i], F), 0 if fixed else unwritten, np.uint32)   # fixed mode: +0.0 behind the kept rows; default: not touched
        for (j, p), (ti, k) in owner.items():
            if ti == i:
                expect[start[i][p] + k] = up[0, j, p].view(np.uint32)
        assert np.array_equal(pay, expect), "grad_emb %d: the kept rows are their slots, the rest %s" % (i, "+0.0" if fixed else "untouched")
        written = pay[pay != unwritten].view(np.float32)
        assert not np.isnan(written).any(), "grad_emb %d: the padding slot was read" % i
