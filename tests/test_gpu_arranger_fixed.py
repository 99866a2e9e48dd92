"""The fixed-shape arranger on the device (arranger_fixed_kernels.hip and arranger_cols_kernels.hip through dynenv_arrange_fixed_* and
GpuInOutArranger / GpuInputLayer (fixed=...)), bit for bit against the numpy statement of its contract (tests/arranger_fixed_ref.py) and, where nothing is dropped,
against the default mode on the same device; guard bands around every output of the C ABI; autograd; and a whole rollout step -
environment step, counts, input layer - captured into one graph and replayed.  -m gpu."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_ref as R  # noqa: E402
import arranger_fixed_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu
ROW, ENV, CONST = R.COUNT_ROW, R.COUNT_ENV, R.COUNT_CONST
# caps 5, 7, 1 and 0; the three count modes; raw counts from below 0 to above cap (CONST: 2 > 1, 3 > 0)
SPECS = [(3, 5, ROW, -2, 7), (2, 7, ENV, -1, 9), (4, 1, CONST, 2, 2), (2, 0, CONST, 3, 3)]


def _arr_types(types):
    from dynenv_amd import _capi
    return [_capi.ArrType(*(ty.astuple() + (0,))) for ty in types]


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _same(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint8 if got.itemsize == 1 else np.uint32) != want.view(np.uint8 if want.itemsize == 1 else np.uint32))
        raise AssertionError("%s: %d of %d elements differ, first at %s" % (what, len(bad), got.size, bad[0].tolist()))


def check_fixed(obs_np, types, ce_np, rows, M, F, seed=0, calls=1):
    """rearrange_inputs + rearrange_outputs + backward of a fixed-shape arranger == arranger_fixed_ref, every output bit for bit.  The
    embeddings are random in EVERY capacity row and the upstream gradient is NaN in every padding slot.  Returns the reference's plan."""
    import torch
    from dynenv_amd import GpuInOutArranger
    E, T, A, D = obs_np.shape
    P, n = E * A, len(types)
    arr = GpuInOutArranger(_arr_types(types), E, A, T, D, fixed=dict(max_count=M, rows=rows))
    obs, ce = torch.from_numpy(obs_np).cuda(), torch.from_numpy(np.ascontiguousarray(ce_np, np.int32)).cuda()
    pl = FR.plan(obs_np, types, rows, M, ce_np)
    r_in, r_mask = FR.gather(obs_np, types, rows, M, pl)
    for call in range(calls):
        inputs, countArr = arr.rearrange_inputs(obs, ce)
        _same(arr.dropped, (pl["dropped"] * (call + 1)).astype(np.int32), "dropped after %d calls" % (call + 1))
    counts, max_count, obj_counts, slots, mask = countArr
    assert max_count == M and type(max_count) is int and slots == [None] * n
    _same(counts, pl["counts"].astype(np.int32), "counts")
    _same(obj_counts, pl["obj_counts"].astype(np.int32), "obj_counts")
    _same(mask, r_mask, "mask")
    for i in range(n):
        assert tuple(inputs[i].shape) == (T * P * rows[i], types[i].feat)
        _same(inputs[i], r_in[i], "inputs of type %d" % i)
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal((T * P * rows[i], F)).astype(np.float32) if rows[i] else None for i in range(n)]
    if all(h is None for h in host):
        return pl
    dev = [torch.from_numpy(h).cuda().requires_grad_() if h is not None else None for h in host]
    padded, masks = arr.rearrange_outputs(dev, countArr)
    assert tuple(padded.shape) == (T, M, P, F) and padded.grad_fn is not None
    _same(padded, FR.pad(host, rows, M, pl, F), "padded")
    assert len(masks) == T and all(m.dtype == torch.bool for m in masks)
    if M:
        _same(torch.stack(masks), r_mask.astype(bool), "masks")
    up = rng.standard_normal((T, M, P, F)).astype(np.float32)
    up[r_mask.transpose(0, 2, 1).astype(bool)] = np.nan
    padded.backward(torch.from_numpy(up).cuda())
    want = FR.unpad(up, rows, pl)
    for i in range(n):
        if rows[i]:
            _same(dev[i].grad, want[i], "gradient of type %d" % i)
    with torch.no_grad():   # nothing to differentiate: the same launch, no grad_fn
        again, _ = arr.rearrange_outputs([d.detach() if d is not None else None for d in dev], countArr)
    assert again.grad_fn is None and _bits(again) == _bits(padded)
    return pl


def _batch_max(obs_np, types, ce_np):
    return R.plan(obs_np, types, ce_np)["max_count"]


@pytest.mark.parametrize("F", [4, 8, 12])
@pytest.mark.parametrize("E, T, A", [(1, 1, 1), (3, 2, 2), (43, 2, 3)])   # the last: T*P = 258 and, at F = 8, P*F/4 = 258: a block boundary
def test_contract(E, T, A, F):
    rng = np.random.default_rng(E * 100 + F)
    obs, types, ce = R.make_dense(rng, E, T, A, SPECS, lead=1, trail=1)
    rows = [ty.cap for ty in types]
    m0 = _batch_max(obs, types, ce)
    for M in sorted({m0, sum(rows), 4}):
        pl = check_fixed(obs, types, ce, rows, M, F, seed=M)
        assert bool(pl["dropped"].any()) == (M < m0)
    if E == 43:
        assert m0 > 4, "M = 4 drops"


@pytest.mark.parametrize("F", [4, 16])
def test_count_residues(F):
    """kept counts 0..9 and zero-fill lengths 0..9 in one batch: the copy loops and the zero-fill loop of the backward go four rows at
    a time, then one by one"""
    rng = np.random.default_rng(F)
    specs = [(3, 9, ROW, 0, 9), (2, 9, ENV, 0, 9), (1, 2, CONST, 1, 1)]
    obs, types, ce = R.make_dense(rng, 64, 2, 2, specs)
    pl = check_fixed(obs, types, ce, [9, 9, 2], 20, F, seed=1)
    for i in (0, 1):
        assert set(np.unique(pl["counts"][i]).tolist()) == set(range(10)), "kept 0..9, hence zero fill 9..0"


@pytest.mark.parametrize("what", ["M = batch max", "M = sum of rows", "M small", "M = 1", "M = 0", "rows below caps", "rows all zero",
                                  "dropped over two calls"])
def test_sizes(what):
    rng = np.random.default_rng(17)
    obs, types, ce = R.make_dense(rng, 43, 2, 3, SPECS, lead=2)
    caps = [ty.cap for ty in types]
    m0 = _batch_max(obs, types, ce)
    rows, M, calls = caps, m0, 1
    if what == "M = sum of rows":
        M = sum(caps)
    elif what == "M small":
        M = 5
    elif what == "M = 1":
        M = 1
    elif what == "M = 0":
        M = 0
    elif what == "rows below caps":
        rows = [2, 3, 1, 0]
    elif what == "rows all zero":
        rows = [0, 0, 0, 0]
    elif what == "dropped over two calls":
        rows, M, calls = [4, 5, 0, 0], 7, 2
    pl = check_fixed(obs, types, ce, rows, M, 8, seed=3, calls=calls)
    assert bool(pl["dropped"].any()) == (what not in ("M = batch max", "M = sum of rows"))
    if what == "M small":
        assert (pl["counts"][0] == 5).any() and (pl["counts"][1][pl["counts"][0] == 5] == 0).all(), "earlier types win"


def test_bad_widths_name_the_default_mode():
    import torch
    from dynenv_amd import GpuInOutArranger, _capi
    rng = np.random.default_rng(2)
    obs_np, types, ce_np = R.make_dense(rng, 4, 1, 2, SPECS)
    E, T, A, D = obs_np.shape
    arr = GpuInOutArranger(_arr_types(types), E, A, T, D, fixed=True)
    assert arr.rows == [5, 7, 1, 0] and arr.max_count == 13
    inputs, countArr = arr.rearrange_inputs(torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda())
    TP = T * E * A
    with pytest.raises(_capi.DynEnvError, match="default mode"):
        arr.rearrange_outputs([torch.ones((TP * r, 6), device="cuda") if r else None for r in arr.rows], countArr)
    buf = torch.ones((TP * 5 * 8 + 1,), device="cuda")
    off = [buf[1:].view(TP * 5, 8)] + [torch.ones((TP * r, 8), device="cuda") if r else None for r in arr.rows[1:]]
    assert off[0].is_contiguous() and off[0].data_ptr() % 16 == 4
    with pytest.raises(_capi.DynEnvError, match="default mode"):
        arr.rearrange_outputs(off, countArr)
    with pytest.raises(ValueError):   # a type with rows > 0 needs its embedding
        arr.rearrange_outputs([None] + off[1:], countArr)
    with pytest.raises(ValueError):
        GpuInOutArranger(_arr_types(types), E, A, T, D, fixed=dict(max_count=3, rows=[6, 7, 1, 0]))


def test_against_the_default_mode_on_the_device():
    """the same obs through both modes: rows = caps and M = maxCount + 2, embeddings drawn at capacity and their kept rows compacted for
    the default path.  Leading slots of padded and mask, the kept rows of the inputs and the gradient handed to each embedding: identical"""
    import torch
    from dynenv_amd import GpuInOutArranger
    rng = np.random.default_rng(23)
    obs_np, types, ce_np = R.make_dense(rng, 43, 2, 3, SPECS, lead=1)
    E, T, A, D = obs_np.shape
    P, n, F = E * A, len(types), 8
    obs, ce = torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda()
    dflt = GpuInOutArranger(_arr_types(types), E, A, T, D)
    d_in, d_plan = dflt.rearrange_inputs(obs, ce)
    M0 = d_plan[1]
    rows, M = [ty.cap for ty in types], M0 + 2
    fx = GpuInOutArranger(_arr_types(types), E, A, T, D, fixed=dict(max_count=M, rows=rows))
    f_in, f_plan = fx.rearrange_inputs(obs, ce)
    assert torch.equal(f_plan[0], d_plan[0]) and torch.equal(f_plan[2], d_plan[2]) and not bool(fx.dropped.any())
    kept = [(torch.arange(rows[i], device="cuda")[None, :] < f_plan[0][i].reshape(-1, 1)).reshape(-1) for i in range(n)]
    f_emb = [torch.randn((T * P * rows[i], F), device="cuda").requires_grad_() if rows[i] else None for i in range(n)]
    d_emb = [f_emb[i].detach()[kept[i]].clone().requires_grad_() if rows[i] else None for i in range(n)]
    for i in range(n):
        if rows[i]:
            assert _bits(f_in[i][kept[i]]) == _bits(d_in[i]), "inputs of type %d" % i
    f_pad, f_masks = fx.rearrange_outputs(f_emb, f_plan)
    d_pad, d_masks = dflt.rearrange_outputs(d_emb, d_plan)
    assert _bits(f_pad[:, :M0]) == _bits(d_pad) and not bool(f_pad[:, M0:].view(torch.int32).any())
    assert torch.equal(torch.stack(f_masks)[..., :M0], torch.stack(d_masks)) and bool(torch.stack(f_masks)[..., M0:].all())
    up = torch.randn((T, M, P, F), device="cuda")
    f_pad.backward(up)
    d_pad.backward(up[:, :M0].contiguous())
    assert dflt.last_backward == "fused"
    for i in range(n):
        if rows[i]:
            assert _bits(f_emb[i].grad[kept[i]]) == _bits(d_emb[i].grad), "gradient of type %d" % i
            assert not bool(f_emb[i].grad[~kept[i]].view(torch.int32).any())


def test_c_abi_writes_every_byte_of_its_outputs_and_nothing_else():
    """dynenv_arrange_fixed_gather / _pad / _pad_backward with every output a slice of a larger buffer: the guard bands survive; inputs,
    padded and each grad_emb are pre-filled with 0xA5 bytes, of which none remains; the upstream gradient is NaN in every padding slot
    and the gradients are finite; a NULL grad_emb entry is stepped over.  More than one block in every launch."""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(9)
    E, T, A, F = 150, 2, 2, 8
    obs_np, types, ce_np = R.make_dense(rng, E, T, A, SPECS, lead=1)
    D, P, n = obs_np.shape[3], E * A, len(types)
    TP = T * P
    rows, M = [4, 7, 1, 0], 9    # (rows[0] below its cap, M below the sum: drops)
    pl = FR.plan(obs_np, types, rows, M, ce_np)
    r_in, r_mask = FR.gather(obs_np, types, rows, M, pl)
    assert pl["dropped"][:2].all()
    G = 64   # guard elements on either side (keeps 16-byte alignment)
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    A5 = 0xA5

    def guarded(count, itemsize):
        """a byte buffer of guards | count elements | guards, everything 0xA5; returns (whole, the payload's bytes)"""
        buf = torch.full(((count + 2 * G) * itemsize,), A5, dtype=torch.uint8, device="cuda")
        return buf, buf[G * itemsize:(G + count) * itemsize]

    def intact(buf, itemsize, what):
        b = buf.cpu()
        assert bool((b[:G * itemsize] == A5).all()) and bool((b[-G * itemsize:] == A5).all()), what + ": guard band overwritten"

    def no_a5_words(view, what):
        assert not bool((view.view(torch.int32) == -0x5A5A5A5B).any()), what + ": a word was left unwritten"   # 0xA5A5A5A5

    obs, ce = torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda()
    aty = (_capi.ArrType * n)(*_arr_types(types))
    rows_c = (C.c_int32 * n)(*rows)
    cb, counts = guarded(n * TP, 4)
    ob, objc = guarded(TP, 4)
    mb, mask = guarded(TP * M, 1)
    db, dropped = guarded(n, 4)
    dropped.zero_()
    ins = [guarded(TP * rows[i] * types[i].feat, 4) for i in range(n)]
    in_ptrs = (vp * n)(*[v.data_ptr() if v.numel() else None for _, v in ins])
    _capi.check(lib.dynenv_arrange_fixed_gather(vp(obs.data_ptr()), E, T, A, D, aty, n, vp(ce.data_ptr()), rows_c, M, vp(counts.data_ptr()),
                                                vp(objc.data_ptr()), in_ptrs, vp(mask.data_ptr()), vp(dropped.data_ptr()), st), "gather")
    assert np.array_equal(counts.view(torch.int32).cpu().numpy().reshape(n, T, P), pl["counts"])
    assert np.array_equal(objc.view(torch.int32).cpu().numpy().reshape(T, P), pl["obj_counts"])
    assert np.array_equal(mask.cpu().numpy().reshape(T, P, M), r_mask)
    assert dropped.view(torch.int32).cpu().tolist() == pl["dropped"].tolist()
    for (b, v), what, size in ((cb, counts), "counts", 4), ((ob, objc), "obj_counts", 4), ((mb, mask), "mask", 1), ((db, dropped), "dropped", 4):
        intact(b, size, what)
    for i in range(n):
        if rows[i]:
            no_a5_words(ins[i][1], "inputs %d" % i)
            assert ins[i][1].view(torch.float32).cpu().numpy().tobytes() == r_in[i].tobytes(), "inputs %d" % i
        intact(ins[i][0], 4, "inputs %d" % i)

    host = [rng.standard_normal((TP * rows[i], F)).astype(np.float32) for i in range(n)]
    embs = [torch.from_numpy(h).cuda() for h in host]
    e_ptrs = (vp * n)(*[e.data_ptr() if e.numel() else None for e in embs])
    pb, padded = guarded(T * M * P * F, 4)
    _capi.check(lib.dynenv_arrange_fixed_pad(e_ptrs, vp(counts.data_ptr()), rows_c, n, T, P, M, F, vp(padded.data_ptr()), st), "pad")
    no_a5_words(padded, "padded")
    assert padded.view(torch.float32).cpu().numpy().tobytes() == FR.pad(host, rows, M, pl, F).tobytes()
    intact(pb, 4, "padded")
    # a NULL embedding writes zeros in its slots
    pb2, padded2 = guarded(T * M * P * F, 4)
    e_ptrs2 = (vp * n)(None, *[e.data_ptr() if e.numel() else None for e in embs[1:]])
    _capi.check(lib.dynenv_arrange_fixed_pad(e_ptrs2, vp(counts.data_ptr()), rows_c, n, T, P, M, F, vp(padded2.data_ptr()), st), "pad")
    assert padded2.view(torch.float32).cpu().numpy().tobytes() == FR.pad([None] + host[1:], rows, M, pl, F).tobytes()
    intact(pb2, 4, "padded (NULL embedding)")

    up = rng.standard_normal((T, M, P, F)).astype(np.float32)
    up[r_mask.transpose(0, 2, 1).astype(bool)] = np.nan
    want = FR.unpad(up, rows, pl)
    upd = torch.from_numpy(up).cuda()
    for null in (None, 1):
        gs = [guarded(TP * rows[i] * F, 4) for i in range(n)]
        g_ptrs = (vp * n)(*[v.data_ptr() if (v.numel() and i != null) else None for i, (_, v) in enumerate(gs)])
        _capi.check(lib.dynenv_arrange_fixed_pad_backward(vp(upd.data_ptr()), vp(counts.data_ptr()), rows_c, n, T, P, M, F, g_ptrs, st),
                    "pad_backward")
        for i in range(n):
            intact(gs[i][0], 4, "grad_emb %d" % i)
            if i == null:
                assert bool((gs[i][1] == A5).all()), "a NULL grad_emb entry's neighbour buffer was written"
            elif rows[i]:
                no_a5_words(gs[i][1], "grad_emb %d" % i)
                got = gs[i][1].view(torch.float32).cpu().numpy()
                assert np.isfinite(got).all() and got.tobytes() == want[i].tobytes(), "grad_emb %d" % i

    # M == 0: the gather writes zero counts, the full dropped totals and zeroed inputs; the pad calls launch nothing
    pl0 = FR.plan(obs_np, types, rows, 0, ce_np)
    dropped.zero_()
    for _, v in ins:
        v.fill_(A5)
    _capi.check(lib.dynenv_arrange_fixed_gather(vp(obs.data_ptr()), E, T, A, D, aty, n, vp(ce.data_ptr()), rows_c, 0, vp(counts.data_ptr()),
                                                vp(objc.data_ptr()), in_ptrs, None, vp(dropped.data_ptr()), st), "gather, M = 0")
    assert not bool(counts.view(torch.int32).any()) and not bool(objc.view(torch.int32).any())
    assert dropped.view(torch.int32).cpu().tolist() == pl0["dropped"].tolist() == pl0["c"].reshape(n, -1).sum(1).tolist()
    assert all(not bool(v.any()) for _, v in ins), "zeroed inputs"
    padded.fill_(A5)
    assert lib.dynenv_arrange_fixed_pad(e_ptrs, vp(counts.data_ptr()), rows_c, n, T, P, 0, F, vp(padded.data_ptr()), st) == 0
    assert lib.dynenv_arrange_fixed_pad_backward(vp(upd.data_ptr()), vp(counts.data_ptr()), rows_c, n, T, P, 0, F, g_ptrs, st) == 0
    assert bool((padded == A5).all())
    for b, what, size in ((cb, "counts", 4), (ob, "obj_counts", 4), (mb, "mask", 1), (db, "dropped", 4)):
        intact(b, size, what + " (M = 0)")


def test_input_layer_trains_its_blocks():
    """GpuInputLayer(fixed=...) with Linear + LayerNorm + ReLU blocks (row-wise), loss = (padded * W).sum() with W NaN in every padding
    slot: the gradient arriving at each block's output (a hook on the tensor) is the contract's, bit for bit - the upstream gradient of
    that loss is W itself; parameter gradients are torch's own backward: finite and non-zero.  The block of the third type is frozen
    and its input needs no gradient: no gradient is computed for its embedding (None)."""
    import torch
    from dynenv_amd import GpuInputLayer
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    specs = [(3, 4, ROW, -1, 5), (2, 3, ENV, 0, 4), (5, 2, CONST, 1, 1), (4, 0, CONST, 0, 0)]
    E, T, A, F = 24, 2, 3, 8
    obs_np, types, ce_np = R.make_dense(rng, E, T, A, specs)
    obs, ce = torch.from_numpy(obs_np).cuda(), torch.from_numpy(ce_np).cuda()
    rows, M = [3, 3, 2, 0], 6
    seq = lambda f: torch.nn.Sequential(torch.nn.Linear(f, F), torch.nn.LayerNorm(F), torch.nn.ReLU())
    blocks = torch.nn.ModuleList([seq(ty.feat) for ty in types]).cuda()
    for p in blocks[2].parameters():
        p.requires_grad_(False)
    layer = GpuInputLayer(blocks, _arr_types(types), E, A, T, obs_np.shape[3], fixed=dict(max_count=M, rows=rows))
    assert layer.blocks is blocks and layer.arranger.fixed
    seen, handed = {}, []
    def watch(i):
        def forward_hook(mod, args, out):   # (returns None: the output stays the block's)
            if out.requires_grad:
                out.register_hook(lambda g: seen.__setitem__(i, g.clone()))
        return forward_hook

    hooks = [b.register_forward_hook(watch(i)) for i, b in enumerate(blocks)]
    unpad = layer.arranger._unpad_as
    layer.arranger._unpad_as = lambda *a: handed.append(unpad(*a)) or handed[-1]
    padded, masks = layer(obs, ce)
    P = E * A
    assert padded.grad_fn is not None and tuple(padded.shape) == (T, M, P, F) and len(masks) == T
    pl = FR.plan(obs_np, types, rows, M, ce_np)
    assert pl["dropped"].any(), "the case drops rows"
    _same(layer.arranger.dropped, pl["dropped"].astype(np.int32), "dropped")
    _, r_mask = FR.gather(obs_np, types, rows, M, pl)
    W = rng.standard_normal((T, M, P, F)).astype(np.float32)
    W[r_mask.transpose(0, 2, 1).astype(bool)] = np.nan
    (padded * torch.from_numpy(W).cuda()).sum().backward()
    for h in hooks:
        h.remove()
    want = FR.unpad(W, rows, pl)
    assert sorted(seen) == [0, 1], "blocks 0 and 1 get a gradient, the frozen block 2 and the empty type 3 none"
    for i in (0, 1):
        _same(seen[i], want[i], "gradient at the output of block %d" % i)
    assert len(handed) == 1 and handed[0][2] is None and handed[0][3] is None and handed[0][0] is not None
    for i in (0, 1):
        for name, p in blocks[i].named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), (i, name)
    assert all(p.grad is None for p in blocks[2].parameters()) and all(p.grad is None for p in blocks[3].parameters())


def _make_env(cfg, E, seed=11):
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    if cfg == "driving_full":
        return BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed), [3, 3]
    if cfg == "driving_partial":
        return BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed, observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC,
                             noiseMagnitude=3), [3, 3]
    return BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=seed), [5, 3, 3, 7]


def _rowwise_block(feat, F, seed):
    """an embedding block that is row-wise AND the same arithmetic whatever the number of rows: out[n, f] = x[n, f % feat] * w[f] + b[f]
    (a matrix product may round differently at another row count; the two modes hand their blocks different row counts)"""
    import torch

    class Rowwise(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.register_buffer("idx", torch.arange(F) % feat)
            self.w = torch.nn.Parameter(torch.randn(F, generator=g))
            self.b = torch.nn.Parameter(torch.randn(F, generator=g))

        def forward(self, x):
            return x.index_select(1, self.idx) * self.w + self.b

    return Rowwise()


@pytest.mark.parametrize("cfg", ["driving_full", "driving_partial", "robocup_full"])
def test_a_captured_rollout_step(cfg):
    """step_flat(auto_reset=False) + counts() + GpuInputLayer(fixed=True) of both object groups, recorded ONCE with torch.cuda.graph on
    one stream - a capture fails at the first synchronisation or host copy - and replayed five times with new actions copied into the
    captured action tensor.  After every replay padded, masks and arranger.dropped (zero: rows = caps drops nothing) equal an eagerly
    stepped twin handle run through the DEFAULT arranger with the same blocks: leading slots bit for bit, zero / True behind them."""
    import torch
    from dynenv_amd import GpuInputLayer, groups_for
    E, F = 64, 8
    env, hi = _make_env(cfg, E)
    twin, _ = _make_env(cfg, E)
    env.reset_flat()
    twin.reset_flat()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    groups = groups_for(env)
    fixed, dflt = {}, {}
    for g, name in enumerate(("movable", "static")):
        blocks = torch.nn.ModuleList([_rowwise_block(t.feat, F, 10 * g + i) for i, t in enumerate(groups[name])]).cuda()
        fixed[name] = GpuInputLayer(blocks, groups[name], E, A, T, D, fixed=True)
        dflt[name] = GpuInputLayer(blocks, groups[name], E, A, T, D)
    static_a = torch.zeros((E, A, env.action_dim), dtype=torch.int32, device="cuda")
    out = {}
    with torch.no_grad():   # one eager call first, as before any capture: the kernels' code objects are loaded outside the recording
        for name in fixed:
            fixed[name](env.obs, env.counts())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        obs, _, _ = env.step_flat(static_a, auto_reset=False)
        ce = env.counts()
        for name in fixed:
            out[name] = fixed[name](obs, ce)
    twin.step_flat(static_a.clone(), auto_reset=False)   # (the capture ran nothing: the twin is where `env` is after its first replay)
    rng = np.random.default_rng(2)
    for r in range(5):
        if r:
            act = np.stack([rng.integers(0, k, (E, A)) for k in hi], -1).astype(np.int32)
            static_a.copy_(torch.from_numpy(act).cuda())
            twin.step_flat(static_a.clone(), auto_reset=False)
        graph.replay()
        assert torch.equal(env.obs.view(torch.int32), twin.obs.view(torch.int32)), "replay %d: the twin is elsewhere" % r
        for name in fixed:
            with torch.no_grad():
                want, want_masks = dflt[name](twin.obs, twin.counts())
            got, got_masks = out[name]
            M0 = want.shape[1]
            assert 0 < M0 <= got.shape[1] == sum(t.cap for t in groups[name])
            assert _bits(got[:, :M0]) == _bits(want), "replay %d, %s: padded" % (r, name)
            assert not bool(got[:, M0:].view(torch.int32).any())
            assert torch.equal(torch.stack(got_masks)[..., :M0], torch.stack(want_masks)) and bool(torch.stack(got_masks)[..., M0:].all())
            assert not bool(fixed[name].arranger.dropped.any())
    assert env.error_flags() == 0
    env.close()
    twin.close()
