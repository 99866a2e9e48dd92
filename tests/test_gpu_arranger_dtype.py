"""The 16-bit padded tensor on the device (csrc/arranger_cols_kernels.hip: the narrowing kernels and the bit-copy launches of the
copying ones, through dynenv_arrange_*_as and GpuInOutArranger / GpuInputLayer(padded_dtype=...)), bit for bit - no tolerance anywhere - against the numpy
statements of the arranger (tests/arranger_ref.py, arranger_grad_ref.py, arranger_fixed_ref.py) converted by tests/arranger_dtype_ref.py,
against the float32 path of the same device, and against the reference's recorded vectors.  Bit-compared inputs hold no NaN; one
assertion of its own checks that a NaN embedding gives a NaN slot.  -m gpu.

Shapes: four object types - caps 10 and 9 (a player runs the four-deep loop twice and the remainder loop), 3, and 0 (the None / NULL
type) - raw counts from below zero to above the caps, so the kept counts cover every residue mod 4; T = 1 and 3; P * F / 8 = 15 (less
than a wave), 45 (not a multiple of 64) and 340 (two blocks of 256, the second partial).  The C ABI test also runs the converting pairs at
F / 8 = 2 .. 64 (GROUP_SHAPES): the widening backward's lanes exchange their units in groups of that many before they store."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_ref as R  # noqa: E402
import arranger_grad_ref as GR  # noqa: E402
import arranger_fixed_ref as FR  # noqa: E402
import arranger_dtype_ref as DR  # noqa: E402

pytestmark = pytest.mark.gpu
ROW, ENV, CONST = R.COUNT_ROW, R.COUNT_ENV, R.COUNT_CONST
SPECS = [(3, 10, ROW, -2, 13), (2, 9, ENV, -1, 11), (4, 3, CONST, 2, 2), (2, 0, CONST, 3, 3)]
SHAPES = {"P15 F8 T1": (5, 3, 1, 8), "P15 F24 T3": (5, 3, 3, 24), "P20 F136 T3": (10, 2, 3, 136)}   # (E, A, T, F)
# F / 8 = 2 .. 64: the widening backward lets the 2 .. 64 lanes that share a row exchange their units before they store (at the shapes
# above the group is one lane); at F = 128 a wave holds four players with counts of their own
GROUP_SHAPES = {"F16 G2": (4, 2, 2, 16), "F32 G4": (4, 2, 2, 32), "F64 G8": (4, 2, 2, 64), "F128 G16": (4, 2, 2, 128), "F256 G32": (4, 2, 1, 256),
                "F512 G64": (4, 2, 1, 512), "F48 G2": (4, 2, 2, 48)}
FIXED_ROWS, FIXED_M = [9, 9, 2, 0], 17      # rows below the caps and M below their sum: rows are dropped, and rows behind the kept ones exist
PAIRS = [("f32", "bf16"), ("f32", "f16"), ("bf16", "bf16"), ("f16", "f16")]   # (embeddings, padded tensor)
CODE = {"f32": 0, "bf16": 1, "f16": 2}
SENTINEL = 0x7FA5    # a NaN in bf16 and in fp16 (and 0x7FA57FA5 one in float32): no expected output holds it


def _tdtype(kind):
    import torch
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _arr_types(types):
    from dynenv_amd import _capi
    return [_capi.ArrType(*(ty.astuple() + (0,))) for ty in types]


def _bits16(t):
    """a 16-bit device tensor's bit patterns, uint16 on the host"""
    import torch
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _to_dev(bits_or_f32, kind):
    """host float32 array, or uint16 bits of a 16-bit type -> device tensor of `kind`"""
    import torch
    if kind == "f32":
        return torch.from_numpy(np.ascontiguousarray(bits_or_f32, np.float32)).cuda()
    return torch.from_numpy(np.ascontiguousarray(bits_or_f32, np.uint16).view(np.int16)).cuda().view(_tdtype(kind))


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        v = {2: np.uint16, 4: np.uint32}[got.itemsize]
        bad = np.argwhere(got.view(v) != want.view(v))
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got 0x%X, want 0x%X"
                             % (what, len(bad), got.size, bad[0].tolist(), int(got.view(v)[at]), int(want.view(v)[at])))


def _host(t):
    """a device tensor on the host: float32 as it is, a 16-bit type as uint16 bits"""
    import torch
    return t.detach().cpu().numpy() if t.dtype == torch.float32 else _bits16(t)


@functools.lru_cache(maxsize=None)
def _case(shape, fixed):
    """One synthetic batch per shape and mode, computed once and shared (nothing in it is written to afterwards): the observation, the
    reference plan, and for every (embedding, padded) pair the embeddings, the expected padded bits, an upstream gradient that cycles
    through all non-NaN patterns in the real slots and is NaN in every padding slot, and the expected gradients."""
    E, A, T, F = SHAPES[shape] if shape in SHAPES else GROUP_SHAPES[shape]
    rng = np.random.default_rng(F * 7 + T)
    obs, types, ce = R.make_dense(rng, E, T, A, SPECS, lead=1, trail=2)
    P, n = E * A, len(types)
    if fixed:
        rows, M = FIXED_ROWS, FIXED_M
        pl = FR.plan(obs, types, rows, M, ce)
        assert pl["dropped"][:3].all() or shape not in SHAPES, "rows and slots are dropped"
        nrows = [T * P * r for r in rows]
        mask = FR.gather(obs, types, rows, M, pl)[1]
        pad = lambda embs: FR.pad(embs, rows, M, pl, F)
        unpad = lambda g: FR.unpad(g, rows, pl)
    else:
        pl = R.plan(obs, types, ce)
        M = pl["max_count"]
        _, slots, mask = R.gather(obs, types, pl)
        nrows = [int(v) for v in pl["total"]]
        pad = lambda embs: R.pad(embs, slots, T, M, P, F)
        unpad = lambda g: GR.unpad(g, slots)
    kept = pl["counts"][:2]   # the two long types: every residue mod 4, nothing kept, and two rounds of the four-deep loop plus a remainder
    if shape in SHAPES:
        assert set(range(4)) <= set((np.unique(kept) % 4).tolist()) and kept.max() >= 9 and (kept == 0).any()
    real = ~mask.transpose(0, 2, 1).astype(bool)    # [T, M, P]: slots that hold an object
    out = dict(E=E, A=A, T=T, F=F, P=P, n=n, M=M, obs=obs, types=types, ce=ce, pl=pl, nrows=nrows, mask=mask, rows=FIXED_ROWS if fixed else None,
               pairs={})
    for emb_kind, pad_kind in PAIRS:
        if emb_kind == "f32":   # values a rounding can get wrong: random mantissas over the whole exponent range of the type's normals
            embs = [(rng.standard_normal((r, F)) * np.exp2(rng.integers(-12, 13, (r, F)))).astype(np.float32) if r else None for r in nrows]
            embs32 = embs
        else:
            pats = DR.non_nan_patterns(emb_kind)
            embs = [pats[rng.integers(0, pats.size, (r, F))] if r else None for r in nrows]
            embs32 = [DR.widen(e, emb_kind) if e is not None else None for e in embs]
        padded = DR.narrow(pad(embs32), pad_kind)
        pats = DR.non_nan_patterns(pad_kind)
        nan = np.uint16(0x7FC1 if pad_kind == "bf16" else 0x7E01)
        up = np.full((T, M, P, F), nan, np.uint16)
        up[real] = pats[np.arange(int(real.sum()) * F) % pats.size].reshape(-1, F)
        g32 = unpad(DR.widen(up, pad_kind))
        grads = g32 if emb_kind == "f32" else [DR.narrow(g, emb_kind) for g in g32]
        out["pairs"][(emb_kind, pad_kind)] = dict(embs=embs, padded=padded, up=up, grads=grads, n_real=int(real.sum()) * F, n_pats=pats.size)
    return out


class Guarded(object):
    """`count` elements of `itemsize` bytes between two guard bands of 64 elements, every 16-bit word SENTINEL"""
    G = 64

    def __init__(self, count, itemsize):
        import torch
        self.words = itemsize // 2
        self.buf = torch.full(((count + 2 * self.G) * self.words,), SENTINEL, dtype=torch.int16, device="cuda")
        self.payload = self.buf[self.G * self.words:(self.G + count) * self.words]
        assert self.payload.data_ptr() % 16 == 0

    def ptr(self):
        return self.payload.data_ptr() if self.payload.numel() else None

    def check(self, what, written):
        b = self.buf.cpu().numpy().view(np.uint16)
        g = self.G * self.words
        assert (b[:g] == SENTINEL).all() and (b[b.size - g:] == SENTINEL).all(), what + ": a guard band was written"
        pay = b[g:b.size - g]
        if not written:
            assert (pay == SENTINEL).all(), what + ": written although its entry was NULL"
        elif self.words == 1:
            assert not (pay == SENTINEL).any(), what + ": an element was left unwritten"
        else:
            assert not (pay.view(np.uint32) == (SENTINEL << 16 | SENTINEL)).any(), what + ": an element was left unwritten"
        return pay if self.words == 1 else pay.view(np.float32)


C_ABI_CASES = [(s, fx, pr) for s in SHAPES for fx in (False, True) for pr in PAIRS] + \
              [(s, fx, pr) for s in GROUP_SHAPES for fx in (False, True) for pr in PAIRS[:2]]   # (the exchange is the converting pairs')


@pytest.mark.parametrize("shape, fixed, pair", C_ABI_CASES,
                         ids=["%s-%s-%s->%s" % (s, "fixed" if fx else "default", pr[0], pr[1]) for s, fx, pr in C_ABI_CASES])
def test_c_abi_writes_every_element_of_its_outputs_and_nothing_else(shape, fixed, pair):
    """dynenv_arrange_pad_as / _pad_backward_as and the fixed pair with every output inside a larger buffer of NaN sentinels.  The counts
    handed to the fixed calls are NOT yet limited to rows[i] and M: the kernels' own clamps do that."""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    c = _case(shape, fixed)
    d = c["pairs"][pair]
    T, P, M, F, n = c["T"], c["P"], c["M"], c["F"], c["n"]
    if shape == "P20 F136 T3":
        assert d["n_real"] >= d["n_pats"] and T * M * P * F >= 65536, "the gradient holds every non-NaN pattern of the type"
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    ec, pc = CODE[pair[0]], CODE[pair[1]]
    esize = 4 if pair[0] == "f32" else 2
    if fixed:
        counts = torch.from_numpy(c["pl"]["c"].astype(np.int32)).cuda()     # clamp(count, 0, cap) only
        third = (C.c_int32 * n)(*c["rows"])
        pad_fn, bwd_fn = lib.dynenv_arrange_fixed_pad_as, lib.dynenv_arrange_fixed_pad_backward_as
    else:
        counts = torch.from_numpy(c["pl"]["counts"].astype(np.int32)).cuda()
        base = torch.from_numpy(c["pl"]["base"].astype(np.int32)).cuda()
        third = vp(base.data_ptr())
        pad_fn, bwd_fn = lib.dynenv_arrange_pad_as, lib.dynenv_arrange_pad_backward_as
    embs = [_to_dev(e, pair[0]) if e is not None else None for e in d["embs"]]
    assert embs[3] is None, "the fourth type is the NULL one"
    e_ptrs = (vp * n)(*[e.data_ptr() if e is not None else None for e in embs])
    out = Guarded(T * M * P * F, 2)
    _capi.check(pad_fn(e_ptrs, ec, vp(counts.data_ptr()), third, n, T, P, M, F, vp(out.ptr()), pc, st), "pad")
    _same(out.check("padded", True).reshape(T, M, P, F), d["padded"], "padded")
    # a NULL embedding of a type WITH objects: zeros in its slots, everything else as before
    out2 = Guarded(T * M * P * F, 2)
    e_null = (vp * n)(e_ptrs[0], None, e_ptrs[2], None)
    _capi.check(pad_fn(e_null, ec, vp(counts.data_ptr()), third, n, T, P, M, F, vp(out2.ptr()), pc, st), "pad, NULL type")
    got2 = out2.check("padded (NULL type)", True).reshape(T, M, P, F)
    changed = got2 != d["padded"]
    assert changed.any() and not got2[changed].any(), "+0.0 exactly where type 1's embeddings were"

    up = _to_dev(d["up"], pair[1])
    for null in (None, 1):
        gs = [Guarded(r * F, esize) for r in c["nrows"]]
        g_ptrs = (vp * n)(*[g.ptr() if i != null else None for i, g in enumerate(gs)])
        _capi.check(bwd_fn(vp(up.data_ptr()), pc, vp(counts.data_ptr()), third, n, T, P, M, F, g_ptrs, ec, st), "pad_backward")
        for i, g in enumerate(gs):
            pay = g.check("grad_emb %d" % i, i != null)
            if i != null and c["nrows"][i]:
                _same(pay.reshape(-1, F), d["grads"][i], "grad_emb %d" % i)
                assert not (np.isnan(pay).any() if esize == 4 else DR.is_nan_bits(pay, pair[0]).any()), "a padding slot was read"
    if fixed:   # rows behind the kept ones: +0.0, all-zero bits
        k = c["pl"]["counts"][0].reshape(-1)
        behind = np.arange(c["rows"][0])[None, :] >= k[:, None]
        assert behind.any() and not d["grads"][0].reshape(T * P, c["rows"][0], F)[behind].view(np.uint8).any()

    # max_count == 0: nothing is launched, nothing written
    out0 = Guarded(8, 2)
    assert pad_fn(e_ptrs, ec, vp(counts.data_ptr()), third, n, T, P, 0, F, vp(out0.ptr()), pc, st) == 0
    g0 = [Guarded(r * F, esize) for r in c["nrows"]]
    assert bwd_fn(vp(up.data_ptr()), pc, vp(counts.data_ptr()), third, n, T, P, 0, F, (vp * n)(*[g.ptr() for g in g0]), ec, st) == 0
    out0.check("padded (max_count 0)", False)
    for i, g in enumerate(g0):
        g.check("grad_emb %d (max_count 0)" % i, False)


def test_c_abi_float32_pair_is_the_existing_call():
    """(F32, F32) is forwarded: the same bytes as dynenv_arrange_pad / _pad_backward"""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    c = _case("P15 F24 T3", False)
    d = c["pairs"][("f32", "bf16")]
    T, P, M, F, n = c["T"], c["P"], c["M"], c["F"], c["n"]
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    counts = torch.from_numpy(c["pl"]["counts"].astype(np.int32)).cuda()
    base = torch.from_numpy(c["pl"]["base"].astype(np.int32)).cuda()
    embs = [_to_dev(e, "f32") if e is not None else None for e in d["embs"]]
    e_ptrs = (vp * n)(*[e.data_ptr() if e is not None else None for e in embs])
    a, b = torch.empty((T, M, P, F), device="cuda"), torch.empty((T, M, P, F), device="cuda")
    _capi.check(lib.dynenv_arrange_pad_as(e_ptrs, 0, vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, vp(a.data_ptr()), 0, st), "pad_as")
    _capi.check(lib.dynenv_arrange_pad(e_ptrs, vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, vp(b.data_ptr()), st), "pad")
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == R.pad(d["embs"], R.gather(c["obs"], c["types"], c["pl"])[1], T, M, P, F).tobytes()
    ga, gb = [torch.full_like(e, 7.0) for e in embs[:3]], [torch.full_like(e, 9.0) for e in embs[:3]]
    for fn_as, gs in ((True, ga), (False, gb)):
        ptrs = (vp * n)(*[g.data_ptr() for g in gs], None)
        if fn_as:
            _capi.check(lib.dynenv_arrange_pad_backward_as(vp(a.data_ptr()), 0, vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, ptrs, 0, st), "bwd_as")
        else:
            _capi.check(lib.dynenv_arrange_pad_backward(vp(a.data_ptr()), vp(counts.data_ptr()), vp(base.data_ptr()), n, T, P, M, F, ptrs, st), "bwd")
    for i in range(3):   # (the gradient of the padded tensor itself: every embedding comes back)
        assert ga[i].cpu().numpy().tobytes() == gb[i].cpu().numpy().tobytes() == d["embs"][i].tobytes()


def _arranger(c, fixed, padded_dtype):
    from dynenv_amd import GpuInOutArranger
    fx = dict(max_count=FIXED_M, rows=FIXED_ROWS) if fixed else None
    return GpuInOutArranger(_arr_types(c["types"]), c["E"], c["A"], c["T"], c["obs"].shape[3], fixed=fx, padded_dtype=padded_dtype)


def _plan_on_device(arr, c):
    import torch
    return arr.rearrange_inputs(torch.from_numpy(c["obs"]).cuda(), torch.from_numpy(c["ce"]).cuda())


@pytest.mark.parametrize("kind", DR.KINDS)
@pytest.mark.parametrize("fixed", [False, True], ids=["default", "fixed"])
def test_conversion_on_the_device(fixed, kind):
    """the edge table of tests/test_arranger_dtype_ref.py in real slots: ties, carries into the exponent, overflow, subnormal results,
    signed zeros and infinities come out as arranger_dtype_ref (= torch's CPU cast) says; separately, a NaN stays a NaN"""
    import torch
    c = _case("P15 F24 T3", fixed)
    arr = _arranger(c, fixed, _tdtype(kind))
    _, countArr = _plan_on_device(arr, c)
    table = DR.edge_table()
    embs = [np.resize(np.roll(table, i), (r, c["F"])).astype(np.float32) if r else None for i, r in enumerate(c["nrows"])]
    assert embs[0].size >= table.size
    padded, _ = arr.rearrange_outputs([torch.from_numpy(e).cuda() if e is not None else None for e in embs], countArr)
    assert padded.dtype == _tdtype(kind) and tuple(padded.shape) == (c["T"], c["M"], c["P"], c["F"])
    pad32 = FR.pad(embs, c["rows"], c["M"], c["pl"], c["F"]) if fixed else \
        R.pad(embs, R.gather(c["obs"], c["types"], c["pl"])[1], c["T"], c["M"], c["P"], c["F"])
    _same(_bits16(padded), DR.narrow(pad32, kind), "padded")
    seen = set(np.unique(pad32.view(np.uint32)).tolist())
    assert set(table.view(np.uint32).tolist()) <= seen, "every edge sits in a real slot"
    # a NaN embedding gives a NaN slot (its payload is not compared), and nothing else changes
    nan_embs = [e.copy() if e is not None else None for e in embs]
    row = int(np.flatnonzero(c["pl"]["counts"][0].reshape(-1) > 0)[0]) * FIXED_ROWS[0] if fixed else 0   # a row that owns a slot
    nan_embs[0][row, 3] = np.nan
    nan_embs[0][row, 4] = np.uint32(0xFFC12345).view(np.float32)
    padded2, _ = arr.rearrange_outputs([torch.from_numpy(e).cuda() if e is not None else None for e in nan_embs], countArr)
    got, want = _bits16(padded2), _bits16(padded)
    isnan = DR.is_nan_bits(got, kind)
    assert int(isnan.sum()) == 2 and np.array_equal(got[~isnan], want[~isnan]) and bool(torch.isnan(padded2).sum() == 2)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s->%s" % p)
@pytest.mark.parametrize("fixed", [False, True], ids=["default", "fixed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_float32_path_on_the_device(shape, fixed, pair):
    """padded_16 == padded_32.to(dtype) for float32 embeddings and == float32_path(o.float()).to(dtype) for 16-bit embeddings o, the
    float32 arranger being the same mode with padded_dtype=None; inputs, counts and masks are unchanged by the option"""
    import torch
    c = _case(shape, fixed)
    d = c["pairs"][pair]
    a16, a32 = _arranger(c, fixed, _tdtype(pair[1])), _arranger(c, fixed, None)
    in16, plan16 = _plan_on_device(a16, c)
    in32, plan32 = _plan_on_device(a32, c)
    for x, y in zip(in16, in32):
        assert torch.equal(x, y)
    assert torch.equal(plan16[0], plan32[0]) and plan16[1] == plan32[1] == c["M"] and torch.equal(plan16[2], plan32[2])
    embs = [_to_dev(e, pair[0]) if e is not None else None for e in d["embs"]]
    p16, m16 = a16.rearrange_outputs(embs, plan16)
    p32, m32 = a32.rearrange_outputs([e.float() if e is not None else None for e in embs], plan32)
    assert p16.dtype == _tdtype(pair[1]) and p32.dtype == torch.float32 and p16.grad_fn is None
    _same(_bits16(p16), _bits16(p32.to(_tdtype(pair[1]))), "padded against the float32 path")
    _same(_bits16(p16), d["padded"], "padded against the reference")
    assert all(torch.equal(x, y) for x, y in zip(m16, m32)) and len(m16) == c["T"]
    if not fixed:
        assert np.array_equal(torch.stack(m16).cpu().numpy(), c["mask"].astype(bool))


def test_the_recorded_reference_vectors_in_bfloat16():
    """tests/golden/arranger.npz, the reference's own InOutArranger, through padded_dtype=bfloat16"""
    import torch
    from arranger_golden import CASES, G, ragged_from_golden
    from dynenv_amd import GpuInOutArranger, _capi
    from test_gpu_arranger import dense_from_ragged
    for name in CASES:
        x, (E, T, A, nT) = ragged_from_golden(name)
        feats = [int(f) for f in G[name + "/feats"]]
        caps = [int(G[name + "/x_counts"][..., i].max()) + 1 for i in range(nT)]
        o, offs, D = dense_from_ragged(x, feats, caps)
        types = [_capi.ArrType(int(offs[i]), feats[i], caps[i], _capi.ARR_COUNT_ROW, 0, D - nT + i, 0, 0) for i in range(nT)]
        arr = GpuInOutArranger(types, E, A, T, D, padded_dtype=torch.bfloat16)
        inputs, countArr = arr.rearrange_inputs(torch.tensor(o, device="cuda"))
        outs = []
        for i in range(nT):
            got = inputs[i].cpu().numpy()
            assert np.array_equal(got, G["%s/inputs%d" % (name, i)])
            outs.append(torch.tensor(got @ G["%s/W%d" % (name, i)], device="cuda") if got.size else None)
        padded, masks = arr.rearrange_outputs(outs, countArr)
        assert padded.dtype == torch.bfloat16
        _same(_bits16(padded), DR.narrow(G[name + "/padded"], "bf16"), name)
        assert np.array_equal(torch.stack(masks).cpu().numpy(), G[name + "/masks"])


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s->%s" % p)
@pytest.mark.parametrize("fixed", [False, True], ids=["default", "fixed"])
def test_autograd_hands_every_embedding_a_gradient_of_its_own_dtype(fixed, pair):
    """leaf embeddings of either dtype; type 1 needs no gradient and gets None; the plan outlives a later rearrange_inputs; the upstream
    gradient arrives once in the padded tensor's dtype, once as float32 through a permuted view"""
    import torch
    c = _case("P20 F136 T3", fixed)
    d = c["pairs"][pair]
    arr = _arranger(c, fixed, _tdtype(pair[1]))
    _, countArr = _plan_on_device(arr, c)
    calls = []
    unpad = arr._unpad_as
    arr._unpad_as = lambda *a: calls.append(unpad(*a)) or calls[-1]
    up = _to_dev(d["up"], pair[1])
    for upstream in ("own dtype", "float32, permuted"):
        embs = [_to_dev(e, pair[0]).requires_grad_(i != 1) if e is not None else None for i, e in enumerate(d["embs"])]
        padded, _ = arr.rearrange_outputs(embs, countArr)
        assert padded.grad_fn is not None and padded.dtype == _tdtype(pair[1])
        _same(_bits16(padded), d["padded"], "padded")
        # a later call of the same arranger on another batch: the plan of `padded` is its own
        other = R.make_dense(np.random.default_rng(99), c["E"], c["T"], c["A"], SPECS, lead=1, trail=2)
        arr.rearrange_inputs(torch.from_numpy(other[0]).cuda(), torch.from_numpy(other[2]).cuda())
        if upstream == "own dtype":
            padded.backward(up)
        else:   # [T, P, M, F] float32 handed back as a permuted view; the values are the 16-bit ones, so the cast back is exact
            g = up.float().permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
            assert not g.is_contiguous()
            padded.backward(g)
        for i in (0, 2):
            assert embs[i].grad.dtype == _tdtype(pair[0])
            _same(_host(embs[i].grad), d["grads"][i], "gradient of type %d, upstream %s" % (i, upstream))
        assert embs[1].grad is None and calls[-1][1] is None and calls[-1][3] is None, "no gradient is computed where none is wanted"
        if not fixed:
            assert arr.last_backward == "fused"
    assert len(calls) == 2


def test_bad_widths_and_alignment_raise():
    import torch
    from dynenv_amd import _capi
    for fixed in (False, True):
        c = _case("P15 F8 T1", fixed)
        arr = _arranger(c, fixed, torch.bfloat16)
        _, countArr = _plan_on_device(arr, c)
        with pytest.raises(_capi.DynEnvError, match="multiple of 8"):
            arr.rearrange_outputs([torch.ones((r, 12), device="cuda") if r else None for r in c["nrows"]], countArr)
        buf = torch.ones((c["nrows"][0] * 8 + 1,), device="cuda")
        off = [buf[1:].view(c["nrows"][0], 8)] + [torch.ones((r, 8), device="cuda") if r else None for r in c["nrows"][1:]]
        assert off[0].is_contiguous() and off[0].data_ptr() % 16 == 4
        with pytest.raises(_capi.DynEnvError, match="16-byte aligned"):
            arr.rearrange_outputs(off, countArr)
        with pytest.raises(ValueError):   # the row counts are the plan's
            arr.rearrange_outputs([torch.ones((r + 1, 8), device="cuda") if r else None for r in c["nrows"]], countArr)
    with pytest.raises(ValueError, match="padded_dtype"):
        _arranger(c, False, torch.float64)


def test_the_default_stays_float32():
    """padded_dtype=None is the code path it was: bf16 embeddings are cast to float32 outside and a float32 tensor comes back; mixed dtypes
    with a 16-bit padded tensor are cast to float32 too, and their gradients come back in each embedding's own dtype through torch's cast"""
    import torch
    c = _case("P15 F8 T1", False)
    d = c["pairs"][("bf16", "bf16")]
    arr = _arranger(c, False, None)
    assert arr.padded_dtype is None
    _, countArr = _plan_on_device(arr, c)
    embs = [_to_dev(e, "bf16") if e is not None else None for e in d["embs"]]
    padded, _ = arr.rearrange_outputs(embs, countArr)
    assert padded.dtype == torch.float32
    _same(_bits16(padded.to(torch.bfloat16)), d["padded"], "the float32 tensor holds the bf16 values")
    a16 = _arranger(c, False, torch.bfloat16)
    _, plan16 = _plan_on_device(a16, c)
    mixed = [embs[0].clone().requires_grad_(), embs[1].float().requires_grad_(), embs[2].clone().requires_grad_(), None]
    p16, _ = a16.rearrange_outputs(mixed, plan16)
    want, _ = a16.rearrange_outputs([m.detach().float() if m is not None else None for m in mixed], plan16)
    assert p16.dtype == torch.bfloat16 and torch.equal(p16.view(torch.int16), want.view(torch.int16))
    p16.backward(_to_dev(d["up"], "bf16"))
    assert [m.grad.dtype for m in mixed[:3]] == [torch.bfloat16, torch.float32, torch.bfloat16]
    _same(_host(mixed[0].grad), d["grads"][0], "gradient of the bf16 embedding among mixed ones")
    _same(_host(mixed[1].grad), DR.widen(d["grads"][1], "bf16"), "gradient of the float32 embedding among mixed ones")


def _blocks(kind, types, F):
    """embedding blocks whose output under torch.autocast(bfloat16) is float32 (a LayerNorm at the end, like the reference's EmbedBlock),
    bfloat16 (Linear only), or one of each"""
    import torch
    ln = lambda f: torch.nn.Sequential(torch.nn.Linear(f, F), torch.nn.LayerNorm(F))
    lin = lambda f: torch.nn.Linear(f, F)
    make = {"layernorm": [ln] * 4, "linear": [lin] * 4, "mixed": [ln, lin, ln, lin]}[kind]
    return torch.nn.ModuleList([m(ty.feat) for m, ty in zip(make, types)]).cuda()


@pytest.mark.parametrize("kind", ["layernorm", "linear", "mixed"])
@pytest.mark.parametrize("fixed", [False, True], ids=["default", "fixed"])
def test_input_layer_under_autocast(fixed, kind):
    """GpuInputLayer(padded_dtype=bfloat16) under torch.autocast(bfloat16) against a twin that shares the blocks, has padded_dtype=None and
    is followed by .to(bfloat16): with loss = (padded.float() * W).sum(), outputs and parameter gradients are equal"""
    import torch
    from dynenv_amd import GpuInputLayer
    torch.manual_seed(4)
    c = _case("P15 F24 T3", fixed)
    F = 16
    blocks = _blocks(kind, c["types"], F)
    fx = dict(max_count=FIXED_M, rows=FIXED_ROWS) if fixed else None
    args = (blocks, _arr_types(c["types"]), c["E"], c["A"], c["T"], c["obs"].shape[3])
    layer, twin = GpuInputLayer(*args, fixed=fx, padded_dtype=torch.bfloat16), GpuInputLayer(*args, fixed=fx)
    assert layer.blocks is twin.blocks and layer.arranger.padded_dtype is torch.bfloat16 and twin.arranger.padded_dtype is None
    obs, ce = torch.from_numpy(c["obs"]).cuda(), torch.from_numpy(c["ce"]).cuda()
    W = torch.randn((c["T"], c["M"], c["P"], F), device="cuda")
    seen = []
    hooks = [b.register_forward_hook(lambda mod, a, out: seen.append(out.dtype)) for b in blocks]
    results = []
    for net, cast in ((layer, False), (twin, True)):
        blocks.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            padded, masks = net(obs, ce)
            if cast:
                assert padded.dtype == torch.float32
                padded = padded.to(torch.bfloat16)
            assert padded.dtype == torch.bfloat16 and padded.grad_fn is not None
            loss = (padded.float() * W).sum()
        loss.backward()
        results.append((padded.detach().clone(), loss.detach().clone(), [None if p.grad is None else p.grad.clone() for p in blocks.parameters()], masks))
    for h in hooks:
        h.remove()
    want_kinds = {"layernorm": {torch.float32}, "linear": {torch.bfloat16}, "mixed": {torch.float32, torch.bfloat16}}[kind]
    assert set(seen) == want_kinds, "the blocks hand over what the case is about"
    (p_a, l_a, g_a, m_a), (p_b, l_b, g_b, m_b) = results
    assert torch.equal(p_a.view(torch.int16), p_b.view(torch.int16)) and torch.equal(l_a, l_b)
    assert all(torch.equal(x, y) for x, y in zip(m_a, m_b))
    n_grads = 0
    for x, y in zip(g_a, g_b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y) and bool(torch.isfinite(x).all())
            n_grads += bool(x.abs().sum() > 0)
    assert n_grads >= 6, "the first three types' blocks train (the fourth type has no rows)"


def _rowwise_block(feat, F, seed):
    """out[n, f] = x[n, f % feat] * w[f] + b[f]: row-wise and the same arithmetic whatever the number of rows"""
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


def test_a_captured_step_with_a_bfloat16_input_layer():
    """step_flat(auto_reset=False) + counts() + GpuInputLayer(fixed=True, padded_dtype=bfloat16), recorded once with torch.cuda.graph - a
    capture fails at the first synchronisation or host copy - and replayed twice on changing observations, against an eagerly stepped
    twin through the float32 fixed layer followed by .to(bfloat16)"""
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuInputLayer, groups_for
    E, F = 16, 8
    env, twin = BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=11), BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=11)
    env.reset_flat()
    twin.reset_flat()
    T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
    types = groups_for(env)["movable"]
    blocks = torch.nn.ModuleList([_rowwise_block(t.feat, F, i) for i, t in enumerate(types)]).cuda()
    layer = GpuInputLayer(blocks, types, E, A, T, D, fixed=True, padded_dtype=torch.bfloat16)
    eager = GpuInputLayer(blocks, types, E, A, T, D, fixed=True)
    static_a = torch.zeros((E, A, env.action_dim), dtype=torch.int32, device="cuda")
    with torch.no_grad():   # one eager call first, as before any capture: the kernels' code objects are loaded outside the recording
        layer(env.obs, env.counts())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        obs, _, _ = env.step_flat(static_a, auto_reset=False)
        out = layer(obs, env.counts())
    twin.step_flat(static_a.clone(), auto_reset=False)
    rng = np.random.default_rng(2)
    previous = None
    for r in range(2):
        if r:
            act = np.stack([rng.integers(0, k, (E, A)) for k in (3, 3)], -1).astype(np.int32)
            static_a.copy_(torch.from_numpy(act).cuda())
            twin.step_flat(static_a.clone(), auto_reset=False)
        graph.replay()
        assert torch.equal(env.obs.view(torch.int32), twin.obs.view(torch.int32)), "replay %d: the twin is elsewhere" % r
        with torch.no_grad():
            want, want_masks = eager(twin.obs, twin.counts())
        got, got_masks = out
        assert got.dtype == torch.bfloat16 and want.dtype == torch.float32
        assert torch.equal(got.view(torch.int16), want.to(torch.bfloat16).view(torch.int16)), "replay %d: padded" % r
        assert torch.equal(torch.stack(got_masks), torch.stack(want_masks))
        assert previous is None or not torch.equal(previous, got.view(torch.int16)), "the observations changed between the replays"
        previous = got.view(torch.int16).clone()
        assert not bool(layer.arranger.dropped.any())
    assert env.error_flags() == 0
    env.close()
    twin.close()
