"""The numpy conversions of tests/arranger_dtype_ref.py against torch's own CPU casts, bit for bit: the GPU tests of the 16-bit padded tensor
compare the kernels with arranger_dtype_ref, and the conversion contract (include/dynenv.h) promises torch's `.to(dtype)` for every
non-NaN input.  No device."""
import numpy as np
import pytest

import arranger_dtype_ref as DR

torch = pytest.importorskip("torch")
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16}


def _torch_narrow(x, kind):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(TORCH[kind]).view(torch.int16).numpy().view(np.uint16)


def _torch_widen(bits, kind):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(TORCH[kind]).float().numpy()


def _same_bits(got, want, inputs, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d differ, first input bits 0x%08X: got 0x%04X, torch 0x%04X" % (
        what, bad.size, int(np.asarray(inputs).view(np.uint32)[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


@pytest.mark.parametrize("kind", DR.KINDS)
def test_the_edge_table(kind):
    t = DR.edge_table()
    _same_bits(DR.narrow(t, kind), _torch_narrow(t, kind), t, "edge table -> " + kind)


def test_the_edges_land_where_the_contract_says():
    n = lambda bits, kind: int(DR.narrow(DR.f32(bits), kind)[0])
    assert n(0x3F808000, "bf16") == 0x3F80 and n(0x3F818000, "bf16") == 0x3F82, "ties go to the even neighbour"
    assert n(0x3F808001, "bf16") == 0x3F81 and n(0x3F807FFF, "bf16") == 0x3F80
    assert n(0x3F7FFFFF, "bf16") == 0x3F80 and n(0x3F7FFFFF, "f16") == 0x3C00, "the carry runs into the exponent: 1.0"
    assert n(0x7F7FFFFF, "bf16") == 0x7F80 and n(0xFF7FFFFF, "bf16") == 0xFF80, "overflow to infinity"
    assert n(0x00400000, "bf16") == 0x0040, "a float32 subnormal is a bf16 subnormal"
    v = lambda x, kind: int(DR.narrow(np.array([x], np.float32), kind)[0])
    assert v(65519.99, "f16") == 0x7BFF and v(65520.0, "f16") == 0x7C00 and v(-65520.0, "f16") == 0xFC00
    assert v(5.9604644775390625e-08, "f16") == 0x0001 and v(2.98023223876953125e-08, "f16") == 0x0000, "2^-25 is a tie: to even, zero"
    assert v(2.9802325940409414e-08, "f16") == 0x0001 and v(8.94069671630859375e-08, "f16") == 0x0002
    assert v(-1e-9, "f16") == 0x8000 and v(1e-9, "f16") == 0x0000, "underflow keeps the sign"
    for kind in DR.KINDS:
        assert [n(b, kind) for b in (0x00000000, 0x80000000)] == [0x0000, 0x8000]
    assert [n(b, "bf16") for b in (0x7F800000, 0xFF800000)] == [0x7F80, 0xFF80]
    assert [n(b, "f16") for b in (0x7F800000, 0xFF800000)] == [0x7C00, 0xFC00]


@pytest.mark.parametrize("kind", DR.KINDS)
def test_random_bit_patterns(kind):
    rng = np.random.default_rng(5)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    # around every 16-bit value of the type: the halfway patterns and their neighbours
    shift = 16 if kind == "bf16" else 13
    near = (rng.integers(0, 2 ** 32 >> shift, 50000, dtype=np.uint64).astype(np.uint32) << np.uint32(shift)) | np.uint32(1 << (shift - 1))
    u = np.concatenate([u, near, near - np.uint32(1), near + np.uint32(1)])
    x = u.view(np.float32)
    x = x[~np.isnan(x)]
    _same_bits(DR.narrow(x, kind), _torch_narrow(x, kind), x, "random -> " + kind)


@pytest.mark.parametrize("kind", DR.KINDS)
def test_widening_is_exact_on_every_pattern(kind):
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got, want = DR.widen(allb, kind), _torch_widen(allb, kind)
    ok = ~DR.is_nan_bits(allb, kind)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])
    assert np.isnan(got[~ok]).all() and not np.isnan(got[ok]).any()
    # and narrowing takes every non-NaN pattern back to itself
    pats = DR.non_nan_patterns(kind)
    assert pats.size == (65536 - 254 if kind == "bf16" else 65536 - 2046)
    assert np.array_equal(DR.narrow(DR.widen(pats, kind), kind), pats)
