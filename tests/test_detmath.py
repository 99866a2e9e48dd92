"""include/dynenv_math.h (host build, through the oracle library): accuracy vs glibc/numpy, edge cases, Philox KATs."""
import ctypes as C

import numpy as np
import pytest

import detmath_common as dc
import oracle_lib as ol
from detmath_common import _fdlibm_atan2, _fdlibm_atan_pos, _fma  # noqa: F401  (the references live in tests/detmath_common.py)


@pytest.fixture(scope="module", autouse=True)
def _built(oracle_built):
    return oracle_built


def _ulps(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.abs(b)), 5e-324)


def test_sincos_atan2_sqrt_within_2_ulp_of_libm():
    rng = np.random.default_rng(0)
    n = 400000
    x = np.concatenate([(rng.random(n // 2) - 0.5) * 2000.0, (rng.random(n // 2) - 0.5) * 8.0])
    y = np.concatenate([(rng.random(n // 2) - 0.5) * 2000.0, (rng.random(n // 2) - 0.5) * 1e-3])
    out = np.zeros((n, 5))
    ol.lib().oracle_math(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p))
    assert _ulps(out[:, 0], np.sin(x)).max() <= 2.0
    assert _ulps(out[:, 1], np.cos(x)).max() <= 2.0
    assert _ulps(out[:, 2], np.arctan2(y, x)).max() <= 2.0
    assert np.array_equal(out[:, 3], np.sqrt(np.abs(x)))  # correctly rounded
    assert np.array_equal(out[:, 4], x / y)


def test_fused_sincos_of_the_observation_code_within_2_ulp_of_libm():
    """dm_sincos_f (the vision passes' variant: Horner chains of fma) against glibc, and against the unfused dm_sincos: the two
    may differ in the last place, not more."""
    rng = np.random.default_rng(3)
    n = 400000
    x = np.ascontiguousarray(np.concatenate([(rng.random(n // 2) - 0.5) * 2000.0, (rng.random(n // 2) - 0.5) * 8.0]))
    out = np.zeros((n, 2))
    ol.lib().oracle_math_f(x.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p))
    assert _ulps(out[:, 0], np.sin(x)).max() <= 2.0
    assert _ulps(out[:, 1], np.cos(x)).max() <= 2.0
    ref = np.zeros((n, 5))
    ol.lib().oracle_math(x.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), n, ref.ctypes.data_as(C.c_void_p))
    assert _ulps(out[:, 0], ref[:, 0]).max() <= 2.0 and _ulps(out[:, 1], ref[:, 1]).max() <= 2.0
    ang = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 2 * np.pi / 180])
    o = np.zeros((len(ang), 2))
    ol.lib().oracle_math_f(ang.ctypes.data_as(C.c_void_p), len(ang), o.ctypes.data_as(C.c_void_p))
    assert _ulps(o[:, 0], np.sin(ang)).max() <= 1.0 and _ulps(o[:, 1], np.cos(ang)).max() <= 1.0


def test_special_angles_used_by_the_scene_constants():
    x = np.array([0.0, -0.0, 90.0, -90.0, -0.0, 0.0, 1.0])
    y = np.array([90.0, -90.0, 0.0, -0.0, -0.0, 0.0, 1.0])
    # atan2(y, x) as used by Road.getSpot's spotDir.angle (Road.py:114): math.atan2 semantics incl. signed zeros
    xs = np.array([0.0, -0.0, 90.0, -90.0, -90.0, 90.0])
    ys = np.array([90.0, -90.0, 0.0, -0.0, 0.0, -0.0])
    out = np.zeros((len(xs), 5))
    ol.lib().oracle_math(xs.ctypes.data_as(C.c_void_p), ys.ctypes.data_as(C.c_void_p), len(xs), out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out[:, 2], np.arctan2(ys, xs))
    ang = np.array([np.pi / 2, -np.pi / 2, -np.pi, np.pi, 0.0, 2 * np.pi / 180])
    out = np.zeros((len(ang), 5))
    ol.lib().oracle_math(ang.ctypes.data_as(C.c_void_p), ang.ctypes.data_as(C.c_void_p), len(ang), out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out[:, 0], np.sin(ang)) and np.array_equal(out[:, 1], np.cos(ang))


def test_philox4x32_10_known_answers():
    """Random123 kat_vectors for philox4x32-10."""
    l = ol.lib()
    cases = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    l.oracle_philox.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    for key, ctr, exp in cases:
        c = np.array(ctr, np.uint32)
        o = np.zeros(4, np.uint32)
        l.oracle_philox(key[0], key[1], c.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p))
        assert tuple(int(v) for v in o) == exp


def test_atan2_is_the_branching_fdlibm_evaluation_bit_for_bit():
    """dm_atan2 selects numerator, denominator, hi and lo instead of branching over the five ranges (one division instead of
    five arms on a diverging wavefront); it must stay the same arithmetic: bit patterns against the branching form, over the
    simulators' ranges, the range boundaries +- a few ulp, extreme magnitudes, zeros and infinities.  (The first range's
    t - t s: the header computes 0 - (fma(t, s, -0) - t), and fma(t, s, -0) = t s rounded once = the product.)"""
    x, y = dc.atan2_inputs(np.random.default_rng(5), 4000)
    out = np.zeros((len(x), 5))
    ol.lib().oracle_math(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p))
    with np.errstate(all="ignore"):
        ref = _fdlibm_atan2(y, x)
    got = out[:, 2]
    same = (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), [(y[i], x[i], got[i], ref[i]) for i in np.flatnonzero(~same)[:5]]


# ------------------------------------------------------------------------------------------------------------------------------------
# The math probe (include/dynenv_math_probe.h) on the host: oracle_math_probe over the whole input table of tests/detmath_common.py,
# every column against its independent reference.  tests/test_gpu_detmath.py then holds the device to the oracle AND to the same
# references: what passes here makes the oracle a verified stand-in there.
# ------------------------------------------------------------------------------------------------------------------------------------
def test_probe_table_is_what_its_tags_promise():
    """the header's sizes, and the properties of the input sets the other tests lean on"""
    assert dc.header_sizes() == (dc.NIN, dc.NOUT)
    tab = dc.table()
    assert 3000 <= len(tab) <= 12000 and tab.inp.shape == (len(tab), 4)
    a, b = tab.inp[:, 0], tab.inp[:, 1]
    # sincos inside the contract: finite, |x| < 1e6; outside: nothing finite
    for name in ("sincos.random", "sincos.quadrant", "sincos.tie", "sincos.tiny"):
        assert (np.abs(a[tab.rows(name)]) < 1.0e6).all(), name
    assert not np.isfinite(a[tab.rows("sincos.outside")]).any()
    # the tie set: x * invpio2 within a few ulp of a half-integer, and some rows exactly on it
    t = a[tab.rows("sincos.tie")] * dc.INVPIO2
    frac = np.abs(t - np.floor(t) - 0.5)
    assert (frac <= 8 * np.spacing(np.abs(t))).all() and (frac == 0.0).sum() >= 20
    # the wavefront block: starts on a wavefront, and EVERY group of 64 rows holds the five ranges with both signs of x and of y
    w0 = tab.start["atan2.wave"]
    n = int(tab.rows("atan2.wave").sum())
    assert w0 % 64 == 0 and n % 64 == 0 and n >= 64
    for g in range(w0, w0 + n, 64):
        x, y = a[g:g + 64], b[g:g + 64]
        combos = set(zip(dc.atan_row(np.abs(y / x)).tolist(), (x < 0).tolist(), (y < 0).tolist()))
        assert combos == {(r, sx, sy) for r in range(5) for sx in (False, True) for sy in (False, True)}, g
    # the atan2 set holds the range bounds +- 3 ulp, denormals, infinities and signed zeros
    x, y = a[tab.rows("atan2.host")], b[tab.rows("atan2.host")]
    with np.errstate(all="ignore"):
        q = np.abs(y / x)
    for bound in dc.ATAN_BOUNDS:
        assert (q == bound).any() and (q == np.nextafter(bound, 0.0)).any() and (q == np.nextafter(bound, 9.0)).any(), bound
    assert np.isinf(x).any() and (np.abs(x) == 5e-324).any() and (np.signbit(x) & (x == 0)).any()
    # rint's ties and the ends of the integers' range; the arithmetic sets reach the denormals and the infinities
    r = a[tab.rows("rint")]
    assert {0.5, 1.5, 2.5, -0.5, 2.0 ** 52 - 1, 2.0 ** 52 + 1, 2.0 ** 53, 0.49999999999999994, -0.49999999999999994} <= set(r.tolist())
    ar = tab.inp[tab.rows("arith.log") | tab.rows("arith.edges")]
    assert (np.abs(ar[np.isfinite(ar) & (ar != 0)]) < 2.2250738585072014e-308).any() and np.isinf(ar).any()
    # the powi set: the five bases, exponents 0 and 4096 among them
    pw = tab.inp[tab.rows("powi")]
    assert set(pw[:, 0].tolist()) == set(dc.POWI_BASES) and {0.0, 1.0, 4096.0, 1074.0, 1075.0} <= set(pw[:, 1].tolist())


def test_probe_exact_columns_match_their_references_bit_for_bit():
    """/, sqrt, rint (numpy IEEE), fma and every dms_* (exact rational arithmetic, composed as the header composes them), dm_atan2 and
    dm_atan (the branching fdlibm restatement), Philox, dm_unit and dm_randint (Python integers): bit patterns, over the whole table"""
    tab, got, ref = dc.table(), dc.oracle_table(), dc.references()
    assert set(ref) == set(range(dc.NOUT)) - set(dc.SINCOS_COLS) - {dc.COL["powi"]}
    for col, want in sorted(ref.items()):
        bad = dc.bit_mismatches(got[:, col], want, nan_equal=col not in dc.PACKED_COLS)
        assert len(bad) == 0, dc.describe(tab.inp, tab.set_of, col, bad, got[:, col], want, "oracle_math_probe against the reference")
    # the Random123 vectors sit in the table as they are published
    p0 = tab.start["philox"]
    for i, (_, _, exp) in enumerate(dc.PHILOX_KATS):
        words = got[p0 + i, list(dc.PACKED_COLS)].view(np.uint64)
        assert (int(words[0]) & dc.M32, int(words[0]) >> 32, int(words[1]) & dc.M32, int(words[1]) >> 32) == exp


def test_probe_powi_within_the_bound_of_square_and_multiply():
    """dm_powi against exact rational powers: relative error <= gamma(n - 1) = (n - 1) u / (1 - (n - 1) u), u = 2^-53 (n - 1 rounding
    errors in all: tests/detmath_common.py derives the count), and the exact result for powers of two to the ends of the range"""
    tab, got = dc.table(), dc.oracle_table()
    assert float(dc.powi_bound(4096)) < 4096 * 2.0 ** -53 * (1 + 1e-12)
    bad = dc.powi_failures(tab.inp, got[:, dc.COL["powi"]])
    assert not bad, "\n".join("row %d (set %s): %s" % (i, tab.set_of(i), m) for i, m in bad[:5])
    pw = tab.rows("powi")
    assert (got[pw & (tab.inp[:, 0] == 1.0), dc.COL["powi"]] == 1.0).all()
    assert (got[pw & (tab.inp[:, 1] == 0.0), dc.COL["powi"]] == 1.0).all()


def test_probe_sincos_columns_on_the_host():
    """sincos has no exact reference here: <= 2 ulp of libm over the ranges the environments use (NOT at the quadrant boundaries,
    where the two-stage reduction loses relative accuracy by design), the out-of-line and the inline column the same function, NaN
    outside the contract.  Everything else about these columns is the device test's: bit identity with this host evaluation."""
    tab, got = dc.table(), dc.oracle_table()
    r = tab.rows("sincos.random")
    x = tab.inp[r, 0]
    for k, f in ((0, np.sin), (1, np.cos), (4, np.sin), (5, np.cos)):
        assert _ulps(got[r, k], f(x)).max() <= 2.0, dc.COLS[k]
    assert _ulps(got[r, 4], got[r, 0]).max() <= 2.0 and _ulps(got[r, 5], got[r, 1]).max() <= 2.0
    ok = dc.sincos_compared(tab.inp)
    for k in (0, 1):
        assert len(dc.bit_mismatches(got[ok, k], got[ok, k + 2], True)) == 0
    out = tab.rows("sincos.outside")
    assert out.sum() == 3 and np.isnan(got[out][:, list(dc.SINCOS_COLS)]).all()
    inside = ok & np.isfinite(tab.inp[:, 0])
    assert not np.isnan(got[inside][:, list(dc.SINCOS_COLS)]).any()
    # exact values at the tiny end: sin x = x and cos x = 1 below 2^-28 (by value: the reduction turns sin(-0) into +0, on both sides)
    tiny = tab.rows("sincos.tiny") & (np.abs(tab.inp[:, 0]) < 2.0 ** -28)
    for k in (0, 4):
        assert (got[tiny, k] == tab.inp[tiny, 0]).all() and (got[tiny, k + 1] == 1.0).all()
