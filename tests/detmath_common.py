"""What tests/test_detmath.py (CPU) and tests/test_gpu_detmath.py (-m gpu) share: the input table of the math probe
(include/dynenv_math_probe.h: dynenv_math_probe on the device, oracle_math_probe on the host), the probe's column names, and the
INDEPENDENT references of its columns - numpy IEEE arithmetic, an exact-rational fma, Python integers, a restatement of fdlibm's
branching atan.  None of them is the code under test.  A helper module: no tests in it.

The table is built once (table()): rows of (a, b, c, d), every row tagged with the input set it belongs to, so that a failure names its
set.  The references are computed once as well (references()) and never written to.

Which column means what on which inputs:
  * sincos (columns 0-5) has no exact reference here.  The header's domain is finite |x| < 1e6; a row with a finite |a| >= 1e6 is not
    compared in these columns at all ((int64_t)fn is undefined from 2^63 on, and the quadrant may differ between host and device);
    +-inf and NaN must give NaN on both sides.
  * every other column is defined for every row of the table, and compared for every row.
"""
import ctypes as C
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np

from rng_key_common import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIN = 4
COLS = ("sincos.sin", "sincos.cos", "sincos_inl.sin", "sincos_inl.cos", "sincos_v.sin", "sincos_v.cos", "atan2", "atan2_t", "atan",
        "sqrt", "div", "rint", "fma", "dms_dot", "dms_cross", "dms_point_vx", "dms_point_vy", "dms_rotate_x", "dms_rotate_y",
        "dms_xform_x", "dms_xform_y", "dms_k_scalar", "dms_acc_clamp0", "powi", "philox01", "philox23", "unit0", "unit1", "randint")
NOUT = len(COLS)
COL = {name: i for i, name in enumerate(COLS)}
SINCOS_COLS = tuple(range(6))
PACKED_COLS = (COL["philox01"], COL["philox23"])   # bit patterns, not numbers: never NaN-tolerant, never counted as NaN
UNIT_ROBOCUP, UNIT_DRIVING = 0, 1                  # DYNENV_MATH_UNIT_* of include/dynenv.h
UNITS = {"robocup-O3": UNIT_ROBOCUP, "driving-Os": UNIT_DRIVING}
M32 = 0xFFFFFFFF


def header_sizes():
    """(DM_PROBE_NIN, DM_PROBE_NOUT) as include/dynenv_math_probe.h spells them"""
    txt = open(os.path.join(ROOT, "include", "dynenv_math_probe.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % n, txt).group(1)) for n in ("DM_PROBE_NIN", "DM_PROBE_NOUT"))


# ------------------------------------------------------------------------------------------------ the references
def _fma(a, b, c):
    """a * b + c with one rounding, elementwise: exact rational arithmetic (the operands as integer ratios, one common denominator),
    then integer / integer -> float, which Python rounds correctly"""
    isfinite, inf = math.isfinite, math.inf

    def one(x, y, z):
        if not (isfinite(x) and isfinite(y) and isfinite(z)):
            if isfinite(x) and isfinite(y):
                return z      # a finite product, however large, plus an infinity or a NaN (the unfused x * y may overflow first)
            return x * y + z  # an infinite or NaN factor: the product is that exactly
        (nx, dx), (ny, dy), (nz, dz) = x.as_integer_ratio(), y.as_integer_ratio(), z.as_integer_ratio()
        num = nx * ny * dz + nz * dx * dy
        if num == 0:
            return x * y + z  # the sign of a zero result follows the IEEE rule of the unfused expression here
        try:
            return num / (dx * dy * dz)
        except OverflowError:
            return inf if num > 0 else -inf
    a, b, c = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(c, float))
    with np.errstate(all="ignore"):
        return np.array([one(x, y, z) for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())]).reshape(a.shape)


def _fdlibm_atan_pos(ax):
    """fdlibm __atan for ax >= 0 in its branching form (one arm per range), the polynomial's and the last range's multiply-adds
    fused as include/dynenv_math.h fuses them; evaluated with numpy (IEEE double) and an exact fma"""
    hi_t = np.array([4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00])
    lo_t = np.array([2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17])
    aT = [3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
          9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
          4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02]
    idx = np.where(ax < 0.4375, -1, np.where(ax < 0.6875, 0, np.where(ax < 1.1875, 1, np.where(ax < 2.4375, 2, 3))))
    t = np.where(idx == -1, ax, np.where(idx == 0, (2.0 * ax - 1.0) / (2.0 + ax), np.where(idx == 1, (ax - 1.0) / (ax + 1.0),
                 np.where(idx == 2, (ax - 1.5) / _fma(1.5, ax, 1.0), -1.0 / ax))))
    z = t * t
    w = z * z
    s1 = z * _fma(w, _fma(w, _fma(w, _fma(w, _fma(w, aT[10], aT[8]), aT[6]), aT[4]), aT[2]), aT[0])
    s2 = w * _fma(w, _fma(w, _fma(w, _fma(w, aT[9], aT[7]), aT[5]), aT[3]), aT[1])
    hi, lo = hi_t[np.maximum(idx, 0)], lo_t[np.maximum(idx, 0)]
    r = np.where(idx < 0, t - t * (s1 + s2), hi - (_fma(t, s1 + s2, -lo) - t))
    r = np.where(ax < 3.7252902984619140625e-09, ax, r)
    return np.where(ax >= 1.0e300, hi_t[3] + lo_t[3], r)


def _fdlibm_atan2(y, x):
    pi, pi_lo = 3.1415926535897931160e+00, 1.2246467991473531772e-16
    aq = np.abs(y / x)
    z = np.where(aq > 1.0e300, 1.5707963267948966, np.where((x < 0.0) & (aq < 1.0e-300), 0.0, _fdlibm_atan_pos(aq)))
    sx, sy = np.signbit(x), np.signbit(y)
    r = np.where(~sx, np.where(sy, -z, z), np.where(~sy, pi - (z - pi_lo), (z - pi_lo) - pi))
    r = np.where(x == 0.0, np.where(sy, -1.5707963267948966, 1.5707963267948966), r)
    return np.where(y == 0.0, np.where(sx, np.where(sy, -pi, pi), y), r)


def _fdlibm_atan(x):
    """dm_atan: the branching form on |x|, the sign put back the way the header does (x < 0 ? -r : r, so atan(-0) = +0)"""
    r = _fdlibm_atan_pos(np.abs(x))
    return np.where(x < 0.0, -r, r)


# the atan2 test's inputs: the special values (every pair of them is an input) ...
ATAN2_SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e300, -1e300, 1e-300, -1e-300, 5e-324, -5e-324, 1e-310, 0.4375, 0.6875,
                           1.1875, 2.4375, 3.7252902984619140625e-09, 2.0 ** -28, 1e308, 90.0, -90.0, 1e-9, 1e150, 1e-150])
ATAN_BOUNDS = (0.4375, 0.6875, 1.1875, 2.4375)


def atan2_special_grid():
    """(x, y): every pair of ATAN2_SPECIALS"""
    gx, gy = np.meshgrid(ATAN2_SPECIALS, ATAN2_SPECIALS)
    return gx.ravel(), gy.ravel()


def atan2_inputs(rng, n):
    """(x, y) of the fdlibm test: the special-value grid, then n each of the simulators' two ranges, log-uniform magnitudes over +-1400 in
    the exponent, a special value against a small one, and quotients at the four range bounds +- 3 ulp (the draws are made in this
    order: the host test's inputs for a given generator stay what they were)"""
    sp = ATAN2_SPECIALS
    gx, gy = atan2_special_grid()
    sgn = lambda: rng.choice([-1.0, 1.0], n)
    bx = (rng.random(n) + 0.5) * sgn()
    by = rng.choice(list(ATAN_BOUNDS), n) * (1 + rng.integers(-3, 4, n) * 2.2e-16) * bx * sgn()
    x = np.concatenate([gx, (rng.random(n) - 0.5) * 2000.0, (rng.random(n) - 0.5) * 8.0, np.exp((rng.random(n) - 0.5) * 1400) * sgn(), rng.choice(sp, n), bx])
    y = np.concatenate([gy, (rng.random(n) - 0.5) * 2000.0, (rng.random(n) - 0.5) * 1e-3, np.exp((rng.random(n) - 0.5) * 1400) * sgn(), (rng.random(n) - 0.5) * 8.0, by])
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def atan_row(aq):
    """the range of |y / x|, 0..4: number of range bounds <= aq (dm_atan_row, restated)"""
    return sum((~(aq < b)).astype(int) for b in ATAN_BOUNDS)


# ------------------------------------------------------------------------------------------------ words <-> doubles
def words_to_double(lo, hi):
    """the double whose bit pattern is hi << 32 | lo (uint32 arrays)"""
    return ((np.asarray(hi, np.uint64) << np.uint64(32)) | np.asarray(lo, np.uint64)).view(np.float64)


def double_words(x):
    """(low word, high word) of the bit patterns, as Python-int-safe uint64 arrays"""
    u = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return u & np.uint64(M32), u >> np.uint64(32)


def randint_range(b):
    """the (lo, hi) the probe hands dm_randint for a row's b: lo = (low word & 0xFFFFF) - 2^19, hi = lo + (high word & 0x3FFFFFFF)"""
    u2, u3 = double_words(b)
    lo = (u2 & np.uint64(0xFFFFF)).astype(np.int64) - (1 << 19)
    return lo, lo + (u3 & np.uint64(0x3FFFFFFF)).astype(np.int64)


def randint_b(lo, hi):
    """the b that makes the probe call dm_randint(u, lo, hi): -2^19 <= lo < 2^19, 0 <= hi - lo < 2^30"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    assert ((lo >= -(1 << 19)) & (lo < (1 << 19)) & (hi >= lo) & (hi - lo < (1 << 30))).all()
    return words_to_double((lo + (1 << 19)).astype(np.uint64), (hi - lo).astype(np.uint64))


# ------------------------------------------------------------------------------------------------ the input table
PHILOX_KATS = (((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
               ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
               ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
POWI_BASES = (0.9999, 0.999, 1.0, 0.5, 2.0)
INVPIO2 = 6.36619772367581382433e-01
# the ranges dm_randint is called with at reset (lanes, positions in a list, car types, sides, small counts), and the edges
RANDINT_RANGES = ((0, 0), (5, 5), (-3, -3), (-5, 5), (-1, 1), (0, 1), (0, 2), (0, 3), (1, 4), (1, 6), (0, 7), (0, 9), (0, 19), (0, 39),
                  (-(1 << 19), (1 << 19) - 1), (0, (1 << 30) - 1), ((1 << 19) - 1, (1 << 19) - 1 + (1 << 30) - 1))
U_EDGES = (0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)


def _ulp_steps(x, steps):
    """every x moved by each of `steps` units in the last place (np.nextafter, repeated)"""
    out = []
    for k in steps:
        v = x.copy()
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        out.append(v)
    return np.concatenate(out)


def _log_uniform(rng, n, lo_exp=-1074, hi_exp=1023):
    """magnitudes log-uniform over the doubles, denormals included, random sign"""
    return np.ldexp(1.0 + rng.random(n), rng.integers(lo_exp, hi_exp, n)) * rng.choice([-1.0, 1.0], n)


def _build_sets():
    rng = np.random.default_rng(20240607)
    sets = []

    def add(name, a, b=None, c=None, d=None):
        a = np.asarray(a, np.float64)
        n = len(a)
        fill = lambda v, scale: (rng.random(n) - 0.5) * scale if v is None else np.broadcast_to(np.asarray(v, np.float64), (n,))
        sets.append((name, np.stack([a, fill(b, 2000.0), fill(c, 8.0), fill(d, 2000.0)], axis=1)))

    # --- atan2, one wavefront at a time: rows 64 g .. 64 g + 63 hold all five ranges and both signs of x and y (row j: range j % 5,
    #     sign of x from bit 0 of j // 5, sign of y from bit 1).  FIRST in the table, so that a group is a wavefront of the probe.
    n = 64 * 8
    j = np.arange(n) % 64
    edges = np.array([0.0, 0.4375, 0.6875, 1.1875, 2.4375, 40.0])
    rg = j % 5
    q = edges[rg] + (edges[rg + 1] - edges[rg]) * (0.02 + 0.96 * rng.random(n))   # well inside its range: y / x rounds nowhere near a bound
    x = np.exp((rng.random(n) - 0.5) * 12.0) * np.where((j // 5) & 1, -1.0, 1.0)
    y = q * np.abs(x) * np.where((j // 10) & 1, -1.0, 1.0)
    add("atan2.wave", x, y)

    # --- sincos inside the contract (finite |x| < 1e6)
    add("sincos.random", np.concatenate([(rng.random(1000) - 0.5) * 2000.0, (rng.random(1000) - 0.5) * 8.0]))
    k = np.concatenate([np.arange(-40, 41), rng.integers(41, 600001, 100) * rng.choice([-1, 1], 100)]).astype(np.float64)
    add("sincos.quadrant", _ulp_steps(k * (np.pi / 2), range(-3, 4)))
    h = (np.concatenate([np.arange(0, 41), rng.integers(41, 600000, 60)]) + 0.5) * np.concatenate([rng.choice([-1.0, 1.0], 101)])
    add("sincos.tie", _ulp_steps(h / INVPIO2, range(-3, 4)))
    add("sincos.tiny", [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308, 2.0 ** -28,
                        -2.0 ** -28, 2.0 ** -27, 2.0 ** -29, 1e-300, -1e-300, 1e-9, -1e-9])
    # --- ... and outside it: NaN on both sides, whatever its sign and payload
    add("sincos.outside", [np.inf, -np.inf, np.nan], 1.0, 1.0, 1.0)

    # --- atan2(b, a): the whole input set of the host-only fdlibm test, at 200 samples per range
    x, y = atan2_inputs(rng, 200)
    add("atan2.host", x, y)

    # --- sqrt, /, rint, fma (and every dms_* with them) over the whole double range
    add("arith.log", _log_uniform(rng, 600), _log_uniform(rng, 600), _log_uniform(rng, 600), _log_uniform(rng, 600))
    # denormal operands and results, quotients and products that overflow or underflow, zeros and infinities: every pair of these
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308,
                   1.7976931348623157e308, -1.7976931348623157e308, 1e-160, -1e-160, 1e160, 1e-300, 1e300, 1.5, -3.0, 2.0 ** -537,
                   4.4501477170144023e-308])
    ga, gb = np.meshgrid(sp, sp)
    ga, gb = ga.ravel(), gb.ravel()
    add("arith.edges", ga, gb, np.roll(ga, 7), np.roll(gb, 3))
    # products that land in the denormals, with an addend there too (fma's one rounding at the bottom of the range)
    m = 200
    pa = _log_uniform(rng, m, -600, -400)
    add("arith.denormal", pa, _log_uniform(rng, m, -470, -430) / np.abs(pa) * 2.0 ** -600, _log_uniform(rng, m, -1074, -1040), _log_uniform(rng, m, -600, -400))
    kk = np.arange(0, 24, dtype=np.float64)
    r = np.concatenate([kk + 0.5, -(kk + 0.5), [2.0 ** 52 - 1, 2.0 ** 52 + 1, 2.0 ** 52 - 0.5, 2.0 ** 52, -(2.0 ** 52) - 1, -(2.0 ** 52) + 0.5,
                                                2.0 ** 51 + 0.5, 2.0 ** 51 + 1.5, 2.0 ** 53, -(2.0 ** 53), 0.49999999999999994, -0.49999999999999994,
                                                0.5000000000000001, 1e300, -1e300, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324]])
    add("rint", r)

    # --- dms_*: the solver's ranges (positions up to ~2000, unit normals, inverse masses and inertias as in the scenes) ...
    m = 200
    ang = rng.random(m) * 2 * np.pi
    pos = lambda: (rng.random(m) - 0.5) * 4000.0
    add("dms.solver", np.concatenate([pos(), np.cos(ang), 1.0 / rng.choice([1200.0, 1800.0, 3500.0, 5000.0, 90.0], m)]),
        np.concatenate([pos(), np.sin(ang), 1.0 / (rng.random(m) * 4e5 + 1e3)]),
        np.concatenate([np.cos(ang), pos(), (rng.random(m) - 0.5) * 50.0]),
        np.concatenate([np.sin(ang), pos(), (rng.random(m) - 0.5) * 50.0]))
    # ... and cancelling operands, where the fused and the unfused result part ways in more than the last place: for each of
    # a c + b d (dot), a d - b c (cross), a c - b d (rotate_x), a d + b c (rotate_y) the fourth operand solves "= 0", +- a few ulp
    m = 150
    blocks = []
    for form in range(4):
        a_, b_, t_ = pos(), pos(), (rng.random(m) - 0.5) * 4.0
        a_, b_, t_ = a_[:m], b_[:m], t_[:m]
        ul = 1.0 + rng.integers(-3, 4, m) * 2.2e-16
        if form == 0:
            c_, d_ = t_, -(a_ * t_) / b_ * ul          # a c = -b d
        elif form == 1:
            c_, d_ = t_, (b_ * t_) / a_ * ul           # a d = b c
        elif form == 2:
            c_, d_ = t_, (a_ * t_) / b_ * ul           # a c = b d
        else:
            c_, d_ = t_, -(b_ * t_) / a_ * ul          # a d = -b c
        blocks.append(np.stack([a_, b_, c_, d_], axis=1))
    cz = np.concatenate(blocks)
    F = Fraction
    keep = [all(v != 0 for v in (F(a) * F(c) + F(b) * F(d), F(a) * F(d) - F(b) * F(c), F(a) * F(c) - F(b) * F(d), F(a) * F(d) + F(b) * F(c)))
            for a, b, c, d in cz.tolist()]   # (the exact results are non-zero: the references' rule for the sign of a zero is the unfused one)
    cz = cz[np.array(keep)]
    add("dms.cancel", cz[:, 0], cz[:, 1], cz[:, 2], cz[:, 3])

    # --- dm_powi(a, (int)b): the dice thresholds' bases, exponents 0..4096 (all up to 64, around every power of two, around the ends
    #     of the double range for 0.5 and 2, and a random hundred)
    ex = sorted(set(list(range(0, 65)) + [p + s for p in (128, 256, 512, 1024, 2048, 4096) for s in (-1, 0, 1) if p + s <= 4096] +
                    [1021, 1022, 1073, 1074, 1075, 1076, 1077, 4000] + rng.integers(65, 4097, 100).tolist()))
    add("powi", np.repeat(POWI_BASES, len(ex)), np.tile(np.array(ex, np.float64), len(POWI_BASES)))

    # --- dm_unit / dm_randint: the words of a are u (both of them), the words of b the range
    us = np.array([(u0, u1) for u0 in U_EDGES for u1 in U_EDGES], np.uint64)
    lohi = np.array(RANDINT_RANGES, np.int64)
    ia, ib = np.meshgrid(np.arange(len(us)), np.arange(len(lohi)))
    ia, ib = ia.ravel(), ib.ravel()
    m = 300
    ra, rb = rng.integers(0, 2 ** 32, (m, 2), dtype=np.uint64), lohi[rng.integers(0, len(lohi), m)]
    add("int", np.concatenate([words_to_double(us[ia, 0], us[ia, 1]), words_to_double(ra[:, 0], ra[:, 1])]),
        np.concatenate([randint_b(lohi[ib, 0], lohi[ib, 1]), randint_b(rb[:, 0], rb[:, 1])]),
        words_to_double(rng.integers(0, 2 ** 32, len(ia) + m, dtype=np.uint64), rng.integers(0, 2 ** 32, len(ia) + m, dtype=np.uint64)),
        words_to_double(rng.integers(0, 2 ** 32, len(ia) + m, dtype=np.uint64), rng.integers(0, 2 ** 32, len(ia) + m, dtype=np.uint64)))

    # --- Philox: counter = the four words of (a, b), key = the low words of c and d; the Random123 vectors first
    m = 300
    w = rng.integers(0, 2 ** 32, (m, 8), dtype=np.uint64)
    w[:, 6:] = w[:, 6:] >> np.uint64(2)   # (the unused high words of c and d: any finite pattern)
    kat = np.array([[c[0], c[1], c[2], c[3], k[0], k[1], 0, 0] for k, c, _ in PHILOX_KATS], np.uint64)
    w = np.concatenate([kat, w])
    add("philox", words_to_double(w[:, 0], w[:, 1]), words_to_double(w[:, 2], w[:, 3]), words_to_double(w[:, 4], w[:, 6]), words_to_double(w[:, 5], w[:, 7]))
    return sets


class Table:
    def __init__(self, sets):
        self.names = [n for n, _ in sets]
        self.inp = np.ascontiguousarray(np.concatenate([r for _, r in sets]))
        self.set_id = np.concatenate([np.full(len(r), i) for i, (_, r) in enumerate(sets)])
        self.start = dict(zip(self.names, np.cumsum([0] + [len(r) for _, r in sets])[:-1]))
        self.inp.setflags(write=False)
        self.set_id.setflags(write=False)

    def __len__(self):
        return len(self.inp)

    def rows(self, name):
        """boolean mask of a set's rows"""
        return self.set_id == self.names.index(name)

    def set_of(self, i):
        return self.names[self.set_id[i]]


@functools.lru_cache(maxsize=None)
def table():
    return Table(_build_sets())


def sincos_compared(inp):
    """rows whose sincos columns mean something: not a finite |a| >= 1e6 (the header's domain; non-finite a must give NaN)"""
    a = inp[:, 0]
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(a) & (np.abs(a) >= 1.0e6))


def powi_exponent(b):
    """the n the probe hands dm_powi: (int)b for 0 <= b <= 4096, else 0"""
    with np.errstate(invalid="ignore"):
        return np.where((b >= 0.0) & (b <= 4096.0), np.trunc(np.where(np.isfinite(b), b, 0.0)), 0.0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def references():
    """column index -> the reference's values over the whole table, for every column that has an exact one (all but sincos and powi)"""
    return references_for(table().inp)


def references_for(inp):
    a, b, c, d = (np.ascontiguousarray(inp[:, i]) for i in range(4))
    ref = {}
    with np.errstate(all="ignore"):
        ref[COL["atan2"]] = ref[COL["atan2_t"]] = _fdlibm_atan2(b, a)
        ref[COL["atan"]] = _fdlibm_atan(a)
        ref[COL["sqrt"]] = np.sqrt(np.where(a < 0.0, -a, a))
        ref[COL["div"]] = a / b
        ref[COL["rint"]] = np.rint(a)
        ref[COL["fma"]] = _fma(a, b, c)
        # every dms_* composed as include/dynenv_math.h composes it, on the probe's operands
        ref[COL["dms_dot"]] = _fma(a, c, b * d)
        ref[COL["dms_cross"]] = _fma(a, d, -(b * c))
        ref[COL["dms_point_vx"]] = _fma(-b, c, a)
        ref[COL["dms_point_vy"]] = _fma(b, c, a)
        ref[COL["dms_rotate_x"]] = _fma(a, c, -(b * d))
        ref[COL["dms_rotate_y"]] = _fma(a, d, b * c)
        ref[COL["dms_xform_x"]] = _fma(a, c, _fma(-b, d, c))
        ref[COL["dms_xform_y"]] = _fma(b, c, _fma(a, d, d))
        rcn = _fma(c, a, -(d * b))
        ref[COL["dms_k_scalar"]] = _fma(b * rcn, rcn, a)
        s = _fma(a, b, c)
        ref[COL["dms_acc_clamp0"]] = np.where(s > 0.0, s, 0.0)
    # the integer routines, on Python integers
    u0, u1 = (w.tolist() for w in double_words(a))
    u2, u3 = (w.tolist() for w in double_words(b))
    k0, k1 = double_words(c)[0].tolist(), double_words(d)[0].tolist()
    lo, hi = (v.tolist() for v in randint_range(b))
    ph = [philox4x32_10((k0[i], k1[i]), (u0[i], u1[i], u2[i], u3[i])) for i in range(len(a))]
    ref[COL["philox01"]] = np.array([p[0] | (p[1] << 32) for p in ph], np.uint64).view(np.float64)
    ref[COL["philox23"]] = np.array([p[2] | (p[3] << 32) for p in ph], np.uint64).view(np.float64)
    ref[COL["unit0"]] = np.array([float(Fraction(u, 2 ** 32)) for u in u0])
    ref[COL["unit1"]] = np.array([float(Fraction(u, 2 ** 32)) for u in u1])
    ref[COL["randint"]] = np.array([float(lo[i] + ((u0[i] * (hi[i] - lo[i] + 1)) >> 32)) for i in range(len(a))])
    for v in ref.values():
        v.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------ dm_powi
# Square-and-multiply: b_k = b^(2^k) comes out of k squarings, each rounded once, so it carries e_k = 2 e_(k-1) + 1 = 2^k - 1 factors
# (1 + delta), |delta| <= u = 2^-53.  The result multiplies the b_k of n's set bits: popcount(n) - 1 rounded products (the first,
# 1.0 * b_k, is exact).  Altogether sum(2^k - 1) + popcount(n) - 1 = n - 1 factors: |r / b^n - 1| <= (1 + u)^(n-1) - 1 <= gamma(n - 1),
# gamma(m) = m u / (1 - m u) - the "n 2^-53" the dice thresholds of robocup_kernels.hip rely on.  It holds while nothing leaves the
# normal range (if the result is normal, so is every b_k that went into it).
U53 = Fraction(1, 2 ** 53)
MIN_NORMAL, MAX_DOUBLE = Fraction(2.2250738585072014e-308), Fraction(1.7976931348623157e308)


def powi_bound(n):
    m = max(n - 1, 0)
    return m * U53 / (1 - m * U53)


def powi_failures(inp, got):
    """rows whose dm_powi column breaks its claim: [(row, message)].  Finite base, exact power in the normal range (or exactly 0 or 1):
    relative error <= powi_bound(n).  A base that is a power of two outside that range: every step is exact until the range ends, so
    the result is the correctly rounded exact power (0 or inf in the end).  Other rows have no reference here.
    (Integers throughout: exact = N / D with D a power of two, got = gn / gd, bound = m / (2^53 - m) for m = n - 1.)"""
    n_all = powi_exponent(inp[:, 1])
    bad = []
    cache = {}
    lo_n, lo_d = (2.2250738585072014e-308).as_integer_ratio()
    hi_n = int(1.7976931348623157e308)
    for i, (base, n, g) in enumerate(zip(inp[:, 0].tolist(), n_all.tolist(), got.tolist())):
        if not math.isfinite(base):
            continue
        if (base, n) not in cache:
            p, q = base.as_integer_ratio()
            cache[(base, n)] = (p ** n, q ** n)
        N, D = cache[(base, n)]
        mag = abs(N)
        if mag == 0 or (mag * lo_d >= lo_n * D and mag <= hi_n * D):
            m = max(n - 1, 0)
            ok = math.isfinite(g)
            if ok:
                gn, gd = g.as_integer_ratio()
                ok = abs(gn * D - N * gd) * (2 ** 53 - m) <= m * mag * gd
            if not ok:
                bad.append((i, "dm_powi(%r, %d) = %r %s, exact %.17g, allowed relative error %.3g" % (base, n, g, hex64(g), N / D, float(powi_bound(n)))))
        elif math.frexp(base)[0] in (0.5, -0.5):
            try:
                want = N / D
            except OverflowError:
                want = math.inf if N > 0 else -math.inf
            if hex64(g) != hex64(want):
                bad.append((i, "dm_powi(%r, %d) = %r %s, the exact power rounds to %r %s" % (base, n, g, hex64(g), want, hex64(want))))
    return bad


# ------------------------------------------------------------------------------------------------ comparing bit patterns
def hex64(x):
    return "0x%016x" % int(np.float64(x).view(np.uint64))


def bit_mismatches(got, ref, nan_equal):
    """rows where the two columns differ in their bit patterns; two NaNs count as equal where `nan_equal` (bool or mask) says so"""
    got, ref = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(ref, np.float64)
    same = got.view(np.uint64) == ref.view(np.uint64)
    same |= np.isnan(got) & np.isnan(ref) & nan_equal
    return np.flatnonzero(~same)


def describe(tab_inp, set_of, col, rows, got, ref, what):
    """the failure message: the column, then for the first few rows the input set, the inputs and both bit patterns"""
    lines = ["%s: %d row(s) differ in column %d (%s)" % (what, len(rows), col, COLS[col])]
    for i in rows[:5]:
        lines.append("  row %d, set %s, (a, b, c, d) = (%s) [%s]: got %r %s, expected %r %s" %
                     (i, set_of(i), ", ".join(repr(float(v)) for v in tab_inp[i]), " ".join(hex64(v) for v in tab_inp[i]),
                      float(got[i]), hex64(got[i]), float(ref[i]), hex64(ref[i])))
    return "\n".join(lines)


def run_oracle(inp):
    """oracle_math_probe over [n, 4] -> [n, NOUT]"""
    import oracle_lib as ol
    inp = np.ascontiguousarray(inp, np.float64)
    out = np.zeros((len(inp), NOUT))
    fn = ol.lib().oracle_math_probe
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_void_p], None
    fn(inp.ctypes.data_as(C.c_void_p), len(inp), out.ctypes.data_as(C.c_void_p))
    return out


@functools.lru_cache(maxsize=None)
def oracle_table():
    out = run_oracle(table().inp)
    out.setflags(write=False)
    return out
