"""The deterministic math header ON THE DEVICE, routine by routine and build by build: dynenv_math_probe (include/dynenv_math_probe.h)
runs every routine of include/dynenv_math.h - and the kernels' own variants of csrc/dev_common.h: dev_sincos, dev_sincos_inl,
dev_sincos_v, dev_atan2, dev_atan2_t with its table in LDS - in the kernel of one translation unit: the RoboCup / C ABI unit (-O3)
or the Driving unit (-Os).  Each carries its own compiled copy of all of them.

Compared, per unit, over the whole input table of tests/detmath_common.py (a few thousand rows: quadrant boundaries and rint ties of
the reduction, the five atan ranges in every wavefront, range bounds +- 3 ulp, denormals, overflow, infinities, signed zeros, the
solver's cancelling operands, the Random123 vectors ...):
  * every column with oracle_math_probe, the host evaluation of the same row (tests/test_detmath.py pins that to the references);
  * every column that has an exact independent reference with that reference directly;
  * dev_atan2_t with dev_atan2 of the same launch - device against device, the claim in dev_common.h;
  * the first n rows alone, for n that leave a partial last wavefront.
Bit patterns throughout.  Two NaNs count as equal only where the host gives a NaN as well, and the numbers of NaNs must agree."""
import ctypes as C

import numpy as np
import pytest

import detmath_common as dc
import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from dynenv_amd import _capi
    ol.build()
    return _capi.load()


def _probe(lib, unit, inp):
    inp = np.ascontiguousarray(inp, np.float64)
    out = np.full((len(inp), dc.NOUT), -7.0)   # (no routine leaves this value in every column: an unwritten row shows)
    rc = lib.dynenv_math_probe(unit, inp.ctypes.data_as(C.c_void_p), len(inp), out.ctypes.data_as(C.c_void_p), 0)
    assert rc == 0, lib.dynenv_last_error()
    return out


@pytest.fixture(scope="module")
def device_tables(lib):
    """unit name -> the probe's output over the whole table: ONE launch per unit, shared by every test below, never written to"""
    outs = {}
    for name, unit in dc.UNITS.items():
        out = _probe(lib, unit, dc.table().inp)
        out.setflags(write=False)
        outs[name] = out
    return outs


@pytest.mark.parametrize("unit", list(dc.UNITS))
def test_device_matches_host_bit_for_bit(device_tables, unit):
    tab, dev, host = dc.table(), device_tables[unit], dc.oracle_table()
    sincos_ok = dc.sincos_compared(tab.inp)
    for col in range(dc.NOUT):
        rows = sincos_ok if col in dc.SINCOS_COLS else np.ones(len(tab), bool)
        idx = np.flatnonzero(rows)
        # (a NaN equals a NaN where the host's value is one - whatever the set, "outside the contract" included - and nowhere else)
        bad = idx[dc.bit_mismatches(dev[idx, col], host[idx, col], nan_equal=col not in dc.PACKED_COLS)]
        assert len(bad) == 0, dc.describe(tab.inp, tab.set_of, col, bad, dev[:, col], host[:, col], "unit %s, gfx950 against the host" % unit)
        if col not in dc.PACKED_COLS:
            assert np.isnan(dev[idx, col]).sum() == np.isnan(host[idx, col]).sum(), "unit %s, column %s: NaN counts differ" % (unit, dc.COLS[col])
    out = tab.rows("sincos.outside")
    assert np.isnan(dev[out][:, list(dc.SINCOS_COLS)]).all(), "unit %s: sincos of +-inf / NaN must be NaN" % unit


@pytest.mark.parametrize("unit", list(dc.UNITS))
def test_device_matches_the_independent_references(device_tables, unit):
    """/, sqrt, rint, fma, every dms_*, atan2 (both variants), atan, Philox, dm_unit, dm_randint: the device against numpy / exact
    rational / integer arithmetic, not through the oracle; dm_powi against exact powers within the bound of square-and-multiply"""
    tab, dev, ref = dc.table(), device_tables[unit], dc.references()
    for col, want in sorted(ref.items()):
        bad = dc.bit_mismatches(dev[:, col], want, nan_equal=col not in dc.PACKED_COLS)
        assert len(bad) == 0, dc.describe(tab.inp, tab.set_of, col, bad, dev[:, col], want, "unit %s, gfx950 against the reference" % unit)
    p0 = tab.start["philox"]
    for i, (_, _, exp) in enumerate(dc.PHILOX_KATS):
        w = dev[p0 + i, list(dc.PACKED_COLS)].view(np.uint64)
        assert (int(w[0]) & dc.M32, int(w[0]) >> 32, int(w[1]) & dc.M32, int(w[1]) >> 32) == exp, "unit %s: Random123 vector %d" % (unit, i)
    pw = np.flatnonzero(tab.rows("powi"))
    bad = dc.powi_failures(tab.inp[pw], dev[pw, dc.COL["powi"]])
    assert not bad, "unit %s\n" % unit + "\n".join("row %d: %s" % (pw[i], m) for i, m in bad[:5])


@pytest.mark.parametrize("unit", list(dc.UNITS))
def test_table_lookup_atan2_is_the_selecting_atan2_on_the_device(device_tables, unit):
    """dev_atan2_t (the range's constants from the LDS table, row address per lane) against dev_atan2 (select chains) of the same
    launch: 'bit-identical to dm_atan2' (dev_common.h).  Likewise the out-of-line and the inline dm_sincos."""
    tab, dev = dc.table(), device_tables[unit]
    for col, other, rows in ((dc.COL["atan2_t"], dc.COL["atan2"], np.ones(len(tab), bool)), (2, 0, dc.sincos_compared(tab.inp)),
                             (3, 1, dc.sincos_compared(tab.inp))):
        idx = np.flatnonzero(rows)
        bad = idx[dc.bit_mismatches(dev[idx, col], dev[idx, other], nan_equal=True)]
        assert len(bad) == 0, dc.describe(tab.inp, tab.set_of, col, bad, dev[:, col], dev[:, other],
                                          "unit %s, %s against %s of the same launch" % (unit, dc.COLS[col], dc.COLS[other]))


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
@pytest.mark.parametrize("unit", list(dc.UNITS))
def test_partial_wavefronts_give_the_same_rows(lib, device_tables, unit, n):
    """the first n rows alone: the last wavefront's out-of-line calls and its LDS lookup run under a partial exec mask (n = 1000: 40 of
    64 lanes).  The rows are the atan2 block that puts all five ranges into every wavefront, then the sincos sets."""
    full = device_tables[unit]
    out = _probe(lib, dc.UNITS[unit], dc.table().inp[:n])
    assert out.shape == (n, dc.NOUT)
    for col in range(dc.NOUT):
        bad = dc.bit_mismatches(out[:, col], full[:n, col], nan_equal=col not in dc.PACKED_COLS)
        assert len(bad) == 0, dc.describe(dc.table().inp, dc.table().set_of, col, bad, out[:, col], full[:, col],
                                          "unit %s, n = %d against the first rows of the full launch" % (unit, n))


def test_no_rows_is_ok_and_bad_arguments_are_refused_on_a_machine_with_a_device(lib):
    buf = np.zeros((1, dc.NOUT))
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.dynenv_math_probe(0, p, 0, p, 0) == 0
    assert lib.dynenv_math_probe(2, p, 1, p, 0) == -1 and lib.dynenv_math_probe(0, None, 1, p, 0) == -1
    assert lib.dynenv_math_probe(0, p, -1, p, 0) == -1 and lib.dynenv_math_probe(0, p, 1, p, 1 << 20) == -1
    assert (buf == 0).all()
