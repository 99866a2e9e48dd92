"""CPU-side checks of dynenv_math_probe, the per-unit device probe of the deterministic math header: the header declares it and the
binding lists it, the ABI version stays, bad arguments are refused before a device is looked for, and without a device the call fails
loudly (there is no host evaluation behind this entry point: that is oracle_math_probe, test infrastructure)."""
import ctypes as C
import os

import numpy as np
import pytest

import detmath_common as dc
from host_common import ERR_ARG, ROOT, built_capi, header_without_comments


@pytest.fixture(scope="module")
def capi():
    return built_capi()


def test_header_declares_the_probe_and_the_binding_lists_it(capi):
    h = header_without_comments()
    assert "int dynenv_math_probe(int32_t unit, const double* in_host, int32_t n, double* out_host, int32_t device_id);" in h
    assert "#define DYNENV_MATH_UNIT_ROBOCUP 0" in h and "#define DYNENV_MATH_UNIT_DRIVING 1" in h
    assert (dc.UNIT_ROBOCUP, dc.UNIT_DRIVING) == (0, 1)
    assert "#define DYNENV_ABI_VERSION 3" in h, "an addition only: the ABI version stays"
    assert "dynenv_math_probe" in capi.EXPORTS and "dynenv_math_selftest" in capi.EXPORTS
    assert capi.SIGNATURES["dynenv_math_probe"] == (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32])
    lib = capi.load()
    assert hasattr(lib, "dynenv_math_probe") and lib.dynenv_abi_version() == 3
    # the header's comment gives the row sizes the probe's own header defines
    assert dc.header_sizes() == (4, 29)
    txt = open(os.path.join(ROOT, "include", "dynenv.h")).read()
    assert "[n, 4]" in txt and "[n, 29]" in txt


def test_both_units_include_the_one_row_and_the_oracle_does(capi):
    """the row is written once (include/dynenv_math_probe.h): each device unit wraps it in a kernel of its own, the oracle loops over it"""
    src = lambda *p: open(os.path.join(ROOT, *p)).read()
    for unit, kernel in (("dynenv_capi.hip", "rc_math_probe_kernel"), ("driving_tu.hip", "drv_math_probe_kernel")):
        txt = src("dynenv_amd", "csrc", unit)
        assert '#include "dynenv_math_probe.h"' in txt
        assert "%s(const double* in, int n, double* out) { dm_probe_wave(in, n, out); }" % kernel in txt, unit
    assert "dm_probe_row(" in src("oracle", "oracle_api.c") and '#include "dynenv_math_probe.h"' in src("oracle", "oracle_api.c")
    from dynenv_amd import build
    assert os.path.join(ROOT, "include", "dynenv_math_probe.h") in build.DEPS, "an edit of the row rebuilds the library"


def test_bad_arguments_are_refused_before_any_device_is_looked_for(capi):
    lib = capi.load()
    inp = np.zeros((2, dc.NIN))
    out = np.full((2, dc.NOUT), 3.0)
    pi, po = inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args, what in (((0, None, 2, po, 0), b"null"), ((1, pi, 2, None, 0), b"null"), ((0, pi, -1, po, 0), b"negative"),
                       ((2, pi, 2, po, 0), b"unit"), ((-1, pi, 2, po, 0), b"unit")):
        assert lib.dynenv_math_probe(*args) == ERR_ARG, args
        assert what in lib.dynenv_last_error(), (args, lib.dynenv_last_error())
    # no rows: nothing to do, with or without a device, either unit
    assert lib.dynenv_math_probe(0, pi, 0, po, 0) == 0 and lib.dynenv_math_probe(1, pi, 0, po, 0) == 0
    assert (out == 3.0).all()


def test_without_a_device_the_probe_fails_loudly(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    lib = capi.load()
    inp = np.zeros((2, dc.NIN))
    out = np.full((2, dc.NOUT), 3.0)
    for unit in (0, 1):
        rc = lib.dynenv_math_probe(unit, inp.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p), 0)
        assert rc == capi.ERR_NO_DEVICE and b"no HIP device" in lib.dynenv_last_error()
    # ... exactly as the existing self-test does
    x = np.zeros(2)
    assert lib.dynenv_math_selftest(x.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p), 0) == capi.ERR_NO_DEVICE
    assert (out == 3.0).all(), "nothing was computed on the host instead"
