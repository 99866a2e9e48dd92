"""CPU-side checks of the arranger's backward entry points (dynenv_arrange_pad_backward / dynenv_arrange_scatter_backward): the header
declares them, the library exports them and the binding lists them, and every argument error is reported before a device is looked for,
so that it is the same with and without a GPU."""
import ctypes as C

import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_without_comments


@pytest.fixture(scope="module")
def capi():
    # torch before the library, the order every GPU test has: torch brings a HIP runtime of its own, and a process in which the library
    # was loaded first sees no device through it afterwards (this module sorts in front of the tests that would import torch first)
    import torch  # noqa: F401
    return built_capi()


def test_header_declares_both_entry_points_and_the_library_exports_them(capi):
    h = header_without_comments()
    assert ("int dynenv_arrange_pad_backward(const float* grad_padded_dev, const int32_t* counts_dev, const int32_t* base_dev, "
            "int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, float* const* grad_emb_dev, void* stream);") in h
    assert ("int dynenv_arrange_scatter_backward(const float* grad_padded_dev, const int32_t* slot_dev, int64_t N, int32_t F, "
            "float* grad_emb_dev, void* stream);") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    lib = capi.load()
    for name in ("dynenv_arrange_pad_backward", "dynenv_arrange_scatter_backward"):
        assert name in capi.EXPORTS
        assert hasattr(lib, name), "libdynenv_hip.so does not export " + name
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.dynenv_arrange_pad_backward.argtypes == [vp, vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp), vp]
    assert lib.dynenv_arrange_scatter_backward.argtypes == [vp, vp, C.c_int64, i32, vp, vp]


def test_header_comments_cite_the_reference(capi):
    c = comment_before("dynenv_arrange_pad_backward")
    assert "models.py:250-274" in c and ":147-166" in c and "catAndPad" in c
    assert "NULL" in c and "DYNENV_ERR_ARG" in c and "16-byte" in c
    c = comment_before("dynenv_arrange_scatter_backward")
    assert "dynenv_arrange_scatter" in c and "DYNENV_ERR_ARG" in c


# never dereferenced on the host: stand-ins for device pointers, 16-byte aligned like the real ones
def _fake():
    buf = (C.c_uint8 * 64)()
    return buf, C.cast(buf, C.c_void_p)


GOOD = dict(n_types=3, T=2, P=5, max_count=4, F=8)


@pytest.mark.parametrize("what, change", [
    ("null grad_padded", dict(grad=None)), ("null counts", dict(counts=None)), ("null base", dict(base=None)),
    ("null grad_emb", dict(gemb=None)),
    ("n_types 0", dict(n_types=0)), ("n_types 5", dict(n_types=5)), ("n_types < 0", dict(n_types=-1)),
    ("T 0", dict(T=0)), ("P 0", dict(P=0)), ("max_count < 0", dict(max_count=-1)),
    ("F 0", dict(F=0)), ("F 2", dict(F=2)), ("F 6", dict(F=6)), ("F 13", dict(F=13)), ("F < 0", dict(F=-4)),
    ("T above the grid's y limit", dict(T=65536)),
    ("P * F / 4 at 2^31", dict(P=2 ** 30, F=8)),
])
def test_pad_backward_argument_errors_come_before_the_device(capi, what, change):
    lib = capi.load()
    keep = [_fake() for _ in range(3)]
    vp = C.c_void_p
    ptrs = (vp * 4)(None, None, None, None)   # (a NULL destination is legal: no gradient wanted for that type)
    a = dict(GOOD, grad=keep[0][1], counts=keep[1][1], base=keep[2][1], gemb=ptrs)
    a.update(change)
    rc = lib.dynenv_arrange_pad_backward(a["grad"], a["counts"], a["base"], a["n_types"], a["T"], a["P"], a["max_count"], a["F"],
                                         a["gemb"], None)
    assert rc == ERR_ARG, what
    assert lib.dynenv_last_error()


@pytest.mark.parametrize("what, change", [
    ("N < 0", dict(N=-1)), ("F 0", dict(F=0)), ("F < 0", dict(F=-3)),
    ("null grad_padded", dict(grad=None)), ("null slot", dict(slot=None)), ("null grad_emb", dict(gemb=None)),
    ("more than one launch", dict(N=2 ** 40, F=2 ** 20)), ("N * F overflows", dict(N=2 ** 62, F=2 ** 30)),
])
def test_scatter_backward_argument_errors_come_before_the_device(capi, what, change):
    lib = capi.load()
    keep = [_fake() for _ in range(3)]
    a = dict(N=7, F=5, grad=keep[0][1], slot=keep[1][1], gemb=keep[2][1])
    a.update(change)
    assert lib.dynenv_arrange_scatter_backward(a["grad"], a["slot"], a["N"], a["F"], a["gemb"], None) == ERR_ARG, what
    assert lib.dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the two tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    lib = capi.load()
    keep = [_fake() for _ in range(3)]
    ptrs = (C.c_void_p * 4)(None, None, None, None)
    rc = lib.dynenv_arrange_pad_backward(keep[0][1], keep[1][1], keep[2][1], GOOD["n_types"], GOOD["T"], GOOD["P"], GOOD["max_count"],
                                         GOOD["F"], ptrs, None)
    assert rc == capi.ERR_NO_DEVICE
    assert lib.dynenv_arrange_scatter_backward(keep[0][1], keep[1][1], 7, 5, keep[2][1], None) == capi.ERR_NO_DEVICE
    assert lib.dynenv_arrange_scatter_backward(None, None, 0, 5, None, None) == capi.ERR_NO_DEVICE   # (N == 0: no pointer needed)
