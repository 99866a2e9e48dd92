"""CPU-side checks of the fixed-shape arranger's entry points (dynenv_arrange_fixed_gather / _pad / _pad_backward): the header declares
them, the library exports them and the binding lists them with as many parameters, and every argument error is reported before a
device is looked for, so that it is the same with and without a GPU."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_without_comments

NAMES = ("dynenv_arrange_fixed_gather", "dynenv_arrange_fixed_pad", "dynenv_arrange_fixed_pad_backward")


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_points_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_arrange_fixed_gather(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, "
            "const dynenv_arr_type_t* types, int32_t n_types, const int32_t* count_env_dev, const int32_t* rows , int32_t max_count, "
            "int32_t* counts_dev, int32_t* obj_counts_dev, float* const* inputs_dev, uint8_t* mask_dev, int32_t* dropped_dev, "
            "void* stream);") in h
    assert ("int dynenv_arrange_fixed_pad(const float* const* emb_dev, const int32_t* counts_dev, const int32_t* rows, int32_t n_types, "
            "int32_t T, int32_t P, int32_t max_count, int32_t F, float* padded_dev, void* stream);") in h
    assert ("int dynenv_arrange_fixed_pad_backward(const float* grad_padded_dev, const int32_t* counts_dev, const int32_t* rows, "
            "int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, float* const* grad_emb_dev, void* stream);") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    lib = capi.load()
    for name in NAMES:
        params = re.search(r"int %s ?\(([^()]*)\) ?;" % name, h).group(1)
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == params.count(",") + 1, name
        assert hasattr(lib, name), "libdynenv_hip.so does not export " + name
        assert getattr(lib, name).argtypes == argtypes


def test_header_comments_state_the_contract_and_cite_the_reference(capi):
    c = comment_before("dynenv_arrange_fixed_gather")
    assert "models.py:219-250" in c and "earlier types win" in c and "dropped_dev" in c and "DYNENV_ERR_ARG" in c and "hipGraph" in c
    c = comment_before("dynenv_arrange_fixed_pad")
    assert "models.py:252-274" in c and ":147-180" in c and "16-byte" in c and "NULL" in c
    c = comment_before("dynenv_arrange_fixed_pad_backward")
    assert ":147-180" in c and "exactly once" in c and "never read" in c


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


def _types(capi, specs):
    return (capi.ArrType * len(specs))(*[capi.ArrType(*s) for s in specs])


def _gather_args(capi):
    """well-formed: three types (ROW / ENV / CONST counts) inside a row of 40 floats"""
    keep = [_fake() for _ in range(6)]
    C0, CE, CR = capi.ARR_COUNT_CONST, capi.ARR_COUNT_ENV, capi.ARR_COUNT_ROW
    types = _types(capi, [(0, 3, 5, CR, 0, 38, 0, 0), (15, 2, 7, CE, 0, 1, 2, 0), (29, 4, 2, C0, 1, 0, 0, 0)])
    a = dict(obs=keep[0][1], E=3, T=2, A=2, D=40, types=types, n_types=3, count_env=keep[1][1], rows=(C.c_int32 * 3)(5, 7, 2),
             max_count=14, counts=keep[2][1], obj_counts=keep[3][1], inputs=(C.c_void_p * 3)(None, None, None), mask=keep[4][1],
             dropped=keep[5][1])
    return keep, a


def _gather(lib, a):
    return lib.dynenv_arrange_fixed_gather(a["obs"], a["E"], a["T"], a["A"], a["D"], a["types"], a["n_types"], a["count_env"], a["rows"],
                                           a["max_count"], a["counts"], a["obj_counts"], a["inputs"], a["mask"], a["dropped"], None)


@pytest.mark.parametrize("what, change", [
    ("null obs", dict(obs=None)), ("null types", dict(types=None)), ("null rows", dict(rows=None)), ("null counts", dict(counts=None)),
    ("null obj_counts", dict(obj_counts=None)),
    ("n_types 0", dict(n_types=0)), ("n_types 5", dict(n_types=5)), ("n_types < 0", dict(n_types=-1)),
    ("rows[0] above its cap", dict(rows=(C.c_int32 * 3)(6, 7, 2))), ("rows[2] above its cap", dict(rows=(C.c_int32 * 3)(5, 7, 3))),
    ("rows[1] < 0", dict(rows=(C.c_int32 * 3)(5, -1, 2))),
    ("max_count < 0", dict(max_count=-1)),
    ("count_env missing for a COUNT_ENV type", dict(count_env=None)),
    ("E 0", dict(E=0)), ("T 0", dict(T=0)), ("A 0", dict(A=0)), ("a type outside the row", dict(D=36)),
])
def test_gather_argument_errors_come_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _gather_args(capi)
    a.update(change)
    assert _gather(lib, a) == ERR_ARG, what
    assert lib.dynenv_last_error()


GOOD = dict(n_types=3, T=2, P=5, max_count=4, F=8)


def _pad_args():
    keep = [_fake() for _ in range(5)]
    ptrs = (C.c_void_p * 4)(keep[2][1], None, keep[3][1], None)   # (a NULL entry is legal: zeros / no gradient wanted)
    return keep, dict(GOOD, big=keep[0][1], counts=keep[1][1], rows=(C.c_int32 * 3)(4, 0, 2), per_type=ptrs)


def _pad(lib, which, a):
    if which == "pad":
        return lib.dynenv_arrange_fixed_pad(a["per_type"], a["counts"], a["rows"], a["n_types"], a["T"], a["P"], a["max_count"], a["F"],
                                            a["big"], None)
    return lib.dynenv_arrange_fixed_pad_backward(a["big"], a["counts"], a["rows"], a["n_types"], a["T"], a["P"], a["max_count"], a["F"],
                                                 a["per_type"], None)


def _off(p, by):
    return C.c_void_p(p.value + by)


@pytest.mark.parametrize("which", ["pad", "backward"])
@pytest.mark.parametrize("what, change", [
    ("null padded / grad_padded", dict(big=None)), ("null counts", dict(counts=None)), ("null rows", dict(rows=None)),
    ("null emb / grad_emb", dict(per_type=None)),
    ("n_types 0", dict(n_types=0)), ("n_types 5", dict(n_types=5)), ("n_types < 0", dict(n_types=-1)),
    ("rows[2] < 0", dict(rows=(C.c_int32 * 3)(4, 0, -2))),
    ("T 0", dict(T=0)), ("P 0", dict(P=0)), ("max_count < 0", dict(max_count=-1)),
    ("F 0", dict(F=0)), ("F 2", dict(F=2)), ("F 6", dict(F=6)), ("F 13", dict(F=13)), ("F < 0", dict(F=-4)),
    ("T above the grid's y limit", dict(T=65536)),
    ("P * F / 4 at 2^31", dict(P=2 ** 30, F=8, T=1)),
    ("T * P above 2^30 (a player's index is an int)", dict(T=2048, P=2 ** 20, F=4)),
    ("padded / grad_padded 4 bytes off", "big+4"), ("padded / grad_padded 8 bytes off", "big+8"),
    ("a per-type buffer 4 bytes off", "per_type+4"), ("a per-type buffer 12 bytes off", "per_type+12"),
])
def test_pad_argument_errors_come_before_the_device(capi, which, what, change):
    lib = capi.load()
    keep, a = _pad_args()
    if isinstance(change, dict):
        a.update(change)
    elif change.startswith("big+"):
        a["big"] = _off(a["big"], int(change[4:]))
    else:
        a["per_type"] = (C.c_void_p * 4)(keep[2][1], None, _off(keep[3][1], int(change[9:])), None)
    assert _pad(lib, which, a) == ERR_ARG, what
    assert lib.dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    lib = capi.load()
    keep, a = _gather_args(capi)
    assert _gather(lib, a) == capi.ERR_NO_DEVICE
    a.update(max_count=0, mask=None, dropped=None, inputs=None, rows=(C.c_int32 * 3)(0, 0, 0))   # (every optional output left out)
    assert _gather(lib, a) == capi.ERR_NO_DEVICE
    keep, a = _pad_args()
    for which in ("pad", "backward"):
        assert _pad(lib, which, a) == capi.ERR_NO_DEVICE
        assert _pad(lib, which, dict(a, max_count=0)) == capi.ERR_NO_DEVICE
