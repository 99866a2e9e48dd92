"""CPU-side checks of the entry points of the 16-bit padded tensor (dynenv_arrange_pad_as / _pad_backward_as / _fixed_pad_as /
_fixed_pad_backward_as): the header declares them, the library exports them and the binding lists them with as many parameters; the ABI
version stays; every argument error is DYNENV_ERR_ARG and an unsupported dtype pair DYNENV_ERR_UNSUPPORTED before a device is looked
for, so that both are the same with and without a GPU."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_without_comments

NAMES = ("dynenv_arrange_pad_as", "dynenv_arrange_pad_backward_as", "dynenv_arrange_fixed_pad_as", "dynenv_arrange_fixed_pad_backward_as")
F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_points_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_arrange_pad_as(const void* const* emb_dev, int32_t emb_dtype, const int32_t* counts_dev, const int32_t* base_dev, "
            "int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* padded_dev, int32_t padded_dtype, void* stream);") in h
    assert ("int dynenv_arrange_pad_backward_as(const void* grad_padded_dev, int32_t padded_dtype, const int32_t* counts_dev, "
            "const int32_t* base_dev, int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* const* grad_emb_dev, "
            "int32_t emb_dtype, void* stream);") in h
    assert ("int dynenv_arrange_fixed_pad_as(const void* const* emb_dev, int32_t emb_dtype, const int32_t* counts_dev, const int32_t* rows, "
            "int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* padded_dev, int32_t padded_dtype, void* stream);") in h
    assert ("int dynenv_arrange_fixed_pad_backward_as(const void* grad_padded_dev, int32_t padded_dtype, const int32_t* counts_dev, "
            "const int32_t* rows, int32_t n_types, int32_t T, int32_t P, int32_t max_count, int32_t F, void* const* grad_emb_dev, "
            "int32_t emb_dtype, void* stream);") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert "#define DYNENV_ARR_F32 0" in h and "#define DYNENV_ARR_BF16 1" in h and "#define DYNENV_ARR_F16 2" in h
    assert (capi.ARR_F32, capi.ARR_BF16, capi.ARR_F16) == (F32, BF16, F16) and capi.DYNENV_ABI_VERSION == 3
    lib = capi.load()
    assert lib.dynenv_abi_version() == 3
    for name in NAMES:
        params = re.search(r"int %s ?\(([^()]*)\) ?;" % name, h).group(1)
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == params.count(",") + 1 == 12, name
        assert hasattr(lib, name), "libdynenv_hip.so does not export " + name
        assert getattr(lib, name).argtypes == argtypes


def test_header_comments_state_the_contract_and_cite_the_reference():
    for name in NAMES:
        c = comment_before(name)
        assert ":147-180" in c and "DYNENV_ERR_ARG" in c and "DYNENV_ERR_UNSUPPORTED" in c and "before a device" in c, name
    assert "models.py:252-274" in comment_before("dynenv_arrange_pad_as") and "models.py:252-274" in comment_before("dynenv_arrange_fixed_pad_as")
    for name in NAMES[1::2]:
        c = comment_before(name)
        assert "exactly once" in c and "never read" in c and "stepped over" in c, name
    from host_common import header_text   # the comment the four share stands in front of the dtype constants
    shared = re.sub(r"\s+", " ", header_text().split("#define DYNENV_ARR_F32")[0].rsplit("/*", 1)[1])
    for word in ("round to nearest, ties to even", "overflow to infinity", "subnormal", "signed zero", "NaN stays a NaN", "exact for every bit pattern",
                 "multiple of 8", "16-byte aligned", "DYNENV_ERR_UNSUPPORTED", "max_count == 0"):
        assert word in shared, word


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


GOOD = dict(n_types=3, T=2, P=5, max_count=4, F=16, emb=F32, padded=BF16)


def _args():
    keep = [_fake() for _ in range(6)]
    ptrs = (C.c_void_p * 4)(keep[2][1], None, keep[3][1], None)   # (a NULL entry is legal: zeros / no gradient wanted)
    return keep, dict(GOOD, big=keep[0][1], counts=keep[1][1], base=keep[4][1], rows=(C.c_int32 * 3)(4, 0, 2), per_type=ptrs)


def _call(lib, which, a):
    if which == "pad":
        return lib.dynenv_arrange_pad_as(a["per_type"], a["emb"], a["counts"], a["base"], a["n_types"], a["T"], a["P"], a["max_count"], a["F"],
                                         a["big"], a["padded"], None)
    if which == "backward":
        return lib.dynenv_arrange_pad_backward_as(a["big"], a["padded"], a["counts"], a["base"], a["n_types"], a["T"], a["P"], a["max_count"],
                                                  a["F"], a["per_type"], a["emb"], None)
    if which == "fixed pad":
        return lib.dynenv_arrange_fixed_pad_as(a["per_type"], a["emb"], a["counts"], a["rows"], a["n_types"], a["T"], a["P"], a["max_count"],
                                               a["F"], a["big"], a["padded"], None)
    return lib.dynenv_arrange_fixed_pad_backward_as(a["big"], a["padded"], a["counts"], a["rows"], a["n_types"], a["T"], a["P"], a["max_count"],
                                                    a["F"], a["per_type"], a["emb"], None)


WHICH = ["pad", "backward", "fixed pad", "fixed backward"]


def _off(p, by):
    return C.c_void_p(p.value + by)


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("what, change", [
    ("null padded / grad_padded", dict(big=None)), ("null counts", dict(counts=None)), ("null base / rows", dict(base=None, rows=None)),
    ("null emb / grad_emb", dict(per_type=None)),
    ("n_types 0", dict(n_types=0)), ("n_types 5", dict(n_types=5)), ("n_types < 0", dict(n_types=-1)),
    ("T 0", dict(T=0)), ("P 0", dict(P=0)), ("max_count < 0", dict(max_count=-1)),
    ("emb_dtype 3", dict(emb=3)), ("emb_dtype -1", dict(emb=-1)), ("padded_dtype 3", dict(padded=3)), ("padded_dtype -1", dict(padded=-1)),
    ("F 0", dict(F=0)), ("F 4 (a float32 unit, not a 16-bit one)", dict(F=4)), ("F 12", dict(F=12)), ("F 20", dict(F=20)), ("F 13", dict(F=13)),
    ("F < 0", dict(F=-8)), ("F 4 into fp16", dict(F=4, padded=F16)), ("F 12, bf16 into bf16", dict(F=12, emb=BF16)),
    ("F 6 into float32", dict(F=6, padded=F32)), ("F 2 into float32", dict(F=2, padded=F32)),
    ("T above the grid's y limit", dict(T=65536)),
    ("P * F / 8 at 2^31", dict(P=2 ** 30, F=16, T=1)),
    ("padded / grad_padded 4 bytes off", "big+4"), ("padded / grad_padded 8 bytes off", "big+8"), ("padded / grad_padded 2 bytes off", "big+2"),
    ("a per-type buffer 4 bytes off", "per_type+4"), ("a per-type buffer 2 bytes off", "per_type+2"), ("a per-type buffer 8 bytes off", "per_type+8"),
    ("a per-type buffer 4 bytes off, float32 into float32", "per_type+4 f32"),
])
def test_argument_errors_come_before_the_device(capi, which, what, change):
    lib = capi.load()
    keep, a = _args()
    if isinstance(change, dict):
        a.update(change)
    elif change.startswith("big+"):
        a["big"] = _off(a["big"], int(change[4:]))
    else:
        a["per_type"] = (C.c_void_p * 4)(keep[2][1], None, _off(keep[3][1], int(change.split()[0][9:])), None)
        if change.endswith("f32"):
            a["padded"] = F32
    assert _call(lib, which, a) == ERR_ARG, what
    assert lib.dynenv_last_error()


@pytest.mark.parametrize("which", ["fixed pad", "fixed backward"])
@pytest.mark.parametrize("what, change", [
    ("rows[2] < 0", dict(rows=(C.c_int32 * 3)(4, 0, -2))), ("rows[0] < 0", dict(rows=(C.c_int32 * 3)(-1, 0, 2))),
    ("T * P above 2^30 (a player's index is an int)", dict(T=2048, P=2 ** 20, F=8)),
])
def test_fixed_mode_argument_errors(capi, which, what, change):
    lib = capi.load()
    keep, a = _args()
    a.update(change)
    assert _call(lib, which, a) == ERR_ARG, what
    assert lib.dynenv_last_error()


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("emb, padded", [(BF16, F32), (F16, F32), (BF16, F16), (F16, BF16)])
def test_unsupported_pairs_are_refused_before_the_device(capi, which, emb, padded):
    lib = capi.load()
    keep, a = _args()
    a.update(emb=emb, padded=padded)
    assert _call(lib, which, a) == capi.ERR_UNSUPPORTED
    assert b"float32 or of the padded tensor's own dtype" in lib.dynenv_last_error()
    a.update(F=12)   # an argument error comes first
    assert _call(lib, which, a) == (ERR_ARG if padded != F32 else capi.ERR_UNSUPPORTED)


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    lib = capi.load()
    keep, a = _args()
    for which in WHICH:
        for emb, padded, F in ((F32, BF16, 16), (F32, F16, 8), (BF16, BF16, 16), (F16, F16, 24), (F32, F32, 4), (F32, F32, 16)):
            b = dict(a, emb=emb, padded=padded, F=F)
            assert _call(lib, which, b) == capi.ERR_NO_DEVICE, (which, emb, padded)
            assert _call(lib, which, dict(b, max_count=0)) == capi.ERR_NO_DEVICE, (which, emb, padded)
