"""CPU-side checks of the entry point of the fused embed-and-pad (dynenv_arrange_embed_pad): the header declares it and cites the
reference, the binding lists it parameter for parameter, the library exports it, the ABI version stays 3, and every argument error is
DYNENV_ERR_ARG - what the kernels do not take DYNENV_ERR_UNSUPPORTED - before a device is looked for, so that both are the same with
and without a GPU."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_text, header_without_comments

NAME = "dynenv_arrange_embed_pad"
F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_point_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_arrange_embed_pad(const float* obs_dev, int32_t E, int32_t T, int32_t A, int32_t D, const dynenv_arr_type_t* types, "
            "int32_t n_types, const int32_t* counts_dev, int32_t max_count, const dynenv_embed_block_t* blocks, int32_t F, float slope, "
            "float eps, void* padded_dev, int32_t padded_dtype, void* stream);") in h
    assert ("typedef struct dynenv_embed_block { const float *w1; const float *ln1_w, *ln1_b; const float *w2; const float *ln2_w, *ln2_b; } "
            "dynenv_embed_block_t;") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.DYNENV_ABI_VERSION == 3
    lib = capi.load()
    assert lib.dynenv_abi_version() == 3
    params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % NAME, h).group(1).split(",")]
    restype, argtypes = capi.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == len(params) == 16
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const float*": vp, "const int32_t*": vp, "void*": vp, "int32_t": i32, "float": C.c_float,
             "const dynenv_arr_type_t*": C.POINTER(capi.ArrType), "const dynenv_embed_block_t*": C.POINTER(capi.EmbedBlock)}
    for p, got in zip(params, argtypes):   # parameter for parameter
        assert kinds[p.rsplit(" ", 1)[0]] is got, p
    assert hasattr(lib, NAME), "libdynenv_hip.so does not export " + NAME
    assert getattr(lib, NAME).argtypes == argtypes
    assert [n for n, _ in capi.EmbedBlock._fields_] == ["w1", "ln1_w", "ln1_b", "w2", "ln2_w", "ln2_b"]
    assert C.sizeof(capi.EmbedBlock) == 6 * C.sizeof(C.c_void_p)


def test_header_comments_state_the_contract_and_cite_the_reference():
    c = comment_before(NAME)
    for word in ("DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "exactly once", "max_count == 0", "16-byte aligned", "capturable",
                 "64 or 128", "above 16", "+0.0", "dynenv_arrange_plan", "dynenv_arrange_fixed_gather", "fixed order"):
        assert word in c, word
    shared = re.sub(r"\s+", " ", header_text().split("typedef struct dynenv_embed_block")[0].rsplit("/*", 1)[1])
    assert "models.py:99-124" in shared and "models.py:278-307" in shared and "biased variance" in shared


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


def _args(capi):
    keep = [_fake() for _ in range(4)]
    w = keep[3][1].value
    types = (capi.ArrType * 3)(capi.ArrType(1, 7, 3, 0, 2, 0, 0, 0), capi.ArrType(22, 4, 2, 1, 0, 1, 3, 0), capi.ArrType(30, 2, 4, 2, 0, 38, 0, 0))
    blocks = (capi.EmbedBlock * 3)(capi.EmbedBlock(w, w, w, w, w, w), capi.EmbedBlock(), capi.EmbedBlock(w, w, w, w, w, w))   # (an all-NULL block is legal)
    return keep, dict(obs=keep[0][1], E=3, T=2, A=2, D=41, types=types, n_types=3, counts=keep[1][1], max_count=9, blocks=blocks, F=128,
                      slope=0.1, eps=1e-5, padded=keep[2][1], dtype=F32)


def _call(lib, a):
    return lib.dynenv_arrange_embed_pad(a["obs"], a["E"], a["T"], a["A"], a["D"], a["types"], a["n_types"], a["counts"], a["max_count"], a["blocks"],
                                        a["F"], a["slope"], a["eps"], a["padded"], a["dtype"], None)


def _types(capi, i, **kw):
    def change(a):
        t = a["types"][i]
        for k, v in kw.items():
            setattr(t, k, v)
    return change


def _partial_block(capi):
    def change(a):
        a["blocks"][2].ln2_b = None
    return change


CHANGES = [
    ("null obs", dict(obs=None)), ("null types", dict(types=None)), ("null counts", dict(counts=None)), ("null blocks", dict(blocks=None)),
    ("null padded", dict(padded=None)),
    ("n_types 0", dict(n_types=0)), ("n_types 5", dict(n_types=5)), ("n_types < 0", dict(n_types=-1)),
    ("E 0", dict(E=0)), ("T 0", dict(T=0)), ("A 0", dict(A=0)), ("D 0", dict(D=0)), ("E * T * A above 2^30", dict(E=2 ** 20, T=2 ** 10, A=2)),
    ("a type outside the row", dict(D=37)), ("a type at a negative offset", (0, dict(offset=-1))), ("a type of no features", (1, dict(feat=0))),
    ("a type of negative capacity", (1, dict(cap=-1))), ("a count index outside the row", (2, dict(count_index=41))),
    ("an unknown count mode", (0, dict(count_mode=3))),
    ("dtype 3", dict(dtype=3)), ("dtype -1", dict(dtype=-1)), ("max_count < 0", dict(max_count=-1)),
    ("padded 4 bytes off", "padded+4"), ("padded 8 bytes off", "padded+8"), ("padded 2 bytes off", "padded+2"),
    ("T * max_count * P at 2^31", dict(E=2 ** 14, T=2 ** 4, A=2 ** 4, max_count=2 ** 9)),
    ("max_count at 2^23", dict(E=1, T=1, A=1, max_count=2 ** 23)),
    ("a block with five of its six pointers", "partial block"),
]


@pytest.mark.parametrize("what, change", CHANGES, ids=[c[0] for c in CHANGES])
def test_argument_errors_come_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _args(capi)
    if isinstance(change, dict):
        a.update(change)
    elif isinstance(change, tuple):
        _types(capi, change[0], **change[1])(a)
    elif change == "partial block":
        _partial_block(capi)(a)
    else:
        a["padded"] = C.c_void_p(a["padded"].value + int(change[7:]))
    assert _call(lib, a) == ERR_ARG, what
    assert lib.dynenv_last_error()
    a["F"] = 48   # an argument error comes before an unsupported width
    assert _call(lib, a) == ERR_ARG, what


@pytest.mark.parametrize("what, change", [("F 48", dict(F=48)), ("F 32", dict(F=32)), ("F 256", dict(F=256)), ("F 0", dict(F=0)), ("F < 0", dict(F=-64)),
                                          ("F 96", dict(F=96)), ("a type of 17 features", "feat 17")])
def test_unsupported_widths_are_refused_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _args(capi)
    if isinstance(change, dict):
        a.update(change)
    else:   # 17 features x 1 row still lies inside the observation row
        _types(capi, 0, feat=17, cap=1)(a)
    assert _call(lib, a) == capi.ERR_UNSUPPORTED, what
    assert b"fused embedding takes" in lib.dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    lib = capi.load()
    keep, a = _args(capi)
    for F in (64, 128):
        for dtype in (F32, BF16, F16):
            b = dict(a, F=F, dtype=dtype)
            assert _call(lib, b) == capi.ERR_NO_DEVICE, (F, dtype)
            assert _call(lib, dict(b, max_count=0)) == capi.ERR_NO_DEVICE, (F, dtype)
