"""CPU-side checks of the entry point of the fused recurrent head (dynenv_recurrent_head): the header declares it and cites the
reference, the binding lists it parameter for parameter, the library exports it, the ABI version stays 3, and every argument error is
DYNENV_ERR_ARG - what the kernel does not take DYNENV_ERR_UNSUPPORTED - before a device is looked for, so that both are the same with
and without a GPU."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_text, header_without_comments

NAME = "dynenv_recurrent_head"
F32, BF16, F16 = 0, 1, 2
FIELDS = ["tr_w", "tr_b", "tr_ln_w", "tr_ln_b", "w_ih", "w_hh", "b_ih", "b_hh", "ln_w", "ln_b"]


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_point_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_recurrent_head(const float* feat_dev, const float* ext_dev, int32_t E, int32_t A, int32_t F, int32_t X, int32_t w_dtype, "
            "const dynenv_rhead_t* w, float slope, float tr_eps, float ln_eps, const uint8_t* reset_env_dev, float* h_dev, float* c_dev, "
            "float* out_dev, void* stream);") in h
    assert ("typedef struct dynenv_rhead { const void *tr_w; const float *tr_b, *tr_ln_w, *tr_ln_b; const void *w_ih, *w_hh; const float *b_ih, *b_hh; "
            "const float *ln_w, *ln_b; } dynenv_rhead_t;") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.DYNENV_ABI_VERSION == 3
    lib = capi.load()
    assert lib.dynenv_abi_version() == 3
    params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % NAME, h).group(1).split(",")]
    restype, argtypes = capi.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == len(params) == 16
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const float*": vp, "float*": vp, "const uint8_t*": vp, "void*": vp, "int32_t": i32, "float": C.c_float,
             "const dynenv_rhead_t*": C.POINTER(capi.Rhead)}
    for p, got in zip(params, argtypes):   # parameter for parameter
        assert kinds[p.rsplit(" ", 1)[0]] is got, p
    assert NAME in capi.EXPORTS and hasattr(lib, NAME), "libdynenv_hip.so does not export " + NAME
    assert getattr(lib, NAME).argtypes == argtypes
    assert [n for n, _ in capi.Rhead._fields_] == FIELDS
    assert C.sizeof(capi.Rhead) == 10 * C.sizeof(C.c_void_p)


def test_header_comments_state_the_contract_and_cite_the_reference():
    c = comment_before(NAME)
    for word in ("DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "exactly once", "X == 0", "16-byte aligned", "capturable",
                 "64 or 128", "X > 32", "+0.0", "WITHOUT", "IN PLACE", "fixed order", "float32", "models.py:611-612", "models.py:45", "p / A",
                 "never rounded", "read completely before", "reset_env_dev[p / A]", "2^30", "dynenv_reset_masked", "same bits", "not finite"):
        assert word in c, word
    shared = re.sub(r"\s+", " ", header_text().split("typedef struct dynenv_rhead")[0].rsplit("/*", 1)[1])
    assert "models.py:16-95" in shared and "models.py:584-594, 610-616" in shared and "LSTMCell" in shared and "TransformNet" in shared


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


def _args(capi):
    keep = [_fake() for _ in range(7)]
    w = keep[6][1].value
    return keep, dict(feat=keep[0][1], ext=keep[1][1], E=5, A=3, F=128, X=6, dtype=BF16, w=capi.Rhead(*[w] * 10), slope=0.1, tr_eps=1e-5, ln_eps=1e-5,
                      reset=keep[2][1], h=keep[3][1], c=keep[4][1], out=keep[5][1])


def _call(lib, a):
    return lib.dynenv_recurrent_head(a["feat"], a["ext"], a["E"], a["A"], a["F"], a["X"], a["dtype"], None if a["w"] is None else C.byref(a["w"]),
                                     a["slope"], a["tr_eps"], a["ln_eps"], a["reset"], a["h"], a["c"], a["out"], None)


CHANGES = [("null " + k, {k: None}) for k in ("feat", "w", "h", "c", "out")] + \
          [("ext NULL with X > 0", dict(ext=None)), ("ext given with X == 0", dict(X=0))] + \
          [("w without " + f, ("w", f, None)) for f in FIELDS] + \
          [("E 0", dict(E=0)), ("E < 0", dict(E=-1)), ("A 0", dict(A=0)), ("A < 0", dict(A=-3)), ("F 0", dict(F=0)), ("F < 0", dict(F=-64)),
           ("X < 0", dict(X=-1)), ("dtype 3", dict(dtype=3)), ("dtype -1", dict(dtype=-1)), ("E * A above 2^30", dict(E=2 ** 20, A=2 ** 11)),
           ("feat 8 bytes off", "feat+8"), ("feat 4 bytes off", "feat+4"), ("h 4 bytes off", "h+4"), ("h 8 bytes off", "h+8"), ("c 4 bytes off", "c+4"),
           ("out 8 bytes off", "out+8"), ("out 4 bytes off", "out+4")] + \
          [("w %s %d bytes off" % (f, off), ("w", f, off)) for f, off in zip(FIELDS, (2, 4, 8, 4, 8, 2, 4, 8, 4, 8))]


def _apply(a, change):
    if isinstance(change, dict):
        a.update(change)
    elif isinstance(change, tuple):
        which, field, off = change
        setattr(a[which], field, None if off is None else getattr(a[which], field) + off)
    else:
        key, off = change.split("+")
        a[key] = C.c_void_p(a[key].value + int(off))


@pytest.mark.parametrize("what, change", CHANGES, ids=[c[0] for c in CHANGES])
def test_argument_errors_come_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _args(capi)
    _apply(a, change)
    assert _call(lib, a) == ERR_ARG, what
    assert lib.dynenv_last_error()
    for unsupported in (dict(F=48), dict(dtype=F32), dict(X=33)):   # an argument error comes before an unsupported case
        if not set(unsupported) & set(change if isinstance(change, dict) else ()):
            assert _call(lib, dict(a, **unsupported)) == ERR_ARG, (what, unsupported)


UNSUPPORTED = [("float32 operands", dict(dtype=F32)), ("F 48", dict(F=48)), ("F 32", dict(F=32)), ("F 256", dict(F=256)), ("F 96", dict(F=96)),
               ("F 1", dict(F=1)), ("X 33", dict(X=33)), ("X 4096", dict(X=4096))]


@pytest.mark.parametrize("what, change", UNSUPPORTED, ids=[c[0] for c in UNSUPPORTED])
def test_unsupported_cases_are_refused_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _args(capi)
    a.update(change)
    assert _call(lib, a) == capi.ERR_UNSUPPORTED, what
    assert b"the fused layer takes" in lib.dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    lib = capi.load()
    keep, a = _args(capi)
    for F in (64, 128):
        for dtype in (BF16, F16):
            for X in (1, 6, 13, 32):
                assert _call(lib, dict(a, F=F, dtype=dtype, X=X)) == capi.ERR_NO_DEVICE, (F, dtype, X)
            assert _call(lib, dict(a, F=F, dtype=dtype, X=0, ext=None)) == capi.ERR_NO_DEVICE
    assert _call(lib, dict(a, reset=None)) == capi.ERR_NO_DEVICE, "the mask is optional"
    w = capi.Rhead(*[a["w"].w_ih] * 10)
    w.tr_w = w.tr_b = w.tr_ln_w = w.tr_ln_b = None
    assert _call(lib, dict(a, X=0, ext=None, w=w)) == capi.ERR_NO_DEVICE, "X == 0 ignores w->tr_*, which may be NULL"
    w.tr_w = a["w"].w_ih + 2
    assert _call(lib, dict(a, X=0, ext=None, w=w)) == capi.ERR_NO_DEVICE, "... or anything else"
