"""CPU-side checks of the entry point of the fused attention (dynenv_attend_pool): the header declares it and cites the reference, the
binding lists it parameter for parameter, the library exports it, the ABI version stays 3, and every argument error is DYNENV_ERR_ARG -
what the kernel does not take DYNENV_ERR_UNSUPPORTED - before a device is looked for, so that both are the same with and without a GPU."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_text, header_without_comments

NAME = "dynenv_attend_pool"
F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_point_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_attend_pool(const void* padded_dev, int32_t padded_dtype, const int32_t* obj_counts_dev, int32_t T, int32_t M, int32_t P, "
            "int32_t F, const dynenv_mha_t* obj_att, const dynenv_mha_t* temp_att, const float* ln_w_dev, const float* ln_b_dev, float ln_eps, "
            "const float* conf_w_dev, const float* conf_b_dev, float* out_dev, void* stream);") in h
    assert ("typedef struct dynenv_mha { const void *in_w; const void *out_w; const void *bias_k, *bias_v; const float *in_b; const float *out_b; } "
            "dynenv_mha_t;") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.DYNENV_ABI_VERSION == 3
    lib = capi.load()
    assert lib.dynenv_abi_version() == 3
    params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % NAME, h).group(1).split(",")]
    restype, argtypes = capi.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == len(params) == 16
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const void*": vp, "const float*": vp, "float*": vp, "const int32_t*": vp, "void*": vp, "int32_t": i32, "float": C.c_float,
             "const dynenv_mha_t*": C.POINTER(capi.Mha)}
    for p, got in zip(params, argtypes):   # parameter for parameter
        assert kinds[p.rsplit(" ", 1)[0]] is got, p
    assert NAME in capi.EXPORTS and hasattr(lib, NAME), "libdynenv_hip.so does not export " + NAME
    assert getattr(lib, NAME).argtypes == argtypes
    assert [n for n, _ in capi.Mha._fields_] == ["in_w", "out_w", "bias_k", "bias_v", "in_b", "out_b"]
    assert C.sizeof(capi.Mha) == 6 * C.sizeof(C.c_void_p)


def test_header_comments_state_the_contract_and_cite_the_reference():
    c = comment_before(NAME)
    for word in ("DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "exactly once", "M == 0", "16-byte aligned", "capturable",
                 "64 or 128", "M > 128", "+0.0", "WITHOUT", "prefixes", "fixed order", "float32", "models.py:362-363", "models.py:376-377",
                 "never masked", "max_t c_t", "not finite"):
        assert word in c, word
    shared = re.sub(r"\s+", " ", header_text().split("typedef struct dynenv_mha")[0].rsplit("/*", 1)[1])
    assert "models.py:311-386" in shared and "RecurrentTemporalAttention" in shared and "add_bias_kv=True" in shared


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


def _args(capi):
    keep = [_fake() for _ in range(4)]
    w = keep[3][1].value
    return keep, dict(padded=keep[0][1], dtype=BF16, counts=keep[1][1], T=3, M=40, P=6, F=128, obj=capi.Mha(w, w, w, w, w, w),
                      tmp=capi.Mha(w, w, w, w, w, w), ln_w=C.c_void_p(w), ln_b=C.c_void_p(w), eps=1e-5, conf_w=C.c_void_p(w), conf_b=C.c_void_p(w),
                      out=keep[2][1])


def _call(lib, a):
    ref = lambda m: None if m is None else C.byref(m)  # noqa: E731
    return lib.dynenv_attend_pool(a["padded"], a["dtype"], a["counts"], a["T"], a["M"], a["P"], a["F"], ref(a["obj"]), ref(a["tmp"]), a["ln_w"], a["ln_b"],
                                  a["eps"], a["conf_w"], a["conf_b"], a["out"], None)


MHA_FIELDS = ["in_w", "out_w", "bias_k", "bias_v", "in_b", "out_b"]
CHANGES = [("null " + k, {k: None}) for k in ("padded", "counts", "obj", "tmp", "ln_w", "ln_b", "conf_w", "conf_b", "out")] + \
          [("objAtt without " + f, ("obj", f, None)) for f in MHA_FIELDS] + [("tempAtt without " + f, ("tmp", f, None)) for f in MHA_FIELDS] + \
          [("T 0", dict(T=0)), ("T < 0", dict(T=-1)), ("P 0", dict(P=0)), ("F 0", dict(F=0)), ("F < 0", dict(F=-64)), ("M < 0", dict(M=-1)),
           ("dtype 3", dict(dtype=3)), ("dtype -1", dict(dtype=-1)), ("T * P above 2^30", dict(T=2 ** 11, P=2 ** 20)),
           ("padded 8 bytes off", "padded+8"), ("padded 2 bytes off", "padded+2"), ("out 4 bytes off", "out+4"), ("out 8 bytes off", "out+8"),
           ("ln_w 4 bytes off", "ln_w+4"), ("conf_w 8 bytes off", "conf_w+8"),
           ("objAtt in_w 8 bytes off", ("obj", "in_w", 8)), ("tempAtt out_w 2 bytes off", ("tmp", "out_w", 2)), ("objAtt in_b 4 bytes off", ("obj", "in_b", 4)),
           ("tempAtt bias_k 2 bytes off", ("tmp", "bias_k", 2)), ("objAtt bias_v 4 bytes off", ("obj", "bias_v", 4))]


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
    for unsupported in (dict(F=48), dict(dtype=F32), dict(M=129)):   # an argument error comes before an unsupported case
        if not set(unsupported) & set(change if isinstance(change, dict) else ()):
            assert _call(lib, dict(a, **unsupported)) == ERR_ARG, (what, unsupported)


UNSUPPORTED = [("a float32 padded tensor", dict(dtype=F32)), ("F 48", dict(F=48)), ("F 32", dict(F=32)), ("F 256", dict(F=256)), ("F 96", dict(F=96)),
               ("F 1", dict(F=1)), ("M 129", dict(M=129)), ("M 4096", dict(M=4096))]


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
            for M in (0, 1, 32, 33, 64, 65, 128):
                assert _call(lib, dict(a, F=F, dtype=dtype, M=M)) == capi.ERR_NO_DEVICE, (F, dtype, M)
    assert _call(lib, dict(a, M=0, padded=None)) == capi.ERR_NO_DEVICE, "without slots there is no padded tensor to read"
