"""CPU-side checks of the curiosity module's entry point (dynenv_icm_losses): the header declares it and cites the reference, the binding
lists it parameter for parameter, the library exports it, the ABI version stays 3, and every argument error is DYNENV_ERR_ARG - what the
kernel does not take DYNENV_ERR_UNSUPPORTED - before a device is looked for, so that both are the same with and without a GPU."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, header_text, header_without_comments

NAME = "dynenv_icm_losses"
ORDER = ["features", "actions", "finished", "T", "P", "K", "AD", "nvec", "G", "dtype", "w", "slope", "curiosity", "ce", "losses", "status"]
W_FIELDS = ["fwd_w1", "fwd_w1_act", "fwd_b1", "fwd_w2", "fwd_b2", "inv_w", "inv_b"]


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_point_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_icm_losses(const float* features_dev, const float* actions_dev, const uint8_t* finished_dev, int32_t T, int32_t P, int32_t K, "
            "int32_t action_cols, const int32_t* nvec, int32_t G, int32_t w_dtype, const dynenv_icm_t* w, float slope, float* curiosity_dev, "
            "float* inverse_ce_dev, float* losses_dev, int32_t* status_dev, void* stream);") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.load().dynenv_abi_version() == capi.DYNENV_ABI_VERSION == 3
    struct = re.search(r"typedef struct dynenv_icm \{(.*?)\} dynenv_icm_t;", h).group(1)
    assert re.findall(r"\*(\w+);", struct) == W_FIELDS == [n for n, _ in capi.Icm._fields_]
    assert all(t is C.c_void_p for _, t in capi.Icm._fields_) and C.sizeof(capi.Icm) == 8 * len(W_FIELDS)
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const float*": vp, "float*": vp, "const uint8_t*": vp, "int32_t*": vp, "void*": vp, "const int32_t*": C.POINTER(i32),
             "const dynenv_icm_t*": C.POINTER(capi.Icm), "int32_t": i32, "float": C.c_float}
    params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % NAME, h).group(1).split(",")]
    restype, argtypes = capi.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == len(params) == 17
    for p, got in zip(params, argtypes):   # parameter for parameter
        assert kinds[p.rsplit(" ", 1)[0]] is got, p
    lib = capi.load()
    assert NAME in capi.EXPORTS and hasattr(lib, NAME) and getattr(lib, NAME).argtypes == argtypes
    hidden = {k: int(re.search(r"#define DYNENV_ICM_%s (\d+)" % k, h).group(1)) for k in ("HIDDEN", "HIDDEN_PAD")}
    from dynenv_amd import icm, policy
    assert hidden == {"HIDDEN": icm.HIDDEN, "HIDDEN_PAD": icm.HIDDEN_PAD} == {"HIDDEN": 140, "HIDDEN_PAD": 160} and icm.HIDDEN_PAD % 32 == 0
    assert (icm.MAX_ROWS, icm.MAX_GROUPS, icm.MAX_GROUP, icm.MAX_COLS) == (policy.MAX_ROWS, policy.MAX_GROUPS, policy.MAX_GROUP, policy.MAX_COLS)


def test_header_comment_states_the_contract_and_cites_the_reference():
    txt = header_text()
    at = re.search(r"^\s*int\s*%s\(" % NAME, txt, flags=re.M).start()
    c = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", txt[:at].rsplit("/*", 1)[1]))   # (without the " * " that begins its lines)
    for word in ("DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "exactly once", "capturable", "read at replay", "two launches",
                 "[T+1][P][K]", "[T][AD][P]", "[T][G][P]", "NULL: nobody finished", "0..G-1", "clamped", "bit 0", "IndexError", "in group order",
                 "logsumexp(l_g) - l_g[a_g]", "max-subtracted", "finished rows included", "accumulates in double", "rounds once", "+0 where n == 0",
                 "icm.py:80-86", "icm.py:91, 98-100", "16-byte aligned", "(T + 1) * P > 2^30", "64, 128 or 256", "same bits", "alone", "N > 32"):
        assert word in c, word
    shared =re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", txt[:txt.index("#define DYNENV_ICM_HIDDEN ")].rsplit("/*", 1)[1]))
    for word in ("DynEnv/models/icm.py", "icm.py:112-146", "icm.py:167-179", "icm.py:77-109", "H = 140", "H' = 160", "+0"):
        assert word in shared, word


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


def _args(capi):
    keep = {k: _fake() for k in ["features", "actions", "finished", "curiosity", "ce", "losses", "status"] + W_FIELDS}
    a = {k: v[1] for k, v in keep.items()}
    a.update(T=6, P=40, K=128, AD=4, nvec=[5, 3, 3], G=3, dtype=1, slope=0.1)
    return keep, a


def _call(capi, a):
    w = capi.Icm()
    for k in W_FIELDS:
        setattr(w, k, a[k].value if a[k] is not None else None)
    nvec = None if a["nvec"] is None else (C.c_int32 * max(len(a["nvec"]), 1))(*a["nvec"])
    vals = dict(a, nvec=nvec, w=None if a.get("no_w") else C.byref(w))
    return capi.load().dynenv_icm_losses(*[vals[k] for k in ORDER], None)


def _apply(a, change):
    if isinstance(change, dict):
        a.update(change)
    else:
        key, off = change.split("+")
        a[key] = C.c_void_p(a[key].value + int(off))


CHANGES = [("null " + k, {k: None}) for k in ("features", "actions", "nvec", "curiosity", "ce")] + [("null w", dict(no_w=True))] + \
          [("null w." + k, {k: None}) for k in W_FIELDS] + \
          [("%s %d" % (k, v), {k: v}) for k in ("T", "P", "K") for v in (0, -1)] + \
          [("G 0", dict(G=0, nvec=[])), ("G 9", dict(G=9, AD=8, nvec=[2] * 9)), ("a group of 0", dict(nvec=[5, 0, 3])), ("a group of 17", dict(nvec=[5, 17, 3])),
           ("N 33", dict(nvec=[16, 16, 1])), ("AD below G", dict(AD=2)), ("AD 9", dict(AD=9)), ("dtype -1", dict(dtype=-1)), ("dtype 3", dict(dtype=3)),
           ("(T + 1) * P above 2^30", dict(T=2 ** 10, P=2 ** 20))] + \
          [("%s %d bytes off" % (k, off), "%s+%d" % (k, off)) for k in ["features", "actions", "finished", "curiosity", "ce"] + W_FIELDS for off in (4, 8)] + \
          [("%s 2 bytes off" % k, k + "+2") for k in ("losses", "status")]


@pytest.mark.parametrize("what, change", CHANGES, ids=[c[0] for c in CHANGES])
def test_argument_errors_come_before_the_device(capi, what, change):
    keep, a = _args(capi)
    _apply(a, change)
    assert _call(capi, a) == ERR_ARG, what
    assert b"icm losses" in capi.load().dynenv_last_error()
    for unsupported in (dict(K=96), dict(dtype=0)):   # an argument error comes before an unsupported case
        if not set(unsupported) & set(change if isinstance(change, dict) else ()):
            assert _call(capi, dict(a, **unsupported)) == ERR_ARG, (what, unsupported)


UNSUPPORTED = [("float32 operands", dict(dtype=0)), ("K 96", dict(K=96)), ("K 32", dict(K=32)), ("K 512", dict(K=512)), ("K 1", dict(K=1))]


@pytest.mark.parametrize("what, change", UNSUPPORTED, ids=[c[0] for c in UNSUPPORTED])
def test_unsupported_shapes_are_refused_before_the_device(capi, what, change):
    keep, a = _args(capi)
    a.update(change)
    assert _call(capi, a) == capi.ERR_UNSUPPORTED, what
    assert b"the fused layer takes" in capi.load().dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    keep, a = _args(capi)
    assert _call(capi, a) == capi.ERR_NO_DEVICE
    for change in (dict(finished=None), dict(losses=None), dict(status=None), dict(finished=None, losses=None, status=None), dict(dtype=2), dict(K=64),
                   dict(K=256), dict(G=8, AD=8, nvec=[4] * 8), dict(G=2, AD=2, nvec=[16, 16]), dict(G=1, AD=1, nvec=[1]), dict(T=1, P=1),
                   dict(T=2 ** 10 - 1, P=2 ** 20), dict(AD=8)):
        assert _call(capi, dict(a, **change)) == capi.ERR_NO_DEVICE, change
