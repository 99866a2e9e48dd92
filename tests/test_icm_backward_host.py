"""CPU-side checks of the curiosity module's backward entry points (dynenv_icm_backward, dynenv_icm_backward_workspace): the header
declares them and the two structs and cites the reference, the binding lists them parameter for parameter, the library exports them, the
ABI version stays 3, every argument error is DYNENV_ERR_ARG - what the kernel does not take DYNENV_ERR_UNSUPPORTED - before a device is
looked for, and the workspace query is monotone in K and honours the bound the header states."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, header_text, header_without_comments

NAME, QUERY = "dynenv_icm_backward", "dynenv_icm_backward_workspace"
ORDER = ["features", "actions", "finished", "T", "P", "K", "AD", "nvec", "G", "dtype", "w", "slope", "count", "upstream", "wt", "grad", "d_features",
         "workspace", "workspace_bytes", "status"]
W_FIELDS = ["fwd_w1", "fwd_w1_act", "fwd_b1", "fwd_w2", "fwd_b2", "inv_w", "inv_b"]
T_FIELDS = ["fwd_w2_t", "fwd_w1_t", "inv_w_t"]
G_FIELDS = ["d_fwd_w1", "d_fwd_w1_act", "d_fwd_b1", "d_fwd_w2", "d_fwd_b2", "d_inv_w", "d_inv_b"]
MAX_WORKGROUPS, ROWS = 256, 32


def part(K):
    """float32 per workgroup slice (include/dynenv.h)"""
    return 385 * K + 5312


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_points_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_icm_backward(const float* features_dev, const float* actions_dev, const uint8_t* finished_dev, int32_t T, int32_t P, int32_t K, "
            "int32_t action_cols, const int32_t* nvec, int32_t G, int32_t w_dtype, const dynenv_icm_t* w, float slope, const float* count_dev, "
            "const float* upstream_dev, const dynenv_icm_bwd_t* wt, const dynenv_icm_grad_t* grad, float* d_features_dev, void* workspace_dev, "
            "uint64_t workspace_bytes, int32_t* status_dev, void* stream);") in h
    assert "int dynenv_icm_backward_workspace(int32_t P, int32_t K, uint64_t* bytes);" in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.load().dynenv_abi_version() == capi.DYNENV_ABI_VERSION == 3
    assert int(re.search(r"#define DYNENV_ICM_BWD_MAX_WORKGROUPS (\d+)", h).group(1)) == MAX_WORKGROUPS
    for tag, cls, fields in (("dynenv_icm_bwd", capi.IcmBwd, T_FIELDS), ("dynenv_icm_grad", capi.IcmGrad, G_FIELDS)):
        struct = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (tag, tag), h).group(1)
        assert re.findall(r"\*(\w+);", struct) == fields == [n for n, _ in cls._fields_]
        assert all(t is C.c_void_p for _, t in cls._fields_) and C.sizeof(cls) == 8 * len(fields)
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const float*": vp, "float*": vp, "const uint8_t*": vp, "int32_t*": vp, "void*": vp, "const int32_t*": C.POINTER(i32),
             "const dynenv_icm_t*": C.POINTER(capi.Icm), "const dynenv_icm_bwd_t*": C.POINTER(capi.IcmBwd), "const dynenv_icm_grad_t*": C.POINTER(capi.IcmGrad),
             "int32_t": i32, "float": C.c_float, "uint64_t": C.c_uint64, "uint64_t*": C.POINTER(C.c_uint64)}
    lib = capi.load()
    for name, count in ((NAME, 21), (QUERY, 3)):
        params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % name, h).group(1).split(",")]
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params) == count
        for p, got in zip(params, argtypes):   # parameter for parameter
            assert kinds[p.rsplit(" ", 1)[0]] is got, p
        assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes == argtypes
    from dynenv_amd import icm
    assert icm.FUSED_BACKWARD_K == (64, 128) and set(icm.FUSED_BACKWARD_K) < set(icm.FUSED_K)


def test_header_comment_states_the_contract_and_cites_the_reference():
    txt = header_text()
    at = re.search(r"^\s*int\s*%s\(" % NAME, txt, flags=re.M).start()
    c = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", txt[:at].rsplit("/*", 1)[1]))   # (without the " * " that begins its lines)
    for word in ("DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "exactly once", "capturable", "read at replay", "two launches",
                 "[T+1][P][K]", "count_dev is the forward's losses_dev", "element 2", "{ s_f, s_i }", "alpha = 2 s_f / (n K)", "beta = s_i / (n G)",
                 "h_pre == 0 included", "exactly 0 for a group of one action", "nothing is accumulated into", "the padding is zero", "n == 0 every gradient is +0",
                 "no active row touches is +0", "clamped", "bit 0", "ever rounded to 16 bits", "by a power of two", "no floating-point atomic", "same bits",
                 "alone", "in workgroup order", "16-byte aligned", "(T + 1) * P > 2^30", "a workspace that is too small", "64 or 128", "N > 32",
                 "384 float32 per lane"):
        assert word in c, word
    shared = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", txt[:txt.index("typedef struct dynenv_icm_bwd ")].rsplit("/*", 1)[1]))
    for word in ("icm.py:77-109", "icm.py:207-240", "saves NOTHING", "recomputes", "transposed copies"):
        assert word in shared, word
    at = re.search(r"^\s*int\s*%s\(" % QUERY, txt, flags=re.M).start()
    q = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", txt[:at].rsplit("/*", 1)[1]))
    for word in ("host only", "touches no device", "min(ceil(P / 32), 256) * (385 K + 5312) * 4", "whatever P and T are", "30 670 848", "55 902 208"):
        assert word in q, word
    struct = txt[txt.index("typedef struct dynenv_icm_bwd "):txt.index("} dynenv_icm_grad_t;")]
    for word in ("[160][K]", "[K][160]", "[2K][32]", "[N][160]", "[32][2K]", "[32]"):
        assert word in struct, word


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


POINTERS = ["features", "actions", "finished", "count", "upstream", "d_features", "workspace", "status"]


def _args(capi):
    keep = {k: _fake() for k in POINTERS + W_FIELDS + T_FIELDS + G_FIELDS}
    a = {k: v[1] for k, v in keep.items()}
    a.update(T=6, P=40, K=128, AD=4, nvec=[5, 3, 3], G=3, dtype=1, slope=0.1, workspace_bytes=2 * part(128) * 4)
    return keep, a


def _call(capi, a):
    structs = {}
    for key, cls, fields in (("w", capi.Icm, W_FIELDS), ("wt", capi.IcmBwd, T_FIELDS), ("grad", capi.IcmGrad, G_FIELDS)):
        s = cls()
        for k in fields:
            setattr(s, k, a[k].value if a[k] is not None else None)
        structs[key] = None if a.get("no_" + key) else C.byref(s)
    nvec = None if a["nvec"] is None else (C.c_int32 * max(len(a["nvec"]), 1))(*a["nvec"])
    vals = dict(a, nvec=nvec, **structs)
    return capi.load().dynenv_icm_backward(*[vals[k] for k in ORDER], None)


def _apply(a, change):
    if isinstance(change, dict):
        a.update(change)
    else:
        key, off = change.split("+")
        a[key] = C.c_void_p(a[key].value + int(off))


CHANGES = [("null " + k, {k: None}) for k in ("features", "actions", "nvec", "count", "upstream", "workspace")] + \
          [("null " + k, {"no_" + k: True}) for k in ("w", "wt", "grad")] + \
          [("null %s" % k, {k: None}) for k in W_FIELDS + T_FIELDS + G_FIELDS] + \
          [("%s %d" % (k, v), {k: v}) for k in ("T", "P", "K") for v in (0, -1)] + \
          [("G 0", dict(G=0, nvec=[])), ("G 9", dict(G=9, AD=8, nvec=[2] * 9)), ("a group of 0", dict(nvec=[5, 0, 3])), ("a group of 17", dict(nvec=[5, 17, 3])),
           ("N 33", dict(nvec=[16, 16, 1])), ("AD below G", dict(AD=2)), ("AD 9", dict(AD=9)), ("dtype -1", dict(dtype=-1)), ("dtype 3", dict(dtype=3)),
           ("(T + 1) * P above 2^30", dict(T=2 ** 10, P=2 ** 20, workspace_bytes=2 ** 40)),
           ("a workspace one byte short", dict(workspace_bytes=2 * part(128) * 4 - 1)), ("a workspace of nothing", dict(workspace_bytes=0)),
           ("a workspace for fewer players", dict(P=65)), ("a workspace for K = 64", dict(workspace_bytes=2 * part(64) * 4))] + \
          [("%s %d bytes off" % (k, off), "%s+%d" % (k, off)) for k in ["features", "actions", "finished", "d_features", "workspace"] + W_FIELDS + T_FIELDS + G_FIELDS
           for off in (4, 8)] + \
          [("%s 2 bytes off" % k, k + "+2") for k in ("count", "upstream", "status")]


@pytest.mark.parametrize("what, change", CHANGES, ids=[c[0] for c in CHANGES])
def test_argument_errors_come_before_the_device(capi, what, change):
    keep, a = _args(capi)
    _apply(a, change)
    assert _call(capi, a) == ERR_ARG, what
    assert b"icm backward" in capi.load().dynenv_last_error()
    for unsupported in (dict(K=96), dict(dtype=0)):   # an argument error comes before an unsupported case
        if not set(unsupported) & set(change if isinstance(change, dict) else ()) and "workspace" not in what:
            assert _call(capi, dict(a, **unsupported)) == ERR_ARG, (what, unsupported)


UNSUPPORTED = [("float32 operands", dict(dtype=0)), ("K 96", dict(K=96)), ("K 32", dict(K=32)), ("K 256", dict(K=256)), ("K 512", dict(K=512)), ("K 1", dict(K=1))]


@pytest.mark.parametrize("what, change", UNSUPPORTED, ids=[c[0] for c in UNSUPPORTED])
def test_unsupported_shapes_are_refused_before_the_device(capi, what, change):
    keep, a = _args(capi)
    a.update(change)
    assert _call(capi, a) == capi.ERR_UNSUPPORTED, what
    assert b"the fused backward takes" in capi.load().dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        return
    keep, a = _args(capi)
    assert _call(capi, a) == capi.ERR_NO_DEVICE
    big = MAX_WORKGROUPS * part(128) * 4
    for change in (dict(finished=None), dict(d_features=None), dict(status=None), dict(finished=None, d_features=None, status=None), dict(dtype=2), dict(K=64),
                   dict(G=8, AD=8, nvec=[4] * 8), dict(G=2, AD=2, nvec=[16, 16]), dict(G=1, AD=1, nvec=[1]), dict(T=1, P=1),
                   dict(T=2 ** 10 - 1, P=2 ** 20, workspace_bytes=big), dict(P=10 ** 6, workspace_bytes=big), dict(AD=8), dict(workspace_bytes=2 ** 40)):
        assert _call(capi, dict(a, **change)) == capi.ERR_NO_DEVICE, change


def _query(capi, P, K, out=True):
    n = C.c_uint64(12345)
    rc = capi.load().dynenv_icm_backward_workspace(P, K, C.byref(n) if out else None)
    return rc, n.value


def test_the_workspace_query_touches_no_device_is_monotone_and_honours_its_bound(capi):
    for K in (64, 128):
        bound = MAX_WORKGROUPS * part(K) * 4
        last = 0
        for P in (1, 31, 32, 33, 64, 65, 1000, ROWS * MAX_WORKGROUPS - 1, ROWS * MAX_WORKGROUPS, ROWS * MAX_WORKGROUPS + 1, 40960, 2 ** 30):
            rc, n = _query(capi, P, K)
            assert rc == 0 and n == min(-(-P // ROWS), MAX_WORKGROUPS) * part(K) * 4, (P, K)
            assert last <= n <= bound and n % 16 == 0
            last = n
        assert _query(capi, 2 ** 30, K)[1] == bound
    assert {64: 30670848, 128: 55902208} == {K: MAX_WORKGROUPS * part(K) * 4 for K in (64, 128)}, "the header's figures"
    for P in (1, 40, 40960):
        assert _query(capi, P, 64)[1] < _query(capi, P, 128)[1], "monotone in K"
    for P, K, out in ((0, 128, True), (-1, 128, True), (40, 0, True), (40, -1, True), (40, 128, False)):
        assert _query(capi, P, K, out)[0] == ERR_ARG and b"icm backward workspace" in capi.load().dynenv_last_error()
    for K in (1, 32, 96, 256, 512):
        rc, n = _query(capi, 40, K)
        assert rc == capi.ERR_UNSUPPORTED and n == 12345 and b"the fused backward takes" in capi.load().dynenv_last_error()
