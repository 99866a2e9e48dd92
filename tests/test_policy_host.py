"""CPU-side checks of the entry point of the fused policy head (dynenv_policy_head): the header declares it and cites the reference, the
binding lists it parameter for parameter, the library exports it, the ABI version stays 3, and every argument error is DYNENV_ERR_ARG -
what the kernel does not take DYNENV_ERR_UNSUPPORTED - before a device is looked for, so that both are the same with and without a
GPU."""
import ctypes as C
import os
import re

import pytest

from host_common import ERR_ARG, ROOT, built_capi, comment_before, header_text, header_without_comments

NAME = "dynenv_policy_head"
F32, BF16, F16 = 0, 1, 2
FIELDS = ["actor_w", "actor_b", "cont_scale", "cont_mean", "critic_w1", "critic_b1", "critic_ln_w", "critic_ln_b", "critic_w2", "critic_b2"]
ORDER = ["feat0", "feat1", "E", "A", "F", "dtype", "w", "nvec", "G", "C", "AD", "seed", "draw", "row_base", "slope", "eps", "turn", "actions", "cont",
         "probs", "logp", "value", "next_ext"]


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_point_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_policy_head(const float* feat0_dev, const float* feat1_dev, int32_t E, int32_t A, int32_t F, int32_t w_dtype, "
            "const dynenv_policy_t* w, const int32_t* nvec, int32_t G, int32_t C, int32_t action_cols, uint64_t seed, const uint64_t* draw_dev, "
            "uint64_t row_base, float slope, float ln_eps, int32_t discrete_turn, int32_t* actions_dev, double* cont_dev, float* probs_dev, "
            "float* logp_dev, float* value_dev, float* next_ext_dev, void* stream);") in h
    assert ("typedef struct dynenv_policy { const void *actor_w; const float *actor_b; const float *cont_scale, *cont_mean; const void *critic_w1; "
            "const float *critic_b1, *critic_ln_w, *critic_ln_b; const float *critic_w2, *critic_b2; } dynenv_policy_t;") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.DYNENV_ABI_VERSION == 3
    lib = capi.load()
    assert lib.dynenv_abi_version() == 3
    params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % NAME, h).group(1).split(",")]
    restype, argtypes = capi.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == len(params) == 24
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const float*": vp, "float*": vp, "double*": vp, "int32_t*": vp, "const uint64_t*": vp, "void*": vp, "int32_t": i32, "float": C.c_float,
             "uint64_t": C.c_uint64, "const int32_t*": C.POINTER(i32), "const dynenv_policy_t*": C.POINTER(capi.Policy)}
    for p, got in zip(params, argtypes):   # parameter for parameter
        assert kinds[p.rsplit(" ", 1)[0]] is got, p
    assert NAME in capi.EXPORTS and hasattr(lib, NAME), "libdynenv_hip.so does not export " + NAME
    assert getattr(lib, NAME).argtypes == argtypes
    assert capi.EXPORTS[-1] == NAME and capi.EXPORTS[-2] == "dynenv_recurrent_head", "the table grows at its end"
    assert [n for n, _ in capi.Policy._fields_] == FIELDS
    assert C.sizeof(capi.Policy) == 10 * C.sizeof(C.c_void_p)
    # the purpose of the draw is named by the header, differs from the step kernels' and is the module's
    purpose = int(re.search(r"#define DYNENV_POLICY_RNG_PURPOSE (\d+)u", h).group(1))
    math_h = open(os.path.join(ROOT, "include", "dynenv_math.h")).read()
    step = [int(v) for v in re.findall(r"#define DM_RNG_\w+ (\d+)u", math_h)]
    assert len(step) >= 9 and purpose > max(step), (purpose, step)
    from dynenv_amd import policy
    assert policy.RNG_PURPOSE == purpose
    limits = {k: int(re.search(r"#define DYNENV_POLICY_%s (\d+)" % k, h).group(1)) for k in ("ROWS", "MAX_GROUPS", "MAX_CONT")}
    assert limits == {"ROWS": policy.MAX_ROWS, "MAX_GROUPS": policy.MAX_GROUPS, "MAX_CONT": policy.MAX_CONT} == {"ROWS": 32, "MAX_GROUPS": 8, "MAX_CONT": 4}


def test_header_comments_state_the_contract_and_cite_the_reference():
    c = comment_before(NAME)
    for word in ("DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "exactly once", "C == 0", "16-byte aligned", "capturable",
                 "64 or 128", "fixed order", "float32", "actor_critic.py:204-213, 230-242", "p / A", "2^30", "same bits", "not finite", "dm_philox",
                 "DYNENV_POLICY_RNG_PURPOSE + g / 4", "w.v[g % 4]", "(word >> 8) * 2^-24", "lo32(row_base + p)", "left to right", "c_j <= t",
                 "one rounding", "never drawn", "eps32", "BOTH 1 and 2", "transformActions", "dynenv_step_head", "dynenv_step", "G..AD-1",
                 "draw_dev is NULL", "read at replay", "N + C > 32", "1..16", "1..8", "0..4", "G..8", "bit for bit"):
        assert word in c, word
    shared = re.sub(r"\s+", " ", header_text().split("#define DYNENV_POLICY_ROWS")[0].rsplit("/*", 1)[1])
    for word in ("actor_critic.py:161-242", "actor_critic.py:88", "actor_critic.py:125-140", "train.py:251-266", "utils.py:20-39", "ActorLayer",
                 "CriticLayer"):
        assert word in shared, word


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


def _args(capi):
    keep = [_fake() for _ in range(10)]
    w = keep[9][1].value
    nvec = (C.c_int32 * 8)(5, 3, 3, 7, 2, 2, 2, 2)
    return keep, dict(feat0=keep[0][1], feat1=keep[1][1], E=5, A=3, F=128, dtype=BF16, w=capi.Policy(*[w] * 10), nvec=nvec, G=3, C=1, AD=4,
                      seed=2 ** 40 + 1, draw=keep[2][1], row_base=2 ** 33, slope=0.1, eps=1e-5, turn=0, actions=keep[3][1], cont=keep[4][1],
                      probs=keep[5][1], logp=keep[6][1], value=keep[7][1], next_ext=keep[8][1])


def _call(lib, a):
    args = [a[k] for k in ORDER]
    args[ORDER.index("w")] = None if a["w"] is None else C.byref(a["w"])
    return lib.dynenv_policy_head(*args, None)


def _nvec(*v):
    return (C.c_int32 * 8)(*(list(v) + [1] * (8 - len(v))))


CHANGES = [("null " + k, {k: None}) for k in ("feat0", "w", "nvec", "actions", "probs", "logp", "value")] + \
          [("cont NULL with C > 0", dict(cont=None)), ("cont given with C == 0", dict(C=0, AD=3))] + \
          [("w without " + f, ("w", f, None)) for f in FIELDS] + \
          [("E 0", dict(E=0)), ("E < 0", dict(E=-1)), ("A 0", dict(A=0)), ("A < 0", dict(A=-3)), ("F 0", dict(F=0)), ("F < 0", dict(F=-64)),
           ("G 0", dict(G=0)), ("G < 0", dict(G=-1)), ("G 9", dict(G=9, C=0, cont=None, AD=8, nvec=_nvec(*[2] * 8))),
           ("a group of 0", dict(nvec=_nvec(5, 0, 3))), ("a group of -1", dict(nvec=_nvec(5, 3, -1))), ("a group of 17", dict(nvec=_nvec(17, 3, 3))),
           ("C < 0", dict(C=-1)), ("C 5", dict(C=5, AD=8)), ("N + C 33", dict(nvec=_nvec(16, 13, 3))), ("N 33", dict(nvec=_nvec(16, 16, 1), C=0, cont=None)),
           ("AD below G", dict(AD=2)), ("AD 9", dict(AD=9)), ("AD 0", dict(AD=0)), ("dtype 3", dict(dtype=3)), ("dtype -1", dict(dtype=-1)),
           ("E * A above 2^30", dict(E=2 ** 20, A=2 ** 11)),
           ("feat0 8 bytes off", "feat0+8"), ("feat0 4 bytes off", "feat0+4"), ("feat1 4 bytes off", "feat1+4"), ("feat1 8 bytes off", "feat1+8"),
           ("actions 4 bytes off", "actions+4"), ("actions 8 bytes off", "actions+8"), ("cont 8 bytes off", "cont+8"), ("probs 4 bytes off", "probs+4"),
           ("logp 8 bytes off", "logp+8"), ("value 4 bytes off", "value+4"), ("next_ext 4 bytes off", "next_ext+4"), ("next_ext 8 bytes off", "next_ext+8"),
           ("draw 4 bytes off", "draw+4")] + \
          [("w %s %d bytes off" % (f, off), ("w", f, off)) for f, off in zip(FIELDS, (2, 4, 2, 1, 8, 4, 8, 4, 8, 2))]


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
    for unsupported in (dict(F=48), dict(dtype=F32)):   # an argument error comes before an unsupported case
        if not set(unsupported) & set(change if isinstance(change, dict) else ()):
            assert _call(lib, dict(a, **unsupported)) == ERR_ARG, (what, unsupported)


UNSUPPORTED = [("float32 operands", dict(dtype=F32)), ("F 48", dict(F=48)), ("F 32", dict(F=32)), ("F 256", dict(F=256)), ("F 96", dict(F=96)),
               ("F 1", dict(F=1)), ("F 256 alone", dict(F=256, feat1=None))]


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
            assert _call(lib, dict(a, F=F, dtype=dtype)) == capi.ERR_NO_DEVICE, (F, dtype)
            assert _call(lib, dict(a, F=F, dtype=dtype, feat1=None)) == capi.ERR_NO_DEVICE
    assert _call(lib, dict(a, draw=None)) == capi.ERR_NO_DEVICE, "the counter is optional"
    assert _call(lib, dict(a, next_ext=None)) == capi.ERR_NO_DEVICE, "next_ext is optional"
    assert _call(lib, dict(a, turn=1, seed=2 ** 64 - 1, row_base=2 ** 64 - 1)) == capi.ERR_NO_DEVICE
    w = capi.Policy(*[a["w"].actor_w] * 10)
    w.cont_scale = w.cont_mean = None
    assert _call(lib, dict(a, C=0, cont=None, AD=3, w=w)) == capi.ERR_NO_DEVICE, "C == 0 ignores cont_scale and cont_mean, which may be NULL"
    for nv, G, Cn, AD in (((16, 16), 2, 0, 2), ((16, 12), 2, 4, 6), ((2, 2, 1, 2, 2, 2, 2, 2), 8, 0, 8), ((1,), 1, 0, 1), ((3, 3), 2, 0, 8)):
        assert _call(lib, dict(a, nvec=_nvec(*nv), G=G, C=Cn, AD=AD, cont=a["cont"] if Cn else None)) == capi.ERR_NO_DEVICE, (nv, Cn, AD)
