"""CPU-side checks of the two entry points of the rollout storage (dynenv_rollout_insert, dynenv_rollout_returns): the header declares
them and cites the reference, the binding lists them parameter for parameter, the library exports them, the ABI version stays 3, and every
argument error is DYNENV_ERR_ARG - what the kernel does not take DYNENV_ERR_UNSUPPORTED - before a device is looked for, so that both are
the same with and without a GPU."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, header_text, header_without_comments

INSERT, RETURNS = "dynenv_rollout_insert", "dynenv_rollout_returns"
I_ORDER = ["cursor", "T", "E", "A", "F", "G", "AD", "N", "only", "rewards_in", "finished_in", "feat0", "feat1", "actions_in", "logp_in", "logp_old_in",
           "value_in", "dones_in", "probs_in", "rewards", "finished", "features", "actions", "logp", "logp_old", "values", "dones", "probs", "status"]
R_ORDER = ["rewards", "values", "dones", "final", "T", "E", "A", "mode", "gamma", "lam", "returns", "advantages"]
PAIRS = [("rewards_in", "rewards"), ("finished_in", "finished"), ("feat0", "features"), ("actions_in", "actions"), ("logp_in", "logp"),
         ("logp_old_in", "logp_old"), ("value_in", "values"), ("dones_in", "dones"), ("probs_in", "probs")]


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has: see test_arranger_grad_host.py)
    return built_capi()


def test_header_declares_the_entry_points_and_the_binding_matches(capi):
    h = header_without_comments()
    assert ("int dynenv_rollout_insert(const int32_t* cursor_dev, int32_t T, int32_t E, int32_t A, int32_t F, int32_t G, int32_t action_cols, int32_t N, "
            "int32_t row_features_only, const double* rewards_in_dev, const uint8_t* finished_in_dev, const float* feat0_dev, const float* feat1_dev, "
            "const int32_t* actions_in_dev, const float* logp_in_dev, const float* logp_old_in_dev, const float* value_in_dev, const uint8_t* dones_in_dev, "
            "const float* probs_in_dev, float* rewards_dev, uint8_t* finished_dev, float* features_dev, float* actions_dev, float* logp_dev, "
            "float* logp_old_dev, float* values_dev, float* dones_dev, float* probs_dev, int32_t* status_dev, void* stream);") in h
    assert ("int dynenv_rollout_returns(const float* rewards_dev, const float* values_dev, const float* dones_dev, const float* final_value_dev, "
            "int32_t T, int32_t E, int32_t A, int32_t mode, float gamma, float gae_lambda, float* returns_dev, float* advantages_dev, void* stream);") in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.DYNENV_ABI_VERSION == 3
    lib = capi.load()
    assert lib.dynenv_abi_version() == 3
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const float*": vp, "float*": vp, "const double*": vp, "const int32_t*": vp, "int32_t*": vp, "const uint8_t*": vp, "uint8_t*": vp, "void*": vp,
             "int32_t": i32, "float": C.c_float}
    for name, count in ((INSERT, 30), (RETURNS, 13)):
        params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % name, h).group(1).split(",")]
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params) == count
        for p, got in zip(params, argtypes):   # parameter for parameter
            assert kinds[p.rsplit(" ", 1)[0]] is got, p
        assert name in capi.EXPORTS and hasattr(lib, name), "libdynenv_hip.so does not export " + name
        assert getattr(lib, name).argtypes == argtypes
    modes = {k: int(re.search(r"#define DYNENV_RETURNS_%s (\d+)" % k, h).group(1)) for k in ("REFERENCE", "DONES", "GAE")}
    assert modes == {"REFERENCE": capi.RETURNS_REFERENCE, "DONES": capi.RETURNS_DONES, "GAE": capi.RETURNS_GAE} == {"REFERENCE": 0, "DONES": 1, "GAE": 2}
    from dynenv_amd import policy, rollout
    assert rollout.RETURN_MODES == {"reference": 0, "dones": 1, "gae": 2}
    assert (rollout.MAX_GROUPS, rollout.MAX_COLS, rollout.MAX_PROBS) == (policy.MAX_GROUPS, policy.MAX_COLS, policy.MAX_ROWS) == (8, 8, 32)


def _comment(txt, before):
    """the last comment in front of the declaration (or the line) `before`, without the " * " that begins its lines - a phrase may straddle
    two of them - and white space collapsed"""
    at = txt.index(before) if before.startswith("#") else re.search(r"^\s*int\s*%s\(" % re.escape(before), txt, flags=re.M).start()
    return re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", txt[:at].rsplit("/*", 1)[1]))


def test_header_comments_state_the_contract_and_cite_the_reference():
    c = _comment(header_text(), INSERT)
    for word in ("DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "exactly once", "capturable", "cursor_dev[0]", "read at replay",
                 "does not advance", "storage.py:134-166", "train.py:277", "train.py:290", "storage.py:158", "storage.py:166", "rounded once to nearest",
                 "transposed", "never materialised", "0.0 or 1.0", "may be NULL", "not touched", "row_features_only", "t = T", "writes NOTHING",
                 "status_dev[0]", "16-byte aligned", "multiple of 4", "G > 8", "action_cols > 8", "N > 32", "2^30", "E * A * K > 2^32", "same bits"):
        assert word in c, word
    c = _comment(header_text(), RETURNS)
    for word in ("DYNENV_ERR_ARG", "before a device", "exactly once", "capturable", "storage.py:168-209", "storage.py:195", "float32 throughout",
                 "rounded on its own", "no fused multiply-add", "t = T-1 .. 0", "nd = 1 - dones[t][p / A]", "R = rewards[t] + g * R", "NOT looked at",
                 "R = rewards[t] + (g * R) * nd", "next = t == T-1 ? final_value : values[t+1]", "delta = (rewards[t] + (g * next) * nd) - values[t]",
                 "adv = delta + ((g * lambda) * adv) * nd", "returns[t] = adv + values[t]", "advantages[t] = returns[t] - values[t]", "p / A"):
        assert word in c, word
    shared = _comment(header_text(), "#define DYNENV_RETURNS_REFERENCE")
    for word in ("DynEnv/models/storage.py", "storage.py:76-111", "reset_buffers", "[T+1][P][K]", "[T][AD][P]", "[T][G][P]", "[T][E]", "[T][P][N]", "agentFinished"):
        assert word in shared, word


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


def _insert_args():
    names = [k for k in I_ORDER if k not in ("T", "E", "A", "F", "G", "AD", "N", "only")]
    keep = {k: _fake() for k in names}
    a = {k: v[1] for k, v in keep.items()}
    a.update(T=6, E=5, A=3, F=64, G=3, AD=4, N=11, only=0)
    return keep, a


def _returns_args():
    names = ["rewards", "values", "dones", "final", "returns", "advantages"]
    keep = {k: _fake() for k in names}
    a = {k: v[1] for k, v in keep.items()}
    a.update(T=6, E=5, A=3, mode=2, gamma=0.99, lam=0.95)
    return keep, a


def _insert(lib, a):
    return lib.dynenv_rollout_insert(*[a[k] for k in I_ORDER], None)


def _returns(lib, a):
    return lib.dynenv_rollout_returns(*[a[k] for k in R_ORDER], None)


def _apply(a, change):
    if isinstance(change, dict):
        a.update(change)
    else:
        key, off = change.split("+")
        a[key] = C.c_void_p(a[key].value + int(off))


I_CHANGES = [("null cursor", dict(cursor=None)), ("null status", dict(status=None))] + \
            [("%s %d" % (k, v), {k: v}) for k in ("T", "E", "A", "F", "G", "AD") for v in (0, -1)] + \
            [("N < 0", dict(N=-1)), ("T above 2^24", dict(T=2 ** 24 + 1)), ("E * A above 2^30", dict(E=2 ** 20, A=2 ** 11)),
             ("a feature row above 2^32", dict(E=2 ** 20, A=2 ** 10, F=2 ** 11)), ("feat1 without feat0", dict(feat0=None)), ("features only without feat0", dict(only=1, feat0=None, feat1=None)),
             ("probs with N 0", dict(N=0))] + \
            [("%s without its buffer" % i, {o: None}) for i, o in PAIRS] + \
            [("%s %d bytes off" % (k, off), "%s+%d" % (k, off)) for k in ("feat0", "feat1", "features") for off in (4, 8)] + \
            [("%s 2 bytes off" % k, k + "+2") for k in ("cursor", "status", "actions_in", "logp_in", "logp_old_in", "value_in", "probs_in", "rewards", "actions",
                                                         "logp", "logp_old", "values", "dones", "probs")] + \
            [("rewards_in 4 bytes off", "rewards_in+4")]


@pytest.mark.parametrize("what, change", I_CHANGES, ids=[c[0] for c in I_CHANGES])
def test_insert_argument_errors_come_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _insert_args()
    _apply(a, change)
    assert _insert(lib, a) == ERR_ARG, what
    assert b"rollout insert" in lib.dynenv_last_error()
    for unsupported in (dict(F=66), dict(G=9, AD=9), dict(N=33)):   # an argument error comes before an unsupported case
        if not set(unsupported) & set(change if isinstance(change, dict) else ()):
            assert _insert(lib, dict(a, **unsupported)) == ERR_ARG, (what, unsupported)


I_UNSUPPORTED = [("F 66", dict(F=66)), ("F 1", dict(F=1)), ("F 2 twice", dict(F=2)), ("F 63 alone", dict(F=63, feat1=None)), ("G 9", dict(G=9)),
                 ("AD 9", dict(AD=9)), ("N 33", dict(N=33)), ("N 33 without probs", dict(N=33, probs_in=None, probs=None))]


@pytest.mark.parametrize("what, change", I_UNSUPPORTED, ids=[c[0] for c in I_UNSUPPORTED])
def test_insert_unsupported_shapes_are_refused_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _insert_args()
    a.update(change)
    assert _insert(lib, a) == capi.ERR_UNSUPPORTED, what
    assert b"the fused insert takes" in lib.dynenv_last_error()


R_CHANGES = [("null " + k, {k: None}) for k in ("rewards", "final", "returns")] + \
            [("mode -1", dict(mode=-1)), ("mode 3", dict(mode=3)), ("dones NULL in mode 1", dict(mode=1, dones=None)), ("dones NULL in mode 2", dict(dones=None)),
             ("values NULL in mode 2", dict(values=None)), ("values NULL with advantages", dict(mode=0, values=None))] + \
            [("%s %d" % (k, v), {k: v}) for k in ("T", "E", "A") for v in (0, -1)] + \
            [("T above 2^24", dict(T=2 ** 24 + 1)), ("E * A above 2^30", dict(E=2 ** 20, A=2 ** 11))] + \
            [("%s 2 bytes off" % k, k + "+2") for k in ("rewards", "values", "dones", "final", "returns", "advantages")]


@pytest.mark.parametrize("what, change", R_CHANGES, ids=[c[0] for c in R_CHANGES])
def test_returns_argument_errors_come_before_the_device(capi, what, change):
    lib = capi.load()
    keep, a = _returns_args()
    _apply(a, change)
    assert _returns(lib, a) == ERR_ARG, what
    assert b"rollout returns" in lib.dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    lib = capi.load()
    keep, a = _insert_args()
    assert _insert(lib, a) == capi.ERR_NO_DEVICE
    for i, o in PAIRS:   # every input may be NULL, and its buffer with it
        drop = {i: None, o: None}
        if i == "feat0":
            drop["feat1"] = None
        assert _insert(lib, dict(a, **drop)) == capi.ERR_NO_DEVICE, i
    assert _insert(lib, dict(a, feat1=None)) == capi.ERR_NO_DEVICE
    assert _insert(lib, dict(a, only=1)) == capi.ERR_NO_DEVICE
    assert _insert(lib, dict(a, N=0, probs_in=None, probs=None)) == capi.ERR_NO_DEVICE
    for change in (dict(F=4), dict(F=256), dict(G=8, AD=8, N=32), dict(G=1, AD=1, N=1), dict(T=1, E=1, A=1), dict(T=2 ** 24), dict(E=2 ** 15, A=2 ** 10, F=2 ** 6)):
        assert _insert(lib, dict(a, **change)) == capi.ERR_NO_DEVICE, change
    keep2, r = _returns_args()
    for mode in (0, 1, 2):
        assert _returns(lib, dict(r, mode=mode)) == capi.ERR_NO_DEVICE
        assert _returns(lib, dict(r, mode=mode, advantages=None)) == capi.ERR_NO_DEVICE
    assert _returns(lib, dict(r, mode=0, dones=None)) == capi.ERR_NO_DEVICE, "mode 0 does not look at dones"
    assert _returns(lib, dict(r, mode=1, values=None, advantages=None)) == capi.ERR_NO_DEVICE
