"""CPU-side checks of the policy head over a stored rollout (dynenv_policy_eval, dynenv_policy_eval_backward,
dynenv_policy_eval_backward_workspace; GpuPolicyHead.evaluate; GpuRolloutStorage.a2c_loss(evaluation=...)): the header declares the
entry points and the two structs, the binding lists them parameter for parameter, the library exports them, the ABI version stays 3,
every argument error is DYNENV_ERR_ARG - what the kernels do not take DYNENV_ERR_UNSUPPORTED - before a device is looked for, the
workspace query follows its formula; on CPU tensors evaluate names its fallback, a2c_loss(evaluation=ev) is a2c_loss() on a storage
that holds the same tensors, bit for bit, and its gradients reach every actor.* and critic.* parameter."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from host_common import ERR_ARG, built_capi, header_text, header_without_comments

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_eval_ref as ER  # noqa: E402
import policy_ref as PR  # noqa: E402

FWD, BWD, QUERY = "dynenv_policy_eval", "dynenv_policy_eval_backward", "dynenv_policy_eval_backward_workspace"
HEAD = ["features", "actions", "T", "P", "K", "dtype", "w", "nvec", "G", "AD", "slope", "ln_eps"]
ORDER = {FWD: HEAD + ["logp", "probs", "value", "status"],
         BWD: HEAD + ["d_logp", "d_probs", "d_value", "wt", "grad", "d_features", "workspace", "workspace_bytes", "status"]}
W_FIELDS = ["actor_w", "actor_b", "critic_w1", "critic_b1", "critic_ln_w", "critic_ln_b", "critic_w2", "critic_b2"]   # (cont_scale, cont_mean: unused)
T_FIELDS = ["actor_w_t", "critic_w1_t", "actor_w_t_lo", "critic_w1_t_lo"]
G_FIELDS = ["d_actor_w", "d_actor_b", "d_critic_w1", "d_critic_b1", "d_critic_ln_w", "d_critic_ln_b", "d_critic_w2", "d_critic_b2"]


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch before the library, the order every GPU test has)
    return built_capi()


def test_header_declares_the_entry_points_and_the_binding_matches(capi):
    h = header_without_comments()
    head = ("const float* features_dev, const float* actions_dev, int32_t T, int32_t P, int32_t K, int32_t w_dtype, const dynenv_policy_t* w, "
            "const int32_t* nvec, int32_t G, int32_t action_cols, float slope, float ln_eps, ")
    assert "int dynenv_policy_eval(" + head + "float* logp_dev, float* probs_dev, float* value_dev, int32_t* status_dev, void* stream);" in h
    assert ("int dynenv_policy_eval_backward(" + head + "const float* d_logp_dev, const float* d_probs_dev, const float* d_value_dev, "
            "const dynenv_policy_bwd_t* wt, const dynenv_policy_grad_t* grad, float* d_features_dev, void* workspace_dev, uint64_t workspace_bytes, "
            "int32_t* status_dev, void* stream);") in h
    assert "int dynenv_policy_eval_backward_workspace(int32_t rows, int32_t K, uint64_t* bytes);" in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    assert capi.load().dynenv_abi_version() == capi.DYNENV_ABI_VERSION == 3
    from dynenv_amd import policy
    limits = {k: int(re.search(r"#define DYNENV_POLICY_EVAL_%s (\d+)" % k, h).group(1)) for k in ("ROWS", "MAX_WORKGROUPS")}
    assert limits == {"ROWS": policy.EVAL_ROWS, "MAX_WORKGROUPS": policy.EVAL_MAX_WORKGROUPS} == {"ROWS": ER.ROWS, "MAX_WORKGROUPS": ER.MAX_WORKGROUPS}
    assert policy.EVAL_K == (64, 128)
    for tag, cls, fields in (("dynenv_policy_bwd", capi.PolicyBwd, T_FIELDS), ("dynenv_policy_grad", capi.PolicyGrad, G_FIELDS)):
        struct = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (tag, tag), h).group(1)
        assert re.findall(r"\*(\w+)[,;]", struct) == fields == [n for n, _ in cls._fields_]
        assert all(t is C.c_void_p for _, t in cls._fields_) and C.sizeof(cls) == 8 * len(fields)
    vp, i32 = C.c_void_p, C.c_int32
    kinds = {"const float*": vp, "float*": vp, "int32_t*": vp, "void*": vp, "const int32_t*": C.POINTER(i32), "const dynenv_policy_t*": C.POINTER(capi.Policy),
             "const dynenv_policy_bwd_t*": C.POINTER(capi.PolicyBwd), "const dynenv_policy_grad_t*": C.POINTER(capi.PolicyGrad), "int32_t": i32,
             "float": C.c_float, "uint64_t": C.c_uint64, "uint64_t*": C.POINTER(C.c_uint64)}
    lib = capi.load()
    for name, count in ((FWD, 17), (BWD, 22), (QUERY, 3)):
        params = [p.strip() for p in re.search(r"int %s ?\(([^()]*)\) ?;" % name, h).group(1).split(",")]
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params) == count
        for p, got in zip(params, argtypes):   # parameter for parameter
            assert kinds[p.rsplit(" ", 1)[0]] is got, p
        assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes == argtypes


def test_header_comment_states_the_contract():
    txt = header_text()

    def comment(name):
        at = re.search(r"^\s*int\s*%s\(" % name, txt, flags=re.M).start()
        return re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", txt[:at].rsplit("/*", 1)[1]))
    c = comment(FWD)
    for word in ("one launch", "capturable", "[T][P][K]", "[T][AD][P]", "[T][G][P]", "[T][P][N] or NULL", "exactly once", "SAME device function", "bit 0",
                 "eps32", "DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device", "T * P > 2^30", "64 or 128", "storage.py:211-262"):
        assert word in c, word
    c = comment(BWD)
    for word in ("two launches", "capturable", "saved NOTHING", "recomputed", "not clamped", "exactly 0 for a group of one action", "h_pre == 0 included",
                 "nothing is accumulated into", "from N on are +0", "Zero upstream gives +0", "NEVER float16", "THE CHOICE", "bf16 whatever w_dtype is",
                 "by it exactly", "no floating-point atomic", "same bits", "alone", "in workgroup order", "a workspace that is too small", "64 or 128",
                 "DYNENV_ERR_ARG", "DYNENV_ERR_UNSUPPORTED", "before a device"):
        assert word in c, word
    q = comment(QUERY)
    for word in ("host only", "touches no device", "min(ceil(rows / 64), 256) * (K K / 2 + 34 K + 36) * 4", "4 362 240", "12 881 920"):
        assert word in q, word


def _fake(n=64):
    """never dereferenced on the host: a stand-in for a device pointer, 16-byte aligned like the real ones"""
    buf = (C.c_uint8 * (n + 16))()
    at = C.addressof(buf)
    return buf, C.c_void_p(at + (-at) % 16)


POINTERS = ["features", "actions", "logp", "probs", "value", "status", "d_logp", "d_probs", "d_value", "d_features", "workspace"]


def _args():
    keep = {k: _fake() for k in POINTERS + W_FIELDS + T_FIELDS + G_FIELDS}
    a = {k: v[1] for k, v in keep.items()}
    a.update(T=6, P=40, K=128, AD=4, nvec=[5, 3, 3], G=3, dtype=1, slope=0.1, ln_eps=1e-5, workspace_bytes=4 * ER.part(128) * 4)   # (240 rows: 4 blocks)
    return keep, a


def _call(capi, name, a):
    structs = {}
    for key, cls, fields in (("w", capi.Policy, W_FIELDS), ("wt", capi.PolicyBwd, T_FIELDS), ("grad", capi.PolicyGrad, G_FIELDS)):
        s = cls()
        for k in fields:
            setattr(s, k, a[k].value if a[k] is not None else None)
        structs[key] = None if a.get("no_" + key) else C.byref(s)
    nvec = None if a["nvec"] is None else (C.c_int32 * max(len(a["nvec"]), 1))(*a["nvec"])
    vals = dict(a, nvec=nvec, **structs)
    return getattr(capi.load(), name)(*[vals[k] for k in ORDER[name]], None)


def _apply(a, change):
    if isinstance(change, dict):
        a.update(change)
    else:
        key, off = change.split("+")
        a[key] = C.c_void_p(a[key].value + int(off))


SHARED = [("null " + k, {k: None}) for k in ("features", "actions", "nvec")] + [("null w", {"no_w": True})] + \
         [("null %s" % k, {k: None}) for k in W_FIELDS] + \
         [("%s %d" % (k, v), {k: v}) for k in ("T", "P", "K") for v in (0, -1)] + \
         [("G 0", dict(G=0, nvec=[])), ("G 9", dict(G=9, AD=8, nvec=[2] * 9)), ("a group of 0", dict(nvec=[5, 0, 3])), ("a group of 17", dict(nvec=[5, 17, 3])),
          ("N 33", dict(nvec=[16, 16, 1])), ("AD below G", dict(AD=2)), ("AD 9", dict(AD=9)), ("dtype -1", dict(dtype=-1)), ("dtype 3", dict(dtype=3)),
          ("T * P above 2^30", dict(T=2 ** 10 + 1, P=2 ** 20, workspace_bytes=2 ** 40))] + \
         [("%s %d bytes off" % (k, off), "%s+%d" % (k, off)) for k in ["features", "actions"] + W_FIELDS[:-1] for off in (4, 8)] + \
         [("%s 2 bytes off" % k, k + "+2") for k in ("critic_b2", "status")]
CHANGES = {
    FWD: SHARED + [("null " + k, {k: None}) for k in ("logp", "value")] + [("%s %d bytes off" % (k, off), "%s+%d" % (k, off)) for k in ("logp", "probs", "value") for off in (4, 8)],
    BWD: SHARED + [("null " + k, {k: None}) for k in ("d_logp", "d_value", "workspace")] + [("null " + k, {"no_" + k: True}) for k in ("wt", "grad")] +
    [("null %s" % k, {k: None}) for k in T_FIELDS[:2] + G_FIELDS] + [("null %s with float16" % k, {k: None, "dtype": 2}) for k in T_FIELDS[2:]] +
    [("a workspace one byte short", dict(workspace_bytes=4 * ER.part(128) * 4 - 1)), ("a workspace of nothing", dict(workspace_bytes=0)),
     ("a workspace for fewer rows", dict(P=43)), ("a workspace for K = 64", dict(workspace_bytes=4 * ER.part(64) * 4))] +
    [("%s %d bytes off" % (k, off), "%s+%d" % (k, off)) for k in ["d_logp", "d_probs", "d_value", "d_features", "workspace"] + T_FIELDS + G_FIELDS[:-1] for off in (4, 8)] +
    [("d_critic_b2 2 bytes off", "d_critic_b2+2")]}
ALL = [(name, what, change) for name in (FWD, BWD) for what, change in CHANGES[name]]


@pytest.mark.parametrize("name, what, change", ALL, ids=["%s: %s" % (n[len("dynenv_policy_"):], w) for n, w, _ in ALL])
def test_argument_errors_come_before_the_device(capi, name, what, change):
    keep, a = _args()
    _apply(a, change)
    assert _call(capi, name, a) == ERR_ARG, what
    assert b"policy eval" in capi.load().dynenv_last_error()
    for unsupported in (dict(K=96), dict(dtype=0)):   # an argument error comes before an unsupported case
        if not set(unsupported) & set(change if isinstance(change, dict) else ()) and "workspace" not in what:
            assert _call(capi, name, dict(a, **unsupported)) == ERR_ARG, (what, unsupported)


UNSUPPORTED = [("float32 operands", dict(dtype=0)), ("K 96", dict(K=96)), ("K 32", dict(K=32)), ("K 256", dict(K=256)), ("K 512", dict(K=512)), ("K 1", dict(K=1))]


@pytest.mark.parametrize("name", [FWD, BWD])
@pytest.mark.parametrize("what, change", UNSUPPORTED, ids=[c[0] for c in UNSUPPORTED])
def test_unsupported_shapes_are_refused_before_the_device(capi, name, what, change):
    keep, a = _args()
    a.update(change)
    assert _call(capi, name, a) == capi.ERR_UNSUPPORTED, what
    assert b"takes" in capi.load().dynenv_last_error()


def test_well_formed_calls_get_past_the_argument_checks(capi):
    """the same stand-in arguments, unchanged, are not an argument error: what the tests above see is the change they made.  (Only
    without a GPU, where the call stops at the device check - on a GPU it would launch on pointers that are not the device's.)"""
    import torch
    if torch.cuda.is_available():
        return
    keep, a = _args()
    big = ER.MAX_WORKGROUPS * ER.part(128) * 4
    for name in (FWD, BWD):
        assert _call(capi, name, a) == capi.ERR_NO_DEVICE
        for change in (dict(probs=None), dict(d_probs=None), dict(actor_w_t_lo=None, critic_w1_t_lo=None), dict(d_features=None), dict(status=None), dict(dtype=2), dict(K=64), dict(G=8, AD=8, nvec=[4] * 8),
                       dict(G=2, AD=2, nvec=[16, 16]), dict(G=1, AD=1, nvec=[1]), dict(T=1, P=1), dict(T=2 ** 10, P=2 ** 20, workspace_bytes=big),
                       dict(P=10 ** 6, workspace_bytes=big), dict(AD=8), dict(workspace_bytes=2 ** 40)):
            assert _call(capi, name, dict(a, **change)) == capi.ERR_NO_DEVICE, (name, change)


def _query(capi, rows, K, out=True):
    n = C.c_uint64(12345)
    rc = capi.load().dynenv_policy_eval_backward_workspace(rows, K, C.byref(n) if out else None)
    return rc, n.value


def test_the_workspace_query_touches_no_device_and_follows_its_formula(capi):
    ROWS, CAP = ER.ROWS, ER.MAX_WORKGROUPS
    for K in (64, 128):
        assert ER.part(K) == K * K // 2 + 34 * K + 36
        bound = CAP * ER.part(K) * 4
        last = 0
        for rows in (1, 63, 64, 65, 128, 129, 1000, ROWS * CAP - 1, ROWS * CAP, ROWS * CAP + 1, 204800, 2 ** 30):
            rc, n = _query(capi, rows, K)
            assert rc == 0 and n == min(-(-rows // ROWS), CAP) * ER.part(K) * 4, (rows, K)
            assert last <= n <= bound and n % 16 == 0
            last = n
        assert _query(capi, 2 ** 30, K)[1] == bound
    assert {64: 4362240, 128: 12881920} == {K: CAP * ER.part(K) * 4 for K in (64, 128)}, "the header's figures"
    for rows, K, out in ((0, 128, True), (-1, 128, True), (40, 0, True), (40, -1, True), (40, 128, False), (2 ** 30 + 1, 128, True)):
        assert _query(capi, rows, K, out)[0] == ERR_ARG and b"policy eval backward workspace" in capi.load().dynenv_last_error()
    for K in (1, 32, 96, 256, 512):
        rc, n = _query(capi, 40, K)
        assert rc == capi.ERR_UNSUPPORTED and n == 12345 and b"the fused backward takes" in capi.load().dynenv_last_error()


# ---- the module and the loss, on the CPU
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _head(K, groups, pr, **kw):
    from dynenv_amd import GpuPolicyHead
    return PR.load(GpuPolicyHead(K, PR.space(groups), **kw), pr)


def test_evaluate_on_cpu_tensors_names_its_fallback_and_the_default_route(monkeypatch):
    import torch
    from dynenv_amd.policy import PolicyEval
    T, P, K, groups, AD = 3, 7, 64, (3, 3), 2
    pr = PR.make_params(K, groups, seed=1)
    c = ER.make_case(T, P, K, groups, AD, seed=2)
    f, a = _t(c["features"]), _t(c["actions"])
    m = _head(K, groups, pr)
    assert m.last_eval_route is None and m.fused_backward is False
    ev = m.evaluate(f, a)
    assert isinstance(ev, PolicyEval) and ev._fields == ("log_probs", "probs", "values") and m.last_eval_route == "torch"
    assert tuple(ev.log_probs.shape) == (T, len(groups), P) and tuple(ev.probs.shape) == (T, P, sum(groups)) and tuple(ev.values.shape) == (T, P)
    assert all(x.dtype == torch.float32 and x.grad_fn is not None for x in ev)
    on = _head(K, groups, pr, fused_backward=True)
    on.evaluate(f, a)
    assert on.last_eval_route == "torch (fallback: features that are not on the device)"
    with torch.no_grad():
        plain = on.evaluate(f, a, want_probs=False)
    assert on.last_eval_route == "torch (fallback: features that are not on the device)" and plain.probs is None and plain.values.grad_fn is None
    monkeypatch.setenv("DYNENV_POLICY_FUSED", "0")
    on.evaluate(f, a)
    assert on.last_eval_route == "torch (fallback: DYNENV_POLICY_FUSED=0)"
    monkeypatch.delenv("DYNENV_POLICY_FUSED")
    big = _head(256, groups, PR.make_params(256, groups), fused_backward=True)
    big.evaluate(torch.zeros((T, P, 256)), a)
    assert big.last_eval_route == "torch (fallback: K = 256, not 64 or 128)"
    from dynenv_amd import GpuPolicyHead
    box = GpuPolicyHead(K, PR.space(groups, 1), fused_backward=True)
    ev = box.evaluate(f, torch.zeros((T, 3, P)))
    assert box.last_eval_route == "torch (fallback: a Box block)"
    (ev.log_probs.sum() + ev.values.sum() + (ev.probs ** 2).sum()).backward()
    assert all(p.grad is None for p in box.actor.blocks[-1].parameters()) and all(p.grad is not None for p in box._eval_params())
    with pytest.raises(AssertionError):
        m.evaluate(f, a[:, :1])
    with pytest.raises(AssertionError):
        m.evaluate(f[:, :, :32], a)


def _storage(T, E, A, groups, AD, K, rng, **kw):
    """a CPU storage filled with a rollout's worth of values"""
    import torch
    from dynenv_amd import GpuRolloutStorage
    st = GpuRolloutStorage(T, E, A, AD, groups, K, n_probs=sum(groups), device="cpu", **kw)
    P = E * A
    st.rewards.copy_(_t(rng.standard_normal((T, P)).astype(np.float32)))
    st.dones.copy_(_t((rng.random((T, E)) < 0.3).astype(np.float32)))
    st.features.copy_(_t(rng.standard_normal((T + 1, P, K)).astype(np.float32)))
    for g, n in enumerate(groups):
        st.actions[:, g] = _t(rng.integers(0, n, size=(T, P)).astype(np.float32))
    if st.log_probs_old is not None:
        st.log_probs_old.copy_(_t(-rng.random((T, len(groups), P)).astype(np.float32)))
    return st, torch.from_numpy(rng.standard_normal((P, 1)).astype(np.float32))


LOSSES = [dict(), dict(use_full_entropy=True), dict(use_ppo=True), dict(mode="gae"), dict(use_full_entropy=True, use_ppo=True, mode="dones")]


@pytest.mark.parametrize("kw", LOSSES, ids=str)
def test_a2c_loss_with_an_evaluation_is_a2c_loss_on_a_storage_that_holds_the_same_tensors(kw):
    import torch
    T, E, A, K, groups, AD = 3, 2, 5, 64, (5, 3, 3), 4
    kw = dict(kw)
    mode = kw.pop("mode", "reference")
    pr = PR.make_params(K, groups, seed=4)
    rng = np.random.default_rng(7)
    st, final = _storage(T, E, A, groups, AD, K, rng, **kw)
    stored_values = _t(rng.standard_normal((T, E * A)).astype(np.float32))   # (what the rollout stored: returns() reads these)
    st.values.copy_(stored_values)
    m = _head(K, groups, pr)
    ev = m.evaluate(st.features[:-1], st.actions)
    before = {k: b.clone() for k, b in st.buffers().items()}
    got = st.a2c_loss(final, mode=mode, evaluation=ev)
    assert all(torch.equal(b, before[k]) for k, b in st.buffers().items()), "the storage is not written to"
    got.loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert sorted(grads) == sorted(ER.names(groups)) and all(bool(g.any()) and bool(torch.isfinite(g).all()) for g in grads.values()), \
        "gradients reach every actor.* and critic.* parameter"
    # the same tensors IN the storage's three buffers (the reference's storage after a differentiable rollout); returns() must read the
    # stored values in both, so the twin's values buffer holds the evaluation's only where the loss reads it: patch returns()
    m2 = _head(K, groups, pr)
    ev2 = m2.evaluate(st.features[:-1], st.actions)
    twin, _ = _storage(T, E, A, groups, AD, K, np.random.default_rng(7), **kw)
    ret = st.returns(final, 0.99, mode, 0.95)
    twin.returns = lambda *a, **k: ret
    twin.log_probs, twin.values, twin.probs = ev2.log_probs, ev2.values, ev2.probs
    want = twin.a2c_loss(final, mode=mode)
    for k in ("loss", "policy", "value", "entropy", "temp_entropy"):
        assert torch.equal(getattr(got, k).view(torch.int32), getattr(want, k).view(torch.int32)), k
    want.loss.backward()
    for k, p in m2.named_parameters():
        assert torch.equal(grads[k].view(torch.int32), p.grad.view(torch.int32)), k
    # evaluation=None is the function as it was: the stored buffers
    st.log_probs.copy_(ev.log_probs.detach()), st.probs.copy_(ev.probs.detach())
    plain, again = st.a2c_loss(final, mode=mode), st.a2c_loss(final, mode=mode, evaluation=None)
    assert plain.loss.grad_fn is None and torch.equal(plain.loss, again.loss)
    # without probs in the evaluation the loss asks for action_probs
    bare = type(ev)(ev.log_probs, None, ev.values)
    with pytest.raises(AssertionError):
        st_np, _ = _storage(T, E, A, groups, AD, K, np.random.default_rng(7), **kw)
        st_np.probs = None
        st_np.a2c_loss(final, mode=mode, evaluation=bare)
