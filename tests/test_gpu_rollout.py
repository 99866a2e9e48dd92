"""The rollout storage on the device (-m gpu): dynenv_rollout_insert and dynenv_rollout_returns through the C ABI against the numpy
statements of tests/rollout_ref.py, bit for bit and between guard bands; GpuRolloutStorage's routes; BatchedDynEnv.agent_finished()
against the compat step(); and GpuRollout - step, extractor, policy and insert as one recorded graph - against an eagerly looped twin.

The insert's tiling: workgroup b of 256 threads copies the chunk of 1024 16-byte pieces of the feature row from piece 1024 b on, a
thread four of them, and takes the row group of the 64 players from 64 b on for everything else; the grid is the larger count.  The cases
sit on both sides of both: one player (16 pieces); 65 players of 13 environments with K = 64 - one player past a row group, 1040 pieces:
one ROW past a chunk, the chunks decide the grid, and the dones' 13 elements end inside the first workgroup; 130 players with K = 256
from two features (8320 pieces: eight chunks and an eighth, three row groups) and G < AD; the kernel's caps with 21 players."""
import ctypes as C

import numpy as np
import pytest

import rollout_ref as RR

pytestmark = pytest.mark.gpu

GUARD = 256   # bytes on either side of a buffer
BAND = 0xA5


class Band(object):
    """an array's bytes on the device between two guard bands (the Guarded of test_gpu_arranger_dtype.py for a pre-filled buffer of
    any item size): the payload starts 16-byte aligned"""

    def __init__(self, array):
        import torch
        self.dtype, self.shape, self.n = array.dtype, array.shape, array.nbytes
        self.buf = torch.full((self.n + 2 * GUARD,), BAND, dtype=torch.uint8, device="cuda")
        self.buf[GUARD:GUARD + self.n] = torch.from_numpy(np.frombuffer(array.tobytes(), np.uint8).copy()).cuda()
        assert (self.buf.data_ptr() + GUARD) % 16 == 0

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def get(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == BAND).all() and (b[GUARD + self.n:] == BAND).all(), what + ": a guard band was written"
        return b[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape)


def _pattern(seed):
    rng = np.random.default_rng(seed)

    def fill(name, shape, dt):
        if dt == np.uint8:
            return np.full(shape, 7, np.uint8)
        return (rng.random(shape) + 100.0).astype(np.float32)   # no step writes a value near 100
    return fill


def _same(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


INPUTS = ("rewards", "finished", "feat0", "feat1", "actions", "log_probs", "log_probs_old", "value", "dones", "probs")
OUTPUTS = ("rewards", "agentFinished", "features", "actions", "log_probs", "log_probs_old", "values", "dones", "probs")
OUT_OF = dict(zip(INPUTS, ("rewards", "agentFinished", "features", "features", "actions", "log_probs", "log_probs_old", "values", "dones", "probs")))

INSERT_CASES = [(1, 1, 1, 64, False, 2, 2, 6), (3, 13, 5, 64, False, 2, 2, 6), (6, 13, 10, 128, True, 3, 4, 11), (2, 7, 3, 64, True, 8, 8, 32)]


@pytest.mark.parametrize("case", INSERT_CASES, ids=["T%d-E%d-A%d-F%d-%s-G%d-AD%d-N%d" % (c[:4] + ("two" if c[4] else "one",) + c[5:]) for c in INSERT_CASES])
def test_c_abi_insert_writes_its_row_exactly_and_nothing_else(case):
    """every output between guard bands and pre-filled with a pattern; after every call ALL buffers equal the numpy statement's bit for
    bit, which covers the row written, every other row's pattern, the buffers of NULL inputs and the guard bands: at cursor 0 and T - 1,
    with inputs left out, at the cursors T and -1 (nothing but the status word), with row_features_only at T and T + 1, and for every
    row of a full rollout"""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    T, E, A, F, two, G, AD, N = case
    P, K = E * A, F * (2 if two else 1)
    rng = np.random.default_rng(sum(case))
    want = RR.make_buffers(T, E, A, K, G, AD, N, fill=_pattern(1))
    bands = {k: Band(v) for k, v in want.items()}
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    at = {}

    def call(t, step, only=False, leave_out=()):
        dev = {k: (None if v is None or k in leave_out else torch.from_numpy(v).cuda()) for k, v in step.items()}
        out = {k: (bands[OUT_OF[k]].ptr() if dev[k] is not None else None) for k in INPUTS}
        cursor.fill_(t)
        at["t"] = t
        p = _capi.ptr
        rc = lib.dynenv_rollout_insert(p(cursor), T, E, A, F, G, AD, N, int(only), p(dev["rewards"]), p(dev["finished"]), p(dev["feat0"]), p(dev["feat1"]),
                                       p(dev["actions"]), p(dev["log_probs"]), p(dev["log_probs_old"]), p(dev["value"]), p(dev["dones"]), p(dev["probs"]),
                                       out["rewards"], out["finished"], out["feat0"], out["actions"], out["log_probs"], out["log_probs_old"], out["value"],
                                       out["dones"], out["probs"], p(status), None)
        assert rc == 0, lib.dynenv_last_error()
        torch.cuda.synchronize()
        return {k: v for k, v in step.items() if k not in leave_out}

    def check(what, flagged=False):
        assert int(status) == int(flagged), what + ": the status word"
        status.zero_()
        assert int(cursor) == at["t"], what + ": the kernel does not move the cursor"
        for k in OUTPUTS:
            assert _same(bands[k].get(what + ": " + k), want[k]), "%s: %s" % (what, k)

    step = lambda: RR.make_step(rng, E, A, F, two, G, AD, N)
    for t in (0, T - 1):
        RR.insert_row(want, t, **call(t, step()))
        check("cursor %d" % t)
    RR.insert_row(want, 0, **call(0, step(), leave_out=("finished", "actions", "log_probs_old", "dones", "probs")))
    check("NULL finished, actions, log_probs_old, dones, probs")
    RR.insert_row(want, T - 1, **call(T - 1, step(), leave_out=("rewards", "feat0", "feat1", "log_probs", "value")))
    check("NULL rewards, features, log_probs, value")
    for t in (T, -1):
        call(t, step())
        check("cursor %d writes nothing" % t, flagged=True)
    RR.insert_row(want, T, features_only=True, **call(T, step(), only=True))
    check("row_features_only at T")
    assert not _same(want["features"][T], RR.make_buffers(T, E, A, K, G, AD, N, fill=_pattern(1))["features"][T])
    call(T + 1, step(), only=True)
    check("row_features_only at T + 1 writes nothing", flagged=True)
    for t in range(T):
        RR.insert_row(want, t, **call(t, step()))
        check("row %d of a full rollout" % t)
    fresh = RR.make_buffers(T, E, A, K, G, AD, N, fill=_pattern(1))
    for k in OUTPUTS:   # the rollout replaced every element of every row (features: and the bootstrap's)
        assert (want[k] <= 1).all() if k == "agentFinished" else not (want[k] >= 100).any(), k
    assert fresh["agentFinished"].min() == 7 and fresh["values"].min() >= 100


def _dones(kind, T, E):
    d = np.zeros((T, E), np.float32)
    if kind == "last":
        d[T - 1] = 1
    elif kind == "mid":
        d[T // 2, E // 2] = 1
    return d


RETURN_SHAPES = [(T, E, A) for T in (1, 6) for E, A in ((1, 1), (13, 5), (13, 10), (60, 5))]   # P = 1, 65, 130 and 300: a second workgroup of 256 lanes


@pytest.mark.parametrize("shape", RETURN_SHAPES, ids=["T%d-E%d-A%d" % s for s in RETURN_SHAPES])
def test_c_abi_returns_are_the_statement_bit_for_bit(shape):
    """the three modes, with and without advantages, between guard bands, for no done, a whole batch done at the last step and one
    environment done in mid-rollout"""
    import torch
    from dynenv_amd import _capi
    lib = _capi.load()
    T, E, A = shape
    P = E * A
    rng = np.random.default_rng(T * 1000 + P)
    rewards, values = rng.standard_normal((T, P)).astype(np.float32), rng.standard_normal((T, P)).astype(np.float32)
    final = rng.standard_normal(P).astype(np.float32)
    dev = lambda x: torch.from_numpy(x).cuda()
    r_d, v_d, f_d = dev(rewards), dev(values), dev(final)
    p = _capi.ptr
    for kind in ("none", "last", "mid"):
        dones = _dones(kind, T, E)
        d_d = dev(dones)
        for mode, name in enumerate(("reference", "dones", "gae")):
            want_r, want_a = RR.returns(rewards, values, dones, final, A, 0.99, name, 0.95)
            for with_adv in (True, False):
                ret, adv = Band(np.full((T, P), 100, np.float32)), Band(np.full((T, P), 100, np.float32))
                rc = lib.dynenv_rollout_returns(p(r_d), p(v_d), p(d_d), p(f_d), T, E, A, mode, 0.99, 0.95, ret.ptr(), adv.ptr() if with_adv else None, None)
                assert rc == 0, lib.dynenv_last_error()
                torch.cuda.synchronize()
                what = "%s %s" % (kind, name)
                assert _same(ret.get(what), want_r), what
                assert _same(adv.get(what), want_a if with_adv else np.full((T, P), 100, np.float32)), what
        if kind == "mid" and T > 1:
            cut, _ = RR.returns(rewards, values, dones, final, A, 0.99, "dones")
            ref, _ = RR.returns(rewards, values, dones, final, A, 0.99, "reference")
            assert not np.array_equal(cut, ref), "the done changes mode 1"


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _fill(st, steps, ppo):
    for s in steps:
        a = dict(rewards=_t(s["rewards"]), finished=_t(s["finished"]), feat0=_t(s["feat0"]), feat1=None if s["feat1"] is None else _t(s["feat1"]),
                 actions=_t(s["actions"]), log_probs=_t(s["log_probs"]), value=_t(s["value"]), dones=_t(s["dones"]),
                 probs=None if s["probs"] is None else _t(s["probs"]),
                 log_probs_old=_t(s["log_probs_old"]) if ppo else None)
        st.insert(**a)


def test_module_routes_are_bit_identical_and_the_fallbacks_are_named(monkeypatch):
    import torch
    from dynenv_amd import GpuRolloutStorage
    T, E, A, F, G, AD, groups = 4, 13, 5, 64, 2, 3, (5, 6)
    P, N = E * A, sum(groups)
    rng = np.random.default_rng(5)
    steps = [RR.make_step(rng, E, A, F, True, G, AD, N) for _ in range(T + 1)]
    make = lambda **kw: GpuRolloutStorage(T, E, A, AD, groups, 2 * F, n_probs=N, use_ppo=True, **kw)
    fused, plain = make(), make()
    ptrs = {k: b.data_ptr() for k, b in fused.buffers().items()}
    _fill(fused, steps[:T], True)
    assert fused.last_route == "fused" and int(fused.cursor) == T and int(fused.status) == 0
    monkeypatch.setenv("DYNENV_ROLLOUT_FUSED", "0")
    _fill(plain, steps[:T], True)
    assert plain.last_route == "torch (fallback: DYNENV_ROLLOUT_FUSED=0)"
    plain.insert_final(_t(steps[T]["feat0"]), _t(steps[T]["feat1"]))
    monkeypatch.delenv("DYNENV_ROLLOUT_FUSED")
    fused.insert_final(_t(steps[T]["feat0"]), _t(steps[T]["feat1"]))
    assert fused.last_route == "fused" and plain.last_route == "torch (fallback: DYNENV_ROLLOUT_FUSED=0)" and int(fused.cursor) == T
    want = RR.make_buffers(T, E, A, 2 * F, G, AD, N)
    for t, s in enumerate(steps[:T]):
        RR.insert_row(want, t, **s)
    RR.insert_row(want, T, feat0=steps[T]["feat0"], feat1=steps[T]["feat1"], features_only=True)
    for k, b in fused.buffers().items():
        assert torch.equal(b, plain.buffers()[k]), k
        assert _same(b.cpu().numpy(), want[k]), k
    assert fused.agentFinished.dtype == torch.bool and int(fused.status) == 0 and int(plain.status) == 0
    # one insert too many: both routes write nothing but the status word
    before = {k: b.clone() for k, b in fused.buffers().items()}
    for st in (fused, plain):
        st.cursor.fill_(T)
        if st is plain:
            monkeypatch.setenv("DYNENV_ROLLOUT_FUSED", "0")
        _fill(st, steps[:1], True)
        monkeypatch.delenv("DYNENV_ROLLOUT_FUSED", raising=False)
        assert int(st.status) == 1 and all(torch.equal(b, before[k]) for k, b in st.buffers().items())
    # the returns: kernel and torch statements, every mode
    final = _t(rng.standard_normal(P).astype(np.float32)).view(P, 1)
    fused.dones[1, 3] = 1
    for mode in ("reference", "dones", "gae"):
        got = fused.returns(final, 0.97, mode, 0.9)
        assert fused.last_returns_route == "fused"
        monkeypatch.setenv("DYNENV_ROLLOUT_FUSED", "0")
        alt = fused.returns(final, 0.97, mode, 0.9)
        assert fused.last_returns_route == "torch (fallback: DYNENV_ROLLOUT_FUSED=0)"
        monkeypatch.delenv("DYNENV_ROLLOUT_FUSED")
        ref = RR.returns(fused.rewards.cpu().numpy(), fused.values.cpu().numpy(), fused.dones.cpu().numpy(), final.cpu().numpy().reshape(-1), A, 0.97, mode, 0.9)
        for g, a, r in zip(got, alt, ref):
            assert torch.equal(g, a) and _same(g.cpu().numpy(), r), mode
    # after_update: the same memory, zeroed, the cursor rewound
    fused.after_update()
    assert {k: b.data_ptr() for k, b in fused.buffers().items()} == ptrs and int(fused.cursor) == 0 and int(fused.status) == 0
    assert not any(bool(b.any()) for b in fused.buffers().values())
    # the other fallbacks, by name; each is the numpy row all the same
    s = steps[0]
    fused.insert(_t(s["rewards"]).float(), _t(s["finished"]), _t(s["feat0"]), _t(s["feat1"]), _t(s["actions"]), _t(s["log_probs"]), _t(s["value"]), _t(s["dones"]))
    assert fused.last_route == "torch (fallback: rewards that is not torch.float64, contiguous and on cuda:0)", fused.last_route
    wide = torch.zeros((P, F + 4), device="cuda")
    wide[:, :F] = _t(s["feat0"])
    fused.insert(_t(s["rewards"]), _t(s["finished"]), wide[:, :F], _t(s["feat1"]), _t(s["actions"]), _t(s["log_probs"]), _t(s["value"]), _t(s["dones"]))
    assert fused.last_route == "torch (fallback: feat0 that is not torch.float32, contiguous and on cuda:0)", fused.last_route
    lp = _t(s["log_probs"]).requires_grad_(True)
    fused.insert(_t(s["rewards"]), _t(s["finished"]), _t(s["feat0"]), _t(s["feat1"]), _t(s["actions"]), lp, _t(s["value"]), _t(s["dones"]))
    assert fused.last_route == "torch" and fused.log_probs.grad_fn is not None
    fused.insert(_t(s["rewards"]), _t(s["finished"]), _t(s["feat0"]), _t(s["feat1"]), _t(s["actions"]), _t(s["log_probs"]), _t(s["value"]), _t(s["dones"]))
    assert fused.last_route == "torch (fallback: a log_probs that carries a gradient: after_update() first)", fused.last_route
    want = RR.make_buffers(T, E, A, 2 * F, G, AD, N)
    for t in range(4):
        RR.insert_row(want, t, **{k: v for k, v in s.items() if k not in ("probs", "log_probs_old")})
    for k, b in fused.buffers().items():
        assert _same(b.detach().cpu().numpy(), want[k]), k
    fused.after_update()
    assert {k: b.data_ptr() for k, b in fused.buffers().items()} == ptrs and fused.log_probs.grad_fn is None
    odd = GpuRolloutStorage(2, 3, 2, 2, (3, 3), 6)
    step = RR.make_step(rng, 3, 2, 6, False, 2, 2, 0)
    _fill(odd, [step], False)
    assert odd.last_route == "torch (fallback: F = 6, not a multiple of 4)" and _same(odd.features[0].cpu().numpy(), step["feat0"])


def test_a2c_loss_on_the_device_matches_the_float64_statement_within_the_derived_bound():
    """the bound of tests/test_rollout_ref.py (rollout_ref.a2c_loss derives it from its own float64 terms), A2C and PPO, batch and full
    entropy, on the golden cases' inputs; the distances are printed beside it"""
    from dynenv_amd import GpuRolloutStorage
    for i, (use_ppo, full) in enumerate(((False, False), (True, True), (False, True), (True, False))):
        T, E, A, groups, F = 5, 13, 5, (3, 3), 8
        steps, final = RR.golden_case(T, E, A, groups, F, 40 + i)
        st = GpuRolloutStorage(T, E, A, 2, groups, F, n_probs=6, use_full_entropy=full, use_ppo=use_ppo)
        _fill(st, steps, use_ppo)
        assert st.last_route == "fused"
        got = st.a2c_loss(_t(final), None, 0.5, 0.1)
        assert st.last_returns_route == "fused"
        ret, adv = RR.returns(st.rewards.cpu().numpy(), st.values.cpu().numpy(), st.dones.cpu().numpy(), final, A)
        ref = RR.a2c_loss(ret, adv, st.values.cpu().numpy(), st.log_probs.cpu().numpy(), st.probs.cpu().numpy(), groups, 0.5, 0.1, full,
                          st.log_probs_old.cpu().numpy() if use_ppo else None)
        for k in ("loss", "policy", "value", "entropy", "temp_entropy"):
            err = abs(float(getattr(got, k)) - getattr(ref, k))
            print("ppo=%d full=%d %-12s exact %+.9e  distance %.3g  bound %.3g" % (use_ppo, full, k, getattr(ref, k), err, ref.bound[k]))
            assert err <= ref.bound[k], k


def _twin_pair(env_type, players, E=4, **kw):
    from dynenv_amd import BatchedDynEnv
    envs = [BatchedDynEnv(env_type, E, players, seed=21, **kw) for _ in range(2)]
    for e in envs:
        e.reset_flat()
    return envs


def test_agent_finished_is_the_last_column_of_the_compat_full_state_driving():
    """a set_state scene with a finished car (and one that crashed), stepped in lock step by step_flat() here and the compat step() there"""
    import torch
    from dynenv_amd import DynEnvType, NoiseType, ObservationType
    for kw in ({}, dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=3)):
        env, twin = _twin_pair(DynEnvType.DRIVE, 10, **kw)
        E, A = env.num_envs, env.n_agents
        for e, car, crashed in ((0, 2, 0), (2, 0, 1), (2, 9, 0)):
            for h in (env, twin):
                st = h.get_state(e)
                st.cars[car].finished, st.cars[car].crashed = 1, crashed
                h.set_state(e, st)
        acts = np.ones((E, A, 2), np.int32)
        for s in range(2):
            env.step_flat(torch.from_numpy(acts).cuda(), auto_reset=False)
            _, _, _, infos = twin.step(acts)
            want = np.stack([np.asarray(infos[e]["Full State"][0])[:, -1] for e in range(E)]) != 0
            got = env.agent_finished()
            assert got.dtype == torch.bool and tuple(got.shape) == (E, A) and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), want), s
            assert want[0, 2] and want[2, 0] and want[2, 9] and not want[1].any() and not want[0, 0]
            out = torch.zeros((E, A), dtype=torch.bool, device="cuda")
            assert env.agent_finished(out=out) is out and torch.equal(out, got)
        for h in (env, twin):
            h.close()


def test_agent_finished_is_the_last_column_of_the_compat_full_state_robocup():
    """a scene with a fallen robot (and a penalized one)"""
    import torch
    from dynenv_amd import DynEnvType
    env, twin = _twin_pair(DynEnvType.ROBO_CUP, 5)
    E, A = env.num_envs, env.n_agents
    for h in (env, twin):
        st = h.get_state(1)
        st.robots[3].fallen, st.robots[3].fall_time, st.robots[3].fall_cntr = 1, 2000.0, 1
        st.robots[7].penalized, st.robots[7].penal_time = 1, 15000.0
        h.set_state(1, st)
    acts = np.zeros((E, A, 4), np.int32)
    for s in range(2):
        env.step_flat(torch.from_numpy(acts).cuda(), auto_reset=False)
        _, _, _, infos = twin.step(acts)
        want = np.stack([np.asarray(infos[e]["Full State"][0])[:, -1] for e in range(E)]) != 0
        got = env.agent_finished()
        assert got.dtype == torch.bool and tuple(got.shape) == (E, A)
        assert np.array_equal(got.cpu().numpy(), want), s
        assert want[1, 3] and want[1, 7] and not want.all()
    for h in (env, twin):
        h.close()


SEED, DRAW = 77, 5


def _stack(E, F, T, per_env=False, seed=11):
    """two Driving handles, extractors, policies and storages with the same parameters"""
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuFeatureExtractor, GpuPolicyHead, GpuRolloutStorage, groups_for
    kw = dict(episodes="per_env") if per_env else {}
    envs = [BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed, **kw) for _ in range(2)]
    for e in envs:
        e.reset_flat()
    env = envs[0]
    Tn, A, D, X = env.n_time_steps, env.n_agents, env.obs_dim, env.action_dim
    types = groups_for(env)["movable"]
    torch.manual_seed(9)
    nets = [GpuFeatureExtractor(types, F, E, A, Tn, D, extended_feature_cnt=X, fixed=True, padded_dtype=torch.bfloat16).requires_grad_(False) for _ in range(2)]
    pols = [GpuPolicyHead(F, env.action_space, seed=SEED, device="cuda").requires_grad_(False) for _ in range(2)]
    with torch.no_grad():
        for m in (nets[0], pols[0]):
            for k, p in m.named_parameters():
                if "bias" in k:
                    p.uniform_(-0.5, 0.5)
    nets[1].load_state_dict(nets[0].state_dict(), strict=True)
    pols[1].load_state_dict(pols[0].state_dict(), strict=True)
    for pol in pols:
        pol.reseed(SEED, DRAW)
    sts = [GpuRolloutStorage(T, E, A, pols[0].action_cols, pols[0].nvec, F, n_probs=sum(pols[0].nvec)) for _ in range(2)]
    return envs, nets, pols, sts


class _Twin(object):
    """the iteration of GpuRollout's docstring, looped eagerly by hand, inserting through the torch fallback"""

    def __init__(self, env, net, pol, st):
        import torch
        self.env, self.net, self.pol, self.st = env, net, pol, st
        E, A, X = env.num_envs, env.n_agents, env.action_dim
        self.acts = torch.zeros((E, A, X), dtype=torch.int32, device="cuda")
        self.ext = torch.zeros((E * A, X), device="cuda")
        self.prev = torch.zeros((E,), dtype=torch.uint8, device="cuda")

    def iteration(self, monkeypatch):
        env = self.env
        feature = self.net(env.obs, self.ext, env.counts(), reset_env=self.prev)
        out = self.pol.act(feature, out_actions=self.acts)
        self.ext.copy_(out.next_ext)
        env.step_flat(self.acts, auto_reset=env.per_env)
        monkeypatch.setenv("DYNENV_ROLLOUT_FUSED", "0")
        self.st.insert(env.rewards, env.agent_finished(), feature, None, out.actions, out.log_probs, out.value, env.dones, out.probs)
        monkeypatch.delenv("DYNENV_ROLLOUT_FUSED")
        assert self.st.last_route == "torch (fallback: DYNENV_ROLLOUT_FUSED=0)"
        self.prev.copy_(env.dones)

    def bootstrap(self, monkeypatch):
        """train.py:284-290 -> final_value, with the state and the counter put back"""
        h, c, d = self.net.h.clone(), self.net.c.clone(), self.pol.draw.clone()
        feature = self.net(self.env.obs, self.ext, self.env.counts(), reset_env=self.prev)
        value = self.pol.act(feature).value
        monkeypatch.setenv("DYNENV_ROLLOUT_FUSED", "0")
        self.st.insert_final(feature)
        monkeypatch.delenv("DYNENV_ROLLOUT_FUSED")
        self.net.h.copy_(h), self.net.c.copy_(c), self.pol.draw.copy_(d)
        return value


def _equal_bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_the_collector_records_one_iteration_and_matches_an_eager_twin(monkeypatch):
    """Driving, E = 16, F = 64, T = 3: step, extractor, policy and insert recorded once with torch.cuda.graph - a capture fails at the
    first host read - and replayed T times; after collect() every storage tensor is bit-identical to the twin's, h, c and the draw
    counter equal the twin's BEFORE its bootstrap, and a second collect() after after_update() continues the twin's trajectory"""
    import torch
    from dynenv_amd import GpuRollout
    E, F, T = 16, 64, 3
    envs, nets, pols, sts = _stack(E, F, T)
    ro = GpuRollout(envs[0], nets[0], pols[0], sts[0])
    twin = _Twin(envs[1], nets[1], pols[1], sts[1])
    ptrs = {k: b.data_ptr() for k, b in sts[0].buffers().items()}
    for r in range(2):
        final = ro.collect()
        assert ro.graph is not None and ro.routes == (("fused", "fused", "fused"), "fused", "fused"), ro.routes
        assert sts[0].last_route == "fused" and int(sts[0].cursor) == T and int(sts[0].status) == 0
        for t in range(T):
            twin.iteration(monkeypatch)
        assert _equal_bits(nets[0].h, nets[1].h) and _equal_bits(nets[0].c, nets[1].c), "rollout %d: the state is the twin's without a bootstrap" % r
        assert int(pols[0].draw) == int(pols[1].draw) == DRAW + T * (r + 1)
        want = twin.bootstrap(monkeypatch)
        assert _equal_bits(final, want), "rollout %d: final_value" % r
        for k, b in sts[0].buffers().items():
            assert _equal_bits(b, sts[1].buffers()[k]), "rollout %d: %s" % (r, k)
        assert _equal_bits(envs[0].obs, envs[1].obs) and torch.equal(ro.static_actions, twin.acts) and torch.equal(ro.ext, twin.ext)
        assert bool(sts[0].features[T].any()) and bool(sts[0].rewards.any()) and bool(sts[0].log_probs.any()) and bool(sts[0].probs.any())
        assert not _equal_bits(sts[0].features[0], sts[0].features[T - 1])
        if r == 0:
            losses = sts[0].a2c_loss(final)
            assert bool(torch.isfinite(losses.loss)) and sts[0].last_returns_route == "fused"
        for st in sts:
            st.after_update()
        assert {k: b.data_ptr() for k, b in sts[0].buffers().items()} == ptrs
    assert envs[0].error_flags() == 0 and envs[1].error_flags() == 0
    # graph=False: the same iteration eagerly, one more rollout on both sides
    eager = GpuRollout(envs[0], nets[0], pols[0], sts[0], graph=False)
    eager.static_actions.copy_(ro.static_actions), eager.ext.copy_(ro.ext), eager.prev_dones.copy_(ro.prev_dones)
    final = eager.collect()
    for t in range(T):
        twin.iteration(monkeypatch)
    assert eager.graph is None and _equal_bits(final, twin.bootstrap(monkeypatch))
    for k, b in sts[0].buffers().items():
        assert _equal_bits(b, sts[1].buffers()[k]), k
    for e in envs:
        e.close()


def test_a_done_inside_a_collected_rollout_cuts_mode_1_for_that_environment_alone(monkeypatch):
    """one per_env handle whose environment 2 is placed two steps before its episode's end by set_states: its done lands at step 1 of
    the recorded rollout - and the step resets it on the device -, the stored dones show it, and the returns of mode 1 differ from mode
    0's at and before that step for that environment's players alone"""
    import torch
    from dynenv_amd import GpuRollout, _capi
    E, F, T, A = 4, 64, 3, 10
    envs, nets, pols, sts = _stack(E, F, T, per_env=True)
    for env in envs:
        blobs = env.get_states().cpu().numpy()
        _capi.blobs_as_states(blobs, env.env_type)["elapsed"][2] = 6000 - 2 * 10
        env.set_states(None, blobs)
    ro = GpuRollout(envs[0], nets[0], pols[0], sts[0])
    twin = _Twin(envs[1], nets[1], pols[1], sts[1])
    final = ro.collect()
    for t in range(T):
        twin.iteration(monkeypatch)
    assert _equal_bits(final, twin.bootstrap(monkeypatch))
    for k, b in sts[0].buffers().items():
        assert _equal_bits(b, sts[1].buffers()[k]), k
    dones = sts[0].dones.cpu().numpy()
    want = np.zeros((T, E), np.float32)
    want[1, 2] = 1
    assert np.array_equal(dones, want)
    assert envs[0].get_state(2).episode == envs[0].get_state(0).episode + 1, "the step reset the environment that ended"
    r0, _ = sts[0].returns(final, mode="reference")
    r1, _ = sts[0].returns(final, mode="dones")
    same = (r0.view(torch.int32) == r1.view(torch.int32)).cpu().numpy()
    players = np.arange(E * A) // A == 2
    assert same[2].all() and same[:, ~players].all() and not same[:2, players].any()
    assert torch.equal(r1[1, 2 * A:3 * A], sts[0].rewards[1, 2 * A:3 * A]), "at the done the return is the reward alone"
    assert envs[0].error_flags() == 0
    for e in envs:
        e.close()
