"""CPU checks of the rollout storage (dynenv_amd/rollout.py) against the reference's own RolloutStorage: its recorded results
(tests/golden/rollout_storage.json, written by tests/golden/gen_golden_rollout_storage.py) and, where the reference is on the machine, the
live class; against the numpy statements of tests/rollout_ref.py; and the properties of the two return modes the reference does not have."""
import os

import numpy as np
import pytest

import rollout_ref as RR

HAVE_REFERENCE = os.path.exists(RR.REF_STORAGE) and os.path.exists(RR.REF_LOSSES)
live = pytest.mark.skipif(not HAVE_REFERENCE, reason="the reference is not on this machine")
FIELDS = ("loss", "policy", "value", "entropy", "temp_entropy")


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.fixture(scope="module")
def golden():
    cases = RR.load_golden()
    for c in cases:   # the inputs are the case maker's: the file records their words
        steps, final = RR.golden_case(c["T"], c["E"], c["A"], tuple(c["groups"]), c["F"], c["seed"])
        assert RR.bits(final) == c["inputs"]["final_value"]
        for s, w in zip(steps, c["inputs"]["steps"]):
            for k in ("rewards", "feat0", "log_probs", "log_probs_old", "value", "probs"):
                assert RR.bits(s[k]) == w[k], k
            assert s["finished"].reshape(-1).tolist() == w["finished"] and s["actions"].reshape(-1).tolist() == w["actions"] and s["dones"].tolist() == w["dones"]
        c["steps"], c["final"] = steps, final
    return cases


def _storage(c, steps=None, device="cpu", grad=False):
    """the module's storage after its own insert of every step"""
    from dynenv_amd import GpuRolloutStorage
    groups = tuple(c["groups"])
    st = GpuRolloutStorage(c["T"], c["E"], c["A"], len(groups), groups, c["F"], n_probs=sum(groups), use_full_entropy=c["use_full_entropy"],
                           use_ppo=c["use_ppo"], device=device)
    for s in (steps if steps is not None else c["steps"]):
        st.insert(_t(s["rewards"]), _t(s["finished"]), _t(s["feat0"]), None, _t(s["actions"]), _t(s["log_probs"]), _t(s["value"]), _t(s["dones"]),
                  probs=_t(s["probs"]), log_probs_old=_t(s["log_probs_old"]) if c["use_ppo"] else None)
        assert st.last_route == "torch (fallback: a storage that is not on the device)"
    assert int(st.cursor) == c["T"] and int(st.status) == 0
    return st


def _numpy_buffers(c):
    groups = tuple(c["groups"])
    bufs = RR.make_buffers(c["T"], c["E"], c["A"], c["F"], len(groups), len(groups), sum(groups), ppo=c["use_ppo"])
    for t, s in enumerate(c["steps"]):
        RR.insert_row(bufs, t, **{k: v for k, v in s.items() if k != "log_probs_old" or c["use_ppo"]})
    return bufs


def test_insert_on_the_cpu_is_the_numpy_statement(golden):
    for c in golden:
        st, bufs = _storage(c), _numpy_buffers(c)
        for k, want in bufs.items():
            got = getattr(st, k).numpy()
            assert got.dtype == (np.bool_ if k == "agentFinished" else np.float32) and got.shape == want.shape, k
            assert np.array_equal(got.view(np.uint8) if k == "agentFinished" else got.view(np.uint32), want if k == "agentFinished" else want.view(np.uint32)), k
        assert st.log_probs_old is None or c["use_ppo"]


def test_mode_0_is_the_recorded_discount_rewards_bit_for_bit(golden):
    from dynenv_amd import rollout
    for c in golden:
        T, P = c["T"], c["E"] * c["A"]
        want = np.array(c["returns"], np.uint32).reshape(T, P)
        bufs = _numpy_buffers(c)
        ret, adv = RR.returns(bufs["rewards"], bufs["values"], bufs["dones"], c["final"], c["A"])
        assert np.array_equal(ret.view(np.uint32), want), "the numpy statement"
        st = _storage(c)
        got, got_adv = st.returns(_t(c["final"]).view(-1, 1))
        assert st.last_returns_route.startswith("torch (fallback")
        assert np.array_equal(got.numpy().view(np.uint32), want), "the module's torch statements"
        assert np.array_equal(got_adv.numpy().view(np.uint32), adv.view(np.uint32))
        assert np.array_equal(RR.bits(st.rewards.numpy()), c["stored_rewards"])
        r2, _ = rollout.returns_torch(st.rewards, st.values, st.dones, _t(c["final"]), c["A"])
        assert np.array_equal(r2.numpy().view(np.uint32), want)


@live
def test_mode_0_and_the_loss_are_the_live_reference_bit_for_bit(golden):
    """the same operations in the same order on the same machine: every field of the reference's A2CLosses, the returned rewards and
    _discount_rewards equal the module's bit for bit, for the reference's list of action_probs and for the stored probs alike"""
    import torch
    cls = RR.reference_class()
    for c in golden:
        groups = tuple(c["groups"])
        ref, action_probs = RR.reference_filled(cls, c["steps"], c["E"], c["A"], groups, c["F"], c["use_ppo"], c["use_full_entropy"])
        final = _t(c["final"]).view(-1, 1)
        st = _storage(c)
        for k in ("rewards", "agentFinished", "features", "actions", "log_probs", "values", "dones"):
            assert torch.equal(getattr(ref, k), getattr(st, k)), k
        assert torch.equal(ref._discount_rewards(final), st.returns(final)[0])
        want, rewards = ref.a2c_loss(final, action_probs, c["value_coeff"], c["entropy_coeff"])
        for probs in (action_probs, None):
            got = st.a2c_loss(final, probs, c["value_coeff"], c["entropy_coeff"])
            assert np.float32(got.loss.item()).view(np.uint32) == np.float32(want.loss.item()).view(np.uint32)
            for k in FIELDS[1:]:
                assert float(getattr(got, k)) == getattr(want, k), k
            assert torch.equal(got.rewards, rewards)


def test_the_loss_matches_the_recorded_results_and_the_float64_statement_within_the_derived_bound(golden):
    """The bound is derived, not picked (rollout_ref.mean_bound, _entropy, a2c_loss).  With U = 2^-24: a float32 mean of n terms summed
    in any order lies within n U mean|term| of the exact mean to first order, plus one U per float32 operation that formed a term: the
    policy term one product (PPO: difference, exp, + delta, clamp, product: 7), the value term the difference - counted twice by the
    square - and the square.  An entropy takes probabilities that are means of T or P positive terms (relative T U or P U), normalises
    them (the sum of n_g terms and a division), takes one rounding of a log per term (two units allowed) and sums n_g products; the
    conditioning of -p log p is |log p| + 1.  A mean of means adds its own n U mean|term|, a coefficient one U, the sum of the four
    fields 4 U of their magnitudes.  Both float32 evaluations - the module's here and the reference's recorded one - must lie within
    the bound of the float64 statement, hence within twice the bound of each other.  The measured distances are printed beside it."""
    for c in golden:
        st = _storage(c)
        T, P = c["T"], c["E"] * c["A"]
        ret, adv = RR.returns(st.rewards.numpy(), st.values.numpy(), st.dones.numpy(), c["final"], c["A"])
        ref = RR.a2c_loss(ret, adv, st.values.numpy(), st.log_probs.numpy(), st.probs.numpy(), c["groups"], c["value_coeff"], c["entropy_coeff"],
                          c["use_full_entropy"], st.log_probs_old.numpy() if c["use_ppo"] else None)
        got = st.a2c_loss(_t(c["final"]), None, c["value_coeff"], c["entropy_coeff"])
        for k in FIELDS:
            exact, bound = getattr(ref, k), ref.bound[k]
            mine, recorded = float(getattr(got, k)), float(RR.from_bits([c[k]], (1,))[0])
            print("T=%d ppo=%d full=%d %-12s exact %+.9e  module %.3g  recorded %.3g  module-recorded %.3g  bound %.3g" % (
                T, c["use_ppo"], c["use_full_entropy"], k, exact, abs(mine - exact), abs(recorded - exact), abs(mine - recorded), bound))
            assert 0 < bound < 1e-4 * max(abs(exact), 1e-2), "a bound that bounds nothing"
            assert abs(mine - exact) <= bound and abs(recorded - exact) <= bound and abs(mine - recorded) <= 2 * bound, k


def _hand(rewards, values, dones, final, A=1):
    f = lambda x: np.array(x, np.float32)
    return f(rewards), f(values), f(dones), f(final), A


def test_a_done_cuts_the_chain_exactly_there_and_without_dones_mode_1_is_mode_0():
    rng = np.random.default_rng(3)
    T, E, A = 6, 3, 2
    P = E * A
    rewards, values = rng.standard_normal((T, P)).astype(np.float32), rng.standard_normal((T, P)).astype(np.float32)
    final = rng.standard_normal(P).astype(np.float32)
    none = np.zeros((T, E), np.float32)
    r0, a0 = RR.returns(rewards, values, none, final, A, mode="reference")
    r1, a1 = RR.returns(rewards, values, none, final, A, mode="dones")
    assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32)) and np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    dones = none.copy()
    dones[3, 1] = 1   # environment 1 ends at step 3
    rd, _ = RR.returns(rewards, values, dones, final, A, mode="dones")
    rg, ag = RR.returns(rewards, values, dones, final, A, mode="gae")
    cut = slice(2, 4)   # environment 1's players
    # at and before the done the chain restarts from the reward alone: the rollout [0..3] of that environment with final_value 0 ...
    rs, _ = RR.returns(rewards[:4], values[:4], none[:4], np.zeros(P, np.float32), A, mode="dones")
    assert np.array_equal(rd[:4, cut].view(np.uint32), rs[:4, cut].view(np.uint32))
    assert np.array_equal(rd[3, cut], rewards[3, cut])
    # ... behind it, and for the other environments, nothing changes
    assert np.array_equal(rd[4:].view(np.uint32), r0[4:].view(np.uint32))
    others = [0, 1, 4, 5]
    assert np.array_equal(rd[:, others].view(np.uint32), r0[:, others].view(np.uint32)) and not np.array_equal(rd[:3, cut], r0[:3, cut])
    gs, as_ = RR.returns(rewards[:4], values[:4], none[:4], np.zeros(P, np.float32), A, mode="gae")
    assert np.array_equal(ag[:4, cut].view(np.uint32), as_[:4, cut].view(np.uint32)) and np.array_equal(rg[:4, cut].view(np.uint32), gs[:4, cut].view(np.uint32))
    assert np.array_equal(ag[3, cut], rewards[3, cut] - values[3, cut])
    # the module's torch statements are the numpy statements bit for bit, in every mode
    from dynenv_amd import rollout
    for mode in ("reference", "dones", "gae"):
        want = RR.returns(rewards, values, dones, final, A, 0.97, mode, 0.9)
        got = rollout.returns_torch(_t(rewards), _t(values), _t(dones), _t(final), A, 0.97, mode, 0.9)
        for w, g in zip(want, got):
            assert np.array_equal(w.view(np.uint32), g.numpy().view(np.uint32)), mode


def test_the_gae_identities_on_hand_made_two_step_inputs():
    """values exactly representable, gamma = 0.5: every product below is exact, so the identities hold bit for bit.
    lambda = 1: returns are the discounted returns of mode 1; lambda = 0: the advantage is the one-step TD error"""
    rewards, values, dones, final, A = _hand([[1.0, 2.0], [3.0, -1.0]], [[0.5, 0.25], [2.0, 4.0]], [[0.0, 0.0], [0.0, 0.0]], [8.0, -4.0])
    r1, _ = RR.returns(rewards, values, dones, final, A, 0.5, "dones")
    assert r1.tolist() == [[1 + 0.5 * (3 + 0.5 * 8), 2 + 0.5 * (-1 + 0.5 * -4)], [3 + 0.5 * 8, -1 + 0.5 * -4]]
    rg, ag = RR.returns(rewards, values, dones, final, A, 0.5, "gae", 1.0)
    assert np.array_equal(rg, r1) and np.array_equal(ag, r1 - values)
    rg, ag = RR.returns(rewards, values, dones, final, A, 0.5, "gae", 0.0)
    td = np.array([[1 + 0.5 * 2.0 - 0.5, 2 + 0.5 * 4.0 - 0.25], [3 + 0.5 * 8 - 2.0, -1 + 0.5 * -4 - 4.0]], np.float32)
    assert np.array_equal(ag, td) and np.array_equal(rg, td + values)
    # a done at the last step: the bootstrap value is not used; at the first step: the second step's advantage does not flow back
    dones = np.array([[0.0, 1.0], [1.0, 0.0]], np.float32)
    rg, ag = RR.returns(rewards, values, dones, final, A, 0.5, "gae", 1.0)
    assert ag[1].tolist() == [3 - 2.0, -1 + 0.5 * -4 - 4.0] and ag[0].tolist() == [1 + 0.5 * 2.0 - 0.5 + 0.5 * ag[1, 0], 2 - 0.25]
    r1, _ = RR.returns(rewards, values, dones, final, A, 0.5, "dones")
    assert r1.tolist() == [[1 + 0.5 * 3, 2.0], [3.0, -1 + 0.5 * -4]]
    # and the module's torch statements give the same on the same inputs
    from dynenv_amd import rollout
    tr, ta = rollout.returns_torch(_t(rewards), _t(values), _t(dones), _t(final), A, 0.5, "gae", 1.0)
    assert np.array_equal(tr.numpy(), rg) and np.array_equal(ta.numpy(), ag)
    assert np.array_equal(rollout.returns_torch(_t(rewards), _t(values), _t(dones), _t(final), A, 0.5, "dones")[0].numpy(), r1)


def test_the_torch_route_passes_a_gradient_through_log_probs_and_values():
    """insert() of tensors that carry a gradient takes the "torch" route on any device; d loss / d (log_probs, value) of a2c_loss equal a
    float64 twin's - the same statements on float64 leaves through the numpy-indexed buffers - to 1e-5 of the largest entry: the float32
    backward of sums of T * P = 30 terms (30 U = 2e-6, and the chain through the mean and the square a few units more)"""
    import torch
    from dynenv_amd import GpuRolloutStorage
    T, E, A, groups, F = 5, 3, 2, (3, 3), 8
    P, G = E * A, len(groups)
    steps, final = RR.golden_case(T, E, A, groups, F, 7)
    st = GpuRolloutStorage(T, E, A, G, groups, F, n_probs=sum(groups), device="cpu")
    leaves = []
    for s in steps:
        lp, v = _t(s["log_probs"]).requires_grad_(True), _t(s["value"]).view(P, 1).requires_grad_(True)
        leaves.append((lp, v))
        st.insert(_t(s["rewards"]), _t(s["finished"]), _t(s["feat0"]), None, _t(s["actions"]), lp, v, _t(s["dones"]), probs=_t(s["probs"]))
        assert st.last_route == "torch"
    out = st.a2c_loss(_t(final), None, 0.5, 0.1)
    out.loss.backward()
    # the twin: float64 leaves, the buffers assembled by indexing, the loss's statements
    lp64 = [_t(s["log_probs"]).double().requires_grad_(True) for s in steps]
    v64 = [_t(s["value"]).double().requires_grad_(True) for s in steps]
    log_probs, values = torch.stack([x.t() for x in lp64]), torch.stack(v64)
    ret = st.returns(_t(final))[0].double()
    advantage = ret - values
    policy = torch.stack([(-log_probs[:, g] * advantage.detach()).mean() for g in range(G)]).mean()
    (policy + 0.5 * advantage.pow(2).mean()).backward()
    for (lp, v), a, b in zip(leaves, lp64, v64):
        for got, want in ((lp.grad, a.grad), (v.grad.view(-1), b.grad)):
            scale = float(want.abs().max())
            assert scale > 0 and float((got.double() - want).abs().max()) <= 1e-5 * scale
    ptrs = {k: b.data_ptr() for k, b in st.buffers().items()}
    st.after_update()
    assert {k: b.data_ptr() for k, b in st.buffers().items()} == ptrs and all(b.grad_fn is None and not b.any() for b in st.buffers().values())
    assert int(st.cursor) == 0


def test_a_cursor_outside_the_rollout_writes_nothing_but_the_status_word():
    c = dict(T=2, E=2, A=2, groups=[3, 3], F=4, use_ppo=True, use_full_entropy=False)
    steps, _ = RR.golden_case(3, 2, 2, (3, 3), 4, 5)
    st = _storage(c, steps[:2])
    before = {k: b.clone() for k, b in st.buffers().items()}
    s = steps[2]
    st.insert(_t(s["rewards"]), _t(s["finished"]), _t(s["feat0"]), None, _t(s["actions"]), _t(s["log_probs"]), _t(s["value"]), _t(s["dones"]),
              probs=_t(s["probs"]), log_probs_old=_t(s["log_probs_old"]))
    assert int(st.status) == 1 and all((before[k] == b).all() for k, b in st.buffers().items())
    st.status.zero_()
    st.cursor.fill_(2)
    st.insert_final(_t(s["feat0"]))
    assert int(st.status) == 0 and (st.features[2] == _t(s["feat0"])).all() and (st.features[:2] == before["features"][:2]).all()
    st.cursor.fill_(-1)
    st.insert_final(_t(steps[0]["feat0"]))
    assert int(st.status) == 1 and (st.features[2] == _t(s["feat0"])).all() and (st.features[:2] == before["features"][:2]).all()
