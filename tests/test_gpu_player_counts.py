"""Every player count the C ABI accepts (-m gpu): Driving with 1..10 cars and RoboCup with 1..5 robots a team, the HIP path against
the oracle bit for bit, on batches whose environments are ON the contact path at that count (tests/player_count_scenes.py; what each
batch reaches is pinned on the oracle alone by tests/test_player_count_scenes.py).

The kernels are not uniform in the player count: the Driving Full observation has a vector writer for A in {2, 6, 10} and a scalar
one for the rest, pairs are enumerated and lanes guarded by `lane < A`, RoboCup splits its teams by `lane < n` and guards bodies by
`lane < 2 R`.  Random play does not touch the solver at small counts within a test's length, so every case here carries a chain of
A cars (a column of 2 n robots) in environment 0, a truncated collision scenario in environment 1 (Driving), a ball that rolls past
the second team's first robot in environment 2 (RoboCup: a ball at rest pays no team reward, and random play does not move it), a
second chain with pedestrians wedged in (a second column) in environment 4, and random play in the rest.

  1. the tour: 12 Driving / 8 RoboCup steps; observations, rewards, dones and every state blob at every step, the episode statistics,
     counts, global state and - for Partial handles - the true Full state at the end;
  2. more players than there are: both sides clamp;
  3. the per-environment calls (get_states / set_states, get_exact / set_exact, the masked step, reset_envs) at 3 and 7 cars and at
     3 and 4 robots a team, from the batch a few steps in: contacts are cached in environments 0, 1 and 4.

No tolerance anywhere: int views of the tensors, or the blobs' bytes."""
import numpy as np
import pytest

import per_env_common as pc
import player_count_scenes as ps
import step_masked_common as sm
from parity_common import _assert_rc_state_equal, _assert_state_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import dynenv_amd
    return dynenv_amd


def _assert_states(c, env, ora, what, envs=None):
    same = _assert_state_equal if pc.driving(c) else _assert_rc_state_equal
    for e in range(ps.E) if envs is None else envs:
        same(env.get_state(e), ora.get_state(e), "%s env %d" % (what, e))


class Both:
    """one HIP handle and one oracle over the same batch, stepped together and compared bit for bit.  Partial handles get a second oracle
    that runs Full observations on the same seed and actions: its observation is the true state full_state_obs() must return."""

    def __init__(self, family, players, **kw):
        self.c = ps.cfg(family, players)
        self.seed = ps.seed_of(family, players)
        self.name = "%s %d" % (family, players)
        self.batch = ps.OracleBatch(self.c, self.seed)
        self.ora = self.batch.ora
        self.truth = ps.OracleBatch(self.c._replace(partial=False), self.seed).ora if self.c.partial else None
        self.env = pc.make(self.c, ps.E, self.seed, **kw)
        self.env.reset_flat()
        for e, st in self.batch.blobs.items():
            self.env.set_state(e, st)
        assert self.env.n_agents == self.ora.A
        self.steps = 0

    def step(self, a):
        """one step on both sides; observations, rewards, dones and all state blobs must be identical"""
        og, rg, dg = pc.step(self.env, a, auto_reset=False)
        oc, rc, dc = self.ora.step(a)
        self.steps += 1
        msg = "%s step %d" % (self.name, self.steps)
        np.testing.assert_array_equal(dg.cpu().numpy(), dc, err_msg=msg + " dones")
        np.testing.assert_array_equal(rg.cpu().numpy(), rc, err_msg=msg + " rewards")
        np.testing.assert_array_equal(og.cpu().numpy(), oc, err_msg=msg + " observations")
        assert pc.same_f64(rg, rc) and pc.same_f32(og, oc), msg + " (a zero's sign)"
        _assert_states(self.c, self.env, self.ora, msg)
        if self.truth:
            full = self.truth.step(a)[0]
            assert pc.same_f32(self.env.full_state_obs(), full[:, -1]), msg + " full_state_obs"

    def run(self, steps, first=0):
        for a in self.batch.actions(steps, first):
            self.step(a)

    def end(self):
        """what is compared once, after the last step"""
        env, ora = self.env, self.ora
        for g, o in zip(env.episode_stats(), ora.episode_stats()):
            np.testing.assert_array_equal(g.cpu().numpy(), o, err_msg=self.name + " episode_stats")
        np.testing.assert_array_equal(env.counts().cpu().numpy(), ora.counts(), err_msg=self.name + " counts")
        if not pc.driving(self.c):
            assert pc.same_f32(env.global_state(), ora.global_state()), self.name + " global_state"
        assert env.error_flags() == 0 and ora.overflow() == 0 and ora.degenerate() == 0, self.name

    def close(self):
        self.env.close()


# ------------------------------------------------------------------------------------------------ 1. the tour
@pytest.mark.parametrize("family,players", ps.TOUR)
def test_tour(gpu, family, players):
    b = Both(family, players)
    b.run(ps.tour_steps(b.c))
    b.end()
    if pc.driving(b.c):
        dc = b.env.debug_counters()
        print("\n%s: A = %d contact = %d split = %d" % (family, players, dc["contact"], dc["split"]))
        assert dc["contact"] > 0, "no substep of this case took the contact path: %s" % dc
        if players == 10:
            assert dc["split"] > 0, "a chain ten levels deep never took the general multi-level solver"
    b.close()


# ------------------------------------------------------------------------------------------------ 2. more players than there are
@pytest.mark.parametrize("family,players", ps.CLAMPED)
def test_too_many_players_are_clamped_on_both_sides(gpu, family, players):
    b = Both(family, players)
    assert b.env.n_agents == b.ora.A == 10
    b.run(4)
    b.end()
    b.close()


# ------------------------------------------------------------------------------------------------ 3. the per-environment calls
WARM = 4   # steps before a per-environment call: the scenes' contacts are cached
M = [1, 2, 4]   # a listed set that splits the scene environments (Driving: 0 | 1, 4; RoboCup: 0 | 2, 4) and the random ones
REST = [e for e in range(ps.E) if e not in M]


def _warm(family, players):
    """a per_env handle and its oracle WARM steps into the batch"""
    b = Both(family, players, episodes="per_env")
    b.run(WARM)
    for e in (ps.CHAIN_ENV, ps.CHAIN2_ENV):
        assert b.ora.active_contacts(e) > 0
    return b


def _eq(a, b):
    import torch
    return bool(torch.equal(a, b))


@pytest.mark.parametrize("family,players", ps.PER_ENV)
def test_get_states_and_set_states(gpu, family, players):
    """get_states() is the get_state(e) loop; the blobs written into a fresh handle (one set_states) and into a fresh oracle (set_state)
    - both start without a contact cache - step identically"""
    b = _warm(family, players)
    c = b.c
    blobs = b.env.get_states().cpu().numpy()
    assert blobs.shape == (ps.E, b.env.state_size)
    for e in range(ps.E):
        assert blobs[e].tobytes() == bytes(b.env.get_state(e)), "get_states row %d is not get_state(%d)" % (e, e)
        _assert_states(c, b.env, b.ora, "before the transfer", [e])
    b.close()
    env = pc.make(c, ps.E, b.seed, episodes="per_env")
    env.reset_flat()
    ora = pc.oracle(c, ps.E, b.seed)
    ora.reset()
    assert env.set_states(None, blobs).cpu().tolist() == [0] * ps.E
    for e in range(ps.E):
        ora.set_state(e, ps.blob_class(c).from_buffer_copy(blobs[e].tobytes()))
    assert env.get_states().cpu().numpy().tobytes() == blobs.tobytes()
    for s, a in enumerate(b.batch.actions(3, WARM)):
        og, rg, dg = pc.step(env, a, auto_reset=False)
        oc, rc, dc = ora.step(a)
        assert pc.same_f32(og, oc) and pc.same_f64(rg, rc) and np.array_equal(dg.cpu().numpy(), dc), "step %d after set_states" % s
        _assert_states(c, env, ora, "step %d after set_states" % s)
    assert ora.active_contacts(ps.CHAIN_ENV) > 0 and env.error_flags() == 0 and ora.overflow() == 0
    env.close()


@pytest.mark.parametrize("family,players", ps.PER_ENV)
def test_get_exact_and_set_exact(gpu, family, players):
    """three steps, restore, the same three steps: outputs and final blobs are the first run's - and the oracle's, which just went on"""
    b = _warm(family, players)
    saved = b.env.get_exact().clone()
    assert tuple(saved.shape) == (ps.E, b.env.exact_size)
    acts = b.batch.actions(3, WARM)
    first = []
    for a in acts:
        b.step(a)   # (against the oracle)
        first.append(sm.outputs(b.env))
    end = b.env.get_exact().clone()
    assert not _eq(end, saved)
    assert b.env.set_exact(None, saved).cpu().tolist() == [0] * ps.E
    assert _eq(b.env.get_exact(), saved)
    for s, a in enumerate(acts):
        pc.step(b.env, a, auto_reset=False)
        assert sm.same_outputs(first[s], sm.outputs(b.env)) == "", "replayed step %d" % s
    assert _eq(b.env.get_exact(), end), "the replay ends where the first pass ended"
    _assert_states(b.c, b.env, b.ora, "after the replay")
    b.end()
    b.close()


@pytest.mark.parametrize("family,players", ps.PER_ENV)
def test_a_masked_step_and_its_complement_are_one_plain_step(gpu, family, players):
    a, b = _warm(family, players), _warm(family, players)
    assert pc.ckpt_diff(a.env, b.env) == "", "same configuration, same history"
    act = a.batch.actions(1, WARM)[0]
    a.step(act)   # the plain step (against the oracle)
    want = sm.outputs(a.env)
    sm.fill_sentinels(b.env)
    frozen = b.env.get_exact(REST).clone()
    pc.step(b.env, act, auto_reset=False, active=M)
    mid = sm.outputs(b.env)
    assert sm.rows_are_sentinel(mid, REST), "output rows of unlisted environments were written"
    assert _eq(b.env.get_exact(REST), frozen), "an unlisted environment changed"
    assert sm.same_outputs(mid, want, rows=M) == ""
    pc.step(b.env, act, auto_reset=False, active=sm.mask_tensor(ps.E, REST))
    assert sm.same_outputs(sm.outputs(b.env), want) == ""
    assert _eq(a.env.get_exact(), b.env.get_exact()) and pc.ckpt_diff(a.env, b.env) == ""
    assert a.env.error_flags() == b.env.error_flags() == 0
    a.close()
    b.close()


@pytest.mark.parametrize("family,players", ps.PER_ENV)
def test_reset_envs_of_a_subset(gpu, family, players):
    """the listed environments - the second chain / column with its live contacts among them - are per-environment oracles reset into
    the same episode, and play on like them; the unlisted ones keep every byte of their exact blob"""
    b = _warm(family, players)
    c = b.c
    frozen = b.env.get_exact(REST).clone()
    sm.fill_sentinels(b.env)
    obs = b.env.reset_envs(M)
    assert _eq(b.env.get_exact(REST), frozen), "an unlisted environment changed"
    assert (pc.bits32(obs)[REST] == sm.OBS_SENTINEL).all(), "observation rows of unlisted environments were written"
    ora = {e: pc.env_oracle(c, e, b.seed) for e in M}
    for e in M:
        ora[e].reset()                                     # episode 1: where the batch started
        assert pc.same_f32(obs[e], ora[e].reset()[0]), "the reset observation of environment %d" % e   # episode 2
        st = b.env.get_state(e)
        assert st.elapsed == 0 and st.episode == 2
        (_assert_state_equal if pc.driving(c) else _assert_rc_state_equal)(st, ora[e].get_state(0), "reset environment %d" % e)
    for s, act in enumerate(pc.actions(c, ps.E, b.env.n_agents, 3, b.seed + 50)):
        og, rg, dg = pc.step(b.env, act, auto_reset=False, active=M)
        for e in M:
            oc, rc, dc = ora[e].step(act[e:e + 1])
            assert pc.same_f32(og[e], oc[0]) and pc.same_f64(rg[e], rc[0]) and int(dg[e]) == dc[0], "environment %d, step %d of its next episode" % (e, s)
    assert _eq(b.env.get_exact(REST), frozen)
    assert b.env.error_flags() == 0
    b.close()
