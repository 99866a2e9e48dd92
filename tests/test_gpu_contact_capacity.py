"""The contact paths at the capacity of their fixed tables (-m gpu): the HIP path against the oracle on the scenes of
tests/capacity_scenes.py, whose preconditions tests/test_capacity_scenes.py establishes on the oracle alone.

An environment's arbiters live in DRV_NS = 24 / RC_NS = 16 slots, a substep's candidate pairs in a list of 128 that goes through the
narrowphase in passes of 16 / 64.  At or below these limits every observation, reward, done flag and state blob must be the oracle's
bit for bit; one above them a pair is dropped and error bit 0 is raised on that environment - reported, sticky, and contained: its
neighbours (whose LDS tile and HBM rows an overrun would hit) stay the oracle's, and a whole-handle checkpoint differs from a twin
handle's in that environment's rows only.

Every test uses one handle of 8 environments and 6 to 12 steps; the scenes go into some environments through set_state / set_states,
the others keep their reset state and play randomly.  RoboCup has no scene for a second narrowphase pass (see
tests/test_capacity_scenes.py)."""
import ctypes as C

import numpy as np
import pytest

import capacity_scenes as cs
import oracle_lib as ol
from parity_common import _assert_rc_state_equal, _assert_state_equal, _rc_actions

pytestmark = pytest.mark.gpu

E = 8
DRV, RC = "driving", "robocup"


@pytest.fixture(scope="module")
def gpu(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import dynenv_amd
    return dynenv_amd


class Pair:
    """one HIP handle and one oracle over the same 8 environments, stepped together and compared bit for bit"""

    def __init__(self, gpu, kind, seed=21, flags=ol.ROBOCUP_DEFAULT_FLAGS, num_envs=E, oracle=True):
        self.kind, self.E = kind, num_envs
        if kind == DRV:
            self.env = gpu.BatchedDynEnv(gpu.DynEnvType.DRIVE, num_envs, 10, seed=seed)
            self.ora = ol.OracleEnv(num_envs=num_envs, n_players=10, seed=seed, threads=4) if oracle else None
        else:
            self.env = gpu.BatchedDynEnv(gpu.DynEnvType.ROBO_CUP, num_envs, 5, seed=seed, flags=flags)
            self.ora = ol.OracleEnv(env_type=0, num_envs=num_envs, n_players=5, seed=seed, flags=flags, threads=4) if oracle else None
        self.env.reset_flat()
        self.ref = ol.OracleEnv(num_envs=1, n_players=10, seed=seed) if kind == DRV else \
            ol.OracleEnv(env_type=0, num_envs=1, n_players=5, seed=seed, flags=flags)   # a source of blank blobs when there is no oracle
        self.ref.reset()
        if self.ora:
            self.ora.reset()
        self.rng = np.random.default_rng(seed)
        self.scene_envs = set()
        self.steps = 0

    def blob(self, scene, **kw):
        st = self.ref.get_state(0)
        scene(st, **kw)
        return st

    def put(self, e, st, batched=False):
        """the blob goes into environment e of both sides: set_state, or set_states (one launch, device side); it takes the batch's
        position in the (lock-step) episode"""
        st.elapsed = self.steps * (10 if self.kind == DRV else 50)
        if batched:
            row = np.frombuffer(bytes(st), np.uint8).reshape(1, -1).copy()
            status = self.env.set_states([e], row)
            assert status.cpu().numpy().tolist() == [0]
        else:
            self.env.set_state(e, st)
        if self.ora:
            self.ora.set_state(e, st)
        self.scene_envs.add(e)

    def actions(self):
        if self.kind == DRV:
            a = self.rng.integers(0, 3, size=(self.E, 10, 2)).astype(np.int32)
            for e in self.scene_envs:
                a[e] = 1
        else:
            a = _rc_actions(self.rng, self.E, 10)
            for e in self.scene_envs:
                a[e] = cs_idle()
        return a

    def step(self, compare=None, what=""):
        """one step on both sides; observations, rewards, dones and the state blobs of `compare` (default: all) must be identical"""
        a = self.actions()
        og, rg, dg = self.env.step_flat(a, auto_reset=False)
        self.steps += 1
        if not self.ora:
            return
        oc, rc, dc = self.ora.step(a)
        envs = list(range(self.E)) if compare is None else list(compare)
        msg = "%s step %d" % (what, self.steps)
        np.testing.assert_array_equal(dg.cpu().numpy(), dc, err_msg=msg + " dones")
        np.testing.assert_array_equal(rg.cpu().numpy()[envs], rc[envs], err_msg=msg + " rewards")
        np.testing.assert_array_equal(og.cpu().numpy()[envs], oc[envs], err_msg=msg + " observations")
        for e in envs:
            (_assert_state_equal if self.kind == DRV else _assert_rc_state_equal)(self.env.get_state(e), self.ora.get_state(e), msg + " env %d" % e)

    def flags(self):
        return self.env.error_flags_per_env().cpu().numpy().tolist()

    def close(self):
        self.env.close()


def cs_idle():
    a = np.zeros((10, 4), np.int32)
    a[:, 3] = 3   # nobody walks, turns or kicks; no head turn
    return a


SCENES = {  # name -> (kind, full scene, over scene, table size, RoboCup flags)
    "drv_isolated": (DRV, cs.drv_full, cs.drv_over, cs.DRV_NS, None),
    "drv_coupled": (DRV, cs.drv_full_coupled, cs.drv_over_coupled, cs.DRV_NS, None),
    "rc_resting": (RC, cs.rc_full, cs.rc_over, cs.RC_NS, 8),                          # the fall dice off: all arbiters rest
    "rc_falling": (RC, cs.rc_full, cs.rc_over, cs.RC_NS, ol.ROBOCUP_DEFAULT_FLAGS),   # robots knock each other over while the table is full
}


# ------------------------------------------------------------------------------------------------ the full table
@pytest.mark.parametrize("name", sorted(SCENES))
def test_full_table_is_still_the_oracles(gpu, name):
    kind, full, _, NS, flags = SCENES[name]
    p = Pair(gpu, kind, flags=flags)
    st = p.blob(full)
    p.put(1, st)
    p.put(4, st, batched=True)
    p.put(6, st, batched=True)
    for s in range(8):
        p.step(what=name)
    assert p.flags() == [0] * E and p.env.error_flags() == 0 and p.ora.overflow() == 0
    for e in (1, 4, 6):
        assert p.ora.peak_arbiters(e) == NS, "the scene must fill the table exactly (environment %d: %d)" % (e, p.ora.peak_arbiters(e))
    assert p.ora.degenerate() == 0
    p.close()


def test_full_driving_table_in_every_substep(gpu):
    """slot_sum adds the number of occupied slots at the start of every substep (before that substep's narrowphase hands out any):
    0 in the first substep after set_state, then 24 in each of the other 59 - only a table that is full all the time gets there, and no
    substep with an occupied slot may take the `fast` path."""
    p = Pair(gpu, DRV, num_envs=1)
    p.put(0, p.blob(cs.drv_full))
    steps = 6
    for s in range(steps):
        p.step(what="drv_full alone")
    dc = p.env.debug_counters()
    assert dc["slot_sum"] == cs.DRV_NS * (10 * steps - 1), dc
    assert dc["fast"] == 0 and dc["contact"] >= 1, dc
    assert dc["fast"] + dc["quiescent"] + dc["contact"] + dc["steady"] == 10 * steps, dc
    assert p.env.error_flags() == 0 and p.ora.peak_arbiters(0) == cs.DRV_NS
    p.close()


# ------------------------------------------------------------------------------------------------ one too many
def _checkpoint_owner(ck, kind):
    """which environment owns each byte of a whole-handle checkpoint of an 8-environment handle (-1: the header and arrays that belong to
    no environment).  The payload is the handle's device arrays in allocation order (dynenv_host.h: that order is the checkpoint format),
    each [planes][E][row]: (planes, bytes of a row); one row size per kind is left open (None) and follows from the payload's size."""
    if kind == DRV:   # driving_tu.hip: body, carx, flags, aux, obst, envi, epr, s_pair, s_meta, s_hash, s_imp, lastcand
        arrays = [(9, 32 * 8), (6, 16 * 8), (1, 32 * 4), (1, 32 * 4), (2, 20 * 8), (1, None), (2, 16 * 8), (1, 24 * 4), (1, 24 * 4), (2, 24 * 4),
                  (4, 24 * 8), (1, 64 * 4)]
        tail = 0
    else:             # robocup_host.hip: body, rob, robi, envi, envd, epr, epo, snap, prew0, s_pair, s_meta, s_hash, s_imp; then pairTab
        arrays = [(16, 32 * 8), (12, 16 * 8), (3, 16 * 4), (1, 40 * 4), (1, 8 * 8), (2, 16 * 8), (1, 16 * 8), (1, None), (1, 16 * 8), (1, 16 * 4),
                  (1, 16 * 4), (2, 16 * 4), (4, 16 * 8)]
        tail = 64 * 2 * 8
    header = C.sizeof(ol.Cfg) + 24
    payload = len(ck) - header
    assert int(np.frombuffer(ck[header - 8:header].tobytes(), np.uint64)[0]) == payload, "checkpoint header: update _checkpoint_owner"
    known = sum(pl * E * row for pl, row in arrays if row is not None) + tail
    rest = payload - known
    assert rest > 0 and rest % (E * 4) == 0, "checkpoint layout: update _checkpoint_owner (%d bytes left for the open array)" % rest
    owner = [np.full(header, -1, np.int8)]
    for pl, row in arrays:
        row = rest // E if row is None else row
        owner.append(np.tile(np.repeat(np.arange(E, dtype=np.int8), row), pl))
    owner.append(np.full(tail, -1, np.int8))
    owner = np.concatenate(owner)
    assert owner.size == len(ck)
    return owner


def _assert_valid_blob(kind, st, like, elapsed):
    """finite and structurally what went in"""
    if kind == DRV:
        assert (st.n_cars, st.n_peds, st.n_obst, st.elapsed) == (like.n_cars, like.n_peds, like.n_obst, elapsed)
        d = ol.state_to_dict(st)
        for k in ("cars_f", "peds_f", "obst", "episode_r", "episode_pos_r"):
            assert np.isfinite(d[k]).all(), k
        assert (np.abs(d["cars_f"][:, :2]) < 4000.0).all() and (d["cars_i"][:, 0] == [like.cars[k].type for k in range(10)]).all()
    else:
        assert (st.n_robots, st.elapsed) == (like.n_robots, elapsed)
        d = ol.rc_state_to_dict(st)
        for k in ("robots_f", "floats", "episode_r", "episode_pos_r"):
            assert np.isfinite(d[k]).all(), k
        assert (np.abs(d["robots_f"][:, :2]) < 4000.0).all()


@pytest.mark.parametrize("name", ["drv_isolated", "drv_coupled", "rc_resting"])
def test_one_arbiter_too_many_is_reported_and_contained(gpu, name):
    kind, full, over, NS, flags = SCENES[name]
    sub = 10 if kind == DRV else 50
    p = Pair(gpu, kind, flags=flags)                       # environment 3 runs one arbiter too many between two full tables
    twin = Pair(gpu, kind, flags=flags, oracle=False)      # the same with a full table in environment 3
    st_full, st_over = p.blob(full), p.blob(over)
    for q, st3 in ((p, st_over), (twin, st_full)):
        q.put(2, st_full)
        q.put(3, st3)
        q.put(4, st_full, batched=True)
    others = [e for e in range(E) if e != 3]
    want = [0, 0, 0, 1, 0, 0, 0, 0]
    for s in range(4):
        p.step(compare=others, what=name)
        twin.step()
        assert p.flags() == want, "bit 0 on environment 3 alone, from the first step on, sticky (step %d)" % s
        _assert_valid_blob(kind, p.env.get_state(3), st_over, sub * (s + 1))
    assert p.env.error_flags() == 1 and twin.flags() == [0] * E
    assert p.ora.peak_arbiters(3) == NS + 1 and p.ora.peak_arbiters(2) == NS and p.ora.peak_arbiters(4) == NS
    # whole-handle checkpoints, byte for byte: the two handles differ in environment 3's rows only
    ck, ck_twin = p.env.checkpoint(), twin.env.checkpoint()
    owner = _checkpoint_owner(ck, kind)
    diff = np.nonzero(ck != ck_twin)[0]
    assert diff.size > 0, "the error word of environment 3 differs at the least"
    assert set(owner[diff].tolist()) == {3}, "bytes outside environment 3's rows differ: owners %s" % sorted(set(owner[diff].tolist()))
    twin.close()
    # set_state clears the bit and leaves no persistent structure inconsistent: environment 3 is the oracle's again, bit for bit
    p.put(3, st_full)
    assert p.flags() == [0] * E
    for s in range(4):
        p.step(what=name + " after set_state")
    assert p.flags() == [0] * E and p.ora.peak_arbiters(3) == NS
    # ... and so does reset
    p.put(3, st_over)
    p.step(compare=others, what=name + " over again")
    assert p.flags() == want
    og = p.env.reset_flat().cpu().numpy()
    oc = p.ora.reset()
    assert p.flags() == [0] * E
    np.testing.assert_array_equal(og, oc)
    p.scene_envs.clear()
    p.step(what=name + " after reset")
    assert p.flags() == [0] * E
    p.close()


@pytest.mark.parametrize("name", ["drv_isolated", "rc_resting"])
def test_compat_step_raises_on_a_dropped_pair(gpu, name):
    """a dropped pair means the state is not the reference's any more: the compat step() raises and names the environment, like bits 3
    to 6; step_flat() leaves the check to the caller"""
    from dynenv_amd import _capi
    kind, full, over, NS, flags = SCENES[name]
    p = Pair(gpu, kind, flags=flags, oracle=False)
    p.env.reset()
    p.put(3, p.blob(over))
    p.put(5, p.blob(full))
    a = p.actions()
    with pytest.raises(_capi.DynEnvError, match=r"error bit 0.*environment 3\b"):
        p.env.step(a.astype(np.int64))
    assert p.flags() == [0, 0, 0, 1, 0, 0, 0, 0]
    p.env.step_flat(p.actions(), auto_reset=False)   # no check here: the caller's
    assert p.flags() == [0, 0, 0, 1, 0, 0, 0, 0]
    p.put(3, p.blob(full))
    obs, rew, dones, infos = p.env.step(p.actions().astype(np.int64))   # repaired: steps again
    assert rew.shape == (E, 10) and p.flags() == [0] * E
    p.close()


# ------------------------------------------------------------------------------------------------ the candidate list
def test_candidate_list_at_and_past_128(gpu):
    """128 candidates fill the list to its last entry - and that entry is the pair that touches; with 129 that pair is the one that
    does not fit (the flag is asserted, not a difference: a dropped pair that did not touch would change nothing)"""
    p = Pair(gpu, DRV)
    p.put(5, p.blob(cs.drv_clist))
    p.put(6, p.blob(cs.drv_clist), batched=True)
    p.put(3, p.blob(cs.drv_clist, over=True))
    others = [e for e in range(E) if e != 3]
    for s in range(6):
        p.step(compare=others, what="drv_clist")
        assert p.flags() == [0, 0, 0, 1, 0, 0, 0, 0], "step %d" % s
    for e in (3, 5, 6):
        assert p.ora.peak_arbiters(e) == 2 and p.ora.active_contacts(e) == 2
    assert len(cs.drv_candidates(p.ora.get_state(5))) == 128 and len(cs.drv_candidates(p.ora.get_state(3))) == 129
    _assert_valid_blob(DRV, p.env.get_state(3), p.blob(cs.drv_clist, over=True), 60)
    p.put(3, p.blob(cs.drv_clist))   # back to 128: the list that was cut short must not survive the set_state
    for s in range(3):
        p.step(what="drv_clist after set_state")
    assert p.flags() == [0] * E
    p.close()


# ------------------------------------------------------------------------------------------------ passes
def test_first_contacts_in_later_narrowphase_passes(gpu):
    """60 to 62 candidates in 4 passes of 16: slots are handed out in passes 0, 1 and 2 of the first substep; later a first contact
    arrives in pass 0 in front of cached pairs that are re-touched in passes 1 and 2, and one in the last pass behind them"""
    p = Pair(gpu, DRV)
    p.put(2, p.blob(cs.drv_passes))
    p.put(5, p.blob(cs.drv_passes), batched=True)
    peaks = []
    for s in range(8):
        p.step(what="drv_passes")
        peaks.append(p.ora.peak_arbiters(2))
    assert peaks[0] == 4 and peaks[-1] == 6 and sorted(peaks) == peaks, peaks
    assert p.flags() == [0] * E and p.ora.overflow() == 0
    p.close()


# ------------------------------------------------------------------------------------------------ deep chains
@pytest.mark.parametrize("kind,seed,mixed", [(DRV, 1, False), (DRV, 2, False), (DRV, 3, False), (DRV, 4, False), (DRV, 5, True), (DRV, 6, True),
                                             (RC, 0, False)])
def test_deep_chains(gpu, kind, seed, mixed):
    """Driving: all ten cars in one row against an obstacle, ten arbiters deep (thirteen with pedestrians wedged in), canonical order a
    permutation of the spatial one.  RoboCup: a column of ten robots, nine arbiters chained through the joints."""
    p = Pair(gpu, kind, flags=8)
    st = p.blob(cs.drv_chain10, seed=seed, mixed=mixed) if kind == DRV else p.blob(cs.rc_chain)
    p.put(1, st)
    p.put(6, st, batched=True)
    deep = 0
    for s in range(8):
        p.step(what="chain %s seed %d" % (kind, seed))
        deep = max(deep, p.ora.active_contacts(1))
    assert deep >= (10 if kind == DRV else 9), deep
    assert p.flags() == [0] * E and p.ora.overflow() == 0 and p.ora.degenerate() == 0
    p.close()
    if kind == DRV:   # the counters are summed over a handle's environments: the chain once more on its own
        alone = Pair(gpu, DRV, num_envs=1)
        alone.put(0, st)
        for s in range(3):
            alone.step(what="drv_chain10 alone")
        assert alone.env.debug_counters()["split"] > 0, "a chain ten levels deep never took the general multi-level solver"
        alone.close()
