"""Batched, device-side state transfer (dynenv_get_states / dynenv_set_states / dynenv_error_flags_env; BatchedDynEnv.get_states,
set_states, fork, error_flags_per_env).  Everything is compared bit for bit, against the per-environment calls (get_state / set_state:
the same kernels for ONE blob, through host memory), against whole checkpoints (every non-scratch device array of the handle) and
against the CPU oracle.  What the per-environment calls themselves produce is pinned by tests/test_gpu_state_digests.py.

Shapes: Driving with 10 cars and with 2 (car slots left empty), RoboCup with 5 and with 1 robot per team, one Partial + Realistic handle per
environment type; E = 1 with n = 1, E = 5 with the permuted subset [3, 0, 4], E = 70 with every environment (more than one 64-wide
block of the per-environment kernels; the random resets give the environments differing pedestrian and obstacle counts)."""
import numpy as np
import pytest

from per_env_common import (DONOR_SEED, HISTORY, NAMES, SEED, STATE_CASES as CASES, STATE_SHAPES as SHAPES, actions as _actions,
                            donor_blobs as _donor_blobs, listed_ids as _ids, make as _make, oracle, select, started as _started, step)

pytestmark = pytest.mark.gpu

CFGS = select(*NAMES[:6])   # (robocup5_random is the masked reset's)


def _make_oracle(cfg, E, seed):
    return oracle(cfg, E, seed, threads=8)


def _run(env, acts):
    for a in acts:
        step(env, a, auto_reset=False)


@pytest.mark.parametrize("cfg,shape", CASES)
def test_get_states_equals_get_state(cfg, shape):
    """1. every row of get_states() is the bytes of get_state(e) - zeroed pads and unused slots included -, for the full list and for
    the subset, whichever form the ids come in"""
    import torch
    E, listed = SHAPES[shape]
    env = _started(cfg, E, SEED)
    want = [bytes(env.get_state(e)) for e in range(E)]
    assert len(set(want)) == E, "the environments should differ from each other"
    if cfg.startswith("driving") and E == 70:
        sts = [env.get_state(e) for e in range(E)]
        assert len({s.n_peds for s in sts}) > 1 and len({s.n_obst for s in sts}) > 1, "differing pedestrian / obstacle counts"
    got = env.get_states()
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (E, env.state_size) == (E, len(want[0]))
    got = got.cpu().numpy()
    for e in range(E):
        assert got[e].tobytes() == want[e], "environment %d of the full list" % e
    ids = _ids(E, listed)
    for form in (ids, np.asarray(ids, dtype=np.int64), torch.tensor(ids, device="cuda", dtype=torch.int64)):
        sub = env.get_states(form).cpu().numpy()
        assert sub.shape == (len(ids), env.state_size)
        for k, e in enumerate(ids):
            assert sub[k].tobytes() == want[e], "row %d (environment %d) of the listed environments" % (k, e)
    assert env.error_flags() == 0
    env.close()


@pytest.mark.parametrize("cfg,shape", CASES)
def test_set_states_equals_a_set_state_loop(cfg, shape):
    """2. two handles with the same configuration and history: A filled by a set_state(e, blob) loop, B by ONE set_states.  Their
    checkpoints - every non-scratch device array: the cleared caches, RoboCup's shape cache and constraint order, the environments
    that were not listed - are byte-identical, and so are 20 further steps."""
    import torch
    E, listed = SHAPES[shape]
    ids = _ids(E, listed)
    sts, blobs = _donor_blobs(cfg, E, ids)
    a, b = _started(cfg, E, SEED), _started(cfg, E, SEED)
    assert a.checkpoint().tobytes() == b.checkpoint().tobytes(), "same configuration, same history"
    before = a.checkpoint().tobytes()
    for e, st in zip(ids, sts):
        a.set_state(e, st)
    pos = b._episode_step
    status = b.set_states(None if listed is None else ids, blobs)   # (numpy blobs: one upload)
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0] * len(ids)
    assert b._episode_step == pos == a._episode_step, "the host's lock-step position stays where it was"
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.tobytes() != before, "the blobs should have changed the handle"
    diff = np.nonzero(ca != cb)[0]
    assert diff.size == 0, "checkpoints differ in %d bytes, first at offset %d of %d" % (diff.size, diff[0], ca.size)
    for s, act in enumerate(_actions(cfg, E, a.n_agents, 20, 13)):
        t = torch.tensor(act, device="cuda")
        oa, ra, da = a.step_flat(t, auto_reset=False)
        ob, rb, db = b.step_flat(t, auto_reset=False)
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(oa, ob), "step %d after the fill" % s
    assert a.checkpoint().tobytes() == b.checkpoint().tobytes()
    assert a.error_flags() == b.error_flags() == 0
    # a device tensor of blobs is used in place, and what was written reads back as written
    c = _started(cfg, E, SEED)
    dev = torch.tensor(blobs, device="cuda")
    c.set_states(torch.tensor(ids, device="cuda", dtype=torch.int32), dev)
    assert torch.equal(c.get_states(ids), dev)
    for x in (a, b, c):
        x.close()


@pytest.mark.parametrize("cfg,shape", CASES)
def test_set_states_then_steps_like_the_oracle(cfg, shape, oracle_built):
    """3. the same blobs go into the CPU oracle through its own set_state: ten steps of the handle against the oracle are
    bit-identical (Full and Partial observations), listed and unlisted environments alike"""
    import torch
    ol = oracle_built
    E, listed = SHAPES[shape]
    ids = _ids(E, listed)
    sts, blobs = _donor_blobs(cfg, E, ids)
    env = _started(cfg, E, SEED)
    ora = _make_oracle(cfg, E, SEED)
    ora.reset()
    if listed is not None:  # the environments that are not overwritten must have lived the handle's history
        for act in _actions(cfg, E, env.n_agents, HISTORY, 5):
            ora.step(act)
    env.set_states(None if listed is None else ids, torch.tensor(blobs, device="cuda"))
    ost = ol.DrivingState if CFGS[cfg][0] == 1 else ol.RoboCupState
    for e, st in zip(ids, sts):
        ora.set_state(e, ost.from_buffer_copy(bytes(st)))
    for s, act in enumerate(_actions(cfg, E, env.n_agents, 10, 21)):
        og, rg, dg = env.step_flat(torch.tensor(act, device="cuda"), auto_reset=False)
        oc, rc, dc = ora.step(act)
        assert np.array_equal(rg.cpu().numpy(), rc), "rewards, step %d" % s
        assert np.array_equal(dg.cpu().numpy().astype(np.uint8), dc), "dones, step %d" % s
        assert np.array_equal(og.cpu().numpy(), oc), "observations, step %d" % s
    assert env.error_flags() == 0
    env.close()
    ora.close()


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_fork_branches_one_state_into_many(cfg, oracle_built):
    """4. fork([1, 1], [0, 4]) on E = 5: rows 0 and 4 become row 1, rows 2 and 3 stay; the checkpoint is that of a twin filled by
    set_state(d, get_state(1)); ten further steps match the oracle treated the same way"""
    import torch
    E = 5
    env, twin = _started(cfg, E, SEED), _started(cfg, E, SEED)
    ora = _make_oracle(cfg, E, SEED)
    ora.reset()
    for act in _actions(cfg, E, env.n_agents, HISTORY, 5):
        ora.step(act)
    before = env.get_states().cpu().numpy()
    status = env.fork([1, 1], [0, 4])
    assert status.cpu().tolist() == [0, 0]
    rows = env.get_states().cpu().numpy()
    assert rows[0].tobytes() == rows[4].tobytes() == rows[1].tobytes() == before[1].tobytes()
    assert rows[0].tobytes() != before[0].tobytes() and rows[4].tobytes() != before[4].tobytes()
    assert rows[2].tobytes() == before[2].tobytes() and rows[3].tobytes() == before[3].tobytes()
    src = twin.get_state(1)
    for d in (0, 4):
        twin.set_state(d, src)
    assert env.checkpoint().tobytes() == twin.checkpoint().tobytes()
    osrc = ora.get_state(1)   # (the source itself is not written on either side: it keeps its contact cache)
    for d in (0, 4):
        ora.set_state(d, osrc)
    for s, act in enumerate(_actions(cfg, E, env.n_agents, 10, 23)):
        og, rg, dg = env.step_flat(torch.tensor(act, device="cuda"), auto_reset=False)
        oc, rc, dc = ora.step(act)
        assert np.array_equal(rg.cpu().numpy(), rc) and np.array_equal(dg.cpu().numpy().astype(np.uint8), dc), "step %d" % s
        assert np.array_equal(og.cpu().numpy(), oc), "observations, step %d" % s
    # device-resident ids: nothing is read back, the same result
    env2 = _started(cfg, E, SEED)
    env2.fork(torch.tensor([1, 1], device="cuda"), torch.tensor([0, 4], device="cuda"))
    assert torch.equal(env2.get_states(), torch.tensor(rows, device="cuda"))
    for x in (env, twin, env2):
        x.close()
    ora.close()


@pytest.mark.parametrize("cfg", ["driving10", "driving2", "robocup5", "robocup1"])
def test_a_blob_that_does_not_fit_is_rejected_and_reported(cfg):
    """5. one blob with n_peds = 21 (Driving) / n_robots = R + 1 (RoboCup) among valid ones, and one index equal to E: status 0 / 1 / 2
    in the right places, the rejected environment untouched, error bit 6 on it alone, the compat step() raises and names it, a valid
    set_states of it clears the bit"""
    from dynenv_amd import _capi
    E = 5
    driving = CFGS[cfg][0] == 1
    sts, blobs = _donor_blobs(cfg, E, [0, 1, 2, 3])
    env = _make(cfg, E, SEED)
    env.reset()
    _run(env, _actions(cfg, E, env.n_agents, 10, 5))
    view = _capi.blobs_as_states(blobs, env.env_type)
    good1 = blobs[1].copy()
    if driving:
        view["n_peds"][1] = 21
    else:
        view["n_robots"][1] = env.n_agents + 1
    ids = [2, 0, E, 3]
    want = {e: bytes(env.get_state(e)) for e in range(E)}
    pos = env._episode_step
    status = env.set_states(ids, blobs)
    assert status.cpu().tolist() == [0, 1, 2, 0]
    assert bytes(env.get_state(0)) == want[0], "a rejected blob leaves its environment untouched"
    assert bytes(env.get_state(1)) == want[1] and bytes(env.get_state(4)) == want[4], "environments that were not listed"
    assert bytes(env.get_state(2)) == bytes(sts[0]) and bytes(env.get_state(3)) == bytes(sts[3]), "the valid blobs were written"
    assert env.error_flags_per_env().cpu().tolist() == [64, 0, 0, 0, 0]
    assert env.error_flags() == 64
    assert env._episode_step == pos
    with pytest.raises(_capi.DynEnvError, match=r"error bit 6.*environment 0\b"):
        env.step(_actions(cfg, E, env.n_agents, 1, 3)[0])
    assert env.error_flags_per_env().cpu().tolist() == [64, 0, 0, 0, 0], "sticky"
    assert env.set_states([0], good1[None]).cpu().tolist() == [0]
    assert env.error_flags_per_env().cpu().tolist() == [0] * E and env.error_flags() == 0
    assert bytes(env.get_state(0)) == bytes(sts[1])
    env.step(_actions(cfg, E, env.n_agents, 1, 4)[0])   # ... and the compat step runs again
    want[4] = bytes(env.get_state(4))                   # (the steps moved every environment on)
    if not driving:  # the defender lists are checked too: a count outside 0..10, an id outside 0..9
        for field, val in (("n_def", 11), ("n_def", -1), ("defenders", 10), ("defenders", -1)):
            bad = good1.copy()
            v = _capi.blobs_as_states(bad[None], env.env_type)
            if field == "n_def":
                v["n_def"][0, 1] = val
            else:
                v["n_def"][0, 0] = 1
                v["defenders"][0, 0, 0] = val
            assert env.set_states([4], v).cpu().tolist() == [1], (field, val)
            assert bytes(env.get_state(4)) == want[4]
        assert env.error_flags_per_env().cpu().tolist() == [0, 0, 0, 0, 64]
    else:
        for field, val in (("n_cars", env.n_agents + 1), ("n_peds", -1), ("n_obst", 21), ("n_obst", -1)):
            v = _capi.blobs_as_states(good1[None].copy(), env.env_type)
            v[field][0] = val
            assert env.set_states([4], v).cpu().tolist() == [1], (field, val)
            assert bytes(env.get_state(4)) == want[4]
        assert env.error_flags_per_env().cpu().tolist() == [0, 0, 0, 0, 64]
    env.reset_flat()
    assert env.error_flags() == 0, "a reset clears the bit"
    env.close()


# what test 5 writes into a blob to make it a misfit, per environment type: (field, value); "n_def" goes to team 1, "defenders" to the
# first id of team 0 with n_def[0] = 1
MISFITS = {1: [("n_cars", "A+1"), ("n_peds", 21), ("n_peds", -1), ("n_obst", 21), ("n_obst", -1)],
           0: [("n_robots", "A+1"), ("n_def", 11), ("n_def", -1), ("defenders", 10), ("defenders", -1)]}
SYNC_CASES = [(c, f, v) for c in ("driving10", "robocup5") for f, v in MISFITS[CFGS[c][0]]]


@pytest.mark.parametrize("cfg,field,val", SYNC_CASES)
def test_set_state_returns_the_error_of_a_blob_that_does_not_fit(cfg, field, val):
    """5b. the synchronous call has a return code: a misfit is DYNENV_ERR_ARG ("does not match"), the environment - every environment -
    stays as it was, NO error bit is raised (a sticky bit 6 would make a later compat step() raise), and a valid set_state of the same
    environment succeeds.  The staging area the call goes through is not part of a checkpoint: its size is the recorded one."""
    import json
    import os
    from dynenv_amd import _capi
    E = 5
    env = _started(cfg, E, SEED)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_digests.json")) as f:
        assert env.checkpoint().size == json.load(f)["digests"]["state/%s/E5_subset" % cfg]["checkpoint_size"]
    sts, _ = _donor_blobs(cfg, E, [0])
    good = sts[0]
    bad = type(good).from_buffer_copy(bytes(good))
    if field == "n_def":
        bad.n_def[1] = val
    elif field == "defenders":
        bad.n_def[0] = 1
        bad.defenders[0][0] = val
    else:
        setattr(bad, field, env.n_agents + 1 if val == "A+1" else val)
    before = env.get_states().cpu().numpy().tobytes()
    ckpt = env.checkpoint().tobytes()
    with pytest.raises(_capi.DynEnvError, match="does not match"):
        env.set_state(4, bad)
    assert env.get_states().cpu().numpy().tobytes() == before, "a rejected blob leaves every environment untouched"
    assert env.checkpoint().tobytes() == ckpt
    assert env.error_flags_per_env().cpu().tolist() == [0] * E and env.error_flags() == 0
    env.set_state(4, good)
    assert bytes(env.get_state(4)) == bytes(good)
    assert env.error_flags_per_env().cpu().tolist() == [0] * E
    env.close()


@pytest.mark.parametrize("cfg", ["driving10", "robocup5"])
def test_error_flags_per_env_ors_to_error_flags(cfg):
    """6. the OR of error_flags_per_env() over the environments is error_flags(): clean, and with different bits up in different
    environments on both sides of a 64-wide block"""
    import torch
    from dynenv_amd import _capi
    E = 70
    env = _started(cfg, E, SEED)
    per = env.error_flags_per_env()
    assert per.dtype == torch.int32 and per.is_cuda and tuple(per.shape) == (E,)
    assert int(per.cpu().numpy().any()) == 0 and env.error_flags() == 0
    act = _actions(cfg, E, env.n_agents, 1, 3)[0]
    act[66, 0, 0] = 9                        # outside the action space: error bit 1 on environment 66
    _run(env, [act])
    bad = _capi.blobs_as_states(env.get_states([7]).cpu().numpy(), env.env_type)
    bad["n_cars" if CFGS[cfg][0] == 1 else "n_robots"][0] += 1
    assert env.set_states([7], bad).cpu().tolist() == [1]   # error bit 6 on environment 7
    per = env.error_flags_per_env().cpu().numpy()
    want = np.zeros((E,), np.int32)
    want[66], want[7] = 2, 64
    assert np.array_equal(per, want)
    assert int(np.bitwise_or.reduce(per)) == env.error_flags() == 66
    env.close()


def test_set_states_python_surface():
    """the host side of set_states / get_states: the cached counts are dropped, the lock-step position moves only when told to, a
    handle that was never reset needs to be told, ids listed twice on the host are refused"""
    import torch
    from dynenv_amd import _capi
    cfg, E = "driving10", 5
    src = _started(cfg, E, DONOR_SEED)
    blobs = src.get_states()
    fresh = _make(cfg, E, SEED)
    with pytest.raises(_capi.DynEnvError, match="episode_step"):
        fresh.set_states(None, blobs)
    with pytest.raises(_capi.DynEnvError, match="episode_step"):
        fresh.fork([0], [1])
    fresh.set_states(None, blobs, episode_step=HISTORY)
    assert fresh._episode_step == HISTORY and not fresh._needs_reset
    assert torch.equal(fresh.get_states(), blobs)
    assert np.array_equal(fresh.counts().cpu().numpy(), src.counts().cpu().numpy())
    env = _make(cfg, E, SEED)
    env.reset()
    c0 = env._host_counts().copy()
    env.set_states([1, 3], blobs[:2])
    assert env._counts_np is None and env._episode_step == 0
    c1 = env._host_counts()
    assert np.array_equal(c1[[1, 3]], src.counts().cpu().numpy()[:2]) and np.array_equal(c1[[0, 2, 4]], c0[[0, 2, 4]])
    with pytest.raises(_capi.DynEnvError, match="twice"):
        env.set_states([1, 1], blobs[:2])
    with pytest.raises(_capi.DynEnvError):
        env.set_states([1, 2], blobs[:3])               # ids and blobs disagree
    with pytest.raises(_capi.DynEnvError):
        env.set_states(None, torch.zeros((E + 1, env.state_size), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_capi.DynEnvError):
        env.set_states([0], torch.zeros((1, env.state_size - 8), dtype=torch.uint8, device="cuda"))
    assert tuple(env.get_states([]).shape) == (0, env.state_size)
    assert env.error_flags() == 0
    for x in (src, fresh, env):
        x.close()
