"""Exact device-side save and restore of chosen environments (dynenv_get_exact / dynenv_set_exact; BatchedDynEnv.get_exact, set_exact,
fork(exact=True)).  -m gpu.

An exact blob is every simulation-state row of an environment, so a restore followed by the same actions must be the run the blob was
saved from, bit for bit: every comparison is of int views or of checkpoint() bytes.  Configurations, shapes, pile environments, per-env
oracles and the checkpoint comparison (which leaves Driving Partial's timing word EI_DEFER_OBS out) are those of the masked reset and
the masked step (tests/per_env_common.py, tests/step_masked_common.py)."""
import numpy as np
import pytest

import per_env_common as pc
import step_masked_common as sm

pytestmark = pytest.mark.gpu

STEPS = 6


def _situation(cfg, E, **kw):
    return pc.situation(cfg, E, episodes="per_env", **kw)


def _scribble(env, cfg):
    """every byte of every per-environment array of the handle inverted (through a checkpoint; nothing is stepped on it)"""
    junk = env.checkpoint().copy()
    end = junk.size if pc.driving(cfg) else junk.size - pc.RC_PAIRTAB_BYTES
    junk[pc.CKPT_HEADER:end] ^= 0xFF
    env.restore(junk)


def _eq(a, b):
    import torch
    return bool(torch.equal(a, b))


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("cfg,shape", pc.CASES)
def test_round_trip_then_replay(cfg, shape):
    """1. save every environment, take six steps, restore: the checkpoint is the one from before, byte for byte, and every status is 0.
    Between the steps and the restore EVERY byte of every per-environment array is inverted, so no array can come back right by not
    having changed (the piles alone do not move the obstacles, say).
    2. the same six actions again: every step's observations, rewards and dones are the first pass's, and so is the final checkpoint."""
    E, _ = pc.SHAPES[shape]
    env = _situation(cfg, E)
    assert env.exact_size % 16 == 0 and env.exact_size > env.state_size
    c0 = pc.ckpt(env)
    blobs = env.get_exact()
    assert tuple(blobs.shape) == (E, env.exact_size)
    assert pc.ckpt(env).tobytes() == c0.tobytes(), "a save changes nothing"
    acts = pc.actions(cfg, E, env.n_agents, STEPS, 7, idle=pc.pile_envs(cfg, E))
    first = []
    for a in acts:
        pc.step(env, a, auto_reset=False)
        first.append(sm.outputs(env))
    c1 = pc.ckpt(env)
    assert c1.tobytes() != c0.tobytes()
    _scribble(env, cfg)
    status = env.set_exact(None, blobs)
    assert status.cpu().tolist() == [0] * E
    back = pc.ckpt(env)
    diff = np.nonzero(back != c0)[0]
    assert diff.size == 0, "after the restore the checkpoint differs in %d bytes, first at offset %d of %d" % (diff.size, diff[0], c0.size)
    assert _eq(env.get_exact(), blobs), "saving again gives the same blobs"
    for s, a in enumerate(acts):
        pc.step(env, a, auto_reset=False)
        assert sm.same_outputs(first[s], sm.outputs(env)) == "", "replayed step %d" % s
    assert pc.ckpt(env).tobytes() == c1.tobytes(), "the replay ends where the first pass ended"
    assert env.error_flags() == 0
    env.close()


# ------------------------------------------------------------------------------------------------ 2'
@pytest.mark.parametrize("cfg,shape", [(c, s) for c, s in pc.CASES if c in ("driving_partial", "robocup_partial")])
def test_replay_with_the_scheduler_left_as_it_is(cfg, shape):
    """2'. the Partial configurations once more WITHOUT the inversion in between (which goes through restore() and so starts the
    scheduler's scratch - Driving Partial's deferred-observation lists and their parity, the forecasts - over): the restore comes
    straight behind the sixth step's deferred launch, and the replayed steps are still the first pass's."""
    E, _ = pc.SHAPES[shape]
    env = _situation(cfg, E)
    c0 = pc.ckpt(env)
    blobs = env.get_exact()
    acts = pc.actions(cfg, E, env.n_agents, STEPS, 7, idle=pc.pile_envs(cfg, E))
    first = []
    for a in acts:
        pc.step(env, a, auto_reset=False)
        first.append(sm.outputs(env))
    c1 = pc.ckpt(env)
    assert env.set_exact(None, blobs).cpu().tolist() == [0] * E
    assert pc.ckpt(env).tobytes() == c0.tobytes()
    for s, a in enumerate(acts):
        pc.step(env, a, auto_reset=False)
        assert sm.same_outputs(first[s], sm.outputs(env)) == "", "replayed step %d" % s
    assert pc.ckpt(env).tobytes() == c1.tobytes(), "the replay ends where the first pass ended"
    assert env.error_flags() == 0
    env.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("cfg,shape", [(c, s) for c, s in pc.CASES if s != "E1"])
def test_a_subset_against_the_masked_step(cfg, shape):
    """3. A saves M, steps everyone six times and restores M; its twin B steps the complement of M alone.  The handles are the same
    bytes: the listed environments are back where they were and no byte of an unlisted one was touched."""
    E, M = pc.SHAPES[shape]
    rest = [e for e in range(E) if e not in M]
    a, b = _situation(cfg, E), _situation(cfg, E)
    assert pc.ckpt_diff(a, b) == "", "same configuration, same history"
    blobs = a.get_exact(M)
    for act in pc.actions(cfg, E, a.n_agents, STEPS, 7, idle=pc.pile_envs(cfg, E)):
        pc.step(a, act, auto_reset=False)
        pc.step(b, act, auto_reset=False, active=rest)
    assert pc.ckpt_diff(a, b) != "", "the listed environments moved"
    import torch
    ids = M if E <= 5 else torch.tensor(M, dtype=torch.int32, device="cuda")
    assert a.set_exact(ids, blobs).cpu().tolist() == [0] * len(M)
    assert pc.ckpt_diff(a, b) == ""
    assert a.error_flags() == b.error_flags() == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cfg", pc.PILE_CFGS)
def test_the_detour_the_oracle_never_sees(cfg, oracle_built):
    """4. environments 0 and 1 hold a pile with live contacts (asserted on the per-env oracles) when they are saved.  Three steps with
    other actions, a restore, and the next eight steps are the oracle's next eight: which takes the contact cache with its warm-start
    impulses, the shortcut state and the call-to-call caches to be the saved ones - what get_states / set_states cannot do."""
    E, piles = 5, [0, 1]
    env = pc.make(cfg, E, episodes="per_env")
    env.reset_flat()
    ora = {e: pc.env_oracle(cfg, e) for e in piles}
    A = env.n_agents
    for a in pc.actions(cfg, E, A, pc.HISTORY, 5):
        pc.step(env, a, auto_reset=False)
    for e in piles:
        ora[e].reset()
        st = pc.write_pile(cfg, ora[e].get_state(0), pc.HISTORY)
        env.set_state(e, st)
        ora[e].set_state(0, st)

    def both(act, what):
        og, rg, dg = pc.step(env, act, auto_reset=False)
        og, rg, dg = og.cpu().numpy(), rg.cpu().numpy(), dg.cpu().numpy()
        for e in piles:
            oc, rc, dc = ora[e].step(act[e:e + 1])
            assert pc.same_f32(og[e], oc[0]), "%s: observations of environment %d" % (what, e)
            assert pc.same_f64(rg[e], rc[0]) and dg[e] == dc[0], "%s: rewards / dones of environment %d" % (what, e)
    for s, act in enumerate(pc.actions(cfg, E, A, 2, 6, idle=piles)):
        both(act, "pile step %d" % s)
    for e in piles:
        assert ora[e].active_contacts(0) > 0, "environment %d holds no live contact when it is saved" % e
    blobs = env.get_exact(piles)
    for act in pc.actions(cfg, E, A, 3, 21):   # the detour: the piles are driven too
        pc.step(env, act, auto_reset=False)
    assert not _eq(env.get_exact(piles), blobs)
    assert env.set_exact(piles, blobs).cpu().tolist() == [0, 0]
    for s, act in enumerate(pc.actions(cfg, E, A, 8, 8, idle=piles)):
        both(act, "step %d after the restore" % s)
    for e in piles:
        assert ora[e].overflow() == 0
        assert env.get_state(e).elapsed == ora[e].get_state(0).elapsed == (pc.HISTORY + 2 + 8) * pc.sub(cfg)[0]
    assert env.get_state(2).elapsed == (pc.HISTORY + 2 + 3 + 8) * pc.sub(cfg)[0]
    assert env.error_flags_per_env().cpu().tolist() == [0] * E
    env.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("cfg", ["driving10", "robocup5"])
def test_exact_fork(cfg):
    """5. fork([0], [3], exact=True): environment 3 is environment 0 in every row - and in the canonical blob -, the others keep every
    byte; a blob saved from a handle of five environments loads into a handle of one."""
    E = 5
    env = _situation(cfg, E)
    before = env.get_exact()
    assert not _eq(before[3], before[0])
    assert env.fork([0], [3], exact=True).cpu().tolist() == [0]
    assert _eq(env.get_exact([3]), env.get_exact([0])) and _eq(env.get_exact([3]), before[0:1])
    assert _eq(env.get_states([3]), env.get_states([0]))
    after = env.get_exact()
    for e in (0, 1, 2, 4):
        assert _eq(after[e], before[e]), "environment %d changed" % e
    one = pc.make(cfg, 1, episodes="per_env")
    assert one.exact_size == env.exact_size
    assert one.set_exact([0], after[2:3]).cpu().tolist() == [0]
    assert _eq(one.get_exact(), after[2:3])
    assert one.get_state(0).elapsed == env.get_state(2).elapsed
    assert one.error_flags() == 0 and env.error_flags() == 0
    one.close()
    env.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("cfg", ["driving10", "robocup5"])
def test_refusals(cfg):
    """6. destinations [1, 7, -1, 2] with a zero-filled last blob: status [0, 2, 2, 1]; environment 2 keeps every byte but error bit 6,
    which a reset clears; 0, 3 and 4 are untouched; a blob of another configuration is refused; get_exact skips a bad index."""
    import torch
    from dynenv_amd import _capi
    E = 5
    env = _situation(cfg, E)
    before, canon = env.get_exact(), env.get_states()
    blobs = torch.stack([before[4], before[0], before[3], torch.zeros_like(before[0])])
    assert env.set_exact([1, 7, -1, 2], blobs).cpu().tolist() == [_capi.SET_WRITTEN, _capi.SET_BAD_INDEX, _capi.SET_BAD_INDEX, _capi.SET_REJECTED]
    after = env.get_exact()
    assert _eq(after[1], before[4]), "the valid blob was written"
    for e in (0, 3, 4):
        assert _eq(after[e], before[e]), "environment %d changed" % e
    w0, w1 = before[2].cpu().numpy().view(np.int32), after[2].cpu().numpy().view(np.int32)
    changed = np.nonzero(w0 != w1)[0]
    assert changed.size == 1 and w1[changed[0]] == w0[changed[0]] | _capi.ERR_BAD_BLOB, "environment 2: nothing but error bit 6"
    assert _eq(env.get_states([0, 2, 3, 4]), canon[[0, 2, 3, 4]])
    assert env.error_flags_per_env().cpu().tolist() == [0, 0, _capi.ERR_BAD_BLOB, 0, 0]
    env.reset_envs([2])
    assert env.error_flags_per_env().cpu().tolist() == [0] * E
    if pc.driving(cfg):   # a RoboCup blob, cut to this handle's blob size: another configuration's tag
        rc = pc.make("robocup5", 1, episodes="per_env")
        rc.reset_flat()
        foreign = rc.get_exact()
        cut = torch.zeros((1, env.exact_size), dtype=torch.uint8, device="cuda")
        n = min(env.exact_size, int(foreign.shape[1]))
        cut[0, :n] = foreign[0, :n]
        mid, canon = env.get_exact(), env.get_states()
        assert env.set_exact([4], cut).cpu().tolist() == [_capi.SET_REJECTED]
        assert env.error_flags_per_env().cpu().tolist() == [0, 0, 0, 0, _capi.ERR_BAD_BLOB]
        assert _eq(env.get_states(), canon) and _eq(env.get_exact()[:4], mid[:4])
        env.reset_envs([4])
        assert env.error_flags() == 0
        rc.close()
    # get_exact: the row of an index outside [0, E) keeps its bytes
    now = env.get_exact()
    out = torch.full((3, env.exact_size), 0xA5, dtype=torch.uint8, device="cuda")
    assert env.get_exact([0, 9, 4], out=out) is out
    assert _eq(out[0], now[0]) and _eq(out[2], now[4]) and bool((out[1] == 0xA5).all())
    env.close()


# ------------------------------------------------------------------------------------------------ 7
def test_a_captured_restore_reads_ids_and_blobs_at_replay():
    """7. set_exact(ids, blobs) alone in a graph - one launch -, replayed after new blob contents were written and one id was set to
    -1: the listed environments are the new blobs, the switched-off one is untouched.  Then the same behind a captured step, in one
    graph, against an eager twin."""
    import torch
    cfg, E = "driving10", 5
    env, twin = _situation(cfg, E), _situation(cfg, E)
    assert pc.ckpt_diff(env, twin) == ""
    saved = env.get_exact().clone()
    size = env.exact_size
    ids = torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda")
    blobs = torch.zeros((3, size), dtype=torch.uint8, device="cuda")
    blobs.copy_(saved[[0, 2, 4]])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        status = env.set_exact(ids, blobs)
    acts = pc.actions(cfg, E, env.n_agents, 3, 13, idle=pc.pile_envs(cfg, E))
    for a in acts[:2]:
        pc.step(env, a, auto_reset=False)
        pc.step(twin, a, auto_reset=False)
    mid = env.get_exact().clone()
    ids.copy_(torch.tensor([0, -1, 4], dtype=torch.int32, device="cuda"))
    blobs.copy_(saved[[4, 2, 0]])   # new contents: 0 <- 4's blob, 4 <- 0's
    g.replay()
    assert status.cpu().tolist() == [0, 2, 0]
    now = env.get_exact()
    assert _eq(now[0], saved[4]) and _eq(now[4], saved[0])
    for e in (1, 2, 3):
        assert _eq(now[e], mid[e]), "environment %d was touched" % e
    assert twin.set_exact([0, 4], saved[[4, 0]]).cpu().tolist() == [0, 0]
    assert pc.ckpt_diff(env, twin) == ""
    # a step and the restore behind it, in one graph
    static_a = torch.zeros((E, env.n_agents, env.action_dim), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        env.step_flat(static_a, auto_reset=False)
        status2 = env.set_exact(ids, blobs)
    static_a.copy_(torch.tensor(acts[2], device="cuda"))
    ids.copy_(torch.tensor([1, 3, -1], dtype=torch.int32, device="cuda"))
    blobs.copy_(saved[[1, 3, 2]])
    before = env.get_exact().clone()
    g2.replay()
    assert status2.cpu().tolist() == [0, 0, 2]
    now = env.get_exact()
    assert _eq(now[1], saved[1]) and _eq(now[3], saved[3])
    for e in (0, 2, 4):
        assert not _eq(now[e], before[e]), "environment %d was not stepped" % e
    pc.step(twin, acts[2], auto_reset=False)
    assert twin.set_exact([1, 3], saved[[1, 3]]).cpu().tolist() == [0, 0]
    assert pc.ckpt_diff(env, twin) == ""
    assert sm.same_outputs(sm.outputs(env), sm.outputs(twin)) == ""
    assert env.error_flags() == 0 and twin.error_flags() == 0
    env.close()
    twin.close()
