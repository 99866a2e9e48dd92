"""The C ABI's caller-owned buffers (include/dynenv.h: "pointers named *_dev are DEVICE pointers owned by the caller ... ordered on
`stream`"), used the way a caller that binds the library itself uses them and BatchedDynEnv never does: slices of one slab at the
weakest alignment the header allows, NULL where NULL is allowed, a stream that is not torch's current one.  -m gpu.

  a. bounds: every call writes its rows and nothing else - the guard bands around every buffer of the arena
     (tests/abi_buffers_common.py) stay intact after each call, the interiors hold the oracle's bits, inputs stay what they were;
  b. NULL outputs against the oracle: steps and resets without an observation buffer, episode statistics with pointers left out,
     RoboCup Partial's refusal;
  c. stream order of the calls no capture test covers, behind a delay on a side stream;
  d. a misaligned observation buffer is refused on the host and nothing is touched.

Configurations, shapes, pile situations and actions are tests/per_env_common.py's; the oracle is the reference throughout, bit for bit:
nothing in here takes a tolerance.  Every buffer handed to the library lies fully inside the arena."""
import numpy as np
import pytest

import abi_buffers_common as ab
import per_env_common as pc

pytestmark = pytest.mark.gpu

CONFIGS = ("driving10", "driving2", "robocup5", "robocup1", "driving_partial", "robocup_partial", "driving3", "driving6", "robocup5_head")
STEPS = 12
NULL_STEPS = (2, 3, 4, 7)   # steps 3 to 5 and 8 of the twelve pass no observation buffer


class Run:
    """a handle, its oracles and an arena with every buffer its calls take; each method makes ONE call of the C ABI with arena pointers,
    the oracle's counterpart, and then checks the whole arena: guards, outputs, inputs"""

    def __init__(self, cfg, shape, reset=True):
        self.name, self.cfg = cfg, ab.cfg_of(cfg)
        self.c = pc.cfg_of(self.cfg)
        self.E, self.M = pc.SHAPES[shape]
        self.sub = self.M[::-1]   # the listed set of the blob calls, permuted
        self.env, self.ora, self.truth = ab.prepared(cfg, self.E, reset)
        self.piles = pc.pile_envs(self.cfg, self.E)
        self.A, self.K = self.env.n_agents, self.env.action_dim
        self.with_head = bool(self.c.flags & 16)
        self.ar = ab.arena_for(self.env, len(self.M))
        self.abi = ab.Abi(self.env, self.ar)
        self.ar.put("env_idx", np.asarray(self.sub, np.int32))
        self.ar.put("exact_idx", np.asarray(self.sub + [-1], np.int32))
        self.calls = 0
        self.ar.verify("%s %s: the arena as built" % (cfg, shape))

    def what(self, call):
        self.calls += 1
        return "%s E=%d call %d (%s)" % (self.name, self.E, self.calls, call)

    def actions(self, steps, seed):
        acts = pc.actions(self.cfg, self.E, self.A, steps, seed, idle=self.piles)
        heads = ab.head_actions(self.E, self.A, steps, seed + 1) if self.with_head else [None] * steps
        return list(zip(acts, heads))

    def mask(self, listed):
        m = np.zeros((self.E,), np.uint8)
        m[listed] = 1
        m[listed[0]] = 0x80   # (listed is "!= 0")
        return m

    # -------------------------------------------------------------------------------------------- the calls that change state
    def reset(self, listed=None, obs=True):
        buf = "obs" if obs else None
        if listed is None:
            rc, what = self.abi.reset(buf), self.what("dynenv_reset")
        else:
            self.ar.put("mask", self.mask(listed))
            rc, what = self.abi.reset_masked(buf), self.what("dynenv_reset_masked")
        assert rc == ab.OK, (what, self.abi.last_error())
        first = self.ora.reset(listed)
        if self.truth:
            self.truth.reset(listed)
        if obs:
            self.ar.expect_rows("obs", listed, first)
        self.ar.verify(what)

    def step(self, act, head=None, listed=None, obs=True):
        buf = "obs" if obs else None
        self.ar.put("actions", act)
        if head is not None:
            self.ar.put("head", head)
        if listed is not None:
            self.ar.put("mask", self.mask(listed))
            rc, what = self.abi.step_masked(buf, head=None if head is None else "head"), self.what("dynenv_step_masked")
        elif head is not None:
            rc, what = self.abi.step_head(buf), self.what("dynenv_step_head")
        else:
            rc, what = self.abi.step(buf), self.what("dynenv_step")
        assert rc == ab.OK, (what, self.abi.last_error())
        o, r, d = self.ora.step(act, listed, head, noobs=not obs)
        if self.truth:
            self.truth.step(act, listed, head)
        if obs:
            self.ar.expect_rows("obs", listed, o)
        self.ar.expect_rows("rewards", listed, r)
        self.ar.expect_rows("dones", listed, d)
        self.ar.verify(what)

    # -------------------------------------------------------------------------------------------- the calls that read it
    def full_obs(self):
        """(the oracles' last observation is the current state's: call it behind a step or reset that had a buffer)"""
        rc, what = self.abi.full_obs(), self.what("dynenv_full_obs")
        assert rc == ab.OK, (what, self.abi.last_error())
        src = self.truth or self.ora
        self.ar.expect_rows("full", None, [o.obs[0, -1] for o in src.o])
        self.ar.verify(what)

    def global_state(self):
        rc, what = self.abi.global_state(), self.what("dynenv_global_state")
        if pc.driving(self.cfg):
            assert rc == -4, what   # DYNENV_ERR_UNSUPPORTED, and nothing written
        else:
            assert rc == ab.OK, (what, self.abi.last_error())
            self.ar.expect_rows("global", None, self.ora.global_state())
        self.ar.verify(what)

    def counts(self):
        rc, what = self.abi.counts(), self.what("dynenv_counts")
        assert rc == ab.OK, (what, self.abi.last_error())
        self.ar.expect_rows("counts", None, self.ora.counts())
        self.ar.verify(what)

    def episode_stats(self, names=("ep_r", "ep_p", "ep_o", "goals")):
        """names: the four buffers, None for a pointer left out"""
        rc, what = self.abi.episode_stats(*names), self.what("dynenv_episode_stats" + str(tuple(n is not None for n in names)))
        assert rc == ab.OK, (what, self.abi.last_error())
        for name, want in zip(names, self.ora.stats()):
            if name is not None:
                self.ar.expect_rows(name, None, want)
        self.ar.verify(what)

    def error_flags_env(self):
        rc, what = self.abi.error_flags_env(), self.what("dynenv_error_flags_env")
        assert rc == ab.OK, (what, self.abi.last_error())
        assert self.ora.clean(), what
        self.ar.expect_rows("flags", None, np.zeros((self.E, 1), np.int32))
        self.ar.verify(what)

    def get_states(self, listed=None, per_env_call=True):
        """all environments (no index list) or the permuted subset: every blob is the oracle's state field by field and - per_env_call -
        the bytes of dynenv_get_state for that environment"""
        ids = list(range(self.E)) if listed is None else listed
        buf = "blobs" if listed is None else "blobs_sub"
        rc, what = self.abi.get_states(None if listed is None else "env_idx", len(ids), buf), self.what("dynenv_get_states")
        assert rc == ab.OK, (what, self.abi.last_error())
        got = self.ar.get(buf, shape=(len(ids), -1))
        for k, e in enumerate(ids):
            assert not (got[k] == np.resize(ab.PATTERN, got[k].size)).all(), "%s: blob %d was not written" % (what, k)
            ab.assert_blob_is_oracle_state(self.cfg, got[k], self.ora.get_state(e), "%s blob %d environment %d" % (what, k, e))
        self.ar.expect_rows(buf, None, [bytes(self.env.get_state(e)) for e in ids] if per_env_call else got.copy())
        self.ar.verify(what)

    def get_exact(self):
        """no oracle for the opaque blob: two saves over two different fills are the same bytes - so every byte of a listed blob was
        written, and an unchanged environment saves the same blob twice -, and the blob behind index -1 keeps its fill"""
        n = len(self.sub)
        saves = []
        for fill in (ab.PATTERN, ab.PATTERN ^ 0xFF):
            self.ar.refill("exact", fill)
            rc, what = self.abi.get_exact("exact_idx", n + 1), self.what("dynenv_get_exact")
            assert rc == ab.OK, (what, self.abi.last_error())
            got = self.ar.get("exact", shape=(n + 1, -1))
            assert (got[n] == np.resize(fill, got[n].size)).all(), "%s: the blob of index -1 was written" % what
            assert (got[:n] != np.resize(fill, got[0].size)).any(axis=1).all(), "%s: a listed blob was not written" % what
            self.ar.expect_rows("exact", range(n), got[:n])
            self.ar.verify(what)
            saves.append(got[:n].copy())
        d = np.nonzero(saves[0] != saves[1])
        assert d[0].size == 0, "dynenv_get_exact left %d bytes of the listed blobs unwritten, first: blob %d byte %d" % (d[0].size, d[0][0], d[1][0])
        assert len({saves[0][k].tobytes() for k in range(n)}) == n or self.E == 1, "the environments differ from each other"

    def reads(self):
        self.full_obs()
        self.global_state()
        self.counts()
        self.episode_stats()
        self.error_flags_env()
        self.get_states()
        self.get_states(self.sub)
        self.get_exact()

    def close(self):
        assert self.env.error_flags() == 0 and self.ora.clean()
        self.env.close()
        for o in (self.ora, self.truth):
            if o:
                o.close()


def test_the_arena_names_a_stray_byte():
    """the instrument itself: a byte written one past a buffer's end, and one before its start, is reported with the buffer and the side"""
    ar = ab.Arena([("a", 100, ab.U8, 1), ("b", 64, ab.OBS, 600)])
    assert ar.bufs["a"].start % 2 == 1 and ar.bufs["b"].start % 256 == 16 and ar.bufs["b"].start - ar.bufs["a"].end >= 1280 + 256
    ar.verify("untouched")
    ar.mem[ar.bufs["a"].end + 2] = 7
    with pytest.raises(AssertionError, match=r"ABOVE a .* offset 2 past"):
        ar.verify("stray")
    ar.mem[ar.bufs["a"].end + 2] = ab.FILL
    ar.mem[ar.bufs["b"].start - 1] = 0
    with pytest.raises(AssertionError, match=r"BELOW b .* 1 bytes before"):
        ar.verify("stray")
    ar.mem[ar.bufs["b"].start - 1] = ab.FILL
    ar.mem[ar.bufs["b"].start + 5] = 0
    with pytest.raises(AssertionError, match=r"b differs .* first at byte 5"):
        ar.verify("interior")


# ------------------------------------------------------------------------------------------------ a. bounds
@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
@pytest.mark.parametrize("cfg", CONFIGS)
def test_every_call_writes_its_rows_and_nothing_else(cfg, shape, oracle_built):
    """a. twelve steps, a masked step and a masked reset over the listed set, the reading calls, then a reset of everything and the reading
    calls again - the arena checked after every call.  A pile configuration starts from its situation (live contacts; the deferred
    launches of the Partial paths run), so its dynenv_reset comes last, from there; the others are reset first, too."""
    r = Run(cfg, shape, reset=False)
    if not r.piles:
        r.reset()
    acts = r.actions(STEPS + 1, 7)
    for a, hd in acts[:STEPS]:
        r.step(a, hd)
    r.step(*acts[STEPS], listed=r.M)
    r.reset(listed=r.M)
    r.reads()
    r.reset()
    r.reads()
    r.close()


# ------------------------------------------------------------------------------------------------ b. NULL outputs
@pytest.mark.parametrize("shape", ["E5", "E70"])
@pytest.mark.parametrize("cfg", ["driving10", "driving_partial", "robocup5"])
def test_steps_without_an_observation_buffer_are_the_oracles(cfg, shape, oracle_built):
    """b. twelve steps of which steps 3 to 5 and 8 pass obs_dev == NULL (Driving Partial: another kernel and no parity flip; RoboCup
    Full: no snapshot writes), then a masked step without a buffer and a plain one with: rewards and dones of every step, the
    observations of the steps that have a buffer, the states, the episode statistics and the error words are the oracle's - whose
    own steps without a buffer are step_noobs.  The eager, small, oracle-checked form of what tests/test_gpu_graph.py runs graphed."""
    r = Run(cfg, shape)
    acts = r.actions(STEPS + 2, 17)
    for k in range(STEPS):
        r.step(*acts[k], obs=k not in NULL_STEPS)
    r.step(*acts[STEPS], listed=r.M, obs=False)
    r.step(*acts[STEPS + 1])
    r.reads()
    assert r.env.error_flags() == 0, "error bit 2: the deferred list of a step without a buffer"
    r.close()


def test_robocup_partial_refuses_a_null_observation_buffer(oracle_built):
    """its rewards hold the observation reward, which comes out of the observation pass: DYNENV_ERR_ARG, and no byte of rewards, dones
    or of the handle changes"""
    r = Run("robocup_partial", "E5")
    twin = pc.situation("robocup_partial", r.E, episodes="per_env")
    assert pc.ckpt_diff(r.env, twin) == "", "same configuration, same history"
    a, _ = r.actions(1, 23)[0]
    r.ar.put("actions", a)
    r.ar.put("mask", r.mask(r.M))
    assert r.abi.step(None) == ab.ERR_ARG and "observation buffer is required" in r.abi.last_error()
    assert r.abi.step_masked(None) == ab.ERR_ARG and "observation buffer is required" in r.abi.last_error()
    r.ar.verify("refused steps")
    assert pc.ckpt_diff(r.env, twin) == ""
    r.step(a)   # ... and with a buffer it is the oracle's next step
    twin.close()
    r.close()


@pytest.mark.parametrize("shape", ["E5", "E70"])
@pytest.mark.parametrize("cfg", ["driving10", "driving_partial", "robocup5", "robocup_partial"])
def test_resets_without_an_observation_buffer(cfg, shape, oracle_built):
    """dynenv_reset and dynenv_reset_masked with obs_dev == NULL leave the states the oracle's reset leaves, write nothing, and the next
    step's observation - a noisy draw for Partial - is the oracle's"""
    r = Run(cfg, shape)
    acts = r.actions(2, 29)
    r.reset(obs=False)
    r.get_states()
    r.step(*acts[0])
    r.reset(listed=r.M, obs=False)
    r.get_states()
    r.get_states(r.sub)
    r.step(*acts[1])
    r.full_obs()
    r.close()


@pytest.mark.parametrize("cfg", ["driving10", "driving3", "robocup5", "robocup_partial"])
def test_episode_stats_with_pointers_left_out(cfg, oracle_built):
    """each of the four pointers NULL in turn, and all four: DYNENV_OK, the others written as before, nothing else touched"""
    r = Run(cfg, "E70")
    for a, hd in r.actions(3, 31):
        r.step(a, hd)
    names = ("ep_r", "ep_p", "ep_o", "goals")
    r.episode_stats()
    for out in list(range(4)) + [None]:
        for n in names:
            r.ar.refill(n)
        r.episode_stats(tuple(None if (out is None or k == out) else n for k, n in enumerate(names)))
    r.close()


# ------------------------------------------------------------------------------------------------ c. stream order
@pytest.mark.parametrize("cfg", ["driving_partial", "robocup_partial"])
def test_calls_are_ordered_on_the_stream_they_are_given(cfg, oracle_built):
    """c. everything goes to a side stream that is NOT torch's current stream while the library is called: a delay, the copies that put
    the inputs in place, one step and the seven calls that are never captured, one copy of the whole arena to the host, one
    synchronize.  A launch that went to any other stream runs during the delay, before its inputs arrive, and cannot produce the
    oracle's bytes.  The delay is bracketed by two events and must have lasted 10 ms: two orders of magnitude above a step of 70
    environments."""
    import torch
    r = Run(cfg, "E70")
    E, ids = r.E, r.M   # the blob calls list M in ascending order here; the arena holds the permuted list from before the delay
    _, src = pc.donor_blobs(cfg, E, ids)
    (act, _), (after, _) = r.actions(2, 37)
    cycles = ab.delay_cycles()
    s = torch.cuda.Stream()
    r.abi.stream = s
    host = torch.empty((r.ar.size,), dtype=torch.uint8).pin_memory()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t0.record()
        ab.enqueue_delay(cycles)
        t1.record()
        for name, value in (("actions", act), ("mask", r.mask(ids)), ("env_idx", np.asarray(ids, np.int32)), ("src_blobs", src)):
            r.ar.put(name, value, non_blocking=True)
    assert torch.cuda.current_stream() != s and torch.cuda.current_stream().query(), "the library is called with torch on its idle default stream"
    abi, n = r.abi, len(ids)
    rcs = [abi.step(), abi.full_obs(), abi.global_state(), abi.counts(), abi.episode_stats(), abi.error_flags_env(),
           abi.get_states(None, E, "blobs"), abi.set_states("env_idx", n, "src_blobs"), abi.get_states("env_idx", n, "blobs_sub")]
    with torch.cuda.stream(s):
        host.copy_(r.ar.mem, non_blocking=True)
    s.synchronize()
    ms = t0.elapsed_time(t1)
    print("\n%s: delay of %d cycles took %.1f ms" % (cfg, cycles, ms))
    assert ms >= 10.0, "the delay took %.2f ms: too short to tell a stream from another" % ms
    assert rcs == [ab.OK, ab.OK, ab.OK if not pc.driving(cfg) else -4] + [ab.OK] * 6, (rcs, abi.last_error())
    # the oracle's side of the same sequence
    img = host.numpy()
    o, rw, d = r.ora.step(act)
    r.truth.step(act)
    ex = r.ar.expect_rows
    ex("obs", None, o), ex("rewards", None, rw), ex("dones", None, d)
    ex("full", None, [t.obs[0, -1] for t in r.truth.o])
    if not pc.driving(cfg):
        ex("global", None, r.ora.global_state())
    ex("counts", None, r.ora.counts())
    for name, want in zip(("ep_r", "ep_p", "ep_o", "goals"), r.ora.stats()):
        ex(name, None, want)
    ex("flags", None, np.zeros((E, 1), np.int32))
    got = r.ar.get("blobs", shape=(E, -1), image=img)
    for e in range(E):
        ab.assert_blob_is_oracle_state(cfg, got[e], r.ora.get_state(e), "dynenv_get_states on the side stream, environment %d" % e)
    ex("blobs", None, got.copy())
    ex("status", None, np.zeros((n, 1), np.int32))
    ex("blobs_sub", None, src)   # what dynenv_set_states wrote reads back as written
    r.ar.verify("%s: the sequence on the side stream" % cfg, image=img)
    # dynenv_set_states took effect where the oracle's set_state did: the next step, on torch's current stream again
    from dynenv_amd import _capi
    for k, e in enumerate(ids):
        r.ora.set_state(e, _capi.state_struct(r.c.env_type).from_buffer_copy(src[k].tobytes()))
        r.truth.set_state(e, _capi.state_struct(r.c.env_type).from_buffer_copy(src[k].tobytes()))
    abi.stream = None
    r.step(after)
    r.close()


# ------------------------------------------------------------------------------------------------ d. alignment
def test_a_misaligned_observation_buffer_is_refused_and_nothing_is_touched(oracle_built):
    """d. a driving10 handle twelve steps into its situation, obs_dev / full_dev at 16 k + 4 (and + 8, + 12): DYNENV_ERR_ARG from every
    call that takes one, no byte of the arena and none of the handle changes, no error bit"""
    r = Run("driving10", "E5")
    twin = pc.situation("driving10", r.E, episodes="per_env")
    for a, _ in r.actions(STEPS, 41):
        r.step(a)
        pc.step(twin, a, auto_reset=False)
    assert pc.ckpt_diff(r.env, twin) == "", "same configuration, same history"
    a, _ = r.actions(1, 43)[0]
    r.ar.put("actions", a)
    r.ar.put("mask", r.mask(r.M))
    assert r.ar.bufs["obs"].start % 16 == 0 and r.ar.bufs["full"].start % 16 == 0
    for plus in (4, 8, 12):
        for name, call in (("dynenv_step", r.abi.step), ("dynenv_step_masked", r.abi.step_masked), ("dynenv_reset", r.abi.reset),
                           ("dynenv_reset_masked", r.abi.reset_masked)):
            assert call("obs", plus) == ab.ERR_ARG, (name, plus)
            assert "obs_dev must be 16-byte aligned" in r.abi.last_error(), (name, r.abi.last_error())
        assert r.abi.full_obs(plus) == ab.ERR_ARG and "full_dev must be 16-byte aligned" in r.abi.last_error()
    r.ar.verify("refused calls")
    assert pc.ckpt_diff(r.env, twin) == ""
    assert r.env.error_flags() == 0
    r.step(a)   # ... and at 16 k the same call is the oracle's next step
    twin.close()
    r.close()
