"""What the tests of the C ABI's caller-owned buffers share (tests/test_gpu_abi_buffers.py): an ARENA - one device allocation out of which
every buffer a call takes is carved, at the weakest alignment include/dynenv.h allows and with a guard band on either side -, thin
wrappers that call the C ABI directly with arena pointers, the per-environment oracles the arena's contents are held against, and the
delay of the stream-order test.  A helper module: no test in here.

The arena keeps, next to the device bytes, what every interior is EXPECTED to hold (`exp`): the sentinel pattern at first, what put()
wrote for an input, the oracle's rows once a test says so (expect_rows).  verify() then checks in one pass that no guard byte changed,
that every output holds the oracle's bits in the rows a call wrote and what it held before in the others, that no call wrote into a
buffer it was not given, and that every input is byte for byte what was put there."""
import collections
import ctypes as C

import numpy as np

import per_env_common as pc
from parity_common import _assert_rc_state_equal, _assert_state_equal

FILL = 0xC3                                                                   # the guard bands' byte
PATTERN = np.frombuffer(np.int32(pc.SENTINEL).tobytes(), dtype=np.uint8)      # what interiors are pre-filled with: 55 1E A7 5E
OK, ERR_ARG = 0, -1
# a buffer's byte offset modulo 256, by kind: the weakest alignment the header allows
OBS, F64, I32, U8, BLOB, EXACT = 16, 8, 4, 1, 8, 16   # obs / full: 16 mod 256; float64: 8 mod 16; int32 / float32: 4 mod 8; bytes: odd; blobs: 8 mod 16, exact 16 mod 32

# configurations of this module's own, on top of per_env_common's table: Driving Full with 3 cars (obs_dim 183: the scalar path of the
# Full writer) and with 6 (the float4 path at a car count that is neither 2 nor 10), RoboCup with the continuous head channel
EXTRA = {"driving3": pc.Cfg(1, 3, (3, 3), False, 0, 12), "driving6": pc.Cfg(1, 6, (3, 3), False, 0, 12),
         "robocup5_head": pc.CFGS["robocup5"]._replace(flags=pc.CFGS["robocup5"].flags | 16)}


def cfg_of(name):
    return EXTRA[name] if name in EXTRA else name   # (a name of per_env_common's table stays a name: pile_envs looks names up)


Buf = collections.namedtuple("Buf", "name lo start end hi")   # guards: [lo, start) below, [end, hi) above


class Arena:
    def __init__(self, specs):
        """specs: (name, bytes, offset modulo 256, bytes of ONE environment's slab of it); a guard band is at least twice the slab,
        rounded up to 256 bytes, so that an environment index one too high lands in the guard and not outside the allocation"""
        import torch
        self.bufs, off = {}, 0
        for name, nbytes, residue, slab in specs:
            guard = max(256, -(-2 * slab // 256) * 256)
            start = off + guard
            start += (residue - start) % 256
            self.bufs[name] = Buf(name, off, start, start + nbytes, start + nbytes + guard)
            off = start + nbytes + guard
            assert start % 256 == residue and start - self.bufs[name].lo >= guard
        self.size = -(-off // 256) * 256
        self.mem = torch.full((self.size,), FILL, dtype=torch.uint8, device="cuda")
        assert self.mem.data_ptr() % 256 == 0
        guard = np.ones((self.size,), np.bool_)
        self.exp = {}
        for b in self.bufs.values():
            guard[b.start:b.end] = False
            self.exp[b.name] = np.resize(PATTERN, b.end - b.start).copy()
            self.mem[b.start:b.end].copy_(torch.from_numpy(self.exp[b.name]))
        self.is_guard = guard

    def ptr(self, name, plus=0):
        return None if name is None else C.c_void_p(self.mem.data_ptr() + self.bufs[name].start + plus)

    def view(self, name):
        b = self.bufs[name]
        return self.mem[b.start:b.end]

    def put(self, name, array, non_blocking=False):
        """write an input (on torch's current stream) and expect it to stay what it is"""
        import torch
        host = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert host.size == self.exp[name].size, (name, host.size, self.exp[name].size)
        self.exp[name] = host.copy()
        src = torch.from_numpy(self.exp[name])
        self.view(name).copy_(src.pin_memory() if non_blocking else src, non_blocking=non_blocking)

    def refill(self, name, pattern=PATTERN):
        import torch
        self.exp[name] = np.resize(np.asarray(pattern, np.uint8), self.exp[name].size).copy()
        self.view(name).copy_(torch.from_numpy(self.exp[name]))

    def image(self):
        return self.mem.cpu().numpy()

    def get(self, name, dtype=np.uint8, shape=(-1,), image=None):
        b = self.bufs[name]
        raw = self.view(name).cpu().numpy() if image is None else image[b.start:b.end]
        return np.ascontiguousarray(raw).view(dtype).reshape(shape)

    def expect_rows(self, name, rows, values):
        """rows `rows` (None: all) of buffer `name`, seen as [len(values-of-all-rows), -1], now hold `values` (any dtype, one entry per row)"""
        values = [np.ascontiguousarray(v).view(np.uint8).reshape(-1) for v in values]
        e = self.exp[name].reshape(-1, values[0].size)
        for r, v in zip(range(e.shape[0]) if rows is None else rows, values):
            e[r] = v

    def assert_guards(self, what="", image=None):
        img = self.image() if image is None else image
        bad = np.nonzero((img != FILL) & self.is_guard)[0]
        if bad.size:
            i = int(bad[0])
            for b in self.bufs.values():
                if b.lo <= i < b.start:
                    raise AssertionError("%s: the guard band BELOW %s was written: first changed byte %d bytes before the buffer (arena offset %d), "
                                         "%d guard bytes changed in all" % (what, b.name, b.start - i, i, bad.size))
                if b.end <= i < b.hi:
                    raise AssertionError("%s: the guard band ABOVE %s was written: first changed byte at offset %d past the buffer's end (arena "
                                         "offset %d), %d guard bytes changed in all" % (what, b.name, i - b.end, i, bad.size))
            raise AssertionError("%s: the arena's tail was written at offset %d" % (what, i))

    def verify(self, what="", image=None):
        """no guard byte changed, and every interior - outputs and inputs alike - holds what it is expected to hold"""
        img = self.image() if image is None else image
        self.assert_guards(what, img)
        for b in self.bufs.values():
            got = img[b.start:b.end]
            if not np.array_equal(got, self.exp[b.name]):
                d = np.nonzero(got != self.exp[b.name])[0]
                raise AssertionError("%s: %s differs from what it should hold in %d of %d bytes, first at byte %d" % (what, b.name, d.size, got.size, d[0]))


def arena_for(env, n_listed):
    """every buffer the environment calls of `env` take; rewards, obs and full first, in this order"""
    E, T, A, D, K = env.num_envs, env.n_time_steps, env.n_agents, env.obs_dim, env.action_dim
    Fd, S, X, n = env.full_obs_dim, env.state_size, env.exact_size, n_listed
    G = 6 * A + 3
    specs = [("rewards", E * A * 8, F64, A * 8), ("obs", E * T * A * D * 4, OBS, T * A * D * 4), ("full", E * A * Fd * 4, OBS, A * Fd * 4),
             ("global", E * G * 4, I32, G * 4), ("dones", E, U8, 1), ("mask", E, U8, 1), ("actions", E * A * K * 4, I32, A * K * 4),
             ("head", E * A * 8, F64, A * 8), ("counts", E * 8, I32, 8), ("goals", E * 8, I32, 8), ("flags", E * 4, I32, 4),
             ("ep_r", E * A * 8, F64, A * 8), ("ep_p", E * A * 8, F64, A * 8), ("ep_o", E * A * 8, F64, A * 8),
             ("env_idx", n * 4, I32, 4), ("exact_idx", (n + 1) * 4, I32, 4), ("status", n * 4, I32, 4), ("blobs", E * S, BLOB, S),
             ("blobs_sub", n * S, BLOB, S), ("src_blobs", n * S, BLOB, S), ("exact", (n + 1) * X, EXACT, X)]
    return Arena(specs)


class Abi:
    """the C ABI called directly with arena pointers; every method returns the call's return code.  `stream`: a torch stream to pass
    (None: torch's current one)"""

    def __init__(self, env, arena, stream=None):
        self.env, self.lib, self.h, self.ar, self.stream = env, env._lib, env._h, arena, stream

    def s(self):
        return self.env._stream() if self.stream is None else C.c_void_p(self.stream.cuda_stream)

    def reset(self, obs="obs", plus=0):
        return self.lib.dynenv_reset(self.h, self.ar.ptr(obs, plus), self.s())

    def reset_masked(self, obs="obs", plus=0):
        return self.lib.dynenv_reset_masked(self.h, self.ar.ptr("mask"), self.ar.ptr(obs, plus), self.s())

    def step(self, obs="obs", plus=0):
        p = self.ar.ptr
        return self.lib.dynenv_step(self.h, p("actions"), p(obs, plus), p("rewards"), p("dones"), self.s())

    def step_head(self, obs="obs", plus=0, head="head"):
        p = self.ar.ptr
        return self.lib.dynenv_step_head(self.h, p("actions"), p(head), p(obs, plus), p("rewards"), p("dones"), self.s())

    def step_masked(self, obs="obs", plus=0, head=None):
        p = self.ar.ptr
        return self.lib.dynenv_step_masked(self.h, p("mask"), p("actions"), p(head), p(obs, plus), p("rewards"), p("dones"), self.s())

    def full_obs(self, plus=0):
        return self.lib.dynenv_full_obs(self.h, self.ar.ptr("full", plus), self.s())

    def global_state(self):
        return self.lib.dynenv_global_state(self.h, self.ar.ptr("global"), self.s())

    def counts(self):
        return self.lib.dynenv_counts(self.h, self.ar.ptr("counts"), self.s())

    def episode_stats(self, r="ep_r", p="ep_p", o="ep_o", g="goals"):
        q = self.ar.ptr
        return self.lib.dynenv_episode_stats(self.h, q(r), q(p), q(o), q(g), self.s())

    def error_flags_env(self):
        return self.lib.dynenv_error_flags_env(self.h, self.ar.ptr("flags"), self.s())

    def get_states(self, idx, n, blobs):
        return self.lib.dynenv_get_states(self.h, self.ar.ptr(idx), n, self.ar.ptr(blobs), self.s())

    def set_states(self, idx, n, blobs, status="status"):
        return self.lib.dynenv_set_states(self.h, self.ar.ptr(idx), n, self.ar.ptr(blobs), self.ar.ptr(status), self.s())

    def get_exact(self, idx, n, blobs="exact"):
        return self.lib.dynenv_get_exact(self.h, self.ar.ptr(idx), n, self.ar.ptr(blobs), self.s())

    def last_error(self):
        return self.lib.dynenv_last_error().decode("utf-8", "replace")


# ------------------------------------------------------------------------------------------------ the oracle's side
class Oracles:
    """environment e of a batch as an oracle of its own (per_env_common.env_oracle), E of them: what a masked call leaves alone is an
    oracle that is not called.  truth=True: the same batch with Full observations - its observation is the noise-free state that
    dynenv_full_obs of a Partial handle must return (tests/test_gpu_player_counts.py)"""

    def __init__(self, cfg, E, truth=False):
        c = pc.cfg_of(cfg)
        self.c = c._replace(partial=False) if truth else c
        self.E = E
        self.o = [pc.env_oracle(self.c, e) for e in range(E)]

    def envs(self, listed):
        return range(self.E) if listed is None else listed

    def reset(self, listed=None):
        """-> the first observations of the listed environments, in that order"""
        return [self.o[e].reset()[0].copy() for e in self.envs(listed)]

    def step(self, act, listed=None, head=None, noobs=False):
        """-> (observations or None, rewards, dones) of the listed environments, in that order"""
        obs, rew, done = [], [], []
        for e in self.envs(listed):
            if noobs:
                r, d = self.o[e].step_noobs(act[e:e + 1])
            else:
                o, r, d = self.o[e].step(act[e:e + 1], None if head is None else head[e:e + 1])
                obs.append(o[0].copy())
            rew.append(r[0].copy())
            done.append(d[0].copy())
        return (None if noobs else obs), rew, done

    def set_state(self, e, st):
        self.o[e].set_state(0, st)

    def get_state(self, e):
        return self.o[e].get_state(0)

    def stats(self):
        """-> (r, p, o [E, A] float64, g [E, 2] int32)"""
        per = [o.episode_stats() for o in self.o]
        return tuple(np.concatenate([p[k] for p in per]) for k in range(4))

    def counts(self):
        return np.concatenate([o.counts() for o in self.o])

    def global_state(self):
        return np.concatenate([o.global_state() for o in self.o])

    def clean(self):
        return all(o.overflow() == 0 and o.degenerate() == 0 for o in self.o)

    def close(self):
        for o in self.o:
            o.close()


def copy_of(st):
    return type(st).from_buffer_copy(bytes(st))


def prepared(cfg, E, reset=True):
    """-> (handle, its oracles, the Full-observation oracles of a Partial handle or None).  A pile configuration: per_env_common.situation
    - HISTORY + 2 steps in, live contacts in the pile environments - and oracles brought there by the same calls.  Any other
    configuration: a new handle, reset (reset=False: not yet, and neither are the oracles)."""
    name = cfg
    cfg = cfg_of(cfg)
    c = pc.cfg_of(cfg)
    sides = [Oracles(cfg, E)] + ([Oracles(cfg, E, truth=True)] if c.partial else [])
    piles = pc.pile_envs(cfg, E)
    if not piles:
        env = pc.make(cfg, E, episodes="per_env")
        if reset:
            env.reset_flat()
            for o in sides:
                o.reset()
        return env, sides[0], (sides[1] if c.partial else None)
    env = pc.situation(name, E, episodes="per_env")
    new = pc.make(cfg, E)   # the blobs situation() wrote its piles into: those of a handle just reset
    new.reset_flat()
    blank = {e: new.get_state(e) for e in piles}
    new.close()
    A = env.n_agents
    for o in sides:
        o.reset()
        for a in pc.actions(cfg, E, A, pc.HISTORY, 5):
            o.step(a)
        for e in piles:
            o.set_state(e, pc.write_pile(cfg, copy_of(blank[e]), pc.HISTORY))
        for a in pc.actions(cfg, E, A, 2, 6, idle=piles):
            o.step(a)
    return env, sides[0], (sides[1] if c.partial else None)


def assert_blob_is_oracle_state(cfg, blob_bytes, want, msg):
    """a canonical blob as the device wrote it, against the oracle's state of that environment: field by field, bit for bit"""
    from dynenv_amd import _capi
    c = pc.cfg_of(cfg_of(cfg))
    st = _capi.state_struct(c.env_type).from_buffer_copy(bytes(blob_bytes))
    (_assert_state_equal if c.env_type == 1 else _assert_rc_state_equal)(st, want, msg)


def head_actions(E, A, steps, seed):
    """the continuous head channel, Box(-3, 3): [steps] of float64 [E, A]"""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-3.0, 3.0, (E, A)) for _ in range(steps)]


# ------------------------------------------------------------------------------------------------ the stream test's delay
SLEEP_PROBE_CYCLES = 2_000_000
_sleep_cycles = {}


def delay_cycles(target_ms=25.0):
    """how many cycles torch.cuda._sleep must spin for about `target_ms`: its clock's rate is the device's business, so it is timed once
    (a probe of SLEEP_PROBE_CYCLES between two events) and scaled; 0 if this build has no working _sleep"""
    import torch
    if target_ms not in _sleep_cycles:
        cycles = 0
        if hasattr(torch.cuda, "_sleep"):
            try:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(1000)   # (first use)
                a.record()
                torch.cuda._sleep(SLEEP_PROBE_CYCLES)
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
                if ms > 0.05:
                    cycles = int(min(SLEEP_PROBE_CYCLES * target_ms / ms, 2e9))
            except Exception:
                cycles = 0
        _sleep_cycles[target_ms] = cycles
    return _sleep_cycles[target_ms]


def enqueue_delay(cycles):
    """a delay on torch's CURRENT stream: _sleep(cycles), or - cycles == 0 - a chain of large tensor operations"""
    import torch
    if cycles > 0:
        torch.cuda._sleep(cycles)
        return
    x = torch.ones((8192, 8192), device="cuda")
    for _ in range(40):
        x = x * 1.0000001 + 1e-9
