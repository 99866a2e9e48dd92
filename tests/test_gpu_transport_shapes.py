"""The multi-GPU transport kernels (dynenv_obs_pack / _unpack / _unpack_ranks / _pack_peers / _unpack_peers_ranks) bit for bit
against their numpy index maps (dynenv_amd.distributed.pack_*_np / unpack_*_np) at the shapes that select each expansion kernel:
the row kernel with several rows per block (batches of 4 double-buffered in LDS, partial last batches and blocks, the configs[4]
shape of 8 ranks x 4096 Driving Full environments), the float4 and the scalar per-thread kernels, a misaligned destination.
The ranks' packed blocks sit `src_stride` apart with junk in the gaps, and every dense output has guard bands."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64                     # floats on either side of an output (keeps 16-byte alignment)
SENT = np.float32(-31415.25)   # guard bands
GAP_JUNK = np.float32(999.5)   # between the ranks' packed blocks
PEER_SELF, PEER_COLS = 9, 7


def _lib():
    import torch
    from dynenv_amd import _capi
    return _capi, _capi.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n, offset=0):
    import torch
    buf = torch.full((n + 2 * GUARD + offset,), float(SENT), dtype=torch.float32, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _assert_guards(buf, n, offset=0):
    b = buf.cpu().numpy()
    assert (b[:GUARD + offset] == SENT).all(), "guard band before the output overwritten"
    assert (b[GUARD + offset + n:] == SENT).all(), "guard band after the output overwritten"


def _gathered(rng, G, nET, row, gap):
    """G packed blocks of nET rows of `row` floats, `row * nET + gap` floats apart, junk in the gaps"""
    stride = nET * row + gap
    g = np.full((G, stride), GAP_JUNK, np.float32)
    g[:, :nET * row] = rng.standard_normal((G, nET * row)).astype(np.float32)
    return g, stride


def _peer_kernel(nET, G, A, D, aligned):
    """which expansion kernel dynenv_obs_unpack_peers_ranks selects (csrc/dynenv_capi.hip), and the row kernel's rows per block"""
    vec = D % 4 == 0 and aligned
    if vec and A <= 16 and D - (PEER_SELF + (A - 1) * PEER_COLS) <= 160:
        return "rows", min(max((nET * G + 4095) // 4096, 1), 32)
    return ("peers4" if vec else "peers1"), 0


# (kernel, rows per block, ranks, n_env_time, A, tail, destination offset in floats)
PEER_CASES = [
    ("rows", 8, 8, 4096, 10, 160, 0),     # configs[4]: 8 ranks x 4096 Driving Full (D = 232), two batches of 4 per block
    ("rows", 5, 4, 4099, 10, 160, 0),     # a batch of 4 and one of 1; the last block 4 rows
    ("rows", 3, 3, 3001, 2, 0, 0),        # tail 0; the last block 1 row
    ("rows", 2, 2, 2051, 1, 3, 0),        # A = 1 (no other car)
    ("rows", 3, 2, 4099, 16, 158, 0),     # A = 16, the row kernel's largest
    ("rows", 32, 1, 130001, 2, 0, 0),     # the 32-row cap: 8 batches, the last block 17 rows
    ("rows", 1, 1, 100, 14, 160, 0),
    ("peers4", 0, 2, 333, 17, 3, 0),      # A = 17
    ("peers4", 0, 3, 257, 10, 164, 0),    # tail 164
    ("peers1", 0, 2, 301, 10, 161, 0),    # D % 4 != 0
    ("peers1", 0, 2, 301, 1, 0, 0),       # A = 1, D = 9
    ("peers1", 0, 2, 300, 10, 160, 1),    # D = 232 but the destination one float off 16-byte alignment
]


@pytest.mark.parametrize("kernel, rpb, G, nET, A, tail, off", PEER_CASES,
                         ids=["%s-rpb%d-G%d-n%d-A%d-tail%d-off%d" % c for c in PEER_CASES])
def test_unpack_peers_ranks(kernel, rpb, G, nET, A, tail, off):
    import torch
    from dynenv_amd.distributed import unpack_peers_np
    capi, lib, st = _lib()
    D = PEER_SELF + (A - 1) * PEER_COLS + tail
    P = A * PEER_SELF + tail
    assert _peer_kernel(nET, G, A, D, off % 4 == 0) == (kernel, rpb)
    rng = np.random.default_rng(nET + A)
    g, stride = _gathered(rng, G, nET, P, gap=37)
    want = np.concatenate([unpack_peers_np(g[r, :nET * P].reshape(nET, P), A, D) for r in range(G)])
    src = torch.from_numpy(g).cuda()
    n = G * nET * A * D
    buf, out = _guarded(n, off)
    capi.check(lib.dynenv_obs_unpack_peers_ranks(C.c_void_p(src.data_ptr()), stride, G, nET, A, D, C.c_void_p(out.data_ptr()), st),
               "dynenv_obs_unpack_peers_ranks")
    got = out.cpu().numpy().reshape(want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%d of %d floats differ, first at (row, agent, col) %s" % (len(bad), got.size, bad[0].tolist()))
    _assert_guards(buf, n, off)


@pytest.mark.parametrize("nET, A, tail", [(301, 10, 160), (77, 1, 0), (129, 17, 3), (50, 16, 161)])
def test_pack_peers(nET, A, tail):
    """dynenv_obs_pack_peers == pack_peers_np on any dense tensor (agent 0's tail), nothing written past the packed rows"""
    import torch
    from dynenv_amd.distributed import pack_peers_np
    capi, lib, st = _lib()
    D = PEER_SELF + (A - 1) * PEER_COLS + tail
    rng = np.random.default_rng(A * 1000 + tail)
    x = rng.standard_normal((nET, A, D)).astype(np.float32)
    want = pack_peers_np(x)
    buf, out = _guarded(want.size)
    capi.check(lib.dynenv_obs_pack_peers(C.c_void_p(torch.from_numpy(x).cuda().data_ptr()), nET, A, D, C.c_void_p(out.data_ptr()), st),
               "dynenv_obs_pack_peers")
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    _assert_guards(buf, want.size)


# (ranks, n_env_time, A, D, split): split 0 (all tail), split D (no tail), A = 1; totals not multiples of the 256-thread block
TAIL_CASES = [(3, 37, 3, 11, 0), (3, 37, 3, 11, 11), (2, 1001, 10, 232, 72), (5, 7, 1, 5, 2), (4, 513, 5, 217, 100)]


@pytest.mark.parametrize("G, nET, A, D, split", TAIL_CASES)
def test_tail_pack_and_unpack_ranks(G, nET, A, D, split):
    import torch
    from dynenv_amd.distributed import pack_tail_np, unpack_tail_np
    capi, lib, st = _lib()
    vp = C.c_void_p
    rng = np.random.default_rng(G * 100 + D + split)
    P = A * split + (D - split)
    # pack: every rank's dense tensor into its block of the gathered buffer (the tail of agent 0 travels)
    x = rng.standard_normal((G, nET, A, D)).astype(np.float32)
    for r in range(G):
        want = pack_tail_np(x[r], split)
        buf, out = _guarded(nET * P)
        capi.check(lib.dynenv_obs_pack(vp(torch.from_numpy(x[r]).cuda().data_ptr()), nET, A, D, split, vp(out.data_ptr()), st),
                   "dynenv_obs_pack")
        assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
        _assert_guards(buf, nET * P)
    # unpack_ranks: G blocks `stride` apart, junk in the gaps
    g, stride = _gathered(rng, G, nET, P, gap=29)
    want = np.concatenate([unpack_tail_np(g[r, :nET * P].reshape(nET, P), A, D, split) for r in range(G)])
    src = torch.from_numpy(g).cuda()
    n = G * nET * A * D
    buf, out = _guarded(n)
    capi.check(lib.dynenv_obs_unpack_ranks(vp(src.data_ptr()), stride, G, nET, A, D, split, vp(out.data_ptr()), st),
               "dynenv_obs_unpack_ranks")
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    _assert_guards(buf, n)
    # unpack of one block
    buf, out = _guarded(nET * A * D)
    capi.check(lib.dynenv_obs_unpack(vp(src[1 % G].data_ptr()), nET, A, D, split, vp(out.data_ptr()), st), "dynenv_obs_unpack")
    assert np.array_equal(out.cpu().numpy().reshape(nET, A, D), want[(1 % G) * nET:(1 % G + 1) * nET])
    _assert_guards(buf, nET * A * D)
