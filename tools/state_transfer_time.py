#!/usr/bin/env python3
"""What moving every environment's state costs, per environment through the host (get_state / set_state loops: one launch of the state
kernels for ONE blob and one copy through host memory per call) against one batched, device-side call of the same kernels (get_states /
set_states), for Driving with 10 cars and RoboCup with 5 robots per team.  The loops are timed on the
wall clock (they synchronise the device themselves); each batched call is timed with a pair of HIP events around the C entry point on
preallocated buffers, median (min .. max) of --calls calls after a warm-up, next to a plain device-to-device copy of the same
n x state_size bytes timed the same way in the same run.  "Rate" is blob bytes per second (n x state_size / time) for the kernels and
for the copy alike.  --repeats repeats the whole measurement on fresh handles: the run-to-run spread.
Usage (GPU box): python tools/state_transfer_time.py [--envs 4096] [--calls 20] [--repeats 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dynenv_amd import BatchedDynEnv, DynEnvType, _capi  # noqa: E402


def event_times(f, calls, warmup=5):
    """device microseconds of each of `calls` calls of f, every call between its own pair of events"""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def summary(us):
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us))


def measure(name, env_type, players, hi, E, calls, seed):
    env = BatchedDynEnv(env_type, E, players, seed=seed)
    env.reset_flat()
    rng = np.random.default_rng(seed)
    for _ in range(30):  # mid-episode: pedestrians under way, contacts cached
        a = np.stack([rng.integers(0, h, (E, env.n_agents)) for h in hi], -1).astype(np.int32)
        env.step_flat(torch.tensor(a, device="cuda"), auto_reset=False)
    torch.cuda.synchronize()
    size, lib, h = env.state_size, env._lib, env._h
    nbytes = E * size
    t0 = time.perf_counter()
    sts = [env.get_state(e) for e in range(E)]
    t_get_loop = time.perf_counter() - t0
    t0 = time.perf_counter()
    for e, st in enumerate(sts):
        env.set_state(e, st)
    torch.cuda.synchronize()
    t_set_loop = time.perf_counter() - t0
    blobs = torch.empty((E, size), dtype=torch.uint8, device="cuda")
    other = torch.empty_like(blobs)
    status = torch.empty((E,), dtype=torch.int32, device="cuda")
    stream = env._stream()
    get = lambda: _capi.check(lib.dynenv_get_states(h, None, E, C.c_void_p(blobs.data_ptr()), stream), "dynenv_get_states")
    put = lambda: _capi.check(lib.dynenv_set_states(h, None, E, C.c_void_p(blobs.data_ptr()), C.c_void_p(status.data_ptr()), stream),
                              "dynenv_set_states")
    g = summary(event_times(get, calls))
    host = np.stack([np.frombuffer(bytes(s), np.uint8) for s in sts])
    assert np.array_equal(blobs.cpu().numpy(), host), "the batched read must be the loop's bytes"
    s = summary(event_times(put, calls))
    assert int(status.abs().sum()) == 0 and env.error_flags() == 0
    c = summary(event_times(lambda: other.copy_(blobs), calls))
    # (the permuted list: the same work through an index list)
    perm = torch.randperm(E, device="cuda").to(torch.int32)
    gp = summary(event_times(lambda: _capi.check(lib.dynenv_get_states(h, C.c_void_p(perm.data_ptr()), E, C.c_void_p(blobs.data_ptr()), stream),
                                                 "dynenv_get_states"), calls))
    env.close()
    rate = lambda t: nbytes / (t["median_us"] * 1e-6) / 1e9
    res = dict(config=name, envs=E, state_size=size, blob_bytes=nbytes, get_state_loop_s=t_get_loop, set_state_loop_s=t_set_loop,
               get_states=g, set_states=s, get_states_permuted=gp, d2d_copy=c, get_states_GBps=rate(g), set_states_GBps=rate(s),
               d2d_copy_GBps=rate(c), get_speedup=t_get_loop / (g["median_us"] * 1e-6), set_speedup=t_set_loop / (s["median_us"] * 1e-6))
    fmt = lambda t: "%8.1f us (%.1f .. %.1f)" % (t["median_us"], t["min_us"], t["max_us"])
    print("== %s: %d environments x %d bytes = %.2f MB" % (name, E, size, nbytes / 1e6))
    print("get_state loop           %8.3f s      set_state loop           %8.3f s" % (t_get_loop, t_set_loop))
    print("get_states, one call     %s  %7.1f GB/s   x %.0f" % (fmt(g), rate(g), res["get_speedup"]))
    print("get_states, permuted ids %s  %7.1f GB/s" % (fmt(gp), rate(gp)))
    print("set_states, one call     %s  %7.1f GB/s   x %.0f" % (fmt(s), rate(s), res["set_speedup"]))
    print("device-to-device copy    %s  %7.1f GB/s" % (fmt(c), rate(c)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the results as JSON to this file as well")
    args = ap.parse_args()
    results = []
    for r in range(args.repeats):
        print("---- repeat %d of %d" % (r + 1, args.repeats))
        results.append(measure("Driving, 10 cars", DynEnvType.DRIVE, 10, [3, 3], args.envs, args.calls, 42 + r))
        results.append(measure("RoboCup, 5 per team", DynEnvType.ROBO_CUP, 5, [5, 3, 3, 7], args.envs, args.calls, 42 + r))
        sys.stdout.flush()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
