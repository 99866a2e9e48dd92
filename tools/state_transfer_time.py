#!/usr/bin/env python3
"""What moving every environment's state costs, per environment through the host (get_state / set_state loops: one launch of the state
kernels for ONE blob and one copy through host memory per call) against one batched, device-side call of the same kernels (get_states /
set_states), for Driving with 10 cars and RoboCup with 5 robots per team.  The loops are timed on the
wall clock (they synchronise the device themselves); each batched call is timed with a pair of HIP events around the C entry point on
preallocated buffers, median (min .. max) of --calls calls after a warm-up, next to a plain device-to-device copy of the same
n x state_size bytes timed the same way in the same run.  "Rate" is blob bytes per second (n x state_size / time) for the kernels and
for the copy alike.  --repeats repeats the whole measurement on fresh handles: the run-to-run spread.
Usage (GPU box): python tools/state_transfer_time.py [--envs 4096] [--calls 20] [--repeats 3] [--out FILE]"""
import statistics
import sys
import time

from timing_common import action_pool, base_parser, event_times, mid_episode, parse_positive, write_json

import numpy as np
import torch
from dynenv_amd import BatchedDynEnv, DynEnvType, _capi


def summary(us):
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us))


def measure(name, env_type, players, hi, E, calls, seed):
    env = BatchedDynEnv(env_type, E, players, seed=seed)
    mid_episode(env, action_pool(torch, np, hi, E, env.n_agents, seed, n=30))   # (30 steps, each with actions of its own)
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
    get = lambda: _capi.check(lib.dynenv_get_states(h, None, E, _capi.ptr(blobs), stream), "dynenv_get_states")
    put = lambda: _capi.check(lib.dynenv_set_states(h, None, E, _capi.ptr(blobs), _capi.ptr(status), stream),
                              "dynenv_set_states")
    g = summary(event_times(torch, get, calls, warmup=5))
    host = np.stack([np.frombuffer(bytes(s), np.uint8) for s in sts])
    assert np.array_equal(blobs.cpu().numpy(), host), "the batched read must be the loop's bytes"
    s = summary(event_times(torch, put, calls, warmup=5))
    assert int(status.abs().sum()) == 0 and env.error_flags() == 0
    c = summary(event_times(torch, lambda: other.copy_(blobs), calls, warmup=5))
    # (the permuted list: the same work through an index list)
    perm = torch.randperm(E, device="cuda").to(torch.int32)
    gp = summary(event_times(torch, lambda: _capi.check(lib.dynenv_get_states(h, _capi.ptr(perm), E, _capi.ptr(blobs), stream),
                                                 "dynenv_get_states"), calls, warmup=5))
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
    args = parse_positive(base_parser(__doc__, calls_help="timed calls of every batched call"))
    results = []
    for r in range(args.repeats):
        print("---- repeat %d of %d" % (r + 1, args.repeats))
        results.append(measure("Driving, 10 cars", DynEnvType.DRIVE, 10, [3, 3], args.envs, args.calls, 42 + r))
        results.append(measure("RoboCup, 5 per team", DynEnvType.ROBO_CUP, 5, [5, 3, 3, 7], args.envs, args.calls, 42 + r))
        sys.stdout.flush()
    write_json(results, args.out)


if __name__ == "__main__":
    main()
