#!/usr/bin/env python3
"""The input layer's arranger in its two modes, from ONE run: rearrange_inputs + rearrange_outputs + backward on the movable group of real
observations, (a) the default mode (shapes from the batch: dynenv_arrange_plan waits for the device), (b) the fixed-shape mode with
rows = the types' capacities and M = their sum (GpuInOutArranger(fixed=True)), (c) the fixed-shape mode with M = the batch's own maxCount.
Per leg: the device time between HIP events, the host time for which the call holds the CPU (wall time around the call, nothing
synchronised inside it) and the bytes it writes.  The legs take turns inside every repeat.

Usage (GPU box):  python tools/fixed_arranger_time.py [--envs 4096] [--feat 128] [--calls 20] [--repeats 3] [--out FILE]

The fixed mode writes M / maxCount times the padded bytes and hands the blocks capacity rows; what it buys is that the host does not
wait (the host column) and that the calls can be captured.  The embedding blocks themselves are not part of any leg: the embeddings are
given tensors of the shape each mode would hand on."""
import json
import statistics
import time

import timing_common as tc

# (name, DynEnvType's name, players, the actions' exclusive upper bounds, keyword arguments of the handle)
CONFIGS = (("Driving Full", "DRIVE", 10, (3, 3), {}),
           ("Driving Partial + Realistic 3", "DRIVE", 10, (3, 3), dict(partial=True, noise=3)),
           ("RoboCup Full", "ROBO_CUP", 5, (5, 3, 3, 7), {}))


def make_leg(torch, arr, obs, ce, F):
    """(call, bytes written) of one arranger: the call is rearrange_inputs + rearrange_outputs + backward; its embeddings and its upstream
    gradient have the shapes a first call of this arranger on this batch gives"""
    inputs, plan = arr.rearrange_inputs(obs, ce)
    outs = [torch.randn((int(i.shape[0]), F), device="cuda").requires_grad_() if i.shape[0] else None for i in inputs]
    live = [o for o in outs if o is not None]
    padded, _ = arr.rearrange_outputs(outs, plan)
    up = torch.randn(tuple(padded.shape), device="cuda")

    def call():
        _, p = arr.rearrange_inputs(obs, ce)
        pad, _ = arr.rearrange_outputs(outs, p)
        return torch.autograd.grad(pad, live, up)

    n, T, P = (int(v) for v in plan[0].shape)
    M = int(plan[1])
    rows_in = sum(int(i.numel()) for i in inputs) * 4
    plan_ints = n * T * P + T * P + (0 if arr.fixed else n * T * P + sum(int(i.shape[0]) for i in inputs))   # counts, objCounts (+ base, slots)
    written = rows_in + plan_ints * 4 + T * P * M + int(padded.numel()) * 4 + sum(int(o.numel()) for o in live) * 4
    return call, written, M, sum(int(i.shape[0]) for i in inputs)


def time_legs(torch, legs, calls, repeats):
    """{leg: (device us per repeat, host us per repeat)}: medians over `calls` calls, the legs taking turns inside every repeat"""
    dev, host = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(repeats):
        for k, call in legs.items():
            wall = []

            def timed():
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e6)

            dev[k].append(statistics.median(tc.event_times(torch, timed, calls)))
            host[k].append(statistics.median(wall[-calls:]))
    return dev, host


def main(argv=None):
    ap = tc.base_parser(__doc__, calls_help="timed calls per leg and repeat")
    ap.add_argument("--feat", type=int, default=128, help="embedding width F (a multiple of 4)")
    args = tc.parse_positive(ap, argv, also=("feat",))
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuInOutArranger, NoiseType, ObservationType, groups_for
    E, F = args.envs, args.feat
    results = []
    for name, env_type, players, hi, kw in CONFIGS:
        extra = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=kw["noise"]) if kw else {}
        env = BatchedDynEnv(DynEnvType[env_type], E, players, seed=42, **extra)
        tc.mid_episode(env, tc.action_pool(torch, np, hi, E, env.n_agents, seed=1), steps=20)
        obs, ce = env.obs.contiguous(), env.counts()
        types = groups_for(env)["movable"]
        shape = (types, E, env.n_agents, env.n_time_steps, env.obs_dim)
        default = GpuInOutArranger(*shape)
        m0 = int(default.rearrange_inputs(obs, ce)[1][1])
        caps = [int(t.cap) for t in types]
        arrs = {"default": default, "fixed, M = sum of caps": GpuInOutArranger(*shape, fixed=True),
                "fixed, M = batch maxCount": GpuInOutArranger(*shape, fixed=dict(max_count=m0, rows=caps))}
        made = {k: make_leg(torch, a, obs, ce, F) for k, a in arrs.items()}
        dev, host = time_legs(torch, {k: m[0] for k, m in made.items()}, args.calls, args.repeats)
        assert not any(bool(a.dropped.any()) for a in arrs.values() if a.fixed), "rows = caps and M >= maxCount drop nothing"
        print("%s, %d environments, F = %d, caps %s, batch maxCount %d" % (name, E, F, caps, m0))
        legs = {}
        for k, (_, written, M, n_rows) in made.items():
            print("  %-26s M %3d  rows %9d  written %7.1f MB  device %s  host %s" % (k, M, n_rows, written / 1e6, tc.fmt(dev[k]), tc.fmt(host[k])))
            legs[k] = {"max_count": M, "embedding_rows": n_rows, "bytes_written": written, "device_us": dev[k], "host_us": host[k]}
        results.append({"config": name, "envs": E, "embed_width": F, "caps": caps, "batch_max_count": m0, "calls": args.calls, "legs": legs})
        env.close()
    print(json.dumps(results))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
