#!/usr/bin/env python3
"""The input layer's arranger in its two modes, from ONE run: rearrange_inputs + rearrange_outputs + backward on the movable group of real
observations, (a) the default mode (shapes from the batch: dynenv_arrange_plan waits for the device), (b) the fixed-shape mode with
rows = the types' capacities and M = their sum (GpuInOutArranger(fixed=True)), (c) the fixed-shape mode with M = the batch's own maxCount.
Per leg: the device time between HIP events, the host time for which the call holds the CPU (wall time around the call, nothing
synchronised inside it) and the bytes it writes.  The legs take turns inside every repeat.

Usage (GPU box):  python tools/fixed_arranger_time.py [--envs 4096] [--feat 128] [--calls 20] [--repeats 3] [--out FILE]
                  [--padded-dtype bf16|f16 [--emb-dtype f32|bf16|f16]]

--padded-dtype bf16|f16 runs every one of the three arrangers with a float32 padded tensor AND with one of that type
(GpuInOutArranger(padded_dtype=...)), from float32 embeddings (the converting kernels) and from embeddings already in that type (a bit
copy; --emb-dtype keeps one of the two): all legs from the same run, taking turns, with the bytes each moves (read + written).

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


def make_leg(torch, arr, obs, ce, F, emb_dtype=None):
    """(call, bytes written, M, embedding rows, bytes moved) of one arranger: the call is rearrange_inputs + rearrange_outputs + backward;
    its embeddings (of emb_dtype, float32 if None) and its upstream gradient (of the padded tensor's type) have the shapes a first call
    of this arranger on this batch gives"""
    inputs, plan = arr.rearrange_inputs(obs, ce)
    emb_dtype = emb_dtype or torch.float32
    outs = [torch.randn((int(i.shape[0]), F), device="cuda").to(emb_dtype).requires_grad_() if i.shape[0] else None for i in inputs]
    live = [o for o in outs if o is not None]
    padded, _ = arr.rearrange_outputs(outs, plan)
    up = torch.randn(tuple(padded.shape), device="cuda").to(padded.dtype)

    def call():
        _, p = arr.rearrange_inputs(obs, ce)
        pad, _ = arr.rearrange_outputs(outs, p)
        return torch.autograd.grad(pad, live, up)

    n, T, P = (int(v) for v in plan[0].shape)
    M = int(plan[1])
    rows_in = sum(int(i.numel()) for i in inputs) * 4
    plan_ints = n * T * P + T * P + (0 if arr.fixed else n * T * P + sum(int(i.shape[0]) for i in inputs))   # counts, objCounts (+ base, slots)
    esize, psize = live[0].element_size(), padded.element_size()
    written = rows_in + plan_ints * 4 + T * P * M + int(padded.numel()) * psize + sum(int(o.numel()) for o in live) * esize
    kept = [int(k) for k in plan[0].reshape(n, -1).sum(1)]   # objects that own a slot: what the gather, the pad and the backward READ
    read = sum(k * int(i.shape[1]) * 4 for k, i in zip(kept, inputs)) + plan_ints * 4 + sum(kept) * F * (esize + psize)
    return call, written, M, sum(int(i.shape[0]) for i in inputs), written + read


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
    ap.add_argument("--feat", type=int, default=128, help="embedding width F (a multiple of 4; of 8 with --padded-dtype)")
    ap.add_argument("--padded-dtype", choices=("f32", "bf16", "f16"), default="f32",
                    help="bf16 / f16: every arranger also with a padded tensor of that type, beside its float32 leg, in the same run")
    ap.add_argument("--emb-dtype", choices=("f32", "bf16", "f16"), default=None,
                    help="with --padded-dtype: the embeddings' type of the 16-bit legs, f32 (converting) or the padded type (bit copy); default both")
    args = tc.parse_positive(ap, argv, also=("feat",))
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuInOutArranger, NoiseType, ObservationType, groups_for
    E, F = args.envs, args.feat
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    pk = args.padded_dtype
    emb_kinds = [] if pk == "f32" else ([args.emb_dtype] if args.emb_dtype else ["f32", pk])
    if any(k not in ("f32", pk) for k in emb_kinds):
        ap.error("--emb-dtype is f32 or the --padded-dtype")
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
        kinds = {"default": None, "fixed, M = sum of caps": True, "fixed, M = batch maxCount": dict(max_count=m0, rows=caps)}
        made = {k: make_leg(torch, a, obs, ce, F) for k, a in arrs.items()}
        for ek in emb_kinds:   # the 16-bit legs: the same three arrangers with padded_dtype set
            for k, fx in kinds.items():
                arrs["%s, %s -> %s" % (k, ek, pk)] = a = GpuInOutArranger(*shape, fixed=fx, padded_dtype=tdt[pk])
                made["%s, %s -> %s" % (k, ek, pk)] = make_leg(torch, a, obs, ce, F, tdt[ek])
        dev, host = time_legs(torch, {k: m[0] for k, m in made.items()}, args.calls, args.repeats)
        assert not any(bool(a.dropped.any()) for a in arrs.values() if a.fixed), "rows = caps and M >= maxCount drop nothing"
        print("%s, %d environments, F = %d, caps %s, batch maxCount %d" % (name, E, F, caps, m0))
        legs = {}
        for k, (_, written, M, n_rows, moved) in made.items():
            print("  %-42s M %3d  rows %9d  written %7.1f MB  moved %7.1f MB  device %s  host %s"
                  % (k, M, n_rows, written / 1e6, moved / 1e6, tc.fmt(dev[k]), tc.fmt(host[k])))
            legs[k] = {"max_count": M, "embedding_rows": n_rows, "bytes_written": written, "bytes_moved": moved, "device_us": dev[k],
                       "host_us": host[k]}
        results.append({"config": name, "envs": E, "embed_width": F, "caps": caps, "batch_max_count": m0, "calls": args.calls, "legs": legs})
        env.close()
    print(json.dumps(results))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
