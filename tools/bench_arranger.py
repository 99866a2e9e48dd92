#!/usr/bin/env python3
"""Throughput of the GPU arranger on real observations at BASELINE sizes: one JSON line per config with
the HBM roofline of the gather kernel and the numpy oracle (a restatement of the reference's InOutArranger) timed on a
bounded sample.  Usage (GPU box):  python tools/bench_arranger.py [--envs 4096] [--feat 128] [--backward]

--backward adds, from the same run and on the same plan: the backward of rearrange_outputs (GpuInOutArranger._unpad: the fused HIP
kernel), the torch composition a user would write without it (per type G.reshape(-1, F).index_select(0, slot_i)) and the forward,
each as the median over --reps of HIP-event timings of --inner back-to-back calls, the three taking turns inside every repetition;
algorithmic bytes of the backward are 2 * n_obj * F * 4 (every gradient row read once and written once) plus counts and bases.

--padded-dtype bf16|f16 adds, from the same run and on the same plan, the padded tensor in that type (GpuInOutArranger(padded_dtype=...))
beside the float32 one: the float32 leg, the converting leg (float32 embeddings) and the same-type leg (embeddings already in that type;
--emb-dtype keeps one of the two), forward only or, with --backward, forward and backward, the legs taking turns inside every
repetition; per leg the device time (median, min .. max over --reps), the bytes moved and its time relative to the float32 leg.

--fused-embed adds, from the same run and on the same observations, the whole input layer with its embedding blocks (GpuEmbedInputLayer):
the fused route (dynenv_arrange_embed_pad: observation rows in, padded tensor out) against the unfused route of the same module
(rearrange_inputs, the blocks as torch modules, rearrange_outputs), under no_grad, the two taking turns inside every repetition, for
F = 128 and 64, a float32 and a bf16 padded tensor, the default and the fixed-shape mode (rows = capacities); per leg the device time
(median, min .. max) of a whole forward, and for the fused leg the bytes it moves (object rows read, every padded element written,
counts and mask) and TB/s, its FLOP rate, and the unfused leg's time over its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def backward_leg(torch, arr, outs, countArr, padded, args, plan_bytes):
    """medians (ms) of the fused backward, the torch composition and the forward on one plan, and what they move"""
    import statistics
    F = args.feat
    plan = arr._plan_of(countArr)
    slots = plan[3]
    rows = [int(o.shape[0]) for o in outs]
    wanted = [True] * len(outs)
    G = torch.randn(tuple(padded.shape), device=padded.device)
    legs = {
        "backward": lambda: arr._unpad(G, rows, F, wanted, *plan),
        "torch_index_select": lambda: [G.reshape(-1, F).index_select(0, s) for s, n in zip(slots, rows) if n],
        "forward": lambda: arr.rearrange_outputs(outs, countArr),
    }
    got = legs["backward"]()
    ref = legs["torch_index_select"]()
    assert arr.last_backward == "fused", "the fused kernel is what is measured (F % 4 == 0)"
    assert all(torch.equal(a, b) for a, b in zip([g for g, n in zip(got, rows) if n], ref)), "backward != torch composition"
    for fn in legs.values():   # warm-up of every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(args.inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.inner)
    n_obj = sum(rows)
    b_bwd = 2 * n_obj * F * 4 + plan_bytes                      # gradient rows read + written, counts and bases read
    b_sel = 2 * n_obj * F * 4 + n_obj * 4                       # the same rows, one slot per row
    b_fwd = n_obj * F * 4 + padded.numel() * 4 + plan_bytes     # embeddings read, every padded element written
    out = {"reps": args.reps, "inner": args.inner, "occupancy": n_obj / (padded.numel() // F)}
    for k, b in (("backward", b_bwd), ("torch_index_select", b_sel), ("forward", b_fwd)):
        t = sorted(times[k])
        med = statistics.median(t)
        out[k] = {"median_ms": med, "min_ms": t[0], "p90_ms": t[int(0.9 * (len(t) - 1))], "alg_bytes": b,
                  "achieved": b / (med * 1e-3) / 1e9, "unit": "GB/s"}
    out["speedup_over_torch"] = out["torch_index_select"]["median_ms"] / out["backward"]["median_ms"]
    return out


def dtype_legs(torch, GpuInOutArranger, shape, countArr, n_obj, args, plan_bytes):
    """forward (and backward) of rearrange_outputs with a float32 and with a 16-bit padded tensor on one plan: {leg: {forward, backward}}"""
    import statistics
    F = args.feat
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    size = {"f32": 4, "bf16": 2, "f16": 2}
    pk = args.padded_dtype
    emb_kinds = [args.emb_dtype] if args.emb_dtype else ["f32", pk]
    if any(k not in ("f32", pk) for k in emb_kinds):
        raise SystemExit("--emb-dtype is f32 or the --padded-dtype")
    pairs = [("f32", "f32")] + [(k, pk) for k in emb_kinds]
    arrs = {"f32": GpuInOutArranger(*shape), pk: GpuInOutArranger(*shape, padded_dtype=tdt[pk])}
    plan = arrs["f32"]._plan_of(countArr)
    counts, base, max_count = plan[:3]
    base32 = [torch.randn((n, F), device="cuda") for n in n_obj]
    wanted = [True] * len(n_obj)
    legs, nbytes = {}, {}
    with torch.no_grad():
        for ek, pd in pairs:
            arr = arrs[pd]
            outs = [o.to(tdt[ek]) for o in base32]
            G = torch.randn((arr.nTime, max_count, arr.nPlayers, F), device="cuda").to(tdt[pd])
            name = "%s -> %s" % (ek, pd)
            legs[name, "forward"] = (lambda arr=arr, outs=outs: arr.rearrange_outputs(outs, countArr))
            nbytes[name, "forward"] = sum(n_obj) * F * size[ek] + G.numel() * size[pd] + plan_bytes
            if args.backward:
                if pd == "f32":
                    legs[name, "backward"] = (lambda arr=arr, G=G: arr._unpad(G, n_obj, F, wanted, *plan))
                else:
                    legs[name, "backward"] = (lambda arr=arr, G=G, ek=ek: arr._unpad_as(G, n_obj, tdt[ek], F, wanted, counts, base, max_count))
                nbytes[name, "backward"] = sum(n_obj) * F * (size[ek] + size[pd]) + plan_bytes
        for fn in legs.values():   # warm-up of every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _i in range(args.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.inner)
    out = {}
    for (name, way), t in times.items():
        med = statistics.median(t)
        ref = statistics.median(times["f32 -> f32", way])
        out.setdefault(name, {})[way] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes_moved": nbytes[name, way],
                                         "achieved": nbytes[name, way] / (med * 1e-3) / 1e12, "unit": "TB/s", "vs_f32": med / ref}
    return out


def fused_embed_legs(torch, GpuEmbedInputLayer, shape, obs, count_env, args):
    """{F: {padded dtype: {mode: {fused, blocks, speedup}}}} of GpuEmbedInputLayer's two routes on one batch"""
    import statistics
    types, E, A, T, D = shape
    out = {}
    for F in (128, 64):
        for pk, pdt in (("f32", None), ("bf16", torch.bfloat16)):
            for mode, fixed in (("default", None), ("fixed", True)):
                torch.manual_seed(F)
                layer = GpuEmbedInputLayer(types, F, E, A, T, D, fixed=fixed, padded_dtype=pdt).requires_grad_(False)
                legs = {"fused": lambda: layer(obs, count_env), "blocks": lambda: layer._forward_blocks(obs, count_env)}
                with torch.no_grad():
                    padded, _ = legs["fused"]()
                    assert layer.last_route == "fused", layer.last_route
                    ref, _ = legs["blocks"]()
                    err = float((padded.float() - ref.float()).abs().max())
                    for fn in legs.values():   # warm-up of every shape
                        for _ in range(2):
                            fn()
                    torch.cuda.synchronize()
                    times = {k: [] for k in legs}
                    for _ in range(args.reps):
                        for k, fn in legs.items():
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _i in range(args.inner):
                                fn()
                            e1.record()
                            e1.synchronize()
                            times[k].append(e0.elapsed_time(e1) / args.inner)
                n_obj = [int(v) for v in layer.last_counts.clamp(min=0).sum((1, 2)).tolist()]
                TP = T * E * A
                nbytes = sum(n * t.feat * 4 for n, t in zip(n_obj, types)) + padded.numel() * padded.element_size() + TP * len(types) * 8 + TP * padded.shape[1]
                flop = sum(n * 2 * (t.feat * F // 2 + F * F // 2) for n, t in zip(n_obj, types))
                res = {}
                for k, t in times.items():
                    res[k] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
                fm = res["fused"]["median_ms"]
                res["fused"].update(bytes_moved=nbytes, achieved=nbytes / (fm * 1e-3) / 1e12, unit="TB/s", tflops=flop / (fm * 1e-3) / 1e12)
                res["speedup"] = res["blocks"]["median_ms"] / fm
                res["objects"], res["max_count"], res["max_abs_difference"] = n_obj, int(padded.shape[1]), err
                out.setdefault("F%d" % F, {}).setdefault(pk, {})[mode] = res
                del layer, padded, ref
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--feat", type=int, default=128, help="embedding width F of rearrange_outputs")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--backward", action="store_true", help="also time the backward of rearrange_outputs against the torch composition")
    ap.add_argument("--inner", type=int, default=10, help="--backward: calls between two events (keeps the queue full)")
    ap.add_argument("--padded-dtype", choices=("f32", "bf16", "f16"), default="f32",
                    help="bf16 / f16: also time rearrange_outputs with a padded tensor of that type, beside the float32 leg, in the same run")
    ap.add_argument("--emb-dtype", choices=("f32", "bf16", "f16"), default=None,
                    help="with --padded-dtype: the embeddings' type of the 16-bit leg, f32 (converting) or the padded type (bit copy); default both")
    ap.add_argument("--fused-embed", action="store_true",
                    help="also time GpuEmbedInputLayer's fused route (embed and pad in one kernel) against its unfused route, in the same run")
    args = ap.parse_args()
    import numpy as np
    import torch
    import arranger as oa
    from compat_ref import compat_obs_of
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuEmbedInputLayer, GpuInOutArranger, NoiseType, ObservationType, groups_for
    E = args.envs
    for cfg in ("driving_full", "robocup", "driving_partial"):
        if cfg == "robocup":
            env = BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=42); hi = [5, 3, 3, 7]
        elif cfg == "driving_partial":
            env = BatchedDynEnv(DynEnvType.DRIVE, E, 10, observationType=ObservationType.PARTIAL,
                                noiseType=NoiseType.REALISTIC, noiseMagnitude=3, seed=42); hi = [3, 3]
        else:
            env = BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=42); hi = [3, 3]
        env.reset_flat()
        g = torch.Generator(device="cuda").manual_seed(1)
        hit = torch.tensor(hi, device="cuda")
        for _ in range(20):
            a = (torch.rand((E, env.n_agents, len(hi)), generator=g, device="cuda") * hit).to(torch.int32)
            obs, _, _ = env.step_flat(a, auto_reset=False)
        obs = obs.contiguous()
        count_env = env.counts() if env.env_type == DynEnvType.DRIVE else None
        types = groups_for(env)["movable"]
        arr = GpuInOutArranger(types, E, env.n_agents, env.n_time_steps, env.obs_dim)
        inputs, countArr = arr.rearrange_inputs(obs, count_env)
        outs = [torch.randn((i.shape[0], args.feat), device="cuda") for i in inputs]
        arr.rearrange_outputs(outs, countArr)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        for _ in range(args.reps):
            inputs, countArr = arr.rearrange_inputs(obs, count_env)
        ev[1].record()
        for _ in range(args.reps):
            padded, masks = arr.rearrange_outputs(outs, countArr)
        ev[2].record()
        torch.cuda.synchronize()
        ms_in = ev[0].elapsed_time(ev[1]) / args.reps
        ms_out = ev[1].elapsed_time(ev[2]) / args.reps
        n_obj = [int(i.shape[0]) for i in inputs]
        TP = env.n_time_steps * E * env.n_agents
        # algorithmic bytes: rows read + rows written + slot per object + mask + counts/base per (type, time, player)
        b_in = sum(n * t.feat * 4 * 2 + n * 4 for n, t in zip(n_obj, types)) + TP * countArr[1] + TP * len(types) * 8 + TP * 4
        b_out = sum(n_obj) * args.feat * 4 + padded.numel() * 4  # embeddings read once + every padded element written once
        # CPU: the numpy restatement of the reference arranger on a bounded sample of the same observations
        Es = min(E, 128)
        compat = compat_obs_of(env, obs[:Es], count_env[:Es] if count_env is not None else None)
        x = [[[list(compat[e, t, p, 0]) for p in range(env.n_agents)] for t in range(env.n_time_steps)] for e in range(Es)]
        t0 = time.perf_counter()
        o_in, o_cnt = oa.rearrange_inputs(x, len(types), Es * env.n_agents, env.n_time_steps)
        o_outs = [np.zeros((len(i), args.feat), np.float32) if len(i) else None for i in o_in]
        oa.rearrange_outputs(o_outs, o_cnt)
        cpu_s = time.perf_counter() - t0
        agent_rows = E * env.n_agents * env.n_time_steps
        bwd = backward_leg(torch, arr, outs, countArr, padded, args, TP * len(types) * 8) if args.backward else None
        dt = None
        if args.padded_dtype != "f32":
            dt = dtype_legs(torch, GpuInOutArranger, (types, E, env.n_agents, env.n_time_steps, env.obs_dim), countArr, n_obj, args,
                            TP * len(types) * 8)
        fe = None
        if args.fused_embed:
            fe = fused_embed_legs(torch, GpuEmbedInputLayer, (types, E, env.n_agents, env.n_time_steps, env.obs_dim), obs, count_env, args)
        print(json.dumps({
            "metric": "arranged agent-observations/s", "config": cfg, "envs": E, "players": E * env.n_agents,
            "time_steps": env.n_time_steps, "objects": n_obj, "max_count": countArr[1], "embed_width": args.feat,
            "rearrange_inputs_ms": ms_in, "rearrange_outputs_ms": ms_out,
            "value": agent_rows / ((ms_in + ms_out) * 1e-3), "unit": "agent-observations/s",
            "roofline": {"bound": "hbm", "unit": "GB/s", "peak": 8000.0,
                         "rearrange_inputs": {"alg_bytes": b_in, "achieved": b_in / (ms_in * 1e-3) / 1e9},
                         "rearrange_outputs": {"alg_bytes": b_out, "achieved": b_out / (ms_out * 1e-3) / 1e9}},
            "cpu_baseline": {"kind": "port", "cores": 1, "value": Es * env.n_agents * env.n_time_steps / cpu_s,
                             "unit": "agent-observations/s",
                             "sample": "oracle/arranger.py (numpy restatement of InOutArranger) on the first %d envs, %.2f s" % (Es, cpu_s)},
            **({"backward": bwd} if bwd is not None else {}),
            **({"padded_dtype": {"dtype": args.padded_dtype, "reps": args.reps, "inner": args.inner, "legs": dt}} if dt is not None else {}),
            **({"fused_embed": {"reps": args.reps, "inner": args.inner, "legs": fe}} if fe is not None else {}),
        }))
        env.close()


if __name__ == "__main__":
    main()
