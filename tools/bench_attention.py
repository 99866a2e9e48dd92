"""Time the attention over the padded tensor (GpuTemporalAttention): its fused route (dynenv_attend_pool, one launch) against its torch
route under autocast and against its torch route in float32, on the real padded tensors of a mid-episode batch.

For both object groups of the four configurations, in the arranger's default and fixed mode: GpuEmbedInputLayer writes the padded tensor
(bfloat16 for the fused and the autocast leg, float32 for the float32 leg) once, untimed; every leg is then timed on it with HIP events,
each call between its own pair of events (tools/timing_common.py), medians of --calls calls.  One JSON line per (configuration, group,
mode), then a table.

    python tools/bench_attention.py --envs 4096 --feat 128 --out attention.json"""
import json
import os
import statistics
import sys

import timing_common as tc

CONFIGS = ("driving_full", "driving_partial", "robocup_full", "robocup_partial")


def make_env(cfg, E):
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    part = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=3) if cfg.endswith("partial") else {}
    if cfg.startswith("driving"):
        return BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=42, **part), (3, 3)
    return BatchedDynEnv(DynEnvType.ROBO_CUP, E, 5, seed=42, **part), (5, 3, 3, 7)


def main(argv=None):
    ap = tc.base_parser(__doc__, calls_help="timed calls per leg")
    ap.add_argument("--feat", type=int, default=128, help="feature width F (64 or 128 for the fused route)")
    ap.add_argument("--dtype", choices=("bf16", "f16"), default="bf16", help="the 16-bit type of the padded tensor and of autocast")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--steps", type=int, default=20, help="steps into the episode before the observation is taken")
    args = tc.parse_positive(ap, argv, also=("feat",))
    import numpy as np
    import torch
    from dynenv_amd import GpuEmbedInputLayer, GpuTemporalAttention, groups_for
    os.environ["DYNENV_ATT_FUSED"] = "1"   # the kernel wherever it can run: the shape the module routes to torch by measurement is measured too
    E, F = args.envs, args.feat
    dt16 = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    results, table = [], []
    for cfg in args.configs.split(","):
        env, hi = make_env(cfg, E)
        acts = tc.action_pool(torch, np, hi, E, env.n_agents, seed=1, n=4)
        tc.mid_episode(env, acts, steps=args.steps)
        obs, ce = env.obs.contiguous(), env.counts()
        T, A, D = env.n_time_steps, env.n_agents, env.obs_dim
        for group, types in groups_for(env).items():
            for mode, fixed in (("default", None), ("fixed", True)):
                torch.manual_seed(F)
                att = GpuTemporalAttention(F, device="cuda").requires_grad_(False)
                with torch.no_grad():
                    for m in (att.objAtt, att.tempAtt):   # (torch starts these at zero)
                        m.in_proj_bias.uniform_(-0.5, 0.5)
                        m.out_proj.bias.uniform_(-0.5, 0.5)
                    torch.manual_seed(F + 1)
                    emb16 = GpuEmbedInputLayer(types, F, E, A, T, D, fixed=fixed, padded_dtype=dt16).requires_grad_(False)
                    emb32 = GpuEmbedInputLayer(types, F, E, A, T, D, fixed=fixed).requires_grad_(False)
                    emb32.load_state_dict(emb16.state_dict(), strict=True)
                    x16, x32 = emb16(obs, ce), emb32(obs, ce)
                    counts = emb16.last_obj_counts
                    M = int(x16[0].shape[1])
                    n = counts.clamp(0, M).max(0).values.float()

                    def autocast():
                        with torch.autocast("cuda", dtype=dt16):
                            return att._forward_torch(x16)
                    legs = {"fused": lambda: att(x16, counts), "torch_autocast": autocast, "torch_float32": lambda: att._forward_torch(x32)}
                    out = legs["fused"]()
                    assert att.last_route == "fused", att.last_route
                    ref = legs["torch_float32"]()
                    err = {"fused": float((out - ref).abs().max()), "torch_autocast": float((legs["torch_autocast"]().float() - ref).abs().max())}
                    del out, ref
                    times = {k: tc.event_times(torch, fn, args.calls, warmup=2) for k, fn in legs.items()}
                res = {"config": cfg, "group": group, "mode": mode, "envs": E, "players": E * A, "time_steps": T, "max_count": M, "feat": F,
                       "dtype": args.dtype, "objects_per_player": {"mean_n": float(n.mean()), "max_n": int(n.max())}, "calls": args.calls,
                       "legs": {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()},
                       "max_abs_difference_to_float32": err}
                fused = res["legs"]["fused"]["median_us"]
                res["speedup"] = {k: res["legs"][k]["median_us"] / fused for k in ("torch_autocast", "torch_float32")}
                results.append(res)
                print(json.dumps(res))
                sys.stdout.flush()
                table.append("%-16s %-8s %-8s M %3d  n %5.1f / %3d  fused %9.1f us  autocast %10.1f us (%5.1fx)  float32 %10.1f us (%5.1fx)" % (
                    cfg, group, mode, M, res["objects_per_player"]["mean_n"], res["objects_per_player"]["max_n"], fused,
                    res["legs"]["torch_autocast"]["median_us"], res["speedup"]["torch_autocast"], res["legs"]["torch_float32"]["median_us"],
                    res["speedup"]["torch_float32"]))
                del att, emb16, emb32, x16, x32
                torch.cuda.empty_cache()
        env.close()
    print("\n".join(table))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
