"""Time the policy head (GpuPolicyHead.act): its fused route (dynenv_policy_head, one launch) against its torch route under autocast
and against its torch route in float32, on random features.

For the two flagship configurations (tools/timing_common.CONFIGS: Driving, 10 players, [3, 3]; RoboCup, 5 players, [5, 3, 3, 7]) at
--envs environments and K in --widths: every leg makes the same draws on the same features, each call between its own pair of HIP
events (tools/timing_common.py), medians of --calls calls with min and max.  The fused leg includes what the module does around the
launch (the 16-bit copies of the weights, made with torch ops at every call, and the counter's increment).  One JSON line per
(configuration, K), then a table.

    python tools/bench_policy.py --envs 4096 --calls 15 --out policy.json"""
import json
import os
import statistics
import sys

import timing_common as tc


def main(argv=None):
    ap = tc.base_parser(__doc__, calls_help="timed calls per leg")
    ap.add_argument("--widths", default="128,256", help="feature widths K: 64, 128 (one feature) or 256 (two features of 128) for the fused route")
    ap.add_argument("--dtype", choices=("bf16", "f16"), default="bf16", help="the 16-bit type of the operands and of autocast")
    args = tc.parse_positive(ap, argv)
    import torch
    from dynenv_amd import GpuPolicyHead, spaces
    os.environ.pop("DYNENV_POLICY_FUSED", None)
    E = args.envs
    dt16 = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    results, table = [], []
    for name, _, A, nvec in tc.CONFIGS:
        P = E * A
        for K in (int(k) for k in args.widths.split(",")):
            torch.manual_seed(K + A)
            head = GpuPolicyHead(K, spaces.Tuple((spaces.MultiDiscrete(list(nvec)),)), operand_dtype=dt16, seed=7, device="cuda").requires_grad_(False)
            feats = (torch.randn((P, K), device="cuda"),) if K < 256 else (torch.randn((P, K // 2), device="cuda"), torch.randn((P, K // 2), device="cuda"))
            static = torch.zeros((E, A, len(nvec)), dtype=torch.int32, device="cuda")
            with torch.no_grad():
                def fused():
                    return head.act(*feats, out_actions=static)

                def autocast():
                    with torch.autocast("cuda", dtype=dt16):
                        return head._act_torch(feats[0], feats[1] if len(feats) > 1 else None, static, 0)

                def float32():
                    return head._act_torch(feats[0], feats[1] if len(feats) > 1 else None, static, 0)
                legs = {"fused": fused, "torch_autocast": autocast, "torch_float32": float32}
                outs = {}
                for k, fn in legs.items():
                    head.reseed(7, 0)
                    o = fn()
                    outs[k] = (torch.cat(o.probs, 1).float(), o.value.float(), o.actions.clone())
                head.reseed(7, 0)
                fused()
                assert head.last_route == "fused", head.last_route
                err = {k: {"probs": float((outs[k][0] - outs["torch_float32"][0]).abs().max()),
                           "value": float((outs[k][1] - outs["torch_float32"][1]).abs().max()),
                           "actions_that_differ": int((outs[k][2] != outs["torch_float32"][2]).any(1).sum())} for k in ("fused", "torch_autocast")}
                times = {k: tc.event_times(torch, fn, args.calls, warmup=3) for k, fn in legs.items()}
            res = {"config": name, "envs": E, "players": A, "rows": P, "K": K, "nvec": list(nvec), "dtype": args.dtype, "calls": args.calls,
                   "legs": {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()},
                   "difference_to_float32": err}
            fused_us = res["legs"]["fused"]["median_us"]
            res["speedup"] = {k: res["legs"][k]["median_us"] / fused_us for k in ("torch_autocast", "torch_float32")}
            results.append(res)
            print(json.dumps(res))
            sys.stdout.flush()
            line = lambda k: "%8.1f (%.1f .. %.1f)" % (res["legs"][k]["median_us"], res["legs"][k]["min_us"], res["legs"][k]["max_us"])  # noqa: E731
            table.append("%-24s P %6d  K %3d  fused %s us  autocast %s us (%5.1fx)  float32 %s us (%5.1fx)" % (
                name, P, K, line("fused"), line("torch_autocast"), res["speedup"]["torch_autocast"], line("torch_float32"),
                res["speedup"]["torch_float32"]))
            del head, feats, static
            torch.cuda.empty_cache()
    print("\n".join(table))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
