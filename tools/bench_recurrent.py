"""Time the recurrent head (GpuRecurrentHead): its fused route (dynenv_recurrent_head, one launch) against its torch route under
autocast and against its torch route in float32, on random features.

For F in --feats and X in --exts at --envs environments of --players players: every leg runs from the same state, each call between its
own pair of HIP events (tools/timing_common.py), medians of --calls calls; the state runs on from call to call.  The fused leg
includes what the module does around the launch (the 16-bit copies of the weights, made with torch ops at every call).  One JSON line
per (F, X), then a table.

    python tools/bench_recurrent.py --envs 4096 --players 10 --calls 7 --out recurrent.json"""
import json
import os
import statistics
import sys

import timing_common as tc


def main(argv=None):
    ap = tc.base_parser(__doc__, calls_help="timed calls per leg")
    ap.add_argument("--players", type=int, default=10)
    ap.add_argument("--feats", default="64,128", help="feature widths F (64 or 128 for the fused route)")
    ap.add_argument("--exts", default="0,6", help="extended feature counts X (0: no TransformNet)")
    ap.add_argument("--dtype", choices=("bf16", "f16"), default="bf16", help="the 16-bit type of the operands and of autocast")
    args = tc.parse_positive(ap, argv, also=("players",))
    import torch
    from dynenv_amd import GpuRecurrentHead
    os.environ["DYNENV_RHEAD_FUSED"] = "1"   # the kernel wherever it can run: a shape the module routes to torch by measurement is measured too
    E, A = args.envs, args.players
    P = E * A
    dt16 = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    results, table = [], []
    for F in (int(f) for f in args.feats.split(",")):
        for X in (int(x) for x in args.exts.split(",")):
            torch.manual_seed(F + X)
            head = GpuRecurrentHead(F, A, E, X, operand_dtype=dt16, device="cuda").requires_grad_(False)
            feat = torch.randn((P, F), device="cuda")
            pos = torch.randn((P, X), device="cuda") if X else None
            mask = (torch.arange(E, device="cuda") % 7 == 0)
            with torch.no_grad():
                for _ in range(3):   # a live state
                    head(feat, pos)
                assert head.last_route == "fused", head.last_route
                state = head.get_states()

                def autocast():
                    with torch.autocast("cuda", dtype=dt16):
                        return head._forward_torch(feat, pos, mask)
                legs = {"fused": lambda: head(feat, pos, mask), "torch_autocast": autocast, "torch_float32": lambda: head._forward_torch(feat, pos, mask)}
                outs = {}
                for k, fn in legs.items():
                    head.set_states(state)
                    outs[k] = fn().float()
                err = {k: float((outs[k] - outs["torch_float32"]).abs().max()) for k in ("fused", "torch_autocast")}
                times = {}
                for k, fn in legs.items():
                    head.set_states(state)   # (float32 again: under autocast on the device the cell returns a 16-bit state)
                    times[k] = tc.event_times(torch, fn, args.calls, warmup=2)
            res = {"envs": E, "players": A, "rows": P, "feat": F, "ext": X, "dtype": args.dtype, "calls": args.calls,
                   "legs": {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()},
                   "max_abs_difference_to_float32": err}
            fused = res["legs"]["fused"]["median_us"]
            res["speedup"] = {k: res["legs"][k]["median_us"] / fused for k in ("torch_autocast", "torch_float32")}
            results.append(res)
            print(json.dumps(res))
            sys.stdout.flush()
            table.append("P %6d  F %3d  X %2d  fused %8.1f us  autocast %8.1f us (%5.1fx)  float32 %8.1f us (%5.1fx)" % (
                P, F, X, fused, res["legs"]["torch_autocast"]["median_us"], res["speedup"]["torch_autocast"],
                res["legs"]["torch_float32"]["median_us"], res["speedup"]["torch_float32"]))
            del head, feat, pos
            torch.cuda.empty_cache()
    print("\n".join(table))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
