"""Time the curiosity module (dynenv_amd/icm.py) over a stored rollout: the fused route (dynenv_icm_losses: the row kernel and the masked
means, two launches) against the module's torch route in float32 and against the torch route under torch.autocast in the operands' 16-bit
type, all under no_grad on the same tensors.

For the two flagship configurations (tools/timing_common.CONFIGS) at --envs environments, K in --widths and T = --rollout steps.  The
legs alternate inside every repeat; every call sits between its own pair of HIP events (tools/timing_common.py); medians of --calls
calls with min and max.  Bytes: the algorithmic traffic of a call is the feature tensor once, (T + 1) P K 4 bytes, the actions and
the mask once and the two outputs once; the torch route also writes and reads the one-hot, the two cats, the hidden layer, the
prediction and the logits.  One JSON line per (configuration, K), then a table.

    python tools/bench_icm.py --envs 4096 --calls 15 --out icm.json"""
import json
import os
import statistics
import sys

import timing_common as tc


def main(argv=None):
    ap = tc.base_parser(__doc__, calls_help="timed calls per leg and repeat")
    ap.add_argument("--widths", default="128", help="feature widths K")
    ap.add_argument("--rollout", type=int, default=6, help="T, the steps of a rollout")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f16"))
    args = tc.parse_positive(ap, argv, also=("rollout",))
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuICM
    os.environ.pop("DYNENV_ICM_FUSED", None)
    E, T = args.envs, args.rollout
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    results, table = [], []
    for name, type_name, players, nvec in tc.CONFIGS:
        env = BatchedDynEnv(getattr(DynEnvType, type_name), E, players, seed=3)
        A = env.n_agents
        env.close()
        for K in (int(k) for k in args.widths.split(",")):
            P, G, N = E * A, len(nvec), sum(nvec)
            rng = np.random.default_rng(K + A)
            torch.manual_seed(K)
            icm = GpuICM(K, nvec, T, w_dtype=dt, device="cuda").requires_grad_(False)
            features = torch.randn((T + 1, P, K), device="cuda")
            actions = torch.tensor(np.stack([rng.integers(0, n, (T, P)) for n in nvec], 1).astype(np.float32), device="cuda")
            finished = torch.tensor(rng.random((T, P)) < 0.3, device="cuda")

            def fused():
                return icm(features, actions, finished)

            def torch_f32():
                return icm._forward_torch(features, actions, finished, False)

            def torch_autocast():
                with torch.autocast("cuda", dtype=dt):
                    return icm._forward_torch(features, actions, finished, False)
            def fused_rows():   # (the row kernel without the masked means)
                return icm.rows(features, actions)
            legs = {"fused": fused, "fused_rows": fused_rows, "torch_f32": torch_f32, "torch_autocast": torch_autocast}
            times = {k: [] for k in legs}
            with torch.no_grad():
                got = fused()
                assert icm.last_route == "fused", icm.last_route
                want = torch_f32()
                assert abs(float(got.loss) - float(want.loss)) < 0.02 * abs(float(want.loss)), (float(got.loss), float(want.loss))
                for _ in range(args.repeats):
                    for k, fn in legs.items():
                        times[k] += tc.event_times(torch, fn, args.calls, warmup=2)
            res = {"config": name, "envs": E, "players": A, "rows": P, "K": K, "T": T, "dtype": args.dtype, "calls": args.calls * args.repeats,
                   "legs": {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}}
            moved = 4 * (T + 1) * P * K + 4 * T * G * P + T * P + 4 * T * P * (1 + G)   # features, the actions read, the mask, the two outputs
            res["bytes"] = {"algorithmic": moved, "features": 4 * (T + 1) * P * K}
            res["tb_per_s"] = {"fused": moved / res["legs"]["fused"]["median_us"] * 1e-6}
            res["fused_wins"] = res["legs"]["fused"]["median_us"] <= min(res["legs"]["torch_f32"]["median_us"], res["legs"]["torch_autocast"]["median_us"])
            results.append(res)
            print(json.dumps(res))
            sys.stdout.flush()
            L = res["legs"]
            line = lambda k: "%8.1f (%.1f .. %.1f)" % (L[k]["median_us"], L[k]["min_us"], L[k]["max_us"])  # noqa: E731
            table.append("%-24s P %6d K %3d T %d N %2d | fused %s rows alone %s torch f32 %s autocast %s us | %.1f MB, %.2f TB/s" % (
                name, P, K, T, N, line("fused"), line("fused_rows"), line("torch_f32"), line("torch_autocast"), moved * 1e-6, res["tb_per_s"]["fused"]))
            del icm, features, actions, finished
            torch.cuda.empty_cache()
    print("\n".join(table))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
