"""Time the curiosity module (dynenv_amd/icm.py) over a stored rollout: the fused route (dynenv_icm_losses: the row kernel and the masked
means, two launches) against the module's torch route in float32 and against the torch route under torch.autocast in the operands' 16-bit
type, all under no_grad on the same tensors.

For the two flagship configurations (tools/timing_common.CONFIGS) at --envs environments, K in --widths and T = --rollout steps.  The
legs alternate inside every repeat; every call sits between its own pair of HIP events (tools/timing_common.py); medians of --calls
calls with min and max.  Bytes: the algorithmic traffic of a call is the feature tensor once, (T + 1) P K 4 bytes, the actions and
the mask once and the two outputs once; the torch route also writes and reads the one-hot, the two cats, the hidden layer, the
prediction and the logits.  One JSON line per (configuration, K), then a table.

    python tools/bench_icm.py --envs 4096 --calls 15 --out icm.json

--backward times a gradient call instead - the module's forward with gradients enabled plus loss.backward(), the parameters' .grad
cleared before every call - for three routes on the same tensors: GpuICM(fused_backward=True) (dynenv_icm_losses, then
dynenv_icm_backward: the row kernel and the reduction of the workgroups' slices), the torch route under torch.autocast and the torch
route in float32.  --features-grad lets `features` want a gradient too.  The algorithmic traffic of the fused backward is the feature
tensor read once and, with --features-grad, its gradient written once: (T + 1) P K 4 bytes each.

    python tools/bench_icm.py --backward --envs 4096 --calls 15 --out icm_backward.json"""
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
    ap.add_argument("--backward", action="store_true", help="time forward + loss.backward() of the three differentiable routes")
    ap.add_argument("--features-grad", action="store_true", help="with --backward: features.requires_grad_(True)")
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
            if args.backward:
                res, line = backward_legs(args, tc, torch, GpuICM, icm.state_dict(), name, nvec, dt, features, actions, finished)
                results.append(res)
                table.append(line)
                del icm, features, actions, finished
                torch.cuda.empty_cache()
                continue

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


def backward_legs(args, tc, torch, GpuICM, state, name, nvec, dt, features, actions, finished):
    """one (configuration, K) of --backward -> (the JSON record, the table's line)"""
    T, P, K = features.shape[0] - 1, features.shape[1], features.shape[2]
    mods = {"fused_backward": GpuICM(K, nvec, T, w_dtype=dt, device="cuda", fused_backward=True), "torch_autocast": GpuICM(K, nvec, T, w_dtype=dt, device="cuda"),
            "torch_f32": GpuICM(K, nvec, T, w_dtype=dt, device="cuda")}
    for m in mods.values():
        m.load_state_dict(state, strict=True)
    features = features.clone().requires_grad_(args.features_grad)

    def leg(k):
        m = mods[k]

        def call():
            m.zero_grad(set_to_none=True)
            features.grad = None
            if k == "torch_autocast":
                with torch.autocast("cuda", dtype=dt):
                    out = m(features, actions, finished)
            else:
                out = m(features, actions, finished)
            out.loss.backward()
            return out
        return call
    legs = {k: leg(k) for k in mods}
    routes = {}
    for k, fn in legs.items():
        fn()
        routes[k] = mods[k].last_route
    assert routes == {"fused_backward": "fused (backward)", "torch_autocast": "torch", "torch_f32": "torch"}, routes
    g, w = mods["fused_backward"].pred_net.fwd_net.fc2.weight.grad, mods["torch_f32"].pred_net.fwd_net.fc2.weight.grad
    assert float((g - w).abs().max()) < 0.05 * float(w.abs().max()), "the routes' gradients differ by the operands' rounding only"
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            times[k] += tc.event_times(torch, fn, args.calls, warmup=2)
    res = {"config": name, "mode": "backward", "features_grad": bool(args.features_grad), "rows": P, "K": K, "T": T, "dtype": args.dtype,
           "calls": args.calls * args.repeats, "routes": routes,
           "legs": {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}}
    L = res["legs"]
    res["bytes"] = {"features": 4 * (T + 1) * P * K, "algorithmic": 4 * (T + 1) * P * K * (2 if args.features_grad else 1)}
    res["fused_wins"] = L["fused_backward"]["max_us"] < min(L["torch_f32"]["min_us"], L["torch_autocast"]["min_us"])   # (by more than the spread)
    print(json.dumps(res))
    sys.stdout.flush()
    fmt = lambda k: "%8.1f (%.1f .. %.1f)" % (L[k]["median_us"], L[k]["min_us"], L[k]["max_us"])  # noqa: E731
    return res, "%-24s P %6d K %3d T %d backward%s | fused %s torch autocast %s torch f32 %s us | features %.1f MB" % (
        name, P, K, T, " + d_features" if args.features_grad else "", fmt("fused_backward"), fmt("torch_autocast"), fmt("torch_f32"), res["bytes"]["features"] * 1e-6)


if __name__ == "__main__":
    main()
