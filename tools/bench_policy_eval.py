"""Time the training step of the policy head over a stored rollout: GpuPolicyHead.evaluate + GpuRolloutStorage.a2c_loss(evaluation=...) +
loss.backward() on three routes, on the same tensors: GpuPolicyHead(fused_backward=True) (dynenv_policy_eval, then
dynenv_policy_eval_backward: the row kernel and the reduction of the workgroups' slices; the loss stays torch's), the torch route in
float32 and the torch route under torch.autocast in the operands' 16-bit type.

For the two flagship configurations (tools/timing_common.CONFIGS) at --envs environments, K in --widths and T = --rollout steps (the
reference's default, 6): feature tensors of a rollout's shape [T, P, K], P = environments * players, standard normal - the head's
kernels do not look at the values - with random stored actions, rewards, values and dones.  The legs alternate inside every repeat.
Every call has three HIP events around its two halves (tools/timing_common.py's way): forward = evaluate + a2c_loss, backward =
loss.backward(); medians of --calls calls with min and max.  The parameters' .grad is cleared, untimed, before every call.
Bytes: the algorithmic traffic of the fused forward is the feature tensor once, T P K 4 bytes, the actions once and the three outputs
once; of the fused backward the feature tensor and the actions once, the three upstream tensors once and, with --features-grad, the
features' gradient once.  "moved" adds what the implementation moves on top: the workspace slices written and read.  The loss's own
elementwise traffic over [T, P], [T, G, P] and [T, P, N] is the same on every route and is part of both halves.  One JSON line per
(configuration, K), then a table.

    python tools/bench_policy_eval.py --envs 4096 --calls 15 --out policy_eval.json"""
import ctypes as C
import json
import os
import statistics
import sys

import timing_common as tc


def split_times(torch, prepare, forward, calls, warmup=2):
    """device microseconds (forward, backward) of each of `calls` calls: three events around forward() and its result's backward()"""
    for _ in range(warmup):
        prepare()
        forward().backward()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        prepare()
        e[0].record()
        loss = forward()
        e[1].record()
        loss.backward()
        e[2].record()
        e[2].synchronize()
        out.append((e[0].elapsed_time(e[1]) * 1e3, e[1].elapsed_time(e[2]) * 1e3))
    return out


def main(argv=None):
    ap = tc.base_parser(__doc__, calls_help="timed calls per leg and repeat")
    ap.add_argument("--widths", default="128", help="feature widths K")
    ap.add_argument("--rollout", type=int, default=6, help="T, the steps of a rollout")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f16"))
    ap.add_argument("--features-grad", action="store_true", help="features.requires_grad_(True): d_features is written too")
    ap.add_argument("--full-entropy", action="store_true", help="use_full_entropy=True in the loss")
    args = tc.parse_positive(ap, argv, also=("rollout",))
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuPolicyHead, GpuRolloutStorage, _capi, spaces
    os.environ.pop("DYNENV_POLICY_FUSED", None)
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
            space = spaces.Tuple([spaces.MultiDiscrete(list(nvec))])
            mods = {"fused_backward": GpuPolicyHead(K, space, operand_dtype=dt, device="cuda", fused_backward=True),
                    "torch_autocast": GpuPolicyHead(K, space, operand_dtype=dt, device="cuda"), "torch_f32": GpuPolicyHead(K, space, operand_dtype=dt, device="cuda")}
            for m in mods.values():
                m.load_state_dict(mods["torch_f32"].state_dict(), strict=True)
            st = GpuRolloutStorage(T, E, A, G, nvec, K, n_probs=0, use_full_entropy=args.full_entropy, device="cuda")
            st.features.normal_()
            st.rewards.normal_()
            st.values.normal_()
            st.dones.copy_(torch.tensor(rng.random((T, E)) < 0.1, device="cuda").float())
            st.actions.copy_(torch.tensor(np.stack([rng.integers(0, n, (T, P)) for n in nvec], 1).astype(np.float32), device="cuda"))
            final = torch.randn((P, 1), device="cuda")
            features = st.features[:-1].clone().requires_grad_(args.features_grad)

            def leg(k):
                m = mods[k]

                def prepare():
                    m.zero_grad(set_to_none=True)
                    features.grad = None

                def forward():
                    if k == "torch_autocast":
                        with torch.autocast("cuda", dtype=dt):
                            ev = m.evaluate(features, st.actions)
                    else:
                        ev = m.evaluate(features, st.actions)
                    return st.a2c_loss(final, evaluation=ev).loss
                return prepare, forward
            legs = {k: leg(k) for k in mods}
            routes, losses = {}, {}
            for k, (prepare, forward) in legs.items():
                prepare()
                loss = forward()
                loss.backward()
                routes[k], losses[k] = mods[k].last_eval_route, float(loss)
            assert routes == {"fused_backward": "fused (backward)", "torch_autocast": "torch", "torch_f32": "torch"}, routes
            g, w = mods["fused_backward"].critic.blocks.Layer1.weight.grad, mods["torch_f32"].critic.blocks.Layer1.weight.grad
            assert float((g - w).abs().max()) < 0.05 * float(w.abs().max()), "the routes' gradients differ by the operands' rounding only"
            times = {k: [] for k in legs}
            for _ in range(args.repeats):
                for k, (prepare, forward) in legs.items():
                    times[k] += split_times(torch, prepare, forward, args.calls)
            need = C.c_uint64(0)
            _capi.check(_capi.load().dynenv_policy_eval_backward_workspace(T * P, K, C.byref(need)), "dynenv_policy_eval_backward_workspace")

            def stats(v):
                return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
            rows = T * P
            fwd_bytes = 4 * rows * K + 4 * rows * G + 4 * rows * (G + N + 1)
            bwd_bytes = 4 * rows * K * (2 if args.features_grad else 1) + 4 * rows * G + 4 * rows * (G + N + 1)
            res = {"config": name, "envs": E, "players": A, "rows": rows, "K": K, "T": T, "dtype": args.dtype, "features_grad": bool(args.features_grad),
                   "full_entropy": bool(args.full_entropy), "calls": args.calls * args.repeats, "routes": routes, "loss": losses,
                   "legs": {k: {"forward": stats([t[0] for t in v]), "backward": stats([t[1] for t in v]), "total": stats([t[0] + t[1] for t in v])}
                            for k, v in times.items()},
                   "bytes": {"forward_algorithmic": fwd_bytes, "forward_moved": fwd_bytes, "backward_algorithmic": bwd_bytes,
                             "backward_moved": bwd_bytes + 2 * need.value, "workspace": need.value}}
            L = res["legs"]
            res["fused_wins"] = L["fused_backward"]["total"]["max_us"] < min(L["torch_f32"]["total"]["min_us"], L["torch_autocast"]["total"]["min_us"])
            results.append(res)
            print(json.dumps(res))
            sys.stdout.flush()
            fmt = lambda k, h: "%8.1f (%.1f .. %.1f)" % (L[k][h]["median_us"], L[k][h]["min_us"], L[k][h]["max_us"])  # noqa: E731
            for h in ("forward", "backward", "total"):
                table.append("%-24s rows %7d K %3d T %d %-8s | fused %s torch autocast %s torch f32 %s us" % (
                    name, rows, K, T, h, fmt("fused_backward", h), fmt("torch_autocast", h), fmt("torch_f32", h)))
            table.append("%-24s bytes: forward %.1f MB algorithmic = moved; backward %.1f MB algorithmic, %.1f MB moved (workspace %.1f MB written and read)" % (
                name, fwd_bytes * 1e-6, bwd_bytes * 1e-6, res["bytes"]["backward_moved"] * 1e-6, need.value * 1e-6))
            del mods, st, features, final
            torch.cuda.empty_cache()
    print("\n".join(table))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
