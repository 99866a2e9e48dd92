"""Time the rollout storage (dynenv_amd/rollout.py): the fused insert (dynenv_rollout_insert, one launch) against its torch route and
against the copy_ of the same feature tensor - the bandwidth the insert is held against: the feature rows are nearly all of its bytes -,
the returns by the kernel (dynenv_rollout_returns) against the reference's loop of 2 T + 2 launches, and a collected rollout
(GpuRollout.collect: step, extractor, policy and insert, T times, and the bootstrap) recorded as a graph against the same run eagerly.

For the two flagship configurations (tools/timing_common.CONFIGS) at --envs environments, K in --widths (256: two features of 128) and
T = --rollout steps.  The legs alternate inside every repeat; every call sits between its own pair of HIP events
(tools/timing_common.py); medians of --calls calls with min and max.  One JSON line per (configuration, K), then a table.

    python tools/bench_rollout.py --envs 4096 --calls 15 --out rollout.json"""
import json
import os
import statistics
import sys

import timing_common as tc


def _legs_times(torch, legs, calls, repeats):
    """name -> microseconds of calls * repeats calls; the legs take turns inside every repeat"""
    out = {k: [] for k in legs}
    for _ in range(repeats):
        for k, (fn, prepare) in legs.items():
            out[k] += tc.event_times(torch, fn, calls, warmup=2, prepare=prepare)
    return out


def main(argv=None):
    ap = tc.base_parser(__doc__, calls_help="timed calls per leg and repeat")
    ap.add_argument("--widths", default="128,256", help="feature widths K; 256 is two features of 128")
    ap.add_argument("--rollout", type=int, default=6, help="T, the steps of a rollout")
    ap.add_argument("--collect-calls", type=int, default=3, help="timed rollouts per collector leg and repeat (0: skip the collector)")
    args = tc.parse_positive(ap, argv, also=("rollout",))
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuFeatureExtractor, GpuPolicyHead, GpuRollout, GpuRolloutStorage, groups_for, rollout
    os.environ.pop("DYNENV_ROLLOUT_FUSED", None)
    E, T = args.envs, args.rollout
    results, table = [], []
    for name, type_name, players, nvec in tc.CONFIGS:
        for K in (int(k) for k in args.widths.split(",")):
            two = K >= 256
            F = K // 2 if two else K
            env = BatchedDynEnv(getattr(DynEnvType, type_name), E, players, seed=3)
            env.reset_flat()
            A = env.n_agents
            P, G, N = E * A, len(nvec), sum(nvec)
            st = GpuRolloutStorage(T, E, A, G, nvec, K, n_probs=N)
            rng = np.random.default_rng(K + A)
            feats = [torch.randn((P, F), device="cuda") for _ in range(2 if two else 1)] + ([] if two else [None])
            actions = torch.tensor(rng.integers(0, 3, (P, G)).astype(np.int32), device="cuda")
            logp, value = -torch.rand((P, G), device="cuda"), torch.randn((P,), device="cuda")
            probs = torch.rand((P, N), device="cuda")
            rewards, dones = torch.randn((E, A), dtype=torch.float64, device="cuda"), torch.zeros((E,), dtype=torch.uint8, device="cuda")
            finished = torch.zeros((E, A), dtype=torch.bool, device="cuda")
            whole = feats[0] if not two else torch.cat(feats, dim=1)
            final = torch.randn((P, 1), device="cuda")

            def insert():
                st.insert(rewards, finished, feats[0], feats[1], actions, logp, value, dones, probs)

            def insert_torch():
                os.environ["DYNENV_ROLLOUT_FUSED"] = "0"
                try:
                    insert()
                finally:
                    del os.environ["DYNENV_ROLLOUT_FUSED"]

            def feature_copy():
                st.features[0].copy_(whole)

            def returns_fused():
                return st.returns(final)

            def returns_loop():
                return rollout.returns_torch(st.rewards, st.values, st.dones, final, A)
            rewind = st.cursor.zero_
            with torch.no_grad():
                insert()
                assert st.last_route == "fused", st.last_route
                returns_fused()
                assert st.last_returns_route == "fused", st.last_returns_route
                legs = {"insert_fused": (insert, rewind), "insert_torch": (insert_torch, rewind), "feature_copy": (feature_copy, None),
                        "returns_fused": (returns_fused, None), "returns_loop": (returns_loop, None)}
                times = _legs_times(torch, legs, args.calls, args.repeats)
            res = {"config": name, "envs": E, "players": A, "rows": P, "K": K, "T": T, "calls": args.calls * args.repeats,
                   "legs": {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}}
            moved = 2 * 4 * P * K   # the feature row, read and written
            small = P * (8 + 4 + 1 + 1 + 2 * 4 * G + 2 * 4 * G + 2 * 4 + 2 * 4 * N) + E * 5   # rewards, finished, actions, log_probs, value, probs; dones
            res["bytes"] = {"insert": moved + small, "feature_copy": moved}
            res["tb_per_s"] = {"insert_fused": (moved + small) / res["legs"]["insert_fused"]["median_us"] * 1e-6,
                               "feature_copy": moved / res["legs"]["feature_copy"]["median_us"] * 1e-6}
            del st
            if args.collect_calls > 0:
                groups = list(groups_for(env).values())
                Tn, D, X = env.n_time_steps, env.obs_dim, env.action_dim
                torch.manual_seed(K)
                kw = dict(fixed=True, padded_dtype=torch.bfloat16)
                net = GpuFeatureExtractor(groups[0], F, E, A, Tn, D, extended_feature_cnt=X, **kw).requires_grad_(False)
                net2 = GpuFeatureExtractor(groups[1], F, E, A, Tn, D, **kw).requires_grad_(False) if two else None
                pol = GpuPolicyHead(K, env.action_space, seed=7, device="cuda").requires_grad_(False)
                sto = GpuRolloutStorage(T, E, A, pol.action_cols, pol.nvec, K, n_probs=sum(pol.nvec))
                ctimes = {}
                for leg, graph in (("collect_graph", True), ("collect_eager", False)):
                    ro = GpuRollout(env, net, pol, sto, net2=net2, graph=graph)
                    ctimes[leg] = []
                    for _ in range(args.repeats):
                        ctimes[leg] += tc.event_times(torch, ro.collect, args.collect_calls, warmup=1, prepare=sto.after_update)
                    assert ro.routes[1:] == ("fused", "fused"), ro.routes
                res["legs"].update({k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in ctimes.items()})
                assert env.error_flags() == 0
                del net, net2, pol, sto, ro
            env.close()
            results.append(res)
            print(json.dumps(res))
            sys.stdout.flush()
            L = res["legs"]
            line = lambda k: "%8.1f (%.1f .. %.1f)" % (L[k]["median_us"], L[k]["min_us"], L[k]["max_us"]) if k in L else "-"  # noqa: E731
            table.append("%-24s P %6d K %3d | insert fused %s torch %s copy_ %s us | %.2f vs %.2f TB/s | returns fused %s loop %s us | collect graph %s eager %s us" % (
                name, P, K, line("insert_fused"), line("insert_torch"), line("feature_copy"), res["tb_per_s"]["insert_fused"], res["tb_per_s"]["feature_copy"],
                line("returns_fused"), line("returns_loop"), line("collect_graph"), line("collect_eager")))
            torch.cuda.empty_cache()
    print("\n".join(table))
    return tc.write_json(results, args.out)


if __name__ == "__main__":
    main()
