#!/usr/bin/env python3
"""What saving and restoring environments on the device costs, exactly (dynenv_get_exact / dynenv_set_exact) and canonically
(dynenv_get_states / dynenv_set_states), for Driving Full with 10 cars and RoboCup Full with 5 robots per team.  One process, HIP
events around the C entry points on preallocated device buffers, a warm-up, and the variants alternating within every repeat
(--repeats: the run-to-run spread).  The handle is 30 steps into its episode.
  per call, in microseconds, with all / 64 / 7 environments listed (spread over the batch, as an index list; "all" without one):
      get_states, get_exact, set_states, set_exact      (the blobs a set writes are the ones the get of the same listed set saved)
  a lookahead: get_exact of every environment + 5 steps + set_exact of every environment, against the same 5 steps alone (both from
  the same state with the same actions: the state is put back, untimed, in front of every timed call).
Usage (GPU box): python tools/exact_state_time.py [--envs 4096] [--calls 20] [--repeats 3] [--out FILE]"""
import statistics
import sys

from timing_common import CONFIGS, action_pool, base_parser, event_times, fmt, mid_episode, parse_positive, spread_ids, write_json

CALLS = ("get_states", "get_exact", "set_states", "set_exact")
SETS = ("all", "64", "7")
VARIANTS = tuple("%s_%s" % (c, s) for s in SETS for c in CALLS)
LOOKAHEAD = ("steps5", "save_steps5_restore")
LOOKAHEAD_STEPS = 5


def parse_args(argv=None):
    return parse_positive(base_parser(__doc__), argv)


def listed_sets(E):
    """name -> the environments listed: "all" = None (no index list: environments 0..E-1), "64" and "7" = that many distinct
    environments spread evenly over [0, E) (all of them where E is smaller)"""
    return {"all": None, "64": spread_ids(E, 64), "7": spread_ids(E, 7)}


def listed_count(E, listed):
    return E if listed is None else len(listed)


def measure(name, type_name, players, hi, args, seed):
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, _capi
    E = args.envs
    env = BatchedDynEnv(getattr(DynEnvType, type_name), E, players, seed=seed, episodes="per_env")
    acts = action_pool(torch, np, hi, E, env.n_agents, seed)
    mid_episode(env, acts)
    lib, h, stream = env._lib, env._h, env._stream()
    obs, rew, don = (_capi.ptr(t) for t in (env.obs, env.rewards, env.dones))
    sizes = {"states": env.state_size, "exact": env.exact_size}
    calls, keep = {}, []
    for sname, listed in listed_sets(E).items():
        n = listed_count(E, listed)
        ids = None if listed is None else torch.tensor(listed, dtype=torch.int32, device="cuda")
        idp = _capi.ptr(ids)
        status = torch.zeros((n,), dtype=torch.int32, device="cuda")
        keep += [ids, status]
        for kind in ("states", "exact"):
            blobs = torch.zeros((n, sizes[kind]), dtype=torch.uint8, device="cuda")
            keep.append(blobs)
            get, put = getattr(lib, "dynenv_get_" + kind), getattr(lib, "dynenv_set_" + kind)
            bp, sp = _capi.ptr(blobs), _capi.ptr(status)
            calls["get_%s_%s" % (kind, sname)] = (lambda get=get, idp=idp, n=n, bp=bp, kind=kind:
                                                  _capi.check(get(h, idp, n, bp, stream), "dynenv_get_" + kind))
            calls["set_%s_%s" % (kind, sname)] = (lambda put=put, idp=idp, n=n, bp=bp, sp=sp, kind=kind:
                                                  _capi.check(put(h, idp, n, bp, sp, stream), "dynenv_set_" + kind))
            calls["get_%s_%s" % (kind, sname)]()   # (the blobs every timed set writes)
    nxt = [0]

    def steps():
        for _ in range(LOOKAHEAD_STEPS):
            nxt[0] += 1
            _capi.check(lib.dynenv_step(h, _capi.ptr(acts[nxt[0] % len(acts)]), obs, rew, don, stream), "dynenv_step")

    def lookahead():
        calls["get_exact_all"]()
        steps()
        calls["set_exact_all"]()

    start = env.get_exact()

    def rewind():
        env.set_exact(None, start)
        nxt[0] = 0

    times = {k: [] for k in VARIANTS + LOOKAHEAD}
    for r in range(args.repeats):
        for k in VARIANTS:   # (alternating: every variant once per repeat)
            times[k].append(statistics.median(event_times(torch, calls[k], args.calls)))
        for k, f in zip(LOOKAHEAD, (steps, lookahead)):   # (every timed call from the same state, with the same actions)
            times[k].append(statistics.median(event_times(torch, f, max(2, args.calls // LOOKAHEAD_STEPS), warmup=1, prepare=rewind)))
    assert env.error_flags() == 0
    env.close()
    print("== %s: %d environments, medians of %d calls; canonical blob %d bytes, exact blob %d bytes" % (name, E, args.calls, sizes["states"], sizes["exact"]))
    for sname, listed in listed_sets(E).items():
        for c in CALLS:
            print("%-10s %4d listed   %s" % (c, listed_count(E, listed), fmt(times["%s_%s" % (c, sname)])))
    print("%d steps alone                             %s" % (LOOKAHEAD_STEPS, fmt(times["steps5"])))
    print("get_exact(all) + %d steps + set_exact(all)  %s" % (LOOKAHEAD_STEPS, fmt(times["save_steps5_restore"])))
    sys.stdout.flush()
    return dict(config=name, envs=E, calls=args.calls, state_bytes=sizes["states"], exact_bytes=sizes["exact"],
                **{k + "_us": v for k, v in times.items()})


def main(argv=None):
    args = parse_args(argv)
    results = [measure(name, type_name, players, hi, args, 42) for name, type_name, players, hi in CONFIGS]
    return write_json(results, args.out)


if __name__ == "__main__":
    main()
