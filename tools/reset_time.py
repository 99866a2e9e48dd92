#!/usr/bin/env python3
"""What a reset costs, for the whole batch and for chosen environments, for Driving Full with 10 cars and RoboCup Full with 5 robots per
team.  One process, HIP events around the C entry points on the handle's own buffers, a warm-up, and the variants alternating within
every repeat (--repeats: the run-to-run spread):
  (a) dynenv_reset                       every environment: the reset kernels (one wave per environment) launched without a mask
  (b) dynenv_reset_masked, all listed    the same kernels and the same work behind a mask of ones: (b) - (a) is what the mask test costs
  (c) dynenv_reset_masked, 0 listed      what the launches cost when nothing is to be done
  (d) dynenv_reset_masked, E / 600 (7 of 4096) and 64 listed, also as a share of the mean step time of (e)
  (e) the mean step time over one whole episode in lock-step, against the mean of step + reset_masked(dones) over as many steps of a
      batch whose environments are staggered evenly over the episode's phases (episodes="per_env").  The staggered batch is written with
      set_states from blobs of environments that really are at that phase - a donor runs one episode and keeps get_states() every
      10 steps - with `elapsed` edited to the environment's exact step.
Usage (GPU box): python tools/reset_time.py [--envs 4096] [--calls 20] [--repeats 3] [--no-episode] [--out FILE]"""
import statistics
import sys

from timing_common import CONFIGS, action_pool, base_parser, event_times, fmt, mid_episode, parse_positive, spread_ids, write_json

SNAP_EVERY = 10


def parse_args(argv=None):
    ap = base_parser(__doc__)
    ap.add_argument("--no-episode", action="store_true", help="skip (e), the two whole-episode runs per repeat")
    return parse_positive(ap, argv)


def mean_step_us(torch, env, acts, steps, auto_reset):
    """mean device time of `steps` calls of step_flat, one pair of events around all of them"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for s in range(steps):
        env.step_flat(acts[s % len(acts)], auto_reset=auto_reset)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def staggered_blobs(torch, make, acts, E, steps, sub):
    """uint8 [E, state_size] on the device: environment e at step e * steps // E of its episode"""
    donor = make()
    donor.reset_flat()
    snaps = [donor.get_states()]
    for s in range(steps - 1):
        donor.step_flat(acts[s % len(acts)], auto_reset=False)
        if (s + 1) % SNAP_EVERY == 0:
            snaps.append(donor.get_states())
    phase = (torch.arange(E, device="cuda") * steps) // E
    allb = torch.stack(snaps)                                   # [K, E, size]
    blobs = allb[phase // SNAP_EVERY, torch.arange(E, device="cuda")].contiguous()
    blobs.view(torch.int32)[:, 0] = (phase * sub).to(torch.int32)   # `elapsed` is the first word of both blob types
    donor.close()
    return blobs


def measure(name, type_name, players, hi, args, seed):
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, _capi
    E = args.envs
    env_type = getattr(DynEnvType, type_name)
    make = lambda **kw: BatchedDynEnv(env_type, E, players, seed=seed, **kw)
    env = make()
    A = env.n_agents
    acts = action_pool(torch, np, hi, E, A, seed)
    mid_episode(env, acts)
    lib, h, stream, obs = env._lib, env._h, env._stream(), _capi.ptr(env.obs)
    n_small = max(1, round(E / 600))
    masks = {}
    for key, ids in (("all", list(range(E))), ("none", []), ("few", spread_ids(E, n_small)), ("64", spread_ids(E, 64))):
        m = torch.zeros((E,), dtype=torch.uint8, device="cuda")
        if ids:
            m[ids] = 1
        masks[key] = m
    variants = [("reset", lambda: _capi.check(lib.dynenv_reset(h, obs, stream), "dynenv_reset"))]
    for key in ("all", "none", "few", "64"):
        ptr = _capi.ptr(masks[key])
        variants.append(("masked_" + key, lambda ptr=ptr: _capi.check(lib.dynenv_reset_masked(h, ptr, obs, stream), "dynenv_reset_masked")))
    steps = env.steps_per_episode
    sub = env._substeps()
    times = {k: [] for k, _ in variants}
    lock, stag = [], []
    blobs = None if args.no_episode else staggered_blobs(torch, make, acts, E, steps, sub)
    for r in range(args.repeats):
        for k, f in variants:   # (alternating: every variant once per repeat)
            times[k].append(statistics.median(event_times(torch, f, args.calls)))
        if args.no_episode:
            continue
        a = make()
        a.reset_flat()
        mean_step_us(torch, a, acts, 20, False)   # warm-up
        a.reset_flat()
        lock.append(mean_step_us(torch, a, acts, steps, False))
        a.close()
        b = make(episodes="per_env")
        b.set_states(None, blobs)
        mean_step_us(torch, b, acts, 20, True)
        b.set_states(None, blobs)
        stag.append(mean_step_us(torch, b, acts, steps, True))
        assert b.error_flags() == 0
        b.close()
    assert env.error_flags() == 0
    env.close()
    step_us = statistics.median(lock) if lock else None
    share = lambda v: "" if step_us is None else "  = %.2f %% of a step" % (100.0 * statistics.median(v) / step_us)
    print("== %s: %d environments, medians of %d calls" % (name, E, args.calls))
    print("(a) dynenv_reset                      %s" % fmt(times["reset"]))
    print("(b) dynenv_reset_masked, all listed   %s" % fmt(times["masked_all"]))
    print("(c) dynenv_reset_masked, 0 listed     %s" % fmt(times["masked_none"]))
    print("(d) dynenv_reset_masked, %4d listed  %s%s" % (n_small, fmt(times["masked_few"]), share(times["masked_few"])))
    print("(d) dynenv_reset_masked,   64 listed  %s%s" % (fmt(times["masked_64"]), share(times["masked_64"])))
    if lock:
        print("(e) mean step, lock-step episode      %s  (%d steps)" % (fmt(lock), steps))
        print("(e) mean step + reset_masked(dones), staggered batch   %s  (%d steps, ~%.1f environments end per step)" % (fmt(stag), steps, E / steps))
    sys.stdout.flush()
    return dict(config=name, envs=E, calls=args.calls, listed_few=n_small, reset_us=times["reset"], masked_all_us=times["masked_all"],
                masked_none_us=times["masked_none"], masked_few_us=times["masked_few"], masked_64_us=times["masked_64"],
                lockstep_mean_step_us=lock, staggered_mean_step_us=stag, steps=steps)


def main(argv=None):
    args = parse_args(argv)
    results = [measure(name, type_name, players, hi, args, 42) for name, type_name, players, hi in CONFIGS]
    return write_json(results, args.out)


if __name__ == "__main__":
    main()
