#!/usr/bin/env python3
"""What a step of chosen environments costs (dynenv_step_masked), for Driving Full with 10 cars and RoboCup Full with 5 robots per team.
One process, HIP events around the C entry points on the handle's own buffers, a warm-up, and the variants alternating within every
repeat (--repeats: the run-to-run spread).  Every variant's calls start from the same checkpoint, 30 steps into the episode:
  (a) dynenv_step                               every environment
  (b) dynenv_step_masked, all listed            the same kernel behind a mask of ones: (b) - (a) is what the mask test costs
  (c) dynenv_step_masked, 0 listed              a launch of blocks that end at once
  (d) dynenv_step_masked, every other listed    half the work on every SIMD; the launch lasts as long as its slowest listed environment
  (e) dynenv_step_masked, the slowest tenth frozen
      "slowest": the batch is cut into groups of consecutive environments (--groups), each group is stepped alone from the checkpoint
      (the median of three launches: a launch lasts as long as its slowest environment) and the slowest groups that make up a tenth
      of the batch are the ones left out.
Usage (GPU box): python tools/step_masked_time.py [--envs 4096] [--calls 20] [--repeats 3] [--groups 64] [--out FILE]"""
import statistics
import sys

from timing_common import CONFIGS, action_pool, base_parser, event_times, fmt, mid_episode, parse_positive, write_json

VARIANTS = ("step", "masked_all", "masked_none", "masked_half", "masked_fast")


def parse_args(argv=None):
    ap = base_parser(__doc__)
    ap.add_argument("--groups", type=int, default=64, help="groups of consecutive environments timed alone to find the slowest tenth")
    return parse_positive(ap, argv, also=("groups",))


def group_bounds(E, groups):
    """[(first, end)] of min(groups, E) groups of consecutive environments that cover [0, E), sizes differing by at most one"""
    g = max(1, min(groups, E))
    return [((k * E) // g, ((k + 1) * E) // g) for k in range(g)]


def slowest_tenth(bounds, group_us, E):
    """the environments of the slowest groups, slowest first, until a tenth of the batch (rounded up, at least one group) is reached"""
    want, out = -(-E // 10), []
    for k in sorted(range(len(bounds)), key=lambda k: (-group_us[k], k)):
        if len(out) >= want:
            break
        out.extend(range(*bounds[k]))
    return sorted(out)


def mask_bytes(E, listed):
    """uint8 [E] as a list: 1 for the listed environments"""
    m = [0] * E
    for e in listed:
        m[e] = 1
    return m


def measure(name, type_name, players, hi, args, seed):
    import numpy as np
    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType, _capi
    E = args.envs
    env = BatchedDynEnv(getattr(DynEnvType, type_name), E, players, seed=seed, episodes="per_env")
    acts = action_pool(torch, np, hi, E, env.n_agents, seed)
    mid_episode(env, acts)
    start = env.checkpoint()
    lib, h, stream = env._lib, env._h, env._stream()
    obs, rew, don = (_capi.ptr(t) for t in (env.obs, env.rewards, env.dones))
    nxt = [0]

    def action():
        nxt[0] += 1
        return _capi.ptr(acts[nxt[0] % len(acts)])

    def masked(m):
        ptr = _capi.ptr(m)
        return lambda: _capi.check(lib.dynenv_step_masked(h, ptr, action(), None, obs, rew, don, stream), "dynenv_step_masked")

    def tensor(listed):
        return torch.tensor(mask_bytes(E, listed), dtype=torch.uint8, device="cuda")

    # the slowest tenth: every group of consecutive environments alone, from the checkpoint
    bounds = group_bounds(E, args.groups)
    group_us = []
    for first, end in bounds:
        f = masked(tensor(range(first, end)))
        one = []
        for _ in range(3):
            env.restore(start)
            one.append(event_times(torch, f, 1, warmup=0)[0])
        group_us.append(statistics.median(one))
    frozen = slowest_tenth(bounds, group_us, E)
    keep = (tensor(range(E)), tensor([]), tensor(range(0, E, 2)), tensor(sorted(set(range(E)) - set(frozen))))   # (alive while timed)
    calls = {"step": lambda: _capi.check(lib.dynenv_step(h, action(), obs, rew, don, stream), "dynenv_step"),
             "masked_all": masked(keep[0]), "masked_none": masked(keep[1]), "masked_half": masked(keep[2]), "masked_fast": masked(keep[3])}
    times = {k: [] for k in VARIANTS}
    for r in range(args.repeats):
        for k in VARIANTS:   # (alternating: every variant once per repeat, each from the same state and with the same actions)
            env.restore(start)
            nxt[0] = 0
            times[k].append(statistics.median(event_times(torch, calls[k], args.calls)))
    assert env.error_flags() == 0
    env.close()
    print("== %s: %d environments, medians of %d calls" % (name, E, args.calls))
    print("(a) dynenv_step                                %s" % fmt(times["step"]))
    print("(b) dynenv_step_masked, all listed             %s" % fmt(times["masked_all"]))
    print("(c) dynenv_step_masked, 0 listed               %s" % fmt(times["masked_none"]))
    print("(d) dynenv_step_masked, every other listed     %s" % fmt(times["masked_half"]))
    print("(e) dynenv_step_masked, slowest tenth frozen   %s  (%d environments of the %d slowest of %d groups; a group alone: %.1f .. %.1f us)"
          % (fmt(times["masked_fast"]), len(frozen), sum(1 for b in bounds if b[0] in frozen), len(bounds), min(group_us), max(group_us)))
    sys.stdout.flush()
    return dict(config=name, envs=E, calls=args.calls, groups=len(bounds), group_us=group_us, frozen=len(frozen),
                **{k + "_us": v for k, v in times.items()})


def main(argv=None):
    args = parse_args(argv)
    results = [measure(name, type_name, players, hi, args, 42) for name, type_name, players, hi in CONFIGS]
    return write_json(results, args.out)


if __name__ == "__main__":
    main()
