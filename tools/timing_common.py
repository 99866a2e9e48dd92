"""What the per-environment timing tools share (reset_time.py, step_masked_time.py, exact_state_time.py, state_transfer_time.py): the two
configurations they time, HIP-event timing of a call, environment ids spread over a batch, a pool of random actions, a handle that
is some steps into its episode, the base argument parser, the "median (min .. max)" line and the JSON tail.  A tool keeps the variants
it times and the lines it prints."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, DynEnvType's name, players, the actions' exclusive upper bounds)
CONFIGS = (("Driving Full, 10 cars", "DRIVE", 10, (3, 3)), ("RoboCup Full, 5 per team", "ROBO_CUP", 5, (5, 3, 3, 7)))


def base_parser(doc, calls_help="timed calls per variant and repeat"):
    """--envs, --calls, --repeats and --out; a tool adds its own options and hands the parser to parse_positive"""
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20, help=calls_help)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the results as JSON to this file as well")
    return ap


def parse_positive(ap, argv=None, also=()):
    """the arguments, after the check that --envs, --calls, --repeats and the options named in `also` are positive"""
    args = ap.parse_args(argv)
    names = ("envs", "calls", "repeats") + tuple(also)
    if any(getattr(args, n) < 1 for n in names):
        ap.error("%s and --%s must be positive" % (", ".join("--" + n for n in names[:-1]), names[-1]))
    return args


def spread_ids(E, n):
    """n environment ids spread evenly over [0, E) (all of them where E is smaller)"""
    n = max(0, min(n, E))
    return sorted(set((k * E) // n for k in range(n))) if n else []


def event_times(torch, f, calls, warmup=3, prepare=None):
    """device microseconds of each of `calls` calls of f, every call between its own pair of events; `prepare` runs, untimed, in front
    of every call"""
    for _ in range(warmup):
        if prepare:
            prepare()
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if prepare:
            prepare()
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def action_pool(torch, np, hi, E, A, seed, n=16):
    """n random int32 [E, A, len(hi)] action tensors on the device"""
    rng = np.random.default_rng(seed)
    return [torch.tensor(np.stack([rng.integers(0, h, (E, A)) for h in hi], -1).astype(np.int32), device="cuda") for _ in range(n)]


def mid_episode(env, acts, steps=30):
    """reset `env` and step it `steps` times with the pool's actions: pedestrians under way, contacts cached"""
    env.reset_flat()
    for s in range(steps):
        env.step_flat(acts[s % len(acts)], auto_reset=False)
    return env


def fmt(v):
    """a variant's medians, one per repeat"""
    return "%8.1f us (%.1f .. %.1f over %d repeats)" % (statistics.median(v), min(v), max(v), len(v))


def write_json(results, out):
    """the results to the file --out names, if it names one"""
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
    return results
