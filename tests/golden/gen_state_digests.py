#!/usr/bin/env python3
"""SHA-256 digests of what a reset and the per-environment state transfer produce, on the device: tests/golden/state_digests.json.

The library has ONE implementation of each (csrc/driving_reset.hip, csrc/robocup_reset.hip; the state kernels behind
dynenv_get_states / dynenv_set_states, which dynenv_get_state / dynenv_set_state launch for one blob).  The file was first written with
the library that still had a second one - a reset kernel with one thread per environment, a host path that moved an environment row by
row - and pins the bytes of both: tests/test_gpu_state_digests.py recomputes every entry.

  reset/<cfg>/<shape>   situation(cfg, E) of tests/per_env_common.py, then reset_flat() twice: after each, the digest of
                        _ckpt(env) (the checkpoint without Driving Partial's EI_DEFER_OBS) and of the observation's int32 view
  state/<cfg>/<shape>   started(cfg, E, SEED) of tests/per_env_common.py: the digest of get_state(e) for e in range(E),
                        concatenated, and of checkpoint() after the set_state(e, blob) loop over _donor_blobs
  every entry           checkpoint().size: the staging area of the synchronous calls is scratch, not part of a checkpoint

REGENERATE the file whenever the state layout (an array, a blob field, the checkpoint's order) or a reset draw changes ON PURPOSE,
and only then: a digest that changes for any other reason is a bug.  The design is bit-exact, so two runs write the same file; an
entry that differs between two runs of one library goes under "left_out" with the reason, by hand.

Usage (needs the GPU):  python tests/golden/gen_state_digests.py [output.json]"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository
OUT = os.path.join(HERE, "state_digests.json")


def _sha(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def reset_entry(cfg, shape):
    import per_env_common as pc
    env = pc.situation(cfg, pc.SHAPES[shape][0])
    entry = dict(checkpoint_size=int(env.checkpoint().size), ckpt=[], obs=[])
    for _ in range(2):
        obs = env.reset_flat()
        entry["ckpt"].append(_sha(pc.ckpt(env).tobytes()))
        entry["obs"].append(_sha(pc.bits32(obs).tobytes()))
    env.close()
    return entry


def state_entry(cfg, shape):
    import per_env_common as pc
    E, listed = pc.STATE_SHAPES[shape]
    ids = pc.listed_ids(E, listed)
    sts, _ = pc.donor_blobs(cfg, E, ids)
    env = pc.started(cfg, E, pc.SEED)
    entry = dict(checkpoint_size=int(env.checkpoint().size), get_state=_sha(b"".join(bytes(env.get_state(e)) for e in range(E))))
    for e, st in zip(ids, sts):
        env.set_state(e, st)
    entry["set_state_ckpt"] = _sha(env.checkpoint().tobytes())
    env.close()
    return entry


def cases():
    """-> [(key, function, cfg, shape)] in the order of the two test modules' CASES"""
    import per_env_common as pc
    return [("reset/%s/%s" % c, reset_entry) + c for c in pc.CASES] + [("state/%s/%s" % c, state_entry) + c for c in pc.STATE_CASES]


def main(out):
    import torch
    if not torch.cuda.is_available():
        sys.exit("gen_state_digests.py: no HIP device visible - the digests are of what the kernels write, run it on the GPU machine")
    digests = {}
    for key, fn, cfg, shape in cases():
        digests[key] = fn(cfg, shape)
        print(key, flush=True)
    doc = dict(about="SHA-256 of reset and state-transfer results; written by tests/golden/gen_state_digests.py, read by "
                     "tests/test_gpu_state_digests.py", left_out={}, digests=digests)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d entries" % (out, len(digests)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
