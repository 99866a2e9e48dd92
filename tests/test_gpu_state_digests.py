"""The bytes a reset and the per-environment state transfer produce, against recorded digests (tests/golden/state_digests.json).  -m gpu.

The library has one implementation of each; the file was recorded with the library that still had two (a reset with one thread per
environment, a host path that moved an environment row by row through hipMemcpy) and holds what THOSE produced.  Every entry is
recomputed by the code that wrote it (tests/golden/gen_state_digests.py: reset_flat() twice on per_env_common.situation, get_state(e) of every
environment and the set_state loop on per_env_common.started, at the shapes of tests/test_gpu_reset_masked.py and tests/test_gpu_state_batch.py) and
compared.  checkpoint().size is recorded too: the staging area of dynenv_get_state / dynenv_set_state is not part of a checkpoint."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import gen_state_digests as gen  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "state_digests.json")) as f:
    DOC = json.load(f)
CASES = gen.cases()


def test_every_case_is_recorded():
    """the file holds exactly the cases of the two test modules, but for those left out on purpose, each with its reason"""
    assert set(DOC["digests"]) | set(DOC["left_out"]) == {key for key, _, _, _ in CASES}
    assert not set(DOC["digests"]) & set(DOC["left_out"])
    assert all(isinstance(why, str) and why for why in DOC["left_out"].values())


@pytest.mark.parametrize("key,fn,cfg,shape", [c for c in CASES if c[0] in DOC["digests"]], ids=[c[0] for c in CASES if c[0] in DOC["digests"]])
def test_digests(key, fn, cfg, shape):
    got, want = fn(cfg, shape), DOC["digests"][key]
    assert got == want, "%s: %s" % (key, ", ".join(sorted(k for k in want if got.get(k) != want[k])))
