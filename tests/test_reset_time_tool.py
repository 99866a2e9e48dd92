"""tools/reset_time.py on the CPU, as far as it goes without a GPU: it imports, its arguments parse, and the environments it lists
for the partial resets are what its output says they are."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_reset_time_tool_parses_its_arguments():
    import reset_time as rt
    a = rt.parse_args([])
    assert (a.envs, a.calls, a.repeats, a.no_episode, a.out) == (4096, 20, 3, False, None)
    a = rt.parse_args(["--envs", "256", "--calls", "5", "--repeats", "2", "--no-episode", "--out", "x.json"])
    assert (a.envs, a.calls, a.repeats, a.no_episode, a.out) == (256, 5, 2, True, "x.json")
    for bad in (["--envs", "0"], ["--calls", "-1"], ["--steps", "3"]):
        with pytest.raises(SystemExit):
            rt.parse_args(bad)
    assert round(4096 / 600) == 7 and len(rt.spread_ids(4096, 7)) == 7 and len(rt.spread_ids(4096, 64)) == 64
    assert rt.spread_ids(4096, 64)[:3] == [0, 64, 128] and rt.spread_ids(5, 64) == [0, 1, 2, 3, 4] and rt.spread_ids(70, 0) == []
    assert [c[0] for c in rt.CONFIGS] == ["Driving Full, 10 cars", "RoboCup Full, 5 per team"]
