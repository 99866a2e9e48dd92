"""tools/exact_state_time.py on the CPU, as far as it goes without a GPU: it imports, its arguments parse, and the listed sets and the
variants it times are what its output says they are."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_exact_state_time_tool_parses_its_arguments():
    import exact_state_time as et
    a = et.parse_args([])
    assert (a.envs, a.calls, a.repeats, a.out) == (4096, 20, 3, None)
    a = et.parse_args(["--envs", "256", "--calls", "5", "--repeats", "2", "--out", "x.json"])
    assert (a.envs, a.calls, a.repeats, a.out) == (256, 5, 2, "x.json")
    for bad in (["--envs", "0"], ["--calls", "-1"], ["--repeats", "0"], ["--steps", "3"]):
        with pytest.raises(SystemExit):
            et.parse_args(bad)
    assert [c[0] for c in et.CONFIGS] == ["Driving Full, 10 cars", "RoboCup Full, 5 per team"]


def test_the_variants_are_the_four_calls_for_each_listed_set():
    import exact_state_time as et
    assert et.CALLS == ("get_states", "get_exact", "set_states", "set_exact") and et.SETS == ("all", "64", "7")
    assert len(et.VARIANTS) == 12 and len(set(et.VARIANTS)) == 12
    assert et.VARIANTS[:4] == ("get_states_all", "get_exact_all", "set_states_all", "set_exact_all")
    assert set(et.VARIANTS) == {"%s_%s" % (c, s) for c in et.CALLS for s in et.SETS}
    assert et.LOOKAHEAD == ("steps5", "save_steps5_restore") and et.LOOKAHEAD_STEPS == 5


def test_listed_sets_are_all_64_and_7_spread_over_the_batch():
    import exact_state_time as et
    s = et.listed_sets(4096)
    assert tuple(s) == et.SETS
    assert s["all"] is None and et.listed_count(4096, s["all"]) == 4096
    assert s["64"] == list(range(0, 4096, 64)) and et.listed_count(4096, s["64"]) == 64
    assert len(s["7"]) == 7 and s["7"][0] == 0 and s["7"][-1] == (6 * 4096) // 7 and s["7"] == sorted(set(s["7"]))
    s = et.listed_sets(70)
    assert len(s["64"]) == 64 and len(set(s["64"])) == 64 and 0 <= min(s["64"]) and max(s["64"]) < 70
    s = et.listed_sets(5)   # fewer environments than asked for: each of them once
    assert s["64"] == s["7"] == [0, 1, 2, 3, 4]
    assert et.listed_sets(1)["7"] == [0]
