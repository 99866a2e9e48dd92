"""tools/step_masked_time.py on the CPU, as far as it goes without a GPU: it imports, its arguments parse, and the groups it times and
the tenth it freezes are what its output says they are."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_step_masked_time_tool_parses_its_arguments():
    import step_masked_time as st
    a = st.parse_args([])
    assert (a.envs, a.calls, a.repeats, a.groups, a.out) == (4096, 20, 3, 64, None)
    a = st.parse_args(["--envs", "256", "--calls", "5", "--repeats", "2", "--groups", "8", "--out", "x.json"])
    assert (a.envs, a.calls, a.repeats, a.groups, a.out) == (256, 5, 2, 8, "x.json")
    for bad in (["--envs", "0"], ["--calls", "-1"], ["--groups", "0"], ["--steps", "3"]):
        with pytest.raises(SystemExit):
            st.parse_args(bad)
    assert [c[0] for c in st.CONFIGS] == ["Driving Full, 10 cars", "RoboCup Full, 5 per team"]
    assert st.VARIANTS == ("step", "masked_all", "masked_none", "masked_half", "masked_fast")


def test_groups_cover_the_batch_and_the_slowest_tenth_is_the_slowest_groups():
    import step_masked_time as st
    b = st.group_bounds(4096, 64)
    assert len(b) == 64 and b[0] == (0, 64) and b[-1] == (4032, 4096) and all(x[1] == y[0] for x, y in zip(b, b[1:]))
    b = st.group_bounds(70, 64)
    assert len(b) == 64 and b[0][0] == 0 and b[-1][1] == 70 and {e - f for f, e in b} == {1, 2}
    assert st.group_bounds(5, 64) == [(k, k + 1) for k in range(5)]
    b = st.group_bounds(4096, 64)
    us = [100.0 + k for k in range(64)]           # the last groups are the slowest
    frozen = st.slowest_tenth(b, us, 4096)
    assert len(frozen) == 7 * 64 and frozen[0] == 57 * 64 and frozen[-1] == 4095, "410 environments rounded up to whole groups"
    us[3] = 1000.0
    assert st.slowest_tenth(b, us, 4096)[:64] == list(range(192, 256))
    assert st.slowest_tenth([(0, 1)], [5.0], 1) == [0]
    assert st.mask_bytes(5, [3, 0, 4]) == [1, 0, 0, 1, 1] and st.mask_bytes(3, []) == [0, 0, 0]
