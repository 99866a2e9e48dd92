"""The numpy restatement of the arranger's backward (tests/arranger_grad_ref.py: unpad) against the gradients autograd returned through
the reference's own InOutArranger.rearrange_outputs (tests/golden/arranger_grad.npz), bit for bit; the adjoint identity with
arranger_ref.pad; the helper's slot arithmetic against arranger_ref.gather; and, where the reference is present, the fixture itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_ref as R  # noqa: E402
import arranger_grad_ref as GR  # noqa: E402

EXPECTED_CASES = ["driving_full", "driving_partial", "empty_type", "robocup", "robocup_t5", "static", "width12"]


def test_fixture_holds_the_cases_it_should():
    assert GR.CASES == EXPECTED_CASES
    assert os.path.getsize(GR.GOLDEN) < 512 * 1024
    c = GR.golden_case("robocup_t5")
    assert c["T"] == 5 and c["nT"] == 4
    assert GR.golden_case("width12")["F"] == 12
    e = GR.golden_case("empty_type")
    assert e["has_emb"] == [True, False, True] and e["embs"][1] is None and len(e["slots"][1]) == 0
    for name in GR.CASES:
        c = GR.golden_case(name)
        assert c["G"].shape == c["padded"].shape == (c["T"], c["plan"]["max_count"], c["P"], c["F"])
        assert len(np.unique(c["plan"]["obj_counts"])) > 1, "ragged"


@pytest.mark.parametrize("name", EXPECTED_CASES)
def test_unpad_reproduces_the_reference_gradients(name):
    c = GR.golden_case(name)
    # the slots are the forward's: pad() of the recorded embeddings is the recorded padded tensor
    assert np.array_equal(R.pad(c["embs"], c["slots"], c["T"], c["plan"]["max_count"], c["P"], c["F"]), c["padded"])
    got = GR.unpad(c["G"], c["slots"])
    for i in range(c["nT"]):
        if c["has_emb"][i]:
            assert got[i].dtype == np.float32 and got[i].tobytes() == c["grads"][i].tobytes(), "gradient of type %d" % i
        else:
            assert got[i].shape == (0, c["F"])
    # no slot is used twice, so nothing is summed
    allslots = np.concatenate(c["slots"])
    assert len(np.unique(allslots)) == len(allslots)


def test_slots_from_counts_alone_are_the_gathered_slots():
    rng = np.random.default_rng(4)
    specs = [(3, 4, R.COUNT_ROW, -1, 6), (2, 3, R.COUNT_ENV, -1, 4), (5, 2, R.COUNT_CONST, 1, 2), (2, 0, R.COUNT_CONST, 3, 3)]
    obs, types, ce = R.make_dense(rng, 37, 3, 2, specs, lead=1)
    pl = R.plan(obs, types, ce)
    _, slots, _ = R.gather(obs, types, pl)
    pl2 = GR.plan_from_counts(pl["counts"])
    assert pl2["max_count"] == pl["max_count"] and np.array_equal(pl2["base"], pl["base"])
    for a, b in zip(GR.slots_from_plan(pl2), slots):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_unpad_is_the_adjoint_of_pad(seed):
    """sum(pad(x) * G) == sum_i sum(x_i * unpad(G)_i), on small integers held in float32: every product and partial sum is an integer
    far below 2^24, so both sides are exact and compared with =="""
    rng = np.random.default_rng(seed)
    specs = [(3, 5, R.COUNT_ROW, -1, 6), (2, 3, R.COUNT_ENV, 0, 3), (1, 0, R.COUNT_CONST, 2, 2), (4, 2, R.COUNT_CONST, 1, 2)]
    E, T, A, F = 9, 2 + seed, 3, 5 + seed
    obs, types, ce = R.make_dense(rng, E, T, A, specs)
    pl = R.plan(obs, types, ce)
    _, slots, _ = R.gather(obs, types, pl)
    P, M = E * A, pl["max_count"]
    xs = [rng.integers(-8, 9, (len(s), F)).astype(np.float32) if len(s) else None for s in slots]
    Gr = rng.integers(-8, 9, (T, M, P, F)).astype(np.float32)
    lhs = np.sum(R.pad(xs, slots, T, M, P, F) * Gr, dtype=np.float32)
    gs = GR.unpad(Gr, slots)
    rhs = np.float32(sum(np.sum(x * g, dtype=np.float32) for x, g in zip(xs, gs) if x is not None))
    assert abs(float(lhs)) < 2 ** 24 and lhs == rhs
    assert lhs == np.sum(R.pad(xs, slots, T, M, P, F).astype(np.int64) * Gr.astype(np.int64))   # (and exact: the integer sum)


def test_fixture_is_what_the_reference_computes_today():
    """regenerated in memory from the reference and compared byte for byte (only where the reference is present)"""
    before = dict(sys.modules)
    path = list(sys.path)
    golden = os.path.join(GR.ROOT, "tests", "golden")
    foreign = [golden]
    try:
        sys.path.insert(0, golden)
        import gen_golden as gg
        foreign.append(gg.REF)
        if not os.path.isdir(os.path.join(gg.REF, "DynEnv")):
            pytest.skip("the reference is not on this machine")
        import gen_golden_arranger_grad as gen
        fresh = gen.generate()
    finally:
        # the generator imports the reference behind stand-ins for pymunk & co.: leave neither to other tests.  A stand-in has no
        # import spec; the reference's and the generators' modules are known by their files.  (Real modules imported on the way stay.)
        for k, m in list(sys.modules.items()):
            if k not in before and (getattr(m, "__spec__", None) is None
                                    or str(getattr(m, "__file__", None) or "").startswith(tuple(foreign))):
                del sys.modules[k]
        sys.modules.update(before)
        sys.path[:] = path
    assert sorted(fresh) == sorted(GR.G.files)
    for k in GR.G.files:
        a, b = GR.G[k], fresh[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
