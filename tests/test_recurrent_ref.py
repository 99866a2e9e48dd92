"""tests/recurrent_ref.py - the numpy float64 statement the GPU tests of the fused recurrent head compare against - held to the torch
route of GpuRecurrentHead in float64 on the CPU, and, where the reference is on this machine, that route to the tail of the reference's
own DynEnvFeatureExtractor (DynEnv/models/models.py:574-619: TransformNet, LSTMLayer, bn) bit for bit, with its state_dict() loaded
strict=True.  The names and shapes of a whole DynEnvFeatureExtractor.state_dict() are kept in tests/golden/ (the device test loads
them into GpuFeatureExtractor, which needs a device to exist) and held to the reference here.  No GPU."""
import ast
import itertools
import json
import os
import sys
from typing import List

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recurrent_ref as RR  # noqa: E402

REF_MODELS = "/root/reference/DynEnv/models/models.py"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_extractor_state_dict.json")
SHAPES = [(1, 1, 64, 0), (6, 3, 128, 6), (5, 2, 64, 13), (3, 4, 32, 5)]   # (E, A, F, X)


def _inputs(E, A, F, X, steps=3, seed=0):
    rng = np.random.default_rng(seed + 7 * E + F + X)
    P = E * A
    feats = rng.standard_normal((steps, P, F))
    exts = rng.standard_normal((steps, P, X)) if X else [None] * steps
    masks = [None] * steps
    masks[1] = np.arange(E) % 2 == 0   # the mask at step 2
    return feats, exts, masks


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_statement_is_the_torch_route_in_float64_over_chained_steps(shape):
    import torch
    from dynenv_amd import GpuRecurrentHead
    E, A, F, X = shape
    feats, exts, masks = _inputs(*shape)
    pr = RR.make_params(F, X, seed=E)
    layer = RR.load(GpuRecurrentHead(F, A, E, X), pr, torch.float64)
    assert layer.last_route is None and layer.h.dtype == torch.float64 and tuple(layer.h.shape) == (E * A, F)
    h = c = np.zeros((E * A, F))
    for s in range(3):
        h, c, want = RR.head_step(feats[s], exts[s], h, c, masks[s], A, pr)
        with torch.no_grad():
            got = layer(torch.from_numpy(feats[s]), None if exts[s] is None else torch.from_numpy(exts[s]),
                        None if masks[s] is None else torch.from_numpy(masks[s]))
        assert layer.last_route.startswith("torch (fallback: "), "a CPU call reports a fallback"
        assert got.dtype == torch.float64 and tuple(got.shape) == (E * A, F)
        assert np.abs(got.numpy() - want).max() < 1e-12, s
        assert np.abs(layer.h.numpy() - h).max() < 1e-12 and np.abs(layer.c.numpy() - c).max() < 1e-12, s
    assert np.abs(h).max() > 0.01 and np.abs(c).max() > 0.01
    # the statement never looks at the state of a reset environment
    junk_h, junk_c = h.copy(), c.copy()
    rows = np.repeat(masks[1], A)
    junk_h[rows] = np.nan
    junk_c[rows] = np.nan
    a = RR.head_step(feats[0], exts[0], h, c, masks[1], A, pr)
    b = RR.head_step(feats[0], exts[0], junk_h, junk_c, masks[1], A, pr)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # uint8 masks are bool masks; gradients wanted: the same values through the differentiable route
    twin = RR.load(GpuRecurrentHead(F, A, E, X), pr, torch.float64)
    twin.set_states(layer.get_states())
    ext0 = None if exts[0] is None else torch.from_numpy(exts[0])
    with torch.no_grad():
        want = layer(torch.from_numpy(feats[0]), ext0, torch.from_numpy(masks[1]))
    got = twin(torch.from_numpy(feats[0]), ext0, torch.from_numpy(masks[1].astype(np.uint8)))
    assert twin.last_route == "torch" and got.grad_fn is not None and twin.h.grad_fn is not None
    assert torch.equal(got.detach(), want) and torch.equal(twin.c.detach(), layer.c)


def test_names_and_shapes_are_the_reference_architecture():
    import dynenv_amd
    from dynenv_amd import GpuRecurrentHead
    assert "GpuRecurrentHead" in dynenv_amd.__all__ and "GpuFeatureExtractor" in dynenv_amd.__all__
    F, X = 64, 6
    layer = GpuRecurrentHead(F, 3, 2, X)
    assert not list(layer.buffers()), "h and c are plain attributes: state_dict() holds parameters alone"
    assert tuple(layer.state_dict()) == RR.NAMES
    want = {"TransformNet.0.weight": (F, F + X), "TransformNet.0.bias": (F,), "TransformNet.2.weight": (F,), "TransformNet.2.bias": (F,),
            "LSTM.cell.weight_ih": (4 * F, F), "LSTM.cell.weight_hh": (4 * F, F), "LSTM.cell.bias_ih": (4 * F,), "LSTM.cell.bias_hh": (4 * F,),
            "LSTM.transformer.0.weight": (F, 6), "LSTM.transformer.0.bias": (F,), "bn.weight": (F,), "bn.bias": (F,)}
    assert {k: tuple(v.shape) for k, v in layer.named_parameters()} == want
    assert layer.TransformNet[1].negative_slope == RR.SLOPE and layer.TransformNet[2].eps == layer.bn.eps == RR.EPS
    pr = RR.make_params(F, X)
    assert tuple(pr) == RR.NAMES and all(np.abs(v).max() > 0.1 for k, v in pr.items() if "bias" in k)


def test_state_semantics_are_the_reference_lstm_layers():
    import torch
    from dynenv_amd import GpuRecurrentHead
    E, A, F = 3, 2, 64
    layer = GpuRecurrentHead(F, A, E)
    P = E * A
    assert tuple(layer.h.shape) == tuple(layer.c.shape) == (P, F) and not layer.h.any() and not layer.c.any()
    x = torch.randn(P, F)
    out = layer(x)
    assert layer.last_route == "torch" and layer.h.grad_fn is not None, "gradients wanted: h and c are the cell's results"
    layer.detach()
    assert layer.h.grad_fn is None and layer.c.grad_fn is None and out.grad_fn is not None
    # get_states clones, set_states clones
    h, c = layer.get_states()
    assert torch.equal(h, layer.h) and h.data_ptr() != layer.h.data_ptr()
    given = [torch.full((P, F), 0.25), torch.full((P, F), -0.5)]
    layer.set_states(given)
    assert torch.equal(layer.h, given[0]) and torch.equal(layer.c, given[1]) and layer.h.data_ptr() != given[0].data_ptr()
    # reset_envs: the listed environments' rows, nothing else; NaN goes too
    layer.h[0, 0] = float("nan")
    layer.reset_envs(torch.tensor([1, 0, 1], dtype=torch.uint8))
    assert not layer.h[:A].any() and not layer.c[4:].any() and bool((layer.h[A:2 * A] == 0.25).all()) and bool((layer.c[A:2 * A] == -0.5).all())
    # reset zeroes every environment whatever reset_indices says (models.py:40-55), in place in the module's two tensors
    layer.set_states(given)
    layer.reset(torch.tensor([True, False, False]))
    assert not layer.h.any() and not layer.c.any()
    first = (layer.h.data_ptr(), layer.c.data_ptr())
    with torch.no_grad():
        layer(x)
    layer.reset()
    assert (layer.h.data_ptr(), layer.c.data_ptr()) == first and not layer.h.any() and not layer.c.any()
    # set_state: c = transformer(locInits), as the reference (models.py:68-72)
    loc = torch.randn(P, 6)
    layer.set_state(loc)
    assert torch.equal(layer.c, torch.tanh(loc @ layer.LSTM.transformer[0].weight.T + layer.LSTM.transformer[0].bias)) and layer.f is layer.c
    # .double() takes the state along, as the reference's _apply does
    layer.double()
    assert layer.h.dtype == layer.c.dtype == torch.float64


def test_cpu_calls_report_a_fallback(monkeypatch):
    import torch
    from dynenv_amd import GpuRecurrentHead
    layer = GpuRecurrentHead(64, 2, 2, 4).requires_grad_(False)
    out = layer(torch.zeros(4, 64), torch.zeros(4, 4))
    assert layer.last_route.startswith("torch (fallback: features that are not on the device") and tuple(out.shape) == (4, 64)
    monkeypatch.setenv("DYNENV_RHEAD_FUSED", "0")
    layer(torch.zeros(4, 64))
    assert layer.last_route == "torch (fallback: DYNENV_RHEAD_FUSED=0)"
    monkeypatch.delenv("DYNENV_RHEAD_FUSED")
    other = GpuRecurrentHead(32, 2, 2).requires_grad_(False)
    other(torch.zeros(4, 32))
    assert other.last_route.startswith("torch (fallback: F = 32")
    wide = GpuRecurrentHead(64, 2, 2, 33).requires_grad_(False)
    wide(torch.zeros(4, 64), torch.zeros(4, 33))
    assert wide.last_route.startswith("torch (fallback: X = 33")
    layer.requires_grad_(True)
    layer(torch.zeros(4, 64))
    assert layer.last_route == "torch"
    with torch.no_grad():
        layer(torch.zeros(4, 64))
    assert layer.last_route.startswith("torch (fallback: ")


def _reference_classes():
    """the reference's classes as its own file defines them, compiled from it (the package around it needs gym and pymunk)"""
    import torch
    names = {"LSTMLayer", "EmbedBlock", "Indexer", "InOutArranger", "InputLayer", "RecurrentTemporalAttention", "DynEnvFeatureExtractor"}
    tree = ast.parse(open(REF_MODELS).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    ns = dict(torch=torch, nn=torch.nn, np=np, F=torch.nn.functional, List=List, itertools=itertools)
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_MODELS, "exec"), ns)
    return ns


@pytest.mark.skipif(not os.path.exists(REF_MODELS), reason="the reference is not on this machine")
@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
def test_torch_route_is_the_reference_tail_bit_for_bit(shape):
    import torch
    from dynenv_amd import GpuRecurrentHead
    E, A, F, X = shape
    feats, exts, _ = _inputs(*shape, seed=3)
    torch.manual_seed(E)
    ref = _reference_classes()["DynEnvFeatureExtractor"]([5, 3], F, E, 1, A, 2, 2, extended_feature_cnt=X)
    tail = {k: v for k, v in ref.state_dict().items() if not k.startswith(("InNet.", "AttNet."))}
    assert tuple(tail) == RR.NAMES
    RR.load(ref, dict(ref.state_dict(), **{k: torch.from_numpy(v) for k, v in RR.make_params(F, X, seed=A).items()}))
    ref = ref.double()
    ours = GpuRecurrentHead(F, A, E, X).double()
    ours.load_state_dict({k: v for k, v in ref.state_dict().items() if k in tail}, strict=True)
    assert tuple(ref.LSTM.h.shape) == tuple(ours.h.shape) and ref.LSTM.h.dtype == ours.h.dtype == torch.float64

    def ref_tail(f, pos):   # models.py:610-616
        if pos is not None:
            f = ref.TransformNet(torch.cat((f, pos), dim=1))
        return ref.bn(ref.LSTM(f))
    for s in range(3):
        f = torch.from_numpy(feats[s])
        pos = None if exts[s] is None else torch.from_numpy(exts[s])
        with torch.no_grad():
            want = ref_tail(f, pos)
            got = ours(f, pos)
        assert torch.equal(got, want) and torch.equal(ours.h, ref.LSTM.h) and torch.equal(ours.c, ref.LSTM.c), s
    got = ours(f, pos)   # the differentiable call
    with torch.no_grad():
        want = ref_tail(f, pos)
    assert ours.last_route == "torch" and torch.equal(got.detach(), want)
    ours.detach()
    ref.detach()
    a, b = ours.get_states(), ref.LSTM.get_states()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ours.reset(torch.tensor([True] + [False] * (E - 1)))
    ref.reset(torch.tensor([True] + [False] * (E - 1)))
    assert torch.equal(ours.h, ref.LSTM.h.double()) and torch.equal(ours.c, ref.LSTM.c.double()) and not ours.h.any()


def test_the_golden_state_dict_names_hold_the_head_and_are_the_references():
    """tests/golden/feature_extractor_state_dict.json: the names and shapes of DynEnvFeatureExtractor([5, 3], 64, 2, 1, 3, 2, 2,
    extended_feature_cnt=6).state_dict(), which test_gpu_recurrent.py loads into GpuFeatureExtractor strict=True"""
    import torch  # noqa: F401
    from dynenv_amd import GpuRecurrentHead
    gold = json.load(open(GOLDEN))
    entries = [(k, tuple(s)) for k, s in gold["state_dict"]]
    F, X = gold["feature_size"], gold["extended_feature_cnt"]
    head = GpuRecurrentHead(F, gold["num_players"], gold["num_envs"], X)
    tail = [(k, s) for k, s in entries if not k.startswith(("InNet.", "AttNet."))]
    assert tail == [(k, tuple(v.shape)) for k, v in head.state_dict().items()]
    from dynenv_amd import GpuTemporalAttention
    att = [(k[len("AttNet."):], s) for k, s in entries if k.startswith("AttNet.")]
    assert att == [(k, tuple(v.shape)) for k, v in GpuTemporalAttention(F).state_dict().items()]
    if os.path.exists(REF_MODELS):
        ref = _reference_classes()["DynEnvFeatureExtractor"](gold["features_per_object_type"], F, gold["num_envs"], 1, gold["num_players"],
                                                               len(gold["features_per_object_type"]), gold["num_time"], extended_feature_cnt=X)
        assert entries == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
