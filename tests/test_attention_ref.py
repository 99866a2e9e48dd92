"""tests/attention_ref.py - the numpy float64 statement the GPU tests of the fused attention compare against - held to the torch route of
GpuTemporalAttention in float64 on the CPU, and, where the reference is on this machine, that route to the reference's own
RecurrentTemporalAttention (DynEnv/models/models.py:311-386) bit for bit, with its state_dict() loaded strict=True.  No GPU."""
import ast
import contextlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as AR  # noqa: E402

REF_MODELS = "/root/reference/DynEnv/models/models.py"
SHAPES = [(1, 20, 9, 64), (3, 10, 12, 64), (5, 7, 11, 128), (2, 1, 7, 64)]   # (T, M, P, F)


def _inputs(T, M, P, F, seed=0):
    import torch
    rng = np.random.default_rng(seed + T + M)
    counts = AR.make_counts(T, M, P)
    padded = rng.standard_normal((T, M, P, F))
    padded[np.transpose(AR.masks_of(counts, M), (0, 2, 1))] = 0.0   # (the arranger's padding)
    masks = [torch.from_numpy(m) for m in AR.masks_of(counts, M)]
    return counts, padded, masks


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_statement_is_the_torch_route_in_float64(shape):
    import torch
    from dynenv_amd import GpuTemporalAttention
    T, M, P, F = shape
    counts, padded, masks = _inputs(*shape)
    pr = AR.make_params(F, seed=T)
    layer = AR.load(GpuTemporalAttention(F), pr, torch.float64)
    with torch.no_grad():
        want = layer((torch.from_numpy(padded), masks)).numpy()
    assert layer.last_route.startswith("torch (fallback: ")
    got = AR.attend_pool(padded, counts, pr)
    assert got.shape == want.shape == (P, F) and got.dtype == np.float64
    assert (counts.max(0) == 0).any() and not got[counts.max(0) == 0].any(), "a player without objects"
    assert np.abs(got - want).max() < 1e-12
    # the statement never looks behind a count
    junk = padded.copy()
    junk[np.transpose(AR.masks_of(counts, M), (0, 2, 1))] = np.nan
    assert np.array_equal(AR.attend_pool(junk, counts, pr), got)
    # gradients wanted: the same values through the differentiable route
    out = layer((torch.from_numpy(padded), masks))
    assert layer.last_route == "torch" and out.grad_fn is not None and np.array_equal(out.detach().numpy(), want)


def test_names_and_shapes_are_the_reference_architecture():
    from dynenv_amd import GpuTemporalAttention
    import dynenv_amd
    assert "GpuTemporalAttention" in dynenv_amd.__all__
    F = 64
    layer = GpuTemporalAttention(F)
    assert layer.last_route is None and not list(layer.buffers())
    assert tuple(k for k, _ in layer.named_parameters()) == AR.NAMES
    shapes = {"in_proj_weight": (3 * F, F), "in_proj_bias": (3 * F,), "bias_k": (1, 1, F), "bias_v": (1, 1, F), "out_proj.weight": (F, F),
              "out_proj.bias": (F,)}
    want = {"%s.%s" % (a, k): s for a in ("objAtt", "tempAtt") for k, s in shapes.items()}
    want.update({"bn.weight": (F,), "bn.bias": (F,), "confLayer.0.weight": (1, F), "confLayer.0.bias": (1,)})
    assert {k: tuple(v.shape) for k, v in layer.named_parameters()} == want
    assert layer.bn.eps == AR.EPS and layer.objAtt.num_heads == layer.tempAtt.num_heads == 1
    pr = AR.make_params(F)
    assert tuple(pr) == AR.NAMES and all(np.abs(v).max() > 0.1 for k, v in pr.items() if "bias" in k)


def _reference_class():
    """RecurrentTemporalAttention as the reference defines it, compiled from its own file (the package around it needs gym and pymunk)"""
    import torch
    tree = ast.parse(open(REF_MODELS).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "RecurrentTemporalAttention"]
    ns = dict(torch=torch, nn=torch.nn, np=np, F=torch.nn.functional)
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_MODELS, "exec"), ns)
    return ns["RecurrentTemporalAttention"]


@pytest.mark.skipif(not os.path.exists(REF_MODELS), reason="the reference is not on this machine")
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_torch_route_is_the_reference_class_bit_for_bit(shape):
    import torch
    from dynenv_amd import GpuTemporalAttention
    T, M, P, F = shape
    counts, padded, masks = _inputs(*shape, seed=3)
    torch.manual_seed(T)
    ref = AR.load(_reference_class()(F), AR.make_params(F, seed=M)).double()
    ours = GpuTemporalAttention(F).double()
    ours.load_state_dict(ref.state_dict(), strict=True)
    assert sorted(ours.state_dict()) == sorted(ref.state_dict())
    x = torch.from_numpy(padded)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()) as said:
        want = ref((x.clone(), masks))
    assert said.getvalue() == "", "finite inputs: the reference's NaN prints stay silent"
    with torch.no_grad():
        got = ours((x, masks))
    assert got.dtype == want.dtype == torch.float64 and torch.equal(got, want)
    got2 = ours((x, masks))   # the differentiable call
    assert ours.last_route == "torch" and torch.equal(got2.detach(), want)
