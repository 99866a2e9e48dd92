"""tests/arranger_embed_ref.py - the numpy float64 statement the GPU tests of the fused embed-and-pad compare against - held to a torch
float64 twin on the CPU, to arranger_ref / arranger_fixed_ref for the placement, and, where the reference is on this machine, to its own
EmbedBlock (DynEnv/models/models.py:99-124) and to an InputLayer.state_dict() (:278-307) loaded with strict=True into our blocks.  No GPU."""
import ast
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arranger_embed_ref as ER  # noqa: E402
import arranger_fixed_ref as FR  # noqa: E402
import arranger_ref as R  # noqa: E402

REF_MODELS = "/root/reference/DynEnv/models/models.py"
SPECS = [(7, 3, R.COUNT_CONST, 2, 2), (4, 2, R.COUNT_ENV, -1, 3), (2, 4, R.COUNT_ROW, -1, 6)]


def _twin(feat, F, p, dtype):
    """our EmbedBlock (the reference's architecture and names) holding the six arrays of p"""
    import torch
    from dynenv_amd.arranger import EmbedBlock
    b = EmbedBlock(feat, F).to(dtype)
    b.load_state_dict({k: torch.from_numpy(np.asarray(a)).to(dtype) for k, a in zip(ER.PARAMS, p)}, strict=True)
    return b


@pytest.mark.parametrize("F", [64, 128, 16])
def test_block_is_torch_in_float64(F):
    import torch
    rng = np.random.default_rng(F)
    for feat, p in zip((1, 4, 9, 16), ER.make_params(rng, (1, 4, 9, 16), F)):
        x = rng.uniform(-1, 1, (37, feat))
        with torch.no_grad():
            want = _twin(feat, F, p, torch.float64)(torch.from_numpy(x)).numpy()
        got = ER.block(x, p)
        assert got.dtype == np.float64 and got.shape == (37, F)
        assert np.abs(got - want).max() < 1e-12
        # float32 torch is a few ulp from it: the order of magnitude the GPU tests' bound is about
        with torch.no_grad():
            f32 = _twin(feat, F, p, torch.float32)(torch.from_numpy(x.astype(np.float32))).numpy()
        assert np.abs(f32 - ER.block(x.astype(np.float32), p)).max() < 2e-5


def test_block_names_and_shapes_are_the_reference_architecture():
    from dynenv_amd.arranger import EmbedBlock
    b = EmbedBlock(5, 64)
    assert [k for k, _ in b.named_parameters()] == list(ER.PARAMS)
    assert [tuple(v.shape) for v in b.parameters()] == [(32, 5), (32,), (32,), (64, 32), (64,), (64,)]
    assert b.relu.negative_slope == 0.1 and b.bn1.eps == b.bn2.eps == 1e-5 and not list(b.buffers())


def test_padded_builder_places_rows_like_the_arranger_references():
    """with every block output replaced by a tag of its row, the builder's tensor is arranger_ref.pad / arranger_fixed_ref.pad of the
    float32 path: same slots, zeros elsewhere; M above the batch's maximum adds zero slots, M below it drops the same objects"""
    rng = np.random.default_rng(3)
    obs, types, ce = R.make_dense(rng, 3, 2, 2, SPECS, lead=1, trail=2)
    F = 64
    params = ER.make_params(rng, [t.feat for t in types], F)
    pl = R.plan(obs, types, ce)
    inputs, slots, _ = R.gather(obs, types, pl)
    M = pl["max_count"]
    want = R.pad([ER.block(x, p).astype(np.float32) for x, p in zip(inputs, params)], slots, 2, M, 6, F)
    got, _ = ER.padded_default(obs, types, params, F, ce)
    assert got.shape == (2, M, 6, F) and np.array_equal(got.astype(np.float32), want)
    assert (got[np.arange(M)[None, :, None] >= pl["obj_counts"][:, None, :]] == 0).all() and (pl["obj_counts"] < M).any()
    more, _ = ER.padded_default(obs, types, params, F, ce, M=M + 3)
    assert np.array_equal(more[:, :M], got) and not more[:, M:].any()
    rows = [2, 2, 3]
    for Mf in (M + 2, M - 2):
        fp = FR.plan(obs, types, rows, Mf, ce)
        fin, _ = FR.gather(obs, types, rows, Mf, fp)
        wantf = FR.pad([ER.block(x, p).astype(np.float32) for x, p in zip(fin, params)], rows, Mf, fp, F)
        gotf, pl2 = ER.padded_fixed(obs, types, rows, Mf, params, F, ce)
        assert np.array_equal(gotf.astype(np.float32), wantf) and np.array_equal(pl2["dropped"], fp["dropped"])
        assert fp["dropped"].any()
    less, _ = ER.padded_default(obs, types, params, F, ce, M=M - 2)   # the default counts clamped to the slots left: rows = caps
    assert np.array_equal(less, ER.padded_fixed(obs, types, [t.cap for t in types], M - 2, params, F, ce)[0])
    none = ER.padded_default(obs, types, [params[0], None, params[2]], F, ce)[0]
    assert (none != got).any() and not none[none != got].any()


def _reference_classes():
    """EmbedBlock and InputLayer as the reference defines them, compiled from its own file (the package around them needs gym and pymunk)"""
    import itertools
    from typing import List
    import torch
    tree = ast.parse(open(REF_MODELS).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("ObsMask", "Indexer", "EmbedBlock", "InOutArranger", "InputLayer")]
    ns = dict(torch=torch, nn=torch.nn, np=np, F=torch.nn.functional, itertools=itertools, List=List)
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_MODELS, "exec"), ns)
    return ns["EmbedBlock"], ns["InputLayer"]


@pytest.mark.skipif(not os.path.exists(REF_MODELS), reason="the reference is not on this machine")
def test_against_the_reference_embed_block_and_state_dict():
    import torch
    from dynenv_amd.arranger import EmbedBlock
    RefBlock, RefLayer = _reference_classes()
    torch.manual_seed(5)
    rng = np.random.default_rng(5)
    feats, F = [7, 4, 2], 64
    ref = RefLayer(feats, F, nEnvs=3, nPlayers=2, nObjectTypes=3, nTime=2)
    for b in ref.blocks:   # (LayerNorm starts at weight 1, bias 0: move them)
        for ln in (b.bn1, b.bn2):
            ln.weight.data.uniform_(0.5, 1.5)
            ln.bias.data.uniform_(-0.5, 0.5)
    ours = torch.nn.Module()
    ours.blocks = torch.nn.ModuleList([EmbedBlock(f, F) for f in feats])
    ours.load_state_dict(ref.state_dict(), strict=True)
    assert sorted(ours.state_dict()) == sorted(ref.state_dict())
    for f, rb, ob in zip(feats, ref.blocks, ours.blocks):
        x = rng.uniform(-1, 1, (29, f)).astype(np.float32)
        with torch.no_grad():
            want = rb(torch.from_numpy(x))
            assert torch.equal(ob(torch.from_numpy(x)), want)
        p = [rb.state_dict()[k].numpy() for k in ER.PARAMS]
        assert np.abs(ER.block(x, p) - want.numpy()).max() < 2e-5
        assert np.abs(ER.block(x, p) - rb.double()(torch.from_numpy(x).double()).detach().numpy()).max() < 1e-12
