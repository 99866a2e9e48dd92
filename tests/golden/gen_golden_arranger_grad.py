#!/usr/bin/env python3
"""Golden vectors for the BACKWARD of the ragged->padded arranger: what autograd returns through the REFERENCE's own
InOutArranger.rearrange_outputs (/root/reference/DynEnv/models/models.py:250-274: out[range] -> torch.cat -> F.pad ->
torch.stack, catAndPad :147-166).  The ragged inputs come from gen_golden_arranger.make_case, the embeddings are leaf tensors
with requires_grad (None for a type without objects), G is an upstream gradient of `padded`'s shape, and the recorded
gradients are `outs[i].grad` after `padded.backward(G)`.  Numbers only.
Run in the build container only (the reference never ships):  python tests/golden/gen_golden_arranger_grad.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_arranger as ga  # noqa: E402

# the five cases of gen_golden_arranger.py, a RoboCup-shaped one with five time steps, and a width that is no power of two
CASES = {
    "driving_full": dict(E=3, T=1, A=4, feats=(7, 4, 2), max_counts=(3, 6, 5)),
    "driving_partial": dict(E=2, T=1, A=5, feats=(7, 6, 2), max_counts=(6, 8, 9)),
    "robocup": dict(E=2, T=5, A=4, feats=(4, 6), max_counts=(1, 3)),
    "static": dict(E=2, T=1, A=3, feats=(9, 5), max_counts=(1, 8)),
    "empty_type": dict(E=2, T=2, A=3, feats=(7, 4, 2), max_counts=(2, 3, 4), allow_empty_type=True),
    "robocup_t5": dict(E=3, T=5, A=5, feats=(4, 4, 6, 3), max_counts=(1, 4, 2, 5)),
    "width12": dict(E=3, T=2, A=3, feats=(7, 4, 2), max_counts=(5, 2, 3)),
}
WIDTH = {"width12": 12}   # embedding width F per case (default 8)


def generate():
    """-> {key: array}, what arranger_grad.npz holds"""
    import torch
    mm = ga.ref_arranger_module()
    rng = np.random.default_rng(11)
    out = {}
    for name, kw in CASES.items():
        x = ga.make_case(rng, **kw)
        E, T, A, nT, F = kw["E"], kw["T"], kw["A"], len(kw["feats"]), WIDTH.get(name, 8)
        arr = mm.InOutArranger(nT, E * A, T)
        inputs, (counts, maxCount, objCounts) = arr.rearrange_inputs(x)
        embs = [torch.tensor(rng.standard_normal((len(inp), F)).astype(np.float32), requires_grad=True) if len(inp) else None
                for inp in inputs]
        padded, _ = arr.rearrange_outputs(embs, (counts, maxCount, objCounts), "cpu")
        assert padded.grad_fn is not None and tuple(padded.shape) == (T, maxCount, E * A, F)
        G = torch.tensor(rng.standard_normal(tuple(padded.shape)).astype(np.float32))
        padded.backward(G)
        out[name + "/shape"] = np.array([E, T, A, nT, F], np.int64)
        out[name + "/counts"] = np.array(counts, np.int64)          # [type, T, P]
        out[name + "/maxCount"] = np.array(maxCount, np.int64)
        out[name + "/has_emb"] = np.array([e is not None for e in embs], np.bool_)   # False: the reference was given None
        for i, e in enumerate(embs):
            out["%s/emb%d" % (name, i)] = e.detach().numpy() if e is not None else np.zeros((0, F), np.float32)
            out["%s/grad%d" % (name, i)] = e.grad.numpy() if e is not None else np.zeros((0, F), np.float32)
        out[name + "/G"] = G.numpy()
        out[name + "/padded"] = padded.detach().numpy()
    return out


def main():
    out = generate()
    np.savez_compressed(os.path.join(HERE, "arranger_grad.npz"), **out)
    print("wrote arranger_grad.npz:", {k: v.shape for k, v in out.items() if k.endswith("/padded")})


if __name__ == "__main__":
    main()
