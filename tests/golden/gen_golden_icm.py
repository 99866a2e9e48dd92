#!/usr/bin/env python3
"""Golden results of the REFERENCE's own ICMNet (DynEnv/models/icm.py: forward :53-75, _calc_loss :77-109) on CPU float32 at the tiny
cases of icm_ref.GOLDEN_CASES - T = 3, P = 6, K = 16, groups (3, 3) and (5, 3, 3); masks random, all finished, exactly one active and
nobody finished; loss_attn on and off - kept small because the reference's one-hot is a Python loop.  The class is compiled out of its
file with ast (tests/icm_ref.py, reference_classes: the package around it does not import); the outputs are what it returned.
Run where the reference is (DYNENV_REFERENCE; it never ships):  python tests/golden/gen_golden_icm.py
Writes tests/golden/icm.json: a list of cases {T, P, K, groups, mask, loss_attn, seed, forward_coeff, icm_beta, long_horizon_coeff, n,
forward, inverse, long_horizon_forward, loss, inputs}; the parameters and the case are icm_ref.golden_inputs(case), checked by "inputs",
their float32 words.  Every float32 is kept as its 32-bit word, so the file holds them exactly.  Data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import icm_ref as IR  # noqa: E402


def input_words(pr, case):
    return dict(features=IR.bits(case["features"]), actions=IR.bits(case["actions"]), finished=case["finished"].reshape(-1).astype(int).tolist(),
                params_head={k: IR.bits(v.reshape(-1)[:4]) for k, v in pr.items()})   # (the first four words of every parameter)


def main():
    ns = IR.reference_classes()
    out = []
    for c in IR.GOLDEN_CASES:
        pr, case = IR.golden_inputs(c)
        net = IR.reference_net(ns, c["K"], c["groups"], c["T"], c["P"], pr, loss_attn=c["loss_attn"], dtype=torch.float32, **IR.GOLDEN_COEFFS)
        with torch.no_grad():
            got = net(torch.from_numpy(case["features"]), torch.from_numpy(case["actions"]), torch.from_numpy(case["finished"]))
        f32 = lambda x: IR.bits(np.float32(x.detach().reshape(-1)[0].item()))[0]   # noqa: E731
        out.append(dict(c, groups=list(c["groups"]), n=int((~case["finished"]).sum()), forward=f32(got.forward), inverse=f32(got.inverse),
                        long_horizon_forward=f32(got.long_horizon_forward), loss=f32(got.loss), inputs=input_words(pr, case), **IR.GOLDEN_COEFFS))
    with open(IR.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", IR.GOLDEN, len(out), "cases,", os.path.getsize(IR.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
