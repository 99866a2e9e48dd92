#!/usr/bin/env python3
"""Golden results of the REFERENCE's own RolloutStorage (/root/reference/DynEnv/models/storage.py): _discount_rewards (:168-209) and
a2c_loss (:211-290) after its own insert (:134-166) of every step, on CPU float32 - A2C and PPO, batch and full entropy, at T = 5, E = 3,
A = 2 with groups (3, 3), and at T = 1.  The class is compiled out of its file with ast (tests/rollout_ref.py, reference_class: the
package around it does not import); the outputs are what it returned.
Run in the build container only (the reference never ships):  python tests/golden/gen_golden_rollout_storage.py
Writes tests/golden/rollout_storage.json: a list of cases {T, E, A, groups, F, seed, use_ppo, use_full_entropy, value_coeff, entropy_coeff,
returns, loss, policy, value, entropy, temp_entropy}; the inputs are rollout_ref.golden_case(T, E, A, groups, F, seed), checked by
"inputs", their float32 words.  Every float32 is kept as its 32-bit word, so the file holds them exactly.  Data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rollout_ref as RR  # noqa: E402

CASES = [(T, use_ppo, full) for T in (5, 1) for use_ppo in (False, True) for full in (False, True)]
E, A, GROUPS, F = 3, 2, (3, 3), 8
VALUE_COEFF, ENTROPY_COEFF = 0.5, 0.1


def input_words(steps, final_value):
    keys = ("rewards", "feat0", "log_probs", "log_probs_old", "value", "probs")
    return {"final_value": RR.bits(final_value), "steps": [dict({k: RR.bits(s[k]) for k in keys}, finished=s["finished"].reshape(-1).tolist(),
                                                                actions=s["actions"].reshape(-1).tolist(), dones=s["dones"].tolist()) for s in steps]}


def main():
    cls = RR.reference_class()
    out = []
    for i, (T, use_ppo, full) in enumerate(CASES):
        seed = 100 + i
        steps, final_value = RR.golden_case(T, E, A, GROUPS, F, seed)
        st, action_probs = RR.reference_filled(cls, steps, E, A, GROUPS, F, use_ppo, full)
        final = torch.from_numpy(final_value).view(-1, 1)
        returns = st._discount_rewards(final)
        losses, rewards = st.a2c_loss(final, action_probs, VALUE_COEFF, ENTROPY_COEFF)
        f32 = lambda x: RR.bits(np.float32(x))[0]
        out.append(dict(T=T, E=E, A=A, groups=list(GROUPS), F=F, seed=seed, use_ppo=use_ppo, use_full_entropy=full, value_coeff=VALUE_COEFF,
                        entropy_coeff=ENTROPY_COEFF, inputs=input_words(steps, final_value), returns=RR.bits(returns.numpy()),
                        stored_rewards=RR.bits(rewards.numpy()), loss=f32(losses.loss.item()), policy=f32(losses.policy), value=f32(losses.value),
                        entropy=f32(losses.entropy), temp_entropy=f32(losses.temp_entropy)))
    with open(RR.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", RR.GOLDEN, len(out), "cases,", os.path.getsize(RR.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
