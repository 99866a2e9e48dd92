#!/usr/bin/env python3
"""Golden results of the REFERENCE's own transformActions (/root/reference/DynEnv/utils/utils.py:20-39) for every action tuple of the
two environments: the 9 Driving tuples ([3, 3]) and the 315 RoboCup tuples ([5, 3, 3, 7]), each with discreteTurn False and True.  The
function is compiled out of its file (the module around it imports plotting packages); the outputs are what it returned.
Run in the build container only (the reference never ships):  python tests/golden/gen_golden_transform_actions.py
Writes tests/golden/transform_actions.json: {"driving" | "robocup": {"nvec", "actions", "false", "true"}}."""
import ast
import itertools
import json
import os

import torch

REF_UTILS = "/root/reference/DynEnv/utils/utils.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "transform_actions.json")


def reference_function():
    tree = ast.parse(open(REF_UTILS).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "transformActions"]
    ns = dict(torch=torch)
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_UTILS, "exec"), ns)
    return ns["transformActions"]


def main():
    fn = reference_function()
    out = {}
    for name, nvec in (("driving", [3, 3]), ("robocup", [5, 3, 3, 7])):
        actions = torch.tensor(list(itertools.product(*[range(n) for n in nvec])), dtype=torch.int64)
        out[name] = {"nvec": nvec, "actions": actions.tolist(), "false": fn(actions, False).tolist(), "true": fn(actions, True).tolist()}
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, {k: len(v["actions"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
