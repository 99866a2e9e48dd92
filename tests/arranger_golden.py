"""The reference's recorded arranger vectors (tests/golden/arranger.npz) and the ragged input they were computed from, for the oracle's
and the GPU arranger's tests.  A helper module: no test in here."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G = np.load(os.path.join(ROOT, "tests", "golden", "arranger.npz"))
CASES = sorted({k.split("/")[0] for k in G.files})


def ragged_from_golden(name):
    E, T, A, nT = (int(v) for v in G[name + "/shape"])
    cnt = G[name + "/x_counts"]
    pos = [0] * nT
    x = []
    for e in range(E):
        env = []
        for t in range(T):
            players = []
            for a in range(A):
                s = []
                for i in range(nT):
                    c = int(cnt[e, t, a, i])
                    rows = G["%s/x_rows%d" % (name, i)]
                    s.append(rows[pos[i]:pos[i] + c])
                    pos[i] += c
                players.append(s)
            env.append(players)
        x.append(env)
    return x, (E, T, A, nT)
