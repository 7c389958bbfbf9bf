"""
What the surface-surface tests share: the goldens of tests/golden/surfaces.npz as splines, byte comparison of two
``trace_pair`` results, a Lipschitz bound of a surface and a host evaluation of a fitted curve.
"""
import os

import numpy as np

import bspy_amd
from bspy_amd import surfaces
from conftest import GOLDEN

GOLD = np.load(os.path.join(GOLDEN, "surfaces.npz"))
NAMES = sorted({key.split("/")[0] for key in GOLD.files})
PER_PAIR = ("pair_seg", "pair_cell", "roots", "near", "count", "status", "nodes", "keep")


def load_case(name):
    c = {key.split("/", 1)[1]: GOLD[key] for key in GOLD.files if key.startswith(name + "/")}
    c["name"], c["depth"], c["kind"] = name, int(c["depth"]), str(c["kind"])
    return c


def make(c, scale=1.0):
    out = []
    for side in "ab":
        coefs = c[side + "_coefs"]
        out.append(bspy_amd.Spline(2, 3, [int(k) for k in c[side + "_order"]], list(coefs.shape[1:]), [c[side + "_knots0"], c[side + "_knots1"]],
                                   coefs * coefs.dtype.type(scale)))
    return out


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def same_result(r, s):
    return (same(r[0], s[0]) and same(r[1], s[1]) and same(r[2], s[2]) and same(r[3].segments, s[3].segments) and same(r[3].leaves, s[3].leaves)
            and all(same(r[4]["families"][f][k], s[4]["families"][f][k]) for f in range(4) for k in PER_PAIR))


def lipschitz(s):
    """A bound on |ds/du| + |ds/dv| of a surface: the control net's differences per unit of the parameter."""
    plan, rows, _ = surfaces.host_tables(s)
    total = 0.0
    for ax in range(2):
        K = plan.order[ax]
        h = float(np.diff(np.asarray(plan.breaks[ax], np.float64)).min())
        total += (K - 1) * float(np.sqrt((np.diff(rows, axis=ax + 1) ** 2).sum(axis=0)).max()) / h
    return total


def curve_at(curve, t):
    """A fitted curve (nInd 1, nDep 2) at t, by de Boor on the host."""
    k, knots, coefs = int(curve.order[0]), np.asarray(curve.knots[0], np.float64), np.asarray(curve.coefs, np.float64)
    n = len(knots) - k
    span = np.clip(np.searchsorted(knots, t, "right") - 1, k - 1, n - 1)
    out = np.zeros((2, len(t)))
    for j, (x, mu) in enumerate(zip(t, span)):
        d = [coefs[:, mu - k + 1 + r].copy() for r in range(k)]
        for r in range(1, k):
            for i in range(k - 1, r - 1, -1):
                lo, hi = knots[mu - k + 1 + i], knots[mu + 1 + i - r]
                alpha = (x - lo) / (hi - lo)
                d[i] = (1.0 - alpha) * d[i - 1] + alpha * d[i]
        out[:, j] = d[k - 1]
    return out
