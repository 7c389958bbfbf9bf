"""
The data of tests/test_robust_host.py and tests/test_gpu_robust.py: points evaluated from a known spline on dyadic parameters
(dyadic knots, small dyadic coefficients; a point is the statement's basis times the coefficients in doubles), m of them displaced grossly, m under a
quarter of every cell's points.

    curve     order 4, 11 coefficients, 8 cells of width 1/8, 16 points a cell (128), 3 displaced a cell; nDep 2
    surface   6 x 5 bicubic, knots 0, 1/4, 1/2, 1 and 0, 1/2, 1: 3 x 2 cells, 6 x 6 points a cell (216), 8 displaced a cell; nDep 1

``clean(case)`` is the record of tests/scatter_ref.py for the clean subset: the exact coefficients of its least-squares fit
rounded once and the family's bar c eps |N^-1| (Nbar |c| + A^T W |p|), computed once and shared.
"""
import functools

import numpy as np

import scatter_ref
from bspy_amd import scatter


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64).tolist() if a.dtype == np.float64 else a.tolist()


def evaluate(order, knots, coefs, uvw):
    """(nDep, N) of the statement's basis: plain floats."""
    out = np.zeros((coefs.shape[0], uvw.shape[1]))
    for i in range(uvw.shape[1]):
        mus = [scatter.find_span(list(t), k - 1, scatter.top_span(k, t), float(u)) for k, t, u in zip(order, knots, uvw[:, i])]
        B = np.array(scatter.basis(order[0], list(knots[0]), mus[0], float(uvw[0, i])))
        window = coefs[:, mus[0] - order[0] + 1:mus[0] + 1]
        if len(order) == 2:
            Bv = np.array(scatter.basis(order[1], list(knots[1]), mus[1], float(uvw[1, i])))
            out[:, i] = np.einsum("a,b,dab->d", B, Bv, window[:, :, mus[1] - order[1] + 1:mus[1] + 1])
        else:
            out[:, i] = window @ B
    return out


def _curve():
    order = (4,)
    knots = [np.concatenate((np.zeros(3), np.arange(9) / 8.0, np.ones(3)))]
    rng = np.random.default_rng(11)
    coefs = rng.integers(-16, 17, (2, 11)) / 4.0
    u = np.array([(c + (2 * q + 1) / 32.0) / 8.0 for c in range(8) for q in range(16)])
    out = np.zeros(128, bool)
    for c in range(8):
        out[16 * c + rng.choice(16, 3, replace=False)] = True
    return order, knots, coefs, u.reshape(1, -1), out, rng


def _surface():
    order = (4, 4)
    knots = [np.array([0, 0, 0, 0, 0.25, 0.5, 1, 1, 1, 1.0]), np.array([0, 0, 0, 0, 0.5, 1, 1, 1, 1.0])]
    rng = np.random.default_rng(12)
    coefs = rng.integers(-16, 17, (1, 6, 5)) / 4.0
    uv, out = [], []
    for c0 in range(3):
        for c1 in range(2):
            lo0, hi0, lo1, hi1 = knots[0][3 + c0], knots[0][4 + c0], knots[1][3 + c1], knots[1][4 + c1]
            uv += [(lo0 + (hi0 - lo0) * (2 * a + 1) / 16.0, lo1 + (hi1 - lo1) * (2 * b + 1) / 16.0) for a in range(6) for b in range(6)]
            mark = np.zeros(36, bool)
            mark[rng.choice(36, 8, replace=False)] = True
            out += list(mark)
    return order, knots, coefs, np.array(uv).T.copy(), np.array(out), rng


@functools.lru_cache(maxsize=None)
def case(name):
    order, knots, coefs, uvw, out, rng = _curve() if name == "curve" else _surface()
    points = evaluate(order, knots, coefs, uvw)
    shift = rng.choice([-1.0, 1.0], (points.shape[0], int(out.sum()))) * rng.integers(64, 257, (points.shape[0], int(out.sum())))
    points[:, out] += shift
    return dict(order=order, knots=knots, coefs=coefs, uvw=np.ascontiguousarray(uvw), points=np.ascontiguousarray(points), displaced=out)


@functools.lru_cache(maxsize=None)
def clean(name):
    c = case(name)
    keep = ~c["displaced"]
    exact, bar, count = scatter_ref.record(dict(order=c["order"], knots=c["knots"], uvw=c["uvw"][:, keep], points=c["points"][:, keep],
                                                weights=None, smoothing=0.0, penalty=None))
    return exact, bar


def fit(name, **more):
    c = case(name)
    return scatter.fit_batch(c["uvw"], c["points"], c["order"], c["knots"], **more)
