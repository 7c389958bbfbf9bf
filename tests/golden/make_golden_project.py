"""
Writes tests/golden/project.npz: small curves and surfaces, query points and, from the exact oracle tests/project_ref.py,
the certified global minimiser of every point.  Run on the CPU from the repository root:

    python tests/golden/make_golden_project.py

A query point is recorded when (1) its global minimiser is certified unique with a relative gap of the squared distance
to the runner-up above MARGIN, (2) the minimiser is a critical point inside a knot cell or sits on a domain bound (not on
an interior knot line), and (3) the Python statement of bspy_amd/project.py, run on the host tables, lands within BASIN
of the domain width of it.  A point that fails a condition, or on which the oracle raises ArithmeticError, is replaced by
the next one the generator draws: the tests use every recorded point.
Per case and point: u (the centre of the certified box), radius (its half width), the enclosure [dist_lo, dist_hi] of the
exact distance, and what the tests' error bar needs from the exact derivatives at the minimiser: hinv (the row-sum norm
of the inverse of the Hessian of |S - p|^2 / 2 restricted to the free axes; 0 when no axis is free), jmax (the largest
|dS_d / du_a|) and hmin (the smallest width of the minimiser's cell).
"""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import project_ref  # noqa: E402

import bspy_amd  # noqa: E402
from bspy_amd import project  # noqa: E402

MARGIN = 1e-3
BASIN = 1e-6


def knots_of(K, n, interior, lo=0.0, hi=1.0, dtype=np.float64):
    t = np.concatenate([[0.0] * K, interior, [1.0] * K])
    assert len(t) == n + K
    return (lo + (hi - lo) * t).astype(dtype)


def cases(rng):
    """name -> dict(order, knots, coefs, samples, special: extra points to try first)."""
    out = {}

    def curve(name, K, interior, nDep, dtype=np.float64, lo=0.0, hi=1.0, scale=1.0, shift=0.0, samples=None, coefs=None):
        n = K + len(interior)
        t = knots_of(K, n, interior, lo, hi, dtype)
        if coefs is None:
            c = rng.standard_normal((nDep, n)) * 0.5
            c[0] = np.linspace(0.0, 3.0, n) + 0.2 * rng.standard_normal(n)
            coefs = np.round(c * 64) / 64
        out[name] = dict(order=[K], knots=[t], coefs=(np.asarray(coefs) * scale + shift).astype(dtype), samples=samples)

    def surface(name, K, interior, nDep, dtype=np.float64, lo=(0.0, 0.0), hi=(1.0, 1.0), scale=1.0, shift=0.0):
        n = [K[d] + len(interior[d]) for d in range(2)]
        t = [knots_of(K[d], n[d], interior[d], lo[d], hi[d], dtype) for d in range(2)]
        c = np.zeros((nDep, n[0], n[1]))
        c[0] = np.linspace(0.0, 2.0, n[0])[:, None] + 0.1 * rng.standard_normal(n)
        c[1] = np.linspace(0.0, 2.0, n[1])[None, :] + 0.1 * rng.standard_normal(n)
        if nDep == 3:
            c[2] = 0.4 * rng.standard_normal(n)
        out[name] = dict(order=list(K), knots=t, coefs=(np.round(c * 64) / 64 * scale + shift).astype(dtype), samples=None)

    curve("curve_k4_uniform", 4, [0.2, 0.4, 0.6, 0.8], 2)
    curve("curve_k3_nonuniform", 3, [0.1, 0.15, 0.55, 0.9], 3)
    curve("curve_k4_double_knot", 4, [0.3, 0.5, 0.5, 0.8], 2)
    curve("curve_k6", 6, [0.2, 0.35, 0.5, 0.6, 0.7, 0.85], 3)
    curve("curve_k2", 2, [0.4, 0.7], 2)
    curve("curve_k4_float32", 4, [0.25, 0.5, 0.75], 2, dtype=np.float32)
    curve("curve_k3_shifted", 3, [0.3, 0.6], 2, lo=100.0, hi=103.0, scale=1000.0, shift=5000.0)
    # a parabola symmetric about x = 1/2 on one cell, two samples: a point on the axis is equally far from both
    curve("curve_tie", 3, [], 2, samples=2, coefs=[[0.0, 0.5, 1.0], [0.0, 1.0, 0.0]])
    surface("surface_k44_uniform", (4, 4), ([1 / 3, 2 / 3], [1 / 3, 2 / 3]), 3)
    surface("surface_k24_mixed", (2, 4), ([0.5], [0.4, 0.7]), 3)
    surface("surface_k33_planar", (3, 3), ([0.3, 0.8], [0.6]), 2)
    surface("surface_k43_float32", (4, 3), ([0.5], [0.5]), 3, dtype=np.float32)
    surface("surface_k22", (2, 2), ([0.5], []), 3)
    surface("surface_k44_shifted", (4, 4), ([0.5, 0.5], []), 3, lo=(-40.0, 7.0), hi=(-38.0, 7.5), scale=250.0, shift=-3000.0)
    return out


def spline_of(case):
    order, knots, coefs = case["order"], case["knots"], case["coefs"]
    return bspy_amd.Spline(len(order), coefs.shape[0], order, list(coefs.shape[1:]), knots, coefs)


def rounded_out(lo, hi):
    a, b = np.sqrt(float(max(lo, 0))), np.sqrt(float(hi))
    return float(np.nextafter(np.nextafter(a, -np.inf), -np.inf)) if a > 0 else 0.0, float(np.nextafter(np.nextafter(b, np.inf), np.inf))


def record(case, spline, tables, p):
    """None, or the row of one query point."""
    order, knots, coefs = case["order"], case["knots"], case["coefs"]
    try:
        best = project_ref.closest(order, knots, coefs, p)
    except ArithmeticError:
        return None
    if best["gap"] is not None and not best["gap"] > MARGIN * max(best["d"][1] + best["gap"], Fraction(1, 10 ** 30)):
        return None
    if any(f is None for f in best["free"]):
        return None
    plan, rows, grid = tables
    uvw, dist, status, steps = project.statement(plan.tables(rows), grid, np.asarray(p, np.float64)[:, None])
    width = [float(k[-1]) - float(k[0]) for k in knots]
    mid = [float((lo + hi) / 2) for lo, hi in best["u"]]
    if any(abs(float(uvw[a, 0]) - mid[a]) > BASIN * width[a] for a in range(len(order))) or status[0] & 5:
        return None
    S, J, H = project_ref.derivatives_at(order, knots, coefs, best)
    r = [s - Fraction(float(x)) for s, x in zip(S, p)]
    free = [a for a, f in enumerate(best["free"]) if f]
    hess = np.array([[float(sum(J[d][a] * J[d][b] + r[d] * H[d][a][b] for d in range(len(S)))) for b in free] for a in free])
    hinv = float(np.abs(np.linalg.inv(hess)).sum(axis=1).max()) if free else 0.0
    cellw = []
    for a, k in enumerate(knots):
        b = np.unique(np.asarray(k, np.float64))
        cellw.append(float(np.diff(b).min()))
    dist_lo, dist_hi = rounded_out(*best["d"])
    gap = 1.0 if best["gap"] is None else float(best["gap"] / max(best["d"][1] + best["gap"], Fraction(1, 10 ** 30)))
    return dict(u=mid, radius=[float((hi - lo) / 2) * (1 + 2.0 ** -50) for lo, hi in best["u"]], dist_lo=dist_lo, dist_hi=dist_hi,
                gap=gap, hinv=hinv, jmax=max(abs(float(v)) for row in J for v in row), hmin=min(cellw),
                free=[int(bool(f)) for f in best["free"]], steps=int(steps[0]))


def special_points(name, case, spline, rng):
    """Points that must be there: on the spline, foot points on a domain end / edge / corner, the tie."""
    nDep = case["coefs"].shape[0]
    lo = [float(k[0]) for k in case["knots"]]
    hi = [float(k[-1]) for k in case["knots"]]
    out = []

    def at(u, which=0):
        found = project_ref.point(case["order"], case["knots"], case["coefs"], u)
        return np.array([float(v) for v in found[0]]) if which == 0 else np.array([float(row[0]) for row in found[1]])

    if name == "curve_tie":
        return [np.array([0.5, 2.0]), np.array([0.5, 0.75]), np.array([0.5, -1.0])]
    for _ in range(2):                                      # on the spline (rounded to the coefficients' dtype, widened)
        u = [lo[a] + (hi[a] - lo[a]) * rng.uniform(0.05, 0.95) for a in range(len(lo))]
        out.append(at(u))
    span = float(np.abs(case["coefs"]).max())
    if len(lo) == 1:
        for end, u in ((-1.0, lo[0]), (1.0, hi[0])):        # beyond an end of the curve, along its tangent
            tangent = at([u], 1)
            out.append(at([u]) + end * 0.3 * tangent / np.abs(tangent).max() * max(1.0, span * 1e-3))
    else:
        c = case["coefs"].astype(np.float64)
        size = max(1.0, float(np.ptp(c[0])))
        corner = c[:, 0, 0].copy()
        corner[:2] -= 0.4 * size                            # beyond the corner (lo, lo)
        out.append(corner)
        corner = c[:, -1, -1].copy()
        corner[:2] += 0.3 * size
        out.append(corner)
        edge = at([lo[0], lo[1] + 0.45 * (hi[1] - lo[1])])
        edge[0] -= 0.5 * size                               # beyond the edge u = lo
        out.append(edge)
        edge = at([lo[0] + 0.6 * (hi[0] - lo[0]), hi[1]])
        edge[1] += 0.35 * size
        out.append(edge)
    return out


def main():
    rng = np.random.default_rng(20261019)
    store = {}
    names = []
    for name, case in cases(rng).items():
        spline = spline_of(case)
        tables = project.host_tables(spline, case["samples"])
        nDep = case["coefs"].shape[0]
        want = 8 if len(case["order"]) == 1 else 7
        rows = []
        todo = special_points(name, case, spline, rng)
        c = case["coefs"].astype(np.float64).reshape(nDep, -1)
        centre, size = c.mean(axis=1), np.ptp(c, axis=1).max()
        tried = 0
        while len(rows) < want and tried < 60:
            p = todo.pop(0) if todo else centre + size * 0.6 * rng.standard_normal(nDep)
            p = np.asarray(p, np.float64)
            tried += 1
            row = record(case, spline, tables, p)
            print(name, "point", tried, "kept" if row else "replaced", flush=True)
            if row:
                row["p"] = p
                rows.append(row)
        assert len(rows) == want, name
        names.append(name)
        store[name + ".order"] = np.array(case["order"], np.int32)
        for a, k in enumerate(case["knots"]):
            store[f"{name}.knots{a}"] = k
        store[name + ".coefs"] = case["coefs"]
        store[name + ".samples"] = np.array(0 if case["samples"] is None else case["samples"], np.int32)
        store[name + ".points"] = np.stack([r["p"] for r in rows], axis=1)
        for key in ("u", "radius", "free"):
            store[f"{name}.{key}"] = np.array([r[key] for r in rows]).T
        for key in ("dist_lo", "dist_hi", "gap", "hinv", "jmax", "hmin", "steps"):
            store[f"{name}.{key}"] = np.array([r[key] for r in rows])
    store["names"] = np.array(names)
    store["margin"] = np.array(MARGIN)
    np.savez_compressed(os.path.join(HERE, "project.npz"), **store)
    print("wrote", len(names), "cases")


if __name__ == "__main__":
    main()
