"""
Writes tests/golden/scatter.npz: small scattered fits and, from the exact oracle tests/scatter_ref.py, the exact
coefficients rounded once and the per-coefficient bar.  Run on the CPU from the repository root:

    python tests/golden/make_golden_scatter.py

Per case: order, knots0[, knots1], uvw (nInd, N), points (nDep, N), weights (N,) where the case has them, smoothing,
penalty, coefs (nDep, n), bar (nDep, n) and c, the counted roundings of the bar:

    bar_j = c eps (|N^-1| (Nbar |c| + A^T W |p|))_j,   Nbar = A^T W A + lambda |E|

c is COUNTED, not fitted: the roundings on the longest chain of the statement of bspy_amd/scatter.py, as
``scatter_ref.roundings`` adds them up:

    c =   2 (5 (K0 - 1) + 5 (K1 - 1) + 1) + 2        two basis values and the products w B_a B_b
        + ceil(SEG / Q)                              the longest strand of a unit
        + log2(Q) + ceil(log2(units))                the strands' tree and the units' tree of the fullest cell
        + K0 K1                                      the cells of a stencil entry
        + 2 (3 m + 6 K) + 2 K + 6 + m                the penalty (smoothing > 0 only), K = max(order)
        + 3 (half bandwidth + 1)                     the banded factorisation and the two substitutions

The inputs are dyadic rationals of a few bits (knots on a grid of 1/16 of the domain, parameters on one of 2^-12,
coordinates on one of 2^-10): the exact elimination stays affordable, and the basis values, whose knot differences are
not powers of two, still round at every step.  The cases are the smallest that can go wrong: every order pair 2 .. 4 x 2 .. 4 on 7 x 6 coefficients,
curves of orders 2 .. 6, nDep 1 .. 4, non-uniform knots with a double interior knot (a cell of zero width), a shifted and
stretched domain, cells with 0, 1, Q - 1, SEG, SEG + 1 and 2 SEG + 5 points, points on an interior knot and on the right
domain end, weights with zeros, float32 points, and a hole in the data with smoothing > 0 for both penalties.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import scatter_ref  # noqa: E402


def clamped(K, interior, lo=0.0, hi=1.0):
    t = np.concatenate([[0.0] * K, np.asarray(interior, np.float64), [1.0] * K])
    return lo + (hi - lo) * t


def grid(rng, n, lo, hi, bits=12):
    return lo + (hi - lo) * rng.integers(0, 2 ** bits + 1, n) / 2.0 ** bits


def values(rng, shape, bits=10):
    return rng.integers(-2 ** bits, 2 ** bits + 1, shape) / 2.0 ** bits


def surface_case(rng, order, N=300, nDep=3, lo=(0.0, 0.0), hi=(1.0, 1.0), hole=False, **more):
    inner = [[3 / 16, 5 / 16, 9 / 16, 11 / 16, 14 / 16][:7 - order[0]],
             {2: [3 / 16, 7 / 16, 10 / 16, 13 / 16], 3: [5 / 16, 10 / 16, 10 / 16], 4: [10 / 16, 10 / 16]}[order[1]]]
    knots = [clamped(order[0], inner[0], lo[0], hi[0]), clamped(order[1], inner[1], lo[1], hi[1])]
    uvw = np.stack([grid(rng, N, lo[0], hi[0]), grid(rng, N, lo[1], hi[1])])
    if hole:
        mid = [(l + h) / 2 for l, h in zip(lo, hi)]
        out = (np.abs(uvw[0] - mid[0]) > 0.22 * (hi[0] - lo[0])) | (np.abs(uvw[1] - mid[1]) > 0.22 * (hi[1] - lo[1]))
        uvw = uvw[:, out]
    return dict(order=order, knots=knots, uvw=uvw, points=values(rng, (nDep, uvw.shape[1])), **more)


def curve_case(rng, K, N=200, nDep=2, **more):
    knots = clamped(K, [3 / 16, 7 / 16, 7 / 16, 13 / 16][:max(2, 7 - K)] if K >= 3 else [3 / 16, 7 / 16, 11 / 16, 13 / 16])
    return dict(order=(K,), knots=[knots], uvw=grid(rng, N, 0.0, 1.0)[None], points=values(rng, (nDep, N)), **more)


def counts_case(rng):
    """A cubic curve whose cells hold 0, 1, Q - 1 = 15, SEG, SEG + 1 and 2 SEG + 5 points (and the rest a few)."""
    K, SEG = 4, scatter_ref.SEG
    knots = clamped(K, np.arange(1, 8) / 8.0)
    want = [6, 0, 1, scatter_ref.strands(K) - 1, SEG, SEG + 1, 2 * SEG + 5, 7]
    u = np.concatenate([(c + rng.integers(1, 2 ** 9, m) / 2.0 ** 9) / 8.0 for c, m in enumerate(want)])
    u = u[rng.permutation(len(u))]
    return dict(order=(K,), knots=[knots], uvw=u[None], points=values(rng, (2, len(u))))


def cases():
    rng = np.random.default_rng(20250)
    out = {}
    for k0 in (2, 3, 4):
        for k1 in (2, 3, 4):
            out[f"pair{k0}{k1}"] = surface_case(rng, (k0, k1), nDep=1 + (k0 + k1) % 4)
    for K in (2, 3, 4, 5, 6):
        out[f"curve{K}"] = curve_case(rng, K, nDep=1 + (K - 2) % 4)
    out["shifted"] = surface_case(rng, (4, 3), lo=(3.0, -2.0), hi=(7.0, -1.0))
    out["counts"] = counts_case(rng)
    on = surface_case(rng, (3, 4), N=200, nDep=2)
    t0, t1 = on["knots"]
    on["uvw"][0, :20] = t0[4]                      # on an interior knot
    on["uvw"][1, 10:30] = t1[-1]                   # on the right domain end
    on["uvw"][0, 30:40] = t0[-1]
    on["uvw"][1, 40:50] = t1[5]                    # on the double knot
    out["onknots"] = on
    w = surface_case(rng, (4, 4), N=400)
    w["weights"] = rng.integers(0, 9, w["uvw"].shape[1]) / 4.0
    out["weights"] = w
    f = surface_case(rng, (3, 3), N=300)
    f["points"] = f["points"].astype(np.float32)
    f["uvw"] = f["uvw"].astype(np.float32)
    out["float32"] = f
    for m in (1, 2):
        out[f"hole{m}"] = surface_case(rng, (4, 4), N=500, hole=True, smoothing=2.0 ** -20, penalty=m)
    out["smoothcurve"] = curve_case(rng, 4, N=40, smoothing=2.0 ** -10, penalty=2)
    return out


def main():
    store = {}
    names = []
    for name, case in cases().items():
        coefs, bar, c = scatter_ref.record(case)
        names.append(name)
        store[f"{name}.order"] = np.array(case["order"], np.int32)
        for d, t in enumerate(case["knots"]):
            store[f"{name}.knots{d}"] = np.asarray(t, np.float64)
        store[f"{name}.uvw"] = case["uvw"]
        store[f"{name}.points"] = case["points"]
        if case.get("weights") is not None:
            store[f"{name}.weights"] = case["weights"]
        store[f"{name}.smoothing"] = np.float64(case.get("smoothing", 0.0))
        store[f"{name}.penalty"] = np.int32(case.get("penalty", 0))
        store[f"{name}.coefs"], store[f"{name}.bar"], store[f"{name}.c"] = coefs, bar, np.int32(c)
        print(name, case["uvw"].shape, "c =", c, "max |coef| %.3g" % np.abs(coefs).max(), "max bar %.3g" % bar.max(), flush=True)
    store["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "scatter.npz"), **store)


if __name__ == "__main__":
    main()
