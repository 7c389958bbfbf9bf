"""
Writes tests/golden/orders_scatter.npz: one scattered fit per order tuple the ``bsk_scatter_*`` kernels are built for, with
every edge of the kernels' point loop in it, and two fits on shifted and stretched domains; from the exact oracle
tests/scatter_ref.py the exact coefficients rounded once and the per-coefficient bar.  Run on the CPU from the repository
root:

    python tests/golden/make_golden_scatter_orders.py

The layout is that of tests/golden/scatter.npz (tests/golden/make_golden_scatter.py; ``scatter_ref.load`` reads both).  Per
case: order, knots0[, knots1], uvw (nInd, N), points (4, N), smoothing (0), penalty (0), counts (the points per flat knot
cell, as constructed), coefs (4, n), bar (4, n) and c, the counted roundings of the bar (``scatter_ref.roundings``).

The cases are named by their order tuple (``orders_util.case_id``): k2, k3, k4 and k22 .. k44, the tuples of
``orders_util.dispatched("scatter")``, which reads ``scatter.DEVICE_MAX_K``.  scatter_gram<K0, K1, NDEP> is built for every
one of them with NDEP 1 .. 4: a case has nDep 4, and the tests fit its first d channels.

    curves     10 knot cells, interior knots on the 1/16 grid with the widths 1 1 1 3 1 1 1 3 1 3 (sixteenths)
    surfaces   4 x 4 knot cells (n_d = K_d + 3), interior knots 3/16, 8/16, 11/16 and 5/16, 8/16, 13/16
               The widths are not all powers of two, so the basis values of order 2 round too (on equal dyadic cells every
               operation of an order-2 assembly is exact and the ratio to the bar is 0: it would test nothing).
    counts     with Q = strands(K0 K1) and SEG = 256, cells hold 3, 0, 1, Q - 1, Q + 1, 63, 65, SEG, SEG + 1 and 2 SEG + 5
               points: the strand deal (j = q; j < cnt; j += Q), the batch of 64 (cnt < 64, lane < cnt) and the unit (SEG)
               each from both sides.  The empty cell and the one-point cell are interior cells, so every coefficient's
               support holds data; the other six cells of a surface hold 5 to 11 points.  About 1200 points per case.
    points     parameters on a 2^-9 grid of their cell, strictly inside it; coordinates on the 2^-10 grid; permuted.
    shift4     the cubic curve on [2^20, 2^20 + 1]
    shift34    the (3, 4) surface on [-2^10, -2^10 + 3] x [2^16, 2^16 + 1/4]
               Every knot and parameter is representable there (checked below), and the oracle takes the stored values.
"""
import os
import sys
import zipfile
from fractions import Fraction as F

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import orders_util as ou  # noqa: E402
import scatter_ref  # noqa: E402

SEG = scatter_ref.SEG
CURVE_WIDTHS = (1, 1, 1, 3, 1, 1, 1, 3, 1, 3)                  # sixteenths of the domain
SURFACE_INNER = ((3, 8, 11), (5, 8, 13))


def edges(Q):
    return [3, 0, 1, Q - 1, Q + 1, 63, 65, SEG, SEG + 1, 2 * SEG + 5]


def cell_counts(rng, order):
    """The points per flat knot cell."""
    want = edges(scatter_ref.strands(int(np.prod(order))))
    if len(order) == 1:
        return np.array(want, np.int64)
    counts = rng.integers(5, 12, 16)
    counts[[0, 5, 10, 1, 2, 3, 4, 6, 7, 8]] = want                 # 5 and 10: the interior cells (1, 1) and (2, 2)
    return counts.astype(np.int64)


def knot_vector(K, inner, lo, hi):
    t = lo + (hi - lo) * (np.array([0] * K + list(inner) + [16] * K) / 16.0)
    assert all(F(float(x)) == F(lo) + (F(hi) - F(lo)) * F(int(i), 16) for x, i in zip(t[K:-K], inner))   # nothing was rounded
    return t


def order_case(rng, order, lo=None, hi=None):
    nind = len(order)
    lo, hi = lo or (0.0,) * nind, hi or (1.0,) * nind
    inner = [tuple(np.cumsum(CURVE_WIDTHS)[:-1])] if nind == 1 else SURFACE_INNER
    knots = [knot_vector(K, inner[d], lo[d], hi[d]) for d, K in enumerate(order)]
    counts = cell_counts(rng, order)
    nc1 = 4 if nind == 2 else 1
    uvw = np.empty((nind, int(counts.sum())))
    at = 0
    for cell, m in enumerate(counts):
        for d, c in enumerate((cell // nc1, cell % nc1) if nind == 2 else (cell,)):
            left, right = knots[d][order[d] - 1 + c], knots[d][order[d] + c]
            breaks = (0,) + tuple(inner[d]) + (16,)
            i = rng.integers(32 * breaks[c] + 1, 32 * breaks[c + 1], m)            # the 2^-9 grid of the domain, inside the cell
            u = lo[d] + (hi[d] - lo[d]) * (i / 512.0)
            assert all(F(float(x)) == F(lo[d]) + (F(hi[d]) - F(lo[d])) * F(int(k), 512) for x, k in zip(u, i))   # nothing was rounded
            assert ((u > left) & (u < right)).all()
            uvw[d, at:at + m] = u
        at += m
    perm = rng.permutation(uvw.shape[1])
    points = rng.integers(-2 ** 10, 2 ** 10 + 1, (4, uvw.shape[1])) / 2.0 ** 10
    return dict(order=tuple(order), knots=knots, uvw=uvw[:, perm], points=points, counts=counts)


def cases():
    from bspy_amd import scatter
    top = scatter.DEVICE_MAX_K
    tuples = ou.dispatched("scatter")
    assert tuples == [(k,) for k in range(2, top + 1)] + [(a, b) for a in range(2, top + 1) for b in range(2, top + 1)]
    rng = np.random.default_rng(20251)
    out = {ou.case_id(order): order_case(rng, order) for order in tuples}
    out["shift4"] = order_case(rng, (4,), lo=(2.0 ** 20,), hi=(2.0 ** 20 + 1.0,))
    out["shift34"] = order_case(rng, (3, 4), lo=(-2.0 ** 10, 2.0 ** 16), hi=(-2.0 ** 10 + 3.0, 2.0 ** 16 + 0.25))
    return out


def save(path, store):
    """np.savez_compressed with a fixed time stamp per member: two runs write the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, value in store.items():
            member = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            member.compress_type = zipfile.ZIP_DEFLATED
            with z.open(member, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(value), allow_pickle=False)


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
        store[f"{name}.counts"] = case["counts"]
        store[f"{name}.smoothing"] = np.float64(0.0)
        store[f"{name}.penalty"] = np.int32(0)
        store[f"{name}.coefs"], store[f"{name}.bar"], store[f"{name}.c"] = coefs, bar, np.int32(c)
        print(name, case["uvw"].shape, "c =", c, "max |coef| %.3g" % np.abs(coefs).max(), "max bar %.3g" % bar.max(), flush=True)
    store["names"] = np.array(names)
    save(os.path.join(HERE, "orders_scatter.npz"), store)


if __name__ == "__main__":
    main()
