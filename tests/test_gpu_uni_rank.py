"""eval_uni ranks the lanes of a half-wave inside their bank class by wave ballots (csrc/bsk_rank.hpp), jac_uni and the
fused normal by an LDS atomic.

A wrong rank cannot change a sum's terms, only their order and the row each lane starts at: the rotated basis and the
rotated row addresses must belong together, and the (q0+q2)+(q1+q3) tree makes the result independent of the rotation.
So every result here is checked twice: against the oracle, at the tolerance of test_gpu_parity.py's
test_uniform_knot_path (1e-12 of the result scale in fp64; unit normals 1e-10, as there), and bitwise against itself
with the same points at other positions of the batch - other lanes, other half-waves, other class mates.

Batch sizes straddle the wave (1 .. 65), the workgroup (1023, 1025) and, at 70 001, leave every workgroup a ragged last
round; the point sets put all lanes in one class (ranks up to 31), in two cells of one class, in as many classes as
there are (a sweep over consecutive spans) and at random.

Order 4 with nCoef 7 x 9 has fewer than 2 * order control points in a variable: its two clamped ends overlap and the
host keeps it on the general kernels (eval_rowrot / jac_rowrot), which rank with the same rotation; it runs here with
the same checks.
"""
import numpy as np
import pytest

import oracle
from bspy_amd import DeviceSpline

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 63, 64, 65, 1023, 1025, 70_001)
NMAX = max(SIZES)
TOL = 1e-12             # test_uniform_knot_path, fp64
TOL_NORMAL = 1e-10      # the same test's bar for unit normals

SHAPES = {
    "o4_8x8": (4, (8, 8)),
    "o4_7x9": (4, (7, 9)),
    "o2_5x6": (2, (5, 6)),
}


def _scale(ref):
    return max(1.0, float(np.max(np.abs(ref))))


def _knots(order, ncoef, lo, hi):
    dom = np.linspace(lo, hi, ncoef - order + 2)
    return np.concatenate([np.full(order - 1, lo), dom, np.full(order - 1, hi)])


def _point_sets(order, ncoef, dom, rng):
    """name -> [u, v] of NMAX points."""
    ns = [nc - order + 1 for nc in ncoef]
    h = [(hi - lo) / n for (lo, hi), n in zip(dom, ns)]

    def in_cells(c0, c1):
        # interior of the cells (c0[i], c1[i]): 0.02 .. 0.98 of the span, so rounding cannot move a point to a neighbour
        f = 0.02 + 0.96 * rng.random((2, NMAX))
        return [dom[0][0] + (np.asarray(c0) + f[0]) * h[0], dom[1][0] + (np.asarray(c1) + f[1]) * h[1]]

    i = np.arange(NMAX)
    two = rng.integers(0, 2, NMAX)
    sets = {
        "random": [lo + (hi - lo) * rng.random(NMAX) for lo, hi in dom],
        "one_cell": in_cells(np.full(NMAX, ns[0] - 1), np.full(NMAX, 1 % ns[1])),
        # neighbours along the first variable: the bases differ by one row stride = 32 / order (mod 32)
        "two_cells": in_cells(ns[0] - 2 + two, np.full(NMAX, ns[1] - 1)),
        # consecutive lanes in consecutive spans of the second variable, the first one moving on after each pass
        "sweep": in_cells((i // ns[1]) % ns[0], i % ns[1]),
    }
    for p in sets.values():
        for iv in range(2):
            np.clip(p[iv], dom[iv][0], dom[iv][1], out=p[iv])
    return sets


_CACHE = {}


def _case(shape, nDep):
    """Spline, point sets and oracle results on NMAX points, computed once and never written again."""
    key = (shape, nDep)
    if key not in _CACHE:
        order, ncoef = SHAPES[shape]
        rng = np.random.default_rng(1000 * nDep + sum(ncoef) + order)
        dom = ((-1.0, 2.0), (0.25, 1.0))
        knots = [_knots(order, nc, lo, hi) for nc, (lo, hi) in zip(ncoef, dom)]
        coefs = rng.standard_normal((nDep, *ncoef))
        if nDep == 3:
            # a graph with noise: the normal stays far from zero, so its unit vector is as well conditioned as the jacobian
            g0, g1 = np.meshgrid(np.linspace(*dom[0], ncoef[0]), np.linspace(*dom[1], ncoef[1]), indexing="ij")
            coefs[0] = g0 + 0.05 * coefs[0]
            coefs[1] = g1 + 0.05 * coefs[1]
            coefs[2] *= 0.3
        od = (order, order)
        sets = _point_sets(order, ncoef, dom, rng)
        ref = {}
        for name, pts in sets.items():
            r = {"evaluate": oracle.c_evaluate(od, ncoef, knots, coefs, [0, 0], pts),
                 "d11": oracle.c_evaluate(od, ncoef, knots, coefs, [1, 1], pts),
                 "jacobian": oracle.c_jacobian(od, ncoef, knots, coefs, pts)}
            if abs(2 - nDep) == 1:
                r["normal"] = oracle.c_normal(od, ncoef, knots, coefs, pts)
            for k, (arr, bad) in r.items():
                assert bad == -1, (name, k, bad)
                arr.setflags(write=False)
            for p in pts:
                p.setflags(write=False)
            ref[name] = {k: v[0] for k, v in r.items()}
        uni = all(nc >= 2 * order for nc in ncoef)
        _CACHE[key] = (od, ncoef, knots, coefs, sets, ref, uni)
    return _CACHE[key]


def _ops(t, has_normal):
    ops = [("evaluate", lambda p: t.evaluate(p), 0), ("d11", lambda p: t.evaluate(p, [1, 1]), 0),
           ("jacobian", lambda p: t.jacobian(p), 1)]
    if has_normal:
        ops.append(("normal", lambda p: t.normal(p), 1))
    return ops


@pytest.mark.parametrize("nDep", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_against_the_oracle(shape, nDep):
    od, ncoef, knots, coefs, sets, ref, uni = _case(shape, nDep)
    t = DeviceSpline(od, ncoef, knots, coefs, np.float64)
    fam = ("eval_uni", "jac_uni") if uni else ("eval_rowrot", "jac_rowrot")
    worst = {}
    for name, pts in sets.items():
        for n in SIZES:
            p = [np.ascontiguousarray(q[:n]) for q in pts]
            for op, fn, k in _ops(t, "normal" in ref[name]):
                out = fn(p)
                assert t.last_kernel() == fam[k], (name, n, op, t.last_kernel())
                r = ref[name][op][..., :n]
                assert out.shape == r.shape
                err = float(np.abs(out - r).max()) / (1.0 if op == "normal" else _scale(r))
                worst[op] = max(worst.get(op, 0.0), err)
                assert err <= (TOL_NORMAL if op == "normal" else TOL), (name, n, op, err)
    print(f"{shape} nDep {nDep}: worst error against the oracle {worst}")


@pytest.mark.parametrize("nDep", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_position_independence(shape, nDep):
    """The same points, shifted cyclically by 1, 31, 32 and 33 positions and reversed: bitwise the same results once
    the permutation is undone."""
    od, ncoef, knots, coefs, sets, ref, uni = _case(shape, nDep)
    t = DeviceSpline(od, ncoef, knots, coefs, np.float64)
    for name, pts in sets.items():
        for n in SIZES:
            p = [np.ascontiguousarray(q[:n]) for q in pts]
            perms = [np.roll(np.arange(n), -s) for s in (1, 31, 32, 33)] + [np.arange(n)[::-1]]
            for op, fn, _ in _ops(t, "normal" in ref[name]):
                out = fn(p)
                for j, perm in enumerate(perms):
                    got = fn([np.ascontiguousarray(q[perm]) for q in p])
                    back = np.empty_like(got)
                    back[..., perm] = got
                    assert np.array_equal(back, out, equal_nan=True), (name, n, op, j)
