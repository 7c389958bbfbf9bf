"""
What the tests of the cell families' shared front (``_cells.coefs_arg``, ``bezier_rows``, ``level_batch``) share: one small
batch call per family that takes a coefficient net, with two members that differ, float32, on the smallest shapes that
still have a neighbour cell and mixed orders.  A case is (spline, call, coefs): ``call(coefs, **more)`` is the public
batch call on the spline's knots.
"""
import numpy as np

import bspy_amd
import iso_cases
import mesh_cases
from bspy_amd import contours, isosurface, mesh, roots, roots2, roots3

NAMES = ("zeros", "zeros2", "zeros3", "contours", "isosurface", "triangulate")
MODULES = dict(zeros=roots, zeros2=roots2, zeros3=roots3, contours=contours, isosurface=isosurface, triangulate=mesh)
MESH_TOLERANCE = float(mesh_cases.GOLD["bump/tolerance"])


def clamped(order, breaks):
    return np.array([breaks[0]] * order + list(breaks[1:-1]) + [breaks[-1]] * order, np.float64)


def _net(seed, order, breaks, lead):
    """(knots, nCoef, float32 standard-normal coefficients of the shape lead + nCoef)."""
    rng = np.random.default_rng(seed)
    knots = [clamped(k, b) for k, b in zip(order, breaks)]
    shape = [len(t) - k for t, k in zip(knots, order)]
    coefs = rng.standard_normal(tuple(lead) + tuple(shape))
    return knots, shape, coefs.astype(np.float32)


def case(name):
    if name == "zeros":                                  # order 4, three spans, two components
        knots, shape, coefs = _net(1, (4,), [[0.0, 0.3, 0.7, 1.0]], (2,))
        s = bspy_amd.Spline(1, 2, [4], shape, knots, coefs)
        return s, (lambda c, **more: roots.zeros_batch(s, coefs=c, **more)), coefs
    if name == "zeros2":                                 # orders (3, 4), 2 x 2 cells
        knots, shape, coefs = _net(2, (3, 4), [[0.0, 0.4, 1.0], [0.0, 0.7, 1.0]], (2, 2))
        s = bspy_amd.Spline(2, 2, [3, 4], shape, knots, coefs[0])
        return s, (lambda c, **more: roots2.zeros2_batch(s, coefs=c, **more)), coefs
    if name == "zeros3":                                 # orders (2, 3, 4), 1 x 1 x 2 cells
        knots, shape, coefs = _net(3, (2, 3, 4), [[0.0, 1.0], [0.0, 1.0], [0.0, 0.6, 1.0]], (2, 3))
        s = bspy_amd.Spline(3, 3, [2, 3, 4], shape, knots, coefs[0])
        return s, (lambda c, **more: roots3.zeros3_batch(s, coefs=c, **more)), coefs
    if name == "contours":                               # orders (3, 4), 2 x 2 cells, depth 2
        knots, shape, coefs = _net(4, (3, 4), [[0.0, 0.4, 1.0], [0.0, 0.7, 1.0]], (2,))
        s = bspy_amd.Spline(2, 1, [3, 4], shape, knots, coefs[:1])
        return s, (lambda c, **more: contours.trace_batch(s, coefs=c, depth=2, **more)), coefs
    if name == "isosurface":                             # orders (2, 3, 4), 2 x 1 x 1 cells, depth 1
        s, coefs = iso_cases.drawn((2, 3, 4), (2, 1, 1), 5, fields=2)
        return s, (lambda c, **more: isosurface.extract_batch(s, coefs=c, depth=1, **more)), coefs.astype(np.float32)
    # orders (3, 4), 2 x 2 cells, nDep 3, with normals; the four cells of member 0 get four different levels at this tolerance
    s, coefs = mesh_cases.drawn((3, 4), (2, 2), 145, members=2)
    return s, (lambda c, **more: mesh.triangulate_batch(s, MESH_TOLERANCE, coefs=c, normals=True, **more)), coefs.astype(np.float32)
