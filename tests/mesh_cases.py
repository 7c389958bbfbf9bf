"""
What the triangulate tests share: the recorded cases of tests/golden/mesh.npz (tests/golden/make_golden_mesh.py), drawn
surfaces for the launch layouts, the raw result of a path as a tuple of NumPy arrays, and the integer geometry of the keys.
"""
import os

import numpy as np

import bspy_amd
from bspy_amd import mesh
from conftest import GOLDEN

GOLD = np.load(os.path.join(GOLDEN, "mesh.npz"))
NAMES = [str(n) for n in GOLD["names"]]
ORDERS = [(k0, k1) for k0 in (2, 3, 4) for k1 in (2, 3, 4)]
FIELDS = ("uv", "xyz", "vertex_offsets", "triangles", "triangle_offsets", "levels", "bound", "status", "normals")
L = mesh.L


def members_of(name):
    return int(GOLD[f"{name}/coefs"].shape[0])


def spline_of(name, member=0):
    order = [int(k) for k in GOLD[f"{name}/order"]]
    coefs = GOLD[f"{name}/coefs"][member]
    metadata = {"negateNormal": True} if f"{name}/negate" in GOLD.files else {}
    return bspy_amd.Spline(2, coefs.shape[0], order, list(coefs.shape[1:]), [GOLD[f"{name}/knots{a}"] for a in range(2)], coefs, metadata=metadata)


def arguments(name):
    return dict(tolerance=float(GOLD[f"{name}/tolerance"]), coefs=GOLD[f"{name}/coefs"], max_level=int(GOLD[f"{name}/max_level"]))


def clamped(order, breaks):
    return np.array([breaks[0]] * order + list(breaks[1:-1]) + [breaks[-1]] * order, np.float64)


def drawn(order, ncells, seed, ndep=3, members=1, noise=0.3):
    """A surface on ncells cells (uneven breaks) and ``members`` coefficient sets of growing amplitude."""
    rng = np.random.default_rng(seed)
    knots, shape = [], []
    for K, n in zip(order, ncells):
        breaks = np.concatenate(([0.0], np.sort(rng.uniform(0.2, 0.8, n - 1)), [1.0]))
        knots.append(clamped(K, list(breaks)))
        shape.append(len(knots[-1]) - K)
    coefs = noise * rng.standard_normal((members, ndep) + tuple(shape)) * (2.0 ** np.arange(members)).reshape(-1, 1, 1, 1)
    return bspy_amd.Spline(2, ndep, list(order), shape, knots, coefs[0]), coefs


def numpy_of(result):
    return tuple(a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in result)


def same(a, b):
    """Two raw results, byte for byte."""
    a, b = numpy_of(a), numpy_of(b)
    assert len(a) == len(b)
    for name, x, y in zip(FIELDS, a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    return True


def points_of(keys):
    """(X, Y) int64 of an array of keys."""
    keys = np.asarray(keys, np.int64)
    return keys >> mesh.SHIFT, keys & ((1 << mesh.SHIFT) - 1)


def doubled_areas(tkeys):
    """Twice the signed area of every triangle (m, 3) of keys, in integers."""
    X, Y = points_of(tkeys)
    return (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])


def cells_of(tkeys):
    """The cell (i, j) of every triangle: where its centroid lies."""
    X, Y = points_of(tkeys)
    return np.stack([X.sum(axis=1) // (3 << L), Y.sum(axis=1) // (3 << L)], axis=1)


def directed_edges(triangles):
    """{(a, b): how often the directed edge occurs}."""
    count = {}
    for t in np.asarray(triangles).tolist():
        for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            count[e] = count.get(e, 0) + 1
    return count
