"""
What the isosurface tests share: the recorded cases of tests/golden/iso.npz (tests/golden/make_golden_iso.py), drawn
splines for the launch layouts, the raw result of a path as a tuple of NumPy arrays, and the mesh checks.
"""
import os

import numpy as np

import bspy_amd
from bspy_amd import isosurface as iso
from conftest import GOLDEN

GOLD = np.load(os.path.join(GOLDEN, "iso.npz"))
NAMES = [str(n) for n in GOLD["names"]]
ORDERS = [(k0, k1, k2) for k0 in (2, 3, 4) for k1 in (2, 3, 4) for k2 in (2, 3, 4)]
FIELDS = ("vertices", "keys", "vertex_offsets", "triangles", "triangle_offsets", "cells", "status")


def spline_of(name):
    order = [int(k) for k in GOLD[f"{name}/order"]]
    coefs = GOLD[f"{name}/coefs"]
    return bspy_amd.Spline(3, 1, order, list(coefs.shape), [GOLD[f"{name}/knots{a}"] for a in range(3)], coefs[None])


def levels_of(name):
    return [float(v) for v in GOLD[f"{name}/levels"]]


def clamped(order, breaks):
    return np.array([breaks[0]] * order + list(breaks[1:-1]) + [breaks[-1]] * order, np.float64)


def drawn(order, ncells, seed, fields=1, noise=0.4):
    """A spline on ncells cells (uneven breaks) and ``fields`` coefficient sets: a slope through the domain with noise."""
    rng = np.random.default_rng(seed)
    knots, shape = [], []
    for K, n in zip(order, ncells):
        breaks = np.concatenate(([0.0], np.sort(rng.uniform(0.2, 0.8, n - 1)), [1.0]))
        knots.append(clamped(K, list(breaks)))
        shape.append(len(knots[-1]) - K)
    slope = sum(np.linspace(-1.0, 1.0, m).reshape([-1 if a == axis else 1 for a in range(3)]) for axis, m in enumerate(shape))
    coefs = slope[None] + noise * rng.standard_normal((fields,) + tuple(shape)) + np.linspace(0.0, 0.5, fields).reshape(-1, 1, 1, 1)
    return bspy_amd.Spline(3, 1, list(order), shape, knots, coefs[:1]), coefs


def numpy_of(result):
    return tuple(a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in result)


def same(a, b):
    """Two raw results, byte for byte."""
    a, b = numpy_of(a), numpy_of(b)
    for name, x, y in zip(FIELDS, a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    return True


def directed_edges(triangles):
    """{(a, b): how often the directed edge occurs}."""
    count = {}
    for t in np.asarray(triangles).tolist():
        for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            count[e] = count.get(e, 0) + 1
    return count
