"""
Golden values of ``Spline.isosurface``: inputs and the recorded results of the exact rational oracle tests/iso_ref.py.  The
reference has nothing to compare with (its ``contours`` needs nInd - nDep == 1), so this generator needs no reference
checkout.  Run time: about half a minute, all of it exact arithmetic.

``iso.npz``, per case: the inputs (order, knots, coefficients, depth, levels) and, per level, what is exactly true of the
marched zero set: the triangles as triples of lattice-edge keys in (leaf, tetrahedron, triangle) order, the sorted vertex
keys, per vertex the middle of the exact root's bracket in (u, v, w) rounded to doubles, |df/ds| along its edge there and the
edge's extent per axis, the zero cells, the cells with an exactly-zero node, the components and the Euler characteristic.
The generator refuses a case that breaks one of these (a condition, not a tolerance):
  * no node has 0 < |exact value| < 16 (K0 + K1 + K2) eps S: signs are decidable in floats;
  * every exactly-zero node evaluates to exactly 0.0 in floats (such cases have small dyadic coefficients);
  * every crossed edge has exactly one exact root.

    python tests/golden/make_golden_iso.py
"""
import os
import sys
import time
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ.setdefault("BSPY_AMD_NO_TORCH", "1")
import iso_ref  # noqa: E402

EPS = 2.0 ** -52


def clamped(order, breaks, dtype=np.float64):
    return np.array([breaks[0]] * order + list(breaks[1:-1]) + [breaks[-1]] * order, dtype)


def polar2(c, t):
    """(x - c)^2 in the quadratic B-spline basis of the knots t: the blossom (a - c)(b - c) at consecutive knots."""
    return np.array([(t[i + 1] - c) * (t[i + 2] - c) for i in range(len(t) - 3)])


def build_cases(attempt=0):
    """``attempt`` reseeds the drawn cases (the generator replaces a drawn case that breaks a condition)."""
    cases = {}

    def add(name, order, knots, coefs, depth, levels=(0.0,), **extra):
        cases[name] = dict(order=np.array(order, np.int64), knots=[np.asarray(k) for k in knots], coefs=np.asarray(coefs), depth=int(depth),
                           levels=np.array(levels, np.float64), extra=extra)

    # a plane, trilinear on one cell: f = x + y / 2 + z / 4 - 0.8
    k2 = clamped(2, [0.0, 1.0])
    corner = np.array([[[x + 0.5 * y + 0.25 * z - 0.8 for z in (0.0, 1.0)] for y in (0.0, 1.0)] for x in (0.0, 1.0)])
    for name, depth in (("plane_d0", 0), ("plane_d1", 1), ("plane", 3)):
        add(name, [2, 2, 2], [k2, k2, k2], corner, depth, normal=np.array([1.0, 0.5, 0.25]))
    # a sphere of radius 0.3 around (0.47, 0.52, 0.49), tri-quadratic on 2 x 2 x 2 cells: strictly inside
    k3 = clamped(3, [0.0, 0.5, 1.0])
    centre = np.array([0.47, 0.52, 0.49])
    ball = polar2(centre[0], k3)[:, None, None] + polar2(centre[1], k3)[None, :, None] + polar2(centre[2], k3)[None, None, :]
    add("sphere", [3, 3, 3], [k3, k3, k3], ball - 0.09, 2, centre=centre)
    # the same sphere with radius 0.55: cut by the domain boundary
    add("sphere_cut", [3, 3, 3], [k3, k3, k3], ball - 0.3025, 2, centre=centre)
    # three levels of it in one call
    add("levels", [3, 3, 3], [k3, k3, k3], ball, 1, levels=(0.09, 0.16, 0.3025), centre=centre)
    # a tricubic on 2 x 3 x 2 cells with two blobs and noise
    rng = np.random.default_rng(2025 + attempt)
    ka, kb = clamped(4, [0.0, 0.5, 1.0]), clamped(4, [0.0, 0.3, 0.7, 1.0])
    g = np.array([0.6, -0.9, 2.0, -0.9, 0.6])
    h = np.array([0.5, 0.0, -0.3, -0.3, 0.0, 0.5])
    k = np.array([0.5, -0.1, -0.3, -0.1, 0.5])
    add("random_444", [4, 4, 4], [ka, kb, ka], g[:, None, None] + h[None, :, None] + k[None, None, :] + 0.05 * rng.standard_normal((5, 6, 5)), 1)
    # mixed orders on 2 x 2 x 2 cells: a slope with noise
    for name, order in (("random_234", (2, 3, 4)), ("random_423", (4, 2, 3))):
        knots = [clamped(K, [0.0, 0.4, 1.0]) for K in order]
        slope = sum(np.linspace(-1.0, 1.0, K + 1).reshape([-1 if a == axis else 1 for a in range(3)]) for axis, K in enumerate(order))
        add(name, order, knots, slope + 0.4 * rng.standard_normal(tuple(K + 1 for K in order)), 1)
    # a double knot plane: a C0 crease at x = 0.5
    kc = np.array([0.0, 0.0, 0.0, 0.5, 0.5, 1.0, 1.0, 1.0])
    roof = np.array([-0.6, -0.1, 0.45, -0.1, -0.6])
    add("crease", [3, 2, 2], [kc, k2, k2], roof[:, None, None] + np.array([0.0, 0.13])[None, :, None] + np.array([0.0, -0.07])[None, None, :], 2)
    # x + y + z = 1 through lattice nodes: exact float zeros, the sign-of-0 rule and status bit 2
    add("diagonal", [2, 2, 2], [k2, k2, k2], np.array([[[x + y + z - 1.0 for z in (0.0, 1.0)] for y in (0.0, 1.0)] for x in (0.0, 1.0)]), 2,
        normal=np.array([1.0, 1.0, 1.0]))
    # a zero cell between a negative and a positive one
    kz = clamped(2, [0.0, 1.0, 2.0, 3.0])
    face = np.array([[-1.0, -2.0], [-1.5, -1.25]])
    add("zero_cell", [2, 2, 2], [kz, k2, k2], np.stack([face, 0.0 * face, 0.0 * face, -face]), 1)
    # float32 input
    k32 = clamped(3, [0.0, 0.5, 1.0], np.float32)
    add("float32", [3, 3, 3], [k32, k32, k32], (ball - 0.09).astype(np.float32), 1, centre=centre)
    # far from the origin and large: [100, 103] x [-40, -38] x [7, 8], coefficients of 5000
    add("shifted", [3, 3, 3], [clamped(3, [100.0, 101.0, 102.0, 103.0]), clamped(3, [-40.0, -39.0, -38.0]), clamped(3, [7.0, 8.0])],
        5000.0 * (np.linspace(-1.0, 1.0, 5)[:, None, None] + 0.3 * rng.standard_normal((5, 4, 3))), 1)
    return cases


def record(name, case):
    out = {f"{name}/order": case["order"], f"{name}/coefs": case["coefs"], f"{name}/depth": np.int64(case["depth"]),
           f"{name}/levels": case["levels"]}
    for axis in range(3):
        out[f"{name}/knots{axis}"] = case["knots"][axis]
    for label, value in case["extra"].items():
        out[f"{name}/{label}"] = value
    K = [int(k) for k in case["order"]]
    wide = np.asarray(case["coefs"]).astype(np.float64)
    for b, level in enumerate(case["levels"]):
        S = float(np.abs(wide - level).max())
        breaks, cells = iso_ref.bezier_cells(K, case["knots"], case["coefs"], level)
        zero = iso_ref.zero_cells(cells, S)
        res = iso_ref.extract(K, case["knots"], case["coefs"], case["depth"], level, skip=set(zero))
        ex = res["exact"]
        bar = Fraction(16.0 * sum(K) * EPS * S)
        for at, value in ex._nodes.items():
            assert value == 0 or abs(value) >= bar, f"{name}: node {at} has the undecidable value {float(value):.3e}"
        roots, slopes, reach = [], [], []
        for key in res["keys"]:
            box, slope, width = ex.vertex(key)                 # asserts exactly one root
            roots.append([float((lo + hi) / 2) for lo, hi in box])
            slopes.append(float(slope))
            reach.append([float(w) for w in width])
        out[f"{name}/{b}/triangles"] = np.array(res["triangles"], np.int64).reshape(-1, 3)
        out[f"{name}/{b}/keys"] = np.array(res["keys"], np.int64)
        out[f"{name}/{b}/roots"] = np.array(roots, np.float64).reshape(-1, 3)
        out[f"{name}/{b}/slopes"] = np.array(slopes, np.float64)
        out[f"{name}/{b}/reach"] = np.array(reach, np.float64).reshape(-1, 3)
        out[f"{name}/{b}/zero"] = np.array(zero, np.int64).reshape(-1, 3)
        out[f"{name}/{b}/zero_nodes"] = np.array(res["zero_nodes"], np.int64).reshape(-1, 3)
        out[f"{name}/{b}/topology"] = np.array([res["components"], res["chi"]], np.int64)
        # the floats agree with the exact zeros (bspy_amd's plain-Python statement: no native code is needed)
        from bspy_amd import isosurface as iso
        if all(len(np.unique(k)) == 2 for k in case["knots"]):                    # one cell: the rows are the coefficients
            class OneCell:
                order, ncells, first, breaks = tuple(K), (1, 1, 1), [[0]] * 3, [np.unique(k) for k in case["knots"]]
            lat = iso.Lattice(wide, OneCell, level, case["depth"])
            for at, value in ex._nodes.items():
                assert (value == 0) == (lat.node_value(*at) == 0.0), f"{name}: node {at} is zero in one arithmetic only"
        else:
            assert not any(v == 0 for v in ex._nodes.values()) or name == "zero_cell", f"{name}: exact zeros on more than one cell"
        print(f"{name}/{b}: {len(res['triangles'])} triangles, {len(res['keys'])} vertices, components {res['components']}, chi {res['chi']}, "
              f"zero cells {len(zero)}", flush=True)
    return out


def main():
    t0 = time.time()
    cases = build_cases()
    out = {"names": np.array(sorted(cases))}
    for name in sorted(cases):
        for attempt in range(50):
            try:
                out.update(record(name, build_cases(attempt)[name]))
                break
            except AssertionError as e:
                if name not in ("random_444", "random_234", "random_423", "shifted"):
                    raise
                print(f"{name}: attempt {attempt} refused: {e}", flush=True)
        else:
            raise SystemExit(f"{name}: no draw passes the conditions")
    topo = {n: out[f"{n}/0/topology"].tolist() for n in cases}
    assert topo["sphere"] == [1, 2], topo["sphere"]
    assert topo["random_444"][0] >= 2, topo["random_444"]
    assert len(out["zero_cell/0/zero"]) == 1 and len(out["diagonal/0/zero_nodes"]) >= 1
    out["generator_seconds"] = np.float64(time.time() - t0)
    np.savez_compressed(os.path.join(HERE, "iso.npz"), **out)
    print("wrote iso.npz", os.path.getsize(os.path.join(HERE, "iso.npz")), "bytes in", round(time.time() - t0), "s")


if __name__ == "__main__":
    main()
