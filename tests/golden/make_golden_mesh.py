"""
Golden values of ``Spline.triangulate``: inputs and the recorded results of the exact rational oracle tests/mesh_ref.py.
The reference has no callable counterpart outside its OpenGL viewer, so this generator needs no reference checkout.  Run
time: about a minute, all of it exact arithmetic.

``mesh.npz``, per case: the inputs (order, knots, coefficients (B, nDep, n0, n1), tolerance, max_level) and, per member,
what is exactly true: Q (rounded once), the levels, which cells are capped, the sorted vertex keys, the triangles as key
triples with the cell of each, the exact vertex positions and parameters rounded once, and the exact surface rounded once
at seven points of every triangle: the centroid, the three edge midpoints and the three (2/3, 1/6, 1/6) points (WEIGHTS).
The generator refuses a case (a condition, not a tolerance) whose Q comes within 2^-20 (relative) of a level threshold, so
that no rounding can move a level, and a case that has lost the structure its name promises.

    python tests/golden/make_golden_mesh.py
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
import mesh_ref  # noqa: E402

WEIGHTS = [(Fraction(1, 3),) * 3, (Fraction(1, 2), Fraction(1, 2), Fraction(0)), (Fraction(0), Fraction(1, 2), Fraction(1, 2)),
           (Fraction(1, 2), Fraction(0), Fraction(1, 2)), (Fraction(2, 3), Fraction(1, 6), Fraction(1, 6)),
           (Fraction(1, 6), Fraction(2, 3), Fraction(1, 6)), (Fraction(1, 6), Fraction(1, 6), Fraction(2, 3))]


def clamped(order, breaks, dtype=np.float64):
    return np.array([breaks[0]] * order + list(breaks[1:-1]) + [breaks[-1]] * order, dtype)


def greville(order, knots):
    return np.array([np.mean(knots[i + 1:i + order]) for i in range(len(knots) - order)])


def graph(order, knots, z):
    """The surface (u, v, z(u, v)): x and y from the Greville abscissae; z (n0, n1)."""
    gu, gv = greville(order[0], knots[0]), greville(order[1], knots[1])
    return np.stack([np.broadcast_to(gu[:, None], z.shape), np.broadcast_to(gv[None, :], z.shape), z])


def build_cases():
    cases = {}
    rng = np.random.default_rng(2026)

    def add(name, order, knots, coefs, tolerance, max_level=8, **extra):
        coefs = np.asarray(coefs)
        cases[name] = dict(order=np.array(order, np.int64), knots=[np.asarray(k) for k in knots],
                           coefs=coefs if coefs.ndim == 4 else coefs[None], tolerance=float(tolerance), max_level=int(max_level), extra=extra)

    one3, one4 = clamped(3, [0.0, 1.0]), clamped(4, [0.0, 1.0])
    tol = 1e-3
    # 1: one cell at (0, 0)
    dent = np.zeros((3, 3))
    dent[1, 1] = 0.35 * tol
    add("one_00", [3, 3], [one3, one3], graph([3, 3], [one3, one3], dent), tol)
    # 2: one cell at (3, 1), and 12: one that needs (4, 1) capped at 2: z = A u^2 + C v^2, |S_uu| = 2 A = 0.7 (2 tol 4^3), |S_vv| = 2 C = 0.7 (2 tol 4)
    sq = np.array([0.0, 0.0, 1.0])
    bowl = lambda a, b: 0.7 * tol * (4.0 ** a * sq[:, None] + 4.0 ** b * sq[None, :])
    add("one_31", [3, 3], [one3, one3], graph([3, 3], [one3, one3], bowl(3, 1)), tol)
    add("capped", [3, 3], [one3, one3], graph([3, 3], [one3, one3], bowl(4, 1)), tol, max_level=2)
    # 13: one cell at (5, 4): 512 quads, one dependent variable
    add("one_54", [3, 3], [one3, one3], bowl(5, 4)[None], tol)
    # 3, 4: 2 x 1 cells, z = g(u) v^2: the levels along the shared edge differ by 1 and by 3
    two3 = clamped(3, [0.0, 0.5, 1.0])
    for name, X in (("step_1", 3.0), ("step_3", 33.0)):
        z = 0.7 * tol * np.array([1.0, 1.0, 1.0, X])[:, None] * sq[None, :]
        add(name, [3, 3], [two3, one3], graph([3, 3], [two3, one3], z), tol)
    # 5: 3 x 3 cells, a bump: the centre finer than all eight neighbours
    three3 = clamped(3, [0.0, 1.0, 2.0, 3.0])
    bump = np.zeros((5, 5))
    bump[2, 2] = 1.0
    add("bump", [3, 3], [three3, three3], graph([3, 3], [three3, three3], bump), 0.7)
    # 6: 3 x 3 cells, the centre flat and every neighbour finer: one quad with four fine sides
    ring = np.array([[(-1.0) ** (i + j) for j in range(5)] for i in range(5)])
    ring[1:4, 1:4] = 0.0
    add("ring", [3, 3], [three3, three3], graph([3, 3], [three3, three3], ring), 0.7)
    # 7, 8: a double and a triple interior knot, order 4
    for name, mult in (("double_knot", 2), ("triple_knot", 3)):
        ku = np.array([0.0] * 4 + [0.5] * mult + [1.0] * 4)
        kv = clamped(4, [0.0, 0.4, 1.0])
        add(name, [4, 4], [ku, kv], 0.3 * rng.standard_normal((3, len(ku) - 4, len(kv) - 4)), 2.56)
    # 9: all nine order tuples on 2 x 2 cells
    for K0 in (2, 3, 4):
        for K1 in (2, 3, 4):
            knots = [clamped(K0, [0.0, 0.45, 1.0]), clamped(K1, [0.0, 0.6, 1.0])]
            add(f"orders_{K0}{K1}", [K0, K1], knots, 0.2 * rng.standard_normal((3, K0 + 1, K1 + 1)), 0.2 if (K0, K1) == (2, 2) else 1.6 if K0 == 4 and K1 > 2 else 0.8)
    # 10: nDep 1, 2 and 3
    kq = [clamped(3, [0.0, 0.5, 1.0]), clamped(4, [0.0, 0.5, 1.0])]
    for ndep in (1, 2, 3):
        add(f"ndep_{ndep}", [3, 4], kq, 0.2 * rng.standard_normal((ndep, 4, 5)), 0.8)
    # 11: a plane on dyadic knots: every Q is 0
    plane = graph([3, 3], [two3, two3], np.zeros((4, 4)))
    plane[2] = plane[0] + 2.0 * plane[1]
    add("plane", [3, 3], [two3, two3], plane, tol)
    # 14: three nets with different levels
    add("batch", [3, 3], [two3, two3], np.stack([amp * rng.standard_normal((2, 4, 4)) for amp in (0.1, 1.0, 1.7)]), 1.28)
    # 15: the domain [3, 7] x [-2, -1]
    kd = [clamped(3, [3.0, 4.0, 6.0, 7.0]), clamped(3, [-2.0, -1.5, -1.0])]
    add("domain", [3, 3], kd, 0.3 * rng.standard_normal((3, 5, 4)), 0.8)
    # 16: float32 input
    k32 = [clamped(3, [0.0, 0.5, 1.0], np.float32), clamped(3, [0.0, 0.25, 1.0], np.float32)]
    add("float32", [3, 3], k32, (0.3 * rng.standard_normal((3, 4, 4))).astype(np.float32), 1.6)
    # 17: negateNormal
    add("negate", [3, 3], [two3, one3], 0.3 * rng.standard_normal((3, 4, 3)), 0.8, negate=np.bool_(True))
    return cases


def structure(name, members):
    """The structure that the name of a case promises."""
    lev = [np.array(m["lev"]) for m in members]
    first = lev[0]
    if name == "one_00":
        assert first.tolist() == [[[0, 0]]] and len(members[0]["triangles"]) == 2
    if name == "one_31":
        assert first.tolist() == [[[3, 1]]]
    if name == "capped":
        assert first.tolist() == [[[2, 1]]] and members[0]["capped"] == [[True]]
    if name == "one_54":
        assert first.tolist() == [[[5, 4]]]
    if name in ("step_1", "step_3"):
        assert abs(int(first[0, 0, 1]) - int(first[1, 0, 1])) == int(name[-1]), first.tolist()
    if name == "bump":
        assert all(first[1, 1, a] > first[i, j, a] for i in range(3) for j in range(3) for a in range(2) if (i, j) != (1, 1)), first.tolist()
    if name == "ring":
        assert first[1, 1].tolist() == [0, 0] and first[0, 1, 1] > 0 and first[2, 1, 1] > 0 and first[1, 0, 0] > 0 and first[1, 2, 0] > 0, first.tolist()
    if name == "plane":
        assert not first.any() and all(q == 0 for line in members[0]["Q"] for cell in line for q in cell)
    if name == "batch":
        assert len({l.tobytes() for l in lev}) == 3
    if name not in ("capped",):
        assert not any(c for m in members for line in m["capped"] for c in line), name


def record(name, case):
    out = {f"{name}/order": case["order"], f"{name}/coefs": case["coefs"], f"{name}/tolerance": np.float64(case["tolerance"]),
           f"{name}/max_level": np.int64(case["max_level"]), f"{name}/knots0": case["knots"][0], f"{name}/knots1": case["knots"][1]}
    for label, value in case["extra"].items():
        out[f"{name}/{label}"] = value
    K = [int(k) for k in case["order"]]
    members = []
    for b, coefs in enumerate(case["coefs"]):
        res = mesh_ref.mesh(K, case["knots"], coefs, case["tolerance"], case["max_level"])
        members.append(res)
        assert res["margin"] >= Fraction(1, 2 ** 20), f"{name}/{b}: a Q is within {float(res['margin']):.3e} of a threshold: change the tolerance"
        exact = {}

        def at(p, cell=None):
            if (p, cell) not in exact:
                exact[p, cell] = mesh_ref.point(res, p, cell)
            return exact[p, cell]

        index = {key: n for n, key in enumerate(res["keys"])}
        where = {}
        seven, tkeys, tcell = [], [], []
        for cell, corners in res["triangles"]:
            tkeys.append([mesh_ref.key(p) for p in corners])
            tcell.append(cell)
            for p in corners:
                where[mesh_ref.key(p)] = p
            seven.append([[float(v) for v in at((sum(w * p[0] for w, p in zip(ws, corners)), sum(w * p[1] for w, p in zip(ws, corners))), cell)]
                          for ws in WEIGHTS])
        assert sorted(where) == res["keys"] and len(index) == len(where)
        out[f"{name}/{b}/Q"] = np.array([[[float(q) for q in cell] for cell in line] for line in res["Q"]], np.float64)
        out[f"{name}/{b}/lev"] = np.array(res["lev"], np.int32)
        out[f"{name}/{b}/capped"] = np.array(res["capped"], np.uint8)
        out[f"{name}/{b}/keys"] = np.array(res["keys"], np.int64)
        out[f"{name}/{b}/triangles"] = np.array(tkeys, np.int64).reshape(-1, 3)
        out[f"{name}/{b}/tcell"] = np.array(tcell, np.int16).reshape(-1, 2)
        out[f"{name}/{b}/xyz"] = np.array([[float(v) for v in at(where[key])] for key in res["keys"]], np.float64)
        out[f"{name}/{b}/uv"] = np.array([[float(v) for v in mesh_ref.parameters(res, where[key])] for key in res["keys"]], np.float64)
        out[f"{name}/{b}/seven"] = np.array(seven, np.float64)
        print(f"{name}/{b}: levels {np.array(res['lev']).reshape(-1, 2).tolist()}, {len(tkeys)} triangles, {len(res['keys'])} vertices, "
              f"margin {float(res['margin']):.2e}", flush=True)
    structure(name, members)
    return out


def main():
    t0 = time.time()
    cases = build_cases()
    out = {"names": np.array(sorted(cases)), "weights": np.array([[float(w) for w in ws] for ws in WEIGHTS])}
    for name in sorted(cases):
        out.update(record(name, cases[name]))
    out["generator_seconds"] = np.float64(time.time() - t0)
    path = os.path.join(HERE, "mesh.npz")
    np.savez_compressed(path, **out)
    print("wrote mesh.npz", os.path.getsize(path), "bytes in", round(time.time() - t0), "s")


if __name__ == "__main__":
    main()
