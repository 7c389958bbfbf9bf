"""
Golden values of ``zeros`` for systems of three scalar splines in three variables (``Spline.zeros3`` here).  Runs ONLY where
the reference checkout is importable (see make_golden.load_reference).  The outputs:

``roots3.npz``, per case: the inputs, the kind, what is exactly true and what the reference's ``spline.zeros()`` returned.
    "coupled"    random triples and a bicubic surface minus a cubic curve, decided by the certified oracle
                 tests/zeros3_ref.py: per zero the cell, the proposal x and the radius of its certified box (cell-local) and
                 the preconditioner Y.  The generator asserts the conditioning the tests' bar is a first-order statement
                 for: max_i sum_d |Y_id| S_d <= 1e3 in cell-local units, zeros at least 1e-3 of a cell apart and at least
                 2^-8 of a cell away from the cell's faces.
    "separable"  (p(u), q(v), r(w)): the zeros are the product of the exact roots of p, q and r (tests/zeros_ref.py); they lie
                 on a knot plane, on a cell edge, at the corner of eight cells and on the domain boundary.
    "line"       the graph surface (u, v, g(u, v)) on [0, 3]^2 (knots whose Greville abscissae are exact, so that u and v are
                 exact cubic splines) minus the line (3 t, 3/2, z0 + 3 m t), everything on a grid of 2^-10: the zeros are
                 (u, 3/2, u / 3) for the exact roots u of the cubic spline g(u, 3/2) - z0 - m u.
    "zero"       one zero cell.    "tangent"   a paraboloid touching a plane.    "empty"   candidates, but no zeros.
``ref_roots`` (n x 3, sorted), ``ref_error`` (what the reference raised, or ""), ``ref_complete`` (as many zeros as there are,
each within 1e-6 of its own), ``ref_dev`` (the largest max-norm distance of a reference zero from the exact one it is paired
with in (u, v, w) order; nan when the counts differ or the reference raised).  The reference is recorded, not followed: the
oracle is the yardstick for counts.

``roots3_semantics.json``: the messages and small outcomes.

    python tests/golden/make_golden_roots3.py

npz keys: ``<case>/order`` (3), ``<case>/knots0``, ``knots1``, ``knots2``, ``<case>/coefs`` (3, n0, n1, n2), ``<case>/kind``,
``<case>/exact_uvw`` (n x 3 float64, sorted), ``<case>/exact_cells`` (m x 6: u0, u1, v0, v1, w0, w1 of the zero cells);
coupled and zero: ``<case>/cert_cell`` (n x 3), ``<case>/cert_x`` (n x 3), ``<case>/cert_radius`` (n), ``<case>/cert_Y`` (n x 3 x 3);
separable and line: ``<case>/u_order``, ``u_knots``, ``u_coefs``, ``u_lo``, ``u_hi``, ``u_fprime`` and, separable only, the same
with ``v_`` and ``w_``; ``<case>/ref_roots``, ``ref_error``, ``ref_complete``, ``ref_dev``.
"""
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
from make_golden_refine import knot_vector  # noqa: E402
from make_golden_roots2 import conditioned_1d, one_d  # noqa: E402
import zeros3_ref  # noqa: E402


def certified(order, knots, coefs):
    """The certified zeros when the case is as well conditioned as the generator promises, else None."""
    try:
        exact = zeros3_ref.zeros(order, knots, coefs)
    except ArithmeticError:
        return None
    S = [float(np.abs(comp.astype(np.float64)).max()) for comp in coefs]
    for z in exact:
        if max(sum(abs(float(z["Y"][i][d])) * S[d] for d in range(3)) for i in range(3)) > 1e3:
            return None
        if not all(Fraction(1, 256) <= z["lo"][d] and z["hi"][d] <= 1 - Fraction(1, 256) for d in range(3)):
            return None
    for a in exact:
        for b in exact:
            if a is not b and a["cell"] == b["cell"] and max(abs(a["x"][d] - b["x"][d]) for d in range(3)) < Fraction(1, 1000):
                return None
    return exact


def cases():
    rng = np.random.default_rng(20251018)
    out = {}

    def put(name, kind, order, knots, coefs, **extra):
        out[name] = dict(kind=kind, order=[int(k) for k in order], knots=[np.asarray(t) for t in knots], coefs=np.asarray(coefs), **extra)
        print(f"  {name}: drawn", flush=True)

    def coupled(name, order, ncoef, dtype=np.float64, kdtype=np.float64, minimum=1, repeat=((), (), ())):
        for _ in range(200):
            knots = [knot_vector(rng, k, n, repeat=r).astype(kdtype) for k, n, r in zip(order, ncoef, repeat)]
            coefs = rng.standard_normal((3, *ncoef)).astype(dtype)
            exact = certified(order, knots, coefs)
            if exact is not None and len(exact) >= minimum:
                return put(name, "coupled", order, knots, coefs)
        raise AssertionError(f"{name}: no well conditioned draw")

    coupled("rand_222", (2, 2, 2), (3, 3, 3), minimum=2)              # 2 x 2 x 2 cells
    coupled("rand_333", (3, 3, 3), (5, 4, 3), minimum=2)              # 3 x 2 x 1 cells
    coupled("rand_444", (4, 4, 4), (6, 5, 4))
    coupled("rand_442", (4, 4, 2), (6, 5, 2))
    coupled("rand_234", (2, 3, 4), (4, 4, 4))
    coupled("f32_coefs_332", (3, 3, 2), (4, 4, 3), dtype=np.float32)
    coupled("f32_knots_233", (2, 3, 3), (4, 4, 3), kdtype=np.float32)
    coupled("double_knot_333", (3, 3, 3), (6, 4, 3), repeat=((0,), (), ()))
    for _ in range(200):                                              # surface.subtract(curve): s(u, v) - c(t), exact on a grid
        ks = [knot_vector(rng, 4, 5), np.array([0, 0, 0, 0, 1, 1, 1, 1.0])]
        kc = np.array([0, 0, 0, 0, 1, 1, 1, 1.0])
        gu, gv = np.meshgrid(np.linspace(0, 1, 5), np.linspace(0, 1, 4), indexing="ij")
        s = np.round((np.stack([gu, gv, 0.0 * gu]) + 0.15 * rng.standard_normal((3, 5, 4))) * 1024) / 1024
        c = np.stack([rng.uniform(0.2, 0.8, 4), rng.uniform(0.2, 0.8, 4), np.linspace(-0.6, 0.6, 4) + 0.1 * rng.standard_normal(4)])
        c = np.round(c * 1024) / 1024
        coefs = s[:, :, :, None] - c[:, None, None, :]
        exact = certified((4, 4, 4), ks + [kc], coefs)
        if exact is not None and len(exact) >= 1:
            put("bicubic_minus_cubic", "coupled", (4, 4, 4), ks + [kc], coefs)
            break
    else:
        raise AssertionError("bicubic_minus_cubic: no well conditioned draw")

    # roots of p at 1/8 and at the knot 1/2; the root of q at the knot 1/2; roots of r at the end 0, at 3/8 and at the knot 3/4:
    # (1/8, 1/2, 3/8) lies on a knot plane, (1/2, 1/2, 3/8) and (1/8, 1/2, 3/4) on cell edges, (1/2, 1/2, 3/4) at the corner of
    # eight cells, (1/8, 1/2, 0) and (1/2, 1/2, 0) on the domain boundary
    tp, p = [0, 0, 0.25, 0.5, 1, 1], [1.0, -1.0, 0.0, 1.0]
    tq, q = [0, 0, 0.5, 1, 1], [1.0, 0.0, -1.0]
    tr, r = [0, 0, 0.25, 0.5, 0.75, 1, 1], [0.0, 1.0, -1.0, 0.0, 1.0]
    coefs = np.stack([np.broadcast_to(np.array(p)[:, None, None], (4, 3, 5)), np.broadcast_to(np.array(q)[None, :, None], (4, 3, 5)),
                      np.broadcast_to(np.array(r)[None, None, :], (4, 3, 5))])
    put("sep_knots_222", "separable", (2, 2, 2), [np.array(tp, float), np.array(tq, float), np.array(tr, float)], coefs,
        lines=[(2, np.array(tp, float), np.array(p)), (2, np.array(tq, float), np.array(q)), (2, np.array(tr, float), np.array(r))])

    for _ in range(400):                                              # graph surface minus line, see the head of this file
        ku, kv, kt = np.array([0, 0, 0, 0, 1.5, 3, 3, 3, 3.0]), np.array([0, 0, 0, 0, 3, 3, 3, 3.0]), np.array([0, 0, 1, 1.0])
        g = np.round(rng.standard_normal((5, 4)) * 512) / 1024
        z0, m = np.round(rng.standard_normal() * 128) / 1024, np.round(rng.standard_normal() * 256) / 1024
        greville_u, greville_v = np.array([0, 0.5, 1.5, 2.5, 3.0]), np.array([0, 1, 2, 3.0])
        line = (g[:, 0] + 3 * g[:, 1] + 3 * g[:, 2] + g[:, 3]) / 8 - z0 - m * greville_u
        e = conditioned_1d(4, ku, line)
        if e is None or len(e["brackets"]) < 2:
            continue
        us = [float(lo + hi) / 2 for lo, hi in e["brackets"]]
        if any(min(abs(u - k) for k in (0.0, 1.5, 3.0)) < 3e-2 for u in us):
            continue
        s = np.stack([np.broadcast_to(greville_u[:, None], (5, 4)), np.broadcast_to(greville_v[None, :], (5, 4)), g])
        c = np.array([[0.0, 3.0], [1.5, 1.5], [z0, z0 + 3 * m]])
        put("bicubic_minus_line", "line", (4, 4, 2), [ku, kv, kt], s[:, :, :, None] - c[:, None, None, :], line=(4, ku, line))
        break
    else:
        raise AssertionError("bicubic_minus_line: no well conditioned draw")

    # one zero cell: component 0 vanishes on the first cell; component 1 is positive there and around it
    for _ in range(200):
        knots = [knot_vector(rng, 3, 4), knot_vector(rng, 3, 4), knot_vector(rng, 2, 3)]
        coefs = rng.standard_normal((3, 4, 4, 3))
        coefs[0, :3, :3, :2] = 0.0
        coefs[1] = np.abs(coefs[1]) + 0.1
        coefs[1, 3:, 3:, :] = -coefs[1, 3:, 3:, :]
        if certified((3, 3, 2), knots, coefs) is not None:
            put("zero_one_cell", "zero", (3, 3, 2), knots, coefs)
            break
    else:
        raise AssertionError("zero_one_cell: no draw")
    # (u - w, v - w, (u - 1/2)^2 + (v - 1/2)^2): the paraboloid touches the plane of height 0 at u = v = 1/2, where w = 1/2
    bez = [[0, 0, 0, 1, 1, 1.0], [0, 0, 0, 1, 1, 1.0], [0, 0, 1, 1.0]]
    i, j, k = np.meshgrid(np.arange(3), np.arange(3), np.arange(2), indexing="ij")
    a = np.array([0.25, -0.25, 0.25])
    put("tangent", "tangent", (3, 3, 2), bez, np.stack([i / 2 - k, j / 2 - k, a[i] + a[j]]).astype(float))
    # u - v and u - v - 1/20 are parallel planes; w - 1/2
    lin = [[0, 0, 1, 1.0]] * 3
    i, j, k = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    put("empty", "empty", (2, 2, 2), lin, np.stack([i - j, i - j - 0.05, k - 0.5]).astype(float))
    return out


def exact_of(c):
    """(exact_uvw sorted, extra arrays) of a case."""
    order, knots, coefs = c["order"], c["knots"], c["coefs"]
    extra = {}
    if c["kind"] in ("coupled", "zero", "empty"):
        exact = zeros3_ref.zeros(order, knots, coefs)
        uvw = [tuple(float(z["t0"][a] + z["x"][a] * z["h"][a]) for a in range(3)) for z in exact]
        if c["kind"] in ("coupled", "zero"):
            extra = dict(cert_cell=np.array([z["cell"] for z in exact], np.int32).reshape(-1, 3),
                         cert_x=np.array([[float(v) for v in z["x"]] for z in exact]).reshape(-1, 3),
                         cert_radius=np.array([float(z["radius"]) for z in exact]),
                         cert_Y=np.array([[[float(v) for v in row] for row in z["Y"]] for z in exact]).reshape(-1, 3, 3))
    elif c["kind"] == "separable":
        roots_of = []
        for prefix, line in zip("uvw", c["lines"]):
            arrays, found = one_d(prefix, *line)
            extra.update(arrays)
            roots_of.append(found)
        uvw = [(u, v, w) for u in roots_of[0] for v in roots_of[1] for w in roots_of[2]]
    elif c["kind"] == "line":
        extra, us = one_d("u", *c["line"])
        uvw = [(u, 1.5, u / 3.0) for u in us]
    else:
        uvw = []
    uvw = np.array(sorted(uvw), np.float64).reshape(-1, 3)
    cells = []
    if c["kind"] == "zero":
        breaks, _ = zeros3_ref.bezier_cells(order, knots, coefs)
        cells = [[float(breaks[a][at[a] + n]) for a in range(3) for n in range(2)] for at in zeros3_ref.zero_cells(order, knots, coefs)]
    return uvw, dict(extra, exact_cells=np.array(cells, np.float64).reshape(-1, 6))


SEMANTICS = [
    ("nind_ne_ndep", dict(order=[2, 2, 2], knots=[[0.0, 0.0, 1.0, 1.0]] * 3, coefs=[[[[1.0, -2.0], [0.5, 1.0]], [[1.0, 2.0], [0.5, -1.0]]]] * 2)),
    ("no_zeros", dict(order=[2, 2, 2], knots=[[0.0, 0.0, 1.0, 1.0]] * 3,
                      coefs=[[[[1.0, 2.0], [0.5, 1.0]], [[1.0, 2.0], [0.5, 1.0]]], [[[1.0, -2.0], [0.5, 1.0]], [[1.0, 2.0], [0.5, -1.0]]],
                             [[[1.0, -2.0], [0.5, 1.0]], [[-1.0, 2.0], [0.5, 1.0]]]])),
    # (u - 1/4, v - 1/2, w - 3/4)
    ("one_zero", dict(order=[2, 2, 2], knots=[[0.0, 0.0, 1.0, 1.0]] * 3,
                      coefs=[[[[-0.25, -0.25], [-0.25, -0.25]], [[0.75, 0.75], [0.75, 0.75]]],
                             [[[-0.5, -0.5], [0.5, 0.5]], [[-0.5, -0.5], [0.5, 0.5]]],
                             [[[-0.75, 0.25], [-0.75, 0.25]], [[-0.75, 0.25], [-0.75, 0.25]]]])),
]


def main():
    bspy = load_reference()
    out = {}
    for name, c in cases().items():
        uvw, extra = exact_of(c)
        spline = bspy.Spline(3, 3, c["order"], list(c["coefs"].shape[1:]), c["knots"], c["coefs"])
        started = time.perf_counter()
        try:
            found = [r for r in spline.zeros() if not isinstance(r, tuple)]
            error = ""
        except Exception as e:                                          # recorded: the tests do not follow it
            found, error = [], f"{type(e).__name__}: {e}"
        seconds = time.perf_counter() - started
        ref = np.array(sorted(tuple(float(v) for v in r) for r in found), np.float64).reshape(-1, 3)
        dev = float(np.abs(ref - uvw).max()) if len(ref) == len(uvw) and len(uvw) else float("nan")
        complete = not error and len(ref) == len(uvw) and (len(uvw) == 0 or dev <= 1e-6)
        print(f"{name}: {len(uvw)} zeros; reference {len(ref)} in {seconds:.2f} s, complete {complete}, ref_dev {dev:.3e} {error}", flush=True)
        rec = dict(order=np.array(c["order"], np.int32), knots0=c["knots"][0], knots1=c["knots"][1], knots2=c["knots"][2], coefs=c["coefs"],
                   kind=np.array(c["kind"]), exact_uvw=uvw, ref_roots=ref, ref_error=np.array(error), ref_complete=np.array(bool(complete)),
                   ref_dev=np.float64(dev), ref_seconds=np.float64(seconds), **extra)
        for key, val in rec.items():
            out[f"{name}/{key}"] = val

    records = []
    for name, s in SEMANTICS:
        coefs = np.array(s["coefs"])
        spline = bspy.Spline(3, len(coefs), s["order"], list(coefs.shape[1:]), [np.array(k) for k in s["knots"]], coefs)
        record = dict(name=name, spline=s, error=None, result=None)
        try:
            record["result"] = sorted([float(v) for v in r] for r in spline.zeros())
        except ValueError as e:
            record["error"] = str(e)
        print(f"{name}: {record['error']!r} {record['result']}")
        records.append(record)

    path = os.path.join(HERE, "roots3.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "roots3_semantics.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
