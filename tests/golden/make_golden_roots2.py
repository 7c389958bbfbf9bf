"""
Golden values of ``zeros`` for systems of two scalar splines in two variables (``Spline.zeros2`` here).  Runs ONLY where
the reference checkout is importable (see make_golden.load_reference).  The outputs:

``roots2.npz``, per case: the inputs, the kind, what is exactly true and what the reference's ``spline.zeros()`` returned.
    "coupled"    random pairs and curve minus curve, decided by the certified oracle tests/zeros2_ref.py: per zero the cell,
                 the proposal (x, y) and the radius of its certified box (cell-local) and the preconditioner Y.  The
                 generator asserts the conditioning the tests' bar is a first-order statement for: max_i sum_d |Y_id| S_d
                 <= 1e3 in cell-local units, zeros at least 1e-3 of a cell apart and at least 2^-8 of a cell away from the
                 cell's edges.
    "separable"  f = p(u), g = q(v): the zeros are the product of the exact roots of p and q (tests/zeros_ref.py).  One
                 case has roots at a knot line, at a cell corner and on the domain boundary.
    "line"       a(u) - b(v), b a line p0 + v d, on a grid of 2^-10 so that the differences are exact: the exact roots of
                 n . (a(u) - p0), n normal to d.  The generator asserts that v is at least 1e-3 inside (0, 1) or outside.
    "zero"       one zero cell.        "tangent"   a curve touching a line.        "empty"   candidates, but no zeros.
``ref_roots`` (n x 2, sorted), ``ref_complete`` (as many zeros as there are, each within 1e-6 of its own), ``ref_dev`` (the
largest max-norm distance of a reference zero from the exact one it is paired with in (u, v) order; nan when the counts
differ or the reference raised).  The generator refuses to write unless ``ref_complete`` holds on at least three quarters
of the coupled, separable and line cases.

``roots2_semantics.json``: the messages and small outcomes.

    python tests/golden/make_golden_roots2.py

npz keys: ``<case>/order`` (2), ``<case>/knots0``, ``<case>/knots1``, ``<case>/coefs`` (2, n0, n1), ``<case>/kind``,
``<case>/exact_uv`` (n x 2 float64, sorted by (u, v)), ``<case>/exact_cells`` (m x 4: u0, u1, v0, v1 of the zero cells);
coupled and zero: ``<case>/cert_cell`` (n x 2), ``<case>/cert_xy`` (n x 2), ``<case>/cert_radius`` (n), ``<case>/cert_Y`` (n x 2 x 2);
separable and line: ``<case>/u_order``, ``<case>/u_knots``, ``<case>/u_coefs``, ``<case>/u_lo``, ``<case>/u_hi``,
``<case>/u_fprime`` and, separable only, the same with ``v_``; ``<case>/ref_roots``, ``<case>/ref_complete``, ``<case>/ref_dev``.
"""
import json
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
from make_golden_refine import knot_vector  # noqa: E402
import zeros2_ref  # noqa: E402
import zeros_ref  # noqa: E402


def certified(order, knots, coefs):
    """The certified zeros when the case is as well conditioned as the generator promises, else None."""
    try:
        exact = zeros2_ref.zeros(order, knots, coefs)
    except ArithmeticError:
        return None
    S = [float(np.abs(comp.astype(np.float64)).max()) for comp in coefs]
    for z in exact:
        if max(sum(abs(float(z["Y"][i][d])) * S[d] for d in range(2)) for i in range(2)) > 1e3:
            return None
        if not all(Fraction(1, 256) <= z["lo"][d] and z["hi"][d] <= 1 - Fraction(1, 256) for d in range(2)):
            return None
    for a in exact:
        for b in exact:
            if a is not b and a["cell"] == b["cell"] and max(abs(a["x"] - b["x"]), abs(a["y"] - b["y"])) < Fraction(1, 1000):
                return None
    return exact


def conditioned_1d(order, knots, coefs):
    try:
        exact = zeros_ref.roots(order, knots, coefs)
    except ArithmeticError:
        return None
    width = float(knots[len(knots) - order]) - float(knots[order - 1])
    mids = [float(lo + hi) / 2 for lo, hi in exact["brackets"]]
    if exact["intervals"] or any(abs(float(d)) * width < 1e-3 * exact["scale"] for d in exact["fprime"]):
        return None
    if any(b - a < 1e-3 * width for a, b in zip(mids[:-1], mids[1:])):
        return None
    return exact


def one_d(prefix, order, knots, coefs):
    exact = zeros_ref.roots(order, knots, coefs)
    return {f"{prefix}_order": np.array(order, np.int32), f"{prefix}_knots": np.asarray(knots, np.float64),
            f"{prefix}_coefs": np.asarray(coefs, np.float64),
            f"{prefix}_lo": np.array([float(lo) for lo, _ in exact["brackets"]]),
            f"{prefix}_hi": np.array([float(hi) for _, hi in exact["brackets"]]),
            f"{prefix}_fprime": np.array([float(d) for d in exact["fprime"]])}, [float(lo + hi) / 2 for lo, hi in exact["brackets"]]


def cases():
    rng = np.random.default_rng(20250921)
    out = {}

    def put(name, kind, order, knots, coefs, **extra):
        out[name] = dict(kind=kind, order=[int(k) for k in order], knots=[np.asarray(t) for t in knots], coefs=np.asarray(coefs), **extra)

    def coupled(name, order, ncoef, dtype=np.float64, kdtype=np.float64, minimum=2, **kw):
        for _ in range(400):
            knots = [knot_vector(rng, k, n, **kw).astype(kdtype) for k, n in zip(order, ncoef)]
            coefs = rng.standard_normal((2, *ncoef)).astype(dtype)
            exact = certified(order, knots, coefs)
            if exact is not None and len(exact) >= minimum:
                return put(name, "coupled", order, knots, coefs)
        raise AssertionError(f"{name}: no well conditioned draw")

    coupled("rand_22", (2, 2), (5, 5))
    coupled("rand_34", (3, 4), (5, 6))
    coupled("rand_44", (4, 4), (5, 6))
    coupled("rand_44_8x8", (4, 4), (8, 8), minimum=6)
    coupled("rand_42", (4, 2), (6, 4), minimum=1)
    coupled("rand_55", (5, 5), (6, 6))
    coupled("f32_coefs_44", (4, 4), (6, 5), dtype=np.float32)
    coupled("f32_knots_34", (3, 4), (6, 6), kdtype=np.float32)
    coupled("double_knot_44", (4, 4), (7, 7), repeat=(0,))
    for _ in range(400):                                                 # a.subtract(b) of two planar cubics: a(u) - b(v)
        ka, kb = knot_vector(rng, 4, 6), knot_vector(rng, 4, 5)
        a, b = np.round(rng.standard_normal((2, 6)) * 512) / 1024, np.round(rng.standard_normal((2, 5)) * 512) / 1024
        coefs = a[:, :, None] - b[:, None, :]
        exact = certified((4, 4), [ka, kb], coefs)
        if exact is not None and len(exact) >= 2:
            put("cubic_minus_cubic", "coupled", (4, 4), [ka, kb], coefs)
            break
    else:
        raise AssertionError("cubic_minus_cubic: no well conditioned draw")

    def separable(name, ku, tu, p, kv, tv, q):
        coefs = np.stack([np.repeat(np.asarray(p, np.float64)[:, None], len(q), axis=1),
                          np.repeat(np.asarray(q, np.float64)[None, :], len(p), axis=0)])
        put(name, "separable", (ku, kv), [np.asarray(tu, np.float64), np.asarray(tv, np.float64)], coefs)

    for _ in range(400):
        tu, tv = knot_vector(rng, 4, 6), knot_vector(rng, 3, 5)
        p, q = rng.standard_normal(6), rng.standard_normal(5)
        eu, ev = conditioned_1d(4, tu, p), conditioned_1d(3, tv, q)
        if eu is not None and ev is not None and len(eu["brackets"]) >= 2 and len(ev["brackets"]) >= 2:
            separable("sep_43", 4, tu, p, 3, tv, q)
            break
    else:
        raise AssertionError("sep_43: no well conditioned draw")
    # roots of p at 0.125 and at the knot 0.5; roots of q at the end 0 and at the knot 0.5: (0.125, 0) and (0.5, 0) lie on the
    # domain boundary, (0.125, 0.5) on a knot line, (0.5, 0.5) at the corner of four cells
    separable("sep_knots_22", 2, [0, 0, 0.25, 0.5, 0.75, 1, 1], [1.0, -1.0, 0.0, 1.0, 1.0], 2, [0, 0, 0.25, 0.5, 1, 1], [0.0, 1.0, 0.0, -1.0])

    for _ in range(400):                                                 # cubic minus line, on a grid so that all is exact
        ka = knot_vector(rng, 4, 7)
        a = np.round(rng.standard_normal((2, 7)) * 512) / 1024
        p0, d = np.round(rng.standard_normal(2) * 256) / 1024, np.round(rng.standard_normal(2) * 1024) / 1024
        if not d.any():
            continue
        normal = np.array([-d[1], d[0]])
        line = normal @ (a - p0[:, None])
        e = conditioned_1d(4, ka, line)
        if e is None or not e["brackets"]:
            continue
        vs = []
        for lo, hi in e["brackets"]:
            u = (lo + hi) / 2
            at = [zeros_ref.value(4, ka, a[k], u) for k in range(2)]
            vs.append(float(sum(Fraction(float(d[k])) * (at[k] - Fraction(float(p0[k]))) for k in range(2))
                            / sum(Fraction(float(x)) ** 2 for x in d)))
        if any(abs(v) < 1e-3 or abs(v - 1.0) < 1e-3 for v in vs) or sum(0.0 < v < 1.0 for v in vs) < 2:
            continue
        b = np.stack([p0, p0 + d], axis=1)
        put("cubic_minus_line", "line", (4, 2), [ka, np.array([0.0, 0.0, 1.0, 1.0])], a[:, :, None] - b[:, None, :],
            line=(4, ka, line), inside=[0.0 < v < 1.0 for v in vs], v=vs)
        break
    else:
        raise AssertionError("cubic_minus_line: no well conditioned draw")

    # one zero cell: component 0 vanishes on the first cell; component 1 is positive there and around it
    knots = [knot_vector(rng, 4, 7), knot_vector(rng, 4, 7)]
    coefs = rng.standard_normal((2, 7, 7))
    coefs[0, :4, :4] = 0.0
    coefs[1] = np.abs(coefs[1]) + 0.1
    coefs[1, 5:, 5:] = -coefs[1, 5:, 5:]
    put("zero_one_cell", "zero", (4, 4), knots, coefs)
    # (u - v, (u - 1/2)^2): the parabola (u, (u - 1/2)^2) touches the line (v, 0) at u = v = 1/2
    bez = [[0, 0, 0, 1, 1, 1.0], [0, 0, 1, 1.0]]
    put("tangent", "tangent", (3, 2), bez, [[[0.0, -1.0], [0.5, -0.5], [1.0, 0.0]], [[0.25, 0.25], [-0.25, -0.25], [0.25, 0.25]]])
    # u - v and u - v - 1/20: two parallel lines
    lin = [[0, 0, 1, 1.0], [0, 0, 1, 1.0]]
    put("empty", "empty", (2, 2), lin, [[[0.0, -1.0], [1.0, 0.0]], [[-0.05, -1.05], [0.95, -0.05]]])
    return out


def exact_of(c):
    """(exact_uv sorted, extra arrays) of a case."""
    order, knots, coefs = c["order"], c["knots"], c["coefs"]
    extra = {}
    if c["kind"] in ("coupled", "zero", "empty"):
        exact = zeros2_ref.zeros(order, knots, coefs)
        uv = [(float(z["t0"][0] + z["x"] * z["h"][0]), float(z["t0"][1] + z["y"] * z["h"][1])) for z in exact]
        if c["kind"] in ("coupled", "zero"):
            extra = dict(cert_cell=np.array([z["cell"] for z in exact], np.int32).reshape(-1, 2),
                         cert_xy=np.array([[float(z["x"]), float(z["y"])] for z in exact]).reshape(-1, 2),
                         cert_radius=np.array([float(z["radius"]) for z in exact]),
                         cert_Y=np.array([[[float(v) for v in row] for row in z["Y"]] for z in exact]).reshape(-1, 2, 2))
    elif c["kind"] == "separable":
        eu, us = one_d("u", order[0], knots[0], coefs[0][:, 0])
        ev, vs = one_d("v", order[1], knots[1], coefs[1][0, :])
        extra = {**eu, **ev}
        uv = [(u, v) for u in us for v in vs]
    elif c["kind"] == "line":
        eu, us = one_d("u", *c["line"])
        keep = np.array(c["inside"], bool)
        extra = {key: (val[keep] if key in ("u_lo", "u_hi", "u_fprime") else val) for key, val in eu.items()}
        uv = [(u, v) for u, v, k in zip(us, c["v"], keep) if k]
    else:
        uv = []
    uv = np.array(sorted(uv), np.float64).reshape(-1, 2)
    b0, b1, _ = zeros2_ref.bezier_cells(order, knots, coefs) if c["kind"] == "zero" else (None, None, None)
    cells = [[float(b0[i]), float(b0[i + 1]), float(b1[j]), float(b1[j + 1])] for i, j in zeros2_ref.zero_cells(order, knots, coefs)] \
        if c["kind"] == "zero" else []
    return uv, dict(extra, exact_cells=np.array(cells, np.float64).reshape(-1, 4))


SEMANTICS = [
    ("nind_ne_ndep", dict(order=[2, 2], knots=[[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]], coefs=[[[1.0, -2.0], [0.5, 1.0]]])),
    ("no_zeros", dict(order=[2, 2], knots=[[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]],
                      coefs=[[[1.0, 2.0], [0.5, 1.0]], [[1.0, -2.0], [0.5, 1.0]]])),
    ("one_zero", dict(order=[2, 2], knots=[[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]],
                      coefs=[[[-0.25, -0.25], [0.75, 0.75]], [[-0.5, 0.5], [-0.5, 0.5]]])),
]


def main():
    bspy = load_reference()
    out, counted = {}, []
    for name, c in cases().items():
        uv, extra = exact_of(c)
        n0, n1 = c["coefs"].shape[1:]
        spline = bspy.Spline(2, 2, c["order"], [n0, n1], c["knots"], c["coefs"])
        try:
            found = [r for r in spline.zeros() if not isinstance(r, tuple)]
            error = None
        except Exception as e:                                          # recorded: the tests do not follow it
            found, error = [], f"{type(e).__name__}: {e}"
        ref = np.array(sorted((float(r[0]), float(r[1])) for r in found), np.float64).reshape(-1, 2)
        dev = float(np.abs(ref - uv).max()) if len(ref) == len(uv) and len(uv) else float("nan")
        complete = error is None and len(ref) == len(uv) and (len(uv) == 0 or dev <= 1e-6)
        if c["kind"] in ("coupled", "separable", "line"):
            counted.append(complete)
        print(f"{name}: {len(uv)} zeros; reference {len(ref)}, complete {complete}, ref_dev {dev:.3e} {error or ''}", flush=True)
        rec = dict(order=np.array(c["order"], np.int32), knots0=c["knots"][0], knots1=c["knots"][1], coefs=c["coefs"],
                   kind=np.array(c["kind"]), exact_uv=uv, ref_roots=ref, ref_complete=np.array(bool(complete)), ref_dev=np.float64(dev), **extra)
        for key, val in rec.items():
            out[f"{name}/{key}"] = val
    good = sum(counted)
    assert 4 * good >= 3 * len(counted), f"the reference is complete on only {good} of {len(counted)} coupled, separable and line cases"
    print(f"the reference is complete on {good} of {len(counted)} coupled, separable and line cases")

    records = []
    for name, s in SEMANTICS:
        coefs = np.array(s["coefs"])
        spline = bspy.Spline(2, len(coefs), s["order"], list(coefs.shape[1:]), [np.array(k) for k in s["knots"]], coefs)
        record = dict(name=name, spline=s, error=None, result=None)
        try:
            record["result"] = sorted([float(r[0]), float(r[1])] for r in spline.zeros())
        except ValueError as e:
            record["error"] = str(e)
        print(f"{name}: {record['error']!r} {record['result']}")
        records.append(record)

    path = os.path.join(HERE, "roots2.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "roots2_semantics.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
