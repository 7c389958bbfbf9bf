"""
Golden values of remove_knot and remove_knots.  Runs ONLY where the reference checkout is importable (see
make_golden.load_reference).  The outputs:

``remove.npz``

  ``knot/<case>/...``   remove_knot: ``order``, ``knots``, ``coefs`` (nDep, nCoef), ``iKnot``, ``nLeft``, ``nRight`` and
                        what the reference returned: ``out_knots``, ``out_coefs``, ``residual``.  The generator asserts
                        that every exact operator weight (tests/remove_ref.py) is at most 1e3 in magnitude, so that the
                        parity bar of the tests is a statement about rounding and not about conditioning.
  ``recover/<case>/...`` insert-then-remove: ``order``, ``knots<iv>``, ``coefs`` of a spline, ``new<iv>`` the knots
                        inserted into it, ``in_knots<iv>``, ``in_coefs`` the reference's result of that insertion (the
                        input of remove_knots), ``ref_ncoef`` what the reference's remove_knots(1e-12) is left with.
                        The expected result is the original knots.
  ``reduce/<case>/...`` tolerance cases: ``order``, ``knots<iv>``, ``coefs``, ``tolerance`` and ``ref_ncoef``, the
                        nCoef of the reference's remove_knots(tolerance), ``ref_seconds`` its time here.

``remove_semantics.json``: the messages of the reference's ValueErrors.

    python tests/golden/make_golden_remove.py
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
from make_golden_refine import knot_vector, inside  # noqa: E402
import remove_ref  # noqa: E402

TOLERANCES = (1e-2, 1e-3, 1e-5, 1e-8)


def knot_cases():
    rng = np.random.default_rng(20250301)
    out = {}

    def add(name, order, ncoef, ndep, iKnot, nLeft=0, nRight=0, dtype=np.float64, lo=0.0, hi=1.0, scale=1.0, **kw):
        t = knot_vector(rng, order, ncoef, lo=lo, hi=hi, **kw).astype(dtype)
        c = (scale * (rng.standard_normal((ndep, ncoef)) + 0.3)).astype(dtype)
        out[name] = dict(order=order, knots=t, coefs=c, iKnot=iKnot if iKnot >= 0 else ncoef + iKnot, nLeft=nLeft, nRight=nRight)

    for k in range(2, 8):
        n = 3 * k + 4
        add(f"o{k}_middle", k, n, 2, n // 2, kind="jittered")
        add(f"o{k}_first", k, n, 2, k)
        add(f"o{k}_last", k, n, 3, -1, kind="jittered")
    # double knots: the jittered vectors repeat interior positions 1 and 3 (knot indices k + 1, k + 2 and k + 4, k + 5)
    for k in (3, 4, 6):
        n = 2 * k + 7
        add(f"o{k}_double_a", k, n, 2, k + 1, kind="jittered", repeat=(1, 3))
        add(f"o{k}_double_b", k, n, 2, k + 2, kind="jittered", repeat=(1, 3))
        add(f"o{k}_double_first", k, n, 2, k, kind="jittered", repeat=(0,))
        add(f"o{k}_double_last", k, n, 2, -1, kind="jittered", repeat=(n - k - 2,))
    # fixed coefficients at the ends
    for k in (3, 4, 5):
        n = 2 * k + 5
        for nl in (1, 2):
            add(f"o{k}_left{nl}_first", k, n, 2, k, nLeft=nl, kind="jittered")
            add(f"o{k}_left{nl}_second", k, n, 2, k + 1, nLeft=nl, kind="jittered")
            add(f"o{k}_right{nl}_last", k, n, 2, -1, nRight=nl, kind="jittered")
            add(f"o{k}_right{nl}_before_last", k, n, 2, -2, nRight=nl, kind="jittered")
        add(f"o{k}_both_far", k, 3 * k + 6, 2, (3 * k + 6) // 2, nLeft=2, nRight=2, kind="jittered")
    # float32 coefficients and knots
    add("f32_o4", 4, 14, 3, 8, dtype=np.float32, kind="jittered")
    add("f32_o3_left1", 3, 11, 2, 3, nLeft=1, dtype=np.float32, kind="jittered")
    add("f32_o6_last", 6, 20, 2, -1, dtype=np.float32, kind="jittered")
    # away from unit scale: a shifted, short domain and large coefficients
    add("shifted_o4", 4, 15, 2, 9, lo=1e3, hi=1e3 + 1e-2, scale=1e6, kind="jittered")
    add("shifted_o5_right1", 5, 16, 2, -1, nRight=1, lo=1e3, hi=1e3 + 1e-2, scale=1e6, kind="jittered")
    add("shifted_o3_double", 3, 13, 2, 5, lo=1e3, hi=1e3 + 1e-2, scale=1e6, kind="jittered", repeat=(1, 3))
    return out


def greville(t, k):
    n = len(t) - k
    return np.array([t[i + 1:i + k].mean() for i in range(n)]) if k > 1 else 0.5 * (t[:n] + t[1:n + 1])


def uniform_knots(k, n):
    return np.concatenate((k * [0.0], np.linspace(0.0, 1.0, n - k + 2)[1:-1], k * [1.0]))


def shape_functions(g):
    return np.sin(3.0 * g), np.exp(-30.0 * (g - 0.4) ** 2)


def recover_cases():
    rng = np.random.default_rng(20250302)
    out = {}

    def add(name, orders, ncoefs, ndep, counts, dtype=np.float64):
        knots = [knot_vector(rng, k, n, kind="jittered").astype(dtype) for k, n in zip(orders, ncoefs)]
        coefs = (rng.standard_normal((ndep, *ncoefs)) + 0.3).astype(dtype)
        new = [inside(rng, t, k, c) for t, k, c in zip(knots, orders, counts)]
        out[name] = dict(order=list(orders), knots=knots, coefs=coefs, new=new)

    for k in range(2, 7):
        add(f"curve_o{k}", (k,), (2 * k + 6,), 2, (5,))
    add("surface_o43", (4, 3), (10, 8), 3, (4, 3))
    add("volume_o323", (3, 2, 3), (6, 5, 4), 2, (2, 2, 1))
    return out


def reduce_cases():
    out = {}
    for n in (40, 120):
        t = uniform_knots(4, n)
        coefs = np.stack(shape_functions(greville(t, 4)))
        for tol in TOLERANCES:
            out[f"curve_{n}_{tol:.0e}"] = dict(order=[4], knots=[t], coefs=coefs, tolerance=tol)
    tu, tv = uniform_knots(4, 20), uniform_knots(4, 16)
    su, eu = shape_functions(greville(tu, 4))
    sv, ev = shape_functions(greville(tv, 4))
    out["surface_20x16_1e-03"] = dict(order=[4, 4], knots=[tu, tv], coefs=np.stack((np.outer(su, ev), np.outer(eu, sv))), tolerance=1e-3)
    return out


CURVE = dict(order=[3], knots=[[0.0, 0.0, 0.0, 0.25, 0.5, 0.5, 0.75, 1.0, 1.0, 1.0]], coefs=[[1.0, 2.0, 0.5, -1.0, 3.0, 2.0, 0.0]])
SURFACE = dict(order=[2, 3], knots=[[0.0, 0.0, 0.5, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]],
               coefs=[[[0.0, 1.0, 2.0], [1.0, 3.0, 2.0], [0.5, 0.0, 1.0]]])


def semantics():
    return [
        ("remove_knot_surface", SURFACE, [2]),
        ("remove_knot_below", CURVE, [2]),
        ("remove_knot_above", CURVE, [7]),
        ("remove_knot_first", CURVE, [3]),
        ("remove_knot_last", CURVE, [6]),
    ]


def main():
    bspy = load_reference()

    def make(order, knots, coefs):
        ncoef = np.shape(coefs)[1:]
        return bspy.Spline(len(order), np.shape(coefs)[0], order, ncoef, [np.array(k) for k in knots], np.array(coefs))

    out = {}
    for name, c in knot_cases().items():
        k, t = c["order"], c["knots"]
        W = remove_ref.removal_rows(t, k, c["iKnot"], c["nLeft"], c["nRight"])
        largest = max(abs(float(v)) for row in W for v in row)
        assert largest <= 1e3, f"{name}: an exact operator weight is {largest:.3e}"
        spline = make([k], [t], c["coefs"])
        r, residual = spline.remove_knot(c["iKnot"], c["nLeft"], c["nRight"])
        assert r.coefs.dtype == c["coefs"].dtype and np.all(np.isfinite(r.coefs)), name
        print(f"knot/{name}: iKnot {c['iKnot']} largest weight {largest:.2e} residual {np.max(residual):.3e}", flush=True)
        for key in ("order", "iKnot", "nLeft", "nRight"):
            out[f"knot/{name}/{key}"] = np.int32(c[key])
        out[f"knot/{name}/knots"] = t
        out[f"knot/{name}/coefs"] = c["coefs"]
        out[f"knot/{name}/out_knots"] = np.asarray(r.knots[0])
        out[f"knot/{name}/out_coefs"] = np.asarray(r.coefs)
        out[f"knot/{name}/residual"] = np.asarray(residual)

    for name, c in recover_cases().items():
        spline = make(c["order"], c["knots"], c["coefs"])
        refined = spline.insert_knots(c["new"])
        back = refined.remove_knots(1e-12)
        print(f"recover/{name}: nCoef {tuple(spline.nCoef)} -> {tuple(refined.nCoef)} -> reference {tuple(back.nCoef)}", flush=True)
        out[f"recover/{name}/order"] = np.array(c["order"], np.int32)
        out[f"recover/{name}/coefs"] = c["coefs"]
        out[f"recover/{name}/in_coefs"] = np.asarray(refined.coefs)
        out[f"recover/{name}/ref_ncoef"] = np.array(back.nCoef, np.int32)
        for iv in range(len(c["order"])):
            out[f"recover/{name}/knots{iv}"] = c["knots"][iv]
            out[f"recover/{name}/new{iv}"] = np.array(c["new"][iv], np.float64)
            out[f"recover/{name}/in_knots{iv}"] = np.asarray(refined.knots[iv])

    for name, c in reduce_cases().items():
        spline = make(c["order"], c["knots"], c["coefs"])
        start = time.perf_counter()
        r = spline.remove_knots(c["tolerance"])
        seconds = time.perf_counter() - start
        print(f"reduce/{name}: nCoef {tuple(spline.nCoef)} -> reference {tuple(r.nCoef)} in {seconds:.2f} s", flush=True)
        out[f"reduce/{name}/order"] = np.array(c["order"], np.int32)
        out[f"reduce/{name}/coefs"] = c["coefs"]
        out[f"reduce/{name}/tolerance"] = np.float64(c["tolerance"])
        out[f"reduce/{name}/ref_ncoef"] = np.array(r.nCoef, np.int32)
        out[f"reduce/{name}/ref_seconds"] = np.float64(seconds)
        for iv in range(len(c["order"])):
            out[f"reduce/{name}/knots{iv}"] = c["knots"][iv]

    records = []
    for name, s, args in semantics():
        spline = make(s["order"], s["knots"], s["coefs"])
        record = dict(name=name, spline=s, args=args, error=None)
        try:
            spline.remove_knot(*args)
        except ValueError as e:
            record["error"] = str(e)
        print(f"{name}: {record['error']!r}")
        records.append(record)

    path = os.path.join(HERE, "remove.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "remove_semantics.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
