"""
Golden values of ``zeros`` for scalar curves.  Runs ONLY where the reference checkout is importable (see
make_golden.load_reference).  The outputs:

``roots.npz``, per case: the inputs; the exact roots of tests/zeros_ref.py (rational arithmetic: brackets of width
eps (b - a) / 16 or less, rounded to float64, with f' at each, and the zero intervals); what the reference returned (its
scalar roots and its intervals); ``ref_complete``: whether the reference returned as many roots and intervals as there
are; ``ref_dev``: the largest distance of a reference root from the exact bracket it belongs to (nearest bracket when
the counts differ; nan when the reference returned none or raised).  The reference's recursion loses roots now and
then, and next to a zero interval it returns stray roots; such cases are kept on purpose and the tests pin them to the
exact result only.  So that the comparison with the reference cannot become empty, the generator refuses to write unless
``ref_complete`` holds on at least three quarters of the simple-root cases.

Every simple-root case is well conditioned, which the generator asserts: |f'(r)| (b - a) >= 1e-3 S at every exact root
and neighbouring roots at least 1e-6 (b - a) apart, S = max |coefficient|.  The accuracy bar of the tests is then a
first-order statement.

``roots_semantics.json``: the messages and small outcomes.

    python tests/golden/make_golden_roots.py

npz keys: ``<case>/order``, ``<case>/knots``, ``<case>/coefs``, ``<case>/kind`` ("simple", "knot", "touch", "zero",
"jump"), ``<case>/exact_lo``, ``<case>/exact_hi``, ``<case>/exact_fprime``, ``<case>/exact_intervals`` (n x 2),
``<case>/ref_roots``, ``<case>/ref_intervals`` (n x 2), ``<case>/ref_complete``, ``<case>/ref_dev``.
"""
import json
import os
import sys
from fractions import Fraction
from math import comb

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
from make_golden_refine import knot_vector  # noqa: E402
import zeros_ref  # noqa: E402


def conditioned(order, knots, coefs):
    """The exact roots when every one is simple and well conditioned, else None."""
    try:
        exact = zeros_ref.roots(order, knots, coefs)
    except ArithmeticError:
        return None
    k = int(order)
    width = float(knots[len(knots) - k]) - float(knots[k - 1])
    mids = [float(lo + hi) / 2 for lo, hi in exact["brackets"]]
    if any(abs(float(d)) * width < 1e-3 * exact["scale"] for d in exact["fprime"]):
        return None
    if any(b - a < 1e-6 * width for a, b in zip(mids[:-1], mids[1:])):
        return None
    return exact


def chebyshev_bernstein(degree):
    """Bernstein coefficients on [0, 1] of T_degree(2 x - 1), rounded once."""
    prev, cur = [Fraction(1)], [Fraction(-1), Fraction(2)]              # T0, T1 of 2x - 1 in powers of x
    for _ in range(degree - 1):
        nxt = [Fraction(0)] * (len(cur) + 1)
        for i, a in enumerate(cur):
            nxt[i] += -2 * a
            nxt[i + 1] += 4 * a
        for i, a in enumerate(prev):
            nxt[i] -= a
        prev, cur = cur, nxt
    n = degree
    return np.array([float(sum(Fraction(comb(i, j), comb(n, j)) * cur[j] for j in range(i + 1))) for i in range(n + 1)])


def cases():
    rng = np.random.default_rng(20250803)
    out = {}

    def put(name, kind, order, knots, coefs):
        out[name] = dict(kind=kind, order=int(order), knots=np.asarray(knots), coefs=np.asarray(coefs))

    def random_curve(name, order, ncoef, dtype=np.float64, kdtype=np.float64, signs=None, **kw):
        for _ in range(200):
            knots = knot_vector(rng, order, ncoef, **kw).astype(kdtype)
            coefs = rng.standard_normal(ncoef)
            if signs is not None:
                coefs = np.abs(coefs) * np.array(signs, np.float64)
            coefs = coefs.astype(dtype)
            if conditioned(order, knots, coefs) is not None:
                return put(name, "simple", order, knots, coefs)
        raise AssertionError(f"{name}: no well conditioned draw")

    # the reference lost a root on a curve with these signs; whether it does here is recorded, not assumed
    random_curve("rand_o2_9", 2, 9, signs=[-1, 1, -1, -1, 1, 1, 1, 1, -1])
    random_curve("rand_o3_20", 3, 20)
    random_curve("rand_o4_50", 4, 50)
    random_curve("rand_o4_200", 4, 200)
    random_curve("rand_o5_30", 5, 30)
    random_curve("rand_o6_40", 6, 40)
    random_curve("rand_o8_25", 8, 25)
    random_curve("double_knot_o4", 4, 16, repeat=(3,))
    random_curve("unclamped_o4", 4, 14, unclamped=True)
    random_curve("shifted_2_5_o4", 4, 18, lo=2.0, hi=5.0)
    random_curve("shifted_m3000_o3", 3, 15, lo=-3000.0, hi=-2999.0)
    random_curve("f32_coefs_o4", 4, 20, dtype=np.float32)
    random_curve("f32_knots_o3", 3, 16, kdtype=np.float32)
    put("chebyshev_o6", "simple", 6, [0.0] * 6 + [1.0] * 6, chebyshev_bernstein(5))
    assert conditioned(6, out["chebyshev_o6"]["knots"], out["chebyshev_o6"]["coefs"]) is not None

    put("zero_at_c0_knot", "knot", 3, [0, 0, 0, 0.5, 0.5, 1, 1, 1.0], [1.0, 0.5, 0.0, -0.75, -1.0])
    put("touch", "touch", 3, [0, 0, 0, 1, 1, 1.0], [0.25, -0.25, 0.25])
    put("touch_raised", "touch", 3, [0, 0, 0, 1, 1, 1.0], [0.25 + 1e-9, -0.25 + 1e-9, 0.25 + 1e-9])
    knots = knot_vector(rng, 4, 16)
    coefs = rng.standard_normal(16)
    coefs[5:10] = 0.0
    put("zero_one_run", "zero", 4, knots, coefs)
    knots = knot_vector(rng, 4, 24)
    coefs = rng.standard_normal(24)
    coefs[4:8] = 0.0
    coefs[13:19] = 0.0
    put("zero_two_runs", "zero", 4, knots, coefs)
    put("jump_opposite_signs", "jump", 3, [0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1.0], [1.0, 2.0, 1.5, -1.0, -2.0, 0.5])
    return out


def distance(r, bracket):
    lo, hi = bracket
    return max(0.0, float(lo) - r, r - float(hi))


SEMANTICS = [
    ("nind_ne_ndep", dict(order=[2], knots=[[0.0, 0.0, 0.5, 1.0, 1.0]], coefs=[[1.0, -2.0, 4.0], [0.0, 1.0, 0.5]])),
    ("zero_interval", dict(order=[2], knots=[[0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.0]], coefs=[[1.0, 0.0, 0.0, 0.0, 2.0]])),
    ("touch", dict(order=[3], knots=[[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]], coefs=[[0.25, -0.25, 0.25]])),
    ("root_at_knot", dict(order=[2], knots=[[0.0, 0.0, 0.5, 1.0, 1.0]], coefs=[[1.0, 0.0, -1.0]])),
    ("no_roots", dict(order=[3], knots=[[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]], coefs=[[1.0, 2.0, 0.5]])),
]


def main():
    bspy = load_reference()
    out, simple = {}, []
    for name, c in cases().items():
        exact = zeros_ref.roots(c["order"], c["knots"], c["coefs"])
        spline = bspy.Spline(1, 1, [c["order"]], [len(c["coefs"])], [c["knots"]], [c["coefs"]])
        try:
            found = list(spline.zeros())
            error = None
        except Exception as e:                                          # recorded: the tests do not follow it
            found, error = [], f"{type(e).__name__}: {e}"
        ref_roots = np.array([float(r) for r in found if not isinstance(r, tuple)], np.float64)
        ref_intervals = np.array([[float(r[0]), float(r[1])] for r in found if isinstance(r, tuple)], np.float64).reshape(-1, 2)
        brackets = exact["brackets"]
        complete = error is None and len(ref_roots) == len(brackets) and len(ref_intervals) == len(exact["intervals"])
        if len(ref_roots) and brackets:
            pairs = zip(ref_roots, brackets) if len(ref_roots) == len(brackets) else \
                ((r, min(brackets, key=lambda b: distance(r, b))) for r in ref_roots)
            dev = max(distance(float(r), b) for r, b in pairs)
        else:
            dev = float("nan")
        if c["kind"] == "simple":
            simple.append(complete)
        print(f"{name}: {len(brackets)} roots, {len(exact['intervals'])} intervals; reference {len(ref_roots)} roots, "
              f"{len(ref_intervals)} intervals, complete {complete}, ref_dev {dev:.3e} {error or ''}", flush=True)
        out[f"{name}/order"] = np.array(c["order"], np.int32)
        out[f"{name}/knots"] = c["knots"]
        out[f"{name}/coefs"] = c["coefs"]
        out[f"{name}/kind"] = np.array(c["kind"])
        out[f"{name}/exact_lo"] = np.array([float(lo) for lo, _ in brackets], np.float64)
        out[f"{name}/exact_hi"] = np.array([float(hi) for _, hi in brackets], np.float64)
        out[f"{name}/exact_fprime"] = np.array([float(d) for d in exact["fprime"]], np.float64)
        out[f"{name}/exact_intervals"] = np.array(exact["intervals"], np.float64).reshape(-1, 2)
        out[f"{name}/ref_roots"] = ref_roots
        out[f"{name}/ref_intervals"] = ref_intervals
        out[f"{name}/ref_complete"] = np.array(bool(complete))
        out[f"{name}/ref_dev"] = np.float64(dev)
    good = sum(simple)
    assert 4 * good >= 3 * len(simple), f"the reference is complete on only {good} of {len(simple)} simple-root cases"
    print(f"the reference is complete on {good} of {len(simple)} simple-root cases")

    records = []
    for name, s in SEMANTICS:
        ndep = len(s["coefs"])
        spline = bspy.Spline(1, ndep, s["order"], [len(s["coefs"][0])], [np.array(k) for k in s["knots"]], np.array(s["coefs"]))
        record = dict(name=name, spline=s, error=None, result=None)
        try:
            record["result"] = [[float(r[0]), float(r[1])] if isinstance(r, tuple) else float(r) for r in spline.zeros()]
        except ValueError as e:
            record["error"] = str(e)
        print(f"{name}: {record['error']!r} {record['result']}")
        records.append(record)

    path = os.path.join(HERE, "roots.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "roots_semantics.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
