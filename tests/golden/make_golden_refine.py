"""
Golden values of insert_knots, elevate, elevate_and_insert_knots, trim, clamp and differentiate.  Runs ONLY where the
reference checkout is importable (see make_golden.load_reference).  The outputs:

``refine.npz``, per case: the inputs, the knots and coefficients the reference returned, and ``ref_dev``: the largest
difference, relative to max |coef|, between the reference's coefficients and the exact result of tests/refine_ref.py
(rational arithmetic, rounded once to the coefficients' dtype), over the entries that exist there (refine_ref.py:
basis functions with a cell inside the domain).  The reference's elevation differentiates to order k - 1 and integrates
back, which loses accuracy on uneven knots and large orders; three such cases ("bad_*") are kept on purpose, the tests
pin them to the exact result only.  So that ref_dev cannot turn the comparison with the reference into nothing, the
generator refuses to write unless at least half of the cases of every operation have ref_dev <= 1e-12.

``refine_semantics.json``: what the reference does with small inputs that raise or change nothing - the message of its
ValueError, or whether it returned the spline itself.

    python tests/golden/make_golden_refine.py

npz keys: ``<case>/op``, ``<case>/order``, ``<case>/knots<iv>``, ``<case>/coefs``; arguments ``<case>/new<iv>`` (n x 2:
knot, multiplicity) with ``<case>/pair<iv>`` (whether the entry is passed as a pair or a scalar), ``<case>/m``,
``<case>/domain`` (nInd x 2, nan = None), ``<case>/left``, ``<case>/right``, ``<case>/wrt``; results
``<case>/out_order``, ``<case>/out_knots<iv>``, ``<case>/out_coefs``, ``<case>/ref_dev``.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
import refine_ref  # noqa: E402

OPS = ("insert_knots", "elevate", "elevate_and_insert_knots", "trim", "clamp", "differentiate")


def knot_vector(rng, order, ncoef, kind="random", lo=0.0, hi=1.0, repeat=(), unclamped=False):
    """kind: "random" or "jittered" interior knots; repeat: interior positions (indices) whose knot is doubled;
    unclamped: simple knots all the way, the domain is the middle."""
    if unclamped:
        n = order + ncoef
        t = np.linspace(lo - 0.4 * (hi - lo), hi + 0.4 * (hi - lo), n)
        t[1:-1] += (rng.random(n - 2) - 0.5) * 0.5 * (t[1] - t[0])
        return t
    n_int = ncoef - order
    n_distinct = n_int - len(repeat)
    if kind == "random":
        interior = np.sort(lo + (hi - lo) * rng.random(n_distinct))
    else:
        interior = np.linspace(lo, hi, n_distinct + 2)[1:-1]
        interior += (rng.random(n_distinct) - 0.5) * 0.6 * (hi - lo) / (n_distinct + 1)
    reps = np.ones(n_distinct, int)
    reps[list(repeat)] += 1
    return np.concatenate((order * [lo], np.repeat(interior, reps), order * [hi]))


def spline_data(rng, orders, ncoefs, ndep, dtype=np.float64, **kw):
    knots = [knot_vector(rng, k, n, **kw).astype(dtype) for k, n in zip(orders, ncoefs)]
    coefs = (rng.standard_normal((ndep, *ncoefs)) + 0.3).astype(dtype)
    return dict(order=list(orders), knots=knots, coefs=coefs)


def inside(rng, t, order, count):
    """`count` new knots strictly inside the domain of t, away from its knots."""
    lo, hi = t[order - 1], t[len(t) - order]
    return [float(v) for v in lo + (hi - lo) * (0.02 + 0.96 * rng.random(count))]


def cases():
    rng = np.random.default_rng(20250117)
    out = {}

    def add(name, op, s, **args):
        out[name] = dict(op=op, **s, **args)

    # ---- insert_knots: entries are scalars or (knot, multiplicity)
    s = spline_data(rng, (4,), (12,), 2)
    t = s["knots"][0]
    add("ins_curve_o4", "insert_knots", s,
        new=[[*inside(rng, t, 4, 5), (float(t[6]), 3), (0.31, 2), (0.77, 0), (float(t[8]), 1), 0.31]])
    s = spline_data(rng, (3,), (14,), 3, repeat=(2, 5))
    add("ins_curve_o3_repeated", "insert_knots", s, new=[[*inside(rng, s["knots"][0], 3, 6), (float(s["knots"][0][3]), 2)]])
    s = spline_data(rng, (4, 3), (10, 8), 3, kind="jittered")
    add("ins_surface_o43", "insert_knots", s, new=[inside(rng, s["knots"][0], 4, 7), [*inside(rng, s["knots"][1], 3, 4), (0.5, 3)]])
    s = spline_data(rng, (3, 4), (7, 9), 2)
    add("ins_surface_last_only", "insert_knots", s, new=[[], inside(rng, s["knots"][1], 4, 6)])
    s = spline_data(rng, (3, 2, 3), (5, 6, 5), 2, kind="jittered")
    add("ins_volume_o323", "insert_knots", s, new=[inside(rng, s["knots"][0], 3, 3), [(0.4, 2), 0.9], inside(rng, s["knots"][2], 3, 4)])
    s = spline_data(rng, (4,), (11,), 2, unclamped=True)
    add("ins_unclamped_o4", "insert_knots", s, new=[inside(rng, s["knots"][0], 4, 6)])
    s = spline_data(rng, (6,), (30,), 2)
    add("ins_curve_o6", "insert_knots", s, new=[inside(rng, s["knots"][0], 6, 25)])
    s = spline_data(rng, (4, 4), (12, 9), 3, dtype=np.float32, kind="jittered")
    add("ins_f32_surface", "insert_knots", s, new=[inside(rng, s["knots"][0], 4, 5), inside(rng, s["knots"][1], 4, 5)])

    # ---- elevate
    add("elev_curve_o4_m1", "elevate", spline_data(rng, (4,), (14,), 2), m=[1])
    add("elev_curve_o3_m2", "elevate", spline_data(rng, (3,), (12,), 3, repeat=(3,)), m=[2])
    add("elev_curve_o4_m3", "elevate", spline_data(rng, (4,), (10,), 1, kind="jittered"), m=[3])
    add("elev_curve_o3_m2_b", "elevate", spline_data(rng, (3,), (16,), 2, kind="jittered"), m=[2])
    add("elev_surface_o43_m12", "elevate", spline_data(rng, (4, 3), (9, 8), 3, kind="jittered"), m=[1, 2])
    add("elev_surface_o34_m10", "elevate", spline_data(rng, (3, 4), (8, 7), 2), m=[1, 0])
    add("elev_volume_o333_m111", "elevate", spline_data(rng, (3, 3, 3), (5, 4, 5), 2, kind="jittered"), m=[1, 1, 1])
    add("elev_unclamped_o3_m1", "elevate", spline_data(rng, (3,), (10,), 2, unclamped=True), m=[1])
    add("elev_f32_surface", "elevate", spline_data(rng, (3, 3), (8, 7), 2, dtype=np.float32, kind="jittered"), m=[1, 1])
    add("bad_elev_o6_30_m1", "elevate", spline_data(rng, (6,), (30,), 2), m=[1])
    add("bad_elev_o4_300_m1", "elevate", spline_data(rng, (4,), (300,), 2), m=[1])

    # ---- elevate_and_insert_knots: plain new knots
    s = spline_data(rng, (4,), (12,), 2)
    add("eik_curve_o4_m1", "elevate_and_insert_knots", s, m=[1], new=[[*inside(rng, s["knots"][0], 4, 4), float(s["knots"][0][5])]])
    s = spline_data(rng, (3,), (10,), 2, kind="jittered")
    add("eik_curve_o3_m2", "elevate_and_insert_knots", s, m=[2], new=[[0.35, 0.35, *inside(rng, s["knots"][0], 3, 3)]])
    s = spline_data(rng, (3,), (12,), 3)
    add("eik_curve_o3_m0", "elevate_and_insert_knots", s, m=[0], new=[inside(rng, s["knots"][0], 3, 5)])
    s = spline_data(rng, (3, 4), (7, 8), 2, kind="jittered")
    add("eik_surface_o34_m11", "elevate_and_insert_knots", s, m=[1, 1], new=[inside(rng, s["knots"][0], 3, 3), inside(rng, s["knots"][1], 4, 2)])
    s = spline_data(rng, (3, 3), (6, 9), 2)
    add("eik_surface_o33_m20", "elevate_and_insert_knots", s, m=[2, 0], new=[[], inside(rng, s["knots"][1], 3, 4)])
    s = spline_data(rng, (3,), (9,), 2, unclamped=True)
    add("eik_unclamped_o3_m1", "elevate_and_insert_knots", s, m=[1], new=[inside(rng, s["knots"][0], 3, 3)])
    s = spline_data(rng, (5,), (200,), 2, kind="jittered")
    add("bad_eik_o5_200_m3", "elevate_and_insert_knots", s, m=[3], new=[inside(rng, s["knots"][0], 5, 20)])

    # ---- trim: None bounds, a bound on a knot, a bound within eps of a knot (from below and from above), interior bounds
    s = spline_data(rng, (4,), (12,), 2)
    t = s["knots"][0]
    add("trim_curve_none_left", "trim", s, domain=[[np.nan, 0.6180339]])
    add("trim_curve_none_right", "trim", s, domain=[[0.2718281, np.nan]])
    add("trim_curve_on_knots", "trim", s, domain=[[t[5], t[9]]])
    add("trim_curve_eps_below", "trim", s, domain=[[np.nextafter(t[5], 0.0), np.nextafter(t[9], 0.0)]])
    add("trim_curve_eps_above", "trim", s, domain=[[np.nextafter(t[5], 1.0), np.nextafter(t[9], 1.0)]])
    add("trim_curve_interior", "trim", s, domain=[[0.123456, 0.87654]])
    s = spline_data(rng, (3,), (12,), 2, repeat=(4,))
    t = s["knots"][0]
    add("trim_curve_on_double_knot", "trim", s, domain=[[t[7], 0.95]])
    s = spline_data(rng, (4, 3), (10, 9), 3, kind="jittered")
    add("trim_surface_mixed", "trim", s, domain=[[np.nan, np.nan], [0.21, 0.83]])
    add("trim_surface_both", "trim", s, domain=[[0.3, 0.7], [float(s["knots"][1][4]), np.nan]])
    s = spline_data(rng, (3, 3, 2), (5, 6, 4), 2, kind="jittered")
    add("trim_volume", "trim", s, domain=[[0.1, 0.9], [np.nan, 0.5], [0.25, 0.75]])
    s = spline_data(rng, (4,), (12,), 2, unclamped=True)
    add("trim_unclamped", "trim", s, domain=[[0.2, 0.7]])
    s = spline_data(rng, (4, 3), (9, 8), 2, dtype=np.float32, kind="jittered")
    add("trim_f32_surface", "trim", s, domain=[[0.15, 0.8], [0.3, 0.9]])

    # ---- clamp
    s = spline_data(rng, (4,), (11,), 2, unclamped=True)
    add("clamp_curve_both", "clamp", s, left=[0], right=[0])
    add("clamp_curve_left", "clamp", s, left=[0], right=[])
    s = spline_data(rng, (3, 4), (8, 9), 2, unclamped=True)
    add("clamp_surface_mixed", "clamp", s, left=[0, 1], right=[1])
    s = spline_data(rng, (3, 3), (7, 8), 2, dtype=np.float32, unclamped=True)
    add("clamp_f32_surface", "clamp", s, left=[1], right=[0])

    # ---- differentiate, in every variable
    add("diff_curve_o4", "differentiate", spline_data(rng, (4,), (12,), 3), wrt=0)
    add("diff_curve_o3_repeated", "differentiate", spline_data(rng, (3,), (12,), 2, repeat=(1, 4)), wrt=0)
    s = spline_data(rng, (4, 3), (9, 8), 3, kind="jittered")
    add("diff_surface_0", "differentiate", s, wrt=0)
    add("diff_surface_1", "differentiate", s, wrt=1)
    s = spline_data(rng, (3, 4, 3), (5, 6, 4), 2, kind="jittered")
    for iv in range(3):
        add(f"diff_volume_{iv}", "differentiate", s, wrt=iv)
    add("diff_unclamped", "differentiate", spline_data(rng, (4,), (10,), 2, unclamped=True), wrt=0)
    add("diff_f32_surface", "differentiate", spline_data(rng, (3, 4), (7, 8), 2, dtype=np.float32, kind="jittered"), wrt=1)
    return out


def call(spline, c):
    op = c["op"]
    if op == "insert_knots":
        return spline.insert_knots(c["new"])
    if op == "elevate":
        return spline.elevate(c["m"])
    if op == "elevate_and_insert_knots":
        return spline.elevate_and_insert_knots(c["m"], c["new"])
    if op == "trim":
        return spline.trim([[None if np.isnan(b) else b for b in bounds] for bounds in c["domain"]])
    if op == "clamp":
        return spline.clamp(c["left"], c["right"])
    return spline.differentiate(c["wrt"])


CURVE = dict(order=[3], knots=[[0.0, 0.0, 0.0, 0.25, 0.5, 0.5, 0.75, 1.0, 1.0, 1.0]], coefs=[[1.0, 2.0, 0.5, -1.0, 3.0, 2.0, 0.0]])
OPEN = dict(order=[3], knots=[[-0.2, -0.1, 0.0, 0.25, 0.5, 0.5, 0.75, 1.0, 1.1, 1.2]], coefs=[[1.0, 2.0, 0.5, -1.0, 3.0, 2.0, 0.0]])
SURFACE = dict(order=[2, 3], knots=[[0.0, 0.0, 0.5, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]],
               coefs=[[[0.0, 1.0, 2.0], [1.0, 3.0, 2.0], [0.5, 0.0, 1.0]]])
CONSTANT = dict(order=[1], knots=[[0.0, 0.5, 1.0]], coefs=[[1.0, 2.0]])
ABOVE = float(np.nextafter(0.5, 1.0))


def semantics():
    """(name, op, spline, args): small calls whose outcome is a message or an identity."""
    return [
        ("insert_wrong_length", "insert_knots", CURVE, [[[0.3], [0.4]]]),
        ("insert_outside_domain", "insert_knots", CURVE, [[[0.3, 1.5]]]),
        ("insert_below_domain", "insert_knots", OPEN, [[[-0.05]]]),
        ("insert_multiplicity", "insert_knots", CURVE, [[[0.5, 0.5]]]),
        ("insert_multiplicity_pair", "insert_knots", CURVE, [[[[0.25, 3]]]]),
        ("insert_accumulates", "insert_knots", CURVE, [[[[0.3, 2], 0.3, 0.3]]]),
        ("insert_nothing", "insert_knots", CURVE, [[[]]]),
        ("insert_skipped_pair", "insert_knots", CURVE, [[[[0.3, 0]]]]),
        ("insert_second_variable_fails", "insert_knots", SURFACE, [[[0.25], [2.0]]]),
        ("elevate_wrong_length", "elevate", CURVE, [[1, 1]]),
        ("elevate_negative", "elevate", CURVE, [[-1]]),
        ("elevate_nothing", "elevate", SURFACE, [[0, 0]]),
        ("eik_wrong_new_length", "elevate_and_insert_knots", SURFACE, [[1, 0], [[0.3]]]),
        ("eik_wrong_m_length", "elevate_and_insert_knots", SURFACE, [[1], [[], []]]),
        ("eik_nothing", "elevate_and_insert_knots", SURFACE, [[0, 0], [[], []]]),
        ("eik_negative_second", "elevate_and_insert_knots", SURFACE, [[1, -2], [[], []]]),
        ("trim_wrong_length", "trim", CURVE, [[[0.1, 0.9], [0.1, 0.9]]]),
        ("trim_three_bounds", "trim", CURVE, [[[0.1, 0.5, 0.9]]]),
        ("trim_outside_left", "trim", CURVE, [[[-0.5, 0.9]]]),
        ("trim_outside_right", "trim", CURVE, [[[0.1, 1.5]]]),
        ("trim_empty", "trim", CURVE, [[[0.6, 0.6]]]),
        ("trim_reversed", "trim", CURVE, [[[0.8, 0.3]]]),
        ("trim_nothing", "trim", CURVE, [[[None, None]]]),
        ("trim_whole_domain", "trim", CURVE, [[[0.0, 1.0]]]),
        ("trim_open_right_above_double_knot", "trim", OPEN, [[[None, ABOVE]]]),
        ("trim_open_whole_domain", "trim", OPEN, [[[0.0, 1.0]]]),
        ("clamp_clamped", "clamp", CURVE, [[0], [0]]),
        ("clamp_none", "clamp", OPEN, [[], []]),
        ("differentiate_negative", "differentiate", CURVE, [-1]),
        ("differentiate_too_large", "differentiate", SURFACE, [2]),
        ("differentiate_constant", "differentiate", CONSTANT, [0]),
    ]


def main():
    bspy = load_reference()

    def make(s):
        ncoef = np.shape(s["coefs"])[1:]
        return bspy.Spline(len(s["order"]), np.shape(s["coefs"])[0], s["order"], ncoef, [np.array(k) for k in s["knots"]],
                           np.array(s["coefs"]))

    out, devs = {}, {op: [] for op in OPS}
    for name, c in cases().items():
        spline = make(c)
        r = call(spline, c)
        assert r.coefs.dtype == c["coefs"].dtype, f"{name}: the reference changed the dtype"
        if c["op"] == "differentiate":
            exact, mask = refine_ref.differentiate(c["order"], c["knots"], c["coefs"], c["wrt"]), None
        else:
            exact, mask = refine_ref.change_basis(c["order"], c["knots"], c["coefs"], list(r.order), list(r.knots))
        got = np.asarray(r.coefs, np.float64)
        diff = np.abs(got - exact.astype(np.float64))
        if mask is not None:
            diff = diff[mask]
        dev = float(diff.max() / np.abs(exact[mask] if mask is not None else exact).max())
        devs[c["op"]].append((name, dev, c["coefs"].dtype))
        missing = 0 if mask is None else int((~mask).sum())
        print(f"{name}: nCoef {tuple(r.nCoef)} ref_dev {dev:.3e} entries outside the domain {missing}", flush=True)
        n = len(c["order"])
        out[f"{name}/op"] = np.array(c["op"])
        out[f"{name}/order"] = np.array(c["order"], np.int32)
        out[f"{name}/coefs"] = c["coefs"]
        for iv in range(n):
            out[f"{name}/knots{iv}"] = c["knots"][iv]
            out[f"{name}/out_knots{iv}"] = np.asarray(r.knots[iv])
            if "new" in c:
                entries = c["new"][iv]
                out[f"{name}/new{iv}"] = np.array([e if isinstance(e, tuple) else (e, 1) for e in entries], np.float64).reshape(-1, 2)
                out[f"{name}/pair{iv}"] = np.array([isinstance(e, tuple) for e in entries], bool)
        for key in ("m", "left", "right", "wrt"):
            if key in c:
                out[f"{name}/{key}"] = np.array(c[key], np.int32)
        if "domain" in c:
            out[f"{name}/domain"] = np.array(c["domain"], np.float64)
        out[f"{name}/out_order"] = np.array(r.order, np.int32)
        out[f"{name}/out_coefs"] = np.asarray(r.coefs)
        out[f"{name}/ref_dev"] = np.float64(dev)
    for op, rows in devs.items():
        good = sum(dev <= 1e-12 for _, dev, _ in rows)
        assert rows and 2 * good >= len(rows), f"{op}: only {good} of {len(rows)} cases have ref_dev <= 1e-12"
        print(f"{op}: {good} of {len(rows)} cases have ref_dev <= 1e-12")

    records = []
    for name, op, s, args in semantics():
        spline = make(s)
        record = dict(name=name, op=op, spline=s, args=args, error=None, is_self=False)
        try:
            record["is_self"] = getattr(spline, op)(*args) is spline
        except ValueError as e:
            record["error"] = str(e)
        print(f"{name}: {record['error']!r} is_self {record['is_self']}")
        records.append(record)

    path = os.path.join(HERE, "refine.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "refine_semantics.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
