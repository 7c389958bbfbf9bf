"""
Golden values of add, subtract, integrate and contract.  Runs ONLY where the reference checkout is importable (see
make_golden.load_reference).  The outputs:

``sum.npz``, per case: the inputs, the order, knots and coefficients the reference returned, and ``ref_dev``: the
largest difference, relative to max |exact coefficient|, between the reference's coefficients and the exact result of
tests/sum_ref.py (rational arithmetic, rounded once to the result's dtype).  ``add`` goes through the reference's
``common_basis``, whose elevation differentiates and integrates back and loses accuracy on many knots and on large order
differences; two such cases ("bad_*") are kept on purpose, the tests pin them to the exact result only.  So that ref_dev
cannot turn the comparison with the reference into nothing, the generator refuses to write unless at least half of the
float64 cases of every operation have ref_dev <= 1e-12.

``sum_semantics.json``: what the reference does with small calls whose outcome is a message, an identity or a small
result: the message of its ValueError, whether it returned the spline itself, else the result's orders, knots and
coefficients.

    python tests/golden/make_golden_sum.py

npz keys: ``<case>/op``, ``<case>/order``, ``<case>/knots<iv>``, ``<case>/coefs``; the second operand ``<case>/b_order``,
``<case>/b_knots<iv>``, ``<case>/b_coefs``; arguments ``<case>/pairs`` (n x 2; absent: indMap None), ``<case>/scalar``
(whether the entry was passed as one index), ``<case>/wrt``, ``<case>/uvw`` (nan = None); results ``<case>/out_order``,
``<case>/out_knots<iv>``, ``<case>/out_coefs``, ``<case>/ref_dev``.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
from make_golden_refine import knot_vector, spline_data  # noqa: E402
import sum_ref  # noqa: E402

OPS = ("add", "subtract", "integrate", "contract")


def cases():
    rng = np.random.default_rng(20250611)
    out = {}

    def put(name, op, s, other=None, **args):
        out[name] = dict(op=op, **s, other=other, **args)

    # ---- add / subtract: the mapped variables of the ordinary cases have at most 12 coefficients
    put("add_curve_o44", "add", spline_data(rng, (4,), (12,), 2), spline_data(rng, (4,), (9,), 2), pairs=[(0, 0)])
    put("add_curve_o34", "add", spline_data(rng, (3,), (10,), 3), spline_data(rng, (4,), (9,), 3, kind="jittered"), pairs=[0])
    put("add_surface_o43_43", "add", spline_data(rng, (4, 3), (9, 8), 3, kind="jittered"), spline_data(rng, (4, 3), (7, 9), 3),
        pairs=[(0, 0), (1, 1)])
    put("add_surface_o34_43", "add", spline_data(rng, (3, 4), (8, 7), 2), spline_data(rng, (4, 3), (7, 9), 2, kind="jittered"),
        pairs=[(0, 0), (1, 1)])
    put("add_partial_volume_surface", "add", spline_data(rng, (3, 2, 3), (5, 4, 6), 2, kind="jittered"),
        spline_data(rng, (3, 4), (6, 7), 2), pairs=[0, (2, 1)])
    put("add_outer", "add", spline_data(rng, (3,), (7,), 2), spline_data(rng, (4, 3), (6, 5), 2, unclamped=True), pairs=None)
    s = spline_data(rng, (4,), (11,), 2, unclamped=True)
    t = s["knots"][0]
    put("add_unclamped", "add", s, spline_data(rng, (3,), (8,), 2, lo=float(t[3]), hi=float(t[11])), pairs=[(0, 0)])
    a = spline_data(rng, (4,), (10,), 2)
    a["knots"][0][4:10] = [0.25, 0.5, 0.5, 0.5, 0.75, 0.875]
    b = spline_data(rng, (4,), (8,), 2)
    b["knots"][0][4:8] = [0.125, 0.5, 0.75, 0.75]
    put("add_shared_knot", "add", a, b, pairs=[(0, 0)])
    put("add_f32_surface", "add", spline_data(rng, (3, 4), (8, 7), 2, dtype=np.float32, kind="jittered"),
        spline_data(rng, (4, 3), (7, 9), 2, dtype=np.float32), pairs=[(0, 0), (1, 1)])
    put("add_f32_f64", "add", spline_data(rng, (3,), (9,), 2, dtype=np.float32, kind="jittered"), spline_data(rng, (4,), (8,), 2),
        pairs=[(0, 0)])
    put("sub_curve_o44", "subtract", spline_data(rng, (4,), (11,), 2, kind="jittered"), spline_data(rng, (4,), (10,), 2), pairs=[(0, 0)])
    put("sub_surface_curve", "subtract", spline_data(rng, (3, 4), (7, 8), 3), spline_data(rng, (4,), (9,), 3), pairs=[(1, 0)])
    put("sub_outer", "subtract", spline_data(rng, (3,), (6,), 1), spline_data(rng, (2,), (5,), 1), pairs=None)
    put("bad_add_o44_300_200", "add", spline_data(rng, (4,), (300,), 2), spline_data(rng, (4,), (200,), 2), pairs=[(0, 0)])
    put("bad_add_o46_40_30", "add", spline_data(rng, (4,), (40,), 2), spline_data(rng, (6,), (30,), 2), pairs=[(0, 0)])

    # ---- integrate, in every variable
    put("int_curve_o4", "integrate", spline_data(rng, (4,), (12,), 3), wrt=0)
    s = spline_data(rng, (4, 3), (9, 8), 3, kind="jittered")
    for iv in range(2):
        put(f"int_surface_{iv}", "integrate", s, wrt=iv)
    s = spline_data(rng, (3, 4, 2), (5, 6, 4), 2, kind="jittered")
    for iv in range(3):
        put(f"int_volume_{iv}", "integrate", s, wrt=iv)
    put("int_curve_o3_repeated", "integrate", spline_data(rng, (3,), (12,), 2, repeat=(1, 4)), wrt=0)
    put("int_unclamped", "integrate", spline_data(rng, (4,), (10,), 2, unclamped=True), wrt=0)
    put("int_f32_surface", "integrate", spline_data(rng, (3, 4), (7, 8), 2, dtype=np.float32, kind="jittered"), wrt=1)
    put("int_curve_300", "integrate", spline_data(rng, (4,), (300,), 2), wrt=0)

    # ---- contract: one, some and all variables; the right end; a value on an interior knot
    s = spline_data(rng, (4, 3), (9, 8), 3, kind="jittered")
    put("con_surface_one", "contract", s, uvw=[0.3, np.nan])
    put("con_surface_right_end", "contract", s, uvw=[np.nan, 1.0])
    put("con_surface_on_knot", "contract", s, uvw=[float(s["knots"][0][5]), np.nan])
    s = spline_data(rng, (3, 4, 2), (5, 6, 4), 2, kind="jittered")
    put("con_volume_some", "contract", s, uvw=[np.nan, 0.4, 0.7])
    put("con_volume_all", "contract", s, uvw=[0.21, 1.0, 0.0])
    put("con_unclamped", "contract", spline_data(rng, (4,), (10,), 2, unclamped=True), uvw=[0.45])
    put("con_f32_surface", "contract", spline_data(rng, (3, 4), (7, 8), 2, dtype=np.float32, kind="jittered"), uvw=[0.6, np.nan])
    return out


def ind_map(c):
    return None if c["pairs"] is None else [p if np.isscalar(p) else tuple(p) for p in c["pairs"]]


def call(spline, other, c):
    if c["op"] == "add":
        return spline.add(other, ind_map(c))
    if c["op"] == "subtract":
        return spline.subtract(other, ind_map(c))
    if c["op"] == "integrate":
        return spline.integrate(c["wrt"])
    return spline.contract([None if np.isnan(u) else u for u in c["uvw"]])


def exact_of(c, r_order, r_knots, dtype):
    if c["op"] in ("add", "subtract"):
        pairs = None if c["pairs"] is None else [(p, p) if np.isscalar(p) else p for p in c["pairs"]]
        return sum_ref.add(c, c["other"], pairs, r_order, r_knots, 1 if c["op"] == "add" else -1, dtype)
    if c["op"] == "integrate":
        return sum_ref.integrate(c["order"], c["knots"], c["coefs"], c["wrt"], dtype)[0]
    return sum_ref.contract(c["order"], c["knots"], c["coefs"], [None if np.isnan(u) else u for u in c["uvw"]], dtype)


CURVE = dict(order=[3], knots=[[0.0, 0.0, 0.0, 0.25, 0.5, 0.5, 0.75, 1.0, 1.0, 1.0]], coefs=[[1.0, 2.0, 0.5, -1.0, 3.0, 2.0, 0.0]])
LINE = dict(order=[2], knots=[[0.0, 0.0, 0.5, 1.0, 1.0]], coefs=[[1.0, -2.0, 4.0]])
SHORT = dict(order=[2], knots=[[0.0, 0.0, 0.5, 0.75, 0.75]], coefs=[[1.0, -2.0, 4.0]])
OPEN = dict(order=[3], knots=[[-0.2, -0.1, 0.0, 0.25, 0.5, 0.5, 0.75, 1.0, 1.1, 1.2]], coefs=[[1.0, 2.0, 0.5, -1.0, 3.0, 2.0, 0.0]])
PLANAR = dict(order=[2], knots=[[0.0, 0.0, 0.5, 1.0, 1.0]], coefs=[[1.0, -2.0, 4.0], [0.0, 1.0, 0.5]])
SURFACE = dict(order=[2, 3], knots=[[0.0, 0.0, 0.5, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]],
               coefs=[[[0.0, 1.0, 2.0], [1.0, 3.0, 2.0], [0.5, 0.0, 1.0]]])


def semantics():
    """(name, op, spline, other or None, args): small calls whose outcome is a message, an identity or a small result.
    ``other`` is the first argument of the method (for common_basis: the second spline of the pair)."""
    return [
        ("add_ndep_mismatch", "add", CURVE, PLANAR, [[[0, 0]]]),
        ("add_invalid_map", "add", CURVE, LINE, [[[0, 0, 0]]]),
        ("add_domains", "add", CURVE, SHORT, [[[0, 0]]]),
        ("add_empty_map", "add", OPEN, LINE, [[]]),
        ("add_scalar_entry", "add", CURVE, LINE, [[0]]),
        ("add_none", "add", OPEN, LINE, [None]),
        ("add_surface_curve", "add", SURFACE, LINE, [[[0, 0]]]),
        ("subtract_ndep_mismatch", "subtract", CURVE, PLANAR, [[[0, 0]]]),
        ("subtract_domains", "subtract", CURVE, SHORT, [[0]]),
        ("subtract_scalar_entry", "subtract", CURVE, LINE, [[0]]),
        ("operator_add", "__add__", CURVE, LINE, []),
        ("operator_sub", "__sub__", SURFACE, LINE, []),
        ("operator_add_vector", "__add__", PLANAR, None, [[1.0, 2.0]]),
        ("operator_radd_scalar", "__radd__", CURVE, None, [2.0]),
        ("operator_sub_vector", "__sub__", PLANAR, None, [[1.0, 2.0]]),
        ("operator_rsub_scalar", "__rsub__", CURVE, None, [2.0]),
        ("operator_add_wrong_vector", "__add__", PLANAR, None, [[1.0, 2.0, 3.0]]),
        ("translate", "translate", PLANAR, None, [[0.5, -1.0]]),
        ("translate_scalar", "translate", CURVE, None, [3.0]),
        ("translate_wrong_length", "translate", PLANAR, None, [[0.5]]),
        ("common_basis_invalid_map", "common_basis", CURVE, LINE, [[[0]]]),
        ("common_basis_domains", "common_basis", CURVE, SHORT, [None]),
        ("common_basis_same", "common_basis", CURVE, CURVE, [None]),
        ("common_basis_pair", "common_basis", CURVE, LINE, [[[0, 0]]]),
        ("integrate_negative", "integrate", CURVE, None, [-1]),
        ("integrate_too_large", "integrate", SURFACE, None, [2]),
        ("integrate_second", "integrate", SURFACE, None, [1]),
        ("contract_nothing", "contract", SURFACE, None, [[None, None]]),
        ("contract_outside", "contract", SURFACE, None, [[0.5, 1.5]]),
        ("contract_below", "contract", OPEN, None, [[-0.05]]),
        ("contract_all", "contract", SURFACE, None, [[0.25, 0.5]]),
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
        other = make(c["other"]) if c["other"] is not None else None
        r = call(spline, other, c)
        assert r.coefs.dtype == c["coefs"].dtype, f"{name}: the reference changed the dtype"
        r_knots = [np.asarray(k) for k in r.knots]
        exact = exact_of(c, list(r.order), r_knots, r.coefs.dtype)
        assert exact.shape == np.shape(r.coefs), name
        dev = float(np.abs(np.asarray(r.coefs, np.float64) - exact.astype(np.float64)).max() / np.abs(exact).max())
        devs[c["op"]].append((name, dev, c["coefs"].dtype))
        print(f"{name}: order {tuple(r.order)} nCoef {tuple(r.nCoef)} ref_dev {dev:.3e}", flush=True)
        out[f"{name}/op"] = np.array(c["op"])
        out[f"{name}/order"] = np.array(c["order"], np.int32)
        out[f"{name}/coefs"] = c["coefs"]
        for iv, t in enumerate(c["knots"]):
            out[f"{name}/knots{iv}"] = t
        if other is not None:
            out[f"{name}/b_order"] = np.array(c["other"]["order"], np.int32)
            out[f"{name}/b_coefs"] = c["other"]["coefs"]
            for iv, t in enumerate(c["other"]["knots"]):
                out[f"{name}/b_knots{iv}"] = t
            if c["pairs"] is not None:
                out[f"{name}/pairs"] = np.array([(p, p) if np.isscalar(p) else p for p in c["pairs"]], np.int32).reshape(-1, 2)
                out[f"{name}/scalar"] = np.array([bool(np.isscalar(p)) for p in c["pairs"]], bool)
        if "wrt" in c:
            out[f"{name}/wrt"] = np.array(c["wrt"], np.int32)
        if "uvw" in c:
            out[f"{name}/uvw"] = np.array(c["uvw"], np.float64)
        out[f"{name}/out_order"] = np.array(r.order, np.int32)
        for iv, t in enumerate(r_knots):
            out[f"{name}/out_knots{iv}"] = t
        out[f"{name}/out_coefs"] = np.asarray(r.coefs)
        out[f"{name}/ref_dev"] = np.float64(dev)
    for op, rows in devs.items():
        rows64 = [row for row in rows if row[2] == np.float64]
        good = sum(dev <= 1e-12 for _, dev, _ in rows64)
        assert rows64 and 2 * good >= len(rows64), f"{op}: only {good} of {len(rows64)} float64 cases have ref_dev <= 1e-12"
        print(f"{op}: {good} of {len(rows64)} float64 cases have ref_dev <= 1e-12")

    def describe(r):
        return dict(order=[int(k) for k in r.order], knots=[np.asarray(k, np.float64).tolist() for k in r.knots],
                    coefs=np.asarray(r.coefs, np.float64).tolist())

    records = []
    for name, op, s, o, args in semantics():
        spline = make(s)
        other = make(o) if o is not None else None
        record = dict(name=name, op=op, spline=s, other=o, args=args, error=None, is_self=False, result=None)
        try:
            if op == "common_basis":
                pair = bspy.Spline.common_basis((spline, other), *args)
                record["is_self"] = pair[0] is spline
                record["result"] = [describe(r) for r in pair]
            else:
                r = getattr(spline, op)(*(([other] if other is not None else []) + list(args)))
                record["is_self"] = r is spline
                if r is not spline:
                    record["result"] = describe(r)
        except ValueError as e:
            record["error"] = str(e)
        print(f"{name}: {record['error']!r} is_self {record['is_self']}")
        records.append(record)

    path = os.path.join(HERE, "sum.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "sum_semantics.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
