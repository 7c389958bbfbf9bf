"""
Golden values of Spline.multiply.  Runs ONLY where the reference checkout is importable (see make_golden.load_reference).

``product.npz``, per case: the two splines, ``indMap``, ``productType``, the order, knots and coefficients the reference
returned, and ``ref_dev``: the largest difference between the reference's coefficients and the exact product of
tests/product_ref.py (rational arithmetic, rounded once to the result's dtype), relative to
S = nTerms * max |self.coefs| * max |other.coefs| (nTerms: 1 for 'S', nDep for 'D', 2 for 'C').

The reference's coefficients are wrong where the two orders of a mapped variable differ and the knots are not shared
(its knots are right): the ``uneq_*`` cases keep that on record, with ref_dev of 1e-6 .. 1e1.  ``hi_*`` are orders 6 x 6
and 8 x 8, where its Taylor expansions lose digits.  The tests pin both groups to the exact result only.  So that ref_dev
cannot turn the comparison with the reference into nothing, the generator refuses to write unless every other case has
ref_dev <= 1e-12 and, for every productType, at least half of all its cases do (float32 results: see bar_of).

One call differs from the case as stored: with the map [(0, 1), (1, 0)] the reference fails while it renumbers the
remaining pairs ("not enough values to unpack": it drops a field of its own tuple), so it is given the same pairs in the
order [(1, 0), (0, 1)], which it can take; a map is a set of pairs, the product is the same.

``product_semantics.json``: for small inputs, the message of the reference's ValueError, or the result's nDep, orders,
knots dtype, coefficient dtype and metadata.

    python tests/golden/make_golden_product.py

npz keys: ``<case>/order1``, ``<case>/knots1_<iv>``, ``<case>/coefs1`` (and 2), ``<case>/ptype``, ``<case>/map`` (n x 2;
absent: indMap None), ``<case>/scalar`` (whether the entry is passed as one index), ``<case>/out_order``,
``<case>/out_knots<iv>``, ``<case>/out_coefs``, ``<case>/exact`` (what product_ref.multiply returned: the tests compute
it again but for the ``hi_*`` cases, whose exact rows take a minute), ``<case>/ref_dev``.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
from make_golden_refine import knot_vector  # noqa: E402
import product_ref  # noqa: E402

N_TERMS = {"S": lambda n: 1, "D": lambda n: n, "C": lambda n: 2}


def spline_data(rng, orders, ncoefs, ndep, dtype=np.float64, shared=None, **kw):
    """shared: per variable a list of knots (of the other operand) of which every second interior one is taken over."""
    knots = []
    for iv, (k, n) in enumerate(zip(orders, ncoefs)):
        t = knot_vector(rng, k, n, **kw)
        if shared is not None:
            take = np.unique(shared[iv][1:-1])
            take = take[(take > 0.0) & (take < 1.0)][::2][:n - k]
            t[k:k + len(take)] = take
            t[k:n] = np.sort(t[k:n])
        knots.append(t.astype(dtype))
    coefs = (rng.standard_normal((ndep, *ncoefs)) + 0.3).astype(dtype)
    return dict(order=list(orders), knots=knots, coefs=coefs)


def cases():
    rng = np.random.default_rng(20250412)
    out = {}

    def add(name, a, b, indMap, ptype):
        out[name] = dict(a=a, b=b, map=indMap, ptype=ptype)

    def curves(name, k1, n1, d1, k2, n2, d2, ptype, kind="random", **kw):
        add(name, spline_data(rng, (k1,), (n1,), d1, kind=kind, **kw), spline_data(rng, (k2,), (n2,), d2, kind=kind), [0], ptype)

    # ---- curves of equal orders: every dependent-variable rule, random and jittered knots
    curves("cur_o2_S11", 2, 9, 1, 2, 7, 1, "S")
    curves("cur_o3_S31", 3, 10, 3, 3, 8, 1, "S", kind="jittered")
    curves("cur_o4_S13", 4, 12, 1, 4, 9, 3, "S")
    curves("cur_o5_S33", 5, 11, 3, 5, 9, 3, "S", kind="jittered")
    curves("cur_o4_D2", 4, 13, 2, 4, 8, 2, "D")
    curves("cur_o3_D3", 3, 9, 3, 3, 12, 3, "D", kind="jittered")
    curves("cur_o2_D3", 2, 8, 3, 2, 6, 3, "D")
    curves("cur_o4_C2", 4, 10, 2, 4, 11, 2, "C", kind="jittered")
    curves("cur_o3_C3", 3, 12, 3, 3, 7, 3, "C")
    curves("cur_o5_C3", 5, 10, 3, 5, 8, 3, "C")
    curves("cur_o4_40_S33", 4, 40, 3, 4, 33, 3, "S", kind="jittered")
    # repeated interior knots in either operand
    curves("cur_o4_repeated_self", 4, 13, 2, 4, 9, 2, "D", repeat=(1, 3))
    add("cur_o3_repeated_other", spline_data(rng, (3,), (9,), 3), spline_data(rng, (3,), (12,), 3, repeat=(0, 4)), [0], "C")
    # knots shared between the operands
    a = spline_data(rng, (4,), (14,), 3)
    add("cur_o4_shared", a, spline_data(rng, (4,), (11,), 3, shared=a["knots"]), [(0, 0)], "S")
    a = spline_data(rng, (3,), (12,), 2, repeat=(2,))
    add("cur_o3_shared_repeated", a, spline_data(rng, (3,), (10,), 2, shared=a["knots"]), [0], "C")
    # one unclamped operand (its domain is [0, 1]: the other one is clamped to it)
    add("cur_o4_unclamped", spline_data(rng, (4,), (12,), 2, unclamped=True), None, [0], "D")
    add("cur_o3_unclamped_other", None, spline_data(rng, (3,), (10,), 3, unclamped=True), [0], "S")
    for name, k in (("cur_o4_unclamped", 4), ("cur_o3_unclamped_other", 3)):
        c = out[name]
        given = c["a"] or c["b"]
        t = given["knots"][0]
        lo, hi = t[k - 1], t[len(t) - k]
        other = spline_data(rng, (k,), (k + 5,), given["coefs"].shape[0])
        other["knots"][0] = lo + (hi - lo) * other["knots"][0]
        other["knots"][0][:k], other["knots"][0][-k:] = lo, hi
        c["a" if c["a"] is None else "b"] = other
    # float32
    add("cur_o4_f32", spline_data(rng, (4,), (12,), 3, dtype=np.float32), spline_data(rng, (4,), (9,), 3, dtype=np.float32), [0], "C")
    add("cur_o3_f32_S", spline_data(rng, (3,), (10,), 2, dtype=np.float32), spline_data(rng, (3,), (8,), 2, dtype=np.float32), [0], "S")

    # ---- surfaces
    def surf(orders, ncoefs, ndep, **kw):
        return spline_data(rng, orders, ncoefs, ndep, kind="jittered", **kw)

    add("surf_both_S", surf((4, 3), (8, 7), 3), surf((4, 3), (7, 6), 3), [0, 1], "S")
    add("surf_both_D", surf((3, 4), (7, 8), 3), surf((3, 4), (6, 9), 3), [(0, 0), (1, 1)], "D")
    add("surf_both_C", surf((4, 4), (8, 8), 3), surf((4, 4), (7, 9), 3), [0, (1, 1)], "C")
    add("surf_both_repeated", surf((3, 3), (9, 8), 2, repeat=(1,)), surf((3, 3), (7, 7), 2), [0, 1], "C")
    add("surf_swapped_D", surf((4, 3), (8, 7), 3), surf((3, 4), (6, 7), 3), [(0, 1), (1, 0)], "D")
    add("surf_swapped_S", surf((3, 4), (7, 9), 1), surf((4, 3), (8, 6), 2), [(0, 1), (1, 0)], "S")
    add("surf_x_curve", surf((3, 4), (6, 9), 3), spline_data(rng, (4,), (8,), 1), [(1, 0)], "S")
    add("surf_x_curve_C", surf((3, 3), (7, 6), 3), spline_data(rng, (3,), (9,), 3), [(0, 0)], "C")
    add("surf_partial", surf((3, 4), (6, 8), 2), surf((4, 2), (7, 5), 2), [(1, 0)], "D")
    add("vol_x_surf_partial", surf((2, 3, 3), (4, 5, 6), 3), surf((3, 2), (7, 4), 3), [(2, 0)], "C")
    add("surf_none", surf((3, 2), (5, 4), 3), surf((2, 3), (4, 5), 3), None, "C")
    add("cur_none", spline_data(rng, (4,), (9,), 2), spline_data(rng, (3,), (7,), 2), None, "D")
    add("surf_f32_both", surf((3, 3), (8, 7), 3, dtype=np.float32), surf((3, 3), (6, 8), 3, dtype=np.float32), [0, 1], "D")

    # ---- three mapped variables (host path)
    add("tri_all_S", surf((2, 3, 2), (4, 5, 4), 2), surf((2, 3, 2), (5, 4, 4), 2), [0, 1, 2], "S")
    add("tri_all_D", surf((3, 2, 3), (5, 4, 4), 3), surf((3, 2, 3), (4, 5, 5), 3), [0, 1, 2], "D")

    # ---- orders that differ in a mapped variable: the reference's coefficients are wrong
    curves("uneq_o35", 3, 10, 2, 5, 9, 2, "S")
    curves("uneq_o53", 5, 11, 3, 3, 8, 3, "D")
    curves("uneq_o26", 2, 9, 1, 6, 10, 3, "S")
    curves("uneq_o46", 4, 12, 3, 6, 9, 3, "C")
    add("uneq_surf_o3443", surf((3, 4), (7, 8), 3), surf((4, 3), (8, 6), 3), [0, 1], "S")

    # ---- high orders
    curves("hi_o66", 6, 12, 2, 6, 10, 2, "S")
    curves("hi_o88", 8, 9, 1, 8, 8, 1, "S")
    return out


def bar_of(dtype):
    """1e-12 is about 4500 eps of float64.  A float32 result cannot be nearer than eps of float32 to anything: its bar is
    the same number of its own eps (5.4e-4)."""
    return 1e-12 if dtype == np.float64 else 1e-12 * float(np.finfo(np.float32).eps / np.finfo(np.float64).eps)


def pairs_of(indMap):
    return None if indMap is None else [(m, m) if np.isscalar(m) else tuple(m) for m in indMap]


def reference_map(indMap):
    """The map as the reference can take it (see the header)."""
    pairs = pairs_of(indMap)
    if pairs is not None and any(pairs[i][1] > pairs[at][1] for at in range(len(pairs)) for i in range(at)):
        return list(reversed(indMap))
    return indMap


CURVE = dict(order=[3], knots=[[0.0, 0.0, 0.0, 0.25, 0.5, 0.5, 0.75, 1.0, 1.0, 1.0]], coefs=[[1.0, 2.0, 0.5, -1.0, 3.0, 2.0, 0.0]])
CURVE2 = dict(order=[2], knots=[[0.0, 0.0, 0.4, 1.0, 1.0]], coefs=[[1.0, -2.0, 0.5], [0.0, 1.0, 2.0]])
CURVE3 = dict(order=[2], knots=[[0.0, 0.0, 0.4, 1.0, 1.0]], coefs=[[1.0, -2.0, 0.5], [0.0, 1.0, 2.0], [3.0, 1.0, 1.0]])
CURVE4 = dict(order=[2], knots=[[0.0, 0.0, 1.0, 1.0]], coefs=[[1.0, -2.0], [0.0, 1.0], [3.0, 1.0], [1.0, 1.0]])
SHIFTED = dict(order=[2], knots=[[0.0, 0.0, 0.5, 1.5, 1.5]], coefs=[[1.0, -2.0, 0.5]])
SURFACE = dict(order=[2, 3], knots=[[0.0, 0.0, 0.5, 1.0, 1.0], [0.0, 0.0, 0.0, 2.0, 2.0, 2.0]],
               coefs=[[[0.0, 1.0, 2.0], [1.0, 3.0, 2.0], [0.5, 0.0, 1.0]]])
CURVE_F32 = dict(CURVE, dtype="float32")


def semantics():
    """(name, self, other, indMap, productType)."""
    return [
        ("bad_product_type", CURVE, CURVE, [0], "X"),
        ("dot_mismatched", CURVE2, CURVE3, [0], "D"),
        ("cross_mismatched", CURVE2, CURVE3, [0], "C"),
        ("cross_four", CURVE4, CURVE4, [0], "C"),
        ("cross_one", CURVE, CURVE, [0], "C"),
        ("scalar_mismatched", CURVE2, CURVE3, [0], "S"),
        ("domain_differs", CURVE, SHIFTED, [0], "S"),
        ("domain_differs_pair", SURFACE, CURVE, [[1, 0]], "S"),
        ("same_variable_twice", SURFACE, CURVE, [[0, 0], [1, 0]], "S"),
        ("bad_type_checked_first", CURVE2, CURVE3, [0], "Q"),
        ("ok_scalar", CURVE, CURVE2, [0], "S"),
        ("ok_broadcast_other", CURVE2, CURVE, [0], "S"),
        ("ok_dot", CURVE3, CURVE3, [0], "D"),
        ("ok_cross2", CURVE2, CURVE2, [0], "C"),
        ("ok_surface_curve", SURFACE, CURVE, [0], "S"),
        ("ok_no_map", CURVE, CURVE2, None, "S"),
        ("ok_f32_self", CURVE_F32, CURVE2, [0], "S"),
        ("ok_f32_other", CURVE2, CURVE_F32, [0], "S"),
    ]


def main():
    bspy = load_reference()

    def make(s, metadata={}):
        dtype = np.dtype(s.get("dtype", "float64")) if isinstance(s["coefs"], list) else None
        knots = [np.array(k, dtype) if dtype else np.array(k) for k in s["knots"]]
        coefs = np.array(s["coefs"], dtype) if dtype else np.array(s["coefs"])
        return bspy.Spline(len(s["order"]), coefs.shape[0], s["order"], coefs.shape[1:], knots, coefs, metadata)

    out, devs = {}, {}
    for name, c in cases().items():
        a, b = c["a"], c["b"]
        r = make(a).multiply(make(b), reference_map(c["map"]), c["ptype"])
        pairs = pairs_of(c["map"]) or []
        new_knots = [np.asarray(r.knots[p[0]]) for p in pairs]
        exact = product_ref.multiply(a["order"], a["knots"], a["coefs"], b["order"], b["knots"], b["coefs"], pairs, c["ptype"],
                                     new_knots, r.coefs.dtype)
        assert exact.shape == r.coefs.shape, (name, exact.shape, r.coefs.shape)
        scale = N_TERMS[c["ptype"]](a["coefs"].shape[0]) * np.abs(a["coefs"]).max() * np.abs(b["coefs"]).max()
        dev = float(np.abs(np.asarray(r.coefs, np.float64) - exact.astype(np.float64)).max() / scale)
        devs.setdefault(c["ptype"], []).append((name, dev))
        print(f"{name}: nDep {r.nDep} order {tuple(r.order)} nCoef {tuple(r.nCoef)} {r.coefs.dtype} ref_dev {dev:.3e}", flush=True)
        for tag, s in (("1", a), ("2", b)):
            out[f"{name}/order{tag}"] = np.array(s["order"], np.int32)
            out[f"{name}/coefs{tag}"] = s["coefs"]
            for iv, k in enumerate(s["knots"]):
                out[f"{name}/knots{tag}_{iv}"] = k
        out[f"{name}/ptype"] = np.array(c["ptype"])
        if c["map"] is not None:
            out[f"{name}/map"] = np.array(pairs, np.int32).reshape(-1, 2)
            out[f"{name}/scalar"] = np.array([np.isscalar(m) for m in c["map"]], bool)
        out[f"{name}/out_order"] = np.array(r.order, np.int32)
        for iv, k in enumerate(r.knots):
            out[f"{name}/out_knots{iv}"] = np.asarray(k)
        out[f"{name}/out_coefs"] = np.asarray(r.coefs)
        out[f"{name}/exact"] = exact
        out[f"{name}/ref_dev"] = np.float64(dev)
    for ptype, rows in devs.items():
        for name, dev in rows:
            assert name.startswith(("uneq_", "hi_")) or dev <= bar_of(out[f"{name}/out_coefs"].dtype), f"{name}: ref_dev {dev:.3e}"
        good = sum(dev <= bar_of(out[f"{name}/out_coefs"].dtype) for name, dev in rows)
        assert 2 * good >= len(rows), f"{ptype}: only {good} of {len(rows)} cases have ref_dev <= 1e-12"
        print(f"{ptype}: {good} of {len(rows)} cases have ref_dev <= 1e-12")

    records = []
    for name, a, b, indMap, ptype in semantics():
        record = dict(name=name, a=a, b=b, map=indMap, ptype=ptype, error=None)
        try:
            pairs = None if indMap is None else [m if np.isscalar(m) else tuple(m) for m in indMap]
            r = make(a, {"tag": 1}).multiply(make(b, {"tag": 2}), pairs, ptype)
            record.update(nDep=int(r.nDep), order=[int(o) for o in r.order], nCoef=[int(n) for n in r.nCoef],
                          knots_dtype=[str(k.dtype) for k in r.knots], coefs_dtype=str(r.coefs.dtype), metadata=r.metadata)
        except ValueError as e:
            record["error"] = str(e)
        print(f"{name}: {record['error']!r} {record.get('order')} {record.get('coefs_dtype')}")
        records.append(record)

    path = os.path.join(HERE, "product.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "product_semantics.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
