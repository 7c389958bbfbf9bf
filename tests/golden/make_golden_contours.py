"""
Golden values of ``Spline.contours``.  Runs ONLY where the reference checkout is importable (see
make_golden.load_reference).  Run time: about 2 minutes: the reference's ``contours()`` runs on all cases at once with a
budget of 60 s each, the exact oracle tests/contours_ref.py takes the rest (``generator_seconds`` in the file records it).

``contours.npz``, per case: the inputs (order, knots, coefficients, depth, level), and what is exactly true of the marched
zero set (tests/contours_ref.py): the segments as pairs of lattice-edge keys, per vertex its key, edge (I, J, dir), the
middle of the exact root's bracket in (u, v) as a double-double, the bracket's width and |df/ds| along the edge there;
the saddle cells, the zero cells, the components (closed flags and lengths).  The generator asserts what the tests' bars
assume and replaces a drawn case that fails one of them:
  * every lattice edge outside the closure of a zero cell has at most one exact root;
  * every node value that is not exactly zero is at least 1e-6 S in magnitude;
  * every exactly-zero node evaluates to exactly 0.0 in floats (such cases are built from small dyadic coefficients).
``ref_count`` is the number of curves the reference's ``contours()`` returned, -1 where it had not returned after 60 s or
raised; the generator refuses to write if fewer than half of the cases return.  ``circle/ref_dev`` is the largest
| |c(t) - centre| - r | of the reference's contour of the circle over 257 parameter values.

``contours_semantics.json``: the messages.

    python tests/golden/make_golden_contours.py
"""
import json
import multiprocessing
import os
import sys
import time
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import load_reference  # noqa: E402
import contours_ref  # noqa: E402

REF_BUDGET = 60.0
os.environ.setdefault("BSPY_AMD_NO_TORCH", "1")     # the host drivers only: torch must not be imported behind the reference's stubs


def clamped(order, breaks):
    return np.array([breaks[0]] * order + list(breaks[1:-1]) + [breaks[-1]] * order, np.float64)


def build_cases(bspy):
    cases = {}

    def add(name, order, knots, coefs, depth, level=0.0, kind="plain"):
        cases[name] = dict(order=np.array(order, np.int64), knots=[np.asarray(k) for k in knots], coefs=np.asarray(coefs),
                           depth=int(depth), level=float(level), kind=kind)

    # a circle of radius 0.7 as a biquadratic on [-1, 1]^2, knots inserted to 3 x 4 cells
    x2, one = np.array([1.0, -1.0, 1.0]), np.ones(3)
    k = clamped(3, [-1.0, 1.0])
    circle = bspy.Spline(2, 1, [3, 3], [3, 3], [k, k], (np.outer(x2, one) + np.outer(one, x2) - 0.49)[None])
    circle = circle.insert_knots([[-0.3, 0.45], [-0.5, 0.1, 0.55]])
    add("circle", circle.order, circle.knots, circle.coefs[0], 4, kind="circle")
    # two disjoint circles of radius 0.6 around (-1, 0) and (1, 0): (|x| - 1)^2 + y^2 - 0.36 with a double knot at x = 0
    gx = np.array([1.0, -1.0, 1.0, -1.0, 1.0])
    y2 = 2.25 * np.array([1.0, -1.0, 1.0])
    add("two_circles", [3, 3], [np.array([-2.0, -2, -2, 0, 0, 2, 2, 2]), clamped(3, [-1.5, 1.5])],
        gx[:, None] + y2[None, :] - 0.36, 3)
    # a plane section of a bilinear patch: 0.7 u + 0.45 v + 0.2 u v - 0.61 on 2 x 2 cells
    g = np.array([0.0, 0.5, 1.0])
    # at the depths 0, 1 and 4 (a bilinear piece has at most one root on a lattice edge, however coarse the lattice is)
    for depth in (0, 1, 4):
        add("plane" if depth == 4 else f"plane_d{depth}", [2, 2], [clamped(2, g), clamped(2, g)],
            0.7 * g[:, None] + 0.45 * g[None, :] + 0.2 * g[:, None] * g[None, :] - 0.61, depth)
    # a crease the contour crosses: y = g(x), g with a kink at the double knot x = 0
    gk = np.array([0.12, 0.31, 0.8, 0.52, 0.15])
    add("crease", [3, 2], [np.array([-1.0, -1, -1, 0, 0, 1, 1, 1]), clamped(2, [0.0, 1.0])], gk[:, None] - np.array([0.0, 1.0])[None, :], 3)
    # the diagonal u = v: through lattice nodes and the corner of four cells, exactly
    add("diagonal", [2, 2], [clamped(2, g), clamped(2, g)], g[:, None] - g[None, :], 2, kind="dyadic")
    # one saddle leaf: (u - 3/8)(v - 5/8) + 1/256 on one cell, leaves of 1/4
    c = np.array([0.0, 1.0])
    add("saddle", [2, 2], [clamped(2, c), clamped(2, c)], (c[:, None] - 0.375) * (c[None, :] - 0.625) + 1.0 / 256.0, 2)
    # one zero cell: the 3 x 3 block of coefficients of cell (0, 0) is zero, a negative corner far from it
    z = np.ones((6, 6))
    z[:3, :3] = 0.0
    z[4:, 4:] = -1.0
    add("zero_cell", [3, 3], [clamped(3, [0.0, 1, 2, 3, 4]), clamped(3, [0.0, 1, 2, 3, 4])], z, 2, kind="dyadic")
    return cases


def random_case(seed, order, cells, dtype=np.float64, domain=((0.0, 1.0), (0.0, 1.0)), scale=1.0, depth=3):
    rng = np.random.default_rng(seed)
    knots = []
    for d in range(2):
        lo, hi = domain[d]
        inner = np.sort(lo + (hi - lo) * (np.arange(1, cells[d]) + rng.uniform(-0.2, 0.2, cells[d] - 1)) / cells[d])
        knots.append(clamped(order[d], [lo] + list(inner) + [hi]).astype(dtype))
    shape = tuple(len(knots[d]) - order[d] for d in range(2))
    coefs = (scale * rng.uniform(-1.0, 1.0, shape)).astype(dtype)
    return dict(order=np.array(order, np.int64), knots=knots, coefs=coefs, depth=depth, level=0.0, kind="random")


RANDOM = [("random_22", (2, 2), (3, 2), {}), ("random_34", (3, 4), (3, 2), {}), ("random_44", (4, 4), (2, 2), {}),
          ("random_42", (4, 2), (2, 3), {}), ("float32", (3, 3), (3, 2), dict(dtype=np.float32)),
          ("shifted", (4, 4), (2, 2), dict(domain=((100.0, 103.0), (-40.0, -38.0)), scale=5000.0))]


def decide(case, why):
    """The exact record of a case, or None (and the reason appended to ``why``) when it breaks an assumption of the bars."""
    import bspy_amd.contours as C
    coefs64 = np.asarray(case["coefs"], np.float64)
    S = float(np.abs(coefs64 - case["level"]).max())
    ex = contours_ref.Exact(case["order"], case["knots"], coefs64, case["depth"], case["level"])
    zero = contours_ref.zero_cells(ex.cells, S)
    res = contours_ref.trace(case["order"], case["knots"], coefs64, case["depth"], case["level"], skip=set(zero))
    ex = res["exact"]
    G = ex.G
    # node values: not tiny, and exactly 0.0 in floats where they are exactly zero
    spline = type("S", (), dict(order=tuple(int(k) for k in case["order"]), knots=case["knots"], coefs=case["coefs"][None], nInd=2, nDep=1))
    plan, rows, _, _ = C.tables(spline, None if case["level"] == 0.0 else [case["level"]])
    lat = C.Lattice(rows[0], plan, case["level"], case["depth"])
    for I in range(ex.nc0 * G + 1):
        for J in range(ex.nc1 * G + 1):
            v = ex.node(I, J)
            if v == 0:
                if lat.node_value(I, J) != 0.0:
                    return why.append(f"node {I, J} is exactly zero and {lat.node_value(I, J)} in floats")
            elif abs(v) < Fraction(1, 10 ** 6) * Fraction(S):
                return why.append(f"node {I, J} has the value {float(v)}")
    closure = set()
    for i, j in zero:
        for a in range(G + 1):
            for b in range(G + 1):
                closure.add((i * G + a, j * G + b))
    for I in range(ex.nc0 * G + 1):
        for J in range(ex.nc1 * G + 1):
            for direction, (I1, J1) in enumerate(((I + 1, J), (I, J + 1))):
                if I1 > ex.nc0 * G or J1 > ex.nc1 * G or ((I, J) in closure and (I1, J1) in closure):
                    continue
                if len(ex.edge_roots(I, J, direction)) > 1:
                    return why.append(f"edge {I, J, direction} has more than one root")
    vkeys = sorted(res["vertices"])
    mid_hi, mid_lo, width, slope, edge = [], [], [], [], []
    for key in vkeys:
        I, J, direction = res["vertices"][key]
        u, v, sl = ex.vertex(I, J, direction)
        mids = [(u[0] + u[1]) / 2, (v[0] + v[1]) / 2]
        mid_hi.append([float(m) for m in mids])
        mid_lo.append([float(m - Fraction(float(m))) for m in mids])
        width.append([float(u[1] - u[0]), float(v[1] - v[0])])
        slope.append(float(sl))
        edge.append([I, J, direction])
    comps = res["components"]
    return dict(segments=np.array(sorted(res["segments"]), np.int64).reshape(-1, 2), vkeys=np.array(vkeys, np.int64),
                vedge=np.array(edge, np.int64).reshape(-1, 3), vmid_hi=np.array(mid_hi).reshape(-1, 2), vmid_lo=np.array(mid_lo).reshape(-1, 2),
                vwidth=np.array(width).reshape(-1, 2), vslope=np.array(slope), saddles=np.array(res["saddles"], np.int64).reshape(-1, 2),
                zero=np.array(zero, np.int64).reshape(-1, 2), closed=np.array([c[0] for c in comps], bool),
                lengths=np.array([len(c[1]) for c in comps], np.int64), first_keys=np.array([c[1][0] for c in comps], np.int64), scale=S)


def _reference_worker(queue, case, want_dev):
    bspy = load_reference_module()
    s = bspy.Spline(2, 1, [int(k) for k in case["order"]], list(case["coefs"].shape), case["knots"], np.asarray(case["coefs"])[None] - case["level"])
    try:
        curves = s.contours()
    except Exception as e:  # noqa: BLE001 - recorded
        queue.put((-1, float("nan"), repr(e)))
        return
    dev = float("nan")
    if want_dev:
        t = np.linspace(0.0, 1.0, 257)
        dev = max(float(np.abs(np.hypot(*np.array([c(x) for x in t]).T) - 0.7).max()) for c in curves)
    queue.put((len(curves), dev, ""))


def load_reference_module():
    load_reference()
    import bspy
    return bspy


def reference(cases):
    """{name: (count, dev, note)}: every case in a process of its own, all at once, each with REF_BUDGET seconds."""
    ctx = multiprocessing.get_context("fork")
    running = {}
    for name, case in cases.items():
        queue = ctx.Queue()
        p = ctx.Process(target=_reference_worker, args=(queue, case, name == "circle"))
        p.start()
        running[name] = (p, queue, time.time())
    out = {}
    for name, (p, queue, t) in running.items():
        p.join(max(0.0, REF_BUDGET - (time.time() - t)))
        if p.is_alive():
            p.terminate()
            p.join()
            out[name] = (-1, float("nan"), f"not returned after {REF_BUDGET:.0f} s")
        else:
            count, dev, err = queue.get()
            out[name] = (count, dev, err or "returned")
    return out


def semantics(bspy):
    k2 = [0.0, 0.0, 1.0, 1.0]
    entries = []

    def ref_error(nInd, nDep, order, knots, coefs):
        try:
            bspy.Spline(nInd, nDep, order, [len(k) - o for k, o in zip(knots, order)], [np.array(k) for k in knots], np.array(coefs)).contours()
        except ValueError as e:
            return str(e)
        raise AssertionError("the reference did not refuse")

    coefs = [[[1.0, -2.0], [0.5, 1.0]], [[1.0, 2.0], [0.5, 1.0]]]
    entries.append(dict(name="free_variables", spline=dict(nInd=2, nDep=2, order=[2, 2], knots=[k2, k2], coefs=coefs), type="ValueError",
                        error=ref_error(2, 2, [2, 2], [k2, k2], coefs)))
    entries.append(dict(name="three_variables", spline=dict(nInd=3, nDep=2, order=[2, 2, 2], knots=[k2, k2, k2], coefs=np.ones((2, 2, 2, 2)).tolist()),
                        type="NotImplementedError", error="contours: two independent variables only (scalar fields over a surface's parameters)"))
    k5 = [0.0] * 5 + [1.0] * 5
    entries.append(dict(name="order_five", spline=dict(nInd=2, nDep=1, order=[5, 2], knots=[k5, k2], coefs=np.ones((1, 5, 2)).tolist()),
                        type="NotImplementedError", error="contours: orders from 2 to 4"))
    kj = [0.0, 0.0, 0.5, 0.5, 1.0, 1.0]
    entries.append(dict(name="jump", spline=dict(nInd=2, nDep=1, order=[2, 2], knots=[kj, k2], coefs=np.ones((1, 4, 2)).tolist()),
                        type="ValueError", error="contours: the knot 0.5 of variable 0 has multiplicity 2 >= order 2 (a jump: no contour crosses it; trim the spline there)"))
    return entries


def main():
    started = time.time()
    bspy = load_reference_module()
    cases = build_cases(bspy)
    records = {}
    for name, case in cases.items():
        why = []
        rec = decide(case, why)
        assert rec is not None, f"{name}: a built case breaks an assumption of the bars: {why}"
        records[name] = rec
    for name, order, cells, extra in RANDOM:
        for seed in range(1000):
            case = random_case(seed + 1000 * len(name), order, cells, **extra)
            rec = decide(case, [])
            if rec is not None and len(rec["segments"]):
                case["seed"] = seed
                cases[name], records[name] = case, rec
                break
        else:
            raise AssertionError(f"{name}: no seed gives a case the bars hold for")
    out = {}
    returned = 0
    ref = reference(cases)
    for name, case in cases.items():
        count, dev, note = ref[name]
        returned += count >= 0
        print(f"{name}: {len(records[name]['closed'])} components, reference {count} ({note})")
        out[f"{name}/order"], out[f"{name}/knots0"], out[f"{name}/knots1"] = case["order"], case["knots"][0], case["knots"][1]
        out[f"{name}/coefs"], out[f"{name}/depth"], out[f"{name}/level"], out[f"{name}/kind"] = case["coefs"], case["depth"], case["level"], case["kind"]
        out[f"{name}/ref_count"] = count
        if name == "circle":
            out[f"{name}/ref_dev"] = dev
        for key, value in records[name].items():
            out[f"{name}/{key}"] = value
    assert 2 * returned >= len(cases), "the reference returned on fewer than half of the cases"
    out["names"] = np.array(sorted(cases))
    out["generator_seconds"] = time.time() - started
    np.savez_compressed(os.path.join(HERE, "contours.npz"), **out)
    with open(os.path.join(HERE, "contours_semantics.json"), "w") as f:
        json.dump(semantics(bspy), f, indent=1)
    print(f"wrote contours.npz and contours_semantics.json in {time.time() - started:.0f} s")


if __name__ == "__main__":
    main()
