"""
Writes tests/golden/orders_<family>.npz for the six cell families whose spline orders are template constants (zeros2,
zeros3, contours, project, rays, surfaces): one small fp64 case for EVERY order tuple the family dispatches
(tests/orders_util.py: ``dispatched``, read from the families' own range constants, never typed out), each in the family's
own key layout so that the family's own checks run on it unchanged (tests/test_orders_host.py, tests/test_gpu_orders.py).
What is exactly true comes from the repository's rational oracles alone: zeros2_ref, zeros3_ref, contours_ref,
project_ref, surfaces_ref and the rays oracle of make_golden_rays.py.  Nothing is read from the reference checkout.

    python tests/golden/make_golden_orders.py [family ...]

Shapes: 2 or 3 knot cells per axis, unequal counts and unequal widths, so that the windows step by K - 1 and a transposed
stride shows; one case per family has a double interior knot.  Every draw is seeded by (family, tuple): a family whose range
grows gets new cases and keeps its old ones.

The generator asserts, of the oracle's answer alone (conditions on the inputs, not measurements):
  * every case is transversal: certified by the family's own conditioning rule (``certified`` of make_golden_roots2/3,
    ``within_bars`` of make_golden_rays, ``decide`` of make_golden_contours, ``record`` of make_golden_project,
    ``surfaces_ref.vertices`` without a raise), no zero cell, no special ray;
  * content: zeros2 / zeros3: at least 3 zeros over at least 2 cells in the case's two systems, every system has a zero, and
    a cell whose components both change sign holds none; rays: 14 rays of which at least 8 hit and 2 miss; surfaces: every
    line family has at least 2 vertices; contours: a component crosses a knot line; project: 8 certified points;
  * the tuples with content are the tuples the family dispatches.

Run time on 8 CPUs: 80 s in all (zeros2 1 s, zeros3 52 s, contours 1 s, project 15 s, rays 3 s, surfaces 6 s; zeros2, zeros3
and surfaces run one tuple per process).  The files are byte-identical from run to run.
"""
import itertools
import os
import sys
import time
import zlib
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ.setdefault("BSPY_AMD_NO_TORCH", "1")             # the host drivers only

import orders_util as ou  # noqa: E402


def rng_of(family, order, salt=0):
    return np.random.default_rng([zlib.crc32(family.encode()), salt, *(int(k) for k in order)])


def axis_knots(rng, K, ncells, double=False):
    """Clamped knots on [0, 1]: ncells cells whose widths differ by a fifth of a cell or more; double: the first interior knot twice."""
    while True:
        inner = np.sort(np.round(rng.uniform(0.15, 0.85, ncells - 1) * 64) / 64)
        widths = np.diff(np.concatenate(([0.0], inner, [1.0])))
        if widths.min() >= 0.15 and (np.abs(np.diff(np.sort(widths))) >= 0.2 / ncells).all():
            break
    if double:
        inner = np.sort(np.concatenate((inner, inner[:1])))
    return np.concatenate((K * [0.0], inner, K * [1.0]))


def ncells_of(order):
    """3 and 2 cells in turn, starting with 3 on the first axis when the orders' sum is even."""
    first = 3 if sum(order) % 2 == 0 else 2
    return [first if a % 2 == 0 else 5 - first for a in range(len(order))]


def doubled(family, order):
    """The case of a family that carries the double knot (on axis 0): the first dispatched tuple whose first order is 3 or
    more, so that the spline stays continuous there."""
    return tuple(order) == next(t for t in ou.dispatched(family) if len(t) > 1 and t[0] >= 3)


def store(family, out, started):
    path = ou.path_of(family)
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    print(f"{path}: {os.path.getsize(path)} bytes in {time.time() - started:.0f} s", flush=True)


# ------------------------------------------------------------------------------------------ zeros2, zeros3
def pool_map(work, items):
    """``work`` over ``items`` in processes of their own, results in the order of the items (every item has its own seed)."""
    import multiprocessing
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        return pool.map(work, items, chunksize=1)


def near_linear(rng, order, knots):
    """The B-spline coefficients of Q (x - p), Q orthogonal and p in the middle of the domain (the Greville abscissae carry a
    linear function exactly).  A random trivariate system of orders up to (4, 4, 4) has tens of zeros, some of them nearly
    singular, and the rational oracle needs a minute per draw to say so; with half a unit of noise on this map a system has one
    to three well conditioned zeros and the oracle's sign test discards most boxes at once."""
    g = np.meshgrid(*(np.array([t[i + 1:i + k].mean() for i in range(len(t) - k)]) for k, t in zip(order, knots)), indexing="ij")
    Q, p = np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.uniform(0.25, 0.75, 3)
    return np.stack([sum(Q[d, a] * (g[a] - p[a]) for a in range(3)) for d in range(3)])


def zeros_case(order):
    """(the two systems' entries, a line for the log) of one order tuple."""
    import make_golden_roots2 as g2
    import make_golden_roots3 as g3
    import zeros2_ref
    import zeros3_ref
    nind = len(order)
    family, g, ref = (f"zeros{nind}", g2, zeros2_ref) if nind == 2 else (f"zeros{nind}", g3, zeros3_ref)
    started = time.time()
    rng = rng_of(family, order)
    ncells = ncells_of(order) if nind == 2 else [[2, 3, 2], [3, 2, 2], [2, 2, 3]][sum(order) % 3]
    for draw in range(2000):
        knots = [axis_knots(rng, k, nc, doubled(family, order) and a == 0) for a, (k, nc) in enumerate(zip(order, ncells))]
        ncoef = [len(t) - k for t, k in zip(knots, order)]
        coefs = rng.standard_normal((2, nind, *ncoef))
        if nind == 3:                                          # see ``near_linear``
            coefs = np.stack([near_linear(rng, order, knots) + 0.5 * c for c in coefs])
        coefs = np.round(coefs * 256) / 256
        exact = []
        for c in coefs:
            e = g.certified(list(order), knots, c)
            if e is None or len(e) < 1 or ref.zero_cells(list(order), knots, c):
                break
            exact.append(e)
        if len(exact) < 2 or sum(len(e) for e in exact) < 3 or len({(b, tuple(z["cell"])) for b, e in enumerate(exact) for z in e}) < 2:
            continue
        empty = 0                                              # candidate cells (every component changes sign) without a zero
        for b, c in enumerate(coefs):
            cells = ref.bezier_cells(list(order), knots, c)[-1]
            for at in itertools.product(*(range(n) for n in ncells)):
                cell = cells
                for i in at:
                    cell = cell[i]
                if not any(ref.one_sign(comp) for comp in cell) and not any(tuple(z["cell"]) == at for z in exact[b]):
                    empty += 1
        if empty:
            break
    else:
        raise AssertionError(f"{family} {order}: no draw with content")
    out = {}
    for b, c in enumerate(coefs):
        uv, extra = g.exact_of(dict(kind="coupled", order=list(order), knots=knots, coefs=c))
        assert len(uv) == len(exact[b]) and len(extra["exact_cells"]) == 0
        rec = dict(order=np.array(order, np.int32), coefs=c, kind=np.array("coupled"), ref_roots=np.empty((0, nind)),
                   ref_complete=np.array(False), ref_dev=np.float64("nan"), **{f"knots{a}": t for a, t in enumerate(knots)}, **extra)
        rec["exact_uv" if nind == 2 else "exact_uvw"] = uv
        for key, val in rec.items():
            out[f"{ou.case_id(order)}.{b}/{key}"] = val
    return out, (f"{family} {order}: {ncells} cells, {[len(e) for e in exact]} zeros, {empty} empty candidates, draw {draw}, "
                 f"{time.time() - started:.0f} s")


def zeros_family(nind):
    family = f"zeros{nind}"
    started = time.time()
    out = {}
    for rec, line in pool_map(zeros_case, ou.dispatched(family)):
        out.update(rec)
        print(line, flush=True)
    out["names"] = np.array([ou.case_id(t) for t in ou.dispatched(family)])
    assert all(f"{n}.{b}/coefs" in out for n in out["names"] for b in range(2))
    store(family, out, started)


# ------------------------------------------------------------------------------------------ contours
def contours_family():
    import make_golden_contours as gc
    started = time.time()
    out, names = {}, []
    for order in ou.dispatched("contours"):
        rng = rng_of("contours", order)
        ncells = ncells_of(order)
        G = 1 << 2
        for draw in range(1000):
            knots = [axis_knots(rng, k, nc, doubled("contours", order) and a == 0) for a, (k, nc) in enumerate(zip(order, ncells))]
            coefs = np.round(rng.uniform(-1.0, 1.0, [len(t) - k for t, k in zip(knots, order)]) * 256) / 256
            case = dict(order=np.array(order, np.int64), knots=knots, coefs=coefs, depth=2, level=0.0, kind="random")
            rec = gc.decide(case, [])
            if rec is None or not len(rec["segments"]) or len(rec["zero"]) or len(rec["saddles"]):
                continue
            # a vertex on an interior knot line: its component crosses from one cell into the next
            crossing = [(d == 0 and J % G == 0 and 0 < J < ncells[1] * G) or (d == 1 and I % G == 0 and 0 < I < ncells[0] * G)
                        for I, J, d in rec["vedge"]]
            if any(crossing):
                break
        else:
            raise AssertionError(f"contours {order}: no draw with content")
        name = ou.case_id(order)
        names.append(name)
        for key, value in dict(order=case["order"], knots0=knots[0], knots1=knots[1], coefs=coefs, depth=2, level=0.0, kind="random",
                               ref_count=-1, **rec).items():
            out[f"{name}/{key}"] = value
        print(f"contours {order}: {ncells} cells, {len(rec['closed'])} components, {len(rec['vkeys'])} vertices, {sum(crossing)} on knot lines, "
              f"draw {draw}, {time.time() - started:.0f} s", flush=True)
    assert names == [ou.case_id(t) for t in ou.dispatched("contours")]
    out["names"] = np.array(names)
    store("contours", out, started)


# ------------------------------------------------------------------------------------------ project
def project_family():
    import make_golden_project as gp
    from bspy_amd import project
    started = time.time()
    out, names = {}, []
    for order in ou.dispatched("project"):
        rng = rng_of("project", order)
        if len(order) == 2:
            ncells, nDep = ncells_of(order), 3
        else:
            ncells, nDep = [3], 2 + order[0] % 2                # curves: nDep 2 and 3 in turn
        knots = [axis_knots(rng, k, nc, doubled("project", order) and a == 0) for a, (k, nc) in enumerate(zip(order, ncells))]
        n = [len(t) - k for t, k in zip(knots, order)]
        if len(order) == 2:                                    # the shapes of make_golden_project.cases
            c = np.zeros((3, *n))
            c[0] = np.linspace(0.0, 2.0, n[0])[:, None] + 0.1 * rng.standard_normal(n)
            c[1] = np.linspace(0.0, 2.0, n[1])[None, :] + 0.1 * rng.standard_normal(n)
            c[2] = 0.4 * rng.standard_normal(n)
        else:
            c = rng.standard_normal((nDep, n[0])) * 0.5
            c[0] = np.linspace(0.0, 3.0, n[0]) + 0.2 * rng.standard_normal(n[0])
        name = ou.case_id(order)
        case = dict(order=list(order), knots=knots, coefs=np.round(c * 64) / 64, samples=None)
        spline = gp.spline_of(case)
        tables = project.host_tables(spline, None)
        todo = gp.special_points(name, case, spline, rng)
        flat = case["coefs"].reshape(nDep, -1)
        centre, size = flat.mean(axis=1), np.ptp(flat, axis=1).max()
        rows, tried = [], 0
        while len(rows) < 8 and tried < 80:
            p = np.asarray(todo.pop(0) if todo else centre + size * 0.6 * rng.standard_normal(nDep), np.float64)
            tried += 1
            row = gp.record(case, spline, tables, p)
            if row:
                rows.append(dict(row, p=p))
        assert len(rows) == 8, f"project {order}: {len(rows)} certified points"
        names.append(name)
        out[name + ".order"] = np.array(order, np.int32)
        for a, k in enumerate(knots):
            out[f"{name}.knots{a}"] = k
        out[name + ".coefs"], out[name + ".samples"] = case["coefs"], np.array(0, np.int32)
        out[name + ".points"] = np.stack([r["p"] for r in rows], axis=1)
        for key in ("u", "radius", "free"):
            out[f"{name}.{key}"] = np.array([r[key] for r in rows]).T
        for key in ("dist_lo", "dist_hi", "gap", "hinv", "jmax", "hmin", "steps"):
            out[f"{name}.{key}"] = np.array([r[key] for r in rows])
        assert np.all(out[name + ".gap"] > gp.MARGIN)
        print(f"project {order}: {ncells} cells, nDep {nDep}, 8 points of {tried} drawn, {int((1 - out[name + '.free']).any(axis=0).sum())} on a bound, "
              f"{time.time() - started:.0f} s", flush=True)
    assert names == [ou.case_id(t) for t in ou.dispatched("project")]
    out["names"], out["margin"] = np.array(names), np.array(gp.MARGIN)
    store("project", out, started)


# ------------------------------------------------------------------------------------------ rays
def ray_kinds(rng, s):
    """(kind, draws): per kind of ray an endless iterator of (o, d) on the graph surface s (x = u on [0, 1], y = v on [0, 2],
    z small).  Every non-zero component of d is at least 0.05 in size, so that the ray's extent through the box stays small."""
    def small():
        return float(rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 0.2))

    def at():
        return 0.1 + 0.8 * rng.random(), 0.2 + 1.6 * rng.random()

    def vertical(sign):                                        # dominant z: from above (sign -1) or from below
        while True:
            (x, y), dx, dy = at(), small(), small()
            yield (x + 3.0 * sign * dx, y + 3.0 * sign * dy, -3.0 * sign), (dx, dy, sign)

    def along(axis, sign):                                     # dominant x or y, descending through z = 0 above (x, y)
        while True:
            (x, y), other, dz = at(), small(), -rng.uniform(0.3, 0.45)
            d = [other, other, dz]
            d[axis] = sign
            o = [x - 2.0 * d[0], y - 2.0 * d[1], -2.0 * dz]
            yield tuple(o), tuple(d)

    def zeros(count):
        while True:
            (x, y), dy = at(), small()
            yield ((x, y - 3.0 * dy, 3.0), (0.0, dy, -1.0)) if count == 1 else ((x, y, 3.0), (0.0, 0.0, -1.0))

    def tie():                                                 # |d_x| = |d_z|
        while True:
            (x, y), dy = at(), small()
            yield (x + 1.5, y - 1.5 * dy, 1.5), (-1.0, dy, -1.0)

    def near():                                                # the hit lies before tmin
        while True:
            (x, y), dx, dy = at(), small(), small()
            yield (x - 0.5 * dx, y - 0.5 * dy, 0.5), (dx, dy, -1.0)

    def away():                                                # leaves upwards from above the surface
        while True:
            (x, y), dx, dy = at(), small(), small()
            yield (x, y, 1.0), (dx, dy, 1.0)

    def beside():                                              # comes down beside the footprint
        while True:
            _, dx, dy = at(), small(), small()
            yield (1.5 + rng.random(), 2.5 + rng.random(), 3.0), (abs(dx), abs(dy), -1.0)

    return [("down", vertical(-1.0)), ("up", vertical(1.0)), ("+x", along(0, 1.0)), ("-x", along(0, -1.0)), ("+y", along(1, 1.0)),
            ("-y", along(1, -1.0)), ("one zero", zeros(1)), ("two zeros", zeros(2)), ("tie", tie()), ("near", near()), ("away", away()),
            ("beside", beside()), ("down", vertical(-1.0)), ("up", vertical(1.0))]


def rays_family():
    import make_golden_rays as gr
    started = time.time()
    out, names = {}, []
    for order in ou.dispatched("rays"):
        rng = rng_of("rays", order)
        ncells = ncells_of(order)
        s = gr.graph(order, ncells, amp=0.05, seed=int(rng.integers(1 << 30)), double=1 if doubled("rays", order) else None)
        b0, b1, windows = gr.exact_windows(s)
        widths = [np.diff(np.unique(s[f"knots{a}"])) for a in range(2)]
        assert all(len(np.unique(np.round(w, 6))) == len(w) for w in widths), "unequal widths"
        kept, hits_of = [], []
        for kind, draws in ray_kinds(rng, s):
            for _ in range(200):
                o, d = (np.asarray(x, np.float64) for x in next(draws))
                try:
                    hits = gr.exact_hits(s, b0, b1, windows, o, d, 0.0, gr.INF)
                except ArithmeticError:
                    continue
                if not gr.within_bars(hits, s, o, d, 0.0) or (len(hits) == 0) != (kind in ("away", "beside")):
                    continue
                kept.append((kind, o, d))
                hits_of.append(hits)
                break
            else:
                raise AssertionError(f"rays {order}: no {kind} ray")
        kinds = [k for k, _, _ in kept]
        cut = kinds.index("near")
        t_cut = max(float(h["t"]) for h in hits_of[cut])
        tmin = float(np.round(1.5 * t_cut * 64) / 64)
        others = [float(h["t"]) for n, hits in enumerate(hits_of) if n != cut for h in hits]
        assert t_cut < tmin < 1.0 < min(others), (order, t_cut, tmin, min(others))
        dominant = {(int(np.argmax(np.abs(d))), float(np.sign(d[np.argmax(np.abs(d))]))) for _, _, d in kept}
        assert dominant == {(a, sg) for a in range(3) for sg in (-1.0, 1.0)}, dominant
        assert sorted(int((d == 0).sum()) for _, _, d in kept)[-2:] == [1, 2] and any(abs(d[0]) == abs(d[2]) for _, _, d in kept)
        name = ou.case_id(order)
        rec = gr.build(name, s, iter([(o, d) for _, o, d in kept]), want=len(kept), tmin=tmin)
        count = np.bincount(rec[name + "/hit_ray"], minlength=len(kept))
        assert rec[name + "/origins"].shape == (3, 14) and (count > 0).sum() >= 8 and (count == 0).sum() >= 2 and count[cut] == 0
        assert all((count[n] == 0) == (k in ("near", "away", "beside")) for n, k in enumerate(kinds))
        out.update(rec)
        names.append(name)
        print(f"rays {order}: {ncells} cells, {int((count > 0).sum())} rays hit, {int((count == 0).sum())} miss, tmin {tmin}, "
              f"{time.time() - started:.0f} s", flush=True)
    assert names == [ou.case_id(t) for t in ou.dispatched("rays")]
    out["names"] = np.array(names)
    store("rays", out, started)


# ------------------------------------------------------------------------------------------ surfaces
def surface_pairs():
    """Pairs (oa, ob) of surface orders whose line families' (KR; K1, K2) cover every dispatched triple, chosen greedily: the
    pair that adds the most new triples, the first such in sorted order.  Every (K1, K2) needs all KR, and one pair brings
    the two orders of one surface only, so no choice has fewer than two pairs per (K1, K2): 9 for orders 2 .. 4."""
    import bspy_amd.surfaces as S
    want = set(ou.dispatched("surfaces"))
    orders = sorted(itertools.product(range(S.MIN_K, S.MAX_K + 1), repeat=2))
    pairs, covered = [], set()
    while covered != want:
        best = max(((oa, ob) for oa in orders for ob in orders), key=lambda p: len(set(ou.triples_of(*p)) - covered))
        pairs.append(best)
        covered |= set(ou.triples_of(*best))
    return pairs


def surfaces_case(item):
    """(entries, log line) of one pair of orders: a is a gentle graph over 2 x 2 cells, b a tilted sheet over 2 x 1 cells whose
    footprint lies in the middle of a's, so that the curve crosses b from side to side through the middle of both."""
    import surfaces_ref as sr
    double, (oa, ob) = item
    started = time.time()
    rng = rng_of("surfaces", oa + ob)
    for draw in range(40):
        e = rng.uniform(-0.02, 0.02, 8)
        a = sr.patch(oa, ([0.0, 0.45 + e[0], 1.0], [0.0, 0.55 + e[1], 1.0]), lambda u, v: u, lambda u, v: v,
                     lambda u, v: 0.06 * np.sin(3.0 * u + 1.0) * np.cos(2.0 * v))
        bknots = None
        if not double:
            bbreaks = ([0.0, 0.6 + e[2], 1.0], [0.0, 1.0])
        else:
            t = 0.6 + e[2]
            bbreaks, bknots = None, [np.array([0.0] * ob[0] + [t, t] + [1.0] * ob[0]), sr.knots_of(ob[1], [0.0, 1.0])]
        b = sr.patch(ob, bbreaks, lambda s, t: 0.17 + e[3] + 0.61 * s + 0.05 * t, lambda s, t: 0.21 + e[4] + 0.04 * s + 0.56 * t,
                     lambda s, t: (0.25 + e[5]) * (s - 0.5) - (0.22 + e[6]) * (t - 0.5) + 0.03 + e[7], knots=bknots)
        rec = {}
        name = f"{ou.case_id(oa)}_{ou.case_id(ob)}"
        try:
            verts, findings = sr.record(rec, name, dict(a=a, b=b, depth=1, kind="sweep"))
        except (ArithmeticError, AssertionError):
            continue
        per = [sum(z["fam"] == f for z in verts) for f in range(4)]
        apart = all(abs(p["w"] - q["w"]) >= Fraction(1, 1000) for p in verts for q in verts
                    if p is not q and (p["fam"], p["n"]) == (q["fam"], q["n"]))
        if min(per) >= 2 and not findings and apart:
            return rec, f"surfaces {oa} x {ob}: vertices per line family {per}, draw {draw}, {time.time() - started:.0f} s"
    raise AssertionError(f"surfaces {oa} x {ob}: no draw with content")


def surfaces_family():
    started = time.time()
    pairs = surface_pairs()
    first = next(n for n, (_, ob) in enumerate(pairs) if ob[0] >= 3)       # the double knot: b's first variable stays continuous
    out = {}
    for rec, line in pool_map(surfaces_case, [(n == first, p) for n, p in enumerate(pairs)]):
        out.update(rec)
        print(line, flush=True)
    assert set().union(*(ou.triples_of(*p) for p in pairs)) == set(ou.dispatched("surfaces"))
    out["names"] = np.array([f"{ou.case_id(oa)}_{ou.case_id(ob)}" for oa, ob in pairs])
    print(f"surfaces: {len(pairs)} pairs for {len(ou.dispatched('surfaces'))} triples")
    store("surfaces", out, started)


FAMILIES = {"zeros2": lambda: zeros_family(2), "zeros3": lambda: zeros_family(3), "contours": contours_family, "project": project_family,
            "rays": rays_family, "surfaces": surfaces_family}


def main(argv):
    for family in argv or ou.FAMILIES:
        FAMILIES[family]()


if __name__ == "__main__":
    main(sys.argv[1:])
