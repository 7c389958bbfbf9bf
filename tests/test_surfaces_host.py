"""
Spline.intersect_surface and surfaces.trace_pair on the host path (no GPU): every golden of tests/golden/surfaces.npz
against what is exactly true (tests/surfaces_ref.py: every pair's system formed in rationals and solved by the certified
oracle tests/zeros3_ref.py); the pure-Python statement of bspy_amd/surfaces.py against the host drivers, bit for bit; the
invariances (prefilter, chunks, passes, scale); scope, arguments and the warning rule.

The bar (derived, not tuned), in cell-local units of the pair's three variables.  A reported zero r of the pair's system
F, evaluated exactly at the reported doubles, Y the certificate's preconditioner, must have
    2 |Y F(r)| <= 8 (KR + K1 + K2) eps max_i sum_d |Y_id| S_d + 4 eps max_i max(|a_i|, |b_i|) / h_i
``roots3``'s coupled bar with S_d = max |a's d| + max |b's d|, which bounds every formed
coefficient; forming one is a single rounded subtraction of size <= S_d and a line point is K - 1 more lerps of the kind
the walk makes anyway.  The vertices are float64 (no rounding to the knots' dtype), so float32 knots add nothing.  The
oracle's bracket (the certificate's radius) is added where the distance to the recorded centre is measured.
In space: a(u, v) - b(s, t) evaluated in rationals at the vertex is F(r) of ITS pair up to the exactness of the fixed
coordinate (the canonical float of the line against the exact line, eps |t|), so |a - b|_d <= sum_axis D_d,axis (bar +
eps max|t| / h), D the largest Bernstein coefficient of the derivative of component d of a or b per unit of the cell.
"""
from fractions import Fraction

import numpy as np
import pytest

import bspy_amd
import surfaces_ref
import zeros3_ref
from bspy_amd import _cells, contours, surfaces
from bspy_amd import _native as nv
from conftest import observe
from surfaces_util import GOLD, NAMES, PER_PAIR, lipschitz, load_case, make, same, same_result

EPS = float(np.finfo(np.float64).eps)


_RUNS = {}


def run(name):
    """trace_pair of a golden on the host path, once per session."""
    if name not in _RUNS:
        c = load_case(name)
        a, b = make(c)
        _RUNS[name] = (c, a, b, surfaces.trace_pair(a, b, depth=c["depth"], _path="host"), list(surfaces.LAST_PATHS))
    return _RUNS[name]


def ranked(info, plans):
    """[(fam, n, rank)] of the library's vertices (key order), ranked along their line by the running coordinate."""
    ids = []
    for f, res in enumerate(info["families"]):
        X = plans[0] if f < 2 else plans[1]
        ncrun = X.ncells[1 - (f & 1)]
        at = np.argwhere(res["keep"] != 0)
        n = res["pair_seg"][at[:, 0]].astype(np.int64) // ncrun
        w = res["roots"][at[:, 0], at[:, 1], 0]
        rank = np.zeros(len(n), np.int64)
        for line in np.unique(n):
            mine = np.flatnonzero(n == line)
            rank[mine[np.argsort(w[mine], kind="stable")]] = np.arange(len(mine))
        ids += [(f, int(a), int(b)) for a, b in zip(n, rank)]
    return ids


# ------------------------------------------------------------------------------------------ statement against the drivers
@pytest.mark.parametrize("name", NAMES)
def test_statement_and_host_drivers_agree_bit_for_bit(name):
    c, a, b, res, _ = run(name)
    info = res[4]
    be = _cells.Host()
    tabs = [surfaces.Tables(be, *surfaces.host_tables(s)) for s in (a, b)]
    scale = tabs[0].cmax + tabs[1].cmax
    stated = []
    for fam in range(4):
        X, Y = (tabs[0], tabs[1]) if fam < 2 else (tabs[1], tabs[0])
        want = surfaces.statement_family(X, Y, fam & 1, c["depth"], scale)
        for key in PER_PAIR:
            assert same(want[key], info["families"][fam][key]), (name, fam, key)
        stated.append(want)
    plans = [t.plan for t in tabs]
    verts, _, _, leaves = surfaces.vertices_of(stated, plans, c["depth"])
    points, offsets, closed, findings = surfaces.link(leaves)
    assert same(verts[points].reshape(-1, 4), res[0]) and same(offsets, res[1]) and same(closed, res[2]) and same(findings, res[3].leaves)


# ------------------------------------------------------------------------------------------ against the exact oracle
_ROWS = {}


def vertex_rows(name):
    """Per vertex of the library (key order): dict(vid, k, fam, F, t0, h, local, x, radius, cert, bar, cellterm, S), the bar of
    this file's docstring in cell-local units; once per session."""
    if name not in _ROWS:
        c, a, b, res, _ = run(name)
        info = res[4]
        plans = [surfaces.Plan(s.order, s.knots) for s in (a, b)]
        G = 1 << c["depth"]
        ids = ranked(info, plans)
        want = [tuple(int(x) for x in row) for row in c["vert_id"]]
        assert sorted(ids) == sorted(want), (name, "the vertices per lattice line")
        A, B = surfaces_ref.Surface(a.order, a.knots, a.coefs), surfaces_ref.Surface(b.order, b.knots, b.coefs)
        cmax = [np.abs(np.asarray(s.coefs, np.float64)).max(axis=(1, 2)) for s in (a, b)]
        S = cmax[0] + cmax[1]
        where = {v: k for k, v in enumerate(want)}
        V = info["vertices"]
        rows = []
        for k, vid in enumerate(ids):
            fam, n, _ = vid
            ax, g = fam & 1, where[vid]
            X, Y = (A, B) if fam < 2 else (B, A)
            run_col = (1 - ax) if fam < 2 else (3 - ax)
            seg, cell = (int(x) for x in c["vert_pair"][g])
            F, (t0, h), _, _ = surfaces_ref.pair_system(X, Y, ax, G, seg, cell)
            zero = (V[k, run_col],) + ((V[k, 2], V[k, 3]) if fam < 2 else (V[k, 0], V[k, 1]))
            local = [(Fraction(float(z)) - t0[m]) / h[m] for m, z in enumerate(zero)]
            x, radius = [Fraction(float(v)) for v in c["vert_x"][g]], Fraction(float(c["vert_radius"][g]))
            cert = dict(lo=tuple(max(Fraction(0), v - radius) for v in x), hi=tuple(min(Fraction(1), v + radius) for v in x),
                        Y=[[Fraction(float(v)) for v in row] for row in c["vert_Y"][g]])
            ys = max(sum(abs(float(cert["Y"][m][d])) * S[d] for d in range(3)) for m in range(3))
            cellterm = max(max(abs(float(t0[m])), abs(float(t0[m] + h[m]))) / float(h[m]) for m in range(3))
            KR, K1, K2 = F[0].shape
            rows.append(dict(vid=vid, k=k, fam=fam, n=n, ax=ax, F=F, t0=t0, h=h, local=local, x=x, radius=radius, cert=cert,
                             bar=8 * (KR + K1 + K2) * EPS * ys + 4 * EPS * cellterm, cellterm=cellterm, S=S, X=X, A=A, B=B))
        _ROWS[name] = rows, ids, want
    return _ROWS[name]


@pytest.mark.parametrize("name", [n for n in NAMES if str(GOLD[n + "/kind"]) not in ("edge", "corner", "flat")])
def test_counts_bars_segments_and_components_are_the_exact_ones(name):
    c, a, b, res, _ = run(name)
    vertices, offsets, closed, status, info = res
    G = 1 << c["depth"]
    rows, ids, want = vertex_rows(name)
    V = info["vertices"]
    worst = worst_xyz = 0.0
    for r in rows:
        k, fam, ax, n, F, bar, S = r["k"], r["fam"], r["ax"], r["n"], r["F"], r["bar"], r["S"]
        # the fixed coordinate against the oracle's exact line, not against the function that wrote it: equal at x = 0 and
        # x = 1 (a break), else (1 - x) t0 + x t1 in floats: two rounded products and a rounded sum, below 2 eps max |t|
        fixed_col = ax if fam < 2 else 2 + ax
        breaks = r["X"].breaks[ax]
        exact = surfaces_ref.line_value(breaks, n, G)
        _, x = surfaces_ref.owner(n, G, len(breaks) - 1)
        slack = 0 if x in (0, 1) else 2 * EPS * max(abs(float(t)) for t in breaks)
        assert abs(Fraction(float(V[k, fixed_col])) - exact) <= slack, (name, r["vid"], "fixed coordinate")
        assert V[k, fixed_col].tobytes() == surfaces.line_values([float(t) for t in breaks], G)[n].tobytes()
        err = float(zeros3_ref.error_bound(F, r["cert"], r["local"]))
        worst = max(worst, err / bar)
        assert max(abs(float(r["local"][m] - r["x"][m])) for m in range(3)) <= bar + float(r["radius"]), (name, r["vid"], "distance to the recorded zero")
        # independently of the pair's frame: a(u, v) - b(s, t) in rationals
        pa, pb = r["A"].value(*(Fraction(float(z)) for z in V[k, :2])), r["B"].value(*(Fraction(float(z)) for z in V[k, 2:]))
        for d in range(3):
            slope = sum(max(abs(float(v)) for v in zeros3_ref.derivative(F[d], m).reshape(-1)) for m in range(3))
            worst_xyz = max(worst_xyz, abs(float(pa[d] - pb[d])) / (slope * (bar + EPS * r["cellterm"]) + 4 * EPS * S[d]))
    if ids:
        observe(f"surfaces zero / bar, {name}", worst, 1.0)
        observe(f"surfaces |a - b| / bar, {name}", worst_xyz, 1.0)
    # the segment set, the components and the findings
    index = {v: k for k, v in enumerate(ids)}
    back = [index[v] for v in want]                            # oracle vertex -> library vertex
    got_segments, got_components = set(), []
    for m in range(len(offsets) - 1):
        chain = [int(np.flatnonzero((V == row).all(axis=1))[0]) for row in vertices[offsets[m]:offsets[m + 1]]]
        got_segments |= {frozenset(p) for p in zip(chain[:-1], chain[1:])}
        got_components.append((bool(closed[m]), frozenset(chain)))
        assert (chain[0] == chain[-1] and len(chain) > 2) == bool(closed[m])
    assert got_segments == {frozenset(back[v] for v in s) for s in c["segments"]}, (name, "segments")
    off = c["comp_offsets"]
    want_components = [(bool(c["comp_closed"][m]), frozenset(back[v] for v in c["comp_vertices"][off[m]:off[m + 1]])) for m in range(len(off) - 1)]
    assert sorted(got_components, key=lambda p: min(p[1])) == sorted(want_components, key=lambda p: min(p[1])), (name, "components")
    assert same(status.leaves, c["findings"]), (name, "findings")
    assert not (status.bits & 31), (name, "a pair carries a status bit")


def test_kinds():
    """What each special case is: loop, open chain, no hits, coincident region, two pieces in one leaf."""
    c, a, b, (vertices, offsets, closed, status, info), paths = run("loop")
    assert closed.tolist() == [True] and status.bits == 0 and same(vertices[0], vertices[-1])
    leaves = info["leaves"]
    assert (leaves >= 0).all()                                 # every vertex bounds two leaves: degree 2
    c, a, b, (vertices, offsets, closed, status, info), paths = run("open_b")
    assert closed.tolist() == [False] and status.bits == 0
    for end in (vertices[0], vertices[-1]):                   # the chain ends on boundary lines of b, inside a
        on_b = [end[2] in (0.0, 1.0), end[3] in (0.0, 1.0)]
        assert any(on_b) and 0.0 < end[0] < 1.0 and 0.0 < end[1] < 1.0
    for name in ("disjoint", "overlap_nohit"):
        c, a, b, (vertices, offsets, closed, status, info), paths = run(name)
        assert len(vertices) == 0 and len(offsets) == 1 and status.bits == 0
    assert run("disjoint")[4][-1] == "host ssx_count" and run("disjoint")[3][4]["candidates"] == 0
    assert run("overlap_nohit")[3][4]["candidates"] > 0       # boxes overlap: pairs were walked and held nothing
    c, a, b, (vertices, offsets, closed, status, info), paths = run("coincident")
    assert status.bits == surfaces.STATUS_FLAT and len(vertices) == 0 and info["candidates"] > 0 and info["nodes"] == 0
    c, a, b, (vertices, offsets, closed, status, info), paths = run("two_in_leaf")
    assert status.bits == surfaces.STATUS_MANY and len(offsets) == 1 and len(info["vertices"]) == 4
    # plane_d0: two branches through one product leaf, and chains that run into it: each chain ends at a vertex that bounds
    # the leaf with bit 64, where no segment is made
    c, a, b, (vertices, offsets, closed, status, info), paths = run("plane_d0")
    assert status.bits == surfaces.STATUS_MANY and len(status.leaves) == 1 and len(offsets) - 1 == 3 and not closed.any()
    many = int(status.leaves[0, 0])
    V, leaves = info["vertices"], info["leaves"]
    inside = {k for k in range(len(V)) if many in leaves[k].tolist()}
    assert len(inside) >= 3
    for m in range(len(offsets) - 1):
        chain = [int(np.flatnonzero((V == row).all(axis=1))[0]) for row in vertices[offsets[m]:offsets[m + 1]]]
        assert chain[0] in inside or chain[-1] in inside, (m, chain)
        assert not any(k in inside for k in chain[1:-1])
    assert inside <= {int(np.flatnonzero((V == row).all(axis=1))[0]) for m in range(len(offsets) - 1)
                      for row in (vertices[offsets[m]], vertices[offsets[m + 1] - 1])}


@pytest.mark.parametrize("name", ["edge", "corner"])
def test_a_hit_on_a_cell_edge_or_corner_of_the_other_surface_is_merged(name):
    c, a, b, (vertices, offsets, closed, status, info), paths = run(name)
    fam = info["families"][0]                                  # a's lines with u fixed; line n = 1 is u = 1/2
    mine = np.flatnonzero(fam["pair_seg"] == 1)
    raw = int(fam["count"][mine].sum())
    kept = int(fam["keep"][mine].sum())
    assert raw == (2 if name == "edge" else 4) and kept == 1, (raw, kept)
    assert "host ssx_merge" in paths
    at = np.argwhere(fam["keep"][mine] != 0)[0]
    w, s, t = fam["roots"][mine[at[0]], at[1]]
    assert max(abs(w - c["point"][1]), abs(s - c["point"][2]), abs(t - c["point"][3])) <= 64 * EPS
    assert int(fam["pair_cell"][mine[at[0]]]) == 0             # the lowest cell keeps it


@pytest.mark.parametrize("name", ["plane_d0", "plane_d1", "plane_d2"])
def test_plane_section_agrees_with_contours_on_the_same_lattice(name):
    """b's lattice lines against the plane a are the lattice edges of ``contours`` of the field f = n . (b - p0) on b's
    lattice: the same count per line and each vertex within the sum of the two bars, in the moving parameter:
      ours       the bar of this file's docstring for the vertex's own pair, times the width of its running cell;
      contours'  2 (K0 + K1) eps S_f / |df/ds| + 4 eps max |domain end| (tests/test_contours_host.py), S_f = max |coefficient of
                 f|, df/ds the derivative of the exact field along the line at the vertex, per unit of the parameter;
      the field  f is built here in floats and a's four corners are floats too, so the zero set of the field that ``contours``
                 sees is not the intersection: every coefficient of f carries the rounding of the cross product, the dot
                 product and the subtraction, below 8 eps sum_d |n_d| (max |b_d| + |p0_d|), and a's fourth corner lies off
                 the plane of the other three by |n . (p11 - p0)| (measured exactly); both displace the zero by their sum
                 over |df/ds|.
    ``contours`` sees a lattice edge's crossing through the signs of its two nodes: one vertex when the edge holds an odd
    number of crossings, none when it holds two (its docstring: not promised).  plane_d0 has such an edge on t = 0.45, so
    there the counts agree per edge modulo 2; at depths 1 and 2 the counts per line are equal."""
    c, a, b, (vertices, offsets, closed, status, info), paths = run(name)
    rows, ids, _ = vertex_rows(name)
    P = np.asarray(a.coefs, np.float64)
    p0, e1, e2 = P[:, 0, 0], P[:, 1, 0] - P[:, 0, 0], P[:, 0, 1] - P[:, 0, 0]
    normal = np.cross(e1, e2)
    bc = np.asarray(b.coefs, np.float64)
    field = np.tensordot(normal, bc, 1) - normal @ p0
    f = bspy_amd.Spline(2, 1, b.order, b.nCoef, b.knots, field[None])
    cv, coff, _, _, _, _ = contours.trace_batch(f, depth=c["depth"], _path="host")
    G = 1 << c["depth"]
    plan = surfaces.Plan(b.order, b.knots)
    lines = [surfaces.line_values(plan.breaks[ax], G) for ax in range(2)]
    V = info["vertices"]
    nf = [Fraction(float(x)) for x in normal]
    twist = abs(float(sum(nf[d] * (Fraction(float(P[d, 1, 1])) - Fraction(float(p0[d]))) for d in range(3))))
    forming = 8 * EPS * float(sum(abs(normal[d]) * (np.abs(bc[d]).max() + abs(p0[d])) for d in range(3))) + twist
    ends = max(max(abs(float(br[0])), abs(float(br[-1]))) for br in plan.breaks)
    B = rows[0]["B"]
    pts = np.unique(cv, axis=0)
    worst = 0.0
    for ax in range(2):
        mine = [r for r in rows if r["fam"] == 2 + ax]
        for n, value in enumerate(lines[ax]):
            theirs = np.sort(pts[pts[:, ax] == value][:, 1 - ax])
            on_line = [r for r in mine if r["n"] == n]
            ours = np.array([V[r["k"], 3 - ax] for r in on_line])
            edge = np.searchsorted(lines[1 - ax], ours, "right")
            their_edge = np.searchsorted(lines[1 - ax], theirs, "right")
            if name != "plane_d0":
                assert len(theirs) == len(ours), (name, ax, n)
            for e in np.unique(np.concatenate((edge, their_edge))):
                assert np.count_nonzero(their_edge == e) == np.count_nonzero(edge == e) % 2, (name, ax, n, e)
            for x in theirs:
                r = on_line[int(np.abs(ours - x).argmin())]
                st = [Fraction(float(z)) for z in V[r["k"], 2:]]
                step = Fraction(1, 2 ** 20)
                moved = list(st)
                moved[1 - ax] += step if st[1 - ax] + step <= Fraction(float(plan.breaks[1 - ax][-1])) else -step
                # |df/ds| of the exact field along the line: a difference quotient of the exact surface over 2^-20, whose
                # own error (second derivative times 2^-21) is far below the slope on these cases
                slope = abs(float(sum(nf[d] * (B.value(*moved)[d] - B.value(*st)[d]) for d in range(3)) / (moved[1 - ax] - st[1 - ax])))
                K0, K1 = plan.order
                bar = r["bar"] * float(r["h"][0]) + 2 * (K0 + K1) * EPS * float(np.abs(field).max()) / slope + 4 * EPS * ends + forming / slope
                worst = max(worst, abs(float(V[r["k"], 3 - ax]) - float(x)) / bar)
    observe(f"surfaces against contours / sum of the bars, {name}", worst, 1.0)


# ------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("name", NAMES)
def test_prefilter_chunks_and_passes_change_no_byte(name):
    c, a, b, res, _ = run(name)
    again = surfaces.trace_pair(a, b, depth=c["depth"], _path="host")
    assert same_result(res, again)
    for kw in (dict(_prefilter=False), dict(_chunk=1), dict(_chunk=7), dict(_chunk=10 ** 6), dict(_pairs=3)):
        assert same_result(res, surfaces.trace_pair(a, b, depth=c["depth"], _path="host", **kw)), (name, kw)
    surfaces.trace_pair(a, b, depth=c["depth"], _path="host", _pairs=3)
    if res[4]["candidates"] > 12:
        assert surfaces.LAST_PATHS.count("host ssx_count") > 4        # the passes were split


@pytest.mark.parametrize("k", [-40, 40])
def test_scaling_both_surfaces_by_a_power_of_two_changes_no_byte(k):
    c, a, b, res, _ = run("plane_d1")
    a2, b2 = make(c, 2.0 ** k)
    assert same_result(res, surfaces.trace_pair(a2, b2, depth=c["depth"], _path="host"))


# ------------------------------------------------------------------------------------------ the public call
def test_scope_and_errors():
    c, a, b, _, _ = run("plane_d1")
    curve = bspy_amd.Spline(1, 3, [3], [3], [np.array([0, 0, 0, 1, 1, 1.0])], np.zeros((3, 3)))
    k5 = np.array([0.0] * 5 + [1.0] * 5)
    quintic = bspy_amd.Spline(2, 3, [5, 5], [5, 5], [k5, k5], np.zeros((3, 5, 5)))
    for other in (curve, quintic, 3.0):
        with pytest.raises(NotImplementedError, match="orders 2 to 4"):
            a.intersect_surface(other)
        with pytest.raises(NotImplementedError, match="orders 2 to 4"):
            surfaces.trace_pair(a, other)
    jump = bspy_amd.Spline(2, 3, [2, 2], [4, 2], [np.array([0, 0, 0.5, 0.5, 1, 1.0]), np.array([0, 0, 1, 1.0])], np.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match="knot 0.5 of variable 0 has multiplicity 2"):
        a.intersect_surface(jump)
    with pytest.raises(ValueError, match="depth must be in 0 .. 6"):
        surfaces.trace_pair(a, b, depth=7)
    with pytest.raises(ValueError, match="_chunk and _pairs"):
        surfaces.trace_pair(a, b, _chunk=0)
    with pytest.raises(ValueError, match="_path"):
        surfaces.trace_pair(a, b, _path="gpu")
    n = (1 << 15) // 64 + 1
    knots = np.concatenate(([0.0], np.linspace(0.0, 1.0, n + 1), [1.0]))
    long = bspy_amd.Spline(2, 3, [2, 2], [n + 1, 2], [knots, np.array([0, 0, 1, 1.0])], np.zeros((3, n + 1, 2)))
    with pytest.raises(ValueError, match="more than 32768 leaves along one variable"):
        surfaces.trace_pair(a, long, depth=6)
    assert surfaces.depth_of(None, []) == 2 and hasattr(nv.lib(), "bsk_ssx_last_kernel")
    assert surfaces.roots3.WALK == nv.lib().bsk_roots3_walk_bound()


@pytest.mark.parametrize("name", ["loop", "open_b", "plane_d2", "cells5x4"])
def test_the_polyline_stays_within_the_sagitta_bound_in_space(name):
    """The reference of the curve test of tests/test_gpu_surfaces.py alone: the polyline, linear in the chord parameter
    that ``fit_pair`` uses, at 33 values.  A chord of one leaf leaves the true curve by at most the sagitta
    (h 2^-depth)^2 / L in its own parameters (``contours.depth_of``'s rule, L the larger extent of the domain), so the
    two points in space differ by no more than (M_a + M_b) (h 2^-depth)^2 / L (1 + L), M the bound ``lipschitz``."""
    c, a, b, (vertices, offsets, closed, status, info), _ = run(name)
    plans = [surfaces.Plan(s.order, s.knots) for s in (a, b)]
    L = max(float(br[-1]) - float(br[0]) for plan in plans for br in plan.breaks)
    tol = max((float(np.diff(np.asarray(br, np.float64)).max()) * 2.0 ** -c["depth"]) ** 2 / L for plan in plans for br in plan.breaks)
    bound = (lipschitz(a) + lipschitz(b)) * tol * (1.0 + L)
    t = np.linspace(0.0, 1.0, 33)
    for m in range(len(offsets) - 1):
        pts = vertices[offsets[m]:offsets[m + 1]]
        xyz = surfaces._evaluate(a, pts[:, 0], pts[:, 1])
        chord = np.concatenate(([0.0], np.cumsum(np.sqrt((np.diff(xyz, axis=0) ** 2).sum(axis=1)))))
        q = np.stack([np.interp(t, chord / chord[-1], pts[:, k]) for k in range(4)])
        gap = np.abs(surfaces._evaluate(a, q[0], q[1]) - surfaces._evaluate(b, q[2], q[3])).max()
        observe(f"surfaces polyline |a - b| / bound, {name}", gap / bound, 1.0)


def test_status_bits_warn_once_and_never_raise():
    c, a, b, _, _ = run("two_in_leaf")
    with pytest.warns(RuntimeWarning, match="more than two vertices in one product leaf") as record:
        found = a.intersect_surface(b, depth=0, _path="host")
    assert found == [] and len(record) == 1
    c, a, b, _, _ = run("coincident")
    with pytest.warns(RuntimeWarning, match="coincident"):
        assert a.intersect_surface(b, depth=0, _path="host") == []
