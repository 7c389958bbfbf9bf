"""
``Spline.isosurface`` without a GPU: the host drivers (the functions of bsk_iso.hpp on the CPU) against the exact oracle
tests/iso_ref.py as recorded in tests/golden/iso.npz, against the Python statement of bspy_amd/isosurface.py bit for bit,
and against themselves at every split level.  ``normals=True`` needs ``jacobian`` and so the device: test_gpu_iso.py.

THE BAR OF A VERTEX.  A vertex lies on a lattice edge; on an axis edge its two fixed coordinates are bit-equal to their
lattice planes (asserted).  Along the edge it is the root of the cell's polynomial, found by sign bisection of float values:
  * a sign of a float value is wrong only where the exact value is below the rounding of the evaluation.  Counted from
    the stated association, first order, S = max |coefficient|, eps = 2^-52 (unit roundoff eps / 2): a lerp s a + t b with
    a rounded s = 1 - x costs 3 roundings, 1.5 eps S, and a value is K0 + K1 + K2 - 3 levels of them whatever the order of
    the axes: 1.5 (K0 + K1 + K2 - 3) eps S; the host's Bezier extraction sums at most K products per axis with rounded
    weights, (K + 1) eps S / 2 per axis; subtracting the level rounds once more on values up to 2 S: eps S.  Together
    2 (K0 + K1 + K2) - 2 < c = 2 (K0 + K1 + K2).  The bisection therefore stops within c eps S / |df/ds| of the exact
    root in the edge's own parameter s, |df/ds| the exact derivative along the edge at the root (recorded), which is
    (h_a / G) times that along axis a (recorded as the edge's reach);
  * y = a / G + s / G, 1 - y, the two products and the sum of the map to the parameters, and the last step of the
    bisection (half an eps of the edge): 4 eps max |domain end| covers them;
  * the oracle's own bracket of the exact root (at most 2^-70 of the edge) and the rounding of its middle to a double.
The generator asserts what this first-order statement needs: one root per crossed edge, no undecidable node value.
"""
import os
import re

import numpy as np
import pytest

import bspy_amd
import iso_ref
import oracle
from bspy_amd import _native as nv
from bspy_amd import isosurface as iso
from conftest import observe
from iso_cases import GOLD, NAMES, ORDERS, directed_edges, drawn, levels_of, same, spline_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
FAMILY = ("bsk_iso_flag_host", "bsk_iso_flag", "bsk_iso_walk_host", "bsk_iso_walk", "bsk_iso_leaf_host", "bsk_iso_leaf",
          "bsk_iso_vertex_host", "bsk_iso_vertex", "bsk_iso_last_kernel")
PAIRS = [(name, b) for name in NAMES for b in range(len(GOLD[f"{name}/levels"]))]

_RAW = {}


def raw(name, split=None):
    """The host drivers' raw result of a case (computed once per split level and shared, never changed)."""
    if (name, split) not in _RAW:
        plan, rows, levels, scale = iso.tables(spline_of(name), levels_of(name))
        _RAW[name, split] = (plan, rows, levels, scale, iso._run_host(rows, plan, levels, scale, int(GOLD[f"{name}/depth"]), split))
    return _RAW[name, split]


def field(res, b):
    """(keys, xyz, triangles as key triples, triangles as indices into the field's own vertices) of field b."""
    v0, v1 = res["vertex_offsets"][b:b + 2]
    t0, t1 = res["triangle_offsets"][b:b + 2]
    return res["keys"][v0:v1], res["xyz"][v0:v1], res["keys"][res["triangles"][t0:t1]], res["triangles"][t0:t1] - v0


def test_the_cases_are_the_ones_the_issue_lists():
    assert {"plane_d0", "plane_d1", "plane", "sphere", "sphere_cut", "random_444", "random_234", "random_423", "crease", "diagonal",
            "zero_cell", "float32", "shifted", "levels"} <= set(NAMES)
    assert [int(GOLD[f"{n}/depth"]) for n in ("plane_d0", "plane_d1", "plane")] == [0, 1, 3]
    assert all(GOLD[f"{n}/order"].tolist() == [2, 2, 2] for n in ("plane_d0", "plane_d1", "plane"))
    cells = lambda n: [len(np.unique(GOLD[f"{n}/knots{a}"])) - 1 for a in range(3)]
    assert cells("sphere") == [2, 2, 2] and GOLD["sphere/order"].tolist() == [3, 3, 3] and int(GOLD["sphere/depth"]) == 2
    assert GOLD["sphere/0/topology"].tolist() == [1, 2]
    assert cells("random_444") == [2, 3, 2] and int(GOLD["random_444/depth"]) == 1 and GOLD["random_444/0/topology"][0] >= 2
    assert GOLD["random_234/order"].tolist() == [2, 3, 4] and GOLD["random_423/order"].tolist() == [4, 2, 3]
    assert np.count_nonzero(GOLD["crease/knots0"] == 0.5) == 2 and GOLD["crease/order"][0] == 3
    assert len(GOLD["diagonal/0/zero_nodes"]) > 0 and len(GOLD["zero_cell/0/zero"]) == 1
    assert GOLD["float32/coefs"].dtype == np.float32 and GOLD["float32/knots0"].dtype == np.float32
    assert [GOLD[f"shifted/knots{a}"][[0, -1]].tolist() for a in range(3)] == [[100.0, 103.0], [-40.0, -38.0], [7.0, 8.0]]
    assert np.abs(GOLD["shifted/coefs"]).max() > 4000.0 and len(GOLD["levels/levels"]) == 3
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "iso.npz")) < 200 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_host_drivers_equal_the_statement_at_every_split(name):
    plan, rows, levels, scale, res = raw(name)
    depth = int(GOLD[f"{name}/depth"])
    want = iso.statement(rows, plan, levels, scale, depth)                      # every leaf of every candidate, no pruning
    for split in [None] + list(range(depth + 1)):
        got = raw(name, split)[4]
        for label, value in want.items():
            assert np.asarray(got[label]).tobytes() == value.tobytes(), f"{name}: {label} at split {split}"
        assert got["split"] == (iso.split_of(int(want["cand"].sum()), depth) if split is None else split)


@pytest.mark.parametrize("name,b", PAIRS)
def test_keys_and_triangles_equal_the_oracle(name, b):
    res = raw(name)[4]
    keys, _, triangles, _ = field(res, b)
    assert keys.tobytes() == GOLD[f"{name}/{b}/keys"].tobytes()
    assert triangles.tobytes() == GOLD[f"{name}/{b}/triangles"].tobytes()
    assert np.argwhere(res["zero"][b]).tolist() == GOLD[f"{name}/{b}/zero"].tolist()
    assert np.argwhere(res["status"][b] & iso.STATUS_ZERO_CELL).tolist() == GOLD[f"{name}/{b}/zero"].tolist()
    assert np.argwhere(res["status"][b] & iso.STATUS_ZERO_NODE).tolist() == GOLD[f"{name}/{b}/zero_nodes"].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_the_public_calls_return_the_raw_result(name):
    s, depth = spline_of(name), int(GOLD[f"{name}/depth"])
    res = raw(name)[4]
    out = iso.extract_batch(s, levels=levels_of(name), depth=depth, _path="host")
    assert iso.LAST_PATHS[-6:] == ["host iso_flag", "host iso_walk count", "host iso_walk emit", "host iso_leaf count", "host iso_leaf emit",
                                   "host iso_vertex"]
    assert nv.lib().bsk_iso_last_kernel().decode() == "host iso_vertex"
    for got, label in zip(out, ("xyz", "keys", "vertex_offsets", "triangles", "triangle_offsets", None, "status")):
        if label:
            assert got.tobytes() == np.asarray(res[label]).tobytes(), label
    assert out[0].dtype == np.float64 and out[3].dtype == np.int64 and out[6].dtype == np.uint8
    assert out[5].shape == (sum(len(GOLD[f"{name}/{b}/zero"]) for b in range(len(levels_of(name)))), 7)
    level = levels_of(name)[0]
    vertices, triangles = s.isosurface(level=level, depth=depth, _path="host")
    _, xyz, _, index = field(res, 0)
    assert vertices.tobytes() == xyz.tobytes() and triangles.tobytes() == index.tobytes()


@pytest.mark.parametrize("name,b", PAIRS)
def test_vertices_within_the_derived_bar(name, b):
    plan, _, _, scale, res = raw(name)
    depth = int(GOLD[f"{name}/depth"])
    keys, xyz, _, _ = field(res, b)
    lat = iso.Lattice(None, plan, 0.0, depth)
    c = 2.0 * sum(plan.order)
    S = float(scale[b])
    ends = max(max(abs(float(t[0])), abs(float(t[-1]))) for t in plan.breaks)
    roots, slopes, reach = (GOLD[f"{name}/{b}/{label}"] for label in ("roots", "slopes", "reach"))
    inv = 1.0 / float(1 << depth)
    worst = 0.0
    for n, key in enumerate(keys.tolist()):
        I, J, K, d = lat.unkey(key)
        where = lat.edge_cell(I, J, K, d)
        for axis in range(3):
            if (d >> (2 - axis)) & 1:
                continue
            if d in (1, 2, 4):                                  # an axis edge: the fixed coordinates are the lattice planes
                cell, a = where[axis]
                y = float(a) * inv
                t = plan.breaks[axis]
                assert xyz[n, axis] == (1.0 - y) * float(t[cell]) + y * float(t[cell + 1]), f"{name}: vertex {key} left its lattice plane"
        along = c * EPS * S / slopes[n]
        for axis in range(3):
            bar = along * reach[n, axis] + 4.0 * EPS * ends + float(iso_ref.WIDTH) * reach[n, axis] + 0.5 * EPS * abs(roots[n, axis])
            worst = max(worst, abs(xyz[n, axis] - roots[n, axis]) / bar)
    observe(f"isosurface vertex / derived bar [{name}/{b}]", worst, 1.0)


def on_a_free_plane(lat, plan, depth, zero, key_a, key_b):
    """Both lattice edges lie in one plane of the domain boundary or of a zero cell's boundary."""
    free = set()
    for axis in range(3):
        free |= {(axis, 0), (axis, int(plan.ncells[axis]) << depth)}
    for cell in zero:
        for axis in range(3):
            free |= {(axis, int(cell[axis]) << depth), (axis, (int(cell[axis]) + 1) << depth)}

    def planes(key):
        at = lat.unkey(key)
        return {(axis, at[axis]) for axis in range(3) if not (at[3] >> (2 - axis)) & 1}

    return bool(planes(key_a) & planes(key_b) & free)


@pytest.mark.parametrize("name,b", PAIRS)
def test_the_mesh_is_an_oriented_manifold_with_the_oracles_topology(name, b):
    plan, _, _, _, res = raw(name)
    depth = int(GOLD[f"{name}/depth"])
    keys, _, _, index = field(res, b)
    lat = iso.Lattice(None, plan, 0.0, depth)
    edges = directed_edges(index)
    assert max(edges.values()) == 1                              # every directed edge at most once
    zero = GOLD[f"{name}/{b}/zero"]
    open_edges = 0
    for (p, q) in edges:
        if (q, p) not in edges:
            open_edges += 1
            assert on_a_free_plane(lat, plan, depth, zero, int(keys[p]), int(keys[q])), f"{name}: the edge {keys[p]} -> {keys[q]} has no partner"
    ncomp, chi = iso_ref.topology([tuple(t) for t in index.tolist()])
    assert [ncomp, chi] == GOLD[f"{name}/{b}/topology"].tolist()
    assert len(keys) - (len(edges) + open_edges) // 2 + len(index) == chi
    if name == "sphere":
        assert open_edges == 0 and chi == 2 and ncomp == 1


@pytest.mark.parametrize("name,b", [(n, b) for n, b in PAIRS if f"{n}/centre" in GOLD.files or f"{n}/normal" in GOLD.files])
def test_normals_point_into_the_positive_side(name, b):
    _, xyz, _, index = field(raw(name)[4], b)
    corners = xyz[index]
    normal = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    if f"{name}/centre" in GOLD.files:
        gradient = 2.0 * (corners.mean(axis=1) - GOLD[f"{name}/centre"])      # of |x - c|^2 - r^2, exactly
    else:
        gradient = GOLD[f"{name}/normal"][None]
    dots = (normal * gradient).sum(axis=1)
    area = np.linalg.norm(normal, axis=1)
    # a triangle of zero area has no normal (the statement does not remove them); every other one faces f >= 0
    assert np.all(dots[area > 1e-30] > 0.0) and np.count_nonzero(area > 1e-30) >= len(index) // 2


@pytest.mark.parametrize("name,b", PAIRS)
def test_the_field_vanishes_at_the_vertices(name, b):
    """|f(vertex) - level| against the value form of the bar: c eps S for the bisection, the evaluator's own
    (K0 + K1 + K2) eps S, and the 4 eps max |domain end| per axis of the map times a bound of |df/du_a|:
    (K_a - 1) max |difference of adjacent coefficients| / the narrowest knot cell."""
    plan, _, _, scale, res = raw(name)
    _, xyz, _, _ = field(res, b)
    s = spline_of(name)
    coefs = np.asarray(s.coefs, np.float64)
    knots = [np.asarray(k, np.float64) for k in s.knots]
    values, bad = oracle.c_evaluate(list(s.order), list(coefs.shape[1:]), knots, coefs, [0, 0, 0], [xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()])
    assert bad == -1
    level, S, K = levels_of(name)[b], float(scale[b]), plan.order
    ends = max(max(abs(float(t[0])), abs(float(t[-1]))) for t in plan.breaks)
    lipschitz = sum((K[a] - 1) * np.abs(np.diff(coefs[0], axis=a)).max() / float(np.diff(np.asarray(plan.breaks[a], np.float64)).min()) for a in range(3))
    bar = (2.0 * sum(K) + sum(K)) * EPS * S + 4.0 * EPS * ends * lipschitz
    observe(f"isosurface |f(vertex) - level| / bar [{name}/{b}]", np.abs(np.asarray(values).reshape(-1) - level).max() / bar, 1.0)


@pytest.mark.parametrize("order", ORDERS, ids=lambda k: "%d%d%d" % k)
def test_every_order_tuple_and_two_variables_swapped(order):
    s, _ = drawn(order, (2, 2, 2), 100 + 16 * order[0] + 4 * order[1] + order[2])
    found = []
    for swap in (False, True):
        t = s
        if swap:                                                # variables 0 and 2 exchanged
            t = bspy_amd.Spline(3, 1, list(s.order)[::-1], list(s.nCoef)[::-1], list(s.knots)[::-1], np.ascontiguousarray(np.transpose(s.coefs, (0, 3, 2, 1))))
        plan, rows, levels, scale = iso.tables(t)
        got = iso._run_host(rows, plan, levels, scale, 1, None)
        want = iso.statement(rows, plan, levels, scale, 1)
        for label, value in want.items():
            assert np.asarray(got[label]).tobytes() == value.tobytes(), label
        assert len(got["triangles"]) > 0
        found.append(got)
    # the six tetrahedra are the same set whatever the names of the axes: the same crossed edges, the same points
    a, b = found[0]["xyz"], found[1]["xyz"][:, ::-1]
    assert len(found[0]["triangles"]) == len(found[1]["triangles"]) and a.shape == b.shape
    assert np.abs(np.sort(a, axis=0) - np.sort(b, axis=0)).max() < 1e-12


@pytest.mark.parametrize("name", ["sphere", "random_444", "levels", "shifted"])
def test_the_scale_law(name):
    """coefficients and levels times 2^k: every float of the computation is scaled exactly, the signs and the bisection
    are the same, so keys, triangles and vertices are the same bytes."""
    s, depth = spline_of(name), int(GOLD[f"{name}/depth"])
    levels = np.array(levels_of(name))
    base = iso.extract_batch(s, levels=levels, depth=depth, _path="host")
    for k in (-40, 7, 300):
        scaled = bspy_amd.Spline(3, 1, s.order, s.nCoef, s.knots, np.ldexp(np.asarray(s.coefs, np.float64), k))
        assert same(base, iso.extract_batch(scaled, levels=np.ldexp(levels, k), depth=depth, _path="host"))


def test_coefs_levels_and_splits_agree():
    s, coefs = drawn((3, 4, 2), (2, 2, 3), 11, fields=3)
    whole = iso.extract_batch(s, coefs=coefs, depth=2, _path="host")
    for split in (0, 1, 2):
        assert same(whole, iso.extract_batch(s, coefs=coefs, depth=2, _path="host", _split=split))
    for b in range(3):
        one = iso.extract_batch(s, coefs=coefs[b:b + 1], depth=2, _path="host")
        v0, v1 = whole[2][b:b + 2]
        t0, t1 = whole[4][b:b + 2]
        assert one[0].tobytes() == whole[0][v0:v1].tobytes() and one[3].tobytes() == (whole[3][t0:t1] - v0).tobytes()
    # levels subtract as a cell is loaded: the field f - 0.25 with a level of an exactly representable value
    shifted = iso.extract_batch(s, levels=[0.25], depth=2, _path="host")
    moved = iso.extract_batch(s, coefs=np.asarray(s.coefs) - 0.25, depth=2, _path="host")
    assert shifted[1].tobytes() == moved[1].tobytes() and shifted[3].tobytes() == moved[3].tobytes()
    assert np.abs(shifted[0] - moved[0]).max() < 1e-12
    empty = iso.extract_batch(s, coefs=coefs[:0], depth=2, _path="host")
    assert empty[0].shape == (0, 3) and empty[2].tolist() == [0] and empty[6].shape == (0, 2, 2, 3)


def test_depth_from_tolerance_and_the_split_rule():
    s = spline_of("sphere")
    plan = iso.Plan(s.order, s.knots)
    assert iso.depth_of(None, plan) == iso.DEFAULT_DEPTH == 3 and iso.MAX_DEPTH == 6
    assert [iso.depth_of(t, plan) for t in (1.0, 0.25, 0.0625, 1e-3, 1e-9)] == [0, 0, 1, 4, 6]      # (0.5 2^-d)^2 <= t
    with pytest.raises(ValueError, match="tolerance must be positive"):
        iso.depth_of(0.0, plan)
    assert iso.FILL_WAVES == 256 * 4 * 8
    assert [iso.split_of(n, 6) for n in (1, 16, 17, 1024, 8192, 100000)] == [5, 3, 3, 1, 0, 0]
    assert iso.split_of(1, 2) == 2
    v, t = s.isosurface(tolerance=0.0625, _path="host")
    v1, t1 = s.isosurface(depth=1, _path="host")
    assert v.tobytes() == v1.tobytes() and t.tobytes() == t1.tobytes()


def test_error_messages():
    k2 = np.array([0.0, 0.0, 1.0, 1.0])
    surface = bspy_amd.Spline(2, 1, [2, 2], [2, 2], [k2, k2], np.zeros((1, 2, 2)))
    with pytest.raises(ValueError, match="three independent variables and one dependent variable"):
        surface.isosurface()
    solid = bspy_amd.Spline(3, 3, [2, 2, 2], [2, 2, 2], [k2, k2, k2], np.zeros((3, 2, 2, 2)))
    with pytest.raises(ValueError, match="three independent variables and one dependent variable"):
        solid.isosurface()
    with pytest.raises(ValueError, match=r"one dependent variable, or coefs \(B, n0, n1, n2\)"):
        iso.extract_batch(solid)
    k5 = np.array([0.0] * 5 + [1.0] * 5)
    quartic = bspy_amd.Spline(3, 1, [5, 2, 2], [5, 2, 2], [k5, k2, k2], np.zeros((1, 5, 2, 2)))
    with pytest.raises(NotImplementedError, match="orders from 2 to 4"):
        quartic.isosurface()
    jump = bspy_amd.Spline(3, 1, [2, 2, 2], [4, 2, 2], [np.array([0.0, 0.0, 0.5, 0.5, 1.0, 1.0]), k2, k2], np.zeros((1, 4, 2, 2)))
    with pytest.raises(ValueError, match=r"isosurface: the knot 0\.5 of variable 0 has multiplicity 2 >= order 2"):
        jump.isosurface()
    s = spline_of("plane")
    with pytest.raises(ValueError, match="depth must be in 0 .. 6"):
        s.isosurface(depth=7)
    with pytest.raises(ValueError, match="_split must be in 0 .. depth"):
        iso.extract_batch(s, depth=2, _split=3)
    with pytest.raises(ValueError, match="levels or coefs, not both"):
        iso.extract_batch(s, levels=[0.0], coefs=np.zeros((1, 2, 2, 2)))
    with pytest.raises(ValueError, match=r"coefs must have the shape \(B, 2, 2, 2\)"):
        iso.extract_batch(s, coefs=np.zeros((1, 3, 2, 2)))
    with pytest.raises(ValueError, match="_path must be None, 'device' or 'host'"):
        s.isosurface(_path="gpu")

    class Huge:
        ncells = (1 << 14, 1 << 14, 1 << 14)
    iso._check_keys(Huge, 5, 1)                                  # 8 (2^19 + 1)^3 < 2^62
    with pytest.raises(ValueError, match="keys beyond 62 bits"):
        iso._check_keys(Huge, 6, 1)
    with pytest.raises(nv.BskError, match="bsk_iso_walk_host: depth must be in"):
        plan, rows, levels, scale = iso.tables(s)
        iso._run_host(rows, plan, levels, scale, 7, 0)


def test_the_family_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "bspy_amd.h")).read()
    declared = set(re.findall(r"\b(bsk_iso_[a-z_]+)\s*\(", header))
    assert declared == set(FAMILY) and declared <= set(nv.PRODUCT_SYMBOLS)
    assert all(hasattr(nv.lib(), name) for name in FAMILY)
    makefile = open(os.path.join(ROOT, "bspy_amd", "csrc", "Makefile")).read()
    assert "bsk_iso_tu.hip" in makefile and "bsk_iso_tu.o: bsk_roots.hpp bsk_iso.hpp" in makefile
    spills = open(os.path.join(ROOT, "bspy_amd", "csrc", "check_spills.py")).read()
    assert all(f'"{kernel}"' in spills for kernel in ("iso_flag", "iso_walk", "iso_leaf", "iso_vertex"))
