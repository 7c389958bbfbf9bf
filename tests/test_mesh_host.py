"""
``Spline.triangulate`` without a GPU: the host drivers (the functions of bsk_mesh.hpp on the CPU) against the exact oracle
tests/mesh_ref.py as recorded in tests/golden/mesh.npz, against the Python statement of bspy_amd/mesh.py bit for bit, and
the mesh itself in integer arithmetic on its keys.

THE BARS (S = max |coefficient| of the member, eps = 2^-52, first order):
  * a vertex: the host's Bezier extraction sums at most K products per axis with rounded weights, (K + 1) eps S / 2 per
    axis; de Casteljau is K0 + K1 - 2 levels of a lerp with a rounded 1 - t, 3 roundings each, 1.5 eps S: together
    (K0 + K1 + 2) / 2 + 1.5 (K0 + K1 - 2) = 2 (K0 + K1) - 2 < 2 (K0 + K1) times eps S; the golden value is the exact point
    rounded once, eps |x| / 2;
  * a parameter: lo + t (hi - lo) is three roundings on numbers up to 2 max |domain end|: 3 eps max |domain end|, plus the
    golden's own rounding;
  * a point of a triangle: |S - L| <= bound[cell] for the exact interpolant (the claim, with Q's roundings inside bound);
    the test's L interpolates the returned vertices, each within the vertex bar, with weights that sum to 1, in four more
    roundings: bound + (2 (K0 + K1) + 4) eps S.
"""
import os
import re
import warnings

import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import mesh
from conftest import observe
from mesh_cases import GOLD, L, NAMES, ORDERS, arguments, cells_of, directed_edges, doubled_areas, drawn, members_of, points_of, same, spline_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
FAMILY = ("bsk_mesh_bound_host", "bsk_mesh_bound", "bsk_mesh_count_host", "bsk_mesh_count", "bsk_mesh_emit_host", "bsk_mesh_emit",
          "bsk_mesh_vertex_host", "bsk_mesh_vertex", "bsk_mesh_last_kernel")
HOST = ["host mesh_bound", "host mesh_count", "host mesh_emit", "host mesh_vertex"]
PAIRS = [(name, b) for name in NAMES for b in range(members_of(name))]

_RAW = {}


def raw(name):
    """The host drivers' raw result of a case (computed once and shared, never changed): (plan, rows, scale, result, bound)."""
    if name not in _RAW:
        args = arguments(name)
        plan, rows, scale = mesh.tables(spline_of(name), args["coefs"])
        res = mesh._run_host(rows, plan, args["tolerance"], args["max_level"], normals=rows.shape[1] == 3)
        _RAW[name] = (plan, rows, scale, res, mesh.bound_of(res["Q"], res["lev"], plan.order, scale, rows.shape[1]))
    return _RAW[name]


def member(res, b):
    """(keys, uv, xyz, triangles as key triples, triangles as indices into the member's own vertices) of member b."""
    v0, v1 = res["vertex_offsets"][b:b + 2]
    t0, t1 = res["triangle_offsets"][b:b + 2]
    return res["keys"][v0:v1], res["uv"][v0:v1], res["xyz"][v0:v1], res["keys"][res["triangles"][t0:t1]], res["triangles"][t0:t1] - v0


def test_the_cases_are_the_ones_the_issue_lists():
    lev = lambda n, b=0: GOLD[f"{n}/{b}/lev"]
    cells = lambda n: [len(np.unique(GOLD[f"{n}/knots{a}"])) - 1 for a in range(2)]
    assert lev("one_00").tolist() == [[[0, 0]]] and len(GOLD["one_00/0/triangles"]) == 2
    assert lev("one_31").tolist() == [[[3, 1]]]
    for name, step in (("step_1", 1), ("step_3", 3)):
        assert cells(name) == [2, 1] and abs(int(lev(name)[0, 0, 1]) - int(lev(name)[1, 0, 1])) == step
    assert cells("bump") == [3, 3] and all((lev("bump")[1, 1] > lev("bump")[i, j]).all() for i in range(3) for j in range(3) if (i, j) != (1, 1))
    ring = lev("ring")
    assert cells("ring") == [3, 3] and ring[1, 1].tolist() == [0, 0] and min(ring[0, 1, 1], ring[2, 1, 1], ring[1, 0, 0], ring[1, 2, 0]) > 0
    assert np.count_nonzero(GOLD["double_knot/knots0"] == 0.5) == 2 and np.count_nonzero(GOLD["triple_knot/knots0"] == 0.5) == 3
    assert GOLD["double_knot/order"].tolist() == [4, 4] and GOLD["triple_knot/order"].tolist() == [4, 4]
    assert all(GOLD[f"orders_{k0}{k1}/order"].tolist() == [k0, k1] for k0, k1 in ORDERS)
    assert [GOLD[f"ndep_{d}/coefs"].shape[1] for d in (1, 2, 3)] == [1, 2, 3]
    assert not GOLD["plane/0/Q"].any() and not lev("plane").any()
    assert int(GOLD["capped/max_level"]) == 2 and GOLD["capped/0/capped"].tolist() == [[1]] and lev("capped").tolist() == [[[2, 1]]]
    assert lev("one_54").tolist() == [[[5, 4]]] and len(GOLD["one_54/0/triangles"]) == 2 * 512
    assert members_of("batch") == 3 and len({lev("batch", b).tobytes() for b in range(3)}) == 3
    assert [GOLD[f"domain/knots{a}"][[0, -1]].tolist() for a in range(2)] == [[3.0, 7.0], [-2.0, -1.0]]
    assert GOLD["float32/coefs"].dtype == np.float32 and GOLD["float32/knots0"].dtype == np.float32
    assert bool(GOLD["negate/negate"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mesh.npz")) < 300 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_host_drivers_equal_the_statement(name):
    plan, rows, _, res, _ = raw(name)
    args = arguments(name)
    want = mesh.statement(rows, plan, args["tolerance"], args["max_level"], normals=rows.shape[1] == 3)
    for label, value in want.items():
        assert np.asarray(res[label]).tobytes() == value.tobytes(), f"{name}: {label}"


@pytest.mark.parametrize("name,b", PAIRS)
def test_levels_keys_and_triangles_equal_the_oracle(name, b):
    res = raw(name)[3]
    keys, _, _, triangles, _ = member(res, b)
    assert res["lev"][b].tobytes() == GOLD[f"{name}/{b}/lev"].tobytes()
    assert res["status"][b].tobytes() == GOLD[f"{name}/{b}/capped"].tobytes()
    assert keys.tobytes() == GOLD[f"{name}/{b}/keys"].tobytes()
    assert triangles.tobytes() == GOLD[f"{name}/{b}/triangles"].tobytes()
    assert cells_of(triangles).tolist() == GOLD[f"{name}/{b}/tcell"].tolist()
    Q, exact = res["Q"][b], GOLD[f"{name}/{b}/Q"]
    S = float(raw(name)[2][b])
    assert np.all(np.abs(np.sqrt(Q) - np.sqrt(exact)) <= 16.0 * (2.0 * sum(raw(name)[0].order) + 8.0) * EPS * S * np.sqrt(3.0))


@pytest.mark.parametrize("name,b", PAIRS)
def test_vertices_within_the_derived_bar(name, b):
    plan, _, scale, res, _ = raw(name)
    _, uv, xyz, _, _ = member(res, b)
    S = float(scale[b])
    exact = GOLD[f"{name}/{b}/xyz"]
    bar = 2.0 * sum(plan.order) * EPS * S + 0.5 * EPS * np.abs(exact)
    observe(f"triangulate vertex / derived bar [{name}/{b}]", (np.abs(xyz - exact) / np.maximum(bar, 1e-300)).max() if S else 0.0, 1.0)
    ends = max(max(abs(float(t[0])), abs(float(t[-1]))) for t in plan.breaks)
    observe(f"triangulate parameter / derived bar [{name}/{b}]", np.abs(uv - GOLD[f"{name}/{b}/uv"]).max() / (3.5 * EPS * ends), 1.0)


@pytest.mark.parametrize("name,b", PAIRS)
def test_the_seven_points_of_every_triangle_are_within_the_bound(name, b):
    plan, _, scale, res, bound = raw(name)
    _, _, xyz, triangles, index = member(res, b)
    tolerance = arguments(name)["tolerance"]
    S = float(scale[b])
    seven = GOLD[f"{name}/{b}/seven"]                                        # (m, 7, nDep): the exact surface, rounded once
    L7 = np.einsum("pk,mkd->mpd", GOLD["weights"], xyz[index])               # the interpolant of the returned vertices
    deviation = np.sqrt(((seven - L7) ** 2).sum(axis=2)).max(axis=1)
    cell = cells_of(triangles)
    allowed = bound[b][cell[:, 0], cell[:, 1]] + (2.0 * sum(plan.order) + 4.0) * EPS * S * np.sqrt(xyz.shape[1])
    observe(f"triangulate |S - L| / (bound + vertex bar) [{name}/{b}]", (deviation / np.maximum(allowed, 1e-300)).max(), 1.0)
    free = res["status"][b] == 0
    assert np.all(bound[b][free] <= tolerance)
    if name == "capped":
        assert not free.any() and bound[b][0, 0] > tolerance


@pytest.mark.parametrize("name,b", PAIRS)
def test_the_triangles_tile_the_domain_exactly(name, b):
    plan, _, _, res, _ = raw(name)
    keys, _, _, triangles, index = member(res, b)
    nc0, nc1 = (int(n) for n in plan.ncells)
    areas = doubled_areas(triangles)
    assert np.all(areas > 0)
    cell = cells_of(triangles)
    total = np.zeros((nc0, nc1), np.int64)
    np.add.at(total, (cell[:, 0], cell[:, 1]), areas)
    assert np.all(total == 2 * 4 ** L)
    edges = directed_edges(index)
    assert max(edges.values()) == 1
    X, Y = points_of(keys)
    once = 0
    for (p, q) in edges:
        if (q, p) not in edges:
            once += 1
            assert (X[p] == X[q] and X[p] in (0, nc0 << L)) or (Y[p] == Y[q] and Y[p] in (0, nc1 << L)), f"{name}: the edge {keys[p]} -> {keys[q]} is a crack"
    assert len(keys) - (len(edges) + once) // 2 + len(index) == 1


@pytest.mark.parametrize("name", NAMES)
def test_the_public_calls_return_the_raw_result(name):
    plan, rows, _, res, bound = raw(name)
    args = arguments(name)
    ndep = rows.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = mesh.triangulate_batch(spline_of(name), args["tolerance"], coefs=args["coefs"], max_level=args["max_level"], normals=ndep == 3, _path="host")
        assert mesh.LAST_PATHS[-4:] == HOST and nv.lib().bsk_mesh_last_kernel().decode() == "host mesh_vertex"
        labels = ("uv", "xyz", "vertex_offsets", "triangles", "triangle_offsets", "lev", None, "status") + (("normals",) if ndep == 3 else ())
        assert len(out) == len(labels)
        for got, label in zip(out, labels):
            assert got.tobytes() == (bound if label is None else np.asarray(res[label])).tobytes(), label
        assert out[1].dtype == np.float64 and out[3].dtype == np.int64 and out[5].dtype == np.int32 and out[7].dtype == np.uint8
        s = spline_of(name)
        got = s.triangulate(args["tolerance"], parameters=True, normals=ndep == 3, max_level=args["max_level"], _path="host")
    _, uv, xyz, _, index = member(res, 0)
    negate = f"{name}/negate" in GOLD.files
    assert got[0].tobytes() == xyz.tobytes() and got[2].tobytes() == uv.tobytes()
    assert got[1].tobytes() == np.ascontiguousarray(index[:, [0, 2, 1]] if negate else index).tobytes()
    if ndep == 3:
        n0, n1 = res["vertex_offsets"][:2]
        rawn = res["normals"][n0:n1] * (-1.0 if negate else 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            assert got[3].tobytes() == (rawn / np.sqrt((rawn * rawn).sum(axis=1, keepdims=True))).tobytes()
        # the raw normal is S_u x S_v: it agrees with the triangles' own orientation wherever it is not tiny
        corners = xyz[index]
        facet = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
        mean = res["normals"][n0:n1][index].sum(axis=1)
        if name in ("one_00", "plane", "bump", "step_1"):                       # graphs of small slope: S_u x S_v points up
            assert np.all((facet * mean).sum(axis=1) > 0.0) and np.all(res["normals"][n0:n1][:, 2] > 0.0)


def test_negate_normal_flips_triangles_and_normals():
    s = spline_of("negate")
    plain = bspy_amd.Spline(2, 3, s.order, s.nCoef, s.knots, s.coefs)
    tol = arguments("negate")["tolerance"]
    a, b = s.triangulate(tol, normals=True, _path="host"), plain.triangulate(tol, normals=True, _path="host")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1][:, [0, 2, 1]].tobytes() and np.array_equal(a[2], -b[2])
    assert a[1].flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("name", ["ring", "step_3", "batch", "orders_43", "domain"])
def test_the_scale_law(name):
    """Coefficients and tolerance times 2^k: every Q is scaled by 4^k exactly and compared with an exact multiple, every
    lerp is scaled exactly: the same levels, keys and triangles, and xyz scaled bit for bit."""
    args = arguments(name)
    s = spline_of(name)
    base = mesh.triangulate_batch(s, args["tolerance"], coefs=args["coefs"], max_level=args["max_level"], _path="host")
    for k in (-40, -7, 3, 40):
        got = mesh.triangulate_batch(s, np.ldexp(args["tolerance"], k), coefs=np.ldexp(args["coefs"].astype(np.float64), k), max_level=args["max_level"],
                                     _path="host")
        for n in (0, 2, 3, 4, 5, 7):
            assert got[n].tobytes() == base[n].tobytes(), (k, n)
        assert got[1].tobytes() == np.ldexp(base[1], k).tobytes()


@pytest.mark.parametrize("name", ["ring", "step_3", "double_knot", "domain"])
def test_scaled_knots_keep_the_triangles_and_scale_the_parameters(name):
    args = arguments(name)
    s = spline_of(name)
    base = mesh.triangulate_batch(s, args["tolerance"], coefs=args["coefs"], _path="host")
    for k in (-40, -7, 3, 40):
        t = bspy_amd.Spline(2, s.nDep, s.order, s.nCoef, [np.ldexp(np.asarray(x, np.float64), k) for x in s.knots], s.coefs)
        got = mesh.triangulate_batch(t, args["tolerance"], coefs=args["coefs"], _path="host")
        for n in (1, 2, 3, 4, 5, 6, 7):
            assert got[n].tobytes() == base[n].tobytes(), (k, n)
        assert got[0].tobytes() == np.ldexp(base[0], k).tobytes()


def test_a_cell_changes_no_triangle_of_a_cell_that_is_not_its_neighbour():
    """The first coefficient of a clamped spline reaches cell (0, 0) alone: its level may change the triangles of (0, 0) and
    of the two cells that share an edge with it, and of no other cell."""
    s, coefs = drawn((3, 4), (5, 4), 21)
    base = mesh.triangulate_batch(s, 0.05, coefs=coefs, _path="host")
    moved = coefs.copy()
    moved[0, :, 0, 0] += 40.0
    got = mesh.triangulate_batch(s, 0.05, coefs=moved, _path="host")
    assert got[5][0, 0, 0].tolist() != base[5][0, 0, 0].tolist() and got[5].reshape(-1, 2)[1:].tobytes() == base[5].reshape(-1, 2)[1:].tobytes()

    def far(which):
        plan, rows, _ = mesh.tables(s, which)
        res = mesh._run_host(rows, plan, 0.05)
        tkeys = res["keys"][res["triangles"]]
        cell = cells_of(tkeys)
        keep = ~(((cell[:, 0] == 0) & (cell[:, 1] <= 1)) | ((cell[:, 0] == 1) & (cell[:, 1] == 0)))
        return tkeys[keep]

    a, b = far(coefs), far(moved)
    assert len(a) > 0 and a.tobytes() == b.tobytes()
    assert len(got[3]) != len(base[3])


@pytest.mark.parametrize("order", ORDERS, ids=lambda k: "%d%d" % k)
def test_every_order_tuple_and_the_variables_swapped(order):
    s, coefs = drawn(order, (2, 3), 300 + 4 * order[0] + order[1], members=2)
    plan, rows, _ = mesh.tables(s, coefs)
    got = mesh._run_host(rows, plan, 0.1, normals=True)
    want = mesh.statement(rows, plan, 0.1, normals=True)
    for label, value in want.items():
        assert np.asarray(got[label]).tobytes() == value.tobytes(), label
    t = bspy_amd.Spline(2, 3, list(s.order)[::-1], list(s.nCoef)[::-1], list(s.knots)[::-1], np.ascontiguousarray(np.transpose(coefs[0], (0, 2, 1))))
    a = mesh.triangulate_batch(s, 0.1, coefs=coefs[:1], _path="host")
    b = mesh.triangulate_batch(t, 0.1, coefs=np.ascontiguousarray(np.transpose(coefs[:1], (0, 1, 3, 2))), _path="host")
    # Quu and Qvv change places, Quv stays: the levels are the transposed ones and the meshes have the same size
    assert np.array_equal(a[5][0], np.transpose(b[5][0], (1, 0, 2))[:, :, ::-1]) and len(a[3]) == len(b[3]) and len(a[1]) == len(b[1])


def test_chunks_members_and_empty_batches_agree():
    s, coefs = drawn((3, 3), (3, 2), 31, members=3)
    whole = mesh.triangulate_batch(s, 0.1, coefs=coefs, normals=True, _path="host")
    assert len(set(np.diff(whole[4]).tolist())) == 3
    for chunk in (1, 7, 64):
        assert same(whole, mesh.triangulate_batch(s, 0.1, coefs=coefs, normals=True, _path="host", _chunk=chunk))
    for b in range(3):
        one = mesh.triangulate_batch(s, 0.1, coefs=coefs[b:b + 1], _path="host")
        v0, v1 = whole[2][b:b + 2]
        t0, t1 = whole[4][b:b + 2]
        assert one[1].tobytes() == whole[1][v0:v1].tobytes() and one[3].tobytes() == (whole[3][t0:t1] - v0).tobytes()
    empty = mesh.triangulate_batch(s, 0.1, coefs=coefs[:0], _path="host")
    assert empty[1].shape == (0, 3) and empty[2].tolist() == [0] and empty[5].shape == (0, 3, 2, 2) and empty[6].shape == (0, 3, 2)
    f32 = mesh.triangulate_batch(s, 0.1, coefs=coefs.astype(np.float32), _path="host")
    assert same(f32, mesh.triangulate_batch(s, 0.1, coefs=coefs.astype(np.float32).astype(np.float64), _path="host"))


def test_refusals_and_the_warning():
    k2, k5 = np.array([0.0, 0.0, 1.0, 1.0]), np.array([0.0] * 5 + [1.0] * 5)
    flat = bspy_amd.Spline(2, 3, [2, 2], [2, 2], [k2, k2], np.zeros((3, 2, 2)))
    curve = bspy_amd.Spline(1, 2, [2], [2], [k2], np.zeros((2, 2)))
    four = bspy_amd.Spline(2, 4, [2, 2], [2, 2], [k2, k2], np.zeros((4, 2, 2)))
    quartic = bspy_amd.Spline(2, 3, [5, 2], [5, 2], [k5, k2], np.zeros((3, 5, 2)))
    for bad in (curve, four, quartic):
        with pytest.raises(ValueError, match=re.escape(mesh.SCOPE)):
            bad.triangulate(1e-3)
    jump = bspy_amd.Spline(2, 3, [2, 2], [4, 2], [np.array([0.0, 0.0, 0.5, 0.5, 1.0, 1.0]), k2], np.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match=r"triangulate: the knot 0\.5 of variable 0 has multiplicity 2 >= order 2 \(a jump: no mesh crosses it"):
        jump.triangulate(1e-3)
    for tolerance in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="tolerance must be finite and > 0"):
            flat.triangulate(tolerance)
    for value in (np.nan, np.inf):
        broken = np.zeros((3, 2, 2))
        broken[1, 0, 1] = value
        with pytest.raises(ValueError, match="the coefficients must be finite"):
            bspy_amd.Spline(2, 3, [2, 2], [2, 2], [k2, k2], broken).triangulate(1e-3, _path="host")
    with pytest.raises(ValueError, match="max_level must be in 0 .. 10"):
        flat.triangulate(1e-3, max_level=11)
    with pytest.raises(ValueError, match=r"coefs must have the shape \(B, nDep, 2, 2\)"):
        mesh.triangulate_batch(flat, 1e-3, coefs=np.zeros((1, 3, 3, 2)))
    with pytest.raises(ValueError, match="normals take three dependent variables"):
        bspy_amd.Spline(2, 1, [2, 2], [2, 2], [k2, k2], np.zeros((1, 2, 2))).triangulate(1e-3, normals=True)
    with pytest.raises(ValueError, match="_path must be None, 'device' or 'host'"):
        flat.triangulate(1e-3, _path="gpu")
    with pytest.raises(ValueError, match="_chunk must be >= 1"):
        mesh.triangulate_batch(flat, 1e-3, _chunk=0)
    s = spline_of("one_54")
    with pytest.raises(ValueError, match=r"triangulate: 1024 triangles exceed max_triangles = 1000"):
        s.triangulate(arguments("one_54")["tolerance"], max_triangles=1000, _path="host")
    assert mesh.DEFAULT_MAX_TRIANGLES == 1 << 28 and mesh.DEFAULT_MAX_LEVEL == 8 and mesh.MAX_LEVEL == 10
    capped = spline_of("capped")
    with pytest.warns(RuntimeWarning, match="1 cells need more than max_level = 2") as caught:
        xyz, triangles = capped.triangulate(arguments("capped")["tolerance"], max_level=2, _path="host")
    assert len(caught) == 1 and len(triangles) == 16
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        capped.triangulate(arguments("capped")["tolerance"], _path="host")       # at the default cap nothing warns
    with pytest.raises(nv.BskError, match="bsk_mesh_bound_host: max_level must be in"):
        plan, rows, _ = mesh.tables(flat)
        mesh._run_host(rows, plan, 1e-3, 11)


def test_the_family_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "bspy_amd.h")).read()
    declared = set(re.findall(r"\b(bsk_mesh_[a-z_]+)\s*\(", header))
    assert declared == set(FAMILY) and declared <= set(nv.PRODUCT_SYMBOLS)
    assert all(hasattr(nv.lib(), name) for name in FAMILY)
    makefile = open(os.path.join(ROOT, "bspy_amd", "csrc", "Makefile")).read()
    assert "bsk_mesh_tu.hip" in makefile and "bsk_mesh_tu.o: bsk_roots.hpp bsk_mesh.hpp" in makefile
    spills = open(os.path.join(ROOT, "bspy_amd", "csrc", "check_spills.py")).read()
    assert all(f'"{kernel}"' in spills for kernel in ("mesh_bound", "mesh_count", "mesh_emit", "mesh_vertex"))
