"""
``Spline.contours`` without a GPU: the host drivers (the functions of bsk_contour.hpp on the CPU) against the exact oracle
tests/contours_ref.py as recorded in tests/golden/contours.npz, against the Python statement of bspy_amd/contours.py bit
for bit, and against themselves at every split level.  The fit (``Spline.least_squares``) needs the device and is tested
in test_gpu_contours.py.

THE BAR OF A VERTEX.  A vertex lies on a lattice line; its fixed coordinate is bit-equal to the line (asserted).  Its moving
coordinate is the root of the cell's polynomial on the line, found by sign bisection of float values:
  * a sign of a float value is wrong only where the exact value is below the rounding of the evaluation, which is
    2 (K0 + K1) eps S for the K0 + K1 - 2 lerps of a value and the restriction before them (first order, S = max
    |coefficient|); the bisection therefore stops within 2 (K0 + K1) eps S / |df/ds| of the exact root, |df/ds| the exact
    derivative along the edge at the root, in units of the parameter (recorded by the generator);
  * the map from the cell to the parameter, (1 - x) t0 + x t1, and the sum a / G + s / G round three times: 4 eps max |domain
    end| covers them;
  * the oracle's own bracket of the exact root (its recorded width, at most 2^-70 of an edge).
The generator asserts what this first-order statement needs: one root per lattice edge, no node value below 1e-6 S.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import contours as C
from conftest import GOLDEN, observe

GOLD = np.load(os.path.join(GOLDEN, "contours.npz"))
NAMES = [str(n) for n in GOLD["names"]]
EPS = 2.0 ** -52
FAMILY = ("bsk_contour_flag_host", "bsk_contour_flag", "bsk_contour_march_host", "bsk_contour_march", "bsk_contour_last_kernel")


def spline_of(name):
    order = [int(k) for k in GOLD[f"{name}/order"]]
    coefs = GOLD[f"{name}/coefs"]
    return bspy_amd.Spline(2, 1, order, list(coefs.shape), [GOLD[f"{name}/knots0"], GOLD[f"{name}/knots1"]], coefs[None])


_RAW = {}


def raw(name, split=0):
    """The host drivers' raw result of a case (computed once per split level and shared)."""
    if (name, split) not in _RAW:
        s = spline_of(name)
        level = float(GOLD[f"{name}/level"])
        plan, rows, levels, scale = C.tables(s, None if level == 0.0 else [level])
        _RAW[name, split] = (plan, rows, levels, scale, C._run_host(rows, plan, levels, scale, int(GOLD[f"{name}/depth"]), split))
    return _RAW[name, split]


def by_key(res):
    order = np.lexsort((res["keys"][:, 1], res["keys"][:, 0]))
    return res["keys"][order], res["xy"][order]


def test_the_cases_are_the_ones_the_issue_lists():
    assert {"circle", "two_circles", "plane", "plane_d0", "plane_d1", "random_22", "random_34", "random_44", "random_42", "crease",
            "diagonal", "saddle", "zero_cell", "float32", "shifted"} <= set(NAMES)
    assert [int(GOLD[f"{n}/depth"]) for n in ("plane_d0", "plane_d1", "plane")] == [0, 1, 4]
    assert GOLD["float32/coefs"].dtype == np.float32 and GOLD["float32/knots0"].dtype == np.float32
    assert GOLD["shifted/knots0"][0] == 100.0 and GOLD["shifted/knots1"][-1] == -38.0 and np.abs(GOLD["shifted/coefs"]).max() > 4000.0
    for n in NAMES:
        assert (len(np.unique(GOLD[f"{n}/knots0"])) - 1) <= 9 and (len(np.unique(GOLD[f"{n}/knots1"])) - 1) <= 7
    assert len(GOLD["saddle/saddles"]) == 1 and len(GOLD["zero_cell/zero"]) == 1
    assert GOLD["circle/closed"].tolist() == [True] and GOLD["two_circles/closed"].tolist() == [True, True]
    assert GOLD["plane/closed"].tolist() == [False]


@pytest.mark.parametrize("name", NAMES)
def test_keys_and_segments_equal_the_oracle(name):
    plan, _, _, _, res = raw(name)
    keys, _ = by_key(res)
    assert keys.tobytes() == GOLD[f"{name}/segments"].tobytes()
    assert np.argwhere(res["zero"][0]).tolist() == GOLD[f"{name}/zero"].tolist()
    assert np.argwhere(res["status"][0] & C.STATUS_SADDLE).tolist() == GOLD[f"{name}/saddles"].tolist()
    points, offsets, closed, field = C.link(res["keys"], res["field"], 1)
    assert closed.tolist() == GOLD[f"{name}/closed"].tolist() and not field.any()
    assert np.diff(offsets).tolist() == GOLD[f"{name}/lengths"].tolist()
    first = res["keys"].reshape(-1)[points[offsets[:-1]]]
    assert first.tolist() == GOLD[f"{name}/first_keys"].tolist()
    # the public call: the same polylines, rounded once to the knots' dtype
    s = spline_of(name)
    level = float(GOLD[f"{name}/level"])
    vertices, off, cl, fld, cells, status = C.trace_batch(s, levels=None if level == 0.0 else [level], depth=int(GOLD[f"{name}/depth"]), _path="host")
    kdtype = np.result_type(s.knots[0].dtype, s.knots[1].dtype)
    assert vertices.dtype == kdtype and vertices.tobytes() == res["xy"].reshape(-1, 2)[points].astype(kdtype).tobytes()
    assert off.tolist() == offsets.tolist() and cl.tolist() == closed.tolist() and status.tobytes() == res["status"].tobytes()
    for m in np.flatnonzero(cl):
        assert vertices[off[m]].tobytes() == vertices[off[m + 1] - 1].tobytes()
    assert len(cells) == len(GOLD[f"{name}/zero"])
    ref = int(GOLD[f"{name}/ref_count"])
    if ref >= 0:                                               # the reference returned within its 60 s
        assert len(off) - 1 == ref


@pytest.mark.parametrize("name", NAMES)
def test_vertices_within_the_derived_bar(name):
    plan, _, _, scale, res = raw(name)
    depth = int(GOLD[f"{name}/depth"])
    K0, K1 = plan.order
    inv = 1.0 / float(1 << depth)
    where = {int(k): n for n, k in enumerate(GOLD[f"{name}/vkeys"])}
    ends = max(max(abs(float(b[0])), abs(float(b[-1]))) for b in plan.breaks)
    worst = 0.0
    for (ka, kb), pts in zip(res["keys"], res["xy"]):
        for key, (u, v) in ((int(ka), pts[:2]), (int(kb), pts[2:])):
            n = where[key]
            I, J, direction = (int(x) for x in GOLD[f"{name}/vedge"][n])
            fixed, moving = (1, 0) if direction == 0 else (0, 1)
            cell, a = C.owner_of(J if direction == 0 else I, depth)
            y = float(a) * inv
            t = plan.breaks[fixed]
            line = (1.0 - y) * float(t[cell]) + y * float(t[cell + 1])
            got = (float(u), float(v))
            assert got[fixed] == line, f"{name}: vertex {key} is not on its lattice line"
            err = abs((got[moving] - float(GOLD[f"{name}/vmid_hi"][n][moving])) - float(GOLD[f"{name}/vmid_lo"][n][moving]))
            bar = 2.0 * (K0 + K1) * EPS * float(scale[0]) / float(GOLD[f"{name}/vslope"][n]) + 4.0 * EPS * ends + float(GOLD[f"{name}/vwidth"][n][moving])
            worst = max(worst, err / bar)
    observe(f"contours vertex / bar, {name}", worst, 1.0)


def degrees_ok(keys, NI, NJ):
    flat, count = np.unique(keys.reshape(-1), return_counts=True)
    assert count.max() <= 2
    for key in flat[count == 1]:
        node, direction = int(key) >> 1, int(key) & 1
        I, J = divmod(node, NJ)
        assert (J in (0, NJ - 1)) if direction == 0 else (I in (0, NI - 1)), f"a chain ends inside the domain at edge {I, J, direction}"


@pytest.mark.parametrize("name", NAMES)
def test_every_vertex_has_degree_two_or_lies_on_the_boundary(name):
    plan, _, _, _, res = raw(name)
    G = 1 << int(GOLD[f"{name}/depth"])
    degrees_ok(res["keys"], plan.ncells[0] * G + 1, plan.ncells[1] * G + 1)


def test_degrees_on_100_random_bicubic_fields():
    rng = np.random.default_rng(2024)
    k = np.array([0.0] * 4 + [0.2, 0.4, 0.6, 0.8] + [1.0] * 4)
    coefs = rng.uniform(-1.0, 1.0, (100, 8, 8))
    s = bspy_amd.Spline(2, 1, [4, 4], [8, 8], [k, k], coefs[:1])
    plan, rows, _, scale = C.tables(s, None, coefs)
    res = C._run_host(rows, plan, None, scale, C.DEFAULT_DEPTH, None)
    G = 1 << C.DEFAULT_DEPTH
    assert plan.ncells == [5, 5] and len(np.unique(res["field"])) == 100
    for b in range(100):
        degrees_ok(res["keys"][res["field"] == b], 5 * G + 1, 5 * G + 1)


@pytest.mark.parametrize("name", NAMES)
def test_the_python_statement_and_the_host_drivers_agree_bit_for_bit(name):
    plan, rows, levels, scale, res = raw(name)
    want = C.statement(rows, plan, levels, scale, int(GOLD[f"{name}/depth"]))
    for key in ("cand", "zero", "status", "keys", "xy", "field"):
        assert res[key].tobytes() == want[key].tobytes(), key


@pytest.mark.parametrize("name", NAMES)
def test_identical_for_every_split_level(name):
    depth = int(GOLD[f"{name}/depth"])
    s = spline_of(name)
    level = float(GOLD[f"{name}/level"])
    keys0, xy0 = by_key(raw(name)[4])
    base = None
    for P in range(depth + 1):
        res = raw(name, P)[4]
        assert res["split"] == P
        keys, xy = by_key(res)
        assert keys.tobytes() == keys0.tobytes() and xy.tobytes() == xy0.tobytes()
        assert res["status"].tobytes() == raw(name)[4]["status"].tobytes()
        out = C.trace_batch(s, levels=None if level == 0.0 else [level], depth=depth, _path="host", _split=P)
        blob = [np.asarray(a).tobytes() for a in out]
        base = base or blob
        assert blob == base


def test_a_levels_batch_equals_three_single_calls():
    s = spline_of("circle")
    levels = [-0.2, 0.0, 0.3]
    vertices, offsets, closed, field, cells, status = C.trace_batch(s, levels=levels, _path="host")
    assert C.LAST_PATHS.count("host roots_extract") == 2                     # one extraction per axis for all levels
    assert field.tolist() == sorted(field.tolist()) and set(field.tolist()) == {0, 1, 2}
    for b, level in enumerate(levels):
        v1, o1, c1, f1, _, s1 = C.trace_batch(s, levels=[level], _path="host")
        mine = np.flatnonzero(field == b)
        assert len(mine) == len(o1) - 1 and closed[mine].tolist() == c1.tolist()
        assert vertices[offsets[mine[0]]:offsets[mine[-1] + 1]].tobytes() == v1.tobytes()
        assert (np.diff(offsets)[mine]).tolist() == np.diff(o1).tolist()
        assert status[b].tobytes() == s1[0].tobytes()
    # level 0.0 is the spline itself, to the bit
    v0, o0, *_ = C.trace_batch(s, _path="host")
    v1, o1, *_ = C.trace_batch(s, levels=[0.0], _path="host")
    assert v0.tobytes() == v1.tobytes() and o0.tolist() == o1.tolist()


def test_numpy_coefs_are_fields_of_their_own():
    s = spline_of("circle")
    coefs = np.stack([s.coefs[0], s.coefs[0] - 0.3, np.abs(s.coefs[0]) + 1.0])
    vertices, offsets, closed, field, _, status = C.trace_batch(s, coefs=coefs, _path="host")
    assert field.tolist() == [0, 1] and status.shape == (3, 3, 4) and closed.tolist() == [True, True]
    assert C.LAST_PATHS[-3:] == ["host contour_flag", "host contour_march count", "host contour_march emit"]
    # field 0 is the spline itself, to the bit (field 1 is extracted after the shift, a level is subtracted behind the extraction)
    want = C.trace_batch(s, _path="host")
    assert vertices[:offsets[1]].tobytes() == want[0].tobytes() and status[0].tobytes() == want[5][0].tobytes()
    none = C.trace_batch(s, coefs=coefs[2:], _path="host")                 # a field without a candidate: no march
    assert len(none[0]) == 0 and none[1].tolist() == [0] and C.LAST_PATHS[-1] == "host contour_flag"


def test_depth_from_tolerance():
    plan = C.Plan([3, 3], [np.array([0.0, 0, 0, 0.5, 1, 1, 1]), np.array([0.0, 0, 0, 2, 2, 2])])
    assert C.depth_of(None, plan) == 4
    # h = 2, L = 2: (2 / 2^d)^2 <= 2 tolerance
    assert [C.depth_of(t, plan) for t in (2.0, 0.5, 0.124, 1e-12)] == [0, 1, 3, 8]
    with pytest.raises(ValueError):
        C.depth_of(0.0, plan)
    assert [C.split_of(n, 4) for n in (1, 16, 1 << 16)] == [4, 4, 0] and C.split_of(1 << 10, 8) == 3


def test_error_messages():
    with open(os.path.join(GOLDEN, "contours_semantics.json")) as f:
        entries = json.load(f)
    assert {e["name"] for e in entries} == {"free_variables", "three_variables", "order_five", "jump"}
    for e in entries:
        d = e["spline"]
        knots = [np.array(k) for k in d["knots"]]
        s = bspy_amd.Spline(d["nInd"], d["nDep"], d["order"], [len(k) - o for k, o in zip(knots, d["order"])], knots, np.array(d["coefs"]))
        with pytest.raises(getattr(__import__("builtins"), e["type"])) as caught:
            s.contours()
        assert str(caught.value) == e["error"], e["name"]
    s = spline_of("plane")
    for bad in (dict(depth=9), dict(depth=-1), dict(depth=2, _split=3), dict(_path="gpu"), dict(levels=[0.0], coefs=s.coefs)):
        with pytest.raises(ValueError):
            C.trace_batch(s, **bad)


def test_the_drivers_refuse_what_they_cannot_index():
    plan, rows, _, scale, res = raw("plane")
    L = nv.lib()
    first0, first1 = plan.first
    b0, b1 = (np.ascontiguousarray(b, np.float64) for b in plan.breaks)
    grid = C._grid(plan, rows, lambda a: a.ctypes.data, None, 1, scale, first0, first1)
    idx = np.flatnonzero(res["cand"]).astype(np.int64)
    counts, lane_status = np.empty(len(idx), np.int32), np.empty(len(idx), np.uint8)
    march = grid + (b0.ctypes.data, b1.ctypes.data, idx.ctypes.data, len(idx))
    assert L.bsk_contour_march_host(*march, 9, 0, 0, None, 0, counts.ctypes.data, lane_status.ctypes.data, None, None) == nv.BSK_ERR_INVALID
    assert L.bsk_contour_march_host(*march, 2, 3, 0, None, 0, counts.ctypes.data, lane_status.ctypes.data, None, None) == nv.BSK_ERR_INVALID
    assert L.bsk_contour_march_host(*march, 2, 0, 1, None, 0, None, None, None, None) == nv.BSK_ERR_INVALID
    # a candidate index that is no cell, and a window that leaves the rows, give no segment and no read out of bounds
    bad = np.array([-1, 10 ** 9], np.int64)
    c2, s2 = np.full(2, -1, np.int32), np.full(2, 255, np.uint8)
    assert L.bsk_contour_march_host(*grid, b0.ctypes.data, b1.ctypes.data, bad.ctypes.data, 2, 2, 0, 0, None, 0, c2.ctypes.data, s2.ctypes.data,
                                    None, None) == nv.BSK_OK
    assert c2.tolist() == [0, 0] and s2.tolist() == [0, 0]
    far = np.full_like(first0, 10 ** 6)
    grid_far = C._grid(plan, rows, lambda a: a.ctypes.data, None, 1, scale, far, first1)
    cand, zero = np.full(res["cand"].shape, 7, np.uint8), np.full(res["cand"].shape, 7, np.uint8)
    assert L.bsk_contour_flag_host(*grid_far, cand.ctypes.data, zero.ctypes.data) == nv.BSK_OK and not cand.any() and not zero.any()


def test_library_exports_the_declared_family():
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bspy_amd.h")).read()
    declared = set(re.findall(r"\b(bsk_contour_[a-z_]+)\s*\((?:void|int )", header))
    assert declared == set(FAMILY) and declared <= set(nv.PRODUCT_SYMBOLS)
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
