"""
Spline.intersect_surface and surfaces.trace_pair on the GPU (ray_boxes, ssx_count, ssx_emit, ssx_isolate, ssx_merge, the
band kernels for the extraction): every golden of tests/golden/surfaces.npz through ``_path="device"`` with the kernels that
ran asserted from ``surfaces.LAST_PATHS`` and ``bsk_ssx_last_kernel``, bit-equal to the host path (which
tests/test_surfaces_host.py holds to the exact oracle) and on a second run; both surfaces x 2^+-40 with the same bytes; the
layouts of the launches; the fused family
against the parent's only alternative, ``roots3.zeros3_batch`` on the materialised systems of every line, byte for byte;
and the fitted curves of ``Spline.intersect_surface`` (``Spline.least_squares`` needs the device).  No kernel of the family
uses LDS (the resource log shows 0 bytes for all 32), so there is no stale-LDS test to go with it.
"""
import warnings

import numpy as np
import pytest

import bspy_amd
import surfaces_ref
from bspy_amd import _native as nv
from bspy_amd import roots, roots3, surfaces
from conftest import observe
from surfaces_util import NAMES, curve_at, lipschitz, load_case, make, same_result

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BANDS = {"band_apply", "band_apply_line"}


def launches(ran):
    return [p for p in ran if p not in BANDS]


def expected(host_ran):
    """The launches of the device path from those of the host path on the same numbers."""
    return [p[len("host "):] for p in host_ran if p.startswith(("host ray_", "host ssx_"))]


def spline_of(case):
    order, knots, coefs = case
    return bspy_amd.Spline(2, 3, order, list(coefs.shape[1:]), knots, coefs)


@pytest.mark.parametrize("name", NAMES)
def test_golden_device(name):
    c = load_case(name)
    a, b = make(c)
    host = surfaces.trace_pair(a, b, depth=c["depth"], _path="host")
    host_ran = list(surfaces.LAST_PATHS)
    dev = surfaces.trace_pair(a, b, depth=c["depth"], _path="device")
    ran = launches(surfaces.LAST_PATHS)
    assert ran == expected(host_ran) and ran[:2] == ["ray_boxes", "ray_boxes"] and ran[2] == "ssx_count"
    assert nv.lib().bsk_ssx_last_kernel().decode() == [p for p in ran if p.startswith("ssx_")][-1]
    assert same_result(host, dev)
    assert same_result(dev, surfaces.trace_pair(a, b, depth=c["depth"], _path="device"))
    if c["kind"] in ("edge", "corner"):
        assert "ssx_merge" in ran
    if name == "disjoint":                                  # no candidates: emit, isolate and merge are skipped
        assert ran[2:] == ["ssx_count"] * 4


@pytest.mark.parametrize("name", ["plane_d1", "loop"])
@pytest.mark.parametrize("k", [-40, 40])
def test_scaling_both_surfaces_by_a_power_of_two_changes_no_byte_on_the_device(name, k):
    """The device twin of the test of its name in tests/test_surfaces_host.py: the walk's thresholds are relative and a power
    of two commutes with every rounding, so both surfaces x 2^k give the bytes of the unscaled device run and of the host
    run, from the ssx_* kernels."""
    c = load_case(name)
    a, b = make(c)
    host = surfaces.trace_pair(a, b, depth=c["depth"], _path="host")
    host_ran = list(surfaces.LAST_PATHS)
    dev = surfaces.trace_pair(a, b, depth=c["depth"], _path="device")
    ran = launches(surfaces.LAST_PATHS)
    a2, b2 = make(c, 2.0 ** k)
    scaled = surfaces.trace_pair(a2, b2, depth=c["depth"], _path="device")
    ran2 = launches(surfaces.LAST_PATHS)
    assert ran2 == ran == expected(host_ran) and {"ssx_count", "ssx_emit", "ssx_isolate"} <= set(ran2)
    assert nv.lib().bsk_ssx_last_kernel().decode() == [p for p in ran2 if p.startswith("ssx_")][-1]
    assert same_result(dev, scaled) and same_result(host, scaled)
    assert same_result(scaled, surfaces.trace_pair(a2, b2, depth=c["depth"], _path="host"))


def test_layouts_against_the_host_drivers():
    """A 5 x 3-cell surface against a 9 x 7-cell one at depth 2: families of 63, 65, 259 and 261 line segments (one
    workgroup less one lane, one more, more than 256), against 63 and 15 cells; 1, 3 and 13 chunks of the cells; passes
    halved down to single segments; without the prefilter."""
    a = spline_of(surfaces_ref.patch((3, 4), (np.linspace(0, 1, 6) ** 1.2, np.linspace(0, 1, 4)), lambda u, v: 0.03 + 0.9 * u + 0.05 * v,
                                     lambda u, v: 0.02 - 0.04 * u + 0.95 * v, lambda u, v: 0.45 + 0.2 * u - 0.1 * v + 0.1 * u * v))
    b = spline_of(surfaces_ref.patch((4, 4), (np.linspace(0, 1, 10), np.linspace(0, 1, 8) ** 0.9), lambda u, v: u, lambda u, v: v,
                                     lambda u, v: 0.5 + 0.3 * np.sin(5 * u) * np.cos(4 * v)))
    host = surfaces.trace_pair(a, b, depth=2, _path="host")
    assert [f["nseg"] for f in host[4]["families"]] == [63, 65, 259, 261] and host[4]["candidates"] > 256 and len(host[0]) > 20
    for kw in ({}, dict(_chunk=5), dict(_chunk=10 ** 6), dict(_prefilter=False), dict(_pairs=1), dict(_pairs=40, _chunk=7)):
        dev = surfaces.trace_pair(a, b, depth=2, _path="device", **kw)
        assert same_result(host, dev), kw
        counts = surfaces.LAST_PATHS.count("ssx_count")
        assert counts == 4 if "_pairs" not in kw else counts > 4, kw        # a family that exceeds _pairs is split


def bezier_knots(breaks, K):
    b = np.asarray(breaks, np.float64)
    return np.concatenate(([b[0]] * K, np.repeat(b[1:-1], K - 1), [b[-1]] * K))


def test_zeros_equal_zeros3_batch_on_the_materialised_systems():
    """2 x 2 cells against 2 x 2 cells at depth 1.  Per family, every line's system is materialised in Bezier form on the
    knots (X's running variable, Y's two): coefficient (i, j, k) = L_i - Y_jk, one NumPy subtraction of the extracted
    isocurve and the extracted rows of Y, which is what the kernel forms in registers.  ``roots3.zeros3_batch`` on the
    device walks them with S_d of its own (the scale enters the status bits only): the zeros must be the same bytes."""
    a = spline_of(surfaces_ref.patch((3, 4), ([0.0, 0.45, 1.0], [0.0, 0.6, 1.0]), lambda u, v: 0.03 + 0.9 * u + 0.05 * v,
                                     lambda u, v: 0.02 - 0.04 * u + 0.95 * v, lambda u, v: 0.45 + 0.2 * u - 0.1 * v + 0.1 * u * v))
    b = spline_of(surfaces_ref.patch((4, 4), ([0.0, 0.55, 1.0], [0.0, 0.4, 1.0]), lambda u, v: u, lambda u, v: v,
                                     lambda u, v: 0.5 + 0.3 * np.sin(5 * u) * np.cos(4 * v)))
    depth, G = 1, 2
    res = surfaces.trace_pair(a, b, depth=depth, _path="device")
    tabs = [surfaces.host_tables(s) for s in (a, b)]
    total = 0
    for fam, got in enumerate(res[4]["families"]):
        ax = fam & 1
        (planX, rowsX, _), (planY, rowsY, _) = (tabs[0], tabs[1]) if fam < 2 else (tabs[1], tabs[0])
        ncfix, ncrun, KR = planX.ncells[ax], planX.ncells[1 - ax], planX.order[1 - ax]
        lines = []
        for n in range(ncfix * G + 1):
            c, g = surfaces.line_owner(n, G, ncfix)
            x = float(g) / float(G)
            f = int(planX.first[ax][c])
            cols = np.moveaxis(rowsX, ax + 1, -1)[:, :, f:f + planX.order[ax]]        # (3, running rows, KF)
            L = np.array([[cols[d, r, 0] if x == 0.0 else (cols[d, r, -1] if x == 1.0 else roots.value([float(v) for v in cols[d, r]], x))
                           for r in range(cols.shape[1])] for d in range(3)])
            lines.append(L[:, :, None, None] - rowsY[:, None, :, :])
        knots = [bezier_knots(planX.breaks[1 - ax], KR), bezier_knots(planY.breaks[0], planY.order[0]), bezier_knots(planY.breaks[1], planY.order[1])]
        coefs = np.stack(lines)
        system = bspy_amd.Spline(3, 3, [KR, *planY.order], list(coefs.shape[2:]), knots, coefs[0])
        values, offsets, cells, status = roots3.zeros3_batch(system, coefs=coefs, _path="device")
        assert len(cells) == 0 and not status.any()
        at = np.argwhere(got["keep"] != 0)
        line_of = got["pair_seg"][at[:, 0]] // ncrun
        for n in range(len(lines)):
            mine = got["roots"][at[line_of == n, 0], at[line_of == n, 1]]
            mine = mine[np.lexsort((mine[:, 2], mine[:, 1], mine[:, 0]))].reshape(-1, 3)
            assert mine.tobytes() == values[offsets[n]:offsets[n + 1]].tobytes(), (fam, n)
            total += len(mine)
    assert total >= 8


@pytest.mark.parametrize("name,tolerance", [("loop", 2.0 ** -8), ("open_b", 2.0 ** -8), ("plane_d2", None)])
def test_intersect_surface_curves_lie_on_both_surfaces(name, tolerance):
    """self(*ca(t)) and other(*cb(t)) at 33 parameter values.  Both curves are fitted to ``tolerance`` (the residual at a
    vertex, in parameter units) and a chord of one leaf leaves the true curve by the sagitta that ``depth_of`` bounds by
    ``tolerance`` L, L the larger extent of the domain, so each curve is within tolerance (1 + L) of the true one in
    its own parameters and the two points in space differ by no more than (M_a + M_b) tolerance (1 + L), M the bound
    ``lipschitz``.  (tests/test_surfaces_host.py holds the polyline itself to the same bound: the reference alone passes.)"""
    c = load_case(name)
    a, b = make(c)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        depth = None if tolerance is not None else c["depth"]
        found = a.intersect_surface(b, depth=depth, tolerance=tolerance)
    plans = [surfaces.Plan(s.order, s.knots) for s in (a, b)]
    L = max(float(br[-1]) - float(br[0]) for plan in plans for br in plan.breaks)
    tol = tolerance if tolerance is not None else max((float(np.diff(np.asarray(br, np.float64)).max()) * 2.0 ** -c["depth"]) ** 2 / L
                                                      for plan in plans for br in plan.breaks)
    bound = (lipschitz(a) + lipschitz(b)) * tol * (1.0 + L)
    closed = surfaces.trace_pair(a, b, depth=surfaces.depth_of(tolerance, plans) if tolerance is not None else c["depth"], _path="host")[2]
    assert len(found) == len(closed) == 1
    t = np.linspace(0.0, 1.0, 33)
    for m, (ca, cb) in enumerate(found):
        assert (ca.nInd, ca.nDep, cb.nInd, cb.nDep) == (1, 2, 1, 2) and max(ca.order[0], cb.order[0]) <= 4
        assert float(ca.knots[0][0]) == 0.0 and float(ca.knots[0][-1]) == 1.0
        pa, pb = curve_at(ca, t), curve_at(cb, t)
        gap = np.abs(surfaces._evaluate(a, pa[0], pa[1]) - surfaces._evaluate(b, pb[0], pb[1])).max()
        observe(f"surfaces curves |a(ca) - b(cb)| / bound, {name}", gap / bound, 1.0)
        if closed[m]:
            for curve in (ca, cb):
                assert np.asarray(curve.coefs)[:, 0].tobytes() == np.asarray(curve.coefs)[:, -1].tobytes()
                ends = curve_at(curve, t[[0, -1]])
                assert ends[:, 0].tobytes() == ends[:, 1].tobytes()
