"""
The device half of remove_knots (bspy_amd/reduction.py): bsk_band_absmax (band_absmax, band_absmax_line and the fold)
against bsk_band_absmax_host bit for bit, planted maxima and NaNs, and remove_knots end to end on the device against the
host path, the goldens of tests/golden/remove.npz and the checks of tests/test_remove_host.py.  Every test is tied to
its kernel through reduction.LAST_PATHS / bsk_band_last_kernel.
"""
import numpy as np
import pytest

from bspy_amd import Spline, reduction
from bspy_amd.refinement import BandMap
from conftest import observe
from test_remove_host import (RECOVER_NAMES, REDUCE_NAMES, check_recovered, check_reduced, check_rounds, golden,  # noqa: F401
                              random_knots, some_map, spline_of)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS, LINE = "band_absmax", "band_absmax_line"

# (name, shape, axis, groups, nOut, kernel, how the device tensor is made)
SHAPES = [
    ("scalar_lanes", (3, 37, 29), 1, 3, 41, ROWS, "plain"),
    ("wide_lanes", (3, 36, 32), 1, 1, 40, ROWS, "plain"),
    ("wide_shape_misaligned", (3, 36, 32), 1, 3, 40, ROWS, "offset"),
    ("wide_shape_view", (3, 36, 32), 1, 1, 40, ROWS, "view"),
    ("line", (3, 29, 37), 2, 3, 43, LINE, "plain"),
    ("line_two_tiles", (2, 300), 1, 2, 290, LINE, "plain"),
    ("line_misaligned", (2, 300), 1, 1, 290, LINE, "offset"),
    ("groups_middle_axis", (3, 5, 40, 7), 2, 3, 44, ROWS, "plain"),
    ("many_partials_rows", (1, 40, 5000), 1, 1, 37, ROWS, "plain"),
    ("many_partials_line", (6000, 45), 1, 4, 50, LINE, "plain"),
]


def on_device(a, how):
    """The array as a CUDA tensor: as it is, one element off the allocation's alignment, or a non-contiguous view."""
    t = torch.from_numpy(a)
    if how == "plain":
        return t.cuda()
    if how == "offset":
        flat = torch.empty(a.size + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.reshape(-1).cuda()
        out = flat[1:].view(a.shape)
        assert out.is_contiguous() and out.data_ptr() % 16 != 0
        return out
    moved = t.movedim(-1, 0).contiguous().cuda().movedim(0, -1)
    assert not moved.is_contiguous()
    return moved


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_absmax_matches_the_host_driver(case, dtype):
    name, shape, axis, groups, n_out, kernel, how = case
    rng = np.random.default_rng(len(name) + shape[0])
    a = rng.standard_normal(shape).astype(dtype)
    out_shape = list(shape)
    out_shape[axis] = n_out
    minus = rng.standard_normal(out_shape).astype(dtype)
    ta, tm = on_device(a, how), on_device(minus, how)
    for K in (2, 5, 8):
        first, w = some_map(rng, K, shape[axis], n_out)
        band = BandMap(first, w, shape[axis])
        try:
            for m, tmm in ((None, None), (minus, tm)):
                got = reduction.absmax(band, ta, axis, groups, tmm)
                assert got.shape == (groups, n_out) and got.dtype == torch.float64 and got.is_cuda
                assert band.last_kernel() == kernel and reduction.LAST_PATHS == [kernel]
                want = reduction.absmax_host(band, a, axis, groups, m)
                assert np.array_equal(got.cpu().numpy(), want), (name, K, m is not None)
        finally:
            band.close()


@pytest.mark.parametrize("case", [SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[7], SHAPES[8], SHAPES[9]], ids=lambda c: c[0])
def test_planted_values_and_nan(case):
    name, shape, axis, groups, n_out, kernel, _ = case
    rng = np.random.default_rng(99)
    K = 4
    first = np.floor(np.linspace(0, shape[axis] - K, n_out) + 0.5).astype(np.int32)      # every column lies under a row
    w = 0.5 + rng.random((n_out, K))                        # no cancellation: a planted value shows in every row over it
    band = BandMap(first, w, shape[axis])
    base = (2.0 * rng.random(shape) - 1.0)
    last = tuple(s - 1 for s in shape)
    middle = tuple(s - 1 if d != axis else s // 2 for d, s in enumerate(shape))       # the last line, a row in the middle
    lines_per_group = int(np.prod(shape[:axis])) // groups
    try:
        for spot in ((0,) * len(shape), last, middle):
            for value in (1e6, np.nan):
                a = base.copy()
                a[spot] = value
                got = reduction.absmax(band, torch.from_numpy(a).cuda(), axis, groups).cpu().numpy()
                assert band.last_kernel() == kernel
                assert np.array_equal(got, reduction.absmax_host(band, a, axis, groups))
                group = int(np.ravel_multi_index(spot[:axis], shape[:axis])) // lines_per_group if axis else 0
                hit = np.zeros((groups, n_out), bool)
                hit[group] = (first <= spot[axis]) & (spot[axis] < first + K)
                assert hit.any()
                if np.isnan(value):
                    assert np.all(np.isposinf(got[hit])) and np.all(np.isfinite(got[~hit]))
                else:
                    assert np.all(got[hit] > 4e5) and np.all(got[~hit] <= 1.5 * K)
    finally:
        band.close()


# ------------------------------------------------------------------------------------------ remove_knots end to end
def both_paths(s, tolerance):
    host = s.remove_knots(tolerance, _path="host")
    host_rounds = [list(map(list, v)) for v in reduction.LAST_ROUNDS]
    dev = s.remove_knots(tolerance, _path="device")
    paths = list(reduction.LAST_PATHS)
    assert [list(map(list, v)) for v in reduction.LAST_ROUNDS] == host_rounds
    again = s.remove_knots(tolerance, _path="device")
    for other in (host, again):
        assert dev.coefs.tobytes() == other.coefs.tobytes() and dev.nCoef == other.nCoef
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dev.knots, other.knots))
    assert paths and all(not p.startswith("host") for p in paths)
    check_rounds(s.order)
    return dev, paths


@pytest.mark.parametrize("name", RECOVER_NAMES)
def test_device_recovers_inserted_knots(golden, name):  # noqa: F811
    p = f"recover/{name}/"
    s = spline_of(golden, p, "in_knots", "in_coefs")
    r, paths = both_paths(s, 1e-12)
    err = check_recovered(r, [golden[f"{p}knots{iv}"] for iv in range(s.nInd)], golden[p + "coefs"])
    observe("remove_knots on the device, recovery of inserted knots, coefficients", err, 1e-12)
    assert r.metadata == s.metadata
    if s.nInd > 1:
        assert {"band_absmax", "band_absmax_line", "band_apply", "band_apply_line"} <= set(paths)
    else:
        assert {"band_absmax_line", "band_apply_line"} == set(paths)


@pytest.mark.parametrize("name", REDUCE_NAMES)
def test_device_tolerance_cases(golden, name):  # noqa: F811
    p = f"reduce/{name}/"
    s = spline_of(golden, p)
    tolerance = float(golden[p + "tolerance"])
    r, _ = both_paths(s, tolerance)
    ratio = check_reduced(s, r, tolerance, golden[p + "ref_ncoef"])
    observe("remove_knots on the device, exact certified error / bound", ratio, 1.0)


def test_surface_40x36x3_is_recovered():
    rng = np.random.default_rng(4036)
    t = [random_knots(rng, 4, 28), random_knots(rng, 3, 27)]
    s = Spline(2, 3, [4, 3], [28, 27], t, rng.standard_normal((3, 28, 27)) + 0.3)
    fine = s.insert_knots([list(0.02 + 0.96 * rng.random(12)), list(0.02 + 0.96 * rng.random(9))], _path="host")
    assert fine.nCoef == (40, 36)
    r, paths = both_paths(fine, 1e-12)
    observe("remove_knots on the device, 40 x 36 x 3 surface, coefficients", check_recovered(r, s.knots, s.coefs), 1e-12)
    assert {"band_absmax", "band_absmax_line", "band_apply", "band_apply_line"} <= set(paths)


def test_default_path_is_the_device_from_the_threshold():
    rng = np.random.default_rng(150)
    n = 150
    assert 3 * n * n >= reduction.DEVICE_MIN_ELEMENTS > 3 * 40 * 36
    t = [random_knots(rng, 3, n), random_knots(rng, 3, n)]
    s = Spline(2, 3, [3, 3], [n, n], t, rng.standard_normal((3, n, n)))
    r = s.remove_knots()
    assert reduction.LAST_PATHS == ["band_absmax", "band_absmax_line"] and r.nCoef == s.nCoef
    assert r.coefs.tobytes() == s.coefs.tobytes() and r is not s


def test_order_8_variable_takes_the_host_path():
    rng = np.random.default_rng(83)
    t = [random_knots(rng, 8, 13), random_knots(rng, 3, 9)]
    s = Spline(2, 2, [8, 3], [13, 9], t, rng.standard_normal((2, 13, 9)))
    fine = s.insert_knots([[0.4], [0.3, 0.7]], _path="host")
    r = fine.remove_knots(1e-12, _path="device")
    assert set(reduction.LAST_PATHS) == {"host band", "host band_absmax"}
    assert check_recovered(r, s.knots, s.coefs) <= 1e-12
