"""
remove_knot, remove_knots and range_bounds without a GPU: the reference's messages, the operator maps, the host half of
the library (bsk_band_absmax_host and bsk_band_apply_fma_host through ctypes, which make no HIP call) against the
goldens of tests/golden/remove.npz (written by tests/golden/make_golden_remove.py from the reference) and against the
exact results of tests/remove_ref.py.  The device half is covered by tests/test_gpu_remove.py, which takes its helpers
and checks from here.

Bars:
  remove_knot                coefficients and residual against the reference and against the exact result: 1e-12 of
                             max |coef| (the parity bar of tests/test_gpu_parity.py), 2^-23 for float32; knots and the
                             coefficients outside the window bit for bit
  operator maps              rows of removal_map sum to 1 within 64 eps; a residual_map row annihilates a spline that
                             lacks the knot within 64 eps of max |coef|
  recovery                   insert-then-remove at tolerance 1e-12: the original knots bit for bit, the original
                             coefficients within 1e-12 of max |coef|
  certified error            exact E_d (rational arithmetic) <= tolerance S_d + 16 (k + 1) nInd eps S_d: the second term
                             is the rounding of one band row per reduced variable (k the largest order)
  count                      nCoef <= the reference's nCoef + max(2, 10 % of the knots the reference removed), per variable
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import remove_ref
from bspy_amd import Spline, reduction, refinement
from bspy_amd import _native as nv
from bspy_amd.refinement import BandMap
from conftest import GOLDEN, observe

EPS = np.finfo(np.float64).eps


def _group(prefix):
    with np.load(os.path.join(GOLDEN, "remove.npz")) as g:
        return sorted({k.split("/")[1] for k in g.files if k.startswith(prefix + "/")})


KNOT_NAMES, RECOVER_NAMES, REDUCE_NAMES = _group("knot"), _group("recover"), _group("reduce")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "remove.npz"))


def curve(order, knots, coefs):
    return Spline(1, coefs.shape[0], [order], [coefs.shape[1]], [knots], coefs)


def spline_of(g, prefix, knots="knots", coefs="coefs"):
    order = [int(o) for o in g[prefix + "order"]]
    c = g[prefix + coefs]
    return Spline(len(order), c.shape[0], order, c.shape[1:], [g[f"{prefix}{knots}{iv}"] for iv in range(len(order))], c,
                  {"Name": prefix})


def bar_of(dtype):
    return 1e-12 if np.dtype(dtype) == np.float64 else 2.0 ** -23


# ------------------------------------------------------------------------------------------ remove_knot
@pytest.mark.parametrize("name", KNOT_NAMES)
def test_remove_knot_against_reference_and_exact(golden, name):
    p = f"knot/{name}/"
    k, t, c = int(golden[p + "order"]), golden[p + "knots"], golden[p + "coefs"]
    i, nLeft, nRight = int(golden[p + "iKnot"]), int(golden[p + "nLeft"]), int(golden[p + "nRight"])
    r, residual = curve(k, t, c).remove_knot(i, nLeft, nRight)
    assert r.coefs.dtype == c.dtype and residual.dtype == c.dtype and residual.shape == (c.shape[0],)
    assert r.order == (k,) and r.nCoef == (c.shape[1] - 1,)
    # knots and the coefficients away from the window: bit for bit
    assert r.knots[0].dtype == t.dtype and r.knots[0].tobytes() == golden[p + "out_knots"].tobytes()
    assert r.coefs[:, :i - k].tobytes() == np.ascontiguousarray(c[:, :i - k]).tobytes()
    assert r.coefs[:, i:].tobytes() == np.ascontiguousarray(c[:, i + 1:]).tobytes()

    want, want_res = golden[p + "out_coefs"].astype(np.float64), golden[p + "residual"].astype(np.float64)
    exact, res2 = remove_ref.remove_knot(t, k, c, i, nLeft, nRight)
    exact = remove_ref.refine_ref.to_float(exact, c.dtype).astype(np.float64)
    exact_res = np.array([math.sqrt(v) for v in res2]).astype(c.dtype).astype(np.float64)
    scale = np.abs(exact).max()
    kind = np.dtype(c.dtype).name
    bar = bar_of(c.dtype)
    got, got_res = r.coefs.astype(np.float64), residual.astype(np.float64)
    observe(f"remove_knot coefs vs reference ({kind})", np.abs(got - want).max() / scale, bar)
    observe(f"remove_knot coefs vs exact ({kind})", np.abs(got - exact).max() / scale, bar)
    observe(f"remove_knot residual vs reference ({kind})", np.abs(got_res - want_res).max() / scale, bar)
    observe(f"remove_knot residual vs exact ({kind})", np.abs(got_res - exact_res).max() / scale, bar)


def test_remove_knot_messages():
    with open(os.path.join(GOLDEN, "remove_semantics.json")) as f:
        records = json.load(f)
    assert {r["error"] for r in records} >= {"Must have one independent variable", "Must specify interior knots for removal", None}
    for record in records:
        s = record["spline"]
        coefs = np.array(s["coefs"])
        spline = Spline(len(s["order"]), coefs.shape[0], s["order"], coefs.shape[1:], [np.array(k) for k in s["knots"]], coefs)
        if record["error"] is None:
            r, residual = spline.remove_knot(*record["args"])
            assert r.nCoef[0] == spline.nCoef[0] - 1 and residual.shape == (spline.nDep,)
        else:
            with pytest.raises(ValueError) as info:
                spline.remove_knot(*record["args"])
            assert str(info.value) == record["error"], record["name"]


def test_remove_knot_refuses_weights_that_are_not_finite():
    # a fixed unknown whose pivot 1 - alpha is zero (a knot of full multiplicity): the reference returns inf / nan
    t = np.array([0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 1.0, 1.0, 1.0])
    s = curve(3, t, np.arange(12.0).reshape(2, 6))
    with pytest.raises(ValueError, match="not finite"):
        s.remove_knot(5, nLeft=4)
    r = s.remove_knots(1e-3, nLeft=4, _path="host")             # the knot is skipped, nothing fails
    assert r.nCoef[0] <= 6


def test_range_bounds():
    rng = np.random.default_rng(3)
    for dtype in (np.float64, np.float32):
        c = rng.standard_normal((3, 5, 4)).astype(dtype)
        t = [np.array([0, 0, 0, .3, .6, 1, 1, 1.0]), np.array([0, 0, .3, .6, 1, 1.0])]
        b = Spline(2, 3, [3, 2], [5, 4], t, c).range_bounds()
        assert b.dtype == dtype and b.shape == (3, 2)
        assert np.array_equal(b, np.stack((c.reshape(3, -1).min(axis=1), c.reshape(3, -1).max(axis=1)), axis=1))


# ------------------------------------------------------------------------------------------ operator maps
def random_knots(rng, k, n, double=()):
    interior = np.sort(rng.random(n - k - len(double)))
    reps = np.ones(len(interior), int)
    reps[list(double)] += 1
    return np.concatenate((k * [0.0], np.repeat(interior, reps), k * [1.0]))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8])
def test_removal_map_rows_and_units(k):
    rng = np.random.default_rng(k)
    n = 4 * k + 9
    t = random_knots(rng, k, n, double=(2,))
    indices = [k, 2 * k + 2, n - 1]
    for nLeft, nRight in ((0, 0), (1, 0), (0, 2), (2, 1)):
        newKnots, first, w = reduction.removal_map(t, k, indices, nLeft, nRight)
        assert np.array_equal(newKnots, np.delete(t, indices)) and w.shape == (n - 3, k + 1)
        assert np.all(np.diff(first) >= 0) and first.min() >= 0 and first.max() + k + 1 <= n
        assert np.abs(w.sum(axis=1) - 1.0).max() <= 64 * EPS
        window = np.zeros(n - 3, bool)
        for s, i in enumerate(indices):
            window[i - k - s:i - s] = True
        units = w[~window]
        assert np.all((units == 0.0) | (units == 1.0)) and np.all((units == 1.0).sum(axis=1) == 1)
        # one knot at a time gives the same rows
        for s, i in enumerate(indices):
            _, f1, w1 = reduction.removal_map(t, k, [i], nLeft, nRight)
            assert np.array_equal(w1[i - k:i], w[i - k - s:i - s]) and np.all(f1[i - k:i] == i - k)
    with pytest.raises(ValueError):
        reduction.removal_map(t, k, [k, 2 * k], 0, 0)
    with pytest.raises(ValueError, match="Must specify interior knots for removal"):
        reduction.removal_map(t, k, [k - 1], 0, 0)


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
def test_residual_map_annihilates_splines_without_the_knot(k):
    rng = np.random.default_rng(10 + k)
    n = 2 * k + 8
    t = random_knots(rng, k, n, double=(1,))
    indices, first, v = reduction.residual_map(t, k)
    assert np.array_equal(indices, np.arange(k, n)) and np.array_equal(first, indices - k) and v.shape == (n - k, k + 1)
    worst = 0.0
    for row, i in enumerate(indices):
        small = curve(k, np.delete(t, i), rng.standard_normal((2, n - 1)) + 0.3)
        big = small.insert_knots([[t[i]]], _path="host")
        assert np.array_equal(big.knots[0], t)
        value = np.abs(big.coefs[:, i - k:i + 1] @ v[row]).max()
        worst = max(worst, value / np.abs(big.coefs).max())
        # and remove_knot reports |row . line|
        _, residual = big.remove_knot(int(i))
        assert np.abs(residual).max() <= 64 * EPS * np.abs(big.coefs).max()
    observe("residual_map row on a spline without the knot (of scale)", worst, 64 * EPS)


def test_select():
    rho = np.array([0.5, 1e-3, 2e-3, 1e-3, np.inf, 0.0, 1e-4, 1e-3, 1e-3, 1e-3, 1e-3])
    assert reduction.select(rho, 3, 1e-3) == [8, 4, 12]        # 0.0 at index 8, then 1e-4 at 9 is too near, ties by index
    assert reduction.select(rho, 3, -1.0) == [] and reduction.select(np.array([np.nan, np.inf]), 3, 1.0) == []
    assert reduction.select(np.zeros(9), 1, 0.0) == [1, 3, 5, 7, 9]


# ------------------------------------------------------------------------------------------ remove_knots
def check_recovered(r, knots, coefs):
    """The checks of an insert-then-remove case: the original knots bit for bit, coefficients within 1e-12 of scale."""
    for got, want in zip(r.knots, knots):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert r.coefs.dtype == coefs.dtype and r.coefs.shape == coefs.shape
    return np.abs(r.coefs.astype(np.float64) - coefs).max() / np.abs(coefs).max()


def check_rounds(order):
    for iv, rounds in enumerate(reduction.LAST_ROUNDS):
        for kept in rounds:
            assert kept and all(abs(a - b) >= order[iv] + 1 for n, a in enumerate(kept) for b in kept[:n])


@pytest.mark.parametrize("name", RECOVER_NAMES)
def test_insert_then_remove_recovers_the_knots(golden, name):
    p = f"recover/{name}/"
    s = spline_of(golden, p, "in_knots", "in_coefs")
    r = s.remove_knots(1e-12, _path="host")
    assert r is not s and r.metadata == s.metadata
    nInd = s.nInd
    err = check_recovered(r, [golden[f"{p}knots{iv}"] for iv in range(nInd)], golden[p + "coefs"])
    observe("remove_knots recovery of inserted knots, coefficients", err, 1e-12)
    check_rounds(s.order)
    assert sum(len(kept) for rounds in reduction.LAST_ROUNDS for kept in rounds) == sum(s.nCoef) - sum(r.nCoef)
    assert set(reduction.LAST_PATHS) == {"host band", "host band_absmax"}
    assert tuple(golden[p + "ref_ncoef"]) == r.nCoef            # the reference recovers these at 1e-12 too


def test_hundred_random_curves_recover():
    worst, recovered = 0.0, 0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        for k in range(2, 7):
            n = k + 3 + int(rng.integers(0, 8))
            t = random_knots(rng, k, n)
            s = curve(k, t, rng.standard_normal((2, n)))
            new = list(0.02 + 0.96 * rng.random(5))
            r = s.insert_knots([new], _path="host").remove_knots(1e-12, _path="host")
            worst = max(worst, check_recovered(r, s.knots, s.coefs))
            recovered += 1
    assert recovered == 100
    observe("remove_knots recovery, 100 random curves, coefficients", worst, 1e-12)


def check_reduced(s, r, tolerance, ref_ncoef):
    """The checks of a tolerance case; returns (excess of the exact certified error over its bound, nCoef)."""
    nInd, k = s.nInd, max(s.order)
    scale = np.abs(s.coefs.reshape(s.nDep, -1)).max(axis=1)
    scale[scale == 0.0] = 1.0
    E = remove_ref.certified_error(list(s.order), list(s.knots), s.coefs, list(r.knots), r.coefs)
    bound = tolerance * scale + 16 * (k + 1) * nInd * np.finfo(s.coefs.dtype).eps * scale
    for iv in range(nInd):
        removed = s.nCoef[iv] - int(ref_ncoef[iv])
        assert r.nCoef[iv] <= int(ref_ncoef[iv]) + max(2, 0.1 * removed), (iv, r.nCoef, tuple(ref_ncoef))
        # the result's knots are knots of the input
        rest = list(s.knots[iv])
        for value in r.knots[iv]:
            rest.remove(value)
    return float(np.max(E / bound))


@pytest.mark.parametrize("name", REDUCE_NAMES)
def test_certified_error_and_count(golden, name):
    p = f"reduce/{name}/"
    s = spline_of(golden, p)
    tolerance = float(golden[p + "tolerance"])
    r = s.remove_knots(tolerance, _path="host")
    rounds = [list(map(list, v)) for v in reduction.LAST_ROUNDS]
    check_rounds(s.order)
    print(f"{name}: nCoef {s.nCoef} -> {r.nCoef}, reference {tuple(golden[p + 'ref_ncoef'])}, rounds {[len(v) for v in rounds]}")
    ratio = check_reduced(s, r, tolerance, golden[p + "ref_ncoef"])
    observe("remove_knots exact certified error / (tolerance S + 16 (k + 1) nInd eps S)", ratio, 1.0)
    # a second run gives the same bits and the same rounds
    again = s.remove_knots(tolerance, _path="host")
    assert again.coefs.tobytes() == r.coefs.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(again.knots, r.knots))
    assert [list(map(list, v)) for v in reduction.LAST_ROUNDS] == rounds
    assert r.metadata == s.metadata and r is not s


def host_apply(first, w, data, axis):
    band = BandMap(first, w, data.shape[axis])
    try:
        return reduction.apply_fma_host(band, data, axis)
    finally:
        band.close()


def host_absmax(first, w, data, axis, groups, minus=None):
    band = BandMap(first, w, data.shape[axis])
    try:
        return reduction.absmax_host(band, data, axis, groups, minus)
    finally:
        band.close()


@pytest.mark.parametrize("name", [n for n in REDUCE_NAMES if n.startswith("curve")])
def test_no_removable_knot_is_left(golden, name):
    """After the call the smallest remaining rho is above the tolerance, or removing that knot alone fails the certificate."""
    p = f"reduce/{name}/"
    s = spline_of(golden, p)
    tolerance = float(golden[p + "tolerance"])
    r = s.remove_knots(tolerance, _path="host")
    k, t = r.order[0], r.knots[0]
    if r.nCoef[0] == k:
        return
    scale = np.abs(s.coefs).max(axis=1)
    indices, first, v = reduction.residual_map(t, k)
    rho = (host_absmax(first, v, r.coefs, 1, s.nDep) / scale[:, None]).max(axis=0)
    best = int(np.argmin(rho))
    if rho[best] > tolerance:
        return
    newKnots, first, w = reduction.removal_map(t, k, [int(indices[best])])
    candidate = host_apply(first, w, r.coefs, 1)
    first, w = refinement.refine_map(newKnots, k, s.knots[0], 0, origin=reduction._origin(newKnots, s.knots[0]))
    E = host_absmax(first, w, candidate, 1, s.nDep, s.coefs).max(axis=1)
    assert np.max(E / scale) > tolerance


def test_float32_and_default_path():
    rng = np.random.default_rng(5)
    t = random_knots(rng, 4, 12).astype(np.float32)
    s = curve(4, t, rng.standard_normal((2, 12)).astype(np.float32))
    fine = s.insert_knots([[0.21, 0.47, 0.83]], _path="host")
    r = fine.remove_knots(1e-5)                                 # a small tensor: the host path
    assert set(reduction.LAST_PATHS) == {"host band", "host band_absmax"}
    assert r.coefs.dtype == np.float32 and r.knots[0].dtype == np.float32
    assert check_recovered(r, s.knots, s.coefs) <= 1e-5
    same = s.remove_knots()                                     # nothing to remove at 1e-14: a new spline, same bits
    assert same is not s and same.coefs is not s.coefs and same.coefs.tobytes() == s.coefs.tobytes()
    assert reduction.LAST_ROUNDS == [[]]
    with pytest.raises(ValueError):
        s.remove_knots(1e-3, _path="gpu")


# ------------------------------------------------------------------------------------------ host drivers and the ABI
def some_map(rng, K, n_in, n_out):
    first = np.sort(rng.integers(0, n_in - K + 1, n_out)).astype(np.int32)
    return first, rng.standard_normal((n_out, K))


def absmax_numpy(first, w, a, groups, minus=None):
    """a: (outer, nIn, inner): the statement in NumPy, sums rounded per product (within an ulp of the fused chain)."""
    K = w.shape[1]
    acc = np.zeros((a.shape[0], len(first), a.shape[2]))
    for t in range(K):
        acc += w[:, t][None, :, None] * a[:, first + t, :].astype(np.float64)
    acc = acc.astype(a.dtype).astype(np.float64)
    if minus is not None:
        acc = acc - minus.astype(np.float64)
    mag = np.abs(acc)
    mag[np.isnan(mag)] = np.inf
    return mag.reshape(groups, -1, len(first), a.shape[2]).max(axis=(1, 3))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_drivers(dtype):
    rng = np.random.default_rng(21)
    for K, shape, groups in ((2, (4, 13, 5), 2), (5, (3, 29, 1), 3), (8, (6, 40, 7), 1), (9, (2, 30, 3), 2)):
        first, w = some_map(rng, K, shape[1], 17)
        a = rng.standard_normal(shape).astype(dtype)
        minus = rng.standard_normal((shape[0], 17, shape[2])).astype(dtype)
        band = BandMap(first, w, shape[1])
        fused = reduction.apply_fma_host(band, a, 1)
        assert band.last_kernel() == "host band"
        plain = band.apply_host(a, shape[0], shape[2])
        tol = 4 * np.finfo(dtype).eps * (np.abs(w).sum(axis=1).max() * np.abs(a).max())
        assert np.abs(fused.astype(np.float64) - plain).max() <= tol
        for m in (None, minus):
            got = reduction.absmax_host(band, a, 1, groups, m)
            assert band.last_kernel() == "host band_absmax" and got.shape == (groups, 17) and got.dtype == np.float64
            want = absmax_numpy(first, w, a, groups, m)
            assert np.abs(got - want).max() <= tol
            # the maxima are those of the fused rows, exactly
            exact = np.abs(fused.astype(np.float64) - (0.0 if m is None else m.astype(np.float64)))
            assert np.array_equal(got, exact.reshape(groups, -1, 17, shape[2]).max(axis=(1, 3)))
        # one NaN gives +inf in its rows only
        a[shape[0] - 1, 11, 0] = np.nan
        got = reduction.absmax_host(band, a, 1, groups)
        hit = (first <= 11) & (11 < first + K)
        assert np.all(np.isinf(got[groups - 1, hit])) and np.all(np.isfinite(got[groups - 1, ~hit]))
        assert np.all(np.isfinite(got[:groups - 1]))
        band.close()


def test_abi_argument_checks():
    L = nv.lib()
    rng = np.random.default_rng(2)
    a = rng.standard_normal((4, 12, 3))
    out = np.zeros((4, 7))
    first, w = some_map(rng, 3, 12, 7)
    band = BandMap(first, w, 12)
    stream = ctypes.c_void_p(0)
    F64 = nv.BSK_F64
    try:
        for groups in (3, 0, -1, 8):
            assert L.bsk_band_absmax_host(band._handle, F64, a.ctypes.data, 4, 3, groups, None, out.ctypes.data) == nv.BSK_ERR_INVALID
            assert L.bsk_band_absmax(band._handle, F64, a.ctypes.data, 4, 3, groups, None, out.ctypes.data, stream) == nv.BSK_ERR_INVALID
        assert b"groups" in L.bsk_last_error()
        for args in ((None, F64, a.ctypes.data, 4, 3, 2, None, out.ctypes.data), (band._handle, F64, None, 4, 3, 2, None, out.ctypes.data),
                     (band._handle, F64, a.ctypes.data, 4, 3, 2, None, None), (band._handle, 7, a.ctypes.data, 4, 3, 2, None, out.ctypes.data),
                     (band._handle, F64, a.ctypes.data, 0, 3, 1, None, out.ctypes.data)):
            assert L.bsk_band_absmax_host(*args) == nv.BSK_ERR_INVALID
            assert L.bsk_band_absmax(*args, stream) == nv.BSK_ERR_INVALID
        assert L.bsk_band_apply_fma_host(None, F64, a.ctypes.data, 4, 3, out.ctypes.data) == nv.BSK_ERR_INVALID
        assert L.bsk_band_apply_fma_host(band._handle, F64, None, 4, 3, out.ctypes.data) == nv.BSK_ERR_INVALID
        assert L.bsk_band_apply_fma_host(band._handle, F64, a.ctypes.data, 4, 3, None) == nv.BSK_ERR_INVALID
    finally:
        band.close()
    # K outside 2 .. 8: the device entry refuses before it touches a device; the host driver takes them
    for K in (1, 9):
        first, w = some_map(rng, K, 12, 7)
        band = BandMap(first, w, 12)
        try:
            assert L.bsk_band_absmax(band._handle, F64, a.ctypes.data, 4, 3, 2, None, out.ctypes.data, stream) == nv.BSK_ERR_UNSUPPORTED
            assert L.bsk_band_absmax_host(band._handle, F64, a.ctypes.data, 4, 3, 2, None, out.ctypes.data) == nv.BSK_OK
        finally:
            band.close()


def test_order_8_takes_the_host_path_and_says_so():
    rng = np.random.default_rng(8)
    t = random_knots(rng, 8, 14)
    s = curve(8, t, rng.standard_normal((2, 14)))
    fine = s.insert_knots([[0.3, 0.6]], _path="host")
    r = fine.remove_knots(1e-12, _path="device")
    assert set(reduction.LAST_PATHS) == {"host band", "host band_absmax"}
    assert check_recovered(r, s.knots, s.coefs) <= 1e-12
