"""
Spline.project and project.project_batch on the host path (no GPU): the goldens of tests/golden/project.npz (made by
tests/golden/make_golden_project.py from the exact oracle tests/project_ref.py) within a derived bar, the Python statement
of bspy_amd/project.py against the host drivers bit for bit, the tie rule, the status bits, and the argument checks of the
Python layer and of every C entry point.

THE BAR of ``test_golden_host`` (eps of float64; S = max |coefficient, point coordinate| of the case; K = the sum of the
orders; the oracle supplies, from exact derivatives at the certified minimiser, hinv = the row-sum norm of the inverse
Hessian of |S - p|^2 / 2 on the free axes, jmax = max |dS_d / du_a|, hmin = the smallest cell width, and the enclosure
[dist_lo, dist_hi] of the exact distance):
  * a de Casteljau value takes K0 - 1 + K1 - 1 levels of lerps on numbers of size S, two roundings each, and one
    subtraction of p: |delta r_d| <= e_val = 2 K eps S;
  * a first derivative is (K_a - 1) (b_1 - b_0) / h_a of two such intermediates: |delta J_da| <= e_jac = 2 (Kmax - 1) e_val / hmin;
  * carried through g = J^T r: |delta g_a| <= sum_d (|delta r_d| |J_da| + |r_d| |delta J_da|) <= nDep (e_val jmax + dist e_jac);
    the roundings of the products and of the sum itself are relative eps of terms already counted: a factor 2 covers them;
  * the iteration stops when its steps no longer shrink, that is when the computed gradient is rounding noise: the last two
    iterates both lie within hinv |delta g| of the minimiser, so the parameter error is at most 2 hinv |delta g|, with
    |delta g| = 2 nDep (e_val jmax + dist_hi e_jac);
  * plus 4 eps max |domain end| for left + x h and the clamp, the half width of the oracle's certified box, and for
    float32 knots one float32 spacing at the largest domain end (the result is rounded once to the knots' dtype).
  An axis on which the minimiser sits on a domain bound is returned exactly (hinv covers the free axes only).
  The distance: |r| moves by at most sqrt(nDep) jmax per unit of parameter error (along a fixed axis the gradient does not
  vanish), the value rounding gives sqrt(nDep) e_val, the sum of squares and the square root 4 eps dist_hi, and the oracle's
  enclosure its width.
Observed / bar goes through ``observe``; the worst ratio is in the README row.
"""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import project
from conftest import GOLDEN, observe

EPS = float(np.finfo(np.float64).eps)
DATA = np.load(os.path.join(GOLDEN, "project.npz"))
NAMES = [str(n) for n in DATA["names"]]
FAMILY = ("bsk_project_seed_host", "bsk_project_seed", "bsk_project_newton_host", "bsk_project_newton", "bsk_project_last_kernel")


def load_case(name):
    order = [int(k) for k in DATA[name + ".order"]]
    case = dict(order=order, knots=[DATA[f"{name}.knots{a}"] for a in range(len(order))], coefs=DATA[name + ".coefs"],
                samples=int(DATA[name + ".samples"]) or None)
    for key in ("points", "u", "radius", "free", "dist_lo", "dist_hi", "gap", "hinv", "jmax", "hmin", "steps"):
        case[key] = DATA[f"{name}.{key}"]
    return case


def make_spline(case):
    coefs = case["coefs"]
    return bspy_amd.Spline(len(case["order"]), coefs.shape[0], case["order"], list(coefs.shape[1:]), case["knots"], coefs)


def bars(case):
    """(parameter bar (N), distance bar (N)) of the docstring."""
    coefs, points = case["coefs"].astype(np.float64), case["points"]
    nDep = coefs.shape[0]
    S = np.maximum(np.abs(coefs).max(), np.abs(points).max(axis=0))
    K, Kmax = sum(case["order"]), max(case["order"])
    e_val = 2.0 * K * EPS * S
    e_jac = 2.0 * (Kmax - 1) * e_val / case["hmin"]
    dg = 2.0 * nDep * (e_val * case["jmax"] + case["dist_hi"] * e_jac)
    end = max(abs(float(k[0])) for k in case["knots"])
    end = max(end, max(abs(float(k[-1])) for k in case["knots"]))
    par = 2.0 * case["hinv"] * dg + 4.0 * EPS * end + case["radius"].max(axis=0)
    if any(k.dtype == np.float32 for k in case["knots"]):
        par = par + float(np.spacing(np.float32(end)))
    dist = np.sqrt(nDep) * (case["jmax"] * par + e_val) + 4.0 * EPS * case["dist_hi"] + (case["dist_hi"] - case["dist_lo"])
    return par, dist


def check_golden(name, uvw, distance, status, label):
    case = load_case(name)
    assert np.all(DATA[name + ".gap"] > float(DATA["margin"]))             # every recorded point is used, none is left out
    par, dist = bars(case)
    assert uvw.shape == case["u"].shape and distance.shape == par.shape
    assert uvw.dtype == np.result_type(*(k.dtype for k in case["knots"])) and distance.dtype == np.float64
    assert not (status & project.WARN_BITS).any()
    on_bound = ~case["free"].astype(bool)
    assert np.array_equal((status & project.STATUS_BOUND) != 0, on_bound.any(axis=0))
    err = np.abs(uvw.astype(np.float64) - case["u"]).max(axis=0)
    mid = 0.5 * (case["dist_lo"] + case["dist_hi"])
    observe(f"project {label}: parameter error / derived bar", (err / par).max(), 1.0)
    observe(f"project {label}: distance error / derived bar", (np.abs(distance - mid) / dist).max(), 1.0)


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", NAMES)
def test_golden_host(name):
    case = load_case(name)
    spline = make_spline(case)
    uvw, distance, status, steps = project.project_batch(spline, case["points"], samples=case["samples"], _path="host")
    assert project.LAST_PATHS[-2:] == ["host project_seed", "host project_newton"]
    assert set(project.LAST_PATHS[:-2]) <= {"host roots_extract"} and len(project.LAST_PATHS) >= 2 + spline.nInd
    check_golden(name, uvw, distance, status, "host")
    assert steps.tolist() == case["steps"].tolist()                    # the goldens were recorded from the Python statement
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                 # bit 2 alone produces no warning
        again = spline.project(case["points"], samples=case["samples"], _path="host")
    assert again[0].tobytes() == uvw.tobytes() and again[1].tobytes() == distance.tobytes()


def test_float32_points_are_widened_first():
    case = load_case("surface_k44_uniform")
    spline = make_spline(case)
    p32 = case["points"].astype(np.float32)
    a = project.project_batch(spline, p32, _path="host")
    b = project.project_batch(spline, p32.astype(np.float64), _path="host")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    shaped = project.project_batch(spline, p32[:, :6].reshape(3, 2, 3), _path="host")
    assert shaped[0].shape == (2, 2, 3) and shaped[1].shape == (2, 3) and shaped[0].reshape(2, 6).tobytes() == a[0][:, :6].tobytes()
    empty = project.project_batch(spline, np.empty((3, 0)), _path="host")
    assert empty[0].shape == (2, 0) and empty[1].shape == (0,) and empty[2].dtype == np.uint8 and empty[3].dtype == np.int32


# ------------------------------------------------------------------------------------------ the statement, bit for bit
@pytest.mark.parametrize("name", NAMES)
def test_statement_equals_host_drivers(name):
    case = load_case(name)
    spline = make_spline(case)
    rng = np.random.default_rng(7)
    extra = case["points"] + 0.05 * np.abs(case["points"]).max() * rng.standard_normal(case["points"].shape)
    points = np.concatenate((case["points"], extra), axis=1)
    plan, rows, grid = project.host_tables(spline, case["samples"])
    tab = plan.tables(rows)
    for chunk in (None, 5, 2):                                         # C = 1, and C > 1 with a ragged last chunk
        want = project.statement(tab, grid, points, chunk=chunk)
        got = project.project_batch(spline, points, samples=case["samples"], _path="host", _chunk=chunk)
        for w, g in zip(want, got):
            assert w.astype(g.dtype).tobytes() == g.tobytes()
    width = np.array([float(k[-1]) - float(k[0]) for k in case["knots"]])[:, None]
    guess = want[0] + 0.01 * width * rng.standard_normal(want[0].shape)          # also outside the domain: clamped
    want = project.statement(tab, grid, points, guess=guess)
    got = project.project_batch(spline, points, guess=guess, _path="host")
    assert project.LAST_PATHS[-1] == "host project_newton" and "host project_seed" not in project.LAST_PATHS
    for w, g in zip(want, got):
        assert w.astype(g.dtype).tobytes() == g.tobytes()


def test_sample_weights_are_the_rounded_bernstein_basis():
    from fractions import Fraction
    from math import comb
    for K in range(2, 7):
        for G in range(1, 9):
            w = project.sample_weights(K, G)
            for a in range(G):
                x = Fraction(2 * a + 1, 2 * G)
                exact = [comb(K - 1, i) * x ** i * (1 - x) ** (K - 1 - i) for i in range(K)]
                assert np.abs(w[a] - np.array([float(v) for v in exact])).max() <= EPS / 2


def test_tie_goes_to_the_lowest_index():
    case = load_case("curve_tie")
    spline = make_spline(case)
    plan, rows, grid = project.host_tables(spline, case["samples"])
    assert grid.shape == (2, 2)
    samples = grid.tolist()
    for n in range(2):                                                 # the two recorded points on the axis of symmetry
        p = [float(x) for x in case["points"][:, n]]
        assert p[0] == 0.5
        d0, d1 = project.seed_point(samples, p, 0, 1)[0], project.seed_point(samples, p, 1, 2)[0]
        assert d0 == d1 and project.seed_point(samples, p, 0, 2) == (d0, 0)
    points = np.ascontiguousarray(case["points"][:, :2])
    for chunk in (2, 1):
        C = -(-2 // chunk)
        d2, idx = np.empty((C, 2)), np.empty((C, 2), np.int32)
        nv.check(nv.lib().bsk_project_seed_host(2, grid.ctypes.data, 2, points.ctypes.data, 2, chunk, d2.ctypes.data, idx.ctypes.data))
        assert idx.T.tolist() == ([[0], [0]] if C == 1 else [[0, 1], [0, 1]]) and (C == 1 or np.array_equal(d2[0], d2[1]))
    uvw, _, _, _ = project.project_batch(spline, points, samples=2, _path="host", _chunk=1)
    plan1 = project.statement(plan.tables(rows), grid, points, chunk=1)
    assert uvw.tobytes() == plan1[0].tobytes() and np.abs(uvw - 0.5).max() <= 1e-12


# ------------------------------------------------------------------------------------------ status bits
def polyline():
    return bspy_amd.Spline(1, 2, [2], [3], [np.array([0.0, 0.0, 0.5, 1.0, 1.0])], np.array([[0.0, 1.0, 2.0], [0.0, 1.0, 0.0]]))


def test_status_bits():
    case = load_case("surface_k44_uniform")
    spline = make_spline(case)
    points = case["points"].copy()
    points[0, 1], points[2, 4] = np.nan, np.inf
    uvw, distance, status, steps = project.project_batch(spline, points, _path="host")
    assert status[1] == status[4] == project.STATUS_SKIPPED and steps[1] == steps[4] == 0
    assert np.isnan(uvw[:, [1, 4]]).all() and np.isnan(distance[[1, 4]]).all()
    keep = [n for n in range(points.shape[1]) if n not in (1, 4)]
    clean = project.project_batch(spline, case["points"], _path="host")
    assert all(a[..., keep].tobytes() == b[..., keep].tobytes() for a, b in zip((uvw, distance, status, steps), clean))
    with pytest.warns(RuntimeWarning, match=r"2 of 7 points .* flat index 1"):
        spline.project(points, _path="host")
    # a foot point on a domain bound: bit 2, no warning (test_golden_host runs every case under "error")
    assert (clean[2] == project.STATUS_BOUND).sum() == (~case["free"].astype(bool)).any(axis=0).sum() > 0
    # a crease: the closest point of the polyline is its vertex, where Newton's method alternates between the two cells
    uvw, distance, status, steps = project.project_batch(polyline(), np.array([[1.0, 0.2], [2.0, 0.6]]), _path="host")
    assert status[0] & project.STATUS_EVALS and steps[0] == project.EVALS and abs(uvw[0, 0] - 0.5) < 1e-3 and status[1] == 0
    with pytest.warns(RuntimeWarning, match=r"1 of 2 points .* flat index 0"):
        found = polyline().project(np.array([[1.0, 0.2], [2.0, 0.6]]), _path="host")
    assert found[0].tobytes() == uvw.tobytes()


def test_singular_step_is_flagged():
    # a curve that stands still at u = 0 (a double control point): J = 0 there, and with r = 0 nothing is positive definite
    spline = bspy_amd.Spline(1, 2, [3], [3], [np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])], np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]))
    uvw, distance, status, steps = project.project_batch(spline, np.zeros((2, 1)), guess=np.zeros((1, 1)), _path="host")
    assert status[0] & project.STATUS_SINGULAR and uvw[0, 0] == 0.0 and distance[0] == 0.0 and steps[0] == 1


# ------------------------------------------------------------------------------------------ scope and arguments
def test_scope_and_argument_errors():
    rng = np.random.default_rng(0)

    def spline(order, nDep):
        knots = [np.concatenate((k * [0.0], k * [1.0])) for k in order]
        return bspy_amd.Spline(len(order), nDep, list(order), list(order), knots, rng.standard_normal((nDep, *order)))

    for order, nDep in (((3, 3, 3), 3), ((7,), 2), ((5, 3), 3), ((3,), 1), ((3, 3), 4), ((1,), 2)):
        with pytest.raises(NotImplementedError, match="curves .* order 2 to 6 .* surfaces .* orders 2 to 4"):
            spline(order, nDep).project(np.zeros((nDep, 2)))
    s = spline((3, 3), 3)
    pts = np.zeros((3, 4))
    for bad in (np.zeros((2, 4)), np.zeros(())):
        with pytest.raises(ValueError, match=r"points must have the shape \(3, \.\.\.\)"):
            s.project(bad)
    for bad in (np.zeros((3, 4), np.int64), np.zeros((3, 4), np.float16)):
        with pytest.raises(TypeError, match="float32 or float64"):
            s.project(bad)
    with pytest.raises(ValueError, match="guess must have the shape"):
        s.project(pts, guess=np.zeros((2, 3)))
    with pytest.raises(TypeError, match="guess as float32 or float64"):
        s.project(pts, guess=np.zeros((2, 4), np.int32))
    for bad in (0, 9, (2, 2, 2), (0, 3)):
        with pytest.raises(ValueError, match="samples must be from 1 to 8"):
            s.project(pts, samples=bad)
    with pytest.raises(ValueError, match="_path must be"):
        s.project(pts, _path="gpu")
    with pytest.raises(ValueError, match="_chunk must be >= 1"):
        s.project(pts, _chunk=0)
    assert s.project(pts, samples=(2, 5), _path="host")[0].shape == (2, 4)


def newton_args(case, name=None):
    """Valid arguments of bsk_project_newton_host for a golden case, as a dict in the order of the C signature."""
    spline = make_spline(case)
    plan, rows, grid = project.host_tables(spline, case["samples"])
    N = case["points"].shape[1]
    points = np.ascontiguousarray(case["points"])
    tabs = project._axis_tables(plan)
    d2, idx = np.empty((1, N)), np.empty((1, N), np.int32)
    nv.check(nv.lib().bsk_project_seed_host(points.shape[0], grid.ctypes.data, plan.nsamples, points.ctypes.data, N, plan.nsamples,
                                            d2.ctypes.data, idx.ctypes.data))
    out = dict(uvw=np.empty((plan.nind, N)), distance=np.empty(N), status=np.empty(N, np.uint8), steps=np.empty(N, np.int32))
    grid_args = project._grid(plan, rows.ctypes.data, [t.ctypes.data for t in tabs])
    keys = ("nind", "K0", "K1", "ndep", "rows", "R0", "R1", "nc0", "nc1", "first0", "first1", "breaks0", "breaks1", "g0", "g1")
    args = dict(zip(keys, grid_args))
    args["ndep"] = points.shape[0]
    args.update(points=points.ctypes.data, npts=N, part_d2=d2.ctypes.data, part_idx=idx.ctypes.data, nchunks=1, guess=None,
                uvw=out["uvw"].ctypes.data, distance=out["distance"].ctypes.data, status=out["status"].ctypes.data,
                steps=out["steps"].ctypes.data)
    return args, out, (rows, grid, points, tabs, d2, idx, plan)


def test_abi_argument_checks():
    L = nv.lib()
    case = load_case("surface_k33_planar")
    args, out, keep = newton_args(case)
    rows, grid, points, tabs, d2, idx, plan = keep
    N, M = points.shape[1], plan.nsamples
    assert L.bsk_project_newton_host(*args.values()) == nv.BSK_OK and L.bsk_project_last_kernel() == b"host project_newton"
    want = project.project_batch(make_spline(case), points, _path="host")
    assert out["uvw"].tobytes() == want[0].tobytes() and out["status"].tobytes() == want[2].tobytes()

    seed = dict(ndep=2, samples=grid.ctypes.data, nsamples=M, points=points.ctypes.data, npts=N, chunk=4, part_d2=d2.ctypes.data,
                part_idx=idx.ctypes.data)
    for entry, tail in ((L.bsk_project_seed_host, ()), (L.bsk_project_seed, (None,))):       # checked before the device is touched
        for key in ("samples", "points", "part_d2", "part_idx"):
            assert entry(*dict(seed, **{key: None}).values(), *tail) == nv.BSK_ERR_INVALID
        for key in ("nsamples", "npts", "chunk"):
            assert entry(*dict(seed, **{key: 0}).values(), *tail) == nv.BSK_ERR_INVALID
        assert entry(*dict(seed, nsamples=2 ** 31).values(), *tail) == nv.BSK_ERR_INVALID
        assert entry(*dict(seed, nsamples=2 ** 20, chunk=8).values(), *tail) == nv.BSK_ERR_INVALID          # more than 65535 chunks
        for ndep in (1, 4):
            assert entry(*dict(seed, ndep=ndep).values(), *tail) == nv.BSK_ERR_UNSUPPORTED
            assert b"ndep must be 2 or 3" in L.bsk_last_error()

    for entry, tail in ((L.bsk_project_newton_host, ()), (L.bsk_project_newton, (None,))):
        for key in ("rows", "first0", "first1", "breaks0", "breaks1", "points", "part_d2", "part_idx", "uvw", "distance", "status", "steps"):
            assert entry(*dict(args, **{key: None}).values(), *tail) == nv.BSK_ERR_INVALID, key
        for key in ("npts", "nc0", "nc1", "nchunks", "g0", "g1", "R0", "R1"):
            assert entry(*dict(args, **{key: 0}).values(), *tail) == nv.BSK_ERR_INVALID, key
        assert entry(*dict(args, g0=9).values(), *tail) == nv.BSK_ERR_INVALID
        assert entry(*dict(args, K0=1).values(), *tail) == nv.BSK_ERR_INVALID
        assert entry(*dict(args, nind=1).values(), *tail) == nv.BSK_ERR_INVALID                  # a curve has K1 = R1 = nc1 = g1 = 1
        for change in (dict(nind=3), dict(nind=0), dict(ndep=1), dict(ndep=4), dict(K0=5), dict(K1=5),
                       dict(nind=1, K0=7, K1=1, R1=1, nc1=1, g1=1)):
            assert entry(*dict(args, **change).values(), *tail) == nv.BSK_ERR_UNSUPPORTED, change

    # a window that leaves the rows, a seed index that is no sample: flagged points, no read out of bounds
    first0 = tabs[0].copy()
    first0[-1] = rows.shape[1]
    assert L.bsk_project_newton_host(*dict(args, first0=first0.ctypes.data).values()) == nv.BSK_OK
    flagged = (out["status"] & project.STATUS_SINGULAR) != 0              # the points whose walk met the last row of cells
    assert flagged.any() and not flagged.all() and (want[0][0][flagged] >= float(tabs[2][-2]) - 0.5).all()
    assert np.array_equal(out["status"][~flagged], want[2][~flagged]) and out["uvw"][:, ~flagged].tobytes() == want[0][:, ~flagged].tobytes()
    bad = idx.copy()
    bad[0, 0], bad[0, 1] = M, -1
    assert L.bsk_project_newton_host(*dict(args, part_idx=bad.ctypes.data).values()) == nv.BSK_OK
    assert out["status"][:2].tolist() == [project.STATUS_SKIPPED] * 2 and np.isnan(out["uvw"][:, :2]).all()
    assert out["status"][2:].tobytes() == want[2][2:].tobytes()


def test_library_exports_the_declared_family():
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bspy_amd.h")).read()
    declared = set(re.findall(r"\b(bsk_project_[a-z_]+)\s*\((?:void|int )", header))
    assert declared == set(FAMILY) and declared <= set(nv.PRODUCT_SYMBOLS)
    assert {s for s in nv.SYMBOLS if s.startswith("bsk_project")} == declared
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(nv.LIB_PATH), "bsk_project.hpp")).read()

    def constant(name):
        return re.search(rf"constexpr \w+ {name} = ([^;]+);", text).group(1)

    assert int(constant("PROJECT_EVALS")) == project.EVALS and int(constant("PROJECT_HALVINGS")) == project.HALVINGS
    assert float.fromhex(constant("PROJECT_TRUST")) == project.TRUST and float.fromhex(constant("PROJECT_SMALL_STEP")) == project.SMALL_STEP
    assert int(constant("PROJECT_MAX_SAMPLES")) == project.MAX_SAMPLES
    assert 2.0 ** -project.HALVINGS <= project.TRUST                      # a clamped step halved HALVINGS times is a small one
