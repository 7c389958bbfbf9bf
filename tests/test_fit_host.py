"""
Spline.least_squares without a GPU: argument checks, the knot rule, derivative rows, and the host half of the solver
(the banded Givens plan of libbspy_amd.so through ctypes, which makes no HIP call) against NumPy and against the
reference's results in tests/golden/least_squares.npz (written by tests/golden/make_golden_fit.py).  The collocation
matrices come from tests/fit_ref.py here; the library's own (a GPU call) are covered by tests/test_gpu_fit.py.

Bars (relative to max |coef|): 1e-10, the project's contract, for cases whose recorded kappa (product of cond_2(A)
over the variables) is <= 1e3; otherwise 10 x the recorded ref_spread (the distance between the reference's
SVD-based lstsq and a Householder QR of the same systems).
"""
import os

import numpy as np
import pytest

import fit_ref
import bspy_amd
from bspy_amd import Spline, fitting
from bspy_amd.collocation import derivative_orders
from conftest import GOLDEN, observe


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "least_squares.npz"))


def case_names(g):
    return sorted({k.split("/")[0] for k in g.files})


def load_case(g, name):
    order = [int(o) for o in g[f"{name}/order"]]
    n = len(order)
    compression, tolerance, fix = g[f"{name}/args"]
    return dict(u=[g[f"{name}/u{i}"] for i in range(n)], data=g[f"{name}/data"], order=order,
                knots_in=[g[f"{name}/knots_in{i}"] for i in range(n)] if f"{name}/knots_in0" in g.files else None,
                compression=float(compression), tolerance=None if np.isnan(tolerance) else float(tolerance),
                fixEnds=bool(fix), knots=[g[f"{name}/knots{i}"] for i in range(n)], coefs=g[f"{name}/coefs"],
                kappa=float(g[f"{name}/kappa"]), ref_spread=float(g[f"{name}/ref_spread"]))


def bar_of(case):
    return 1e-10 if case["kappa"] <= 1e3 else 10.0 * case["ref_spread"]


PLAIN = ["curve2000", "surface_o43", "surface_o65", "interpolation", "hermite", "knots_curve", "knots_surface", "volume",
         "float32", "tolerance_franke", "tolerance_jittered"]


# ------------------------------------------------------------------------------------------ arguments
def test_argument_errors_in_reference_order():
    u = np.linspace(0.0, 1.0, 10)
    good = np.zeros((2, 10))
    with pytest.raises(ValueError, match="Independent variable values are out of order"):
        Spline.least_squares(u[::-1], np.zeros((2, 10, 3)))           # the first check wins over the shape
    with pytest.raises(ValueError, match="dataPoints has the wrong shape"):
        Spline.least_squares(u, np.zeros((2, 10, 3)))
    with pytest.raises(ValueError, match="Wrong number of parameter values in one or more directions"):
        Spline.least_squares(u, np.zeros((2, 9)))
    with pytest.raises(ValueError, match="Not enough points in one or more directions"):
        Spline.least_squares(u, good, order=[11], compression=2.0)    # before the compression check
    with pytest.raises(ValueError, match="compression not between 0.0 and 1.0"):
        Spline.least_squares(u, good, compression=1.5)
    with pytest.raises(ValueError, match="compression not between 0.0 and 1.0"):
        Spline.least_squares(u, good, compression=-0.1)
    with pytest.raises(ValueError, match="One or more dataPoints are outside the domain of the spline"):
        Spline.least_squares(u, good, order=[3], knots=[[0.1, 0.1, 0.1, 0.5, 1, 1, 1]])
    with pytest.raises(ValueError, match="One or more dataPoints are outside the domain of the spline"):
        Spline.least_squares([u, u], np.zeros((1, 10, 10)), order=[3, 3], knots=[[0, 0, 0, 0.5, 1, 1, 1], [0, 0, 0, 0.5, 0.9, 0.9, 0.9]])
    with pytest.raises(ValueError, match="_path"):
        Spline.least_squares(u, good, _path="gpu")


def test_spline_valued_data_is_not_implemented():
    s = Spline(1, 1, (2,), (2,), [[0.0, 0, 1, 1]], [[0.0, 1.0]])
    with pytest.raises(NotImplementedError, match="Spline-valued"):
        Spline.least_squares([0.0, 0.5, 1.0], [s, s, s])


def test_exported():
    assert bspy_amd.least_squares is fitting.least_squares
    assert Spline.least_squares.__doc__ and "fixEnds" in Spline.least_squares.__doc__


# ------------------------------------------------------------------------------------------ knots, derivative rows
def test_knot_rule_bitwise(golden):
    seen = 0
    for name in case_names(golden):
        c = load_case(golden, name)
        if c["knots_in"] is not None or c["tolerance"] is not None:
            continue
        for u, o, k in zip(c["u"], c["order"], c["knots"]):
            assert np.array_equal(fitting.auto_knots(u, o, c["compression"]), k), name
            seen += 1
    assert seen >= 12
    u = np.sort(np.random.default_rng(3).random(57))
    for compression in (0.0, 0.3, 0.9, 1.0):
        assert np.array_equal(fitting.auto_knots(u, 4, compression), fit_ref.auto_knots(u, 4, compression))
    assert len(fitting.auto_knots(u, 4, 1.0)) == 8 and len(fitting.auto_knots(u, 4, 0.0)) == 57 + 4


def test_derivative_rows(golden):
    u = golden["hermite/u0"]
    d = derivative_orders(u)
    assert np.array_equal(d, fit_ref.derivative_orders(u))
    assert d.max() == 2 and (d == 1).sum() == 5 and (d == 2).sum() == 2 and d[0] == 0 and d[1] == 1


# ------------------------------------------------------------------------------------------ the plan
def _plan(knots, order, u):
    first, values = fit_ref.banded_matrix(knots, order, u)
    return fitting.Plan(first, values, len(knots) - order), first, values


@pytest.mark.parametrize("name", ["curve2000", "surface_o65", "interpolation", "hermite", "knots_surface"])
def test_plan_r_against_numpy_qr(golden, name):
    c = load_case(golden, name)
    for iv, (u, o, k) in enumerate(zip(c["u"], c["order"], c["knots"])):
        plan, first, values = _plan(k, o, u)
        ncols = len(k) - o
        band = plan.r_band()
        R = np.zeros((ncols, ncols))
        for t in range(o):
            R[np.arange(ncols - t), np.arange(ncols - t) + t] = band[:ncols - t, t]
        assert np.all(band[:, 0] > 0.0)
        for t in range(1, o):                                       # nothing stored past the last column
            assert np.all(band[ncols - t:, t] == 0.0)
        Rn = np.linalg.qr(fit_ref.dense_matrix(k, o, u), mode="r")
        Rn *= np.sign(np.diag(Rn))[:, None]
        observe(f"fit plan: R vs numpy.linalg.qr, {name} variable {iv}", np.abs(R - Rn).max() / np.abs(Rn).max(), 1e-12)
        assert plan.rank_indicator() == pytest.approx(np.abs(np.diag(Rn)).min() / np.abs(np.diag(Rn)).max(), rel=1e-9)
        assert not plan.deficient()


def _host_fit(c):
    """The per-variable driver with fit_ref matrices and the host plan; knots as the golden has them."""
    data = c["data"]
    for iv, (u, o, k) in enumerate(zip(c["u"], c["order"], c["knots"])):
        plan, first, values = _plan(k, o, u)
        outer = int(np.prod(data.shape[:iv + 1]))
        inner = int(np.prod(data.shape[iv + 2:]))
        x = plan.solve_host(data, outer, inner)
        assert plan.last_kernel() == "host plan"
        data = x.reshape(data.shape[:iv + 1] + (len(k) - o,) + data.shape[iv + 2:])
    return data


@pytest.mark.parametrize("name", PLAIN)
def test_host_solve_against_golden(golden, name):
    c = load_case(golden, name)
    got = _host_fit(c)
    assert got.shape == c["coefs"].shape
    observe(f"fit host plan vs reference, {name}", np.abs(got - c["coefs"]).max() / np.abs(c["coefs"]).max(), bar_of(c))


def test_host_solve_against_lstsq_and_residual(golden):
    c = load_case(golden, "surface_o65")
    u, o, k = c["u"][0], c["order"][0], c["knots"][0]
    plan, first, values = _plan(k, o, u)
    b = c["data"]                                                    # (1, 200, 150): outer 1, inner 150
    x = plan.solve_host(b, 1, b.shape[2])
    A = fit_ref.dense_matrix(k, o, u)
    want, _, _, _ = np.linalg.lstsq(A, b[0], rcond=None)
    observe("fit host plan vs numpy lstsq, one variable", np.abs(x[0] - want).max() / np.abs(want).max(), 1e-12)
    rows = fitting.residual_rows_host(first, values, b, x)
    want_rows = np.sum((b[0] - A @ want) ** 2, axis=1)
    observe("fit residual rows (host) vs numpy", np.abs(rows - want_rows).max() / want_rows.max(), 1e-10)
    # float32 right-hand sides are read as float32 and computed in float64
    x32 = plan.solve_host(b.astype(np.float32), 1, b.shape[2])
    assert np.array_equal(x32, plan.solve_host(b.astype(np.float32).astype(np.float64), 1, b.shape[2]))


def test_plan_rejects_bad_bands():
    vals = np.ones((3, 2))
    for first, ncols in (([0, 2, 1], 4), ([0, 1, 3], 4), ([-1, 0, 1], 4), ([0, 0, 0], 1)):
        with pytest.raises(bspy_amd._native.BskError):
            fitting.Plan(np.array(first, np.int32), vals, ncols)
    with pytest.raises(bspy_amd._native.BskError):
        fitting.Plan(np.array([0, 1, 2], np.int32), np.array([[1, 1], [np.nan, 1], [1, 1.0]]), 4)


# ------------------------------------------------------------------------------------------ rank deficiency, fixEnds
def test_rank_indicator_and_minimum_norm_fallback(golden):
    c = load_case(golden, "deficient")
    u, o, k = c["u"][0], c["order"][0], c["knots"][0]
    plan, first, values = _plan(k, o, u)
    assert plan.deficient() and plan.rank_indicator() < 1e-14
    with pytest.raises(bspy_amd._native.BskError, match="singular"):
        plan.solve_host(c["data"], 2, 1)
    A = fitting.dense_matrix(first, values, len(k) - o)
    assert np.array_equal(A, fit_ref.dense_matrix(k, o, u))
    x, resid = fitting.fallback_solve(A, c["data"].T)
    observe("fit fallback (minimum norm) vs reference", np.abs(x.T - c["coefs"]).max() / np.abs(c["coefs"]).max(), bar_of(c))
    assert np.allclose(resid, c["data"].T - A @ x)


@pytest.mark.parametrize("name", ["fixends_curve", "fixends_surface"])
def test_fix_ends_fallback_against_golden(golden, name):
    c = load_case(golden, name)
    data = c["data"]
    for iv, (u, o, k) in enumerate(zip(c["u"], c["order"], c["knots"])):
        A = fit_ref.dense_matrix(k, o, u)
        fixed = [r for r in range(len(u)) if u[r] == u[0] or u[r] == u[-1]]
        b = np.moveaxis(data, iv + 1, 0)
        x, _ = fitting.fallback_solve(A, b.reshape(len(u), -1), fixed)
        assert np.abs(A[fixed] @ x - b.reshape(len(u), -1)[fixed]).max() <= 1e-12
        data = np.moveaxis(x.reshape((A.shape[1],) + b.shape[1:]), 0, iv + 1)
    observe(f"fit fallback (fixEnds) vs reference, {name}", np.abs(data - c["coefs"]).max() / np.abs(c["coefs"]).max(), bar_of(c))


# ------------------------------------------------------------------------------------------ the NumPy statement itself
@pytest.mark.parametrize("name", ["tolerance_franke", "tolerance_jittered"])
def test_restated_tolerance_loop_finds_the_reference_knots(golden, name):
    c = load_case(golden, name)
    knots, coefs = fit_ref.fit(c["u"], c["data"], c["order"], tolerance=c["tolerance"])
    for a, b in zip(knots, c["knots"]):
        assert np.array_equal(a, b)
    observe(f"fit_ref vs reference, {name}", np.abs(coefs - c["coefs"]).max() / np.abs(c["coefs"]).max(), bar_of(c))
