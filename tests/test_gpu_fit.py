"""
Spline.least_squares on the GPU: every golden case (tests/golden/least_squares.npz) through the forced device path,
device against host path, data layouts, reproducibility, and one large property test.  (Stale LDS: the fills live in
tests/test_gpu_stale_lds_fit.py, which sorts behind every other GPU test file, so that no other test runs on poisoned LDS.)

Bars (relative to max |coef|): 1e-10 for cases with recorded kappa <= 1e3, otherwise 10 x the recorded ref_spread
(see tests/test_fit_host.py).  ``fitting.LAST_PATHS`` / ``Plan.last_kernel`` name the path every solve took and are
asserted, so that a host solve cannot pass as a GPU result.
"""
import numpy as np
import pytest

import fit_ref
from bspy_amd import Spline, collocation_matrix, fitting
from conftest import observe
from test_fit_host import PLAIN, bar_of, golden, load_case  # noqa: F401  (golden is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _fit(c, **kw):
    u = c["u"] if len(c["u"]) > 1 else c["u"][0]
    return Spline.least_squares(u, kw.pop("data", c["data"]), c["order"], c["knots_in"], c["compression"], c["tolerance"],
                                c["fixEnds"], **kw)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _device_paths():
    assert fitting.LAST_PATHS and all(p in ("fit_sweep", "fit_sweep turned") for p in fitting.LAST_PATHS), fitting.LAST_PATHS


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", PLAIN)
def test_golden_device_path(golden, name):
    c = load_case(golden, name)
    s = _fit(c, _path="device")
    _device_paths()
    assert s.coefs.dtype == np.float64 and all(k.dtype == np.float64 for k in s.knots)
    assert s.order == tuple(c["order"]) and s.coefs.shape == c["coefs"].shape
    for a, b in zip(s.knots, c["knots"]):
        assert np.array_equal(a, b), f"{name}: knots differ from the reference's"
    observe(f"fit device vs reference, {name}", _rel(s.coefs, c["coefs"]), bar_of(c))
    if len(c["u"]) > 1:
        assert "fit_sweep turned" in fitting.LAST_PATHS and "fit_sweep" in fitting.LAST_PATHS
    if c["tolerance"] is not None:
        # independent check: the criterion holds for the returned spline, residual rows recomputed in NumPy
        b = np.asarray(c["data"], np.float64)
        limit = c["tolerance"] / len(c["u"])
        cur = b
        for iv, (u, o) in enumerate(zip(c["u"], c["order"])):
            A = fit_ref.dense_matrix(s.knots[iv], o, u)
            lines = np.moveaxis(cur, iv + 1, 0)
            x = fit_ref.qr_solve(A, lines.reshape(len(u), -1))
            norms = np.sqrt(np.sum((lines.reshape(len(u), -1) - A @ x) ** 2, axis=1))
            assert norms.max() <= limit
            cur = np.moveaxis(x.reshape((A.shape[1],) + lines.shape[1:]), 0, iv + 1)


@pytest.mark.parametrize("name", PLAIN)
def test_device_path_against_host_path(golden, name):
    c = load_case(golden, name)
    dev = _fit(c, _path="device")
    _device_paths()
    host = _fit(c, _path="host")
    assert fitting.LAST_PATHS and all(p == "host plan" for p in fitting.LAST_PATHS), fitting.LAST_PATHS
    for a, b in zip(dev.knots, host.knots):
        assert np.array_equal(a, b)
    observe(f"fit device vs host plan, {name}", _rel(dev.coefs, host.coefs), bar_of(c))


@pytest.mark.parametrize("name", ["fixends_curve", "fixends_surface", "deficient"])
def test_golden_fallback(golden, name):
    c = load_case(golden, name)
    s = _fit(c)
    assert "fallback" in fitting.LAST_PATHS
    if c["fixEnds"]:
        assert all(p == "fallback" for p in fitting.LAST_PATHS)
    observe(f"fit fallback vs reference, {name}", _rel(s.coefs, c["coefs"]), bar_of(c))


def test_default_dispatch(golden):
    """A curve (3 lines) takes the host plan, a surface with enough lines in both variables the kernel."""
    _fit(load_case(golden, "curve2000"))
    assert fitting.LAST_PATHS == ["host plan"]
    n = 2 * fitting.DEVICE_MIN_LINES + 8
    u = np.linspace(0.0, 1.0, n)
    s = Spline.least_squares([u, u], _franke(u[:, None], u[None, :])[None], compression=0.4)
    assert fitting.LAST_PATHS == ["fit_sweep", "fit_sweep turned"]
    assert min(s.nCoef) >= fitting.DEVICE_MIN_LINES


# ------------------------------------------------------------------------------------------ layouts
def _system(order, nrows, ncols, seed):
    rng = np.random.default_rng(seed)
    u = np.sort(rng.random(nrows))
    u[0], u[-1] = 0.0, 1.0
    interior = fit_ref.auto_knots(u, order, 0.0)[order:-order][1::3]       # at least two parameter values per span
    keep = np.sort(rng.choice(len(interior), ncols - order, replace=False)) if ncols > order else []
    knots = np.concatenate((np.zeros(order), interior[keep], np.ones(order)))
    first, values = collocation_matrix(knots, order, u, dense=False)
    return fitting.Plan(first, values, ncols), first, np.asarray(values, np.float64)


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("outer,inner", [(1, 1), (63, 1), (64, 1), (65, 1), (1000, 1), (1, 200), (3, 37), (2, 64), (1, 4133), (5, 1031)])
def test_layouts_against_host_plan(order, outer, inner):
    nrows, ncols = 91, 23
    plan, first, values = _system(order, nrows, ncols, 100 + order)
    rng = np.random.default_rng(outer * 7 + inner)
    b = rng.standard_normal((outer, nrows, inner))
    want = plan.solve_host(b, outer, inner)
    tb = torch.as_tensor(b, device="cuda")
    x = plan.sweep(tb, outer, inner)
    assert plan.last_kernel() == ("fit_sweep turned" if inner == 1 and outer > 1 else "fit_sweep")
    got = x.cpu().numpy()
    observe(f"fit_sweep vs host plan, order {order}", _rel(got, want), 1e-10)
    rows = plan.residual_rows(tb, x, outer, inner)
    assert plan.last_kernel() == ("fit_residual turned" if inner == 1 and outer > 1 else "fit_residual")
    want_rows = fitting.residual_rows_host(first, values, b, got)
    observe("fit_residual vs NumPy", np.abs(rows - want_rows).max() / want_rows.max(), 1e-10)
    # float32 right-hand sides: read as float32, computed in float64
    b32 = b.astype(np.float32)
    x32 = plan.sweep(torch.as_tensor(b32, device="cuda"), outer, inner).cpu().numpy()
    observe(f"fit_sweep fp32 input vs host plan, order {order}", _rel(x32, plan.solve_host(b32, outer, inner)), 1e-10)


def test_order_above_eight_takes_the_host_plan():
    u = np.linspace(0.0, 1.0, 40)
    data = np.stack([np.sin(3 * u)[:, None] * np.cos(u)[None, :]])
    s = Spline.least_squares([u, u], data, order=[9, 4], compression=0.5)
    assert fitting.LAST_PATHS[0] == "host plan"
    knots, coefs = fit_ref.fit([u, u], data, [9, 4], compression=0.5)
    observe("fit order 9 (host plan) vs NumPy", _rel(s.coefs, coefs), 1e-10)
    with pytest.raises(ValueError, match="orders up to 8"):
        Spline.least_squares([u, u], data, order=[9, 4], compression=0.5, _path="device")


@pytest.mark.parametrize("order", [2, 4, 6])
def test_bezier(order):
    """nRows = nCols = order: one Bezier segment through `order` points (a square system)."""
    u = np.linspace(0.0, 1.0, order) ** 1.5
    data = np.stack([np.cos(2 * u), u ** 2, 1.0 + u])
    s = Spline.least_squares(u, data, order=[order], _path="device")
    _device_paths()
    assert s.nCoef == (order,)
    want = np.linalg.solve(fit_ref.dense_matrix(s.knots[0], order, u), data.T).T
    observe("fit Bezier (square system) vs numpy solve", _rel(s.coefs, want), 1e-10)
    x, y, z = s(u)
    observe("fit Bezier interpolates", np.abs(np.stack([x, y, z]) - data).max(), 1e-12)


# ------------------------------------------------------------------------------------------ reproducibility
def test_torch_input_and_repeat_runs_give_the_same_bits(golden):
    for name in ("surface_o65", "float32", "volume", "tolerance_jittered"):
        c = load_case(golden, name)
        first = _fit(c, _path="device")
        again = _fit(c, _path="device")
        t = torch.as_tensor(c["data"], device="cuda")
        before = t.clone()
        resident = _fit(c, data=t, _path="device")
        _device_paths()
        assert torch.equal(t, before)
        for s in (again, resident):
            assert s.coefs.tobytes() == first.coefs.tobytes(), name
            assert all(np.array_equal(a, b) for a, b in zip(s.knots, first.knots))


# ------------------------------------------------------------------------------------------ large property test
def _franke(x, y):
    return (0.75 * np.exp(-((9 * x - 2) ** 2 + (9 * y - 2) ** 2) / 4) + 0.75 * np.exp(-((9 * x + 1) ** 2) / 49 - (9 * y + 1) / 10)
            + 0.5 * np.exp(-((9 * x - 7) ** 2 + (9 * y - 3) ** 2) / 4) - 0.2 * np.exp(-((9 * x - 4) ** 2 + (9 * y - 7) ** 2)))


def test_large_surface_normal_equations_and_noise():
    """2048 x 2048 x 3 Franke plus noise, compression 0.75, no reference needed.  Per variable, on 4096 random lines (all, where there are fewer):
    |A^T (b - A x)|_2 <= 1e-10 |A|_2 |b|_2 (x minimises |A x - b| exactly when A^T r = 0).  The fitted surface
    reproduces a noise-free 64 x 64 sub-grid within the noise: a least-squares fit cannot amplify the noise (its
    projector has norm 1) and here averages about 16 samples per coefficient, so the RMS error stays under sigma and,
    being close to Gaussian over 12288 values, the largest under 5 sigma; the Franke function itself is resolved by
    515 x 515 cubic coefficients to far below sigma."""
    n, sigma = 2048, 0.01
    rng = np.random.default_rng(2048)
    u = np.linspace(0.0, 1.0, n)
    clean = np.stack([_franke(u[:, None], u[None, :]), 2.0 * _franke(u[None, :], u[:, None]), 1.0 - _franke(u[:, None], u[None, :])])
    data = clean + sigma * rng.standard_normal(clean.shape)
    td = torch.as_tensor(data, device="cuda")
    s = Spline.least_squares([u, u], td, compression=0.75, _path="device")
    assert fitting.LAST_PATHS == ["fit_sweep", "fit_sweep turned"]
    assert s.nCoef == (515, 515)
    cur, shape = td, [3, n, n]
    for iv in range(2):
        first, values = collocation_matrix(s.knots[iv], 4, u, dense=False)
        plan = fitting.Plan(first, values, 515)
        outer, inner = int(np.prod(shape[:iv + 1])), int(np.prod(shape[iv + 2:]))
        x = plan.sweep(cur, outer, inner)
        b = cur.reshape(outer, n, inner).cpu().numpy()
        xh = x.cpu().numpy()
        A = fitting.dense_matrix(first, np.asarray(values, np.float64), 515)
        pick = rng.choice(outer * inner, min(4096, outer * inner), replace=False)    # variable 1 has 1545 lines: all of them
        bl, xl = b[pick // inner, :, pick % inner], xh[pick // inner, :, pick % inner]        # (lines, n), (lines, 515)
        grad = (bl - xl @ A.T) @ A
        ratio = np.linalg.norm(grad, axis=1) / (np.linalg.norm(A, 2) * np.linalg.norm(bl, axis=1))
        observe(f"fit 2048^2 x 3: |A^T r| / (|A| |b|), variable {iv}", ratio.max(), 1e-10)
        cur, shape[iv + 1] = x, 515
    assert cur.cpu().numpy().reshape(3, 515, 515).tobytes() == s.coefs.tobytes()
    pick = np.sort(rng.choice(n, 64, replace=False))
    got = np.stack(s(u[pick][:, None], u[pick][None, :]))
    err = got - clean[:, pick][:, :, pick]
    observe("fit 2048^2 x 3: RMS error on a noise-free sub-grid / sigma", np.sqrt(np.mean(err ** 2)) / sigma, 1.0)
    observe("fit 2048^2 x 3: largest error on a noise-free sub-grid / sigma", np.abs(err).max() / sigma, 5.0)
