"""
Grid and tessellation axes in any order.

Nothing in the C ABI or the Python API asks for sorted grid axes, so a grid point's result must depend only on the
spline and its parameters: shuffled, descending and constant axes, a period-4 pattern that sends the columns of one
lane to different spans, and every knot +- 1 ulp in random order, on patches with several spans in both variables.
Every grid kernel (grid_rows with vector and scalar stores, grid_surface, grid_generic) and every form of tess_rows
(hoisted at 512 and 256 lanes, with normals, mixed orders) against the oracle on the mesh of the same axes and against
the flat evaluation of the same points; last_kernel() names the form each case ran.
"""
import numpy as np
import pytest

import cases
import oracle
import bspy_amd
from bspy_amd import DeviceSpline, Spline
from conftest import observe

pytestmark = pytest.mark.gpu

KINDS = ["shuffled", "descending", "repeated", "period4", "knots"]


def _tol(dt):
    return 2e-5 if dt == np.float32 else 1e-12


def _kind(dt):
    return "fp32" if dt == np.float32 else "fp64"


def _scale(ref):
    return max(1.0, float(np.max(np.abs(ref))))


def _axis(kind, knots, order, ncoef, n, dt, rng):
    lo, hi = dt(knots[order - 1]), dt(knots[ncoef])
    if kind == "shuffled":
        a = rng.permutation(np.linspace(lo, hi, n))
    elif kind == "descending":
        a = np.linspace(hi, lo, n)
    elif kind == "repeated":
        a = np.full(n, lo + 0.37 * (hi - lo))
    elif kind == "period4":                                     # columns 0 and 3 of a lane in one span, 1 and 2 elsewhere
        a = lo + (hi - lo) * np.resize(np.array((0.1, 0.8, 0.7, 0.1)), n)
    else:                                                       # every knot and +- 1 ulp, both ends, random order
        d = np.unique(np.asarray(knots, dt))
        e = np.concatenate((d, np.nextafter(d, dt(-np.inf)), np.nextafter(d, dt(np.inf)), [lo, hi])).astype(dt)
        e = np.unique(e[(e >= lo) & (e <= hi)])
        assert len(e) <= n
        a = rng.permutation(np.concatenate((e, lo + (hi - lo) * rng.random(n - len(e)))))
    return np.clip(np.asarray(a, dt), lo, hi).astype(dt)


def _spline(order, ncoef, ndep, dt, seed):
    rng = np.random.default_rng(seed)
    knots = [cases.nonuniform_knots(rng, o, c, dt, 0.0, 1.0) for o, c in zip(order, ncoef)]
    return knots, rng.standard_normal((ndep, *ncoef)).astype(dt)


def _mesh(axes):
    return [m.ravel() for m in np.meshgrid(*axes, indexing="ij")]


def _check_grid(t, order, ncoef, knots, coefs, dt, axes, w, label):
    """The grid against the oracle on its mesh and against the flat evaluation; returns the grid kernel that ran."""
    g = t.evaluate_grid(axes, w)
    kernel = t.last_kernel()
    ref, bad = oracle.c_evaluate(order, ncoef, knots, coefs, list(w), _mesh(axes))
    assert bad == -1
    ref = ref.reshape(g.shape)
    observe(f"grid axes: {kernel} vs oracle, {_kind(dt)}", np.abs(g - ref).max() / _scale(ref), _tol(dt))
    flat = t.evaluate(_mesh(axes), list(w)).reshape(g.shape)
    assert np.abs(g - flat).max() <= _tol(dt) * _scale(flat), label
    return kernel


# ------------------------------------------------------------------------------------------ bsk_evaluate_grid
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("form,order,n1", [("grid_rows", (4, 4), 128), ("grid_rows", (4, 4), 77), ("grid_rows", (3, 5), 96),
                                           ("grid_surface", (4, 4), 40), ("grid_generic", (7, 3), 96)])
def test_grid_any_axis_order(form, order, n1, dt, kind):
    """n1 % VEC == 0: grid_rows' vector stores; n1 odd: its scalar stores; mixed orders; n1 < 64: grid_surface; order 7:
    grid_generic."""
    ncoef = (11, 9) if order[0] < 7 else (12, 9)
    knots, coefs = _spline(order, ncoef, 3, dt, 31)
    rng = np.random.default_rng(32)
    axes = [_axis(kind, knots[0], order[0], ncoef[0], 36, dt, rng), _axis(kind, knots[1], order[1], ncoef[1], n1, dt, rng)]
    t = DeviceSpline(order, ncoef, knots, coefs, dt)
    for w in ([0, 0], [1, 1]):
        kernel = _check_grid(t, order, ncoef, knots, coefs, dt, axes, w, (form, kind, w))
        assert kernel == form, (kernel, form)


@pytest.mark.parametrize("kind", KINDS)
def test_grid_generic_volume_any_axis_order(kind):
    c = {x.name: x for x in cases.parity_cases()}["volume_o3x4x2"]
    rng = np.random.default_rng(33)
    axes = [_axis(kind, k, o, nc, m, np.float64, rng) for k, o, nc, m in zip(c.knots, c.order, c.nCoef, (16, 20, 16))]
    t = DeviceSpline(c.order, c.nCoef, c.knots, c.coefs)
    assert _check_grid(t, c.order, c.nCoef, c.knots, c.coefs, np.float64, axes, [0, 1, 1], kind) == "grid_generic"


@pytest.mark.parametrize("kind", KINDS)
def test_spline_broadcast_any_axis_order(kind):
    """The Spline broadcast form u[:, None], v[None, :] takes the grid path (> 4096 points)."""
    order, ncoef = (4, 4), (11, 9)
    knots, coefs = _spline(order, ncoef, 3, np.float64, 34)
    s = Spline(2, 3, order, ncoef, knots, coefs)
    rng = np.random.default_rng(35)
    u = _axis(kind, knots[0], 4, ncoef[0], 72, np.float64, rng)
    v = _axis(kind, knots[1], 4, ncoef[1], 96, np.float64, rng)
    for w in ([0, 0], [1, 2]):
        g = np.stack(s.derivative(w, u[:, None], v[None, :]))
        assert s.device_tables().last_kernel() == "grid_rows", s.device_tables().last_kernel()
        ref, bad = oracle.c_evaluate(order, ncoef, knots, coefs, w, _mesh([u, v]))
        assert bad == -1
        ref = ref.reshape(g.shape)
        observe("grid axes: Spline broadcast vs oracle, fp64", np.abs(g - ref).max() / _scale(ref), 1e-12)
        uu, vv = _mesh([u, v])
        flat = np.stack(s.derivative(w, uu, vv)).reshape(g.shape)
        assert np.abs(g - flat).max() <= 1e-12 * _scale(flat)


def test_grid_first_offender_on_a_shuffled_axis():
    """The out-of-domain index of a grid is the first offender in flat (row-major) order, whatever the axis order."""
    order, ncoef = (4, 4), (11, 9)
    knots, coefs = _spline(order, ncoef, 3, np.float64, 36)
    rng = np.random.default_rng(37)
    u = _axis("shuffled", knots[0], 4, ncoef[0], 36, np.float64, rng)
    v = _axis("shuffled", knots[1], 4, ncoef[1], 128, np.float64, rng)
    t = DeviceSpline(order, ncoef, knots, coefs)
    u2, v2 = u.copy(), v.copy()
    u2[[29, 7]] = (1.5, -0.5)                                   # rows 7 and 29 out: the first offender is (7, 0)
    with pytest.raises(bspy_amd.DomainError) as e:
        t.evaluate_grid([u2, v])
    assert e.value.index == 7 * 128
    v2[[100, 45]] = (-1.0, 2.0)                                 # and columns 45, 100: now (0, 45)
    with pytest.raises(bspy_amd.DomainError) as e:
        t.evaluate_grid([u2, v2])
    assert e.value.index == 45
    patches = [DeviceSpline(order, ncoef, knots, coefs)]
    with pytest.raises(bspy_amd.DomainError) as e:
        bspy_amd.tessellate_tables(patches, (u2, v))
    assert e.value.index == 7 * 128
    with pytest.raises(bspy_amd.DomainError) as e:
        bspy_amd.tessellate_tables(patches, (u, v2), normals=False)
    assert e.value.index == 45


# ------------------------------------------------------------------------------------------ bsk_tessellate
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["hoisted 512", "hoisted 256", "normals", "mixed", "columns"])
def test_tessellate_any_axis_order(form, dt, kind, monkeypatch):
    """Positions (and area / unit normals) of three patches with several spans in both variables, on axes of every
    kind, against the oracle on the mesh and against the flat evaluation of each patch."""
    order = (3, 4) if form == "mixed" else (4, 4)
    ncoef = (9, 8)
    rng = np.random.default_rng(40)
    knots = [cases.nonuniform_knots(rng, o, c, dt, 0.0, 1.0) for o, c in zip(order, ncoef)]
    patches = [rng.standard_normal((3, *ncoef)).astype(dt) for _ in range(3)]
    tabs = [DeviceSpline(order, ncoef, knots, cf, dt) for cf in patches]
    u = _axis(kind, knots[0], order[0], ncoef[0], 32, dt, rng)
    v = _axis(kind, knots[1], order[1], ncoef[1], 127 if form == "columns" else 128, dt, rng)
    if form == "hoisted 256":
        monkeypatch.setenv("BSK_TESS_T", "256")
    normals = form in ("normals", "mixed")
    out = bspy_amd.tessellate_tables(tabs, (u, v), normals=normals, normalize=False)
    assert tabs[0].last_kernel() == f"tess_rows {form}", tabs[0].last_kernel()
    pos, nrm = out if normals else (out, None)
    uu, vv = _mesh([u, v])
    tol = _tol(dt)
    for p, cf in enumerate(patches):
        ref, bad = oracle.c_evaluate(order, ncoef, knots, cf, [0, 0], [uu, vv])
        assert bad == -1
        got = pos[p].reshape(3, -1)
        observe(f"tessellate axes: tess_rows {form} positions vs oracle, {_kind(dt)}", np.abs(got - ref).max() / _scale(ref), tol)
        flat = tabs[p].evaluate([uu, vv])
        assert np.abs(got - flat).max() <= tol * _scale(flat), (form, kind, p)
        if normals:
            area, _ = oracle.c_normal(order, ncoef, knots, cf, [uu, vv], False, False)
            got = nrm[p].reshape(3, -1)
            observe(f"tessellate axes: tess_rows {form} area normals vs oracle, {_kind(dt)}", np.abs(got - area).max() / _scale(area), tol)
    if normals:
        # unit normals, where the area normal is not small against the largest (its direction is ill-conditioned there)
        _, unit = bspy_amd.tessellate_tables(tabs, (u, v), normals=True, normalize=True)
        for p, cf in enumerate(patches):
            area, _ = oracle.c_normal(order, ncoef, knots, cf, [uu, vv], False, False)
            ref, _ = oracle.c_normal(order, ncoef, knots, cf, [uu, vv], True, False)
            ln = np.sqrt((np.asarray(area, np.float64) ** 2).sum(axis=0))
            ok = ln >= 1e-2 * ln.max()
            observe(f"tessellate axes: tess_rows {form} unit normals vs oracle, {_kind(dt)}",
                    np.abs(unit[p].reshape(3, -1)[:, ok] - ref[:, ok]).max(), tol)
