"""
``Spline.fit_points`` on the device path: every recorded case of tests/golden/scatter.npz that the kernels cover (orders
2 .. 4, nDep 1 .. 4) against the exact coefficients within the counted bar, with the launches asserted from
``scatter.LAST_PATHS``; then the device path against the host path BYTE FOR BYTE (keys, status, unit slabs, cell slabs,
stencil, right-hand side, coefficients, residuals): there is no tolerance.  The same with CUDA tensors in, with the input
permuted so that every cell keeps its internal order, and twice in a row.  One property case of 2 x 10^5 points on 20 x 20
bicubic coefficients (cells of several units, two levels of the tree).  Gridded data against ``Spline.least_squares``.
The host results are computed once per case and shared.
"""
import functools
import os
import warnings

import numpy as np
import pytest

import scatter_ref
from bspy_amd import Spline, scatter
from conftest import GOLDEN, observe

pytestmark = pytest.mark.gpu

CASES = scatter_ref.load(os.path.join(GOLDEN, "scatter.npz"))
COVERED = sorted(n for n, c in CASES.items() if max(c["order"]) <= scatter.DEVICE_MAX_K)
KERNELS = ["scatter_key", "scatter_gram", "scatter_cell", "scatter_fold", "host scatter_solve", "scatter_residual"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64).tolist() if a.dtype == np.float64 else a.tolist()


def arrays(case):
    nind = len(case["order"])
    uvw = np.ascontiguousarray(case["uvw"].reshape(nind, -1), np.float64)
    w = None if case["weights"] is None else np.ascontiguousarray(case["weights"], np.float64)
    return uvw, np.ascontiguousarray(case["points"], np.float64), w


def fit(case, path, **more):
    args = dict(weights=case["weights"], smoothing=case["smoothing"], penalty=case["penalty"], _path=path)
    args.update(more)
    return scatter.fit_batch(case["uvw"], case["points"], case["order"], case["knots"], **args)


@functools.lru_cache(maxsize=None)
def host(name):
    """The host path's results of a case, computed once: (coefs, info, assembled tables)."""
    case = CASES[name]
    s, info = fit(case, "host")
    res = scatter.assemble(scatter.Host(), scatter.Shape(case["order"], case["knots"]), *arrays(case), keep=True)
    return s.coefs.copy(), info, res


def device_tables(case):
    import torch
    be = scatter.Device.current()
    put = [None if a is None else torch.from_numpy(a).to(be.dev) for a in arrays(case)]
    res = scatter.assemble(be, scatter.Shape(case["order"], case["knots"]), *put, keep=True)
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", COVERED)
def test_golden_device(name):
    case = CASES[name]
    s, info = fit(case, "device")
    assert info["paths"] == KERNELS and scatter.LAST_PATHS == KERNELS           # a host assembly cannot pass as a GPU result
    got = s.coefs.reshape(case["coefs"].shape)
    observe(f"fit_points device {name}: coefficient error / counted bar (c = {case['c']})", (np.abs(got - case["coefs"]) / case["bar"]).max(), 1.0)
    coefs, hinfo, _ = host(name)
    assert bits(s.coefs) == bits(coefs)
    assert bits(info["residual"]) == bits(hinfo["residual"]) and bits(info["status"]) == bits(hinfo["status"])
    assert info["objective"] == hinfo["objective"] and info["empty"] == hinfo["empty"]


@pytest.mark.parametrize("name", COVERED)
def test_device_tables_equal_host_tables_byte_for_byte(name):
    have, want = device_tables(CASES[name]), host(name)[2]
    for what in ("key", "status", "counts", "units", "cells", "stencil", "rhs"):
        assert have[what].shape == np.asarray(want[what]).shape, what
        assert bits(have[what].reshape(-1)) == bits(np.asarray(want[what]).reshape(-1)), what


def test_orders_above_four_take_the_host_path():
    for name in ("curve5", "curve6"):
        case = CASES[name]
        with pytest.raises(ValueError, match="device path covers orders 2 to 4"):
            fit(case, "device")
        s, info = fit(case, None)
        assert info["paths"][0] == "host scatter_key"


@pytest.mark.parametrize("name", ["pair44", "weights", "counts", "hole2"])
def test_cuda_tensors_permutations_and_repeats(name):
    import torch
    case = CASES[name]
    coefs = host(name)[0]
    uvw, pts, w = arrays(case)
    t = [None if a is None else torch.from_numpy(a).cuda() for a in (uvw, pts, w)]
    more = dict(smoothing=case["smoothing"], penalty=case["penalty"])
    s, info = scatter.fit_batch(t[0], t[1], case["order"], case["knots"], weights=t[2], **more)
    assert info["paths"] == KERNELS and info["status"].is_cuda and info["residual"].is_cuda
    assert bits(s.coefs) == bits(coefs) and bits(info["residual"].cpu().numpy()) == bits(host(name)[1]["residual"])
    # float32 tensors are widened first
    s32, _ = scatter.fit_batch(t[0], t[1].float(), case["order"], case["knots"], weights=t[2], **more)
    s64, _ = scatter.fit_batch(uvw, pts.astype(np.float32).astype(np.float64), case["order"], case["knots"], weights=w, _path="host", **more)
    assert bits(s32.coefs) == bits(s64.coefs)
    # a permutation that keeps every cell's internal order: the cells in decreasing order of their key
    key = host(name)[2]["key"]
    perm = np.argsort(-key, kind="stable")
    s, _ = scatter.fit_batch(uvw[:, perm], pts[:, perm], case["order"], case["knots"], weights=None if w is None else w[perm],
                             _path="device", **more)
    assert bits(s.coefs) == bits(coefs)
    # and one that does not may change bits, but stays within the bar
    back = perm[::-1]
    s, _ = scatter.fit_batch(uvw[:, back], pts[:, back], case["order"], case["knots"], weights=None if w is None else w[back],
                             _path="device", **more)
    assert (np.abs(s.coefs.reshape(case["coefs"].shape) - case["coefs"]) <= case["bar"]).all()
    # twice: the same bytes
    again, _ = fit(case, "device")
    assert bits(again.coefs) == bits(coefs)


def test_two_hundred_thousand_points_device_equals_host():
    rng = np.random.default_rng(11)
    order = (4, 4)
    knots = [np.concatenate(([0.0] * 4, np.sort(rng.random(16)), [1.0] * 4)) for _ in range(2)]
    N = 200000
    uvw = rng.random((2, N)) ** 2                                              # crowded cells: several units, two tree levels
    pts = rng.standard_normal((3, N))
    w = rng.random(N)
    sh = scatter.Shape(order, knots)
    want = scatter.assemble(scatter.Host(), sh, uvw, pts, w)
    assert int(np.max(want["counts"])) > scatter.FAN * scatter.SEG              # a cell of more than FAN units: a second level
    have = device_tables(dict(order=order, knots=knots, uvw=uvw, points=pts, weights=w))
    for what in ("key", "status", "counts", "stencil", "rhs"):
        assert bits(have[what].reshape(-1)) == bits(np.asarray(want[what]).reshape(-1)), what
    s_dev, info = scatter.fit_batch(uvw, pts, order, knots, weights=w, _path="device")
    s_host, _ = scatter.fit_batch(uvw, pts, order, knots, weights=w, _path="host")
    assert info["paths"].count("scatter_cell") == 2
    assert bits(s_dev.coefs) == bits(s_host.coefs)
    s_auto, info = scatter.fit_batch(uvw, pts, order, knots, weights=w)
    assert info["paths"][0] == "scatter_key"                                   # above DEVICE_MIN_WORK: the device path by itself


def test_parameter_correction_on_the_device():
    rng = np.random.default_rng(5)
    order, knots = (4, 4), [np.array([0, 0, 0, 0, 0.3, 0.6, 1, 1, 1, 1.0])] * 2
    u = rng.random((2, 400))
    truth = np.stack([u[0], u[1], 0.3 * np.sin(3 * u[0]) * np.cos(2 * u[1])])
    pts = truth + 0.01 * rng.standard_normal(truth.shape)
    start = np.clip(u + 0.03 * rng.standard_normal(u.shape), 0.0, 1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        s, info = scatter.fit_batch(start, pts, order, knots, correct=2, _path="device")
        h, hinfo = scatter.fit_batch(start, pts, order, knots, correct=2, _path="host")
    obj = info["objective"]
    assert len(obj) == 3 and obj[-1] < obj[0] and "project_newton" in info["paths"]
    for before, after in zip(obj, obj[1:]):
        assert after <= before * (1.0 + 36 * 2.0 ** -52)
    assert bits(s.coefs) == bits(h.coefs)                                      # project and fit_points: both paths, the same bits


def test_gridded_data_agrees_with_least_squares():
    """Gridded data fed as scattered points has the minimiser of Spline.least_squares on the same knots, which solves by
    QR.  Both are within their bars of the exact coefficients; the QR's bar is below the normal equations' counted bar
    (its error grows with cond(A), not cond(A)^2), so the difference is within twice the counted bar."""
    rng = np.random.default_rng(9)
    order = (3, 4)
    knots = [np.array([0, 0, 0, 0.25, 0.5, 0.75, 1, 1, 1.0]), np.array([0, 0, 0, 0, 0.4, 0.7, 1, 1, 1, 1.0])]
    u0, u1 = np.linspace(0, 1, 11), np.linspace(0, 1, 13)
    data = rng.integers(-512, 513, (2, 11, 13)) / 512.0
    ref = Spline.least_squares([u0, u1], data, order, knots)
    g0, g1 = np.meshgrid(u0, u1, indexing="ij")
    uvw = np.stack([g0.ravel(), g1.ravel()])
    s, info = scatter.fit_batch(uvw, data.reshape(2, -1), order, knots, _path="device")
    exact, bar, c = scatter_ref.record(dict(order=order, knots=knots, uvw=uvw, points=data.reshape(2, -1)))
    observe(f"fit_points on a grid: coefficient error / counted bar (c = {c})", (np.abs(s.coefs.reshape(2, -1) - exact) / bar).max(), 1.0)
    err = np.abs(s.coefs.reshape(2, -1) - ref.coefs.reshape(2, -1))
    observe("fit_points on a grid against least_squares: difference / (2 x counted bar)", (err / (2.0 * bar)).max(), 1.0)
