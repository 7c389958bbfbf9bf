"""
``Spline.fit_points`` away from unit scale, on the host path (CPU only).  The cases and the ``check_*`` functions are shared
with tests/test_gpu_scatter_scale.py, which runs them with path="device" and path="cuda" (CUDA tensors in) and compares every
run with the host path byte for byte.  Every run asserts the launches from ``info["paths"]`` and ``scatter.LAST_PATHS``.

The cases are k4, k34 and k44 of tests/golden/orders_scatter.npz (cells of 3, 0, 1, Q - 1, Q + 1, 63, 65, SEG, SEG + 1 and
2 SEG + 5 points), each without weights and with weights on the 1/4 grid that include zeros.  The weighted ones are also
held to the plain-Python ``scatter.statement`` bit for bit: only with weights do the two triangles of a slab differ.

A. Exact laws, bit for bit.  Every threshold of the statement is relative, and a power of two commutes with every rounding
   as long as nothing leaves the normal range (the values here stay within 2^-100 .. 2^100), so there is no tolerance:
     points x 2^k                 stencil the same, rhs x 2^k, coefs x 2^k, residual x 2^k  (sqrt(2^2k x) = 2^k sqrt(x))
     weights x 2^k                stencil and rhs x 2^k, the same coefs and residual  (the U^T D U solve divides by the pivots)
     knots and uvw x 2^kp         per variable: key, status, units, cells, stencil, rhs, coefs and residual the same
     with smoothing               knots x 2^kp in all variables and smoothing x 2^(kp (2 m - nInd)): the same coefs
   k in -40, -7, 3, 40; kp in -20, 7 and the anisotropic pair (9, -5) (a curve takes its first entry).
B. Shifted and stretched domains: shift4 on [2^20, 2^20 + 1] and shift34 on [-2^10, -2^10 + 3] x [2^16, 2^16 + 1/4] against
   the exact oracle on the stored values: the assembly within ``scatter_ref.assembly_check``, the coefficients within the
   recorded bar.
C. Locality and independence, no tolerance.  One point's coordinates x 2^40, and separately its weight x 2^20: every slab
   of another unit, every slab of another cell and every stencil and right-hand-side row of a coefficient whose support
   does not hold that cell are the bits of the base run.  The points of one cell alone, in their order, give that cell's
   unit and cell slabs bit for bit (the cells of 2 SEG + 5 and of Q - 1 points).  A permutation of the input that keeps
   every cell's internal order gives the same bytes.
"""
import os

import numpy as np
import pytest

import scatter_ref
from bspy_amd import scatter
from conftest import GOLDEN, observe

GOLD = scatter_ref.load(os.path.join(GOLDEN, "orders_scatter.npz"))
DEVICE_PATHS = ["scatter_key", "scatter_gram", "scatter_cell", "scatter_fold", "host scatter_solve", "scatter_residual"]
HOST_PATHS = ["host " + p.replace("host ", "") for p in DEVICE_PATHS]
TABLES = ("key", "status", "counts", "units", "cells", "stencil", "rhs")
POWERS = (-40, -7, 3, 40)
KNOT_POWERS = ((-20, -20), (7, 7), (9, -5))


def _cases():
    rng = np.random.default_rng(404)
    out = {}
    for name in ("k4", "k34", "k44"):
        c = GOLD[name]
        base = dict(order=c["order"], knots=[np.array(t) for t in c["knots"]], uvw=np.array(c["uvw"]), points=np.array(c["points"]),
                    weights=None, counts=c["counts"])
        out[name] = base
        out[name + "-w"] = dict(base, weights=rng.integers(0, 9, base["uvw"].shape[1]) / 4.0)
    return out


CASES = _cases()
NAMES = sorted(CASES)
SHIFTED = ("shift4", "shift34")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64).tolist() if a.dtype == np.float64 else a.tolist()


def assert_bits(have, want, what):
    have, want = np.asarray(have), np.asarray(want)
    assert have.shape == want.shape, what
    assert bits(have.reshape(-1)) == bits(want.reshape(-1)), what


def run(case, path, tables=True, fit=True, **over):
    """One fit (``fit``) and one assembly (``tables``) of the case with the given entries replaced, on "host", "device" (NumPy
    in) or "cuda" (CUDA tensors in): dict of the tables, coefs (nDep, n), residual and status as NumPy arrays."""
    c = dict(case, **over)
    nind = len(c["order"])
    arrays = [np.ascontiguousarray(c["uvw"].reshape(nind, -1), np.float64), np.ascontiguousarray(c["points"], np.float64),
              None if c["weights"] is None else np.ascontiguousarray(c["weights"], np.float64)]
    more = dict(smoothing=c.get("smoothing", 0.0), penalty=c.get("penalty"))
    want = HOST_PATHS if path == "host" else DEVICE_PATHS
    out = {}
    if path == "host":
        be, put = scatter.Host(), arrays
    else:
        import torch
        be = scatter.Device.current()
        put = [None if a is None else torch.from_numpy(a).to(be.dev) for a in arrays]
    if fit:
        out = fitted(c, path, arrays, put, more, want)
    if tables:
        del scatter.LAST_PATHS[:]
        res = scatter.assemble(be, scatter.Shape(c["order"], c["knots"]), *put, keep=True)
        assert scatter.LAST_PATHS == want[:4], (path, scatter.LAST_PATHS)
        out.update({k: np.asarray(be.get(res[k])) for k in TABLES})
    return out


def fitted(c, path, arrays, put, more, want):
    if path == "host":
        s, info = scatter.fit_batch(*arrays[:2], c["order"], c["knots"], weights=arrays[2], _path="host", **more)
    elif path == "cuda":
        s, info = scatter.fit_batch(*put[:2], c["order"], c["knots"], weights=put[2], **more)
        assert info["status"].is_cuda and info["residual"].is_cuda
        info = dict(info, status=info["status"].cpu().numpy(), residual=info["residual"].cpu().numpy())
    else:
        s, info = scatter.fit_batch(*arrays[:2], c["order"], c["knots"], weights=arrays[2], _path="device", **more)
    assert info["paths"] == want and scatter.LAST_PATHS == want, (path, info["paths"])   # a host run cannot pass as a GPU result
    return dict(coefs=np.asarray(s.coefs).reshape(arrays[1].shape[0], -1).copy(), residual=info["residual"], fit_status=info["status"])


def same_run(have, want, what, skip=()):
    for key in want:
        if key not in skip:
            assert_bits(have[key], want[key], f"{what}: {key}")


# ------------------------------------------------------------------------------------------ A
def check_points_law(case, path):
    base = run(case, path)
    assert not base["fit_status"].any()
    for k in POWERS:
        f = 2.0 ** k
        got = run(case, path, points=case["points"] * f)
        for key in ("key", "status", "counts", "stencil"):
            assert_bits(got[key], base[key], f"points x 2^{k}: {key}")
        for key in ("rhs", "coefs", "residual"):
            assert_bits(got[key], base[key] * f, f"points x 2^{k}: {key}")
        K = int(np.prod(case["order"]))
        for key in ("units", "cells"):
            assert_bits(got[key][:, :, :K], base[key][:, :, :K], f"points x 2^{k}: {key}, the Gram part")
            assert_bits(got[key][:, :, K:], base[key][:, :, K:] * f, f"points x 2^{k}: {key}, the right-hand sides")
    return base


def check_weights_law(case, path):
    base = run(case, path)
    ones = np.ones(case["uvw"].shape[-1]) if case["weights"] is None else case["weights"]
    for k in POWERS:
        f = 2.0 ** k
        got = run(case, path, weights=ones * f)
        for key in ("key", "status", "counts", "coefs", "residual"):
            assert_bits(got[key], base[key], f"weights x 2^{k}: {key}")
        for key in ("units", "cells", "stencil", "rhs"):
            assert_bits(got[key], base[key] * f, f"weights x 2^{k}: {key}")
    return base


def scaled_domain(case, kp):
    nind = len(case["order"])
    f = [2.0 ** kp[d] for d in range(nind)]
    return dict(knots=[t * f[d] for d, t in enumerate(case["knots"])], uvw=case["uvw"].reshape(nind, -1) * np.array(f)[:, None])


def check_domain_law(case, path):
    base = run(case, path)
    for kp in KNOT_POWERS:
        got = run(case, path, **scaled_domain(case, kp))
        same_run(got, base, f"knots and uvw x 2^{kp}")
    nind = len(case["order"])
    for m in (1, 2):
        smooth = run(case, path, tables=False, smoothing=2.0 ** -12, penalty=m)
        assert bits(smooth["coefs"]) != bits(base["coefs"])
        for kp in KNOT_POWERS[:2]:
            got = run(case, path, tables=False, smoothing=2.0 ** (-12 + kp[0] * (2 * m - nind)), penalty=m, **scaled_domain(case, kp))
            same_run(got, smooth, f"knots x 2^{kp[0]}, smoothing x 2^({kp[0]} (2 {m} - {nind}))")
    return base


@pytest.mark.parametrize("name", NAMES)
def test_points_scaling_law(name):
    check_points_law(CASES[name], "host")


@pytest.mark.parametrize("name", NAMES)
def test_weights_scaling_law(name):
    check_weights_law(CASES[name], "host")


@pytest.mark.parametrize("name", NAMES)
def test_domain_scaling_law(name):
    check_domain_law(CASES[name], "host")


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith("-w")])
def test_statement_bit_for_bit_with_weights(name):
    """With weights other than 1.0 the two triangles of a slab differ in bits ((w B_a) B_b against (w B_b) B_a): the fold
    must read a <= b, and without weights no test can tell."""
    case = CASES[name]
    have = run(case, "host", fit=False)
    want = scatter.statement(case["order"], case["knots"], case["uvw"], case["points"], case["weights"])
    for key in ("key", "status", "units", "cells", "stencil", "rhs"):
        assert_bits(have[key].reshape(-1), want[key].reshape(-1), f"{name}: {key} against scatter.statement")
    K, cells = int(np.prod(case["order"])), have["cells"]
    assert bits(cells[:, :, :K]) != bits(np.swapaxes(cells[:, :, :K], 1, 2))       # the triangles do differ


def test_the_weighted_cases_hold_zero_weights():
    for name in NAMES:
        w = CASES[name]["weights"]
        assert (w is None) == (not name.endswith("-w"))
        if w is not None:
            assert (w == 0.0).sum() > 50 and ((w * 4.0) % 1.0 == 0.0).all() and w.max() == 2.0


# ------------------------------------------------------------------------------------------ B
def check_shifted(name, paths, oracle=True):
    case = GOLD[name]
    runs = [run(case, path) for path in paths]
    first = runs[0]
    assert not first["fit_status"].any() and first["counts"].tolist() == case["counts"].tolist()
    if oracle:
        rs, rr, c = scatter_ref.assembly_check(case, first["stencil"], first["rhs"])
        observe(f"fit_points {paths[0]} {name}: stencil error / counted bar (c_asm = {c})", rs, 1.0)
        observe(f"fit_points {paths[0]} {name}: right-hand side error / counted bar (c_asm = {c})", rr, 1.0)
    observe(f"fit_points {paths[0]} {name}: coefficient error / counted bar (c = {case['c']})",
            (np.abs(first["coefs"] - case["coefs"]) / case["bar"]).max(), 1.0)
    for path, other in zip(paths[1:], runs[1:]):
        same_run(other, first, f"{name}: {path} against {paths[0]}")
    return first


@pytest.mark.parametrize("name", SHIFTED)
def test_shifted_domain(name):
    case = GOLD[name]
    lo = [float(t[0]) for t in case["knots"]]
    assert lo == ([2.0 ** 20] if name == "shift4" else [-2.0 ** 10, 2.0 ** 16])
    check_shifted(name, ["host"])


# ------------------------------------------------------------------------------------------ C
def sorted_layout(case, key):
    """(order, first unit of every cell): the stable sort by key and where the cells' units start."""
    order = np.argsort(key, kind="stable")
    counts = np.bincount(key, minlength=len(case["counts"]))
    units = -(-counts // scatter.SEG)
    return order, np.cumsum(units) - units


def supports(case, cell):
    """bool (n,): the coefficients whose support holds the flat cell."""
    order = case["order"]
    ncoef = [len(t) - k for t, k in zip(case["knots"], order)]
    nc = [n - k + 1 for n, k in zip(ncoef, order)]
    at = np.unravel_index(cell, nc)
    grid = np.meshgrid(*[np.arange(n) for n in ncoef], indexing="ij")
    hit = np.ones(ncoef, bool)
    for g, c, k in zip(grid, at, order):
        hit &= (g >= c) & (g < c + k)
    return hit.reshape(-1)


def check_locality(case, path):
    base = run(case, path)
    counts = case["counts"]
    cell = int(np.argmax(counts))                                               # 2 SEG + 5 points: three units
    order, start = sorted_layout(case, base["key"])
    position = scatter.SEG + 3                                                  # in the cell's second unit
    first = int(np.cumsum(counts)[cell] - counts[cell])
    while case["weights"] is not None and case["weights"][order[first + position]] == 0.0:
        position += 1                                                           # a point that counts
    assert position < 2 * scatter.SEG
    point = int(order[first + position])
    unit = int(start[cell]) + 1
    assert base["key"][point] == cell
    pts = case["points"].copy()
    pts[:, point] *= 2.0 ** 40
    w = np.ones(case["uvw"].shape[-1]) if case["weights"] is None else case["weights"].copy()
    w[point] = max(w[point], 0.25) * 2.0 ** 20
    inside = supports(case, cell)
    assert 0 < inside.sum() == int(np.prod(case["order"])) < len(inside)
    for what, got in (("coordinates x 2^40", run(case, path, points=pts)), ("weight x 2^20", run(case, path, weights=w))):
        others = np.arange(len(base["units"])) != unit
        assert_bits(got["units"][others], base["units"][others], f"{what}: the other units")
        assert bits(got["units"][unit]) != bits(base["units"][unit]), what
        others = np.arange(len(base["cells"])) != cell
        assert_bits(got["cells"][others], base["cells"][others], f"{what}: the other cells")
        for key in ("stencil", "rhs"):
            assert_bits(got[key][~inside], base[key][~inside], f"{what}: {key} rows outside the support")
        assert bits(got["rhs"][inside]) != bits(base["rhs"][inside]), what
        for key in ("key", "status", "counts"):
            assert_bits(got[key], base[key], f"{what}: {key}")
    return base


def check_cell_alone(case, path):
    base = run(case, path)
    counts = case["counts"].tolist()
    Q = scatter.strands(int(np.prod(case["order"])))
    _, start = sorted_layout(case, base["key"])
    for m in (2 * scatter.SEG + 5, Q - 1):
        cell = counts.index(m)
        mine = np.flatnonzero(base["key"] == cell)                              # in input order: the cell's own order
        assert len(mine) == m
        alone = run(case, path, uvw=case["uvw"].reshape(len(case["order"]), -1)[:, mine], points=case["points"][:, mine],
                    weights=None if case["weights"] is None else case["weights"][mine], fit=False)
        assert alone["counts"].tolist() == [m if c == cell else 0 for c in range(len(counts))]
        nunits = -(-m // scatter.SEG)
        assert_bits(alone["units"], base["units"][start[cell]:start[cell] + nunits], f"the cell of {m} points alone: units")
        assert_bits(alone["cells"][cell], base["cells"][cell], f"the cell of {m} points alone: the cell slab")
        assert not np.delete(alone["cells"], cell, axis=0).any()
    return base


def check_permutation(case, path):
    base = run(case, path)
    perm = np.argsort(-base["key"], kind="stable")                              # the cells in decreasing order, each in its own order
    got = run(case, path, uvw=case["uvw"].reshape(len(case["order"]), -1)[:, perm], points=case["points"][:, perm],
              weights=None if case["weights"] is None else case["weights"][perm])
    for key in ("counts", "units", "cells", "stencil", "rhs", "coefs"):
        assert_bits(got[key], base[key], f"permuted: {key}")
    for key in ("key", "status", "residual"):
        assert_bits(got[key], base[key][perm], f"permuted: {key}")
    return base


@pytest.mark.parametrize("name", NAMES)
def test_locality_of_one_point(name):
    check_locality(CASES[name], "host")


@pytest.mark.parametrize("name", NAMES)
def test_one_cell_alone(name):
    check_cell_alone(CASES[name], "host")


@pytest.mark.parametrize("name", NAMES)
def test_permutation_within_the_cells_order(name):
    check_permutation(CASES[name], "host")
