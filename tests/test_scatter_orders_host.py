"""
Every instantiation of the ``bsk_scatter_*`` family on the host path (CPU only): the 12 cases of
tests/golden/orders_scatter.npz (tests/golden/make_golden_scatter_orders.py), one per order tuple the kernels are built for,
each fitted with its first d = 1 .. 4 channels: the 48 (K0, K1, nDep) of scatter_gram.  Every case holds cells with
3, 0, 1, Q - 1, Q + 1, 63, 65, SEG, SEG + 1 and 2 SEG + 5 points, Q = strands(K0 K1).

    assembly       stencil and right-hand side against the exact normal equations within the counted bar of
                   ``scatter_ref.assembly_check`` (c_asm eps of the entry's own absolute sum; no elimination)
    symmetry       the stencil is symmetric bit for bit
    channels       the statement sums every r_ad on its own and the solve substitutes column by column: the stencil is the
                   same bits for every d, and rhs[:, :d], coefs[:d], residual-free tables (the unit and cell slabs'
                   columns 0 .. K + d) are the bits of d = 4
    coefficients   at d = 4 within the recorded bar of the exact coefficients
    counts         the points per cell are the constructed ones
    statement      on k2, k3, k4, k22, k34 and k44 the plain-Python ``scatter.statement`` is bit-equal to the host tables
    knots          per order tuple one point on every knot value, the domain ends among them (the fixture's parameters lie
                   strictly inside their cells): the keys by the rule of the statement, the assembly within its bar, the
                   statement bit for bit

The device twin is tests/test_gpu_scatter_orders.py; it imports the cases and ``host`` from here.
"""
import functools
import os

import numpy as np
import pytest

import orders_util as ou
import scatter_ref
from bspy_amd import scatter
from conftest import GOLDEN, observe

CASES = scatter_ref.load(os.path.join(GOLDEN, "orders_scatter.npz"))
TUPLES = ou.dispatched("scatter")
TRIPLES = ou.scatter_triples()
STATEMENT = ("k2", "k3", "k4", "k22", "k34", "k44")
HOST_PATHS = ["host scatter_key", "host scatter_gram", "host scatter_cell", "host scatter_fold", "host scatter_solve",
              "host scatter_residual"]


def triple_id(t):
    return f"k{t[0]}{t[1] if t[1] > 1 else ''}-d{t[2]}"


def name_of(t):
    return f"k{t[0]}{t[1] if t[1] > 1 else ''}"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64).tolist() if a.dtype == np.float64 else a.tolist()


def arrays(case, d):
    nind = len(case["order"])
    w = None if case["weights"] is None else np.ascontiguousarray(case["weights"], np.float64)
    return np.ascontiguousarray(case["uvw"].reshape(nind, -1), np.float64), np.ascontiguousarray(case["points"][:d], np.float64), w


@functools.lru_cache(maxsize=None)
def host(name, d):
    """The host path's results of a case with its first d channels, computed once: (coefs, info, assembled tables)."""
    case = CASES[name]
    uvw, pts, w = arrays(case, d)
    s, info = scatter.fit_batch(uvw, pts, case["order"], case["knots"], weights=w, _path="host")
    assert info["paths"] == HOST_PATHS
    res = scatter.assemble(scatter.Host(), scatter.Shape(case["order"], case["knots"]), uvw, pts, w, keep=True)
    return s.coefs.reshape(d, -1).copy(), info, res


@functools.lru_cache(maxsize=None)
def exact(name):
    """``scatter_ref.normal`` of a case with all its channels, computed once; d channels are its first d columns."""
    return scatter_ref.normal(dict(CASES[name], smoothing=0.0))


def test_the_cases_are_the_dispatched_tuples():
    top = scatter.DEVICE_MAX_K
    assert TUPLES == [(k,) for k in range(2, top + 1)] + [(a, b) for a in range(2, top + 1) for b in range(2, top + 1)]
    assert sorted(n for n in CASES if not n.startswith("shift")) == sorted(ou.case_id(o) for o in TUPLES)
    assert len(TRIPLES) == len(set(TRIPLES)) == 12 * scatter.DEVICE_MAX_NDEP
    for order in TUPLES:
        case = CASES[ou.case_id(order)]
        assert case["order"] == order and case["points"].shape[0] == scatter.DEVICE_MAX_NDEP
        assert [len(t) - 2 * k + 1 for t, k in zip(case["knots"], order)] == ([10] if len(order) == 1 else [4, 4])
    assert [scatter.strands(K) for K in (2, 3, 4, 6, 8, 9, 12, 16)] == [32, 16, 16, 8, 8, 4, 4, 4]
    assert scatter_ref.assembly_roundings(CASES["k2"], CASES["k2"]["counts"]) == 31
    assert scatter_ref.assembly_roundings(CASES["k4"], CASES["k4"]["counts"]) == 60
    assert scatter_ref.assembly_roundings(CASES["k44"], CASES["k44"]["counts"]) == 148


@pytest.mark.parametrize("order", TUPLES, ids=ou.case_id)
def test_counts_are_the_constructed_ones(order):
    name = ou.case_id(order)
    case, res = CASES[name], host(name, 4)[2]
    Q, SEG = scatter.strands(int(np.prod(order))), scatter.SEG
    edges = [3, 0, 1, Q - 1, Q + 1, 63, 65, SEG, SEG + 1, 2 * SEG + 5]
    counts = res["counts"].tolist()
    assert counts == case["counts"].tolist()
    rest = sorted(counts)
    for m in edges:
        rest.remove(m)
    assert len(rest) == (0 if len(order) == 1 else 6) and all(5 <= m <= 11 for m in rest)
    assert len(res["units"]) == int(np.sum(-(-res["counts"] // SEG)))
    # the empty and the one-point cell are interior cells
    shape = (10,) if len(order) == 1 else (4, 4)
    for m in (0, 1):
        at = np.unravel_index(counts.index(m), shape)
        assert all(0 < c < n - 1 for c, n in zip(at, shape))


@pytest.mark.parametrize("triple", TRIPLES, ids=triple_id)
def test_assembly_against_the_exact_normal_equations(triple):
    name, d = name_of(triple), triple[2]
    case, res = CASES[name], host(name, d)[2]
    N, Nbar, R, Rabs, counts = exact(name)
    cut = (N, Nbar, [row[:d] for row in R], [row[:d] for row in Rabs], counts)
    rs, rr, c = scatter_ref.assembly_check(dict(case, points=case["points"][:d]), res["stencil"], res["rhs"], exact=cut)
    observe(f"fit_points host assembly {triple_id(triple)}: stencil error / counted bar (c_asm = {c})", rs, 1.0)
    observe(f"fit_points host assembly {triple_id(triple)}: right-hand side error / counted bar (c_asm = {c})", rr, 1.0)
    # bitwise symmetry: entry (i, j) is entry (j, i)
    K0, K1 = (tuple(case["order"]) + (1,))[:2]
    n0, n1 = ([len(t) - k for t, k in zip(case["knots"], case["order"])] + [1])[:2]
    S = np.asarray(res["stencil"]).reshape(n0, n1, 2 * K0 - 1, 2 * K1 - 1)
    for e0 in range(2 * K0 - 1):
        for e1 in range(2 * K1 - 1):
            d0, d1 = e0 - (K0 - 1), e1 - (K1 - 1)
            i0 = np.arange(max(0, -d0), min(n0, n0 - d0))
            i1 = np.arange(max(0, -d1), min(n1, n1 - d1))
            here = S[np.ix_(i0, i1)][:, :, e0, e1]
            there = S[np.ix_(i0 + d0, i1 + d1)][:, :, 2 * K0 - 2 - e0, 2 * K1 - 2 - e1]
            assert bits(here) == bits(there)


@pytest.mark.parametrize("triple", TRIPLES, ids=triple_id)
def test_channels_are_independent_bit_for_bit(triple):
    name, d = name_of(triple), triple[2]
    K = triple[0] * triple[1]
    coefs, info, res = host(name, d)
    coefs4, info4, res4 = host(name, 4)
    for what in ("key", "status", "counts", "stencil"):
        assert bits(res[what]) == bits(res4[what]), what
    assert bits(res["rhs"]) == bits(res4["rhs"][:, :d])
    for what in ("units", "cells"):
        assert res[what].shape == res4[what].shape[:2] + (K + d,)
        assert bits(res[what]) == bits(res4[what][:, :, :K + d]), what
    assert bits(coefs) == bits(coefs4[:d])


@pytest.mark.parametrize("order", TUPLES, ids=ou.case_id)
def test_coefficients_within_the_recorded_bar(order):
    name = ou.case_id(order)
    case = CASES[name]
    coefs, info, _ = host(name, 4)
    assert not info["status"].any() and np.isfinite(info["residual"]).all()
    observe(f"fit_points host {name} with every loop edge: coefficient error / counted bar (c = {case['c']})",
            (np.abs(coefs - case["coefs"]) / case["bar"]).max(), 1.0)


def on_the_knots(order):
    """A case of its own per order tuple: one point on every knot value (for a surface on every pair of them), the domain
    ends among them.  -> (case, the keys by the rule of the statement: a knot belongs to the cell on its right, the right
    domain end to the last cell)."""
    case = CASES[ou.case_id(order)]
    breaks = [np.unique(t) for t in case["knots"]]
    uvw = np.stack([g.ravel() for g in np.meshgrid(*breaks, indexing="ij")])
    cells = [np.minimum(np.searchsorted(b, u, side="right") - 1, len(b) - 2) for b, u in zip(breaks, uvw)]
    key = cells[0] if len(order) == 1 else cells[0] * (len(breaks[1]) - 1) + cells[1]
    pts = ((np.arange(4 * uvw.shape[1]).reshape(4, -1) * 37 % 129) - 64) / 64.0
    return dict(case, uvw=uvw, points=pts, weights=None), key.astype(np.int64)


@pytest.mark.parametrize("order", TUPLES, ids=ou.case_id)
def test_points_on_the_knots_and_the_domain_ends(order):
    case, key = on_the_knots(order)
    uvw, pts, _ = arrays(case, 4)
    res = scatter.assemble(scatter.Host(), scatter.Shape(case["order"], case["knots"]), uvw, pts, None, keep=True)
    assert not res["status"].any() and res["key"].tolist() == key.tolist()
    assert res["key"][0] == 0 and res["key"][-1] == len(res["counts"]) - 1 == key.max()
    rs, rr, c = scatter_ref.assembly_check(case, res["stencil"], res["rhs"])
    observe(f"fit_points host assembly {ou.case_id(order)} on the knots: stencil error / counted bar (c_asm = {c})", rs, 1.0)
    observe(f"fit_points host assembly {ou.case_id(order)} on the knots: right-hand side error / counted bar (c_asm = {c})", rr, 1.0)
    want = scatter.statement(case["order"], case["knots"], uvw, pts, None)
    for what in ("key", "status", "units", "cells", "stencil", "rhs"):
        assert bits(np.asarray(res[what]).reshape(-1)) == bits(want[what].reshape(-1)), what


@pytest.mark.parametrize("name", STATEMENT)
def test_statement_bit_for_bit(name):
    case = CASES[name]
    uvw, pts, w = arrays(case, 4)
    res = host(name, 4)[2]
    want = scatter.statement(case["order"], case["knots"], uvw, pts, w)
    for what in ("key", "status", "units", "cells", "stencil", "rhs"):
        have = np.asarray(res[what])
        assert have.reshape(-1).shape == want[what].reshape(-1).shape, what
        assert bits(have.reshape(-1)) == bits(want[what].reshape(-1)), what
