"""
insert_knots, elevate, elevate_and_insert_knots, trim, clamp and differentiate without a GPU: the knot logic, the
reference's messages and identities, the band operator's properties, and the host half of the library
(bsk_band_apply_host through ctypes, which makes no HIP call) against the goldens of tests/golden/refine.npz (written
by tests/golden/make_golden_refine.py) and against the exact results of tests/refine_ref.py.  The device half is
covered by tests/test_gpu_refine.py, which takes its helpers from here.

Bars, relative to max |coef| of the expected result:
  against the exact result       1e-12 (the parity bar of tests/test_gpu_parity.py); observed values are recorded
  against the reference          max(1e-12, 10 x ref_dev), ref_dev = the reference's own recorded distance from exact
  "bad_*" cases                  the reference's elevation is off by 1e-10 .. 1e-7 there: pinned to the exact result only,
                                 and our error must be below the reference's ref_dev
  float32 splines                against the exact result rounded to float32 and against the reference: 10 x ref_dev,
                                 the reference's own float32 deviation from exact
Entries of a result whose basis function has no cell inside the domain (elevation of an unclamped spline) have no
exact value and no influence inside the domain: they are left out of the coefficient comparison, and the result is
compared with the original by evaluation over the domain.
"""
import json
import math
import os

import numpy as np
import pytest

import oracle
import refine_ref
from bspy_amd import Spline, refinement
from conftest import GOLDEN, observe

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "refine.npz"))


def _names():
    with np.load(os.path.join(GOLDEN, "refine.npz")) as g:
        return sorted({k.split("/")[0] for k in g.files})


NAMES = _names()


def load_case(g, name):
    order = [int(o) for o in g[f"{name}/order"]]
    n = len(order)
    c = dict(name=name, op=str(g[f"{name}/op"]), order=order, knots=[g[f"{name}/knots{i}"] for i in range(n)],
             coefs=g[f"{name}/coefs"], out_order=[int(o) for o in g[f"{name}/out_order"]],
             out_knots=[g[f"{name}/out_knots{i}"] for i in range(n)], out_coefs=g[f"{name}/out_coefs"],
             ref_dev=float(g[f"{name}/ref_dev"]))
    if f"{name}/new0" in g.files:
        c["new"] = [[(float(k), int(m)) if pair else float(k) for (k, m), pair in zip(g[f"{name}/new{i}"], g[f"{name}/pair{i}"])]
                    for i in range(n)]
    for key in ("m", "left", "right"):
        if f"{name}/{key}" in g.files:
            c[key] = [int(v) for v in g[f"{name}/{key}"]]
    if f"{name}/wrt" in g.files:
        c["wrt"] = int(g[f"{name}/wrt"])
    if f"{name}/domain" in g.files:
        c["domain"] = [[None if np.isnan(b) else b for b in bounds] for bounds in g[f"{name}/domain"]]
    return c


def make_spline(c):
    return Spline(len(c["order"]), c["coefs"].shape[0], c["order"], c["coefs"].shape[1:], c["knots"], c["coefs"])


def run_case(s, c, path):
    op = c["op"]
    if op == "insert_knots":
        return s.insert_knots(c["new"], _path=path)
    if op == "elevate":
        return s.elevate(c["m"], _path=path)
    if op == "elevate_and_insert_knots":
        return s.elevate_and_insert_knots(c["m"], c["new"], _path=path)
    if op == "trim":
        return s.trim(c["domain"], _path=path)
    if op == "clamp":
        return s.clamp(c["left"], c["right"], _path=path)
    return s.differentiate(c["wrt"], _path=path)


_EXACT = {}


def exact_of(c):
    """(exact result rounded once to the coefficients' dtype, mask of the entries that exist), per case once a session."""
    if c["name"] not in _EXACT:
        if c["op"] == "differentiate":
            e = refine_ref.differentiate(c["order"], c["knots"], c["coefs"], c["wrt"])
            _EXACT[c["name"]] = (e, np.ones(e.shape, bool))
        else:
            _EXACT[c["name"]] = refine_ref.change_basis(c["order"], c["knots"], c["coefs"], c["out_order"], c["out_knots"])
    return _EXACT[c["name"]]


def domain_points(order, knots, count, seed):
    rng = np.random.default_rng(seed)
    return [k[o - 1] + (k[len(k) - o] - k[o - 1]) * rng.random(count) for o, k in zip(order, knots)]


def values(s, points, wrt=None):
    v, bad = oracle.c_evaluate(list(s.order), list(s.nCoef), [np.asarray(k, np.float64) for k in s.knots],
                               np.asarray(s.coefs, np.float64), wrt if wrt is not None else [0] * s.nInd, points)
    assert bad == -1
    return v


def check_golden(c, r, label):
    """The result r of case c against the golden: knots bit for bit, coefficients at the bars of this file's header."""
    assert list(r.order) == c["out_order"]
    assert r.coefs.dtype == c["coefs"].dtype and r.coefs.shape == c["out_coefs"].shape
    for got, want in zip(r.knots, c["out_knots"]):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), f"{c['name']}: knots differ from the reference's"
    exact, mask = exact_of(c)
    scale = float(np.abs(exact[mask]).max())
    ours = np.asarray(r.coefs, np.float64)
    err_exact = float(np.abs(ours - exact.astype(np.float64))[mask].max() / scale)
    err_ref = float(np.abs(ours - np.asarray(c["out_coefs"], np.float64))[mask].max() / scale)
    print(f"{label} {c['name']}: against exact {err_exact:.3e}, against the reference {err_ref:.3e}, ref_dev {c['ref_dev']:.3e}")
    if c["coefs"].dtype == np.float32:
        observe(f"{label} fp32 {c['name']}", err_exact, 10.0 * c["ref_dev"])
        assert err_ref <= max(1e-12, 10.0 * c["ref_dev"])
    else:
        observe(f"{label} fp64 against exact", err_exact, 1e-12)
        if c["name"].startswith("bad_"):
            assert c["ref_dev"] > 1e-12, "a bad case must be one the reference misses"
            assert err_exact < c["ref_dev"]
        else:
            assert err_ref <= max(1e-12, 10.0 * c["ref_dev"])
    if not mask.all():
        pts = domain_points(c["order"], c["knots"], 400, 5)
        before, after = values(make_spline(c), pts), values(r, pts)
        observe(f"{label} outside rows by evaluation", np.abs(after - before).max() / np.abs(c["coefs"]).max(), 1e-12)


# ------------------------------------------------------------------------------------------ goldens, host path
@pytest.mark.parametrize("name", NAMES)
def test_golden_host(golden, name):
    c = load_case(golden, name)
    r = run_case(make_spline(c), c, "host")
    assert refinement.LAST_PATHS and set(refinement.LAST_PATHS) == {"host band"}
    check_golden(c, r, "refine host")


def test_golden_file_keeps_the_reference_comparison_alive(golden):
    by_op = {}
    for name in NAMES:
        c = load_case(golden, name)
        by_op.setdefault(c["op"], []).append(c["ref_dev"])
    assert set(by_op) == {"insert_knots", "elevate", "elevate_and_insert_knots", "trim", "clamp", "differentiate"}
    for op, devs in by_op.items():
        assert 2 * sum(d <= 1e-12 for d in devs) >= len(devs), op
    assert 2 <= sum(n.startswith("bad_") for n in NAMES) <= 3


# ------------------------------------------------------------------------------------------ messages and identities
def _semantics():
    with open(os.path.join(GOLDEN, "refine_semantics.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("record", _semantics(), ids=lambda r: r["name"])
def test_reference_messages_and_identities(record):
    s = record["spline"]
    spline = Spline(len(s["order"]), len(s["coefs"]), s["order"], np.shape(s["coefs"])[1:], s["knots"], s["coefs"], metadata={"tag": 7})
    method = getattr(spline, record["op"])
    if record["error"] is not None:
        with pytest.raises(ValueError) as info:
            method(*record["args"])
        assert str(info.value) == record["error"]
    else:
        r = method(*record["args"])
        assert (r is spline) == record["is_self"]
        assert isinstance(r, Spline) and r.metadata == {"tag": 7} and r.coefs.dtype == spline.coefs.dtype


def test_path_argument_is_checked():
    s = Spline(1, 1, (2,), (3,), [[0.0, 0, 0.5, 1, 1]], [[0.0, 1.0, 3.0]])
    with pytest.raises(ValueError, match="_path"):
        s.insert_knots([[0.25]], _path="gpu")


# ------------------------------------------------------------------------------------------ the operator
def random_knots(rng, order, ncoef, unclamped=False):
    if unclamped:
        return np.sort(rng.random(order + ncoef) * 3.0 - 1.0)
    interior = np.sort(rng.random(ncoef - order))
    if ncoef - order > 4 and order > 1:
        interior[2] = interior[1]                   # a double knot
    return np.concatenate((order * [0.0], interior, order * [1.0]))


def check_operator(first, w, order, n_in, exists=None):
    """exists: the rows whose basis function has a cell inside the domain (default all); the others hold the
    coefficients of a polynomial extension, which are affine but not convex combinations."""
    assert w.shape[1] <= order
    assert np.all(np.diff(first) >= 0) and first[0] >= 0 and first[-1] + w.shape[1] <= n_in
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 64 * EPS
    assert (w if exists is None else w[exists]).min() >= 0.0


def check_zero_pattern(first, w, rows, n_in, label):
    """(w != 0) is the pattern of the exact rows (refine_ref.refine_rows): a weight whose exact value is zero is stored as
    0.0, and no weight that is not zero in exact arithmetic has gone.  Rows without an exact value are left out."""
    k = w.shape[1]
    for j, row in enumerate(rows):
        if row is None:
            continue
        got, want = np.zeros(n_in, bool), np.zeros(n_in, bool)
        got[first[j]:first[j] + k] = w[j] != 0.0
        want[row[0]:row[0] + len(row[1])] = [v != 0 for v in row[1]]
        assert np.array_equal(got, want), f"{label}, row {j}: stored non-zeros at {np.flatnonzero(got)}, exact ones at {np.flatnonzero(want)}"


def random_operators():
    """The sixty random operators of test_operator_properties_random: (trial, order, m, knots, new knots)."""
    rng = np.random.default_rng(11)
    for trial in range(60):
        order = int(rng.integers(1, 9))
        ncoef = order + int(rng.integers(0, 40))
        t = random_knots(rng, order, ncoef)
        m = int(rng.integers(0, 4))
        new = list(rng.random(int(rng.integers(0 if m else 1, 30))))
        yield trial, order, m, t, new


# Exact rows cost rows x subsets x order^2 Fraction operations.  Above this the pattern of an operator is not computed in
# the test but read from tests/golden/refine_patterns.npz, which tests/golden/make_golden_refine_patterns.py wrote from
# the same refine_ref.refine_rows (14 of the 60 operators, 1 to 23 s each, two minutes together).
EXACT_ROWS_BUDGET = 40_000


def exact_rows_cost(order, m, n_out):
    return n_out * math.comb(order + m - 1, order - 1) * order * order


def dense_pattern(rows, n_in):
    """(rows, n_in) bool: where the exact rows are not zero (every row must exist)."""
    out = np.zeros((len(rows), n_in), bool)
    for j, (at, weights) in enumerate(rows):
        out[j, at:at + len(weights)] = [v != 0 for v in weights]
    return out


def test_operator_properties_random():
    """Every one of the sixty operators: the band's shape, rows that sum to one, no negative weight, and (w != 0) equal
    to the exact rows' pattern, computed here or recorded (the recorded ones are tied to their knots bit for bit)."""
    recorded = np.load(os.path.join(GOLDEN, "refine_patterns.npz"))
    from_file = 0
    for trial, order, m, t, new in random_operators():
        ncoef = len(t) - order
        if m:
            tbar = refinement.elevated_knots(t, order, m, new)
            first, w = refinement.refine_map(t, order, tbar, m)
        else:
            tbar, origin = refinement.merged_knots(t, order, new)
            first, w = refinement.refine_map(t, order, tbar, 0, origin=origin)
        assert len(first) == len(tbar) - order - m
        check_operator(first, w, order, ncoef)
        label = f"trial {trial}: order {order}, m {m}"
        if exact_rows_cost(order, m, len(first)) <= EXACT_ROWS_BUDGET:
            assert f"{trial}/pattern" not in recorded.files
            check_zero_pattern(first, w, refine_ref.refine_rows(t, order, tbar, m), ncoef, label)
            continue
        assert recorded[f"{trial}/knots"].tobytes() == t.tobytes() and recorded[f"{trial}/new_knots"].tobytes() == tbar.tobytes(), \
            f"{label}: the recorded pattern belongs to other knots"
        got = np.zeros((len(first), ncoef), bool)
        for j in range(len(first)):
            got[j, first[j]:first[j] + order] = w[j] != 0.0
        want = recorded[f"{trial}/pattern"]
        assert got.shape == want.shape
        differ = np.flatnonzero((got != want).any(axis=1))
        assert not len(differ), f"{label}: rows {differ} differ from the recorded exact pattern"
        from_file += 1
    assert from_file == len(recorded.files) // 3 == 14


def test_zero_pattern_of_trim_rows_and_tiny_weights():
    """The ``rows=`` / ``origin=`` form (trim, clamp) stores the same structural zeros; a weight that is tiny but not zero
    (a new knot 1e-9 of a cell away from an old one) stays."""
    rng = np.random.default_rng(12)
    for order, unclamped in ((4, False), (6, True), (8, False)):
        t = random_knots(rng, order, order + 25, unclamped)
        lo, hi = t[order - 1], t[len(t) - order]
        wanted = [(lo + 0.31 * (hi - lo), order), (lo + 0.72 * (hi - lo), order)]
        merged, origin = refinement.merged_knots(t, order, wanted)
        row0, row1 = int(np.searchsorted(merged, wanted[0][0])), int(np.searchsorted(merged, wanted[1][0]))
        first, w = refinement.refine_map(t, order, merged, 0, rows=slice(row0, row1), origin=origin)
        rows = refine_ref.refine_rows(t, order, merged, 0)[row0:row1]
        check_operator(first, w, order, len(t) - order, np.array([row is not None for row in rows]))
        check_zero_pattern(first, w, rows, len(t) - order, f"trim rows, order {order}")
    t = random_knots(rng, 4, 12)
    near = t[6] + 1e-9 * (t[7] - t[6])
    merged, origin = refinement.merged_knots(t, 4, [near])
    first, w = refinement.refine_map(t, 4, merged, 0, origin=origin)
    check_zero_pattern(first, w, refine_ref.refine_rows(t, 4, merged, 0), 12, "a nearly coincident knot")
    assert 0.0 < w[w > 0.0].min() < 1e-8


def test_operator_properties_goldens(golden):
    for name in NAMES:
        c = load_case(golden, name)
        if c["op"] == "differentiate":
            continue
        for k, t, k2, t2 in zip(c["order"], c["knots"], c["out_order"], c["out_knots"]):
            if k == k2 and len(t) == len(t2):
                continue
            first, w = refinement.refine_map(t, k, t2, k2 - k)
            rows = refine_ref.refine_rows(t, k, t2, k2 - k)
            check_operator(first, w, k, len(t) - k, np.array([row is not None for row in rows]))
            check_zero_pattern(first, w, rows, len(t) - k, name)
            dense = np.zeros((len(first), len(t) - k))
            for j in range(len(first)):
                dense[j, first[j]:first[j] + k] = w[j]
            for j, row in enumerate(rows):
                if row is not None:
                    want = np.zeros(len(t) - k)
                    want[row[0]:row[0] + k] = [float(v) for v in row[1]]
                    assert np.abs(dense[j] - want).max() <= 64 * EPS, (name, j)


def test_unit_rows_are_exact():
    """Coefficients away from the inserted knots are copied, not recomputed."""
    rng = np.random.default_rng(3)
    t = random_knots(rng, 4, 30)
    coefs = rng.standard_normal((2, 30))
    s = Spline(1, 2, (4,), (30,), [t], coefs)
    r = s.insert_knots([[0.5 * (t[15] + t[16])]], _path="host")
    assert np.array_equal(r.coefs[:, :13], coefs[:, :13]) and np.array_equal(r.coefs[:, 16:], coefs[:, 15:])


def test_band_map_apply_line_is_the_host_driver():
    rng = np.random.default_rng(5)
    t = random_knots(rng, 5, 40)
    tbar = refinement.elevated_knots(t, 5, 2, list(rng.random(9)))
    band = refinement.BandMap(*refinement.refine_map(t, 5, tbar, 2), 40)
    for dtype in (np.float64, np.float32):
        a = rng.standard_normal((3, 40, 4)).astype(dtype)
        got = band.apply_host(a, 3, 4)
        assert got.dtype == dtype and band.last_kernel() == "host band"
        for o in range(3):
            for i in range(4):
                assert np.array_equal(got[o, :, i], band.apply_line(a[o, :, i]))
    band.close()


# ------------------------------------------------------------------------------------------ invariants through the oracle
def surface(rng, dtype=np.float64, unclamped=False):
    order, ncoef = (4, 3), (13, 11)
    knots = [random_knots(rng, o, n, unclamped) for o, n in zip(order, ncoef)]
    return Spline(2, 3, order, ncoef, knots, rng.standard_normal((3, *ncoef)).astype(dtype))


def test_evaluate_invariant():
    rng = np.random.default_rng(21)
    s = surface(rng)
    scale = np.abs(s.coefs).max()
    pts = domain_points(s.order, s.knots, 500, 1)
    before = values(s, pts)
    r = s.insert_knots([list(rng.random(9)), [(0.37, 2), 0.81]], _path="host")
    assert r.nCoef == (22, 14)
    observe("refine invariant insert_knots", np.abs(values(r, pts) - before).max() / scale, 1e-12)
    r = s.elevate([1, 2], _path="host")
    assert r.order == (5, 5)
    observe("refine invariant elevate", np.abs(values(r, pts) - before).max() / scale, 1e-12)
    r = s.elevate_and_insert_knots([2, 0], [[0.2, 0.2], [0.55]], _path="host")
    observe("refine invariant elevate_and_insert_knots", np.abs(values(r, pts) - before).max() / scale, 1e-12)
    r = s.trim([[0.2, 0.7], [None, 0.6]], _path="host")
    assert np.array_equal(r.domain(), [[0.2, 0.7], [0.0, 0.6]])
    inside = [0.2 + 0.5 * rng.random(500), 0.6 * rng.random(500)]
    observe("refine invariant trim", np.abs(values(r, inside) - values(s, inside)).max() / scale, 1e-12)
    u = surface(rng, unclamped=True)
    pts = domain_points(u.order, u.knots, 500, 2)
    r = u.clamp([0, 1], [0, 1], _path="host")
    for k, o, d in zip(r.knots, r.order, u.domain()):
        assert np.all(k[:o] == d[0]) and np.all(k[-o:] == d[1])
    observe("refine invariant clamp", np.abs(values(r, pts) - values(u, pts)).max() / np.abs(u.coefs).max(), 1e-12)
    r = u.elevate([1, 1], _path="host")
    observe("refine invariant elevate unclamped", np.abs(values(r, pts) - values(u, pts)).max() / np.abs(u.coefs).max(), 1e-12)


def test_differentiate_is_the_derivative():
    rng = np.random.default_rng(22)
    s = surface(rng)
    pts = domain_points(s.order, s.knots, 500, 3)
    for iv in range(2):
        d = s.differentiate(iv, _path="host")
        assert d.order[iv] == s.order[iv] - 1 and d.nCoef[iv] == s.nCoef[iv] - 1
        wrt = [int(i == iv) for i in range(2)]
        observe("refine differentiate against the oracle's derivative",
                np.abs(values(d, pts) - values(s, pts, wrt)).max() / np.abs(d.coefs).max(), 1e-12)


def test_insert_then_trim_is_trim():
    rng = np.random.default_rng(23)
    s = surface(rng)
    dom = [[0.3, 0.6], [0.25, None]]
    alone = s.trim(dom, _path="host")
    both = s.insert_knots([[0.05, 0.1, 0.8, (0.9, 2)], [0.1, 0.2]], _path="host").trim(dom, _path="host")
    assert both.nCoef == alone.nCoef
    for a, b in zip(alone.knots, both.knots):
        assert np.array_equal(a, b)
    observe("refine insert then trim", np.abs(both.coefs - alone.coefs).max() / np.abs(alone.coefs).max(), 1e-12)


def test_float32_keeps_dtype_and_metadata():
    rng = np.random.default_rng(24)
    s = surface(rng, np.float32)
    s.metadata["name"] = "patch"
    for r in (s.insert_knots([[0.5], []]), s.elevate([1, 0]), s.trim([[0.1, 0.9], [None, None]]), s.differentiate(1)):
        assert r.coefs.dtype == np.float32 and r.metadata == {"name": "patch"}


# ------------------------------------------------------------------------------------------ dispatch
def test_order_nine_takes_the_host_driver():
    rng = np.random.default_rng(25)
    t = random_knots(rng, 9, 24)
    s = Spline(1, 2, (9,), (24,), [t], rng.standard_normal((2, 24)))
    new = list(rng.random(7))
    r = s.insert_knots([new])
    assert refinement.LAST_PATHS == ["host band"]
    exact, mask = refine_ref.change_basis([9], [t], s.coefs, [9], r.knots)
    assert mask.all()
    observe("refine order 9 against exact", np.abs(r.coefs - exact).max() / np.abs(exact).max(), 1e-12)
    with pytest.raises(ValueError, match="device path covers K"):
        s.insert_knots([new], _path="device")
    refinement.DEVICE_MIN_ELEMENTS, keep = 1, refinement.DEVICE_MIN_ELEMENTS
    try:
        s.insert_knots([new])                       # even when the size asks for the device
        assert refinement.LAST_PATHS == ["host band"]
    finally:
        refinement.DEVICE_MIN_ELEMENTS = keep


def test_small_tensors_take_the_host_driver_and_shrinking_maps_go_first():
    rng = np.random.default_rng(26)
    s = surface(rng)
    s.trim([[0.4, 0.6], [None, None]])
    assert refinement.LAST_PATHS == ["host band"]
    # variable 0 grows (insertion), variable 1 shrinks (differentiate has no partner here: use trim + insertion)
    calls = []
    keep = refinement.BandMap.apply_host

    def spy(self, a, outer, inner):
        calls.append((self.nIn, self.nOut))
        return keep(self, a, outer, inner)

    refinement.BandMap.apply_host = spy
    try:
        s.trim([[None, 0.999], [0.4, 0.6]])
    finally:
        refinement.BandMap.apply_host = keep
    assert len(calls) == 2 and calls[0][1] / calls[0][0] <= calls[1][1] / calls[1][0] and calls[0][0] == s.nCoef[1]


def test_last_paths_hold_the_last_call_only():
    """A call that returns the spline itself, or whose clamp step has nothing to do, must not keep an earlier call's paths."""
    rng = np.random.default_rng(27)
    s = surface(rng)
    refinement.LAST_PATHS[:] = ["band_apply", "band_apply_line"]          # what an earlier device call would leave
    assert s.trim([[None, None], [None, None]]) is s and refinement.LAST_PATHS == []
    refinement.LAST_PATHS[:] = ["band_apply_line"]
    s.elevate([1, 0], _path="host")                                        # already clamped: the clamp step runs nothing
    assert refinement.LAST_PATHS == ["host band"]
    refinement.LAST_PATHS[:] = ["band_apply_line"]
    assert s.elevate([0, 0]) is s and refinement.LAST_PATHS == []
    u = surface(rng, unclamped=True)
    u.elevate([1, 1], _path="host")                                        # clamp (two variables) + elevation (two)
    assert refinement.LAST_PATHS == 4 * ["host band"]


def test_differentiate_refuses_a_full_multiplicity_interior_knot():
    """alpha_j = (k - 1) / 0 there: the reference returns inf / nan coefficients, this library says what is wrong."""
    s = Spline(1, 1, (3,), (6,), [[0.0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1]], [[0.0, 1.0, 2.0, 5.0, 3.0, 1.0]])
    with pytest.raises(ValueError, match="full multiplicity"):
        s.differentiate(0)
    assert refinement.LAST_PATHS == []
