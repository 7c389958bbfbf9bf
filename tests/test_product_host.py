"""
Spline.multiply, dot, cross, scale, transform and the operators without a GPU: the knot rule, the reference's messages,
the bilinear operator's properties, and the host half of the library (bsk_product_apply_host through ctypes, which makes
no HIP call) against the goldens of tests/golden/product.npz (written by tests/golden/make_golden_product.py) and against
the exact products of tests/product_ref.py.  The device half is covered by tests/test_gpu_product.py, which takes its
helpers from here.

Bars, relative to S = nTerms x max |self.coefs| x max |other.coefs| (nTerms: 'S' 1, 'D' nDep, 'C' 2):
  against the exact result       1e-12 (the parity bar of tests/test_gpu_parity.py); observed values are recorded
  against the reference          max(1e-12, 10 x ref_dev), ref_dev = the reference's own recorded distance from exact
  "uneq_*" and "hi_*" cases      orders that differ in a mapped variable (the reference is off by 1e-5 .. 1) and orders
                                 6 x 6, 8 x 8: pinned to the exact result only, and our error must be below ref_dev
  float32                        2^-23 against the exact result rounded to float32 (the sums run in fp64 and round once);
                                 against the reference max(2^-23, 10 x ref_dev)
The exact result is computed here by product_ref but for the hi_* cases, whose exact rows take a minute: those take the
array the generator stored from the same function.
"""
import json
import os

import numpy as np
import pytest

import oracle
import product_ref
from bspy_amd import Spline, product
from conftest import GOLDEN, observe

EPS = np.finfo(np.float64).eps
F32_ULP = 2.0 ** -23
N_TERMS = {"S": lambda n: 1, "D": lambda n: n, "C": lambda n: 2}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "product.npz"))


def _names():
    with np.load(os.path.join(GOLDEN, "product.npz")) as g:
        return sorted({k.split("/")[0] for k in g.files})


NAMES = _names()


def load_case(g, name):
    c = dict(name=name, ptype=str(g[f"{name}/ptype"]), ref_dev=float(g[f"{name}/ref_dev"]), stored_exact=g[f"{name}/exact"],
             out_order=[int(o) for o in g[f"{name}/out_order"]], out_coefs=g[f"{name}/out_coefs"])
    for tag in ("1", "2"):
        order = [int(o) for o in g[f"{name}/order{tag}"]]
        c["order" + tag] = order
        c["knots" + tag] = [g[f"{name}/knots{tag}_{i}"] for i in range(len(order))]
        c["coefs" + tag] = g[f"{name}/coefs{tag}"]
    c["out_knots"] = [g[f"{name}/out_knots{i}"] for i in range(len(c["out_order"]))]
    c["pairs"], c["map"] = [], None
    if f"{name}/map" in g.files:
        c["pairs"] = [(int(a), int(b)) for a, b in g[f"{name}/map"]]
        c["map"] = [p[0] if one else p for p, one in zip(c["pairs"], g[f"{name}/scalar"])]
    c["scale"] = N_TERMS[c["ptype"]](c["coefs1"].shape[0]) * float(np.abs(c["coefs1"]).max()) * float(np.abs(c["coefs2"]).max())
    return c


def make_splines(c):
    return tuple(Spline(len(c["order" + t]), c["coefs" + t].shape[0], c["order" + t], c["coefs" + t].shape[1:], c["knots" + t],
                        c["coefs" + t]) for t in ("1", "2"))


def run_case(c, path):
    a, b = make_splines(c)
    return a.multiply(b, c["map"], c["ptype"], _path=path)


_EXACT = {}


def exact_of(c):
    """The exact product rounded once to the result's dtype, per case once a session."""
    if c["name"] not in _EXACT:
        if c["name"].startswith("hi_"):
            _EXACT[c["name"]] = c["stored_exact"]
        else:
            new_knots = [c["out_knots"][p[0]] for p in c["pairs"]]
            _EXACT[c["name"]] = product_ref.multiply(c["order1"], c["knots1"], c["coefs1"], c["order2"], c["knots2"], c["coefs2"],
                                                     c["pairs"], c["ptype"], new_knots, c["out_coefs"].dtype)
            assert np.array_equal(_EXACT[c["name"]], c["stored_exact"]), "the stored exact result is not product_ref's"
    return _EXACT[c["name"]]


def check_golden(c, r, label):
    """The result r of case c against the golden: knots bit for bit, coefficients at the bars of this file's header."""
    assert list(r.order) == c["out_order"] and r.nDep == c["out_coefs"].shape[0]
    assert r.coefs.dtype == c["out_coefs"].dtype and r.coefs.shape == c["out_coefs"].shape and r.nCoef == c["out_coefs"].shape[1:]
    for got, want in zip(r.knots, c["out_knots"]):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), f"{c['name']}: knots differ from the reference's"
    exact = exact_of(c)
    ours = np.asarray(r.coefs, np.float64)
    err_exact = float(np.abs(ours - exact.astype(np.float64)).max() / c["scale"])
    err_ref = float(np.abs(ours - np.asarray(c["out_coefs"], np.float64)).max() / c["scale"])
    print(f"{label} {c['name']}: against exact {err_exact:.3e}, against the reference {err_ref:.3e}, ref_dev {c['ref_dev']:.3e}")
    if r.coefs.dtype == np.float32:
        observe(f"{label} fp32 against exact", err_exact, F32_ULP)
        assert err_ref <= max(F32_ULP, 10.0 * c["ref_dev"])
        return
    observe(f"{label} fp64 against exact", err_exact, 1e-12)
    if c["name"].startswith(("uneq_", "hi_")):
        assert err_exact < c["ref_dev"]
    else:
        assert err_ref <= max(1e-12, 10.0 * c["ref_dev"])


# ------------------------------------------------------------------------------------------ goldens, host path
@pytest.mark.parametrize("name", NAMES)
def test_golden_host(golden, name):
    c = load_case(golden, name)
    r = run_case(c, "host")
    assert product.LAST_PATHS == (["host product"] if c["pairs"] else ["outer"])
    check_golden(c, r, "product host")


def test_golden_file_keeps_the_reference_comparison_alive(golden):
    by_type, uneq = {}, []
    for name in NAMES:
        c = load_case(golden, name)
        bar = 1e-12 if c["out_coefs"].dtype == np.float64 else 1e-12 * 2.0 ** 29
        by_type.setdefault(c["ptype"], []).append(c["ref_dev"] <= bar)
        assert name.startswith(("uneq_", "hi_")) or c["ref_dev"] <= bar, name
        if name.startswith("uneq_"):
            uneq.append(c["ref_dev"])
    assert set(by_type) == {"S", "D", "C"}
    for ptype, good in by_type.items():
        assert 2 * sum(good) >= len(good), ptype
    assert len(uneq) >= 5 and min(uneq) > 1e-6, "the uneq cases are the ones the reference misses"


# ------------------------------------------------------------------------------------------ messages and identities
def _semantics():
    with open(os.path.join(GOLDEN, "product_semantics.json")) as f:
        return json.load(f)


def _spline(s, tag):
    dtype = np.dtype(s.get("dtype", "float64"))
    coefs = np.array(s["coefs"], dtype)
    return Spline(len(s["order"]), len(coefs), s["order"], coefs.shape[1:], [np.array(k, dtype) for k in s["knots"]], coefs,
                  metadata={"tag": tag})


@pytest.mark.parametrize("record", _semantics(), ids=lambda r: r["name"])
def test_reference_messages_and_identities(record):
    a, b = _spline(record["a"], 1), _spline(record["b"], 2)
    indMap = None if record["map"] is None else [m if np.isscalar(m) else tuple(m) for m in record["map"]]
    if record["error"] is not None:
        with pytest.raises(ValueError) as info:
            a.multiply(b, indMap, record["ptype"])
        assert str(info.value) == record["error"]
        return
    r = a.multiply(b, indMap, record["ptype"])
    assert isinstance(r, Spline) and r.nDep == record["nDep"] and list(r.order) == record["order"] and list(r.nCoef) == record["nCoef"]
    assert [str(k.dtype) for k in r.knots] == record["knots_dtype"] and r.metadata == record["metadata"] == {"tag": 1}
    if not (record["a"].get("dtype") != record["b"].get("dtype") and len(record["b"]["coefs"]) == 1 < len(record["a"]["coefs"])):
        assert str(r.coefs.dtype) == record["coefs_dtype"]


def test_same_variable_mapped_twice():
    s = Spline(2, 1, (2, 2), (2, 2), [[0.0, 0, 1, 1]] * 2, np.ones((1, 2, 2)))
    c = Spline(1, 1, (2,), (2,), [[0.0, 0, 1, 1]], np.ones((1, 2)))
    with pytest.raises(ValueError, match="You can't map the same independent variable to multiple others."):
        s.multiply(c, [(0, 0), (1, 0)])
    with pytest.raises(NotImplementedError, match="at most 3"):
        q = Spline(4, 1, (2,) * 4, (2,) * 4, [[0.0, 0, 1, 1]] * 4, np.ones((1, 2, 2, 2, 2)))
        q.multiply(q, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="_path"):
        c.multiply(c, [0], _path="gpu")
    assert not hasattr(Spline, "convolve")


# ------------------------------------------------------------------------------------------ the operator
def random_knots(rng, order, ncoef, unclamped=False):
    if unclamped:
        t = np.sort(rng.random(order + ncoef))
        return (t - t[order - 1]) / (t[ncoef] - t[order - 1])                 # the domain is [0, 1]
    interior = np.sort(rng.random(ncoef - order))
    if ncoef - order > 4 and order > 1:
        interior[2] = interior[1]                   # a double knot
    return np.concatenate((order * [0.0], interior, order * [1.0]))


def check_operator(f, g, W, k1, n1, k2, n2):
    assert W.shape[1:] == (k1, k2)
    for first, k, n in ((f, k1, n1), (g, k2, n2)):
        assert np.all(np.diff(first) >= 0) and first[0] >= 0 and first[-1] + k <= n
    assert np.abs(W.sum(axis=(1, 2)) - 1.0).max() <= 64 * EPS
    assert W.min() >= -64 * EPS


def test_operator_properties_random():
    rng = np.random.default_rng(31)
    seen = set()
    for trial in range(40):
        k1, k2 = (int(rng.integers(1, 9)), int(rng.integers(1, 9))) if trial >= 2 else ((8, 8), (1, 8))[trial]
        seen.add((k1, k2))
        n1, n2 = k1 + int(rng.integers(0, 64 // (k1 + k2))), k2 + int(rng.integers(0, 64 // (k1 + k2)))
        t = random_knots(rng, k1, n1, unclamped=trial % 5 == 4)
        s = random_knots(rng, k2, n2)
        if trial % 3 == 0 and n2 - k2 > 1 and n1 - k1 > 1:
            s[k2] = t[k1 + 1]                        # a shared knot
            s[k2:n2] = np.sort(s[k2:n2])
        if trial % 5 == 4:
            s[:k2], s[n2:] = t[k1 - 1], t[n1]
        tbar = product.product_knots(t, k1, s, k2)
        f, g, W = product.product_map(t, k1, s, k2, tbar)
        assert len(f) == len(tbar) - (k1 + k2 - 1) and tbar[0] == tbar[k1 + k2 - 2] and tbar[-1] == tbar[-(k1 + k2 - 1)]
        check_operator(f, g, W, k1, n1, k2, n2)
    assert (8, 8) in seen and len(seen) > 20


def test_operator_rows_are_the_exact_rows(golden):
    for name in ("cur_o4_S13", "cur_o3_shared_repeated", "uneq_o35", "cur_o4_unclamped"):
        c = load_case(golden, name)
        k1, k2, t, s, tbar = c["order1"][0], c["order2"][0], c["knots1"][0], c["knots2"][0], c["out_knots"][0]
        f, g, W = product.product_map(t, k1, s, k2, tbar)
        dense = np.zeros((len(f), len(t) - k1, len(s) - k2))
        for j in range(len(f)):
            dense[j, f[j]:f[j] + k1, g[j]:g[j] + k2] = W[j]
        for j, (fe, ge, We, den) in enumerate(product_ref.product_rows(t, k1, s, k2, tbar)):
            want = np.zeros(dense.shape[1:])
            want[fe:fe + k1, ge:ge + k2] = [[w / den for w in row] for row in We]
            # the two sides may stand on different cells of the support; on a shared knot line the same bilinear form
            # is then written on other coefficients, so compare where both use the same window
            if (fe, ge) == (f[j], g[j]):
                assert np.abs(dense[j] - want).max() <= 64 * EPS, (name, j)


def test_operator_is_the_mean_over_subsets_of_blossom_products():
    """W[j][a][b] = C(p - 1, k1 - 1)^-1 sum_S D1_S[a] D2_S'[b] with refinement's recurrence, subset by subset."""
    import itertools
    from bspy_amd.refinement import blossom_weights
    rng = np.random.default_rng(38)
    for k1, k2 in ((1, 4), (2, 2), (3, 5), (4, 4), (6, 3)):
        t, s = random_knots(rng, k1, k1 + 7), random_knots(rng, k2, k2 + 5)
        tbar = product.product_knots(t, k1, s, k2)
        f, g, W = product.product_map(t, k1, s, k2, tbar)
        n, j = k1 + k2 - 2, np.arange(len(f))
        tl, sl, tb = t.astype(np.longdouble), s.astype(np.longdouble), tbar.astype(np.longdouble)
        want, count = np.zeros(W.shape, np.longdouble), 0
        for subset in itertools.combinations(range(n), k1 - 1):
            rest = [i for i in range(n) if i not in subset]
            d1 = blossom_weights(tl, k1, f.astype(np.int64), tb[j[:, None] + 1 + np.array(subset, np.int64)])
            d2 = blossom_weights(sl, k2, g.astype(np.int64), tb[j[:, None] + 1 + np.array(rest, np.int64)])
            want += d1[:, :, None] * d2[:, None, :]
            count += 1
        assert np.abs(W - (want / count).astype(np.float64)).max() <= 4 * EPS


def test_product_map_apply_line_is_the_host_driver():
    rng = np.random.default_rng(32)
    t, s = random_knots(rng, 4, 30), random_knots(rng, 3, 17)
    maps, _ = product.ProductMap.from_knots([(t, 4, s, 3)])
    terms = product.plane_table(product.dependent_terms("S", 3, 3))
    for dtype in (np.float64, np.float32):
        a, b = rng.standard_normal((3, 30)).astype(dtype), rng.standard_normal((3, 17)).astype(dtype)
        got = maps.apply_host(a, b, terms)
        assert got.dtype == dtype and maps.last_kernel() == "host product"
        for d in range(3):
            assert np.array_equal(got[d], maps.apply_line(a[d], b[d]))
    with pytest.raises(product.nv.BskError, match="plane outside"):
        maps.apply_host(a, b, np.array([[[0, 3, 1]]], np.int32))
    maps.close()


# ------------------------------------------------------------------------------------------ meaning, through the oracle
def values(s, points):
    v, bad = oracle.c_evaluate(list(s.order), list(s.nCoef), [np.asarray(k, np.float64) for k in s.knots],
                               np.asarray(s.coefs, np.float64), [0] * s.nInd, points)
    assert bad == -1
    return v


def combine(ptype, va, vb):
    if ptype == "D":
        return (va * vb).sum(axis=0, keepdims=True)
    if ptype == "C":
        return np.cross(va.T, vb.T).T if len(va) == 3 else (va[0] * vb[1] - va[1] * vb[0])[None]
    return va * vb


@pytest.mark.parametrize("name", ["cur_o5_S33", "cur_o4_unclamped", "surf_both_C", "surf_swapped_D", "surf_partial", "vol_x_surf_partial",
                                  "surf_none", "tri_all_D", "uneq_o46", "uneq_surf_o3443", "hi_o88", "surf_x_curve"])
def test_result_is_the_product_of_the_values(golden, name):
    c = load_case(golden, name)
    a, b = make_splines(c)
    r = run_case(c, "host")
    rng = np.random.default_rng(33)
    free2 = [v for v in range(b.nInd) if v not in [p[1] for p in c["pairs"]]]
    assert r.nInd == a.nInd + len(free2)
    pts = [lo + (hi - lo) * rng.random(300) for lo, hi in r.domain()]
    pts_b = [None] * b.nInd
    for i1, i2 in c["pairs"]:
        pts_b[i2] = pts[i1]
    for n, v in enumerate(free2):
        pts_b[v] = pts[a.nInd + n]
    want = combine(c["ptype"], values(a, pts[:a.nInd]), values(b, pts_b))
    observe("product meaning: result(u) against self(u) o other(u)", np.abs(values(r, pts) - want).max() / c["scale"], 1e-12)


# ------------------------------------------------------------------------------------------ ties to existing code
def test_multiply_by_one_is_elevate():
    rng = np.random.default_rng(34)
    s = Spline(2, 3, (4, 3), (12, 9), [random_knots(rng, 4, 12), random_knots(rng, 3, 9)], rng.standard_normal((3, 12, 9)))
    for m in (1, 2):
        one = Spline(1, 1, (m + 1,), (m + 1,), [np.concatenate(((m + 1) * [0.0], (m + 1) * [1.0]))], np.ones((1, m + 1)))
        r, e = s.multiply(one, [(1, 0)], _path="host"), s.elevate([0, m], _path="host")
        assert r.order == e.order and all(np.array_equal(x, y) for x, y in zip(r.knots, e.knots))
        observe("product by one against elevate", np.abs(r.coefs - e.coefs).max() / np.abs(s.coefs).max(), 1e-12)


def test_product_commutes():
    rng = np.random.default_rng(35)
    a = Spline(1, 3, (4,), (11,), [random_knots(rng, 4, 11)], rng.standard_normal((3, 11)))
    b = Spline(1, 3, (3,), (9,), [random_knots(rng, 3, 9)], rng.standard_normal((3, 9)))
    ab, ba = a * b, b * a
    assert ab.order == ba.order == (6,) and np.array_equal(ab.knots[0], ba.knots[0])
    scale = np.abs(a.coefs).max() * np.abs(b.coefs).max()
    observe("product a * b against b * a", np.abs(ab.coefs - ba.coefs).max() / scale, 1e-12)
    observe("product a x b against -(b x a)", np.abs(a.cross(b).coefs + b.cross(a).coefs).max() / (2 * scale), 1e-12)


# ------------------------------------------------------------------------------------------ operators and the thin forms
def test_operators_route_as_the_reference_does():
    rng = np.random.default_rng(36)
    t = random_knots(rng, 3, 8)
    a = Spline(1, 3, (3,), (8,), [t], rng.standard_normal((3, 8)), metadata={"n": 1})
    b = Spline(1, 3, (3,), (8,), [t], rng.standard_normal((3, 8)))
    one = Spline(1, 1, (3,), (8,), [t], rng.standard_normal((1, 8)))
    vec, mat = np.array([1.0, -2.0, 0.5]), rng.standard_normal((2, 3))
    same = lambda x, y: x.nDep == y.nDep and x.order == y.order and np.array_equal(x.coefs, y.coefs) and x.metadata == y.metadata
    assert same(a * b, a.multiply(b, [0], "S")) and same(a @ b, a.multiply(b, [0], "D")) and (a @ b).nDep == 1
    assert same(a * 2.0, a.scale(2.0)) and same(2.0 * a, a.scale(2.0)) and np.array_equal((a * 2.0).coefs, 2.0 * a.coefs)
    assert same(np.float64(2.0) * a, a.scale(2.0))
    assert same(a * vec, a.scale(vec)) and np.array_equal((a * vec).coefs, a.coefs * vec[:, None])
    assert (one * vec).nDep == 3 and np.array_equal((one * vec).coefs, vec[:, None] * one.coefs)
    assert same(-a, a.scale(-1.0)) and same(a / 4.0, a.scale(0.25))
    assert same(a @ vec, a.dot(vec)) and same(vec @ a, a.dot(vec)) and (a @ vec).nDep == 1
    assert np.allclose((a @ vec).coefs[0], np.tensordot(vec, a.coefs, 1))
    assert same(mat @ a, a.transform(mat)) and same(a @ mat.T, a.transform(mat)) and (mat @ a).nDep == 2
    assert np.allclose((mat @ a).coefs, np.tensordot(mat, a.coefs, 1))
    assert same(a.cross(b), a.multiply(b, [0], "C")) and same(a.dot(b), a @ b) and same(a.scale(one), a.multiply(one, [0], "S"))
    assert np.allclose(a.cross(vec).coefs, np.cross(a.coefs.T, vec).T)
    flat = Spline(1, 2, (3,), (8,), [t], rng.standard_normal((2, 8)))
    assert flat.cross([3.0, 5.0]).nDep == 1 and np.allclose(flat.cross([3.0, 5.0]).coefs[0], 5.0 * flat.coefs[0] - 3.0 * flat.coefs[1])
    for call, message in ((lambda: a / vec, "Divisor must be a scalar"), (lambda: a.dot([1.0, 2.0]), "Invalid vector"),
                          (lambda: a.cross([1.0, 2.0]), "Invalid vector"), (lambda: a.scale([1.0, 2.0]), "Invalid multiplier"),
                          (lambda: a.transform(np.ones((2, 2))), "Invalid matrix"), (lambda: (one * one).cross([1.0]), "Invalid nDep")):
        with pytest.raises(ValueError) as info:
            call()
        assert str(info.value) == message
    assert (a * 2.0).metadata == {"n": 1} and (a * b).metadata == {"n": 1} and (b * a).metadata == {}


# ------------------------------------------------------------------------------------------ dispatch
def test_dispatch():
    rng = np.random.default_rng(37)
    t7 = random_knots(rng, 7, 10)
    big = Spline(1, 1, (7,), (10,), [t7], rng.standard_normal((1, 10)))
    with pytest.raises(ValueError, match="device path covers"):
        big.multiply(big, [0], _path="device")
    keep, product.DEVICE_MIN_ELEMENTS = product.DEVICE_MIN_ELEMENTS, 1
    try:
        big.multiply(big, [0])                      # even when the size asks for the device
        assert product.LAST_PATHS == ["host product"]
    finally:
        product.DEVICE_MIN_ELEMENTS = keep
    small = Spline(1, 1, (3,), (6,), [random_knots(rng, 3, 6)], rng.standard_normal((1, 6)))
    small.multiply(small, [0])
    assert product.LAST_PATHS == ["host product"]
    small.multiply(small)
    assert product.LAST_PATHS == ["outer"]
