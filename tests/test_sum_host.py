"""
common_basis, add, subtract, translate, the + and - operators, integrate and contract without a GPU: the reference's
messages, identities, result knots and dtypes, and the host half of the library (bsk_band_apply_host,
bsk_sum_apply_host and bsk_scan_apply_host through ctypes, which make no HIP call) against the goldens of
tests/golden/sum.npz (written by tests/golden/make_golden_sum.py) and against the exact results of tests/sum_ref.py.
The device half is covered by tests/test_gpu_sum.py, which takes its helpers from here.

Bars, relative to the scale S of the operation:
  S                              add / subtract: max |a| + max |b| of the operands' coefficients (a refined operand is
                                 a convex combination of its coefficients); integrate: the largest sum of |g c| over a
                                 line; contract: max |c|
  float64 against exact          1e-12 (the project's parity bar).  For the running sum any association of n <= 4096
                                 terms is within (n + 2) 2^-53 S < 1e-12
  float32 against exact          2^-23: integrate and contract round once (2^-24) and the margin covers the float32
                                 weights; add rounds each refined operand once (2^-24 max |.| each) and the sum once
  against the reference          the same bar plus ref_dev, the reference's own recorded distance from exact
  "bad_*" cases                  the reference's elevation is off by 1e-9 there: pinned to the exact result only
"""
import json
import os

import numpy as np
import pytest

import oracle
import sum_ref
from bspy_amd import Spline, sums
from conftest import GOLDEN, observe

F32_BAR = 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sum.npz"))


def _names():
    with np.load(os.path.join(GOLDEN, "sum.npz")) as g:
        return sorted({k.split("/")[0] for k in g.files})


NAMES = _names()


def _operand(g, name, prefix):
    order = [int(o) for o in g[f"{name}/{prefix}order"]]
    return dict(order=order, knots=[g[f"{name}/{prefix}knots{i}"] for i in range(len(order))], coefs=g[f"{name}/{prefix}coefs"])


def load_case(g, name):
    c = dict(name=name, op=str(g[f"{name}/op"]), **_operand(g, name, ""), other=None, pairs=None,
             out_order=[int(o) for o in g[f"{name}/out_order"]], out_coefs=g[f"{name}/out_coefs"], ref_dev=float(g[f"{name}/ref_dev"]))
    c["out_knots"] = [g[f"{name}/out_knots{i}"] for i in range(len(c["out_order"]))]
    if f"{name}/b_order" in g.files:
        c["other"] = _operand(g, name, "b_")
    if f"{name}/pairs" in g.files:
        c["pairs"] = [(int(p[0]), int(p[1])) for p in g[f"{name}/pairs"]]
        c["indMap"] = [p[0] if scalar else p for p, scalar in zip(c["pairs"], g[f"{name}/scalar"])]
    if f"{name}/wrt" in g.files:
        c["wrt"] = int(g[f"{name}/wrt"])
    if f"{name}/uvw" in g.files:
        c["uvw"] = [None if np.isnan(u) else float(u) for u in g[f"{name}/uvw"]]
    return c


def make_spline(s, metadata={}):
    return Spline(len(s["order"]), np.shape(s["coefs"])[0], s["order"], np.shape(s["coefs"])[1:], s["knots"], s["coefs"], metadata)


def run_case(c, path, **kwargs):
    s = make_spline(c)
    if c["op"] in ("add", "subtract"):
        return getattr(s, c["op"])(make_spline(c["other"]), c.get("indMap"), _path=path)
    if c["op"] == "integrate":
        return s.integrate(c["wrt"], _path=path, **kwargs)
    return s.contract(c["uvw"], _path=path)


_EXACT = {}


def exact_of(c):
    """(exact result rounded once to the result's dtype, the scale S), per case once a session."""
    if c["name"] not in _EXACT:
        dtype = c["out_coefs"].dtype
        if c["op"] in ("add", "subtract"):
            e = sum_ref.add(c, c["other"], c["pairs"], c["out_order"], c["out_knots"], 1 if c["op"] == "add" else -1, dtype)
            scale = float(np.abs(c["coefs"]).max() + np.abs(c["other"]["coefs"]).max())
        elif c["op"] == "integrate":
            e, scale = sum_ref.integrate(c["order"], c["knots"], c["coefs"], c["wrt"], dtype)
        else:
            e = sum_ref.contract(c["order"], c["knots"], c["coefs"], c["uvw"], dtype)
            scale = float(np.abs(c["coefs"]).max())
        _EXACT[c["name"]] = (e, scale)
    return _EXACT[c["name"]]


def check_golden(c, r, label):
    """The result r of case c against the golden: orders and knots bit for bit, coefficients at the bars of the header."""
    assert list(r.order) == c["out_order"] and r.nInd == len(c["out_order"])
    assert r.coefs.dtype == c["out_coefs"].dtype and r.coefs.shape == c["out_coefs"].shape
    for got, want in zip(r.knots, c["out_knots"]):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), f"{c['name']}: knots differ from the reference's"
    exact, scale = exact_of(c)
    ours = np.asarray(r.coefs, np.float64)
    err_exact = float(np.abs(ours - exact.astype(np.float64)).max() / scale)
    err_ref = float(np.abs(ours - np.asarray(c["out_coefs"], np.float64)).max() / scale)
    ref_dev = c["ref_dev"] * float(np.abs(exact).max()) / scale                  # recorded relative to max |exact|
    print(f"{label} {c['name']}: against exact {err_exact:.3e}, against the reference {err_ref:.3e}, ref_dev {ref_dev:.3e}")
    fp32 = r.coefs.dtype == np.float32
    bar = F32_BAR if fp32 else 1e-12
    observe(f"{label} {c['op']} {'fp32' if fp32 else 'fp64'} against exact", err_exact, bar)
    if c["name"].startswith("bad_"):
        assert c["ref_dev"] > 1e-12, "a bad case must be one the reference misses"
        assert err_exact < ref_dev
    else:
        assert err_ref <= bar + ref_dev


# ------------------------------------------------------------------------------------------ goldens, host path
def host_kernels(c):
    if c["op"] in ("add", "subtract"):
        return {"host sum"} | ({"host band"} if c["pairs"] else set())
    return {"host scan"} if c["op"] == "integrate" else {"host band"}


@pytest.mark.parametrize("name", NAMES)
def test_golden_host(golden, name):
    c = load_case(golden, name)
    r = run_case(c, "host")
    assert set(sums.LAST_PATHS) == host_kernels(c) and sums.LAST_PATHS[-1] in ("host sum", "host scan", "host band")
    check_golden(c, r, "sum host")


def test_golden_file_keeps_the_reference_comparison_alive(golden):
    by_op = {}
    for name in NAMES:
        c = load_case(golden, name)
        if c["coefs"].dtype == np.float64:
            by_op.setdefault(c["op"], []).append(c["ref_dev"])
    assert set(by_op) == {"add", "subtract", "integrate", "contract"}
    for op, devs in by_op.items():
        assert 2 * sum(d <= 1e-12 for d in devs) >= len(devs), op
    assert sum(n.startswith("bad_") for n in NAMES) == 2


# ------------------------------------------------------------------------------------------ messages, identities, small results
def _semantics():
    with open(os.path.join(GOLDEN, "sum_semantics.json")) as f:
        return json.load(f)


def _same(r, want, spline):
    assert isinstance(r, Spline) and list(r.order) == want["order"] and r.metadata == {"tag": 7}
    assert r.coefs.dtype == spline.coefs.dtype
    for got, expected in zip(r.knots, want["knots"]):
        assert np.array_equal(got, expected)
    expected = np.array(want["coefs"])
    assert r.coefs.shape == expected.shape
    assert np.abs(r.coefs - expected).max() <= 1e-12 * max(1.0, np.abs(expected).max())


@pytest.mark.parametrize("record", _semantics(), ids=lambda r: r["name"])
def test_reference_messages_identities_and_small_results(record):
    spline = make_spline(record["spline"], {"tag": 7})
    other = make_spline(record["other"], {"tag": 7}) if record["other"] is not None else None
    if record["op"] == "common_basis":
        call = lambda: Spline.common_basis((spline, other), *record["args"])
    else:
        call = lambda: getattr(spline, record["op"])(*(([other] if other is not None else []) + record["args"]))
    if record["error"] is not None:
        with pytest.raises(ValueError) as info:
            call()
        assert str(info.value) == record["error"]
        return
    r = call()
    if record["op"] == "common_basis":
        assert (r[0] is spline) == record["is_self"]
        for one, want, source in zip(r, record["result"], (spline, other)):
            _same(one, want, source)
    else:
        assert (r is spline) == record["is_self"]
        if not record["is_self"]:
            _same(r, record["result"], spline)


def test_path_argument_is_checked():
    s = Spline(1, 1, (2,), (3,), [[0.0, 0, 0.5, 1, 1]], [[0.0, 1.0, 3.0]])
    for call in (lambda: s.integrate(0, _path="gpu"), lambda: s.add(s, [0], _path="gpu"), lambda: s.contract([0.5], _path="gpu")):
        with pytest.raises(ValueError, match="_path"):
            call()


# ------------------------------------------------------------------------------------------ operator checks
def random_knots(rng, order, ncoef, unclamped=False):
    if unclamped:
        return np.sort(rng.random(order + ncoef) * 3.0 - 1.0)
    return np.concatenate((order * [0.0], np.sort(rng.random(ncoef - order)), order * [1.0]))


def surface(rng, order=(4, 3), ncoef=(13, 11), dtype=np.float64, ndep=3):
    knots = [random_knots(rng, o, n) for o, n in zip(order, ncoef)]
    return Spline(2, ndep, order, ncoef, knots, rng.standard_normal((ndep, *ncoef)).astype(dtype))


def values(s, points):
    v, bad = oracle.c_evaluate(list(s.order), list(s.nCoef), [np.asarray(k, np.float64) for k in s.knots],
                               np.asarray(s.coefs, np.float64), [0] * s.nInd, points)
    assert bad == -1
    return v


def test_differentiate_of_integrate_is_the_spline():
    rng = np.random.default_rng(31)
    s = surface(rng)
    for iv in range(2):
        back = s.integrate(iv, _path="host").differentiate(iv, _path="host")
        assert back.order == s.order and all(np.array_equal(a, b) for a, b in zip(back.knots, s.knots))
        observe("sum differentiate(integrate)", np.abs(back.coefs - s.coefs).max() / np.abs(s.coefs).max(), 1e-12)


def test_last_coefficient_of_an_integrated_clamped_curve_is_the_weighted_sum():
    rng = np.random.default_rng(32)
    t = random_knots(rng, 4, 40)
    c = rng.standard_normal((2, 40))
    r = Spline(1, 2, (4,), (40,), [t], c).integrate(_path="host")
    g = sum_ref.weights(t, 4)
    assert np.all(r.coefs[:, 0] == 0.0)
    observe("sum integral of a clamped curve", np.abs(r.coefs[:, -1] - (g * c).sum(axis=1)).max() / np.abs(g * c).sum(axis=1).max(), 1e-12)


def test_contract_of_all_variables_is_the_value():
    rng = np.random.default_rng(33)
    s = surface(rng)
    for uv in ((0.3, 0.8), (1.0, 0.0), (float(s.knots[0][6]), 0.5)):
        r = s.contract(list(uv), _path="host")
        assert r.nInd == 0 and r.coefs.shape == (3,) and sums.LAST_PATHS == ["host band", "host band"]
        want = values(s, [np.array([uv[0]]), np.array([uv[1]])])[:, 0]
        observe("sum contract against the oracle", np.abs(r.coefs - want).max() / np.abs(s.coefs).max(), 1e-12)


def test_add_then_subtract_has_the_first_function():
    rng = np.random.default_rng(34)
    a, b = surface(rng), surface(rng, (3, 4), (9, 12))
    r = (a + b) - b
    assert r.order == (4, 4)
    pts = [rng.random(300), rng.random(300)]
    scale = np.abs(a.coefs).max() + np.abs(b.coefs).max()
    observe("sum (a + b) - b by evaluation", np.abs(values(r, pts) - values(a, pts)).max() / scale, 1e-12)
    observe("sum a + b by evaluation", np.abs(values(a + b, pts) - values(a, pts) - values(b, pts)).max() / scale, 1e-12)


def test_subtract_is_add_of_the_negated_operand_bit_for_bit():
    rng = np.random.default_rng(35)
    a, b = surface(rng), surface(rng, (3, 4), (9, 12))
    assert a.subtract(b, [0, 1], _path="host").coefs.tobytes() == a.add(b.scale(-1.0), [0, 1], _path="host").coefs.tobytes()
    assert a.subtract(b, _path="host").coefs.tobytes() == a.add(-b, _path="host").coefs.tobytes()


def test_scan_map_apply_line_is_the_host_driver():
    rng = np.random.default_rng(36)
    for n in (1, 31, 32, 33, 100):
        scan = sums.ScanMap(rng.random(n) - 0.3)
        for dtype in (np.float64, np.float32):
            a = rng.standard_normal((3, n, 4)).astype(dtype)
            got = scan.apply_host(a, 3, 4)
            assert got.dtype == dtype and got.shape == (3, n + 1, 4) and scan.last_kernel() == "host scan"
            for o in range(3):
                for i in range(4):
                    assert np.array_equal(got[o, :, i], scan.apply_line(a[o, :, i]))
        scan.close()


def test_sum_layout_merges_axes_and_host_sum_takes_any_view():
    rng = np.random.default_rng(37)
    a, b = rng.standard_normal((3, 4, 5, 1, 1)), rng.standard_normal((3, 4, 1, 6, 7))
    shape, dim, sa, sb = sums.sum_layout(a, b)
    assert (shape, dim, sa, sb) == ([3, 4, 5, 6, 7], [12, 5, 42], [5, 1, 0], [42, 0, 1])
    assert np.array_equal(sums._add_host(a, b, -1), a - b)
    swapped = rng.standard_normal((3, 7, 4)).transpose(0, 2, 1)                      # a view whose last stride is not 1
    assert np.array_equal(sums._add_host(swapped[:, :, None, :], b[:, :, 0, :, :], 1), swapped[:, :, None, :] + b[:, :, 0, :, :])
    for dtype in (np.float32, np.float64):
        x, y = rng.standard_normal((1, 9)).astype(dtype), rng.standard_normal((5, 1)).astype(dtype)
        want = (x.astype(np.float64) + y.astype(np.float64)).astype(dtype)
        assert np.array_equal(sums._add_host(x, y, 1), want)


def test_float32_keeps_dtype_and_metadata_and_mixed_types_follow_self():
    rng = np.random.default_rng(38)
    s, d = surface(rng, dtype=np.float32), surface(rng, (3, 4), (9, 12))
    s.metadata["name"] = "patch"
    for r in (s + d, s - d, s.integrate(1), s + [1.0, 2.0, 3.0], s.add(d)):
        assert r.coefs.dtype == np.float32 and r.metadata == {"name": "patch"}
    # contract multiplies by B-spline values of the knots' type: float64 knots promote, as the reference's matmul does
    assert s.contract([0.5, None]).coefs.dtype == np.float64
    single = Spline(2, 3, s.order, s.nCoef, [k.astype(np.float32) for k in s.knots], s.coefs)
    assert single.contract([0.5, None]).coefs.dtype == np.float32
    assert (d + s).coefs.dtype == np.float64
    with pytest.raises(ValueError, match="one coefficient dtype"):
        s.add(d, [0, 1], _path="device")


def test_small_results_take_the_host_drivers():
    rng = np.random.default_rng(39)
    a, b = surface(rng), surface(rng, (3, 4), (9, 12))
    a + b
    assert sums.LAST_PATHS == 4 * ["host band"] + ["host sum"]
    a.integrate(0)
    assert sums.LAST_PATHS == ["host scan"]
    a.contract([None, 0.5])
    assert sums.LAST_PATHS == ["host band"]
    assert a.contract([None, None]) is a and sums.LAST_PATHS == []
    line = Spline(1, 1, (1,), (2,), [[0.0, 0.5, 1.0]], [[1.0, 2.0]])
    assert line.contract([0.75]).coefs[0] == 2.0 and sums.LAST_PATHS == ["host band"]       # order 1: the host driver
    with pytest.raises(ValueError, match="device path covers K"):
        line.contract([0.75], _path="device")
