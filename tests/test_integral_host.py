"""Spline.integral without a GPU: the Gauss-Kronrod constants, the cells, argument checks, and the CPU
restatement of the quadrature (tests/integral_ref.py) against the reference's values and the analytic ones."""
import math
import os

import numpy as np
import pytest

from bspy_amd import Spline
from bspy_amd import integral as iq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "integral.npz")


def golden_cases():
    """[(case, spline, domain, integrand name, reference value)] of tests/golden/integral.npz."""
    g = np.load(GOLDEN)
    out = []
    for name in sorted({k.split("/")[0] for k in g.files}):
        order, ncoef, coefs = g[f"{name}/order"], g[f"{name}/ncoef"], g[f"{name}/coefs"]
        s = Spline(len(order), coefs.shape[0], order, ncoef, [g[f"{name}/knots{i}"] for i in range(len(order))], coefs)
        dom = g[f"{name}/domain"] if f"{name}/domain" in g.files else None
        for k in sorted(g.files):
            if k.startswith(f"{name}/value/"):
                out.append((name, s, dom, k.rsplit("/", 1)[1], float(g[k])))
    return out


def integrand(name):
    if name == "one":
        return None
    d = int(name[1:])
    return lambda x: x[d]


def quarter_arc():
    """The reference's circular_arc(1, 90) (order 5, 26 coefficients), from the golden file."""
    return next(c[1] for c in golden_cases() if c[0] == "arc")


def annulus():
    return next(c[1] for c in golden_cases() if c[0] == "annulus")


@pytest.mark.parametrize("p", range(23))
def test_kronrod15_exact_to_degree_22(p):
    exact = 0.0 if p % 2 else 2.0 / (p + 1)
    assert abs(math.fsum(iq.GK_WK * iq.GK_X ** p) - exact) <= 2e-16


@pytest.mark.parametrize("p", range(14))
def test_gauss7_exact_to_degree_13(p):
    exact = 0.0 if p % 2 else 2.0 / (p + 1)
    assert abs(math.fsum(iq.GK_WG * iq.GK_X ** p) - exact) <= 2e-16


def test_gauss7_nodes_embedded():
    x, w = np.polynomial.legendre.leggauss(7)
    np.testing.assert_allclose(iq.GK_X[1::2], x, rtol=0, atol=1e-15)          # (numpy's own rule is the less exact one)
    np.testing.assert_allclose(iq.GK_WG[1::2], w, rtol=0, atol=1e-14)
    assert not iq.GK_WG[0::2].any()


def test_cells_with_knot_multiplicity():
    knots = np.array([0, 0, 0, 0.25, 0.25, 0.5, 0.75, 0.75, 0.75, 1, 1, 1.0])
    s = Spline(1, 1, [3], [9], [knots], np.arange(9.0))
    lo, hi, span = iq.cells(s, iq.check_domain(s, None))[0]
    np.testing.assert_array_equal(lo, [0, 0.25, 0.5, 0.75])
    np.testing.assert_array_equal(hi, [0.25, 0.5, 0.75, 1])
    np.testing.assert_array_equal(span, [3, 5, 6, 9])
    for a, b, ix in zip(lo, hi, span):
        assert knots[ix - 1] <= a < b <= knots[ix]


def test_cells_of_a_domain_inside_spans():
    knots = np.array([0, 0, 0, 0.25, 0.25, 0.5, 0.75, 0.75, 0.75, 1, 1, 1.0])
    s = Spline(2, 1, [3, 3], [9, 9], [knots, knots], np.zeros((1, 9, 9)))
    per = iq.cells(s, iq.check_domain(s, [[0.1, 0.6], [0.3, 0.4]]))
    np.testing.assert_array_equal(per[0][0], [0.1, 0.25, 0.5])
    np.testing.assert_array_equal(per[0][1], [0.25, 0.5, 0.6])
    np.testing.assert_array_equal(per[0][2], [3, 5, 6])
    np.testing.assert_array_equal(per[1][0], [0.3])
    np.testing.assert_array_equal(per[1][1], [0.4])
    np.testing.assert_array_equal(per[1][2], [5])
    lo_hi, span = iq.regions(s, iq.check_domain(s, [[0.1, 0.6], [0.3, 0.4]]))
    assert lo_hi.shape == (3, 2, 2) and span.shape == (3, 2)
    # a domain end on a knot: the knot is a breakpoint once
    lo, hi, _ = iq.cells(s, iq.check_domain(s, [[0.25, 0.75], [0, 1]]))[0]
    np.testing.assert_array_equal(lo, [0.25, 0.5])
    np.testing.assert_array_equal(hi, [0.5, 0.75])


def test_split_keeps_spans_and_volume():
    lo_hi = np.array([[[0.0, 1.0], [2.0, 4.0]]])
    ch, sp = iq.split(lo_hi, np.array([[3, 7]], np.int32))
    assert ch.shape == (4, 2, 2) and (sp == [3, 7]).all()
    np.testing.assert_array_equal(ch[0], [[0, 0.5], [2, 3]])
    np.testing.assert_array_equal(ch[3], [[0.5, 1], [3, 4]])
    assert np.prod(ch[:, :, 1] - ch[:, :, 0], axis=1).sum() == 2.0


def test_domain_beyond_the_spline_raises():
    s = quarter_arc()
    with pytest.raises(ValueError, match="Can't integrate beyond the domain of the spline"):
        s.integral(domain=[[-0.1, 0.5]])
    with pytest.raises(ValueError, match="Can't integrate beyond the domain of the spline"):
        annulus().integral(domain=[[0, 1], [0.5, 1.01]])


def test_degenerate_domain_is_zero():
    assert quarter_arc().integral(domain=[[0.3, 0.3]]) == 0.0


def test_nind_4_not_implemented():
    k = np.array([0, 0, 1, 1.0])
    s = Spline(4, 1, [2] * 4, [2] * 4, [k] * 4, np.ones((1, 2, 2, 2, 2)))
    with pytest.raises(NotImplementedError, match="nInd 1 to 3"):
        s.integral()


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: f"{c[0]}-{c[3]}")
def test_reference_rule_against_golden(case):
    from integral_ref import integral_ref
    name, s, dom, f, ref = case
    v = integral_ref(s, integrand(f), dom)
    assert abs(v - ref) <= 1e-12 * max(1.0, abs(ref))


@pytest.mark.parametrize("which,f,exact", [
    ("arc", None, math.pi / 2), ("arc", "x0", 1.0), ("arc", "x1", 1.0),
    ("annulus", None, 0.75 * math.pi), ("annulus", "x0", 7 / 3), ("annulus", "x1", 7 / 3)])
def test_reference_rule_analytic(which, f, exact):
    from integral_ref import integral_ref
    s = quarter_arc() if which == "arc" else annulus()
    v = integral_ref(s, integrand(f) if f else None)
    assert abs(v - exact) <= 1e-12
