"""Spline.integral on the MI355X (bsk_integral): the reference's values, exact cases, cases beyond the reference's
reach against the CPU restatement (tests/integral_ref.py), fp32, domains, callables and reproducibility."""
import math
import warnings

import numpy as np
import pytest

import cases
from bspy_amd import Spline
from bspy_amd import integral as iq
from integral_ref import integral_ref
from test_integral_host import annulus, golden_cases, integrand, quarter_arc

pytestmark = pytest.mark.gpu


def close(v, ref, rel):
    assert abs(v - ref) <= rel * max(1.0, abs(ref)), f"{v!r} vs {ref!r}: {abs(v - ref) / max(1.0, abs(ref)):.2e}"


def spline_of(order, ncoef, coefs, lo=0.0, hi=1.0, dtype=np.float64):
    knots = [cases.clamped_uniform_knots(o, c, dtype, lo, hi) for o, c in zip(order, ncoef)]
    coefs = np.asarray(coefs, dtype)
    return Spline(len(order), coefs.shape[0], order, ncoef, knots, coefs)


def affine(order, ncoef, a, b, lo=0.0, hi=1.0):
    """The affine map x = A u + b as a spline of the given orders (Greville abscissae as coefficients)."""
    knots = [cases.clamped_uniform_knots(o, c, np.float64, lo, hi) for o, c in zip(order, ncoef)]
    grev = [np.array([k[i + 1:i + o].mean() if o > 1 else k[i] for i in range(c)]) for k, o, c in zip(knots, order, ncoef)]
    g = np.meshgrid(*grev, indexing="ij")
    coefs = np.stack([sum(a[d][i] * g[i] for i in range(len(order))) + b[d] for d in range(len(a))])
    return Spline(len(order), len(a), order, ncoef, knots, coefs)


def cfg2_surface():
    """bench.py's cfg2 shape (bicubic, 64 x 64 coefficients, 3,721 knot cells) as a height field: x, y on the
    Greville abscissae, z = 0.05 x the config's random coefficients.  (With all three components random the map
    has isolated rank-deficient points, cone points of the measure where the adaptive rule converges only
    linearly: DESIGN.md section 11.)"""
    nind, ndep, order, ncoef, knots, coefs, dt = cases.bench_spline(2)
    grev = [np.array([k[i + 1:i + 4].mean() for i in range(64)]) for k in knots]
    g = np.meshgrid(*grev, indexing="ij")
    return Spline(nind, ndep, order, ncoef, knots, np.stack([g[0], g[1], 0.05 * coefs[2]]))


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: f"{c[0]}-{c[3]}")
def test_golden(case):
    name, s, dom, f, ref = case
    close(s.integral(integrand(f), dom), ref, 1e-12)


@pytest.mark.parametrize("which,f,exact", [
    ("arc", None, math.pi / 2), ("arc", "x0", 1.0), ("arc", "x1", 1.0),
    ("annulus", None, 0.75 * math.pi), ("annulus", "x0", 7 / 3), ("annulus", "x1", 7 / 3)])
def test_analytic(which, f, exact):
    s = quarter_arc() if which == "arc" else annulus()
    assert abs(s.integral(integrand(f) if f else None) - exact) <= 1e-12


def test_straight_segment_length():
    s = affine((4,), (9,), [[3.0], [-4.0], [12.0]], [1.0, 2.0, 3.0], -1.0, 2.0)
    close(s.integral(), 13.0 * 3.0, 1e-13)


def test_bilinear_affine_patch_area():
    a = [[1.0, 0.5], [0.0, 2.0], [1.0, -1.0]]
    s = affine((2, 2), (5, 3), a, [0.0, 1.0, 2.0])
    cols = np.array(a)
    area = math.sqrt(np.linalg.det(cols.T @ cols))
    close(s.integral(), area, 1e-13)


def test_trivariate_affine_volume_one_round():
    a = [[2.0, 0.3, 0.0], [0.1, 1.5, -0.4], [0.0, 0.2, 0.7]]
    s = affine((3, 2, 4), (4, 3, 5), a, [1.0, 0.0, -1.0], 0.0, 2.0)
    stats = {}
    v = iq.integral(s, stats=stats)
    close(v, abs(np.linalg.det(np.array(a))) * 8.0, 1e-13)
    assert stats["rounds"] == 1


def test_cfg2_bicubic_64x64_against_cpu_rule():
    s = cfg2_surface()
    close(s.integral(), integral_ref(s), 1e-12)


def test_trivariate_order3_volume_against_cpu_rule():
    rng = np.random.default_rng(3)
    g = np.meshgrid(*[np.linspace(0, 1, 5)] * 3, indexing="ij")
    coefs = np.stack(g) + 0.05 * rng.standard_normal((3, 5, 5, 5))
    s = spline_of((3, 3, 3), (5, 5, 5), coefs)
    close(s.integral(), integral_ref(s), 1e-12)


def test_mixed_order_surface_against_cpu_rule():
    rng = np.random.default_rng(4)
    s = spline_of((3, 4), (7, 6), rng.standard_normal((3, 7, 6)))
    close(s.integral(), integral_ref(s), 1e-12)


def test_many_dependents_staged_in_groups():
    # order 12 x 12 in 15-D: 144-value windows, 14 dependents per LDS stage, so two stages per node chunk
    rng = np.random.default_rng(5)
    g = np.meshgrid(*[np.linspace(0, 1, 12)] * 2, indexing="ij")
    coefs = np.concatenate([np.stack(g), 0.05 * rng.standard_normal((13, 12, 12))])
    s = spline_of((12, 12), (12, 12), coefs)
    close(s.integral(), integral_ref(s), 1e-12)


@pytest.mark.parametrize("shape", [(2, 1), (3, 2)], ids=["surface-to-line", "volume-to-plane"])
def test_fewer_dependents_than_variables(shape):
    nind, ndep = shape
    rng = np.random.default_rng(6)
    g = np.meshgrid(*[np.linspace(0, 1, 5)] * nind, indexing="ij")
    coefs = np.stack([sum((d + i + 1) * g[i] for i in range(nind)) for d in range(ndep)])
    coefs = coefs + 0.02 * rng.standard_normal(coefs.shape)
    s = spline_of((3,) * nind, (5,) * nind, coefs)
    close(s.integral(), integral_ref(s), 1e-12)


def test_fp32_bicubic_close_to_fp64():
    rng = np.random.default_rng(8)
    g = np.meshgrid(np.linspace(0, 1, 12), np.linspace(0, 1, 12), indexing="ij")
    coefs = np.stack([g[0], g[1], 0.2 * rng.standard_normal((12, 12))])
    s64 = spline_of((4, 4), (12, 12), coefs)
    s32 = spline_of((4, 4), (12, 12), coefs.astype(np.float32), dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v32 = s32.integral()
    v64 = s64.integral()
    assert abs(v32 - v64) <= 1e-5 * abs(v64)


def test_domain_sub_box():
    s = cfg2_surface()
    dom = [[0.123, 0.456], [0.5, 0.8765]]
    close(s.integral(domain=dom), integral_ref(s, domain=dom), 1e-12)


def test_callable_integrand_on_a_surface():
    rng = np.random.default_rng(9)
    s = spline_of((3, 3), (6, 5), rng.standard_normal((3, 6, 5)))

    def f(x):
        return x[0] * x[1] + math.cos(x[2])
    close(s.integral(f), integral_ref(s, f), 1e-12)


def test_bitwise_reproducible():
    s = cfg2_surface()
    a, b = s.integral(), s.integral()
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    c, d = annulus().integral(lambda x: x[0]), annulus().integral(lambda x: x[0])
    assert np.float64(c).tobytes() == np.float64(d).tobytes()


def test_nodes_mode_matches_measure_mode():
    s = annulus()
    lo_hi, span = iq.regions(s, iq.check_domain(s, None))
    tables = s.device_tables()
    ks = tables.integral_regions(lo_hi, span)
    nodes = tables.integral_regions(lo_hi, span, nodes=True)
    np.testing.assert_allclose(nodes[:, :, -2].sum(axis=1), ks[:, 0], rtol=1e-14)
    np.testing.assert_allclose(nodes[:, :, -1].sum(axis=1), ks[:, 1], rtol=1e-14)
    j = np.indices((15, 15)).reshape(2, -1)
    uv = [(0.5 * (lo_hi[:, i, 0] + lo_hi[:, i, 1]))[:, None] + (0.5 * (lo_hi[:, i, 1] - lo_hi[:, i, 0]))[:, None] * iq.GK_X[j[i]]
          for i in range(2)]
    x, y = s(uv[0].ravel(), uv[1].ravel())
    np.testing.assert_allclose(nodes[:, :, 0].ravel(), x, rtol=0, atol=1e-14)
    np.testing.assert_allclose(nodes[:, :, 1].ravel(), y, rtol=0, atol=1e-14)
