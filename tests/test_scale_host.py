"""
CPU preconditions of the scale tests (tests/test_gpu_scale.py): what must hold on the host so that a GPU failure there
is the GPU's.

* The C oracle obeys the power-of-two scaling laws bit for bit on every family's inputs and transforms
  (tests/cases.py: scale_cases; scale_ref.py states the law).  A normal or curvature case whose ORACLE is not bitwise
  (a library pow or sqrt is not obliged to be) is listed in ORACLE_NOT_BITWISE by name; an unlisted one fails, and so
  does a listed one that is bitwise after all.
* The extended-precision yardstick is a restatement of the oracle's function, not another function: 64 ulp of the
  result scale on the unshifted parity cases.
* bsk_api.hip's axis_is_uniform, restated in Python, accepts exactly the shifted-domain cases listed here: the GPU
  module derives the kernel every case must name from the same rule, and a change of the acceptance constant shows.
"""
import numpy as np
import pytest

import cases
import oracle
import scale_ref as sr

SC = cases.scale_cases()
FAMILIES = {f.name: f for f in SC["families"]}
HOST_POINTS = 30_000            # of a family's batch: the knot points at its front, the NaN parameters and random ones

# (family, call kind, transform label) of normal / curvature / measure cases whose oracle is not bitwise homogeneous
ORACLE_NOT_BITWISE = set()


def _oracle_call(fam, spec, kind, wrt):
    order, ncoef, knots, coefs, pts = spec
    if kind in ("eval", "grid", "tess"):
        return oracle.c_evaluate(order, ncoef, knots, coefs, list(wrt or (0,) * fam.nInd), pts)[0]
    if kind == "jac":
        return oracle.c_jacobian(order, ncoef, knots, coefs, pts)[0]
    if kind in ("normal", "tessn"):
        return oracle.c_normal(order, ncoef, knots, coefs, pts, True, False)[0]
    if kind == "curv":
        return oracle.c_curvature(order, ncoef, knots, coefs, pts)[0]
    raise ValueError(kind)


def family_spec(fam):
    """(order, nCoef, knots, coefs, points) the oracle sees: the batch's front, or the grid's points."""
    if fam.grid is None and fam.n:
        pts = [p[:HOST_POINTS] for p in sr.family_points(fam)]
    else:
        pts = [m.ravel() for m in np.meshgrid(*sr.family_axes(fam), indexing="ij")]
    return fam.order, fam.nCoef, fam.knots, fam.coefs, pts


@pytest.mark.parametrize("name", sorted(n for n, f in FAMILIES.items() if f.calls[0][0] != "integral"))
def test_oracle_is_bitwise_homogeneous(name):
    fam = FAMILIES[name]
    spec = family_spec(fam)
    calls = [(k, w) for k, w, _ in fam.calls] + ([("tess", None)] if fam.calls[0][0] == "tessn" else [])
    base = {(k, w): _oracle_call(fam, spec, k, w) for k, w in calls}
    assert all(np.isfinite(b).mean() > 0.9 for b in base.values())
    seen = set()
    for label, kcs, kp, uniform in sr.family_transforms(fam, SC["exponents"], SC["rows"]):
        tspec = sr.transformed(spec, kcs, kp)
        for k, w in calls:
            e = sr.call_exponent(k, w, kcs, kp, fam.nInd, uniform)
            if e is None:
                continue
            got = _oracle_call(fam, tspec, k, w)
            same = sr.same_bits(sr.undo_law(got, e), base[(k, w)])
            if k in ("normal", "tessn", "curv"):
                if not same:
                    seen.add((name, k, label))
                continue
            assert same, f"{name}: oracle {k} {w} is not bitwise under {label}"
    listed = {x for x in ORACLE_NOT_BITWISE if x[0] == name}
    assert seen == listed, (seen, listed)


def test_cpu_quadrature_rule_is_bitwise_homogeneous():
    """integral_regions' CPU restatement (integral_ref.region_sums) under the same transforms: 2^(nInd kc)."""
    from bspy_amd import Spline
    from bspy_amd import integral as iq
    from integral_ref import region_sums
    fam = FAMILIES["integral_regions"]

    def sums(knots, coefs):
        s = Spline(fam.nInd, fam.nDep, fam.order, fam.nCoef, knots, coefs)
        lo_hi, span = iq.split(*iq.regions(s, iq.check_domain(s, None)))
        return np.stack(region_sums(s, lo_hi, span))
    base = sums(fam.knots, fam.coefs)
    for label, kcs, kp, uniform in sr.family_transforms(fam, SC["exponents"], SC["rows"]):
        if uniform:
            _, _, knots, coefs, _ = sr.transformed((fam.order, fam.nCoef, fam.knots, fam.coefs, []), kcs, kp)
            e = sr.call_exponent("integral", None, kcs, kp, fam.nInd, True)
            assert sr.same_bits(sr.undo_law(sums(knots, coefs), e), base), label


def test_fit_reference_is_bitwise_homogeneous():
    """The host plan of the banded least-squares solve: data x 2^k gives coefficients x 2^k and residual sums x 2^2k."""
    from bspy_amd import fitting
    systems, ks = SC["fit"]
    for sysdef in systems:
        plan, first, values, b = sr.fit_system(*sysdef)
        outer, inner = sysdef[3], sysdef[4]
        x = plan.solve_host(b, outer, inner)
        r = fitting.residual_rows_host(first, values, b, x)
        for k in ks:
            bk = np.ldexp(b, k)
            xk = plan.solve_host(bk, outer, inner)
            assert sr.same_bits(np.ldexp(xk, -k), x), (sysdef, k)
            assert sr.same_bits(np.ldexp(fitting.residual_rows_host(first, values, bk, xk), -2 * k), r), (sysdef, k)


@pytest.mark.parametrize("name", sorted(c.name for c in cases.parity_cases() if c.coefs.dtype == np.float64 and c.knots[0].dtype == np.float64))
def test_extended_reference_agrees_with_oracle(name):
    c = {x.name: x for x in cases.parity_cases()}[name]
    pts = [p[:160] for p in c.points]
    wrts = [tuple(w) for w in c.wrts]
    exts = sr.derivative_ext(c.order, c.knots, c.coefs, wrts, pts)
    for w, ext in zip(wrts, exts):
        orc, bad = oracle.c_evaluate(c.order, c.nCoef, c.knots, c.coefs, list(w), pts)
        assert bad == -1
        d = sr.distance(orc, ext, sr.scale_of(ext))
        assert d <= 64 * np.finfo(np.float64).eps, (name, w, d)


def test_mpmath_arithmetic_is_the_same_restatement():
    """The fallback for platforms whose long double is a double: the same code in mpmath at 40 digits."""
    c = {x.name: x for x in cases.parity_cases()}["volume_o3x4x2"]
    pts = [p[:40] for p in c.points]
    wrts = [(0, 0, 0), (1, 0, 0), (0, 2, 0)]
    mp = sr.derivative_ext(c.order, c.knots, c.coefs, wrts, pts, ar=sr.arithmetic(force_mpmath=True))
    orc = [oracle.c_evaluate(c.order, c.nCoef, c.knots, c.coefs, list(w), pts)[0] for w in wrts]
    for a, o in zip(mp, orc):
        assert a.dtype == object
        assert sr.distance(o, a, sr.scale_of(o)) <= 64 * np.finfo(np.float64).eps
    if not sr.use_mpmath():
        ld = sr.derivative_ext(c.order, c.knots, c.coefs, wrts, pts)
        for a, b in zip(mp, ld):
            assert max(abs(float(x - y)) for x, y in zip(a.ravel(), b.ravel())) <= 1e-17 * sr.scale_of(b)


def test_transforms():
    spec = ((4,), (8,), [cases.clamped_uniform_knots(4, 8)], np.arange(16.0).reshape(2, 8) + 1, [np.array([0.25, 1.0])])
    assert np.array_equal(sr.scale_coefs(spec, 3)[3], spec[3] * 8)
    assert np.array_equal(sr.scale_rows(spec, [1, -1])[3], spec[3] * np.array([[2.0], [0.5]]))
    t = sr.scale_params(spec, -2)
    assert np.array_equal(t[2][0], spec[2][0] / 4) and np.array_equal(t[4][0], spec[4][0] / 4)
    k = sr.map_domain((4,), (8,), spec[2], 33.0, 1.0, np.float64)[0]
    assert np.array_equal(k, cases.clamped_uniform_knots(4, 8, np.float64, 33.0, 34.0))       # as a user builds them
    c, mask = sr.multiply_layers(np.ones((2, 5, 6)), [(0, 0), (1, 1)], 3)
    assert mask.sum() == 6 + 5 - 1 and np.array_equal(c[0], np.where(mask, 8.0, 1.0))
    ix = np.array([[4, 5, 5], [4, 4, 6]])
    assert list(sr.support_is_clean((4, 4), mask, ix)) == [False, True, False]


# --------------------------------------------------------------------------------------------- the uniform path's rule
# Which shifted domains the table-free uniform-knot kernels take, per spline: (lo, width) -> accepted.  The worst knot
# deviation d / h of the accepted ones is asserted below the acceptance constant's 1024 ulp = 2.3e-13, and the cases
# near that edge (33 .. 34, 1000 .. 1064, 3 .. 3.125 with 61 spans) above 1e-13: they are what tests the constant.
ACCEPTED = {(0.0, 1.0): True, (8.0, 1.0): True, (33.0, 1.0): True, (1000.0, 64.0): True, (3.0, 0.125): True,
            (1000.0, 1.0): False, (1e6, 0.021): False, (-1001.0, 1.0): False, (0.1, 3e-7): False, (-5e8, 1e9): True}
ACCEPTED_F32 = {(0.0, 1.0): True, (100.0, 1.0): False, (0.0, 2.0 ** -10): True}


def uniform_path_expected(spl, lo, width):
    """(taken?, worst d / h): the rule on every axis of a cases.ScaleSpline moved to [lo, lo + width]."""
    knots = sr.map_domain(spl.order, spl.nCoef, spl.knots, lo, width, spl.dt)
    r = [sr.axis_is_uniform(k, o, c) for k, o, c in zip(knots, spl.order, spl.nCoef)]
    return all(a for a, _ in r), max(d for _, d in r)


def test_axis_is_uniform_rule():
    assert sr.UNIFORM_ULPS[np.dtype(np.float64)] == 1024.0 and sr.UNIFORM_ULPS[np.dtype(np.float32)] == 32.0
    for spl, table, doms in [(s, ACCEPTED, SC["domains"]) for s in SC["splines"]] + [(s, ACCEPTED_F32, SC["domains_f32"]) for s in SC["splines_f32"]]:
        assert set(doms) == set(table)
        for lo, w in doms:
            took, dev = uniform_path_expected(spl, lo, w)
            assert took == (table[(lo, w)] and spl.uniform), (spl.name, lo, w, dev)
            if took:
                assert dev <= 1024 * np.finfo(spl.dt).eps * (1.0 if spl.dt == np.float64 else 32.0 / 1024.0) * 1.0001
    # the edge cases are at the edge
    cfg2 = SC["splines"][0]
    for lo, w in ((33.0, 1.0), (1000.0, 64.0), (3.0, 0.125)):
        assert 1e-13 < uniform_path_expected(cfg2, lo, w)[1] <= 2.3e-13
    # perturbed and far-away uniform knots are declined, a continued (unclamped) end is accepted
    k = cases.clamped_uniform_knots(4, 64)
    assert sr.axis_is_uniform(k, 4, 64)[0]
    bumped = k.copy()
    bumped[30] += 400 * np.finfo(float).eps * bumped[30]
    assert not sr.axis_is_uniform(bumped, 4, 64)[0]
    assert not sr.axis_is_uniform(cases.clamped_uniform_knots(4, 64, np.float64, 1e6, 1e6 + 0.061), 4, 64)[0]
    open_ends = np.arange(-3.0, 65.0) / 8
    assert sr.axis_is_uniform(open_ends, 4, 64)[0]
    half_clamped = open_ends.copy()
    half_clamped[:3] = half_clamped[3] - np.array([0.3, 0.2, 0.05])
    assert not sr.axis_is_uniform(half_clamped, 4, 64)[0]
