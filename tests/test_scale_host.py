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
* The operator families (band, product, scan / sum, roots) obey their scaling laws, meet the exact references on shifted
  domains and keep locality on the host path: the second half of this file, which tests/test_gpu_scale_ops.py runs on
  the device.
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


# =============================================================================================================
# The operator families (DESIGN.md sections 13-16) on the host path: band (insert_knots, elevate, clamp, trim,
# differentiate), product (multiply), scan / sum (integrate, add, subtract) and roots (zeros_batch).  The device module
# tests/test_gpu_scale_ops.py runs the functions of this section with path="device"; the inputs are
# cases.operator_scale_cases, the transforms scale_ref.op_*.
#
# A. The scaling laws of scale_ref.op_exponent, bit for bit, result knots included, and the planner arrays under kp.
#    trim snaps a bound to a knot within an ABSOLUTE eps of it: that is the reference's rule (bspy/_spline_domain.py), and
#    it keeps the law only while a bound is far from every knot in absolute terms.  The bounds of these cases stay
#    cases.TRIM_CLEARANCE of the width away from every knot, so with widths down to 2^-20 (kp >= -20) the nearest knot
#    is 2^-30 away, far above eps of either type: inside the law.
#    Families moved off the bitwise law: none.
# B. Shifted and stretched domains against the exact references (refine_ref, product_ref, sum_ref, zeros_ref) on the
#    STORED shifted values, relative to the exact result's own scale (products: T max|a| max|b|), no floor of 1:
#    fp64 1e-12 (the parity bar); fp32 2^-23 (fp64 accumulation and one rounding to float32 lie within one float32 unit
#    of the scale of the correctly rounded exact value).  Roots: counts equal the exact counts, every root within
#    test_roots_host.delta (f' of the shifted curve carries the span width) plus 2 ulp of |u|.
# C. Locality, an exact law without a tolerance: one input coefficient x 2^20 and x 2^40 leaves every output whose exact
#    weight on it is zero bit for bit as it was.
# =============================================================================================================
import refine_ref
import product_ref
import sum_ref
import zeros_ref
import test_roots_host as trh
from bspy_amd import Spline, product, refinement, roots, sums
from conftest import observe

OC = cases.operator_scale_cases()
OPS_A = {c.name: c for c in OC["A"]}
OPS_B = {c.name: c for c in OC["B"]}
ALL_KERNELS = set().union(*cases.OPERATOR_KERNELS.values())
HOST_PATHS = {"band": {"host band"}, "product": {"host product"}, "sum": {"host band", "host scan", "host sum"}}
F32_UNIT = 2.0 ** -23
LOCAL_POWERS = (20, 40)


def differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shapes {a.shape} / {b.shape}, types {a.dtype} / {b.dtype}"
    diff = a != b
    rel = np.abs(a[diff].astype(np.float64) - b[diff]) / np.maximum(np.abs(b[diff].astype(np.float64)), np.finfo(np.float64).tiny)
    return f"{int(diff.sum())} of {a.size} values differ, largest relative difference {float(rel.max(initial=0.0)):.2e}"


def op_spline(spec):
    order, knots, coefs = spec
    return Spline(len(order), coefs.shape[0], order, coefs.shape[1:], knots, coefs)


def run_op(case, path):
    """The case's public call on ``path``; the result, with the paths that ran checked against the case."""
    s, a = op_spline(case.operands[0]), case.args
    if case.op == "multiply":
        r, ran = s.multiply(op_spline(case.operands[1]), a["indMap"], a["productType"], _path=path), product.LAST_PATHS
    elif case.op == "integrate":
        r, ran = s.integrate(a["wrt"], _path=path, _segments=a["segments"]), sums.LAST_PATHS
    elif case.op in ("add", "subtract"):
        r, ran = getattr(s, case.op)(op_spline(case.operands[1]), a["indMap"], _path=path), sums.LAST_PATHS
    else:
        positional = {"insert_knots": ("new",), "elevate": ("m",), "elevate_and_insert_knots": ("m", "new"), "clamp": ("left", "right"),
                      "trim": ("domain",), "differentiate": ("wrt",)}[case.op]
        r, ran = getattr(s, case.op)(*[a[key] for key in positional], _path=path), refinement.LAST_PATHS
    assert r is not s and ran, (case.name, "nothing ran")
    if path == "device":
        assert set(ran) == set(case.kernels) and len(ran) >= len(case.kernels), (case.name, list(ran), case.kernels)
    else:
        assert set(ran) <= HOST_PATHS[case.family], (case.name, list(ran))
    return r


def check_op_law(case, path):
    """Part A for one case: the call unscaled, then under every transform with the power of two undone: equal bits."""
    base = run_op(case, path)
    assert np.isfinite(base.coefs).all() and np.abs(base.coefs).max() > 0
    for label, ks, kp in sr.op_transforms(case, OC["exponents"], OC["rows"]):
        got = run_op(sr.op_scaled(case, ks, kp), path)
        assert got.order == base.order and got.nCoef == base.nCoef, (case.name, label)
        for iv, (t2, t) in enumerate(zip(got.knots, base.knots)):
            assert sr.same_bits(sr.undo(t2, kp), t), f"{case.name} [{label}]: result knots of variable {iv} are not x 2^{kp}"
        e = sr.op_exponent(case, ks, kp)
        back = sr.undo_law(got.coefs, e)
        assert sr.same_bits(back, base.coefs), f"{case.name} on {path} under [{label}] is not the unscaled result x 2^{np.unique(e)}: {differing(back, base.coefs)}"


@pytest.mark.parametrize("name", sorted(OPS_A))
def test_operator_scaling_law_host(name):
    check_op_law(OPS_A[name], "host")


def test_operator_cases_are_what_the_laws_need():
    """Trim bounds clear of every knot; every kernel of the four families declared by a case of A, B and C."""
    for case in list(OPS_A.values()) + list(OPS_B.values()):
        if case.op == "trim":
            order, knots, _ = case.operands[0]
            t = knots[0][order[0] - 1:len(knots[0]) - order[0] + 1]
            for bound in case.args["domain"][0]:
                assert np.abs(t - bound).min() >= cases.TRIM_CLEARANCE * (t[-1] - t[0]), case.name
    root_kernels = cases.OPERATOR_KERNELS["roots"]
    for part in (OPS_A.values(), OPS_B.values(), [c for c, _ in locality_cases()]):
        assert set().union(*(c.kernels for c in part)) | root_kernels == ALL_KERNELS      # every part has its roots tests


def test_planner_arrays_obey_their_own_law():
    """refine_map, product_map: unchanged under knots x 2^kp; differentiate_map x 2^-kp; integral_weights, the Bezier
    plan's breaks and margin x 2^kp; every ``first`` unchanged."""
    same = lambda a, b: all(sr.same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    for kp in sorted({kp for _, kp in OC["exponents"]["fp64"]} - {0}):
        p2 = lambda t: np.ldexp(t, kp)
        for case in OPS_A.values():
            order, knots, _ = case.operands[0]
            t, k = knots[0], order[0]
            if case.op == "insert_knots":
                new = case.args["new"][0]
                for m in (0, 1, 3):
                    if m:
                        tb, tb2 = refinement.elevated_knots(t, k, m, new), refinement.elevated_knots(p2(t), k, m, list(p2(new)))
                        maps = refinement.refine_map(t, k, tb, m), refinement.refine_map(p2(t), k, tb2, m)
                    else:
                        (tb, og), (tb2, og2) = refinement.merged_knots(t, k, new), refinement.merged_knots(p2(t), k, list(p2(new)))
                        maps = refinement.refine_map(t, k, tb, 0, origin=og), refinement.refine_map(p2(t), k, tb2, 0, origin=og2)
                    assert sr.same_bits(p2(tb), tb2) and same(*maps), (case.name, m, kp)
            elif case.op in ("trim", "clamp"):
                box = case.args["domain"] if case.op == "trim" else refinement.clamp_box(order, knots, case.args["left"], case.args["right"])
                (out, steps), (out2, steps2) = (refinement.trim_plan(order, [fn(x) for x in knots], sr._scale_arg(box, fn))
                                                for fn in (lambda x: x, p2))
                assert same([p2(x) for x in out], out2) and all(same(a[1:], b[1:]) for a, b in zip(steps, steps2)), (case.name, kp)
            elif case.op == "differentiate":
                (f, w), (f2, w2) = refinement.differentiate_map(t, k), refinement.differentiate_map(p2(t), k)
                assert same((f, np.ldexp(w, -kp)), (f2, w2)), (case.name, kp)
            elif case.op == "integrate":
                iv = case.args["wrt"]
                assert sr.same_bits(p2(sums.integral_weights(knots[iv], order[iv])), sums.integral_weights(p2(knots[iv]), order[iv]))
            elif case.op == "multiply":
                order2, knots2, _ = case.operands[1]
                for ind1, ind2 in case.args["indMap"]:
                    a = (knots[ind1], order[ind1], knots2[ind2], order2[ind2])
                    b = (p2(knots[ind1]), order[ind1], p2(knots2[ind2]), order2[ind2])
                    tb, tb2 = product.product_knots(*a), product.product_knots(*b)
                    assert sr.same_bits(p2(tb), tb2) and same(product.product_map(*a, tb), product.product_map(*b, tb2)), (case.name, kp)
        for spec in list(OC["roots_curves"].values()) + [golden_root_spec(n) for n in ROOT_NAMES]:
            (k,), (t,), _ = spec
            plan, plan2 = roots.BezierPlan(k, t), roots.BezierPlan(k, np.ldexp(t, kp).astype(t.dtype))
            assert sr.same_bits(sr.undo(plan2.breaks, kp), plan.breaks) and plan2.margin == np.ldexp(plan.margin, kp)
            assert same((plan.first, plan.cell), (plan2.first, plan2.cell)) and len(plan.steps) == len(plan2.steps)
            assert all(same(a[1:], b[1:]) for a, b in zip(plan.steps, plan2.steps))


# --------------------------------------------------------------------------------------------- A: roots
ROOT_NAMES = trh.NAMES


def golden_root_spec(name):
    c = trh.load_case(name)
    return (c["order"],), [c["knots"]], c["coefs"][None]


def root_specs():
    out = {f"golden {n}": golden_root_spec(n) for n in ROOT_NAMES}
    out.update({f"257 spans x 3 components {np.dtype(dt).name}": spec for dt, spec in OC["roots_curves"].items()})
    return out


ROOT_SPECS = root_specs()


def run_roots(spec, path, monkeypatch):
    """zeros_batch on ``path`` with what the two launches returned (candidates, padded roots, counts) captured."""
    (k,), (t,), coefs = spec
    seen = {}
    launches = "_run_device" if path == "device" else "_run_host"
    inner = getattr(roots, launches)

    def spy(*args):
        out = inner(*args)
        seen["cand"], seen["roots"], seen["count"] = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in out)
        return out
    monkeypatch.setattr(roots, launches, spy)
    try:
        values, offsets, intervals = roots.zeros_batch(Spline(1, coefs.shape[0], [k], [coefs.shape[1]], [t], coefs), _path=path)
    finally:
        monkeypatch.setattr(roots, launches, inner)
    ran = list(roots.LAST_PATHS)
    plan = roots.BezierPlan(k, t)
    if k >= 2:
        names = ["band_apply_line", "roots_flag", "roots_isolate"] if path == "device" else ["host roots_extract", "host roots_flag", "host roots_isolate"]
        assert ran == names[:1] * bool(plan.steps) + names[1:2] + names[2:] * bool(len(seen["cand"])), (ran, len(seen["cand"]))
        assert trh.nv.lib().bsk_roots_last_kernel().decode() == ran[-1]
    assert values.dtype == t.dtype
    return dict(values=np.asarray(values), offsets=np.asarray(offsets), intervals=intervals, ran=ran, **seen)


def root_kind(spec):
    return "fp32" if np.float32 in (spec[1][0].dtype, spec[2].dtype) else "fp64"


def check_roots_law(spec, path, monkeypatch, what):
    """Roots and intervals x 2^kp; offsets, candidates, counts and what ran unchanged; per-component coefficient scales.
    The flag bytes never leave the launch pair (zeros_batch keeps nonzero(flags), the candidates, and nothing else of
    them), so the candidates stand in for them here: which spans are flagged is pinned, the byte values are not."""
    order, (t,), coefs = spec
    kind = root_kind(spec)
    base = run_roots(spec, path, monkeypatch)
    r = OC["rows"][kind]
    transforms = [([kc] * len(coefs), kp) for kc, kp in OC["exponents"][kind]] + [([r[d % len(r)] for d in range(len(coefs))], 0)]
    for ks, kp in transforms:
        scaled = (order, [sr._p2(t, kp)], np.stack([sr._p2(row, k) for row, k in zip(coefs, ks)]))
        got = run_roots(scaled, path, monkeypatch)
        label = f"{what} on {path}, coefficients x 2^{ks}, knots x 2^{kp}"
        assert got["ran"] == base["ran"], label
        for key in ("offsets", "cand", "count"):
            assert np.array_equal(got.get(key, ()), base.get(key, ())), (label, key)
        assert sr.same_bits(sr.undo(got["values"], kp), base["values"]), f"{label}: {differing(sr.undo(got['values'], kp), base['values'])}"
        if "roots" in base:
            assert sr.same_bits(sr.undo(got["roots"], kp), base["roots"]), label
        assert np.array_equal(got["intervals"][:, 0], base["intervals"][:, 0]), label
        assert sr.same_bits(sr.undo(got["intervals"][:, 1:], kp), base["intervals"][:, 1:]), label
    return base


@pytest.mark.parametrize("name", sorted(ROOT_SPECS))
def test_roots_scaling_law_host(name, monkeypatch):
    base = check_roots_law(ROOT_SPECS[name], "host", monkeypatch, name)
    if name.startswith("257"):
        assert len(base["values"]) > 100 and np.all(np.diff(base["offsets"]) > 20)


# --------------------------------------------------------------------------------------------- B: shifted domains
_EXACT = {}


def op_exact(case, result, key):
    """(exact result rounded once, mask of the entries that exist, scale to judge against), once per key and session."""
    if key not in _EXACT:
        (o1, t1, c1), a = case.operands[0], case.args
        mask = None
        if case.op == "differentiate":
            exact = refine_ref.differentiate(o1, t1, c1, a["wrt"])
        elif case.op == "multiply":
            o2, t2, c2 = case.operands[1]
            exact = product_ref.multiply(o1, t1, c1, o2, t2, c2, a["indMap"], a["productType"], [result.knots[p[0]] for p in a["indMap"]])
            terms = {"S": 1, "D": c1.shape[0], "C": 2}[a["productType"]]
            _EXACT[key] = (exact, np.ones(exact.shape, bool), terms * float(np.abs(c1).max()) * float(np.abs(c2).max()))
            return _EXACT[key]
        elif case.op == "integrate":
            exact, _ = sum_ref.integrate(o1, t1, c1, a["wrt"], c1.dtype)
        elif case.op in ("add", "subtract"):
            spec = lambda s: dict(order=s[0], knots=s[1], coefs=s[2])
            exact = sum_ref.add(spec(case.operands[0]), spec(case.operands[1]), a["indMap"], list(result.order), list(result.knots),
                                1 if case.op == "add" else -1, c1.dtype)
        else:
            exact, mask = refine_ref.change_basis(o1, t1, c1, list(result.order), list(result.knots))
        mask = np.ones(exact.shape, bool) if mask is None else mask
        _EXACT[key] = (exact, mask, float(np.abs(exact[mask]).max()))
    return _EXACT[key]


def domain_id(d):
    return f"{d[0]:g}+{d[1]:g}"


def domain_text(d):
    return f"[{d[0]:g}, {d[0]:g} + {d[1]:g}]"


def op_distance(case, dom, path, reference=None):
    """The shifted case on ``path`` against the exact result: the distance relative to the scale, and the result."""
    moved = sr.op_shifted(case, *dom)
    r = run_op(moved, path)
    assert r.coefs.dtype == case.dt
    if reference is not None:
        assert all(sr.same_bits(a, b) for a, b in zip(r.knots, reference.knots)), (case.name, "the paths' knots differ")
    exact, mask, scale = op_exact(moved, r, (case.name, dom))
    assert r.coefs.shape == exact.shape and np.isfinite(r.coefs).all(), case.name
    return float(np.abs(r.coefs.astype(np.float64) - exact.astype(np.float64))[mask].max()) / scale, r


def cases_b(family, kind):
    return [c for c in OPS_B.values() if c.family == family and c.kind == kind]


def check_shifted_family(family, kind, dom, paths):
    """Every B case of the family on every path, in the order of ``paths``: each distance printed and recorded."""
    bar = F32_UNIT if kind == "fp32" else 1e-12
    for case in cases_b(family, kind):
        first = None
        shown = {}
        for path in paths:
            shown[path], r = op_distance(case, dom, path, first)
            first = r if first is None else first
        print(f"scale ops B: {case.name}, {domain_text(dom)}: " + "  ".join(f"d_{p} {d:.2e}" for p, d in shown.items()))
        for path, d in shown.items():
            observe(f"scale ops B {path}: {family} {kind}, {domain_text(dom)}", d, bar)


@pytest.mark.parametrize("dom", OC["domains"], ids=domain_id)
@pytest.mark.parametrize("family", ["band", "product", "sum"])
def test_operator_shifted_domain_host(family, dom):
    check_shifted_family(family, "fp64", dom, ["host"])


@pytest.mark.parametrize("dom", OC["domains_f32"], ids=domain_id)
@pytest.mark.parametrize("family", ["band", "product", "sum"])
def test_operator_shifted_domain_host_fp32(family, dom):
    check_shifted_family(family, "fp32", dom, ["host"])


_EXACT_ROOTS = {}
ROOT_GAP = 1e-6          # of the domain width: the exact roots of the B curve are further apart, so a count is never a tie


def shifted_root_spec(dt, dom):
    (k,), (t,), coefs = OC["roots_b"][dt]
    return (k,), [sr.map_axis(t, k, dom[0], dom[1], dt)], coefs


def exact_roots(dt, dom):
    key = (np.dtype(dt).name, dom)
    if key not in _EXACT_ROOTS:
        (k,), (t,), coefs = shifted_root_spec(dt, dom)
        _EXACT_ROOTS[key] = [zeros_ref.roots(k, t, row) for row in coefs]
    return _EXACT_ROOTS[key]


def check_shifted_roots(dt, dom, paths, monkeypatch):
    (k,), (t,), coefs = spec = shifted_root_spec(dt, dom)
    exact = exact_roots(dt, dom)
    for path in paths:
        got = run_roots(spec, path, monkeypatch)
        worst = 0.0
        for d, ex in enumerate(exact):
            mine = got["values"][got["offsets"][d]:got["offsets"][d + 1]]
            assert len(mine) == len(ex["brackets"]), f"component {d} on {path}: {len(mine)} roots, exactly {len(ex['brackets'])}"
            assert [list(row[1:]) for row in got["intervals"] if row[0] == d] == [list(i) for i in ex["intervals"]]
            c = dict(order=k, knots=t, coefs=coefs[d], exact_fprime=[float(f) for f in ex["fprime"]])
            for i, (r, (lo, hi)) in enumerate(zip(mine, ex["brackets"])):
                bar = trh.delta(c, i) + 2.0 * float(np.spacing(np.abs(r)))
                worst = max(worst, max(0.0, float(lo) - float(r), float(r) - float(hi)) / bar)
        print(f"scale ops B roots on {path}, {np.dtype(dt).name}, {domain_text(dom)}: worst error / bar {worst:.3e}")
        observe(f"scale ops B {path}: roots {np.dtype(dt).name} error / bar, {domain_text(dom)}", worst, 1.0)


ROOT_DOMAINS = [(np.float64, d) for d in OC["domains"]] + [(np.float32, d) for d in OC["domains_f32"]]
root_domain_id = lambda p: f"{np.dtype(p[0]).name}-{domain_id(p[1])}"


@pytest.mark.parametrize("dt,dom", ROOT_DOMAINS, ids=[root_domain_id(p) for p in ROOT_DOMAINS])
def test_roots_shifted_domain_host(dt, dom, monkeypatch):
    """The input condition first: the exact roots lie ROOT_GAP of the width apart (the brackets are far narrower)."""
    for ex in exact_roots(dt, dom):
        at = np.array([float(lo) for lo, _ in ex["brackets"]])
        assert len(at) >= 3 and np.all(np.diff(at) >= ROOT_GAP * dom[1]), "two exact roots nearly coincide: a count could tie"
    check_shifted_roots(dt, dom, ["host"], monkeypatch)


# --------------------------------------------------------------------------------------------- C: locality
def every_seventh(n):
    return sorted(set(range(0, n, 7)) | {n - 1})


_ROWS = {}


def band_touched(case, result, i):
    """Output rows along variable 0 whose exact weight on input coefficient i is not zero (rows without an exact value
    count as touched: nothing is claimed for them)."""
    (order, knots, _), k = case.operands[0], case.operands[0][0][0]
    if case.name not in _ROWS:
        _ROWS[case.name] = refine_ref.refine_rows(knots[0], k, result.knots[0], result.order[0] - k)
    return np.array([row is None or (row[0] <= i < row[0] + k and row[1][i - row[0]] != 0) for row in _ROWS[case.name]])


def product_touched(case, result, which, pair, i):
    """Output rows along the pair's variable whose exact weights on coefficient i of operand ``which`` are not all zero."""
    (o1, t1, _), (o2, t2, _) = case.operands
    ind1, ind2 = case.args["indMap"][pair]
    if (case.name, pair) not in _ROWS:
        _ROWS[case.name, pair] = product_ref.product_rows(t1[ind1], o1[ind1], t2[ind2], o2[ind2], result.knots[ind1])
    out = []
    for f, g, W, _ in _ROWS[case.name, pair]:
        if which == 0:
            out.append(f <= i < f + len(W) and any(w != 0 for w in W[i - f]))
        else:
            out.append(g <= i < g + len(W[0]) and any(row[i - g] != 0 for row in W))
    return np.array(out)


def locality_cases():
    """[(case, operand to touch)]: the insertions of part C and the band cases of B (m = 0, 1, 3), on lines and on a
    surface, the products of B on either operand, the scans of A (more than one chunk and segment) and the sum of A."""
    out = [(c, 0) for c in OC["C"]]
    for c in OPS_B.values():
        if c.kind == "fp64" and c.op in ("insert_knots", "elevate", "elevate_and_insert_knots"):
            out.append((c, 0))
        if c.kind == "fp64" and c.op == "multiply" and c.args["productType"] == "S":
            out += [(c, 0), (c, 1)]
    for c in OPS_A.values():
        if c.kind == "fp64" and (c.op == "integrate" or c.op == "add"):
            out += [(c, 0)] + ([(c, 1)] if c.op == "add" else [])
    return out


LOCALITY = {f"{c.name}, operand {w}": (c, w) for c, w in locality_cases()}


def check_locality(case, which, path):
    """One coefficient of operand ``which`` (component 0, index i along the operated variable, a fixed place in the others)
    x 2^20 and x 2^40, for every seventh i and both ends: outputs with an exact weight of zero on it keep their bits."""
    base = run_op(case, path)
    order, knots, coefs = case.operands[which]
    axis = case.args["wrt"] + 1 if case.op == "integrate" else 1
    for i in every_seventh(coefs.shape[axis]):
        index = [0] + [min(2, n - 1) for n in coefs.shape[1:]]
        index[axis] = i
        index = tuple(index)
        touched = np.zeros(base.coefs.shape, bool)
        if case.op == "integrate":
            at = list(index)
            at[axis] = slice(i + 1, None)                                # outputs at or before row i keep their bits
            touched[tuple(at)] = True
        elif case.op == "add":                                           # the broadcast operand reaches a whole line
            touched[index + (slice(None),) * (touched.ndim - len(index))] = True
        elif case.op == "multiply":                                      # "S": component d of the result from components d
            assert all(len(o) == len(case.args["indMap"]) for o, _, _ in case.operands), "the products of part B map every variable"
            touched[0] = True
            for pair, variables in enumerate(case.args["indMap"]):
                rows = product_touched(case, base, which, pair, index[1 + variables[which]])
                touched &= rows.reshape([len(rows) if ax == variables[0] + 1 else 1 for ax in range(touched.ndim)])
        else:
            touched[(0, slice(None)) + index[2:]] = band_touched(case, base, i)
        assert 0 < touched.sum() < touched.size
        for power in LOCAL_POWERS:
            operands = list(case.operands)
            operands[which] = (order, knots, sr.multiplied(coefs, index, power))
            got = run_op(case.replaced(operands), path)
            changed = got.coefs != base.coefs
            moved = changed & ~touched
            assert not moved.any(), (f"{case.name} on {path}: coefficient {index} of operand {which} x 2^{power} moves {int(moved.sum())} outputs "
                                     f"whose exact weight on it is zero, by up to {float(np.abs(got.coefs - base.coefs)[moved].max()):.2e}")
            assert changed[touched].any(), "the multiplied coefficient reaches nothing"


@pytest.mark.parametrize("name", sorted(LOCALITY))
def test_locality_host(name):
    check_locality(*LOCALITY[name], "host")


def bezier_case():
    """The Bezier extraction of the B curve as a band step: (knots, order, Bezier knots, steps)."""
    (k,), (t,), coefs = OC["roots_b"][np.float64]
    plan = roots.BezierPlan(k, t)
    values, counts = np.unique(t, return_counts=True)
    bezier = np.repeat(values, np.where((values == t[0]) | (values == t[-1]), k, np.maximum(k - 1, counts)))
    assert plan.steps and len(bezier) - k == plan.rowlen
    return t, k, bezier, plan, coefs


def check_extraction_locality(extract):
    """extract(coefs, plan) -> the extracted rows (NumPy float64)."""
    t, k, bezier, plan, coefs = bezier_case()
    rows = refine_ref.refine_rows(t, k, bezier, 0)
    base = extract(coefs, plan)
    for i in every_seventh(coefs.shape[1]):
        touched = np.zeros(base.shape, bool)
        touched[0] = [row[0] <= i < row[0] + k and row[1][i - row[0]] != 0 for row in rows]
        for power in LOCAL_POWERS:
            got = extract(sr.multiplied(coefs, (0, i), power), plan)
            moved = (got != base) & ~touched
            assert not moved.any(), f"Bezier extraction: coefficient {i} x 2^{power} moves {int(moved.sum())} entries it has no weight on"


def test_extraction_locality_host():
    check_extraction_locality(roots.extract_host)
    assert trh.nv.lib().bsk_roots_last_kernel().decode() == "host roots_extract"


def check_roots_locality(path, monkeypatch):
    """One coefficient of component 1 multiplied: components 0 and 2 keep their roots, bit for bit."""
    order, knots, coefs = spec = OC["roots_curves"][np.float64]
    base = run_roots(spec, path, monkeypatch)
    per = lambda r, d: r["values"][r["offsets"][d]:r["offsets"][d + 1]]
    for i in every_seventh(coefs.shape[1]):
        for power in LOCAL_POWERS:
            got = run_roots((order, knots, sr.multiplied(coefs, (1, i), power)), path, monkeypatch)
            for d in (0, 2):
                assert per(got, d).tobytes() == per(base, d).tobytes(), (path, i, power, d)


def test_roots_locality_host(monkeypatch):
    check_roots_locality("host", monkeypatch)
