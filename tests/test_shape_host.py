"""
CPU preconditions of tests/test_gpu_shape.py: what makes a failure there mean the kernel and not the test.  For every case of
cases.shape_cases, with the CPU oracle (oracle.c_normal, oracle.c_curvature, in the kernels' dtype) alone:
  - the oracle's result is within 1/8 of the bar of tests/shape_ref.py at every kept point;
  - at least 90 % of the sample's finite points are kept (area normals: all of them);
  - NaN results sit exactly where a parameter is NaN (points 3 and 4 of every batch), and nothing is out of the domain;
  - a polyline's curvature is exactly 0.0 wherever it is finite;
  - the oracle's worst error in units of eps * sum |dg/dd_i| * max(1, max |d_i|) is printed, and K of shape_ref is at
    least 8 x that (test_measured_units).
"""
import functools

import numpy as np
import pytest

import cases
import oracle
import shape_ref as sh

CASES = cases.shape_cases()


def oracle_results(case, pts):
    """{quantity: result of the CPU oracle at pts} in the layout shape_ref.Reference.compare takes."""
    spec = (case.order, case.nCoef, case.knots, case.coefs, pts)
    if case.kind == "curvature":
        got, bad = oracle.c_curvature(*spec)
        assert bad == -1
        return {"curvature": got}
    out = {}
    for name, normalize, negate in (("unit normal", True, False), ("area normal", False, False), ("area normal, negated", False, True)):
        out[name], bad = oracle.c_normal(*spec, normalize=normalize, negate=negate)
        assert bad == -1
    return out


@functools.lru_cache(maxsize=None)
def figures(name):
    """[(quantity, worst error / bar, worst error in units, kept share)] of the oracle on the case's sample."""
    case = CASES[name]
    ref = sh.reference(case)
    with np.errstate(all="ignore"):
        return [(q, *ref.compare(q, got)) for q, got in oracle_results(case, ref.pts).items()]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_within_an_eighth_of_the_bar(name):
    case = CASES[name]
    ref = sh.reference(case)
    if not case.zero:                  # no derivative of a polyline that the curvature takes depends on the parameter
        assert ref.nan_mask().tolist() == [i in (3, 4) for i in range(len(ref.idx))], "NaN exactly where a parameter is NaN"
    for q, ratio, units, share in figures(name):
        print(f"{name}: {q}: oracle error / bar {ratio:.3f}, {units:.2f} units, kept {share:.3f}")
        if case.zero:
            got = oracle_results(case, ref.pts)[q]
            assert (got[ref.finite] == 0.0).all(), "the second derivative of a polyline is identically zero"
            continue
        assert share >= (1.0 if q.startswith("area") else sh.KEEP), (name, q, share)
        assert ratio <= 0.125, (name, q, ratio)


def test_measured_units():
    """K of shape_ref.py against the measurement it is defined by: 8 x the oracle's worst error in units, rounded up to a
    power of two and never below shape_ref.K_FLOOR (general-knot cases; the uniform families' bar takes K only for the
    result's own rounding, their units are printed by the test above all the same)."""
    worst = {"fp64": 0.0, "fp32": 0.0}
    for name in sorted(CASES):
        if CASES[name].zero or CASES[name].uniform:
            continue
        for q, ratio, units, share in figures(name):
            worst[CASES[name].type] = max(worst[CASES[name].type], units)
    for kind, dt in (("fp64", np.float64), ("fp32", np.float32)):
        k = max(2.0 ** np.ceil(np.log2(8.0 * worst[kind])), sh.K_FLOOR[np.dtype(dt)])
        print(f"shape bars, {kind}: the oracle's worst error is {worst[kind]:.2f} units -> K = {k:g} (shape_ref.K: {sh.K[np.dtype(dt)]:g})")
        assert sh.K[np.dtype(dt)] == k, (kind, worst[kind], k)
