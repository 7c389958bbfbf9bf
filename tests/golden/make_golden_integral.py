"""
Golden values of Spline.integral (arc length, area, moments).  Runs ONLY where the reference
checkout is importable (see make_golden.load_reference); the output, ``integral.npz``, holds the
splines' data (order, nCoef, knots, coefs, optional domain) and the values the reference's
``Spline.integral`` returned for them.

    python tests/golden/make_golden_integral.py          (about a minute and a half)

Keys: ``<case>/order``, ``<case>/ncoef``, ``<case>/knots<iv>``, ``<case>/coefs`` (nDep, *nCoef),
``<case>/domain`` (when not the spline's own) and ``<case>/value/<integrand>`` with integrand
``one`` (integrand=None) or ``x<d>`` (lambda x: x[d]).
"""
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402


def integrands(name):
    if name == "one":
        return None
    d = int(name[1:])
    return lambda x: x[d]


def bicubic_8x8(bspy):
    """Random bicubic 8 x 8 surface in 3-D near the unit square."""
    rng = np.random.default_rng(7)
    n = 8
    knots = np.concatenate([np.zeros(4), np.arange(1, n - 3) / (n - 3), np.ones(4)])
    g = np.linspace(0.0, 1.0, n)
    coefs = np.empty((3, n, n))
    coefs[0] = g[:, None] + 0.03 * rng.standard_normal((n, n))
    coefs[1] = g[None, :] + 0.03 * rng.standard_normal((n, n))
    coefs[2] = 0.25 * rng.standard_normal((n, n))
    return bspy.Spline(2, 3, (4, 4), (n, n), (knots, knots.copy()), coefs)


def scalar_curve(bspy):
    """nDep 1: increasing coefficients (no kink in |x'|), non-uniform knots."""
    knots = np.array([0.0, 0, 0, 0, 0.2, 0.45, 0.5, 0.8, 1, 1, 1, 1])
    coefs = np.array([[0.0, 0.3, 0.35, 0.9, 1.4, 1.5, 2.2, 2.3]])
    return bspy.Spline(1, 1, (4,), (8,), (knots,), coefs)


def space_curve(bspy):
    """nDep 3: a helix-like cubic with a double knot."""
    knots = np.array([-1.0, -1, -1, -1, -0.4, 0.1, 0.1, 0.7, 2, 2, 2, 2])
    t = np.linspace(0.0, 3.0, 8)
    coefs = np.stack([np.cos(t), np.sin(t), 0.4 * t])
    return bspy.Spline(1, 3, (4,), (8,), (knots,), coefs)


def main():
    bspy = load_reference()
    arc = bspy.Spline.circular_arc(1.0, 90.0)
    annulus = bspy.Spline.ruled_surface(bspy.Spline.circular_arc(2.0, 90.0), arc)
    cases = [
        ("arc", arc, None, ("one", "x0", "x1")),
        ("annulus", annulus, None, ("one", "x0", "x1")),
        ("bicubic8", bicubic_8x8(bspy), None, ("one",)),
        ("scalar_curve", scalar_curve(bspy), None, ("one", "x0")),
        ("space_curve", space_curve(bspy), None, ("one", "x2")),
        # a domain whose ends cut through knot spans of both variables
        ("annulus_cut", annulus, [[0.07, 0.6], [0.25, 0.8]], ("one",)),
        ("arc_cut", arc, [[0.2, 0.81]], ("one", "x1")),
    ]
    out = {}
    for name, s, domain, names in cases:
        out[f"{name}/order"] = np.array(s.order, np.int32)
        out[f"{name}/ncoef"] = np.array(s.nCoef, np.int32)
        for iv, k in enumerate(s.knots):
            out[f"{name}/knots{iv}"] = np.asarray(k, np.float64)
        out[f"{name}/coefs"] = np.asarray(s.coefs, np.float64)
        dom = None if domain is None else np.array(domain, np.float64)
        if dom is not None:
            out[f"{name}/domain"] = dom
        for f in names:
            t0 = time.time()
            with warnings.catch_warnings():
                warnings.simplefilter("error")          # a value the reference's quad did not converge on is no golden
                v = s.integral(integrands(f), dom)
            out[f"{name}/value/{f}"] = np.float64(v)
            print(f"{name} {f}: {v!r}  ({time.time() - t0:.2f} s)", flush=True)
    np.savez_compressed(os.path.join(HERE, "integral.npz"), **out)


if __name__ == "__main__":
    main()
