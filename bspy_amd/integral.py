"""
``Spline.integral`` (reference bspy/spline.py:1249 -> ``composed_integral``, bspy/_spline_evaluation.py:29-73):
the integral of f(S(u)) times the measure of the map, mu(u) = product of the singular values of the jacobian
(arc length, area, volume when f is None; moments with f = lambda x: x[0], ...).

The reference nests scipy.integrate.quad per variable and knot span.  Here every knot cell is integrated by a
tensor Gauss-Kronrod 7/15 rule on the GPU (``bsk_integral``, bsk_integral.hpp), one device call per round of an
adaptive driver: a region whose Kronrod and Gauss sums differ by more than its share of the tolerance is split in
half along every variable (children stay inside their cell, so they keep its span indices), until no region is
rejected or the error estimates of all regions together are within the tolerance.

    cells / regions   breakpoints of every variable (the reference's rule, :42-47), their tensor product
    adaptive()        the driver, with the device round or any other round function (tests/integral_ref.py)
    integral()        the entry point behind Spline.integral
"""
import itertools
import math
import warnings

import numpy as np

# Kronrod 15-point rule on [-1, 1] (ascending) and the 7-point Gauss rule embedded at its odd positions; the same
# constants as bsk_integral.hpp.
GK_X = np.array([
    -0.99145537112081264, -0.94910791234275852, -0.86486442335976907, -0.74153118559939444, -0.58608723546769113,
    -0.40584515137739717, -0.20778495500789847, 0.0, 0.20778495500789847, 0.40584515137739717,
    0.58608723546769113, 0.74153118559939444, 0.86486442335976907, 0.94910791234275852, 0.99145537112081264])
GK_WK = np.array([
    0.022935322010529225, 0.063092092629978553, 0.10479001032225018, 0.14065325971552592, 0.16900472663926790,
    0.19035057806478541, 0.20443294007529889, 0.20948214108472783, 0.20443294007529889, 0.19035057806478541,
    0.16900472663926790, 0.14065325971552592, 0.10479001032225018, 0.063092092629978553, 0.022935322010529225])
GK_WG = np.array([
    0.0, 0.12948496616886969, 0.0, 0.27970539148927667, 0.0, 0.38183005050511894, 0.0, 0.41795918367346939,
    0.0, 0.38183005050511894, 0.0, 0.27970539148927667, 0.0, 0.12948496616886969, 0.0])

TOLERANCE = 1.0e-13        # divided by nInd, as the reference's epsabs = epsrel (:52)
TOLERANCE_F32 = 1.0e-6     # floor of fp32 splines (nodes evaluated in fp32)
MAX_ROUNDS = 40
MAX_REGIONS = 1 << 22
MAX_NIND = 3
_NODE_CHUNK = 1 << 24      # fp64 values per NODES call (callable integrands)


def check_domain(spline, domain):
    """The integration box, nInd x 2: the spline's domain, or ``domain`` validated as the reference does (:31-38)."""
    actual = np.array([[spline.knots[i][spline.order[i] - 1], spline.knots[i][spline.nCoef[i]]]
                       for i in range(spline.nInd)], np.float64).reshape(spline.nInd, 2)
    if domain is None:
        return actual
    domain = np.asarray(domain, np.float64)
    if domain.shape != (spline.nInd, 2):
        raise ValueError(f"domain must be an nInd x 2 array, got shape {domain.shape}")
    for i in range(spline.nInd):
        if domain[i, 0] < actual[i, 0] or domain[i, 1] > actual[i, 1]:
            raise ValueError("Can't integrate beyond the domain of the spline")
    return domain


def breakpoints(knots, lo, hi):
    """Unique knots inside [lo, hi] with both ends inserted: the reference's quadrature intervals (:42-47)."""
    knots = np.asarray(knots, np.float64)
    start = np.searchsorted(knots, lo, side="right")
    end = np.searchsorted(knots, hi, side="right")
    return np.unique(np.concatenate(([lo], knots[start:end], [hi])))


def cells(spline, domain):
    """Per variable: (lo, hi, span) of its integration cells; span = the "rightmost knot of the segment"
    (searchsorted right, clamped to [order, nCoef]) of the cell's left end."""
    out = []
    for i in range(spline.nInd):
        b = breakpoints(spline.knots[i], domain[i, 0], domain[i, 1])
        lo, hi = b[:-1], b[1:]
        span = np.searchsorted(np.asarray(spline.knots[i], np.float64), lo, side="right")
        span = np.clip(span, spline.order[i], spline.nCoef[i]).astype(np.int32)
        out.append((lo, hi, span))
    return out


def regions(spline, domain):
    """Tensor product of the cells: lo_hi (R, nInd, 2), span (R, nInd), first variable slowest."""
    per = cells(spline, domain)
    count = [len(c[0]) for c in per]
    if min(count, default=0) == 0:
        return np.zeros((0, spline.nInd, 2)), np.zeros((0, spline.nInd), np.int32)
    idx = np.indices(count).reshape(spline.nInd, -1)
    lo_hi = np.stack([np.stack([per[i][0][idx[i]], per[i][1][idx[i]]], -1) for i in range(spline.nInd)], 1)
    span = np.stack([per[i][2][idx[i]] for i in range(spline.nInd)], 1).astype(np.int32)
    return lo_hi, span


def split(lo_hi, span):
    """Every region halved along every variable: 2^nInd children per region, region-major."""
    nreg, nind = lo_hi.shape[:2]
    bits = np.array(list(itertools.product((0, 1), repeat=nind)), bool)           # (2^nInd, nInd)
    lo, hi = lo_hi[:, None, :, 0], lo_hi[:, None, :, 1]
    mid = 0.5 * (lo + hi)
    children = np.stack([np.where(bits, mid, lo), np.where(bits, hi, mid)], -1)
    return children.reshape(-1, nind, 2), np.repeat(span, len(bits), axis=0)


def adaptive(round_fn, lo_hi, span, domain, tol):
    """Adaptive driver.  round_fn(lo_hi, span) -> (K, G) per region, e = |K - G|.  With the budget
    B = max(tol, tol |sum K|), region r is accepted when e_r <= B vol(r) / vol(D); the others are split.  The driver
    stops when no region is rejected, or when the error estimates of all regions (accepted and current) sum to at
    most B - the global test of QUADPACK's drivers, which ends the work at isolated points where the measure is
    not smooth (rank-deficient jacobians) once their regions' errors are negligible in total.  Returns (sum of K
    in a fixed order, rounds, final region count, regions evaluated)."""
    total_vol = float(np.prod(domain[:, 1] - domain[:, 0]))
    accepted, accepted_err = [], []
    evaluated = 0
    for rnd in range(1, MAX_ROUNDS + 1):
        k, g = round_fn(lo_hi, span)
        evaluated += len(k)
        err = np.abs(k - g)
        budget = max(tol, tol * abs(math.fsum(np.concatenate(accepted + [k]))))
        vol = np.prod(lo_hi[:, :, 1] - lo_hi[:, :, 0], axis=1)
        ok = err <= budget * (vol / total_vol)
        if ok.all() or math.fsum(np.concatenate(accepted_err + [err])) <= budget:
            accepted.append(k)
            return math.fsum(np.concatenate(accepted)), rnd, sum(len(a) for a in accepted), evaluated
        accepted.append(k[ok])
        accepted_err.append(err[ok])
        if rnd == MAX_ROUNDS or (~ok).sum() << lo_hi.shape[1] > MAX_REGIONS:
            estimate = math.fsum(np.concatenate(accepted_err + [err[~ok]]))
            warnings.warn(f"Spline.integral: adaptive limit reached ({rnd} rounds, {(~ok).sum()} regions not "
                          f"converged); estimated error {estimate:.3e}", RuntimeWarning, stacklevel=3)
            accepted.append(k[~ok])
            return math.fsum(np.concatenate(accepted)), rnd, sum(len(a) for a in accepted), evaluated
        lo_hi, span = split(lo_hi[~ok], span[~ok])


def node_sums(nodes, integrand):
    """(K, G) per region from NODES output (R, 15^nInd, nDep + 2): f called once per node with x (nDep,)."""
    ndep = nodes.shape[2] - 2
    flat = nodes.reshape(-1, ndep + 2)
    f = np.array([float(integrand(x)) for x in flat[:, :ndep]], np.float64).reshape(nodes.shape[:2])
    return np.sum(f * nodes[:, :, ndep], axis=1), np.sum(f * nodes[:, :, ndep + 1], axis=1)


def integral(spline, integrand=None, domain=None, stats=None):
    """Spline.integral: a Python float.  ``stats`` (a dict, optional) receives rounds / regions / evaluated."""
    from . import _spline_evaluation as _ev

    if not 1 <= spline.nInd <= MAX_NIND:
        raise NotImplementedError(f"Spline.integral supports nInd 1 to {MAX_NIND} (this spline has nInd {spline.nInd})")
    domain = check_domain(spline, domain)
    lo_hi, span = regions(spline, domain)
    if len(lo_hi) == 0:
        return 0.0
    tables = _ev.device_tables(spline)
    tol = TOLERANCE / spline.nInd
    if tables.dtype == np.float32:
        tol = max(tol, TOLERANCE_F32)

    if integrand is None:
        def round_fn(lh, sp):
            ks = tables.integral_regions(lh, sp)
            return ks[:, 0], ks[:, 1]
    else:
        per_region = 15 ** spline.nInd * (spline.nDep + 2)
        step = max(1, _NODE_CHUNK // per_region)

        def round_fn(lh, sp):
            parts = [node_sums(tables.integral_regions(lh[i:i + step], sp[i:i + step], nodes=True), integrand)
                     for i in range(0, len(lh), step)]
            return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    value, rounds, final, evaluated = adaptive(round_fn, lo_hi, span, domain, tol)
    if stats is not None:
        stats.update(rounds=rounds, regions=final, evaluated=evaluated, nodes=evaluated * 15 ** spline.nInd)
    return float(value)
