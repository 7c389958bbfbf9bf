"""
TEST INFRASTRUCTURE - NOT PRODUCT CODE.

CPU restatement of Spline.integral's quadrature round (bsk_integral.hpp) in NumPy: the same Gauss-Kronrod 7/15
tensor rule on the same regions, with the point from ``oracle.c_evaluate``, the jacobian from ``oracle.c_jacobian``
and the measure as the product of the jacobian's singular values (checked against np.linalg.svd by
tests/test_integral_host.py), driven by the package's
adaptive driver (bspy_amd/integral.py: cells, acceptance, splitting).
"""
import numpy as np

import oracle
from bspy_amd import integral as _iq

ORACLE_NDEP = 64            # ORC_MAX_NDEP of oracle/bspline_oracle.c


def node_grid(nind):
    """(nInd, 15^nInd) axis indices of the tensor nodes, first variable slowest (the kernel's order)."""
    return np.indices((15,) * nind).reshape(nind, -1)


def measure(jac):
    """Product of the singular values of every (nDep, nInd) jacobian of jac (nDep, nInd, N): the square root of
    the determinant of the smaller Gram matrix (J^T J or J J^T), written out for sizes 1 to 3 (what
    np.linalg.svd returns, at a fraction of its cost on millions of 3 x 2 matrices)."""
    ndep, nind = jac.shape[:2]
    if ndep == nind:
        return np.abs(_det(jac))
    gram = np.einsum("din,djn->ijn", jac, jac) if ndep > nind else np.einsum("din,ein->den", jac, jac)
    return np.sqrt(np.maximum(_det(gram), 0.0))


def _det(m):
    if m.shape[0] == 1:
        return m[0, 0]
    if m.shape[0] == 2:
        return m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def region_sums(spline, lo_hi, span, integrand=None, chunk=8192):
    """(K, G) per region, as bsk_integral's MEASURE mode (integrand None) or the NODES sums."""
    if len(lo_hi) > chunk:
        parts = [region_sums(spline, lo_hi[i:i + chunk], span[i:i + chunk], integrand, chunk)
                 for i in range(0, len(lo_hi), chunk)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    nreg, nind = lo_hi.shape[:2]
    j = node_grid(nind)
    mid = 0.5 * (lo_hi[:, :, 0] + lo_hi[:, :, 1])
    half = 0.5 * (lo_hi[:, :, 1] - lo_hi[:, :, 0])
    pts = [(mid[:, i, None] + half[:, i, None] * _iq.GK_X[j[i]][None, :]).ravel() for i in range(nind)]
    parts = [oracle.c_jacobian(spline.order, spline.nCoef, spline.knots, spline.coefs[d:d + ORACLE_NDEP], pts)
             for d in range(0, spline.nDep, ORACLE_NDEP)]            # the C oracle holds ORC_MAX_NDEP dependents per call
    assert all(bad == -1 for _, bad in parts)
    jac = np.concatenate([p[0] for p in parts])
    mu = measure(np.asarray(jac, np.float64)).reshape(nreg, -1)
    if integrand is not None:
        x, _ = oracle.c_evaluate(spline.order, spline.nCoef, spline.knots, spline.coefs, [0] * nind, pts)
        x = np.asarray(x, np.float64)
        mu = mu * np.array([float(integrand(x[:, n])) for n in range(x.shape[1])]).reshape(nreg, -1)
    vol = np.prod(half, axis=1)[:, None]
    wk = np.prod(_iq.GK_WK[j], axis=0)[None, :] * vol
    wg = np.prod(_iq.GK_WG[j], axis=0)[None, :] * vol
    return np.sum(mu * wk, axis=1), np.sum(mu * wg, axis=1)


def integral_ref(spline, integrand=None, domain=None, stats=None):
    """Spline.integral on the CPU (``spline``: any object with order, nCoef, knots, coefs, nInd, nDep)."""
    domain = _iq.check_domain(spline, domain)
    lo_hi, span = _iq.regions(spline, domain)
    if len(lo_hi) == 0:
        return 0.0
    tol = _iq.TOLERANCE / spline.nInd
    if spline.coefs.dtype == np.float32 and all(np.asarray(k).dtype == np.float32 for k in spline.knots):
        tol = max(tol, _iq.TOLERANCE_F32)
    value, rounds, final, evaluated = _iq.adaptive(lambda lh, sp: region_sums(spline, lh, sp, integrand), lo_hi, span,
                                                   domain, tol)
    if stats is not None:
        stats.update(rounds=rounds, regions=final, evaluated=evaluated)
    return float(value)
