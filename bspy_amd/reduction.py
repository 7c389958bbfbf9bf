"""
Data reduction: ``remove_knot`` and ``remove_knots`` (reference bspy/_spline_domain.py:452 and :518), ``range_bounds``
(bspy/_spline_evaluation.py:248).

Removing knot i of a variable of order k is linear in the coefficients: the k new coefficients of the window are the
least-squares solution of the (k + 1) x k bidiagonal system that re-inserting the knot would have to satisfy, a fixed
combination of the k + 1 old ones with weights that depend on the knots only, and the residual of that system is one
linear functional of the same k + 1 coefficients.  Removals whose windows do not overlap do not see each other.  So
both are ``BandMap`` operators with K = k + 1 (``removal_map``, ``residual_map``), built on the host by running the
reference's elimination (substitution of the nLeft / nRight fixed unknowns, Givens rotations, back substitution) on
the unit matrix in ``numpy.longdouble`` and rounding once to fp64.

The statement of ``remove_knots(tolerance, nLeft, nRight)``, identical on the host and device paths.  It is not the
reference's serial greedy loop.

    S_d = max |coefs[d]| of the input, 1 where that is 0 (the reference's range-bound scales).  The data is never
    pre-scaled: untouched coefficients keep their bits.  Variables are reduced in the order 0 .. nInd - 1.
    For each variable, repeat:
      1. rho_i = max_d (max over all lines of dependent variable d of |residual_i|) / S_d for every interior knot
         index i = order .. nCoef - 1; a value that is not finite counts as +inf.
      2. The candidates are the i with rho_i <= tolerance, sorted by (rho_i, i).  Walk that list and keep i when it is
         at least order + 1 away from every index kept so far (``select``).
      3. The certificate of the kept set: apply ``removal_map``; refine the candidate back to the ORIGINAL input's
         knots in every variable reduced so far (``refinement.refine_map``, the steps in ``refinement._ordered``'s
         order); E_d = max |original - refined| per dependent variable.  The set is accepted when
         max_d E_d / S_d <= tolerance.  B-splines are non-negative and sum to 1, so this bounds the sup-norm error
         of the whole result against the input, cumulatively over rounds and variables.
      4. A refused set of m > 1 indices is cut to its first floor(m / 2) indices, in the order they were kept, and
         step 3 is repeated.
      5. A refused single knot finishes the variable.
      6. An accepted set is applied and the loop returns to step 1.
      7. No candidates: the variable is finished.

Arithmetic: every band operator (removal, residual, the refinements of the certificate) is the chain
acc = fma(w[t], x[t], acc) from 0 in the order of t in fp64, rounded once to the data's type.  That is what the band
kernels compute (DESIGN.md sections 17 and 18); the host path uses ``bsk_band_apply_fma_host`` and
``bsk_band_absmax_host``.  A maximum is exact.  Therefore both paths take the same decisions and return the same bits.

    device path   the coefficient tensor goes to the device once; per round ``bsk_band_absmax`` (band_absmax /
                  band_absmax_line + band_absmax_fold) for the residuals, one ``bsk_band_apply`` for the removal,
                  ``refinement.run_steps`` for all but the last refinement step of the certificate and the maxima
                  against ``minus=original`` for the last one: the refined tensor of the original's size is not
                  written for that step.  Only the (groups, nOut) maxima cross to the host.
    host path     the same operators on the CPU: small tensors, and K = order + 1 above 8

Both paths are one loop on a backend of bspy_amd/_backend.py (``Host`` or ``Device``).

``_path="device" | "host"`` (or ``reduction.FORCE_PATH``) pins the path; a spline with a variable of order above 7 takes
the host path whatever is asked.  ``LAST_PATHS`` lists the kernels of the last call, ``LAST_ROUNDS`` per variable the
list of knot indices removed in each round.
"""
import numpy as np

from . import refinement
from ._backend import Device, Host, is_torch, lines, pick_path
from .refinement import BandMap

# Elements of the coefficient tensor from which remove_knots takes the device path: the whole call on both paths
# crosses between 12 288 and 27 648 elements on an MI355X (tools/remove_time.py).
DEVICE_MIN_ELEMENTS = 1 << 14
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []
LAST_ROUNDS = []


# ------------------------------------------------------------------------------------------ operators
def _eliminate(knots, order, idx, extraLeft, extraRight):
    """The reference's remove_knot on the unit matrix, for the knot indices ``idx`` (all with the same numbers of fixed
    unknowns), in numpy.longdouble.  Returns (W, v): W (n, k, k + 1) the rows of the k new coefficients, v (n, k + 1) the
    row whose absolute value is the residual."""
    k = int(order)
    t = np.asarray(knots, np.float64).astype(np.longdouble)
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    one = np.longdouble(1)
    diag0 = np.zeros((n, k), np.longdouble)
    diag1 = np.zeros((n, k + 1), np.longdouble)
    diag1[:, 0] = one
    with np.errstate(divide="ignore", invalid="ignore"):
        for ix in range(1, k):
            alpha = (t[idx + ix] - t[idx]) / (t[idx + ix] - t[idx + ix - k])
            diag0[:, ix - 1] = alpha
            diag1[:, ix] = one - alpha
        diag0[:, k - 1] = one
        rhs = np.broadcast_to(np.eye(k + 1, dtype=np.longdouble), (n, k + 1, k + 1)).copy()

        for ix in range(extraLeft):
            rhs[:, ix] /= diag1[:, ix, None]
            rhs[:, ix + 1] -= diag0[:, ix, None] * rhs[:, ix]
        for ix in range(extraRight):
            rhs[:, -1 - ix] /= diag0[:, -1 - ix, None]
            rhs[:, -2 - ix] -= diag1[:, -2 - ix, None] * rhs[:, -1 - ix]
        for ix in range(extraLeft, k - extraRight):
            cos, sin = diag1[:, ix].copy(), diag0[:, ix].copy()
            denom = np.sqrt(cos ** 2 + sin ** 2)
            cos /= denom
            sin /= denom
            diag1[:, ix] = denom
            diag0[:, ix] = sin * diag1[:, ix + 1]
            diag1[:, ix + 1] *= cos
            temp = cos[:, None] * rhs[:, ix] + sin[:, None] * rhs[:, ix + 1]
            rhs[:, ix + 1] = cos[:, None] * rhs[:, ix + 1] - sin[:, None] * rhs[:, ix]
            rhs[:, ix] = temp
        for ix in range(1 + extraRight, k - extraLeft):
            rhs[:, -1 - ix] /= diag1[:, -1 - ix, None]
            rhs[:, -2 - ix] -= diag0[:, -1 - ix, None] * rhs[:, -1 - ix]
        rhs[:, -1 - k + extraLeft] /= diag1[:, -1 - k + extraLeft, None]
    v = rhs[:, k - extraRight].copy()
    for ix in range(extraRight):
        rhs[:, k - extraRight + ix] = rhs[:, k + 1 - extraRight + ix]
    return rhs[:, :k], v


def _rows(knots, order, indices, nLeft, nRight):
    """(W, v) as fp64 for the knot indices ``indices``: W (n, k, k + 1), v (n, k + 1)."""
    k = int(order)
    nCoef = len(knots) - k
    indices = np.asarray(indices, np.int64)
    W = np.zeros((len(indices), k, k + 1), np.float64)
    v = np.zeros((len(indices), k + 1), np.float64)
    extraLeft = np.maximum(0, nLeft - indices + k)
    extraRight = np.maximum(0, nRight - nCoef + indices + 1)
    for eL, eR in sorted(set(zip(extraLeft.tolist(), extraRight.tolist()))):
        take = np.nonzero((extraLeft == eL) & (extraRight == eR))[0]
        if eL + eR > k:
            W[take], v[take] = np.nan, np.nan          # more fixed unknowns than unknowns: no such removal
            continue
        Wl, vl = _eliminate(knots, k, indices[take], int(eL), int(eR))
        W[take], v[take] = Wl.astype(np.float64), vl.astype(np.float64)
    return W, v


def _check_indices(knots, order, indices):
    k = int(order)
    nCoef = len(knots) - k
    indices = np.asarray(indices, np.int64).reshape(-1)
    if len(indices) and (indices.min() < k or indices.max() >= nCoef):
        raise ValueError("Must specify interior knots for removal")
    ranked = np.sort(indices)
    if len(ranked) > 1 and np.diff(ranked).min() < k + 1:
        raise ValueError("removal_map: the knot indices must be pairwise at least order + 1 apart")
    return ranked


def removal_map(knots, order, indices, nLeft=0, nRight=0):
    """One BandMap with K = order + 1 that removes all knots ``indices`` (pairwise at least order + 1 apart) at once:
    returns (newKnots, first, w).  Rows outside the windows are exact unit rows."""
    knots = np.asarray(knots)
    k = int(order)
    K = k + 1
    nIn = len(knots) - k
    ranked = _check_indices(knots, k, indices)
    W, _ = _rows(knots, k, ranked, nLeft, nRight)
    if not np.all(np.isfinite(W)):
        raise ValueError("remove_knot: an operator weight is not finite (a fixed unknown whose pivot is zero); "
                         "the reference returns inf / nan coefficients")
    nOut = nIn - len(ranked)
    first = np.zeros(nOut, np.int32)
    w = np.zeros((nOut, K), np.float64)
    j = np.arange(nOut)
    old = j + np.searchsorted(ranked - np.arange(len(ranked)), j, "right")      # unit rows: the old coefficient kept
    first[:] = np.minimum(old, nIn - K)
    w[j, old - first] = 1.0
    for s, i in enumerate(ranked):
        rows = np.arange(i - k - s, i - s)
        first[rows] = i - k
        w[rows] = W[s]
    return np.delete(knots, ranked), first, w


def residual_map(knots, order, nLeft=0, nRight=0):
    """(indices, first, v): one row per interior knot index order .. nCoef - 1, K = order + 1; |row . line| is the residual
    ``remove_knot`` reports for that knot.  A row of a knot that cannot be removed holds values that are not finite."""
    k = int(order)
    nCoef = len(knots) - k
    indices = np.arange(k, nCoef, dtype=np.int64)
    _, v = _rows(knots, k, indices, nLeft, nRight)
    return indices, (indices - k).astype(np.int32), v


def select(rho, order, tolerance):
    """Step 2 of the statement: rho[p] belongs to knot index order + p.  Returns the kept knot indices in the order
    they were kept."""
    kept = []
    ranked = sorted((float(r), order + p) for p, r in enumerate(rho) if r <= tolerance)
    for _, i in ranked:
        if all(abs(i - other) >= order + 1 for other in kept):
            kept.append(i)
    return kept


# ------------------------------------------------------------------------------------------ maxima
def _absmax(be, band, data, axis, groups, minus=None):
    """The launch of ``absmax`` and ``absmax_host``: data (and minus, or None), the entered backend's contiguous arrays;
    axis not negative.  Returns the backend's (groups, band.nOut) float64."""
    outer, inner = lines(data.shape, axis, band.nIn)
    out = be.empty((groups, band.nOut), np.float64)
    be.call("bsk_band_absmax", band._handle, be.code(data), be.ptr(data), outer, inner, groups, be.ptr(minus), be.ptr(out))
    return out


def absmax(band, tensor, axis, groups=1, minus=None):
    """out[g][j] = max over the lines of group g of |(band applied along ``axis``)[j] - minus| for a torch CUDA tensor
    (float32 / float64); groups divides the product of the extents in front of ``axis``; minus: None or a CUDA tensor of
    the result's shape.  Returns a (groups, band.nOut) float64 CUDA tensor.  ``LAST_PATHS`` holds this call's kernel."""
    import torch
    if not (is_torch(tensor) and tensor.is_cuda):
        raise TypeError("reduction.absmax takes a torch CUDA tensor")
    if tensor.dtype not in (torch.float32, torch.float64):
        raise TypeError("reduction.absmax takes float32 or float64")
    axis = axis % tensor.dim()
    if 0 in lines(tensor.shape, axis, band.nIn):
        raise ValueError("reduction.absmax: empty tensor")
    shape = list(tensor.shape)
    shape[axis] = band.nOut
    if minus is not None:
        if list(minus.shape) != shape or minus.dtype != tensor.dtype or minus.device != tensor.device:
            raise ValueError("reduction.absmax: minus must have the result's shape, type and device")
        minus = minus.contiguous()
    with Device(tensor.device) as be:
        out = _absmax(be, band, tensor.contiguous(), axis, groups, minus)
    LAST_PATHS[:] = [band.last_kernel()]
    return out


def absmax_host(band, a, axis, groups=1, minus=None):
    """The same values for NumPy arrays (``bsk_band_absmax_host``): (groups, band.nOut) float64."""
    a = np.ascontiguousarray(a)
    if minus is not None:
        minus = np.ascontiguousarray(minus, a.dtype)
    return _absmax(Host(), band, a, axis % a.ndim, groups, minus)


def apply_fma_host(band, a, axis):
    """``band`` along ``axis`` of a NumPy array with the kernels' fused sums (``bsk_band_apply_fma_host``)."""
    a = np.ascontiguousarray(a)
    return band.along(Host(), a, axis % a.ndim, fused=True)


def _maxima(be, first, w, data, axis, groups, minus=None):
    """``_absmax`` of the band (first, w) on the entered backend's array, brought to NumPy: of a round only these maxima
    cross to the host.  ``LAST_PATHS`` receives what ran."""
    with BandMap(first, w, data.shape[axis]) as band:
        out = be.get(_absmax(be, band, data, axis, groups, minus))
        LAST_PATHS.append(band.last_kernel())
    return out


def _origin(knots, original):
    """For every knot of ``original`` the index of the knot of ``knots`` (a sub-multiset) it is, or -1: the copies of a
    value that ``knots`` holds stand first (``refinement.merged_knots``' convention)."""
    origin = np.full(len(original), -1, np.int64)
    lo = np.searchsorted(knots, original, "left")
    have = np.searchsorted(knots, original, "right") - lo
    rank = np.arange(len(original)) - np.searchsorted(original, original, "left")
    keep = rank < have
    origin[keep] = (lo + rank)[keep]
    return origin


def _certificate(be, candidate, original, order, knots, original_knots, reduced, nDep):
    """E_d of the statement's step 3 for the backend's tensor ``candidate`` on ``knots`` against ``original``."""
    steps = []
    for iv in reduced:
        if len(knots[iv]) != len(original_knots[iv]):
            origin = _origin(knots[iv], original_knots[iv])
            steps.append((iv + 1, *refinement.refine_map(knots[iv], order[iv], original_knots[iv], 0, origin=origin)))
    steps = refinement._ordered(steps, candidate.shape)
    data = refinement.run_steps(be, candidate, steps[:-1], LAST_PATHS, fused=True)
    axis, first, w = steps[-1]
    return _maxima(be, first, w, data, axis, nDep, original).max(axis=1)


def _finite_or_inf(a):
    return np.where(np.isfinite(a), a, np.inf)


def remove_knots(self, tolerance=1e-14, nLeft=0, nRight=0, _path=None):
    path = pick_path(_path, FORCE_PATH)
    del LAST_PATHS[:]
    LAST_ROUNDS[:] = [[] for _ in range(self.nInd)]
    coefs = np.ascontiguousarray(self.coefs)
    order, knots = list(self.order), [np.array(t) for t in self.knots]
    if self.nInd == 0 or coefs.size == 0:
        return refinement._rebuild(self, order, knots, coefs.copy())
    covered = all(refinement.DEVICE_MIN_K <= k + 1 <= refinement.DEVICE_MAX_K for k in order)
    if path is None:
        path = "device" if coefs.size >= DEVICE_MIN_ELEMENTS else "host"
    if not covered:
        path = "host"                       # bsk_band_absmax: BSK_ERR_UNSUPPORTED for K outside [2, 8]
    be = Device.current() if path == "device" else Host()

    nDep = self.nDep
    scale = np.abs(coefs.reshape(nDep, -1)).max(axis=1).astype(np.float64)
    scale[scale == 0.0] = 1.0
    original_knots = [np.asarray(t, np.float64) for t in self.knots]
    original = data = be.put(coefs, coefs.dtype)
    with be:
        for iv in range(self.nInd):
            k, axis = order[iv], iv + 1
            reduced = range(iv + 1)
            while len(knots[iv]) - k > k:
                t = knots[iv]
                _, first, v = residual_map(t, k, nLeft, nRight)
                bad = ~np.all(np.isfinite(v), axis=1)
                v[bad] = 0.0
                res = _maxima(be, first, v, data, axis, nDep)
                rho = _finite_or_inf((res / scale[:, None]).max(axis=0))
                rho[bad] = np.inf
                kept = select(rho, k, tolerance)
                accepted = False
                while kept:
                    try:
                        newKnots, first, w = removal_map(t, k, kept, nLeft, nRight)
                    except ValueError:
                        break                   # a weight that is not finite: this set has no removal
                    candidate = refinement.run_steps(be, data, [(axis, first, w)], LAST_PATHS, fused=True)
                    trial = [np.asarray(x, np.float64) for x in knots]
                    trial[iv] = np.asarray(newKnots, np.float64)
                    E = _certificate(be, candidate, original, order, trial, original_knots, reduced, nDep)
                    if np.max(_finite_or_inf(E / scale)) <= tolerance:
                        accepted = True
                        break
                    kept = kept[:len(kept) // 2]
                if not accepted:
                    break
                data, knots[iv] = candidate, newKnots
                LAST_ROUNDS[iv].append([int(i) for i in kept])
    result = be.get(data)
    if result is coefs:
        result = coefs.copy()
    return refinement._rebuild(self, order, knots, result)


def remove_knot(self, iKnot, nLeft=0, nRight=0):
    if self.nInd != 1:
        raise ValueError("Must have one independent variable")
    k = self.order[0]
    if iKnot < k or iKnot >= self.nCoef[0]:
        raise ValueError("Must specify interior knots for removal")
    del LAST_PATHS[:]
    t = self.knots[0]
    newKnots, first, w = removal_map(t, k, [iKnot], nLeft, nRight)
    _, v = _rows(t, k, [iKnot], nLeft, nRight)
    if not np.all(np.isfinite(v)):
        raise ValueError("remove_knot: an operator weight is not finite (a fixed unknown whose pivot is zero); "
                         "the reference returns inf / nan coefficients")
    coefs = np.ascontiguousarray(self.coefs)
    out = refinement.run_steps(Host(), coefs, [(1, first, w)], LAST_PATHS, fused=True)
    with BandMap(np.zeros(1, np.int32), v, k + 1) as band:
        residual = apply_fma_host(band, coefs[:, iKnot - k:iKnot + 1], 1)
    return type(self)(1, self.nDep, self.order, out.shape[1:], [newKnots], out), np.abs(residual[:, 0])


def range_bounds(self):
    return np.array([[c.min(), c.max()] for c in self.coefs], self.coefs.dtype)
