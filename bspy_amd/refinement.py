"""
Spline to spline: ``insert_knots``, ``elevate``, ``elevate_and_insert_knots``, ``trim``, ``clamp`` and ``differentiate``
(reference bspy/_spline_domain.py:32, :110, :341, :610 and bspy/_spline_operations.py:244).

For one independent variable each of these is one small banded linear operator, the same for every line of the
coefficient tensor along that variable: ``out[j] = sum_t w[j, t] * in[first[j] + t]`` (``BandMap``).  The knot-vector
logic (the reference's checks, messages and resulting knots, bit for bit) and the construction of the operator are
host work in this file; streaming the lines through the operator is the expensive part:

    device path   ``bsk_band_apply``: band_apply (lanes along the inner extent) or band_apply_line (the last variable,
                  whose lines are contiguous); a multi-variable call keeps the intermediate tensors on the device
    host path     ``bsk_band_apply_host``: the same operator on the CPU, for small tensors and K above 8

The refinement operator is exact linear algebra, built by blossoming: new coefficient j of the spline of order k + m
on the knots tbar is the blossom of the order-elevated polynomial piece of one old knot cell mu inside the support of
new basis function j, at tbar[j + 1 .. j + k + m - 1]; the elevated blossom is the mean over the (k - 1)-subsets of its
arguments of the piece's own blossom, which the multi-affine de Boor recurrence on cell mu gives as weights on the old
coefficients mu - k + 1 .. mu.  No derivative is taken and nothing is integrated back, so the operator's error is a
few ulp whatever the knot spacing.

``trim_plan``, ``clamp_box`` and ``elevate_plan`` are the knot logic of trim, clamp and elevate_and_insert_knots without the
coefficients (they return the band steps); ``run_device`` applies steps to a CUDA tensor and returns one: bspy_amd/sums.py
plans ``common_basis`` with them and keeps the intermediates of ``add`` on the device.

``_path="device" | "host"`` (or ``refinement.FORCE_PATH``) pins the path; ``refinement.LAST_PATHS`` lists what every
variable of the last call ran ("band_apply", "band_apply_line", "host band").
"""
import ctypes
import itertools

import numpy as np

from ._backend import FLOATS, Device, Handle, Host, choose, is_torch, lines, pick_path

# Elements of the coefficient tensor (the larger of input and result) from which the device path is taken.  The key is
# the total element count: see DESIGN.md section 13 for its standing.
DEVICE_MIN_ELEMENTS = 1 << 16
DEVICE_MIN_K, DEVICE_MAX_K = 2, 8
UNCOVERED = f"the device path covers K from {DEVICE_MIN_K} to {DEVICE_MAX_K}"
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []


class BandMap(Handle):
    """out[j] = sum_t w[j, t] * in[first[j] + t] (``bsk_band`` handle).  first: (nOut,) non-decreasing; w: (nOut, K)."""
    prefix = "bsk_band"

    def __init__(self, first, w, nIn):
        self.first = np.ascontiguousarray(first, np.int32)
        self.w = np.ascontiguousarray(w, np.float64)
        self.nOut, self.K = self.w.shape
        self.nIn = int(nIn)
        self._open(self.nIn, self.nOut, self.K, self.first.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.w.ctypes.data)

    def apply_line(self, x):
        """One line in NumPy, the statement of what the library computes: fp64 products added in the order of t."""
        x = np.asarray(x)
        acc = np.zeros(self.nOut, np.float64)
        for t in range(self.K):
            acc += self.w[:, t] * x[self.first + t].astype(np.float64)
        return acc.astype(x.dtype)

    def apply(self, be, a, outer, inner, fused=False):
        """The launch: a, the entered backend's contiguous float32 / float64 array of outer * nIn * inner values ->
        (outer, nOut, inner), same type.  fused: sums as the kernels form them; on the host that is an entry point of
        its own, which has no device twin."""
        code = be.code(a)
        out = be.empty((outer, self.nOut, inner), FLOATS[code])
        name = "bsk_band_apply_fma" if fused and isinstance(be, Host) else "bsk_band_apply"
        be.call(name, self._handle, code, be.ptr(a), outer, inner, be.ptr(out))
        return out

    def apply_host(self, a, outer, inner):
        """a: NumPy float32 / float64 of outer * nIn * inner values -> (outer, nOut, inner), same dtype."""
        return self.apply(Host(), np.ascontiguousarray(a), outer, inner)

    def apply_device(self, a, outer, inner):
        """a: contiguous torch CUDA tensor of outer * nIn * inner float32 / float64 -> (outer, nOut, inner), same dtype."""
        with Device(a.device) as be:
            return self.apply(be, a, outer, inner)

    def along(self, be, data, axis, fused=False):
        """``apply`` along ``axis`` (not negative) of the backend's contiguous array: the result has nOut entries there.
        A tensor without lines launches nothing."""
        shape = list(data.shape)
        outer, inner = lines(shape, axis, self.nIn)
        shape[axis] = self.nOut
        if outer * inner == 0:
            return be.empty(shape, FLOATS[be.code(data)])
        if type(be) is Host and not fused:                  # under its public name, which callers may wrap
            return self.apply_host(data, outer, inner).reshape(shape)
        return self.apply(be, data, outer, inner, fused).reshape(shape)


# ------------------------------------------------------------------------------------------ operators
def support_cell(newKnots, j, n):
    """For the rows j of an operator onto ``newKnots`` whose blossoms take n arguments: the non-empty new cell nearest
    the middle of the support newKnots[j .. j + n + 1] (the lower one of two equally near)."""
    tb = newKnots
    cell = np.full(len(j), -1)
    for off in sorted(range(n + 1), key=lambda o: (abs(o - 0.5 * n), o)):
        c = j + off
        take = (cell < 0) & (tb[c + 1] > tb[c])
        cell[take] = c[take]
    cell[cell < 0] = (j + n // 2)[cell < 0]
    return cell


def knot_cell(knots, order, x):
    """The cell mu of ``knots`` (float64) that holds x, clipped to the domain's cells order - 1 .. nCoef - 1."""
    t, k = knots, order
    nIn = len(t) - k
    hi = t[nIn]
    mu = np.searchsorted(t, x, "right") - 1
    mu[x >= hi] = np.searchsorted(t, hi, "left") - 1
    return np.clip(mu, k - 1, nIn - 1)


def blossom_weights(knots, order, first, args):
    """Multi-affine de Boor recurrence: the weights (rows, k) on the coefficients first .. first + k - 1 of the blossom of
    the polynomial piece on cell first + k - 1 at the k - 1 arguments args[row].  ``knots`` and ``args`` (rows, k - 1)
    come in the precision the recurrence is to run in."""
    t, k = knots, order
    D = np.broadcast_to(np.eye(k, dtype=t.dtype), (len(first), k, k)).copy()              # D[row, p] = weights of d_p on the k old coefficients
    for r in range(1, k):
        u = args[:, r - 1]
        for q in range(k - 1, r - 1, -1):
            i = first + q
            left, right = t[i], t[i + k - r]
            den = right - left
            D[:, q] = ((right - u) / den)[:, None] * D[:, q - 1] + ((u - left) / den)[:, None] * D[:, q]
    return D[:, k - 1]


def row_exists(newKnots, j, n, lo, hi):
    """Rows j whose basis function on ``newKnots`` (blossoms of n arguments) has a non-empty cell inside [lo, hi]; the
    others hold the coefficients of a polynomial extension."""
    tb = newKnots
    exists = np.zeros(len(j), bool)
    for off in range(n + 1):
        c = j + off
        exists |= (tb[c + 1] > tb[c]) & (tb[c] >= lo) & (tb[c + 1] <= hi)
    return exists


def weight_support(knots, order, newKnots, m, j, first):
    """(rows, k) mask of the weights w[row, q], on old coefficient i = first[row] + q, that are not zero in exact
    arithmetic, from the knots alone (the support condition of the discrete B-spline).  Old basis function i, raised
    by m, is a positive combination of exactly the new basis functions on the windows of k + m + 1 consecutive knots of
    its own refined knots: t[i .. i + k], every distinct value m times more, and the new knots strictly inside.  Those
    agree with ``newKnots`` inside (t[i], t[i + k]), so row j carries old coefficient i exactly when
    newKnots[j .. j + k + m] lies in [t[i], t[i + k]] and holds no more copies of either end than that."""
    t, tb, k = knots, newKnots, int(order)
    n = k + m - 1
    i = first[:, None] + np.arange(k)                                   # (rows, k)
    tlo, thi = t[i], t[i + k]
    # copies of t[i] (of t[i + k]) among t[i .. i + k]
    span = t[i[:, :, None] + np.arange(k + 1)]
    a = (span == tlo[:, :, None]).sum(axis=2)
    b = (span == thi[:, :, None]).sum(axis=2)
    window = tb[j[:, None] + np.arange(n + 2)]                          # (rows, k + m + 1)
    head = (window == window[:, :1]).sum(axis=1)[:, None]
    tail = (window == window[:, -1:]).sum(axis=1)[:, None]
    wlo, whi = window[:, :1], window[:, -1:]
    return (wlo >= tlo) & (whi <= thi) & ((wlo > tlo) | (head <= a + m)) & ((whi < thi) | (tail <= b + m))


def refine_map(knots, order, newKnots, m=0, rows=None, origin=None):
    """BandMap arrays (first, w) that take the coefficients on ``knots`` (order k) to those of the same function on
    ``newKnots`` (order k + m), for the output rows ``rows`` (a slice; default all).  ``newKnots`` must hold every
    distinct knot of ``knots`` with at least its multiplicity + m.  ``origin`` (m == 0): for every new knot the index
    of the old knot it is, or -1 for an inserted one; a row whose blossom arguments are consecutive old knots is then
    the exact unit row.
    Rows whose support has no cell inside the domain take the domain's nearest cell: they hold the coefficients of
    the polynomial extension of that piece.
    Every weight of a row that exists whose exact value is zero is stored as 0.0 and none is negative, for every m and
    for the ``rows=`` and ``origin=`` forms (``weight_support``): an output never sees an input it has no weight on,
    whatever that input's magnitude, and a row is a convex combination.  Should the recurrence round a weight that is
    positive in exact arithmetic to zero or below (it has to be smaller than the recurrence's own rounding error for
    that; no operator of the tests does it), the smallest positive double is stored in its place, so that the stored
    pattern stays the exact one; the weights themselves still come from the recurrence on the chosen cell, whose
    error grows with the ratio of the knot gaps involved."""
    t = np.asarray(knots, np.float64)
    tb = np.asarray(newKnots, np.float64)
    k = int(order)
    n = k + m - 1                                   # arguments of the elevated blossom
    nIn, nOut = len(t) - k, len(tb) - k - m
    j = np.arange(nOut)[rows if rows is not None else slice(None)]
    cell = support_cell(tb, j, n)
    lo, hi = t[k - 1], t[nIn]
    x = np.clip(0.5 * (tb[cell] + tb[cell + 1]), lo, hi)
    first = knot_cell(t, k, x) - k + 1

    # the recurrence runs in extended precision where the platform has it (x86: 64-bit mantissa), so that the
    # weights are correctly rounded doubles but for rare ties while the knot gaps are of one scale; elsewhere it runs in double
    t, tb = t.astype(np.longdouble), tb.astype(np.longdouble)
    w = np.zeros((len(j), k), np.longdouble)
    subsets = list(itertools.combinations(range(n), k - 1))
    for subset in subsets:
        w += blossom_weights(t, k, first, tb[j[:, None] + 1 + np.array(subset, np.int64)])
    w = (w / len(subsets)).astype(np.float64)
    # the recurrence leaves rounding residue (either sign) where cancellation gives an exact zero: those entries are
    # decided by the knots alone.  A weight of a row that exists is positive where it is not zero; the recurrence
    # can round a positive weight below 1e-19 to the other side, which is stored as the smallest positive double
    exists = row_exists(tb, j, n, lo, hi)
    zero = ~weight_support(np.asarray(knots, np.float64), k, np.asarray(newKnots, np.float64), m, j, first)
    w[exists[:, None] & zero] = 0.0
    w[exists[:, None] & ~zero & (w <= 0.0)] = np.finfo(np.float64).tiny
    if m == 0 and origin is not None and k > 1:
        # the blossom's arguments are k - 1 consecutive old knots: the value is the old coefficient in front of them
        origin = np.asarray(origin)
        old = origin[j + 1] - 1
        unit = origin[j + 1] >= 0
        for s in range(2, k):
            unit &= origin[j + s] == old + s
        unit &= (old >= first) & (old < first + k)
        w[unit] = 0.0
        w[unit, (old - first)[unit]] = 1.0
    return first.astype(np.int32), w


def differentiate_map(knots, order):
    """(first, w) of the derivative's coefficients: K = 2, w = (-alpha_j, alpha_j), alpha_j = (k - 1) / (t[j + k] - t[j + 1]).
    Two limits of this form: an interior knot of multiplicity k makes alpha_j infinite (``differentiate`` refuses such a
    spline; the reference returns inf / nan), and -alpha c[j] + alpha c[j + 1] rounds two products where
    alpha (c[j + 1] - c[j]) rounds one difference, so for coefficients with a large common offset the error relative to
    the derivative's coefficients grows as eps |c| / |c[j + 1] - c[j]|; relative to alpha |c| it stays at eps."""
    t = np.asarray(knots, np.float64)
    k = int(order)
    n = len(t) - k - 1
    with np.errstate(divide="ignore"):
        alpha = (k - 1) / (t[k:k + n] - t[1:1 + n])
    return np.arange(n, dtype=np.int32), np.stack([-alpha, alpha], axis=1)


# ------------------------------------------------------------------------------------------ application
def apply(band, tensor, axis):
    """Apply ``band`` along ``axis`` of a torch CUDA tensor (float32 / float64); returns a new CUDA tensor of the same
    type whose extent along ``axis`` is band.nOut.  For pipelines that stay on the device.  ``LAST_PATHS`` holds this
    call's kernel only (``band.last_kernel()`` says the same)."""
    out = _apply(band, tensor, axis)
    LAST_PATHS[:] = [band.last_kernel()] if out.numel() else []
    return out


def _device_floats(tensor):
    """What every device-resident entry point takes: a torch CUDA tensor of float32 or float64."""
    import torch
    if not (is_torch(tensor) and tensor.is_cuda):
        raise TypeError("refinement.apply takes a torch CUDA tensor")
    if tensor.dtype not in (torch.float32, torch.float64):
        raise TypeError("refinement.apply takes float32 or float64")


def _apply(band, tensor, axis):
    _device_floats(tensor)
    axis = axis % tensor.dim()
    lines(tensor.shape, axis, band.nIn)                      # (this message comes before the next one)
    if not (DEVICE_MIN_K <= band.K <= DEVICE_MAX_K):
        raise ValueError(UNCOVERED)
    with Device(tensor.device) as be:
        return band.along(be, tensor.contiguous(), axis)


def _ordered(steps, shape):
    """The step that shrinks the tensor most first, the one that grows it most last (the operators of different
    variables commute)."""
    return sorted(steps, key=lambda s: len(s[1]) / shape[s[0]])


def steps_covered(steps):
    """Whether the band kernels cover every step (K of the device instantiations)."""
    return all(DEVICE_MIN_K <= np.shape(w)[1] <= DEVICE_MAX_K for _, _, w in steps)


def run_steps(be, data, steps, log, fused=False):
    """The band pipeline: data, the entered backend's contiguous array (nDep, *nCoef), through steps [(axis, first, w)]
    in ``_ordered``'s order, one ``BandMap`` per step; the intermediates stay where the backend keeps them.  ``log``
    receives what every step ran (nothing for an empty result); fused: ``BandMap.apply``'s.  Returns the backend's array."""
    for axis, first, w in _ordered(steps, data.shape):
        with BandMap(first, w, data.shape[axis]) as band:
            data = band.along(be, data, axis, fused)
            if 0 not in data.shape:
                log.append(band.last_kernel())
    return data


def run_device(data, steps):
    """data: torch CUDA tensor (nDep, *nCoef); steps: [(axis, first, w)].  Applies every step with the band kernels and
    returns the CUDA tensor: the intermediates of a pipeline stay on the device.  Returns (tensor, kernels that ran)."""
    _device_floats(data)
    if not steps_covered(steps):
        raise ValueError(UNCOVERED)
    ran = []
    with Device(data.device) as be:
        return run_steps(be, data.contiguous(), steps, ran), ran


def _run(coefs, steps, path):
    """coefs: NumPy (nDep, *nCoef); steps: [(axis, first, w)].  Applies every step (``run_steps``) and returns NumPy."""
    path = pick_path(path, FORCE_PATH)
    del LAST_PATHS[:]
    if not steps:
        return coefs
    steps = _ordered(steps, coefs.shape)
    if coefs.size == 0:
        shape = list(coefs.shape)
        for axis, first, w in steps:
            with BandMap(first, w, shape[axis]) as band:            # the library still checks the step
                shape[axis] = band.nOut
        return np.empty(shape, coefs.dtype)
    size = coefs.size
    for axis, first, _ in steps:
        size = max(size, size // coefs.shape[axis] * len(first))
    path = choose(path, steps_covered(steps), size >= DEVICE_MIN_ELEMENTS, UNCOVERED)
    with (Device.current() if path == "device" else Host()) as be:
        return be.get(run_steps(be, be.put(coefs, coefs.dtype), steps, LAST_PATHS))


# ------------------------------------------------------------------------------------------ knot vectors
def merged_knots(knots, order, entries):
    """Knots of one variable after insert_knots' ``entries`` (values or (value, multiplicity) pairs, taken in turn as the
    reference takes them: a pair with multiplicity < 1 is skipped unseen, a value is cast to the knots' dtype, must lie
    in the domain, and may not raise a knot's multiplicity, with what the list has added so far, above the order).
    Returns (merged, origin): origin[i] is the index of the old knot that merged[i] is, or -1 for a new one; new knots
    stand behind old knots of the same value.  ``knots`` itself comes back when the list adds nothing."""
    lo, hi = knots[order - 1], knots[len(knots) - order]
    added = {}
    for entry in entries:
        value, times = (entry, 1) if np.isscalar(entry) else (entry[0], entry[1])
        if times < 1:
            continue
        value = knots.dtype.type(value)
        if value < lo or value > hi:
            raise ValueError(f"Knot insertion outside domain: {value}")
        if int(np.count_nonzero(knots == value)) + added.get(value, 0) + times > order:
            raise ValueError("Knot multiplicity > order")
        added[value] = added.get(value, 0) + times
    if not added:
        return knots, np.arange(len(knots))
    fresh = np.repeat(np.array(list(added), knots.dtype), list(added.values()))
    both = np.concatenate((knots, fresh))
    rank = np.argsort(both, kind="stable")              # stable: equal values keep old before new
    return both[rank], np.where(rank < len(knots), rank, -1)


def _rebuild(spline, order, knots, coefs):
    return type(spline)(spline.nInd, spline.nDep, order, coefs.shape[1:], knots, coefs, spline.metadata)


def insert_knots(self, newKnots, _path=None):
    del LAST_PATHS[:]
    if len(newKnots) != self.nInd:
        raise ValueError("Invalid newKnots")
    if self.nInd == 0:
        return self
    knots, steps = list(self.knots), []
    for iv, entries in enumerate(newKnots):
        merged, origin = merged_knots(self.knots[iv], self.order[iv], entries)
        if merged is not self.knots[iv]:
            knots[iv] = merged
            steps.append((iv + 1, *refine_map(self.knots[iv], self.order[iv], merged, 0, origin=origin)))
    return _rebuild(self, self.order, knots, _run(self.coefs, steps, _path))


def _bound_plan(knots, order, value, eps, right):
    """Where a trim bound lands and how many copies of it have to be inserted for full multiplicity: the bound snaps to
    a distinct knot less than eps above it, else to one less than eps below it.  For a right bound that snaps downwards
    the reference counts the copies of the FIRST distinct knot as present (its observable result, pinned by goldens)."""
    distinct, counts = np.unique(knots, return_counts=True)
    above = int(np.searchsorted(distinct, value))
    if distinct[above] - value < eps:
        return distinct[above], order - counts[above]
    if above > 0 and value - distinct[above - 1] < eps:
        return distinct[above - 1], order - (counts[0] if right else counts[above - 1])
    return value, order


def trim_plan(order, knots, newDomain):
    """What ``trim`` does to a spline with these orders and knots, without its coefficients: None when the spline itself
    comes back, else (knots of the result, band steps [(axis, first, w)])."""
    nInd = len(order)
    box = np.array(newDomain, knots[0].dtype, copy=True)            # None becomes nan: that side is kept
    eps = np.finfo(box.dtype).eps

    entries, changed = [], False
    for iv, bounds in enumerate(box):
        if len(bounds) != 2:
            raise ValueError("Invalid newDomain")
        t, k = knots[iv], order[iv]
        ends = (t[k - 1], t[len(t) - k])
        wanted = []
        for side in (0, 1):
            if np.isnan(bounds[side]):
                continue
            if not (ends[0] <= bounds[side] <= ends[1]):
                raise ValueError("Invalid newDomain")
            if side == 1 and not np.isnan(bounds[0]) and not (bounds[0] < bounds[1]):
                raise ValueError("Invalid newDomain")
            bounds[side], missing = _bound_plan(t, k, bounds[side], eps, side == 1)
            if missing > 0:
                wanted.append((bounds[side], missing))
            changed = changed or missing > 0 or bounds[side] != ends[side]
        entries.append(wanted)
    if not changed:
        return None

    # one operator per variable: the insertion at the bounds, restricted to the rows between them
    out, steps = [], []
    for iv, (wanted, (lower, upper)) in enumerate(zip(entries, box)):
        t, k = knots[iv], order[iv]
        merged, origin = merged_knots(t, k, wanted)
        row0 = 0 if np.isnan(lower) else int(np.searchsorted(merged, lower))
        row1 = len(merged) - k if np.isnan(upper) else int(np.searchsorted(merged, upper))
        out.append(merged[row0:row1 + k])
        if merged is not t or (row0, row1) != (0, len(t) - k):
            steps.append((iv + 1, *refine_map(t, k, merged, 0, rows=slice(row0, row1), origin=origin)))
    assert len(out) == nInd
    return out, steps


def trim(self, newDomain, _path=None):
    del LAST_PATHS[:]                        # also when the spline itself is returned: nothing ran
    if len(newDomain) != self.nInd:
        raise ValueError("Invalid newDomain")
    if self.nInd < 1:
        return self
    plan = trim_plan(self.order, self.knots, newDomain)
    if plan is None:
        return self
    knots, steps = plan
    return _rebuild(self, self.order, knots, _run(self.coefs, steps, _path))


def clamp_box(order, knots, left, right):
    """The trim box of ``clamp``: the spline's own domain on the listed sides, None elsewhere."""
    variables = range(len(order))
    left, right = {variables[i] for i in left}, {variables[i] for i in right}
    ends = [(t[k - 1], t[len(t) - k]) for t, k in zip(knots, order)]
    return [[lo if iv in left else None, hi if iv in right else None] for iv, (lo, hi) in enumerate(ends)]


def clamp(self, left, right, _path=None):
    """A trim to the spline's own domain on the listed sides."""
    return trim(self, clamp_box(self.order, self.knots, left, right), _path)


def elevated_knots(knots, order, m, newKnots):
    """Knots of a left-clamped variable after elevation by m with the plain values ``newKnots`` added (the reference's
    rule): a distinct old knot gets multiplicity min(max(its count with the new values, its old count + m), order + m),
    a distinct new value keeps its count.  The result has the dtype of the concatenation, as the reference's has."""
    old, old_count = np.unique(knots, return_counts=True)
    values, count = np.unique(np.concatenate((knots, np.ravel(newKnots))), return_counts=True)
    at = np.searchsorted(values, old)
    count[at] = np.minimum(np.maximum(count[at], old_count + m), order + m)
    return np.repeat(values, count)


def elevate_plan(order, knots, m, newKnots):
    """What ``elevate_and_insert_knots`` does to a spline with these orders and knots, without its coefficients: None when
    the spline itself comes back, else (orders, knots of the result, band steps of the left clamp, band steps of the
    elevation and insertion)."""
    nInd = len(order)
    if len(m) != nInd:
        raise ValueError("Invalid m")
    if len(newKnots) != nInd:
        raise ValueError("Invalid newKnots")
    touched = []
    for iv, (raise_by, values) in enumerate(zip(m, newKnots)):
        if not (raise_by >= 0):
            raise ValueError("Invalid m")
        if raise_by + len(values) > 0:
            touched.append(iv)
    if not touched:
        return None
    # the knot rule and the operator assume a clamped left end
    clamped = trim_plan(order, knots, clamp_box(order, knots, touched, []))
    base, clamp_steps = clamped if clamped is not None else (knots, [])
    order, knots, steps = list(order), list(base), []
    for iv in touched:
        k, raise_by = order[iv], int(m[iv])
        knots[iv] = elevated_knots(base[iv], k, raise_by, newKnots[iv])
        order[iv] = k + raise_by
        steps.append((iv + 1, *refine_map(base[iv], k, knots[iv], raise_by)))
    return order, knots, clamp_steps, steps


def elevate_and_insert_knots(self, m, newKnots, _path=None):
    del LAST_PATHS[:]
    plan = elevate_plan(self.order, self.knots, m, newKnots)
    if plan is None:
        return self
    order, knots, clamp_steps, steps = plan
    base = _run(self.coefs, clamp_steps, _path)
    clamp_paths = list(LAST_PATHS)
    coefs = _run(base, steps, _path)
    LAST_PATHS[:0] = clamp_paths
    return _rebuild(self, order, knots, coefs)


def elevate(self, m, _path=None):
    return elevate_and_insert_knots(self, m, self.nInd * [[]], _path)


def differentiate(self, with_respect_to=0, _path=None):
    del LAST_PATHS[:]
    if not (0 <= with_respect_to < self.nInd) or not (self.order[with_respect_to] > 1):
        raise ValueError("Invalid with_respect_to")
    iv = with_respect_to
    first, w = differentiate_map(self.knots[iv], self.order[iv])
    if not np.all(np.isfinite(w)):
        raise ValueError("differentiate: an interior knot of full multiplicity (a discontinuous spline) has no derivative "
                         "spline here; the reference returns inf / nan coefficients")
    order, knots = list(self.order), list(self.knots)
    order[iv] -= 1
    knots[iv] = self.knots[iv][1:-1]
    return _rebuild(self, order, knots, _run(self.coefs, [(iv + 1, first, w)], _path))
