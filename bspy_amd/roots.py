"""
Real roots of scalar spline curves: ``Spline.zeros`` for nInd == nDep == 1 (reference bspy/spline.py:2470 ->
bspy/_spline_intersection.py:12) and ``zeros_batch`` for every component of a curve with any nDep.

After Bezier extraction every knot span is one polynomial in Bernstein form, independent of the others.  Extraction is
one band operator of refinement.py (every interior knot raised to multiplicity K - 1, knots already at K stay, the ends
clamped); almost all spans fail a sign test on their K coefficients (``roots_flag``); the rest are compacted in index
order and each is isolated by one lane, by subdivision in registers (``roots_isolate``).

    device path   ``bsk_band_apply`` (band_apply_line) with the row on the device, ``bsk_roots_flag``, ``torch.nonzero``,
                  ``bsk_roots_isolate``; no candidates: the last launch is skipped
    host path     ``bsk_roots_extract_host``, ``bsk_roots_flag_host``, ``bsk_roots_isolate_host``: the same functions of
                  bsk_roots.hpp on the CPU, for few spans and orders above 8.  The extraction is the same band operator,
                  summed as the band kernels sum it (acc = fma(w, x, acc) in the order of the band): ``bsk_band_apply_host``
                  rounds every product and would differ from the kernels, and so the roots of the two paths, in the last bit

What a root is (S = max |coefficient| of the component, eps of float64, [a, b] the domain):
  * a span whose K B-spline coefficients are all below S eps is a zero span; every maximal run of zero spans is reported
    as (left knot, right knot); in the two spans next to a run no root is reported within sqrt(eps) (b - a) of its end;
  * every sign change inside a span that is not zero is reported once; a span owns [t_j, t_j+1), the last one also b; an
    end coefficient that is exactly 0.0 is a root at that knot, reported by the span that owns it;
  * a touching root shows as a sub-interval of width 2^-50 of the span whose control polygon still has two or more sign
    variations: one root at its midpoint if |f| <= 4 K eps S there;
  * an interior knot of multiplicity K separates independent pieces: a sign change across the jump is no root.

The arithmetic has ONE association on every path (``flag_span`` and ``isolate_span`` state it in plain Python, bit for
bit what bsk_roots.hpp computes): float64 whatever the coefficient dtype (float32 coefficients are widened before the
extraction), every product and sum rounded on its own, de Casteljau steps as (1 - t) * a + t * b, which is exact at both
ends and, at t = 1/2, never leaves [min(a, b), max(a, b)].  A root is rounded once to the knots' dtype at the end.

``_path="device" | "host"`` (or ``roots.FORCE_PATH``) pins the path; ``roots.LAST_PATHS`` lists what the last call ran
("band_apply_line", "roots_flag", "roots_isolate", "host roots_extract", "host roots_flag", "host roots_isolate").
"""
import numpy as np

from . import _cells
from . import _native as nv
from . import refinement
from ._cells import EPS, BezierPlan

# Components x spans from which the device path is taken.  An estimate that the first table of tools/roots_time.py --quick
#  does not move: whole calls take the same time on both paths up to 64 000 coefficients.
DEVICE_MIN_SPANS = 16384
DEVICE_MIN_K, DEVICE_MAX_K = 2, 8
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

DEPTH = 50                 # halvings of a span
BISECT = 60                # steps of the sign bisection
WALK = 128                 # intervals a walk may visit, per K
MASK_SKIP, MASK_LEFT, MASK_RIGHT, MASK_LAST = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------ the statement
def _sign(x):
    return (x > 0.0) - (x < 0.0)


def variations(c):
    """Sign variations of the sequence c, zeros skipped."""
    v, last = 0, 0
    for x in c:
        s = _sign(x)
        if s:
            v += last != 0 and s != last
            last = s
    return v


def _lerp(s, t, a, b):
    return s * a + t * b


def value(c, x):
    b = list(c)
    s = 1.0 - x
    for r in range(1, len(b)):
        for i in range(len(b) - r):
            b[i] = _lerp(s, x, b[i], b[i + 1])
    return b[0]


def split(c, t):
    """de Casteljau at t: (left, right)."""
    b = list(c)
    K = len(b)
    s = 1.0 - t
    left, right = [b[0]] + [0.0] * (K - 1), [0.0] * (K - 1) + [b[K - 1]]
    for r in range(1, K):
        for i in range(K - r):
            b[i] = _lerp(s, t, b[i], b[i + 1])
        left[r] = b[0]
        right[K - 1 - r] = b[K - 1 - r]
    return left, right


def restrict(c, lo, w):
    right = split(c, lo)[1]
    return split(right, w / (1.0 - lo))[0]


def flag_span(c, mask):
    """What ``roots_flag`` writes for one span: c are its K coefficients as Python floats."""
    if mask & MASK_SKIP:
        return 0
    return variations(c) + (c[0] == 0.0) + (bool(mask & MASK_LAST) and c[-1] == 0.0)


def isolate_span(c, t0, t1, mask, margin, S, live=None):
    """What ``roots_isolate`` returns for one span, in plain Python floats: the list of roots, ascending.  ``live``: a list
    that receives the number of live sub-intervals (the one being walked and the waiting ones) at every step; variation
    diminishing keeps it at K - 1 or below, which is asserted."""
    K = len(c)
    c = [float(x) for x in c]
    out = []
    h = t1 - t0
    keep_from, keep_to = t0 + margin, t1 - margin
    touch = 4.0 * K * EPS * S

    def emit(x):
        u = t0 + x * h
        if mask & MASK_LEFT and u <= keep_from:
            return
        if mask & MASK_RIGHT and u >= keep_to:
            return
        if len(out) < K - 1:
            out.append(u)

    if mask & MASK_SKIP:
        return out
    stack = []                                  # waiting right children (lo, w), the nearest first
    cur, lo, w, fresh = list(c), 0.0, 1.0, True
    for _ in range(WALK * K):
        if live is not None:
            live.append(1 + len(stack))
        if fresh and cur[0] == 0.0:
            emit(lo)
        v = variations(cur)
        pop = True
        if v >= 2 and w > 2.0 ** -DEPTH:
            left, right = split(cur, 0.5)
            w = 0.5 * w
            liveL = variations(left) >= 1
            liveR = variations(right) >= 1 or right[0] == 0.0
            if liveL:
                cur, fresh, pop = left, False, False
                if liveR:
                    assert len(stack) + 2 <= max(K - 1, 1), "more than K - 1 live sub-intervals"
                    stack.insert(0, (lo + w, w))
            elif liveR:
                cur, lo, fresh, pop = right, lo + w, True, False
        elif v >= 2:
            x = lo + 0.5 * w
            if abs(value(c, x)) <= touch:
                emit(x)
        elif v == 1:
            sa = next(s for s in map(_sign, cur) if s)
            a, b = lo, lo + w
            for _step in range(BISECT):
                m = 0.5 * (a + b)
                if m == a or m == b:
                    break
                f = value(c, m)
                if f == 0.0:
                    a = b = m
                    break
                if _sign(f) == sa:
                    a = m
                else:
                    b = m
            emit(0.5 * (a + b))
        if pop:
            if not stack:
                break
            lo, w = stack.pop(0)
            cur, fresh = restrict(c, lo, w), True
    if mask & MASK_LAST and c[-1] == 0.0:
        emit(1.0)
    return out


def statement(rows, order, first, mask, breaks, scale, margin, live=None):
    """flags, candidates, roots (NaN padded) and counts of the extracted rows (nDep, rowlen), from the two functions above:
    what the host drivers and the kernels return, bit for bit."""
    K = int(order)
    nDep, nspans = mask.shape
    flags = np.zeros((nDep, nspans), np.uint8)
    for d in range(nDep):
        for s in range(nspans):
            flags[d, s] = flag_span([float(x) for x in rows[d, first[s]:first[s] + K]], int(mask[d, s]))
    cand = np.flatnonzero(flags).astype(np.int64)
    out = np.full((len(cand), K - 1), np.nan)
    count = np.zeros(len(cand), np.int32)
    for i, at in enumerate(cand):
        d, s = divmod(int(at), nspans)
        found = isolate_span(rows[d, first[s]:first[s] + K], float(breaks[s]), float(breaks[s + 1]), int(mask[d, s]),
                             float(margin), float(scale[d]), live)
        out[i, :len(found)] = found
        count[i] = len(found)
    return flags, cand, out, count


# ------------------------------------------------------------------------------------------ plans and tables
def zero_spans(small, plan):
    """small: bool (nDep, nCoef), |coefficient| < S eps.  -> bool (nDep, nspans): all K coefficients of the span are small."""
    k = plan.order
    run = np.concatenate((np.zeros((small.shape[0], 1), np.int64), np.cumsum(small, axis=1, dtype=np.int64)), axis=1)
    return run[:, plan.cell + 1] - run[:, plan.cell + 1 - k] == k


def span_masks(zero, plan):
    """The per-span table of the launches (uint8, nDep x nspans) and the zero runs as rows (component, left, right)."""
    mask = np.zeros(zero.shape, np.uint8)
    mask[zero] |= MASK_SKIP
    mask[:, 1:][zero[:, :-1]] |= MASK_LEFT
    mask[:, :-1][zero[:, 1:]] |= MASK_RIGHT
    mask[:, -1] |= MASK_LAST
    rows = []
    if zero.any():
        edge = np.diff(np.pad(zero.astype(np.int8), ((0, 0), (1, 1))), axis=1)
        for d in np.flatnonzero(zero.any(axis=1)):
            for s0, s1 in zip(np.flatnonzero(edge[d] == 1), np.flatnonzero(edge[d] == -1)):
                rows.append((float(d), float(plan.breaks[s0]), float(plan.breaks[s1])))
    return mask, np.array(rows, np.float64).reshape(-1, 3)


def _last():
    return nv.lib().bsk_roots_last_kernel().decode()


# ------------------------------------------------------------------------------------------ the launches
def extract_host(coefs, plan):
    """NumPy (nDep, nCoef) -> float64 (nDep, rowlen) in Bezier form: the plan's band step, summed as the band kernels do."""
    return _cells.band_host(np.ascontiguousarray(coefs, np.float64), plan.steps, [])   # float32 is widened BEFORE the extraction


def _run(be, rows, plan, mask, scale):
    """rows: the backend's contiguous array (nDep, rowlen), float32 / float64 in Bezier form; mask: NumPy; scale: the
    backend's float64 (nDep).  -> the backend's arrays (cand, roots (ncand, K - 1), count)."""
    k, nDep = plan.order, rows.shape[0]
    with be:
        first, mask = be.put(plan.first, np.int32), be.put(mask, np.uint8)
        grid = (be.code(rows), k, be.ptr(rows), nDep, plan.rowlen, plan.nspans, be.ptr(first), be.ptr(mask))
        flags = be.empty((nDep, plan.nspans), np.uint8)
        be.call("bsk_roots_flag", *grid, be.ptr(flags))
        LAST_PATHS.append(_last())
        cand = be.nonzero(flags)
        roots = be.empty((len(cand), k - 1), np.float64)
        count = be.empty(len(cand), np.int32)
        if len(cand):
            breaks = be.put(plan.breaks, np.float64)
            be.call("bsk_roots_isolate", *grid, be.ptr(breaks), be.ptr(scale), plan.margin, be.ptr(cand), len(cand), be.ptr(roots),
                    be.ptr(count))
            LAST_PATHS.append(_last())
    return cand, roots, count


def _run_host(rows, plan, mask, scale):
    return _run(_cells.Host(), np.ascontiguousarray(rows), plan, mask, scale)


def _run_device(rows, plan, mask, scale):
    return _run(_cells.Device(rows.device), rows, plan, mask, scale)


# ------------------------------------------------------------------------------------------ public
def zeros_batch(spline, coefs=None, _path=None):
    """The real roots of every component of a curve (nInd == 1, any nDep): each dependent variable is a scalar curve on the
    spline's knots.  Returns (values, offsets, intervals): the isolated roots of component d are
    values[offsets[d]:offsets[d + 1]], ascending, in the knots' dtype; ``intervals`` (NumPy float64, n x 3) holds one row
    (component, left, right) per interval on which a component is zero.
    ``coefs``: a torch CUDA tensor (nDep, nCoef), float32 or float64, takes the place of the spline's coefficients (the
    spline gives the order and the knots); values and offsets are then CUDA tensors.  The table of zero spans (one byte
    per component and span) is formed on the device and read back; nothing else leaves the device."""
    del LAST_PATHS[:]
    path = _cells.pick_path(_path, FORCE_PATH)
    if spline.nInd != 1:
        raise ValueError("zeros_batch takes a curve (nInd == 1)")
    k, t = spline.order[0], spline.knots[0]
    coefs, on_device, path = _cells.coefs_arg("zeros_batch", spline.coefs if coefs is None else coefs, path, (len(t) - k,),
                                              f"(nDep, {len(t) - k})")
    nDep = int(coefs.shape[0])
    plan = BezierPlan(k, t)
    kdtype = t.dtype

    def empty():
        be = _cells.backend_of(coefs)
        return be.empty(0, kdtype), be.zeros(nDep + 1, np.int64)

    if nDep == 0:
        return (*empty(), np.empty((0, 3)))
    if on_device:
        wide = coefs.abs().double()
        d_scale = wide.amax(dim=1)
        small = ((wide < (d_scale * EPS)[:, None]) | (d_scale == 0.0)[:, None]).cpu().numpy()
    else:
        wide = np.abs(coefs.astype(np.float64, copy=False))
        scale = np.ascontiguousarray(wide.max(axis=1))
        small = (wide < (scale * EPS)[:, None]) | (scale == 0.0)[:, None]
    mask, intervals = span_masks(zero_spans(small, plan), plan)
    if k < 2:                                               # piecewise constants: zero spans are all there is
        return (*empty(), intervals)
    covered = DEVICE_MIN_K <= k <= DEVICE_MAX_K
    if path is None:
        path = "device" if covered and nDep * plan.nspans >= DEVICE_MIN_SPANS else "host"
    if path == "device":
        if not covered:
            raise ValueError(f"the device path covers orders from {DEVICE_MIN_K} to {DEVICE_MAX_K}")
        import torch
        rows = coefs if on_device else torch.from_numpy(np.ascontiguousarray(coefs)).cuda()
        if not on_device:
            d_scale = torch.from_numpy(scale).to(rows.device)
        if plan.steps:
            rows, ran = refinement.run_device(rows.double(), plan.steps)     # float32 is widened BEFORE the extraction
            LAST_PATHS.extend(ran)
        cand, roots, count = _run_device(rows.contiguous(), plan, mask, d_scale.contiguous())
        values = roots[~torch.isnan(roots)].to(getattr(torch, kdtype.name))
        comp = torch.div(cand, plan.nspans, rounding_mode="floor")
        total = torch.cat((torch.zeros(1, dtype=torch.int64, device=rows.device), torch.cumsum(count.to(torch.int64), 0)))
        offsets = total[torch.searchsorted(comp, torch.arange(nDep + 1, device=rows.device))]
        if not on_device:
            values, offsets = values.cpu().numpy(), offsets.cpu().numpy()
        return values, offsets, intervals
    if k > nv.BSK_MAX_ORDER:
        raise NotImplementedError(f"zeros: orders above {nv.BSK_MAX_ORDER} are out of scope")
    rows = coefs
    if plan.steps:
        rows = _cells.band_host(np.ascontiguousarray(coefs, np.float64), plan.steps, LAST_PATHS)   # widened BEFORE the extraction
    cand, roots, count = _run_host(rows, plan, mask, scale)
    values = roots[~np.isnan(roots)].astype(kdtype)
    per = np.bincount(cand // plan.nspans, weights=count, minlength=nDep).astype(np.int64)
    return values, np.concatenate(([0], np.cumsum(per))).astype(np.int64), intervals


def zeros(self, epsilon=None, initialScale=None, _path=None):
    """``epsilon`` and ``initialScale`` are accepted and ignored, as the reference's curve path ignores them."""
    if not (self.nInd == self.nDep):
        raise ValueError("The number of independent variables (nInd) must match the number of dependent variables (nDep).")
    if self.nInd > 1:
        raise NotImplementedError("zeros: curves only (nInd == nDep == 1); the projected-polyhedron solver of the reference "
                                  "for nInd > 1 is deliberately out of scope")
    if self.nInd == 0:
        return []
    values, _, intervals = zeros_batch(self, _path=_path)
    found = [(v, v) for v in values] + [(left, (left, right)) for left, right in intervals[:, 1:].astype(self.knots[0].dtype)]
    found.sort(key=lambda item: item[0])
    return [item[1] for item in found]
