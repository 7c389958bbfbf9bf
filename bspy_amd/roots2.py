"""
Isolated common zeros of two scalar splines in two variables: ``Spline.zeros2`` for nInd == nDep == 2 and ``zeros2_batch``
for B systems on the same knots (the reference reaches these through ``Spline.zeros`` -> ``zeros_using_projected_polyhedron``,
bspy/_spline_intersection.py, a serial stack of trimmed splines).  ``Spline.zeros`` itself keeps refusing nInd > 1.

After Bezier extraction of both variables every knot cell holds one polynomial pair in tensor-product Bernstein form,
independent of the others.  Extraction is the band operator of refinement.py, once per axis (``roots.BezierPlan``); almost
all cells fail a sign test on their K0 K1 coefficients (``roots2_flag``); the rest are compacted in index order and each is
walked by one lane (``roots2_isolate``); zeros near a cell edge are found by up to four cells and all but one are dropped
(``roots2_merge``).

    device path   ``bsk_band_apply`` per axis with the rows on the device, ``bsk_roots2_flag``, ``torch.nonzero``,
                  ``bsk_roots2_isolate``, ``bsk_roots2_merge``; no candidates: the last two launches are skipped; no zero
                  near an edge: the last one is
    host path     ``bsk_roots_extract_host`` per axis (the same band operators in the same order, summed as the band kernels
                  sum them), ``bsk_roots2_flag_host``, ``bsk_roots2_isolate_host``, ``bsk_roots2_merge_host``: the same
                  functions of bsk_roots2.hpp on the CPU, for few cells and orders 5 and 6

THE STATEMENT (``flag_cell`` and ``isolate_cell`` say it in plain Python floats, bit for bit what bsk_roots2.hpp computes;
S_d = max |coefficient| of component d of the system, eps of float64):
  * extraction: float64 whatever the coefficient dtype (float32 is widened first); cell (i, j) is the K0 x K1 window of
    both components at first0[i], first1[j] of the extracted rows and covers [t0, t1] x [s0, s1];
  * a zero cell is one on which the K0 x K1 B-spline coefficients of either component are all below S_d eps: it is masked
    and reported once as a cell; no runs are merged and there are no margins;
  * a cell is a candidate unless a component's Bernstein coefficients are all > 0 or all < 0;
  * the walk: a stackless depth-first walk of the binary tree of dyadic boxes of the unit cell.  Depth d splits axis
    d mod 2, DEPTH = 24 halvings per axis.  A node is (depth, path bits), the newest choice in bit 0; the corner of its box
    is computed exactly from the bits.  A live node that is no leaf is halved (lerp at 1/2 keeps the sign a hull has); a
    child is dropped when either component's coefficients are strictly of one sign; the left live child is walked next,
    else the right one, with the halved coefficients.  Otherwise the walk strips the trailing 1 bits (back up), sets
    bit 0 (the right sibling) and restricts the cell's own coefficients to that box: every column by
    ``roots.restrict``, then every row.  Every trip is one visited node; more than WALK of them set status bit 1
    (zeros not isolated);
  * a leaf (width w = 2^-24): at most NEWTON = 8 Newton steps from its centre on the cell's polynomial, value and Jacobian
    by bivariate de Casteljau, Cramer's rule with IEEE division.  An iterate farther than 2 w (max-norm) from the box or a
    determinant of 0 ends it unconverged; it has converged when a step is not smaller than the one before, or when all
    steps shrank and the last one is <= 2^-40.  A converged x inside the cell grown by 2^-44 per axis is clamped to
    [0, 1]^2 and becomes (t0 + x h0, s0 + y h1); it is dropped when this cell has already reported a zero within
    2^-20 h on both axes; R = 2 (K0 - 1)(K1 - 1) slots, a further zero sets status bit 2.  An unconverged leaf with
    |f_d(centre)| <= 4 (K0 + K1) eps S_d for both d sets status bit 4 (a tangential or singular zero; nothing is
    reported); any other one is a near miss;
  * a zero within 2^-20 of an edge of its unit cell is dropped when one of the neighbouring cells (i - 1, j - 1),
    (i - 1, j), (i - 1, j + 1), (i, j - 1) of the same system holds a zero within 2^-20 h on both axes, h the dropping
    cell's widths.  Two true zeros closer than that count as one.
A zero is rounded once to the knots' dtype at the end.  No atomics, no waiting: two runs give the same bytes.

``_path="device" | "host"`` (or ``roots2.FORCE_PATH``) pins the path; ``roots2.LAST_PATHS`` lists what the last call ran.
"""
import numpy as np

from . import _cells
from . import refinement
from . import roots
from ._cells import zero_cells

# Systems x cells from which the device path is taken.  AN ESTIMATE from before the first run of tools/roots2_time.py on an
# MI355X; DESIGN.md section 17 has that run's host / device table (dense random systems cross near 64 x 64 cells).
DEVICE_MIN_CELLS = 4096
DEVICE_MIN_K, DEVICE_MAX_K = 2, 4
HOST_MAX_K = 6
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

EPS = roots.EPS
DEPTH = 24                 # halvings per axis
NEWTON = 8
# nodes a walk may visit: 4 x 5052, the largest count on the recorded cases, rounded up to a power of two
WALK = 32768
LEAF_W = 2.0 ** -24
GROW = 2.0 ** -44
SAME = 2.0 ** -20
SMALL_STEP = 2.0 ** -40
STATUS_WALK, STATUS_SLOTS, STATUS_TANGENT = 1, 2, 4
STATUS_TEXT = {STATUS_WALK: "zeros not isolated", STATUS_SLOTS: "more zeros than slots", STATUS_TANGENT: "tangential or singular zero"}


def slots(K0, K1):
    return 2 * (K0 - 1) * (K1 - 1)


# ------------------------------------------------------------------------------------------ the statement
# a cell is [component 0, component 1], a component a list of K0 rows of K1 floats
def _one_sign(comp):
    flat = [x for row in comp for x in row]
    return all(x > 0.0 for x in flat) or all(x < 0.0 for x in flat)


def excluded(cell):
    return _one_sign(cell[0]) or _one_sign(cell[1])


def _along(comp, axis, f):
    """f on every column (axis 0) or row (axis 1) of a component; f returns a tuple of lines -> a tuple of components."""
    K0, K1 = len(comp), len(comp[0])
    lines = [f([comp[i][j] for i in range(K0)]) for j in range(K1)] if axis == 0 else [f(list(row)) for row in comp]
    outs = []
    for which in range(len(lines[0])):
        if axis == 0:
            outs.append([[lines[j][which][i] for j in range(K1)] for i in range(K0)])
        else:
            outs.append([list(lines[i][which]) for i in range(K0)])
    return tuple(outs)


def halve(cell, axis):
    """(left, right) halves of a cell along ``axis``."""
    parts = [_along(comp, axis, lambda line: roots.split(line, 0.5)) for comp in cell]
    return [parts[0][0], parts[1][0]], [parts[0][1], parts[1][1]]


def restrict_box(cell, lo0, w0, lo1, w1):
    out = []
    for comp in cell:
        comp = _along(comp, 0, lambda line: (roots.restrict(line, lo0, w0),))[0]
        out.append(_along(comp, 1, lambda line: (roots.restrict(line, lo1, w1),))[0])
    return out


def eval1(c, x):
    """Value and derivative of the Bernstein coefficients c at x."""
    b = list(c)
    K = len(b)
    s = 1.0 - x
    for r in range(1, K - 1):
        for i in range(K - r):
            b[i] = s * b[i] + x * b[i + 1]
    return s * b[0] + x * b[1], float(K - 1) * (b[1] - b[0])


def eval2(comp, x0, x1):
    """One component at (x0, x1): value, d/dx0, d/dx1."""
    pq = [eval1(row, x1) for row in comp]
    f, f0 = eval1([p for p, _ in pq], x0)
    return f, f0, roots.value([q for _, q in pq], x0)


def node_box(depth, path):
    i0 = i1 = 0
    w0 = w1 = 1.0
    for k in range(depth):
        bit = (path >> (depth - 1 - k)) & 1
        if k % 2 == 0:
            i0, w0 = 2 * i0 + bit, 0.5 * w0
        else:
            i1, w1 = 2 * i1 + bit, 0.5 * w1
    return float(i0) * w0, w0, float(i1) * w1, w1


def flag_cell(cell, mask):
    """What ``roots2_flag`` writes for one cell."""
    return 0 if mask or excluded(cell) else 1


def _outside(x, lo, w):
    if x != x:
        return float("inf")
    return max(0.0, lo - x, x - (lo + w))


def _leaf(cell, lo0, lo1, t0u, hu, t0v, hv, S0, S1, out, near, R):
    """-> status bits.  Appends at most one zero to ``out`` (and its byte to ``near``)."""
    K0, K1 = len(cell[0]), len(cell[0][0])
    w = LEAF_W
    x0, x1 = lo0 + 0.5 * w, lo1 + 0.5 * w
    prev = last = float("inf")
    fc0 = fc1 = 0.0
    conv = ended = False
    for step in range(NEWTON):
        f, fu, fv = eval2(cell[0], x0, x1)
        g, gu, gv = eval2(cell[1], x0, x1)
        if step == 0:
            fc0, fc1 = f, g
        det = fu * gv - fv * gu
        if det == 0.0:
            ended = True
            break
        du = (f * gv - fv * g) / det
        dv = (fu * g - f * gu) / det
        n0, n1 = x0 - du, x1 - dv
        if not max(_outside(n0, lo0, w), _outside(n1, lo1, w)) <= 2.0 * w:
            ended = True
            break
        x0, x1 = n0, n1
        last = max(abs(du), abs(dv))
        if not last < prev:
            conv = ended = True
            break
        prev = last
    if not ended and last <= SMALL_STEP:
        conv = True
    if not conv:
        tol = 4.0 * (K0 + K1) * EPS
        return STATUS_TANGENT if abs(fc0) <= tol * S0 and abs(fc1) <= tol * S1 else 0
    if not (-GROW <= x0 <= 1.0 + GROW and -GROW <= x1 <= 1.0 + GROW):
        return 0
    x0, x1 = min(max(x0, 0.0), 1.0), min(max(x1, 0.0), 1.0)
    u, v = t0u + x0 * hu, t0v + x1 * hv
    tolu, tolv = SAME * hu, SAME * hv
    if any(abs(a - u) <= tolu and abs(b - v) <= tolv for a, b in out):
        return 0
    if len(out) >= R:
        return STATUS_SLOTS
    out.append((u, v))
    near.append(int(x0 <= SAME or x0 >= 1.0 - SAME or x1 <= SAME or x1 >= 1.0 - SAME))
    return 0


def isolate_cell(cell, t0u, t1u, t0v, t1v, S0, S1, walk=None):
    """What ``roots2_isolate`` returns for one candidate cell, in plain Python floats:
    (zeros [(u, v)], near bytes, status, nodes visited)."""
    K0, K1 = len(cell[0]), len(cell[0][0])
    R = slots(K0, K1)
    cell = [[[float(x) for x in row] for row in comp] for comp in cell]
    hu, hv = t1u - t0u, t1v - t0v
    out, near = [], []
    cur, depth, path = cell, 0, 0
    live, done = True, False
    status = nodes = 0
    for _ in range(WALK if walk is None else walk):
        nodes += 1
        if not live:
            while path & 1:
                path >>= 1
                depth -= 1
            if depth == 0:
                done = True
                break
            path |= 1
            cur = restrict_box(cell, *node_box(depth, path))
            live = not excluded(cur)
        elif depth == 2 * DEPTH:
            lo0, _, lo1, _ = node_box(depth, path)
            status |= _leaf(cell, lo0, lo1, t0u, hu, t0v, hv, S0, S1, out, near, R)
            live = False
        else:
            left, right = halve(cur, depth % 2)
            if not excluded(left):
                cur, path, depth = left, path << 1, depth + 1
            elif not excluded(right):
                cur, path, depth = right, (path << 1) | 1, depth + 1
            else:
                live = False
    if not done:
        status |= STATUS_WALK
    return out, near, status, nodes


def merge_keep(found, flags, cand, breaks0, breaks1):
    """The keep bytes of ``roots2_merge`` in Python: found = the (zeros, near) pairs of the candidates, in their order."""
    nsys, nc0, nc1 = flags.shape
    slot_of = {int(at): n for n, at in enumerate(cand)}
    keep = []
    for n, (zeros, near) in enumerate(found):
        b, cell = divmod(int(cand[n]), nc0 * nc1)
        i, j = divmod(cell, nc1)
        tolu, tolv = SAME * (float(breaks0[i + 1]) - float(breaks0[i])), SAME * (float(breaks1[j + 1]) - float(breaks1[j]))
        row = []
        for (u, v), close in zip(zeros, near):
            k = 1
            if close:
                for ni, nj in ((i - 1, j - 1), (i - 1, j), (i - 1, j + 1), (i, j - 1)):
                    if ni < 0 or nj < 0 or nj >= nc1 or not flags[b, ni, nj]:
                        continue
                    for uu, vv in found[slot_of[(b * nc0 + ni) * nc1 + nj]][0]:
                        if abs(uu - u) <= tolu and abs(vv - v) <= tolv:
                            k = 0
            row.append(k)
        keep.append(row)
    return keep


def statement(rows, plan, mask, scale, walk=None):
    """flags, candidates, zeros (NaN padded), near, count, status, nodes and keep of the extracted rows (B, 2, R0, R1), from
    the functions above: what the host drivers and the kernels return, bit for bit."""
    K0, K1 = plan.order
    R = slots(K0, K1)
    B, nc0, nc1 = mask.shape
    f0, f1 = plan.first

    def cell_of(b, i, j):
        return [[[float(x) for x in rows[b, d, f0[i] + r, f1[j]:f1[j] + K1]] for r in range(K0)] for d in range(2)]

    flags = np.zeros(mask.shape, np.uint8)
    for b in range(B):
        for i in range(nc0):
            for j in range(nc1):
                flags[b, i, j] = flag_cell(cell_of(b, i, j), int(mask[b, i, j]))
    cand = np.flatnonzero(flags).astype(np.int64)
    out = np.full((len(cand), R, 2), np.nan)
    near = np.zeros((len(cand), R), np.uint8)
    count, status, nodes = np.zeros(len(cand), np.int32), np.zeros(len(cand), np.uint8), np.zeros(len(cand), np.int32)
    found = []
    for n, at in enumerate(cand):
        b, cell = divmod(int(at), nc0 * nc1)
        i, j = divmod(cell, nc1)
        zeros, close, status[n], nodes[n] = isolate_cell(cell_of(b, i, j), float(plan.breaks[0][i]), float(plan.breaks[0][i + 1]),
                                                         float(plan.breaks[1][j]), float(plan.breaks[1][j + 1]),
                                                         float(scale[b, 0]), float(scale[b, 1]), walk)
        found.append((zeros, close))
        count[n] = len(zeros)
        out[n, :len(zeros)] = np.array(zeros).reshape(-1, 2)
        near[n, :len(zeros)] = close
    keep = np.zeros((len(cand), R), np.uint8)
    for n, row in enumerate(merge_keep(found, flags, cand, plan.breaks[0], plan.breaks[1])):
        keep[n, :len(row)] = row
    return dict(flags=flags, cand=cand, roots=out, near=near, count=count, status=status, nodes=nodes, keep=keep)


# ------------------------------------------------------------------------------------------ plans and launches
Plan2 = _cells.TensorPlan          # one ``roots.BezierPlan`` per axis; the band steps on the axes 1 and 2 of (M, n0, n1)


def extract_host(data, plan):
    """NumPy (M, n0, n1) float64 -> (M, R0, R1) in Bezier form (``_cells.band_host``)."""
    return _cells.band_host(data, plan.steps, LAST_PATHS)


def _run_host(rows, plan, mask, scale):
    """rows: NumPy float64 (B, 2, R0, R1) in Bezier form; mask: uint8 (B, nc0, nc1); scale: float64 (B, 2).  -> dict of
    flags, cand, roots (ncand, R, 2), near, count, status, nodes, keep (``_cells.isolate_cells``)."""
    rows, scale = np.ascontiguousarray(rows, np.float64), np.ascontiguousarray(scale, np.float64)
    return _cells.isolate_cells(_cells.Host(), "bsk_roots2", rows, plan, mask, scale, slots(*plan.order), LAST_PATHS)


# ------------------------------------------------------------------------------------------ public
def _check_spline(spline):
    if spline.nInd != 2:
        raise NotImplementedError("zeros2: two independent variables only (curves: Spline.zeros)")
    if min(spline.order) < 2 or max(spline.order) > HOST_MAX_K:
        raise NotImplementedError(f"zeros2: orders from 2 to {HOST_MAX_K}; the kernels take orders up to {DEVICE_MAX_K}")


def tables(spline, coefs=None):
    """The host path's tables of a system: (plan, rows (B, 2, R0, R1), mask (B, nc0, nc1), scale (B, 2)), all NumPy."""
    plan = Plan2(spline.order, spline.knots)
    data = np.asarray(spline.coefs if coefs is None else coefs)
    data = data.reshape((-1, 2) + data.shape[-2:]).astype(np.float64)            # float32 is widened BEFORE the extraction
    wide = np.abs(data)
    scale = np.ascontiguousarray(wide.max(axis=(2, 3)))
    small = (wide < (scale * EPS)[:, :, None, None]) | (scale == 0.0)[:, :, None, None]
    mask = zero_cells(small, plan).astype(np.uint8)
    rows = data
    if plan.steps:
        rows = extract_host(data.reshape((-1,) + data.shape[2:]), plan).reshape(data.shape[:2] + tuple(plan.rowlen))
    return plan, rows, mask, scale


def zeros2_batch(spline, coefs=None, _path=None):
    """The isolated common zeros of B systems of two scalar splines in two variables on the spline's knots.
    Returns (values, offsets, cells, status): the zeros of system b are values[offsets[b]:offsets[b + 1]], rows (u, v) in
    the knots' dtype sorted by (u, v); ``cells`` (NumPy float64, m x 5) holds one row (system, u0, u1, v0, v1) per zero cell;
    ``status`` (uint8, B x nc0 x nc1) holds the status bits of every cell (1: zeros not isolated, 2: more zeros than slots,
    4: tangential or singular zero), 0 where all is well.
    ``coefs``: a torch CUDA tensor (B, 2, n0, n1), float32 or float64, takes the place of the spline's coefficients (the
    spline gives the orders and the knots); values, offsets and status are then CUDA tensors.  The table of zero cells (one
    byte per system and cell) is formed on the device and read back; nothing else leaves the device."""
    del LAST_PATHS[:]
    path = _cells.pick_path(_path, FORCE_PATH)
    _check_spline(spline)
    K0, K1 = (int(k) for k in spline.order)
    n0, n1 = (len(spline.knots[d]) - spline.order[d] for d in range(2))
    on_device = coefs is not None and _cells.is_torch(coefs)
    if coefs is None:
        if spline.nDep != 2:
            raise ValueError("zeros2_batch takes two dependent variables, or coefs (B, 2, n0, n1)")
        coefs = spline.coefs[None]
    if on_device:
        import torch
        if not coefs.is_cuda or coefs.dtype not in (torch.float32, torch.float64):
            raise TypeError("zeros2_batch takes the coefficients as a float32 or float64 torch CUDA tensor")
        if path == "host":
            raise ValueError("coefficients on the device take the device path")
        path = "device"
    else:
        coefs = np.asarray(coefs)
    if coefs.ndim != 4 or tuple(coefs.shape[1:]) != (2, n0, n1):
        raise ValueError(f"coefs must have the shape (B, 2, {n0}, {n1})")
    B = int(coefs.shape[0])
    plan = Plan2(spline.order, spline.knots)
    nc0, nc1 = plan.ncells
    kdtype = np.result_type(spline.knots[0].dtype, spline.knots[1].dtype)
    covered = DEVICE_MIN_K <= min(K0, K1) and max(K0, K1) <= DEVICE_MAX_K
    if path is None:
        path = "device" if covered and B * nc0 * nc1 >= DEVICE_MIN_CELLS else "host"
    if path == "device" and not covered:
        raise ValueError(f"the device path covers orders from {DEVICE_MIN_K} to {DEVICE_MAX_K}")

    if B == 0:
        return _cells.collect(_cells.Device(coefs.device) if on_device else _cells.Host(), plan, kdtype, 0)

    if path == "device":
        import torch
        data = (coefs if on_device else torch.from_numpy(np.ascontiguousarray(coefs)).cuda()).double()   # widened BEFORE the extraction
        be = _cells.Device(data.device)
        wide = data.abs()
        scale = wide.amax(dim=(2, 3)).contiguous()
        small = ((wide < (scale * EPS)[:, :, None, None]) | (scale == 0.0)[:, :, None, None]).cpu().numpy()
        mask = zero_cells(small, plan).astype(np.uint8)
        rows = data.reshape((2 * B, n0, n1))
        if plan.steps:
            rows, ran = refinement.run_device(rows, plan.steps)
            LAST_PATHS.extend(ran)
        res = _cells.isolate_cells(be, "bsk_roots2", rows.contiguous(), plan, mask, scale, slots(K0, K1), LAST_PATHS)
    else:
        be = _cells.Host()
        _, rows, mask, scale = tables(spline, coefs)
        res = _run_host(rows, plan, mask, scale)             # makes rows and scale contiguous
    return _cells.collect(be, plan, kdtype, B, slots(K0, K1), res, mask, numpy_out=not on_device)


def zeros2(self, _path=None):
    """``Spline.zeros2``: a list, sorted by (u, v), of length-2 arrays (u, v) in the knots' dtype for isolated zeros and of
    ((u0, v0), (u1, v1)) tuples for cells on which a component vanishes."""
    if not (self.nInd == self.nDep):
        raise ValueError("The number of independent variables (nInd) must match the number of dependent variables (nDep).")
    _check_spline(self)
    values, _, cells, status = zeros2_batch(self, _path=_path)
    if status.any():
        _, i, j = (int(x) for x in np.argwhere(status)[0])
        bits = int(status[0, i, j])
        plan = Plan2(self.order, self.knots)
        u, v = plan.breaks
        why = ", ".join(text for bit, text in STATUS_TEXT.items() if bits & bit)
        raise ValueError(f"zeros2: {why} in the cell [{float(u[i])}, {float(u[i + 1])}] x [{float(v[j])}, {float(v[j + 1])}]")
    kdtype = values.dtype
    found = [((float(r[0]), float(r[1])), r) for r in values]
    for _, u0, u1, v0, v1 in cells.astype(kdtype):
        found.append(((float(u0), float(v0)), ((u0, v0), (u1, v1))))
    found.sort(key=lambda item: item[0])
    return [item[1] for item in found]
