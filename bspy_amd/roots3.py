"""
Isolated common zeros of three scalar splines in three variables: ``Spline.zeros3`` for nInd == nDep == 3 and
``zeros3_batch`` for B systems on the same knots (the reference reaches these through ``Spline.zeros`` ->
``zeros_using_projected_polyhedron``, bspy/_spline_intersection.py, a serial stack of trimmed splines).  ``Spline.zeros``
keeps refusing nInd > 1 and ``Spline.zeros2`` nInd != 2.

After Bezier extraction of the three variables every knot cell holds one polynomial triple in tensor-product Bernstein form,
independent of the others.  Extraction is the band operator of refinement.py, once per axis (``roots.BezierPlan``); almost
all cells fail a sign test on their K0 K1 K2 coefficients (``roots3_flag``); the rest are compacted in index order and each
is walked by ONE WAVE, lane = coefficient (``roots3_isolate``); zeros near a cell face are found by up to eight cells and
all but one are dropped (``roots3_merge``).

    device path   ``bsk_band_apply`` per axis with the rows on the device, ``bsk_roots3_flag``, ``torch.nonzero``,
                  ``bsk_roots3_isolate``, ``bsk_roots3_merge``; no candidates: the last two launches are skipped; no zero
                  near a face: the last one is
    host path     ``bsk_roots_extract_host`` per axis (the same band operators in the same order, summed as the band kernels
                  sum them), ``bsk_roots3_flag_host``, ``bsk_roots3_isolate_host``, ``bsk_roots3_merge_host``: the same
                  functions of bsk_roots3.hpp on the CPU, a lane array becoming a loop over 64 entries

THE STATEMENT (``flag_cell``, ``isolate_cell`` and ``merge_keep`` say it in plain Python floats, bit for bit what
bsk_roots3.hpp computes; S_d = max |coefficient| of component d of the system, eps of float64):
  * extraction: float64 whatever the coefficient dtype (float32 is widened first); the axes in the order
    ``refinement._ordered`` gives the device path; cell (i, j, k) is the K0 x K1 x K2 window of the three components at
    first0[i], first1[j], first2[k] of the extracted rows and covers [u0, u1] x [v0, v1] x [w0, w1];
  * a zero cell is one on which the K0 x K1 x K2 B-spline coefficients of any component are all below S_d eps: it is
    masked and reported once as a cell; no runs are merged and there are no margins;
  * a cell is a candidate unless a component's Bernstein coefficients are all > 0 or all < 0;
  * the walk: a stackless depth-first walk of the binary tree of dyadic boxes of the unit cell.  Depth d splits axis
    d mod 3, DEPTH = 19 halvings per axis: a node is (depth, path bits) in one 64-bit integer, 6 bits of depth and
    3 x 19 = 57 path bits, and 19 is the most that fits; the leaves should be as small as the node allows, because what a
    tangential zero leaves at the centre of a leaf shrinks with the square of its width.  The newest choice is bit 0 of the
    path; the corner of a box is computed exactly from the bits.  A live node that is no leaf is halved (lerp at 1/2 keeps
    the sign a hull has); a half is dropped when a component's coefficients are strictly of one sign; the left live half is
    walked next, else the right one, with the halved coefficients.  Otherwise the walk strips the trailing 1 bits (back
    up), sets bit 0 (the right sibling) and REBUILDS that box from the cell's own coefficients BY RESTRICTION, not by
    replaying the path: ``roots.restrict`` along axis 0, then axis 1, then axis 2 (6 (K - 1) lerp rounds at most, where a
    replay takes up to 56 (K - 1)).  Every trip is one visited node; more than WALK of them set status bit 1 (zeros not
    isolated);
  * a leaf (width w = 2^-19): at most NEWTON = 8 Newton steps from its centre on the cell's polynomial, value and 3 x 3
    Jacobian by trivariate de Casteljau (axis 2, then 1, then 0), Cramer's rule with IEEE division, every determinant as
    (a00 m0 - a01 m1) + a02 m2 with the minors m = a11 a22 - a12 a21, a10 a22 - a12 a20, a10 a21 - a11 a20.  An iterate
    farther than 2 w (max-norm) from the box or a determinant of 0 ends it unconverged; it has converged when a step is not
    smaller than the one before, or when all steps shrank and the last one is <= 2^-40.  A converged x inside the cell
    grown by 2^-44 per axis is clamped to [0, 1]^3 and becomes t0 + x h per axis; it is dropped when this cell has already
    reported a zero within SAME h = 2^-20 h on all three axes; R = min(6 (K0 - 1)(K1 - 1)(K2 - 1), 32) slots (the mixed
    volume bound capped: 32 isolated zeros in one knot cell are not a case anybody has), a further zero sets status bit 2.
    An unconverged leaf with |f_d(centre)| <= 4 (K0 + K1 + K2) w^2 S_d for all three d sets status bit 4 (a tangential or
    singular zero; nothing is reported).  In the form c (K0 + K1 + K2) eps S_d this is c = 4 w^2 / eps = 2^18: a component
    that vanishes to second order in a leaf is at its centre below (3 / 8) w^2 max |second derivative|, and the second
    derivatives of a Bernstein polynomial stay below 4 (K - 1)(K - 2) S_d; the leaf of section 17's c = 4 is 2^-24 wide,
    which a 64-bit node cannot reach in three variables.  Any other unconverged leaf is a near miss;
  * a zero within SAME of a face of its unit cell is dropped when one of the 13 neighbouring cells that precede it in
    flat index, (i - 1, *, *), (i, j - 1, *), (i, j, k - 1), of the same system holds a zero within SAME h on all axes, h the
    dropping cell's widths.  Two true zeros closer than that count as one.
A zero is rounded once to the knots' dtype at the end.  No atomics, no waiting: two runs give the same bytes, and so do
the two paths.

``_path="device" | "host"`` (or ``roots3.FORCE_PATH``) pins the path; ``roots3.LAST_PATHS`` lists what the last call ran.
"""
import numpy as np

from . import _cells
from . import refinement
from . import roots
from ._cells import zero_cells

# Systems x cells from which the device path is taken.  Measured with tools/roots3_time.py on an MI355X:
# on candidate-dense systems the device wins from 8 cells on and by a factor 2 at 64; on sparse ones the host wins up to
# about 7000 cells, by at most the 6 ms a device call costs whatever its size.
DEVICE_MIN_CELLS = 64
MIN_K, MAX_K = 2, 4
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

EPS = roots.EPS
DEPTH = 19                 # halvings per axis: 3 x 19 path bits and 6 bits of depth in one 64-bit node
NEWTON = 8
# nodes a walk may visit: 4 x 4065, the largest count on the recorded cases, rounded up to a power of two
WALK = 16384
LEAF_W = 2.0 ** -19
GROW = 2.0 ** -44
SAME = 2.0 ** -20
SMALL_STEP = 2.0 ** -40
TANGENT = 2.0 ** -36       # 4 w^2
MAX_SLOTS = 32
STATUS_WALK, STATUS_SLOTS, STATUS_TANGENT = 1, 2, 4
STATUS_TEXT = {STATUS_WALK: "zeros not isolated", STATUS_SLOTS: "more zeros than slots", STATUS_TANGENT: "tangential or singular zero"}


def slots(K0, K1, K2):
    return min(6 * (K0 - 1) * (K1 - 1) * (K2 - 1), MAX_SLOTS)


# ------------------------------------------------------------------------------------------ the statement
# a cell is (dims, [component 0, 1, 2]); a component is the flat list of its K0 K1 K2 floats, the last index fastest
def _one_sign(comp):
    return all(x > 0.0 for x in comp) or all(x < 0.0 for x in comp)


def excluded(cell):
    return any(_one_sign(comp) for comp in cell[1])


def _along(dims, comp, axis, f):
    """f on every line of a component along ``axis``; f returns a tuple of lines -> a tuple of components."""
    stride = [dims[1] * dims[2], dims[2], 1][axis]
    K = dims[axis]
    outs = None
    for start in range(len(comp)):
        if (start // stride) % K:
            continue
        res = f([comp[start + e * stride] for e in range(K)])
        if outs is None:
            outs = [list(comp) for _ in res]
        for which, line in enumerate(res):
            for e in range(len(line)):
                outs[which][start + e * stride] = line[e]
    return tuple(outs)


def halve(cell, axis):
    """(left, right) halves of a cell along ``axis``."""
    dims, comps = cell
    parts = [_along(dims, comp, axis, lambda line: roots.split(line, 0.5)) for comp in comps]
    return (dims, [p[0] for p in parts]), (dims, [p[1] for p in parts])


def restrict_box(cell, lo, w):
    dims, comps = cell
    out = []
    for comp in comps:
        for axis in range(3):
            comp = _along(dims, comp, axis, lambda line: (roots.restrict(line, lo[axis], w[axis]),))[0]
        out.append(comp)
    return dims, out


def eval1(c, x):
    """Value and derivative of the Bernstein coefficients c at x."""
    b = list(c)
    K = len(b)
    s = 1.0 - x
    for r in range(1, K - 1):
        for i in range(K - r):
            b[i] = s * b[i] + x * b[i + 1]
    return s * b[0] + x * b[1], float(K - 1) * (b[1] - b[0])


def eval3(dims, comp, x):
    """One component at x: value, d/dx0, d/dx1, d/dx2 (axis 2 first, then 1, then 0)."""
    K0, K1, K2 = dims
    pq = [[eval1(comp[(i * K1 + j) * K2:(i * K1 + j + 1) * K2], x[2]) for j in range(K1)] for i in range(K0)]
    pv, pd, qv = [], [], []
    for i in range(K0):
        v, d = eval1([p for p, _ in pq[i]], x[1])
        pv.append(v)
        pd.append(d)
        qv.append(eval1([q for _, q in pq[i]], x[1])[0])
    f, f0 = eval1(pv, x[0])
    return f, f0, eval1(pd, x[0])[0], eval1(qv, x[0])[0]


def det3(a00, a01, a02, a10, a11, a12, a20, a21, a22):
    m0 = a11 * a22 - a12 * a21
    m1 = a10 * a22 - a12 * a20
    m2 = a10 * a21 - a11 * a20
    return (a00 * m0 - a01 * m1) + a02 * m2


def node_box(depth, path):
    at, w = [0, 0, 0], [1.0, 1.0, 1.0]
    for k in range(depth):
        bit = (path >> (depth - 1 - k)) & 1
        at[k % 3], w[k % 3] = 2 * at[k % 3] + bit, 0.5 * w[k % 3]
    return [float(at[a]) * w[a] for a in range(3)], w


def flag_cell(cell, mask):
    """What ``roots3_flag`` writes for one cell."""
    return 0 if mask or excluded(cell) else 1


def _outside(x, lo, w):
    if x != x:
        return float("inf")
    return max(0.0, lo - x, x - (lo + w))


def _leaf(cell, lo, t0, h, S, out, near, R):
    """-> status bits.  Appends at most one zero to ``out`` (and its byte to ``near``)."""
    dims, comps = cell
    w = LEAF_W
    x = [lo[a] + 0.5 * w for a in range(3)]
    prev = last = float("inf")
    fc = [0.0, 0.0, 0.0]
    conv = ended = False
    for step in range(NEWTON):
        FJ = [eval3(dims, comp, x) for comp in comps]
        F = [fj[0] for fj in FJ]
        J = [fj[1:] for fj in FJ]
        if step == 0:
            fc = list(F)
        det = det3(*J[0], *J[1], *J[2])
        if det == 0.0:
            ended = True
            break
        d = [det3(F[0], J[0][1], J[0][2], F[1], J[1][1], J[1][2], F[2], J[2][1], J[2][2]) / det,
             det3(J[0][0], F[0], J[0][2], J[1][0], F[1], J[1][2], J[2][0], F[2], J[2][2]) / det,
             det3(J[0][0], J[0][1], F[0], J[1][0], J[1][1], F[1], J[2][0], J[2][1], F[2]) / det]
        n = [x[a] - d[a] for a in range(3)]
        if not max(_outside(n[a], lo[a], w) for a in range(3)) <= 2.0 * w:
            ended = True
            break
        x = n
        last = max(abs(d[0]), abs(d[1]), abs(d[2]))
        if not last < prev:
            conv = ended = True
            break
        prev = last
    if not ended and last <= SMALL_STEP:
        conv = True
    if not conv:
        tol = float(sum(dims)) * TANGENT
        return STATUS_TANGENT if all(abs(fc[d]) <= tol * S[d] for d in range(3)) else 0
    if not all(-GROW <= x[a] <= 1.0 + GROW for a in range(3)):
        return 0
    x = [min(max(x[a], 0.0), 1.0) for a in range(3)]
    u = tuple(t0[a] + x[a] * h[a] for a in range(3))
    tol = [SAME * h[a] for a in range(3)]
    if any(all(abs(z[a] - u[a]) <= tol[a] for a in range(3)) for z in out):
        return 0
    if len(out) >= R:
        return STATUS_SLOTS
    out.append(u)
    near.append(int(any(x[a] <= SAME or x[a] >= 1.0 - SAME for a in range(3))))
    return 0


def isolate_cell(cell, t0, t1, S, walk=None):
    """What ``roots3_isolate`` returns for one candidate cell, in plain Python floats:
    (zeros [(u, v, w)], near bytes, status, nodes visited)."""
    dims, comps = cell
    R = slots(*dims)
    cell = (dims, [[float(x) for x in comp] for comp in comps])
    h = [t1[a] - t0[a] for a in range(3)]
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
        elif depth == 3 * DEPTH:
            status |= _leaf(cell, node_box(depth, path)[0], t0, h, S, out, near, R)
            live = False
        else:
            left, right = halve(cur, depth % 3)
            if not excluded(left):
                cur, path, depth = left, path << 1, depth + 1
            elif not excluded(right):
                cur, path, depth = right, (path << 1) | 1, depth + 1
            else:
                live = False
    if not done:
        status |= STATUS_WALK
    return out, near, status, nodes


def merge_keep(found, flags, cand, breaks):
    """The keep bytes of ``roots3_merge`` in Python: found = the (zeros, near) pairs of the candidates, in their order."""
    nsys, nc0, nc1, nc2 = flags.shape
    slot_of = {int(at): n for n, at in enumerate(cand)}
    before = [(di, dj, dk) for di in (-1, 0, 1) for dj in (-1, 0, 1) for dk in (-1, 0, 1)][:13]
    keep = []
    for n, (zeros, near) in enumerate(found):
        b, cell = divmod(int(cand[n]), nc0 * nc1 * nc2)
        ijk = (cell // (nc1 * nc2), (cell // nc2) % nc1, cell % nc2)
        tol = [SAME * (float(breaks[a][ijk[a] + 1]) - float(breaks[a][ijk[a]])) for a in range(3)]
        row = []
        for z, close in zip(zeros, near):
            k = 1
            if close:
                for delta in before:
                    ni, nj, nk = (ijk[a] + delta[a] for a in range(3))
                    if min(ni, nj, nk) < 0 or ni >= nc0 or nj >= nc1 or nk >= nc2 or not flags[b, ni, nj, nk]:
                        continue
                    for other in found[slot_of[((b * nc0 + ni) * nc1 + nj) * nc2 + nk]][0]:
                        if all(abs(other[a] - z[a]) <= tol[a] for a in range(3)):
                            k = 0
            row.append(k)
        keep.append(row)
    return keep


def statement(rows, plan, mask, scale, walk=None):
    """flags, candidates, zeros (NaN padded), near, count, status, nodes and keep of the extracted rows (B, 3, R0, R1, R2),
    from the functions above: what the host drivers and the kernels return, bit for bit."""
    K0, K1, K2 = plan.order
    R = slots(K0, K1, K2)
    B, nc0, nc1, nc2 = mask.shape
    f0, f1, f2 = plan.first

    def cell_of(b, i, j, k):
        return plan.order, [[float(x) for x in rows[b, d, f0[i]:f0[i] + K0, f1[j]:f1[j] + K1, f2[k]:f2[k] + K2].reshape(-1)]
                            for d in range(3)]

    def where(at):
        b, cell = divmod(int(at), nc0 * nc1 * nc2)
        return b, cell // (nc1 * nc2), (cell // nc2) % nc1, cell % nc2

    flags = np.zeros(mask.shape, np.uint8)
    for at in range(mask.size):
        flags[where(at)] = flag_cell(cell_of(*where(at)), int(mask[where(at)]))
    cand = np.flatnonzero(flags).astype(np.int64)
    out = np.full((len(cand), R, 3), np.nan)
    near = np.zeros((len(cand), R), np.uint8)
    count, status, nodes = np.zeros(len(cand), np.int32), np.zeros(len(cand), np.uint8), np.zeros(len(cand), np.int32)
    found = []
    for n, at in enumerate(cand):
        b, i, j, k = where(at)
        t0 = [float(plan.breaks[a][c]) for a, c in enumerate((i, j, k))]
        t1 = [float(plan.breaks[a][c + 1]) for a, c in enumerate((i, j, k))]
        zeros, close, status[n], nodes[n] = isolate_cell(cell_of(b, i, j, k), t0, t1, [float(s) for s in scale[b]], walk)
        found.append((zeros, close))
        count[n] = len(zeros)
        out[n, :len(zeros)] = np.array(zeros).reshape(-1, 3)
        near[n, :len(zeros)] = close
    keep = np.zeros((len(cand), R), np.uint8)
    for n, row in enumerate(merge_keep(found, flags, cand, plan.breaks)):
        keep[n, :len(row)] = row
    return dict(flags=flags, cand=cand, roots=out, near=near, count=count, status=status, nodes=nodes, keep=keep)


# ------------------------------------------------------------------------------------------ plans and launches
Plan3 = _cells.TensorPlan          # one ``roots.BezierPlan`` per axis; the band steps on the axes 1, 2 and 3 of (M, n0, n1, n2)


def extract_host(data, plan):
    """NumPy (M, n0, n1, n2) float64 -> (M, R0, R1, R2) in Bezier form (``_cells.band_host``)."""
    return _cells.band_host(data, plan.steps, LAST_PATHS)


def _run_host(rows, plan, mask, scale):
    """rows: NumPy float64 (B, 3, R0, R1, R2) in Bezier form; mask: uint8 (B, nc0, nc1, nc2); scale: float64 (B, 3).
    -> dict of flags, cand, roots (ncand, R, 3), near, count, status, nodes, keep (``_cells.isolate_cells``)."""
    rows, scale = np.ascontiguousarray(rows, np.float64), np.ascontiguousarray(scale, np.float64)
    return _cells.isolate_cells(_cells.Host(), "bsk_roots3", rows, plan, mask, scale, slots(*plan.order), LAST_PATHS)


# ------------------------------------------------------------------------------------------ public
def _check_spline(spline):
    if spline.nInd != 3:
        raise NotImplementedError("zeros3: three independent variables only (curves: Spline.zeros, two variables: Spline.zeros2)")
    if min(spline.order) < MIN_K or max(spline.order) > MAX_K:
        raise NotImplementedError(f"zeros3: orders from {MIN_K} to {MAX_K} (one wave holds the 64 coefficients of a cell)")


def tables(spline, coefs=None):
    """The host path's tables of a system: (plan, rows (B, 3, R0, R1, R2), mask (B, nc0, nc1, nc2), scale (B, 3)), all NumPy."""
    plan = Plan3(spline.order, spline.knots)
    data = np.asarray(spline.coefs if coefs is None else coefs)
    data = data.reshape((-1, 3) + data.shape[-3:]).astype(np.float64)            # float32 is widened BEFORE the extraction
    wide = np.abs(data)
    scale = np.ascontiguousarray(wide.max(axis=(2, 3, 4)))
    small = (wide < (scale * EPS)[:, :, None, None, None]) | (scale == 0.0)[:, :, None, None, None]
    mask = zero_cells(small, plan).astype(np.uint8)
    rows = data
    if plan.steps:
        rows = extract_host(data.reshape((-1,) + data.shape[2:]), plan).reshape(data.shape[:2] + tuple(plan.rowlen))
    return plan, rows, mask, scale


def zeros3_batch(spline, coefs=None, _path=None):
    """The isolated common zeros of B systems of three scalar splines in three variables on the spline's knots.
    Returns (values, offsets, cells, status): the zeros of system b are values[offsets[b]:offsets[b + 1]], rows (u, v, w)
    in the knots' dtype sorted by (u, v, w); ``cells`` (NumPy float64, m x 7) holds one row (system, u0, u1, v0, v1, w0, w1)
    per zero cell; ``status`` (uint8, B x nc0 x nc1 x nc2) holds the status bits of every cell (1: zeros not isolated,
    2: more zeros than slots, 4: tangential or singular zero), 0 where all is well.
    ``coefs``: a torch CUDA tensor (B, 3, n0, n1, n2), float32 or float64, contiguous or not, takes the place of the
    spline's coefficients (the spline gives the orders and the knots); values, offsets and status are then CUDA tensors.
    The zero cells are found on the host: the comparison |coefficient| < S_d eps runs on the device, its result (one
    byte per coefficient, 3 B n0 n1 n2 bytes) is read back and the windowed sums over the cells are NumPy's
    (``zero_cells``), as in roots2.  The coefficients themselves, the extracted rows and the zeros stay on the device."""
    del LAST_PATHS[:]
    path = _cells.pick_path(_path, FORCE_PATH)
    _check_spline(spline)
    K = tuple(int(k) for k in spline.order)
    n0, n1, n2 = (len(spline.knots[d]) - spline.order[d] for d in range(3))
    on_device = coefs is not None and _cells.is_torch(coefs)
    if coefs is None:
        if spline.nDep != 3:
            raise ValueError("zeros3_batch takes three dependent variables, or coefs (B, 3, n0, n1, n2)")
        coefs = spline.coefs[None]
    if on_device:
        import torch
        if not coefs.is_cuda or coefs.dtype not in (torch.float32, torch.float64):
            raise TypeError("zeros3_batch takes the coefficients as a float32 or float64 torch CUDA tensor")
        if path == "host":
            raise ValueError("coefficients on the device take the device path")
        path = "device"
    else:
        coefs = np.asarray(coefs)
    if coefs.ndim != 5 or tuple(coefs.shape[1:]) != (3, n0, n1, n2):
        raise ValueError(f"coefs must have the shape (B, 3, {n0}, {n1}, {n2})")
    B = int(coefs.shape[0])
    plan = Plan3(spline.order, spline.knots)
    ncell = int(np.prod(plan.ncells))
    kdtype = np.result_type(*(spline.knots[d].dtype for d in range(3)))
    if path is None:
        path = "device" if B * ncell >= DEVICE_MIN_CELLS else "host"

    if B == 0:
        return _cells.collect(_cells.Device(coefs.device) if on_device else _cells.Host(), plan, kdtype, 0)

    if path == "device":
        import torch
        data = (coefs if on_device else torch.from_numpy(np.ascontiguousarray(coefs)).cuda()).double()   # widened BEFORE the extraction
        be = _cells.Device(data.device)
        wide = data.abs()
        scale = wide.amax(dim=(2, 3, 4)).contiguous()
        small = ((wide < (scale * EPS)[:, :, None, None, None]) | (scale == 0.0)[:, :, None, None, None]).cpu().numpy()
        mask = zero_cells(small, plan).astype(np.uint8)
        rows = data.reshape((3 * B, n0, n1, n2))
        if plan.steps:
            rows, ran = refinement.run_device(rows, plan.steps)
            LAST_PATHS.extend(ran)
        res = _cells.isolate_cells(be, "bsk_roots3", rows.contiguous(), plan, mask, scale, slots(*K), LAST_PATHS)
    else:
        be = _cells.Host()
        _, rows, mask, scale = tables(spline, coefs)
        res = _run_host(rows, plan, mask, scale)             # makes rows and scale contiguous
    return _cells.collect(be, plan, kdtype, B, slots(*K), res, mask, numpy_out=not on_device)


def zeros3(self, _path=None):
    """``Spline.zeros3``: a list, sorted by (u, v, w), of length-3 arrays (u, v, w) in the knots' dtype for isolated zeros and
    of ((u0, v0, w0), (u1, v1, w1)) tuples for cells on which a component vanishes."""
    if not (self.nInd == self.nDep):
        raise ValueError("The number of independent variables (nInd) must match the number of dependent variables (nDep).")
    _check_spline(self)
    values, _, cells, status = zeros3_batch(self, _path=_path)
    if status.any():
        _, i, j, k = (int(x) for x in np.argwhere(status)[0])
        bits = int(status[0, i, j, k])
        u, v, w = Plan3(self.order, self.knots).breaks
        why = ", ".join(text for bit, text in STATUS_TEXT.items() if bits & bit)
        raise ValueError(f"zeros3: {why} in the cell [{float(u[i])}, {float(u[i + 1])}] x [{float(v[j])}, {float(v[j + 1])}] x "
                         f"[{float(w[k])}, {float(w[k + 1])}]")
    kdtype = values.dtype
    found = [(tuple(float(x) for x in r), r) for r in values]
    for _, u0, u1, v0, v1, w0, w1 in cells.astype(kdtype):
        found.append(((float(u0), float(v0), float(w0)), ((u0, v0, w0), (u1, v1, w1))))
    found.sort(key=lambda item: item[0])
    return [item[1] for item in found]
