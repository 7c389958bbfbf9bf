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
import functools
import sys

from . import _box
from . import _cells
from . import roots
from ._cells import zero_cells

_THIS = sys.modules[__name__]          # the family that ``_box`` and ``_cells`` are handed

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
# ``_box`` has the box and its walk for any number of axes; what is particular to two variables is the leaf.  A cell is
# ((K0, K1), [component 0, component 1]), a component the flat list of its K0 K1 floats, the last index fastest.
excluded, halve, restrict_box = _box.excluded, _box.halve, _box.restrict_box
eval1, flag_cell, _outside = _box.eval1, _box.flag_cell, _box._outside


def eval2(dims, comp, x0, x1):
    """One component at (x0, x1): value, d/dx0, d/dx1."""
    K0, K1 = dims
    pq = [eval1(comp[i * K1:(i + 1) * K1], x1) for i in range(K0)]
    f, f0 = eval1([p for p, _ in pq], x0)
    return f, f0, roots.value([q for _, q in pq], x0)


def _leaf(cell, lo, t0, h, S, out, near, R):
    """-> status bits.  Appends at most one zero to ``out`` (and its byte to ``near``)."""
    dims, comps = cell
    w = LEAF_W
    x = [lo[a] + 0.5 * w for a in range(2)]
    prev = last = float("inf")
    fc = [0.0, 0.0]
    conv = ended = False
    for step in range(NEWTON):
        f, fu, fv = eval2(dims, comps[0], *x)
        g, gu, gv = eval2(dims, comps[1], *x)
        if step == 0:
            fc = [f, g]
        det = fu * gv - fv * gu
        if det == 0.0:
            ended = True
            break
        d = [(f * gv - fv * g) / det, (fu * g - f * gu) / det]
        n = [x[a] - d[a] for a in range(2)]
        if not max(_outside(n[a], lo[a], w) for a in range(2)) <= 2.0 * w:
            ended = True
            break
        x = n
        last = max(abs(d[0]), abs(d[1]))
        if not last < prev:
            conv = ended = True
            break
        prev = last
    if not ended and last <= SMALL_STEP:
        conv = True
    if not conv:
        tol = 4.0 * sum(dims) * EPS
        return STATUS_TANGENT if all(abs(fc[d]) <= tol * S[d] for d in range(2)) else 0
    if not all(-GROW <= x[a] <= 1.0 + GROW for a in range(2)):
        return 0
    x = [min(max(x[a], 0.0), 1.0) for a in range(2)]
    u = tuple(t0[a] + x[a] * h[a] for a in range(2))
    tol = [SAME * h[a] for a in range(2)]
    if any(all(abs(z[a] - u[a]) <= tol[a] for a in range(2)) for z in out):
        return 0
    if len(out) >= R:
        return STATUS_SLOTS
    out.append(u)
    near.append(int(any(x[a] <= SAME or x[a] >= 1.0 - SAME for a in range(2))))
    return 0


# (zeros [(u, v)], near bytes, status, nodes visited) of one candidate cell on [t0, t1] with the scales S, the keep bytes
# of the candidates' (zeros, near) pairs, and all that the host drivers and the kernels return for extracted rows, bit for bit
isolate_cell = functools.partial(_box.isolate_cell, _THIS)          # (cell, t0, t1, S, walk=None): what ``roots2_isolate`` returns
merge_keep = functools.partial(_box.merge_keep, same=SAME)          # (found, flags, cand, breaks): what ``roots2_merge`` writes
statement = functools.partial(_box.statement, _THIS)                # (rows, plan, mask, scale, walk=None) -> dict


# ------------------------------------------------------------------------------------------ plans and launches
Plan2 = _cells.TensorPlan          # one ``roots.BezierPlan`` per axis; the band steps on the axes 1 and 2 of (M, n0, n1)
NIND, WORD, PREFIX = 2, "two", "bsk_roots2"


# rows: NumPy float64 (B, 2, R0, R1) in Bezier form; mask: uint8 (B, *ncells); scale: float64 (B, 2).  -> dict of flags, cand,
# roots (ncand, R, 2), near, count, status, nodes, keep (``_cells.isolate_cells``)
_run_host = functools.partial(_cells.run_host, _THIS)
# (spline, coefs=None) -> the host path's tables of a system: (plan, rows, mask (B, *ncells), scale (B, 2)), all NumPy
tables = functools.partial(_cells.tables, _THIS)


# ------------------------------------------------------------------------------------------ public
def _check_spline(spline):
    if spline.nInd != 2:
        raise NotImplementedError("zeros2: two independent variables only (curves: Spline.zeros)")
    if min(spline.order) < 2 or max(spline.order) > HOST_MAX_K:
        raise NotImplementedError(f"zeros2: orders from 2 to {HOST_MAX_K}; the kernels take orders up to {DEVICE_MAX_K}")


def zeros2_batch(spline, coefs=None, _path=None):
    """The isolated common zeros of B systems of two scalar splines in two variables on the spline's knots.
    Returns (values, offsets, cells, status): the zeros of system b are values[offsets[b]:offsets[b + 1]], rows (u, v) in
    the knots' dtype sorted by (u, v); ``cells`` (NumPy float64, m x 5) holds one row (system, u0, u1, v0, v1) per zero cell;
    ``status`` (uint8, B x nc0 x nc1) holds the status bits of every cell (1: zeros not isolated, 2: more zeros than slots,
    4: tangential or singular zero), 0 where all is well.
    ``coefs``: a torch CUDA tensor (B, 2, n0, n1), float32 or float64, takes the place of the spline's coefficients (the
    spline gives the orders and the knots); values, offsets and status are then CUDA tensors.  The table of zero cells (one
    byte per system and cell) is formed on the device and read back; nothing else leaves the device."""
    return _cells.zeros_batch(_THIS, spline, coefs, _path)


def zeros2(self, _path=None):
    """``Spline.zeros2``: a list, sorted by (u, v), of length-2 arrays (u, v) in the knots' dtype for isolated zeros and of
    ((u0, v0), (u1, v1)) tuples for cells on which a component vanishes."""
    return _cells.zeros(_THIS, self, _path)
