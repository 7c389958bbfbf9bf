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
import functools
import sys

from . import _box
from . import _cells
from . import roots
from ._cells import zero_cells

_THIS = sys.modules[__name__]          # the family that ``_box`` and ``_cells`` are handed

# Systems x cells from which the device path is taken.  Measured with tools/roots3_time.py on an MI355X:
# on candidate-dense systems the device wins from 8 cells on and by a factor 2 at 64; on sparse ones the host wins up to
# about 7000 cells, by at most the 6 ms a device call costs whatever its size.
DEVICE_MIN_CELLS = 64
MIN_K, MAX_K = 2, 4
DEVICE_MIN_K, DEVICE_MAX_K = MIN_K, MAX_K          # the kernels take every order the family does
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
# ``_box`` has the box and its walk for any number of axes; what is particular to three variables is the leaf.  A cell is
# (dims, [component 0, 1, 2]); a component is the flat list of its K0 K1 K2 floats, the last index fastest.
excluded, halve, restrict_box = _box.excluded, _box.halve, _box.restrict_box
eval1, flag_cell, _outside = _box.eval1, _box.flag_cell, _box._outside


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


# (zeros [(u, v, w)], near bytes, status, nodes visited) of one candidate cell on [t0, t1] with the scales S, the keep bytes
# of the candidates' (zeros, near) pairs, and all that the host drivers and the kernels return for extracted rows, bit for bit
isolate_cell = functools.partial(_box.isolate_cell, _THIS)          # (cell, t0, t1, S, walk=None): what ``roots3_isolate`` returns
merge_keep = functools.partial(_box.merge_keep, same=SAME)          # (found, flags, cand, breaks): what ``roots3_merge`` writes
statement = functools.partial(_box.statement, _THIS)                # (rows, plan, mask, scale, walk=None) -> dict


# ------------------------------------------------------------------------------------------ plans and launches
Plan3 = _cells.TensorPlan          # one ``roots.BezierPlan`` per axis; the band steps on the axes 1, 2 and 3 of (M, n0, n1, n2)
NIND, WORD, PREFIX = 3, "three", "bsk_roots3"


# rows: NumPy float64 (B, 3, R0, R1, R2) in Bezier form; mask: uint8 (B, *ncells); scale: float64 (B, 3).  -> dict of flags, cand,
# roots (ncand, R, 3), near, count, status, nodes, keep (``_cells.isolate_cells``)
_run_host = functools.partial(_cells.run_host, _THIS)
# (spline, coefs=None) -> the host path's tables of a system: (plan, rows, mask (B, *ncells), scale (B, 3)), all NumPy
tables = functools.partial(_cells.tables, _THIS)


# ------------------------------------------------------------------------------------------ public
def _check_spline(spline):
    if spline.nInd != 3:
        raise NotImplementedError("zeros3: three independent variables only (curves: Spline.zeros, two variables: Spline.zeros2)")
    if min(spline.order) < MIN_K or max(spline.order) > MAX_K:
        raise NotImplementedError(f"zeros3: orders from {MIN_K} to {MAX_K} (one wave holds the 64 coefficients of a cell)")


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
    return _cells.zeros_batch(_THIS, spline, coefs, _path)


def zeros3(self, _path=None):
    """``Spline.zeros3``: a list, sorted by (u, v, w), of length-3 arrays (u, v, w) in the knots' dtype for isolated zeros and
    of ((u0, v0, w0), (u1, v1, w1)) tuples for cells on which a component vanishes."""
    return _cells.zeros(_THIS, self, _path)
