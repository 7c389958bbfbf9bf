"""
Level curves of a scalar spline in two variables: ``Spline.contours`` for nInd == 2, nDep == 1 and ``trace_batch`` for B
fields on the same knots (the reference's ``contours``, bspy/_spline_intersection.py, is a serial tracer of one curve at a
time from turning points).  Here every knot cell carries a lattice of G x G leaves, G = 2^depth, and the zero set is
marched through the leaves that hold it: the contour is decided on the lattice and on nothing finer.

After Bezier extraction of both variables every knot cell holds one polynomial in tensor-product Bernstein form.
Extraction is the band operator of refinement.py, once per axis (``roots.BezierPlan``); almost all cells fail a sign test
on their K0 K1 coefficients (``contour_flag``); the rest are compacted in index order and each is walked by 4^P lanes
(``contour_march``), once to count its segments and once to write them; the segments are joined into polylines on the host.

    device path   ``bsk_band_apply`` per axis with the rows on the device, ``bsk_contour_flag``, ``torch.nonzero``,
                  ``bsk_contour_march`` (count), ``torch.cumsum``, ``bsk_contour_march`` (emit); no candidates: the march
                  launches are skipped; no segments: the second one is
    host path     ``bsk_roots_extract_host`` per axis, ``bsk_contour_flag_host``, ``bsk_contour_march_host`` twice: the same
                  functions of bsk_contour.hpp on the CPU, for few leaves
    linking       NumPy and a dictionary on the host, on both paths: a sort by integer keys, not a kernel

THE STATEMENT (``node_value``, ``vertex_of``, ``leaf_segments`` and ``flag_cell`` say it in plain Python floats, bit for
bit what bsk_contour.hpp computes; S = max |coefficient| of the field, eps of float64):
  * fields: field b is the spline's coefficients, ``coefs[b]``, or the spline's coefficients minus ``levels[b]``: the
    level is subtracted from every Bezier coefficient as a cell is loaded (a constant has all Bernstein coefficients
    equal), S_b = max |B-spline coefficient - level|;
  * extraction: float64 whatever the coefficient dtype (float32 is widened first); cell (i, j) is the K0 x K1 window at
    first0[i], first1[j] of the extracted rows.  An interior knot of multiplicity >= K is refused (a jump: there is no
    contour across it), so adjacent cells share their end row or column: the same floats;
  * a zero cell is one whose K0 K1 Bezier coefficients are all below S eps in magnitude (the rule of zeros2 on the cell's
    own polynomial): it is reported once as a cell and marched by nobody;
  * depth: ``depth`` if given, else from ``tolerance``: the smallest d in 0 .. 8 with (h 2^-d)^2 <= tolerance L, h the
    widest knot cell and L the larger extent of the domain (the sagitta of a chord of one leaf on a curve whose radius of
    curvature is L / 8), else 4;
  * the lattice: node (I, J) of the whole domain, I = i G + a.  A node is OWNED by the cell with the lowest flat index
    that contains it: io = (I - 1) // G for I > 0 (so a = G there), else 0; its value is de Casteljau of the owner's
    coefficients, every row at b / G, then the results at a / G (``roots.value``: K - 1 levels of s c[i] + t c[i + 1]).
    v >= 0 counts as positive.  Every leaf that touches a node computes the same bits;
  * an edge (I, J, dir) runs from node (I, J) to (I + 1, J) (dir 0) or (I, J + 1) (dir 1) and has the integer key
    ((I NJ + J) << 1) | dir, NJ = nc1 G + 1.  It carries a vertex exactly when the signs of its nodes differ;
  * the vertex of a crossed edge is a function of (field, key): the owner of the lattice line (lowest flat index) is
    restricted to the line by one ``roots.value`` per row (dir 0) or column (dir 1) in the fixed variable; that polynomial
    is restricted to the edge's interval (``roots.restrict(line, a / G, 1 / G)``); s = the sign bisection of
    ``roots_isolate`` on [0, 1] from the sign of node (I, J): at most 60 steps, until the midpoint is an end or the value is
    0.0.  The moving local coordinate is a / G + s / G; a local x of cell i becomes (1 - x) t_i + x t_{i+1}, which is t_i
    and t_{i+1} exactly at the ends, so the fixed coordinate of a vertex is bit-equal to its lattice line;
  * a leaf's perimeter is walked counter-clockwise (bottom, right, top, left).  A crossing from + to - starts a segment,
    one from - to + ends it: f >= 0 lies on the left of every segment.  2 crossings give one segment.  4 crossings give
    two: the canonical value at the leaf's centre (its own cell at ((2a + 1) / 2G, (2b + 1) / 2G)) pairs every start with
    the next end when it is positive, with the previous one otherwise, and status bit 1 is set on the cell;
  * pruning: a box of the walk is dropped when its restricted coefficients are all > tau or all < -tau,
    tau = 32 (K0 + K1) eps S.  Why 32: the restricted coefficients come from the cell's own by two ``roots.restrict`` per
    axis (2 (K - 1) levels of one lerp, 3 eps S each, plus the rounded division, 2 (K - 1) eps S) and at most 8 halvings
    per axis ((K - 1) eps S / 2 each): below 12 (K0 + K1) eps S; a node value is K0 + K1 - 2 lerps: below
    3 (K0 + K1) eps S; the shared floats on a knot line make the neighbour's polynomial there the same one.  A box with
    all coefficients above tau >= 2 x 15 (K0 + K1) eps S is positive by more than either error, so none of its nodes,
    its boundary included, has a negative canonical value, no edge of it is crossed, and its leaves emit nothing.
    Pruning, and so the split level P, changes the cost and never the output.
NOT PROMISED: the contour is decided on the lattice.  A feature smaller than a leaf - a loop inside one leaf, two
crossings of one leaf edge, a component that touches without crossing - is missed without a flag.  A saddle leaf is paired
by one value at its centre.  Contours are not certified; nothing here bounds the distance of the polyline from the zero
set between two vertices, the vertices themselves are zeros of the cell's polynomial on their lattice line to the last
bits.

Segments are joined by their keys: the next segment of (a, b) is the one that starts at b.  An open chain starts where
no segment ends; a loop starts at its smallest key and repeats that vertex at its end.  The components of a field are
ordered by their first key.  ``Spline.contours`` parametrises every polyline by normalised chord length (points that
repeat their predecessor are dropped) and fits it with ``Spline.least_squares``, order 4 (fewer points: their number):
to ``tolerance``, or to 2^-20 L (L the larger extent of the domain) when none is given: knots are added until no vertex is
farther from the curve.  (Interpolating all vertices is not an option: vertices next to a lattice node are 2^-60 of a leaf apart.)

``_path="device" | "host"`` (or ``contours.FORCE_PATH``) pins the path; ``contours.LAST_PATHS`` lists what the last call
ran.
"""
import functools
import sys

import numpy as np

from . import _cells
from . import _native as nv
from . import roots

_THIS = sys.modules[__name__]          # the family that ``_cells`` is handed
NIND, BATCH = 2, "trace_batch"         # the variables of a field and the batch call's name in its messages

# Leaves (fields x cells x 4^depth) from which the device path is taken: read off the table of tools/contours_time.py on an
# MI355X: bicubic, depth 4, 1024 leaves 0.85 ms on the host against 1.2 ms, 4096 leaves 1.36 against 1.26.
DEVICE_MIN_LEAVES = 1 << 12
DEVICE_MIN_K, DEVICE_MAX_K = 2, 4
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

EPS = roots.EPS
DEFAULT_DEPTH, MAX_DEPTH = 4, 8
BISECT = 60
TAU = 32.0
# lanes wanted by a march launch: 256 compute units x 4 waves of 64; the split level P is the smallest that reaches it
FILL_LANES = 1 << 16
STATUS_SADDLE = 1
FIT_TOLERANCE = 2.0 ** -20   # of the domain's larger extent: the fit's tolerance when the caller gives none


# ------------------------------------------------------------------------------------------ the statement
def tau_of(K0, K1, S):
    return TAU * float(K0 + K1) * EPS * S


def one_side(cell, tau):
    flat = [x for row in cell for x in row]
    return all(x > tau for x in flat) or all(x < -tau for x in flat)


def flag_cell(cell, S):
    """What ``contour_flag`` writes for one cell (K0 rows of K1 floats, the level subtracted): (cand, zero)."""
    zero = S == 0.0 or all(abs(x) < S * EPS for row in cell for x in row)
    return int(not zero and not one_side(cell, tau_of(len(cell), len(cell[0]), S))), int(zero)


def value2(cell, x, y):
    return roots.value([roots.value(row, y) for row in cell], x)


def owner_of(I, depth):
    cell = (I - 1) >> depth if I > 0 else 0
    return cell, I - (cell << depth)


def bisect(e, pos):
    a, b = 0.0, 1.0
    for _ in range(BISECT):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        f = roots.value(e, m)
        if f == 0.0:
            a = b = m
            break
        if (f > 0.0) == pos:
            a = m
        else:
            b = m
    return 0.5 * (a + b)


class Lattice:
    """One field in Bezier form with its lattice: ``cell(i, j)`` gives the K0 x K1 floats (level subtracted)."""

    def __init__(self, rows, plan, level, depth):
        self.rows, self.plan, self.level, self.depth = rows, plan, float(level), int(depth)
        self.inv = 1.0 / float(1 << depth)
        self.NJ = (plan.ncells[1] << depth) + 1
        self._values = {}

    def cell(self, i, j):
        K0, K1 = self.plan.order
        f0, f1 = int(self.plan.first[0][i]), int(self.plan.first[1][j])
        return [[float(self.rows[f0 + r, f1 + s]) - self.level for s in range(K1)] for r in range(K0)]

    def node_value(self, I, J):
        """The canonical value of lattice node (I, J)."""
        if (I, J) not in self._values:
            io, a = owner_of(I, self.depth)
            jo, b = owner_of(J, self.depth)
            self._values[I, J] = value2(self.cell(io, jo), float(a) * self.inv, float(b) * self.inv)
        return self._values[I, J]

    def key(self, I, J, direction):
        return ((I * self.NJ + J) << 1) | direction

    def vertex_of(self, I, J, direction, pos):
        """(u, v) of the crossed edge (I, J, direction); pos: the sign of node (I, J)."""
        d, inv = self.depth, self.inv
        if direction == 0:
            i = I >> d
            a = I - (i << d)
            j, b = owner_of(J, d)
        else:
            i, a = owner_of(I, d)
            j = J >> d
            b = J - (j << d)
        c = self.cell(i, j)
        x, y = float(a) * inv, float(b) * inv
        if direction == 0:
            line = [roots.value(row, y) for row in c]
            x = x + bisect(roots.restrict(line, x, inv), pos) * inv
        else:
            line = [roots.value([row[s] for row in c], x) for s in range(len(c[0]))]
            y = y + bisect(roots.restrict(line, y, inv), pos) * inv
        t0, t1 = float(self.plan.breaks[0][i]), float(self.plan.breaks[0][i + 1])
        s0, s1 = float(self.plan.breaks[1][j]), float(self.plan.breaks[1][j + 1])
        return (1.0 - x) * t0 + x * t1, (1.0 - y) * s0 + y * s1

    def leaf_segments(self, i, j, a, b):
        """What leaf (a, b) of cell (i, j) emits: ([(key_a, key_b, ua, va, ub, vb)], status bits)."""
        d = self.depth
        I, J = (i << d) + a, (j << d) + b
        s00, s10 = self.node_value(I, J) >= 0.0, self.node_value(I + 1, J) >= 0.0
        s11, s01 = self.node_value(I + 1, J + 1) >= 0.0, self.node_value(I, J + 1) >= 0.0
        t = [int(s00) - int(s10), int(s10) - int(s11), int(s11) - int(s01), int(s01) - int(s00)]
        ncross = sum(1 for x in t if x)
        if ncross == 0:
            return [], 0
        status, cpos = 0, False
        if ncross == 4:
            half = 0.5 * self.inv
            cpos = value2(self.cell(i, j), float(2 * a + 1) * half, float(2 * b + 1) * half) >= 0.0
            status = STATUS_SADDLE
        edges = [(I, J, 0, s00), (I + 1, J, 1, s10), (I, J + 1, 0, s01), (I, J, 1, s00)]     # bottom, right, top, left
        out = []
        for k in range(4):
            if t[k] <= 0:
                continue
            e = t.index(-1) if ncross == 2 else (k + (1 if cpos else 3)) & 3
            row = []
            for n in (k, e):
                EI, EJ, direction, pos = edges[n]
                row.append((self.key(EI, EJ, direction),) + self.vertex_of(EI, EJ, direction, pos))
            out.append((row[0][0], row[1][0], row[0][1], row[0][2], row[1][1], row[1][2]))
        return out, status


def walk_order(depth):
    """The leaves (a, b) of a cell in the order of the walk at split level 0: axis 0 is halved first."""
    out = []
    for path in range(1 << (2 * depth)):
        a = b = 0
        for k in range(2 * depth):
            bit = (path >> (2 * depth - 1 - k)) & 1
            if k % 2 == 0:
                a = 2 * a + bit
            else:
                b = 2 * b + bit
        out.append((a, b))
    return out


def statement(rows, plan, levels, scale, depth):
    """cand and zero (B, nc0, nc1), keys (n, 2), xy (n, 4), field (n) and status (B, nc0, nc1) of the extracted rows
    (nrows, R0, R1), from the functions above with every leaf of every candidate visited (no pruning), in the order of the
    launches at split level 0: what the host drivers and the kernels return, bit for bit."""
    B = len(scale)
    nc0, nc1 = plan.ncells
    K0, K1 = plan.order
    cand, zero = np.zeros((B, nc0, nc1), np.uint8), np.zeros((B, nc0, nc1), np.uint8)
    status = np.zeros((B, nc0, nc1), np.uint8)
    keys, xy, field = [], [], []
    order = walk_order(depth)
    for b in range(B):
        lat = Lattice(rows[0 if levels is not None else b], plan, 0.0 if levels is None else levels[b], depth)
        for i in range(nc0):
            for j in range(nc1):
                cand[b, i, j], zero[b, i, j] = flag_cell(lat.cell(i, j), float(scale[b]))
                if not cand[b, i, j]:
                    continue
                for a, bb in order:
                    segs, bits = lat.leaf_segments(i, j, a, bb)
                    status[b, i, j] |= bits
                    for s in segs:
                        keys.append(s[:2])
                        xy.append(s[2:])
                        field.append(b)
    return dict(cand=cand, zero=zero, status=status, keys=np.array(keys, np.int64).reshape(-1, 2),
                xy=np.array(xy, np.float64).reshape(-1, 4), field=np.array(field, np.int64))


# depth_of(tolerance, plan): the depth that ``tolerance`` asks for (the statement says why)
depth_of = functools.partial(_cells.depth_of, _THIS)
# split_of(ncand, depth): the split level P of a march launch: the smallest that gives FILL_LANES lanes, at most depth
split_of = functools.partial(_cells.split_of, NIND, FILL_LANES)


# ------------------------------------------------------------------------------------------ linking (host, both paths)
def link(keys, field, B):
    """Join segments (keys (n, 2) int64, field (n)) into polylines.  -> (points, offsets, closed, comp_field): ``points``
    indexes the 2 n segment ends (2 s: the start of segment s, 2 s + 1: its end); component m is
    points[offsets[m]:offsets[m + 1]].  The result does not depend on the order of the segments."""
    keys, field = np.asarray(keys, np.int64).reshape(-1, 2), np.asarray(field, np.int64)
    points, offsets, closed, comp_field = [], [0], [], []
    for b in range(B):
        which = np.flatnonzero(field == b)
        if not len(which):
            continue
        which = which[np.argsort(keys[which, 0], kind="stable")]
        starts = keys[which, 0].tolist()
        if len(set(starts)) != len(starts):
            raise ArithmeticError("contours: two segments start at one lattice edge")
        nxt = {a: (int(e), int(s)) for a, e, s in zip(starts, keys[which, 1].tolist(), which.tolist())}
        ends = set(keys[which, 1].tolist())
        comps = []
        seen = set()
        for a in starts:                                   # ascending: open chains by their start key
            if a in ends:
                continue
            chain, at = [], a
            while at in nxt:
                e, s = nxt[at]
                seen.add(at)
                chain.append(s)
                at = e
            comps.append((a, False, chain))
        for a in starts:                                   # ascending: a loop is met at its smallest key first
            if a in seen:
                continue
            chain, at = [], a
            while at not in seen and at in nxt:
                e, s = nxt[at]
                seen.add(at)
                chain.append(s)
                at = e
            comps.append((a, True, chain))
        comps.sort(key=lambda c: c[0])
        for _, loop, chain in comps:
            points.extend([2 * chain[0]] + [2 * s + 1 for s in chain])
            offsets.append(len(points))
            closed.append(loop)
            comp_field.append(b)
    return (np.array(points, np.int64), np.array(offsets, np.int64), np.array(closed, bool), np.array(comp_field, np.int64))


# ------------------------------------------------------------------------------------------ the launches
def _last():
    return nv.lib().bsk_contour_last_kernel().decode()


def _grid(plan, rows, ptr, levels, B, scale, first0, first1):
    K0, K1 = plan.order
    return (K0, K1, ptr(rows), rows.shape[0], plan.rowlen[0], plan.rowlen[1], plan.ncells[0], plan.ncells[1], ptr(first0), ptr(first1),
            None if levels is None else ptr(levels), B, ptr(scale))


def _run(be, rows, plan, levels, scale, depth, split):
    """rows: float64 (nrows, R0, R1) in Bezier form; levels: float64 (B) or None; scale: float64 (B): the backend's
    contiguous arrays.  -> dict of cand, zero (B, nc0, nc1), keys (n, 2), xy (n, 4), field (n), status (B, nc0, nc1), the
    backend's, and split."""
    B = int(scale.shape[0])
    nc0, nc1 = plan.ncells

    def call(name, *args):
        be.call(name, *args)
        LAST_PATHS.append(_last())

    with be:
        first0, first1 = (be.put(f, np.int32) for f in plan.first)
        grid = _grid(plan, rows, be.ptr, levels, B, scale, first0, first1)
        cand, zero = be.empty((B, nc0, nc1), np.uint8), be.empty((B, nc0, nc1), np.uint8)
        call("bsk_contour_flag", *grid, be.ptr(cand), be.ptr(zero))
        idx = be.nonzero(cand)
        n = len(idx)
        P = split_of(n, depth) if split is None else int(split)
        out = dict(cand=cand, zero=zero, keys=be.empty((0, 2), np.int64), xy=be.empty((0, 4), np.float64), field=be.empty(0, np.int64),
                   status=be.zeros((B, nc0, nc1), np.uint8), split=P)
        if not n:
            return out
        breaks0, breaks1 = (be.put(b, np.float64) for b in plan.breaks)
        lanes = n << (2 * P)
        counts, lane_status = be.empty(lanes, np.int32), be.empty(lanes, np.uint8)
        march = grid + (be.ptr(breaks0), be.ptr(breaks1), be.ptr(idx), n, depth, P)
        call("bsk_contour_march", *march, 0, None, 0, be.ptr(counts), be.ptr(lane_status), None, None)
        out["status"].reshape(-1)[idx] = be.amax(lane_status.reshape(n, -1), 1)
        ends = be.cumsum(counts)
        total = int(ends[-1])
        if not total:
            return out
        offsets = ends - counts                                        # int64, a fresh contiguous array
        keys, xy = be.empty((total, 2), np.int64), be.empty((total, 4), np.float64)
        call("bsk_contour_march", *march, 1, be.ptr(offsets), total, None, None, be.ptr(keys), be.ptr(xy))
        out.update(keys=keys, xy=xy, field=be.repeat(idx // (nc0 * nc1), be.sum(counts.reshape(n, -1), 1)))
    return out


def _run_host(rows, plan, levels, scale, depth, split):
    """``_run`` on NumPy arrays."""
    rows, levels, scale = (None if a is None else np.ascontiguousarray(a, np.float64) for a in (rows, levels, scale))
    return _run(_cells.Host(), rows, plan, levels, scale, depth, split)


# ------------------------------------------------------------------------------------------ public
class Plan(_cells.JumpFreePlan):
    """``_cells.TensorPlan`` that refuses a jump: an interior knot of multiplicity >= K."""
    who, what = "contours", "contour"


def _check_spline(spline):
    if spline.nInd != 2:
        raise NotImplementedError("contours: two independent variables only (scalar fields over a surface's parameters)")
    if min(spline.order) < DEVICE_MIN_K or max(spline.order) > DEVICE_MAX_K:
        raise NotImplementedError(f"contours: orders from {DEVICE_MIN_K} to {DEVICE_MAX_K}")


_check_batch = _check_spline


def _check_keys(plan, depth, B):
    """Nothing to refuse: the edge keys of 2^8 leaves per cell and axis fit 62 bits for any spline that fits memory."""


# tables(spline, levels=None, coefs=None): the host path's tables: (plan, rows (nrows, R0, R1), levels or None, scale (B)),
# all NumPy float64
tables = functools.partial(_cells.level_tables, _THIS)


def trace_batch(spline, levels=None, coefs=None, depth=None, _path=None, _split=None):
    """The zero sets of B scalar fields in two variables on the spline's knots, marched on a lattice of 2^depth x 2^depth
    leaves per knot cell (depth 0 .. 8, default 4).  The fields are the spline itself (nDep 1), the spline minus
    ``levels[b]`` (the topographic-map case: one extraction for all levels), or ``coefs`` (B, n0, n1).
    Returns (vertices, offsets, closed, field, cells, status): polyline m is vertices[offsets[m]:offsets[m + 1]], rows
    (u, v) in the knots' dtype with f >= 0 on its left; closed[m] says that it is a loop (its first vertex is repeated at
    the end); field[m] is its field; the polylines are ordered by field, then by the lattice key of their first vertex.
    ``cells`` (NumPy float64, k x 5) holds one row (field, u0, u1, v0, v1) per zero cell; ``status`` (uint8,
    B x nc0 x nc1) has bit 1 where a leaf of the cell had four crossings (a saddle, paired by its centre value).
    ``coefs``: a float32 / float64 torch CUDA tensor takes the device path; vertices and status are then CUDA tensors and
    the vertices never leave the device (the integer keys of the segments do: linking is a host sort).
    ``_split`` pins the split level P of the march launches (0 .. depth); the result does not depend on it."""
    be, on_device, plan, B, res, cells = _cells.level_batch(_THIS, spline, levels, coefs, depth, _path, _split)
    kdtype = np.result_type(spline.knots[0].dtype, spline.knots[1].dtype)
    if B == 0:
        return (be.empty((0, 2), kdtype), np.zeros(1, np.int64), np.zeros(0, bool), np.zeros(0, np.int64), cells,
                be.zeros((0,) + tuple(plan.ncells), np.uint8))
    points, offsets, closed, comp_field = link(be.get(res["keys"]), be.get(res["field"]), B)
    vertices, status = be.cast(res["xy"].reshape(-1, 2)[be.put(points, np.int64)], kdtype), res["status"]
    if not on_device:
        vertices, status = be.get(vertices), be.get(status)
    return vertices, offsets, closed, comp_field, cells, status


def fit_chords(points, step, groups, tolerance=None, closed=False):
    """The points (n, m) of one polyline and the lengths ``step`` (n - 1) of its chords -> one Spline curve (nInd 1, on
    [0, 1], order 4) per group of columns (``groups``: slices), all fitted to the same normalised chord-length parameters.
    Points behind a chord of length 0 are dropped; ``closed``: the last coefficient is set to the first one, so that the
    end points of the curve are equal to the bit."""
    from .spline import Spline
    keep = np.concatenate(([True], step > 0.0))
    points = points[keep]
    if len(points) < 2:
        points = np.repeat(points[:1], 2, axis=0)
        t = np.array([0.0, 1.0])
    else:
        t = np.concatenate(([0.0], np.cumsum(step[step > 0.0])))
        t /= t[-1]
        t[-1] = 1.0
        if np.any(np.diff(t) <= 0.0):                      # chords below the resolution of [0, 1]: index them instead
            t = np.linspace(0.0, 1.0, len(points))
    order = min(4, len(points))
    curves = []
    for cols in groups:
        curve = Spline.least_squares(t, points[:, cols].T.copy(), order=[order], tolerance=tolerance)
        if closed:
            coefs = np.array(curve.coefs)
            coefs[:, -1] = coefs[:, 0]
            curve = Spline(1, curve.nDep, curve.order, curve.nCoef, curve.knots, coefs)
        curves.append(curve)
    return curves


def fit_polyline(points, tolerance=None, closed=False):
    """One polyline (n, 2) -> a Spline curve (nInd 1, nDep 2) on [0, 1]: normalised chord length, order 4 (``fit_chords``)."""
    points = np.asarray(points, np.float64)
    step = np.hypot(*np.diff(points, axis=0).T) if len(points) > 1 else np.zeros(0)
    return fit_chords(points, step, [slice(None)], tolerance, closed)[0]


def contours(self, tolerance=None, depth=None, _path=None):
    """``Spline.contours``: the curves of {f = 0} (nInd 1, nDep 2, on [0, 1], order 4), one per connected piece of the
    marched zero set, and ((u0, v0), (u1, v1)) for every knot cell on which f vanishes; sorted by their first vertex."""
    if self.nInd - self.nDep != 1:
        raise ValueError("The number of free variables (self.nInd - self.nDep) must be one.")
    _check_spline(self)
    plan = Plan(self.order, self.knots)
    if depth is None:
        depth = depth_of(tolerance, plan)
    if tolerance is None:
        tolerance = FIT_TOLERANCE * max(float(b[-1]) - float(b[0]) for b in plan.breaks)
    vertices, offsets, closed, _, cells, _ = trace_batch(self, depth=depth, _path=_path)
    if _cells.is_torch(vertices):
        vertices = vertices.cpu().numpy()
    found = []
    for m in range(len(offsets) - 1):
        points = vertices[offsets[m]:offsets[m + 1]]
        curve = fit_polyline(points, tolerance, bool(closed[m]))
        found.append(((float(points[0, 0]), float(points[0, 1])), curve))
    kdtype = vertices.dtype
    for _, u0, u1, v0, v1 in cells.astype(kdtype):
        found.append(((float(u0), float(v0)), ((u0, v0), (u1, v1))))
    found.sort(key=lambda item: item[0])
    return [item[1] for item in found]
