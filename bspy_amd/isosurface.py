"""
Level surfaces of a scalar spline in three variables: ``Spline.isosurface`` for nInd == 3, nDep == 1 and ``extract_batch``
for B fields on the same knots (the reference has nothing for it: its ``contours`` needs nInd - nDep == 1).  Every knot
cell carries a lattice of G x G x G leaves, G = 2^depth, every leaf cube is cut into six tetrahedra, and the zero set is a
triangle mesh whose vertices lie on the lattice edges that it crosses: the surface is decided on the lattice and on
nothing finer.  The work is proportional to the surface, not to the volume: a Bernstein sign test drops every box of the
lattice that the surface cannot reach.

After Bezier extraction of the three variables every knot cell holds one polynomial in tensor-product Bernstein form.
Extraction is the band operator of refinement.py, once per axis; almost all cells fail a sign test on their K0 K1 K2
coefficients (``iso_flag``); the rest are compacted in index order and each is walked by 8^P waves (``iso_walk``), one lane
per coefficient, once to count the leaves that survive and once to write them; the leaves are sorted, and each is cut by
one lane (``iso_leaf``), once to count its triangles and once to write them as triples of integer edge keys; the sorted
unique keys of a field are its vertices, and one lane per vertex (``iso_vertex``) finds the point on its edge.

    device path   ``bsk_band_apply`` per axis with the rows on the device, ``bsk_iso_flag``, ``torch.nonzero``,
                  ``bsk_iso_walk`` (count), ``torch.cumsum``, ``bsk_iso_walk`` (emit), ``torch.sort``, ``bsk_iso_leaf``
                  (count), ``torch.cumsum``, ``bsk_iso_leaf`` (emit), ``torch.unique`` per field, ``bsk_iso_vertex``;
                  no candidates: everything behind the flag is skipped; no leaves: everything behind the first walk; no
                  triangles: the second ``iso_leaf`` and ``iso_vertex``
    host path     ``bsk_roots_extract_host`` per axis and the ``bsk_iso_*_host`` twins: the same functions of bsk_iso.hpp
                  on the CPU, NumPy in place of torch, for few leaves

THE STATEMENT (``Lattice`` says it in plain Python floats, bit for bit what bsk_iso.hpp computes; S = max |coefficient|
of the field, eps of float64):
  * fields: field b is ``coefs[b]``, or the spline's coefficients minus ``levels[b]``: the level is subtracted from every
    Bezier coefficient as a cell is loaded, S_b = max |B-spline coefficient - level|;
  * extraction: float64 whatever the coefficient dtype (float32 is widened first); cell (i, j, k) is the K0 x K1 x K2
    window at first0[i], first1[j], first2[k] of the extracted rows.  An interior knot of multiplicity >= K is refused (a
    jump), so adjacent cells share their end plane: the same floats;
  * a zero cell is one whose Bezier coefficients are all below S eps in magnitude: it is reported once as a cell, has
    status bit 1 and is marched by nobody;
  * depth: ``depth`` if given, else from ``tolerance``: the smallest d in 0 .. 6 with (h 2^-d)^2 <= tolerance L, h the
    widest knot cell and L the largest extent of the domain (the sagitta rule of ``contours``), else 3;
  * the lattice: node (I, J, K) of the whole domain, I = i G + a.  Per axis a node is OWNED by the cell with the lowest
    index that contains it: io = (I - 1) // G for I > 0 (so a = G there), else 0; its value is de Casteljau of the owner's
    coefficients (``roots.value``: K - 1 levels of s c[i] + t c[i + 1]) along axis 2 at a2 / G, then along axis 1, then
    along axis 0 (``eval3``).  v >= 0 counts as positive.  A value that is exactly 0.0 sets status bit 2 on the cell of
    every marched leaf that touches the node;
  * tetrahedra: a leaf cube is cut along its diagonal (0,0,0) - (1,1,1) into one tetrahedron per permutation (a, b, c) of
    the axes, numbered 0 .. 5 in lexicographic order, with the corners v0 = (0,0,0), v1 = v0 + e_a, v2 = v1 + e_b and
    v3 = (1,1,1).  The cut is the same in every cube, so two cubes, and two cells, agree on the diagonal of the face
    between them; there is no case table and no ambiguous case;
  * an edge leaves node (I, J, K) in a direction d = 4 d0 + 2 d1 + d2 with d0, d1, d2 in {0, 1}, not all 0: the six edges of
    a tetrahedron run from its corner m to its corner n > m.  The key of the edge is (((I NJ + J) NK + K) << 3) | d,
    NJ = nc1 G + 1, NK = nc2 G + 1.  It carries a vertex exactly when the signs of its two nodes differ;
  * the vertex is a function of (field, key): the owner of the edge is, per axis, the cell I // G where the edge moves
    (d_x = 1) and the owner of I where it does not.  Its coefficients are reduced in the fixed axes first, 2, then 1, then 0
    (de Casteljau at a / G); f(s) is ``eval3`` of what is left at x = a / G + s / G (the product s / G is exact) in the
    moving axes; s is the sign bisection of ``roots_isolate`` on [0, 1] from the sign of the canonical value of node
    (I, J, K): at most 60 steps, until the midpoint is an end or f is 0.0, and the middle of what is left.  A local x
    of cell i becomes (1 - x) t_i + x t_{i+1}, which is t_i and t_{i+1} exactly at the ends: the fixed coordinates of a
    vertex on an axis edge are bit-equal to their lattice planes;
  * triangles of a tetrahedron, m = 0 .. 3 its corners and mn the vertex on the edge between m and n: one corner p on
    its own side, the others q < r < s: the triangle (pq, pr, ps); two negative corners p < q and two positive ones r < s:
    the quad (pr, ps, qs, qr), cut along pr - qs into (pr, ps, qs) and (pr, qs, qr).  With sigma = the sign of (a, b, c)
    times the sign of the permutation (p, q, r, s) of (0, 1, 2, 3), the triangle is taken as written when sigma > 0 and
    the corners q, r, s are positive, or sigma < 0 and p is; the quad when sigma > 0; otherwise it is reversed (the last two
    vertices of the triangle exchanged; the quad (pr, qr, qs, ps)): the right-hand normal in (u, v, w) points into f >= 0;
  * order: a field's vertices by ascending key; triangles by ascending (leaf flat index ((b NL0 + I) NL1 + J) NL2 + K,
    NL = nc G, tetrahedron, triangle);
  * pruning: a box of the walk is dropped when its restricted coefficients are all > tau or all < -tau,
    tau = 32 (K0 + K1 + K2) eps S.  Why 32, the count of ``contours`` with a third axis: the restricted coefficients
    come from the cell's own by two de Casteljau passes per axis (2 (K - 1) levels of one lerp, 3 eps S each, plus the
    rounded division, 2 (K - 1) eps S) and at most 6 halvings per axis ((K - 1) eps S / 2 each): below
    11 (K0 + K1 + K2) eps S; a node value is K0 + K1 + K2 - 3 lerps: below 3 (K0 + K1 + K2) eps S; the shared floats
    on a knot plane make the neighbour's polynomial there the same one.  A box with all coefficients above
    tau >= 2 x 14 (K0 + K1 + K2) eps S is positive by more than either error, so none of its nodes, its boundary
    included, has a negative or zero canonical value, no edge of it is crossed, and its leaves emit nothing.  Pruning,
    and so the split level P, changes the cost and never the output.
NOT PROMISED: the surface is decided on the lattice.  A feature smaller than a leaf - a bubble inside one leaf, two
crossings of one edge, a sheet that touches without crossing - is missed without a flag.  Nothing bounds the distance of
the mesh from the zero set between two vertices, and nothing is certified; the vertices themselves are zeros of the
cell's polynomial on their lattice edge to the last bits.  Triangles of zero area are not removed: vertices next to a
lattice node are 2^-60 of a leaf apart.

``_path="device" | "host"`` (or ``isosurface.FORCE_PATH``) pins the path; ``isosurface.LAST_PATHS`` lists what the last
call ran.
"""
import functools
import itertools
import sys

import numpy as np

from . import _cells
from . import _native as nv
from . import roots

_THIS = sys.modules[__name__]          # the family that ``_cells`` is handed
NIND, BATCH = 3, "extract_batch"       # the variables of a field and the batch call's name in its messages

# Leaves (fields x cells x 8^depth) from which the device path is taken: read off the calls table of tools/iso_time.py on an
# MI355X: tricubic, depth 3, 4096 leaves 0.99 ms on the host against 1.09 ms, 32 768 leaves 17.4 against 2.0.
DEVICE_MIN_LEAVES = 1 << 12
DEVICE_MIN_K, DEVICE_MAX_K = 2, 4
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

EPS = roots.EPS
DEFAULT_DEPTH, MAX_DEPTH = 3, 6
BISECT = 60
TAU = 32.0
# waves wanted by a walk launch: 256 compute units x 4 SIMDs x the 8 waves a SIMD holds of iso_walk (the occupancy the build
# reports for all 27 count kernels and 26 of the emit ones, 7 for (4, 4, 4) emit); the split level P is the smallest that reaches it
FILL_WAVES = 256 * 4 * 8
STATUS_ZERO_CELL, STATUS_ZERO_NODE = 1, 2
TETRAHEDRA = tuple(itertools.permutations(range(3)))


# ------------------------------------------------------------------------------------------ the statement
def tau_of(K0, K1, K2, S):
    return TAU * float(K0 + K1 + K2) * EPS * S


def flatten(cell):
    return [x for plane in cell for row in plane for x in row]


def one_side(cell, tau):
    flat = flatten(cell)
    return all(x > tau for x in flat) or all(x < -tau for x in flat)


def flag_cell(cell, S):
    """What ``iso_flag`` writes for one cell (K0 x K1 x K2 floats, the level subtracted): (cand, zero)."""
    zero = S == 0.0 or all(abs(x) < S * EPS for x in flatten(cell))
    return int(not zero and not one_side(cell, tau_of(len(cell), len(cell[0]), len(cell[0][0]), S))), int(zero)


def reduce(cell, axis, x):
    """de Casteljau at x along ``axis`` of a nested list [N0][N1][N2]: the same with one entry on that axis."""
    N = (len(cell), len(cell[0]), len(cell[0][0]))
    if axis == 0:
        return [[[roots.value([cell[e][s][t] for e in range(N[0])], x) for t in range(N[2])] for s in range(N[1])]]
    if axis == 1:
        return [[[roots.value([cell[r][e][t] for e in range(N[1])], x) for t in range(N[2])]] for r in range(N[0])]
    return [[[roots.value(cell[r][s], x)] for s in range(N[1])] for r in range(N[0])]


def eval3(cell, x0, x1, x2):
    return reduce(reduce(reduce(cell, 2, x2), 1, x1), 0, x0)[0][0][0]


def owner_of(I, depth):
    cell = (I - 1) >> depth if I > 0 else 0
    return cell, I - (cell << depth)


def bisect(f, pos):
    a, b = 0.0, 1.0
    for _ in range(BISECT):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        v = f(m)
        if v == 0.0:
            a = b = m
            break
        if (v > 0.0) == pos:
            a = m
        else:
            b = m
    return 0.5 * (a + b)


def _sign(perm):
    return -1 if sum(1 for i in range(len(perm)) for j in range(i) if perm[j] > perm[i]) & 1 else 1


def tetrahedron_triangles(perm, positive):
    """The triangles of one tetrahedron as pairs of corner numbers: ``perm`` = (a, b, c), ``positive`` = the signs of the
    corners v0 .. v3.  -> [((m, n), (m, n), (m, n))]."""
    pos = [m for m in range(4) if positive[m]]
    neg = [m for m in range(4) if not positive[m]]
    if not pos or not neg:
        return []

    def edge(m, n):
        return (min(m, n), max(m, n))

    if len(pos) == 2:
        (p, q), (r, s) = neg, pos
        quad = [edge(p, r), edge(p, s), edge(q, s), edge(q, r)]
        if _sign(perm) * _sign((p, q, r, s)) < 0:
            quad = [quad[0], quad[3], quad[2], quad[1]]
        return [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    p = (pos if len(pos) == 1 else neg)[0]
    q, r, s = (m for m in range(4) if m != p)
    sigma = _sign(perm) * _sign((p, q, r, s))
    as_written = sigma > 0 if len(neg) == 1 else sigma < 0
    return [(edge(p, q), edge(p, r), edge(p, s)) if as_written else (edge(p, q), edge(p, s), edge(p, r))]


class Lattice:
    """One field in Bezier form with its lattice: ``cell(i, j, k)`` gives the K0 x K1 x K2 floats (level subtracted)."""

    def __init__(self, rows, plan, level, depth):
        self.rows, self.plan, self.level, self.depth = rows, plan, float(level), int(depth)
        self.inv = 1.0 / float(1 << depth)
        self.NJ = (plan.ncells[1] << depth) + 1
        self.NK = (plan.ncells[2] << depth) + 1
        self._values = {}
        self._cells = {}

    def cell(self, i, j, k):
        if (i, j, k) not in self._cells:
            K0, K1, K2 = self.plan.order
            f0, f1, f2 = int(self.plan.first[0][i]), int(self.plan.first[1][j]), int(self.plan.first[2][k])
            self._cells[i, j, k] = [[[float(self.rows[f0 + r, f1 + s, f2 + t]) - self.level for t in range(K2)] for s in range(K1)]
                                    for r in range(K0)]
        return self._cells[i, j, k]

    def node_value(self, I, J, K):
        """The canonical value of lattice node (I, J, K)."""
        if (I, J, K) not in self._values:
            (i, a0), (j, a1), (k, a2) = (owner_of(X, self.depth) for X in (I, J, K))
            self._values[I, J, K] = eval3(self.cell(i, j, k), float(a0) * self.inv, float(a1) * self.inv, float(a2) * self.inv)
        return self._values[I, J, K]

    def key(self, I, J, K, d):
        return (((I * self.NJ + J) * self.NK + K) << 3) | d

    def unkey(self, key):
        node = key >> 3
        return node // (self.NJ * self.NK), (node // self.NK) % self.NJ, node % self.NK, key & 7

    def edge_cell(self, I, J, K, d):
        """The owner of the edge: per axis (cell, local index)."""
        out = []
        for axis, X in enumerate((I, J, K)):
            if (d >> (2 - axis)) & 1:
                c = X >> self.depth
                out.append((c, X - (c << self.depth)))
            else:
                out.append(owner_of(X, self.depth))
        return out

    def vertex_of(self, key):
        """(u, v, w) of the crossed edge ``key``."""
        I, J, K, d = self.unkey(key)
        inv = self.inv
        pos = self.node_value(I, J, K) >= 0.0
        where = self.edge_cell(I, J, K, d)
        moving = [bool((d >> (2 - axis)) & 1) for axis in range(3)]
        x = [float(a) * inv for _, a in where]
        left = self.cell(*(c for c, _ in where))
        for axis in (2, 1, 0):
            if not moving[axis]:
                left = reduce(left, axis, x[axis])

        def f(m):
            t = m * inv
            return eval3(left, *(x[axis] + t if moving[axis] else x[axis] for axis in range(3)))

        t = bisect(f, pos) * inv
        out = []
        for axis in range(3):
            y = x[axis] + t if moving[axis] else x[axis]
            c = where[axis][0]
            t0, t1 = float(self.plan.breaks[axis][c]), float(self.plan.breaks[axis][c + 1])
            out.append((1.0 - y) * t0 + y * t1)
        return tuple(out)

    def leaf_triangles(self, I, J, K):
        """What the leaf at node (I, J, K) emits: ([(key, key, key)], a node value was 0.0)."""
        corner = lambda v: (I + v[0], J + v[1], K + v[2])
        values = {v: self.node_value(*corner(v)) for v in itertools.product((0, 1), repeat=3)}
        zero = any(x == 0.0 for x in values.values())
        out = []
        for perm in TETRAHEDRA:
            corners = [(0, 0, 0)]
            for axis in perm:
                corners.append(tuple(c + (1 if n == axis else 0) for n, c in enumerate(corners[-1])))
            positive = [values[v] >= 0.0 for v in corners]
            for triangle in tetrahedron_triangles(perm, positive):
                keys = []
                for m, n in triangle:
                    d = sum((corners[n][axis] - corners[m][axis]) << (2 - axis) for axis in range(3))
                    keys.append(self.key(*corner(corners[m]), d))
                out.append(tuple(keys))
        return out, zero


def statement(rows, plan, levels, scale, depth):
    """The raw result of the extracted rows (nrows, R0, R1, R2) from the functions above with every leaf of every
    candidate visited (no pruning): dict of cand, zero, status (B, nc0, nc1, nc2), keys (n), xyz (n, 3), vertex_offsets,
    triangles (m, 3), triangle_offsets: what the host drivers and the kernels return, bit for bit."""
    B = len(scale)
    nc = tuple(plan.ncells)
    cand, zero, status = (np.zeros((B,) + nc, np.uint8) for _ in range(3))
    keys, xyz, voff, tris, toff = [], [], [0], [], [0]
    G = 1 << depth
    for b in range(B):
        lat = Lattice(rows[0 if levels is not None else b], plan, 0.0 if levels is None else levels[b], depth)
        found = []
        for at in itertools.product(*(range(n) for n in nc)):
            cand[(b,) + at], zero[(b,) + at] = flag_cell(lat.cell(*at), float(scale[b]))
            status[(b,) + at] = STATUS_ZERO_CELL * zero[(b,) + at]
        for I, J, K in itertools.product(*(range(n * G) for n in nc)):
            at = (b, I >> depth, J >> depth, K >> depth)
            if not cand[at]:
                continue
            triangles, hit = lat.leaf_triangles(I, J, K)
            if hit:
                status[at] |= STATUS_ZERO_NODE
            found.extend(triangles)
        unique = sorted({key for triangle in found for key in triangle})
        index = {key: len(keys) + n for n, key in enumerate(unique)}
        keys.extend(unique)
        xyz.extend(lat.vertex_of(key) for key in unique)
        tris.extend(tuple(index[key] for key in triangle) for triangle in found)
        voff.append(len(keys))
        toff.append(len(tris))
    return dict(cand=cand, zero=zero, status=status, keys=np.array(keys, np.int64), xyz=np.array(xyz, np.float64).reshape(-1, 3),
                vertex_offsets=np.array(voff, np.int64), triangles=np.array(tris, np.int64).reshape(-1, 3),
                triangle_offsets=np.array(toff, np.int64))


# depth_of(tolerance, plan): the depth that ``tolerance`` asks for (the statement says why)
depth_of = functools.partial(_cells.depth_of, _THIS)
# split_of(ncand, depth): the split level P of a walk launch: the smallest that gives FILL_WAVES waves, at most depth
split_of = functools.partial(_cells.split_of, NIND, FILL_WAVES)


# ------------------------------------------------------------------------------------------ the launches
def _last():
    return nv.lib().bsk_iso_last_kernel().decode()


def _run(be, rows, plan, levels, scale, depth, split):
    """rows: float64 (nrows, R0, R1, R2) in Bezier form; levels: float64 (B) or None; scale: float64 (B): the backend's
    contiguous arrays.  -> dict of cand, zero, status (B, nc0, nc1, nc2), keys (n), xyz (n, 3), vertex_offsets (B + 1),
    triangles (m, 3), triangle_offsets (B + 1), the backend's, split and nleaves (the leaves that the walk kept)."""
    B = int(scale.shape[0])
    nc = tuple(plan.ncells)
    ncell = int(np.prod(nc))
    per_field = ncell << (3 * depth)

    def call(name, *args):
        be.call(name, *args)
        LAST_PATHS.append(_last())

    with be:
        first = [be.put(f, np.int32) for f in plan.first]
        grid = tuple(plan.order) + (be.ptr(rows), rows.shape[0]) + tuple(plan.rowlen) + nc + tuple(be.ptr(f) for f in first) + \
            (None if levels is None else be.ptr(levels), B, be.ptr(scale))
        cand, zero = be.empty((B,) + nc, np.uint8), be.empty((B,) + nc, np.uint8)
        call("bsk_iso_flag", *grid, be.ptr(cand), be.ptr(zero))
        idx = be.nonzero(cand)
        n = len(idx)
        P = split_of(n, depth) if split is None else int(split)
        status = be.zeros(B * ncell, np.uint8)
        out = dict(cand=cand, zero=zero, keys=be.empty(0, np.int64), xyz=be.empty((0, 3), np.float64),
                   vertex_offsets=be.zeros(B + 1, np.int64), triangles=be.empty((0, 3), np.int64),
                   triangle_offsets=be.zeros(B + 1, np.int64), split=P, nleaves=0)

        def finish():
            out["status"] = (status + zero.reshape(-1)).reshape((B,) + nc)        # a zero cell is marched by nobody: bits 1 and 2 never meet
            return out

        if not n:
            return finish()
        waves = n << (3 * P)
        counts = be.empty(waves, np.int32)
        walk = grid + (be.ptr(idx), n, depth, P)
        call("bsk_iso_walk", *walk, 0, None, 0, be.ptr(counts), None)
        ends = be.cumsum(counts)
        nleaves = int(ends[-1])
        if not nleaves:
            return finish()
        out["nleaves"] = nleaves
        offsets = ends - counts                                        # int64, a fresh contiguous array
        leaves = be.empty(nleaves, np.int64)
        call("bsk_iso_walk", *walk, 1, be.ptr(offsets), nleaves, None, be.ptr(leaves))
        leaves = be.sort(leaves)
        tcounts = be.empty(nleaves, np.int32)
        leaf = grid + (be.ptr(leaves), nleaves, depth)
        call("bsk_iso_leaf", *leaf, 0, None, 0, be.ptr(tcounts), be.ptr(status), None)
        tends = be.cumsum(tcounts)
        total = int(tends[-1])
        if not total:
            return finish()
        toffsets = tends - tcounts
        tris = be.empty((total, 3), np.int64)
        call("bsk_iso_leaf", *leaf, 1, be.ptr(toffsets), total, None, None, be.ptr(tris))
        # where the fields start among the leaves, the triangles and (below) the vertices
        leaf_start = be.searchsorted(leaves // per_field, B + 1)
        tstart = be.get(be.cat([be.zeros(1, np.int64), tends])[leaf_start]).tolist()
        keys, fields, triangles, vstart = _cells.weld(be, tris, tstart)
        xyz = be.empty((len(keys), 3), np.float64)
        breaks = [be.put(b, np.float64) for b in plan.breaks]
        call("bsk_iso_vertex", *grid, *map(be.ptr, breaks), be.ptr(keys), be.ptr(fields), len(keys), depth, be.ptr(xyz))
        out.update(keys=keys, xyz=xyz, vertex_offsets=vstart, triangles=triangles, triangle_offsets=be.put(tstart, np.int64))
        return finish()


def _run_host(rows, plan, levels, scale, depth, split):
    """``_run`` on NumPy arrays."""
    rows, levels, scale = (None if a is None else np.ascontiguousarray(a, np.float64) for a in (rows, levels, scale))
    return _run(_cells.Host(), rows, plan, levels, scale, depth, split)


# ------------------------------------------------------------------------------------------ public
class Plan(_cells.JumpFreePlan):
    """``_cells.TensorPlan`` that refuses a jump: an interior knot of multiplicity >= K."""
    who, what = "isosurface", "surface"


def _check_spline(spline):
    if spline.nInd != 3:
        raise ValueError("isosurface: three independent variables (a scalar field over a volume's parameters)")
    if min(spline.order) < DEVICE_MIN_K or max(spline.order) > DEVICE_MAX_K:
        raise NotImplementedError(f"isosurface: orders from {DEVICE_MIN_K} to {DEVICE_MAX_K} (one wave holds the 64 coefficients of a cell)")


def _check_batch(spline):
    if spline.nInd != 3:
        raise ValueError("extract_batch takes three independent variables")
    _check_spline(spline)


def _check_keys(plan, depth, B):
    nodes = 1
    for n in plan.ncells:
        nodes *= (int(n) << depth) + 1
    if 8 * nodes >= 1 << 62 or 8 * B * nodes >= 1 << 62:
        raise ValueError(f"isosurface: the lattice of {' x '.join(str((int(n) << depth) + 1) for n in plan.ncells)} nodes has keys beyond 62 bits; "
                         "lower the depth or trim the spline")


# tables(spline, levels=None, coefs=None): the host path's tables: (plan, rows (nrows, R0, R1, R2), levels or None,
# scale (B)), all NumPy float64
tables = functools.partial(_cells.level_tables, _THIS)


def extract_batch(spline, levels=None, coefs=None, depth=None, _path=None, _split=None):
    """The zero sets of B scalar fields in three variables on the spline's knots as triangle meshes on a lattice of
    2^depth leaves per knot cell and axis (depth 0 .. 6, default 3).  The fields are the spline itself (nDep 1), the
    spline minus ``levels[b]`` (one extraction for all levels), or ``coefs`` (B, n0, n1, n2).
    Returns (vertices, keys, vertex_offsets, triangles, triangle_offsets, cells, status): the vertices of field b are
    vertices[vertex_offsets[b]:vertex_offsets[b + 1]], rows (u, v, w) in float64, in ascending order of their integer
    lattice-edge ``keys``; its triangles are triangles[triangle_offsets[b]:triangle_offsets[b + 1]], rows of indices into
    ``vertices`` whose right-hand normal points into f >= 0, in ascending (leaf, tetrahedron, triangle) order.  ``cells``
    (NumPy float64, k x 7) holds one row (field, u0, u1, v0, v1, w0, w1) per zero cell; ``status`` (uint8,
    B x nc0 x nc1 x nc2) has bit 1 on a zero cell and bit 2 where a lattice node value was exactly 0.0.
    ``coefs``: a float32 / float64 torch CUDA tensor (any strides) takes the device path; vertices, keys, triangles and
    status are then CUDA tensors and never leave the device.
    ``_split`` pins the split level P of the walk launches (0 .. depth); the result does not depend on it."""
    be, on_device, plan, B, res, cells = _cells.level_batch(_THIS, spline, levels, coefs, depth, _path, _split)
    if B == 0:
        return (be.empty((0, 3), np.float64), be.empty(0, np.int64), be.zeros(1, np.int64), be.empty((0, 3), np.int64),
                be.zeros(1, np.int64), cells, be.zeros((0,) + tuple(plan.ncells), np.uint8))
    if not on_device:
        res = _cells.to_host(be, res)
    return res["xyz"], res["keys"], res["vertex_offsets"], res["triangles"], res["triangle_offsets"], cells, res["status"]


def isosurface(self, level=0.0, tolerance=None, depth=None, normals=False, _path=None):
    """``Spline.isosurface``: (vertices (n, 3) float64, triangles (m, 3) int64) of {f = level}, and with ``normals`` the
    normalised gradient at every vertex (n, 3), NaN where the gradient is zero."""
    if self.nInd != 3 or self.nDep != 1:
        raise ValueError("The spline must have three independent variables and one dependent variable (nInd == 3, nDep == 1).")
    _check_spline(self)
    if depth is None:
        depth = depth_of(tolerance, Plan(self.order, self.knots))
    vertices, _, _, triangles, _, _, _ = extract_batch(self, levels=[float(level)], depth=depth, _path=_path)
    if not normals:
        return vertices, triangles
    if len(vertices):
        gradient = np.asarray(self.jacobian([vertices[:, 0], vertices[:, 1], vertices[:, 2]]), np.float64)[0].T
    else:
        gradient = vertices[:0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return vertices, triangles, gradient / np.sqrt((gradient * gradient).sum(axis=1, keepdims=True))
