"""
Watertight triangle meshes of parametric surfaces within a tolerance: ``Spline.triangulate`` for nInd == 2, nDep 1 .. 3 and
``triangulate_batch`` for B coefficient nets on the same knots.  The reference has this only as a picture: its
tessellation shaders take a sample rate per knot cell from second derivatives and give every cell edge the larger rate of
its two neighbours.  Here the same is data, with a stated distance bound.

After Bezier extraction of the two variables (the band operator of refinement.py, once per axis) every knot cell of
positive width holds one polynomial patch with the net b[i][j][d], cell-local on [0, 1]^2.  ``mesh_bound`` bounds the second
derivatives of every cell from the second differences of its net and turns them into two levels; the cell carries
2^a x 2^b grid quads.  ``mesh_count`` counts the triangles of every quad from the segments on its four sides, ``mesh_emit``
writes them as triples of integer vertex keys at the scanned offsets, the sorted unique keys of a member are its
vertices, and ``mesh_vertex`` evaluates each one by de Casteljau.

    device path   ``bsk_band_apply`` per axis with the rows on the device, ``bsk_mesh_bound``, ``torch.cumsum``,
                  ``bsk_mesh_count``, ``torch.cumsum``, ``bsk_mesh_emit``, ``torch.unique`` per member, ``bsk_mesh_vertex``
    host path     ``bsk_roots_extract_host`` per axis and the ``bsk_mesh_*_host`` twins: the same functions of bsk_mesh.hpp
                  on the CPU, NumPy in place of torch, for few cells

THE CLAIM.  For every triangle and every point x of it in parameter space |S(x) - L(x)| <= bound[cell] <= tolerance
(1 + 8 eps) + the counted slack below, L the linear interpolant of the exact surface at the triangle's corners; the
returned vertices differ from the exact surface by the arithmetic of the extraction and of de Casteljau, at most
2 (K0 + K1) eps S, S = max |coefficient| of the member.  The triangles tile the domain exactly: no cracks and no
T-junctions, decided in integers.  A cell that needs more than ``max_level`` is meshed at the cap, has status bit 1 and its
true bound in ``bound``.

THE STATEMENT (the functions below say it in plain Python floats, bit for bit what bsk_mesh.hpp computes: fp64, every
product and sum rounded on its own):
  * cells: the knot cells of positive width, ``TensorPlan.breaks``; cell (i, j) of member b, component d is the K0 x K1
    window at first0[i], first1[j] of the extracted rows (B, nDep, R0, R1); float32 is widened before the extraction.  An
    interior knot of multiplicity >= K is refused (a jump), so adjacent cells share their end row: the same floats;
    neighbours are adjacent entries of ``breaks``;
  * bounds (``bounds``): D2u = (b[i+2][j] - b[i+1][j]) - (b[i+1][j] - b[i][j]), D2v alike along j,
    Duv = (b[i+1][j+1] - b[i][j+1]) - (b[i+1][j] - b[i][j]); per (i, j) the squares are summed over d = 0, 1, 2 from 0.0;
    the maximum runs over (i, j) in row-major order from 0.0; Quu = (p (p - 1))^2 max |D2u|^2, Qvv = (q (q - 1))^2
    max |D2v|^2, Quv = (p q)^2 max |Duv|^2 with p = K0 - 1, q = K1 - 1 (the integer factor times the maximum, rounded once).
    By the convex-hull property they bound |S_uu|^2, |S_vv|^2, |S_uv|^2 on the cell, in its own parameters;
  * levels (``level_of``): T = (2 tol) (2 tol); a = the least level in 0 .. max_level with max(Quu, Quv) <= T 16^a, b the same
    with Qvv for Quu; T 16^a is exact, so coefficients and tolerance times 2^k keep every level.  No such level:
    max_level and status bit 1;
  * why it certifies: a triangle with its corners on the surface inside an h_u x h_v rectangle of one cell has
    |S - L| <= (h_u^2 M_uu + 2 h_u h_v M_uv + h_v^2 M_vv) / 8; with h_u = 2^-a, h_v = 2^-b and the
    rule above every term is at most 2 tol, 4 tol, 2 tol;
  * quads: quad l of a cell is (r, s) = (l >> b, l & (2^b - 1)); the quads of all cells are numbered through in
    (member, i, j) order;
  * edge levels: the side of a quad on an edge of its cell carries 2^(e - own) segments, e the larger of the two cells'
    levels along that edge (a domain edge: its own); a multiple knot puts nothing between two cells; every other side: one;
  * triangles (``quad_triangles``): four sides of one segment: (P00, P10, P11), (P00, P11, P01), the diagonal from (r, s) to
    (r + 1, s + 1); otherwise the centre C and one triangle (C, P_k, P_k+1) per segment of the perimeter, counter-clockwise
    from P00 (bottom, right, top, left).  Every triangle is counter-clockwise in (u, v) and lies inside one grid quad;
  * keys: a vertex is (X << 31) | Y, X = (i << 11) + the local coordinate in units of 2^-11 of cell i (a centre is a half
    step of its level, which level 10 still finds in 11 bits), Y alike: both cells of a shared edge give the same key;
  * vertices: a member's vertices are its sorted unique keys (``be.unique``, whose inverse is the ``searchsorted`` of the
    triangles' keys among them).  Per axis the owner is the cell min(X >> 11, nc - 1): a point on an interior knot line
    belongs to the cell above it, t = 0 there, and only the domain's end has t = 1; t = (X - (cell << 11)) 2^-11 exactly.
    Per component (``vertex``): every row of the window is reduced along axis 1 at t1 by de Casteljau (levels of
    (1 - t) c[i] + t c[i + 1]) down to two points, V[r] = (1 - t1) lo + t1 hi, W[r] = hi - lo; V is reduced along
    axis 0 at t0 down to (lo, hi): position = (1 - t0) lo + t0 hi, S_u = p (hi - lo), S_v = q value(W, t0).
    uv = lo + t (hi - lo) of the owner's breaks.  With ``normals`` the raw S_u x S_v (nDep 3) in the cell's own
    parameters: (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); ``Spline.triangulate`` normalises it in NumPy on the host,
    outside the byte claim;
  * order: a member's vertices by ascending key; triangles by ascending (quad, position in the quad);
  * ``bound`` (NumPy on the host, one code path): (h_u^2 sqrt(Quu) + 2 h_u h_v sqrt(Quv) + h_v^2 sqrt(Qvv)) / 8 times
    (1 + 8 eps), plus the slack (h_u^2 p (p - 1) + 2 h_u h_v p q + h_v^2 q (q - 1)) / 8 x (2 (K0 + K1) + 8) eps S sqrt(nDep)
    for the roundings of the net and of the differences (an absolute error: differences cancel).
NOT BUILT: seams and poles are not welded (vertices are identified by parameter, triangles that are degenerate in space
are kept); curves; view-dependent rates; trimmed surfaces; orders 5 and 6.

``_path="device" | "host"`` (or ``mesh.FORCE_PATH``) pins the path; ``mesh.LAST_PATHS`` lists what the last call ran.
"""
import math
import warnings

import numpy as np

from . import _cells
from . import _native as nv
from . import roots

SCOPE = "triangulate: surfaces (nInd == 2) with nDep 1 .. 3 and orders 2 .. 4"
# (member, cell) pairs from which the device path is taken: all that is known before the bound pass.  Read off the calls
# table of tools/mesh_time.py on an MI355X: a bump on a bicubic plate at tolerance 1e-3, 256 cells
# 1.27 ms on the host against 1.65 ms, 1024 cells 2.01 against 1.80.  The triangles matter too: 256 cells with 38 672
# triangles (tolerance 1e-4) already take 3.1 ms on the host against 1.9 ms; ``_path`` pins the path of such a call.
DEVICE_MIN_WORK = 1 << 10
DEVICE_MIN_K, DEVICE_MAX_K = 2, 4
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

EPS = roots.EPS
L = 11
SHIFT = 31
DEFAULT_MAX_LEVEL, MAX_LEVEL = 8, 10
DEFAULT_MAX_TRIANGLES = 1 << 28
QUAD_CHUNK = 1 << 24       # quads per launch of mesh_count and mesh_emit
STATUS_CAPPED = 1


# ------------------------------------------------------------------------------------------ the statement
def threshold(tolerance):
    t2 = 2.0 * float(tolerance)
    return t2 * t2


def cell_net(rows, plan, b, d, i, j):
    """The K0 x K1 floats of component d of cell (i, j) of member b."""
    K0, K1 = plan.order
    f0, f1 = int(plan.first[0][i]), int(plan.first[1][j])
    return [[float(rows[b, d, f0 + r, f1 + s]) for s in range(K1)] for r in range(K0)]


def bounds(nets):
    """(Quu, Qvv, Quv) of one cell: ``nets`` = its K0 x K1 floats per component."""
    K0, K1 = len(nets[0]), len(nets[0][0])
    p, q = K0 - 1, K1 - 1

    def largest(terms):
        m = 0.0
        for at in terms:
            total = 0.0
            for c in nets:
                x = at(c)
                total = total + x * x
            m = total if total > m else m
        return m

    uu = largest([lambda c, r=r, s=s: (c[r + 2][s] - c[r + 1][s]) - (c[r + 1][s] - c[r][s]) for r in range(K0 - 2) for s in range(K1)])
    vv = largest([lambda c, r=r, s=s: (c[r][s + 2] - c[r][s + 1]) - (c[r][s + 1] - c[r][s]) for r in range(K0) for s in range(K1 - 2)])
    uv = largest([lambda c, r=r, s=s: (c[r + 1][s + 1] - c[r][s + 1]) - (c[r + 1][s] - c[r][s]) for r in range(K0 - 1) for s in range(K1 - 1)])
    return float((p * (p - 1)) ** 2) * uu, float((q * (q - 1)) ** 2) * vv, float((p * q) ** 2) * uv


def level_of(q, T, max_level):
    """(level, capped)."""
    for a in range(max_level + 1):
        if q <= T * float(1 << (4 * a)):
            return a, False
    return max_level, True


def key_of(X, Y):
    return (X << SHIFT) | Y


def unkey(key):
    return key >> SHIFT, key & ((1 << SHIFT) - 1)


def side_levels(lev, i, j, r, s):
    """The levels (bottom, right, top, left) of the four sides of quad (r, s) of cell (i, j); lev: (nc0, nc1, 2) ints."""
    nc0, nc1 = len(lev), len(lev[0])
    a, b = int(lev[i][j][0]), int(lev[i][j][1])
    eb = max(a, int(lev[i][j - 1][0])) if s == 0 and j > 0 else a
    et = max(a, int(lev[i][j + 1][0])) if s == (1 << b) - 1 and j + 1 < nc1 else a
    el = max(b, int(lev[i - 1][j][1])) if r == 0 and i > 0 else b
    er = max(b, int(lev[i + 1][j][1])) if r == (1 << a) - 1 and i + 1 < nc0 else b
    return eb, er, et, el


def quad_triangles(lev, i, j, r, s):
    """The key triples of quad (r, s) of cell (i, j)."""
    a, b = int(lev[i][j][0]), int(lev[i][j][1])
    eb, er, et, el = side_levels(lev, i, j, r, s)
    X0 = (i << L) + (r << (L - a))
    X1 = X0 + (1 << (L - a))
    Y0 = (j << L) + (s << (L - b))
    Y1 = Y0 + (1 << (L - b))
    if (eb, et) == (a, a) and (el, er) == (b, b):
        return [(key_of(X0, Y0), key_of(X1, Y0), key_of(X1, Y1)), (key_of(X0, Y0), key_of(X1, Y1), key_of(X0, Y1))]
    C = key_of(X0 + (1 << (L - 1 - a)), Y0 + (1 << (L - 1 - b)))
    hb, hr, ht, hl = (1 << (L - e) for e in (eb, er, et, el))
    out = [(C, key_of(X0 + k * hb, Y0), key_of(X0 + (k + 1) * hb, Y0)) for k in range(1 << (eb - a))]
    out += [(C, key_of(X1, Y0 + k * hr), key_of(X1, Y0 + (k + 1) * hr)) for k in range(1 << (er - b))]
    out += [(C, key_of(X1 - k * ht, Y1), key_of(X1 - (k + 1) * ht, Y1)) for k in range(1 << (et - a))]
    out += [(C, key_of(X0, Y1 - k * hl), key_of(X0, Y1 - (k + 1) * hl)) for k in range(1 << (el - b))]
    return out


def owner_of(X, nc):
    """(cell, t) of the key coordinate X."""
    cell = min(X >> L, nc - 1)
    return cell, float(X - (cell << L)) * 2.0 ** -L


def two_left(c, x):
    """de Casteljau at x down to the last two points."""
    b = list(c)
    s = 1.0 - x
    for r in range(1, len(b) - 1):
        for i in range(len(b) - r):
            b[i] = s * b[i] + x * b[i + 1]
    return b[0], b[1]


def vertex(nets, t0, t1):
    """(position, S_u, S_v) per component of the cell ``nets`` at the local (t0, t1)."""
    K0, K1 = len(nets[0]), len(nets[0][0])
    pos, su, sv = [], [], []
    for c in nets:
        V, W = [], []
        for r in range(K0):
            lo, hi = two_left(c[r], t1)
            V.append((1.0 - t1) * lo + t1 * hi)
            W.append(hi - lo)
        lo, hi = two_left(V, t0)
        pos.append((1.0 - t0) * lo + t0 * hi)
        su.append(float(K0 - 1) * (hi - lo))
        sv.append(float(K1 - 1) * roots.value(W, t0))
    return pos, su, sv


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def statement(rows, plan, tolerance, max_level=DEFAULT_MAX_LEVEL, normals=False):
    """The raw result of the extracted rows (B, nDep, R0, R1) from the functions above: what the host drivers and the
    kernels return, bit for bit."""
    B, ndep = rows.shape[:2]
    nc0, nc1 = plan.ncells
    T = threshold(tolerance)
    Q = np.zeros((B, nc0, nc1, 3))
    lev = np.zeros((B, nc0, nc1, 2), np.int32)
    status = np.zeros((B, nc0, nc1), np.uint8)
    keys, uv, xyz, nrm, voff, tris, toff = [], [], [], [], [0], [], [0]
    for b in range(B):
        nets = {}
        for i in range(nc0):
            for j in range(nc1):
                nets[i, j] = [cell_net(rows, plan, b, d, i, j) for d in range(ndep)]
                Q[b, i, j] = quu, qvv, quv = bounds(nets[i, j])
                la, ca = level_of(max(quu, quv), T, max_level)
                lb, cb = level_of(max(qvv, quv), T, max_level)
                lev[b, i, j] = la, lb
                status[b, i, j] = STATUS_CAPPED * (ca or cb)
        table = lev[b].tolist()
        found = []
        for i in range(nc0):
            for j in range(nc1):
                la, lb = table[i][j]
                for l in range(1 << (la + lb)):
                    found.extend(quad_triangles(table, i, j, l >> lb, l & ((1 << lb) - 1)))
        unique = sorted({key for triangle in found for key in triangle})
        index = {key: len(keys) + n for n, key in enumerate(unique)}
        keys.extend(unique)
        for key in unique:
            X, Y = unkey(key)
            (i, t0), (j, t1) = owner_of(X, nc0), owner_of(Y, nc1)
            pos, su, sv = vertex(nets[i, j], t0, t1)
            xyz.append(pos)
            u0, u1, v0, v1 = (float(x) for x in (plan.breaks[0][i], plan.breaks[0][i + 1], plan.breaks[1][j], plan.breaks[1][j + 1]))
            uv.append((u0 + t0 * (u1 - u0), v0 + t1 * (v1 - v0)))
            if normals:
                nrm.append(cross(su, sv))
        tris.extend(tuple(index[key] for key in triangle) for triangle in found)
        voff.append(len(keys))
        toff.append(len(tris))
    out = dict(Q=Q, lev=lev, status=status, keys=np.array(keys, np.int64), uv=np.array(uv, np.float64).reshape(-1, 2),
               xyz=np.array(xyz, np.float64).reshape(-1, ndep), vertex_offsets=np.array(voff, np.int64),
               triangles=np.array(tris, np.int64).reshape(-1, 3), triangle_offsets=np.array(toff, np.int64))
    if normals:
        out["normals"] = np.array(nrm, np.float64).reshape(-1, 3)
    return out


def bound_of(Q, lev, order, scale, ndep):
    """``bound`` (B, nc0, nc1): the certified |S - L| of every cell at its levels, NumPy on the host (the statement says
    what the two terms are); scale: (B) = max |coefficient|."""
    Q, lev = np.asarray(Q, np.float64), np.asarray(lev)
    p, q = order[0] - 1, order[1] - 1
    hu, hv = np.ldexp(1.0, -lev[..., 0]), np.ldexp(1.0, -lev[..., 1])
    raw = 0.125 * (hu * hu * np.sqrt(Q[..., 0]) + 2.0 * hu * hv * np.sqrt(Q[..., 2]) + hv * hv * np.sqrt(Q[..., 1]))
    slack = 0.125 * (hu * hu * (p * (p - 1)) + 2.0 * hu * hv * (p * q) + hv * hv * (q * (q - 1)))
    slack = slack * ((2.0 * sum(order) + 8.0) * EPS * math.sqrt(ndep)) * np.asarray(scale, np.float64).reshape(-1, 1, 1)
    return raw * (1.0 + 8.0 * EPS) + slack


# ------------------------------------------------------------------------------------------ the launches
def _last():
    return nv.lib().bsk_mesh_last_kernel().decode()


def _run(be, rows, plan, tolerance, max_level, normals, chunk, max_triangles):
    """rows: float64 (B, nDep, R0, R1) in Bezier form, the backend's contiguous array.  -> dict of Q (B, nc0, nc1, 3), lev
    (B, nc0, nc1, 2), status (B, nc0, nc1), keys (n), uv (n, 2), xyz (n, nDep), normals (n, 3) or None, vertex_offsets
    (B + 1), triangles (m, 3), triangle_offsets (B + 1), the backend's, and nquads."""
    B, ndep = int(rows.shape[0]), int(rows.shape[1])
    nc0, nc1 = (int(n) for n in plan.ncells)
    per_member = nc0 * nc1
    ncells = B * per_member
    chunk = QUAD_CHUNK if chunk is None else int(chunk)

    def call(name, *args):
        be.call(name, *args)
        LAST_PATHS.append(_last())

    with be:
        first = [be.put(f, np.int32) for f in plan.first]
        net = tuple(plan.order) + (be.ptr(rows), B, ndep) + tuple(plan.rowlen) + (nc0, nc1) + tuple(be.ptr(f) for f in first)
        Q, lev = be.empty((B, nc0, nc1, 3), np.float64), be.empty((B, nc0, nc1, 2), np.int32)
        status = be.empty((B, nc0, nc1), np.uint8)
        call("bsk_mesh_bound", *net, threshold(tolerance), max_level, be.ptr(Q), be.ptr(lev), be.ptr(status))
        flat = be.cast(lev.reshape(-1, 2), np.int64)
        ends = be.cumsum(2 ** (flat[:, 0] + flat[:, 1]))
        qoff = be.cat([be.zeros(1, np.int64), ends])
        nquads, span = int(ends[-1]), 1 << int(flat.max() - flat.min())
        quads = (be.ptr(qoff), ncells, nc0, nc1, be.ptr(lev), (ncells - 1).bit_length(), span)
        counts = be.empty(nquads, np.int32)
        for start in range(0, nquads, chunk):
            call("bsk_mesh_count", *quads, start, min(chunk, nquads - start), nquads, be.ptr(counts))
        tends = be.cumsum(counts)
        total = int(tends[-1])
        if total > max_triangles:
            raise ValueError(f"triangulate: {total} triangles exceed max_triangles = {max_triangles}; raise the tolerance or max_triangles")
        offsets = tends - be.cast(counts, np.int64)                   # int64, a fresh contiguous array
        tris = be.empty((total, 3), np.int64)
        for start in range(0, nquads, chunk):
            call("bsk_mesh_emit", *quads, start, min(chunk, nquads - start), nquads, be.ptr(offsets), total, be.ptr(tris))
        # where the members start among the triangles and (below) the vertices
        tstart = be.get(be.cat([be.zeros(1, np.int64), tends])[qoff[::per_member]]).tolist()
        keys, members, triangles, vstart = _cells.weld(be, tris, tstart)
        n = len(keys)
        uv, xyz = be.empty((n, 2), np.float64), be.empty((n, ndep), np.float64)
        nrm = be.empty((n, 3), np.float64) if normals else None
        breaks = [be.put(b, np.float64) for b in plan.breaks]
        call("bsk_mesh_vertex", *net, *map(be.ptr, breaks), be.ptr(keys), be.ptr(members), n, be.ptr(uv), be.ptr(xyz), be.ptr(nrm))
        return dict(Q=Q, lev=lev, status=status, keys=keys, uv=uv, xyz=xyz, normals=nrm, vertex_offsets=vstart,
                    triangles=triangles, triangle_offsets=be.put(tstart, np.int64), nquads=nquads)


def _run_host(rows, plan, tolerance, max_level=DEFAULT_MAX_LEVEL, normals=False, chunk=None, max_triangles=DEFAULT_MAX_TRIANGLES):
    """``_run`` on NumPy arrays."""
    return _run(_cells.Host(), np.ascontiguousarray(rows, np.float64), plan, tolerance, max_level, normals, chunk, max_triangles)


# ------------------------------------------------------------------------------------------ public
class Plan(_cells.JumpFreePlan):
    """``_cells.TensorPlan`` that refuses a jump: an interior knot of multiplicity >= K."""
    who, what = "triangulate", "mesh"


def _check_spline(spline):
    if spline.nInd != 2 or not 1 <= spline.nDep <= 3 or min(spline.order) < DEVICE_MIN_K or max(spline.order) > DEVICE_MAX_K:
        raise ValueError(SCOPE)


def tables(spline, coefs=None):
    """The host path's tables: (plan, rows (B, nDep, R0, R1), scale (B)), NumPy float64."""
    plan = Plan(spline.order, spline.knots)
    data = np.asarray(spline.coefs if coefs is None else coefs)
    be, data, rows = _cells.bezier_rows(data.reshape((-1,) + data.shape[-3:]), "host", plan, LAST_PATHS, finite="triangulate")
    return plan, rows, _cells.field_scale(be, data)


def triangulate_batch(spline, tolerance, coefs=None, max_level=DEFAULT_MAX_LEVEL, max_triangles=DEFAULT_MAX_TRIANGLES, normals=False,
                      _path=None, _chunk=None):
    """Triangle meshes within ``tolerance`` of B surfaces on the spline's knots: the spline itself, or ``coefs``
    (B, nDep, n0, n1).  Returns (uv, xyz, vertex_offsets, triangles, triangle_offsets, levels, bound, status) and, with
    ``normals`` (nDep 3), the raw S_u x S_v per vertex behind them.  The vertices of member b are rows
    vertex_offsets[b]:vertex_offsets[b + 1] of uv (n, 2) and xyz (n, nDep), float64, in ascending order of their integer
    keys; its triangles are rows triangle_offsets[b]:triangle_offsets[b + 1] of triangles (m, 3), int64 indices into the
    vertices, counter-clockwise in (u, v).  levels (B, nc0, nc1, 2) int32 holds (a, b) of every knot cell, bound
    (B, nc0, nc1), NumPy float64, the certified |S - L| of every cell, status (B, nc0, nc1) uint8 bit 1 on a cell that is
    meshed at ``max_level`` (0 .. 10) although it needs more: the call then gives one RuntimeWarning.  More than
    ``max_triangles`` triangles: ValueError before they are written.
    ``coefs``: a float32 / float64 torch CUDA tensor (any strides) takes the device path; every result but ``bound`` is then
    a CUDA tensor.  ``_chunk`` pins the quads per launch of the two quad passes; the result does not depend on it."""
    del LAST_PATHS[:]
    path = _cells.pick_path(_path, FORCE_PATH)
    _check_spline(spline)
    tolerance = float(tolerance)
    if not (math.isfinite(tolerance) and tolerance > 0.0):
        raise ValueError("triangulate: tolerance must be finite and > 0")
    max_level = int(max_level)
    if not 0 <= max_level <= MAX_LEVEL:
        raise ValueError(f"triangulate: max_level must be in 0 .. {MAX_LEVEL}")
    if _chunk is not None and int(_chunk) < 1:
        raise ValueError("_chunk must be >= 1")
    n0, n1 = (len(spline.knots[d]) - spline.order[d] for d in range(2))
    if coefs is None:
        coefs = np.asarray(spline.coefs)[None]
    coefs, on_device, path = _cells.coefs_arg("triangulate_batch", coefs, path, (range(1, 4), n0, n1),
                                              f"(B, nDep, {n0}, {n1}) with nDep in 1 .. 3")
    B, ndep = int(coefs.shape[0]), int(coefs.shape[1])
    if normals and ndep != 3:
        raise ValueError("triangulate: normals take three dependent variables")
    plan = Plan(spline.order, spline.knots)
    nc = tuple(int(n) for n in plan.ncells)
    if max(nc) >= 1 << 20:
        raise ValueError("triangulate: more than 2^20 - 1 knot cells per variable do not fit the keys")
    if path is None:
        path = "device" if B * nc[0] * nc[1] >= DEVICE_MIN_WORK else "host"

    if B == 0:
        be = _cells.backend_of(coefs)
        out = (be.empty((0, 2), np.float64), be.empty((0, ndep), np.float64), be.zeros(1, np.int64), be.empty((0, 3), np.int64),
               be.zeros(1, np.int64), be.empty((0,) + nc + (2,), np.int32), np.empty((0,) + nc), be.empty((0,) + nc, np.uint8))
        return out + (be.empty((0, 3), np.float64),) if normals else out

    be, data, rows = _cells.bezier_rows(coefs, path, plan, LAST_PATHS, finite="triangulate")
    scale = be.get(_cells.field_scale(be, data))
    res = _run(be, rows, plan, tolerance, max_level, normals, _chunk, max_triangles)
    Q, lev, flags = (be.get(res[name]) for name in ("Q", "lev", "status"))
    if not on_device:
        res = _cells.to_host(be, res)
    bound = bound_of(Q, lev, plan.order, scale, ndep)
    capped = int(np.count_nonzero(flags))
    if capped:
        warnings.warn(f"triangulate: {capped} cells need more than max_level = {max_level}; they are meshed at the cap and within "
                      f"{float(bound.max()):.3g} of the surface instead of {tolerance:.3g} (status bit 1, bound)", RuntimeWarning, stacklevel=2)
    out = (res["uv"], res["xyz"], res["vertex_offsets"], res["triangles"], res["triangle_offsets"], res["lev"], bound, res["status"])
    return out + (res["normals"],) if normals else out


def triangulate(self, tolerance, parameters=False, normals=False, max_level=DEFAULT_MAX_LEVEL, max_triangles=DEFAULT_MAX_TRIANGLES, _path=None):
    """``Spline.triangulate``: (xyz (n, nDep) float64, triangles (m, 3) int64), then uv (n, 2) with ``parameters`` and the
    unit normals (n, 3) with ``normals`` (NaN where S_u x S_v vanishes); ``metadata['negateNormal']`` flips the triangles
    and the normals."""
    _check_spline(self)
    if normals and self.nDep != 3:
        raise ValueError("triangulate: normals take three dependent variables")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = triangulate_batch(self, tolerance, max_level=max_level, max_triangles=max_triangles, normals=normals, _path=_path)
    for w in caught:
        warnings.warn(w.message, w.category, stacklevel=3)
    uv, xyz, triangles = res[0], res[1], res[3]
    negate = bool(getattr(self, "metadata", {}).get("negateNormal", False))
    if negate:
        triangles = np.ascontiguousarray(triangles[:, [0, 2, 1]])
    out = (xyz, triangles) + ((uv,) if parameters else ())
    if normals:
        raw = -res[8] if negate else res[8]
        with np.errstate(invalid="ignore", divide="ignore"):
            out += (raw / np.sqrt((raw * raw).sum(axis=1, keepdims=True)),)
    return out
