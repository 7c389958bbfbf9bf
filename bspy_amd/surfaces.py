"""
Surface-surface intersection: ``Spline.intersect_surface`` and ``trace_pair`` (the reference's ``intersect`` of two
surfaces, bspy/_spline_intersection.py, is ``contours`` of a four-variable ``subtract``, a serial tracer).  Two surfaces a
and b (nInd 2, nDep 3, orders 2 to 4).  Each carries a lattice of isoparametric lines, G = 2^depth per knot cell and
variable, and every vertex of the intersection curve is a hit of one lattice line of one surface on the other surface: a
``zeros3`` system F(w, s, t) = L(w) - Y(s, t) with the Bernstein coefficients F_ijk = L_i - Y_jk (the partition of unity
makes each one a single subtraction).  The systems are never stored: a pair's coefficients are formed wherever they are
needed, almost every pair (line segment, cell) is discarded by a box test, and the few that remain are walked by the
``roots3`` walk, unchanged, one wave per pair.  The curve is decided on the two lattices and on nothing finer.

    device path   ``bsk_band_apply`` per axis and surface with the rows on the device, ``bsk_rays_boxes`` of both, then
                  per family of lines (a's with u fixed, a's with v fixed, b's with s fixed, b's with t fixed) and per pass
                  of segments ``bsk_ssx_count``, ``torch.cumsum``, ``bsk_ssx_emit``, ``bsk_ssx_isolate`` and, once per family,
                  ``bsk_ssx_merge``; a pass without a pair skips emit and isolate, a family without a zero near a face of
                  its cell skips the merge
    host path     ``bsk_roots_extract_host`` per axis, then the ``*_host`` twins of the same entry points: the same
                  functions of bsk_ssx.hpp on the CPU, a lane array becoming a loop over 64 entries
    linking       NumPy and a walk on the host, on both paths: a sort by integer keys, not a kernel

THE STATEMENT (``line_points``, ``form_pair``, ``pair_kind``, ``merge_keep``, ``roots3.isolate_cell`` and the NumPy text of
``vertices_of`` and ``link`` say it, bit for bit what bsk_ssx.hpp computes; float64 whatever the dtypes, float32 is widened
first, no contraction, ``roots._lerp``'s association s a + t b; eps of float64):
  1. extraction: both surfaces go to Bezier form with the band operators of ``_cells.TensorPlan``; cell (i, j), flat index
     i nc1 + j, is the K0 x K1 window of the three components; boxes[cell] = min and max of the window per component
     (``bsk_rays_boxes``).  An interior knot of multiplicity >= K is refused (a jump).  S_d = max |a's coefficient d| +
     max |b's coefficient d| on the widened B-spline coefficients: it bounds every component of every system and takes the
     place of ``roots3``'s S_d;
  2. lattice: G = 2^depth leaves per knot cell and variable on both surfaces, depth 0 .. 6, default 2 (point 10).  From
     ``tolerance`` the depth is ``contours``' rule ((h 2^-d)^2 <= tolerance L) on each surface, the larger of the two, at
     most 6.  A LINE is (surface X, fixed variable ax, n), 0 <= n <= nc_ax G: it is owned by cell c = min(n // G,
     nc_ax - 1) at the dyadic local value x = (n - c G) / G, so the last line of the domain is owned by the last cell at
     x = 1.  Its parameter value is the canonical float t_c when x = 0, t_{c+1} when x = 1, else (1 - x) t_c + x t_{c+1}
     (``line_values``).  On the running cell e the line is a Bezier curve of KR points per component (KR the order of the
     running variable): point i is ``roots.value`` at x of column i (ax = 0) or row i (ax = 1) of the window of cell
     (c, e) or (e, c); x = 0 and x = 1 copy the first and the last entry;
  3. pair and system: a pair is (line segment (X, ax, n, e), cell (p, q) of the other surface Y); F_ijk = L_i - Y_jk, one
     subtraction each, of orders (KR, KY0, KY1), coefficient (i, j, k) of lane (i KY0 + j) KY1 + k;
  4. candidates: ``roots3``'s rules on the formed coefficients.  ``inbox``: the box of the segment's own KR points and the
     box of Y's cell are not strictly disjoint in any component (an exact comparison).  A pair is FLAT when inbox holds and
     all values of some component are below S_d eps in magnitude (or S_d is 0): status bit 16, nothing reported.  Any
     other pair is a candidate unless a component is strictly of one sign.  The prefilter drops a pair that is not inbox
     before it reads Y's window.  Such a pair is strictly of one sign in that component (the difference of two different
     doubles is not 0 and has the sign of the exact one) and FLAT asks for inbox, so ``_prefilter=False`` gives the same
     bytes in every output.  (The segment's own box, not the box of X's whole cell: in floating point a de Casteljau
     value may leave the hull of its column by an ulp, and only the box of the very numbers that are subtracted makes
     the comparison exact.);
  5. walk: ``roots3.isolate_cell`` unchanged on the formed coefficients with (S_0, S_1, S_2): DEPTH, the Newton rule, the
     slots R = min(6 (KR - 1)(KY0 - 1)(KY1 - 1), 32), WALK, the status bits 1, 2, 4 and the near bytes.  A zero is
     (w, s, t): w on X's running variable in [t_e, t_{e+1}], (s, t) in Y's cell;
  6. merge: ``roots3_merge``'s rule among the pairs of the same line: a near zero is dropped when one of the 13 lower
     neighbours (e + de, p + dp, q + dq) holds a zero within 2^-20 h on all three axes, h the widths of its own pair.  The
     pairs are sorted by (segment, Y cell), so a neighbour is found by binary search in the keys segment ncellY + cell;
  7. vertex: (u, v, s, t); the fixed coordinate is the line's canonical value, the other three are the zero.  The vertex
     key is (family 0 .. 3, n, e, Y cell, slot) in lexicographic order; family = 2 [X is b] + ax;
  8. product leaves: the leaf of a free coordinate z in its cell [t0, t0 + h] is min(floor(((z - t0) / h) G), G - 1), its
     global index cell G + leaf; the fixed coordinate bounds the leaves n - 1 and n of its variable where they exist.  So a
     vertex bounds one or two PRODUCT LEAVES (iA0, iA1, iB0, iB1), packed into one int64 with 15 bits each.  A product
     leaf with exactly two vertices is a segment; with one it sets bit 32 (odd), with three or more bit 64 (many): no
     segment is made and the chains end there.  A vertex on a boundary line of a domain bounds one leaf, so open chains
     end on the boundary of a or of b;
  9. linking: a stable sort of the packed leaves and a walk.  An open chain starts at its end with the smaller vertex key;
     a closed one starts at its smallest vertex, proceeds toward that vertex's smaller neighbour and repeats the vertex at
     its end; the pieces are sorted by their first vertex key;
 10. the default depth: every line costs a three-variable walk where a lattice edge of ``contours`` costs a bisection, so
     the default is two levels below ``contours``' 4 (DESIGN.md section 23 has what was measured).

WHAT IS PROMISED: transversal vertices are as complete as ``zeros3``'s zeros, by the same walk.  Both paths, every
``_chunk``, every ``_pairs`` and two runs give the same bytes: no atomics, no waiting.
WHAT IS NOT: a piece that stays inside one product leaf is missed without a flag.  Tangential contact and coincident
regions give the bits 4 or 16 at best.  A vertex exactly on a lattice node of its own surface, or on a lattice line of
both surfaces at once, appears under two keys and ends in bit 64 (or 32).  Nothing is certified: nothing bounds the
distance of the polyline from the intersection between two vertices.

``_path="device" | "host"`` (or ``surfaces.FORCE_PATH``) pins the path; ``surfaces.LAST_PATHS`` lists what the last call
ran.
"""
import warnings

import numpy as np

from . import _backend
from . import _cells
from . import _native as nv
from . import _pairs as _search        # ``_pairs`` is a knob of trace_pair
from . import contours
from . import refinement
from . import roots
from . import roots3

# Line segments x cells of the other surface, summed over the four families, from which the device path is taken.  Read off
# the table of tools/surfaces_time.py on an MI355X: a device call is 7.2 - 10.9 ms whatever it does
# up to 3.4e7 pairs, the host path 13.0 ms at 3.5e4 pairs (8 x 8 cells, depth 1) and 204 ms at 3.4e7; on 6.4e3 pairs
# (3 x 5 against 8 x 6 cells, depth 1, single runs) the two were 16 and 14 ms.  The host's time follows the candidates
# (about 50 us each) more than the pairs; the crossover was not bracketed tighter.
DEVICE_MIN_WORK = 1 << 14
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

MIN_K, MAX_K = 2, 4
DEFAULT_DEPTH, MAX_DEPTH = 2, 6
# The chunk of the pair search.  There are few segments (about 8000 for 32 x 32 cells at depth 2, 128 workgroups of one
# wave), so the cells of Y are cut into as many chunks as bring the launch to FILL_WAVES workgroups (256 compute units x
# 4 SIMDs), but into chunks of MIN_CHUNK cells at least: a lane forms its KR points once per chunk.
FILL_WAVES = 1024
MIN_CHUNK = 16
SEARCH_BLOCK = 64
# Pairs per launch.  A pass whose pairs exceed PAIRS is halved by segments, so no emit or isolate launch serves more (one
# segment alone is never split), and nothing per pair is allocated before the count is known.  This bounds a launch, NOT
# the workspace: the per-pair arrays of every pass (25 R + 17 bytes per pair: roots R x 24, near R, the pair, count,
# status, nodes; R <= 32) are kept until the family's merge, which needs them all, and are copied once more when they
# are joined: a family with P pairs holds up to 2 (25 R + 17) P bytes, 1.7 GiB at P = 2^20 and R = 32.  Unlike ``rays``, whose
# passes are reduced to per-ray results, the pairs are the result here.
PAIRS = 1 << 20
LEAF_BITS = 15
EPS = roots3.EPS
SAME = roots3.SAME
STATUS_FLAT, STATUS_ODD, STATUS_MANY = 16, 32, 64
STATUS_TEXT = dict(roots3.STATUS_TEXT)
STATUS_TEXT.update({STATUS_FLAT: "coincident (flat) pair of a line and a cell", STATUS_ODD: "a chain ends inside both domains",
                    STATUS_MANY: "more than two vertices in one product leaf"})
SCOPE = "intersect_surface: two surfaces (nInd 2, nDep 3) of orders 2 to 4"
box_of, pair_kind = _search.box_of, _search.pair_kind       # the statement's, shared with ``rays``


# ------------------------------------------------------------------------------------------ the statement
def line_owner(n, G, nc):
    """(cell, g) of lattice line n of a variable with nc cells."""
    c = min(n // G, nc - 1)
    return c, n - c * G


def line_values(breaks, G):
    """The canonical parameter values of the nc G + 1 lattice lines of one variable, float64."""
    b = [float(x) for x in breaks]
    nc = len(b) - 1
    out = []
    for n in range(nc * G + 1):
        c, g = line_owner(n, G, nc)
        x = float(g) / float(G)
        out.append(b[c] if x == 0.0 else (b[c + 1] if x == 1.0 else roots._lerp(1.0 - x, x, b[c], b[c + 1])))
    return np.array(out, np.float64)


def line_points(window, ax, x):
    """The KR Bezier points [x, y, z] of a line on one cell: window = [component][K0 rows of K1 floats]."""
    K0, K1 = len(window[0]), len(window[0][0])

    def at(col):
        return col[0] if x == 0.0 else (col[-1] if x == 1.0 else roots.value(col, x))

    if ax == 0:
        return [[at([window[d][r][i] for r in range(K0)]) for d in range(3)] for i in range(K1)]
    return [[at(window[d][i]) for d in range(3)] for i in range(K0)]


def form_pair(L, ywindow):
    """The cell of ``roots3`` of a pair: (dims, [component]) with F_ijk = L_i - Y_jk, the last index fastest."""
    K1, K2 = len(ywindow[0]), len(ywindow[0][0])
    return (len(L), K1, K2), [[L[i][d] - ywindow[d][j][k] for i in range(len(L)) for j in range(K1) for k in range(K2)] for d in range(3)]


def inbox_of(L, box):
    """False: the box of the points L and ``box`` are strictly disjoint in some component."""
    return all(not (max(p[d] for p in L) < box[2 * d] or min(p[d] for p in L) > box[2 * d + 1]) for d in range(3))


def merge_keep(found, pairs, ncrun, ncy, brun, by0, by1):
    """The keep bytes of ``ssx_merge``: found = [(zeros, near)] of pairs = [(segment, cell)], sorted."""
    where = {p: n for n, p in enumerate(pairs)}
    before = [(de, dp, dq) for de in (-1, 0, 1) for dp in (-1, 0, 1) for dq in (-1, 0, 1)][:13]
    keep = []
    for (seg, cell), (zeros, near) in zip(pairs, found):
        e, (p, q) = seg % ncrun, divmod(cell, ncy[1])
        tol = [SAME * (float(brun[e + 1]) - float(brun[e])), SAME * (float(by0[p + 1]) - float(by0[p])),
               SAME * (float(by1[q + 1]) - float(by1[q]))]
        row = []
        for z, close in zip(zeros, near):
            k = 1
            if close:
                for de, dp, dq in before:
                    ne, np_, nq = e + de, p + dp, q + dq
                    if min(ne, np_, nq) < 0 or ne >= ncrun or np_ >= ncy[0] or nq >= ncy[1]:
                        continue
                    other = where.get((seg + de, np_ * ncy[1] + nq))
                    if other is not None and any(all(abs(o[a] - z[a]) <= tol[a] for a in range(3)) for o in found[other][0]):
                        k = 0
            row.append(k)
        keep.append(row)
    return keep


def _windows(tab):
    plan, rows = tab.plan, tab.rows
    (K0, K1), (nc0, nc1), (f0, f1) = plan.order, plan.ncells, plan.first
    return [[[[float(x) for x in rows[d, f0[i] + r, f1[j]:f1[j] + K1]] for r in range(K0)] for d in range(3)]
            for i in range(nc0) for j in range(nc1)]


def statement_family(X, Y, ax, depth, scale, prefilter=True, walk=None):
    """What the host drivers and the kernels compute for one family (the lines of X with variable ax fixed, against Y),
    from the functions above: a dict of pair_seg, pair_cell, roots (npairs, R, 3; NaN padded), near, count, status, nodes
    and keep.  X, Y: ``Tables`` of NumPy arrays."""
    G = 1 << depth
    ncx, ncy = X.plan.ncells, Y.plan.ncells
    KR = X.plan.order[1 - ax]
    R = roots3.slots(KR, *Y.plan.order)
    ncrun, ncfix = ncx[1 - ax], ncx[ax]
    wx, wy = _windows(X), _windows(Y)
    boxes = [box_of(w) for w in wy]
    brun, (by0, by1) = X.plan.breaks[1 - ax], Y.plan.breaks
    S = [float(s) for s in scale]
    pairs, found, status, nodes = [], [], [], []
    for seg in range((ncfix * G + 1) * ncrun):
        n, e = divmod(seg, ncrun)
        c, g = line_owner(n, G, ncfix)
        i, j = (c, e) if ax == 0 else (e, c)
        L = line_points(wx[i * ncx[1] + j], ax, float(g) / float(G))
        for cell in range(ncy[0] * ncy[1]):
            inbox = inbox_of(L, boxes[cell])
            if prefilter and not inbox:
                continue
            formed = form_pair(L, wy[cell])
            kind = pair_kind(formed, S, inbox)
            if kind == 0:
                continue
            p, q = divmod(cell, ncy[1])
            zeros, close, st, visited = [], [], STATUS_FLAT, 0
            if kind == 1:
                zeros, close, st, visited = roots3.isolate_cell(formed, [float(brun[e]), float(by0[p]), float(by1[q])],
                                                                [float(brun[e + 1]), float(by0[p + 1]), float(by1[q + 1])], S, walk)
            pairs.append((seg, cell))
            found.append((zeros, close))
            status.append(st)
            nodes.append(visited)
    out = np.full((len(found), R, 3), np.nan)
    near, keep = np.zeros((len(found), R), np.uint8), np.zeros((len(found), R), np.uint8)
    for m, ((zeros, close), row) in enumerate(zip(found, merge_keep(found, pairs, ncrun, ncy, brun, by0, by1))):
        out[m, :len(zeros)] = np.array(zeros).reshape(-1, 3)
        near[m, :len(zeros)] = close
        keep[m, :len(zeros)] = row
    return dict(pair_seg=np.array([p[0] for p in pairs], np.int32), pair_cell=np.array([p[1] for p in pairs], np.int32), roots=out,
                near=near, count=np.array([len(z) for z, _ in found], np.int32), status=np.array(status, np.uint8),
                nodes=np.array(nodes, np.int32), keep=keep)


# ------------------------------------------------------------------------------------------ vertices and linking (host, both paths)
def _leaf(z, cell, breaks, G):
    b = np.asarray(breaks, np.float64)
    t0 = b[cell]
    x = (z - t0) / (b[cell + 1] - t0)
    return cell * G + np.clip(np.floor(x * float(G)).astype(np.int64), 0, G - 1)


def vertices_of(families, plans, depth):
    """families: the four dicts (NumPy) of a call in the order a/u, a/v, b/s, b/t; plans: (a's, b's).  -> (vertices (n, 4)
    float64 in key order, family (n), line (n), leaves (n, 2) int64 packed, -1 where the vertex bounds one leaf alone)."""
    G = 1 << depth
    verts, fam_of, line_of, leaves = [], [], [], []
    for fam, res in enumerate(families):
        ax = fam & 1
        X, Y = (plans[0], plans[1]) if fam < 2 else (plans[1], plans[0])
        ncrun, ncfix, ncy1 = X.ncells[1 - ax], X.ncells[ax], Y.ncells[1]
        at = np.argwhere(res["keep"] != 0)                        # (pair, slot), in key order
        pair, slot = at[:, 0], at[:, 1]
        seg, cell = res["pair_seg"][pair].astype(np.int64), res["pair_cell"][pair].astype(np.int64)
        n, e = seg // ncrun, seg % ncrun
        w, s, t = (res["roots"][pair, slot, k] for k in range(3))
        fixed = line_values(X.breaks[ax], G)[n] if len(n) else np.zeros(0)
        own = [fixed, w] if ax == 0 else [w, fixed]
        run = _leaf(w, e, X.breaks[1 - ax], G)
        other = [_leaf(s, cell // ncy1, Y.breaks[0], G), _leaf(t, cell % ncy1, Y.breaks[1], G)]
        verts.append(np.stack(own + [s, t] if fam < 2 else [s, t] + own, axis=1).reshape(-1, 4))
        both = []
        for side in (n - 1, n):
            mine = [side, run] if ax == 0 else [run, side]
            four = mine + other if fam < 2 else other + mine
            packed = ((four[0] << (3 * LEAF_BITS)) | (four[1] << (2 * LEAF_BITS)) | (four[2] << LEAF_BITS) | four[3])
            both.append(np.where((side >= 0) & (side < ncfix * G), packed, -1))
        leaves.append(np.stack(both, axis=1).reshape(-1, 2))
        fam_of.append(np.full(len(n), fam, np.int64))
        line_of.append(n)
    return np.concatenate(verts), np.concatenate(fam_of), np.concatenate(line_of), np.concatenate(leaves)


def link(leaves):
    """leaves (n, 2): the packed product leaves of the vertices in key order.  -> (points, offsets, closed, findings): piece
    m is the vertices points[offsets[m]:offsets[m + 1]]; findings (k, 2) int64 = (packed leaf, bit 32 or 64), ascending."""
    nv_ = len(leaves)
    vert = np.repeat(np.arange(nv_, dtype=np.int64), 2)
    flat = np.asarray(leaves, np.int64).reshape(-1)
    vert, flat = vert[flat >= 0], flat[flat >= 0]
    order = np.argsort(flat, kind="stable")
    vert, flat = vert[order], flat[order]
    uniq, start, count = np.unique(flat, return_index=True, return_counts=True)
    findings = np.stack([uniq[count != 2], np.where(count[count != 2] == 1, STATUS_ODD, STATUS_MANY)], axis=1).reshape(-1, 2)
    adj = [[] for _ in range(nv_)]                                 # (neighbour, segment)
    for m, at in enumerate(start[count == 2].tolist()):
        a, b = int(vert[at]), int(vert[at + 1])
        adj[a].append((b, m))
        adj[b].append((a, m))
    seen = np.zeros(nv_, bool)
    pieces = []

    def walk(first, nxt, via):
        chain = [first]
        seen[first] = True
        while nxt is not None and not seen[nxt]:
            chain.append(nxt)
            seen[nxt] = True
            onward = [(v, m) for v, m in adj[nxt] if m != via]
            nxt, via = onward[0] if onward else (None, None)
        return chain, nxt

    for v in range(nv_):                                           # ascending: an open chain from its smaller end
        if len(adj[v]) == 1 and not seen[v]:
            pieces.append((v, False, walk(v, *adj[v][0])[0]))
    for v in range(nv_):                                           # ascending: a loop is met at its smallest vertex
        if len(adj[v]) == 2 and not seen[v]:
            chain, back = walk(v, *min(adj[v]))
            pieces.append((v, True, chain + [v]))
    pieces.sort(key=lambda p: p[0])
    points, offsets, closed = [], [0], []
    for _, loop, chain in pieces:
        points.extend(chain)
        offsets.append(len(points))
        closed.append(loop)
    return np.array(points, np.int64), np.array(offsets, np.int64), np.array(closed, bool), findings.astype(np.int64)


# ------------------------------------------------------------------------------------------ the launches
class Plan(_cells.JumpFreePlan):
    """``_cells.TensorPlan`` that refuses a jump: an interior knot of multiplicity >= K."""
    who, what = "intersect_surface", "curve"


def Tables(be, plan, rows, cmax):
    """One surface on a backend: ``_pairs.Tables``, logged here."""
    return _search.Tables(be, plan, rows, cmax, LAST_PATHS)


def _run(be, name, *args):
    be.call("bsk_ssx" + name, *args)
    LAST_PATHS.append(nv.lib().bsk_ssx_last_kernel().decode())


def chunk_of(nseg, ncell):
    """The cells per chunk of the pair search (the comment at FILL_WAVES says why)."""
    blocks = -(-nseg // SEARCH_BLOCK)
    want = -(-FILL_WAVES // blocks)
    return max(MIN_CHUNK, -(-ncell // want), -(-ncell // 65535))


def host_tables(spline):
    """The host path's tables of one surface: (plan, rows (3, R0, R1), cmax (3)), NumPy float64."""
    plan = Plan(spline.order, spline.knots)
    return (plan,) + _search.surface_rows(_cells.Host(), spline, plan, LAST_PATHS)


def run_family(X, Y, ax, depth, scale, chunk=None, prefilter=True, limit=None):
    """One family: the lines of X with variable ax fixed against the cells of Y.  -> a dict of the backend's arrays
    pair_seg, pair_cell, roots (npairs, R, 3), near, count, status, nodes, keep and of nseg, tested."""
    be, G = X.be, 1 << depth
    ncrun, ncfix = X.plan.ncells[1 - ax], X.plan.ncells[ax]
    nseg = (ncfix * G + 1) * ncrun
    R = roots3.slots(X.plan.order[1 - ax], *Y.plan.order)
    chunk = chunk_of(nseg, Y.ncell) if chunk is None else int(chunk)
    nchunks = _search.chunks(Y.ncell, chunk)
    limit = PAIRS if limit is None else int(limit)
    side = X.surface + Y.surface + (ax, G)
    done = []

    def count(lo, hi):
        search = side + (lo, hi - lo, chunk, int(bool(prefilter)), be.ptr(Y.boxes), be.ptr(scale))
        partial = be.empty((hi - lo, nchunks), np.int32)
        _run(be, "_count", *search, be.ptr(partial))
        return partial, search

    with be:
        for _, _, search, offset, npairs in _search.passes(be, 0, nseg, nseg, limit, count):     # a pass without a pair is dropped
            res = dict(pair_seg=be.empty(npairs, np.int32), pair_cell=be.empty(npairs, np.int32))
            _run(be, "_emit", *search, be.ptr(offset), be.ptr(res["pair_seg"]), be.ptr(res["pair_cell"]), npairs)
            res.update(_search.isolate_outputs(be, npairs, R, 3))
            _run(be, "_isolate", *side, be.ptr(X.breaks[1 - ax]), be.ptr(Y.breaks[0]), be.ptr(Y.breaks[1]), be.ptr(scale),
                 be.ptr(res["pair_seg"]), be.ptr(res["pair_cell"]), npairs, be.ptr(res["roots"]), be.ptr(res["near"]), be.ptr(res["count"]),
                 be.ptr(res["status"]), be.ptr(res["nodes"]))
            done.append(res)
        if not done:
            done.append(dict(pair_seg=be.empty(0, np.int32), pair_cell=be.empty(0, np.int32), **_search.isolate_outputs(be, 0, R, 3)))
        out = {key: be.cat([res[key] for res in done]) for key in done[0]}
        out["keep"] = be.cast(~be.isnan(out["roots"][:, :, 0]), np.uint8)
        which = be.nonzero(out["near"])
        if len(which):
            key = be.cast(out["pair_seg"], np.int64) * Y.ncell + be.cast(out["pair_cell"], np.int64)
            _run(be, "_merge", R, be.ptr(out["roots"]), ncrun, *Y.plan.ncells, be.ptr(X.breaks[1 - ax]), be.ptr(Y.breaks[0]),
                 be.ptr(Y.breaks[1]), be.ptr(key), len(key), be.ptr(which), len(which), be.ptr(out["keep"]))
    out.update(nseg=nseg, tested=nseg * Y.ncell)
    return out


# ------------------------------------------------------------------------------------------ public
class Status:
    """The status of a ``trace_pair`` call: ``segments`` (uint8, one byte per line segment, the four families one behind the
    other, family f at offsets[f]:offsets[f + 1]): the OR of the bytes of the segment's pairs (1 zeros not isolated, 2 more
    zeros than slots, 4 tangential or singular zero, 16 coincident pair); ``leaves`` (k, 2) int64: (packed product leaf,
    32 one vertex | 64 three or more); ``bits``: the OR of everything."""

    def __init__(self, segments, offsets, leaves):
        self.segments, self.offsets, self.leaves = segments, offsets, leaves
        self.bits = int(np.bitwise_or.reduce(segments, initial=0)) | int(np.bitwise_or.reduce(leaves[:, 1], initial=0))


def _check_spline(spline):
    if getattr(spline, "nInd", None) != 2 or spline.nDep != 3 or min(spline.order) < MIN_K or max(spline.order) > MAX_K:
        raise NotImplementedError(SCOPE)


def depth_of(tolerance, plans):
    """The depth that ``tolerance`` asks for: ``contours``' rule on each surface, the larger of the two, at most MAX_DEPTH."""
    if tolerance is None:
        return DEFAULT_DEPTH
    return min(MAX_DEPTH, max(contours.depth_of(tolerance, plan) for plan in plans))


def trace_pair(a, b, depth=None, _path=None, _chunk=None, _pairs=None, _prefilter=True):
    """The intersection of two surfaces marched on their lattices of 2^depth lines per knot cell and variable (depth
    0 .. 6, default 2).  Returns (vertices, offsets, closed, status, info): piece m is vertices[offsets[m]:offsets[m + 1]],
    rows (u, v, s, t) in float64 with a(u, v) = b(s, t) up to the error bar of ``zeros3``; closed[m] says that it is a loop
    (its first vertex is repeated at the end); the pieces are ordered by the key of their first vertex.  ``status``: a
    ``Status``; ``info``: a dict of tested (pairs of a line segment and a cell), candidates (the pairs that were emitted),
    nodes (visited by the walks), vertices (before linking) and families (the four dicts of per-pair arrays, NumPy).
    ``_chunk`` (cells per chunk of the pair search), ``_pairs`` (pairs per pass) and ``_prefilter=False`` are knobs of the
    tests: they change no result byte.  The module docstring says what is promised and what is not."""
    del LAST_PATHS[:]
    path = _cells.pick_path(_path, FORCE_PATH)
    _check_spline(a)
    _check_spline(b)
    depth = DEFAULT_DEPTH if depth is None else int(depth)
    if not 0 <= depth <= MAX_DEPTH:
        raise ValueError(f"depth must be in 0 .. {MAX_DEPTH}")
    if (_chunk is not None and int(_chunk) < 1) or (_pairs is not None and int(_pairs) < 1):
        raise ValueError("_chunk and _pairs must be >= 1")
    plans = (Plan(a.order, a.knots), Plan(b.order, b.knots))
    G = 1 << depth
    for plan in plans:
        if max(plan.ncells) * G > 1 << LEAF_BITS:
            raise ValueError(f"intersect_surface: more than {1 << LEAF_BITS} leaves along one variable (cells x 2^depth; a leaf "
                             f"index takes {LEAF_BITS} bits of a packed product leaf)")
    work = sum((p.ncells[ax] * G + 1) * p.ncells[1 - ax] * q.ncells[0] * q.ncells[1]
               for p, q in (plans, plans[::-1]) for ax in range(2))
    covered = all(refinement.steps_covered(plan.steps) for plan in plans)
    path = _backend.choose(path, covered, work >= DEVICE_MIN_WORK, "the device path covers the band steps of orders the band kernels take")

    be = _cells.Device.current() if path == "device" else _cells.Host()
    tabs = [Tables(be, plan, *_search.surface_rows(be, spline, plan, LAST_PATHS)) for spline, plan in zip((a, b), plans)]
    scale = be.put(tabs[0].cmax + tabs[1].cmax, np.float64)

    families = []
    for fam in range(4):
        X, Y = (tabs[0], tabs[1]) if fam < 2 else (tabs[1], tabs[0])
        res = run_family(X, Y, fam & 1, depth, scale, _chunk, _prefilter, _pairs)
        families.append({key: (be.get(value) if key not in ("nseg", "tested") else value) for key, value in res.items()})

    verts, _, _, leaves = vertices_of(families, plans, depth)
    points, offsets, closed, findings = link(leaves)
    segments, starts = [], [0]
    for res in families:
        byte = np.zeros(res["nseg"], np.uint8)
        np.bitwise_or.at(byte, res["pair_seg"], res["status"])
        segments.append(byte)
        starts.append(starts[-1] + res["nseg"])
    info = dict(tested=sum(res["tested"] for res in families), candidates=sum(len(res["pair_seg"]) for res in families),
                nodes=int(sum(int(res["nodes"].sum()) for res in families)), vertices=verts, leaves=leaves, families=families)
    return verts[points].reshape(-1, 4), offsets, closed, Status(np.concatenate(segments), np.array(starts, np.int64), findings), info


def _evaluate(spline, u, v):
    """NumPy float64 (n, 3): the surface at (u, v) by de Boor in float64 on the host (a few hundred vertices)."""
    out = np.zeros((len(u), 3))
    coefs = np.asarray(spline.coefs, np.float64)
    basis = []
    for d, x in enumerate((u, v)):
        k, t = int(spline.order[d]), np.asarray(spline.knots[d], np.float64)
        n = len(t) - k
        span = np.clip(np.searchsorted(t, x, "right") - 1, k - 1, n - 1)
        N = np.zeros((len(x), k))
        N[:, 0] = 1.0
        for r in range(1, k):
            saved = np.zeros(len(x))
            for j in range(r):
                left, right = t[span + j + 1] - x, x - t[span + 1 - r + j]
                term = N[:, j] / (left + right)
                N[:, j] = saved + left * term
                saved = right * term
            N[:, r] = saved
        basis.append((span - k + 1, N))
    (s0, N0), (s1, N1) = basis
    for r in range(N0.shape[1]):
        for c in range(N1.shape[1]):
            out += (N0[:, r] * N1[:, c])[:, None] * coefs[:, s0 + r, s1 + c].T
    return out


def fit_pair(points, xyz, tolerance=None, closed=False):
    """One polyline (n, 4) with its points in space (n, 3) -> (curve on a, curve on b): two Spline curves (nInd 1, nDep 2)
    on [0, 1] fitted to the same normalised chord-length parameters, the chords measured in xyz (``contours.fit_chords``).
    Points that repeat their predecessor in space are dropped; ``closed``: the last coefficient is set to the first one."""
    points, xyz = np.asarray(points, np.float64), np.asarray(xyz, np.float64)
    step = np.sqrt((np.diff(xyz, axis=0) ** 2).sum(axis=1)) if len(points) > 1 else np.zeros(0)
    return tuple(contours.fit_chords(points, step, [slice(0, 2), slice(2, 4)], tolerance, closed))


def intersect_surface(self, other, depth=None, tolerance=None, **kwargs):
    """``Spline.intersect_surface``: [(curve on self, curve on other)], one pair per connected piece; one RuntimeWarning when
    a status bit is set.  ``_path="host"`` pins the trace; the fit is ``Spline.least_squares``, whose collocation runs on
    the device on either path, so a call that finds a piece needs a device (``trace_pair`` alone does not)."""
    _check_spline(self)
    _check_spline(other)
    plans = (Plan(self.order, self.knots), Plan(other.order, other.knots))
    if depth is None:
        depth = depth_of(tolerance, plans)
    if tolerance is None:
        tolerance = contours.FIT_TOLERANCE * max(float(b[-1]) - float(b[0]) for plan in plans for b in plan.breaks)
    vertices, offsets, closed, status, _ = trace_pair(self, other, depth=depth, **kwargs)
    if status.bits:
        why = ", ".join(text for bit, text in STATUS_TEXT.items() if status.bits & bit)
        warnings.warn(f"intersect_surface: {int(np.count_nonzero(status.segments))} line segments and {len(status.leaves)} product leaves "
                      f"carry a status bit (surfaces.trace_pair returns them): {why}", RuntimeWarning, stacklevel=3)
    found = []
    for m in range(len(offsets) - 1):
        points = vertices[offsets[m]:offsets[m + 1]]
        found.append(fit_pair(points, _evaluate(self, points[:, 0], points[:, 1]), tolerance, bool(closed[m])))
    return found
