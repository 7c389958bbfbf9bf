"""
Ray-surface hits: ``Spline.intersect_rays`` and ``cast_batch`` (an extension beyond the reference's API, like ``project``).
N independent lines o + t d against one surface (nInd 2, nDep 3, orders 2 to 4): where does each line hit, and which hit
comes first?  A line is the intersection of two planes, so a hit is a common zero of the two scalar fields
g_k(u, v) = n_k . (S(u, v) - o): a ``zeros2`` system per ray.  The systems are never stored: a cell's coefficients of g_k
are formed from the surface's window and the ray wherever they are needed, almost every pair (ray, cell) is discarded by a
box test, and the few that remain are walked by the ``roots2`` walk, unchanged.

    device path   ``bsk_band_apply`` per axis with the rows on the device, ``bsk_rays_boxes``, then per pass of at most
                  PASS rays ``bsk_rays_count``, ``torch.cumsum``, ``bsk_rays_emit``, ``bsk_rays_isolate``,
                  ``bsk_rays_reduce`` (twice for hits="all"); no ray of a pass has a candidate: the launches behind
                  ``bsk_rays_count`` are skipped; no hit in range: the second reduce is
    host path     ``bsk_roots_extract_host`` per axis, then the ``*_host`` twins of the same entry points: the same functions
                  of bsk_rays.hpp on the CPU, for few rays

THE STATEMENT (``frame``, ``form_cell``, ``slab_test``, ``pair_kind``, ``reduce_ray`` and ``roots2.isolate_cell`` say it in
plain Python floats, bit for bit what bsk_rays.hpp computes; float64 whatever the dtypes, float32 is widened first, no
contraction, every product and sum rounded on its own; eps of float64):
  * extraction: every variable goes to Bezier form with the band operators of ``_cells.TensorPlan``; cell (i, j), flat
    index i nc1 + j, is the K0 x K1 window of the three components at first0[i], first1[j] of the rows (3, R0, R1);
  * skipped rays: a non-finite entry of o or d, or d = 0, sets status bit 8; the ray has no pairs and gives NaN;
  * frame: c is the axis of the largest |d_c|, the highest index on ties, so that a < b, the other two, are the axes of the
    two smallest with the lowest index on ties.  n_1 = e_a x d and n_2 = e_b x d: one entry of each is 0, the others are
    +- entries of d, so both planes hold the line exactly and no rounding enters the frame.  For a control point P,
    g_k = w_k0 (P_p - o_p) + w_k1 (P_q - o_q), p < q the axes where n_k is not 0: two differences, two products, one sum.
    Coefficients and origins x 2^k and directions x 2^m give g_k x 2^(k + m), bit for bit;
  * scale: S_k = |w_k0| (C_p + |o_p|) + |w_k1| (C_q + |o_q|), C_m = max |coefficient| of component m (of the widened
    coefficients, before the extraction).  It bounds |g_k| on the whole surface, costs nothing per pair and is a function of
    the ray alone; it takes the place of ``roots2``'s S_d in the tangent threshold and in the zero-cell rule;
  * box test: boxes[cell] = min and max of the window per component, exact.  A true hit X = o + t* d lies in the convex
    hull of the window, so t* lies in the slab [(lo_m - o_m) / d_m, (hi_m - o_m) / d_m] of every axis with d_m != 0 and o_m
    lies in [lo_m, hi_m] on every axis with d_m = 0.  The kernel computes a slab end as (lo_m - o_m) (1 / d_m): a difference,
    a reciprocal and a product, three roundings, relative error below 2 eps; each end is pushed outward by 4 eps |t| +
    2^-1070 (the absolute term covers a product that went subnormal), and an end that is NaN (0 x inf, inf - inf) becomes
    -inf or +inf.  The pair is dropped only when o_m is outside [lo_m, hi_m] for an axis with d_m = 0 (an exact comparison)
    or when max(tmin, the slab entries) > min(tmax, the slab exits), so it is kept for every hit whose exact t* lies in
    [tmin, tmax]: the test is sound for d_m = 0 and for infinite tmin and tmax;
  * candidates: a pair that passes the box test is FLAT when all K0 K1 values of g_1, or all of g_2, are below S_k eps in
    magnitude, or S_k is 0 (the ray lies in the plane of a flat cell): it sets status bit 16 of the ray and reports nothing.  Any other
    pair is a candidate unless g_1 or g_2 is strictly of one sign (``roots2.excluded``).  ``_prefilter=False`` sends every
    pair to the sign test and keeps the box test for the flat rule alone: the hits, their cells and count are the same,
    since a dropped pair holds no hit in range; the status differs only by the bits 1, 2, 4 of dropped pairs whose zeros
    all lie outside [tmin, tmax];
  * walk and leaf: ``roots2.isolate_cell`` on the formed coefficients with (S_1, S_2): DEPTH, the Newton rule, the slots
    R = 2 (K0 - 1)(K1 - 1), WALK, the status bits 1, 2, 4.  Where ``roots2`` reads the cell's own coefficients again, they
    are formed again;
  * merge: ``roots2_merge``'s rule among the ray's own pairs: a zero within 2^-20 of an edge of its unit cell is dropped
    when a pair of the ray on (i - 1, j - 1), (i - 1, j), (i - 1, j + 1) or (i, j - 1) holds one within 2^-20 h on both axes;
  * parameter: t = (S_c(x) - o_c) / d_c, one IEEE division, S_c by ``roots2.eval2`` on the window of component c at the
    cell-local x = ((u - t0u) / hu, (v - t0v) / hv) recovered from the stored zero; a hit has tmin <= t <= tmax in float64;
  * first: the kept hit in range of smallest t, ties to the lowest cell, then the lowest slot; count: the hits in range;
    status: the OR of the pairs' bytes and of bit 8.  hits="all": every hit, a ray's sorted by (t, cell).
uv is rounded once to the knots' dtype at the end.  No atomics, no waiting: two runs, both paths, every ``_chunk`` and every
``_pass`` give the same bytes.

WHAT IS PROMISED: the hits inside a cell are as complete as ``zeros2``'s zeros, by the same walk: every transversal hit is
found.  WHAT IS NOT: a grazing hit (the ray tangent to the surface) may be missed silently.  Status bit 4 is ``roots2``'s
rule, an unconverged leaf whose centre values of BOTH fields are within 4 (K0 + K1) eps S_k; at a tangency only the field
of the tangent plane is that small, so the bit is set only when the other parameter of the hit happens to sit at a leaf
centre.  A generic grazing ray reports no hit and no bit (the recorded cases pin both).  Nothing is promised for a ray whose
origin lies on the surface within the error bar around tmin: the hit may or may not count as in
range.  An early exit for ``first`` that orders the cells by entry t, and a hierarchy over the boxes, are not built: every
ray tests every box.

``_path="device" | "host"`` (or ``rays.FORCE_PATH``) pins the path; ``rays.LAST_PATHS`` lists what the last call ran.
"""
import warnings

import numpy as np

from . import _backend
from . import _cells
from . import _native as nv
from . import _pairs as _search        # ``_pairs`` is a knob of cast_batch
from . import refinement
from . import roots2

# Rays x cells from which the device path is taken.  Read off the table of tools/rays_time.py --quick on an MI355X (DESIGN.md
# section 22): the host path takes about 19 - 42 ns per (ray, cell), a device call 2.8 - 3.4 ms whatever it does below 10^7
# pairs (host 10.8 ms against device 2.8 ms at 2.6e5, host 77 ms against 2.9 ms at 4.1e6), so the paths cross near 10^5.  The
# crossover itself was not bracketed tighter.
DEVICE_MIN_WORK = 1 << 17
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

MIN_K, MAX_K = 2, 4
CHUNK = 512                # cells per chunk of the pair search
# Rays per pass and pairs per pass.  A pass holds 20 nchunks + 30 bytes per ray (partial int32, its running sums and the
# offsets int64, all alive together; then the results) and 17 R + 17 bytes per pair (roots R x 16, near R, the pair, count,
# status, nodes), R <= 18: 2^18 rays on 4096 cells (8 chunks) and 2^21 pairs are under 50 MiB + 0.7 GiB.  A pass whose
# pairs exceed PAIRS is halved: its count launch, whose per-ray part is already counted above, is repeated on the halves,
# and nothing per pair is allocated before the count is known.  One ray alone is never split.
PASS = 1 << 18
PAIRS = 1 << 21
EPS = roots2.EPS
TINY = 2.0 ** -1070
SAME = roots2.SAME
STATUS_SKIPPED, STATUS_FLAT = 8, 16
WARN_BITS = roots2.STATUS_WALK | roots2.STATUS_SLOTS | roots2.STATUS_TANGENT | STATUS_SKIPPED | STATUS_FLAT
STATUS_TEXT = dict(roots2.STATUS_TEXT)
STATUS_TEXT.update({STATUS_SKIPPED: "ray not finite or without direction", STATUS_FLAT: "ray in the plane of a flat cell"})
SCOPE = "intersect_rays: surfaces (nInd 2, nDep 3) of orders 2 to 4"
INF = float("inf")
NAN = float("nan")
box_of, pair_kind = _search.box_of, _search.pair_kind       # the statement's, shared with ``surfaces``


# ------------------------------------------------------------------------------------------ the statement
class RayFrame:
    """The frame of one ray in Python floats: o, d, the dominant axis c, the two terms (p, q, w0, w1) of g_1 and g_2, the
    scales S and ``skipped``."""

    def __init__(self, o, d, C):
        self.o, self.d = [float(x) for x in o], [float(x) for x in d]
        a = [abs(x) for x in self.d]
        ok = all(x - x == 0.0 for x in self.o + self.d)
        self.skipped = not ok or (a[0] == 0.0 and a[1] == 0.0 and a[2] == 0.0)
        self.c = 2 if (a[2] >= a[0] and a[2] >= a[1]) else (1 if a[1] >= a[0] else 0)
        dx, dy, dz = self.d
        # e_x x d = (0, -dz, dy), e_y x d = (dz, 0, -dx), e_z x d = (-dy, dx, 0)
        if self.c == 2:
            self.terms = [(1, 2, -dz, dy), (0, 2, dz, -dx)]
        elif self.c == 1:
            self.terms = [(1, 2, -dz, dy), (0, 1, -dy, dx)]
        else:
            self.terms = [(0, 2, dz, -dx), (0, 1, -dy, dx)]
        cc = [float(C[m]) + abs(self.o[m]) for m in range(3)]
        self.S = [abs(w0) * cc[p] + abs(w1) * cc[q] for p, q, w0, w1 in self.terms]


def frame(o, d, C):
    return RayFrame(o, d, C)


def form_cell(window, fr):
    """The cell ((K0, K1), [g_1, g_2]) of ``roots2`` from the window [x, y, z] (each K0 rows of K1 floats) and the ray's frame."""
    K0, K1 = len(window[0]), len(window[0][0])
    return (K0, K1), [[w0 * (window[p][i][j] - fr.o[p]) + w1 * (window[q][i][j] - fr.o[q]) for i in range(K0) for j in range(K1)]
                      for p, q, w0, w1 in fr.terms]


def slab_test(fr, box, tmin, tmax):
    """False: the line on [tmin, tmax] misses the box."""
    enter, leave, hit = tmin, tmax, True
    for m in range(3):
        lo, hi = box[2 * m], box[2 * m + 1]
        if fr.d[m] == 0.0:
            hit = hit and not (fr.o[m] < lo or fr.o[m] > hi)
            continue
        inv = 1.0 / fr.d[m]
        ta, tb = (lo - fr.o[m]) * inv, (hi - fr.o[m]) * inv
        near, far = (ta, tb) if inv > 0.0 else (tb, ta)
        near = near - (4.0 * EPS * abs(near) + TINY)
        far = far + (4.0 * EPS * abs(far) + TINY)
        if near != near:
            near = -INF
        if far != far:
            far = INF
        enter = near if near > enter else enter
        leave = far if far < leave else leave
    return hit and not enter > leave


def reduce_ray(fr, pairs, windows, breaks0, breaks1, nc1, tmin, tmax):
    """The hits of one ray: pairs = [(cell, zeros, near)] in cell order, windows[cell] = its window.
    -> [(u, v, t, cell)] in (cell, slot) order: what ``ray_reduce`` keeps."""
    hits = []
    for n, (cell, zeros, near) in enumerate(pairs):
        i, j = divmod(cell, nc1)
        t0u, t0v = float(breaks0[i]), float(breaks1[j])
        hu, hv = float(breaks0[i + 1]) - t0u, float(breaks1[j + 1]) - t0v
        tolu, tolv = SAME * hu, SAME * hv
        for (u, v), close in zip(zeros, near):
            keep = True
            if close:
                for other, others, _ in pairs[:n]:
                    oi, oj = divmod(other, nc1)
                    if (oi == i - 1 and oj in (j - 1, j, j + 1)) or (oi == i and oj == j - 1):
                        if any(abs(uu - u) <= tolu and abs(vv - v) <= tolv for uu, vv in others):
                            keep = False
            if not keep:
                continue
            comp = windows[cell][fr.c]
            value = roots2.eval2((len(comp), len(comp[0])), [x for row in comp for x in row], (u - t0u) / hu, (v - t0v) / hv)[0]
            t = (value - fr.o[fr.c]) / fr.d[fr.c]
            if t >= tmin and t <= tmax:
                hits.append((u, v, t, cell))
    return hits


def first_of(hits):
    """(u, v, t, cell) of the hit of smallest t, the first one on ties; (NaN, NaN, NaN, -1) without hits."""
    best = (NAN, NAN, NAN, -1)
    for n, hit in enumerate(hits):
        if n == 0 or hit[2] < best[2]:
            best = hit
    return best


def statement(rows, plan, cmax, origins, directions, tmin=0.0, tmax=INF, prefilter=True, walk=None):
    """What the host drivers and the kernels compute for the extracted rows (3, R0, R1), from the functions above: a dict of
    pair_ray, pair_cell, roots (npairs, R, 2; NaN padded), near, count, status, nodes per pair, of uv (2, N), t, cell, hits,
    rstatus per ray (``first``) and of all = [(u, v, t, cell)] per ray sorted by (t, cell)."""
    K0, K1 = plan.order
    R = roots2.slots(K0, K1)
    nc0, nc1 = plan.ncells
    f0, f1 = plan.first
    N = origins.shape[1]
    windows = [[[[float(x) for x in rows[m, f0[i] + r, f1[j]:f1[j] + K1]] for r in range(K0)] for m in range(3)]
               for i in range(nc0) for j in range(nc1)]
    boxes = [box_of(w) for w in windows]
    pair_ray, pair_cell, found, status, nodes = [], [], [], [], []
    uv, t, cell = np.full((2, N), np.nan), np.full(N, np.nan), np.full(N, -1, np.int32)
    hits, rstatus, every = np.zeros(N, np.int32), np.zeros(N, np.uint8), []
    for ray in range(N):
        fr = frame(origins[:, ray], directions[:, ray], cmax)
        mine = []
        bits = STATUS_SKIPPED if fr.skipped else 0
        for at in range(nc0 * nc1 if not fr.skipped else 0):
            inbox = slab_test(fr, boxes[at], tmin, tmax)
            if prefilter and not inbox:
                continue
            formed = form_cell(windows[at], fr)
            kind = pair_kind(formed, fr.S, inbox)
            if kind == 0:
                continue
            i, j = divmod(at, nc1)
            zeros, close, st, visited = [], [], STATUS_FLAT, 0
            if kind == 1:
                zeros, close, st, visited = roots2.isolate_cell(formed, [float(plan.breaks[0][i]), float(plan.breaks[1][j])],
                                                                [float(plan.breaks[0][i + 1]), float(plan.breaks[1][j + 1])], fr.S, walk)
            pair_ray.append(ray)
            pair_cell.append(at)
            found.append((zeros, close))
            status.append(st)
            nodes.append(visited)
            mine.append((at, zeros, close))
            bits |= st
        got = reduce_ray(fr, mine, windows, plan.breaks[0], plan.breaks[1], nc1, tmin, tmax)
        uv[0, ray], uv[1, ray], t[ray], cell[ray] = first_of(got)
        hits[ray], rstatus[ray] = len(got), bits
        every.append(sorted(got, key=lambda h: (h[2], h[3])))
    roots = np.full((len(found), R, 2), np.nan)
    near = np.zeros((len(found), R), np.uint8)
    for n, (zeros, close) in enumerate(found):
        roots[n, :len(zeros)] = np.array(zeros).reshape(-1, 2)
        near[n, :len(zeros)] = close
    return dict(pair_ray=np.array(pair_ray, np.int32), pair_cell=np.array(pair_cell, np.int32), roots=roots, near=near,
                count=np.array([len(z) for z, _ in found], np.int32), status=np.array(status, np.uint8),
                nodes=np.array(nodes, np.int32), uv=uv, t=t, cell=cell, hits=hits, rstatus=rstatus, all=every)


# ------------------------------------------------------------------------------------------ the launches
Plan = _cells.TensorPlan


def Tables(be, plan, rows, cmax):
    """What every pass of a call shares: ``_pairs.Tables`` and ``dcmax``, cmax as the backend's array (the frames read it)."""
    tab = _search.Tables(be, plan, rows, cmax, LAST_PATHS)
    with be:
        tab.dcmax = be.put(tab.cmax, np.float64)
    return tab


def _run(be, name, *args):
    be.call("bsk_rays" + name, *args)
    LAST_PATHS.append(nv.lib().bsk_rays_last_kernel().decode())


def _finish(tab, out, search, origins, directions, tmin, tmax, every, offset, npairs):
    """What follows the count of a pass of ``npairs`` pairs: emit, isolate, reduce (twice for ``every``); fills ``out``."""
    be, n = tab.be, int(origins.shape[1])
    rays = search[len(tab.surface):len(tab.surface) + 4]
    R = roots2.slots(tab.K0, tab.K1)
    out["npairs"] = npairs
    out["uv"], out["t"] = be.empty((2, n), np.float64), be.empty(n, np.float64)
    out["cell"], out["hits"], out["rstatus"] = be.empty(n, np.int32), be.zeros(n, np.int32), out["skipped"]
    out["all_off"] = be.zeros(n + 1, np.int64)
    out["all_uv"], out["all_t"], out["all_cell"] = be.empty((0, 2), np.float64), be.empty(0, np.float64), be.empty(0, np.int32)
    if npairs == 0:                                       # no ray has a candidate: nothing to emit, walk or reduce
        out["uv"][...] = NAN
        out["t"][...] = NAN
        out["cell"][...] = -1
        return out
    pstart = be.empty(n + 1, np.int64)
    pstart[:n] = offset.reshape(n, -1)[:, 0]
    pstart[n] = npairs
    out["pair_ray"], out["pair_cell"] = be.empty(npairs, np.int32), be.empty(npairs, np.int32)
    _run(be, "_emit", *search, be.ptr(offset), be.ptr(out["pair_ray"]), be.ptr(out["pair_cell"]), npairs)
    out.update(_search.isolate_outputs(be, npairs, R, 2), rstatus=be.empty(n, np.uint8))
    head = tab.surface + tuple(be.ptr(b) for b in tab.breaks) + rays
    _run(be, "_isolate", *head, be.ptr(out["pair_ray"]), be.ptr(out["pair_cell"]), npairs, be.ptr(out["roots"]), be.ptr(out["near"]),
         be.ptr(out["count"]), be.ptr(out["status"]), be.ptr(out["nodes"]))
    reduce = head + (tmin, tmax, be.ptr(pstart), be.ptr(out["pair_cell"]), npairs, be.ptr(out["roots"]), be.ptr(out["near"]),
                     be.ptr(out["count"]), be.ptr(out["status"]), be.ptr(out["skipped"]))
    _run(be, "_reduce", *reduce, 0, None, 0, be.ptr(out["uv"]), be.ptr(out["t"]), be.ptr(out["cell"]), be.ptr(out["hits"]),
         be.ptr(out["rstatus"]))
    if every:
        stops = be.cumsum(out["hits"])
        out["all_off"][1:] = stops
        nhits = int(stops[-1])
        if nhits:
            out["all_uv"], out["all_t"] = be.empty((nhits, 2), np.float64), be.empty(nhits, np.float64)
            out["all_cell"] = be.empty(nhits, np.int32)
            _run(be, "_reduce", *reduce, 1, be.ptr(out["all_off"]), nhits, be.ptr(out["all_uv"]), be.ptr(out["all_t"]),
                 be.ptr(out["all_cell"]), None, None)
    return out


def _passes(tab, origins, directions, tmin, tmax, chunk, rays_per_pass, prefilter, every, limit):
    """The rays of origins, directions (3, N), the backend's float64 arrays, in passes of at most ``rays_per_pass`` rays and
    ``limit`` pairs (``_pairs.passes``) -> [(lo, hi, the pass's dict)].  A pass without a pair is kept: its rays are filled."""
    be, nchunks = tab.be, _search.chunks(tab.ncell, chunk)

    def count(lo, hi):                                    # -> partial and what ``_finish`` takes; o, d live as long as the pass
        o, d = origins[:, lo:hi], directions[:, lo:hi]
        o, d = (np.ascontiguousarray(o), np.ascontiguousarray(d)) if be.__class__ is _cells.Host else (o.contiguous(), d.contiguous())
        search = tab.surface + (be.ptr(tab.dcmax), be.ptr(o), be.ptr(d), hi - lo, tmin, tmax, chunk, int(bool(prefilter)), be.ptr(tab.boxes))
        out = dict(partial=be.empty((hi - lo, nchunks), np.int32), skipped=be.empty(hi - lo, np.uint8))
        _run(be, "_count", *search, be.ptr(out["partial"]), be.ptr(out["skipped"]))
        return out["partial"], (out, search, o, d)

    with be:
        return [(lo, hi, _finish(tab, *back, tmin, tmax, every, offset, npairs))
                for lo, hi, back, offset, npairs in _search.passes(be, 0, int(origins.shape[1]), rays_per_pass, limit, count, empty=True)]


def run_pass(tab, origins, directions, tmin, tmax, chunk=CHUNK, prefilter=True, every=False):
    """One pass, whatever its pairs: origins, directions (3, n), the backend's contiguous float64 arrays.  -> a dict of the
    backend's arrays: partial, skipped, npairs and, unless npairs is 0, pair_ray, pair_cell, roots, near, count, status,
    nodes per pair, uv (2, n), t, cell, hits, rstatus per ray; every: also all_uv (M, 2), all_t, all_cell, all_off (n + 1)
    in (ray, cell, slot) order."""
    return _passes(tab, origins, directions, tmin, tmax, chunk, int(origins.shape[1]), prefilter, every, None)[0][2]


# ------------------------------------------------------------------------------------------ public
def _check_spline(spline):
    if spline.nInd != 2 or spline.nDep != 3 or min(spline.order) < MIN_K or max(spline.order) > MAX_K:
        raise NotImplementedError(SCOPE)


def _rays_arg(a, name, on_device):
    kinds = "float32 or float64, NumPy or a torch CUDA tensor"
    if _cells.is_torch(a) != on_device:
        raise TypeError("origins and directions must be of the same kind (NumPy, or torch CUDA tensors)")
    if on_device:
        import torch
        if not a.is_cuda or a.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"intersect_rays takes the {name} as {kinds}")
        return a
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise TypeError(f"intersect_rays takes the {name} as {kinds}")
    return a


def host_tables(spline):
    """The host path's tables: (plan, rows (3, R0, R1), cmax (3)), NumPy float64."""
    plan = Plan(spline.order, spline.knots)
    return (plan,) + _search.surface_rows(_cells.Host(), spline, plan, LAST_PATHS)


def cast_batch(spline, origins, directions, tmin=0.0, tmax=INF, hits="first", _path=None, _chunk=None, _pass=None, _prefilter=True,
               _pairs=None):
    """The hits of N rays o + t d, tmin <= t <= tmax, on a surface.  ``origins``, ``directions``: (3, N), NumPy float32 /
    float64 or torch CUDA tensors of those types; directions need not be normalised.
    hits="first": (uv (2, N) in the knots' dtype, t (N) float64, cell (N) int32, count (N) int32, status (N) uint8) of the
    hit of smallest t; NaN and cell -1 without a hit; count: the hits in range.
    hits="all": (uv (2, M), t (M), offsets (N + 1) int64, status (N)): the hits of ray r are offsets[r]:offsets[r + 1],
    sorted by (t, cell).
    status bits: 1 zeros not isolated, 2 more zeros than slots, 4 tangential (grazing) or singular hit, not reported, 8 ray
    not finite or d = 0, 16 ray in the plane of a flat cell.  CUDA in gives CUDA out; nothing but two counts per pass leaves
    the device.  ``_chunk`` (cells per chunk of the pair search), ``_pass`` (rays per pass), ``_pairs`` (pairs per pass) and
    ``_prefilter=False`` are knobs of the tests: they change no result byte (the module docstring has the one exception)."""
    del LAST_PATHS[:]
    path = _cells.pick_path(_path, FORCE_PATH)
    _check_spline(spline)
    if hits not in ("first", "all"):
        raise ValueError("hits must be 'first' or 'all'")
    on_device = _cells.is_torch(origins)
    origins, directions = _rays_arg(origins, "origins", on_device), _rays_arg(directions, "directions", on_device)
    if origins.ndim != 2 or origins.shape[0] != 3 or tuple(directions.shape) != tuple(origins.shape):
        raise ValueError("origins and directions must both have the shape (3, N)")
    tmin, tmax = float(tmin), float(tmax)
    if tmin != tmin or tmax != tmax:
        raise ValueError("tmin and tmax must not be NaN")
    chunk = CHUNK if _chunk is None else int(_chunk)
    per_pass = PASS if _pass is None else int(_pass)
    limit = PAIRS if _pairs is None else int(_pairs)
    if chunk < 1 or per_pass < 1 or limit < 1:
        raise ValueError("_chunk, _pass and _pairs must be >= 1")
    if on_device:
        if path == "host":
            raise ValueError("rays on the device take the device path")
        path = "device"
    N = int(origins.shape[1])
    plan = Plan(spline.order, spline.knots)
    nc0, nc1 = plan.ncells
    _search.chunks(nc0 * nc1, chunk)
    kdtype = np.result_type(spline.knots[0].dtype, spline.knots[1].dtype)
    path = _backend.choose(path, refinement.steps_covered(plan.steps), N * nc0 * nc1 >= DEVICE_MIN_WORK,
                         "the device path covers the band steps of orders the band kernels take")
    every = hits == "all"

    if path == "device":
        import torch
        o = (origins if on_device else torch.from_numpy(np.ascontiguousarray(origins)).cuda()).double().contiguous()
        dev = o.device
        d = (directions if on_device else torch.from_numpy(np.ascontiguousarray(directions))).to(dev).double().contiguous()
        be = _cells.Device(dev)
    else:
        be = _cells.Host()
        o, d = origins.astype(np.float64), directions.astype(np.float64)
    rows, cmax = _search.surface_rows(be, spline, plan, LAST_PATHS)

    def finish(*arrays):
        return arrays if on_device or path == "host" else tuple(be.get(a) for a in arrays)

    if N == 0:
        empty = (be.empty((2, 0), kdtype), be.empty(0, np.float64))
        if every:
            return finish(*empty, be.zeros(1, np.int64), be.empty(0, np.uint8))
        return finish(*empty, be.empty(0, np.int32), be.empty(0, np.int32), be.empty(0, np.uint8))

    tab = Tables(be, plan, rows, cmax)
    done = _passes(tab, o, d, tmin, tmax, chunk, per_pass, _prefilter, every, limit)
    status = be.cat([res["rstatus"] for _, _, res in done])
    if not every:
        uv = be.cat([res["uv"].T for _, _, res in done]).T
        first = [be.cat([res[key] for _, _, res in done]) for key in ("t", "cell", "hits")]
        return finish(be.cast(uv, kdtype), *first, status)
    uv = be.cat([res["all_uv"] for _, _, res in done])
    t = be.cat([res["all_t"] for _, _, res in done])
    cell = be.cat([res["all_cell"] for _, _, res in done])
    count = be.cat([res["all_off"][1:] - res["all_off"][:-1] for _, _, res in done])
    offsets = be.zeros(N + 1, np.int64)
    offsets[1:] = be.cumsum(count)
    order = be.lexsort([cell, t, be.repeat(be.arange(N), count)])          # a ray's hits by (t, cell); the sort is stable
    return finish(be.cast(uv[order].T, kdtype), t[order], offsets, status)


def intersect_rays(self, origins, directions, tmin=0.0, tmax=INF, **kwargs):
    """``Spline.intersect_rays``: (uv, t); one RuntimeWarning when a ray carries a warn bit."""
    _check_spline(self)
    on_device = _cells.is_torch(origins)
    origins, directions = _rays_arg(origins, "origins", on_device), _rays_arg(directions, "directions", on_device)
    if origins.ndim < 1 or origins.shape[0] != 3 or tuple(directions.shape) != tuple(origins.shape):
        raise ValueError("origins and directions must both have the shape (3, ...)")
    shape = tuple(origins.shape[1:])
    N = int(np.prod(shape, dtype=np.int64))
    uv, t, _, _, status = cast_batch(self, origins.reshape(3, N), directions.reshape(3, N), tmin, tmax, "first", **kwargs)
    flagged = (status & WARN_BITS) != 0
    count = int(flagged.sum())                                         # a status summary: the only thing that leaves the device
    if count:
        index = int(flagged.nonzero()[0][0]) if on_device else int(np.flatnonzero(flagged)[0])
        bits = int(status[index])
        why = ", ".join(text for bit, text in STATUS_TEXT.items() if bits & bit)
        warnings.warn(f"intersect_rays: {count} of {N} rays carry a status bit (rays.cast_batch returns them); the first one has "
                      f"the flat index {index}: {why}", RuntimeWarning, stacklevel=3)
    return uv.reshape((2,) + shape), t.reshape(shape)
