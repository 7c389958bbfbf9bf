"""
Closest points on curves and surfaces: ``Spline.project`` and ``project_batch`` (an extension beyond the reference's API,
like ``tessellate`` and ``zeros2_batch``).  N independent query points, each a nearest-sample search over a grid of samples
of the spline plus a few Newton steps on g(u) = |S(u) - p|^2 / 2.

    device path   ``bsk_band_apply`` per axis (Bezier extraction, then the sample grid) with the rows on the device,
                  ``bsk_project_seed`` (grid: point blocks x sample chunks), ``bsk_project_newton``
    host path     ``bsk_roots_extract_host`` per axis (the same band operators in the same order, summed as the band
                  kernels sum them), ``bsk_project_seed_host``, ``bsk_project_newton_host``: the same functions of
                  bsk_project.hpp on the CPU, for few points

WHAT IS PROMISED: the result is the local minimiser of the distance that Newton's method reaches from the nearest sample.
It is the global closest point whenever the nearest sample lies in the basin of the global minimiser; the method is NOT
certified global, unlike the ``zeros`` family.  More ``samples`` shrink the set of points for which the two differ.  At a
knot line of multiplicity >= K - 1 (a crease) convergence is not promised; status bit 1 reports it.  The seed search is
brute force: N M squared distances for N points and M samples.

THE STATEMENT (``seed_point`` and ``newton_point`` say it in plain Python floats, bit for bit what bsk_project.hpp computes;
float64 whatever the dtypes, float32 is widened first, every product and sum rounded on its own):
  * extraction: every variable goes to Bezier form with the band operators of ``roots.BezierPlan``; cell (i, j) is the
    K0 x K1 window of every component at first0[i], first1[j] of the rows (nDep, R0[, R1]);
  * sample grid: G_d samples per cell and axis at the local coordinates (a + 1/2) / G_d, by one more band step per axis:
    row s G_d + a has first = first_d[s] and as weights the Bernstein basis of degree K_d - 1 at that coordinate, formed in
    extended precision and rounded once (``sample_step``).  Samples (nDep, M0[, M1]), flat index m0 M1 + m1;
  * seed: the squared distance of a sample is r_0 r_0 + r_1 r_1 (+ r_2 r_2) in component order; a sample wins when its
    squared distance is strictly below the best so far (from +inf), so ties go to the lowest flat index.  The samples are
    cut into chunks of SEED_CHUNK; the chunk partials (d2, index) are reduced in chunk order by the same rule.  A point with
    a NaN or infinite coordinate (no sample below +inf) sets status bit 8, is not iterated and gives NaN;
  * Newton: the start is the seed's parameter, break + ((a + 1/2) / G) width per axis, or the guess, clamped to the domain.
    At most EVALS trips, each one evaluation at a trial t: the cell of t by bisection over the breaks (``find_cell``: the
    last cell whose left break is <= t), x = (t - left) / width, per component S and its first and second local derivatives
    by de Casteljau (``eval1``), then d2 = sum r r, G = J^T r, A = J^T J, B = sum r_d Hess S_d in local coordinates, summed
    in component order.  The trial is taken when it is the first one, when its step is within TRUST of the domain width on
    every axis, when d2 did not grow, or after HALVINGS halvings; otherwise the step is halved and tried again.  A taken
    trial whose step is within TRUST ends the walk converged when that step is within SMALL_STEP of the domain width or
    not smaller than the small step before it (the rule of ``roots2``).  An axis is fixed for a step when the iterate sits
    on a domain bound and the gradient points outward; all axes fixed: converged.  On the free axes the Newton step by
    Cramer's rule with IEEE division when the restricted A + B is positive definite, else the Gauss-Newton step with A,
    else status bit 4 and stop.  The local step times the cell's width is the step; the new trial is clamped to the
    domain.  The iterate moves freely across cells;
  * status: 1 the evaluation bound was reached, 2 the foot point is on a domain bound (informational), 4 singular step,
    8 not iterated.  ``distance`` = sqrt(d2) at the returned parameter, which is rounded once to the knots' dtype;
  * scale: the drivers of both paths hand the statement the (widened) coefficients and points x 2^-e, e the binary exponent
    of max |coefficient| (``norm_exponent``), and return the distances x 2^e: coefficients and points x 2^k give the same
    parameters, status and steps and the distances x 2^k, bit for bit, wherever inputs and outputs are finite.
No atomics, no waiting: two runs give the same bytes.

``_path="device" | "host"`` (or ``project.FORCE_PATH``) pins the path; ``project.LAST_PATHS`` lists what the last call ran.
"""
import math
import warnings

import numpy as np

from . import _cells
from . import _native as nv
from . import refinement

# Points x samples from which the device path is taken; a Newton solve counts as NEWTON_WORK squared distances.  Read off the
# table of tools/project_time.py on an MI355X: the host path takes about 0.8 ns per squared distance
# and 0.1 us per Newton solve, a device call about 1 ms whatever it does below 10^7 squared distances (host 0.74 ms against
# device 0.94 - 1.3 ms at 2.4e5, host 11 ms against device 1.6 ms at 1.3e7).  The crossover itself was not bracketed tighter.
DEVICE_MIN_WORK = 1 << 20
NEWTON_WORK = 128
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []

CURVE_MAX_K, SURFACE_MAX_K = 6, 4
MAX_SAMPLES = 8
SEED_CHUNK = 4096          # samples per chunk of the seed search
EVALS = 32                 # evaluations per point
HALVINGS = 20              # 2^-20 of a clamped step is within TRUST
TRUST = 2.0 ** -20         # of the domain width: steps this small are taken as they are
SMALL_STEP = 2.0 ** -40    # of the domain width: the next Newton step is below float64 resolution
STATUS_EVALS, STATUS_BOUND, STATUS_SINGULAR, STATUS_SKIPPED = 1, 2, 4, 8
WARN_BITS = STATUS_EVALS | STATUS_SINGULAR | STATUS_SKIPPED
SCOPE = "project: curves (nInd 1) of order 2 to 6 and surfaces (nInd 2) of orders 2 to 4, nDep 2 or 3"
INF = float("inf")


# ------------------------------------------------------------------------------------------ the statement
def seed_point(samples, p, begin, end):
    """What ``project_seed`` writes for one point and one chunk: samples is a list of nDep lists of M floats.
    -> (d2, index), (inf, -1) when no sample's squared distance is below inf."""
    best, idx = INF, -1
    for m in range(begin, end):
        acc = 0.0
        for d, comp in enumerate(samples):
            r = comp[m] - p[d]
            acc = r * r if d == 0 else acc + r * r
        if acc < best:
            best, idx = acc, m
    return best, idx


def reduce_partials(partials):
    best, idx = INF, -1
    for d2, k in partials:
        if d2 < best:
            best, idx = d2, k
    return best, idx


def eval1(c, x):
    """Value, first and second derivative of the Bernstein coefficients c at the local coordinate x."""
    b = list(c)
    K = len(b)
    s = 1.0 - x
    for r in range(1, K - 2):
        for i in range(K - r):
            b[i] = s * b[i] + x * b[i + 1]
    d1 = d2 = 0.0
    if K >= 3:
        d2 = float((K - 1) * (K - 2)) * ((b[2] - b[1]) - (b[1] - b[0]))
        b = [s * b[0] + x * b[1], s * b[1] + x * b[2]]
    if K >= 2:
        d1 = float(K - 1) * (b[1] - b[0])
        b = [s * b[0] + x * b[1]]
    return b[0], d1, d2


def find_cell(breaks, u):
    """The last cell whose left break is <= u, by bisection with (nc - 1).bit_length() steps."""
    nc = len(breaks) - 1
    lo, hi = 0, nc - 1
    for _ in range((nc - 1).bit_length()):
        mid = (lo + hi + 1) >> 1
        if breaks[mid] <= u:
            lo = mid
        else:
            hi = mid - 1
    return lo


class Tables:
    """The tables of the statement in Python floats: rows[d][r0][r1], first and breaks per axis (a curve has the axis-1
    tables of one cell [0, 1] of order 1), the orders K and the samples G per cell and axis."""

    def __init__(self, nind, rows, first, breaks, order, G):
        rows = np.asarray(rows, np.float64)
        self.nind = int(nind)
        if self.nind == 1:
            rows = rows.reshape(rows.shape[0], -1, 1)
            first, breaks, order, G = [first[0], [0]], [breaks[0], [0.0, 1.0]], [order[0], 1], [G[0], 1]
        self.rows = rows.tolist()
        self.R = rows.shape[1:]
        self.first = [[int(f) for f in first[d]] for d in range(2)]
        self.breaks = [[float(b) for b in breaks[d]] for d in range(2)]
        self.K = [int(k) for k in order]
        self.G = [int(g) for g in G]


def evaluate(tab, p, u0, u1):
    """-> None (the window leaves the rows) or (d2, g0, g1, a00, a01, a11, b00, b01, b11, h0, h1)."""
    K0, K1 = tab.K
    i = find_cell(tab.breaks[0], u0)
    left0 = tab.breaks[0][i]
    h0 = tab.breaks[0][i + 1] - left0
    x0 = (u0 - left0) / h0
    j, x1, h1 = 0, 0.0, 1.0
    if tab.nind == 2:
        j = find_cell(tab.breaks[1], u1)
        left1 = tab.breaks[1][j]
        h1 = tab.breaks[1][j + 1] - left1
        x1 = (u1 - left1) / h1
    f0, f1 = tab.first[0][i], tab.first[1][j]
    if f0 < 0 or f0 + K0 > tab.R[0] or f1 < 0 or f1 + K1 > tab.R[1]:
        return None
    d2 = g0 = g1 = a00 = a01 = a11 = b00 = b01 = b11 = 0.0
    for d, comp in enumerate(tab.rows):
        lines = [eval1(comp[f0 + r][f1:f1 + K1], x1) for r in range(K0)]
        f, fu, fuu = eval1([line[0] for line in lines], x0)
        r = f - p[d]
        d2 = d2 + r * r
        g0 = g0 + r * fu
        a00 = a00 + fu * fu
        b00 = b00 + r * fuu
        if tab.nind == 2:
            fv, fuv, _ = eval1([line[1] for line in lines], x0)
            fvv = eval1([line[2] for line in lines], x0)[0]
            g1 = g1 + r * fv
            a01 = a01 + fu * fv
            a11 = a11 + fv * fv
            b01 = b01 + r * fuv
            b11 = b11 + r * fvv
    return d2, g0, g1, a00, a01, a11, b00, b01, b11, h0, h1


def solve_step(e, fixed0, fixed1):
    """The local step on the free axes, or None."""
    _, g0, g1, a00, a01, a11, b00, b01, b11, _, _ = e
    if not fixed0 and not fixed1:
        h00, h01, h11 = a00 + b00, a01 + b01, a11 + b11
        det = h00 * h11 - h01 * h01
        if h00 > 0.0 and det > 0.0:
            return (g0 * h11 - h01 * g1) / det, (h00 * g1 - g0 * h01) / det
        det = a00 * a11 - a01 * a01
        if a00 > 0.0 and det > 0.0:
            return (g0 * a11 - a01 * g1) / det, (a00 * g1 - g0 * a01) / det
        return None
    if not fixed0:
        h = a00 + b00
        if h > 0.0:
            return g0 / h, 0.0
        return (g0 / a00, 0.0) if a00 > 0.0 else None
    h = a11 + b11
    if h > 0.0:
        return 0.0, g1 / h
    return (0.0, g1 / a11) if a11 > 0.0 else None


def _clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def _finite(x):
    return abs(x) < INF


def seed_start(tab, idx):
    """The parameters of flat sample ``idx``, or None when it is no sample."""
    G0, G1 = tab.G
    nc0, nc1 = len(tab.breaks[0]) - 1, len(tab.breaks[1]) - 1
    M1 = nc1 * G1
    if idx < 0 or idx >= nc0 * G0 * M1:
        return None
    m0, m1 = divmod(idx, M1)
    i, a = divmod(m0, G0)
    b0 = tab.breaks[0]
    s0 = b0[i] + ((float(a) + 0.5) / float(G0)) * (b0[i + 1] - b0[i])
    s1 = 0.0
    if tab.nind == 2:
        j, b = divmod(m1, G1)
        b1 = tab.breaks[1]
        s1 = b1[j] + ((float(b) + 0.5) / float(G1)) * (b1[j + 1] - b1[j])
    return s0, s1


def newton_point(tab, p, start, evals=None):
    """What ``project_newton`` returns for one point from ``start`` (s0, s1) or None, in plain Python floats:
    ((u0, u1), distance, status, evaluations)."""
    nan = float("nan")
    if start is None or not all(_finite(x) for x in p) or not all(_finite(x) for x in start):
        return (nan, nan), nan, STATUS_SKIPPED, 0
    two = tab.nind == 2
    lo0, hi0 = tab.breaks[0][0], tab.breaks[0][-1]
    lo1, hi1 = (tab.breaks[1][0], tab.breaks[1][-1]) if two else (0.0, 1.0)
    w0, w1 = hi0 - lo0, hi1 - lo1
    u0, u1 = _clamp(start[0], lo0, hi0), _clamp(start[1] if two else lo1, lo1, hi1)
    t0, t1, du0, du1 = u0, u1, 0.0, 0.0
    f = prev = INF
    halvings = n = status = 0
    conv = False
    for trip in range(EVALS if evals is None else evals):
        e = evaluate(tab, p, t0, t1)
        n += 1
        if e is None:
            status |= STATUS_SINGULAR
            break
        rel0, rel1 = abs(t0 - u0) / w0, (abs(t1 - u1) / w1 if two else 0.0)
        last = rel0 if rel0 > rel1 else rel1
        first, small = trip == 0, last <= TRUST
        if not (first or small or halvings == HALVINGS or e[0] <= f):
            halvings += 1
            du0, du1 = 0.5 * du0, 0.5 * du1
            t0, t1 = _clamp(u0 - du0, lo0, hi0), _clamp(u1 - du1, lo1, hi1)
            continue
        u0, u1, f = t0, t1, e[0]
        done = False
        if not first and small:
            done = last <= SMALL_STEP or not last < prev
            prev = last
        else:
            prev = INF
        fixed0 = (u0 <= lo0 and e[1] > 0.0) or (u0 >= hi0 and e[1] < 0.0)
        fixed1 = not two or (u1 <= lo1 and e[2] > 0.0) or (u1 >= hi1 and e[2] < 0.0)
        if done or (fixed0 and fixed1):
            conv = True
            break
        dx = solve_step(e, fixed0, fixed1)
        if dx is None:
            status |= STATUS_SINGULAR
            break
        du0, du1 = dx[0] * e[9], dx[1] * e[10]
        halvings = 0
        t0, t1 = _clamp(u0 - du0, lo0, hi0), _clamp(u1 - du1, lo1, hi1)
    if not conv and not status & STATUS_SINGULAR:
        status |= STATUS_EVALS
    if u0 <= lo0 or u0 >= hi0 or (two and (u1 <= lo1 or u1 >= hi1)):
        status |= STATUS_BOUND
    return (u0, u1), math.sqrt(f), status, n


def statement(tab, samples, points, guess=None, chunk=None):
    """uvw (nInd, N), distance, status and steps of the points (nDep, N) from the functions above: what the host drivers
    and the kernels return, bit for bit.  samples: (nDep, M) as the band steps gave them."""
    samples = np.asarray(samples, np.float64)
    samples = samples.reshape(samples.shape[0], -1).tolist()
    M = len(samples[0])
    chunk = SEED_CHUNK if chunk is None else int(chunk)
    points = np.asarray(points, np.float64)
    N = points.shape[1]
    uvw = np.empty((tab.nind, N))
    distance, status, steps = np.empty(N), np.empty(N, np.uint8), np.empty(N, np.int32)
    for n in range(N):
        p = [float(x) for x in points[:, n]]
        if guess is not None:
            start = (float(guess[0, n]), float(guess[1, n]) if tab.nind == 2 else 0.0)
        else:
            partials = [seed_point(samples, p, begin, min(begin + chunk, M)) for begin in range(0, M, chunk)]
            start = seed_start(tab, reduce_partials(partials)[1])
        u, distance[n], status[n], steps[n] = newton_point(tab, p, start)
        uvw[:, n] = u[:tab.nind]
    return uvw, distance, status, steps


# ------------------------------------------------------------------------------------------ plans and tables
def sample_weights(order, G):
    """(G, K): the Bernstein basis of degree K - 1 at (a + 1/2) / G, formed in extended precision and rounded once."""
    K = int(order)
    x = (np.arange(G, dtype=np.longdouble) + np.longdouble(0.5)) / np.longdouble(G)
    w = np.zeros((G, K), np.longdouble)
    w[:, 0] = 1
    for r in range(1, K):
        for i in range(r, -1, -1):
            w[:, i] = (1 - x) * w[:, i] + (x * w[:, i - 1] if i else 0)
    return w.astype(np.float64)


class Plan(_cells.TensorPlan):
    """``_cells.TensorPlan`` (Bezier extraction of every variable, the band steps on the axes 1 .. nInd of a tensor
    (nDep, *nCoef)) and the band steps of the sample grid on the extracted rows."""

    def __init__(self, order, knots, samples):
        super().__init__(order, knots)
        self.G = tuple(int(g) for g in samples)
        self.sample_steps = [self.sample_step(d) for d in range(self.nind)]
        self.nsamples = int(np.prod([nc * g for nc, g in zip(self.ncells, self.G)], dtype=np.int64))

    def sample_step(self, d):
        G, nc = self.G[d], self.ncells[d]
        return (d + 1, np.repeat(self.first[d], G).astype(np.int32), np.tile(sample_weights(self.order[d], G), (nc, 1)))

    def tables(self, rows):
        return Tables(self.nind, rows, self.first, self.breaks, self.order, self.G)


def _last():
    return nv.lib().bsk_project_last_kernel().decode()


# ------------------------------------------------------------------------------------------ the launches
def band_host(data, steps):
    """NumPy (nDep, ...) float64 through band steps (``_cells.band_host``)."""
    return _cells.band_host(data, steps, LAST_PATHS)


def _grid(plan, rows_ptr, tables):
    """The leading arguments of the newton entry points; ``tables``: first0, first1, breaks0, breaks1 as pointers."""
    K0, K1 = (plan.order + (1,))[:2]
    R0, R1 = (tuple(plan.rowlen) + (1,))[:2]
    nc0, nc1 = (tuple(plan.ncells) + (1,))[:2]
    g0, g1 = (plan.G + (1,))[:2]
    return (plan.nind, K0, K1, None, rows_ptr, R0, R1, nc0, nc1) + tuple(tables) + (g0, g1)


def _axis_tables(plan):
    first = [np.ascontiguousarray(f, np.int32) for f in plan.first]
    breaks = [np.ascontiguousarray(b, np.float64) for b in plan.breaks]
    if plan.nind == 1:
        first.append(np.zeros(1, np.int32))
        breaks.append(np.array([0.0, 1.0]))
    return first + breaks


def run(be, plan, rows, samples, points, guess, chunk):
    """rows (nDep, R0[, R1]), samples (nDep, M0[, M1]), points (nDep, N), guess (nInd, N) or None: the backend's contiguous
    float64 arrays.  -> uvw (nInd, N), distance, status, steps, the backend's."""
    nDep, N = points.shape
    M = plan.nsamples
    C = -(-M // chunk)
    with be:
        part_d2, part_idx = be.empty((C, N), np.float64), be.empty((C, N), np.int32)
        if guess is None:
            be.call("bsk_project_seed", nDep, be.ptr(samples), M, be.ptr(points), N, chunk, be.ptr(part_d2), be.ptr(part_idx))
            LAST_PATHS.append(_last())
        tabs = [be.put(t, t.dtype) for t in _axis_tables(plan)]
        args = list(_grid(plan, be.ptr(rows), [be.ptr(t) for t in tabs]))
        args[3] = nDep
        uvw, distance = be.empty((plan.nind, N), np.float64), be.empty(N, np.float64)
        status, steps = be.empty(N, np.uint8), be.empty(N, np.int32)
        be.call("bsk_project_newton", *args, be.ptr(points), N, be.ptr(part_d2), be.ptr(part_idx), C, be.ptr(guess), be.ptr(uvw),
                be.ptr(distance), be.ptr(status), be.ptr(steps))
        LAST_PATHS.append(_last())
    return uvw, distance, status, steps


def run_host(plan, rows, samples, points, guess, chunk):
    """``run`` on NumPy arrays."""
    rows, samples, points, guess = (None if a is None else np.ascontiguousarray(a, np.float64) for a in (rows, samples, points, guess))
    return run(_cells.Host(), plan, rows, samples, points, guess, chunk)


# ------------------------------------------------------------------------------------------ public
def _check_spline(spline):
    nInd, nDep = spline.nInd, spline.nDep
    top = {1: CURVE_MAX_K, 2: SURFACE_MAX_K}.get(nInd)
    if top is None or nDep not in (2, 3) or min(spline.order) < 2 or max(spline.order) > top:
        raise NotImplementedError(SCOPE)


def _samples(spline, samples):
    if samples is None:
        return tuple(int(k) for k in spline.order)
    G = (int(samples),) * spline.nInd if np.ndim(samples) == 0 else tuple(int(g) for g in samples)
    if len(G) != spline.nInd or min(G) < 1 or max(G) > MAX_SAMPLES:
        raise ValueError(f"samples must be from 1 to {MAX_SAMPLES} per knot cell and axis")
    return G


def host_tables(spline, samples=None):
    """The host path's tables: (plan, rows (nDep, R0[, R1]), samples (nDep, M0[, M1])), NumPy float64."""
    plan = Plan(spline.order, spline.knots, _samples(spline, samples))
    rows = np.asarray(spline.coefs).astype(np.float64)                # float32 is widened BEFORE the extraction
    if plan.steps:
        rows = band_host(rows, plan.steps)
    return plan, rows, band_host(rows, plan.sample_steps)


def norm_exponent(coefs):
    """e with max |coefficient| = m 2^e, 1/2 <= m < 1; 0 when that maximum is 0 or not finite.  The statement squares
    coordinates and multiplies the squares (A + B of ``solve_step``: the fourth power), so both paths work on the
    coefficients and the points x 2^-e and give the distances back x 2^e.  A power of two commutes with every rounding:
    in range (|e| <= 250) no bit of a result changes, and out of it the result is the in-range one."""
    top = float(np.abs(np.asarray(coefs, np.float64)).max(initial=0.0))
    return int(math.frexp(top)[1]) if 0.0 < top < INF else 0


def _ldexp(a, e):
    """a x 2^e for float64 NumPy arrays and torch tensors alike: in two factors, each a power of two in range (2^e
    itself need not be); exact unless the result is subnormal, and then the same on both paths."""
    half = e // 2
    with np.errstate(over="ignore", under="ignore"):                   # a distance beyond float64 is inf, as in the kernels
        return a * 2.0 ** half * 2.0 ** (e - half)


def project_batch(spline, points, guess=None, samples=None, _path=None, _chunk=None):
    """The closest point of the spline to each query point.  ``points``: (nDep, *shape), NumPy float32 / float64 or a torch
    CUDA tensor of those types; ``guess``: (nInd, *shape) of the same kind, takes the place of the seed search.
    Returns (uvw, distance, status, steps): the parameters (nInd, *shape) in the knots' dtype, the distances (*shape) in
    float64, the status bits (uint8; 1: evaluation bound reached, 2: foot point on a domain bound, 4: singular step,
    8: point not finite, not iterated) and the evaluations made (int32) per point.  CUDA in gives CUDA out; nothing leaves
    the device.  A flagged point never raises: it holds the best iterate."""
    del LAST_PATHS[:]
    path = _cells.pick_path(_path, FORCE_PATH)
    _check_spline(spline)
    G = _samples(spline, samples)
    nInd, nDep = spline.nInd, spline.nDep
    on_device = _cells.is_torch(points)
    if on_device:
        import torch
        if not points.is_cuda or points.dtype not in (torch.float32, torch.float64):
            raise TypeError("project takes the points as float32 or float64, NumPy or a torch CUDA tensor")
        if path == "host":
            raise ValueError("points on the device take the device path")
        path = "device"
    else:
        points = np.asarray(points)
        if points.dtype not in (np.float32, np.float64):
            raise TypeError("project takes the points as float32 or float64, NumPy or a torch CUDA tensor")
    if points.ndim < 1 or points.shape[0] != nDep:
        raise ValueError(f"points must have the shape ({nDep}, ...)")
    shape = tuple(points.shape[1:])
    if guess is not None:
        if _cells.is_torch(guess) != on_device:
            raise TypeError("guess must be of the same kind as the points (NumPy, or a torch CUDA tensor)")
        if on_device:
            if not guess.is_cuda or guess.dtype not in (torch.float32, torch.float64):
                raise TypeError("project takes the guess as float32 or float64")
        else:
            guess = np.asarray(guess)
            if guess.dtype not in (np.float32, np.float64):
                raise TypeError("project takes the guess as float32 or float64")
        if tuple(guess.shape) != (nInd,) + shape:
            raise ValueError(f"guess must have the shape {(nInd,) + shape}")
    chunk = SEED_CHUNK if _chunk is None else int(_chunk)
    if chunk < 1:
        raise ValueError("_chunk must be >= 1")
    N = int(np.prod(shape, dtype=np.int64))
    plan = Plan(spline.order, spline.knots, G)
    kdtype = np.result_type(*(k.dtype for k in spline.knots))
    e = norm_exponent(spline.coefs)
    if path is None:
        path = "device" if N * max(plan.nsamples, NEWTON_WORK) >= DEVICE_MIN_WORK and refinement.steps_covered(plan.steps) else "host"

    if N == 0:
        if on_device:
            dev = points.device
            return (torch.empty((nInd,) + shape, dtype=getattr(torch, kdtype.name), device=dev),
                    torch.empty(shape, dtype=torch.float64, device=dev), torch.empty(shape, dtype=torch.uint8, device=dev),
                    torch.empty(shape, dtype=torch.int32, device=dev))
        return np.empty((nInd,) + shape, kdtype), np.empty(shape), np.empty(shape, np.uint8), np.empty(shape, np.int32)

    if path == "device":
        import torch
        pts = (points if on_device else torch.from_numpy(np.ascontiguousarray(points)).cuda()).double().reshape(nDep, N)
        pts = (_ldexp(pts, -e) if e else pts).contiguous()
        dev = pts.device
        start = None
        if guess is not None:
            start = (guess if on_device else torch.from_numpy(np.ascontiguousarray(guess)).to(dev)).double().reshape(nInd, N).contiguous()
        rows = torch.from_numpy(np.ascontiguousarray(spline.coefs)).to(dev).double()   # widened BEFORE the extraction
        rows = _ldexp(rows, -e) if e else rows
        if plan.steps:
            rows, ran = refinement.run_device(rows, plan.steps)
            LAST_PATHS.extend(ran)
        rows = rows.contiguous()
        grid = None
        if start is None:
            grid, ran = refinement.run_device(rows, plan.sample_steps)
            LAST_PATHS.extend(ran)
            grid = grid.contiguous()
        uvw, distance, status, steps = run(_cells.Device(dev), plan, rows, grid, pts, start, chunk)
        uvw = uvw.to(getattr(torch, kdtype.name))
        distance = _ldexp(distance, e) if e else distance
        if not on_device:
            uvw, distance, status, steps = (a.cpu().numpy() for a in (uvw, distance, status, steps))
    else:
        pts = points.astype(np.float64).reshape(nDep, N)
        start = None if guess is None else guess.astype(np.float64).reshape(nInd, N)
        rows = np.asarray(spline.coefs).astype(np.float64)             # widened BEFORE the extraction
        if e:
            pts, rows = _ldexp(pts, -e), _ldexp(rows, -e)
        if plan.steps:
            rows = band_host(rows, plan.steps)
        grid = band_host(rows, plan.sample_steps) if start is None else None
        uvw, distance, status, steps = run_host(plan, rows, grid, pts, start, chunk)
        uvw = uvw.astype(kdtype)
        distance = _ldexp(distance, e) if e else distance
    return uvw.reshape((nInd,) + shape), distance.reshape(shape), status.reshape(shape), steps.reshape(shape)


def project(self, points, guess=None, samples=None, _path=None, _chunk=None):
    """``Spline.project``: (uvw, distance); one RuntimeWarning when a point is flagged (bits 1, 4 or 8)."""
    uvw, distance, status, _ = project_batch(self, points, guess=guess, samples=samples, _path=_path, _chunk=_chunk)
    flagged = (status & WARN_BITS) != 0
    count = int(flagged.sum())                                         # a status summary: the only thing that leaves the device
    if count:
        where = flagged.reshape(-1)
        index = int(where.nonzero()[0][0]) if _cells.is_torch(where) else int(np.flatnonzero(where)[0])
        warnings.warn(f"project: {count} of {where.shape[0]} points did not converge or were not iterated "
                      f"(project_batch returns the status bits); the first one has the flat index {index}", RuntimeWarning, stacklevel=3)
    return uvw, distance
