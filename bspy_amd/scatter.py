"""
Scattered least squares: ``Spline.fit_points`` and ``fit_batch`` (an extension beyond the reference's API, like ``project``
and ``intersect_rays``).  N points (u_i, p_i) without any grid structure, fixed order and knots; the result minimises

    sum_i w_i |S(u_i) - p_i|^2 + smoothing E_m(S),      E_m(S) = sum_{|alpha| = m} (m! / alpha!) int (d^alpha S)^2.

    device path   ``bsk_scatter_key``, a stable sort by key (``be.lexsort``), ``bsk_scatter_gram`` (one wave per unit),
                  ``bsk_scatter_cell`` (one launch per level of the tree), ``bsk_scatter_fold``; the stencil comes to the
                  host, ``bsk_scatter_solve_host``, or stays on the device, ``bsk_scatter_solve`` (``solve=``: a robust fit
                  of a large enough system takes it, a plain fit the host solve); ``bsk_scatter_residual`` and
                  ``bsk_scatter_reweight`` on the device
    host path     the ``*_host`` twins: the same functions of bsk_scatter.hpp on the CPU, for few points and for orders
                  5 and 6 or more than 4 dependent variables, which the kernels do not cover

THE STATEMENT (the functions below say it in plain Python floats, bit for bit what bsk_scatter.hpp computes; float64 whatever
the dtypes, float32 is widened first, every product and sum rounded on its own):
  * cells: variable d has order K_d, n_d coefficients and n_d + K_d knots t.  Knot cell c_d in 0 .. n_d - K_d is the span
    mu = c_d + K_d - 1, [t[mu], t[mu + 1]]; its basis functions are the coefficients c_d .. c_d + K_d - 1.  Cells of zero width
    exist and never hold a point.  The flat cell index is c0 nc1 + c1, nc_d = n_d - K_d + 1; a curve has K1 = n1 = nc1 = 1;
  * key (``point_key``): per variable the last span in K - 1 .. top whose left knot is <= u, by bisection (``find_span``); top
    is the last span of positive width, so the right domain end belongs to the last cell.  The key is the flat cell index.
    A point is excluded (key -1) with a status bit: 1 a parameter outside the domain, 2 a parameter, coordinate or weight that
    is NaN or infinite, 4 a negative weight;
  * order: a stable sort by key (``be.lexsort``): a cell's points keep their input order; the cells' offsets in the sorted
    order by ``be.searchsorted``;
  * units: a cell's points are cut, in that order, into units of SEG points (the last one may hold fewer);
  * basis (``basis``): Cox-de Boor on the 2K local knots l[0 .. 2K) = t[mu - K + 1 .. mu + K]: b = [1]; for j = 1 .. K - 1:
    saved = 0; for r = 0 .. j - 1: temp = b[r] / (l[K + r] - l[K + r - j]); b[r] = saved + (l[K + r] - u) temp;
    saved = (u - l[K + r - j]) temp; then b[j] = saved;
  * Gram slab of a unit (``gram_unit``): per point B_a = Bu_a0 Bv_a1 (a = a0 K1 + a1; Bu_a0 for a curve), t_a = w B_a (w = 1.0
    without weights), G_ab = G_ab + t_a B_b, r_ad = r_ad + t_a p_d, from 0.0.  The unit's points j = 0, 1, ... are dealt to
    Q = ``strands(K)`` strands, the largest power of two with Q K <= 64: strand q takes the points j = q (mod Q) in increasing
    j.  The strands' slabs are combined by the adjacent-pairs tree (``pair_tree``): (0, 1), (2, 3), ... level by level, an
    odd last one is carried up.  The slab is [K][K + nDep], all of it stored;
  * cell slab: the units' slabs of a cell by the same tree, in unit order; a cell without points is zero;
  * fold (``fold``): the normal matrix in stencil form (n0 n1, 2 K0 - 1, 2 K1 - 1), entry [i][d0 + K0 - 1][d1 + K1 - 1] for
    the coefficients i and j = i + (d0, d1) (0.0 where j is no coefficient), and the right-hand side (n0 n1, nDep): each the
    sum, from 0.0 and in increasing flat cell index, over the cells that hold both coefficients.  Entry (a, b) of a slab is
    read with a <= b, so the stencil is symmetric bit for bit;
  * penalty (``penalty_stencil``, NumPy on the host, one code path): per variable and derivative order r the Gram matrix of
    the basis' r-th derivatives by Gauss-Legendre with ``order`` nodes per span, in band form; a surface's penalty is
    sum_{a0 + a1 = m} (m! / (a0! a1!)) G0^(a0) x G1^(a1) in the stencil's layout, never a dense matrix;
  * solve: stencil + smoothing E (the product and the sum rounded on their own), expanded to upper band storage of half
    bandwidth (K0 - 1) n1 + K1 - 1 and factored as U^T D U without square roots on the host (``bsk_scatter_solve_host``,
    one code path): both paths give the same coefficients once their stencils agree, and weights x 2^k give the same bits.
    ``bsk_scatter_solve`` is the same solve on the device: the host's operations on the host's operands in the host's
    order, so its coefficients and its first bad pivot are the host's, bit for bit;
  * robust (``robust=``, ``reweight``, ``lower_median``): round 0 is the fit with the caller's weights w0 (1.0 without).  Each
    of the ``iterations`` rounds takes the residuals r_i = |S(u_i) - p_i| of the last fit, sigma = 1.4826 x the lower median
    (rank (M - 1) // 2 in sorted order) of r_i over the M points with status 0 and w0_i > 0, s = c sigma, and the weights
    Huber: r_i <= s ? w0_i : w0_i (s / r_i); Tukey: r_i < s ? w0_i (q q), q = 1.0 - (r_i / s)(r_i / s) : 0.0 (every operation
    rounded on its own; an excluded point keeps w0_i), then assembles and solves again.  sigma == 0.0 (an exact fit) ends
    the rounds; there is no convergence test, so the result is a function of the inputs alone.
No atomics, no waiting: two runs give the same bytes, and no launch shape enters the result.

``_path="device" | "host"`` (or ``scatter.FORCE_PATH``) pins the path; ``scatter.LAST_PATHS`` lists what the last call ran.
"""
import math
import warnings

import numpy as np

from . import _native as nv
from ._backend import Device, Host, choose, is_torch, pick_path

# Points from which the device path is taken.  Read off the 10^4 rows of the table of tools/scatter_time.py on an MI355X
# (DESIGN.md section 24): a cubic curve of 64 coefficients takes 1.05 ms on the host against 0.99 - 1.32 ms on the device, the
# 64 x 64 bicubic 30 ms against 22 - 23 ms (21 ms of both are the host solve); at 10^5 points the host loses 6 and 2 times.
# Nothing was measured below 10^4, so the crossover is not bracketed from below.
DEVICE_MIN_WORK = 10 ** 4
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []
# n hb^2 (coefficients x half bandwidth squared) from which a robust fit on the device path solves on the device
# (``solve=None``).  Read off the table of ``tools/scatter_time.py --solves`` on an MI355X: the smallest
# measured n hb^2 at which the device solve's slowest run beats the host's fastest is the 64 x 64 bicubic (n = 4096, hb = 195),
# 14.9 against 20.8 ms; the 128 x 128 bicubic wins 4.9 times.  The next smaller row, orders (3, 4) on 48 x 48 (2.3 x 10^7),
# loses, 8.76 against 3.00 ms, and nothing was measured between: the crossover is not bracketed from below.
SOLVE_MIN_WORK = 4096 * 195 * 195
FORCE_SOLVE = None         # None, "device" or "host"
SOLVE_MAX_HALF = 4095      # half bandwidths bsk_scatter_solve covers
LOSSES = {"huber": (0, 1.345), "tukey": (1, 4.685)}
SIGMA = 1.4826             # sigma of a normal distribution = SIGMA x its median absolute value

SEG = 256                  # points per unit: a constant of the statement
FAN = 16                   # inputs per node and level of bsk_scatter_cell: any power of two gives the same tree
HOST_MAX_K, DEVICE_MAX_K, DEVICE_MAX_NDEP = 6, 4, 4
MAX_BAND = 1 << 27         # doubles of band storage the host solve takes
STATUS_OUTSIDE, STATUS_NONFINITE, STATUS_WEIGHT = 1, 2, 4
SCOPE = ("fit_points: curves (nInd 1) and surfaces (nInd 2) of orders 2 to 6; the kernels cover orders 2 to 4 and nDep 1 to 4, "
         "the host path the rest; nInd 3 is not built")
INF = float("inf")


# ------------------------------------------------------------------------------------------ the statement
def strands(K):
    q = 1
    while 2 * q * K <= 64:
        q *= 2
    return q


def find_span(knots, lo, top, u):
    """The last span in lo .. top whose left knot is <= u, by bisection with (top - lo).bit_length() steps."""
    hi = top
    for _ in range((top - lo).bit_length()):
        mid = (lo + hi + 1) >> 1
        if knots[mid] <= u:
            lo = mid
        else:
            hi = mid - 1
    return lo


def top_span(order, knots):
    """The last span of positive width: the largest mu in K - 1 .. n - 1 with t[mu] < t[n]."""
    k, n = int(order), len(knots) - int(order)
    mu = n - 1
    while mu > k - 1 and not knots[mu] < knots[n]:
        mu -= 1
    return mu


def _finite(x):
    return abs(x) < INF


def point_key(order, knots, u, p, w=None):
    """(key, status) of one point: u a tuple of nInd floats, p a list of nDep floats, w a float or None."""
    st = 0
    if not all(_finite(x) for x in u) or not all(_finite(x) for x in p) or (w is not None and not _finite(w)):
        st |= STATUS_NONFINITE
    if w is not None and w < 0.0:
        st |= STATUS_WEIGHT
    for k, t, x in zip(order, knots, u):
        if x < t[k - 1] or x > t[len(t) - k]:
            st |= STATUS_OUTSIDE
    if st:
        return -1, st
    key = 0
    for k, t, x in zip(order, knots, u):
        key = key * (len(t) - 2 * k + 1) + find_span(t, k - 1, top_span(k, t), x) - (k - 1)
    return key, 0


def basis(K, knots, mu, u):
    local = [knots[mu - K + 1 + i] for i in range(2 * K)]
    b = [1.0]
    for j in range(1, K):
        saved = 0.0
        for r in range(j):
            tr, tl = local[K + r], local[K + r - j]
            temp = b[r] / (tr - tl)
            b[r] = saved + (tr - u) * temp
            saved = (u - tl) * temp
        b.append(saved)
    return b


def pair_tree(x):
    """The adjacent-pairs tree of a list of floats; 0.0 for none."""
    x = list(x)
    if not x:
        return 0.0
    while len(x) > 1:
        x = [x[i] + x[i + 1] if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    return x[0]


def reweight(loss, r, w0, key, s):
    """The robust weight of one point in plain floats: loss "huber" or "tukey", residual r, the caller's weight w0 (1.0
    without weights), the point's key and the threshold s = c sigma."""
    if key < 0:
        return w0
    if loss == "huber":
        return w0 if r <= s else w0 * (s / r)
    if r < s:
        t = r / s
        q = 1.0 - t * t
        return w0 * (q * q)
    return 0.0


def lower_median(values):
    """The element of rank (M - 1) // 2 of the M values in sorted order."""
    values = sorted(values)
    return values[(len(values) - 1) // 2]


def solve_statement(order, ncoef, stencil, rhs):
    """The U^T D U solve in plain floats, operation by operation what ``bsk_scatter_solve_host`` and ``bsk_scatter_solve``
    compute: stencil [n][S0 S1] and rhs [n][nDep] as lists.  -> (coefs [nDep][n], bad_row)."""
    K0, K1 = (tuple(order) + (1,))[:2]
    n0, n1 = (tuple(ncoef) + (1,))[:2]
    n, S1 = n0 * n1, 2 * K1 - 1
    hb = min((K0 - 1) * n1 + K1 - 1, n - 1)
    N = {}
    for i0 in range(n0):
        for i1 in range(n1):
            for d0 in range(K0):
                for d1 in range(-(K1 - 1), K1):
                    j0, j1 = i0 + d0, i1 + d1
                    i, j = i0 * n1 + i1, j0 * n1 + j1
                    if j0 < n0 and 0 <= j1 < n1 and j >= i:
                        N[i, j] = float(stencil[i][(d0 + K0 - 1) * S1 + d1 + K1 - 1])
    U, D = {}, [0.0] * n
    for j in range(n):
        low = max(0, j - hb)
        v = {}
        for i in range(low, j):
            acc = N.get((i, j), 0.0)
            for k in range(low, i):
                acc = acc - U[k, i] * v[k]
            v[i] = acc
        pivot = N.get((j, j), 0.0)
        for i in range(low, j):
            U[i, j] = v[i] / D[i]
            pivot = pivot - U[i, j] * v[i]
        if not pivot > 0.0:
            return None, j
        D[j] = pivot
    coefs = []
    for d in range(len(rhs[0])):
        y = [0.0] * n
        for j in range(n):
            acc = float(rhs[j][d])
            for k in range(max(0, j - hb), j):
                acc = acc - U[k, j] * y[k]
            y[j] = acc
        y = [y[j] / D[j] for j in range(n)]
        for i in range(n - 1, -1, -1):
            acc = y[i]
            for k in range(i + 1, min(i + hb, n - 1) + 1):
                acc = acc - U[i, k] * y[k]
            y[i] = acc
        coefs.append(y)
    return coefs, -1


def gram_unit(order, knots, cell, pts):
    """The slab [K][K + nDep] of one unit: ``cell`` the tuple of cell indices, ``pts`` its points (u, p, w) in order."""
    K = int(np.prod(order))
    nDep = len(pts[0][1])
    Q = strands(K)
    acc = [[[0.0] * (K + nDep) for _ in range(K)] for _ in range(Q)]
    for j, (u, p, w) in enumerate(pts):
        B = basis(order[0], knots[0], cell[0] + order[0] - 1, u[0])
        if len(order) == 2:
            Bv = basis(order[1], knots[1], cell[1] + order[1] - 1, u[1])
            B = [bu * bv for bu in B for bv in Bv]
        mine = acc[j % Q]
        for a in range(K):
            t = (1.0 if w is None else w) * B[a]
            for b in range(K):
                mine[a][b] = mine[a][b] + t * B[b]
            for d in range(nDep):
                mine[a][K + d] = mine[a][K + d] + t * p[d]
    return [[pair_tree([acc[q][a][e] for q in range(Q)]) for e in range(K + nDep)] for a in range(K)]


def cell_slab(slabs, K, W):
    """The units' slabs of a cell by the tree, entry by entry."""
    return [[pair_tree([s[a][e] for s in slabs]) for e in range(W)] for a in range(K)]


def fold(order, ncoef, nDep, cells):
    """cells: the slabs by flat cell index.  -> (stencil [n][S0 S1], rhs [n][nDep]) as lists."""
    K0, K1 = (tuple(order) + (1,))[:2]
    n0, n1 = (tuple(ncoef) + (1,))[:2]
    K, S1 = K0 * K1, 2 * K1 - 1
    nc0, nc1 = n0 - K0 + 1, n1 - K1 + 1
    stencil, rhs = [], []
    for i0 in range(n0):
        for i1 in range(n1):
            row = []
            for e in range((2 * K0 - 1) * S1 + nDep):
                j0, j1 = i0, i1
                if e < (2 * K0 - 1) * S1:
                    j0, j1 = i0 + e // S1 - (K0 - 1), i1 + e % S1 - (K1 - 1)
                acc = 0.0
                if 0 <= j0 < n0 and 0 <= j1 < n1:
                    for c0 in range(max(0, max(i0, j0) - K0 + 1), min(i0, j0, nc0 - 1) + 1):
                        for c1 in range(max(0, max(i1, j1) - K1 + 1), min(i1, j1, nc1 - 1) + 1):
                            a, b = (i0 - c0) * K1 + i1 - c1, (j0 - c0) * K1 + j1 - c1
                            slab = cells[c0 * nc1 + c1]
                            acc = acc + (slab[min(a, b)][max(a, b)] if e < (2 * K0 - 1) * S1 else slab[a][K + e - (2 * K0 - 1) * S1])
                row.append(acc)
            stencil.append(row[:(2 * K0 - 1) * S1])
            rhs.append(row[(2 * K0 - 1) * S1:])
    return stencil, rhs


def statement(order, knots, uvw, points, weights=None):
    """keys, status, the units' slabs (in unit order: by cell, then by position), the cells' slabs, stencil and rhs of the
    points, in plain Python floats: what both paths compute, bit for bit."""
    order = [int(k) for k in order]
    knots = [[float(x) for x in t] for t in knots]
    uvw = np.asarray(uvw, np.float64).reshape(len(order), -1)
    points = np.asarray(points, np.float64)
    N, nDep = uvw.shape[1], points.shape[0]
    ncoef = [len(t) - k for k, t in zip(order, knots)]
    nc = [n - k + 1 for n, k in zip(ncoef, order)]
    ncells, K = int(np.prod(nc)), int(np.prod(order))
    pts = [(tuple(float(x) for x in uvw[:, i]), [float(x) for x in points[:, i]], None if weights is None else float(weights[i]))
           for i in range(N)]
    keyed = [point_key(order, knots, *pt) for pt in pts]
    members = [[] for _ in range(ncells)]
    for i, (key, _) in enumerate(keyed):
        if key >= 0:
            members[key].append(pts[i])
    units, cells = [], []
    for c, mine in enumerate(members):
        cell = (c // nc[1], c % nc[1]) if len(order) == 2 else (c,)
        slabs = [gram_unit(order, knots, cell, mine[at:at + SEG]) for at in range(0, len(mine), SEG)]
        units += slabs
        cells.append(cell_slab(slabs, K, K + nDep))
    stencil, rhs = fold(order, ncoef, nDep, cells)
    return dict(key=np.array([k for k, _ in keyed], np.int64), status=np.array([s for _, s in keyed], np.uint8),
                units=np.array(units, np.float64).reshape(-1, K, K + nDep), cells=np.array(cells, np.float64),
                stencil=np.array(stencil, np.float64), rhs=np.array(rhs, np.float64))


# ------------------------------------------------------------------------------------------ the penalty
def _derivative_values(order, knots, mu, x, r):
    """(K,): the r-th derivatives at x of the K basis functions that live on span mu."""
    K, t = int(order), knots
    c = np.eye(K)                                                       # column f: coefficients mu - K + 1 .. mu of function f
    first = mu - K + 1
    for s in range(1, r + 1):                                           # order K - s + 1 -> K - s: coefficients first + s .. mu
        rows = np.arange(first + s, mu + 1)
        c = (K - s) * (c[1:] - c[:-1]) / (t[rows + K - s] - t[rows])[:, None]
    low = K - r
    b = np.array(basis(low, [float(v) for v in t], mu, float(x))) if low > 1 else np.ones(1)
    return b @ c


def gram_band(order, knots, r):
    """(n, 2K - 1): entry [i][d + K - 1] = int B_i^(r) B_(i+d)^(r), by Gauss-Legendre with ``order`` nodes per span (exact)."""
    K, t = int(order), np.asarray(knots, np.float64)
    n = len(t) - K
    out = np.zeros((n, 2 * K - 1))
    if r > K - 1:
        return out
    nodes, wts = np.polynomial.legendre.leggauss(K)
    for mu in range(K - 1, n):
        h = t[mu + 1] - t[mu]
        if not h > 0.0:
            continue
        block = np.zeros((K, K))
        for x, w in zip(nodes, wts):
            v = _derivative_values(K, t, mu, t[mu] + 0.5 * h * (x + 1.0), r)
            block += (0.5 * h * w) * np.outer(v, v)
        for a in range(K):
            out[mu - K + 1 + a, np.arange(K) - a + K - 1] += block[a]
    return out


def penalty_stencil(order, knots, m):
    """The penalty E_m in the stencil's layout (n0 n1, (2 K0 - 1)(2 K1 - 1))."""
    if len(order) == 1:
        return gram_band(order[0], knots[0], m)
    total = None
    for a0 in range(m + 1):
        g0, g1 = gram_band(order[0], knots[0], a0), gram_band(order[1], knots[1], m - a0)
        term = float(math.comb(m, a0)) * (g0[:, None, :, None] * g1[None, :, None, :])
        total = term if total is None else total + term
    return total.reshape(total.shape[0] * total.shape[1], -1)


def stencil_apply(order, ncoef, stencil, x):
    """N x for the stencil and x (n, nDep), NumPy: the objective's quadratic forms."""
    K0, K1 = (tuple(order) + (1,))[:2]
    n0, n1 = (tuple(ncoef) + (1,))[:2]
    S = stencil.reshape(n0, n1, 2 * K0 - 1, 2 * K1 - 1)
    X = np.zeros((n0 + 2 * K0 - 2, n1 + 2 * K1 - 2, x.shape[1]))
    X[K0 - 1:K0 - 1 + n0, K1 - 1:K1 - 1 + n1] = x.reshape(n0, n1, -1)
    out = np.zeros((n0, n1, x.shape[1]))
    for e0 in range(2 * K0 - 1):
        for e1 in range(2 * K1 - 1):
            out += S[:, :, e0, e1, None] * X[e0:e0 + n0, e1:e1 + n1]
    return out.reshape(n0 * n1, -1)


# ------------------------------------------------------------------------------------------ the launches
class Shape:
    """Orders, coefficient counts and knots of a call, and the leading arguments of the entry points."""

    def __init__(self, order, knots):
        self.nind = len(order)
        self.order = tuple(int(k) for k in order)
        self.knots = [np.ascontiguousarray(t, np.float64) for t in knots]
        self.ncoef = tuple(len(t) - k for t, k in zip(self.knots, self.order))
        self.tops = tuple(top_span(k, t) for k, t in zip(self.order, self.knots))
        self.nc = tuple(n - k + 1 for n, k in zip(self.ncoef, self.order))
        self.ncells = int(np.prod(self.nc))
        self.K = int(np.prod(self.order))
        self.n = int(np.prod(self.ncoef))
        self.K01 = (self.order + (1,))[:2]
        self.n01 = (self.ncoef + (1,))[:2]

    def tables(self, be):
        knots = self.knots + ([np.array([0.0, 1.0])] if self.nind == 1 else [])
        return [be.put(t, np.float64) for t in knots]

    def head(self, be, tabs, nDep):
        return (self.nind,) + self.K01 + self.n01 + tuple(be.ptr(t) for t in tabs) + (self.tops + (0,))[:2] + (nDep,)


def _last():
    return nv.lib().bsk_scatter_last_kernel().decode()


def assemble(be, sh, uvw, points, weights, keep=False):
    """uvw (nInd, N), points (nDep, N), weights (N,) or None: the backend's contiguous float64 arrays.  -> dict of key,
    status, counts (the points per cell), stencil (n, S0 S1) and rhs (n, nDep), the backend's; ``keep`` adds the units' and
    the cells' slabs."""
    nDep, N = points.shape
    K, W = sh.K, sh.K + nDep
    with be:
        tabs = sh.tables(be)
        head = sh.head(be, tabs, nDep)
        key, status = be.empty(N, np.int64), be.empty(N, np.uint8)
        be.call("bsk_scatter_key", *head, be.ptr(uvw), be.ptr(points), be.ptr(weights), N, be.ptr(key), be.ptr(status))
        LAST_PATHS.append(_last())
        order = be.lexsort([key])
        offsets = be.searchsorted(key[order], sh.ncells + 1)
        counts = offsets[1:] - offsets[:-1]
        count = (counts + (SEG - 1)) // SEG
        start = be.cumsum(count) - count
        total = int(count.sum())
        node_cell = be.repeat(be.arange(sh.ncells), count)
        level = be.zeros((max(total, 1), K, W), np.float64)
        if total:
            be.call("bsk_scatter_gram", *head, be.ptr(uvw), be.ptr(points), be.ptr(weights), N, be.ptr(order), be.ptr(offsets),
                    be.ptr(node_cell), be.ptr(start), total, be.ptr(level))
            LAST_PATHS.append(_last())
        units = level
        while True:
            nodes = (count + (FAN - 1)) // FAN
            nodes = nodes + (nodes == 0)
            out_start = be.cumsum(nodes) - nodes
            total = int(nodes.sum())
            node_cell = be.repeat(be.arange(sh.ncells), nodes)
            out = be.empty((total, K, W), np.float64)
            be.call("bsk_scatter_cell", K * W, be.ptr(level), be.ptr(start), be.ptr(count), be.ptr(node_cell), be.ptr(out_start), total,
                    be.ptr(out))
            LAST_PATHS.append(_last())
            level, count, start = out, nodes, out_start
            if total == sh.ncells:
                break
        stencil = be.empty((sh.n, (2 * sh.K01[0] - 1) * (2 * sh.K01[1] - 1)), np.float64)
        rhs = be.empty((sh.n, nDep), np.float64)
        be.call("bsk_scatter_fold", sh.nind, *sh.K01, *sh.n01, nDep, be.ptr(level), be.ptr(stencil), be.ptr(rhs))
        LAST_PATHS.append(_last())
    res = dict(key=key, status=status, counts=counts, stencil=stencil, rhs=rhs)
    if keep:
        res.update(units=units, cells=level)
    return res


def residuals(be, sh, coefs, uvw, points, key):
    """|S(u_i) - p_i| per point, NaN for an excluded one: coefs (nDep, n) NumPy, the rest the backend's."""
    nDep, N = points.shape
    with be:
        tabs = sh.tables(be)
        c = be.put(coefs, np.float64)
        out = be.empty(N, np.float64)
        be.call("bsk_scatter_residual", *sh.head(be, tabs, nDep), be.ptr(c), be.ptr(uvw), be.ptr(points), be.ptr(key), N, be.ptr(out))
        LAST_PATHS.append(_last())
    return out


def _not_definite(sh, bad):
    row = tuple(int(x) for x in np.unravel_index(int(bad), sh.ncoef))
    return ValueError(f"fit_points: the normal matrix is not positive definite: the pivot of row {int(bad)} (coefficient {row}) "
                      "is not positive; more data or smoothing > 0 makes it so")


def half_bandwidth(sh):
    return min((sh.K01[0] - 1) * sh.n01[1] + sh.K01[1] - 1, sh.n - 1)


def device_solve_scope(sh, nDep):
    """None when ``bsk_scatter_solve`` covers the system, else the reason."""
    if nDep > DEVICE_MAX_NDEP:
        return f"the device solve covers nDep 1 to {DEVICE_MAX_NDEP}"
    if half_bandwidth(sh) > SOLVE_MAX_HALF:
        return f"the device solve covers half bandwidths up to {SOLVE_MAX_HALF}"
    return None


def solve(sh, stencil, rhs, where=None):
    """The coefficients (nDep, n), NumPy, of the stencil (n, S0 S1) and rhs (n, nDep): the banded U^T D U solve.  NumPy
    arrays are solved on the host (``where`` None or "host") or sent to the device ("device"); torch CUDA tensors are
    solved on the device (None or "device") or fetched ("host").  Both solves give the same bytes."""
    on_device = is_torch(stencil)
    if where not in (None, "host", "device"):
        raise ValueError("where must be None, 'device' or 'host'")
    where = where or ("device" if on_device else "host")
    nDep = rhs.shape[1]
    half = (sh.K01[0] - 1) * sh.n01[1] + sh.K01[1] - 1
    if sh.n * (half + 1) > MAX_BAND:
        raise ValueError(f"fit_points: {sh.n} coefficients with the half bandwidth {half} need more than 2^27 doubles of band storage; "
                         "the solve runs on the host (a device solve is not built)")
    L = nv.lib()
    if where == "device":
        why = device_solve_scope(sh, nDep)
        if why is not None:
            raise ValueError(why)
        import torch
        if on_device:
            be = Device(stencil.device)
            stencil, rhs = stencil.double().contiguous(), rhs.double().contiguous()
        else:
            be = Device.current()
            stencil, rhs = be.put(stencil, np.float64), be.put(rhs, np.float64)
        need = np.zeros(1, np.int64)
        nv.check(L.bsk_scatter_solve_work(sh.nind, *sh.K01, *sh.n01, nDep, need.ctypes.data_as(nv._i64p)))
        with be:
            work = be.empty(int(need[0]), np.float64)
            coefs, bad = be.empty((nDep, sh.n), np.float64), be.empty(1, np.int64)
            be.call("bsk_scatter_solve", sh.nind, *sh.K01, *sh.n01, nDep, be.ptr(stencil), be.ptr(rhs), be.ptr(coefs), be.ptr(work),
                    int(need[0]), be.ptr(bad))
            name = _last()
            bad = int(bad.cpu()[0])
            if bad >= 0:
                raise _not_definite(sh, bad)
            coefs = be.get(coefs)
        LAST_PATHS.append(name)
        return coefs
    if on_device:
        stencil, rhs = stencil.cpu().numpy(), rhs.cpu().numpy()
    stencil, rhs = np.ascontiguousarray(stencil, np.float64), np.ascontiguousarray(rhs, np.float64)
    coefs = np.empty((nDep, sh.n))
    bad = np.zeros(1, np.int64)
    st = L.bsk_scatter_solve_host(sh.nind, *sh.K01, *sh.n01, nDep, stencil.ctypes.data, rhs.ctypes.data, coefs.ctypes.data,
                                  bad.ctypes.data_as(nv._i64p))
    if st != nv.BSK_OK and bad[0] >= 0:
        raise _not_definite(sh, bad[0])
    nv.check(st)
    LAST_PATHS.append(_last())
    return coefs


_solve = solve             # fit_batch has a keyword of that name


def sigma(values):
    """SIGMA x the lower median of the values (NumPy, (M,)); 0.0 for none.  Selection is exact: ``lower_median`` in NumPy."""
    if not len(values):
        return 0.0
    rank = (len(values) - 1) // 2
    return SIGMA * float(np.partition(values, rank)[rank])


def reweights(be, loss, s, residual, weights, key):
    """The robust weights (N,) of a round, the backend's: ``bsk_scatter_reweight``."""
    N = residual.shape[0]
    with be:
        out = be.empty(N, np.float64)
        be.call("bsk_scatter_reweight", LOSSES[loss][0], float(s), be.ptr(residual), be.ptr(weights), be.ptr(key), N, be.ptr(out))
        LAST_PATHS.append(_last())
    return out


def _robust(robust):
    """(loss, c) of ``robust=``, or None."""
    if robust is None:
        return None
    name, c = (robust, None) if isinstance(robust, str) else tuple(robust)
    if name not in LOSSES:
        raise ValueError(f"robust must be None, 'huber', 'tukey' or (name, c), not {name!r}")
    c = LOSSES[name][1] if c is None else float(c)
    if not (c > 0.0 and c < INF):
        raise ValueError("robust: the tuning constant c must be finite and > 0")
    return name, c


# ------------------------------------------------------------------------------------------ public
def _as_rows(a, rows, what, on_device):
    if on_device:
        import torch
        if not is_torch(a) or not a.is_cuda or a.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"fit_points takes {what} as float32 or float64, all NumPy or all torch CUDA tensors")
        a = a.double()
    else:
        if is_torch(a):
            raise TypeError(f"fit_points takes {what} as float32 or float64, all NumPy or all torch CUDA tensors")
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"fit_points takes {what} as float32 or float64, all NumPy or all torch CUDA tensors")
        a = a.astype(np.float64)
    if rows is not None:
        a = a.reshape(1, -1) if a.ndim == 1 and rows == 1 else a
        if a.ndim != 2 or a.shape[0] != rows:
            raise ValueError(f"{what} must have the shape ({rows}, N)")
    return a


def _empty_support(sh, counts):
    """The index tuple of the first coefficient whose support holds no point, or None."""
    free = (np.asarray(counts).reshape(sh.nc) == 0).astype(np.int64)
    for axis, (k, n) in enumerate(zip(sh.order, sh.ncoef)):                # windowed "all cells empty", one axis at a time
        run = np.concatenate((np.zeros_like(np.take(free, [0], axis=axis)), np.cumsum(free, axis=axis)), axis=axis)
        i = np.arange(n)
        lo, hi = np.maximum(i - k + 1, 0), np.minimum(i, n - k) + 1
        width = (hi - lo).reshape([-1 if a == axis else 1 for a in range(sh.nind)])
        free = (np.take(run, hi, axis=axis) - np.take(run, lo, axis=axis) == width).astype(np.int64)
    at = np.argwhere(free)
    return None if not len(at) else tuple(int(x) for x in at[0])


def fit_batch(uvw, points, order, knots, weights=None, smoothing=0.0, penalty=None, correct=0, metadata={}, robust=None,
              iterations=8, solve=None, _path=None):
    """``Spline.fit_points`` and what happened: (spline, info).  info: ``status`` (N,) uint8 (1 a parameter outside the
    domain, 2 something not finite, 4 a negative weight: the point is excluded), ``residual`` (N,) |S(u_i) - p_i| (NaN for
    an excluded point), ``rms`` and ``max`` over the points that count, ``empty`` the knot cells of positive width without a
    point, ``objective`` the objective of every solve, ``uvw`` the parameters of the last fit, ``paths``.  CUDA tensors in
    give CUDA ``status`` and ``residual`` out.

    ``robust`` ("huber", "tukey" or (name, c); c defaults to 1.345 and 4.685) runs exactly ``iterations`` reweighted rounds
    behind the plain fit (fewer only when sigma == 0.0) and adds ``weights`` (the weights of the last solve, CUDA for CUDA
    in), ``scale`` (sigma per round) and ``rounds`` to info; ``residual``, ``rms`` and ``max`` are the last fit's.  Tukey can
    take all weight from under a coefficient: that is the ValueError of the pivot ("not positive definite ... smoothing > 0
    makes it so").  With ``correct`` every fit of the correction loop is the whole robust loop, started from ``weights``.
    ``solve`` ("host", "device" or None, else ``scatter.FORCE_SOLVE``) pins the solve: None is the host solve for a plain
    fit and, for a robust fit on the device path, the device solve when it covers the system and n hb^2 reaches
    ``SOLVE_MIN_WORK``."""
    from . import project as _project
    from .spline import Spline
    del LAST_PATHS[:]
    path = pick_path(_path, FORCE_PATH)
    order = tuple(int(k) for k in (order if np.ndim(order) else (order,)))
    nInd = len(order)
    if nInd not in (1, 2):
        raise NotImplementedError(SCOPE)
    if nInd == 1 and np.ndim(knots[0]) == 0:
        knots = (knots,)
    if len(knots) != nInd:
        raise ValueError("knots must hold one knot array per independent variable")
    knots = [np.asarray(t, np.float64) for t in knots]
    if min(order) < 2 or max(order) > HOST_MAX_K:
        raise NotImplementedError(SCOPE)
    for k, t in zip(order, knots):
        if t.ndim != 1 or len(t) < 2 * k or np.any(np.diff(t) < 0) or not t[k - 1] < t[len(t) - k]:
            raise ValueError("knots must be non-decreasing, at least 2 order of them, with a domain of positive width")
    sh = Shape(order, knots)
    on_device = is_torch(points)
    uvw = _as_rows(uvw, nInd, "uvw", on_device)
    points = _as_rows(points, None, "points", on_device)
    if points.ndim != 2 or points.shape[1] != uvw.shape[1] or points.shape[0] < 1:
        raise ValueError("points must have the shape (nDep, N) for uvw of the shape (nInd, N)")
    nDep, N = points.shape
    if N < 1:
        raise ValueError("fit_points needs at least one point")
    if weights is not None:
        weights = _as_rows(weights, 1, "weights", on_device).reshape(-1)
        if weights.shape[0] != N:
            raise ValueError("weights must have the shape (N,)")
    smoothing = float(smoothing)
    if not smoothing >= 0.0 or smoothing == INF:
        raise ValueError("smoothing must be finite and >= 0")
    m = min(2, min(order) - 1) if penalty is None else int(penalty)
    if smoothing > 0.0 and not 1 <= m <= min(order) - 1:
        raise ValueError(f"penalty must be a derivative order from 1 to min(order) - 1 = {min(order) - 1}")
    correct = int(correct)
    if correct and nDep not in (2, 3):
        raise ValueError("correct > 0 takes nDep 2 or 3 (Spline.project)")
    robust = _robust(robust)
    iterations = int(iterations)
    if robust is not None and iterations < 1:
        raise ValueError("robust takes iterations >= 1")
    where = solve if solve is not None else FORCE_SOLVE
    if where not in (None, "host", "device"):
        raise ValueError("solve must be None, 'device' or 'host'")
    covered = max(order) <= DEVICE_MAX_K and nDep <= DEVICE_MAX_NDEP
    if on_device:
        if path == "host":
            raise ValueError("points on the device take the device path")
        path = "device"
    path = choose(path, covered, N >= DEVICE_MIN_WORK, f"the device path covers orders 2 to {DEVICE_MAX_K} and nDep 1 to {DEVICE_MAX_NDEP}")
    half = (sh.K01[0] - 1) * sh.n01[1] + sh.K01[1] - 1
    if sh.n * (half + 1) > MAX_BAND:
        raise ValueError(f"fit_points: {sh.n} coefficients with the half bandwidth {half} need more than 2^27 doubles of band storage; "
                         "the solve runs on the host (a device solve is not built)")

    if path == "device":
        import torch
        dev = points.device if on_device else torch.device("cuda", torch.cuda.current_device())
        be = Device(dev)
        up = (lambda a: a.contiguous()) if on_device else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    else:
        be, up = Host(), np.ascontiguousarray
    if where == "device":
        why = "the device solve belongs to the device path" if path != "device" else device_solve_scope(sh, nDep)
        if why is not None:
            raise ValueError(f"solve='device': {why}")
    elif where is None:
        hb = half_bandwidth(sh)
        large = robust is not None and path == "device" and device_solve_scope(sh, nDep) is None and sh.n * hb * hb >= SOLVE_MIN_WORK
        where = "device" if large else "host"
    uvw, points, weights = up(uvw), up(points), None if weights is None else up(weights)
    E = penalty_stencil(order, knots, m) if smoothing > 0.0 else None
    E_there = be.put(E, np.float64) if E is not None and where == "device" else None

    def one_fit(current):
        """Assemble with the weights ``current``, solve, residuals, the objective's value."""
        res = assemble(be, sh, uvw, points, current)
        counts = be.get(res["counts"])
        if smoothing == 0.0:
            at = _empty_support(sh, counts)
            if at is not None:
                raise ValueError(f"fit_points: no point lies in the support of the coefficient {at}: the fit is not determined there; "
                                 "smoothing > 0 fills it in")
        if where == "device":                                               # the product and the sum rounded on their own
            total = res["stencil"] if E is None else res["stencil"] + E_there * smoothing
            coefs = _solve(sh, total, res["rhs"], "device")
        else:
            stencil, rhs = be.get(res["stencil"]), be.get(res["rhs"])
            total = stencil if E is None else stencil + smoothing * E
            coefs = _solve(sh, total, rhs)
        residual = residuals(be, sh, coefs, uvw, points, res["key"])
        r = be.get(residual)
        ok = be.get(res["status"]) == 0
        w = np.ones(int(ok.sum())) if current is None else be.get(current)[ok]
        value = float(np.sum(w * r[ok] * r[ok]))
        if E is not None:
            value += smoothing * float(np.sum(coefs.T * stencil_apply(order, sh.ncoef, E, coefs.T)))
        objective.append(value)
        return res, counts, coefs, residual, r, ok

    objective, scale, rounds, last = [], [], 0, weights
    for round_ in range(correct + 1):
        res, counts, coefs, residual, r, ok = one_fit(weights)
        last = weights
        if robust is not None:
            counted = ok if weights is None else ok & (be.get(weights) > 0.0)
            for _ in range(iterations):
                scale.append(sigma(r[counted]))
                if scale[-1] == 0.0:
                    break
                last = reweights(be, robust[0], robust[1] * scale[-1], residual, weights, res["key"])
                res, counts, coefs, residual, r, ok = one_fit(last)
                rounds += 1
        spline = Spline(nInd, nDep, order, sh.ncoef, knots, coefs.reshape((nDep,) + sh.ncoef), metadata)
        if round_ < correct:
            moved, _ = spline.project(points if on_device else be.get(points), guess=uvw if on_device else be.get(uvw),
                                      _path=None if on_device else path)
            LAST_PATHS.extend(_project.LAST_PATHS)
            uvw = up(moved.double() if on_device else np.asarray(moved, np.float64))
    status = res["status"]
    info = dict(status=status, residual=residual, rms=float(np.sqrt(np.mean(r[ok] * r[ok]))) if ok.any() else float("nan"),
                max=float(r[ok].max()) if ok.any() else float("nan"),
                empty=int(np.count_nonzero((np.asarray(counts).reshape(sh.nc) == 0) & _positive(sh))), objective=objective,
                uvw=uvw, paths=list(LAST_PATHS))
    if robust is not None:
        if last is None:
            last = be.put(np.ones(N), np.float64)
        info.update(weights=last, scale=scale, rounds=rounds)
    if not on_device and path == "device":
        info.update(status=be.get(status), residual=r, uvw=be.get(uvw))
        if robust is not None:
            info.update(weights=be.get(last))
    return spline, info


def _positive(sh):
    """bool (nc0[, nc1]): the knot cells of positive width."""
    wide = [np.diff(t[k - 1:len(t) - k + 1]) > 0.0 for t, k in zip(sh.knots, sh.order)]
    return wide[0] if sh.nind == 1 else wide[0][:, None] & wide[1][None, :]


def fit_points(uvw, points, order, knots, weights=None, smoothing=0.0, penalty=None, correct=0, metadata={}, robust=None,
               iterations=8, solve=None, _path=None):
    """``Spline.fit_points``: the spline; one RuntimeWarning when points were excluded."""
    spline, info = fit_batch(uvw, points, order, knots, weights=weights, smoothing=smoothing, penalty=penalty, correct=correct,
                             metadata=metadata, robust=robust, iterations=iterations, solve=solve, _path=_path)
    flagged = info["status"] != 0
    count = int(flagged.sum())
    if count:
        index = int(flagged.nonzero()[0][0]) if is_torch(flagged) else int(np.flatnonzero(flagged)[0])
        warnings.warn(f"fit_points: {count} of {flagged.shape[0]} points were excluded (outside the domain, not finite or of negative "
                      f"weight; fit_batch returns the status bits); the first one has the flat index {index}", RuntimeWarning, stacklevel=3)
    return spline
