"""
The cases, the reference and the bars of the integral sweep (tests/test_integral_sweep_host.py,
tests/test_gpu_integral_sweep.py): every instantiation of ``integral_regions<T, NIND, OMAX>`` (bsk_integral.hpp; 18 =
fp32 / fp64 x nInd 1 - 3 x order bucket 4 / 8 / 16) per node and per region, without the adaptive driver, which
repairs what the kernel gets wrong.  NumPy, ``fractions`` and ``math`` only: no GPU, no pytest.

The reference (``reference``)
    Cox - de Boor and the window contraction in ``np.longdouble`` from the spline, ``lo_hi`` and ``span``.  Per node: x,
    the jacobian J, the measure mu, wK mu and wG mu; per region K and G (``math.fsum`` of the nodes' high and low
    parts).  Nodes are first-variable-slowest, at u = T(0.5 (lo + hi) + half GK_X[j]) formed in fp64 from the bounds
    rounded to T.  tests/test_integral_sweep_host.py holds it to exact rational arithmetic.

The bars are counted, not chosen (unit = the unit roundoff of T, 2^-24 or 2^-53; gamma(n) = n unit / (1 - n unit)):
    x           gamma(n_x) sum |c_k| B_k + sum_i |dx/du_i| ulp_T(u_i).  Longest path of ``basis_bounded``, per value
                level: u - t (1), the stored reciprocal (1), their product alpha (1), 1 - alpha (1), its product with
                the entry (1), the add (1) = 6; order o has o - 1 levels.  The contraction of one variable: the
                product (1) and o adds.  n_x = sum_i (6 (o_i - 1) + o_i + 1).  The ulp term: the kernel forms u in
                fp64, where the expression may be contracted to an fma, and then rounds to T.
    J[., i]     the last level of variable i is a derivative level: the reciprocal (1), times the degree (1), the
                product with the entry (1), the subtraction (1) = 4, so n_J = n_x - 2, on sum |c_k| A_k, where A is
                the derivative basis with both terms of its last level taken positive (the roundings are relative to
                the terms, not to their difference), plus sum_j |d2x/du_i du_j| ulp_T(u_j).
                Both counts are first order in the sense that an error of alpha is charged to the entry that
                (1 - alpha) feeds; the cases keep the coefficients of a window of one sign and comparable size, and
                the C oracle, which rounds at the same places, is held to the same bars on the CPU.
    mu          the bars of J to first order through the Gram matrix (nDep != nInd: a product and nDep or nInd - 1
                adds per entry, n = nDep or nInd) and through the determinant with the sum of the absolute values of
                its expansion terms (2 x 2: 2 roundings, 3 x 3: 5), then through the square root (1 rounding): with d
                the bar of the determinant, mu - sqrt(mu^2 - d), and sqrt(d) where mu^2 <= d.
    wK mu       wK bar(mu) + (2 nInd + 1) 2^-53 wK mu: vol and the weight are products of nInd doubles each.
    K, G        against ``math.fsum`` of the same call's NODES columns: (ceil(NN / BLOCK) + 6 + BLOCK / 64 + 1) 2^-53
                sum |f| - the product (MEASURE may fuse it into the accumulation), the per-lane adds, six shuffle
                levels, the wave adds; against the reference: the node bars summed, plus that.

The conditioning precondition of the non-degenerate cases, mu >= 0.1 prod ||v||, takes for v the vectors whose Gram
determinant mu^2 is: the columns dS/du_i where nDep >= nInd, the rows of J where nDep < nInd (the product of the
columns has another dimension there).
"""
import itertools
import math
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

LD = np.longdouble

# ------------------------------------------------------------------------------------------ the kernel's constants
GK_N = 15
GK_X = np.array([
    -0.99145537112081264, -0.94910791234275852, -0.86486442335976907, -0.74153118559939444, -0.58608723546769113,
    -0.40584515137739717, -0.20778495500789847, 0.0, 0.20778495500789847, 0.40584515137739717,
    0.58608723546769113, 0.74153118559939444, 0.86486442335976907, 0.94910791234275852, 0.99145537112081264])
GK_WK = np.array([
    0.022935322010529225, 0.063092092629978553, 0.10479001032225018, 0.14065325971552592, 0.16900472663926790,
    0.19035057806478541, 0.20443294007529889, 0.20948214108472783, 0.20443294007529889, 0.19035057806478541,
    0.16900472663926790, 0.14065325971552592, 0.10479001032225018, 0.063092092629978553, 0.022935322010529225])
GK_WG = np.array([
    0.0, 0.12948496616886969, 0.0, 0.27970539148927667, 0.0, 0.38183005050511894, 0.0, 0.41795918367346939,
    0.0, 0.38183005050511894, 0.0, 0.27970539148927667, 0.0, 0.12948496616886969, 0.0])
BUCKETS = (4, 8, 16)
LOWEST_MAX = {4: 2, 8: 5, 16: 9}
MIN_CAP = 2048
DTYPES = (np.float32, np.float64)
# the text of the sources that the constants above restate (test_integral_sweep_host.py looks each up)
SOURCE_TEXT = {
    "bsk_integral.hpp": ("constexpr int GK_N = 15;", "static constexpr int BLOCK = NIND == 1 ? 64 : 256;",
                         "static constexpr int CAP = WIN > 2048 ? WIN : 2048;", "const int DG = CAP / W;",
                         "const bool once = nDep <= DG;"),
    "bsk_integral_tu.hip": ("if (omax <= 4) launch_integral<T, NIND, 4>", "else if (omax <= 8) launch_integral<T, NIND, 8>",
                            "else launch_integral<T, NIND, 16>"),
}


def block_of(nind):
    return 64 if nind == 1 else 256


def bucket_of(orders):
    return next(b for b in BUCKETS if max(orders) <= b)


def staging(orders):
    """(W, CAP, DG) of the kernel for these orders."""
    W = int(np.prod(orders))
    CAP = max(MIN_CAP, bucket_of(orders) ** len(orders))
    return W, CAP, CAP // W


def tag(dtype):
    return "fp32" if np.dtype(dtype) == np.float32 else "fp64"


def unit_of(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def gamma(n, unit):
    return n * unit / (1.0 - n * unit)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------ the case table
# kind: allmax, lowmax, pos0 / pos1 / pos2 (that variable alone holds the maximum), order1, nodiv (W does not divide
# CAP), line (all control points on a line), equal (two equal dependents).  stage: "", "DG" or "DG+1".
Case = namedtuple("Case", "dtype nInd bucket orders nDep kind stage")
Instance = namedtuple("Instance", "dtype nInd bucket")
INSTANCES = [Instance(dt, n, b) for dt in DTYPES for n in (1, 2, 3) for b in BUCKETS]
NODIV = {1: (3,), 2: (3, 3), 3: (3, 5, 7)}
DEGENERATE_ORDERS = {2: (3, 4), 3: (3, 2, 4)}


def position_tuples(nind, B):
    """Per variable position, a tuple in which that variable alone holds B and the others are lower, one of them 2."""
    low = LOWEST_MAX[B] if B > 4 else 3
    if nind == 2:
        return [(B, 2), (2, B)]
    return [(B, 2, low), (low, B, 2), (2, low, B)]


def branch(case):
    return "lt" if case.nDep < case.nInd else "eq" if case.nDep == case.nInd else "gt"


def is_degenerate(case):
    return case.kind in ("line", "equal") or (case.kind == "order1" and case.nDep >= case.nInd)


def is_exact_zero(case):
    """An order-1 variable makes a zero column of J: with nDep >= nInd every product of the measure has a zero factor."""
    return case.kind == "order1" and case.nDep >= case.nInd


def case_id(case):
    stage = f"-stage{case.stage}" if case.stage else ""
    return (f"{tag(case.dtype)}-nInd{case.nInd}-b{case.bucket}-o{'x'.join(map(str, case.orders))}-nDep{case.nDep}-{branch(case)}"
            f"-{case.kind}{stage}")


def instance_label(case):
    return f"integral sweep: {tag(case.dtype)} nInd{case.nInd} b{case.bucket}"


def _cases():
    out = []

    def add(dt, orders, ndep, kind, stage=""):
        out.append(Case(dt, len(orders), bucket_of(orders), tuple(orders), ndep, kind, stage))

    for dt, n, B in INSTANCES:
        allmax = (B,) * n
        DG = staging(allmax)[2]
        add(dt, allmax, DG, "allmax", "DG")
        add(dt, allmax, DG + 1, "allmax", "DG+1")
        lowmax = (LOWEST_MAX[B],) * n
        add(dt, lowmax, n, "lowmax")
        add(dt, lowmax, n + 1, "lowmax")
        if n == 2:
            p0, p1 = position_tuples(n, B)
            add(dt, p0, 1, "pos0")
            add(dt, p0, 2, "pos0")
            add(dt, p1, 3, "pos1")
        if n == 3:
            p0, p1, p2 = position_tuples(n, B)
            add(dt, p0, 1, "pos0")
            add(dt, p1, 2, "pos1")
            add(dt, p2, 3, "pos2")
            add(dt, p2, 4, "pos2")
        if B == 4:
            one = {1: (1,), 2: (1, 3), 3: (2, 1, 3)}[n]
            for ndep in sorted({max(1, n - 1), n, n + 1}):
                add(dt, one, ndep, "order1")
        if B == bucket_of(NODIV[n]):
            DG = staging(NODIV[n])[2]
            add(dt, NODIV[n], DG, "nodiv", "DG")
            add(dt, NODIV[n], DG + 1, "nodiv", "DG+1")
        if B == 4 and n >= 2:
            deg = DEGENERATE_ORDERS[n]
            for ndep in sorted({n - 1, n, n + 1} - {1}):              # the three clamps' branches; nDep 1 has no determinant
                add(dt, deg, ndep, "line")
            add(dt, deg, n, "equal")
    return out


CASES = _cases()
CASE_IDS = [case_id(c) for c in CASES]


# ------------------------------------------------------------------------------------------ knots, coefficients, regions
WIDTHS = (0.5, 0.25, 1.0, 0.25, 0.5)                    # the five cells of every variable
DOMAIN_LO = (-1.5, 1.25, 0.5)                           # one negative, one above 1
SCALE, NOISE = 256, 2                                   # coefficients: eighths of rint(8 SCALE affine) + [-NOISE, NOISE]
DEEP = {np.dtype(np.float32): 10, np.dtype(np.float64): 20}
NODE_BUDGET, WORK_BUDGET = 400_000, 45_000_000          # nodes x nDep, and x W, of one case's regions ((16, 16, 16): three)

Built = namedtuple("Built", "case order nCoef knots coefs c8 breaks lo_hi span")


def multiplicities(o):
    """Of the six breakpoints: clamped ends, a simple knot, a double knot (where the order allows), one of multiplicity
    o - 1 and one of multiplicity o (a discontinuity: the span index jumps by the order)."""
    return (o, 1, min(2, max(o - 1, 1)), max(o - 1, 1), o, o)


def domain_lo(case, i):
    salt = case.bucket // 4 + (case.nDep % 2)
    return DOMAIN_LO[(i + salt) % 3]


def axis(case, i):
    """(knots float64, breakpoints, span of each cell) of variable i."""
    o = case.orders[i]
    breaks = domain_lo(case, i) + np.concatenate(([0.0], np.cumsum(WIDTHS)))
    mult = multiplicities(o)
    knots = np.repeat(breaks, mult)
    span = np.cumsum(mult)[:5].astype(np.int32)
    return knots, breaks, span


def greville(knots, o):
    n = len(knots) - o
    return np.array([knots[k + 1:k + o].mean() if o > 1 else knots[k] for k in range(n)])


def coefficients8(case, knots):
    """8 x the coefficients, int64 (nDep, *nCoef): an affine map on the Greville abscissae, kept away from zero by its
    offset, in eighths, plus a perturbation of [-NOISE, NOISE] eighths.  The data of a case do not depend on its dtype."""
    n, ndep = case.nInd, case.nDep
    rng = rng_of("coef", case.nInd, case.orders, case.nDep, case.kind)
    g = np.meshgrid(*[greville(k, o) for k, o in zip(knots, case.orders)], indexing="ij")
    gmax = [np.abs(x).max() for x in g]

    def affine(row, sign):
        off = sign * (1.0 + sum(abs(a) * m for a, m in zip(row, gmax)))
        return np.rint(8 * SCALE * (sum(a * x for a, x in zip(row, g)) + off)).astype(np.int64)

    if case.kind == "line":
        ell = affine(rng.uniform(0.5, 1.0, n), 1.0) + rng.integers(-NOISE, NOISE + 1, g[0].shape)
        alpha, beta = (1, -2, 3, 2), (0, 5, -7, 11)
        return np.stack([alpha[d] * ell + 8 * SCALE * beta[d] for d in range(ndep)])
    A = np.where(np.arange(ndep)[:, None] < n, 0.25, 1.0) * rng.uniform(-1.0, 1.0, (ndep, n))
    for d in range(min(n, ndep)):
        A[d, d] += 1.0
    c8 = np.stack([affine(A[d], 1.0 if d % 2 == 0 else -1.0) for d in range(ndep)])
    c8 = c8 + rng.integers(-NOISE, NOISE + 1, c8.shape)
    if case.kind == "equal":
        c8[1] = c8[0]
    return c8


def region_boxes(case, breaks):
    """[(cells, lo_hi (nInd, 2))] in order of priority: the last cell, its deep child at the upper corner, the first
    cell, five regions through which every variable meets each of its cells (both sides of every multiple knot), and the
    2^nInd children of a cell between two multiple knots."""
    n = case.nInd
    depth = DEEP[np.dtype(case.dtype)]

    def box(cells):
        return np.array([[breaks[i][c], breaks[i][c + 1]] for i, c in enumerate(cells)])

    last, first = (4,) * n, (0,) * n
    deep = box(last)
    deep[:, 0] = deep[:, 1] - (deep[:, 1] - deep[:, 0]) * 2.0 ** -depth
    out = [(last, box(last)), (last, deep), (first, box(first))]
    out += [(cells, box(cells)) for cells in (tuple((r + i) % 5 for i in range(n)) for r in range(5))]
    parent = (2, 3, 1)[:n]
    b = box(parent)
    mid = b.mean(axis=1)
    for bits in itertools.product((0, 1), repeat=n):
        child = np.array([[mid[i], b[i, 1]] if bit else [b[i, 0], mid[i]] for i, bit in enumerate(bits)])
        out.append((parent, child))
    return out


def build(case):
    axes = [axis(case, i) for i in range(case.nInd)]
    knots = [a[0] for a in axes]
    c8 = coefficients8(case, knots)
    coefs = (c8.astype(np.float64) / 8.0).astype(case.dtype)
    boxes = region_boxes(case, [a[1] for a in axes])
    NN = GK_N ** case.nInd
    cap = min(NODE_BUDGET // (NN * case.nDep), WORK_BUDGET // (NN * case.nDep * staging(case.orders)[0]))
    boxes = boxes[:max(3, cap)]
    order = rng_of("regions", case.orders, case.nDep).permutation(len(boxes))
    lo_hi = np.stack([boxes[r][1] for r in order]).astype(case.dtype)
    span = np.array([[axes[i][2][c] for i, c in enumerate(boxes[r][0])] for r in order], np.int32)
    return Built(case, case.orders, tuple(len(k) - o for k, o in zip(knots, case.orders)), [k.astype(case.dtype) for k in knots],
                 coefs, c8, [a[1] for a in axes], lo_hi, span)


def spline_of(b, deps=None):
    """An object with the attributes tests/integral_ref.py and the oracle read; ``deps``: a slice of the dependents."""
    coefs = b.coefs if deps is None else np.ascontiguousarray(b.coefs[deps])
    return namedtuple("SplineLike", "nInd nDep order nCoef knots coefs")(len(b.order), coefs.shape[0], b.order, b.nCoef, b.knots, coefs)


def bitwise_dependents(case):
    """The first dependent, the last one of the first stage, the first and last of the second stage."""
    DG = staging(case.orders)[2]
    deps = {0, min(DG, case.nDep) - 1}
    if case.nDep > DG:
        deps |= {DG, min(2 * DG, case.nDep) - 1}
    return sorted(deps)


# ------------------------------------------------------------------------------------------ the reference
def node_parameters(lo_hi_r, dtype):
    """(nInd, 15) parameters of one region as the kernel forms them: fp64 from the bounds in T, then rounded to T."""
    lo, hi = lo_hi_r[:, 0].astype(np.float64), lo_hi_r[:, 1].astype(np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    prod = half[:, None] * GK_X[None, :]
    return (mid[:, None] + prod).astype(dtype)


def basis(knots, o, ix, u, wrt, zero, absolute=False):
    """(len(u), o) basis of derivative order wrt at the parameters u of the cell with span index ix, in the arithmetic of
    ``zero`` (np.longdouble(0) or Fraction(0)): the recursion of bspy/_spline_evaluation.py:4-27 with true divisions.
    absolute: both terms of a derivative level are added (the sum of the absolute values of its terms)."""
    one = zero + 1
    b = np.full((len(u), o), zero, dtype=object if isinstance(zero, Fraction) else LD)
    if wrt >= o:
        return b
    b[:, o - 1] = one
    for degree in range(1, o):
        for j in range(degree):
            i, bi = ix - degree + j, o - degree + j
            den = knots[i + degree] - knots[i]
            if degree < o - wrt:
                alpha = (u - knots[i]) / den
                b[:, bi - 1] = b[:, bi - 1] + (one - alpha) * b[:, bi]
            else:
                alpha = (zero + degree) / den
                b[:, bi - 1] = b[:, bi - 1] + alpha * b[:, bi] if absolute else b[:, bi - 1] - alpha * b[:, bi]
            b[:, bi] = b[:, bi] * alpha
    return b


def contract(c, mats):
    """out[d, j0, j1, ...] = sum_k c[d, k0, k1, ...] prod_i mats[i][j_i, k_i], last variable first."""
    out = c
    for m in reversed(mats):
        out = np.moveaxis(np.tensordot(out, m, axes=([out.ndim - 1], [1])), -1, 1)
    return out


def window(array, b, r):
    return array[(slice(None),) + tuple(slice(int(s) - o, int(s)) for s, o in zip(b.span[r], b.order))]


def values_and_jacobian(b, r, zero, nodes=None, deps=None):
    """x (nDep, N...) and J (nInd, nDep, N...) of region r in the arithmetic of ``zero``, N... = 15 per variable or the
    axis nodes ``nodes``; with longdouble also the sums of absolute values Sx, SJ and the second derivatives H[i][j]."""
    exact = isinstance(zero, Fraction)
    n = len(b.order)
    u = node_parameters(b.lo_hi[r], b.case.dtype)
    if nodes is not None:
        u = u[:, nodes]
    conv = (lambda a: np.array([Fraction(float(v)) for v in a], object)) if exact else (lambda a: np.asarray(a, np.float64).astype(LD))
    c8 = window(b.c8, b, r)
    if deps is not None:
        c8 = c8[deps]
    c = np.vectorize(lambda v: Fraction(int(v), 8), otypes=[object])(c8) if exact else c8.astype(LD) / LD(8)
    ks = [conv(k) for k in b.knots]
    us = [conv(u[i]) for i in range(n)]
    V = [basis(ks[i], b.order[i], int(b.span[r, i]), us[i], 0, zero) for i in range(n)]
    D = [basis(ks[i], b.order[i], int(b.span[r, i]), us[i], 1, zero) for i in range(n)]

    def with_(mats, i, m):
        return mats[:i] + [m] + mats[i + 1:]

    x = contract(c, V)
    J = [contract(c, with_(V, i, D[i])) for i in range(n)]
    if exact:
        return x, J
    A = [basis(ks[i], b.order[i], int(b.span[r, i]), us[i], 1, zero, absolute=True) for i in range(n)]
    DD = [basis(ks[i], b.order[i], int(b.span[r, i]), us[i], 2, zero) for i in range(n)]
    ca = np.abs(c)
    Sx = contract(ca, V)
    SJ = [contract(ca, with_(V, i, A[i])) for i in range(n)]
    H = [[contract(c, with_(V, i, DD[i]) if i == j else with_(with_(V, i, D[i]), j, D[j])) for j in range(n)] for i in range(n)]
    return u, x, J, Sx, SJ, H


N_DET = {1: 0, 2: 2, 3: 5}


def det_with_bar(M, dM, unit):
    """Determinant of M (m, m, N) and its first-order bar from the entries' bars dM and the roundings of the expansion, on
    the sum of the absolute values of the expansion terms."""
    m = M.shape[0]
    aM = np.abs(M)
    det, absdet, bar = 0, 0, 0
    for perm in itertools.permutations(range(m)):
        sign = (-1) ** sum(perm[a] > perm[b] for a in range(m) for b in range(a + 1, m))
        term, aterm = 1, 1
        for a in range(m):
            term = term * M[a, perm[a]]
            aterm = aterm * aM[a, perm[a]]
        det, absdet = det + sign * term, absdet + aterm
        for a in range(m):
            rest = 1
            for a2 in range(m):
                if a2 != a:
                    rest = rest * aM[a2, perm[a2]]
            bar = bar + dM[a, perm[a]] * rest
    return det, bar + gamma(N_DET[m], unit) * absdet


def measure_with_bar(J, dJ, unit):
    """mu (N,) and its bar from J, dJ (nInd, nDep, N)."""
    n, ndep = J.shape[:2]
    if ndep == n:
        det, bar = det_with_bar(np.swapaxes(J, 0, 1), np.swapaxes(dJ, 0, 1), unit)
        return np.abs(det), bar
    V, dV = (J, dJ) if ndep > n else (np.swapaxes(J, 0, 1), np.swapaxes(dJ, 0, 1))        # the vectors of the Gram matrix
    aV = np.abs(V)
    terms = V.shape[1]
    G = np.einsum("adn,bdn->abn", V, V)
    dG = np.einsum("adn,bdn->abn", aV, dV) + np.einsum("adn,bdn->abn", dV, aV) + gamma(terms, unit) * np.einsum("adn,bdn->abn", aV, aV)
    det, d = det_with_bar(G, dG, unit)
    mu = np.sqrt(np.maximum(det, 0))
    below = mu * mu <= d
    root = np.sqrt(np.where(below, 0, mu * mu - d))
    bar = np.where(below, np.sqrt(d), d / np.where(below, 1, mu + root))              # = mu - sqrt(mu^2 - d), without cancellation
    return mu, bar + unit * (mu + bar)


def fsum_ld(a):
    """math.fsum of longdoubles through their high and low doubles."""
    hi = np.asarray(a, LD).astype(np.float64)
    lo = (np.asarray(a, LD) - hi.astype(LD)).astype(np.float64)
    return math.fsum(np.concatenate((hi.ravel(), lo.ravel())))


def sum_factor(nind):
    NN, BLOCK = GK_N ** nind, block_of(nind)
    return (-(-NN // BLOCK) + 6 + BLOCK // 64 + 1) * 2.0 ** -53


Ref = namedtuple("Ref", "u x bar_x J bar_J mu bar_mu fk bar_fk fg bar_fg K G bar_K bar_G norms")


def reference(b):
    """Per region r: u (nInd, 15) in T; x, bar_x (NN, nDep); J, bar_J (NN, nDep, nInd); mu, fk = wK mu, fg = wG mu and their
    bars (NN,), all longdouble; K, G (floats) and their bars against the reference; norms: prod ||v|| of the precondition."""
    case = b.case
    n, ndep, unit = case.nInd, case.nDep, unit_of(case.dtype)
    n_x = sum(6 * (o - 1) + o + 1 for o in b.order)
    n_J = n_x - 2
    jgrid = np.indices((GK_N,) * n).reshape(n, -1)
    rows = []
    for r in range(len(b.lo_hi)):
        u, x, J, Sx, SJ, H = values_and_jacobian(b, r, LD(0))
        ulp = [np.spacing(np.abs(u[i])).astype(LD)[jgrid[i]] for i in range(n)]                     # (NN,) per variable
        flat = lambda a: a.reshape(ndep, -1)
        x, Sx, J, SJ = flat(x), flat(Sx), np.stack([flat(a) for a in J]), np.stack([flat(a) for a in SJ])
        bar_x = gamma(n_x, unit) * Sx + sum(np.abs(J[i]) * ulp[i] for i in range(n))
        bar_J = np.stack([gamma(n_J, unit) * SJ[i] + sum(np.abs(flat(H[i][j])) * ulp[j] for j in range(n)) for i in range(n)])
        mu, bar_mu = measure_with_bar(J, bar_J, unit)
        lo, hi = b.lo_hi[r, :, 0].astype(np.float64).astype(LD), b.lo_hi[r, :, 1].astype(np.float64).astype(LD)
        vol = np.prod(LD(0.5) * (hi - lo))
        wk = vol * np.prod(GK_WK.astype(LD)[jgrid], axis=0)
        wg = vol * np.prod(GK_WG.astype(LD)[jgrid], axis=0)
        wbar = (2 * n + 1) * 2.0 ** -53
        fk, fg = wk * mu, wg * mu
        bar_fk, bar_fg = wk * bar_mu + wbar * fk, wg * bar_mu + wbar * fg
        V = J if ndep >= n else np.swapaxes(J, 0, 1)
        norms = np.prod(np.sqrt(np.sum(V * V, axis=1)), axis=0)
        K, G = fsum_ld(fk), fsum_ld(fg)
        bar_K = fsum_ld(bar_fk) + sum_factor(n) * K
        bar_G = fsum_ld(bar_fg) + sum_factor(n) * G
        rows.append((u, x.T, bar_x.T, np.moveaxis(J, 0, -1).transpose(1, 0, 2), np.moveaxis(bar_J, 0, -1).transpose(1, 0, 2), mu, bar_mu,
                     fk, bar_fk, fg, bar_fg, K, G, bar_K, bar_G, norms))
    return Ref(*[np.stack(col) if isinstance(col[0], np.ndarray) else np.array(col) for col in zip(*rows)])


# ------------------------------------------------------------------------------------------ comparisons
def ratio(got, want, bar):
    """max |got - want| / bar in longdouble; 0 where the error is 0, inf where only the bar is."""
    err = np.abs(np.asarray(got, np.float64).astype(LD) - np.asarray(want, LD))
    bar = np.asarray(bar, LD) + LD(0) * err
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, LD(0), np.where(bar > 0, err / np.where(bar > 0, bar, 1), LD(np.inf)))
    q = np.where(np.isfinite(err), q, LD(np.inf))
    return float(np.max(q)) if q.size else 0.0


def node_ratios(ref, nodes):
    """Worst |error| / bar of a NODES result (R, NN, nDep + 2) in x, wK mu (label mu) and wG mu (label muG)."""
    return {"x": ratio(nodes[:, :, :-2], ref.x, ref.bar_x), "mu": ratio(nodes[:, :, -2], ref.fk, ref.bar_fk),
            "muG": ratio(nodes[:, :, -1], ref.fg, ref.bar_fg)}


def measure_ratios(ref, sums):
    """Worst |error| / bar of a MEASURE result (R, 2) against the reference."""
    return {"K": ratio(sums[:, 0], ref.K, ref.bar_K), "G": ratio(sums[:, 1], ref.G, ref.bar_G)}


def measure_against_nodes(nind, sums, nodes):
    """Worst |error| / bar of a MEASURE result against math.fsum of the same call's NODES columns (K, G)."""
    out = []
    for col, k in ((-2, 0), (-1, 1)):
        want = np.array([math.fsum(nodes[r, :, col]) for r in range(len(nodes))])
        bar = sum_factor(nind) * np.array([math.fsum(np.abs(nodes[r, :, col])) for r in range(len(nodes))])
        out.append(ratio(sums[:, k], want, bar))
    return {"K": out[0], "G": out[1]}


def bits(a):
    return np.ascontiguousarray(a).tobytes()
