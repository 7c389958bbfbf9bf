"""
Certified closest points on curves and surfaces, for the project tests: plain Python with ``fractions.Fraction``; the
only code shared with anything is the exact Bezier extraction and the certified zero finders of zeros_ref.py and
zeros2_ref.py.  This file decides where the closest point of a case is and how far away.

A float is a rational number, so on every knot cell the Bernstein coefficients of S are rational, and so are those of
D = |S - p|^2 and of the critical-point polynomials F_a = (S - p) . dS/dx_a (``bmul``: exact products of Bernstein
forms).  All coordinates below are cell-local, in [0, 1], until ``closest`` maps them.

Candidates for the global minimiser of D over the domain, complete whatever the smoothness of S:
  * the critical points inside every cell: curves by ``zeros_ref.isolate`` on F (every bracket holds exactly one simple
    root; it is bisected exactly to 2^-80), surfaces by ``zeros2_ref.solve_cell`` on (F_0, F_1) raised to one common
    degree (every certificate holds exactly one zero, within ``zeros2_ref.error_bound`` of the proposal);
  * for surfaces the critical points of D along every cell edge (the same curve routine on the edge's coefficients);
  * every cell corner (for curves: every break), where D is evaluated exactly.
Every candidate carries an enclosure [lo, hi] of D over its box: the smallest and largest Bernstein coefficient of D
restricted to the box, exactly.  The global minimiser is the candidate with the smallest hi; it is CERTIFIED unique when
every other candidate's lo exceeds that hi, and ``gap`` is the difference.  A multiple critical point, a critical point
on a cell edge or a constant D raise ``ArithmeticError``: the cases avoid such points.
"""
from fractions import Fraction
from math import comb

import numpy as np

import zeros2_ref
import zeros_ref

WIDTH = Fraction(1, 2 ** 80)


# ------------------------------------------------------------------------------------------ exact Bernstein algebra
def bmul(a, b):
    """The Bernstein coefficients of the product of two Bernstein forms on the same interval."""
    m, n = len(a) - 1, len(b) - 1
    out = [Fraction(0)] * (m + n + 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += Fraction(comb(m, i) * comb(n, j), comb(m + n, i + j)) * x * y
    return out


def elevate(c):
    n = len(c)
    return [Fraction(i, n) * (c[i - 1] if i else 0) + (1 - Fraction(i, n)) * (c[i] if i < n else 0) for i in range(n + 1)]


def bmul2(A, B):
    """The same for tensor-product forms (lists of rows)."""
    m0, m1, n0, n1 = len(A) - 1, len(A[0]) - 1, len(B) - 1, len(B[0]) - 1
    out = [[Fraction(0)] * (m1 + n1 + 1) for _ in range(m0 + n0 + 1)]
    for i in range(m0 + 1):
        for p in range(n0 + 1):
            w0 = Fraction(comb(m0, i) * comb(n0, p), comb(m0 + n0, i + p))
            for j in range(m1 + 1):
                for q in range(n1 + 1):
                    out[i + p][j + q] += w0 * Fraction(comb(m1, j) * comb(n1, q), comb(m1 + n1, j + q)) * A[i][j] * B[p][q]
    return out


def add2(A, B):
    return [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(A, B)]


def diff(c):
    n = len(c) - 1
    return [n * (c[i + 1] - c[i]) for i in range(n)]


# ------------------------------------------------------------------------------------------ one span of a curve
def line_candidates(comps, p):
    """comps: per component the K exact Bernstein coefficients of one span; p: the point (Fractions).
    -> [(xlo, xhi, dlo, dhi)]: both ends and every critical point of D inside (0, 1)."""
    R = [[c - pd for c in comp] for comp, pd in zip(comps, p)]
    D = [sum(col) for col in zip(*[bmul(r, r) for r in R])]
    out = [(Fraction(0), Fraction(0), D[0], D[0]), (Fraction(1), Fraction(1), D[-1], D[-1])]
    if len(comps[0]) < 2:
        return out
    F = [sum(col) for col in zip(*[bmul(r, diff(r)) for r in R])]
    if not any(F):
        raise ArithmeticError("the distance is constant along a span")
    for lo, hi in zeros_ref.isolate(F, True):
        if lo in (0, 1) and lo == hi:
            continue
        if lo < hi:
            lo, hi = zeros_ref.shrink(F, lo, hi, WIDTH)
        on = zeros_ref.restrict(D, lo, hi)
        out.append((lo, hi, min(on), max(on)))
    return out


def curve_cells(order, knots, coefs):
    """(breaks, [per span: per component K Fractions])."""
    per = [zeros_ref.bezier_spans(order, knots, comp) for comp in np.asarray(coefs)]
    breaks = [s[0] for s in per[0]] + [per[0][-1][1]]
    return breaks, [[per[d][s][2] for d in range(len(per))] for s in range(len(per[0]))]


def surface_cells(order, knots, coefs):
    """(breaks0, breaks1, cells[i][j][d] = K0 rows of K1 Fractions): zeros2_ref.bezier_cells for any nDep."""
    coefs = np.asarray(coefs)
    breaks0 = breaks1 = None
    cells = None
    for d in range(0, coefs.shape[0], 2):
        pair = coefs[d:d + 2] if d + 2 <= coefs.shape[0] else np.stack([coefs[d], coefs[d]])
        breaks0, breaks1, part = zeros2_ref.bezier_cells(order, knots, pair)
        take = 2 if d + 2 <= coefs.shape[0] else 1
        if cells is None:
            cells = [[[] for _ in line] for line in part]
        for i, line in enumerate(part):
            for j, cell in enumerate(line):
                cells[i][j].extend(cell[:take])
    return breaks0, breaks1, cells


def interior_candidates(comps, p):
    """comps: per component K0 rows of K1 Fractions.  -> [(xlo, xhi, ylo, yhi, dlo, dhi)] of the critical points inside."""
    R = [[[v - pd for v in row] for row in comp] for comp, pd in zip(comps, p)]
    D = None
    F = [None, None]
    for r in R:
        sq = bmul2(r, r)
        D = sq if D is None else add2(D, sq)
        dx, dy = zeros2_ref.derivatives(r)
        parts = [bmul2(r, dx), bmul2(r, dy)]
        parts[0] = zeros2_ref.columns([elevate(col) for col in zeros2_ref.columns(parts[0])])
        parts[1] = [elevate(row) for row in parts[1]]
        F = [part if f is None else add2(f, part) for f, part in zip(F, parts)]
    out = []
    for cert in zeros2_ref.solve_cell(F):
        x, y = cert["x"], cert["y"]
        r = zeros2_ref.error_bound(F, cert, x, y)
        box = (max(Fraction(0), x - r), min(Fraction(1), x + r), max(Fraction(0), y - r), min(Fraction(1), y + r))
        on = [v for row in zeros2_ref.restrict2(D, *box) for v in row]
        out.append(box + (min(on), max(on)))
    return out


# ------------------------------------------------------------------------------------------ the minimiser
def _pick(cands):
    """cands: [dict(u=[(lo, hi)] per axis, d=(lo, hi), free=...)], duplicates of exact points removed.  -> (best, gap)."""
    seen, unique = set(), []
    for c in cands:
        key = tuple(c["u"])
        if all(lo == hi for lo, hi in c["u"]):
            if key in seen:
                continue
            seen.add(key)
        unique.append(c)
    unique.sort(key=lambda c: c["d"][1])
    best = unique[0]
    gap = min((c["d"][0] for c in unique[1:]), default=None)
    return best, (None if gap is None else gap - best["d"][1])


def closest(order, knots, coefs, point):
    """The certified global minimiser of |S - p|^2 over the domain.  Returns dict(u: per axis (lo, hi) Fractions in the
    spline's parameters, d: (lo, hi) of the squared distance, free: per axis whether the minimiser is a critical point
    along it (False: it sits on a domain bound, or ``None`` for a minimiser on an interior knot line), gap: the
    runner-up's lo minus d's hi (not positive: the minimiser is not certified unique), cell: its cell index per axis)."""
    p = [Fraction(float(v)) for v in point]
    nind = len(order)
    cands = []
    if nind == 1:
        breaks, cells = curve_cells(order[0], knots[0], coefs)
        for s, comps in enumerate(cells):
            t0, h = breaks[s], breaks[s + 1] - breaks[s]
            for xlo, xhi, dlo, dhi in line_candidates(comps, p):
                u = (t0 + xlo * h, t0 + xhi * h)
                if xlo == xhi and xlo in (0, 1):
                    free = [False] if u[0] in (breaks[0], breaks[-1]) else [None]
                else:
                    free = [True]
                cands.append(dict(u=[u], d=(dlo, dhi), free=free, cell=[s]))
    else:
        breaks0, breaks1, cells = surface_cells(order, knots, coefs)
        ends = ((breaks0[0], breaks0[-1]), (breaks1[0], breaks1[-1]))
        for i, line in enumerate(cells):
            for j, comps in enumerate(line):
                t0, h = (breaks0[i], breaks1[j]), (breaks0[i + 1] - breaks0[i], breaks1[j + 1] - breaks1[j])
                for xlo, xhi, ylo, yhi, dlo, dhi in interior_candidates(comps, p):
                    cands.append(dict(u=[(t0[0] + xlo * h[0], t0[0] + xhi * h[0]), (t0[1] + ylo * h[1], t0[1] + yhi * h[1])],
                                      d=(dlo, dhi), free=[True, True], cell=[i, j]))
                edges = [(0, 0), (1, 0)] + ([(0, 1)] if i == len(cells) - 1 else []) + ([(1, 1)] if j == len(line) - 1 else [])
                for axis, side in edges:                        # the edge on which `axis` is fixed at `side`
                    if axis == 0:
                        along = [comp[-1 if side else 0] for comp in comps]
                    else:
                        along = [[row[-1 if side else 0] for row in comp] for comp in comps]
                    fixed = t0[axis] + side * h[axis]
                    for xlo, xhi, dlo, dhi in line_candidates(along, p):
                        other = 1 - axis
                        run = (t0[other] + xlo * h[other], t0[other] + xhi * h[other])
                        u = [None, None]
                        u[axis], u[other] = (fixed, fixed), run
                        free = [None, None]
                        free[axis] = False if fixed in ends[axis] else None
                        if xlo == xhi and xlo in (0, 1):
                            free[other] = False if run[0] in ends[other] else None
                        else:
                            free[other] = True
                        cands.append(dict(u=u, d=(dlo, dhi), free=free, cell=[i, j]))
    best, gap = _pick(cands)
    return dict(best, gap=gap)


def derivatives_at(order, knots, coefs, best):
    """Exact first and second derivatives of S in the spline's parameters at the centre of the minimiser's box:
    (S (nDep), J (nDep x nInd), H (nDep x nInd x nInd)) as Fractions."""
    nind = len(order)
    mid = [(lo + hi) / 2 for lo, hi in best["u"]]
    if nind == 1:
        breaks, cells = curve_cells(order[0], knots[0], coefs)
        s = best["cell"][0]
        h = breaks[s + 1] - breaks[s]
        x = (mid[0] - breaks[s]) / h
        S, J, H = [], [], []
        for comp in cells[s]:
            d1 = diff(comp)
            d2 = diff(d1) if len(d1) > 1 else [Fraction(0)]
            S.append(zeros_ref.span_value(comp, x))
            J.append([zeros_ref.span_value(d1, x) / h])
            H.append([[zeros_ref.span_value(d2, x) / h / h]])
        return S, J, H
    breaks0, breaks1, cells = surface_cells(order, knots, coefs)
    i, j = best["cell"]
    h = (breaks0[i + 1] - breaks0[i], breaks1[j + 1] - breaks1[j])
    x, y = (mid[0] - breaks0[i]) / h[0], (mid[1] - breaks1[j]) / h[1]

    def val(part):
        return zeros2_ref.value2(part, x, y) if part and part[0] else Fraction(0)

    S, J, H = [], [], []
    for comp in cells[i][j]:
        dx, dy = zeros2_ref.derivatives(comp)
        dxx, dxy = zeros2_ref.derivatives(dx) if dx and dx[0] else ([], [])
        dyy = zeros2_ref.derivatives(dy)[1] if dy and dy[0] else []
        S.append(zeros2_ref.value2(comp, x, y))
        J.append([val(dx) / h[0], val(dy) / h[1]])
        H.append([[val(dxx) / h[0] / h[0], val(dxy) / h[0] / h[1]], [val(dxy) / h[0] / h[1], val(dyy) / h[1] / h[1]]])
    return S, J, H


def point(order, knots, coefs, u):
    """(S, J, H) of ``derivatives_at`` at the parameters u (floats inside the domain)."""
    cell = []
    for k, t, x in zip(order, knots, u):
        tf = sorted(set(Fraction(float(v)) for v in np.asarray(t)[k - 1:len(t) - k + 1]))
        cell.append(max(0, max(i for i, v in enumerate(tf[:-1]) if v <= Fraction(float(x)))))
    return derivatives_at(order, knots, coefs, dict(u=[(Fraction(float(x)), Fraction(float(x))) for x in u], cell=cell))
