"""
Exact reference for knot removal (tests/test_remove_host.py, tests/test_gpu_remove.py, tests/golden/make_golden_remove.py):
rational arithmetic on the float inputs, no floating-point operation before the final rounding.

Removing knot i of a curve of order k: the k new coefficients x[0 .. k - 1] (new indices i - k .. i - 1) would have to
satisfy the k + 1 equations of re-inserting the knot,

    d1[r] x[r] + d0[r - 1] x[r - 1] = c[i - k + r],   r = 0 .. k,
    d1[0] = 1, d1[r] = 1 - alpha_r, d0[r - 1] = alpha_r (0 < r < k), d1[k] = 0, d0[k - 1] = 1,
    alpha_r = (t[i + r] - t[i]) / (t[i + r] - t[i + r - k]).

The first eL = max(0, nLeft - i + k) unknowns are fixed by the equations 0 .. eL - 1 (forward substitution), the last
eR = max(0, nRight - nCoef + i + 1) by the equations k .. k - eR + 1 (backward substitution); the others are the
least-squares solution of the remaining equations eL .. k - eR (normal equations, solved exactly).  The squared residual
is the sum of squares of those equations' defects.

``on_knots`` expresses coefficients on a refined knot vector by exact knot insertion (tests/refine_ref.py).
"""
from fractions import Fraction

import numpy as np

import refine_ref


def _fr(x):
    return Fraction(float(x))


def _solve(A, b):
    """Exact solution of the square system A x = b (lists of Fractions) by Gaussian elimination."""
    n = len(A)
    M = [row[:] + [rhs] for row, rhs in zip(A, b)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c] / M[c][c]
                M[r] = [a - f * p for a, p in zip(M[r], M[c])]
    return [M[r][n] / M[r][r] for r in range(n)]


def system(knots, order, iKnot):
    """(d0, d1): the two diagonals of the (k + 1) x k system as Fractions."""
    k = order
    t = [_fr(v) for v in knots]
    d0, d1 = [], [Fraction(1)]
    for r in range(1, k):
        alpha = (t[iKnot + r] - t[iKnot]) / (t[iKnot + r] - t[iKnot + r - k])
        d0.append(alpha)
        d1.append(1 - alpha)
    d0.append(Fraction(1))
    d1.append(Fraction(0))
    return d0, d1


def solve_window(knots, order, iKnot, c, nLeft=0, nRight=0):
    """c: the k + 1 old coefficients (Fractions) of the window.  Returns (x, squared residual)."""
    k = order
    nCoef = len(knots) - k
    d0, d1 = system(knots, k, iKnot)
    eL = max(0, nLeft - iKnot + k)
    eR = max(0, nRight - nCoef + iKnot + 1)
    x = [None] * k
    for r in range(eL):
        x[r] = (c[r] - (d0[r - 1] * x[r - 1] if r else 0)) / d1[r]
    for s in range(eR):
        r = k - s                                        # equation r fixes unknown r - 1
        x[r - 1] = (c[r] - (d1[r] * x[r] if r < k else 0)) / d0[r - 1]
    free = list(range(eL, k - eR))
    eqs = list(range(eL, k - eR + 1))
    # equation r: d1[r] x[r] + d0[r - 1] x[r - 1] = c[r]; known unknowns go to the right-hand side
    rows, rhs = [], []
    for r in eqs:
        row = [Fraction(0)] * len(free)
        b = c[r]
        for u, coef in ((r, d1[r] if r < k else None), (r - 1, d0[r - 1] if r > 0 else None)):
            if coef is None or u < 0 or u >= k:
                continue
            if x[u] is not None:
                b = b - coef * x[u]
            else:
                row[free.index(u)] = coef
        rows.append(row)
        rhs.append(b)
    if free:
        n = len(free)
        AtA = [[sum(rows[e][a] * rows[e][b] for e in range(len(rows))) for b in range(n)] for a in range(n)]
        Atb = [sum(rows[e][a] * rhs[e] for e in range(len(rows))) for a in range(n)]
        for u, value in zip(free, _solve(AtA, Atb)):
            x[u] = value
    res2 = Fraction(0)
    for row, b in zip(rows, rhs):
        defect = b - sum(coef * x[u] for coef, u in zip(row, free))
        res2 += defect * defect
    return x, res2


def removal_rows(knots, order, iKnot, nLeft=0, nRight=0):
    """The exact operator: W[r][s] = weight of old coefficient iKnot - k + s in new coefficient iKnot - k + r."""
    k = order
    cols = []
    for s in range(k + 1):
        unit = [Fraction(int(q == s)) for q in range(k + 1)]
        cols.append(solve_window(knots, k, iKnot, unit, nLeft, nRight)[0])
    return [[cols[s][r] for s in range(k + 1)] for r in range(k)]


def remove_knot(knots, order, coefs, iKnot, nLeft=0, nRight=0):
    """coefs: float array (nDep, nCoef).  Returns (exact new coefficients: object array (nDep, nCoef - 1) of Fractions,
    squared residuals: list of nDep Fractions)."""
    k = order
    exact = refine_ref.to_exact(np.asarray(coefs))
    out = np.empty((exact.shape[0], exact.shape[1] - 1), object)
    res2 = []
    for d in range(exact.shape[0]):
        x, r2 = solve_window(knots, k, iKnot, list(exact[d, iKnot - k:iKnot + 1]), nLeft, nRight)
        out[d, :iKnot - k] = exact[d, :iKnot - k]
        out[d, iKnot - k:iKnot] = x
        out[d, iKnot:] = exact[d, iKnot + 1:]
        res2.append(r2)
    return out, res2


def on_knots(order, knots, coefs, newKnots):
    """Exact coefficients (object array of Fractions) of the spline (order, knots, float coefs (nDep, *nCoef)) on the
    refined knot vectors newKnots, by exact knot insertion per variable."""
    exact = refine_ref.to_exact(np.asarray(coefs))
    for iv, (k, t, t2) in enumerate(zip(order, knots, newKnots)):
        if len(t) == len(t2) and np.array_equal(np.asarray(t, np.float64), np.asarray(t2, np.float64)):
            continue
        exact, exists = refine_ref.apply_rows(refine_ref.refine_rows(t, k, t2, 0), exact, iv + 1)
        assert exists.all()
    return exact


def certified_error(order, knots, coefs, newKnots, newCoefs):
    """E_d = max |coefs - (newCoefs expressed on knots)| per dependent variable, exact, returned as floats."""
    back = on_knots(order, newKnots, newCoefs, knots)
    diff = refine_ref.to_exact(np.asarray(coefs)) - back
    return np.array([float(max(abs(v) for v in diff[d].ravel())) for d in range(diff.shape[0])])
