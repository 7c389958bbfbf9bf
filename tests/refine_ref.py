"""
Exact change of basis between B-spline knot vectors, for the refinement tests: plain Python / NumPy with
``fractions.Fraction``, no code shared with bspy_amd.

A float is a rational number, so the coefficients of the same function on other knots (finer, of higher order, or
covering a smaller domain) are rational too and are computed here without rounding; ``to_float`` rounds the result once.

    new coefficient j = F(tbar[j + 1], ..., tbar[j + k + m - 1])

where F is the blossom (polar form) of the polynomial piece on any non-empty cell of the support of new basis function j,
seen as a polynomial of degree k + m - 1: the mean over the (k - 1)-subsets of the arguments of the piece's own blossom,
which the de Boor recurrence with one argument per level evaluates from the old coefficients.  The cell used here is the
lowest non-empty new cell of the support that lies inside the old domain.  A new basis function without such a cell
("outside" row: it has no influence on any value inside the domain) gets no value: ``refine_rows`` returns None for
it, and ``change_basis`` returns the mask of the entries that exist.
"""
from fractions import Fraction
from itertools import combinations

import numpy as np


def _fr(a):
    return [Fraction(float(v)) for v in np.asarray(a).ravel()]


def _blossom_row(t, k, mu, args):
    """Weights (Fractions, on old coefficients mu - k + 1 .. mu) of the blossom of the piece on cell mu at args (k - 1 values)."""
    d = [[Fraction(int(p == q)) for q in range(k)] for p in range(k)]
    for r, u in enumerate(args, start=1):
        nxt = [None] * k
        for p in range(r, k):
            i = mu - k + 1 + p
            a = (u - t[i]) / (t[i + k - r] - t[i])
            nxt[p] = [(1 - a) * x + a * y for x, y in zip(d[p - 1], d[p])]
        d = nxt
    return d[k - 1]


def refine_rows(knots, order, newKnots, m=0):
    """[(first, weights) or None per new coefficient]: exact rows of the operator old knots -> new knots, order + m."""
    t, tb = _fr(knots), _fr(newKnots)
    k = int(order)
    n = k + m - 1
    nIn, nOut = len(t) - k, len(tb) - k - m
    lo, hi = t[k - 1], t[nIn]
    rows = []
    for j in range(nOut):
        mu = None
        for cell in range(j, j + n + 1):
            if tb[cell + 1] > tb[cell] and tb[cell] >= lo and tb[cell + 1] <= hi:
                mid = (tb[cell] + tb[cell + 1]) / 2
                mu = max(i for i in range(k - 1, nIn) if t[i] <= mid)
                assert t[mu] <= tb[cell] and tb[cell + 1] <= t[mu + 1], "the new knots do not refine the old ones"
                break
        if mu is None:
            rows.append(None)
            continue
        args = tb[j + 1:j + 1 + n]
        total = [Fraction(0)] * k
        count = 0
        for subset in combinations(range(n), k - 1):
            wrow = _blossom_row(t, k, mu, [args[a] for a in subset])
            total = [x + y for x, y in zip(total, wrow)]
            count += 1
        rows.append((mu - k + 1, [x / count for x in total]))
    return rows


def differentiate_rows(knots, order):
    t = _fr(knots)
    k = int(order)
    rows = []
    for j in range(len(t) - k - 1):
        alpha = Fraction(k - 1) / (t[j + k] - t[j + 1])
        rows.append((j, [-alpha, alpha]))
    return rows


def to_exact(coefs):
    """Object array of Fractions equal to the float array."""
    a = np.asarray(coefs)
    out = np.empty(a.shape, object)
    out.ravel()[:] = _fr(a)
    return out


def apply_rows(rows, exact, axis):
    """Apply the rows along ``axis`` of an object array of Fractions.  Returns the result (outside rows hold zeros) and
    the mask, along that axis, of the rows that exist."""
    moved = np.moveaxis(exact, axis, 0)
    out = np.empty((len(rows),) + moved.shape[1:], object)
    exists = np.ones(len(rows), bool)
    for j, row in enumerate(rows):
        if row is None:
            out[j] = Fraction(0)
            exists[j] = False
            continue
        first, w = row
        acc = w[0] * moved[first]
        for s in range(1, len(w)):
            acc = acc + w[s] * moved[first + s]
        out[j] = acc
    return np.moveaxis(out, 0, axis), exists


def to_float(exact, dtype=np.float64):
    """Round once: Fraction -> float64 is correctly rounded; float32 goes through float64 (the double rounding is
    far below the tests' resolution)."""
    vals = np.array([float(v) for v in exact.ravel()], np.float64).reshape(exact.shape)
    return vals.astype(dtype)


def change_basis(order, knots, coefs, newOrder, newKnots):
    """Exact coefficients of the spline (order, knots, coefs of shape (nDep, *nCoef)) on newKnots with orders newOrder,
    rounded once to the coefficients' dtype, and the mask (same shape) of the entries that exist: an entry does not
    exist when, in some variable, its basis function has no cell inside the old domain."""
    coefs = np.asarray(coefs)
    exact = to_exact(coefs)
    masks = []
    for iv, (k, t, k2, t2) in enumerate(zip(order, knots, newOrder, newKnots)):
        same = k == k2 and len(t) == len(t2) and np.array_equal(np.asarray(t, np.float64), np.asarray(t2, np.float64))
        if same:
            masks.append(np.ones(len(t) - k, bool))
            continue
        exact, exists = apply_rows(refine_rows(t, k, t2, k2 - k), exact, iv + 1)
        masks.append(exists)
    mask = np.ones(exact.shape, bool)
    for iv, e in enumerate(masks):
        shape = [1] * exact.ndim
        shape[iv + 1] = len(e)
        mask &= e.reshape(shape)
    return to_float(exact, coefs.dtype), mask


def differentiate(order, knots, coefs, with_respect_to):
    """Exact coefficients of the derivative spline, rounded once to the coefficients' dtype."""
    coefs = np.asarray(coefs)
    rows = differentiate_rows(knots[with_respect_to], order[with_respect_to])
    exact, _ = apply_rows(rows, to_exact(coefs), with_respect_to + 1)
    return to_float(exact, coefs.dtype)
