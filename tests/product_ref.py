"""
Exact products of B-splines, for the product tests: plain Python / NumPy with ``fractions.Fraction``, no code shared with
bspy_amd (the float-to-rational helpers come from tests/refine_ref.py).

For one pair of mapped variables (orders k1, k2, knots t, s) the product has order p = k1 + k2 - 1 on the knots tbar, and

    coefficient j = (F G)*(tbar[j + 1], ..., tbar[j + p - 1])

the blossom of the product of the two polynomial pieces on any non-empty cell of the support of basis function j.  The
blossom of a product is the mean over the (k1 - 1)-subsets S of the arguments of F*(S) G*(complement of S), and each
factor's blossom is a row of weights on its own coefficients (the de Boor recurrence with one argument per level, as
refine_ref._blossom_row, here in integers).  So coefficient j is a bilinear
form W[j][a][b] on A[f + a], B[g + b] with rational weights: ``product_rows`` returns them, ``multiply`` contracts the
exact outer product of the two coefficient tensors with the rows of every mapped variable and rounds once.
The cell used here is the LOWEST non-empty cell of the support (the library takes the one nearest the middle: the exact
result does not depend on the choice).
"""
from fractions import Fraction
from itertools import combinations

import numpy as np

from refine_ref import _fr, to_exact, to_float


def _cell(t, k, n_in, mid):
    return max(i for i in range(k - 1, n_in) if t[i] <= mid)


def _scaled_knots(*knot_vectors):
    """The knot vectors as Python integers over one common power of two."""
    exact = [_fr(k) for k in knot_vectors]
    d = max(v.denominator for k in exact for v in k)
    return [[int(v * d) for v in k] for k in exact]


def _blossom_integers(t, k, mu, args):
    """The row of refine_ref._blossom_row as integers over one denominator: (numerators, denominator).  Level r divides
    entry p by den(p, r) = t[i + k - r] - t[i], which does not depend on the arguments; every entry of the level is put
    over L_r, the product of the level's den(p, r), so the recurrence runs in integers without a single gcd."""
    d = [[int(p == q) for q in range(k)] for p in range(k)]
    total = 1
    for r, u in enumerate(args, start=1):
        dens = {p: t[mu - k + 1 + p + k - r] - t[mu - k + 1 + p] for p in range(r, k)}
        level = 1
        for v in dens.values():
            level *= v
        nxt = [None] * k
        for p in range(r, k):
            i = mu - k + 1 + p
            lo, hi, scale = u - t[i], t[i + k - r] - u, level // dens[p]
            nxt[p] = [scale * (hi * x + lo * y) for x, y in zip(d[p - 1], d[p])]
        d = nxt
        total *= level
    return d[k - 1], total


def product_rows(knots1, order1, knots2, order2, newKnots):
    """[(f, g, W, den)] per product coefficient: the weight on A[f + a] * B[g + b] is W[a][b] / den, Python integers."""
    t, s, tb = _scaled_knots(knots1, knots2, newKnots)
    k1, k2 = int(order1), int(order2)
    n = k1 + k2 - 2
    n1, n2 = len(t) - k1, len(s) - k2
    assert tb[0] == t[k1 - 1] == s[k2 - 1] and tb[-1] == t[n1] == s[n2], "the domains differ"
    rows = []
    for j in range(len(tb) - n - 1):
        cell = next(c for c in range(j, j + n + 1) if tb[c + 1] > tb[c])
        mu1, mu2 = _cell(t, k1, n1, tb[cell]), _cell(s, k2, n2, tb[cell])          # the cell's lower end picks the old cells
        assert t[mu1] <= tb[cell] and tb[cell + 1] <= t[mu1 + 1] and s[mu2] <= tb[cell] and tb[cell + 1] <= s[mu2 + 1], \
            "the product's knots do not refine the operands'"
        args = tb[j + 1:j + 1 + n]
        W = [[0] * k2 for _ in range(k1)]
        count, den = 0, None
        for subset in combinations(range(n), k1 - 1):
            rest = [i for i in range(n) if i not in subset]
            d1, den1 = _blossom_integers(t, k1, mu1, [args[i] for i in subset])
            d2, den2 = _blossom_integers(s, k2, mu2, [args[i] for i in rest])
            assert den is None or den == den1 * den2                                # the same cells: the same denominators
            den = den1 * den2
            for a in range(k1):
                for b in range(k2):
                    W[a][b] += d1[a] * d2[b]
            count += 1
        rows.append((mu1 - k1 + 1, mu2 - k2 + 1, W, den * count))
    return rows


def dependent_terms(productType, nDep1, nDep2):
    """Per component of the result: [(component of self, component of other, sign)]."""
    if productType == "D":
        return [[(d, d, 1) for d in range(nDep1)]]
    if productType == "C" and nDep1 == 3:
        return [[((d + 1) % 3, (d + 2) % 3, 1), ((d + 2) % 3, (d + 1) % 3, -1)] for d in range(3)]
    if productType == "C":
        return [[(0, 1, 1), (1, 0, -1)]]
    return [[(min(d, nDep1 - 1), min(d, nDep2 - 1), 1)] for d in range(max(nDep1, nDep2))]


def _integers(coefs):
    """(object array of Python ints, d): coefs == ints / d exactly (a float is a dyadic rational)."""
    exact = to_exact(coefs)
    d = max([v.denominator for v in exact.ravel()] or [1])
    ints = np.empty(exact.shape, object)
    ints.ravel()[:] = [int(v * d) for v in exact.ravel()]
    return ints, d


def multiply(order1, knots1, coefs1, order2, knots2, coefs2, pairs, productType, newKnots, dtype=None):
    """Exact coefficients of the product, rounded once to ``dtype`` (default: the common type of the two inputs).
    pairs: [(variable of self, variable of other)]; newKnots: the product's knots per pair.  Variables of the result:
    self's with the mapped ones in place, then other's unmapped ones.
    The sums run in Python integers: the data are integers over one power of two, every row of weights is integers over
    one denominator of its own, so a coefficient is an integer over the product of those; one division rounds it."""
    coefs1, coefs2 = np.asarray(coefs1), np.asarray(coefs2)
    dtype = dtype or np.result_type(coefs1.dtype, coefs2.dtype)
    (A, dA), (B, dB) = _integers(coefs1), _integers(coefs2)
    nInd1, nInd2 = A.ndim - 1, B.ndim - 1
    tables = []
    for (ind1, ind2), tbar in zip(pairs, newKnots):
        tables.append(product_rows(knots1[ind1], order1[ind1], knots2[ind2], order2[ind2], tbar))
    planes = []
    for terms in dependent_terms(productType, A.shape[0], B.shape[0]):
        total = None
        for da, db, sign in terms:
            # the outer product over all variables: axes (self's variables, other's variables)
            outer = np.multiply.outer(A[da], B[db]) * sign
            total = outer if total is None else total + outer
        # contract one mapped pair after the other: the result's axis takes the place of self's variable, other's goes
        other_axes = list(range(nInd2))                      # which of other's variables are still there, in order
        dens = np.empty((1,) * total.ndim, object)                   # per axis of total: the rows' denominators
        dens.ravel()[0] = dA * dB
        for (ind1, ind2), rows in zip(pairs, tables):
            ax2 = nInd1 + other_axes.index(ind2)
            moved = np.moveaxis(total, (ind1, ax2), (0, 1))
            out = np.empty((len(rows),) + moved.shape[2:], object)
            for j, (f, g, W, den) in enumerate(rows):
                acc = 0
                for a, row in enumerate(W):
                    for b, w in enumerate(row):
                        if w != 0:
                            acc = acc + w * moved[f + a, g + b]
                out[j] = acc
            other_axes.remove(ind2)
            total = np.moveaxis(out, 0, ind1)
            dens = dens.reshape([n for axis, n in enumerate(dens.shape) if axis != ax2])    # other's axis has gone
            shape = [1] * total.ndim
            shape[ind1] = len(rows)
            column = np.empty(len(rows), object)
            column[:] = [row[3] for row in rows]
            dens = dens * column.reshape(shape)
        dens = np.broadcast_to(dens, total.shape)
        exact = np.empty(total.shape, object)
        exact.ravel()[:] = [Fraction(int(n), int(d)) for n, d in zip(total.ravel(), dens.ravel())]
        planes.append(exact)
    return to_float(np.stack(planes), dtype)
