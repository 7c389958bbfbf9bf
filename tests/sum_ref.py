"""
Exact references for the sums tests (add / subtract, integrate, contract): plain Python / NumPy with
``fractions.Fraction``, no code shared with bspy_amd.  A float is a rational number, so every result here is computed
without rounding and rounded once at the end (``refine_ref.to_float``).

    add        both operands are brought onto the result's orders and knots with the exact rows of refine_ref.py
               (a clamp, an elevation and an insertion are all one exact change of basis), then added as Fractions
    integrate  out[0] = 0, out[j + 1] = out[j] + g[j] c[j] with g[j] = (t[j + k] - t[j]) / k formed in the knots' own
               precision, as the reference forms it, and taken as the rational number it is
    contract   per fixed variable the coefficients of the cell that holds u are combined with the exact de Boor
               weights at u (refine_ref._blossom_row with every argument equal to u)
"""
from fractions import Fraction

import numpy as np

import refine_ref


def _onto(order, knots, coefs, new_order, new_knots):
    """Exact coefficients (object array of Fractions) of the spline on the new orders and knots; every entry must exist."""
    exact = refine_ref.to_exact(np.asarray(coefs))
    for iv, (k, t, k2, t2) in enumerate(zip(order, knots, new_order, new_knots)):
        if k == k2 and len(t) == len(t2) and np.array_equal(np.asarray(t, np.float64), np.asarray(t2, np.float64)):
            continue
        exact, exists = refine_ref.apply_rows(refine_ref.refine_rows(t, k, t2, k2 - k), exact, iv + 1)
        assert exists.all(), "a result basis function without a cell in the operand's domain"
    return exact


def add(a, b, pairs, out_order, out_knots, sign, dtype):
    """a, b: dicts with order, knots, coefs.  pairs: [(variable of a, variable of b)] or None (the outer sum).
    Returns the exact sum on the result's basis rounded once to dtype, shape (nDep, *nCoef of the result)."""
    n1, n2 = len(a["order"]), len(b["order"])
    target = {} if pairs is None else {int(p[1]): int(p[0]) for p in pairs}
    free2 = [iv for iv in range(n2) if iv not in target]
    where2 = [target[iv] if iv in target else n1 + free2.index(iv) for iv in range(n2)]
    A = _onto(a["order"], a["knots"], a["coefs"], out_order[:n1], out_knots[:n1])
    B = _onto(b["order"], b["knots"], b["coefs"], [out_order[w] for w in where2], [out_knots[w] for w in where2])
    out = np.empty((A.shape[0], *[len(t) - k for t, k in zip(out_knots, out_order)]), object)
    for index in np.ndindex(*out.shape):
        ia = index[:1 + n1]
        ib = (index[0],) + tuple(index[1 + w] for w in where2)
        out[index] = A[ia] + sign * B[ib]
    return refine_ref.to_float(out, dtype)


def weights(knots, order):
    """g[j] = (t[j + k] - t[j]) / k in the knots' dtype."""
    t, k = np.asarray(knots), int(order)
    return (t[k:] - t[:len(t) - k]) / k


def integrate(order, knots, coefs, wrt, dtype):
    """Exact running sum along variable wrt, rounded once to dtype; also the scale S = max over lines of sum |g c|."""
    g = [Fraction(float(v)) for v in weights(knots[wrt], order[wrt])]
    moved = np.moveaxis(refine_ref.to_exact(np.asarray(coefs)), wrt + 1, 0)
    out = np.empty((len(g) + 1,) + moved.shape[1:], object)
    out[0] = Fraction(0)
    mass = np.zeros(moved.shape[1:], object) + Fraction(0)
    for j, gj in enumerate(g):
        out[j + 1] = out[j] + gj * moved[j]
        mass = mass + abs(gj) * np.abs(moved[j])
    scale = max(float(v) for v in np.ravel(mass))
    return refine_ref.to_float(np.moveaxis(out, 0, wrt + 1), dtype), scale


def basis_values(knots, order, u):
    """(first, [Fractions]): the exact B-spline values at u on the cell the reference takes: the cell to the right of
    an interior knot, the last non-empty cell at the right end of the domain."""
    t = [Fraction(float(v)) for v in np.asarray(knots)]
    k = int(order)
    n = len(t) - k
    u = Fraction(float(np.asarray(knots).dtype.type(u)))
    assert t[k - 1] <= u <= t[n]
    if u == t[n]:
        mu = max(i for i in range(k - 1, n) if t[i] < t[n])
    else:
        mu = max(i for i in range(k - 1, n) if t[i] <= u)
    return mu - k + 1, refine_ref._blossom_row(t, k, mu, [u] * (k - 1))


def contract(order, knots, coefs, uvw, dtype):
    """Exact coefficients with the variables whose uvw entry is not None fixed, rounded once to dtype."""
    exact = refine_ref.to_exact(np.asarray(coefs))
    axis = 1
    for iv, u in enumerate(uvw):
        if u is None:
            axis += 1
            continue
        first, w = basis_values(knots[iv], order[iv], u)
        moved = np.moveaxis(exact, axis, 0)
        acc = w[0] * moved[first]
        for s in range(1, len(w)):
            acc = acc + w[s] * moved[first + s]
        exact = np.asarray(acc, object).reshape(moved.shape[1:])
    return refine_ref.to_float(exact, dtype)
