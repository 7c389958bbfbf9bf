"""
Certified common zeros of three scalar splines in three variables, for the zeros3 tests: zeros2_ref.py in three variables,
plain Python with ``fractions.Fraction`` (held in NumPy object arrays so that an axis is a slice); the only code shared
with anything is the exact per-axis Bezier extraction of zeros2_ref.py (``axis_rows``).  This file decides how many zeros
a case has and where they are.

A float is a rational number, so the tensor-product Bernstein coefficients of the three components on every knot cell are
rational (``bezier_cells``).  All coordinates below are cell-local, x in [0, 1]^3.

Certification (``certify``).  A zero gets a box X inside its cell and a rational preconditioner Y, the inverse of the
Jacobian at the centre of X rounded to floats.  With G = Y F:
  * existence, by Poincare-Miranda: for k = 0, 1, 2 the Bernstein coefficients of G_k on the two faces of X across axis k
    are strictly of opposite signs;
  * uniqueness and the error bound: the Bernstein coefficients of the entries of I - Y J on X (differences of those of
    G) bound every entry over X; when every row sum of the bounds is <= 1/2, the mean-value matrix M of G between any
    two points of X (row k taken at its own point) has |I - M| <= 1/2 in the row-sum norm, so X holds one zero r* and
    |x - r*| <= 2 |Y F(x)| (max-norm) for every x in X (``error_bound``).

Completeness (``solve_cell``).  Exact octree subdivision of the cell: a box is dropped when a component's Bernstein
coefficients on it are strictly of one sign, discarded when it lies inside a certified X; a float Newton iteration from
the centre of a surviving box proposes where to certify next.  Whatever survives at ``MAX_DEPTH`` raises
``ArithmeticError``: a tangential zero, a zero on a cell face, a zero set of positive dimension.  The cases say what they
are.
"""
from fractions import Fraction

import numpy as np

import zeros2_ref

MAX_DEPTH = 24
RADII = tuple(Fraction(1, 2 ** e) for e in (6, 8, 10, 14, 20, 28))
ONE, HALF = Fraction(1), Fraction(1, 2)


# ------------------------------------------------------------------------------------------ one component (Fractions or floats)
def exact(a):
    """A float array as an object array of Fractions."""
    a = np.asarray(a)
    out = np.empty(a.shape, object)
    out.reshape(-1)[:] = [Fraction(float(v)) for v in a.reshape(-1)]
    return out


def split(comp, axis, t):
    """de Casteljau at t along ``axis``: (left, right)."""
    b = np.moveaxis(comp, axis, 0)
    left, right = [b[0]], [b[-1]]
    while len(b) > 1:
        b = (1 - t) * b[:-1] + t * b[1:]
        left.append(b[0])
        right.insert(0, b[-1])
    return np.moveaxis(np.array(left), 0, axis), np.moveaxis(np.array(right), 0, axis)


def restrict(comp, lo, hi):
    """The coefficients on the box [lo, hi] (three numbers each)."""
    for axis in range(3):
        if lo[axis] != 0:
            comp = split(comp, axis, lo[axis])[1]
        if hi[axis] != 1:
            comp = split(comp, axis, (hi[axis] - lo[axis]) / (1 - lo[axis]))[0]
    return comp


def value(comp, x):
    b = comp
    for t in x:
        while len(b) > 1:
            b = (1 - t) * b[:-1] + t * b[1:]
        b = b[0]
    return b


def derivative(comp, axis):
    """The Bernstein coefficients of d/dx_axis on the same box, per unit of the box."""
    return (comp.shape[axis] - 1) * np.diff(comp, axis=axis)


def one_sign(comp):
    flat = comp.reshape(-1)
    return all(v > 0 for v in flat) or all(v < 0 for v in flat)


# ------------------------------------------------------------------------------------------ exact cells
def bezier_cells(order, knots, coefs):
    """(breaks [3 lists], cells): cells[i][j][k] = [component 0, 1, 2], a component an object array (K0, K1, K2) of Fractions."""
    coefs = np.asarray(coefs)
    assert coefs.ndim == 4 and coefs.shape[0] == 3
    axes = [zeros2_ref.axis_rows(order[a], knots[a]) for a in range(3)]

    def extract(arr, axis, rows):
        a = np.moveaxis(arr, axis, 0)
        return np.moveaxis(np.array([sum((w * a[first + q] for q, w in enumerate(ws)), 0) for first, ws in rows]), 0, axis)

    whole = [exact(comp) for comp in coefs]
    cells = []
    for rows0 in axes[0][1]:
        slab = [extract(comp, 0, rows0) for comp in whole]
        plane = []
        for rows1 in axes[1][1]:
            bar = [extract(comp, 1, rows1) for comp in slab]
            plane.append([[extract(comp, 2, rows2) for comp in bar] for rows2 in axes[2][1]])
        cells.append(plane)
    return [a[0] for a in axes], cells


# ------------------------------------------------------------------------------------------ certification
def certify(cell, x, radius):
    """A certificate dict(lo, hi, Y, x, radius) of the one zero in the box of ``radius`` around x, clipped to the cell, or None."""
    lo = tuple(max(Fraction(0), v - radius) for v in x)
    hi = tuple(min(ONE, v + radius) for v in x)
    if any(a >= b for a, b in zip(lo, hi)):
        return None
    mid = tuple((a + b) / 2 for a, b in zip(lo, hi))
    J = np.array([[float(value(derivative(comp, l), mid)) for l in range(3)] for comp in cell])
    with np.errstate(all="ignore"):
        try:
            inverse = np.linalg.inv(J)
        except np.linalg.LinAlgError:
            return None
    if not np.isfinite(inverse).all():
        return None
    Y = [[Fraction(float(v)) for v in row] for row in inverse]
    on = [restrict(comp, lo, hi) for comp in cell]
    G = [Y[k][0] * on[0] + Y[k][1] * on[1] + Y[k][2] * on[2] for k in range(3)]
    for k in range(3):
        first, last = np.take(G[k], 0, axis=k).reshape(-1), np.take(G[k], -1, axis=k).reshape(-1)
        if not ((all(v < 0 for v in first) and all(v > 0 for v in last)) or (all(v > 0 for v in first) and all(v < 0 for v in last))):
            return None
    for k in range(3):
        total = Fraction(0)
        for l in range(3):
            flat = derivative(G[k], l).reshape(-1) / (hi[l] - lo[l])
            total += max(abs(int(k == l) - v) for v in flat)
        if total > HALF:
            return None
    return dict(lo=lo, hi=hi, Y=Y, x=tuple(x), radius=radius)


def error_bound(cell, cert, x):
    """2 |Y F(x)| in the max-norm, exactly: the distance bound of x from the certified zero.  x must lie in the
    certificate's box."""
    assert all(cert["lo"][a] <= x[a] <= cert["hi"][a] for a in range(3)), "the point is outside the certified box"
    F = [value(comp, x) for comp in cell]
    return 2 * max(abs(sum(cert["Y"][k][d] * F[d] for d in range(3))) for k in range(3))


def _newton(floats, x):
    """Float Newton from x on float copies of the components: a proposal, nothing is believed."""
    x = np.array(x, float)
    for _ in range(30):
        F = np.array([value(comp, x) for comp in floats])
        J = np.array([[value(derivative(comp, l), x) for l in range(3)] for comp in floats])
        try:
            step = np.linalg.solve(J, F)
        except np.linalg.LinAlgError:
            return None
        x = x - step
        if not (np.isfinite(x).all() and (-1.0 <= x).all() and (x <= 2.0).all()):
            return None
        if np.abs(step).max() <= 1e-15:
            return x
    return None


def solve_cell(cell):
    """The certificates of all zeros of one cell, or ArithmeticError."""
    certs = []
    floats = [comp.astype(float) for comp in cell]

    def inside(lo, w):
        return any(all(c["lo"][a] <= lo[a] and lo[a] + w <= c["hi"][a] for a in range(3)) for c in certs)

    stack = [(cell, (Fraction(0),) * 3, ONE, 0)]
    while stack:
        box, lo, w, depth = stack.pop()
        if inside(lo, w) or any(one_sign(comp) for comp in box):
            continue
        if depth >= 1:
            centre = [float(v + w / 2) for v in lo]
            guess = _newton(floats, centre)
            if guess is not None and ((0.0 <= guess) & (guess <= 1.0)).all() and np.abs(guess - centre).max() <= 2.0 * float(w):
                x = tuple(Fraction(float(g)) for g in guess)
                if not any(all(c["lo"][a] <= x[a] <= c["hi"][a] for a in range(3)) for c in certs):
                    for radius in RADII:
                        cert = certify(cell, x, radius)
                        if cert is not None:
                            certs.append(cert)
                            break
                if inside(lo, w):
                    continue
        if depth >= MAX_DEPTH:
            raise ArithmeticError("a box that is neither excluded nor certified: a tangential zero, a zero on a cell face, or "
                                  "zeros that are not isolated")
        parts = [(box, lo)]
        for axis in range(3):
            parts = [([half[n] for half in (split(comp, axis, HALF) for comp in b)],
                      tuple(v + n * w / 2 if a == axis else v for a, v in enumerate(at)))
                     for b, at in parts for n in range(2)]
        for b, at in parts:
            stack.append((b, at, w / 2, depth + 1))
    certs.sort(key=lambda c: c["lo"])
    return certs


def zero_cells(order, knots, coefs):
    """The contract of bspy_amd/roots3.py on zero cells: [(i, j, k)] of the cells on which the K0 x K1 x K2 B-spline
    coefficients of any component are all below S_d eps, S_d the component's largest absolute coefficient."""
    coefs = np.abs(np.asarray(coefs).astype(np.float64))
    small = [(comp < comp.max() * 2.0 ** -52) | (comp.max() == 0.0) for comp in coefs]
    spans = []
    for k, t in zip(order, knots):
        tf = [Fraction(float(v)) for v in np.asarray(t)]
        breaks = sorted(v for v in set(tf) if tf[k - 1] <= v <= tf[len(tf) - k])
        spans.append([max(i for i, v in enumerate(tf) if v <= t0 and i <= len(tf) - k - 1) for t0 in breaks[:-1]])
    K0, K1, K2 = order
    return [(i, j, k) for i, mu in enumerate(spans[0]) for j, nu in enumerate(spans[1]) for k, xi in enumerate(spans[2])
            if any(s[mu - K0 + 1:mu + 1, nu - K1 + 1:nu + 1, xi - K2 + 1:xi + 1].all() for s in small)]


def zeros(order, knots, coefs):
    """All isolated zeros of the system outside its zero cells, certified.  Returns a list, sorted by (u, v, w), of
    dict(cell=(i, j, k), lo, hi, Y, x, radius, t0, h, u): the box [lo, hi] = x -+ radius clipped to the cell and Y are
    cell-local, (t0, h) the cell's corner and widths, u the box's centre in the parameters, all Fractions.
    Raises ArithmeticError where the zeros of a cell cannot all be certified."""
    breaks, cells = bezier_cells(order, knots, coefs)
    skip = set(zero_cells(order, knots, coefs))
    out = []
    for i, plane in enumerate(cells):
        for j, line in enumerate(plane):
            for k, cell in enumerate(line):
                if (i, j, k) in skip:
                    continue
                at = (i, j, k)
                t0 = tuple(breaks[a][at[a]] for a in range(3))
                h = tuple(breaks[a][at[a] + 1] - breaks[a][at[a]] for a in range(3))
                for cert in solve_cell(cell):
                    mid = [(cert["lo"][a] + cert["hi"][a]) / 2 for a in range(3)]
                    out.append(dict(cert, cell=at, t0=t0, h=h, u=tuple(t0[a] + mid[a] * h[a] for a in range(3))))
    out.sort(key=lambda z: z["u"])
    return out
