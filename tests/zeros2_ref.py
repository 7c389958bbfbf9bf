"""
Certified common zeros of two scalar splines in two variables, for the zeros2 tests: plain Python with
``fractions.Fraction``; the only code shared with anything is the exact blossoming of refine_ref.py and the line
arithmetic of zeros_ref.py.  This file decides how many zeros a case has and where they are.

A float is a rational number, so the tensor-product Bernstein coefficients of both components on every knot cell are
rational (``bezier_cells``: exact Bezier extraction per axis of the float inputs as given).  All coordinates below are
cell-local, (x, y) in [0, 1]^2.

Certification (``certify``).  A zero gets a box X inside its cell and a rational preconditioner Y, the inverse of the
Jacobian at the centre of X rounded to floats.  With G = Y F:
  * existence, by Poincare-Miranda: the Bernstein coefficients of G_1 on the two x-faces of X are strictly of opposite
    signs, and those of G_2 on the two y-faces;
  * uniqueness and the error bound: the Bernstein coefficients of the entries of I - Y J on X (differences of those of
    G) bound every entry over X; when every row sum of the bounds is <= 1/2, the mean-value matrix M of G between any
    two points of X (row k taken at its own point) has |I - M| <= 1/2 in the row-sum norm, so X holds one zero r* and
    |x - r*| <= 2 |Y F(x)| (max-norm) for every x in X (``error_bound``).

Completeness (``solve_cell``).  Exact quadtree subdivision of the cell: a box is dropped when a component's Bernstein
coefficients on it are strictly of one sign, discarded when it lies inside a certified X; a float Newton iteration from
the centre of a surviving box proposes where to certify next.  Whatever survives at ``MAX_DEPTH`` raises
``ArithmeticError``: a tangential zero, a zero on a cell edge, a zero set of positive dimension.  The cases say what they
are.
"""
from fractions import Fraction

import numpy as np

import refine_ref
import zeros_ref

MAX_DEPTH = 40
RADII = (Fraction(1, 2 ** 10), Fraction(1, 2 ** 14), Fraction(1, 2 ** 20), Fraction(1, 2 ** 28))


# ------------------------------------------------------------------------------------------ exact cells
def axis_rows(order, knots):
    """(breaks, rows): the distinct knots of the domain as Fractions and, per span, the K exact rows (first, weights) of
    the Bezier extraction (every interior knot raised to multiplicity K - 1, the ends to K)."""
    k = int(order)
    t = [Fraction(float(v)) for v in np.asarray(knots)]
    n = len(t) - k
    lo, hi = t[k - 1], t[n]
    new = list(t)
    for v in sorted(set(t)):
        if lo <= v <= hi:
            want = k if v in (lo, hi) else max(k - 1, t.count(v))
            new += [v] * (want - t.count(v))
    new.sort()
    rows = refine_ref.refine_rows([float(v) for v in t], k, [float(v) for v in new], 0)
    breaks = sorted(v for v in set(new) if lo <= v <= hi)
    spans = []
    for t0 in breaks[:-1]:
        mu = max(i for i, v in enumerate(new) if v == t0)
        spans.append([rows[j] for j in range(mu - k + 1, mu + 1)])
    return breaks, spans


def bezier_cells(order, knots, coefs):
    """(breaks0, breaks1, cells): cells[i][j] = [component 0, component 1], a component K0 rows of K1 Fractions."""
    coefs = np.asarray(coefs)
    assert coefs.ndim == 3 and coefs.shape[0] == 2
    breaks0, spans0 = axis_rows(order[0], knots[0])
    breaks1, spans1 = axis_rows(order[1], knots[1])
    exact = [[[Fraction(float(v)) for v in row] for row in comp] for comp in coefs]
    cells = []
    for rows0 in spans0:
        line = []
        for rows1 in spans1:
            cell = []
            for comp in exact:
                along0 = [[sum(w * comp[first + p][q] for p, w in enumerate(ws)) for q in range(len(comp[0]))] for first, ws in rows0]
                cell.append([[sum(w * row[first + q] for q, w in enumerate(ws)) for first, ws in rows1] for row in along0])
            line.append(cell)
        cells.append(line)
    return breaks0, breaks1, cells


# ------------------------------------------------------------------------------------------ one component (Fractions or floats)
def value2(comp, x, y):
    return zeros_ref.span_value([zeros_ref.span_value(row, y) for row in comp], x)


def columns(comp):
    return [list(col) for col in zip(*comp)]


def restrict2(comp, lo0, hi0, lo1, hi1):
    comp = columns([zeros_ref.restrict(col, lo0, hi0) for col in columns(comp)])
    return [zeros_ref.restrict(row, lo1, hi1) for row in comp]


def derivatives(comp):
    """The Bernstein coefficients of d/dx and d/dy on the same box, per unit of the box."""
    K0, K1 = len(comp), len(comp[0])
    dx = [[(K0 - 1) * (comp[i + 1][j] - comp[i][j]) for j in range(K1)] for i in range(K0 - 1)]
    dy = [[(K1 - 1) * (comp[i][j + 1] - comp[i][j]) for j in range(K1 - 1)] for i in range(K0)]
    return dx, dy


def one_sign(comp):
    flat = [v for row in comp for v in row]
    return all(v > 0 for v in flat) or all(v < 0 for v in flat)


def quarter(comp):
    """The four quarters of a box, [x half][y half]."""
    halves = [columns(part) for part in zip(*[zeros_ref.halve(col) for col in columns(comp)])]
    return [[[list(r) for r in part] for part in zip(*[zeros_ref.halve(row) for row in half])] for half in halves]


# ------------------------------------------------------------------------------------------ certification
def certify(cell, x, y, radius):
    """A certificate dict(lo, hi, Y, x, y, radius) of the one zero in the box of ``radius`` around (x, y), clipped to the cell, or None."""
    lo = (max(Fraction(0), x - radius), max(Fraction(0), y - radius))
    hi = (min(Fraction(1), x + radius), min(Fraction(1), y + radius))
    if lo[0] >= hi[0] or lo[1] >= hi[1]:
        return None
    mid = ((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2)
    J = [[float(value2(d, *mid)) if all(map(len, d)) else 0.0 for d in derivatives(comp)] for comp in cell]
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
    if det == 0.0 or det != det:
        return None
    Y = [[Fraction(J[1][1] / det), Fraction(-J[0][1] / det)], [Fraction(-J[1][0] / det), Fraction(J[0][0] / det)]]
    on = [restrict2(comp, lo[0], hi[0], lo[1], hi[1]) for comp in cell]
    K0, K1 = len(on[0]), len(on[0][0])
    G = [[[Y[k][0] * on[0][i][j] + Y[k][1] * on[1][i][j] for j in range(K1)] for i in range(K0)] for k in range(2)]
    faces = [(G[0][0], G[0][K0 - 1]), ([row[0] for row in G[1]], [row[K1 - 1] for row in G[1]])]
    for first, last in faces:
        if not ((all(v < 0 for v in first) and all(v > 0 for v in last)) or (all(v > 0 for v in first) and all(v < 0 for v in last))):
            return None
    width = (hi[0] - lo[0], hi[1] - lo[1])
    for k in range(2):
        total = Fraction(0)
        for l, d in enumerate(derivatives(G[k])):
            flat = [v / width[l] for row in d for v in row] or [Fraction(0)]
            total += max(abs(int(k == l) - v) for v in flat)
        if total > Fraction(1, 2):
            return None
    return dict(lo=lo, hi=hi, Y=Y, x=x, y=y, radius=radius)


def error_bound(cell, cert, x, y):
    """2 |Y F(x, y)| in the max-norm, exactly: the distance bound of (x, y) from the certified zero.  (x, y) must lie in
    the certificate's box."""
    assert cert["lo"][0] <= x <= cert["hi"][0] and cert["lo"][1] <= y <= cert["hi"][1], "the point is outside the certified box"
    F = [value2(comp, x, y) for comp in cell]
    return 2 * max(abs(cert["Y"][k][0] * F[0] + cert["Y"][k][1] * F[1]) for k in range(2))


def _newton(cell, x, y):
    """Float Newton from (x, y): a proposal, nothing is believed."""
    f = [[[float(v) for v in row] for row in comp] for comp in cell]
    d = [derivatives(comp) for comp in f]
    for _ in range(30):
        F = [value2(comp, x, y) for comp in f]
        J = [[value2(part, x, y) if part and part[0] else 0.0 for part in d[k]] for k in range(2)]
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        if det == 0.0 or det != det:
            return None
        dx = (F[0] * J[1][1] - J[0][1] * F[1]) / det
        dy = (J[0][0] * F[1] - F[0] * J[1][0]) / det
        x, y = x - dx, y - dy
        if not (-1.0 <= x <= 2.0 and -1.0 <= y <= 2.0):
            return None
        if max(abs(dx), abs(dy)) <= 1e-15:
            return x, y
    return None


def solve_cell(cell):
    """The certificates of all zeros of one cell, or ArithmeticError."""
    certs = []

    def inside(lo0, lo1, w):
        return any(c["lo"][0] <= lo0 and lo0 + w <= c["hi"][0] and c["lo"][1] <= lo1 and lo1 + w <= c["hi"][1] for c in certs)

    stack = [(cell, Fraction(0), Fraction(0), Fraction(1), 0)]
    while stack:
        box, lo0, lo1, w, depth = stack.pop()
        if inside(lo0, lo1, w) or one_sign(box[0]) or one_sign(box[1]):
            continue
        if depth >= 2:
            guess = _newton(cell, float(lo0 + w / 2), float(lo1 + w / 2))
            if guess is not None and all(0.0 <= g <= 1.0 for g in guess) and \
                    max(abs(guess[0] - float(lo0 + w / 2)), abs(guess[1] - float(lo1 + w / 2))) <= 2.0 * float(w):
                x, y = Fraction(guess[0]), Fraction(guess[1])
                if not any(c["lo"][0] <= x <= c["hi"][0] and c["lo"][1] <= y <= c["hi"][1] for c in certs):
                    for radius in RADII:
                        cert = certify(cell, x, y, radius)
                        if cert is not None:
                            certs.append(cert)
                            break
                if inside(lo0, lo1, w):
                    continue
        if depth >= MAX_DEPTH:
            raise ArithmeticError("a box that is neither excluded nor certified: a tangential zero, a zero on a cell edge, or "
                                  "zeros that are not isolated")
        parts = [quarter(comp) for comp in box]
        for a in range(2):
            for b in range(2):
                stack.append(([parts[0][a][b], parts[1][a][b]], lo0 + a * w / 2, lo1 + b * w / 2, w / 2, depth + 1))
    certs.sort(key=lambda c: (c["lo"][0], c["lo"][1]))
    return certs


def zero_cells(order, knots, coefs):
    """The contract of bspy_amd/roots2.py on zero cells: [(i, j)] of the cells on which the K0 x K1 B-spline coefficients
    of either component are all below S_d eps, S_d the component's largest absolute coefficient."""
    coefs = np.abs(np.asarray(coefs).astype(np.float64))
    small = [(comp < comp.max() * 2.0 ** -52) | (comp.max() == 0.0) for comp in coefs]
    spans = []
    for k, t in zip(order, knots):
        tf = [Fraction(float(v)) for v in np.asarray(t)]
        breaks = sorted(v for v in set(tf) if tf[k - 1] <= v <= tf[len(tf) - k])
        spans.append([max(i for i, v in enumerate(tf) if v <= t0 and i <= len(tf) - k - 1) for t0 in breaks[:-1]])
    K0, K1 = order
    return [(i, j) for i, mu in enumerate(spans[0]) for j, nu in enumerate(spans[1])
            if any(s[mu - K0 + 1:mu + 1, nu - K1 + 1:nu + 1].all() for s in small)]


def zeros(order, knots, coefs):
    """All isolated zeros of the system outside its zero cells, certified.  Returns a list, sorted by (u, v), of
    dict(cell=(i, j), lo, hi, Y, x, y, radius, t0, h, u, v): the box [lo, hi] = (x, y) -+ radius clipped to the cell and Y
    are cell-local, (t0, h) the cell's corner and widths, (u, v) the box's centre in the parameters, all Fractions.
    Raises ArithmeticError where the zeros of a cell cannot all be certified."""
    breaks0, breaks1, cells = bezier_cells(order, knots, coefs)
    skip = set(zero_cells(order, knots, coefs))
    out = []
    for i, line in enumerate(cells):
        for j, cell in enumerate(line):
            if (i, j) in skip:
                continue
            t0 = (breaks0[i], breaks1[j])
            h = (breaks0[i + 1] - breaks0[i], breaks1[j + 1] - breaks1[j])
            for cert in solve_cell(cell):
                mid = [(cert["lo"][d] + cert["hi"][d]) / 2 for d in range(2)]
                out.append(dict(cert, cell=(i, j), t0=t0, h=h, u=t0[0] + mid[0] * h[0], v=t0[1] + mid[1] * h[1]))
    out.sort(key=lambda z: (z["u"], z["v"]))
    return out
