"""
The marched zero set of a scalar spline in two variables, exactly, for the contours tests: plain Python with
``fractions.Fraction``; the only code shared with anything is the exact blossoming of refine_ref.py (through
zeros2_ref.axis_rows) and the line arithmetic of zeros_ref.py.  This file decides which lattice edges carry a vertex, where
the vertex is, which segments join them and how many components there are.

A float is a rational number, so the tensor-product Bernstein coefficients of the field on every knot cell are rational
(``bezier_cells``: exact Bezier extraction per axis of the float inputs as given, the level subtracted exactly).  The
exact spline is continuous across knot lines (the cases have no jump), so the value of a lattice node does not depend on
the cell that evaluates it; neither does the polynomial on a lattice line.

``trace`` applies the marching rule of bspy_amd/contours.py to exact signs (0 counts as positive): per lattice edge the
exact roots of the exact restriction (``zeros_ref.isolate``), per crossed edge the bracket of its root shrunk to
2^-70 of the edge, per leaf the segments (a saddle leaf is paired by the exact sign at its centre), and the connected
components of the segments.
"""
from fractions import Fraction

import numpy as np

import zeros2_ref
import zeros_ref

WIDTH = Fraction(1, 2 ** 70)


def bezier_cells(order, knots, coefs, level=0.0):
    """(breaks0, breaks1, cells): cells[i][j] = K0 rows of K1 Fractions, the exact field minus the level."""
    coefs = np.asarray(coefs)
    assert coefs.ndim == 2
    breaks0, spans0 = zeros2_ref.axis_rows(order[0], knots[0])
    breaks1, spans1 = zeros2_ref.axis_rows(order[1], knots[1])
    lev = Fraction(float(level))
    exact = [[Fraction(float(v)) for v in row] for row in coefs]
    cells = []
    for rows0 in spans0:
        line = []
        for rows1 in spans1:
            along0 = [[sum(w * exact[first + p][q] for p, w in enumerate(ws)) for q in range(len(exact[0]))] for first, ws in rows0]
            line.append([[sum(w * row[first + q] for q, w in enumerate(ws)) - lev for first, ws in rows1] for row in along0])
        cells.append(line)
    return breaks0, breaks1, cells


def zero_cells(cells, S):
    """[(i, j)] of the cells whose Bezier coefficients are all below S eps in magnitude (S: float)."""
    small = Fraction(float(S)) * zeros_ref.EPS
    return [(i, j) for i, line in enumerate(cells) for j, cell in enumerate(line)
            if S == 0.0 or all(abs(v) < small for row in cell for v in row)]


def value2(cell, x, y):
    return zeros_ref.span_value([zeros_ref.span_value(row, y) for row in cell], x)


class Exact:
    def __init__(self, order, knots, coefs, depth, level=0.0):
        self.breaks0, self.breaks1, self.cells = bezier_cells(order, knots, coefs, level)
        self.depth, self.G = int(depth), 1 << int(depth)
        self.nc0, self.nc1 = len(self.cells), len(self.cells[0])
        self.NJ = self.nc1 * self.G + 1
        self._nodes = {}

    def local(self, I, nc):
        """A cell that contains lattice coordinate I and the local parameter there."""
        i = min(I // self.G, nc - 1)
        return i, Fraction(I - i * self.G, self.G)

    def node(self, I, J):
        if (I, J) not in self._nodes:
            i, x = self.local(I, self.nc0)
            j, y = self.local(J, self.nc1)
            self._nodes[I, J] = value2(self.cells[i][j], x, y)
        return self._nodes[I, J]

    def key(self, I, J, direction):
        return ((I * self.NJ + J) << 1) | direction

    def edge_line(self, I, J, direction):
        """The exact Bernstein coefficients of the field on the edge, its cell (i, j) and the local start (x, y)."""
        if direction == 0:
            i, x = I // self.G, Fraction(I % self.G, self.G)
            j, y = self.local(J, self.nc1)
            line = [zeros_ref.span_value(row, y) for row in self.cells[i][j]]
            return zeros_ref.restrict(line, x, x + Fraction(1, self.G)), i, j, x, y
        i, x = self.local(I, self.nc0)
        j, y = J // self.G, Fraction(J % self.G, self.G)
        line = [zeros_ref.span_value(list(col), x) for col in zip(*self.cells[i][j])]
        return zeros_ref.restrict(line, y, y + Fraction(1, self.G)), i, j, x, y

    def edge_roots(self, I, J, direction):
        """The exact roots of the field on the closed edge, in the edge's own parameter: [(lo, hi)]."""
        c = self.edge_line(I, J, direction)[0]
        if all(v == 0 for v in c):
            return [(Fraction(0), Fraction(1))] * 2              # the field vanishes on the edge: more than one root
        return zeros_ref.isolate(c, True)

    def vertex(self, I, J, direction):
        """The bracket of the one root of a crossed edge in the parameters: ((ulo, uhi), (vlo, vhi)), the fixed
        coordinate with lo == hi, and |df/ds| along the edge at the bracket's middle, per unit of the parameter."""
        c, i, j, x, y = self.edge_line(I, J, direction)
        found = [r for r in zeros_ref.isolate(c, True)]
        assert len(found) == 1, "a crossed edge with more than one root"
        lo, hi = found[0]
        if lo < hi:
            lo, hi = zeros_ref.shrink(c, lo, hi, WIDTH)
        t0, h0 = self.breaks0[i], self.breaks0[i + 1] - self.breaks0[i]
        s0, h1 = self.breaks1[j], self.breaks1[j + 1] - self.breaks1[j]
        k = len(c)
        d = [(k - 1) * (c[n + 1] - c[n]) for n in range(k - 1)]
        slope = abs(zeros_ref.span_value(d, (lo + hi) / 2)) * self.G
        if direction == 0:
            u = (t0 + (x + lo / self.G) * h0, t0 + (x + hi / self.G) * h0)
            v = (s0 + y * h1,) * 2
            return u, v, slope / h0
        u = (t0 + x * h0,) * 2
        v = (s0 + (y + lo / self.G) * h1, s0 + (y + hi / self.G) * h1)
        return u, v, slope / h1


def trace(order, knots, coefs, depth, level=0.0, skip=()):
    """The marching rule on exact signs.  Returns dict(segments=[(key_a, key_b)], saddles=[(i, j)], vertices={key: (I, J,
    dir)}, components=[(closed, [keys])], exact=Exact).  ``skip``: the cells that nobody marches (zero cells)."""
    ex = Exact(order, knots, coefs, depth, level)
    G = ex.G
    segments, saddles, vertices = [], set(), {}
    for i in range(ex.nc0):
        for j in range(ex.nc1):
            if (i, j) in skip:
                continue
            for a in range(G):
                for b in range(G):
                    I, J = i * G + a, j * G + b
                    s00, s10, s11, s01 = (ex.node(I, J) >= 0, ex.node(I + 1, J) >= 0, ex.node(I + 1, J + 1) >= 0, ex.node(I, J + 1) >= 0)
                    t = [int(s00) - int(s10), int(s10) - int(s11), int(s11) - int(s01), int(s01) - int(s00)]
                    ncross = sum(1 for x in t if x)
                    if not ncross:
                        continue
                    cpos = False
                    if ncross == 4:
                        cpos = value2(ex.cells[i][j], Fraction(2 * a + 1, 2 * G), Fraction(2 * b + 1, 2 * G)) >= 0
                        saddles.add((i, j))
                    edges = [(I, J, 0), (I + 1, J, 1), (I, J + 1, 0), (I, J, 1)]
                    for k in range(4):
                        if t[k] <= 0:
                            continue
                        e = t.index(-1) if ncross == 2 else (k + (1 if cpos else 3)) & 3
                        pair = []
                        for n in (k, e):
                            key = ex.key(*edges[n])
                            vertices[key] = edges[n]
                            pair.append(key)
                        segments.append(tuple(pair))
    return dict(segments=segments, saddles=sorted(saddles), vertices=vertices, components=components(segments), exact=ex)


def components(segments):
    """[(closed, [keys in order])], sorted by first key: open chains from the key where nothing ends, loops from their
    smallest key (repeated at the end)."""
    nxt = {a: b for a, b in segments}
    assert len(nxt) == len(segments), "two segments start at one edge"
    ends = {b for _, b in segments}
    seen, out = set(), []
    for a in sorted(nxt):
        if a in ends:
            continue
        chain = [a]
        while chain[-1] in nxt:
            seen.add(chain[-1])
            chain.append(nxt[chain[-1]])
        out.append((False, chain))
    for a in sorted(nxt):
        if a in seen:
            continue
        chain = [a]
        while chain[-1] not in seen:
            seen.add(chain[-1])
            chain.append(nxt[chain[-1]])
        out.append((True, chain))
    out.sort(key=lambda c: c[1][0])
    return out
