"""
Exact real roots of a scalar spline curve, for the root tests: plain Python with ``fractions.Fraction``; the only code
shared with anything is the exact blossoming of refine_ref.py.  This file decides how many roots a case has and where
they are.

A float is a rational number, so the Bernstein coefficients of every knot span are rational (``bezier_spans``: exact
Bezier extraction of the float inputs as given).  Per span the roots are isolated by Descartes' rule of signs under exact
halving until every sub-interval has 0 or 1 sign variations (``isolate``); a bracket is then bisected exactly to a width of
eps (b - a) / 16 or less.  ``value`` evaluates f exactly at a rational point; ``roots`` returns f' at every root it reports.

``roots`` applies the contract of bspy_amd/roots.py on top: spans whose K B-spline coefficients are all below S eps are
zero spans and every maximal run of them is one interval; next to a run nothing is reported within sqrt(eps) (b - a) of
its end; a span owns [t_j, t_j+1) and the last one also b, so a Bernstein end coefficient that is exactly zero is a root
at that knot for the span that owns it, and a sign change across a jump (a knot of multiplicity K) is no root.  A root of
even multiplicity is found only where halving lands on it (a dyadic point of its span); elsewhere ``isolate`` gives up
at ``MAX_DEPTH`` with an error, so the cases say what they are.
"""
import math
from fractions import Fraction

import numpy as np

import refine_ref

EPS = Fraction(1, 2 ** 52)
MAX_DEPTH = 80


def _sign(x):
    return (x > 0) - (x < 0)


def variations(c):
    v, last = 0, 0
    for x in c:
        s = _sign(x)
        if s:
            v += last != 0 and s != last
            last = s
    return v


def halve(c):
    b = list(c)
    K = len(b)
    left, right = [b[0]], [b[-1]]
    for r in range(1, K):
        b = [(b[i] + b[i + 1]) / 2 for i in range(K - r)]
        left.append(b[0])
        right.insert(0, b[-1])
    return left, right


def span_value(c, x):
    b = list(c)
    for r in range(1, len(b)):
        b = [(1 - x) * b[i] + x * b[i + 1] for i in range(len(b) - 1)]
    return b[0]


def bezier_spans(order, knots, coefs):
    """[(t0, t1, [K Fractions])] for every knot span of the domain, left to right: the exact Bernstein coefficients."""
    k = int(order)
    t = [Fraction(float(v)) for v in np.asarray(knots)]
    n = len(t) - k
    lo, hi = t[k - 1], t[n]
    new = list(t)
    for v in sorted(set(t)):
        if v < lo or v > hi:
            continue
        want = k if v in (lo, hi) else max(k - 1, t.count(v))
        new += [v] * (want - t.count(v))
    new.sort()
    rows = refine_ref.refine_rows([float(v) for v in t], k, [float(v) for v in new], 0)
    exact = [Fraction(float(v)) for v in np.asarray(coefs)]
    breaks = sorted(v for v in set(new) if lo <= v <= hi)
    spans = []
    for t0, t1 in zip(breaks[:-1], breaks[1:]):
        mu = max(i for i, v in enumerate(new) if v == t0)
        c = []
        for j in range(mu - k + 1, mu + 1):
            first, w = rows[j]
            c.append(sum(wi * exact[first + i] for i, wi in enumerate(w)))
        spans.append((t0, t1, c))
    return spans


def isolate(c, last):
    """Roots of the Bernstein polynomial c in [0, 1) (``last``: in [0, 1]) as (lo, hi) pairs of Fractions, ascending:
    lo == hi is an exact root, lo < hi an open interval with exactly one root, a simple one."""
    out = []

    def walk(c, lo, w, depth):
        if c[0] == 0:
            out.append((lo, lo))
        v = variations(c)
        if v == 0:
            return
        if v == 1:
            out.append((lo, lo + w))
            return
        if depth >= MAX_DEPTH:
            raise ArithmeticError("a multiple root that is not a dyadic point of its span, or roots closer than 2^-80")
        left, right = halve(c)
        # the left half keeps lo, which is reported already; the point between the halves belongs to the right one
        if variations(left) >= 1:
            walk_no_start(left, lo, w / 2, depth + 1)
        walk(right, lo + w / 2, w / 2, depth + 1)

    def walk_no_start(c, lo, w, depth):
        v = variations(c)
        if v == 0:
            return
        if v == 1:
            out.append((lo, lo + w))
            return
        if depth >= MAX_DEPTH:
            raise ArithmeticError("a multiple root that is not a dyadic point of its span, or roots closer than 2^-80")
        left, right = halve(c)
        if variations(left) >= 1:
            walk_no_start(left, lo, w / 2, depth + 1)
        walk(right, lo + w / 2, w / 2, depth + 1)

    walk(list(c), Fraction(0), Fraction(1), 0)
    if last and c[-1] == 0:
        out.append((Fraction(1), Fraction(1)))
    return out


def shrink(c, lo, hi, width):
    """Exact bisection of a bracket with one simple root until hi - lo <= width."""
    sa = next(s for s in (_sign(x) for x in restrict(c, lo, hi)) if s)
    while hi - lo > width:
        mid = (lo + hi) / 2
        f = span_value(c, mid)
        if f == 0:
            return mid, mid
        if _sign(f) == sa:
            lo = mid
        else:
            hi = mid
    return lo, hi


def restrict(c, lo, hi):
    """Exact Bernstein coefficients on [lo, hi] by blossoming: coefficient i = f(lo^(n - i), hi^i)."""
    n = len(c) - 1
    out = []
    for i in range(n + 1):
        b = list(c)
        for level, x in enumerate([lo] * (n - i) + [hi] * i):
            b = [(1 - x) * b[j] + x * b[j + 1] for j in range(len(b) - 1)]
        out.append(b[0])
    return out


def roots(order, knots, coefs):
    """The contract applied exactly.  Returns dict(brackets=[(lo, hi)] in the curve's parameter (Fractions, ascending,
    width <= eps (b - a) / 16), fprime=[f' at the bracket's midpoint], intervals=[(left, right)] floats, scale=S)."""
    k = int(order)
    t = np.asarray(knots)
    c = np.asarray(coefs)
    assert c.ndim == 1
    spans = bezier_spans(k, t, c)
    a, b = spans[0][0], spans[-1][1]
    S = float(np.abs(c.astype(np.float64)).max())
    small = np.abs(c.astype(np.float64)) < S * float(EPS)
    tf = [Fraction(float(v)) for v in t]
    zero = []
    for t0, _, _ in spans:
        mu = max(i for i, v in enumerate(tf) if v <= t0 and i <= len(tf) - k - 1)
        zero.append(bool(S == 0.0 or small[mu - k + 1:mu + 1].all()))
    margin = Fraction(math.sqrt(float(EPS)) * (float(b) - float(a)))
    intervals, s = [], 0
    while s < len(spans):
        if zero[s]:
            e = s
            while e + 1 < len(spans) and zero[e + 1]:
                e += 1
            intervals.append((float(spans[s][0]), float(spans[e][1])))
            s = e + 1
        else:
            s += 1
    brackets, fprime = [], []
    width = EPS * (b - a) / 16
    for s, (t0, t1, cs) in enumerate(spans):
        if zero[s]:
            continue
        h = t1 - t0
        for lo, hi in isolate(cs, s == len(spans) - 1):
            if lo < hi:
                lo, hi = shrink(cs, lo, hi, width / h)
            ulo, uhi = t0 + lo * h, t0 + hi * h
            mid = (ulo + uhi) / 2
            if s > 0 and zero[s - 1] and mid <= t0 + margin:
                continue
            if s + 1 < len(spans) and zero[s + 1] and mid >= t1 - margin:
                continue
            brackets.append((ulo, uhi))
            x = (lo + hi) / 2
            d = [(k - 1) * (cs[i + 1] - cs[i]) for i in range(k - 1)]
            fprime.append(span_value(d, x) / h if d else Fraction(0))
    return dict(brackets=brackets, fprime=fprime, intervals=intervals, scale=S)


def value(order, knots, coefs, u):
    """f(u), exactly, u a Fraction inside the domain (at a jump: the right limit)."""
    spans = bezier_spans(order, knots, coefs)
    for s, (t0, t1, c) in enumerate(spans):
        if t0 <= u < t1 or (s == len(spans) - 1 and u == t1):
            return span_value(c, (u - t0) / (t1 - t0))
    raise ValueError("outside the domain")
