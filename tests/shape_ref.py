"""
TEST INFRASTRUCTURE: the extended-precision yardstick and the per-point bars of the normal and curvature tests
(tests/test_shape_host.py, tests/test_gpu_shape.py; inputs: cases.shape_cases).  Nothing here calls bspy_amd.

Yardstick.  scale_ref.derivative_ext gives the first (and second) derivatives at a sample of points in the extended type;
from them, in the extended type, the cofactor normal of the reference (bspy/_spline_evaluation.py:215-246: area-scaled and
unit, negated or not, |nInd - nDep| = 1 up to 4 rows) and its curvature (:80-107: curves, signed for nDep 2, and the
Gaussian curvature of a surface in 3-D).

Bar.  g is the normal or curvature formula, d_i every derivative component that enters it.  A result computed from
derivative values that are off by at most delta_i, and rounded itself, is off by
    bar(p) = 2 * (sum_i |dg/dd_i|(p) * delta_i  +  K * eps * |g(p)|)
to first order; the factor 2 covers the higher-order terms.  The partials are central differences in the extended type
with a step of 2^-24 of the component's scale (max |d_w| over the sample).  The last term is the result's own rounding,
one more error source that enters with partial 1 and scale |g|: without it the bar vanishes where a component of a unit
normal is at +-1 (every partial of that component is zero there while its last rounding is half an ulp), and the CPU oracle
itself misses such a bar - by 2.2 x on the (3, 3, 3) volume with nDep 2, whose normal lies along the third axis by
construction, and by 1.1 x on the order-14 curve (35 to 600 units over seven point seeds, K would have to be 1024 or more).
delta_i for a component of derivative w is
    general-knot families:      K * eps(dtype) * max(1, max |ext_w|)
    table-free uniform families: max(4 * d_orc(w), floor) * max |ext_w|, floor 1e-12 (fp64) / 2e-5 (fp32)
the second being the form tests/test_gpu_scale.py part B already holds jac_uni, jac_stream_uni, eval_uni and
eval_stream_uni to (they accept knots up to 1024 ulp of a span off the nominal grid).  d_orc is the distance of the CPU
oracle's derivative from the extended one, relative to max |ext_w|.

K is set from the reference side only: the worst error of the CPU oracle (oracle.c_normal, oracle.c_curvature, in the
kernels' dtype) over the general-knot cases of cases.shape_cases, in units of eps * (sum_i |dg/dd_i| * max(1, max |ext_w|)
+ |g|), times 8 (another operation order, FMA contraction and reciprocal tables in the kernels), rounded up to a power of
two, and never below K_FLOOR (16 and 32: what a first probe of these shapes gave).
Measured by tests/test_shape_host.py::test_measured_units (printed with -s):
    fp64: 2.64 units (area normal of the order-14 curve: the oracle's own first derivative is 2.8 eps off there)  ->  K = 32
    fp32: 0.42 units (area normal of the order-(3, 3) surface)  ->  8 x gives 4, K_FLOOR holds  ->  K = 32
With these the oracle sits within 0.082 of the bar at every kept point of every case (asserted: 1/8).

Exclusions.  A point whose max(bar) > 0.1 * max(1, |g|) is ill-conditioned (nearly dependent tangents, a vanishing first
fundamental form): the first-order bar does not hold there.  It is left out of the unit-normal and curvature comparison
only (area normals never), at most 10 % of a case's sample may be left out, and NaN positions always have to agree.
"""
import functools

import numpy as np

import scale_ref as sr

K_FLOOR = {np.dtype(np.float64): 16.0, np.dtype(np.float32): 32.0}      # what a first probe of these shapes gave: K is never set below
K = {np.dtype(np.float64): 32.0, np.dtype(np.float32): 32.0}
UNIFORM_FLOOR = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 2e-5}
STEP = 2.0 ** -24
ILL = 0.1                  # a point is ill-conditioned when max(bar) > ILL * max(1, |g|)
KEEP = 0.9                 # share of a case's sample that has to stay
SAMPLE = 200


def sample_indices(n):
    """The reference sample of a batch of n points: the first 100 (domain ends, interior knots and the NaN parameter sit at
    the front, cases.shape_points) and 100 spread over the rest."""
    if n <= SAMPLE:
        return np.arange(n)
    return np.concatenate((np.arange(SAMPLE // 2), np.linspace(SAMPLE // 2, n - 1, SAMPLE // 2).astype(np.int64)))


def wrts_of(kind, nind):
    """The derivative multi-indices that enter the normal or the curvature, in the order the formulas below take them."""
    if kind == "normal":
        return [tuple(int(i == j) for i in range(nind)) for j in range(nind)]
    return [(1,), (2,)] if nind == 1 else [(1, 0), (0, 1), (2, 0), (1, 1), (0, 2)]


def _sqrt(x):
    if x.dtype == object:
        return np.frompyfunc(lambda v: v.sqrt() if hasattr(v, "sqrt") else v ** 0.5, 1, 1)(x)
    return np.sqrt(x)


def _det(rows):
    """Determinant of the m x m matrix given as m rows of m arrays (m <= 3); m = 0 gives 1."""
    m = len(rows)
    if m == 0:
        return 1
    if m == 1:
        return rows[0][0]
    if m == 2:
        return rows[0][0] * rows[1][1] - rows[0][1] * rows[1][0]
    a, b, c = rows
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0])


def cofactors(D, nind, ndep):
    """_spline_evaluation.py:222-240 at every point: D[j] = derivative in variable j, (nDep, N) -> (max(nInd, nDep), N)."""
    big = max(nind, ndep)
    # tangent space with the larger dimension first: T[r][c]; the jacobian is J[d][j] = D[j][d]
    T = [[D[r][c] if nind > ndep else D[c][r] for c in range(big - 1)] for r in range(big)]
    out = []
    for i in range(big):
        v = _det([T[r] for r in range(big) if r != i])
        out.append(-v if i & 1 else v)
    return np.stack([o + 0 * D[0][0] for o in out])


def normal_of(D, nind, ndep, unit=True, negate=False):
    n = cofactors(D, nind, ndep)
    if negate:
        n = -n
    if unit:
        n = n / _sqrt((n * n).sum(0))
    return n


def curvature_of(D, nind, ndep):
    """_spline_evaluation.py:83-107 at every point: D = the derivatives of wrts_of("curvature", nInd) -> (1, N)."""
    if nind == 1:
        fp, fpp = D
        a, b, c = (fp * fp).sum(0), (fp * fpp).sum(0), (fpp * fpp).sum(0)
        num = fp[0] * fpp[1] - fp[1] * fpp[0] if ndep == 2 else _sqrt(c * a - b * b)
        return (num / (a * _sqrt(a)))[None]
    su, sv, suu, suv, svv = D
    nrm = normal_of([su, sv], 2, 3)
    E, F, G = (su * su).sum(0), (su * sv).sum(0), (sv * sv).sum(0)
    L, M, N = (suu * nrm).sum(0), (suv * nrm).sum(0), (svv * nrm).sum(0)
    return ((L * N - M * M) / (E * G - F * F))[None]


def sensitivity(g, D, scales):
    """|dg/dd_i| for every component i = (w, row) of D by central differences: an array (len(D), nDep) + g(D).shape."""
    first = g(D)
    out = np.empty((len(D), D[0].shape[0]) + first.shape, first.dtype)
    for w in range(len(D)):
        h = D[0].dtype.type(STEP * scales[w]) if D[0].dtype != object else STEP * scales[w]
        for d in range(D[0].shape[0]):
            up = [x.copy() for x in D]
            dn = [x.copy() for x in D]
            up[w][d] = up[w][d] + h
            dn[w][d] = dn[w][d] - h
            out[w, d] = np.abs((g(up) - g(dn)) / (2 * h))
    return out


def _worst(err, by):
    """max err / by, an error where `by` is zero counting as infinite (0 / 0 as 0)."""
    with np.errstate(all="ignore"):
        r = np.where(by > 0, err / by, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r, initial=0.0))


class Reference:
    """The yardstick of one case on its sample: per quantity the extended result, sum_i |dg/dd_i| s_i (the bar's unit
    before eps and K) and sum_i |dg/dd_i| delta_i."""

    def __init__(self, case, oracle_fn):
        self.case = case
        dt = np.dtype(case.dt)
        self.eps = float(np.finfo(dt).eps)
        pts = case.points()
        self.idx = sample_indices(case.n)
        self.pts = [p[self.idx] for p in pts]
        nind, ndep = case.nInd, case.nDep
        wrts = wrts_of(case.kind, nind)
        with np.errstate(all="ignore"):
            D = sr.derivative_ext(case.order, case.knots, case.coefs, wrts, self.pts)
        self.D, self.wrts = D, wrts
        finite = ~np.isnan(np.stack([np.asarray(x, np.float64) for x in D])).any(axis=(0, 1))
        self.finite = finite
        absmax = [float(np.abs(np.asarray(x, np.float64)[:, finite]).max()) for x in D]
        self.absmax = absmax
        self.scales = [max(1.0, a) for a in absmax]
        if case.uniform:
            # part-B form: the oracle's own distance from the extended derivative, per derivative
            self.delta = []
            for w, ext, a in zip(wrts, D, absmax):
                orc, bad = oracle_fn(case.order, case.nCoef, case.knots, case.coefs, list(w), [p[finite] for p in self.pts])
                assert bad == -1
                d_orc = sr.distance(orc, ext[:, finite], a)
                self.delta.append(max(4.0 * d_orc, UNIFORM_FLOOR[dt]) * a)
        else:
            self.delta = [K[dt] * self.eps * s for s in self.scales]
        self.q = {}
        steps = [a if a > 0 else 1.0 for a in absmax]
        for name, g in self.formulas().items():
            with np.errstate(all="ignore"):
                ext = g(D)
                sens = sensitivity(g, D, steps)
            own = np.abs(ext)                                                          # the result's own rounding: partial 1, scale |g|
            unit = sum(sens[w] * self.scales[w] for w in range(len(D))).sum(0) + own    # sum_i |dg/dd_i| s_i + |g|
            bar = 2.0 * (sum(sens[w] * self.delta[w] for w in range(len(D))).sum(0) + K[dt] * self.eps * own)
            self.q[name] = (ext, np.asarray(unit, np.float64), np.asarray(bar, np.float64))

    def formulas(self):
        nind, ndep = self.case.nInd, self.case.nDep
        if self.case.kind == "curvature":
            return {"curvature": lambda D: curvature_of(D, nind, ndep)}
        return {"unit normal": lambda D: normal_of(D, nind, ndep, True, False),
                "area normal": lambda D: normal_of(D, nind, ndep, False, False),
                "area normal, negated": lambda D: normal_of(D, nind, ndep, False, True)}

    def kept(self, name):
        """The points a comparison of `name` judges: finite, and well-conditioned unless it is an area normal."""
        ext, _, bar = self.q[name]
        if name.startswith("area"):
            return self.finite.copy()
        with np.errstate(all="ignore"):
            g = np.abs(np.asarray(ext, np.float64)).max(0)
            ok = bar.max(0) <= ILL * np.maximum(1.0, g)
        return self.finite & ok & np.isfinite(g)

    def nan_mask(self):
        return ~self.finite

    def compare(self, name, got):
        """got: the result at the sample points, (rows, len(sample)) or (len(sample),).  Returns (worst |got - ref| / bar
        over the kept points, worst error in units of eps * sum |dg| s, kept share); NaN positions are asserted."""
        ext, unit, bar = self.q[name]
        got = np.asarray(got).reshape(ext.shape)
        keep = self.kept(name)
        assert np.array_equal(np.isnan(got).any(0), self.nan_mask()), f"{self.case.name}: {name}: NaN positions differ from the reference's"
        assert np.isfinite(got[:, keep]).all(), f"{self.case.name}: {name}: non-finite value at a well-conditioned point"
        err = np.asarray(np.abs(got[:, keep].astype(ext.dtype) - ext[:, keep]), np.float64)
        ratio = _worst(err, bar[:, keep])
        units = _worst(err, self.eps * unit[:, keep])
        share = float(keep.sum()) / float(self.finite.sum())
        return ratio, units, share


@functools.lru_cache(maxsize=None)
def _reference(name):
    import cases
    import oracle
    return Reference(cases.shape_cases()[name], oracle.c_evaluate)


def reference(case):
    """The case's Reference, computed once per session and shared (never modified) by every test that needs it."""
    return _reference(case.name)
