"""
TEST INFRASTRUCTURE: the extended-precision yardstick and the input transforms of the scale tests
(tests/test_scale_host.py, tests/test_gpu_scale.py).

Yardstick.  Reference bspy/_spline_evaluation.py:4-27 (bspline_values) and :109-133 (derivative) restated for any
number of independent variables, one point at a time, every operation in an extended type: np.longdouble where its
epsilon is below 1e-18 (x87: 1.1e-19), otherwise mpmath at 40 digits.  The span index is the reference's
(searchsorted on the stored knots, 'right', clamped), so a result is the reference's function of the stored inputs
with ~1e-19 rounding: the distance of an fp64 result from it IS that result's rounding error.

Transforms.  A spec is the tuple (order, nCoef, knots, coefs, points).  Power-of-two scales commute with every
rounding, so the reference's arithmetic obeys, bit for bit and while nothing under- or overflows,
    derivative(w) of (coefs * 2^kc, knots * 2^kp, points * 2^kp)  =  2^(kc - kp |w|) * derivative(w) of the original.
The affine domain map is deliberately NOT a power of two: it produces the knots a user would hand over (np.linspace
on a uniform axis, the mapped knots otherwise).
"""
import numpy as np

MP_DIGITS = 40


def use_mpmath():
    return not (np.finfo(np.longdouble).eps < 1e-18)


class _LongDouble:
    name = "np.longdouble"
    dtype = np.longdouble

    @staticmethod
    def num(x):
        return np.longdouble(x)

    @staticmethod
    def array(a):
        return np.asarray(a).astype(np.longdouble)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, np.longdouble)


class _MpMath:
    name = f"mpmath, {MP_DIGITS} digits"
    dtype = object

    def __init__(self):
        import mpmath
        self.ctx = mpmath.mp.clone()
        self.ctx.dps = MP_DIGITS

    def num(self, x):
        return self.ctx.mpf(float(x))                # every fp32 / fp64 value converts exactly

    def array(self, a):
        a = np.asarray(a)
        out = np.empty(a.shape, object)
        for i, v in np.ndenumerate(a):
            out[i] = self.ctx.mpf(float(v))
        return out

    def zeros(self, shape):
        out = np.empty(shape, object)
        out.fill(self.ctx.mpf(0))
        return out


def arithmetic(force_mpmath=False):
    return _MpMath() if (force_mpmath or use_mpmath()) else _LongDouble


def _span(knots, order, uf):
    """_spline_evaluation.py:7-9: the index the reference finds in the STORED knots (their own dtype)."""
    ix = int(np.searchsorted(knots, uf, side="right"))
    return min(max(ix, order), len(knots) - order)


def _basis(ar, order, k, ix, u, deriv):
    """_spline_evaluation.py:10-27 on the extended knots k at the extended parameter u."""
    b = ar.zeros(order)
    if deriv < order:
        b[-1] = ar.num(1)
        for degree in range(1, order - deriv):
            bi = order - degree
            for i in range(ix - degree, ix):
                alpha = (u - k[i]) / (k[i + degree] - k[i])
                b[bi - 1] += (1 - alpha) * b[bi]
                b[bi] *= alpha
                bi += 1
        for degree in range(order - deriv, order):
            bi = order - degree
            for i in range(ix - degree, ix):
                alpha = ar.num(degree) / (k[i + degree] - k[i])
                b[bi - 1] += -alpha * b[bi]
                b[bi] *= alpha
                bi += 1
    return b


def _curve_derivative_longdouble(order, knots, coefs, deriv, us):
    """Reference bspy/_spline_evaluation.py:4-27 + :109-133 for a curve, every operation in np.longdouble."""
    return derivative_ext((order,), [knots], coefs, [(deriv,)], [us], ar=_LongDouble)[0]


def derivative_ext(order, knots, coefs, wrts, points, ar=None):
    """One extended (nDep, N) array per derivative multi-index of `wrts`.  knots / coefs / points are taken in the
    dtype they come in (convert them to the kernel's dtype first: the yardstick is a function of the stored values)."""
    ar = ar or arithmetic()
    nind = len(order)
    ks = [ar.array(k) for k in knots]
    c = ar.array(coefs)
    n = len(points[0])
    needed = [sorted({w[iv] for w in wrts}) for iv in range(nind)]
    outs = [ar.zeros((c.shape[0], n)) for _ in wrts]
    for p in range(n):
        window = [slice(None)]
        basis = []
        for iv in range(nind):
            uf = points[iv][p]
            ix = _span(knots[iv], order[iv], uf)
            u = ar.num(uf)
            basis.append({d: _basis(ar, order[iv], ks[iv], ix, u, d) for d in needed[iv]})
            window.append(slice(ix - order[iv], ix))
        mine0 = c[tuple(window)]
        for out, w in zip(outs, wrts):
            mine = mine0
            for iv in range(nind - 1, -1, -1):                      # :130-132
                mine = mine @ basis[iv][w[iv]]
            out[:, p] = mine
    return outs


def span_indices(order, knots, points):
    """(nInd, N) span indices ix of the reference: the support of point p is coefs[:, ix - order:ix] per variable."""
    return np.array([[_span(k, o, u) for u in p] for k, o, p in zip(knots, order, points)])


def distance(x, ext, scale):
    """max |x - ext| / scale with the difference taken in the extended type."""
    ext = np.asarray(ext)
    d = np.abs(np.asarray(x).astype(ext.dtype) - ext)
    return float(d.max()) / float(scale)


def scale_of(ext):
    """The result scale the suite uses everywhere: max(1, max |reference|)."""
    return max(1.0, float(np.abs(np.asarray(ext)).max()))


# ------------------------------------------------------------------------------------------------- transforms
def _p2(a, k):
    a = np.asarray(a)
    return np.ldexp(a, k).astype(a.dtype)


def scale_coefs(spec, kc):
    """All coefficients x 2^kc."""
    order, ncoef, knots, coefs, points = spec
    return (order, ncoef, knots, _p2(coefs, kc), points)


def scale_rows(spec, ks):
    """Dependent row d x 2^ks[d]."""
    order, ncoef, knots, coefs, points = spec
    assert len(ks) == coefs.shape[0]
    return (order, ncoef, knots, np.stack([_p2(row, k) for row, k in zip(coefs, ks)]), points)


def scale_params(spec, kp):
    """Knots and parameter points x 2^kp."""
    order, ncoef, knots, coefs, points = spec
    return (order, ncoef, [_p2(k, kp) for k in knots], coefs, [_p2(p, kp) for p in points])


def law_exponent(kc, kp, wrt):
    """derivative(wrt) of the transformed spline = 2^law_exponent x the original's."""
    return kc - kp * int(sum(wrt))


def undo(x, exponent):
    """x x 2^-exponent in x's own dtype (exact while nothing under- or overflows)."""
    return _p2(x, -exponent)


def map_domain(order, ncoef, knots, lo, width, dtype):
    """Knots of the same spline shape on [lo, lo + width] per variable, as a user would produce them: np.linspace
    interior knots where the axis is the clamped uniform one of cases.clamped_uniform_knots, the affinely mapped
    (and re-sorted, end-clamped) knots otherwise."""
    import cases
    out = []
    hi = lo + width
    for o, c, k in zip(order, ncoef, knots):
        k = np.asarray(k, np.float64)
        k0, k1 = k[o - 1], k[c]
        if np.array_equal(k, cases.clamped_uniform_knots(o, c, np.float64, k0, k1)):
            out.append(cases.clamped_uniform_knots(o, c, dtype, lo, hi))
            continue
        m = lo + width * ((k - k0) / (k1 - k0))
        m[:o], m[c:] = lo, hi
        m = np.clip(np.sort(m), lo, hi).astype(dtype)
        m[:o], m[c:] = dtype(lo), dtype(hi)
        out.append(np.sort(m))
    return out


def sample_points(order, ncoef, knots, n, dtype, rng):
    """n points per variable: every distinct domain knot and +-1 ulp either side (in random order, at the front, as many
    as fit), the rest random in the domain."""
    pts = []
    for k, o, c in zip(knots, order, ncoef):
        k = np.asarray(k, dtype)
        lo, hi = k[o - 1], k[c]
        p = (lo + (hi - lo) * rng.random(n)).astype(dtype)
        d = np.unique(k)
        e = np.concatenate((d, np.nextafter(d, dtype(-np.inf)), np.nextafter(d, dtype(np.inf)))).astype(dtype)
        e = rng.permutation(e[(e >= lo) & (e <= hi)])[:n]
        p[:len(e)] = e
        pts.append(np.clip(p, lo, hi).astype(dtype))
    return pts


# ------------------------------------------------------------------------------------------------- axis_is_uniform
UNIFORM_ULPS = {np.dtype(np.float64): 1024.0, np.dtype(np.float32): 32.0}


def axis_is_uniform(k, order, ncoef, ulps=None):
    """bsk_api.hip axis_is_uniform restated: (accepted, worst d / h over the domain knots).  The domain knots sit within
    min(ulps * eps * h, 4 * eps * max|end|) of lo + j h, each end is clamped or continues the spacing."""
    L = np.longdouble
    k = np.asarray(k)
    eps = L(np.finfo(k.dtype).eps)
    ulps = UNIFORM_ULPS[k.dtype] if ulps is None else ulps
    ns = ncoef - order + 1
    lo, hi = L(k[order - 1]), L(k[ncoef])
    if not hi > lo or ns < 1:
        return False, float("inf")
    h = (hi - lo) / ns
    tol = min(L(ulps) * eps * h, 4 * eps * max(abs(lo), abs(hi)))
    dev = np.abs(k[order - 1:ncoef + 1].astype(L) - (lo + np.arange(ns + 1).astype(L) * h))
    ok = bool((dev <= tol).all())
    for low in (True, False):
        i = np.arange(1, order)
        v = (k[order - 1 - i] if low else k[ncoef + i]).astype(L)
        clamped = bool((v == (lo if low else hi)).all())
        continued = bool((np.abs(v - ((lo - i * h) if low else (hi + i * h))) <= tol).all())
        ok = ok and (clamped or continued)
    return ok, float(dev.max() / h)


# ------------------------------------------------------------------------------------------------- shared by both modules
NAN_AT = 5_000           # family batches carry one NaN parameter per end variable, behind the knot points at the front


def family_points(fam):
    """The batch of a point-kernel family (cases.ScaleFamily): sample_points plus a NaN in the first variable at NAN_AT
    and in the last at NAN_AT + 1."""
    pts = sample_points(fam.order, fam.nCoef, fam.knots, fam.n, fam.dt, np.random.default_rng(fam.seed))
    pts[0][NAN_AT] = np.nan
    pts[-1][NAN_AT + 1] = np.nan
    return pts


def family_axes(fam):
    """Grid axes of a grid / tessellation family: the domain ends, every interior knot's neighbourhood left to chance."""
    rng = np.random.default_rng(fam.seed)
    axes = []
    for k, o, c, m in zip(fam.knots, fam.order, fam.nCoef, fam.grid):
        lo, hi = fam.dt(k[o - 1]), fam.dt(k[c])
        a = np.sort((lo + (hi - lo) * rng.random(m)).astype(fam.dt))
        a[0], a[-1] = lo, hi
        d = np.unique(np.asarray(k, fam.dt))[1:-1][:max(0, m // 3)]
        a[1:1 + len(d)] = d
        axes.append(np.sort(np.clip(a, lo, hi)).astype(fam.dt))
    return axes


def family_transforms(fam, exponents, rows):
    """(label, per-row coefficient exponents, parameter exponent, one scale for all rows?)."""
    out = [(f"coefficients x 2^{kc}, knots and parameters x 2^{kp}", [kc] * fam.nDep, kp, True) for kc, kp in exponents[fam.kind]]
    r = [rows[fam.kind][d % len(rows[fam.kind])] for d in range(fam.nDep)]
    out.append((f"dependent rows x 2^{r}", r, 0, False))
    return out


def transformed(spec, kcs, kp):
    return scale_params(scale_rows(spec, kcs), kp)


def call_exponent(kind, wrt, kcs, kp, nind, uniform_rows):
    """Exponents the law predicts for the call's result, one per dependent variable or one for all, or None where the
    law says nothing (normals, curvature and measures under different scales per row).  undo_law applies them."""
    kcs = np.asarray(kcs)
    if kind in ("eval", "grid", "tess"):
        return kcs - kp * int(sum(wrt or ()))
    if kind == "jac":
        return kcs - kp
    if not uniform_rows:
        return None
    if kind in ("normal", "tessn"):                 # unit normal: unchanged
        return np.zeros(1, int)
    if kind == "curv":                              # curve: 1 / length; surface (Gaussian): 1 / length^2
        return np.array([-int(kcs[0]) * (1 if nind == 1 else 2)])
    if kind == "integral":                          # the measure of nInd coefficient lengths; parameters cancel
        return np.array([nind * int(kcs[0])])
    raise ValueError(kind)


def undo_law(x, e):
    """x x 2^-e in x's dtype; e per dependent variable (x's first axis) or a single exponent."""
    x = np.asarray(x)
    e = np.asarray(e)
    if e.size > 1:
        e = e.reshape((-1,) + (1,) * (x.ndim - 1))
    return np.ldexp(x, -e).astype(x.dtype)


def same_bits(a, b):
    """NaN in the same places, every other value bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def yardstick_wrts(order):
    """value, each first derivative, the highest non-zero derivative in the first variable."""
    nind = len(order)
    w = [(0,) * nind] + [tuple(int(i == j) for i in range(nind)) for j in range(nind)]
    top = (order[0] - 1,) + (0,) * (nind - 1)
    return w + ([top] if top not in w else [])


def shifted(spl, lo, width, n, seed=77):
    """(order, nCoef, knots, coefs, points) of a cases.ScaleSpline moved to [lo, lo + width]."""
    knots = map_domain(spl.order, spl.nCoef, spl.knots, lo, width, spl.dt)
    pts = sample_points(spl.order, spl.nCoef, knots, n, spl.dt, np.random.default_rng(seed))
    return spl.order, spl.nCoef, knots, spl.coefs, pts


def yardstick(spec, wrts, oracle_fn):
    """Per derivative multi-index: (extended result, oracle result, pure relative scale = max |extended|, d_orc).
    The jacobian is the first derivatives, so it needs no extended run of its own."""
    order, ncoef, knots, coefs, pts = spec
    exts = derivative_ext(order, knots, coefs, wrts, pts)
    out = {}
    for w, ext in zip(wrts, exts):
        orc, bad = oracle_fn(order, ncoef, knots, coefs, list(w), pts)
        assert bad == -1
        scale = float(np.abs(ext).max())
        out[w] = (ext, orc, scale, distance(orc, ext, scale))
    return out


def multiply_layers(coefs, ends, k=20):
    """coefs with the outermost control-point layer x 2^k at each (variable, end) of `ends` (end 0 = low, 1 = high), and
    the boolean mask of the multiplied control points (without the dependent axis)."""
    c = np.array(coefs)
    mask = np.zeros(c.shape[1:], bool)
    for iv, end in ends:
        sl = [slice(None)] * mask.ndim
        sl[iv] = 0 if end == 0 else -1
        mask[tuple(sl)] = True
    c[:, mask] = np.ldexp(c[:, mask], k)
    return c, mask


def support_is_clean(order, mask, ix):
    """Per point: no multiplied control point among the `order` coefficients below the span index in every variable."""
    n = ix.shape[1]
    clean = np.empty(n, bool)
    for p in range(n):
        win = tuple(slice(ix[iv, p] - order[iv], ix[iv, p]) for iv in range(len(order)))
        clean[p] = not mask[win].any()
    return clean


def fit_system(order, nrows, ncols, outer, inner, seed):
    """A banded least-squares system shaped like those of tests/test_gpu_fit.py: (plan, first, values, b (outer, nrows, inner))."""
    import fit_ref
    from bspy_amd import fitting
    rng = np.random.default_rng(seed)
    u = np.sort(rng.random(nrows))
    u[0], u[-1] = 0.0, 1.0
    interior = fit_ref.auto_knots(u, order, 0.0)[order:-order][1::3]       # at least two parameter values per span
    keep = np.sort(rng.choice(len(interior), ncols - order, replace=False)) if ncols > order else []
    knots = np.concatenate((np.zeros(order), interior[keep], np.ones(order)))
    first, values = fit_ref.banded_matrix(knots, order, u)                  # on the CPU: the host module builds it too
    b = np.random.default_rng(outer * 7 + inner).standard_normal((outer, nrows, inner))
    return fitting.Plan(first, values, ncols), np.asarray(first), np.asarray(values, np.float64), b


# ------------------------------------------------------------------------------------------------- operator specs
# A cases.OpCase is a public spline-to-spline call: operands [(order, knots, coefs)], an operation and its arguments.
# With coefficient row d of operand i x 2^ks[i][d] and every knot, inserted knot and trim bound x 2^kp, the result's
# knots are x 2^kp and row d of its coefficients x 2^op_exponent(...)[d], bit for bit: every weight of an operator is a
# ratio of knot differences (unchanged), a derivative weight 1 / difference (x 2^-kp), an integral weight a difference
# (x 2^kp), and every rounding commutes with a power of two.
PARAMETER_ARGS = ("new", "domain")


def _scale_arg(value, fn):
    """fn on every number of a nested argument (lists, (value, multiplicity) pairs keep their multiplicity, None stays)."""
    if value is None:
        return None
    if isinstance(value, tuple):
        return (fn(value[0]), value[1])
    if isinstance(value, (list, np.ndarray)):
        return [_scale_arg(v, fn) for v in value]
    return fn(value)


def op_scaled(case, ks, kp):
    operands = [(order, [_p2(t, kp) for t in knots], np.stack([_p2(row, k) for row, k in zip(coefs, rows)]))
                for (order, knots, coefs), rows in zip(case.operands, ks)]
    args = {key: _scale_arg(case.args[key], lambda v: float(np.ldexp(np.float64(v), kp))) for key in PARAMETER_ARGS if key in case.args}
    return case.replaced(operands, **args)


def op_exponent(case, ks, kp):
    """Per dependent row of the result (or one for all rows): the exponent the law predicts for its coefficients."""
    k0 = np.asarray(ks[0])
    if case.op == "differentiate":
        return k0 - kp
    if case.op == "integrate":
        return k0 + kp
    if case.op in ("add", "subtract"):
        assert list(ks[0]) == list(ks[1])
        return k0
    if case.op == "multiply":
        k1 = np.asarray(ks[1])
        if case.args["productType"] == "S":
            return k0 + k1
        assert len(set(k0)) == 1 and len(set(k1)) == 1, "a dot or cross product sums planes: one exponent per operand"
        return np.array([int(k0[0] + k1[0])])
    return k0


def op_transforms(case, exponents, rows):
    """[(label, per-operand per-row coefficient exponents, parameter exponent)]: the type's (kc, kp) pairs, then one
    exponent per dependent plane (per operand where the operation sums planes)."""
    ndep = [coefs.shape[0] for _, _, coefs in case.operands]
    two = case.op == "multiply"
    out = []
    for kc, kp in exponents[case.kind]:
        ks = [[kc] * ndep[0]] + ([[kc // 2] * ndep[1]] if two else [[kc] * n for n in ndep[1:]])
        out.append((f"coefficients x 2^{[k[0] for k in ks]}, knots x 2^{kp}", ks, kp))
    r = rows[case.kind]
    cyc = lambda n, shift=0: [r[(d + shift) % len(r)] for d in range(n)]
    if two and case.args["productType"] != "S":
        ks = [[r[0]] * ndep[0], [r[-1] // 2] * ndep[1]]
    elif two:
        ks = [cyc(ndep[0]), cyc(ndep[1], 1)]
    else:
        ks = [cyc(n) for n in ndep]
    out.append((f"dependent rows x 2^{ks}", ks, 0))
    return out


def map_axis(knots, order, lo, width, dtype, values=None):
    """The knots of one variable under the affine map of its domain onto [lo, lo + width], as map_domain maps a
    non-uniform axis (sorted, in ``dtype``; knots outside the domain of an unclamped variable go along); ``values``:
    parameters to map the same way instead, clipped into the new domain."""
    k = np.asarray(knots, np.float64)
    k0, k1 = k[order - 1], k[len(k) - order]
    m = np.sort(lo + width * ((k - k0) / (k1 - k0))).astype(dtype)
    if values is None:
        return m
    a, b = m[order - 1], m[len(k) - order]
    return _scale_arg(values, lambda v: float(np.clip(dtype(lo + width * ((np.float64(v) - k0) / (k1 - k0))), a, b)))


def op_shifted(case, lo, width):
    """The case with every operand's domain moved to [lo, lo + width] (knots in the coefficients' dtype), inserted knots
    and trim bounds mapped as the knots of operand 0 and clipped into the domain."""
    dt = case.dt
    order0, knots0, _ = case.operands[0]
    operands = [(order, [map_axis(t, k, lo, width, dt) for t, k in zip(knots, order)], coefs) for order, knots, coefs in case.operands]
    args = {}
    for key in PARAMETER_ARGS:
        if key in case.args:
            args[key] = [map_axis(t, k, lo, width, dt, values=v) for t, k, v in zip(knots0, order0, case.args[key])]
    return case.replaced(operands, **args)


def multiplied(coefs, index, k):
    """coefs with the one entry ``index`` x 2^k."""
    c = np.array(coefs)
    c[index] = np.ldexp(c[index], k)
    return c


# ------------------------------------------------------------------------------------------------- cell-family specs
# A cases.CellCase is a public batch call of zeros2, zeros3, project, contours or remove_knots.  With the coefficients
# x 2^ks (one exponent per leading index: system and component, field, or dependent row; project and a field with levels take
# one for all, since they subtract points or levels, which go along x 2^ks) and every knot, guess and inserted knot x 2^kp:
# zeros, vertices, foot parameters and result knots are x 2^kp, distances and result coefficients x 2^ks, and offsets, status
# bytes, step counts, polyline structure, zero cells and the choice of removed knots are unchanged, bit for bit.  Every
# threshold of the five families is relative: S_d eps, tau_of(K0, K1, S), 2^-20 h, TRUST of the domain width, a tolerance
# relative to max |coefficient|; every x = (t - left) / width is a ratio; every rounding commutes with a power of two.
def cell_scaled(case, ks, kp):
    ks = np.asarray(ks)
    coefs = _p2(case.coefs, ks.reshape(ks.shape + (1,) * (case.coefs.ndim - ks.ndim)))
    args = {}
    for key, k in (("points", ks), ("levels", ks), ("guess", kp)):
        if case.args.get(key) is not None:
            assert np.ndim(k) == 0, f"{key} go along with one exponent"
            args[key] = _p2(case.args[key], int(k))
    if "new" in case.args:
        args["new"] = _scale_arg(case.args["new"], lambda v: float(np.ldexp(np.float64(v), kp)))
    return case.replaced([_p2(t, kp) for t in case.knots], coefs, **args)


def cell_transforms(case, exponents, rows):
    """[(label, ks, kp)]: the type's (kc, kp) pairs, then the rows pattern cycled over every leading index that takes an
    exponent of its own: per component and per system (zeros2, zeros3), per field (contours with coefs), per dependent row
    (remove_knots); one for all (project, contours with levels): the pattern's exponents one after the other."""
    lead = {"zeros2": 2, "zeros3": 2, "project": 0, "contours": 0 if case.args.get("levels") is not None else 1, "remove_knots": 1}[case.family]
    shape = case.coefs.shape[:lead]
    out = [(f"coefficients x 2^{kc}, knots x 2^{kp}", np.full(shape, kc), kp) for kc, kp in exponents[case.kind]]
    r = rows[case.kind]
    if lead == 0:
        return out + [(f"coefficients x 2^{k}", np.array(k), 0) for k in r if k]
    cyc = np.array(r)[np.arange(shape[-1]) % len(r)]
    out.append((f"the last leading index x 2^{cyc.tolist()}", np.broadcast_to(cyc, shape).copy(), 0))
    if lead == 2:
        per = np.array(r)[(np.arange(shape[0]) + 1) % len(r)]
        out.append((f"systems x 2^{per.tolist()}", np.broadcast_to(per[:, None], shape).copy(), 0))
    return out


def cell_shifted(case, lo, width):
    """The case with every variable's domain moved to [lo, lo + width] (map_axis, in the knots' dtype); a guess and knots
    to insert are mapped along."""
    knots = [map_axis(t, k, lo, width, t.dtype.type) for t, k in zip(case.knots, case.order)]
    args = {}
    if case.args.get("guess") is not None:
        g = case.args["guess"]
        args["guess"] = (lo + width * g.astype(np.float64)).astype(g.dtype)
    if "new" in case.args:
        args["new"] = [map_axis(t, k, lo, width, np.float64, values=v) for t, k, v in zip(case.knots, case.order, case.args["new"])]
    return case.replaced(knots, **args)
