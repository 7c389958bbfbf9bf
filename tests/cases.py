"""
Deterministic input generator shared by the golden-vector script, the oracle
tests and the GPU parity tests.

Nothing in here touches the reference: it only builds *inputs* (spline
definitions and parameter points) from fixed seeds, following the generator
spec of SURVEY.md section 8(c)-2, so the GPU box can regenerate exactly the
inputs whose reference outputs are stored in ``tests/golden/*.npz``.
"""
import functools
import itertools
import numpy as np


def clamped_uniform_knots(order, ncoef, dtype=np.float64, lo=0.0, hi=1.0):
    """concat(lo*order, interior linspace, hi*order): the BASELINE.md generator."""
    interior = np.linspace(lo, hi, ncoef - order + 2)[1:-1]
    return np.concatenate((np.full(order, lo), interior, np.full(order, hi))).astype(dtype)


def nonuniform_knots(rng, order, ncoef, dtype=np.float64, lo=-2.0, hi=3.0):
    """Clamped knots on [lo, hi] with sorted random interior knots, some of
    them repeated (multiplicity 2 .. order-1), total interior count ncoef-order."""
    n_int = ncoef - order
    vals = []
    while len(vals) < n_int:
        x = lo + (hi - lo) * (0.02 + 0.96 * rng.random())
        mult = 1
        if order > 2 and rng.random() < 0.25:
            mult = int(rng.integers(2, order))
        mult = min(mult, n_int - len(vals))
        vals.extend([x] * mult)
    interior = np.sort(np.array(vals, dtype=np.float64))
    return np.concatenate((np.full(order, lo), interior, np.full(order, hi))).astype(dtype)


def all_wrt(nind, max_total):
    """Every derivative multi-index with total order <= max_total."""
    return [w for w in itertools.product(range(max_total + 1), repeat=nind) if sum(w) <= max_total]


class Case:
    """One spline + one batch of points + the derivative multi-indices to pin."""

    def __init__(self, name, seed, nind, ndep, order, ncoef, n, kdtype=np.float64, cdtype=np.float64,
                 pdtype=None, knots="uniform", wrts=None, jacobian=True, edge_points=False):
        self.name = name
        self.nInd, self.nDep = nind, ndep
        self.order, self.nCoef = tuple(order), tuple(ncoef)
        rng = np.random.default_rng(seed)
        if knots == "uniform":
            self.knots = [clamped_uniform_knots(o, c, kdtype) for o, c in zip(order, ncoef)]
        else:
            self.knots = [nonuniform_knots(rng, o, c, kdtype) for o, c in zip(order, ncoef)]
        self.coefs = rng.standard_normal((ndep, *ncoef)).astype(cdtype)
        pdtype = pdtype or (np.float32 if (kdtype == np.float32 and cdtype == np.float32) else np.float64)
        pts = []
        for iv in range(nind):
            k = self.knots[iv]
            lo, hi = float(k[order[iv] - 1]), float(k[ncoef[iv]])
            p = (lo + (hi - lo) * rng.random(n)).astype(pdtype)
            if edge_points:
                # parameters exactly on every distinct knot, on both domain ends and
                # one ulp either side of each interior knot (clipped to the domain)
                d = np.unique(k.astype(pdtype))
                d = d[(d >= pdtype(lo)) & (d <= pdtype(hi))]
                e = np.concatenate((d, np.nextafter(d, pdtype(-np.inf)), np.nextafter(d, pdtype(np.inf))))
                e = e[(e >= pdtype(lo)) & (e <= pdtype(hi))].astype(pdtype)
                e = e[rng.permutation(len(e))]
                m = min(len(e), n)
                p[:m] = e[:m]
            p = np.clip(p, pdtype(lo), pdtype(hi))
            pts.append(p)
        self.points = pts
        self.wrts = wrts if wrts is not None else [tuple([0] * nind)]
        self.jacobian = jacobian

    @property
    def n(self):
        return len(self.points[0]) if self.points else 0


def parity_cases():
    """The randomised parity sets plus the edge set (8c-3)."""
    f32, f64 = np.float32, np.float64
    cs = []
    # cfg1: 1-D cubic, nCoef 32
    cs.append(Case("cfg1_curve", 101, 1, 1, (4,), (32,), 2048, wrts=all_wrt(1, 4), edge_points=True))
    # cfg2 / cfg3: bicubic 64x64x3 fp64 (uniform and non-uniform knots)
    cs.append(Case("cfg2_bicubic", 102, 2, 3, (4, 4), (64, 64), 1024, wrts=all_wrt(2, 3) + [(4, 0), (0, 5), (2, 2)]))
    cs.append(Case("cfg2_bicubic_nonuniform", 103, 2, 3, (4, 4), (64, 64), 1024, knots="nonuniform",
                   wrts=all_wrt(2, 3), edge_points=True))
    # cfg5: trivariate order 5, 40^3, nDep 4, fp32 (coefs regenerated from the seed: 1 MB)
    cs.append(Case("cfg5_trivariate_f32", 105, 3, 4, (5, 5, 5), (40, 40, 40), 1024, f32, f32,
                   wrts=[(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (2, 0, 1)]))
    cs.append(Case("cfg5_trivariate_f64", 106, 3, 4, (5, 5, 5), (12, 11, 10), 512, knots="nonuniform",
                   wrts=[(0, 0, 0), (1, 0, 0), (0, 2, 1), (4, 0, 0), (5, 0, 0)], edge_points=True))
    # teapot-like patch: single Bezier span, fp32
    cs.append(Case("bezier_patch_f32", 107, 2, 3, (4, 4), (4, 4), 512, f32, f32, wrts=all_wrt(2, 2), edge_points=True))
    # orders 1..9 in one variable, nDep 1..6
    for o in range(1, 10):
        cs.append(Case(f"curve_order{o}", 200 + o, 1, 1 + (o % 6), (o,), (o + 7,), 128, knots="nonuniform",
                       wrts=[(d,) for d in range(0, o + 2)], edge_points=True))
    # mixed orders, 2 and 3 variables, various nDep
    cs.append(Case("surface_o3x4", 301, 2, 3, (3, 4), (4, 5), 512, knots="nonuniform", wrts=all_wrt(2, 3), edge_points=True))
    cs.append(Case("surface_o2x6_d1", 302, 2, 1, (2, 6), (9, 8), 512, knots="nonuniform", wrts=all_wrt(2, 2), edge_points=True))
    cs.append(Case("surface_o7x3_d6", 303, 2, 6, (7, 3), (11, 20), 512, wrts=all_wrt(2, 2)))
    cs.append(Case("surface_o1x4_d2", 304, 2, 2, (1, 4), (5, 6), 512, knots="nonuniform", wrts=all_wrt(2, 1), edge_points=True))
    cs.append(Case("volume_o3x4x2", 305, 3, 3, (3, 4, 2), (6, 7, 5), 512, knots="nonuniform", wrts=all_wrt(3, 2), edge_points=True))
    cs.append(Case("volume_o4_d1", 306, 3, 1, (4, 4, 4), (8, 9, 10), 512, wrts=all_wrt(3, 1)))
    cs.append(Case("four_var", 307, 4, 2, (3, 2, 4, 3), (4, 5, 6, 4), 256, knots="nonuniform",
                   wrts=[(0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 1), (0, 2, 0, 0)]))
    cs.append(Case("five_var", 308, 5, 1, (2, 2, 3, 2, 2), (3, 4, 4, 3, 3), 256,
                   wrts=[(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, 0, 0, 0, 1)]))
    # dtypes: fp32 knots + fp32 coefs; mixed fp32 knots / fp64 coefs and the converse
    cs.append(Case("curve_f32", 401, 1, 2, (4,), (12,), 512, f32, f32, wrts=all_wrt(1, 2), edge_points=True))
    cs.append(Case("surface_f32knots_f64coefs", 402, 2, 3, (4, 3), (9, 8), 512, f32, f64, pdtype=f64, wrts=all_wrt(2, 1)))
    cs.append(Case("surface_f64knots_f32coefs", 403, 2, 3, (4, 3), (9, 8), 512, f64, f32, pdtype=f64, wrts=all_wrt(2, 1)))
    # larger orders / wide tables
    cs.append(Case("curve_order12", 501, 1, 2, (12,), (30,), 512, knots="nonuniform", wrts=[(0,), (1,), (3,)], edge_points=True))
    cs.append(Case("curve_many_knots", 502, 1, 3, (4,), (900,), 1024, knots="nonuniform", wrts=[(0,), (1,), (2,)], edge_points=True))
    cs.append(Case("surface_wide", 503, 2, 3, (4, 5), (300, 11), 1024, knots="nonuniform", wrts=all_wrt(2, 1)))
    return cs


class BlockCase:
    """A block of splines (reference bspy/spline_block.py): rows of (map, spline definition) over
    the block's independent variables, plus a batch of points.  Spline definitions are plain
    tuples (nInd, nDep, order, nCoef, knots, coefs) so both the reference and this package can
    build their own Spline objects from them."""

    def __init__(self, name, seed, domains, rows, n, wrts):
        rng = np.random.default_rng(seed)
        self.name = name
        self.nInd = len(domains)
        self.rows = []
        for row in rows:
            new_row = []
            for (imap, ndep, order, ncoef, cdtype) in row:
                knots = []
                for o, c, iv in zip(order, ncoef, imap):
                    lo, hi = domains[iv]
                    interior = np.sort(lo + (hi - lo) * (0.05 + 0.9 * rng.random(c - o)))
                    knots.append(np.concatenate((np.full(o, lo), interior, np.full(o, hi))).astype(np.float64))
                coefs = rng.standard_normal((ndep, *ncoef)).astype(cdtype)
                new_row.append((list(imap), (len(imap), ndep, tuple(order), tuple(ncoef), knots, coefs)))
            self.rows.append(new_row)
        self.nDep = sum(r[0][1][1] for r in self.rows)
        self.points = [lo + (hi - lo) * rng.random(n) for (lo, hi) in domains]
        self.wrts = wrts


def block_cases():
    """SplineBlock evaluation goldens: default maps, mapped
    variables, single-spline rows and a row summing three splines."""
    f64, f32 = np.float64, np.float32
    cs = []
    # [[F(u,v,w), G(u)], [h(u,v)]] with default maps (consecutive variables per row)
    cs.append(BlockCase("block_default_maps", 901, [(0.0, 1.0), (-1.0, 2.0), (0.5, 1.5), (0.0, 1.0)],
                        [[((0, 1, 2), 2, (4, 3, 2), (6, 5, 4), f64), ((3,), 2, (3,), (5,), f64)],
                         [((0, 1), 1, (4, 3), (6, 5), f64)]], 257,
                        [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (0, 0, 0, 2)]))
    # mapped variables over (s,t,u,v,w): F(u,v,w) + G(t,s) = 0, h(u,t,w,s) = 0.  (The splines of
    # a row must map to disjoint variables: the reference constructor rejects anything else,
    # spline_block.py:88-91, although its docstring example shares a variable.)
    cs.append(BlockCase("block_mapped", 902, [(0.0, 1.0), (0.0, 2.0), (-1.0, 1.0), (0.0, 1.0), (1.0, 3.0)],
                        [[((2, 3, 4), 2, (3, 4, 3), (5, 6, 4), f64), ((1, 0), 2, (4, 2), (7, 3), f64)],
                         [((2, 1, 4, 0), 1, (2, 3, 3, 2), (3, 4, 5, 3), f64)]], 193,
                        [(0, 0, 0, 0, 0), (0, 0, 1, 0, 0), (1, 0, 0, 1, 0), (0, 1, 0, 0, 0)]))
    # bicubic surfaces in the fast path: S1(a,b) + S2(d,c) + C(e), and a second row S3(b,a)
    cs.append(BlockCase("block_surfaces_sum", 903, [(0.0, 1.0), (0.0, 1.0), (0.0, 1.0), (-1.0, 1.0), (0.0, 2.0)],
                        [[((0, 1), 3, (4, 4), (16, 12), f64), ((3, 2), 3, (4, 4), (9, 10), f64), ((4,), 3, (4,), (7,), f64)],
                         [((1, 0), 2, (4, 4), (8, 8), f64)]], 1025,
                        [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 1, 0, 0), (0, 0, 0, 0, 2), (0, 0, 0, 1, 0)]))
    # float32 coefficients decide the block's result dtype (first spline of the first row)
    cs.append(BlockCase("block_f32_coefs", 904, [(0.0, 1.0), (0.0, 1.0)],
                        [[((0, 1), 2, (3, 3), (6, 6), f32)], [((1,), 1, (4,), (9,), f32), ((0,), 1, (3,), (5,), f32)]], 129,
                        [(0, 0), (0, 1)]))
    return cs


def teapot_patches(tables, which=None, dtype=np.float32):
    """Control nets of the Utah teapot's bicubic Bezier patches as (order, nCoef, knots, coefs)
    from the reference's data tables (tests/golden/reference_tables.npz: examples/teapot.py:4-346),
    arranged like the reference example does (x, z, y -> nDep 0, 1, 2; examples/teapot.py:349-358)."""
    V, P = tables["teapot_vertices"], tables["teapot_patch_index"]
    knots = np.array((0, 0, 0, 0, 1, 1, 1, 1), dtype)
    out = []
    for pi in (range(len(P)) if which is None else which):
        c = np.empty((3, 4, 4), dtype)
        for i in range(4):
            for j in range(4):
                v = V[P[pi][4 * i + j] - 1]
                c[0, i, j], c[1, i, j], c[2, i, j] = v[0], v[2], v[1]
        out.append(((4, 4), (4, 4), [knots, knots], c))
    return out


def tess_cases():
    """Tessellation batches: name -> (list of (order, nCoef, knots, coefs), u, v).
    The teapot batch is built by the caller from reference_tables.npz (teapot_patches)."""
    rng = np.random.default_rng(4242)
    out = {}
    # five order-3 x 3 patches on shared non-uniform knots, fp64, odd grid sizes
    ku = nonuniform_knots(rng, 3, 6, np.float64, 0.0, 2.0)
    kv = nonuniform_knots(rng, 3, 7, np.float64, -1.0, 1.0)
    patches = [((3, 3), (6, 7), [ku, kv], rng.standard_normal((3, 6, 7))) for _ in range(5)]
    out["o3_f64"] = (patches, np.linspace(0.0, 2.0, 11), np.linspace(-1.0, 1.0, 9))
    # two order-5 patches, fp64, grid sizes divisible by the vector width
    ku = clamped_uniform_knots(5, 9)
    kv = clamped_uniform_knots(5, 8)
    patches = [((5, 5), (9, 8), [ku, kv], rng.standard_normal((3, 9, 8))) for _ in range(2)]
    out["o5_f64"] = (patches, np.linspace(0.0, 1.0, 6), np.linspace(0.0, 1.0, 8))
    # three patches of order (2, 5) - a ruled-surface shape - and grid sizes that take the vector path
    ku = nonuniform_knots(rng, 2, 6, np.float64, 0.0, 1.0)
    kv = nonuniform_knots(rng, 5, 9, np.float64, 0.0, 3.0)
    patches = [((2, 5), (6, 9), [ku, kv], rng.standard_normal((3, 6, 9))) for _ in range(3)]
    out["o2x5_f64"] = (patches, np.linspace(0.0, 1.0, 7), np.linspace(0.0, 3.0, 10))
    return out


def basis_cases():
    """Direct bspline_values goldens: tuples
    (knots, order, u, derivativeOrder, taylorCoefs, explicit_knot_or_None)."""
    rng = np.random.default_rng(777)
    out = []
    for order in range(1, 10):
        for dtype in (np.float64, np.float32):
            ncoef = order + int(rng.integers(0, 8))
            knots = nonuniform_knots(rng, order, ncoef, dtype, -1.0, 2.5)
            lo, hi = knots[order - 1], knots[ncoef]
            us = list(lo + (hi - lo) * rng.random(6)) + [lo, hi] + list(np.unique(knots))
            for u in us:
                u = dtype(u)
                for deriv in range(0, order + 2):
                    for taylor in (False, True):
                        out.append((knots, order, u, deriv, taylor, None))
            # explicit knot argument (no search): evaluate a span's polynomial outside its span
            for _ in range(4):
                ix = int(rng.integers(order, ncoef + 1))
                if knots[ix] - knots[ix - 1] <= 0:
                    continue
                u = dtype(lo + (hi - lo) * rng.random())
                out.append((knots, order, u, int(rng.integers(0, order)), bool(rng.integers(0, 2)), ix))
    return out


def bench_spline(cfg, seed=0):
    """The BASELINE.json configs' splines: returns
    (nInd, nDep, order, nCoef, knots, coefs, dtype)."""
    rng = np.random.default_rng(seed)
    if cfg == 1:
        nind, ndep, order, ncoef, dt = 1, 1, (4,), (32,), np.float64
    elif cfg in (2, 3):
        nind, ndep, order, ncoef, dt = 2, 3, (4, 4), (64, 64), np.float64
    elif cfg == 5:
        nind, ndep, order, ncoef, dt = 3, 4, (5, 5, 5), (40, 40, 40), np.float32
    else:
        raise ValueError(cfg)
    knots = [clamped_uniform_knots(o, c, dt) for o, c in zip(order, ncoef)]
    coefs = rng.standard_normal((ndep, *ncoef)).astype(dt)
    return nind, ndep, order, ncoef, knots, coefs, dt


# ---------------------------------------------------------------------------------------------
# Scale tests (tests/test_scale_host.py, tests/test_gpu_scale.py): identical inputs for the CPU preconditions and the
# GPU checks.  Points are drawn by scale_ref.sample_points(order, nCoef, knots, n, dtype, default_rng(seed)).
# ---------------------------------------------------------------------------------------------
class ScaleFamily:
    """One kernel family of the exact-scaling-law sweep: a spline, a batch size, the BSK_VARIANT that forces the family
    and its calls (kind, wrt, kernel): kind in eval / jac / normal / curv / grid / tess / tessn / integral; `kernel` is
    what last_kernel() must name (a trailing * matches a part of it)."""

    def __init__(self, name, order, ncoef, knots, coefs, dt, n, calls, variant=None, seed=1, env=None, grid=None):
        self.name, self.order, self.nCoef, self.knots, self.coefs, self.dt = name, tuple(order), tuple(ncoef), knots, coefs, dt
        self.n, self.calls, self.variant, self.seed, self.env, self.grid = n, calls, variant, seed, env or {}, grid
        self.nInd, self.nDep = len(order), coefs.shape[0]

    @property
    def kind(self):
        return "fp32" if self.dt == np.float32 else "fp64"


def _scale_spec(order, ncoef, ndep, dt, seed, lo=-1.0, hi=1.0, uniform=False):
    rng = np.random.default_rng(seed)
    if uniform:
        knots = [clamped_uniform_knots(o, c, dt, lo, hi) for o, c in zip(order, ncoef)]
    else:
        knots = [nonuniform_knots(rng, o, c, dt, lo, hi) for o, c in zip(order, ncoef)]
    return tuple(order), tuple(ncoef), knots, rng.standard_normal((ndep, *ncoef)).astype(dt)


def _point_calls(order, ev, jac=None, extra=()):
    """value, a first derivative (variable 0) and the highest non-zero derivative (last variable), then the jacobian."""
    nind = len(order)
    first = (1,) + (0,) * (nind - 1)
    top = (0,) * (nind - 1) + (order[-1] - 1,)
    calls = [("eval", (0,) * nind, ev), ("eval", first, ev)]
    if top not in (first, (0,) * nind):
        calls.append(("eval", top, ev))
    if jac:
        calls.append(("jac", None, jac))
    return calls + list(extra)


def scale_families():
    """The enumeration of tests/test_gpu_stale_lds.py (same shapes, sizes and forcing variants), one entry per family."""
    f32, f64 = np.float32, np.float64
    P = {c.name: c for c in parity_cases()}
    fams = []

    def add(name, spec, dt, n, calls, **kw):
        fams.append(ScaleFamily(name, *spec, dt, n, calls, **kw))

    add("eval_slab2", _scale_spec((5, 3), (12, 40), 4, f32, 534), f32, (1 << 20) + 4_099,
        [("eval", (0, 0), "eval_slab2"), ("eval", (1, 0), "eval_slab2"), ("eval", (4, 0), "eval_slab2"), ("eval", (0, 2), "eval_slab2")])
    _, _, o, nc, k, cf, dt = bench_spline(2)
    add("eval_uni / jac_uni", (o, nc, k, cf), f64, 20_011, _point_calls(o, "eval_uni", "jac_uni", [("normal", None, "jac_uni")]))
    c = P["cfg2_bicubic_nonuniform"]
    add("eval_rowrot / jac_rowrot / curv_rowrot", (c.order, c.nCoef, c.knots, c.coefs), f64, 20_011,
        _point_calls(c.order, "eval_rowrot", "jac_rowrot", [("normal", None, "jac_rowrot"), ("curv", None, "curv_rowrot")]))
    add("eval_rec32", _scale_spec((4, 4), (37, 16), 4, f32, 13, -2.0, 3.0), f32, 20_011, _point_calls((4, 4), "eval_rec32"))
    add("eval_stream / jac_stream", _scale_spec((3, 3, 3), (6, 7, 5), 2, f64, 14), f64, 20_011,
        _point_calls((3, 3, 3), "eval_stream", "jac_stream"), variant="4")
    add("eval_stream_uni / jac_stream_uni, curve", _scale_spec((4,), (40,), 3, f64, 141, 0.0, 1.0, uniform=True), f64, 20_011,
        [("eval", (0,), "eval_stream_uni"), ("eval", (1,), "eval_stream_uni"), ("eval", (3,), "eval_stream_uni"), ("jac", None, "jac_stream_uni")])
    add("eval_stream_uni / jac_stream_uni, volume", _scale_spec((4, 4, 4), (8, 9, 10), 1, f64, 142, 0.0, 1.0, uniform=True), f64, 20_011,
        _point_calls((4, 4, 4), "eval_stream_uni", "jac_stream_uni"))
    add("eval_fixed / jac_fixed", (c.order, c.nCoef, c.knots, c.coefs), f64, 20_011,
        _point_calls(c.order, "eval_fixed", "jac_fixed"), variant="1")
    m = P["surface_o3x4"]
    add("eval_mixed / jac_mixed", (m.order, m.nCoef, m.knots, m.coefs), f64, 20_011, _point_calls(m.order, "eval_mixed", "jac_mixed"))
    add("eval_generic", _scale_spec((14,), (24,), 2, f64, 16), f64, 20_011,
        [("eval", (0,), "eval_generic"), ("eval", (1,), "eval_generic"), ("eval", (13,), "eval_generic")])
    add("eval_gather", _scale_spec((4, 4), (200, 150), 2, f64, 17), f64, 20_011, _point_calls((4, 4), "eval_gather*"))
    _, _, o5, nc5, k5, cf5, _ = bench_spline(5)
    for variant, kernel in (("0", "eval_cellsort, MFMA*"), ("12", "eval_cellsort, VALU*"), ("13", "eval_binned_lds*")):
        add(kernel.rstrip("*"), (o5, nc5, k5, cf5), f32, 400_003, _point_calls(o5, kernel), variant=variant)
    add("fused jacobian", _scale_spec((3, 3, 3), (38, 34, 40), 3, f32, 19, 0.0, 1.0), f32, 280_003, [("jac", None, "fused jacobian*")])
    # grids and tessellation
    g = _scale_spec((4, 4), (20, 18), 3, f64, 21)
    for what, shape in (("grid_rows vector", (40, 128)), ("grid_rows scalar", (40, 77)), ("grid_surface", (40, 40))):
        add(what, g, f64, 0, [("grid", (0, 0), what.split()[0]), ("grid", (1, 0), what.split()[0]), ("grid", (0, 3), what.split()[0])], grid=shape)
    v = P["volume_o3x4x2"]
    add("grid_generic", (v.order, v.nCoef, v.knots, v.coefs), f64, 0,
        [("grid", (0, 0, 0), "grid_generic"), ("grid", (1, 0, 0), "grid_generic"), ("grid", (0, 3, 0), "grid_generic")], grid=(13, 17, 9))
    for dt in (f32, f64):
        for form in ("hoisted 512", "hoisted 256", "normals", "mixed"):
            order = (3, 4) if form == "mixed" else (4, 4)
            kind = "tessn" if form in ("normals", "mixed") else "tess"
            add(f"tess_rows {form}, {'fp32' if dt == f32 else 'fp64'}", _scale_spec(order, (9, 8), 3, dt, 22, 0.0, 1.0), dt, 0,
                [(kind, None, f"tess_rows {form}")], grid=(24, 128), env={"BSK_TESS_T": "256"} if form == "hoisted 256" else None)
    # quadrature: one Gauss-Kronrod round in MEASURE mode
    add("integral_regions", _scale_spec((3, 4), (7, 6), 3, f64, 23, 0.0, 1.0, uniform=True), f64, 0, [("integral", None, "integral_regions")])
    return fams


# (kc, kp): coefficients x 2^kc, knots and parameters x 2^kp; the rows pattern is cycled over the dependent variables
SCALE_EXPONENTS = {"fp64": [(40, 0), (-40, 20), (0, -20)], "fp32": [(12, 0), (-12, 6), (-20, -8)]}
SCALE_ROWS = {"fp64": (30, 0, -30), "fp32": (12, 0, -12)}


def scale_fit_systems():
    """(order, rows, cols, outer, inner, seed) of the banded least-squares systems: fit_sweep, fit_sweep turned (inner 1,
    outer > 1) and fit_residual on each; the data scale 2^k."""
    return [(4, 91, 23, 3, 37, 104), (4, 91, 23, 65, 1, 104), (6, 91, 23, 1, 200, 106), (2, 91, 23, 1000, 1, 102)], (40, -40)


class ScaleSpline:
    """A spline of the shifted-domain sweep, defined on [0, 1]^nInd; scale_ref.map_domain moves it."""

    def __init__(self, name, order, ncoef, ndep, seed, uniform=True, dt=np.float64, general=("eval_stream", "jac_stream"),
                 uni=("eval_stream_uni", "jac_stream_uni")):
        self.name, self.dt, self.uniform = name, dt, uniform
        self.order, self.nCoef, self.knots, self.coefs = _scale_spec(order, ncoef, ndep, dt, seed, 0.0, 1.0, uniform)
        self.general, self.uni = general, uni


def scale_splines():
    rr, un = ("eval_rowrot", "jac_rowrot"), ("eval_uni", "jac_uni")
    _, _, o, nc, k, cf, _ = bench_spline(2)
    cfg2 = ScaleSpline("cfg2 bicubic", o, nc, 3, 0, general=rr, uni=un)
    cfg2.knots, cfg2.coefs = k, cf
    return [cfg2,
            ScaleSpline("cubic curve, 64 coefficients", (4,), (64,), 2, 602),
            ScaleSpline("order 3 volume", (3, 3, 3), (8, 9, 7), 2, 603),
            ScaleSpline("order 5 surface", (5, 5), (12, 11), 3, 604),
            ScaleSpline("cfg2 bicubic, non-uniform", (4, 4), (64, 64), 3, 605, uniform=False, general=rr, uni=un)]


def scale_splines_f32():
    """fp32 takes the uniform path at order 2 only (nothing to unclamp)."""
    return [ScaleSpline("order 2 surface, fp32", (2, 2), (40, 33), 3, 606, dt=np.float32, general=("eval_rowrot", "jac_rowrot"),
                        uni=("eval_uni", "jac_uni"))]


# (lo, width) of the shifted and stretched domains
SCALE_DOMAINS = [(0.0, 1.0), (8.0, 1.0), (33.0, 1.0), (1000.0, 64.0), (3.0, 0.125), (1000.0, 1.0), (1e6, 0.021), (-1001.0, 1.0),
                 (0.1, 3e-7), (-5e8, 1e9)]
SCALE_DOMAINS_F32 = [(0.0, 1.0), (100.0, 1.0), (0.0, 2.0 ** -10)]
SCALE_SAMPLE = 2_000


def scale_illscaled():
    """Surfaces of order 3, 4, 5 and a volume on the unclamping paths; the outermost control-point layer x 2^20."""
    return [ScaleSpline("order 3 surface", (3, 3), (9, 10), 2, 701),
            ScaleSpline("order 4 surface", (4, 4), (12, 11), 3, 702, general=("eval_rowrot", "jac_rowrot"), uni=("eval_uni", "jac_uni")),
            ScaleSpline("order 5 surface", (5, 5), (12, 13), 2, 703),
            ScaleSpline("order 3 volume", (3, 3, 3), (8, 7, 9), 2, 704)]


def scale_cases():
    """Everything the scale tests share, by part: A families / exponents / fit systems, B splines / domains, C splines."""
    return {"families": scale_families(), "exponents": SCALE_EXPONENTS, "rows": SCALE_ROWS, "fit": scale_fit_systems(),
            "splines": scale_splines(), "domains": SCALE_DOMAINS, "splines_f32": scale_splines_f32(),
            "domains_f32": SCALE_DOMAINS_F32, "sample": SCALE_SAMPLE, "illscaled": scale_illscaled()}


# ---------------------------------------------------------------------------------------------
# Scale tests of the operator families (tests/test_scale_host.py, tests/test_gpu_scale_ops.py): band (insert_knots,
# elevate, trim, clamp, differentiate), product (multiply), scan / sum (integrate, add, subtract) and roots (zeros_batch).
# ---------------------------------------------------------------------------------------------
OPERATOR_KERNELS = {"band": {"band_apply", "band_apply_line"}, "product": {"band_product_line", "band_product_tile"},
                    "sum": {"scan_apply", "scan_line", "sum_bcast"}, "roots": {"roots_flag", "roots_isolate"}}
TRIM_CLEARANCE = 2.0 ** -10         # of the domain width: how far a trim bound of these cases stays from every knot


class OpCase:
    """One public call: ``operands`` [(order, knots, coefs)] on [0, 1] (or around it, unclamped), the operation, its
    arguments, and the kernels ``LAST_PATHS`` must name on the device path, in order."""

    def __init__(self, name, family, op, operands, kernels, **args):
        self.name, self.family, self.op, self.operands, self.kernels, self.args = name, family, op, operands, list(kernels), args

    @property
    def dt(self):
        return self.operands[0][2].dtype.type

    @property
    def kind(self):
        return "fp32" if self.dt == np.float32 else "fp64"

    def replaced(self, operands, **args):
        return OpCase(self.name, self.family, self.op, operands, self.kernels, **{**self.args, **args})


def operator_knots(rng, order, ncoef, unclamped=False):
    """Sorted random knots with one double interior knot: clamped on [0, 1], or unclamped with the domain inside [-1, 2]."""
    if unclamped:
        return np.sort(rng.random(order + ncoef) * 3.0 - 1.0)
    interior = np.sort(rng.random(ncoef - order))
    if ncoef - order > 4 and order > 2:
        interior[2] = interior[1]
    return np.concatenate((order * [0.0], interior, order * [1.0]))


def operator_spline(seed, order, ncoef, ndep, dt=np.float64, unclamped=()):
    rng = np.random.default_rng(seed)
    knots = [operator_knots(rng, o, c, iv in unclamped) for iv, (o, c) in enumerate(zip(order, ncoef))]
    return tuple(order), knots, rng.standard_normal((ndep, *ncoef)).astype(dt)


def clear_bound(knots, order, at):
    """A trim bound near the fraction ``at`` of the domain: the middle of the widest knot cell whose middle lies within a
    tenth of the width of it."""
    t = np.unique(np.asarray(knots, np.float64)[order - 1:len(knots) - order + 1])
    mid, gap = 0.5 * (t[1:] + t[:-1]), np.diff(t)
    lo, width = t[0], t[-1] - t[0]
    near = np.abs(mid - (lo + at * width)) <= 0.1 * width
    return float(mid[near][np.argmax(gap[near])])


def band_cases(tag, spline, loose, new, kernel, family="band"):
    """The six band operations on variable 0 of ``spline`` (clamped) and ``loose`` (the same shape, variable 0 unclamped);
    ``new``: knots to insert."""
    order, knots, _ = spline
    rest = len(order) - 1
    pad = lambda first, fill: [first] + rest * [fill]
    bounds = [clear_bound(knots[0], order[0], 0.3), clear_bound(knots[0], order[0], 0.7)]
    k = [kernel]
    return [OpCase(f"insert_knots {tag}", family, "insert_knots", [spline], k, new=pad(list(new), [])),
            OpCase(f"elevate 1 {tag}", family, "elevate", [spline], k, m=pad(1, 0)),
            OpCase(f"elevate_and_insert_knots 3 {tag}", family, "elevate_and_insert_knots", [spline], k, m=pad(3, 0), new=pad(list(new[:5]), [])),
            OpCase(f"clamp {tag}", family, "clamp", [loose], k, left=[0], right=[0]),
            OpCase(f"trim {tag}", family, "trim", [spline], k, domain=pad(bounds, [None, None])),
            OpCase(f"differentiate {tag}", family, "differentiate", [spline], k, wrt=0)]


def product_cases(tag, a, b, indMap, kernel, types=("S", "D", "C")):
    return [OpCase(f"multiply {t} {tag}", "product", "multiply", [a, b], [kernel], indMap=indMap, productType=t) for t in types]


def operator_scale_cases():
    """Part A / C (the smallest shapes of the layout lists that still split every way) and part B (small enough for the
    Fraction references) of the operator sweep, as {"A": [OpCase], "B": [OpCase], "roots_curve": ..., "roots_b": ...}.
    A band: (5, 120, 37) odd inner extent and scalar lanes, (2, 120, 64) vector lanes, (3, 120) lines, (120, 1030) axis 0.
    A product: a line pair (120, 75) with 37 planes; a tile pair (40, 37) x (33, 41), ragged last tiles both ways.
    A scan: n = 1030, ragged chunks and more than one segment.  A sum: a surface plus a curve, broadcast."""
    f32, f64 = np.float32, np.float64
    new = np.random.default_rng(900).random(20)
    A = []
    for dt in (f64, f32):
        for ndep, ncoef in [(5, (120, 37)), (2, (120, 64)), (3, (120,)), (1, (120, 1030))]:
            order = (4, 3)[:len(ncoef)]
            tag = f"({ndep}, {', '.join(map(str, ncoef))}) {np.dtype(dt).name}"
            A += band_cases(tag, operator_spline(901, order, ncoef, ndep, dt), operator_spline(902, order, ncoef, ndep, dt, unclamped=(0,)),
                            new, "band_apply" if len(ncoef) > 1 else "band_apply_line")
    for dt in (f64, f32):
        n = np.dtype(dt).name
        A += product_cases(f"line (120, 75) x 37 planes {n}", operator_spline(903, (2, 4), (37, 120), 3, dt),
                           operator_spline(904, (3,), (75,), 3, dt), [(1, 0)], "band_product_line")
        A += product_cases(f"tile (40, 37) x (33, 41) {n}", operator_spline(905, (4, 3), (40, 37), 3, dt),
                           operator_spline(906, (3, 4), (33, 41), 3, dt), [(0, 0), (1, 1)], "band_product_tile")
        for segments in (1, 2, 5):
            A.append(OpCase(f"integrate scan_apply n 1030 segments {segments} {n}", "sum", "integrate",
                            [operator_spline(907, (4, 3), (1030, 5), 3, dt)], ["scan_apply"], wrt=0, segments=segments))
            A.append(OpCase(f"integrate scan_line n 1030 segments {segments} {n}", "sum", "integrate",
                            [operator_spline(908, (3, 4), (5, 1030), 3, dt)], ["scan_line"], wrt=1, segments=segments))
        surf = operator_spline(909, (4, 3), (40, 37), 3, dt)
        line = (surf[0][:1], surf[1][:1], np.random.default_rng(910).standard_normal((3, 40)).astype(dt))
        for op in ("add", "subtract"):
            A.append(OpCase(f"{op} surface (40, 37) and curve (40) {n}", "sum", op, [surf, line], ["sum_bcast"], indMap=[(0, 0)]))

    # part B: curves of 30 and 25 coefficients, orders 4 and 3, two components; a surface of 12 x 11 and partners
    B = []
    for dt in (f64, f32):
        n = np.dtype(dt).name
        c4, c4u = operator_spline(1, (4,), (30,), 2, dt), operator_spline(2, (4,), (30,), 2, dt, unclamped=(0,))
        c3 = operator_spline(3, (3,), (25,), 2, dt)
        s, su = operator_spline(4, (4, 3), (12, 11), 2, dt), operator_spline(5, (4, 3), (12, 11), 2, dt, unclamped=(0,))
        s2 = operator_spline(6, (3, 3), (11, 12), 2, dt)
        c9 = operator_spline(7, (3,), (9,), 2, dt)
        few = np.random.default_rng(911).random(6)
        B += band_cases(f"curve 30 {n}", c4, c4u, few, "band_apply_line")
        B += band_cases(f"surface 12 x 11 {n}", s, su, few, "band_apply")
        B += product_cases(f"curves 30 x 25 {n}", c4, c3, [(0, 0)], "band_product_line")
        B += product_cases(f"surfaces 12 x 11, 11 x 12 {n}", s, s2, [(0, 0), (1, 1)], "band_product_tile")
        B.append(OpCase(f"integrate curve 30 {n}", "sum", "integrate", [c4], ["scan_line"], wrt=0, segments=None))
        B.append(OpCase(f"integrate surface 12 x 11 {n}", "sum", "integrate", [s], ["scan_apply"], wrt=0, segments=None))
        line = (s[0][:1], s[1][:1], np.random.default_rng(913).standard_normal((2, 12)).astype(dt))
        for op in ("add", "subtract"):
            B.append(OpCase(f"{op} surface 12 x 11 and curve 12 {n}", "sum", op, [s, line], ["sum_bcast"], indMap=[(0, 0)]))
            if dt is f64:
                # the curve is raised to the surface's order and both take each other's knots: band kernels, then the sum
                # (float32 would round twice, which the one-rounding bar of part B does not cover)
                B.append(OpCase(f"{op} surface 12 x 11 and curve 9 {n}", "sum", op, [s, c9],
                                ["band_apply", "band_apply_line", "sum_bcast"], indMap=[(0, 0)]))
    # part C, band: pure knot insertion where rounding residue in structurally zero weights showed (orders 4, 8, 6 with
    # 20, 30 and 200 new knots), on lines and on a surface; parts B's cases (m = 0, 1, 3) are run as well
    C = []
    for order, ncoef, count in ((4, 40, 20), (8, 40, 30), (6, 120, 200)):
        more = np.random.default_rng(920).random(count)
        C.append(OpCase(f"insert_knots {count} into order {order} curve {ncoef}", "band", "insert_knots",
                        [operator_spline(920, (order,), (ncoef,), 2)], ["band_apply_line"], new=[list(more)]))
    C.append(OpCase("insert_knots 30 into order 8 x 3 surface 40 x 6", "band", "insert_knots",
                    [operator_spline(921, (8, 3), (40, 6), 2)], ["band_apply"], new=[list(np.random.default_rng(921).random(30)), []]))
    roots_b = {dt: operator_spline(1, (4,), (30,), 2, dt) for dt in (f64, f32)}

    def many_spans(dt):
        rng = np.random.default_rng(912)
        t = np.concatenate((4 * [0.0], np.sort(rng.random(256)), 4 * [1.0]))
        return (4,), [t], rng.standard_normal((3, len(t) - 4)).astype(dt)
    return {"A": A, "B": B, "C": C, "roots_b": roots_b, "roots_curves": {dt: many_spans(dt) for dt in (f64, f32)},
            "exponents": SCALE_EXPONENTS, "rows": SCALE_ROWS, "domains": SCALE_DOMAINS, "domains_f32": SCALE_DOMAINS_F32}


def band_pipeline(dtype):
    """(data, steps): a (2, 12, 9, 8) tensor and one band step on each of its three variables, K = 2, 4 and 8; the step on
    axis 2 shrinks, the one on axis 3 keeps the extent, the one on axis 1 grows (tests/test_host_logic.py runs them on the
    host, tests/test_gpu_refine.py on the device)."""
    rng = np.random.default_rng(11)
    data = rng.standard_normal((2, 12, 9, 8)).astype(dtype)
    steps = []
    for axis, K, n_out in ((1, 2, 15), (2, 4, 5), (3, 8, 8)):
        first = np.sort(rng.integers(0, data.shape[axis] - K + 1, n_out)).astype(np.int32)
        steps.append((axis, first, rng.random((n_out, K))))
    return data, steps


# ---------------------------------------------------------------------------------------------
# Scale tests of the cell families (tests/test_scale_cells_host.py, tests/test_gpu_scale_cells.py): zeros2, zeros3,
# project, contours and remove_knots (DESIGN.md sections 17-21).
# ---------------------------------------------------------------------------------------------
CELL_KERNELS = {"zeros2": {"roots2_flag", "roots2_isolate", "roots2_merge"}, "zeros3": {"roots3_flag", "roots3_isolate", "roots3_merge"},
                "project": {"project_seed", "project_newton"}, "contours": {"contour_flag", "contour_march"},
                "remove_knots": {"band_absmax", "band_absmax_line"}}


class CellCase:
    """One public batch call of a cell family on [0, 1]: the spline's orders and knots, the coefficients (with their batch
    axis where the call has one), the family's kernels ``LAST_PATHS`` must name on the device path, and the call's
    arguments (points, guess, levels, depth, tolerances, ...)."""

    def __init__(self, name, family, order, knots, coefs, kernels, **args):
        self.name, self.family, self.order, self.knots, self.coefs = name, family, tuple(order), list(knots), coefs
        self.kernels, self.args = set(kernels), args                # args["optional"]: kernels that may run as well

    @property
    def kind(self):
        return "fp32" if self.coefs.dtype == np.float32 else "fp64"

    def replaced(self, knots=None, coefs=None, **args):
        return CellCase(self.name, self.family, self.order, self.knots if knots is None else knots,
                        self.coefs if coefs is None else coefs, self.kernels, **{**self.args, **args})

    def with_kernels(self, kernels):
        return CellCase(self.name, self.family, self.order, self.knots, self.coefs, kernels, **self.args)


def cell_knots(rng, order, ncells, dt=np.float64):
    """Clamped knots on [0, 1] with ncells - 1 simple random interior knots per variable."""
    return [np.concatenate((k * [0.0], np.sort(rng.random(nc - 1)), k * [1.0])).astype(dt) for k, nc in zip(order, ncells)]


def _kind_name(dt):
    return np.dtype(dt).name


def zeros_scale_cases(dt):
    """zeros2 on 9 x 7 cells and zeros3 on 3 x 2 x 3 cells, B = 3 random systems per order class the kernels instantiate (the
    candidates straddle a block of 64), one of them with a zero cell in system 0; and the planted systems of
    tests/test_gpu_roots2.py (test_merge_on_a_3_by_2_grid) and tests/test_gpu_roots3.py (planted), whose zeros on shared
    edges make the merge kernels run, three times over with factors that keep the zero coefficients zero."""
    n, out = _kind_name(dt), []
    for family, ncells, orders in (("zeros2", (9, 7), [(2, 2), (3, 4), (4, 4)]), ("zeros3", (3, 2, 3), [(2, 2, 2), (3, 3, 2), (4, 4, 4)])):
        nind = len(ncells)
        flag, isolate, merge = (f"roots{nind}_{s}" for s in ("flag", "isolate", "merge"))
        for order in orders:
            rng = np.random.default_rng(1000 * nind + 100 * order[0] + 10 * order[1] + order[-1])
            knots = cell_knots(rng, order, ncells, dt)
            ncoef = [len(t) - k for t, k in zip(knots, order)]
            coefs = rng.standard_normal((3, nind, *ncoef)).astype(dt)
            out.append(CellCase(f"{family} {order} {n}", family, order, knots, coefs, {flag, isolate}))
            if order == orders[-1]:
                holed = coefs.copy()
                holed[(0, 0) + tuple(slice(0, k) for k in order)] = 0.0
                out.append(CellCase(f"{family} {order} zero cell {n}", family, order, knots, holed, {flag, isolate}, zero_cells=1))
        factors = np.array([1.0, -3.0, 0.375], dt).reshape((3,) + (1,) * (nind + 1))
        if nind == 2:
            third = 1.0 / 3.0
            p, q = np.array([1.0, 0.0, -1.0, 1.0]), np.array([1.0, -1.0, 1.0, 2.0])
            planted = np.stack([np.repeat(p[:, None], 4, axis=1), np.repeat(q[None, :], 4, axis=0)])
            knots, order = [np.array([0, 0, third, 2 * third, 1, 1.0], dt), np.array([0, 0, 0, 0.5, 1, 1, 1.0], dt)], (2, 3)
        else:
            p = np.array([1.0, -1.0, 0.0, 1.0, 2.0])
            planted = np.stack([np.broadcast_to(p[:, None, None], (5, 5, 5)), np.broadcast_to(p[None, :, None], (5, 5, 5)),
                                np.broadcast_to(p[None, None, :], (5, 5, 5))])
            knots, order = [np.array([0, 0, 0, 0.5, 0.5, 1, 1, 1.0], dt)] * 3, (3, 3, 3)
        out.append(CellCase(f"{family} planted, zeros on shared edges {n}", family, order, knots, (planted[None] * factors).astype(dt),
                            {flag, isolate, merge}))
    return out


def project_scale_cases(dt):
    """A curve of order 6 and surfaces of orders (2, 3) and (4, 4), nDep 2 and 3: graphs over the parameters plus noise (the
    splines of tests/test_gpu_project.py), 300 points of which some lie past the domain's ends, a guess per point inside
    and slightly outside the domain, and a chunk that cuts the samples into three."""
    out = []
    shapes = [((6,), (5,), 2), ((2, 3), (4, 3), 3), ((4, 4), (4, 3), 3)] if dt == np.float64 else [((6,), (5,), 3), ((4, 4), (4, 3), 2)]
    for order, ncells, ndep in shapes:
        rng = np.random.default_rng(2000 + 100 * order[0] + 10 * len(order) + ndep)
        knots = cell_knots(rng, order, ncells, dt)
        ncoef = [len(t) - k for t, k in zip(knots, order)]
        coefs = 0.3 * rng.standard_normal((ndep, *ncoef))
        for a, m in enumerate(ncoef):
            coefs[a] += np.linspace(0.0, 2.0, m).reshape([-1 if b == a else 1 for b in range(len(ncoef))])
        points = (1.0 + 1.2 * rng.standard_normal((ndep, 300))).astype(dt)
        guess = rng.uniform(-0.1, 1.1, (len(order), 300)).astype(dt)
        nsamples = int(np.prod([nc * k for nc, k in zip(ncells, order)]))
        out.append(CellCase(f"project {order} nDep {ndep} {_kind_name(dt)}", "project", order, knots, coefs.astype(dt),
                            {"project_seed", "project_newton"}, points=points, guess=guess, chunk=-(-nsamples // 3)))
    return out


def contour_scale_cases(dt):
    """Three levels of one bicubic field at depth 4 and three fields (B, n0, n1) of orders (2, 3) on 9 x 7 cells at depth 2
    (65 or more candidates: the lanes of split level 0 cross a wave)."""
    n, kernels = _kind_name(dt), {"contour_flag", "contour_march"}
    rng = np.random.default_rng(3000)
    k44 = cell_knots(rng, (4, 4), (3, 2), dt)
    c44 = rng.uniform(-1.0, 1.0, (1, 6, 5)).astype(dt)
    k23 = cell_knots(rng, (2, 3), (9, 7), dt)
    c23 = rng.uniform(-1.0, 1.0, (3, 10, 9)).astype(dt)
    return [CellCase(f"contours (4, 4) three levels depth 4 {n}", "contours", (4, 4), k44, c44, kernels, levels=np.array([-0.2, 0.0, 0.3]), depth=4),
            CellCase(f"contours (2, 3) three fields depth 2 {n}", "contours", (2, 3), k23, c23, kernels, levels=None, depth=2)]


REMOVE_TOLERANCES = (1e-12, 1e-5, 1e-2)


def remove_scale_cases(dt):
    """A coarse, smooth curve and a coarse, smooth (4, 3) surface with the knots to insert into them and the relative size of the noise
    put on the refined coefficients (between the first two tolerances): the test module refines and perturbs."""
    n, out = _kind_name(dt), []
    for tag, order, ncoef, ndep, count, kernels in (("curve", (4,), (12,), 3, (10,), {"band_absmax_line"}),
                                                     ("surface", (4, 3), (9, 8), 2, (7, 6), {"band_absmax", "band_absmax_line"})):
        rng = np.random.default_rng(4000 + len(order))
        knots = cell_knots(rng, order, [m - k + 1 for m, k in zip(ncoef, order)])
        greville = [np.array([t[i + 1:i + k].mean() for i in range(len(t) - k)]) for t, k in zip(knots, order)]
        grid = np.meshgrid(*greville, indexing="ij")
        smooth = np.stack([np.sin((2.0 + d) * sum(grid) + d) for d in range(ndep)])     # the loosest tolerance removes knots of its own
        coefs = (smooth + 2e-3 * rng.standard_normal((ndep, *ncoef))).astype(dt)
        new = [list(0.02 + 0.96 * rng.random(c)) for c in count]
        out.append(CellCase(f"remove_knots {tag} {order} {n}", "remove_knots", order, knots, coefs, kernels, new=new, noise=1e-7, seed=4100))
    return out


def cell_scale_cases():
    """Everything the cell families' scale tests share: part A's cases per family and type, the exponents and the domains."""
    A = {family: [] for family in CELL_KERNELS}
    for dt in (np.float64, np.float32):
        for c in zeros_scale_cases(dt) + project_scale_cases(dt) + contour_scale_cases(dt) + remove_scale_cases(dt):
            A[c.family].append(c)
    return {"A": A, "exponents": SCALE_EXPONENTS, "rows": SCALE_ROWS, "domains": SCALE_DOMAINS, "domains_f32": SCALE_DOMAINS_F32,
            "tolerances": REMOVE_TOLERANCES}


# ---------------------------------------------------------------------------------------------
# Normal and curvature on every kernel family, batch path and chunk (tests/test_shape_host.py, tests/test_gpu_shape.py;
# yardstick and bars: tests/shape_ref.py).
# ---------------------------------------------------------------------------------------------
class ShapeCase:
    """One spline, one batch size and the quantity to pin (kind: normal / curvature).  ``kernel``: what last_kernel() must
    name after the call (a trailing * matches a part of it); ``variant``: the BSK_VARIANT that forces the family;
    ``uniform``: a table-free uniform-knot family (its bar takes the form of test_gpu_scale.py part B); ``zero``: the result
    is exactly 0.0 wherever it is finite (a polyline's curvature)."""

    def __init__(self, name, kind, order, ncoef, knots, coefs, dt, n, kernel, variant=None, uniform=False, zero=False, seed=1):
        self.name, self.kind, self.order, self.nCoef, self.knots, self.coefs, self.dt = name, kind, tuple(order), tuple(ncoef), knots, coefs, dt
        self.n, self.kernel, self.variant, self.uniform, self.zero, self.seed = n, kernel, variant, uniform, zero, seed
        self.nInd, self.nDep = len(self.order), coefs.shape[0]

    @property
    def type(self):
        return "fp32" if self.dt == np.float32 else "fp64"

    def points(self):
        return shape_points(self.order, self.nCoef, self.knots, self.n, self.dt, self.seed)

    def sized(self, n, kernel=None):
        """The same spline and quantity on a batch of n points."""
        return ShapeCase(f"{self.name}, n {n}", self.kind, self.order, self.nCoef, self.knots, self.coefs, self.dt, n,
                         kernel or self.kernel, self.variant, self.uniform, self.zero, self.seed)


def shape_points(order, ncoef, knots, n, dt, seed):
    """n random points of the domain; point 0 lies on the low end of every variable, point 1 on the high end, point 2 on an
    interior knot of every variable that has one, point 3 has a NaN first parameter and point 4 a NaN last one."""
    rng = np.random.default_rng(seed)
    pts = []
    for iv, (k, o, c) in enumerate(zip(knots, order, ncoef)):
        k = np.asarray(k, dt)
        lo, hi = k[o - 1], k[c]
        p = np.clip((lo + (hi - lo) * rng.random(n)).astype(dt), lo, hi)
        if n > 4:
            p[0], p[1] = lo, hi
            inner = np.unique(k[o:c])
            inner = inner[(inner > lo) & (inner < hi)]
            if len(inner):
                p[2] = inner[len(inner) // 2]
            if iv == 0:
                p[3] = np.nan
            if iv == len(order) - 1:
                p[4] = np.nan
        pts.append(p)
    return pts


def graph_spec(order, ncoef, ndep, dt, seed, uniform=False, lo=0.0, hi=1.0):
    """A well-conditioned "graph plus noise" spline (as project_scale_cases): coefficient row a runs from 0 to 2 along
    variable a, plus 0.3 x standard normal noise; clamped uniform knots or the non-uniform ones of nonuniform_knots."""
    rng = np.random.default_rng(seed)
    if uniform:
        knots = [clamped_uniform_knots(o, c, dt, lo, hi) for o, c in zip(order, ncoef)]
    else:
        knots = [nonuniform_knots(rng, o, c, dt, lo, hi) for o, c in zip(order, ncoef)]
    coefs = 0.3 * rng.standard_normal((ndep, *ncoef))
    for a, m in enumerate(ncoef[:ndep]):
        coefs[a] += np.linspace(0.0, 2.0, m).reshape([-1 if b == a else 1 for b in range(len(ncoef))])
    return tuple(order), tuple(ncoef), knots, coefs.astype(dt)


SHAPE_N = 20_011
# above the cell-order cut of dispatch_jac (2^18 points): derivative passes through the cell-order pipeline, and from 2^19 on eval_slab2
SHAPE_CELL_ORDER = {270_001: "cell-order pipeline*", 530_003: "eval_slab2"}
SHAPE_PIPED = (1 << 21) + 5                     # three chunks of 2^20 through the pipelined host path
SHAPE_STAGED = 70_001                           # one chunk of the staged host path
SHAPE_DEVICE_CHUNKS = (1 << 22) + 4_099         # two chunks of the curvature device loop


@functools.lru_cache(maxsize=None)
def shape_cases():
    """{name: ShapeCase}: the normal and curvature cases per kernel family, and the batch-path cases built on three of them."""
    f32, f64 = np.float32, np.float64
    P = {c.name: c for c in parity_cases()}
    out = {}

    def add(kind, label, spec, dt, kernel, n=SHAPE_N, **kw):
        c = ShapeCase(f"{kind}: {label}", kind, *spec, dt, n, kernel, **kw)
        assert c.name not in out
        out[c.name] = c
        return c

    def parity(name):
        c = P[name]
        return c.order, c.nCoef, c.knots, c.coefs

    _, _, o2, nc2, k2, cf2, _ = bench_spline(2)
    _, _, o5, nc5, k5, cf5, _ = bench_spline(5)
    cfg2n = parity("cfg2_bicubic_nonuniform")
    o33 = graph_spec((3, 3), (9, 10), 3, f64, 801)
    o33_32 = graph_spec((3, 3), (9, 10), 3, f32, 801)
    o33u = graph_spec((3, 3), (9, 10), 3, f64, 802, uniform=True)
    l2 = graph_spec((4, 4), (200, 150), 3, f64, 803)

    # ---- normal
    N = "normal"
    add(N, "fused, table-free, cfg2", (o2, nc2, k2, cf2), f64, "jac_uni", uniform=True)
    add(N, "fused, cfg2 non-uniform", cfg2n, f64, "jac_rowrot")
    add(N, "fused, order (2, 2) fp32", graph_spec((2, 2), (40, 33), 3, f32, 804), f32, "jac_rowrot")
    add(N, "general LDS, order (3, 3)", o33, f64, "jac_stream")
    add(N, "general LDS, order (3, 3) fp32", o33_32, f32, "jac_stream")
    add(N, "general LDS, order (3, 3, 3) nDep 2", graph_spec((3, 3, 3), (6, 7, 5), 2, f64, 805), f64, "jac_stream")
    add(N, "general LDS, order (3, 3, 3) nDep 4", graph_spec((3, 3, 3), (6, 7, 5), 4, f64, 806), f64, "jac_stream")
    add(N, "table-free, order (3, 3) uniform", o33u, f64, "jac_stream_uni", uniform=True)
    add(N, "table-free, cubic curve uniform", graph_spec((4,), (40,), 2, f64, 807, uniform=True), f64, "jac_stream_uni", uniform=True)
    add(N, "fixed, cfg2 non-uniform under BSK_VARIANT=1", cfg2n, f64, "jac_fixed", variant="1")
    add(N, "fixed, order (6, 6)", graph_spec((6, 6), (10, 9), 3, f64, 808), f64, "jac_fixed")
    add(N, "fixed, order (5, 5, 5) nDep 4", graph_spec((5, 5, 5), (7, 6, 7), 4, f64, 809), f64, "jac_fixed")
    add(N, "mixed, surface_o3x4", parity("surface_o3x4"), f64, "jac_mixed")
    add(N, "mixed, order (3, 4, 2) nDep 2", graph_spec((3, 4, 2), (6, 7, 5), 2, f64, 810), f64, "jac_mixed")
    add(N, "derivative passes, four variables", graph_spec((3, 2, 4, 3), (4, 5, 6, 4), 3, f64, 811), f64, "eval_mixed")
    add(N, "derivative passes, curve order 12", parity("curve_order12"), f64, "eval_mixed")
    add(N, "derivative passes, curve order 14", graph_spec((14,), (24,), 2, f64, 812), f64, "eval_generic")
    nl2 = add(N, "L2-resident surface", l2, f64, "jac_fixed")
    for n, kernel in SHAPE_CELL_ORDER.items():
        out[nl2.sized(n).name] = nl2.sized(n, kernel)
    add(N, "fused cell-order jacobian, cfg5 fp32", (o5, nc5, k5, cf5), f32, "fused jacobian*", n=280_003)

    # ---- curvature
    C = "curvature"
    rng = np.random.default_rng(31)
    for order, ncoef in (((2, 2), (9, 7)), ((4, 4), (12, 10))):         # the splines of test_fused_curvature_orders_and_sizes
        knots = [nonuniform_knots(rng, o, c, f64, 0.0, 1.0) for o, c in zip(order, ncoef)]
        add(C, f"fused, order {order}", (order, ncoef, knots, rng.standard_normal((3, *ncoef))), f64, "curv_rowrot")
    add(C, "fused, bicubic fp32", graph_spec((4, 4), (12, 10), 3, f32, 813), f32, "curv_rowrot")
    cfused = add(C, "fused, cfg2 non-uniform", cfg2n, f64, "curv_rowrot")
    c33 = add(C, "non-fused surface, order (3, 3)", o33, f64, "jac_stream")
    add(C, "non-fused surface, order (3, 3) fp32", o33_32, f32, "jac_stream")
    add(C, "non-fused surface, order (3, 3) uniform", o33u, f64, "jac_stream_uni", uniform=True)
    add(C, "non-fused surface, surface_o3x4", parity("surface_o3x4"), f64, "jac_mixed")
    add(C, "non-fused surface, cfg2 non-uniform under BSK_VARIANT=1", cfg2n, f64, "jac_fixed", variant="1")
    cl2 = add(C, "non-fused surface, L2-resident", l2, f64, "jac_fixed")
    for n, kernel in SHAPE_CELL_ORDER.items():
        out[cl2.sized(n).name] = cl2.sized(n, kernel)
    cubic = graph_spec((4,), (40,), 2, f64, 814, uniform=True)
    add(C, "curve, cubic uniform nDep 2", cubic, f64, "eval_stream_uni", uniform=True)
    add(C, "curve, cubic uniform nDep 2, reversed", (*cubic[:3], cubic[3][:, ::-1].copy()), f64, "eval_stream_uni", uniform=True)
    add(C, "curve, order 6 nDep 3", graph_spec((6,), (20,), 3, f64, 815), f64, "eval_stream")
    add(C, "curve, order 12 nDep 2", parity("curve_order12"), f64, "eval_mixed")
    add(C, "curve, order 14 nDep 2", graph_spec((14,), (24,), 2, f64, 812), f64, "eval_generic")
    # L2-resident gather: the coefficients exceed LDS, the axis table still fits half of it (50 000 coefficients land on eval_generic)
    add(C, "curve, order 4, 2 500 coefficients nDep 4", graph_spec((4,), (2_500,), 4, f64, 816), f64, "eval_gather*")
    for ndep in (2, 3):
        add(C, f"curve, order 2 polyline nDep {ndep}", graph_spec((2,), (30,), ndep, f64, 817 + ndep), f64, "eval_stream", zero=True)

    # ---- batch paths (section 3 of the tests): the jac_stream surface, the fused cfg2 surface, the L2-resident surface
    n33 = out["normal: general LDS, order (3, 3)"]
    nfused = out["normal: fused, cfg2 non-uniform"]
    for base in (n33, nfused, nl2, c33, cfused, cl2):
        for n in (SHAPE_STAGED, SHAPE_PIPED):
            out[base.sized(n).name] = base.sized(n)
    for base in (c33, cfused):
        out[base.sized(SHAPE_DEVICE_CHUNKS).name] = base.sized(SHAPE_DEVICE_CHUNKS)
    return out
