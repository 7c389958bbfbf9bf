"""
Spline.intersect_rays and rays.cast_batch on the host path (no GPU): every golden of tests/golden/rays.npz against what is
exactly true (the certified oracle tests/zeros2_ref.py on the ray's system formed in rationals, see
tests/golden/make_golden_rays.py); the pure-Python statement of bspy_amd/rays.py against the host drivers, bit for bit; the
fused family against the parent's pipeline (materialised systems through ``roots2.zeros2_batch``), byte for byte; the
invariances (prefilter, first against all, batch, chunks, passes); the scale law; scope, arguments, the warning rule and one
rejected call per failure branch of the bsk_rays_* entry points.

The bars (derived, not tuned), in cell-local units.  uv: a reported hit r must have, F = (g_1, g_2) evaluated exactly at
the reported doubles and Y the certificate's preconditioner,
    2 |Y F(r)| <= 8 (K0 + K1 + 1) eps max_i sum_d |Y_id| S_d + 4 eps max_i max(|a_i|, |b_i|) / h_i:
DESIGN.md section 17's coupled bar with the ray's S_k, one more unit because forming a coefficient is one more rounded sum
of size <= S_k; float32 knots add one float32 spacing of max(|a_i|, |b_i|) over h_i for the final rounding of uv.
t: |t - t*| <= (|d_u S_c| delta_u + |d_v S_c| delta_v + 4 (K0 + K1) eps (C_c + |o_c|)) / |d_c| + 2 eps |t|, delta the uv bar
plus the oracle's bracket (the certificate's radius), |d S_c| the largest Bernstein coefficient of the derivative on the
cell: propagation of the root's error, de Casteljau for S_c, the subtraction and the division.  t is formed from the
unrounded uv, so the float32 term does not enter it.
"""
import ctypes
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

import bspy_amd
import zeros2_ref
from bspy_amd import _cells
from bspy_amd import _native as nv
from bspy_amd import rays, roots2
from conftest import GOLDEN, observe

EPS = float(np.finfo(np.float64).eps)
INF = float("inf")
_GOLDEN = np.load(os.path.join(GOLDEN, "rays.npz"))
NAMES = sorted({key.split("/")[0] for key in _GOLDEN.files})


def load_case(name):
    c = {key.split("/", 1)[1]: _GOLDEN[key] for key in _GOLDEN.files if key.startswith(name + "/")}
    c["name"], c["order"] = name, [int(k) for k in c["order"]]
    c["knots"] = [c["knots0"], c["knots1"]]
    c["tmin"], c["tmax"], c["kind"] = float(c["tmin"]), float(c["tmax"]), [str(k) for k in c["kind"]]
    return c


def make_spline(c, coefs=None):
    coefs = c["coefs"] if coefs is None else coefs
    return bspy_amd.Spline(2, 3, c["order"], list(coefs.shape[1:]), c["knots"], coefs)


def same(a, b):
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ goldens
_EXACT = {}


def exact_windows(c):
    if c["name"] not in _EXACT:
        b0, b1, xy = zeros2_ref.bezier_cells(c["order"], c["knots"], c["coefs"][:2])
        _, _, zz = zeros2_ref.bezier_cells(c["order"], c["knots"], c["coefs"][[2, 2]])
        _EXACT[c["name"]] = b0, b1, [[[xy[i][j][0], xy[i][j][1], zz[i][j][0]] for j in range(len(b1) - 1)] for i in range(len(b0) - 1)]
    return _EXACT[c["name"]]


def exact_system(window, fr):
    o = [Fraction(x) for x in fr.o]
    K0, K1 = len(window[0]), len(window[0][0])
    return [[[Fraction(w0) * (window[p][i][j] - o[p]) + Fraction(w1) * (window[q][i][j] - o[q]) for j in range(K1)] for i in range(K0)]
            for p, q, w0, w1 in fr.terms]


def check_golden(c, every, first, label):
    """every, first: what cast_batch returned for hits="all" and "first" (NumPy).  Counts, bars, specials."""
    K0, K1 = c["order"]
    uv, t, offsets, status = every
    fuv, ft, fcell, fcount, fstatus = first
    N = len(c["kind"])
    kdtype = np.result_type(c["knots0"].dtype, c["knots1"].dtype)
    assert uv.dtype == kdtype and fuv.dtype == kdtype and t.dtype == np.float64 and offsets.shape == (N + 1,)
    assert np.array_equal(status, fstatus) and np.array_equal(np.diff(offsets), fcount)
    b0, b1, windows = exact_windows(c)
    nc1 = len(b1) - 1
    cmax = np.abs(c["coefs"].astype(np.float64)).max(axis=(1, 2))
    dom = [(float(b[0]), float(b[-1])) for b in (b0, b1)]
    for ray in range(N):
        got = slice(int(offsets[ray]), int(offsets[ray + 1]))
        if got.stop > got.start:                           # first = the smallest t of all
            assert ft[ray] == t[got][0] and fuv[:, ray].tobytes() == uv[:, got][:, 0].tobytes()
        else:
            assert np.isnan(ft[ray]) and np.isnan(fuv[:, ray]).all() and fcell[ray] == -1
        kind = c["kind"][ray]
        if kind != "ordinary":
            want = {"miss_box": (0, 0), "miss_surface": (0, 0), "grazing": (0, 4), "grazing_generic": (0, 0), "nan": (0, 8), "zero_direction": (0, 8),
                    "flat": (0, 16), "edge": (1, 0), "corner": (1, 0)}[kind]
            assert (int(fcount[ray]), int(status[ray])) == want, (c["name"], kind, int(fcount[ray]), int(status[ray]))
            if kind in ("edge", "corner"):                 # x = u, y = v: the hit is the ray's foot, on the knot line(s)
                assert abs(float(fuv[0, ray]) - c["origins"][0, ray]) <= 64 * EPS
                assert abs(float(fuv[1, ray]) - c["origins"][1, ray]) <= 64 * EPS * max(1.0, abs(c["origins"][1, ray]))
            continue
        assert status[ray] == 0
        rows = np.flatnonzero(c["hit_ray"] == ray)
        assert got.stop - got.start == len(rows), (c["name"], ray, "count")
        fr = rays.frame(c["origins"][:, ray], c["directions"][:, ray], cmax)
        for n, row in enumerate(rows):
            cell = int(c["hit_cell"][row])
            i, j = divmod(cell, nc1)
            t0, h = (b0[i], b1[j]), (b0[i + 1] - b0[i], b1[j + 1] - b1[j])
            x, y, radius = (Fraction(float(c["hit_" + k][row])) for k in ("x", "y", "radius"))
            cert = dict(lo=(max(Fraction(0), x - radius), max(Fraction(0), y - radius)),
                        hi=(min(Fraction(1), x + radius), min(Fraction(1), y + radius)),
                        Y=[[Fraction(float(v)) for v in r] for r in c["hit_Y"][row]])
            u, v = float(uv[0, got][n]), float(uv[1, got][n])
            local = [(Fraction(u) - t0[0]) / h[0], (Fraction(v) - t0[1]) / h[1]]
            err = zeros2_ref.error_bound(exact_system(windows[i][j], fr), cert, *local)
            ys = max(sum(abs(float(cert["Y"][a][k])) * fr.S[k] for k in range(2)) for a in range(2))
            assert ys <= 1e3
            cellterm = max(max(abs(dom[a][0]), abs(dom[a][1])) / float(h[a]) for a in range(2))
            bar = 8 * (K0 + K1 + 1) * EPS * ys + 4 * EPS * cellterm
            tbar_uv = bar
            if kdtype == np.float32:
                bar += float(np.finfo(np.float32).eps) * cellterm
            observe(f"rays {label} uv error / bar", float(err) / bar, 1.0)
            comp = windows[i][j][fr.c]
            du = max(abs(float((K0 - 1) * (comp[a + 1][b] - comp[a][b]))) for a in range(K0 - 1) for b in range(K1))
            dv = max(abs(float((K1 - 1) * (comp[a][b + 1] - comp[a][b]))) for a in range(K0) for b in range(K1 - 1))
            delta = tbar_uv + float(radius)
            texact = float(c["hit_t"][row])
            tbar = ((du + dv) * delta + 4 * (K0 + K1) * EPS * (cmax[fr.c] + abs(fr.o[fr.c]))) / abs(fr.d[fr.c]) + 2 * EPS * abs(texact)
            observe(f"rays {label} t error / bar", abs(float(t[got][n]) - texact) / tbar, 1.0)


def run_both(s, c, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        every = rays.cast_batch(s, c["origins"], c["directions"], c["tmin"], c["tmax"], hits="all", **kw)
        first = rays.cast_batch(s, c["origins"], c["directions"], c["tmin"], c["tmax"], **kw)
    return every, first


@pytest.mark.parametrize("name", NAMES)
def test_golden_host(name):
    c = load_case(name)
    every, first = run_both(make_spline(c), c, _path="host")
    assert all(p.startswith("host ") for p in rays.LAST_PATHS)
    check_golden(c, every, first, "host")


def test_goldens_cover_the_cases():
    kinds = {k for name in NAMES for k in load_case(name)["kind"]}
    assert kinds == {"ordinary", "miss_box", "miss_surface", "grazing", "grazing_generic", "nan", "zero_direction", "flat", "edge", "corner"}
    assert 200 <= sum(len(load_case(name)["kind"]) for name in NAMES) <= 400             # a few hundred rays in all
    orders = {tuple(load_case(name)["order"]) for name in NAMES}
    assert {(2, 2), (3, 4), (4, 4), (4, 2)} <= orders
    two = load_case("arch_two_hits")
    assert (np.bincount(two["hit_ray"]) == 2).all()
    assert len({int(x) for x in two["hit_cell"][two["hit_ray"] == 0]}) == 2            # in different cells
    assert load_case("graph_42_f32")["coefs"].dtype == np.float32 and load_case("graph_42_f32")["knots0"].dtype == np.float32


def test_specials_are_what_they_are():
    """On the host drivers' own pairs: miss_box has no pair with or without the sign test's help; miss_surface passes the box
    test of the outer cell (the generator asserts it) and the sign test then excludes it: no pair and no hit; a grazing ray's pairs are the two crown cells, with bit 4 where the hit sits at a leaf centre and no bit and no
    hit at a generic v (the silent miss the docstring of bspy_amd/rays.py states); edge and corner are found by two or
    more cells and the merge keeps one."""
    c = load_case("arch_two_hits")
    for kind, pairs, zeros, status in (("miss_box", 0, 0, 0), ("miss_surface", 0, 0, 0), ("grazing", 2, 0, 4), ("grazing_generic", 2, 0, 0)):
        ray = c["kind"].index(kind)
        _, _, _, res = host_pass(make_spline(c), c["origins"][:, ray:ray + 1], c["directions"][:, ray:ray + 1], c["tmin"], c["tmax"])
        assert res["npairs"] == pairs, kind
        assert int(res["hits"][0]) == 0 and int(res["rstatus"][0]) == status, kind
        if res["npairs"]:
            assert (res["nodes"] > 0).all() and int(res["count"].sum()) == zeros, kind
    ray = c["kind"].index("miss_surface")                  # ... and the box test does pass: the statement's own slab test says so
    plan, rows, cmax = rays.host_tables(make_spline(c))
    fr = rays.frame(c["origins"][:, ray], c["directions"][:, ray], cmax)
    boxes = [rays.box_of([[[float(x) for x in rows[m, plan.first[0][i] + r, plan.first[1][0]:plan.first[1][0] + 2]] for r in range(3)]
                          for m in range(3)]) for i in range(plan.ncells[0])]
    assert [rays.slab_test(fr, box, c["tmin"], c["tmax"]) for box in boxes] == [True, False, False, False]
    c = load_case("edge_corner")
    for kind, cells in (("edge", 2), ("corner", 2)):
        ray = c["kind"].index(kind)
        _, _, _, res = host_pass(make_spline(c), c["origins"][:, ray:ray + 1], c["directions"][:, ray:ray + 1], c["tmin"], c["tmax"])
        found = res["pair_cell"][res["count"] > 0]
        assert len(found) >= cells and res["near"][res["count"] > 0, 0].all() and int(res["hits"][0]) == 1, kind
        assert int(res["cell"][0]) == int(found.min())                                   # the copy in the lowest cell is kept


def test_hits_lie_on_ray_and_surface():
    """Independent of the frame: S(uv) - (o + t d) is small in all three components, S by exact de Casteljau on the exact
    Bezier coefficients, for every recorded ray (oblique ones, and rays with the dominant axis c = 0, 1 and 2).  The bar:
    the uv bar's worth of the surface's derivative plus the t bar's worth of d, bounded by 1e-9 of the size of the data."""
    seen = set()
    for name in NAMES:
        c = load_case(name)
        if not len(c["hit_ray"]):
            continue
        b0, b1, windows = exact_windows(c)
        uv, t, offsets, _ = rays.cast_batch(make_spline(c), c["origins"], c["directions"], c["tmin"], c["tmax"], hits="all", _path="host")
        size = float(np.abs(c["coefs"].astype(np.float64)).max() + np.abs(c["origins"][:, np.isfinite(c["origins"]).all(axis=0)]).max())
        for ray in set(int(r) for r in c["hit_ray"]):
            o, d = c["origins"][:, ray], c["directions"][:, ray]
            seen.add(int(np.argmax(np.abs(d) + np.array([0.0, 1e-300, 2e-300]))))
            for n in range(int(offsets[ray]), int(offsets[ray + 1])):
                u, v = Fraction(float(uv[0, n])), Fraction(float(uv[1, n]))
                i = max(k for k in range(len(b0) - 1) if b0[k] <= u)
                j = max(k for k in range(len(b1) - 1) if b1[k] <= v)
                x, y = (u - b0[i]) / (b0[i + 1] - b0[i]), (v - b1[j]) / (b1[j + 1] - b1[j])
                for m in range(3):
                    gap = zeros2_ref.value2(windows[i][j][m], x, y) - (Fraction(float(o[m])) + Fraction(float(t[n])) * Fraction(float(d[m])))
                    observe("rays: |S(uv) - (o + t d)| / size of the data", abs(float(gap)) / size, 1e-6 if uv.dtype == np.float32 else 1e-9)
    assert seen == {0, 2}
    s = graph_surface((4, 4), (3, 2), seed=31)                                           # c = 1 and c = 0 on a tilted copy
    rng = np.random.default_rng(32)
    o, d = down_rays(rng, 60)
    for perm in ([2, 0, 1], [1, 2, 0]):                                                  # the surface and the rays with the axes rotated
        turned = bspy_amd.Spline(2, 3, list(s.order), list(s.nCoef), s.knots, np.asarray(s.coefs)[perm])
        a = rays.cast_batch(s, o, d, hits="all", _path="host")
        b = rays.cast_batch(turned, o[perm], d[perm], hits="all", _path="host")
        assert np.array_equal(a[2], b[2]) and a[2][-1] > 40
        assert np.abs(a[0] - b[0]).max() <= 1e-12 and np.abs(a[1] - b[1]).max() <= 1e-12 * np.abs(a[1]).max()


@pytest.mark.parametrize("name", ["graph_22", "graph_34"])
def test_reference_cross_check(name):
    """Informational in the generator, asserted here: on the recorded rays the reference's ``line.intersect(surface)`` found
    as many crossings as we find hits, and ours is within the reference's recorded error plus our bar of its (u, v)."""
    c = load_case(name)
    uv, t, offsets, _ = rays.cast_batch(make_spline(c), c["origins"], c["directions"], c["tmin"], c["tmax"], hits="all", _path="host")
    at = 0
    assert len(c["bspy_ray"]) == 3
    for ray, count in zip(c["bspy_ray"], c["bspy_count"]):
        assert int(offsets[ray + 1] - offsets[ray]) == int(count)
        for n in range(int(count)):
            ours, theirs = uv[:, int(offsets[ray]) + n], c["bspy_uv"][at]
            width = max(float(k[-1] - k[0]) for k in c["knots"])
            bar = float(c["bspy_err"][at]) + 8 * (sum(c["order"]) + 1) * EPS * 1e3 * width + 4 * EPS * max(abs(float(k[0])) + abs(float(k[-1])) for k in c["knots"])
            observe("rays: |ours - reference's| / (its recorded error + our bar)", float(np.abs(ours - theirs).max()) / bar, 1.0)
            at += 1


# ------------------------------------------------------------------------------------------ the statement
def host_pass(s, o, d, tmin, tmax, **kw):
    plan, rows, cmax = rays.host_tables(s)
    tab = rays.Tables(_cells.Host(), plan, rows, cmax)
    o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
    return plan, rows, cmax, rays.run_pass(tab, o, d, tmin, tmax, every=True, **kw)


PAIR_KEYS = ("pair_ray", "pair_cell", "roots", "near", "count", "status", "nodes")
RAY_KEYS = ("uv", "t", "cell", "hits", "rstatus")


@pytest.mark.parametrize("name", NAMES)
def test_statement_equals_host_drivers(name):
    """Pairs, roots, near, count, status, nodes per pair and first per ray, bit for bit; the keep bytes are not an output of
    ``ray_reduce``: they are pinned through hits="all", which holds exactly the kept hits in range."""
    c = load_case(name)
    plan, rows, cmax, res = host_pass(make_spline(c), c["origins"], c["directions"], c["tmin"], c["tmax"])
    st = rays.statement(rows, plan, cmax, c["origins"].astype(np.float64), c["directions"].astype(np.float64), c["tmin"], c["tmax"])
    keys = RAY_KEYS + (PAIR_KEYS if res["npairs"] else ())
    assert res["npairs"] == len(st["pair_ray"])
    for key in keys:
        assert np.array_equal(res[key], st[key], equal_nan=True) and res[key].dtype == st[key].dtype, (name, key)
    flat = [h for hits in st["all"] for h in hits]
    order = np.lexsort((res["all_cell"], res["all_t"], np.repeat(np.arange(len(c["kind"])), np.diff(res["all_off"]))))
    assert [tuple(r) for r in res["all_uv"][order]] == [(h[0], h[1]) for h in flat]
    assert list(res["all_t"][order]) == [h[2] for h in flat] and list(res["all_cell"][order]) == [h[3] for h in flat]
    if res["npairs"]:
        observe("rays: most nodes of a walk / ROOTS2_WALK", int(res["nodes"].max()) / roots2.WALK, 1.0)


# ------------------------------------------------------------------------------------------ surfaces and rays of the tests
def bezier_knots(K, breaks):
    return np.array([breaks[0]] * K + [b for b in breaks[1:-1] for _ in range(K - 1)] + [breaks[-1]] * K)


def graph_surface(order, ncells, seed=0, amp=0.1, bezier=False, dtype=np.float64):
    """z = a random spline over x = u in [0, 1], y = v in [0, 2] (Greville abscissae)."""
    rng = np.random.default_rng(seed)
    knots = []
    for K, nc, hi in zip(order, ncells, (1.0, 2.0)):
        breaks = list(np.linspace(0.0, hi, nc + 1))
        knots.append(bezier_knots(K, breaks) if bezier else np.array([0.0] * K + breaks[1:-1] + [hi] * K))
    g = [np.array([k[i + 1:i + K].mean() for i in range(len(k) - K)]) for K, k in zip(order, knots)]
    coefs = np.stack([g[0][:, None] + 0 * g[1][None, :], 0 * g[0][:, None] + g[1][None, :], amp * rng.standard_normal((len(g[0]), len(g[1])))])
    return bspy_amd.Spline(2, 3, list(order), list(coefs.shape[1:]), [k.astype(dtype) for k in knots], coefs.astype(dtype))


def arch_surface(ncells=4, bezier=True):
    """Order (3, 2), x = u in [-1, 1], y = v, z = 1 - u^2: horizontal rays cross it twice."""
    breaks = list(np.linspace(-1.0, 1.0, ncells + 1))
    k0 = bezier_knots(3, breaks) if bezier else np.array([-1.0] * 3 + breaks[1:-1] + [1.0] * 3)
    k1 = np.array([0.0, 0.0, 1.0, 1.0])
    n = len(k0) - 3
    g = np.array([k0[i + 1:i + 3].mean() for i in range(n)])
    z = np.array([1.0 - k0[i + 1] * k0[i + 2] for i in range(n)])
    coefs = np.stack([np.repeat(g[:, None], 2, 1), np.repeat(np.array([[0.0, 1.0]]), n, 0), np.repeat(z[:, None], 2, 1)])
    return bspy_amd.Spline(2, 3, [3, 2], [n, 2], [k0, k1], coefs)


def down_rays(rng, N, slope=0.3):
    """Rays from z = 3 down onto a graph surface, aimed at points of its (x, y) range and a little beyond it."""
    target = np.stack([rng.uniform(-0.05, 1.05, N), rng.uniform(-0.1, 2.1, N), np.zeros(N)])
    d = np.stack([slope * rng.standard_normal(N), slope * rng.standard_normal(N), -np.ones(N)])
    return target - 3.0 * d, d * rng.uniform(0.5, 2.0, N)


def across_rays(rng, N):
    o = np.stack([np.full(N, -3.0), rng.uniform(0.1, 0.9, N), rng.uniform(0.2, 0.85, N)])
    d = np.stack([np.ones(N), 0.01 * rng.standard_normal(N), 0.01 * rng.standard_normal(N)])
    return o, d


def materialised(s, o, d):
    """g (N, 2, n0, n1) in NumPy as the statement says: two differences, two products, one sum per coefficient."""
    data = np.asarray(s.coefs, np.float64)
    cmax = np.abs(data).max(axis=(1, 2))
    g = np.empty((o.shape[1], 2) + data.shape[1:])
    for ray in range(o.shape[1]):
        fr = rays.frame(o[:, ray], d[:, ray], cmax)
        for k, (p, q, w0, w1) in enumerate(fr.terms):
            g[ray, k] = w0 * (data[p] - fr.o[p]) + w1 * (data[q] - fr.o[q])
    return g


def parent_pipeline_case(which):
    rng = np.random.default_rng(5)
    if which == "bicubic":
        s = graph_surface((4, 4), (3, 2), seed=11, bezier=True)
        o, d = down_rays(rng, 200)
    else:
        s = arch_surface()
        o, d = across_rays(rng, 200)
    system = bspy_amd.Spline(2, 2, list(s.order), list(s.nCoef), s.knots, np.zeros((2,) + tuple(s.nCoef)))
    return s, o, d, system, materialised(s, o, d)


def compare_with_parent(s, o, d, values, offsets, uv, mine):
    for ray in range(o.shape[1]):
        theirs = values[int(offsets[ray]):int(offsets[ray + 1])]
        ours = uv[:, int(mine[ray]):int(mine[ray + 1])].T
        ours = ours[np.lexsort((ours[:, 1], ours[:, 0]))]
        assert np.ascontiguousarray(ours).tobytes() == np.ascontiguousarray(theirs).tobytes(), ray


@pytest.mark.parametrize("which", ["bicubic", "arch"])
def test_against_the_parents_pipeline(which):
    """Surfaces whose knots are in Bezier form (no band step): the fused family gives, per ray, exactly the (u, v) bytes of
    ``roots2.zeros2_batch`` on the materialised systems."""
    s, o, d, system, g = parent_pipeline_case(which)
    uv, t, mine, status = rays.cast_batch(s, o, d, tmin=-INF, hits="all", _path="host")
    assert not any("extract" in p for p in rays.LAST_PATHS) and not status.any()
    values, offsets, cells, zstatus = roots2.zeros2_batch(system, coefs=g, _path="host")
    assert not zstatus.any() and len(cells) == 0
    assert mine[-1] == offsets[-1] and mine[-1] >= (150 if which == "bicubic" else 390)
    compare_with_parent(s, o, d, values, offsets, uv, mine)


# ------------------------------------------------------------------------------------------ invariance
def test_prefilter_changes_nothing_but_time():
    rng = np.random.default_rng(8)
    s = graph_surface((4, 4), (3, 2), seed=12)
    o, d = down_rays(rng, 10_000)
    a = rays.cast_batch(s, o, d, _path="host")
    b = rays.cast_batch(s, o, d, _path="host", _prefilter=False)
    assert same(a, b) and 5_000 < int((a[3] > 0).sum()) < 10_000
    s = arch_surface(bezier=False)
    o, d = across_rays(rng, 500)
    for tmin, tmax in ((0.0, INF), (3.0, INF), (-INF, 3.0), (2.5, 3.5)):
        assert same(rays.cast_batch(s, o, d, tmin, tmax, hits="all", _path="host"),
                    rays.cast_batch(s, o, d, tmin, tmax, hits="all", _path="host", _prefilter=False))


def test_first_is_the_smallest_t_of_all():
    rng = np.random.default_rng(9)
    s = arch_surface(bezier=False)
    o, d = across_rays(rng, 300)
    uv, t, cell, count, status = rays.cast_batch(s, o, d, _path="host")
    auv, at, off, astatus = rays.cast_batch(s, o, d, hits="all", _path="host")
    assert np.array_equal(np.diff(off), count) and (count == 2).all() and np.array_equal(status, astatus)
    assert np.array_equal(at[off[:-1]], t) and np.array_equal(auv[:, off[:-1]], uv) and (np.diff(at.reshape(-1, 2), axis=1) > 0).all()
    uv3, t3, _, count3, _ = rays.cast_batch(s, o, d, tmin=3.0, _path="host")            # tmin between the two hits
    assert (count3 == 1).all() and np.array_equal(t3, at[off[:-1] + 1]) and np.array_equal(uv3, auv[:, off[:-1] + 1])


def test_batch_chunk_and_pass_invariance():
    rng = np.random.default_rng(10)
    s = graph_surface((3, 4), (3, 2), seed=13)
    o, d = down_rays(rng, 300)
    o[:, 100] = np.nan
    whole = rays.cast_batch(s, o, d, _path="host")
    perm = rng.permutation(300)
    moved = rays.cast_batch(s, o[:, perm], d[:, perm], _path="host")
    assert same([np.asarray(a)[..., perm] for a in whole], moved)
    for ray in (0, 100, 299):
        assert same([np.asarray(a)[..., ray:ray + 1] for a in whole], rays.cast_batch(s, o[:, ray:ray + 1], d[:, ray:ray + 1], _path="host"))
    every = rays.cast_batch(s, o, d, hits="all", _path="host")
    for chunk in (6, 3, 2):                                # 1, 2 and 3 chunks of the 6 cells
        assert same(whole, rays.cast_batch(s, o, d, _path="host", _chunk=chunk))
        assert same(every, rays.cast_batch(s, o, d, hits="all", _path="host", _chunk=chunk, _pass=64))
    assert same(whole, rays.cast_batch(s, o, d, _path="host", _pass=64))
    assert rays.LAST_PATHS.count("host ray_count") == 5
    assert same(whole, rays.cast_batch(s, o, d, _path="host", _pairs=40))                 # passes halved until the pairs fit
    assert rays.LAST_PATHS.count("host ray_count") > 5


@pytest.mark.parametrize("k,m", [(-40, 3), (20, -7), (40, 11)])
def test_scale_law(k, m):
    """Coefficients and origins x 2^k, directions x 2^m: uv, cell, count, status unchanged and t x 2^(k - m), bit for bit."""
    rng = np.random.default_rng(14)
    for s, (o, d) in ((graph_surface((4, 4), (3, 2), seed=15), down_rays(rng, 200)), (arch_surface(bezier=False), across_rays(rng, 100))):
        big = bspy_amd.Spline(2, 3, list(s.order), list(s.nCoef), s.knots, np.asarray(s.coefs) * 2.0 ** k)
        for hits in ("first", "all"):
            a = rays.cast_batch(s, o, d, tmin=1.5, tmax=40.0, hits=hits, _path="host")
            b = rays.cast_batch(big, o * 2.0 ** k, d * 2.0 ** m, tmin=1.5 * 2.0 ** (k - m), tmax=40.0 * 2.0 ** (k - m), hits=hits, _path="host")
            assert same([a[0], a[1] * 2.0 ** (k - m)] + list(a[2:]), b)
            assert np.isfinite(a[1]).sum() > 50


# ------------------------------------------------------------------------------------------ scope and semantics
def test_scope_and_arguments():
    s = graph_surface((4, 4), (3, 2))
    o, d = down_rays(np.random.default_rng(1), 6)
    curve = bspy_amd.Spline(1, 3, [3], [4], [np.array([0, 0, 0, 0.5, 1, 1, 1.0])], np.zeros((3, 4)))
    plane = bspy_amd.Spline(2, 2, [2, 2], [2, 2], [np.array([0, 0, 1, 1.0])] * 2, np.zeros((2, 2, 2)))
    quintic = bspy_amd.Spline(2, 3, [5, 2], [5, 2], [np.array([0.0] * 5 + [1.0] * 5), np.array([0, 0, 1, 1.0])], np.zeros((3, 5, 2)))
    for bad in (curve, plane, quintic):
        with pytest.raises(NotImplementedError, match="surfaces .nInd 2, nDep 3. of orders 2 to 4"):
            bad.intersect_rays(o, d)
        with pytest.raises(NotImplementedError):
            rays.cast_batch(bad, o, d)
    with pytest.raises(ValueError, match="shape"):
        rays.cast_batch(s, o[:2], d[:2])
    with pytest.raises(ValueError, match="shape"):
        rays.cast_batch(s, o, d[:, :3])
    with pytest.raises(ValueError, match="shape"):
        s.intersect_rays(o[:2], d[:2])
    with pytest.raises(TypeError):
        rays.cast_batch(s, o.astype(np.int64), d)
    with pytest.raises(ValueError, match="hits"):
        rays.cast_batch(s, o, d, hits="any")
    with pytest.raises(ValueError, match="_path"):
        rays.cast_batch(s, o, d, _path="gpu")
    with pytest.raises(ValueError, match="NaN"):
        rays.cast_batch(s, o, d, tmin=float("nan"))
    with pytest.raises(ValueError, match=">= 1"):
        rays.cast_batch(s, o, d, _chunk=0)
    empty = rays.cast_batch(s, o[:, :0], d[:, :0], _path="host")
    assert [a.shape for a in empty] == [(2, 0), (0,), (0,), (0,), (0,)]
    assert rays.cast_batch(s, o[:, :0], d[:, :0], hits="all", _path="host")[2].tolist() == [0]


def test_shapes_dtypes_and_the_warning_rule():
    s = graph_surface((4, 2), (3, 2), seed=3)
    rng = np.random.default_rng(2)
    o = np.stack([rng.uniform(0.1, 0.9, (4, 5)), rng.uniform(0.1, 1.9, (4, 5)), np.full((4, 5), 3.0)])
    d = np.zeros((3, 4, 5))
    d[2] = -1.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        uv, t = s.intersect_rays(o, d, _path="host")
        uv32, t32 = s.intersect_rays(o.astype(np.float32), d.astype(np.float32), _path="host")
    assert uv.shape == (2, 4, 5) and t.shape == (4, 5) and uv.dtype == np.float64 and t.dtype == np.float64
    assert np.abs(uv[0] - o[0]).max() <= 8 * EPS and np.abs(uv[1] - o[1]).max() <= 16 * EPS       # x = u, y = v
    assert t32.dtype == np.float64 and np.abs(uv32 - uv).max() < 1e-6
    o[0, 1, 2] = np.inf
    with pytest.warns(RuntimeWarning, match="1 of 20 rays carry a status bit.*flat index 7: ray not finite") as seen:
        uv, t = s.intersect_rays(o, d, _path="host")
    assert len(seen) == 1 and np.isnan(t[1, 2]) and np.isnan(uv[:, 1, 2]).all() and np.isfinite(t).sum() == 19
    far = o.copy()
    far[0] = 7.0                                           # every ray misses: no hit is no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        uv, t = s.intersect_rays(far, d, _path="host")
    assert np.isnan(t).all() and rays.LAST_PATHS[-1] == "host ray_count"                 # the later launches are skipped


def test_exported_family():
    L = nv.lib()
    family = [n for n in nv.PRODUCT_SYMBOLS if n.startswith("bsk_rays_")]
    assert len(family) == 11 and all(hasattr(L, n) for n in family)
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bspy_amd.h")).read()
    import re
    assert set(re.findall(r"\b(bsk_rays_[a-z_]+)\s*\(", header)) == set(family)


# ------------------------------------------------------------------------------------------ rejected calls
def _abi_args():
    """Valid arguments of the five host entry points on a 1 x 1 bilinear cell and one ray."""
    keep = dict(rows=np.zeros((3, 2, 2)), first=np.zeros(1, np.int32), breaks=np.array([0.0, 1.0]), cmax=np.ones(3), o=np.zeros((3, 1)),
                d=np.ones((3, 1)), boxes=np.zeros((1, 6)), partial=np.zeros(1, np.int32), skipped=np.zeros(1, np.uint8),
                offset=np.zeros(1, np.int64), pair=np.zeros(1, np.int32), roots=np.zeros((1, 2, 2)), near=np.zeros((1, 2), np.uint8),
                count=np.zeros(1, np.int32), status=np.zeros(1, np.uint8), nodes=np.zeros(1, np.int32), pstart=np.array([0, 1], np.int64),
                uv=np.zeros((2, 1)), t=np.zeros(1), cell=np.zeros(1, np.int32), hits=np.zeros(1, np.int32))
    p = {k: v.ctypes.data for k, v in keep.items()}
    surface = [2, 2, p["rows"], 2, 2, 1, 1, p["first"], p["first"]]
    ray = [p["cmax"], p["o"], p["d"], 1]
    search = surface + ray + [0.0, INF, 1, 1, p["boxes"]]
    calls = {
        "boxes": surface + [p["boxes"]],
        "count": search + [p["partial"], p["skipped"]],
        "emit": search + [p["offset"], p["pair"], p["pair"], 1],
        "isolate": surface + [p["breaks"], p["breaks"]] + ray + [p["pair"], p["pair"], 1, p["roots"], p["near"], p["count"], p["status"], p["nodes"]],
        "reduce": surface + [p["breaks"], p["breaks"]] + ray + [0.0, INF, p["pstart"], p["pair"], 1, p["roots"], p["near"], p["count"],
                                                               p["status"], p["skipped"], 0, None, 0, p["uv"], p["t"], p["cell"], p["hits"],
                                                               p["status"]],
    }
    return keep, calls


ABI_COMMON = [(0, 1, nv.BSK_ERR_INVALID, "orders must be >= 2"), (1, 5, nv.BSK_ERR_UNSUPPORTED, "order above 4"),
              (2, None, nv.BSK_ERR_INVALID, "NULL argument"), (5, 0, nv.BSK_ERR_INVALID, "nc0 and nc1 must be >= 1"),
              (3, 1, nv.BSK_ERR_INVALID, "the rows must hold one cell"), (5, 1 << 40, nv.BSK_ERR_INVALID, "array too large")]
ABI_RAYS = [(9, None, nv.BSK_ERR_INVALID, "NULL argument"), (12, 0, nv.BSK_ERR_INVALID, "nrays must be in")]
ABI_OWN = {
    "boxes": [(9, None, nv.BSK_ERR_INVALID, "NULL argument")],
    "count": ABI_RAYS + [(17, None, nv.BSK_ERR_INVALID, "NULL argument"), (18, None, nv.BSK_ERR_INVALID, "NULL argument"),
                         (15, 0, nv.BSK_ERR_INVALID, "chunk must be >= 1"), (5, 70000, nv.BSK_ERR_INVALID, "more than 65535 chunks")],
    "emit": ABI_RAYS + [(18, None, nv.BSK_ERR_INVALID, "NULL argument"), (15, 0, nv.BSK_ERR_INVALID, "chunk must be >= 1"),
                        (21, 0, nv.BSK_ERR_INVALID, "npairs must be >= 1"), (5, 70000, nv.BSK_ERR_INVALID, "more than 65535 chunks")],
    "isolate": [(9, None, nv.BSK_ERR_INVALID, "NULL argument"), (14, 0, nv.BSK_ERR_INVALID, "nrays must be in"),
                (15, None, nv.BSK_ERR_INVALID, "NULL argument"), (17, 0, nv.BSK_ERR_INVALID, "npairs must be >= 1")],
    "reduce": [(10, None, nv.BSK_ERR_INVALID, "NULL argument"), (14, 0, nv.BSK_ERR_INVALID, "nrays must be in"),
               (17, None, nv.BSK_ERR_INVALID, "NULL argument"), (19, 0, nv.BSK_ERR_INVALID, "npairs must be >= 1"),
               (25, 1, nv.BSK_ERR_INVALID, "NULL argument"), (32, None, nv.BSK_ERR_INVALID, "NULL argument"),
               ((25, 26), (1, "pstart"), nv.BSK_ERR_INVALID, "nhits must be >= 1")],
}


@pytest.mark.parametrize("entry", sorted(ABI_OWN))
def test_rejected_calls(entry):
    """One rejected call per failure branch of the host entry points (the device twins run the same checks in the same
    function; tests/test_gpu_rays.py calls them), then the valid call."""
    L = nv.lib()
    keep, calls = _abi_args()
    fn = getattr(L, f"bsk_rays_{entry}_host")
    for at, value, status, text in ABI_COMMON + ABI_OWN[entry]:
        args = list(calls[entry])
        if isinstance(at, tuple):                          # several arguments at once; a name stands for that valid buffer
            for where, what in zip(at, value):
                args[where] = keep[what].ctypes.data if isinstance(what, str) else what
        else:
            args[at] = value
        assert fn(*args) == status, (entry, at)
        message = L.bsk_last_error().decode()
        assert message.startswith(f"bsk_rays_{entry}_host: ") and text in message, (entry, at, message)
    assert fn(*calls[entry]) == nv.BSK_OK
    assert L.bsk_rays_last_kernel().decode().startswith("host ray_" + entry)
