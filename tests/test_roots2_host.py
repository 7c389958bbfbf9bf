"""
Spline.zeros2 and roots2.zeros2_batch on the host path (no GPU): every golden of tests/golden/roots2.npz against what is
exactly true (the certified oracle tests/zeros2_ref.py for coupled systems, the exact 1-D roots of tests/zeros_ref.py for
separable systems and curve minus line) and, where the reference was complete, against the reference's zeros; the oracle's
own cross-checks; the semantics file; the pure-Python statement of the arithmetic in bspy_amd/roots2.py against the host
drivers, bit for bit; the node bound; the batched call; argument checks of the bsk_roots2_* entry points.

The bars (derived, not tuned).  Bivariate de Casteljau of K0 + K1 - 2 levels in fp64 is within (K0 + K1) eps S_d of f_d,
S_d = max |coefficient|; Newton therefore stops where |F_d| <= (K0 + K1) eps S_d or so, and with the certified
preconditioner Y the zero r* is within 2 |Y F(r)| of r (zeros2_ref.certify).  With a factor 4 for second-order terms and
the cell mapping a reported zero r of a coupled case must have, in cell-local units,
    2 |Y F(r)| <= 8 (K0 + K1) eps max_i sum_d |Y_id| S_d + 4 eps max_i max(|a_i|, |b_i|) / h_i,
F evaluated exactly at the reported doubles, [a_i, b_i] the domain and h_i the cell's width along axis i; float32 knots add
one float32 spacing of max(|a_i|, |b_i|) over h_i for the final rounding.  Separable systems: the 1-D bar ``delta`` of
test_roots_host.py per axis against the exact brackets.  Curve minus line: u against its 1-D bracket, and
|a(u) - b(v)| <= 8 K eps S (max-norm, K the curve's order), evaluated exactly.
"""
import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import bspy_amd
import zeros2_ref
import zeros_ref
from bspy_amd import _native as nv
from bspy_amd import roots, roots2
from conftest import GOLDEN, observe

EPS = float(np.finfo(np.float64).eps)
_GOLDEN = np.load(os.path.join(GOLDEN, "roots2.npz"))
NAMES = sorted({key.split("/")[0] for key in _GOLDEN.files})
SMALL = ["rand_22", "rand_42", "cubic_minus_cubic"]             # the goldens regenerated from the oracle here


def load_case(name, golden=None):
    golden = _GOLDEN if golden is None else golden
    c = {key.split("/", 1)[1]: golden[key] for key in golden.files if key.startswith(name + "/")}
    c["name"], c["kind"], c["order"] = name, str(c["kind"]), [int(k) for k in c["order"]]
    c["knots"] = [c["knots0"], c["knots1"]]
    return c


def make_spline(c, coefs=None):
    coefs = c["coefs"] if coefs is None else coefs
    return bspy_amd.Spline(2, 2, c["order"], list(coefs.shape[1:]), c["knots"], coefs)


def split_result(found):
    return [r for r in found if not isinstance(r, tuple)], [r for r in found if isinstance(r, tuple)]


def bits(found):
    return [np.asarray(r).tobytes() for r in found]


def pair(points, exact):
    """The reported zero nearest to every exact one (max-norm): one to one, since the cases keep their zeros apart."""
    points = np.array(points, np.float64).reshape(-1, 2)
    at = [int(np.abs(points - e).max(axis=1).argmin()) for e in exact]
    assert sorted(at) == list(range(len(exact))), "the reported zeros do not pair one to one with the exact ones"
    return points[at]


def delta_1d(order, knots, coefs, fprime, kdtype):
    """``delta`` of test_roots_host.py for one root of a 1-D spline."""
    k, t = int(order), knots
    end = max(abs(float(t[k - 1])), abs(float(t[len(t) - k])))
    bar = 4.0 * EPS * end
    if fprime != 0.0:
        bar += 8.0 * k * EPS * float(np.abs(coefs).max()) / abs(float(fprime))
    if kdtype == np.float32:
        bar += float(np.spacing(np.float32(end)))
    return bar


def check_golden(c, found, label):
    """Counts equal the exact counts; every zero within its bar of what is exactly true; where the reference was complete,
    within bar + ref_dev of the reference's zero.  Returns the worst error / bar."""
    points, tuples = split_result(found)
    kdtype = np.result_type(c["knots0"].dtype, c["knots1"].dtype)
    assert all(isinstance(r, np.ndarray) and r.shape == (2,) and r.dtype == kdtype for r in points), "zeros come in the knots' dtype"
    assert len(points) == len(c["exact_uv"]), f"{c['name']}: {len(points)} zeros, exactly {len(c['exact_uv'])}"
    assert [[float(a[0]), float(b[0]), float(a[1]), float(b[1])] for a, b in tuples] == c["exact_cells"].tolist()
    keys = [(float(r[0][0]), float(r[0][1])) if isinstance(r, tuple) else (float(r[0]), float(r[1])) for r in found]
    assert keys == sorted(keys), "sorted by (u, v)"
    if not len(points):
        return 0.0
    got = pair(points, c["exact_uv"])
    K0, K1 = c["order"]
    S = [float(np.abs(comp.astype(np.float64)).max()) for comp in c["coefs"]]
    ends = [max(abs(float(t[k - 1])), abs(float(t[len(t) - k]))) for k, t in zip(c["order"], c["knots"])]
    bars = np.zeros((len(got), 2))                              # per zero and axis, in the parameters
    worst = 0.0
    if c["kind"] in ("coupled", "zero"):
        b0, b1, cells = zeros2_ref.bezier_cells(c["order"], c["knots"], c["coefs"])
        for n, r in enumerate(got):
            i, j = (int(v) for v in c["cert_cell"][n])
            t0, h = (b0[i], b1[j]), (b0[i + 1] - b0[i], b1[j + 1] - b1[j])
            x, y, radius = Fraction(float(c["cert_xy"][n][0])), Fraction(float(c["cert_xy"][n][1])), Fraction(float(c["cert_radius"][n]))
            Y = [[Fraction(float(v)) for v in row] for row in c["cert_Y"][n]]
            cert = dict(lo=(max(0, x - radius), max(0, y - radius)), hi=(min(1, x + radius), min(1, y + radius)), Y=Y)
            at = [(Fraction(float(r[d])) - t0[d]) / h[d] for d in range(2)]
            err = float(zeros2_ref.error_bound(cells[i][j], cert, *at))
            bar = 8.0 * (K0 + K1) * EPS * max(sum(abs(float(Y[k][d])) * S[d] for d in range(2)) for k in range(2)) \
                + 4.0 * EPS * max(ends[d] / float(h[d]) for d in range(2))
            if kdtype == np.float32:
                bar += max(float(np.spacing(np.float32(ends[d]))) / float(h[d]) for d in range(2))
            worst = max(worst, err / bar)
            bars[n] = [bar * float(h[0]), bar * float(h[1])]
    elif c["kind"] in ("separable", "line"):
        axes = (("u", 0), ("v", 1)) if c["kind"] == "separable" else (("u", 0),)
        for n, (r, e) in enumerate(zip(got, c["exact_uv"])):
            for prefix, d in axes:
                lo, hi = c[prefix + "_lo"], c[prefix + "_hi"]
                m = int(np.abs(0.5 * (lo + hi) - e[d]).argmin())
                bar = delta_1d(c[prefix + "_order"], c[prefix + "_knots"], c[prefix + "_coefs"], c[prefix + "_fprime"][m], kdtype)
                err = max(0.0, float(lo[m]) - float(r[d]), float(r[d]) - float(hi[m]))
                worst = max(worst, err / bar)
                bars[n, d] = bar
        if c["kind"] == "line":
            b0, b1, cells = zeros2_ref.bezier_cells(c["order"], c["knots"], c["coefs"])
            residual_bar = 8.0 * K0 * EPS * max(S)
            for n, r in enumerate(got):
                i = max(i for i in range(len(b0) - 1) if b0[i] <= Fraction(float(r[0])))
                i = min(i, len(b0) - 2)
                at = [(Fraction(float(r[0])) - b0[i]) / (b0[i + 1] - b0[i]), (Fraction(float(r[1])) - b1[0]) / (b1[1] - b1[0])]
                residual = max(abs(float(zeros2_ref.value2(comp, *at))) for comp in cells[i][0])
                worst = max(worst, residual / residual_bar)
                bars[n, 1] = np.inf                             # v is pinned by the residual, not by a bracket
    if c["ref_complete"]:
        ref = pair(c["ref_roots"], c["exact_uv"])
        assert (np.abs(got - ref) <= bars + float(c["ref_dev"])).all(), f"{c['name']}: against the reference"
    print(f"{label} {c['name']}: {len(points)} zeros, {len(tuples)} zero cells, worst error / bar {worst:.3e}")
    observe(f"{label} error / bar ({c['kind']}, {'float32' if kdtype == np.float32 else 'float64'} knots)", worst, 1.0)
    return worst


# ------------------------------------------------------------------------------------------ goldens
def test_goldens_cover_the_issue():
    cases = [load_case(n) for n in NAMES]
    assert {c["kind"] for c in cases} == {"coupled", "separable", "line", "zero", "tangent", "empty"}
    coupled = [c for c in cases if c["kind"] == "coupled"]
    assert {tuple(c["order"]) for c in coupled} >= {(2, 2), (3, 4), (4, 4), (4, 2), (5, 5)}
    assert any(c["coefs"].dtype == np.float32 for c in coupled) and any(c["knots0"].dtype == np.float32 for c in coupled)
    assert any(len(np.unique(c["knots0"][4:-4])) < len(c["knots0"][4:-4]) for c in coupled if c["order"] == [4, 4]), "repeated interior knots"
    counted = [c for c in cases if c["kind"] in ("coupled", "separable", "line")]
    assert 4 * sum(bool(c["ref_complete"]) for c in counted) >= 3 * len(counted)
    assert all(c["coefs"].shape[1] <= 8 and c["coefs"].shape[2] <= 8 for c in cases)
    knots = load_case("sep_knots_22")
    u, v = knots["exact_uv"][:, 0], knots["exact_uv"][:, 1]
    assert ((u == 0.5) & (v == 0.5)).any() and (v == 0.0).any() and ((u == 0.125) & (v == 0.5)).any()      # corner, boundary, knot line


@pytest.mark.parametrize("name", NAMES)
def test_golden_host(name):
    c = load_case(name)
    if c["kind"] == "tangent":
        with pytest.raises(ValueError, match=r"zeros2: (tangential or singular zero|zeros not isolated)"):
            make_spline(c).zeros2(_path="host")
        *_, status = roots2.zeros2_batch(make_spline(c), _path="host")
        assert status.max() & (roots2.STATUS_TANGENT | roots2.STATUS_WALK)
        return
    found = make_spline(c).zeros2(_path="host")
    assert all(p.startswith("host ") for p in roots2.LAST_PATHS) and "host roots2_flag" in roots2.LAST_PATHS
    assert nv.lib().bsk_roots2_last_kernel().decode() == roots2.LAST_PATHS[-1]
    check_golden(c, found, "zeros2 host")
    assert bits(make_spline(c).zeros2(_path="host")) == bits(found), "two runs differ"
    assert bits(make_spline(c).zeros2()) == bits(found)                    # few cells: the host


@pytest.mark.parametrize("name", SMALL)
def test_golden_is_the_yardstick(name):
    c = load_case(name)
    exact = zeros2_ref.zeros(c["order"], c["knots"], c["coefs"])
    assert [list(z["cell"]) for z in exact] == c["cert_cell"].tolist()
    assert [[float(z["x"]), float(z["y"])] for z in exact] == c["cert_xy"].tolist()
    assert [float(z["radius"]) for z in exact] == c["cert_radius"].tolist()
    assert [[[float(v) for v in row] for row in z["Y"]] for z in exact] == c["cert_Y"].tolist()
    assert [[float(z["t0"][0] + z["x"] * z["h"][0]), float(z["t0"][1] + z["y"] * z["h"][1])] for z in exact] == c["exact_uv"].tolist()


def test_oracle_on_a_separable_system():
    """f = p(u), g = q(v): the certified zeros are the product of the exact roots of p and q."""
    c = load_case("sep_43")
    exact = zeros2_ref.zeros(c["order"], c["knots"], c["coefs"])
    p = zeros_ref.roots(c["order"][0], c["knots0"], c["coefs"][0][:, 0])["brackets"]
    q = zeros_ref.roots(c["order"][1], c["knots1"], c["coefs"][1][0, :])["brackets"]
    assert len(exact) == len(p) * len(q) > 1
    product = sorted((a, b) for a in p for b in q)
    for z, ((ulo, uhi), (vlo, vhi)) in zip(exact, product):
        box = [(z["t0"][d] + z["lo"][d] * z["h"][d], z["t0"][d] + z["hi"][d] * z["h"][d]) for d in range(2)]
        assert box[0][0] <= ulo <= uhi <= box[0][1] and box[1][0] <= vlo <= vhi <= box[1][1]      # the one zero of the box


def test_oracle_on_curve_minus_line():
    """a(u) - p0 - v d: the certified zeros have the exact roots of n . (a(u) - p0) as their u."""
    c = load_case("cubic_minus_line")
    exact = zeros2_ref.zeros(c["order"], c["knots"], c["coefs"])
    assert len(exact) == len(c["u_lo"]) > 1
    for z, lo, hi in zip(exact, c["u_lo"], c["u_hi"]):
        assert z["t0"][0] + z["lo"][0] * z["h"][0] <= Fraction(float(lo)) and Fraction(float(hi)) <= z["t0"][0] + z["hi"][0] * z["h"][0]
    one = zeros_ref.roots(int(c["u_order"]), c["u_knots"], c["u_coefs"])
    assert len(one["brackets"]) >= len(exact)                              # the others meet the line outside 0 <= v <= 1


def test_semantics():
    with open(os.path.join(GOLDEN, "roots2_semantics.json")) as f:
        records = json.load(f)
    assert {r["name"] for r in records} >= {"nind_ne_ndep", "no_zeros", "one_zero"}
    for r in records:
        s = r["spline"]
        coefs = np.array(s["coefs"])
        spline = bspy_amd.Spline(2, len(coefs), s["order"], list(coefs.shape[1:]), [np.array(k) for k in s["knots"]], coefs)
        if r["error"] is not None:
            with pytest.raises(ValueError) as info:
                spline.zeros2()
            assert str(info.value) == r["error"]
            continue
        found = spline.zeros2(_path="host")
        assert isinstance(found, list)
        assert [[float(v) for v in x] for x in found] == r["result"], r["name"]


def test_scope_and_arguments():
    surface = make_spline(load_case("rand_22"))
    with pytest.raises(NotImplementedError, match="curves only"):          # Spline.zeros stays with curves
        surface.zeros()
    with pytest.raises(ValueError, match="nInd == 1"):
        roots.zeros_batch(surface)
    with pytest.raises(ValueError, match="_path"):
        surface.zeros2(_path="gpu")
    curve = bspy_amd.Spline(1, 1, [2], [2], [[0, 0, 1, 1.0]], [[1.0, -1.0]])
    with pytest.raises(NotImplementedError, match="two independent variables"):
        curve.zeros2()
    volume = bspy_amd.Spline(3, 3, [2, 2, 2], [2, 2, 2], [[0, 0, 1, 1.0]] * 3, np.ones((3, 2, 2, 2)))
    with pytest.raises(NotImplementedError, match="two independent variables"):
        volume.zeros2()
    k = 7
    high = bspy_amd.Spline(2, 2, [k, 2], [k, 2], [[0.0] * k + [1.0] * k, [0, 0, 1, 1.0]], np.ones((2, k, 2)))
    with pytest.raises(NotImplementedError, match="orders from 2 to 6"):
        high.zeros2()
    with pytest.raises(ValueError, match="device path covers orders"):
        make_spline(load_case("rand_55")).zeros2(_path="device")
    with pytest.raises(ValueError, match=r"shape \(B, 2, 5, 5\)"):
        roots2.zeros2_batch(surface, coefs=np.zeros((2, 5, 5)))


# ------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("name", ["rand_22", "rand_42", "rand_34", "sep_knots_22", "zero_one_cell", "tangent", "empty"])
def test_statement_is_the_host_driver(name):
    """flag_cell, isolate_cell and merge_keep in plain Python floats give the bits of the bsk_roots2_*_host drivers: flags,
    candidates, zeros, near bytes, counts, status, visited nodes and keep bytes."""
    c = load_case(name)
    plan, rows, mask, scale = roots2.tables(make_spline(c))
    said = roots2.statement(rows, plan, mask, scale)
    ran = roots2._run_host(rows, plan, mask, scale)
    assert set(said) == set(ran)
    for key in said:
        assert said[key].dtype == ran[key].dtype and said[key].tobytes() == ran[key].tobytes(), key
    if name == "sep_knots_22":
        assert said["near"].any() and not said["keep"][said["near"] == 1].all(), "the merge drops a zero found twice"
    if name == "tangent":
        assert said["status"].tolist() == [roots2.STATUS_TANGENT]


def test_node_bound():
    """ROOTS2_WALK is 4 x the largest number of nodes a walk visits on the recorded cases, rounded up to a power of two.  The
    tangent case is the one whose status may say that the bound was reached: it is not counted.  The recorded cases are
    those of roots2.npz and of the order sweep, orders_zeros2.npz: system k43.1 of the sweep, certified as well conditioned
    as every coupled golden, holds two zeros in one cell whose walk visits 5052 nodes, more than the bound of 4096 that
    roots2.npz alone gave."""
    largest = 0
    sweep = np.load(os.path.join(GOLDEN, "orders_zeros2.npz"))
    for name, golden in [(n, None) for n in NAMES] + [(f"{n}.{b}", sweep) for n in sweep["names"] for b in range(2)]:
        c = load_case(name, golden)
        plan, rows, mask, scale = roots2.tables(make_spline(c))
        ran = roots2._run_host(rows, plan, mask, scale)
        if c["kind"] != "tangent":
            assert not ran["status"].any()
            largest = max([largest] + ran["nodes"].tolist())
    print(f"largest node count of a walk on the recorded cases: {largest}; ROOTS2_WALK = {roots2.WALK}")
    assert 0 < largest <= roots2.WALK // 4
    assert roots2.WALK == 1 << (4 * largest - 1).bit_length()


def test_walk_bound_sets_status_bit_1():
    c = load_case("rand_22")
    plan, rows, mask, scale = roots2.tables(make_spline(c))
    said = roots2.statement(rows, plan, mask, scale, walk=16)
    assert (said["status"] & roots2.STATUS_WALK).any() and said["nodes"].max() == 16


def test_the_halving_never_flips_a_hull():
    rng = np.random.default_rng(5)
    for K0, K1 in ((2, 2), (3, 4), (4, 4), (6, 5)):
        for _ in range(100):
            cell = (K0, K1), [[abs(float(x)) + 1e-300 for x in (rng.standard_normal((K0, K1)) * 10.0 ** rng.integers(-8, 8)).reshape(-1)]
                              for _ in range(2)]
            for axis in (0, 1):
                for part in roots2.halve(cell, axis):
                    assert roots2.excluded(part)
            assert roots2.restrict_box(cell, [0.0, 0.0], [1.0, 1.0]) == cell       # exact on the whole cell


# ------------------------------------------------------------------------------------------ the library's own uses
def test_zero_cells_is_the_window_check():
    """``zero_cells`` (windowed sums, one axis at a time, for any number of variables) against the statement read cell by
    cell: a cell is zero when all K0 x ... x K(n-1) coefficients of its window are small, for any component.  Mixed orders
    and an interior knot of multiplicity 2 on every axis, so that the knot cells of consecutive spans are not consecutive."""
    import itertools
    axis = {2: [0.0, 0, 1, 1, 2, 3, 3], 3: [0.0, 0, 0, 1, 1, 2, 3, 3, 3], 4: [0.0, 0, 0, 0, 1, 2, 2, 3, 4, 4, 4, 4]}
    rng = np.random.default_rng(20)
    for order in ((2, 4), (3, 2, 4)):
        plan = roots2.Plan2(order, [np.array(axis[k]) for k in order])
        cells = [p.cell for p in plan.axes]
        assert all((np.diff(c) > 1).any() for c in cells)
        ncoef = tuple(len(axis[k]) - k for k in order)
        for B in (1, 3):
            small = rng.random((B, len(order)) + ncoef) < 0.5
            forced = tuple(nc - 1 for nc in plan.ncells)
            window = tuple(slice(c[i] - k + 1, c[i] + 1) for c, i, k in zip(cells, forced, order))
            small[(B - 1, 1) + window] = True
            got = roots2.zero_cells(small, plan)
            assert got.dtype == bool and got.shape == (B,) + tuple(plan.ncells) and got[(B - 1,) + forced]
            for b in range(B):
                for at in itertools.product(*(range(nc) for nc in plan.ncells)):
                    window = tuple(slice(c[i] - k + 1, c[i] + 1) for c, i, k in zip(cells, at, order))
                    assert small[(b, 0) + window].shape == tuple(order)
                    want = any(small[(b, d) + window].all() for d in range(len(order)))
                    assert got[(b,) + at] == want, (order, b, at)
            assert not got.all()


def test_layout_of_the_coefficients_does_not_matter():
    """Knots in Bezier form already: no extraction step copies the coefficients, so the drivers see the caller's array.
    Fortran-ordered and strided coefficients give the bytes of the C-ordered ones, through the spline and through coefs=."""
    knots = [np.array([0.0] * 4 + [1.0] * 4)] * 2
    rng = np.random.default_rng(2)
    coefs = rng.standard_normal((2,) + (4,) * 2)
    c = dict(order=[4] * 2, knots=knots)
    assert not roots2.Plan2(c["order"], knots).steps
    want = roots2.zeros2_batch(make_spline(c, coefs), _path="host")
    assert len(want[0]) >= 1 and not want[3].any()
    wide = rng.standard_normal((2,) + (4,) * 1 + (8,))
    wide[..., ::2] = coefs
    for other in (np.asfortranarray(coefs), wide[..., ::2]):
        assert not other.flags.c_contiguous and np.array_equal(other, coefs)
        for got in (roots2.zeros2_batch(make_spline(c, other), _path="host"),
                    roots2.zeros2_batch(make_spline(c, coefs), coefs=other[None], _path="host")):
            assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist()
            assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()


def test_batch_equals_single_calls():
    c = load_case("rand_44")
    rng = np.random.default_rng(11)
    batch = np.stack([c["coefs"], 3.0 * rng.standard_normal(c["coefs"].shape), np.abs(c["coefs"]) + 0.1, 1e-3 * c["coefs"][::-1]])
    batch[1, 0, :4, :4] = 0.0                                       # a zero cell in one system only
    spline = make_spline(c)
    values, offsets, cells, status = roots2.zeros2_batch(spline, coefs=batch, _path="host")
    assert offsets.dtype == np.int64 and offsets[0] == 0 and offsets[-1] == len(values) and not status.any()
    assert offsets[3] == offsets[2], "the positive system has no zeros"
    for b in range(len(batch)):
        single = make_spline(c, batch[b]).zeros2(_path="host")
        points, tuples = split_result(single)
        assert np.array(points, np.float64).reshape(-1, 2).tobytes() == values[offsets[b]:offsets[b + 1]].tobytes()
        assert [[float(b), float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1])] for lo, hi in tuples] == cells[cells[:, 0] == b].tolist()
    assert len(cells) == 1 and cells[0, 0] == 1.0
    assert np.array(make_spline(c).zeros2(_path="host")).tobytes() == values[:offsets[1]].tobytes()


def test_critical_points_of_a_known_surface():
    """Where the gradient of s = (u - 0.3)^2 - (v - 0.6)^2 + u v / 4 vanishes: 2 (u - 0.3) + v / 4 = 0 and
    -2 (v - 0.6) + u / 4 = 0, from differentiate and elevate alone."""
    grid = np.array([[(u - 0.3) ** 2 - (v - 0.6) ** 2 + u * v / 4 for v in (0.0, 0.5, 1.0)] for u in (0.0, 0.5, 1.0)])

    def bezier(a):                                                  # the Bezier points of quadratics from their values, along axis 0
        return np.array([a[0], 2.0 * a[1] - 0.5 * (a[0] + a[2]), a[2]])

    s = bspy_amd.Spline(2, 1, [3, 3], [3, 3], [[0, 0, 0, 1, 1, 1.0]] * 2, bezier(bezier(grid).T).T[None])
    gu = s.differentiate(0, _path="host").elevate([1, 0], _path="host")
    gv = s.differentiate(1, _path="host").elevate([0, 1], _path="host")
    assert gu.order == gv.order == (3, 3)
    found = bspy_amd.Spline(2, 2, [3, 3], [3, 3], s.knots, np.stack([gu.coefs[0], gv.coefs[0]])).zeros2(_path="host")
    u, v = np.linalg.solve([[2.0, 0.25], [0.25, -2.0]], [0.6, -1.2])
    assert len(found) == 1
    # the bar of the coupled goldens with K0 + K1 = 6, |J^-1| <= 1 (rows sum to 0.56) and S <= 2, doubled for the few eps of S
    # that differencing and elevation leave in the gradient's coefficients, plus 4 eps for u and v themselves
    assert np.abs(found[0] - [u, v]).max() <= 2 * 8 * 6 * EPS * 2.0 + 4 * EPS


# ------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_the_declared_family():
    import re
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bspy_amd.h")).read()
    declared = set(re.findall(r"\b(bsk_roots2_[a-z_]+)\s*\(void|\b(bsk_roots2_[a-z_]+)\s*\(int ", header))
    declared = {a or b for a, b in declared}
    assert declared == set(nv.ROOTS2_SYMBOLS) and not set(nv.ROOTS2_SYMBOLS) & set(nv.SYMBOLS)
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_abi_argument_checks():
    L = nv.lib()
    rows = np.array([[[1.0, -2.0], [0.5, 1.0]], [[-0.25, -0.25], [0.75, 0.75]]])          # (1, 2, 2, 2)
    first = np.array([0], np.int32)
    mask, flags = np.zeros((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint8)
    breaks, scale = np.array([0.0, 1.0]), np.array([[2.0, 0.75]])
    cand = np.array([0], np.int64)
    R = roots2.slots(2, 2)
    out, near = np.zeros((1, R, 2)), np.zeros((1, R), np.uint8)
    count, status, nodes = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(1, np.int32)
    keep, table, which = np.ones((1, R), np.uint8), np.zeros(1, np.int64), np.array([0], np.int64)
    p = lambda a: a.ctypes.data

    def flag(K0=2, K1=2, r=p(rows), nsys=1, R0=2, R1=2, nc0=1, nc1=1, f0=p(first), f1=p(first), m=p(mask), o=p(flags)):
        return L.bsk_roots2_flag_host(K0, K1, r, nsys, R0, R1, nc0, nc1, f0, f1, m, o)

    def isolate(cd=p(cand), ncand=1, o=p(out), nr=p(near), st=p(status), b0=p(breaks)):
        return L.bsk_roots2_isolate_host(2, 2, p(rows), 1, 2, 2, 1, 1, p(first), p(first), b0, p(breaks), p(scale), cd, ncand, o, nr,
                                         p(count), st, p(nodes))

    def merge(R_=R, w=p(which), nnear=1, k=p(keep), ncand=1):
        return L.bsk_roots2_merge_host(R_, p(out), 1, 1, 1, p(breaks), p(breaks), p(cand), ncand, p(flags), p(table), w, nnear, k)

    assert flag() == nv.BSK_OK and flags[0, 0, 0] == 1
    assert isolate() == nv.BSK_OK and count[0] == 1 and L.bsk_roots2_last_kernel() == b"host roots2_isolate"
    assert merge() == nv.BSK_OK and keep[0, 0] == 1 and L.bsk_roots2_last_kernel() == b"host roots2_merge"
    for st in (flag(r=None), flag(f0=None), flag(f1=None), flag(m=None), flag(o=None), flag(K0=1), flag(K1=1), flag(nsys=0), flag(nc0=0),
               flag(nc1=0), flag(R0=1), flag(R1=1), isolate(cd=None), isolate(o=None), isolate(nr=None), isolate(st=None),
               isolate(b0=None), isolate(ncand=0), isolate(ncand=2), merge(R_=1), merge(w=None), merge(k=None), merge(nnear=0),
               merge(nnear=R + 1), merge(ncand=0)):
        assert st == nv.BSK_ERR_INVALID
    assert flag(K0=7) == nv.BSK_ERR_UNSUPPORTED and flag(K1=7) == nv.BSK_ERR_UNSUPPORTED
    # the device entry points refuse an order without a kernel before they touch the device
    assert L.bsk_roots2_flag(5, 2, p(rows), 1, 5, 2, 1, 1, p(first), p(first), p(mask), p(flags), None) == nv.BSK_ERR_UNSUPPORTED
    assert L.bsk_roots2_isolate(2, 5, p(rows), 1, 2, 5, 1, 1, p(first), p(first), p(breaks), p(breaks), p(scale), p(cand), 1, p(out), p(near),
                                p(count), p(status), p(nodes), None) == nv.BSK_ERR_UNSUPPORTED
    # a window outside the rows and a candidate outside the table give no zero instead of a read out of bounds
    bad_first = np.array([1], np.int32)
    assert flag(f0=p(bad_first)) == nv.BSK_OK and flags[0, 0, 0] == 0
    assert flag(f1=p(bad_first)) == nv.BSK_OK and flags[0, 0, 0] == 0
    assert flag() == nv.BSK_OK
    for bad in (5, -1):
        bad_cand = np.array([bad], np.int64)
        assert isolate(cd=p(bad_cand)) == nv.BSK_OK and count[0] == 0 and np.isnan(out).all()
    keep[:] = 7
    assert merge(w=p(np.array([99], np.int64))) == nv.BSK_OK and (keep == 7).all()              # no lane, no byte
