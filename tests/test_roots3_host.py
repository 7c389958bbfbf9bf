"""
Spline.zeros3 and roots3.zeros3_batch on the host path (no GPU): every golden of tests/golden/roots3.npz against what is
exactly true (the certified oracle tests/zeros3_ref.py for coupled systems, the exact 1-D roots of tests/zeros_ref.py for
the separable system and the surface minus line); the oracle's own cross-checks; the semantics file; the pure-Python
statement of the arithmetic in bspy_amd/roots3.py against the host drivers, bit for bit; the node bound; the batched call;
argument checks of the bsk_roots3_* entry points.  The reference's zeros are recorded in the goldens and compared where it
was complete; it is not the yardstick for counts.

The bars (derived, not tuned): those of tests/test_roots2_host.py carried to three variables.  Trivariate de Casteljau of
K0 + K1 + K2 - 3 levels in fp64 is within (K0 + K1 + K2) eps S_d of f_d, S_d = max |coefficient|; Newton therefore stops
where |F_d| <= (K0 + K1 + K2) eps S_d or so, and with the certified preconditioner Y the zero r* is within 2 |Y F(r)| of r
(zeros3_ref.certify).  With a factor 4 for second-order terms and the cell mapping a reported zero r of a coupled case must
have, in cell-local units,
    2 |Y F(r)| <= 8 (K0 + K1 + K2) eps max_i sum_d |Y_id| S_d + 4 eps max_i max(|a_i|, |b_i|) / h_i,
F evaluated exactly at the reported doubles, [a_i, b_i] the domain and h_i the cell's width along axis i; float32 knots add
one float32 spacing of max(|a_i|, |b_i|) over h_i for the final rounding.  The separable system: the 1-D bar ``delta`` of
test_roots_host.py per axis against the exact brackets.  Surface minus line: u against its 1-D bracket, and
|s(u, v) - c(t)| <= 8 (K0 + K1 + K2) eps S (max-norm), evaluated exactly.
"""
import ctypes
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bspy_amd
import zeros3_ref
import zeros_ref
from bspy_amd import _native as nv
from bspy_amd import roots3
from conftest import GOLDEN, observe

EPS = float(np.finfo(np.float64).eps)
_GOLDEN = np.load(os.path.join(GOLDEN, "roots3.npz"))
NAMES = sorted({key.split("/")[0] for key in _GOLDEN.files})
SMALL = ["rand_222", "rand_442"]                                # the goldens regenerated from the oracle here


def load_case(name):
    c = {key.split("/", 1)[1]: _GOLDEN[key] for key in _GOLDEN.files if key.startswith(name + "/")}
    c["name"], c["kind"], c["order"] = name, str(c["kind"]), [int(k) for k in c["order"]]
    c["knots"] = [c["knots0"], c["knots1"], c["knots2"]]
    return c


def make_spline(c, coefs=None):
    coefs = c["coefs"] if coefs is None else coefs
    return bspy_amd.Spline(3, 3, c["order"], list(coefs.shape[1:]), c["knots"], coefs)


def split_result(found):
    return [r for r in found if not isinstance(r, tuple)], [r for r in found if isinstance(r, tuple)]


def bits(found):
    return [np.asarray(r).tobytes() for r in found]


def pair(points, exact):
    """The reported zero nearest to every exact one (max-norm): one to one, since the cases keep their zeros apart."""
    points = np.array(points, np.float64).reshape(-1, 3)
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


_CELLS = {}


def exact_cells(c):
    """The exact Bezier cells of a case, computed once and left unchanged."""
    if c["name"] not in _CELLS:
        _CELLS[c["name"]] = zeros3_ref.bezier_cells(c["order"], c["knots"], c["coefs"])
    return _CELLS[c["name"]]


def check_golden(c, found, label):
    """Counts equal the exact counts; every zero within its bar of what is exactly true; where the reference was complete,
    within bar + ref_dev of the reference's zero.  Returns the worst error / bar."""
    points, tuples = split_result(found)
    kdtype = np.result_type(*(t.dtype for t in c["knots"]))
    assert all(isinstance(r, np.ndarray) and r.shape == (3,) and r.dtype == kdtype for r in points), "zeros come in the knots' dtype"
    assert len(points) == len(c["exact_uvw"]), f"{c['name']}: {len(points)} zeros, exactly {len(c['exact_uvw'])}"
    assert [[float(a[0]), float(b[0]), float(a[1]), float(b[1]), float(a[2]), float(b[2])] for a, b in tuples] == c["exact_cells"].tolist()
    keys = [tuple(float(v) for v in (r[0] if isinstance(r, tuple) else r)) for r in found]
    assert keys == sorted(keys), "sorted by (u, v, w)"
    if not len(points):
        return 0.0
    got = pair(points, c["exact_uvw"])
    K = c["order"]
    S = [float(np.abs(comp.astype(np.float64)).max()) for comp in c["coefs"]]
    ends = [max(abs(float(t[k - 1])), abs(float(t[len(t) - k]))) for k, t in zip(K, c["knots"])]
    bars = np.zeros((len(got), 3))                              # per zero and axis, in the parameters
    worst = 0.0
    if c["kind"] in ("coupled", "zero"):
        breaks, cells = exact_cells(c)
        for n, r in enumerate(got):
            at = [int(v) for v in c["cert_cell"][n]]
            t0 = [breaks[a][at[a]] for a in range(3)]
            h = [breaks[a][at[a] + 1] - breaks[a][at[a]] for a in range(3)]
            x, radius = [Fraction(float(v)) for v in c["cert_x"][n]], Fraction(float(c["cert_radius"][n]))
            Y = [[Fraction(float(v)) for v in row] for row in c["cert_Y"][n]]
            cert = dict(lo=[max(0, v - radius) for v in x], hi=[min(1, v + radius) for v in x], Y=Y)
            local = [(Fraction(float(r[a])) - t0[a]) / h[a] for a in range(3)]
            err = float(zeros3_ref.error_bound(cells[at[0]][at[1]][at[2]], cert, local))
            bar = 8.0 * sum(K) * EPS * max(sum(abs(float(Y[k][d])) * S[d] for d in range(3)) for k in range(3)) \
                + 4.0 * EPS * max(ends[a] / float(h[a]) for a in range(3))
            if kdtype == np.float32:
                bar += max(float(np.spacing(np.float32(ends[a]))) / float(h[a]) for a in range(3))
            worst = max(worst, err / bar)
            bars[n] = [bar * float(h[a]) for a in range(3)]
    elif c["kind"] in ("separable", "line"):
        axes = (("u", 0), ("v", 1), ("w", 2)) if c["kind"] == "separable" else (("u", 0),)
        for n, (r, e) in enumerate(zip(got, c["exact_uvw"])):
            for prefix, d in axes:
                lo, hi = c[prefix + "_lo"], c[prefix + "_hi"]
                m = int(np.abs(0.5 * (lo + hi) - e[d]).argmin())
                bar = delta_1d(c[prefix + "_order"], c[prefix + "_knots"], c[prefix + "_coefs"], c[prefix + "_fprime"][m], kdtype)
                err = max(0.0, float(lo[m]) - float(r[d]), float(r[d]) - float(hi[m]))
                worst = max(worst, err / bar)
                bars[n, d] = bar
        if c["kind"] == "line":
            breaks, cells = exact_cells(c)
            residual_bar = 8.0 * sum(K) * EPS * max(S)
            for n, r in enumerate(got):
                i = min(max(i for i in range(len(breaks[0]) - 1) if breaks[0][i] <= Fraction(float(r[0]))), len(breaks[0]) - 2)
                local = [(Fraction(float(r[0])) - breaks[0][i]) / (breaks[0][i + 1] - breaks[0][i])] + \
                        [(Fraction(float(r[a])) - breaks[a][0]) / (breaks[a][1] - breaks[a][0]) for a in (1, 2)]
                residual = max(abs(float(zeros3_ref.value(comp, local))) for comp in cells[i][0][0])
                worst = max(worst, residual / residual_bar)
                bars[n, 1:] = np.inf                            # v and t are pinned by the residual, not by a bracket
    if c["ref_complete"]:
        ref = pair(c["ref_roots"], c["exact_uvw"])
        assert (np.abs(got - ref) <= bars + float(c["ref_dev"])).all(), f"{c['name']}: against the reference"
    print(f"{label} {c['name']}: {len(points)} zeros, {len(tuples)} zero cells, worst error / bar {worst:.3e}")
    observe(f"{label} error / bar ({c['kind']}, {'float32' if kdtype == np.float32 else 'float64'} knots)", worst, 1.0)
    return worst


TANGENT = r"zeros3: (tangential or singular zero|zeros not isolated)"


# ------------------------------------------------------------------------------------------ goldens
def test_goldens_cover_the_issue():
    cases = [load_case(n) for n in NAMES]
    assert {c["kind"] for c in cases} == {"coupled", "separable", "line", "zero", "tangent", "empty"}
    coupled = [c for c in cases if c["kind"] == "coupled"]
    assert {tuple(c["order"]) for c in coupled} >= {(2, 2, 2), (3, 3, 3), (4, 4, 4), (4, 4, 2), (2, 3, 4)}
    assert any(c["coefs"].dtype == np.float32 for c in coupled) and any(c["knots0"].dtype == np.float32 for c in coupled)
    assert any(len(np.unique(c["knots0"])) + 2 * (c["order"][0] - 1) < len(c["knots0"]) for c in coupled), "a repeated interior knot"
    assert all(max(c["coefs"].shape[1:]) <= 6 for c in cases)
    ncells = {tuple(len(np.unique(t)) - 1 for t in c["knots"]) for c in coupled}
    assert (2, 2, 2) in ncells and (3, 2, 1) in ncells
    uvw = load_case("sep_knots_222")["exact_uvw"].tolist()
    assert [0.5, 0.5, 0.75] in uvw and [0.125, 0.5, 0.375] in uvw and [0.5, 0.5, 0.375] in uvw and [0.125, 0.5, 0.0] in uvw
    assert os.path.getsize(os.path.join(GOLDEN, "roots3.npz")) < 3 * os.path.getsize(os.path.join(GOLDEN, "roots2.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_golden_host(name):
    c = load_case(name)
    if c["kind"] == "tangent":
        with pytest.raises(ValueError, match=TANGENT):
            make_spline(c).zeros3(_path="host")
        *_, status = roots3.zeros3_batch(make_spline(c), _path="host")
        assert status.max() & roots3.STATUS_TANGENT and (status != 0).sum() == 1
        return
    found = make_spline(c).zeros3(_path="host")
    assert all(p.startswith("host ") for p in roots3.LAST_PATHS) and "host roots3_flag" in roots3.LAST_PATHS
    assert nv.lib().bsk_roots3_last_kernel().decode() == roots3.LAST_PATHS[-1]
    check_golden(c, found, "zeros3 host")
    assert bits(make_spline(c).zeros3(_path="host")) == bits(found), "two runs differ"
    assert bits(make_spline(c).zeros3()) == bits(found)                    # few cells: the host


@pytest.mark.parametrize("name", SMALL)
def test_golden_is_the_yardstick(name):
    c = load_case(name)
    exact = zeros3_ref.zeros(c["order"], c["knots"], c["coefs"])
    assert [list(z["cell"]) for z in exact] == c["cert_cell"].tolist()
    assert [[float(v) for v in z["x"]] for z in exact] == c["cert_x"].tolist()
    assert [float(z["radius"]) for z in exact] == c["cert_radius"].tolist()
    assert [[[float(v) for v in row] for row in z["Y"]] for z in exact] == c["cert_Y"].tolist()
    assert [[float(z["t0"][a] + z["x"][a] * z["h"][a]) for a in range(3)] for z in exact] == c["exact_uvw"].tolist()


def test_oracle_on_a_separable_system():
    """(p(u), q(v), r(w)): the certified zeros are the product of the exact roots of p, q and r."""
    lines = [(3, np.array([0, 0, 0, 0.4, 1, 1, 1.0]), np.array([1.0, -0.75, 0.5, -1.25])),
             (2, np.array([0, 0, 0.3, 1, 1.0]), np.array([-1.0, 0.5, -0.75])),
             (3, np.array([0, 0, 0, 1, 1, 1.0]), np.array([-0.5, 1.25, -1.0]))]
    shape = tuple(len(line[2]) for line in lines)
    coefs = np.stack([np.broadcast_to(lines[a][2].reshape([-1 if b == a else 1 for b in range(3)]), shape) for a in range(3)])
    exact = zeros3_ref.zeros([line[0] for line in lines], [line[1] for line in lines], coefs)
    brackets = [zeros_ref.roots(*line)["brackets"] for line in lines]
    assert len(exact) == len(brackets[0]) * len(brackets[1]) * len(brackets[2]) > 1
    product = sorted((a, b, c) for a in brackets[0] for b in brackets[1] for c in brackets[2])
    for z, bracket in zip(exact, product):
        for a in range(3):
            lo, hi = z["t0"][a] + z["lo"][a] * z["h"][a], z["t0"][a] + z["hi"][a] * z["h"][a]
            assert lo <= bracket[a][0] <= bracket[a][1] <= hi                 # the one zero of the box


def test_oracle_on_surface_minus_line():
    """(u, v, g(u, v)) - (3 t, 3/2, z0 + 3 m t): the certified zeros have the exact roots of g(u, 3/2) - z0 - m u as their
    u, v = 3/2 and t = u / 3."""
    c = load_case("bicubic_minus_line")
    exact = zeros3_ref.zeros(c["order"], c["knots"], c["coefs"])
    assert len(exact) == len(c["u_lo"]) > 1
    one = zeros_ref.roots(int(c["u_order"]), c["u_knots"], c["u_coefs"])
    assert len(one["brackets"]) == len(exact)
    for z, (lo, hi) in zip(exact, one["brackets"]):
        box = [(z["t0"][a] + z["lo"][a] * z["h"][a], z["t0"][a] + z["hi"][a] * z["h"][a]) for a in range(3)]
        assert box[0][0] <= lo <= hi <= box[0][1]
        assert box[1][0] <= Fraction(3, 2) <= box[1][1]
        assert box[2][0] <= lo / 3 and hi / 3 <= box[2][1]


def test_semantics():
    with open(os.path.join(GOLDEN, "roots3_semantics.json")) as f:
        records = json.load(f)
    assert {r["name"] for r in records} >= {"nind_ne_ndep", "no_zeros", "one_zero"}
    for r in records:
        s = r["spline"]
        coefs = np.array(s["coefs"])
        spline = bspy_amd.Spline(3, len(coefs), s["order"], list(coefs.shape[1:]), [np.array(k) for k in s["knots"]], coefs)
        if r["error"] is not None:
            with pytest.raises(ValueError) as info:
                spline.zeros3()
            assert str(info.value) == r["error"]
            continue
        found = spline.zeros3(_path="host")
        assert isinstance(found, list)
        if r["name"] == "no_zeros":
            assert found == []
        if r["name"] == "one_zero":
            assert [[float(v) for v in x] for x in found] == [[0.25, 0.5, 0.75]]
        if r["result"] is not None and len(r["result"]) == len(found):
            assert np.abs(np.array([[float(v) for v in x] for x in found]).reshape(-1, 3) - np.array(r["result"]).reshape(-1, 3)).max(initial=0.0) <= 1e-6


def test_scope_and_arguments():
    volume = make_spline(load_case("rand_222"))
    with pytest.raises(NotImplementedError, match="curves only"):          # Spline.zeros stays with curves
        volume.zeros()
    with pytest.raises(NotImplementedError, match="two independent variables"):
        volume.zeros2()
    with pytest.raises(ValueError, match="_path"):
        volume.zeros3(_path="gpu")
    curve = bspy_amd.Spline(1, 1, [2], [2], [[0, 0, 1, 1.0]], [[1.0, -1.0]])
    with pytest.raises(NotImplementedError, match="three independent variables"):
        curve.zeros3()
    surface = bspy_amd.Spline(2, 2, [2, 2], [2, 2], [[0, 0, 1, 1.0]] * 2, np.ones((2, 2, 2)))
    with pytest.raises(NotImplementedError, match="three independent variables"):
        surface.zeros3()
    k = 5
    high = bspy_amd.Spline(3, 3, [k, 2, 2], [k, 2, 2], [[0.0] * k + [1.0] * k, [0, 0, 1, 1.0], [0, 0, 1, 1.0]], np.ones((3, k, 2, 2)))
    with pytest.raises(NotImplementedError, match="orders from 2 to 4"):
        high.zeros3()
    with pytest.raises(ValueError, match=r"shape \(B, 3, 3, 3, 3\)"):
        roots3.zeros3_batch(volume, coefs=np.zeros((3, 3, 3, 3)))
    with pytest.raises(ValueError, match=r"shape \(B, 3, 3, 3, 3\)"):
        roots3.zeros3_batch(volume, coefs=np.zeros((1, 3, 3, 3, 4)))


# ------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("name", ["rand_222", "rand_234", "f32_coefs_332", "sep_knots_222", "zero_one_cell", "tangent", "empty"])
def test_statement_is_the_host_driver(name):
    """flag_cell, isolate_cell and merge_keep in plain Python floats give the bits of the bsk_roots3_*_host drivers: flags,
    candidates, zeros, near bytes, counts, status, visited nodes and keep bytes."""
    c = load_case(name)
    plan, rows, mask, scale = roots3.tables(make_spline(c))
    said = roots3.statement(rows, plan, mask, scale)
    ran = roots3._run_host(rows, plan, mask, scale)
    assert set(said) == set(ran)
    for key in said:
        assert said[key].dtype == ran[key].dtype and said[key].tobytes() == ran[key].tobytes(), key
    if name == "sep_knots_222":
        assert said["near"].any() and not said["keep"][said["near"] == 1].all(), "the merge drops a zero found twice"
        assert int(said["keep"].sum()) == 6 and int(said["count"].sum()) == 2 + 2 + 4 + 4 + 4 + 8      # plane, plane, edges, corner
    if name == "tangent":
        assert said["status"].tolist() == [roots3.STATUS_TANGENT]
    if name == "empty":
        assert len(said["cand"]) > 0 and not said["count"].any()


def test_node_bound():
    """ROOTS3_WALK is 4 x the largest number of nodes a walk visits on the recorded cases, rounded up to a power of two.  The
    tangent case is the one whose status may say that the bound was reached: it is not counted."""
    largest = 0
    for name in NAMES:
        c = load_case(name)
        plan, rows, mask, scale = roots3.tables(make_spline(c))
        ran = roots3._run_host(rows, plan, mask, scale)
        if c["kind"] != "tangent":
            assert not ran["status"].any()
            largest = max([largest] + ran["nodes"].tolist())
    print(f"largest node count of a walk on the recorded cases: {largest}; ROOTS3_WALK = {roots3.WALK}")
    assert 0 < largest <= roots3.WALK // 4
    assert roots3.WALK == 1 << (4 * largest - 1).bit_length()
    assert nv.lib().bsk_roots3_walk_bound() == roots3.WALK, "the compiled bound and the statement's differ"


def test_walk_bound_sets_status_bit_1():
    c = load_case("rand_222")
    plan, rows, mask, scale = roots3.tables(make_spline(c))
    said = roots3.statement(rows, plan, mask, scale, walk=16)
    assert (said["status"] & roots3.STATUS_WALK).any() and said["nodes"].max() == 16


def test_the_halving_never_flips_a_hull():
    rng = np.random.default_rng(5)
    for dims in ((2, 2, 2), (2, 3, 4), (4, 4, 4)):
        for _ in range(30):
            cell = (dims, [[abs(float(x)) + 1e-300 for x in rng.standard_normal(dims[0] * dims[1] * dims[2]) * 10.0 ** rng.integers(-8, 8)]
                           for _ in range(3)])
            for axis in range(3):
                for part in roots3.halve(cell, axis):
                    assert roots3.excluded(part)
            assert roots3.restrict_box(cell, [0.0] * 3, [1.0] * 3) == cell         # exact on the whole cell


# ------------------------------------------------------------------------------------------ the library's own uses
def test_layout_of_the_coefficients_does_not_matter():
    """Knots in Bezier form already: no extraction step copies the coefficients, so the drivers see the caller's array.
    Fortran-ordered and strided coefficients give the bytes of the C-ordered ones, through the spline and through coefs=."""
    knots = [np.array([0.0] * 4 + [1.0] * 4)] * 3
    rng = np.random.default_rng(5)
    coefs = rng.standard_normal((3,) + (4,) * 3)
    c = dict(order=[4] * 3, knots=knots)
    assert not roots3.Plan3(c["order"], knots).steps
    want = roots3.zeros3_batch(make_spline(c, coefs), _path="host")
    assert len(want[0]) >= 1 and not want[3].any()
    wide = rng.standard_normal((3,) + (4,) * 2 + (8,))
    wide[..., ::2] = coefs
    for other in (np.asfortranarray(coefs), wide[..., ::2]):
        assert not other.flags.c_contiguous and np.array_equal(other, coefs)
        for got in (roots3.zeros3_batch(make_spline(c, other), _path="host"),
                    roots3.zeros3_batch(make_spline(c, coefs), coefs=other[None], _path="host")):
            assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist()
            assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()


def test_batch_equals_single_calls():
    c = load_case("rand_333")
    rng = np.random.default_rng(11)
    batch = np.stack([c["coefs"], 3.0 * rng.standard_normal(c["coefs"].shape), np.abs(c["coefs"]) + 0.1, 1e-3 * c["coefs"][::-1]])
    batch[1, 0, :3, :3, :3] = 0.0                                   # a zero cell in one system only
    spline = make_spline(c)
    values, offsets, cells, status = roots3.zeros3_batch(spline, coefs=batch, _path="host")
    assert offsets.dtype == np.int64 and offsets[0] == 0 and offsets[-1] == len(values)
    assert status.shape == (4, 3, 2, 1) and cells.shape == (1, 7) and cells[0, 0] == 1.0
    assert offsets[3] == offsets[2], "the positive system has no zeros"
    for b in range(len(batch)):
        if status[b].any():
            continue
        points, tuples = split_result(make_spline(c, batch[b]).zeros3(_path="host"))
        assert np.array(points, np.float64).reshape(-1, 3).tobytes() == values[offsets[b]:offsets[b + 1]].tobytes()
        assert [[float(b)] + [float(v) for pair_ in zip(lo, hi) for v in pair_] for lo, hi in tuples] == cells[cells[:, 0] == b].tolist()
    assert not status[0].any() and offsets[1] == len(c["exact_uvw"])


def test_curve_against_surface_through_subtract():
    """The README's example: ``surface.subtract(curve)`` has nInd == nDep == 3 and its zeros are the crossings.  The golden
    holds d_ijk = s_ij - c_k on a grid, so s' = d_ij0 and c' = d_000 - d_00k are a surface and a curve with s' - c' = d exactly."""
    c = load_case("bicubic_minus_cubic")
    d = c["coefs"]
    surface = bspy_amd.Spline(2, 3, [4, 4], list(d.shape[1:3]), c["knots"][:2], d[:, :, :, 0])
    curve = bspy_amd.Spline(1, 3, [4], [d.shape[3]], c["knots"][2:], d[:, 0, 0, :1] - d[:, 0, 0, :])
    system = surface.subtract(curve, _path="host")
    assert system.nInd == 3 and system.nDep == 3 and tuple(system.order) == (4, 4, 4)
    assert np.asarray(system.coefs).tobytes() == d.tobytes()
    assert bits(system.zeros3(_path="host")) == bits(make_spline(c).zeros3(_path="host")) and len(c["exact_uvw"]) >= 1


# ------------------------------------------------------------------------------------------ one realistic call
def basis(knots, order, x, derivative=False):
    """The B-spline basis functions of ``order`` (or their derivatives) at the points x: (len(x), n), by Cox-de Boor."""
    t = np.asarray(knots, float)
    x = np.asarray(x, float)
    n = len(t) - order
    span = np.clip(np.searchsorted(t, x, "right") - 1, order - 1, n - 1)
    N = np.zeros((len(x), len(t) - 1))
    N[np.arange(len(x)), span] = 1.0
    for k in range(2, order + 1):
        last = derivative and k == order
        new = np.zeros((len(x), len(t) - k))
        for i in range(len(t) - k):
            a, b = t[i + k - 1] - t[i], t[i + k] - t[i + 1]
            if a > 0.0:
                new[:, i] += (k - 1) / a * N[:, i] if last else (x - t[i]) / a * N[:, i]
            if b > 0.0:
                new[:, i] += -(k - 1) / b * N[:, i + 1] if last else (t[i + k] - x) / b * N[:, i + 1]
        N = new
    return N


def curves_and_surface():
    """One bicubic surface on 3 x 3 cells, B = 4 cubic curves of 2 spans that cross it, and the crossings by Newton in NumPy
    from a 5 x 5 x 5 grid of starting points per cell: (knots, surface (3, 6, 6), curves (4, 3, 5), [crossings per curve])."""
    rng = np.random.default_rng(33)
    ku = np.concatenate(([0.0] * 4, [0.3, 0.7], [1.0] * 4))
    kv = np.concatenate(([0.0] * 4, [0.4, 0.6], [1.0] * 4))
    kt = np.concatenate(([0.0] * 4, [0.45], [1.0] * 4))
    gu, gv = np.meshgrid(np.linspace(0, 1, 6), np.linspace(0, 1, 6), indexing="ij")
    surface = np.stack([gu, gv, 0.3 * np.sin(3.0 * gu) * np.cos(2.0 * gv)]) + 0.03 * rng.standard_normal((3, 6, 6))
    curves = np.stack([np.stack([rng.uniform(0.15, 0.85, 5), rng.uniform(0.15, 0.85, 5), np.linspace(-0.8, 0.8, 5) + 0.05 * rng.standard_normal(5)])
                       for _ in range(4)])
    breaks = [np.unique(k) for k in (ku, kv, kt)]
    starts = np.array([[b[i] + f * (b[i + 1] - b[i]) for b, i, f in zip(breaks, cell, frac)]
                       for cell in np.ndindex(3, 3, 2) for frac in np.ndindex(5, 5, 5) for frac in [(np.array(frac) + 0.5) / 5.0]])
    want = []
    for c in curves:
        x = starts.copy()
        with np.errstate(all="ignore"):
            for _ in range(40):
                x = np.clip(np.nan_to_num(x, nan=-1.0), -1.0, 2.0)
                inside = np.clip(x, 0.0, 1.0)
                Bu, Bv, Bt = basis(ku, 4, inside[:, 0]), basis(kv, 4, inside[:, 1]), basis(kt, 4, inside[:, 2])
                Du, Dv, Dt = basis(ku, 4, inside[:, 0], True), basis(kv, 4, inside[:, 1], True), basis(kt, 4, inside[:, 2], True)
                F = np.einsum("pi,pj,dij->pd", Bu, Bv, surface) - Bt @ c.T
                J = np.stack([np.einsum("pi,pj,dij->pd", Du, Bv, surface), np.einsum("pi,pj,dij->pd", Bu, Dv, surface), -(Dt @ c.T)], axis=2)
                ok = np.abs(np.linalg.det(J)) > 1e-12
                step = np.zeros_like(x)
                step[ok] = np.linalg.solve(J[ok], F[ok][:, :, None])[:, :, 0]
                x = np.where(ok[:, None], inside - step, -1.0)
        good = ((x >= 0.0) & (x <= 1.0)).all(axis=1) & (np.abs(F).max(axis=1) <= 1e-13)
        found = []
        for point in x[good][np.lexsort(x[good].T[::-1])]:
            if not any(np.abs(point - f).max() <= 1e-10 for f in found):
                found.append(point)
        want.append(np.array(sorted(map(tuple, found))).reshape(-1, 3))
    return (ku, kv, kt), surface, curves, want


def check_crossings(values, offsets, knots, want):
    breaks = [np.unique(k) for k in knots]
    total = 0
    for q, exact in enumerate(want):
        got = values[offsets[q]:offsets[q + 1]]
        assert len(got) == len(exact), f"curve {q}: {len(got)} crossings, Newton from the grid finds {len(exact)}"
        assert len(exact) == 0 or np.abs(got - exact).max() <= 1e-9
        for a in range(3):                                          # the premise: at least 1e-2 of a cell from every face
            cell = np.clip(np.searchsorted(breaks[a], exact[:, a], "right") - 1, 0, len(breaks[a]) - 2)
            local = (exact[:, a] - breaks[a][cell]) / (breaks[a][cell + 1] - breaks[a][cell])
            assert ((local >= 1e-2) & (local <= 1.0 - 1e-2)).all()
        total += len(got)
    assert total >= 4


def test_curves_against_a_surface_on_the_host():
    """s(u, v) - c_b(t) for B = 4 curves as one zeros3_batch call on the host path, against Newton in NumPy; the GPU test
    makes the same comparison on the device."""
    knots, surface, curves, want = curves_and_surface()
    spline = bspy_amd.Spline(3, 3, [4, 4, 4], [6, 6, 5], list(knots), surface[:, :, :, None] - curves[0][:, None, None, :])
    coefs = surface[None, :, :, :, None] - curves[:, :, None, None, :]
    values, offsets, cells, status = roots3.zeros3_batch(spline, coefs=coefs, _path="host")
    assert len(cells) == 0 and not status.any() and roots3.Plan3(spline.order, spline.knots).ncells == [3, 3, 2]
    check_crossings(values, offsets, knots, want)


# ------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_the_declared_family():
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bspy_amd.h")).read()
    declared = set(re.findall(r"\b(bsk_roots3_[a-z_]+)\s*\(void|\b(bsk_roots3_[a-z_]+)\s*\(int ", header))
    declared = {a or b for a, b in declared}
    assert declared == set(nv.ROOTS3_SYMBOLS) and not set(nv.ROOTS3_SYMBOLS) & set(nv.SYMBOLS + nv.ROOTS2_SYMBOLS)
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_abi_argument_checks():
    L = nv.lib()
    # (u - 1/4, v - 1/2, w - 3/4) on one trilinear cell
    i, j, k = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    rows = np.ascontiguousarray(np.stack([i - 0.25, j - 0.5, k - 0.75])[None].astype(np.float64))
    first = np.array([0], np.int32)
    mask, flags = np.zeros((1, 1, 1, 1), np.uint8), np.zeros((1, 1, 1, 1), np.uint8)
    breaks, scale = np.array([0.0, 1.0]), np.array([[0.75, 0.5, 0.75]])
    cand = np.array([0], np.int64)
    R = roots3.slots(2, 2, 2)
    out, near = np.zeros((1, R, 3)), np.zeros((1, R), np.uint8)
    count, status, nodes = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(1, np.int32)
    keep, table, which = np.ones((1, R), np.uint8), np.zeros(1, np.int64), np.array([0], np.int64)
    p = lambda a: a.ctypes.data

    def grid(K=(2, 2, 2), r=p(rows), nsys=1, Rs=(2, 2, 2), nc=(1, 1, 1), f=(p(first),) * 3):
        return (*K, r, nsys, *Rs, *nc, *f)

    def flag(m=p(mask), o=p(flags), **kw):
        return L.bsk_roots3_flag_host(*grid(**kw), m, o)

    def isolate(cd=p(cand), ncand=1, o=p(out), nr=p(near), st=p(status), b0=p(breaks), **kw):
        return L.bsk_roots3_isolate_host(*grid(**kw), b0, p(breaks), p(breaks), p(scale), cd, ncand, o, nr, p(count), st, p(nodes))

    def merge(R_=R, w=p(which), nnear=1, k_=p(keep), ncand=1):
        return L.bsk_roots3_merge_host(R_, p(out), 1, 1, 1, 1, p(breaks), p(breaks), p(breaks), p(cand), ncand, p(flags), p(table), w, nnear, k_)

    assert flag() == nv.BSK_OK and flags[0, 0, 0, 0] == 1
    assert isolate() == nv.BSK_OK and count[0] == 1 and L.bsk_roots3_last_kernel() == b"host roots3_isolate"
    assert out[0, 0].tolist() == [0.25, 0.5, 0.75] and np.isnan(out[0, 1:]).all() and nodes[0] > 3 * roots3.DEPTH
    assert merge() == nv.BSK_OK and keep[0, 0] == 1 and L.bsk_roots3_last_kernel() == b"host roots3_merge"
    for st in (flag(r=None), flag(f=(None, p(first), p(first))), flag(f=(p(first), p(first), None)), flag(m=None), flag(o=None),
               flag(K=(1, 2, 2)), flag(K=(2, 2, 1)), flag(nsys=0), flag(nc=(0, 1, 1)), flag(nc=(1, 1, 0)), flag(Rs=(1, 2, 2)),
               flag(Rs=(2, 2, 1)), isolate(cd=None), isolate(o=None), isolate(nr=None), isolate(st=None), isolate(b0=None),
               isolate(ncand=0), isolate(ncand=2), merge(R_=5), merge(R_=33), merge(w=None), merge(k_=None), merge(nnear=0),
               merge(nnear=R + 1), merge(ncand=0)):
        assert st == nv.BSK_ERR_INVALID
    assert flag(K=(5, 2, 2), Rs=(5, 2, 2)) == nv.BSK_ERR_UNSUPPORTED and flag(K=(2, 2, 5), Rs=(2, 2, 5)) == nv.BSK_ERR_UNSUPPORTED
    # the device entry points refuse an order without a kernel before they touch the device
    assert L.bsk_roots3_flag(*grid(K=(2, 5, 2), Rs=(2, 5, 2)), p(mask), p(flags), None) == nv.BSK_ERR_UNSUPPORTED
    assert L.bsk_roots3_isolate(*grid(K=(5, 2, 2), Rs=(5, 2, 2)), p(breaks), p(breaks), p(breaks), p(scale), p(cand), 1, p(out), p(near),
                                p(count), p(status), p(nodes), None) == nv.BSK_ERR_UNSUPPORTED
    # a window outside the rows and a candidate outside the table give no zero instead of a read out of bounds
    bad_first = np.array([1], np.int32)
    for axis in range(3):
        f = [p(first)] * 3
        f[axis] = p(bad_first)
        assert flag(f=tuple(f)) == nv.BSK_OK and flags[0, 0, 0, 0] == 0
    assert flag() == nv.BSK_OK
    for bad in (5, -1):
        bad_cand = np.array([bad], np.int64)
        assert isolate(cd=p(bad_cand)) == nv.BSK_OK and count[0] == 0 and np.isnan(out).all()
    keep[:] = 7
    assert merge(w=p(np.array([99], np.int64))) == nv.BSK_OK and (keep == 7).all()              # no lane, no byte
