"""
Spline.zeros2 and roots2.zeros2_batch on the GPU (roots2_flag, roots2_isolate, roots2_merge, the band kernels for the
extraction): every golden of tests/golden/roots2.npz that the kernels cover through ``_path="device"`` (bars of
tests/test_roots2_host.py) with the kernels that ran asserted from ``roots2.LAST_PATHS`` and ``bsk_roots2_last_kernel``,
bit-equal to the host path and on a second run; then the layouts of the three kernels through ``zeros2_batch`` on CUDA
tensors against the host drivers, which run the same functions of bsk_roots2.hpp: bit for bit.  No kernel of the family
uses LDS, so it has no stale-LDS test.
"""
import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import roots2
from test_roots2_host import NAMES, check_golden, load_case, make_spline

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BANDS = {"band_apply", "band_apply_line"}
DEVICE_NAMES = [n for n in NAMES if max(load_case(n)["order"]) <= roots2.DEVICE_MAX_K]       # rand_55 is the host's


def bits(found):
    return [np.asarray(r).tobytes() for r in found]


def launches(ran):
    return [p for p in ran if p not in BANDS]


def expected(host_ran):
    """The launches of the device path from those of the host path on the same numbers."""
    return [p[len("host "):] for p in host_ran if p.startswith("host roots2_")]


def system(rng, order, ncells, B=1, dtype=np.float64, signs=None):
    """B random systems on ncells[0] x ncells[1] cells with simple interior knots."""
    knots, ncoef = [], []
    for k, nc in zip(order, ncells):
        knots.append(np.concatenate((k * [0.0], np.sort(rng.random(nc - 1)), k * [1.0])))
        ncoef.append(len(knots[-1]) - k)
    coefs = rng.standard_normal((B, 2, *ncoef))
    if signs is not None:
        coefs = (np.abs(coefs) + 0.1) * signs
    spline = bspy_amd.Spline(2, 2, list(order), ncoef, knots, coefs[0].astype(dtype))
    return spline, coefs.astype(dtype)


def same_as_host(spline, coefs, device_coefs=None):
    """zeros2_batch on a CUDA tensor against the host drivers on the same numbers: equal bits and the same launches."""
    d = torch.from_numpy(np.ascontiguousarray(coefs)).cuda() if device_coefs is None else device_coefs
    values, offsets, cells, status = roots2.zeros2_batch(spline, coefs=d)
    ran = list(roots2.LAST_PATHS)
    last = nv.lib().bsk_roots2_last_kernel().decode()
    assert values.is_cuda and offsets.is_cuda and status.is_cuda
    h_values, h_offsets, h_cells, h_status = roots2.zeros2_batch(spline, coefs=d.cpu().numpy(), _path="host")
    assert launches(ran) == expected(roots2.LAST_PATHS) and last == ran[-1]
    assert len([p for p in ran if p in BANDS]) == len(roots2.Plan2(spline.order, spline.knots).steps)
    assert offsets.cpu().numpy().tolist() == h_offsets.tolist()
    assert values.cpu().numpy().tobytes() == h_values.tobytes()
    assert cells.tobytes() == h_cells.tobytes()
    assert status.cpu().numpy().tobytes() == h_status.tobytes()
    return h_values, h_offsets, ran


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", DEVICE_NAMES)
def test_golden_device(name):
    c = load_case(name)
    if c["kind"] == "tangent":
        host = roots2.zeros2_batch(make_spline(c), _path="host")
        want = expected(roots2.LAST_PATHS)
        dev = roots2.zeros2_batch(make_spline(c), _path="device")
        assert launches(roots2.LAST_PATHS) == want
        assert [a.tobytes() for a in dev] == [a.tobytes() for a in host] and dev[3].any()
        with pytest.raises(ValueError, match=r"zeros2: (tangential or singular zero|zeros not isolated)"):
            make_spline(c).zeros2(_path="device")
        return
    host = make_spline(c).zeros2(_path="host")
    want = expected(roots2.LAST_PATHS)
    found = make_spline(c).zeros2(_path="device")
    ran = list(roots2.LAST_PATHS)
    assert launches(ran) == want and want[0] == "roots2_flag"
    assert nv.lib().bsk_roots2_last_kernel().decode() == ran[-1]
    check_golden(c, found, "zeros2 device")
    assert bits(found) == bits(host), "the device path and the host path differ"
    assert bits(make_spline(c).zeros2(_path="device")) == bits(found), "two runs differ"


def test_goldens_reach_every_launch():
    ran = set()
    for name in ("rand_44", "sep_knots_22"):
        make_spline(load_case(name)).zeros2(_path="device")
        ran |= set(roots2.LAST_PATHS)
    assert ran >= {"roots2_flag", "roots2_isolate", "roots2_merge"} and ran & BANDS


# ------------------------------------------------------------------------------------------ layouts
def test_merge_on_a_3_by_2_grid():
    """Zeros on a vertical edge, on a horizontal edge and at the interior corner of 3 x 2 cells, each found by two or four
    cells and reported once.  p(u) is piecewise linear with roots at the knot 1/3 and at 5/6; q(v) is a C1 quadratic spline
    with Bezier pieces (1, -1, 0) and (0, 1, 2): roots at 1/6 and at the knot 1/2."""
    third = 1.0 / 3.0
    p, q = np.array([1.0, 0.0, -1.0, 1.0]), np.array([1.0, -1.0, 1.0, 2.0])
    coefs = np.stack([np.repeat(p[:, None], 4, axis=1), np.repeat(q[None, :], 4, axis=0)])
    spline = bspy_amd.Spline(2, 2, [2, 3], [4, 4], [[0, 0, third, 2 * third, 1, 1.0], [0, 0, 0, 0.5, 1, 1, 1.0]], coefs)
    values, offsets, ran = same_as_host(spline, coefs[None])
    assert "roots2_merge" in ran
    assert roots2.Plan2(spline.order, spline.knots).ncells == [3, 2]
    want = np.array([[third, 1 / 6], [third, 0.5], [5 / 6, 1 / 6], [5 / 6, 0.5]])
    assert values.shape == (4, 2)
    # |p'| >= 3 and |q'| >= 2 with S = 2: far inside the separable bar of the goldens, which is below 1e-13 here
    assert np.abs(values - want).max() <= 1e-13
    assert values[1, 0] == third and values[1, 1] == 0.5 and values[0, 0] == third and values[3, 1] == 0.5      # exactly at the knots


def test_every_cell_is_a_candidate_across_blocks():
    """17 x 16 bilinear cells, the coefficients of one component alternating in sign like a chessboard and those of the other
    in stripes: 272 candidates, more than a block of any kernel."""
    rng = np.random.default_rng(4)
    i, j = np.meshgrid(np.arange(18), np.arange(17), indexing="ij")
    spline, coefs = system(rng, (2, 2), (17, 16), signs=np.stack([(-1.0) ** (i + j), (-1.0) ** i]))
    roots2.zeros2_batch(spline, coefs=coefs, _path="host")
    plan, rows, mask, scale = roots2.tables(spline, coefs)
    assert roots2._run_host(rows, plan, mask, scale)["flags"].all()
    values, offsets, ran = same_as_host(spline, coefs)
    assert "roots2_isolate" in ran and len(values) > 17 * 16 // 4


def test_systems_of_different_scale():
    """B = 3 systems on the same knots: S_d differs by 1e6 between them, and the last one has no candidates."""
    rng = np.random.default_rng(6)
    spline, coefs = system(rng, (4, 4), (5, 4), B=3)
    coefs[1] *= 1e6
    coefs[1, 1] *= 1e-9
    coefs[2] = np.abs(coefs[2]) + 0.1
    coefs[0, 0, :4, :4] = 0.0                                        # and a zero cell in the first one only
    values, offsets, ran = same_as_host(spline, coefs)
    assert offsets[3] == offsets[2] and offsets[1] > 0 and offsets[2] > offsets[1]
    for b in range(2):                                              # a system alone gives the same bits
        alone, _, _, _ = roots2.zeros2_batch(spline, coefs=coefs[b:b + 1], _path="host")
        assert alone.tobytes() == values[offsets[b]:offsets[b + 1]].tobytes()


def test_no_candidates_skips_the_last_two_launches():
    rng = np.random.default_rng(3)
    spline, coefs = system(rng, (4, 3), (6, 5), B=2, signs=1.0)
    values, offsets, ran = same_as_host(spline, coefs)
    assert launches(ran) == ["roots2_flag"] and len(values) == 0 and offsets.tolist() == [0, 0, 0]
    positive = bspy_amd.Spline(2, 2, spline.order, spline.nCoef, spline.knots, coefs[0])
    assert positive.zeros2(_path="device") == [] and launches(roots2.LAST_PATHS) == ["roots2_flag"]


def test_misaligned_and_strided_input():
    rng = np.random.default_rng(9)
    for order, dtype in (((4, 4), np.float64), ((3, 4), np.float32)):
        spline, coefs = system(rng, order, (5, 6), B=2, dtype=dtype)
        flat = torch.from_numpy(coefs).cuda()
        base = torch.zeros(flat.numel() + 1, dtype=flat.dtype, device="cuda")
        base[1:] = flat.reshape(-1)
        shifted = base[1:].view(flat.shape)                        # one element past the allocation's alignment
        assert shifted.data_ptr() % 16 != 0
        want, _, _ = same_as_host(spline, coefs, shifted)
        wide = torch.zeros((2, 2, flat.shape[2] + 3, flat.shape[3] + 5), dtype=flat.dtype, device="cuda")
        wide[:, :, 1:1 + flat.shape[2], 2:2 + flat.shape[3]] = flat
        view = wide[:, :, 1:1 + flat.shape[2], 2:2 + flat.shape[3]]
        assert not view.is_contiguous()
        got, _, _ = same_as_host(spline, coefs, view)
        assert got.tobytes() == want.tobytes() and len(want) > 0


@pytest.mark.parametrize("order", [(2, 2), (3, 4), (4, 4), (4, 2)], ids=lambda o: f"{o[0]}{o[1]}")
def test_orders(order):
    """9 x 7 cells and 3 systems per order: odd sizes, and candidates that straddle the isolate kernel's block of 64."""
    rng = np.random.default_rng(10 * order[0] + order[1])
    spline, coefs = system(rng, order, (9, 7), B=3)
    values, offsets, ran = same_as_host(spline, coefs)
    assert "roots2_isolate" in ran and len(values) > 0


# ------------------------------------------------------------------------------------------ one realistic call
def bilinear_patches(rng):
    """A piecewise bilinear surface with 4 x 4 control points in space on 3 x 3 cells: per cell the vectors (A, B, C, D) of
    s = A + B x + C y + D x y in the cell's own coordinates, and the breaks."""
    breaks = [np.array([0.0, 0.3, 0.7, 1.0]), np.array([0.0, 0.4, 0.6, 1.0])]
    gx, gy = np.meshgrid(breaks[0], breaks[1], indexing="ij")
    net = np.stack([gx, gy, 0.4 * np.sin(3.0 * gx) * np.cos(2.0 * gy)], axis=-1) + 0.05 * rng.standard_normal((4, 4, 3))
    patches = {}
    for i in range(3):
        for j in range(3):
            p00, p10, p01, p11 = net[i, j], net[i + 1, j], net[i, j + 1], net[i + 1, j + 1]
            patches[i, j] = (p00, p10 - p00, p01 - p00, p11 - p10 - p01 + p00)
    return breaks, patches


def gradient(patch, query, x, y):
    """((s - p) . s_x, (s - p) . s_y) of one bilinear patch in its own coordinates, and the Jacobian of the pair."""
    A, B, C, D = (v[:, None] for v in patch)
    s = A + B * x + C * y + D * x * y - query[:, None]
    sx, sy = B + D * y, C + D * x
    F = np.stack([(s * sx).sum(0), (s * sy).sum(0)])
    J = np.array([[(sx * sx).sum(0), (sx * sy).sum(0) + (s * D).sum(0)], [(sx * sy).sum(0) + (s * D).sum(0), (sy * sy).sum(0)]])
    return F, J


def test_closest_point_candidates_on_a_surface():
    """Closest-point candidates of 5 query points on a surface with 4 x 4 control points, as ONE zeros2_batch call: system q
    is ((s - p_q) . s_u, (s - p_q) . s_v).  The surface is piecewise bilinear: the same system of a bicubic surface has the
    orders (6, 7), above what the kernels (4) and the host drivers (6) take.  Per cell the pair is a polynomial of degree
    (1, 2) and (2, 1), written exactly as a biquadratic Bezier patch; the cells are independent (knots of multiplicity 3).
    Against Newton in NumPy from a 33 x 33 grid of starting points per cell."""
    rng = np.random.default_rng(21)
    breaks, patches = bilinear_patches(rng)
    queries = np.stack([rng.uniform(0.1, 0.9, 5), rng.uniform(0.1, 0.9, 5), 0.2 * rng.standard_normal(5)], axis=1)      # near the surface
    nodes = np.array([0.0, 0.5, 1.0])
    X, Y = (g.ravel() for g in np.meshgrid(nodes, nodes, indexing="ij"))

    def bezier(a):                                                  # Bezier points of quadratics from their values, along axis 0
        return np.array([a[0], 2.0 * a[1] - 0.5 * (a[0] + a[2]), a[2]])

    coefs = np.zeros((5, 2, 9, 9))
    for q in range(5):
        for (i, j), patch in patches.items():
            F, _ = gradient(patch, queries[q], X, Y)
            for d in range(2):
                coefs[q, d, 3 * i:3 * i + 3, 3 * j:3 * j + 3] = bezier(bezier(F[d].reshape(3, 3)).T).T
    knots = [np.concatenate(([b[0]], np.repeat(b, 3), [b[-1]]))[1:-1] for b in breaks]
    spline = bspy_amd.Spline(2, 2, [3, 3], [9, 9], knots, coefs[0])
    values, offsets, cells, status = roots2.zeros2_batch(spline, coefs=torch.from_numpy(coefs).cuda())
    assert launches(roots2.LAST_PATHS)[:2] == ["roots2_flag", "roots2_isolate"] and len(cells) == 0 and not status.any().item()
    values, offsets = values.cpu().numpy(), offsets.cpu().numpy()
    total = 0
    for q in range(5):
        want = []
        for (i, j), patch in patches.items():
            x, y = (g.ravel() for g in np.meshgrid(np.linspace(0.0, 1.0, 33), np.linspace(0.0, 1.0, 33), indexing="ij"))
            for _ in range(40):
                F, J = gradient(patch, queries[q], x, y)
                det = J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
                with np.errstate(all="ignore"):
                    x, y = x - (F[0] * J[1, 1] - J[0, 1] * F[1]) / det, y - (J[0, 0] * F[1] - F[0] * J[1, 0]) / det
            F, _ = gradient(patch, queries[q], x, y)
            ok = np.isfinite(x) & np.isfinite(y) & (np.abs(F).max(axis=0) <= 1e-12) & (x >= 0) & (x <= 1) & (y >= 0) & (y <= 1)
            for a, b in {(round(float(a), 9), round(float(b), 9)) for a, b in zip(x[ok], y[ok])}:
                want.append((breaks[0][i] + a * (breaks[0][i + 1] - breaks[0][i]), breaks[1][j] + b * (breaks[1][j + 1] - breaks[1][j])))
        got = values[offsets[q]:offsets[q + 1]]
        want = np.array(sorted(want)).reshape(-1, 2)
        assert len(got) == len(want), f"query {q}: {len(got)} candidates, Newton from the grid finds {len(want)}"
        # `want` is rounded to 9 digits of the cell's own coordinates
        assert len(want) == 0 or np.abs(got - want).max() <= 1e-9
        total += len(got)
    assert total >= 5
