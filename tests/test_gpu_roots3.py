"""
Spline.zeros3 and roots3.zeros3_batch on the GPU (roots3_flag, roots3_isolate, roots3_merge, the band kernels for the
extraction): every golden of tests/golden/roots3.npz through ``_path="device"`` (bars of tests/test_roots3_host.py) with
the kernels that ran asserted from ``roots3.LAST_PATHS`` and ``bsk_roots3_last_kernel``, bit-equal to the host path and on
a second run; then the layouts of the three kernels through ``zeros3_batch`` on CUDA tensors against the host drivers,
which run the same functions of bsk_roots3.hpp: bit for bit; then curves against a surface as one batch, against Newton
in NumPy.  No kernel of the family uses LDS, so it has no stale-LDS test.
"""
import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import roots3
from test_roots3_host import NAMES, TANGENT, check_crossings, check_golden, curves_and_surface, load_case, make_spline

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BANDS = {"band_apply", "band_apply_line"}


def bits(found):
    return [np.asarray(r).tobytes() for r in found]


def launches(ran):
    return [p for p in ran if p not in BANDS]


def expected(host_ran):
    """The launches of the device path from those of the host path on the same numbers."""
    return [p[len("host "):] for p in host_ran if p.startswith("host roots3_")]


def system(rng, order, ncells, B=1, dtype=np.float64, signs=None, jitter=1.0):
    """B random systems on ncells[0] x ncells[1] x ncells[2] cells with simple interior knots (jitter < 1: nearly uniform)."""
    knots, ncoef = [], []
    for k, nc in zip(order, ncells):
        inner = np.arange(1, nc) / nc + jitter * (np.sort(rng.random(nc - 1)) - np.arange(1, nc) / nc)
        knots.append(np.concatenate((k * [0.0], inner, k * [1.0])))
        ncoef.append(len(knots[-1]) - k)
    coefs = rng.standard_normal((B, 3, *ncoef))
    if signs is not None:
        coefs = (1.0 + 0.02 * rng.random((B, 3, *ncoef))) * signs(*np.meshgrid(*(np.arange(n) for n in ncoef), indexing="ij"))
    spline = bspy_amd.Spline(3, 3, list(order), ncoef, knots, coefs[0].astype(dtype))
    return spline, coefs.astype(dtype)


def same_as_host(spline, coefs, device_coefs=None):
    """zeros3_batch on a CUDA tensor against the host drivers on the same numbers: equal bits and the same launches."""
    d = torch.from_numpy(np.ascontiguousarray(coefs)).cuda() if device_coefs is None else device_coefs
    values, offsets, cells, status = roots3.zeros3_batch(spline, coefs=d)
    ran = list(roots3.LAST_PATHS)
    last = nv.lib().bsk_roots3_last_kernel().decode()
    assert values.is_cuda and offsets.is_cuda and status.is_cuda
    h_values, h_offsets, h_cells, h_status = roots3.zeros3_batch(spline, coefs=d.cpu().numpy(), _path="host")
    assert launches(ran) == expected(roots3.LAST_PATHS) and last == launches(ran)[-1]
    assert len([p for p in ran if p in BANDS]) == len(roots3.Plan3(spline.order, spline.knots).steps)
    assert offsets.cpu().numpy().tolist() == h_offsets.tolist()
    assert values.cpu().numpy().tobytes() == h_values.tobytes()
    assert cells.tobytes() == h_cells.tobytes()
    assert status.cpu().numpy().tobytes() == h_status.tobytes()
    return h_values, h_offsets, ran, h_status


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", NAMES)
def test_golden_device(name):
    c = load_case(name)
    if c["kind"] == "tangent":
        host = roots3.zeros3_batch(make_spline(c), _path="host")
        want = expected(roots3.LAST_PATHS)
        dev = roots3.zeros3_batch(make_spline(c), _path="device")
        assert launches(roots3.LAST_PATHS) == want
        assert [a.tobytes() for a in dev] == [a.tobytes() for a in host]
        assert dev[3].max() & roots3.STATUS_TANGENT and (dev[3] != 0).sum() == 1           # bit 4, in the one cell
        with pytest.raises(ValueError, match=TANGENT):
            make_spline(c).zeros3(_path="device")
        return
    host = make_spline(c).zeros3(_path="host")
    want = expected(roots3.LAST_PATHS)
    found = make_spline(c).zeros3(_path="device")
    ran = list(roots3.LAST_PATHS)
    assert launches(ran) == want and want[0] == "roots3_flag"
    assert len([p for p in ran if p in BANDS]) == len(roots3.Plan3(c["order"], c["knots"]).steps)
    assert nv.lib().bsk_roots3_last_kernel().decode() == launches(ran)[-1]
    check_golden(c, found, "zeros3 device")
    assert bits(found) == bits(host), "the device path and the host path differ"
    assert bits(make_spline(c).zeros3(_path="device")) == bits(found), "two runs differ"


# ------------------------------------------------------------------------------------------ layouts
def planted():
    """(p(u), p(v), p(w)) on 2 x 2 x 2 cells: p is a C0 quadratic spline with the Bezier pieces (1, -1, 0) and (0, 1, 2) on
    [0, 1/2] and [1/2, 1]: (1 - s)(1 - 3 s) on the first, so it vanishes at 1/6 and at the knot 1/2."""
    knots = [np.array([0, 0, 0, 0.5, 0.5, 1, 1, 1.0])] * 3
    p = np.array([1.0, -1.0, 0.0, 1.0, 2.0])
    coefs = np.stack([np.broadcast_to(p[:, None, None], (5, 5, 5)), np.broadcast_to(p[None, :, None], (5, 5, 5)),
                      np.broadcast_to(p[None, None, :], (5, 5, 5))]).copy()
    return bspy_amd.Spline(3, 3, [3, 3, 3], [5, 5, 5], knots, coefs), coefs


def test_merge_across_faces_edges_and_the_corner():
    """The zeros {1/6, 1/2}^3 on 2 x 2 x 2 cells: one inside a cell, three on a knot plane (found by two cells each), three
    on an edge (four cells) and one at the interior corner (eight cells); each is reported once."""
    spline, coefs = planted()
    assert roots3.Plan3(spline.order, spline.knots).ncells == [2, 2, 2]
    values, offsets, ran, status = same_as_host(spline, coefs[None])
    assert launches(ran) == ["roots3_flag", "roots3_isolate", "roots3_merge"] and not status.any()
    want = np.array(sorted((u, v, w) for u in (1 / 6, 0.5) for v in (1 / 6, 0.5) for w in (1 / 6, 0.5)))
    # |p'| = 4 at both zeros and S = 2: the 1-D bar 4 eps + 8 K eps S / |p'| = 16 eps per axis
    assert values.shape == (8, 3) and np.abs(values - want).max() <= 16 * np.finfo(float).eps
    assert (values[-1] == 0.5).all()                                 # exactly at the corner


ORDERS = [(2, 2, 2), (2, 3, 4), (3, 3, 3), (4, 4, 2), (4, 4, 4)]


def chessboard(order, B=3, seed=0):
    """5 x 4 x 3 nearly uniform cells whose B-spline coefficients alternate in sign along one axis per component, growing
    slowly in size (equal sizes let a quadratic spline touch zero at the knots without crossing): every component has a
    zero in every cell, so every cell is a candidate.  The test asserts it."""
    rng = np.random.default_rng(100 * order[0] + 10 * order[1] + order[2] + seed)
    return system(rng, order, (5, 4, 3), B=B, jitter=0.1, signs=lambda i, j, k: np.stack([(-1.0) ** i * (1 + 0.1 * i), (-1.0) ** j * (1 + 0.1 * j), (-1.0) ** k * (1 + 0.1 * k)])[None])


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "".join(map(str, o)))
def test_every_cell_is_a_candidate(order):
    """B = 3 systems on 5 x 4 x 3 cells, all 180 of them candidates: odd sizes, distinct counts and orders per axis."""
    spline, coefs = chessboard(order)
    plan, rows, mask, scale = roots3.tables(spline, coefs)
    assert roots3.Plan3(spline.order, spline.knots).ncells == [5, 4, 3]
    assert roots3._run_host(rows, plan, mask, scale)["flags"].all()
    values, offsets, ran, status = same_as_host(spline, coefs)
    assert "roots3_isolate" in ran and len(values) > 0


def test_systems_of_different_scale():
    """B = 3 systems on the same knots: S_d differs by 1e6 between them, one has a zero cell and the last one no candidates."""
    rng = np.random.default_rng(6)
    spline, coefs = system(rng, (3, 3, 2), (3, 2, 2), B=3)
    coefs[1] *= 1e6
    coefs[1, 1] *= 1e-9
    coefs[2] = np.abs(coefs[2]) + 0.1
    coefs[0, 0, :3, :3, :2] = 0.0                                    # a zero cell in the first one only
    values, offsets, ran, status = same_as_host(spline, coefs)
    assert offsets[3] == offsets[2] and "roots3_isolate" in ran
    _, _, cells, _ = roots3.zeros3_batch(spline, coefs=coefs, _path="host")
    assert len(cells) == 1 and cells[0, 0] == 0.0
    for b in range(2):                                              # a system alone gives the same bits
        alone, _, _, _ = roots3.zeros3_batch(spline, coefs=coefs[b:b + 1], _path="host")
        assert alone.tobytes() == values[offsets[b]:offsets[b + 1]].tobytes()


def test_a_long_axis_and_rows_far_larger_than_the_tables():
    """A 9 x 8-coefficient bicubic surface against a 64-coefficient cubic curve: 6 x 5 x 61 cells and extracted rows of
    3 x 19 x 16 x 184 doubles, far more than the per-cell tables hold (1830 bytes of flags).  The launches take the number
    of SYSTEMS, not of unfolded components: with 3 B for B the flag kernel would write 2 x 1830 bytes behind the flags and
    read the rows of systems that do not exist."""
    rng = np.random.default_rng(12)
    knots = [np.concatenate((4 * [0.0], np.sort(rng.random(n - 4)), 4 * [1.0])) for n in (9, 8, 64)]
    gu, gv = np.meshgrid(np.linspace(0, 1, 9), np.linspace(0, 1, 8), indexing="ij")
    surface = np.stack([gu, gv, 0.3 * np.sin(5.0 * gu) * np.cos(4.0 * gv)]) + 0.01 * rng.standard_normal((3, 9, 8))
    t = np.linspace(0, 1, 64)
    curve = np.stack([0.5 + 0.4 * np.cos(9.0 * t) * t, 0.5 + 0.4 * np.sin(9.0 * t) * t, 0.5 * np.cos(14.0 * t)])
    coefs = (surface[:, :, :, None] - curve[:, None, None, :])[None]
    spline = bspy_amd.Spline(3, 3, [4, 4, 4], [9, 8, 64], knots, coefs[0])
    plan = roots3.Plan3(spline.order, spline.knots)
    assert plan.ncells == [6, 5, 61] and plan.rowlen == [19, 16, 184]
    values, offsets, ran, status = same_as_host(spline, coefs)
    assert "roots3_isolate" in ran and len(values) > 0 and not status.any()


def test_no_candidates_skips_the_last_two_launches():
    rng = np.random.default_rng(3)
    spline, coefs = system(rng, (4, 3, 2), (3, 3, 2), B=2)
    coefs = np.abs(coefs) + 0.1
    values, offsets, ran, status = same_as_host(spline, coefs)
    assert launches(ran) == ["roots3_flag"] and len(values) == 0 and offsets.tolist() == [0, 0, 0]
    positive = bspy_amd.Spline(3, 3, spline.order, spline.nCoef, spline.knots, coefs[0])
    assert positive.zeros3(_path="device") == [] and launches(roots3.LAST_PATHS) == ["roots3_flag"]


def test_misaligned_and_strided_input():
    rng = np.random.default_rng(9)
    for order, dtype in (((3, 3, 3), np.float64), ((2, 3, 4), np.float32)):
        spline, coefs = system(rng, order, (3, 2, 2), B=2, dtype=dtype)
        flat = torch.from_numpy(coefs).cuda()
        base = torch.zeros(flat.numel() + 1, dtype=flat.dtype, device="cuda")
        base[1:] = flat.reshape(-1)
        shifted = base[1:].view(flat.shape)                        # one element past the allocation's alignment
        assert shifted.data_ptr() % 16 != 0
        want, _, _, _ = same_as_host(spline, coefs, shifted)
        wide = torch.zeros((2, 3, flat.shape[2] + 3, flat.shape[3] + 5, flat.shape[4] + 2), dtype=flat.dtype, device="cuda")
        wide[:, :, 1:1 + flat.shape[2], 2:2 + flat.shape[3], 1:1 + flat.shape[4]] = flat
        view = wide[:, :, 1:1 + flat.shape[2], 2:2 + flat.shape[3], 1:1 + flat.shape[4]]
        assert not view.is_contiguous()
        got, _, _, _ = same_as_host(spline, coefs, view)
        assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------ one realistic call
def test_curves_against_a_surface_as_one_batch():
    """s(u, v) - c_b(t) for B = 4 curves as ONE zeros3_batch call; the (B, 3, 6, 6, 5) tensor is a broadcast subtraction on the
    device.  Against Newton in NumPy; tests/test_roots3_host.py::test_curves_against_a_surface_on_the_host holds the same
    comparison on the host path."""
    knots, surface, curves, want = curves_and_surface()
    spline = bspy_amd.Spline(3, 3, [4, 4, 4], [6, 6, 5], list(knots), surface[:, :, :, None] - curves[0][:, None, None, :])
    s, c = torch.from_numpy(surface).cuda(), torch.from_numpy(curves).cuda()
    coefs = s[None, :, :, :, None] - c[:, :, None, None, :]
    assert tuple(coefs.shape) == (4, 3, 6, 6, 5)
    values, offsets, cells, status = roots3.zeros3_batch(spline, coefs=coefs)
    assert launches(roots3.LAST_PATHS)[:2] == ["roots3_flag", "roots3_isolate"] and len(cells) == 0 and not status.any().item()
    assert len([p for p in roots3.LAST_PATHS if p in BANDS]) == len(roots3.Plan3(spline.order, spline.knots).steps) == 3
    check_crossings(values.cpu().numpy(), offsets.cpu().numpy(), knots, want)
