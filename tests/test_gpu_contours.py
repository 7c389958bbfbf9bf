"""
Spline.contours and contours.trace_batch on the GPU (contour_flag, contour_march count and emit, the band kernels for the
extraction): every golden of tests/golden/contours.npz through ``_path="device"`` with the kernels that ran asserted from
``contours.LAST_PATHS`` and ``bsk_contour_last_kernel``, byte-equal to the host path (which test_contours_host.py holds to
the exact oracle) and on a second run; then the layouts of the launches through ``trace_batch`` on CUDA tensors against the
host drivers, which run the same functions of bsk_contour.hpp: bit for bit.  Then the fitted curves of ``Spline.contours``
(the fit needs the device).  No kernel of the family uses LDS, so it has no stale-LDS test.

THE FITTED CIRCLE.  The largest | |c(t) - centre| - r | over 257 parameter values of our curve must not exceed what the
reference's own contour shows on the same case (``circle/ref_dev`` of the golden file, recorded by the generator); no
margin, the depth is ours to choose.
"""
import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import contours as C
from conftest import observe
from test_contours_host import GOLD, NAMES, spline_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BANDS = {"band_apply", "band_apply_line"}


def launches(ran):
    return [p for p in ran if p not in BANDS]


def expected(host_ran):
    """The launches of the device path from those of the host path on the same numbers."""
    return [p[len("host "):] for p in host_ran if p.startswith("host contour_")]


def blob(out):
    return [(a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).tobytes() for a in out]


def field(rng, order, ncells, B=1, dtype=np.float64):
    """B random fields on ncells[0] x ncells[1] cells with simple interior knots."""
    knots, ncoef = [], []
    for k, nc in zip(order, ncells):
        knots.append(np.concatenate((k * [0.0], np.sort(rng.random(nc - 1)), k * [1.0])))
        ncoef.append(len(knots[-1]) - k)
    coefs = rng.uniform(-1.0, 1.0, (B, *ncoef)).astype(dtype)
    return bspy_amd.Spline(2, 1, list(order), ncoef, knots, coefs[:1]), coefs


def same_as_host(spline, coefs, device_coefs=None, **kwargs):
    """trace_batch on a CUDA tensor against the host drivers on the same numbers: equal bytes and the same launches."""
    d = torch.from_numpy(np.ascontiguousarray(coefs)).cuda() if device_coefs is None else device_coefs
    out = C.trace_batch(spline, coefs=d, **kwargs)
    ran = list(C.LAST_PATHS)
    last = nv.lib().bsk_contour_last_kernel().decode()
    assert out[0].is_cuda and out[5].is_cuda                                  # vertices and status stay on the device
    host = C.trace_batch(spline, coefs=d.cpu().numpy(), _path="host", **kwargs)
    assert launches(ran) == expected(C.LAST_PATHS) and last == ran[-1]
    assert len([p for p in ran if p in BANDS]) == len(C.Plan(spline.order, spline.knots).steps)
    assert blob(out) == blob(host)
    return host, ran


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", NAMES)
def test_golden_device(name):
    s = spline_of(name)
    level = float(GOLD[f"{name}/level"])
    kwargs = dict(levels=None if level == 0.0 else [level], depth=int(GOLD[f"{name}/depth"]))
    host = C.trace_batch(s, _path="host", **kwargs)
    want = expected(C.LAST_PATHS)
    dev = C.trace_batch(s, _path="device", **kwargs)
    ran = list(C.LAST_PATHS)
    assert launches(ran) == want == ["contour_flag", "contour_march count", "contour_march emit"]
    assert nv.lib().bsk_contour_last_kernel().decode() == "contour_march emit"
    assert blob(dev) == blob(host)
    assert blob(C.trace_batch(s, _path="device", **kwargs)) == blob(dev)      # a second run: the same bytes
    assert dev[2].tolist() == GOLD[f"{name}/closed"].tolist()


# ------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("order, ncells, B, depth", [((4, 4), (1, 1), 1, 4), ((3, 4), (3, 2), 1, 3), ((4, 3), (9, 7), 3, 2), ((2, 2), (3, 2), 2, 4)])
def test_layouts_equal_the_host(order, ncells, B, depth):
    spline, coefs = field(np.random.default_rng(11), order, ncells, B)
    host, _ = same_as_host(spline, coefs, depth=depth)
    assert len(host[1]) > 1


def test_a_wave_boundary_and_both_ends_of_the_split():
    # two random fields on 9 x 8 cells: 65 or more candidate cells, so the lanes of P = 0 cross a wave
    spline, coefs = field(np.random.default_rng(5), (3, 3), (9, 8), B=2)
    plan, rows, _, scale = C.tables(spline, None, coefs)
    assert int(C._run_host(rows, plan, None, scale, 2, 0)["cand"].sum()) >= 65
    base = None
    for P in (0, 2):                                           # P = 0 and P = depth
        host, ran = same_as_host(spline, coefs, depth=2, _split=P)
        base = base or blob(host)
        assert blob(host) == base


def test_no_candidate_skips_the_march():
    spline, coefs = field(np.random.default_rng(3), (4, 4), (3, 2))
    host, ran = same_as_host(spline, np.abs(coefs) + 0.5)
    assert launches(ran) == ["contour_flag"] and len(host[0]) == 0 and host[1].tolist() == [0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cuda_coefs_of_both_types_and_a_view(dtype):
    spline, coefs = field(np.random.default_rng(7), (4, 3), (4, 3), B=2, dtype=dtype)
    same_as_host(spline, coefs, depth=3)
    wide = torch.from_numpy(np.ascontiguousarray(np.repeat(coefs, 2, axis=2))).cuda()
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    host, _ = same_as_host(spline, coefs, device_coefs=view, depth=3)
    assert host[0].dtype == np.float64                         # the knots' dtype


def test_levels_on_the_device():
    s = spline_of("circle")
    dev = C.trace_batch(s, levels=[-0.2, 0.0, 0.3], _path="device")
    assert len([p for p in C.LAST_PATHS if p in BANDS]) == len(C.Plan(s.order, s.knots).steps)
    assert blob(dev) == blob(C.trace_batch(s, levels=[-0.2, 0.0, 0.3], _path="host"))


# ------------------------------------------------------------------------------------------ the curves
def test_the_fitted_circle_is_as_round_as_the_reference_s():
    curves = spline_of("circle").contours(_path="device")
    assert len(curves) == 1
    c = curves[0]
    assert c.nInd == 1 and c.nDep == 2 and tuple(c.order) == (4,) and float(c.knots[0][0]) == 0.0 and float(c.knots[0][-1]) == 1.0
    xy = np.array(c(np.linspace(0.0, 1.0, 257)))
    assert np.asarray(c.coefs)[:, 0].tobytes() == np.asarray(c.coefs)[:, -1].tobytes()     # a closed piece has equal end points
    assert np.abs(xy[:, 0] - xy[:, -1]).max() <= 1e-10 * 0.7                # evaluated: the parity bar of the evaluation kernels
    dev = float(np.abs(np.hypot(xy[0], xy[1]) - 0.7).max())
    observe("contours fitted circle | |c(t)| - r | (bar: the reference's own)", dev, float(GOLD["circle/ref_dev"]))


def test_curves_are_sorted_and_zero_cells_come_back_as_cells():
    found = spline_of("zero_cell").contours()
    assert isinstance(found[0], tuple) and found[0] == ((0.0, 0.0), (1.0, 1.0))
    assert len(found) == 2 and found[1].nDep == 2
    curves = spline_of("random_42").contours(_path="device")
    starts = [tuple(float(x) for x in np.array(c(0.0)).reshape(-1)) for c in curves]
    assert len(curves) >= 1 and all(tuple(c.order) == (4,) for c in curves)
    host = spline_of("random_42").contours(_path="host")
    assert [np.asarray(c.coefs).tobytes() for c in curves] == [np.asarray(c.coefs).tobytes() for c in host]
    vertices, offsets, *_ = C.trace_batch(spline_of("random_42"))
    firsts = sorted(tuple(float(x) for x in vertices[o]) for o in offsets[:-1])
    assert len(firsts) == len(starts) and np.allclose(np.array(sorted(starts)), np.array(firsts), atol=1e-9) and starts == sorted(starts)
