"""
Spline.project and project.project_batch on the GPU (project_seed, project_newton, the band kernels for the extraction
and the sample grid): every golden of tests/golden/project.npz through ``_path="device"`` within the bars of
tests/test_project_host.py and bit-equal to the host path, with the kernels that ran asserted from ``project.LAST_PATHS``
and ``bsk_project_last_kernel``; then the layouts of the two kernels against the host drivers, which run the same functions
of bsk_project.hpp: bit for bit.  The shapes are the smallest at which the kernels can go wrong: 1, 63, 65 and 300 points
(a partial wave, a partial block, two blocks of project_seed and five of project_newton), a 1-cell spline and a 3 x 2-cell
surface, sample counts below, above and no multiple of the tile of 8, a chunk size forced small so that 1, 2 and 3 chunks
occur, 1 and 8 samples per cell, every (nInd, nDep) pair and the lowest and highest order of each.  No kernel of the family
uses LDS, so it has no stale-LDS test.
"""
import warnings

import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import project
from test_project_host import NAMES, check_golden, load_case, make_spline

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BANDS = {"band_apply", "band_apply_line"}


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() and x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a, b))


def check_launches(spline, plan, seeded=True):
    ran = list(project.LAST_PATHS)
    tail = ["project_seed", "project_newton"] if seeded else ["project_newton"]
    assert ran[-len(tail):] == tail and nv.lib().bsk_project_last_kernel().decode() == "project_newton"
    bands = ran[:-len(tail)]
    assert set(bands) <= BANDS and len(bands) == len(plan.steps) + (spline.nInd if seeded else 0)


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", NAMES)
def test_golden_device(name):
    case = load_case(name)
    spline = make_spline(case)
    got = project.project_batch(spline, case["points"], samples=case["samples"], _path="device")
    plan = project.Plan(spline.order, spline.knots, project._samples(spline, case["samples"]))
    check_launches(spline, plan)
    check_golden(name, got[0], got[1], got[2], "device")
    host = project.project_batch(spline, case["points"], samples=case["samples"], _path="host")
    assert same(got, host)
    assert same(project.project_batch(spline, case["points"], samples=case["samples"], _path="device"), got)      # two runs, the same bytes


# ------------------------------------------------------------------------------------------ layouts
def spline_of(rng, order, ncells, nDep):
    knots, ncoef = [], []
    for k, nc in zip(order, ncells):
        knots.append(np.concatenate((k * [0.0], np.sort(rng.random(nc - 1)), k * [1.0])))
        ncoef.append(len(knots[-1]) - k)
    coefs = 0.3 * rng.standard_normal((nDep, *ncoef))
    for a, n in enumerate(ncoef):                                         # a graph over the parameters plus noise
        coefs[a] += np.linspace(0.0, 2.0, n).reshape([-1 if b == a else 1 for b in range(len(ncoef))])
    return bspy_amd.Spline(len(order), nDep, list(order), ncoef, knots, coefs)


SHAPES = [((2,), (1,), 2), ((2,), (3,), 3), ((6,), (1,), 3), ((6,), (3,), 2),
          ((2, 2), (1, 1), 2), ((2, 2), (3, 2), 3), ((4, 4), (1, 1), 3), ((4, 4), (3, 2), 2), ((2, 4), (3, 2), 3), ((3, 3), (3, 2), 2)]
# (points, samples per cell and axis, chunks)
RUNS = [(1, None, 1), (63, 1, 2), (65, 8, 3), (300, (3, 5), 3), (300, None, 1)]


@pytest.mark.parametrize("order,ncells,nDep", SHAPES)
def test_layouts_equal_the_host_drivers(order, ncells, nDep):
    rng = np.random.default_rng(sum(order) * 100 + sum(ncells) * 10 + nDep)
    spline = spline_of(rng, order, ncells, nDep)
    seen = set()
    for N, samples, chunks in RUNS:
        if isinstance(samples, tuple):
            samples = samples[:len(order)]
        plan = project.Plan(spline.order, spline.knots, project._samples(spline, samples))
        M = plan.nsamples
        chunk = -(-M // min(chunks, M))
        seen.add((-(-M // chunk), M % 8 == 0, M < 8))
        points = 1.0 + 1.2 * rng.standard_normal((nDep, N))
        points[:, N // 2] = np.nan if N > 1 else points[:, N // 2]           # a skipped lane in the middle of a wave
        got = project.project_batch(spline, points, samples=samples, _path="device", _chunk=chunk)
        check_launches(spline, plan)
        host = project.project_batch(spline, points, samples=samples, _path="host", _chunk=chunk)
        assert same(got, host), (N, samples, chunks)
        assert N == 1 or got[2][N // 2] == project.STATUS_SKIPPED
    assert {c for c, _, _ in seen} >= ({1, 2, 3} if max(ncells) > 1 else {1})
    assert any(not multiple and not below for _, multiple, below in seen) or max(ncells) == 1


# ------------------------------------------------------------------------------------------ tensors, guesses, warnings
def test_cuda_tensors_in_cuda_tensors_out():
    case = load_case("surface_k43_float32")
    spline = make_spline(case)
    points = np.tile(case["points"], (1, 20))
    want = project.project_batch(spline, points, _path="device")
    for dtype in (np.float64, np.float32):
        d_points = torch.from_numpy(points.astype(dtype)).cuda()
        got = project.project_batch(spline, d_points)
        assert all(t.is_cuda for t in got) and got[0].dtype == torch.float32 and got[1].dtype == torch.float64
        assert got[2].dtype == torch.uint8 and got[3].dtype == torch.int32
        ref = want if dtype == np.float64 else project.project_batch(spline, points.astype(dtype), _path="host")
        assert same([t.cpu().numpy() for t in got], ref)
    shaped = project.project_batch(spline, d_points.reshape(3, 7, 20))
    assert shaped[0].shape == (2, 7, 20) and shaped[1].shape == (7, 20)
    with pytest.raises(ValueError, match="points on the device take the device path"):
        project.project_batch(spline, d_points, _path="host")
    with pytest.raises(TypeError, match="same kind"):
        project.project_batch(spline, d_points, guess=np.zeros((2, 140)))
    d_points[0, 3] = float("nan")
    with pytest.warns(RuntimeWarning, match=r"1 of 140 points .* flat index 3"):
        uvw, distance = spline.project(d_points)
    assert uvw.is_cuda and distance.is_cuda and bool(torch.isnan(distance[3])) and not bool(torch.isnan(distance[4]))


@pytest.mark.parametrize("name", ["curve_k6", "surface_k24_mixed", "surface_k44_shifted"])
def test_guess_equals_the_host_result(name):
    case = load_case(name)
    spline = make_spline(case)
    rng = np.random.default_rng(3)
    points = np.tile(case["points"], (1, 10))
    width = np.array([float(k[-1]) - float(k[0]) for k in case["knots"]])[:, None]
    guess = np.tile(case["u"], (1, 10)) + 0.02 * width * rng.standard_normal((len(case["order"]), points.shape[1]))
    got = project.project_batch(spline, points, guess=guess, _path="device")
    plan = project.Plan(spline.order, spline.knots, project._samples(spline, None))
    check_launches(spline, plan, seeded=False)
    assert same(got, project.project_batch(spline, points, guess=guess, _path="host"))
    d_got = project.project_batch(spline, torch.from_numpy(points).cuda(), guess=torch.from_numpy(guess).cuda())
    assert same([t.cpu().numpy() for t in d_got], got)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        uvw, distance = spline.project(points, guess=guess, _path="device")
    assert uvw.tobytes() == got[0].tobytes() and distance.tobytes() == got[1].tobytes()
