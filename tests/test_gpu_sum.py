"""
add, subtract, integrate and contract on the GPU: every golden of tests/golden/sum.npz that the device path covers
through ``_path="device"`` (bars of tests/test_sum_host.py), with the kernels that ran asserted from ``sums.LAST_PATHS``,
twice with equal bits, and against the host path; then the layouts of scan_apply, scan_line and sum_bcast against the host
drivers, which state the same association without contraction: bit for bit.
"""
import os
from fractions import Fraction

import numpy as np
import pytest

from bspy_amd import refinement, sums
from conftest import GOLDEN, observe
from test_sum_host import F32_BAR, NAMES, check_golden, load_case, make_spline, run_case, surface

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sum.npz"))


def _band_kernels(shape, steps):
    """The band kernel of every step as refinement runs them: lines along the last axis that is not 1 are contiguous."""
    shape, ran = list(shape), []
    for axis, first, w in refinement._ordered(steps, shape):
        ran.append("band_apply_line" if int(np.prod(shape[axis + 1:])) == 1 else "band_apply")
        shape[axis] = len(first)
    return ran, shape


def expected_kernels(c):
    """None when the device path does not cover the case, else the kernels in the order they run."""
    s = make_spline(c)
    if c["op"] == "integrate":
        return ["scan_line" if c["wrt"] == s.nInd - 1 else "scan_apply"]
    if c["op"] == "contract":
        steps = [(iv + 1, [0], np.zeros((1, s.order[iv]))) for iv, u in enumerate(c["uvw"]) if u is not None]
        return _band_kernels(s.coefs.shape, steps)[0] if all(2 <= np.shape(w)[1] <= 8 for _, _, w in steps) else None
    o = make_spline(c["other"])
    if s.coefs.dtype != o.coefs.dtype:
        return None
    ran = []
    if c["pairs"] is not None:
        for spline, (_, _, stages) in zip((s, o), sums._basis_plans((s, o), c["pairs"])):
            shape = spline.coefs.shape
            for stage in stages:
                kernels, shape = _band_kernels(shape, stage)
                ran += kernels
    return ran + ["sum_bcast"]


@pytest.mark.parametrize("name", NAMES)
def test_golden_device(golden, name):
    c = load_case(golden, name)
    want = expected_kernels(c)
    if want is None:
        with pytest.raises(ValueError, match="device path"):
            run_case(c, "device")
        return
    r = run_case(c, "device")
    assert sums.LAST_PATHS == want
    check_golden(c, r, "sum device")
    again = run_case(c, "device")
    assert again.coefs.tobytes() == r.coefs.tobytes()
    host = run_case(c, "host")
    if c["op"] == "integrate" or c["pairs"] is None and c["op"] != "contract":
        assert host.coefs.tobytes() == r.coefs.tobytes()                 # no band step: one association, no contraction
    else:
        scale = np.abs(c["coefs"]).max() + (np.abs(c["other"]["coefs"]).max() if c["other"] else 0.0)
        bar = F32_BAR if r.coefs.dtype == np.float32 else 1e-12
        observe(f"sum device against host {c['op']} {r.coefs.dtype.name}",
                np.abs(r.coefs.astype(np.float64) - host.coefs.astype(np.float64)).max() / scale, bar)


def test_goldens_reach_every_kernel(golden):
    seen = set()
    for name in NAMES:
        seen.update(expected_kernels(load_case(golden, name)) or [])
    assert seen == {"band_apply", "band_apply_line", "sum_bcast", "scan_apply", "scan_line"}


# ------------------------------------------------------------------------------------------ scan layouts
CHUNK = sums.SCAN_CHUNK
SCAN_N = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 4 * CHUNK, 4 * CHUNK + 1, 8 * CHUNK + 1, 300)
SCAN_SHAPES = (((1, None, 64), 1), ((5, None, 37), 1), ((3, None, 1), 1), ((None, 7, 9), 0), ((4, 6, None), 2), ((2, None, 514), 1),
               ((None, 1030), 0), ((700, None), 1), ((1, None), 1))


def _misaligned(a):
    """The same values in a CUDA tensor whose first element is one element past a 16-byte boundary."""
    flat = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
    flat[1:] = torch.from_numpy(a).cuda().reshape(-1)
    return flat[1:].view(a.shape)


def check_scan(scan, a, axis, segments, label, misaligned=False):
    outer, inner = int(np.prod(a.shape[:axis])), int(np.prod(a.shape[axis + 1:]))
    shape = list(a.shape)
    shape[axis] += 1
    want = scan.apply_host(a, outer, inner).reshape(shape)
    ta = _misaligned(a) if misaligned else torch.from_numpy(a).cuda()
    assert (ta.data_ptr() % 16 != 0) == misaligned
    got = sums.scan(scan, ta, axis, _segments=segments)
    kernel = "scan_line" if inner == 1 else "scan_apply"
    assert sums.LAST_PATHS == [kernel] and scan.last_kernel() == kernel
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == a.dtype
    # the numbers first (against a long double running sum, at the bars of tests/test_sum_host.py), then the bits
    g = scan.g.reshape([-1 if i == axis else 1 for i in range(a.ndim)]).astype(np.longdouble)
    terms = g * a.astype(np.longdouble)
    scale = float(np.abs(terms).sum(axis=axis).max())
    err = float(np.abs(got.astype(np.longdouble).take(range(1, shape[axis]), axis=axis) - np.cumsum(terms, axis=axis)).max())
    observe(f"sum {kernel} {a.dtype.name} {label}", err / scale, F32_BAR if a.dtype == np.float32 else 1e-12)
    assert np.all(got.take([0], axis=axis) == 0.0)
    assert got.tobytes() == want.tobytes(), f"{kernel} differs from the host driver: shape {a.shape} axis {axis} segments {segments}"
    assert sums.scan(scan, ta, axis, _segments=segments).cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("segments", (1, 2, 5))
def test_scan_layouts(dtype, segments):
    rng = np.random.default_rng(41)
    for n in SCAN_N:
        scan = sums.ScanMap(rng.random(n) + 0.1 * rng.standard_normal(n))
        for shape, axis in SCAN_SHAPES:
            a = rng.standard_normal([n if d is None else d for d in shape]).astype(dtype)
            check_scan(scan, a, axis, segments, f"segments {segments}")
        scan.close()


def test_scan_default_segments_and_misaligned_slices():
    rng = np.random.default_rng(42)
    for n, shape, axis in ((300, (None, 1030), 0), (2500, (3, None), 1), (4097, (1, None), 1), (257, (2, None, 6), 1),
                           (1200, (None, 12), 0)):
        scan = sums.ScanMap(rng.random(n))
        for dtype in (np.float64, np.float32):
            a = rng.standard_normal([n if d is None else d for d in shape]).astype(dtype)
            check_scan(scan, a, axis, None, "default segments")
            check_scan(scan, a, axis, 3, "misaligned", misaligned=True)
        scan.close()


def test_scan_checks_its_arguments():
    scan = sums.ScanMap(np.ones(5))
    with pytest.raises(TypeError):
        sums.scan(scan, np.zeros((2, 5)), 1)
    with pytest.raises(ValueError, match="the map takes 5"):
        sums.scan(scan, torch.zeros((2, 6), dtype=torch.float64, device="cuda"), 1)
    assert sums.scan(scan, torch.zeros((0, 5), dtype=torch.float64, device="cuda"), 1).shape == (0, 6) and sums.LAST_PATHS == []
    scan.close()


# ------------------------------------------------------------------------------------------ sum layouts
def check_sum(a, b, sign, misaligned=False):
    ta = _misaligned(a) if misaligned else torch.from_numpy(a).cuda()
    tb = _misaligned(b) if misaligned else torch.from_numpy(b).cuda()
    got = sums.add_tensors(ta, tb, sign)
    assert sums.LAST_PATHS == ["sum_bcast"] and got.is_contiguous()
    want = (a.astype(np.float64) + sign * b.astype(np.float64)).astype(a.dtype)
    assert got.cpu().numpy().tobytes() == want.tobytes(), f"sum_bcast: shapes {a.shape} {b.shape} sign {sign}"
    assert sums._add_host(a, b, sign).tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_sum_layouts(dtype):
    rng = np.random.default_rng(43)
    for last in (1, 37, 514):
        full = (3, 5, 6, last)
        for other in ((1, 5, 6, last), (3, 1, 6, last), (3, 5, 1, last), (3, 5, 6, 1), (3, 1, 1, last), (1, 5, 1, 1), full):
            a, b = rng.standard_normal(full).astype(dtype), rng.standard_normal(other).astype(dtype)
            for sign in (1, -1):
                check_sum(a, b, sign)
                check_sum(b, a, sign)
            check_sum(a, b, -1, misaligned=True)
    # both operands broadcast (the outer sum), permuted views (last stride not 1) and more than one block of rows
    a, b = rng.standard_normal((3, 70, 1, 1)).astype(dtype), rng.standard_normal((3, 1, 9, 130)).astype(dtype)
    check_sum(a, b, 1)
    ta = torch.from_numpy(rng.standard_normal((3, 40, 50)).astype(dtype)).cuda()
    tb = torch.from_numpy(rng.standard_normal((3, 50, 40)).astype(dtype)).cuda()
    got = sums.add_tensors(ta, tb.permute(0, 2, 1), -1)
    want = (ta.cpu().numpy().astype(np.float64) - tb.cpu().numpy().transpose(0, 2, 1).astype(np.float64)).astype(dtype)
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_sum_checks_its_arguments():
    a = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError):
        sums.add_tensors(a, a.float())
    with pytest.raises(ValueError, match="do not broadcast"):
        sums.add_tensors(a, torch.zeros((2, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="sign"):
        sums.add_tensors(a, a, 2)


# ------------------------------------------------------------------------------------------ whole calls
def test_default_dispatch_takes_the_device_for_large_results():
    rng = np.random.default_rng(44)
    a, b = surface(rng, (4, 4), (150, 160)), surface(rng, (3, 4), (120, 130))
    r = a + b
    assert sorted(sums.LAST_PATHS[:-1]) == 2 * ["band_apply"] + 2 * ["band_apply_line"] and sums.LAST_PATHS[-1] == "sum_bcast"
    host = a.add(b, [0, 1], _path="host")
    assert all(np.array_equal(x, y) for x, y in zip(r.knots, host.knots))
    scale = np.abs(a.coefs).max() + np.abs(b.coefs).max()
    observe("sum device against host large surfaces", np.abs(r.coefs - host.coefs).max() / scale, 1e-12)
    for iv, kernel in ((0, "scan_apply"), (1, "scan_line")):
        r = a.integrate(iv)
        assert sums.LAST_PATHS == [kernel]
        assert r.coefs.tobytes() == a.integrate(iv, _path="host").coefs.tobytes()
    r = a.contract([0.37, None])
    assert sums.LAST_PATHS == ["band_apply"]
    observe("sum device against host contract", np.abs(r.coefs - a.contract([0.37, None], _path="host").coefs).max() / np.abs(a.coefs).max(), 1e-12)


def test_integral_of_a_dot_product_along_one_variable():
    """(s . s) integrated in its first variable and contracted at the right end is, per coefficient line, the exact sum
    of g c over the product's coefficients."""
    rng = np.random.default_rng(45)
    s = surface(rng, (4, 4), (64, 64))
    p = s.dot(s)
    right = float(p.domain()[0][1])
    r = p.integrate(0, _path="device").contract([right, None], _path="device")
    assert sums.LAST_PATHS == ["band_apply"] and r.nInd == 1 and r.order == (p.order[1],)
    t, k = p.knots[0], p.order[0]
    g = [Fraction(float(v)) for v in (t[k:] - t[:len(t) - k]) / k]
    want = np.array([float(sum(gi * Fraction(float(c)) for gi, c in zip(g, p.coefs[0, :, j]))) for j in range(p.nCoef[1])])
    scale = float((np.abs(np.array([float(v) for v in g]))[:, None] * np.abs(p.coefs[0])).sum(axis=0).max())
    observe("sum integral of s . s along one variable", np.abs(r.coefs[0] - want).max() / scale, 1e-12)
