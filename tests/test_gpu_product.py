"""
Spline.multiply on the GPU (band_product_line, band_product_tile): every device-eligible golden of
tests/golden/product.npz through ``_path="device"`` at the bars of tests/test_product_host.py (whose helpers are used
here), the device path against the host path, tensor layouts through ``product.apply``, and one realistic call.  Every
device result is tied to the kernel that made it (``product.LAST_PATHS``, bsk_product_last_kernel), so that a host result
cannot pass as a GPU one.

Layout bars: float64 1e-12 of S = nTerms x max |a| x max |b| (the parity bar); float32 2^-23 of S - both paths add the same
fp64 products and round once to float32, so they differ by at most one unit in the last place of the largest value.
"""
import os

import numpy as np
import pytest

from bspy_amd import Spline, product
from conftest import GOLDEN, observe
from test_product_host import NAMES, check_golden, load_case, random_knots, run_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32_ULP = 2.0 ** -23
KERNEL = {1: "band_product_line", 2: "band_product_tile"}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "product.npz"))


def eligible(c):
    return len(c["pairs"]) in (1, 2) and all(2 <= c["order1"][a] <= 6 and 2 <= c["order2"][b] <= 6 for a, b in c["pairs"])


def test_the_goldens_reach_both_kernels(golden):
    counts = {1: 0, 2: 0}
    for name in NAMES:
        c = load_case(golden, name)
        if eligible(c):
            counts[len(c["pairs"])] += 1
    assert counts[1] >= 20 and counts[2] >= 8


@pytest.mark.parametrize("name", NAMES)
def test_golden_device(golden, name):
    c = load_case(golden, name)
    if not eligible(c):
        if c["pairs"]:
            with pytest.raises((ValueError, NotImplementedError)):
                run_case(c, "device")
        return
    r = run_case(c, "device")
    assert product.LAST_PATHS == [KERNEL[len(c["pairs"])]], product.LAST_PATHS
    check_golden(c, r, "product device")
    again = run_case(c, "device")
    assert again.coefs.tobytes() == r.coefs.tobytes(), "two runs differ"
    host = run_case(c, "host")
    assert product.LAST_PATHS == ["host product"]
    err = np.abs(np.asarray(r.coefs, np.float64) - np.asarray(host.coefs, np.float64)).max() / c["scale"]
    if r.coefs.dtype == np.float32:
        observe("product device against host fp32", err, F32_ULP)
    else:
        observe("product device against host fp64", err, 1e-12)


# ------------------------------------------------------------------------------------------ layouts
_MAPS = {}


def some_map(shapes, k1, k2):
    """ProductMap of len(shapes) mapped variables: variable v has shapes[v] = (coefficients of a, coefficients of b) and
    orders (k1, k2), each cut down to the coefficient count where that is smaller.  Random knots with a double knot in a,
    b shares one knot with a.  One map per key and session."""
    key = (tuple(shapes), k1, k2)
    if key not in _MAPS:
        rng = np.random.default_rng(1000 * k1 + 10 * k2 + len(shapes))
        pairs = []
        for n1, n2 in shapes:
            o1, o2 = min(k1, n1), min(k2, n2)
            t, s = random_knots(rng, o1, n1), random_knots(rng, o2, n2)
            if n1 - o1 > 1 and n2 - o2 > 1:
                s[o2] = t[o1 + 1]
                s[o2:n2] = np.sort(s[o2:n2])
            pairs.append((t, o1, s, o2))
        _MAPS[key] = product.ProductMap.from_knots(pairs)[0]
    return _MAPS[key]


def compare(maps, a, b, terms, label):
    """product.apply on the device against the host driver on the same arrays."""
    want = maps.apply_host(a, b, terms)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    del product.LAST_PATHS[:]
    got = product.apply(maps, ta, tb, terms)
    assert product.LAST_PATHS == [KERNEL[maps.M]] and maps.last_kernel() == KERNEL[maps.M]
    assert got.is_cuda and got.dtype == ta.dtype and tuple(got.shape) == want.shape
    again = product.apply(maps, ta, tb, terms)
    assert torch.equal(got, again), "two runs differ"
    scale = terms.shape[1] * np.abs(a).max() * np.abs(b).max()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max() / scale
    if a.dtype == np.float32:
        observe(f"product layouts fp32 {label}", err, F32_ULP)
    else:
        observe(f"product layouts fp64 {label}", err, 1e-12)


ORDER_PAIRS = [(2, 2), (2, 6), (3, 5), (4, 4), (6, 6)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k1,k2", ORDER_PAIRS)
def test_layouts_line(dtype, k1, k2):
    """Lines below, near and above one tile of 256 output rows; 1, 3, 37 and 700 planes; scalar, dot and cross tables."""
    rng = np.random.default_rng(50 + k1 + k2)
    for n1, n2 in ((7, 9), (120, 75), (1030, 640)):
        maps = some_map([(n1, n2)], k1, k2)
        assert maps.nOut[0] % 256 != 0, "the last tile is ragged"
        tables = [(planes, product.plane_table(product.dependent_terms("S", 1, 1), planes, 1)) for planes in (1, 3, 37, 700)]
        tables += [(3 * 37, product.plane_table(product.dependent_terms(ptype, 3, 3), 37, 1)) for ptype in ("D", "C")]
        for planes_a, terms in tables:
            planes_b = int(terms[:, :, 1].max()) + 1
            a = rng.standard_normal((planes_a, n1)).astype(dtype)
            b = rng.standard_normal((planes_b, n2)).astype(dtype)
            compare(maps, a, b, terms, f"line orders {k1} x {k2}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k1,k2", ORDER_PAIRS)
def test_layouts_tile(dtype, k1, k2):
    """Surfaces smaller than one tile, several tiles in both directions, long and thin both ways; the orders are cut down
    to the coefficient count of a variable where that is smaller (120 x 5 with order 6 does not exist)."""
    rng = np.random.default_rng(60 + k1 + k2)
    ragged = [False, False]
    for (n1, n2), (m1, m2) in (((9, 11), (10, 8)), ((40, 37), (33, 41)), ((120, 5), (120, 6)), ((5, 300), (4, 300))):
        maps = some_map([(n1, m1), (n2, m2)], k1, k2)
        ragged[0] |= maps.nOut[0] > 16 and maps.nOut[0] % 16 != 0
        ragged[1] |= maps.nOut[1] > 64 and maps.nOut[1] % 64 != 0
        for ptype, nDep, U in (("S", 1, 1), ("S", 1, 3), ("D", 3, 1), ("C", 3, 2)):
            terms = product.plane_table(product.dependent_terms(ptype, nDep, nDep), U, 1)
            a = rng.standard_normal((nDep * U, n1, n2)).astype(dtype)
            b = rng.standard_normal((nDep, m1, m2)).astype(dtype)
            compare(maps, a, b, terms, f"tile orders {k1} x {k2}")
    assert all(ragged), "a ragged last tile in each direction"


def test_far_jumping_map_reads_the_input_in_place():
    """Maps made by hand whose rows are far apart: the pieces under a tile of rows do not fit LDS."""
    rng = np.random.default_rng(61)
    n_out, k1, k2 = 300, 3, 2
    f, g = np.arange(n_out) * 40, np.arange(n_out) * 25
    W = rng.random((n_out, k1, k2))
    n1, n2 = int(f[-1]) + k1, int(g[-1]) + k2
    line = product.ProductMap([(f, g, W, n1, n2)])
    terms = product.plane_table(product.dependent_terms("C", 3, 3), 2, 1)
    compare(line, rng.standard_normal((6, n1)), rng.standard_normal((3, n2)), terms, "far rows, line")
    line.close()
    rows = 20                                          # variable 1: 20 rows 40 apart; variable 2: 100 rows 10 apart
    f2, g2 = np.arange(100) * 10, np.arange(100) * 7
    tile = product.ProductMap([(f[:rows], g[:rows], W[:rows], int(f[rows - 1]) + k1, int(g[rows - 1]) + k2),
                               (f2, g2, W[:100], int(f2[-1]) + k1, int(g2[-1]) + k2)])
    terms = product.plane_table(product.dependent_terms("D", 2, 2))
    compare(tile, rng.standard_normal((2, *tile.nIn1)), rng.standard_normal((2, *tile.nIn2)), terms, "far rows, tile")
    tile.close()


def test_apply_checks_its_arguments():
    maps = some_map([(20, 12)], 3, 3)
    terms = product.plane_table(product.dependent_terms("S", 1, 1))
    a = torch.zeros(1, 20, device="cuda", dtype=torch.float64)
    b = torch.zeros(1, 12, device="cuda", dtype=torch.float64)
    with pytest.raises(TypeError, match="CUDA"):
        product.apply(maps, a.cpu(), b, terms)
    with pytest.raises(TypeError, match="float32 or two float64"):
        product.apply(maps, a, b.float(), terms)
    with pytest.raises(ValueError, match="the map takes"):
        product.apply(maps, a[:, :19], b, terms)
    with pytest.raises(product.nv.BskError, match="plane outside"):
        product.apply(maps, a, b, np.array([[[1, 0, 1]]], np.int32))
    out = product.apply(maps, a + 2.0, b + 3.0, terms)
    assert torch.allclose(out, torch.full_like(out, 6.0), atol=1e-12)          # rows sum to one


def test_default_dispatch_takes_the_device_for_large_results():
    rng = np.random.default_rng(62)
    t = random_knots(rng, 4, 300)
    s = Spline(2, 3, (4, 4), (300, 300), [t, t], rng.standard_normal((3, 300, 300)))
    (s @ s)
    assert product.LAST_PATHS == ["band_product_tile"]
    c = Spline(1, 3, (4,), (300,), [t], rng.standard_normal((3, 300)))
    (c * c)
    assert product.LAST_PATHS == ["host product"]


# ------------------------------------------------------------------------------------------ one realistic call
def test_normal_field_of_a_surface():
    """128 x 128 x 3 bicubic s: n = s_u x s_v as a spline, on the device; n evaluated on the GPU at 10^4 points against the
    cross product of the evaluated derivatives, within 1e-10 of its scale."""
    rng = np.random.default_rng(128)
    n, k = 128, 4
    knots = []
    for _ in range(2):
        interior = np.linspace(0.0, 1.0, n - k + 2)[1:-1]
        interior += (rng.random(n - k) - 0.5) * 0.6 / (n - k + 1)
        knots.append(np.concatenate((k * [0.0], interior, k * [1.0])))
    s = Spline(2, 3, (k, k), (n, n), knots, rng.standard_normal((3, n, n)))
    su, sv = s.differentiate(0), s.differentiate(1)
    normal = su.cross(sv, _path="device")
    assert product.LAST_PATHS == ["band_product_tile"]
    assert normal.order == (6, 6) and normal.nDep == 3
    uv = rng.random((2, 10_000))
    got = np.stack(normal(uv[0], uv[1]))
    du, dv = np.stack(s.derivative([1, 0], uv[0], uv[1])), np.stack(s.derivative([0, 1], uv[0], uv[1]))
    want = np.cross(du.T, dv.T).T
    observe("product normal field against the cross product of derivatives", np.abs(got - want).max() / np.abs(want).max(), 1e-10)
