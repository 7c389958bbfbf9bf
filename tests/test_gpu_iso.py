"""
``Spline.isosurface`` on the GPU: the kernels of bsk_iso.hpp against the host drivers, which run the same functions on the
CPU and which tests/test_iso_host.py holds to the exact oracle and to the Python statement.  Every comparison is byte for
byte: vertices, keys, offsets, triangles, zero cells and status.
"""
import numpy as np
import pytest

from bspy_amd import _native as nv
from bspy_amd import isosurface as iso
from iso_cases import GOLD, NAMES, ORDERS, drawn, levels_of, numpy_of, same, spline_of

pytestmark = pytest.mark.gpu

FULL = ["iso_flag", "iso_walk count", "iso_walk emit", "iso_leaf count", "iso_leaf emit", "iso_vertex"]


def ran():
    """The iso launches of the last call; nothing of it may have run on the host."""
    assert not any(name.startswith("host") for name in iso.LAST_PATHS)
    return [name for name in iso.LAST_PATHS if name.startswith("iso_")]


def both(spline, expect=FULL, **kwargs):
    host = iso.extract_batch(spline, _path="host", **kwargs)
    device = iso.extract_batch(spline, _path="device", **kwargs)
    assert ran() == expect
    assert nv.lib().bsk_iso_last_kernel().decode() == expect[-1]
    assert same(host, device)
    return numpy_of(device)


@pytest.mark.parametrize("name", NAMES)
def test_goldens_on_the_device(name):
    s, depth = spline_of(name), int(GOLD[f"{name}/depth"])
    first = both(s, levels=levels_of(name), depth=depth)
    assert len(first[3]) == sum(len(GOLD[f"{name}/{b}/triangles"]) for b in range(len(levels_of(name))))
    again = iso.extract_batch(s, levels=levels_of(name), depth=depth, _path="device")
    assert same(first, again)


def test_one_leaf():
    s, _ = drawn((3, 3, 3), (1, 1, 1), 1)
    out = both(s, depth=0)
    assert len(out[3]) > 0


def test_one_cell_at_depth_6_at_both_ends_of_the_split():
    s, _ = drawn((3, 2, 4), (1, 1, 1), 2)
    host = iso.extract_batch(s, depth=6, _path="host")
    assert len(host[3]) > 64 * 64
    for split in (0, 6):
        assert same(host, iso.extract_batch(s, depth=6, _path="device", _split=split)) and ran() == FULL


def test_cells_2_1_3():
    s, _ = drawn((4, 3, 2), (2, 1, 3), 3)
    both(s, depth=2)


def test_cells_5_4_3_and_three_fields():
    s, coefs = drawn((3, 4, 3), (5, 4, 3), 4, fields=3)
    out = both(s, coefs=coefs, depth=1)
    assert np.all(np.diff(out[4]) > 0)


def test_leaf_lanes_one_more_than_a_multiple_of_64():
    """More surviving leaves than one workgroup of iso_leaf lanes, and a count that is 1 mod 64: the level is searched on
    the host, where the walk keeps the same leaves."""
    s, _ = drawn((3, 3, 3), (2, 2, 2), 5)
    plan, rows, _, _ = iso.tables(s)
    for level in np.linspace(-0.5, 0.5, 400):
        _, _, levels, scale = iso.tables(s, [level])
        n = iso._run_host(rows, plan, levels, scale, 3, 1)["nleaves"]
        if n > 256 and n % 64 == 1:
            break
    else:
        pytest.fail("no level with 64 m + 1 surviving leaves")
    both(s, levels=[float(level)], depth=3, _split=1)


def test_a_field_without_candidates():
    s, coefs = drawn((3, 3, 3), (2, 2, 2), 6, fields=3)
    coefs[1] = np.abs(coefs[1]) + 1.0
    out = both(s, coefs=coefs, depth=2)
    assert out[4][1] == out[4][2] and out[4][0] < out[4][1] < out[4][3]
    both(s, coefs=coefs[1:2], depth=2, expect=["iso_flag"])                            # no candidates at all: the walk is skipped


def test_candidates_without_leaves_and_without_triangles():
    """1 - 1.3 B_1(x) + ... is positive on [0, 1] although a coefficient is negative: the cell is a candidate, at depth 1
    every half is dropped, at depth 0 the cell is its own leaf and cuts no edge."""
    s, coefs = drawn((3, 2, 2), (1, 1, 1), 7)
    coefs[0] = np.array([1.0, -0.3, 1.0])[:, None, None]
    assert len(both(s, coefs=coefs, depth=1, expect=FULL[:2])[3]) == 0
    assert len(both(s, coefs=coefs, depth=0, expect=FULL[:4])[3]) == 0


def test_cuda_coefficients_stay_on_the_device():
    import torch
    s, coefs = drawn((4, 4, 4), (2, 3, 2), 8, fields=2)
    host = iso.extract_batch(s, coefs=coefs, depth=2, _path="host")
    for dtype in (torch.float64, torch.float32):
        d = torch.from_numpy(coefs).cuda().to(dtype)
        out = iso.extract_batch(s, coefs=d, depth=2)
        assert ran() == FULL
        assert all(out[n].is_cuda for n in (0, 1, 2, 3, 4, 6)) and out[0].dtype == torch.float64 and out[3].dtype == torch.int64
        assert same(out, host if dtype == torch.float64 else iso.extract_batch(s, coefs=coefs.astype(np.float32), depth=2, _path="host"))
    wide = torch.from_numpy(np.repeat(coefs, 2, axis=3)).cuda()
    view = wide[:, :, :, ::2]
    assert not view.is_contiguous()
    assert same(iso.extract_batch(s, coefs=view, depth=2), host)


def test_levels():
    s, _ = drawn((3, 3, 3), (3, 2, 2), 9)
    out = both(s, levels=[-0.2, 0.0, 0.3], depth=2)
    assert np.all(np.diff(out[2]) > 0)


@pytest.mark.parametrize("order", ORDERS, ids=lambda k: "%d%d%d" % k)
def test_every_order_tuple(order):
    s, _ = drawn(order, (2, 2, 2), 100 + 16 * order[0] + 4 * order[1] + order[2])
    assert len(both(s, depth=1)[3]) > 0


def test_method_and_normals():
    s = spline_of("sphere")
    vh, th = s.isosurface(depth=2, _path="host")
    v, t, n = s.isosurface(depth=2, normals=True, _path="device")
    assert v.tobytes() == vh.tobytes() and t.tobytes() == th.tobytes() and v.dtype == np.float64 and t.dtype == np.int64
    jac = np.asarray(s.jacobian([v[:, 0], v[:, 1], v[:, 2]]), np.float64)[0].T
    assert n.shape == v.shape and n.tobytes() == (jac / np.sqrt((jac * jac).sum(axis=1, keepdims=True))).tobytes()
    radial = v - GOLD["sphere/centre"]
    assert np.abs(n - radial / np.linalg.norm(radial, axis=1, keepdims=True)).max() < 1e-9
