"""
``Spline.triangulate`` on the GPU: the kernels of bsk_mesh.hpp against the host drivers, which run the same functions on the
CPU and which tests/test_mesh_host.py holds to the exact oracle and to the Python statement.  Every comparison is byte for
byte: parameters, vertices, offsets, triangles, levels, bound, status and raw normals.
"""
import warnings

import numpy as np
import pytest

from bspy_amd import _native as nv
from bspy_amd import mesh
from mesh_cases import GOLD, NAMES, ORDERS, arguments, drawn, numpy_of, same, spline_of

pytestmark = pytest.mark.gpu

FULL = ["mesh_bound", "mesh_count", "mesh_emit", "mesh_vertex"]


def ran():
    """The mesh launches of the last call; nothing of it may have run on the host."""
    assert not any(name.startswith("host") for name in mesh.LAST_PATHS)
    return [name for name in mesh.LAST_PATHS if name.startswith("mesh_")]


def both(spline, tolerance, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        host = mesh.triangulate_batch(spline, tolerance, _path="host", **kwargs)
        device = mesh.triangulate_batch(spline, tolerance, _path="device", **kwargs)
    assert ran() == FULL
    assert nv.lib().bsk_mesh_last_kernel().decode() == "mesh_vertex"
    assert same(host, device)
    return numpy_of(device)


@pytest.mark.parametrize("name", NAMES)
def test_goldens_on_the_device(name):
    args = arguments(name)
    s = spline_of(name)
    kwargs = dict(coefs=args["coefs"], max_level=args["max_level"], normals=args["coefs"].shape[1] == 3)
    first = both(s, args["tolerance"], **kwargs)
    assert len(first[3]) == sum(len(GOLD[f"{name}/{b}/triangles"]) for b in range(len(args["coefs"])))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        again = mesh.triangulate_batch(s, args["tolerance"], _path="device", **kwargs)
    assert same(first, again)


@pytest.mark.parametrize("order", ORDERS, ids=lambda k: "%d%d" % k)
def test_every_order_tuple(order):
    s, coefs = drawn(order, (3, 2), 300 + 4 * order[0] + order[1], members=2)
    assert len(both(s, 0.05, coefs=coefs, normals=True)[3]) > 0


def test_more_quads_than_one_workgroup_and_two_chunk_sizes():
    """7 x 5 cells of mixed levels, 1 mod 256 quads or not: the count and emit launches in one piece, in pieces of 256 and in
    pieces of 1000 quads give the same bytes."""
    s, coefs = drawn((4, 3), (7, 5), 41, members=2)
    whole = both(s, 0.01, coefs=coefs, normals=True)
    assert whole[5].max() - whole[5].min() >= 2 and len(whole[3]) > 4096
    for chunk in (256, 1000):
        assert same(whole, mesh.triangulate_batch(s, 0.01, coefs=coefs, normals=True, _path="device", _chunk=chunk))
        assert set(ran()) == set(FULL) and len(ran()) > len(FULL)


def test_the_method_on_the_device():
    s = spline_of("ring")
    tol = arguments("ring")["tolerance"]
    host = s.triangulate(tol, parameters=True, normals=True, _path="host")
    device = s.triangulate(tol, parameters=True, normals=True, _path="device")
    assert ran() == FULL and all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(host, device))
    capped = spline_of("capped")
    with pytest.warns(RuntimeWarning, match="1 cells need more than max_level = 2") as caught:
        capped.triangulate(arguments("capped")["tolerance"], max_level=2, _path="device")
    assert len(caught) == 1
    with pytest.raises(ValueError, match="1024 triangles exceed max_triangles = 1000"):
        spline_of("one_54").triangulate(arguments("one_54")["tolerance"], max_triangles=1000, _path="device")


def test_cuda_coefficients_stay_on_the_device():
    import torch
    s, coefs = drawn((4, 4), (3, 4), 51, members=3)
    host = mesh.triangulate_batch(s, 0.05, coefs=coefs, normals=True, _path="host")
    for dtype in (torch.float64, torch.float32):
        d = torch.from_numpy(coefs).cuda().to(dtype)
        out = mesh.triangulate_batch(s, 0.05, coefs=d, normals=True)
        assert ran() == FULL
        assert all(out[n].is_cuda for n in (0, 1, 2, 3, 4, 5, 7, 8)) and isinstance(out[6], np.ndarray)
        assert out[1].dtype == torch.float64 and out[3].dtype == torch.int64 and out[5].dtype == torch.int32
        assert same(out, host if dtype == torch.float64 else mesh.triangulate_batch(s, 0.05, coefs=coefs.astype(np.float32), normals=True, _path="host"))
    wide = torch.from_numpy(np.repeat(coefs, 2, axis=3)).cuda()
    view = wide[:, :, :, ::2]
    assert not view.is_contiguous()
    assert same(mesh.triangulate_batch(s, 0.05, coefs=view, normals=True), host)
    with pytest.raises(ValueError, match="the coefficients must be finite"):
        bad = torch.from_numpy(coefs).cuda()
        bad[1, 2, 0, 1] = float("nan")
        mesh.triangulate_batch(s, 0.05, coefs=bad)
