"""
The front that the cell families share (``_cells.coefs_arg``, ``bezier_rows``, ``level_batch``) with CUDA coefficients in,
on the two inputs that no family's own GPU tests hold: no member at all (B == 0: every result element has its type, dtype,
shape and device, and nothing is launched) and a float32 view that is not contiguous (B == 2: the bytes of the host path on
the same values, on the input's device).  The cases are those of tests/front_cases.py.
"""
import numpy as np
import pytest
import torch

import iso_cases
import mesh_cases
from front_cases import MODULES, NAMES, case

pytestmark = pytest.mark.gpu

# what a call returns for CUDA float64 coefficients: (where, dtype, shape for B == 0) per element, in the order of the result
EMPTY = {
    "zeros": [("cuda", "float64", (0,)), ("cuda", "int64", (1,)), ("numpy", "float64", (0, 3))],
    "zeros2": [("cuda", "float64", (0, 2)), ("cuda", "int64", (1,)), ("numpy", "float64", (0, 5)), ("cuda", "uint8", (0, 2, 2))],
    "zeros3": [("cuda", "float64", (0, 3)), ("cuda", "int64", (1,)), ("numpy", "float64", (0, 7)), ("cuda", "uint8", (0, 1, 1, 2))],
    "contours": [("cuda", "float64", (0, 2)), ("numpy", "int64", (1,)), ("numpy", "bool", (0,)), ("numpy", "int64", (0,)),
                 ("numpy", "float64", (0, 5)), ("cuda", "uint8", (0, 2, 2))],
    "isosurface": [("cuda", "float64", (0, 3)), ("cuda", "int64", (0,)), ("cuda", "int64", (1,)), ("cuda", "int64", (0, 3)),
                   ("cuda", "int64", (1,)), ("numpy", "float64", (0, 7)), ("cuda", "uint8", (0, 2, 1, 1))],
    "triangulate": [("cuda", "float64", (0, 2)), ("cuda", "float64", (0, 3)), ("cuda", "int64", (1,)), ("cuda", "int64", (0, 3)),
                    ("cuda", "int64", (1,)), ("cuda", "int32", (0, 2, 2, 2)), ("numpy", "float64", (0, 2, 2)), ("cuda", "uint8", (0, 2, 2)),
                    ("cuda", "float64", (0, 3))],
}
# where the members start: the element of the result that holds the offsets (contours: the field of every polyline)
OFFSETS = dict(zeros=1, zeros2=1, zeros3=1, isosurface=2, triangulate=2)


def same(a, b):
    """Two results, byte for byte."""
    a, b = iso_cases.numpy_of(a), iso_cases.numpy_of(b)
    assert len(a) == len(b)
    for n, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), n
    return True


SAME = dict(isosurface=iso_cases.same, triangulate=mesh_cases.same)


def lives(a, where, device):
    if where == "numpy":
        return isinstance(a, np.ndarray)
    return torch.is_tensor(a) and a.device == device


@pytest.mark.parametrize("name", NAMES)
def test_cuda_coefficients_without_a_member(name):
    spline, call, coefs = case(name)
    d = torch.from_numpy(coefs.astype(np.float64)).cuda()[:0]
    out = call(d)
    assert MODULES[name].LAST_PATHS == []
    assert len(out) == len(EMPTY[name])
    for n, (a, (where, dtype, shape)) in enumerate(zip(out, EMPTY[name])):
        assert lives(a, where, d.device) and str(a.dtype).replace("torch.", "") == dtype and tuple(a.shape) == shape, (n, a)
        if shape == (1,):
            assert a.tolist() == [0]
    with pytest.raises(ValueError, match="^coefficients on the device take the device path$"):
        call(d, _path="host")


@pytest.mark.parametrize("name", NAMES)
def test_a_float32_view_that_is_not_contiguous(name):
    spline, call, coefs = case(name)
    assert coefs.dtype == np.float32 and coefs.shape[0] == 2
    host = call(coefs, _path="host")
    if name == "contours":
        assert sorted(set(host[3].tolist())) == [0, 1]
    else:
        assert np.all(np.diff(host[OFFSETS[name]]) > 0)                 # both members have a result, so the second one's offsets count
    stored = torch.from_numpy(np.ascontiguousarray(coefs.transpose())).cuda()          # the axes reversed in memory
    view = stored.permute(*reversed(range(stored.ndim)))
    assert view.shape == coefs.shape and view.dtype == torch.float32 and not view.is_contiguous()
    assert not torch.equal(view[0], view[1])
    out = call(view)
    ran = list(MODULES[name].LAST_PATHS)
    assert ran and not any(p.startswith("host") for p in ran)
    assert SAME.get(name, same)(out, host)
    for n, (a, (where, _, _)) in enumerate(zip(out, EMPTY[name])):
        assert lives(a, where, view.device), n
