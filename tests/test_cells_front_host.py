"""
What the shared front of the cell families (``_cells.coefs_arg``, ``level_batch``) refuses, without a GPU: the class and
the text of every refusal that no family's own host tests match already, and the one that wins where two apply.  The
cases are those of tests/front_cases.py.
"""
import numpy as np
import pytest
import torch

from bspy_amd import contours, isosurface
from front_cases import MODULES, NAMES, case

BATCH = dict(zeros="zeros_batch", zeros2="zeros2_batch", zeros3="zeros3_batch", contours="trace_batch", isosurface="extract_batch",
             triangulate="triangulate_batch")


def refused(call, error, text, *args, **kwargs):
    with pytest.raises(error) as caught:
        call(*args, **kwargs)
    assert type(caught.value) is error and str(caught.value) == text


@pytest.mark.parametrize("name", NAMES)
def test_a_torch_tensor_must_be_a_float_cuda_tensor(name):
    spline, call, coefs = case(name)
    text = f"{BATCH[name]} takes the coefficients as a float32 or float64 torch CUDA tensor"
    MODULES[name].LAST_PATHS.append("stale")
    refused(call, TypeError, text, torch.from_numpy(coefs))
    assert MODULES[name].LAST_PATHS == []                                     # a refused call ran nothing
    refused(call, TypeError, text, torch.from_numpy(coefs), _path="host")
    refused(call, TypeError, text, torch.from_numpy(coefs).long())
    refused(call, ValueError, "_path must be None, 'device' or 'host'", torch.from_numpy(coefs), _path="gpu")      # the path is looked at first


def test_the_shape_of_the_coefficients():
    spline, call, coefs = case("zeros")
    for bad in (coefs[:, :-1], coefs[0], coefs[None]):
        refused(call, ValueError, "coefs must have the shape (nDep, 6)", bad, _path="host")
    spline, call, coefs = case("contours")
    for bad in (coefs[:, :, :-1], coefs[:, :-1], coefs[0], coefs[None]):
        refused(call, ValueError, "coefs must have the shape (B, 4, 5)", bad, _path="host")
    assert len(call(coefs.astype(np.int64), _path="host")[1]) > 1              # integers are NumPy's to widen: not refused


@pytest.mark.parametrize("name, module, most", [("contours", contours, 8), ("isosurface", isosurface, 6)])
def test_the_level_families_refuse_alike(name, module, most):
    spline, call, coefs = case(name)
    refused(call, ValueError, f"{BATCH[name]} takes levels or coefs, not both", coefs, levels=[0.0], _path="host")
    refused(call, ValueError, f"{BATCH[name]} takes levels or coefs, not both", torch.from_numpy(coefs), levels=[0.0])   # before the tensor is looked at
    batch = getattr(module, BATCH[name])
    for depth in (-1, most + 1):
        refused(batch, ValueError, f"depth must be in 0 .. {most}", spline, depth=depth, _path="host")
    for split in (-1, 3):
        refused(batch, ValueError, "_split must be in 0 .. depth", spline, depth=2, _split=split, _path="host")
    refused(batch, ValueError, f"coefs must have the shape (B, {', '.join(str(m) for m in coefs.shape[1:])})", spline, coefs=coefs[0], depth=-1)
    refused(batch, ValueError, "_path must be None, 'device' or 'host'", spline, _path="gpu")
    plan = module.Plan(spline.order, spline.knots)
    for tolerance in (0.0, -1.0, float("nan")):
        refused(module.depth_of, ValueError, "tolerance must be positive", tolerance, plan)
    assert module.depth_of(float("inf"), plan) == 0 and module.depth_of(None, plan) == module.DEFAULT_DEPTH
