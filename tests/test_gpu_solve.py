"""
``bsk_scatter_solve`` against ``bsk_scatter_solve_host`` through the C ABI, BYTE FOR BYTE in ``coefs`` and ``bad_row``: the
systems, stencils, laws and refusals of tests/solve_sweep.py (there is no tolerance).  The workspace is filled with NaN before
every call, so a stale band or workspace can change nothing; one case runs with a workspace of zeros and gives the same bytes.
"""
import ctypes

import numpy as np
import pytest

import solve_sweep as sw
from bspy_amd import _native as nv
from bspy_amd import scatter

pytestmark = pytest.mark.gpu


def device_solver(sy, stencil, rhs, fill=float("nan"), name="bsk_scatter_solve", more=()):
    import torch
    L = nv.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    ndep = rhs.shape[1]
    need = np.zeros(1, np.int64)
    nv.check(L.bsk_scatter_solve_work(*sy.head, ndep, need.ctypes.data_as(nv._i64p)))
    assert need[0] == 2 * sy.n * (sy.hb + 1) + ndep * sy.n
    s = torch.from_numpy(np.ascontiguousarray(stencil, np.float64)).to(dev)
    r = torch.from_numpy(np.ascontiguousarray(rhs, np.float64)).to(dev)
    work = torch.full((int(need[0]) + 8,), fill, dtype=torch.float64, device=dev)
    guard = work[int(need[0]):]
    coefs = torch.full((ndep, sy.n), fill, dtype=torch.float64, device=dev)
    bad = torch.full((1,), 77, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nv.check(getattr(L, name)(*sy.head, ndep, s.data_ptr(), r.data_ptr(), coefs.data_ptr(), work.data_ptr(), int(need[0]), bad.data_ptr(),
                              *more, stream))
    assert L.bsk_scatter_last_kernel() == b"scatter_solve"
    bad = int(bad.cpu()[0])
    assert sw.bits(guard.cpu().numpy()) == sw.bits(np.full(8, fill))           # nothing behind the workspace is written
    return (coefs.cpu().numpy() if bad == -1 else None), bad


@pytest.mark.parametrize("sy", sw.SYSTEMS, ids=repr)
def test_device_solve_is_the_host_solve(sy):
    sw.sweep(device_solver, sw.host_solver, names=(sy.name,))


@pytest.mark.parametrize("name", ["curve2_n32", "curve4_n65", "full_4x4", "edge_2x2_4x31", "panels_10x10", "holes_4x4_9x4", "mixed_34_13x11"])
def test_laws_of_the_device_solve(name):
    sy = sw.BY_NAME[name]
    sw.law_channels(device_solver, sy)
    sw.law_scale(device_solver, sy)
    sw.law_twice(device_solver, sy)
    stencil, rhs = sw.cases(sy)["assembled"]
    assert sw.bits(device_solver(sy, stencil, rhs, fill=0.0)[0]) == sw.bits(device_solver(sy, stencil, rhs)[0])


@pytest.mark.parametrize("name", sw.REFUSALS)
def test_refusals_of_the_device_solve(name):
    sw.check_refusals(device_solver, sw.host_solver, sw.BY_NAME[name])


def test_stages_of_the_measurement_hook_compose():
    sy = sw.BY_NAME["panels_10x10"]
    stencil, rhs = sw.cases(sy)["smoothed"]
    whole = device_solver(sy, stencil, rhs)[0]
    assert sw.bits(device_solver(sy, stencil, rhs, name="bsk_debug_scatter_solve", more=(15,))[0]) == sw.bits(whole)


def test_scatter_solve_takes_cuda_tensors_and_numpy():
    import torch
    sy = sw.BY_NAME["mixed_34_9x7"]
    sh = scatter.Shape(sy.order, sy.knots)
    stencil, rhs = sw.cases(sy)["assembled"]
    want = sw.bits(sw.host_solver(sy, stencil, rhs)[0])
    there = [torch.from_numpy(a).cuda() for a in (stencil, rhs)]
    assert sw.bits(scatter.solve(sh, *there)) == want and scatter.LAST_PATHS[-1] == "scatter_solve"
    assert sw.bits(scatter.solve(sh, *there, where="host")) == want and scatter.LAST_PATHS[-1] == "host scatter_solve"
    assert sw.bits(scatter.solve(sh, stencil, rhs, where="device")) == want and scatter.LAST_PATHS[-1] == "scatter_solve"
    bad, brhs, row = sw.refusals(sw.BY_NAME["panels_10x10"])["negative_later"]
    with pytest.raises(ValueError, match=f"the pivot of row {row} .coefficient .4, 0.. is not positive; more data or smoothing > 0"):
        scatter.solve(scatter.Shape((4, 4), sw.BY_NAME["panels_10x10"].knots), bad, brhs, where="device")
