"""
The banded solve on the CPU: ``bsk_scatter_solve_host`` against the plain-float statement ``scatter.solve_statement`` over the
systems, stencils, laws and refusals of tests/solve_sweep.py, byte for byte; the generators themselves (the integer family
is symmetric, strictly diagonally dominant, made of integers and solved exactly; the systems cross the constants of the
device solve); and ``scatter.solve`` with its arguments.
"""
import numpy as np
import pytest

import solve_sweep as sw
from bspy_amd import _native as nv
from bspy_amd import scatter


def test_systems_cross_the_panel_constants():
    hb = {s.name: s.hb for s in sw.SYSTEMS}
    assert hb["full_4x4"] == 15 == sw.BY_NAME["full_4x4"].n - 1
    assert [hb[f"edge_2x2_4x{n1}"] for n1 in (30, 31, 32)] == [sw.NB - 1, sw.NB, sw.NB + 1]
    assert sw.BY_NAME["panels_10x10"].n == 3 * sw.NB + 4
    assert {s.n for s in sw.SYSTEMS if s.nind == 1} >= {2, 3, 4, sw.NB - 1, sw.NB, sw.NB + 1, 2 * sw.NB + 1}
    assert all(s.ncoef[1] == s.order[1] for s in sw.SYSTEMS if s.name.startswith("holes"))


@pytest.mark.parametrize("sy", sw.SYSTEMS, ids=repr)
def test_integer_family_is_symmetric_dominant_and_integral(sy):
    stencil, rhs, x, dense = sw.integer(sy)
    assert np.array_equal(dense, dense.T) and np.array_equal(dense, np.round(dense)) and np.array_equal(rhs, np.round(rhs))
    off = np.abs(dense).sum(axis=1) - np.abs(np.diag(dense))
    assert (np.diag(dense) > off).all()
    assert np.abs(rhs).max() < 2.0 ** 40


@pytest.mark.parametrize("sy", sw.SYSTEMS, ids=repr)
def test_host_solve_is_the_statement(sy):
    sw.sweep(sw.host_solver, sw.statement_solver, names=(sy.name,))


@pytest.mark.parametrize("name", ["curve3_n33", "edge_2x2_4x31", "mixed_34_9x7"])
def test_laws_of_the_host_solve(name):
    sy = sw.BY_NAME[name]
    sw.law_channels(sw.host_solver, sy)
    sw.law_scale(sw.host_solver, sy)
    sw.law_twice(sw.host_solver, sy)


@pytest.mark.parametrize("name", sw.REFUSALS)
def test_refusals_of_the_host_solve_and_the_statement(name):
    sw.check_refusals(sw.host_solver, sw.statement_solver, sw.BY_NAME[name])


def test_solve_arguments():
    sy = sw.BY_NAME["mixed_34_9x7"]
    sh = scatter.Shape(sy.order, sy.knots)
    stencil, rhs = sw.cases(sy)["assembled"]
    assert sw.bits(scatter.solve(sh, stencil, rhs)) == sw.bits(scatter.solve(sh, stencil, rhs, "host")) == sw.bits(sw.host_solver(sy, stencil, rhs)[0])
    assert scatter.LAST_PATHS[-1] == "host scatter_solve"
    with pytest.raises(ValueError, match="where must be None, 'device' or 'host'"):
        scatter.solve(sh, stencil, rhs, "gpu")
    with pytest.raises(ValueError, match="the device solve covers nDep 1 to 4"):
        scatter.solve(sh, stencil, np.zeros((sy.n, 5)), "device")
    bad, _, row = sw.refusals(sw.BY_NAME["panels_10x10"])["zero_later"]
    with pytest.raises(ValueError, match=f"the pivot of row {row} .coefficient .4, 0.. is not positive; more data or smoothing > 0"):
        scatter.solve(scatter.Shape((4, 4), sw.BY_NAME["panels_10x10"].knots), bad, np.zeros((100, 1)))


def test_header_declares_the_new_entry_points():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bspy_amd.h")).read()
    declared = set(re.findall(r"\b(bsk_scatter_[a-z_]+)\s*\(", header))
    new = {"bsk_scatter_solve_work", "bsk_scatter_solve", "bsk_scatter_reweight_host", "bsk_scatter_reweight"}
    assert new <= declared and declared <= set(nv.PRODUCT_SYMBOLS)
    assert "bsk_debug_scatter_solve" in nv.INTERNAL_SYMBOLS
    L = nv.lib()
    assert all(hasattr(L, name) for name in new | {"bsk_debug_scatter_solve"})


def test_workspace_and_scope_of_the_device_solve():
    L, need = nv.lib(), np.zeros(1, np.int64)
    p = need.ctypes.data_as(nv._i64p)
    assert L.bsk_scatter_solve_work(2, 4, 4, 10, 10, 3, p) == nv.BSK_OK and need[0] == 2 * 100 * 34 + 3 * 100
    assert L.bsk_scatter_solve_work(1, 4, 1, 65, 1, 1, p) == nv.BSK_OK and need[0] == 2 * 65 * 4 + 65
    assert L.bsk_scatter_solve_work(2, 4, 4, 10, 10, 5, p) == nv.BSK_ERR_UNSUPPORTED
    assert b"ndep 1 to 4" in L.bsk_last_error()
    assert L.bsk_scatter_solve_work(2, 4, 4, 4, 1365, 1, p) == nv.BSK_ERR_UNSUPPORTED         # hb = 4098
    assert b"half bandwidths up to 4095" in L.bsk_last_error()
    assert L.bsk_scatter_solve_work(2, 4, 4, 4, 1364, 1, p) == nv.BSK_OK                      # hb = 4095
    assert L.bsk_scatter_solve_work(2, 4, 4, 7000, 7000, 1, p) == nv.BSK_ERR_INVALID
    assert b"exceeds 2^27 doubles" in L.bsk_last_error()
