"""
``Spline.fit_points`` away from unit scale, on the GPU (scatter_key, scatter_gram, scatter_cell, scatter_fold,
scatter_residual).  The cases, the checks and their reasons are those of tests/test_scatter_scale_host.py, run here with
path="device" and path="cuda" (CUDA tensors in); every run asserts the kernel names from ``info["paths"]`` and
``scatter.LAST_PATHS`` (in ``run``), and the base run of every check is byte for byte the host path's.

A. Exact scaling laws: points x 2^k, weights x 2^k, knots and uvw x 2^kp per variable, the same with smoothing.
B. Shifted and stretched domains against the exact oracle on the stored values, and the same bits as the host.
C. Locality under one ill-scaled point, a cell alone, and a permutation that keeps the cells' internal order.
"""
import pytest

import test_scatter_scale_host as host

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PATHS = ["device", "cuda"]


def same_as_host(base, case, what):
    assert set(host.TABLES) < set(base)
    host.same_run(base, host.run(case, "host"), f"{what} against the host path")


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", host.NAMES)
def test_points_scaling_law(name, path):
    same_as_host(host.check_points_law(host.CASES[name], path), host.CASES[name], name)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", host.NAMES)
def test_weights_scaling_law(name, path):
    same_as_host(host.check_weights_law(host.CASES[name], path), host.CASES[name], name)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", host.NAMES)
def test_domain_scaling_law(name, path):
    same_as_host(host.check_domain_law(host.CASES[name], path), host.CASES[name], name)


# ------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("name", host.SHIFTED)
def test_shifted_domain(name):
    host.check_shifted(name, ["device", "cuda", "host"])


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", host.NAMES)
def test_locality_of_one_point(name, path):
    same_as_host(host.check_locality(host.CASES[name], path), host.CASES[name], name)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", host.NAMES)
def test_one_cell_alone(name, path):
    same_as_host(host.check_cell_alone(host.CASES[name], path), host.CASES[name], name)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", host.NAMES)
def test_permutation_within_the_cells_order(name, path):
    same_as_host(host.check_permutation(host.CASES[name], path), host.CASES[name], name)
