"""
The cell families away from unit scale, on the GPU: roots2_flag / roots2_isolate / roots2_merge, roots3_flag /
roots3_isolate / roots3_merge, project_seed / project_newton, contour_flag / contour_march and band_absmax / band_absmax_line
(DESIGN.md sections 17-21).  The cases, the checks and their reasons are those of tests/test_scale_cells_host.py (CPU
preconditions), run here with path="device" and, for the batch calls, with path="cuda": CUDA tensors in, CUDA tensors out.
Every result is tied to the kernels that made it (``LAST_PATHS``, asserted in the run_* functions before and after every
transform).

A. Exact scaling laws through the public batch calls, bit for bit after undoing the power of two.
B. Shifted and stretched domains against the exact references on the stored shifted values, and the same bits as the host.
C. Locality under one ill-scaled coefficient, and batch independence.
D. ``project`` at and beyond the range in which its squares are finite.
"""
import pytest

import cases
import test_scale_cells_host as host

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

A = host.CELLS_A
ZEROS = {**A["zeros2"], **A["zeros3"]}


def same_as_host(dev, on_host, what):
    for key, value in dev.items():
        if key == "ran":
            continue
        if key in ("knots",):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(value, on_host[key])), (what, key)
        elif key == "rounds":
            assert value == on_host[key], (what, key)
        else:
            host.assert_bits(value, on_host[key], f"{what}: {key} on the device against the host path")


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("path", ["device", "cuda"])
@pytest.mark.parametrize("name", sorted(ZEROS))
def test_zeros_scaling_law(name, path):
    base = host.check_zeros_law(ZEROS[name], path)
    same_as_host(base, host.run_zeros(ZEROS[name], "host"), name)


@pytest.mark.parametrize("path", ["device", "cuda"])
@pytest.mark.parametrize("guess", [False, True], ids=["seeded", "guess"])
@pytest.mark.parametrize("name", sorted(A["project"]))
def test_project_scaling_law(name, guess, path):
    base = host.check_project_law(A["project"][name], path, guess)
    same_as_host(base, host.run_project(A["project"][name], "host", guess), name)


@pytest.mark.parametrize("name", sorted(A["contours"]))
def test_contours_scaling_law(name):
    case = A["contours"][name]
    base = host.check_contours_law(case, "device")
    same_as_host(base, host.run_contours(case, "host"), name)
    if case.args["levels"] is None:                                      # fields of their own: CUDA tensors in
        same_as_host(host.check_contours_law(case, "cuda"), base, name + " from CUDA tensors")


@pytest.mark.parametrize("name", sorted(A["remove_knots"]))
def test_remove_knots_scaling_law(name):
    case = A["remove_knots"][name]
    assert host.check_remove_law(case, "device") == host.check_remove_law(case, "host")
    for tolerance in host.CC["tolerances"]:
        same_as_host(host.run_remove(host.refined(case), "device", tolerance), host.run_remove(host.refined(case), "host", tolerance), name)


@pytest.mark.parametrize("name", sorted(host.ABSMAX))
def test_absmax_scaling_law(name):
    host.check_absmax_law(host.ABSMAX[name], "device")


def test_every_kernel_is_named_by_every_part():
    """The cases declare their kernels and the run_* functions assert them on every device run, so the declarations are
    what ran: every kernel of the five families in part A, in part B and in part C."""
    every = host.ALL_KERNELS
    assert every == set().union(*cases.CELL_KERNELS.values()) and len(every) == 12
    part_a = set().union(*(c.kernels for listed in A.values() for c in listed.values())) | {s[6] for s in host.ABSMAX.values()}
    part_c = set().union(*(c.kernels for c in host.INDEPENDENT.values())) | {s[6] for s in host.ABSMAX.values()}
    part_c |= set().union(*(host.local_system(f).kernels for f in host.LOCAL_FAMILIES))
    part_b = set().union(*(c.kernels for c in host.shifted_cases()))
    for part, named in (("A", part_a), ("B", part_b), ("C", part_c)):
        assert named == every, (part, every - named)


# ------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("name", sorted(host.SHIFTED))
def test_shifted_domain(name):
    host.check_shifted(host.SHIFTED[name], ["device", "host"])


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("family", host.LOCAL_FAMILIES)
def test_cell_locality(family):
    same_as_host(host.check_cell_locality(family, "device"), host.check_cell_locality(family, "host"), family)


@pytest.mark.parametrize("name", sorted(host.ABSMAX))
def test_absmax_locality(name):
    host.check_absmax_locality(host.ABSMAX[name], "device")


# levels come with the spline's own NumPy coefficients: no CUDA tensor goes in
INDEPENDENT_RUNS = [(n, p) for n, c in sorted(host.INDEPENDENT.items()) for p in ("device", "cuda")
                    if p == "device" or c.args.get("levels") is None]


@pytest.mark.parametrize("name,path", INDEPENDENT_RUNS)
def test_batch_independence(name, path):
    host.check_independence(host.INDEPENDENT[name], path)


# ------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("path", ["device", "cuda"])
@pytest.mark.parametrize("guess", [False, True], ids=["seeded", "guess"])
@pytest.mark.parametrize("name", sorted(n for n, c in A["project"].items() if c.kind == "fp64"))
def test_project_beyond_the_range_of_its_squares(name, guess, path):
    host.check_project_beyond(A["project"][name], path, guess)
