"""
One run per operator family for tests/test_gpu_side_stream.py and tests/test_poisoned_scratch_host.py: the smallest case
that the family's own GPU test already compares with the host path, as ``run(path) -> Result``.  ``path`` is "host" or
"device"; the inputs are NumPy arrays and go to the device inside the run, on the stream that is current then.  ``bits`` are
the bytes of everything the call returns, ``ran`` the launches that ``LAST_PATHS`` (or the family's own list) names.  No
workload is drawn here: every case is one of the family's test.

``FAMILIES[name] = (run, exact)``: ``exact`` says that the device path gives the host path's bytes.  Where it does not
(band, product and fit kernels: the family's test holds the device to the host at a bar), ``near(name, got, want)`` is that
test's comparison and the bytes are pinned to the device's own first run.
"""
import collections
import functools
import os
import warnings

import numpy as np

import cases
import fit_ref
import iso_cases
import mesh_cases
import robust_cases
import surfaces_util
import test_fit_host
import test_product_host
import test_rays_host
import test_roots_host
import test_scale_cells_host as cells
from bspy_amd import Spline, fitting, isosurface, mesh, product, rays, refinement, roots, sums, surfaces
from bspy_amd._backend import Device, Host
from conftest import GOLDEN

Result = collections.namedtuple("Result", "bits ran")


def bits_of(x):
    """The bytes of a result, whatever it is made of: arrays, CUDA tensors, splines, numbers and containers of them."""
    if isinstance(x, (list, tuple)):
        return tuple(bits_of(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, bits_of(v)) for k, v in sorted(x.items()))
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    if isinstance(x, Spline):
        return bits_of([x.order, x.nCoef, list(x.knots), x.coefs])
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    return repr(x)


def arrays_of(bits):
    """The float arrays among ``bits_of``'s output, flattened: what ``near`` compares."""
    out = []
    for b in bits:
        if isinstance(b, tuple) and len(b) == 3 and isinstance(b[2], bytes):
            if b[0].startswith("float"):
                out.append(np.frombuffer(b[2], np.dtype(b[0])).astype(np.float64))
        elif isinstance(b, tuple):
            out.extend(arrays_of(b))
    return out


def smallest(listed, kind="fp64", needs=()):
    """The smallest case of a family in test_scale_cells_host.CELLS_A that declares the kernels ``needs``."""
    fit = [c for c in listed.values() if c.kind == kind and set(needs) <= c.kernels]
    assert fit, (kind, needs)
    return min(fit, key=lambda c: (c.coefs.size, c.name))


def without_ran(d):
    return {k: v for k, v in d.items() if k != "ran"}


# ------------------------------------------------------------------------------------------ the cell families
def run_zeros(path):
    """roots.zeros_batch on the first golden curve of tests/golden/roots.npz whose host run isolates a root."""
    s = _roots_spline()
    out = roots.zeros_batch(s, _path=path)
    return Result(bits_of(out), tuple(roots.LAST_PATHS))


@functools.lru_cache(maxsize=None)
def _roots_spline():
    for name in test_roots_host.NAMES:
        s = test_roots_host.make_spline(test_roots_host.load_case(name))
        roots.zeros_batch(s, _path="host")
        if "host roots_isolate" in roots.LAST_PATHS and max(s.order) <= 8:
            return s
    raise AssertionError("no golden curve isolates a root")


def zeros_n(family):
    case = smallest(cells.CELLS_A[family], needs={f"roots{family[-1]}_merge"})

    def run(path):
        got = cells.run_zeros(case, path)
        return Result(bits_of(without_ran(got)), tuple(got["ran"]))
    return run


def project_of(guess):
    case = smallest(cells.CELLS_A["project"])

    def run(path):
        got = cells.run_project(case, path, guess)
        return Result(bits_of(without_ran(got)), tuple(got["ran"]))
    return run


def run_contours(path):
    got = cells.run_contours(smallest(cells.CELLS_A["contours"]), path)
    return Result(bits_of(without_ran(got)), tuple(got["ran"]))


def iso_of(order, ncells, seed):
    def run(path):
        s, _ = iso_cases.drawn(order, ncells, seed)
        out = isosurface.extract_batch(s, depth=2, _path=path)
        return Result(bits_of(iso_cases.numpy_of(out)), tuple(isosurface.LAST_PATHS))
    return run


def run_mesh(path):
    s, coefs = mesh_cases.drawn((4, 3), (3, 2), 316, members=2)               # test_gpu_mesh.test_every_order_tuple's (4, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = mesh.triangulate_batch(s, 0.05, coefs=coefs, normals=True, _path=path)
    return Result(bits_of(mesh_cases.numpy_of(out)), tuple(mesh.LAST_PATHS))


def rays_of(hits):
    def run(path):
        s = test_rays_host.graph_surface((4, 4), (3, 2), seed=21)                   # test_gpu_rays.test_no_candidates_and_all_candidates
        o, d = test_rays_host.down_rays(np.random.default_rng(3), 130)
        out = rays.cast_batch(s, o, d, hits=hits, _path=path)
        return Result(bits_of(out), tuple(rays.LAST_PATHS))
    return run


def run_surfaces(path):
    c = surfaces_util.load_case("loop")
    a, b = surfaces_util.make(c)
    r = surfaces.trace_pair(a, b, depth=c["depth"], _path=path)
    pairs = [r[4]["families"][f][k] for f in range(4) for k in surfaces_util.PER_PAIR]
    return Result(bits_of([r[0], r[1], r[2], r[3].segments, r[3].leaves, pairs]), tuple(surfaces.LAST_PATHS))


# ------------------------------------------------------------------------------------------ scatter, fit, band, sum, product
def scatter_of(**more):
    def run(path):
        args = {k: v for k, v in more.items() if not (path == "host" and k == "solve")}     # the host path has one solve
        s, info = robust_cases.fit("curve", _path=path, **args)
        keep = {k: info[k] for k in ("weights", "residual", "scale", "objective", "rounds", "rms", "max") if k in info}
        return Result(bits_of([s.coefs, keep]), tuple(info["paths"]))
    return run


@functools.lru_cache(maxsize=None)
def _fit_case():
    return test_fit_host.load_case(np.load(os.path.join(GOLDEN, "least_squares.npz")), "surface_o43")


def run_least_squares(path):
    c = _fit_case()
    s = Spline.least_squares(c["u"], c["data"], c["order"], c["knots_in"], c["compression"], c["tolerance"], c["fixEnds"], _path=path)
    return Result(bits_of(s), tuple(fitting.LAST_PATHS))


def run_fit_plan(path):
    """The per-variable driver of tests/test_fit_host.py on the same golden: one plan per variable from fit_ref's band, the
    host plan or fit_sweep (the last variable's lines are contiguous: fit_sweep turned).  Needs no GPU on the host path."""
    c = _fit_case()
    data, ran = np.ascontiguousarray(c["data"], np.float64), []
    if path == "device":
        import torch
        data = torch.from_numpy(data).cuda()
    for iv, (u, o, k) in enumerate(zip(c["u"], c["order"], c["knots"])):
        first, values = fit_ref.banded_matrix(k, o, u)
        shape = tuple(data.shape)
        outer, inner = int(np.prod(shape[:iv + 1])), int(np.prod(shape[iv + 2:]))
        with fitting.Plan(first, values, len(k) - o) as plan:
            x = plan.solve_host(data, outer, inner) if path == "host" else plan.sweep(data.contiguous(), outer, inner)
            ran.append(plan.last_kernel())
        data = x.reshape(shape[:iv + 1] + (len(k) - o,) + shape[iv + 2:])
    return Result(bits_of([data]), tuple(ran))


def run_steps_of(dtype):
    def run(path):
        data, steps = cases.band_pipeline(dtype)
        log = []
        if path == "host":
            with Host() as be:
                got = refinement.run_steps(be, data, steps, log)
        else:
            import torch
            t = torch.from_numpy(data).cuda()
            with Device(t.device) as be:
                got = refinement.run_steps(be, t, steps, log)
        return Result(bits_of([got]), tuple(log))
    return run


def run_sums(path):
    """A running sum along a middle axis (scan_apply) and along the last one (scan_line), both over more than one chunk and
    in three segments, and a broadcast sum (sum_bcast): shapes of tests/test_gpu_sum.py."""
    rng = np.random.default_rng(41)
    n = 2 * sums.SCAN_CHUNK + 1
    ran, out = [], []
    with sums.ScanMap(rng.random(n) + 0.1 * rng.standard_normal(n)) as scan:
        for shape, axis in (((5, n, 37), 1), ((700, n), 1)):
            a = rng.standard_normal(shape)
            outer, inner = int(np.prod(shape[:axis])), int(np.prod(shape[axis + 1:]))
            if path == "host":
                out.append(scan.apply_host(a, outer, inner).reshape(shape[:axis] + (n + 1,) + shape[axis + 1:]))
            else:
                import torch
                out.append(sums.scan(scan, torch.from_numpy(a).cuda(), axis, _segments=3))
            ran.append(scan.last_kernel())
    a, b = rng.standard_normal((3, 5, 6, 37)), rng.standard_normal((3, 1, 6, 37))
    if path == "host":
        out.append(sums._add_host(a, b, -1))
        ran.append("host sum")
    else:
        import torch
        out.append(sums.add_tensors(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), -1))
        ran.extend(sums.LAST_PATHS)
    return Result(bits_of(out), tuple(ran))


@functools.lru_cache(maxsize=None)
def _product_case(M):
    g = np.load(os.path.join(GOLDEN, "product.npz"))
    fit = []
    for name in test_product_host.NAMES:
        c = test_product_host.load_case(g, name)
        if len(c["pairs"]) == M and c["coefs1"].dtype == c["coefs2"].dtype == np.float64 and all(2 <= c["order1"][a] <= 6 and 2 <= c["order2"][b] <= 6 for a, b in c["pairs"]):
            fit.append(c)
    return min(fit, key=lambda c: (c["out_coefs"].size, c["name"]))


def product_of(M):
    def run(path):
        r = test_product_host.run_case(_product_case(M), path)
        return Result(bits_of(r), tuple(product.LAST_PATHS))
    return run


def run_remove(path):
    case = smallest(cells.CELLS_A["remove_knots"], needs={"band_absmax", "band_absmax_line"})
    got = cells.run_remove(cells.refined(case), path, cells.CC["tolerances"][1])
    return Result(bits_of(without_ran(got)), tuple(got["ran"]))


FAMILIES = {
    "zeros": (run_zeros, True),
    "zeros2": (zeros_n("zeros2"), True),
    "zeros3": (zeros_n("zeros3"), True),
    "project seeded": (project_of(False), True),
    "project guess": (project_of(True), True),
    "contours": (run_contours, True),
    "isosurface (3, 3, 3) on 2 x 2 x 2 cells": (iso_of((3, 3, 3), (2, 2, 2), 5), True),
    "isosurface (4, 4, 4), 64 coefficients": (iso_of((4, 4, 4), (1, 1, 1), 11), True),
    "mesh": (run_mesh, True),
    "rays first": (rays_of("first"), True),
    "rays all": (rays_of("all"), True),
    "surfaces": (run_surfaces, True),
    "scatter": (scatter_of(), True),
    "scatter robust, device solve": (scatter_of(robust="tukey", solve="device", iterations=2, smoothing=2.0 ** -20), True),
    "least_squares": (run_least_squares, False),
    "fit plan": (run_fit_plan, False),
    "run_steps fp64": (run_steps_of(np.float64), False),
    "run_steps fp32": (run_steps_of(np.float32), False),
    "sums": (run_sums, True),
    "product M = 1": (product_of(1), False),
    "product M = 2": (product_of(2), False),
    "remove_knots": (run_remove, True),
}

# the device path against the host path where the bytes may differ: the bars of the families' own tests, of the result's scale
NEAR = {"least_squares": 1e-10, "fit plan": 1e-10, "run_steps fp64": 1e-12, "run_steps fp32": 2.0 ** -23, "product M = 1": 1e-12, "product M = 2": 1e-12}


# the host path of these calls the library's device code as well (the collocation matrix of Spline.least_squares is made by
# bsk_bspline_values): it is no case of the test that runs without a GPU
HOST_NEEDS_GPU = {"least_squares"}


def near(name, got, want):
    """``got`` (device) within the family's bar of ``want`` (host): every float array, relative to its largest entry."""
    a, b = arrays_of(got.bits), arrays_of(want.bits)
    assert len(a) == len(b) and a, name
    for x, y in zip(a, b):
        assert x.shape == y.shape, name
        scale = max(float(np.abs(y).max()), 1e-300) if y.size else 1.0
        err = float(np.abs(x - y).max()) / scale if y.size else 0.0
        assert err <= NEAR[name], f"{name}: the device path is {err:.3e} of the scale away from the host path (bar {NEAR[name]:g})"


def same_numbers(got, want):
    """Two ``bits_of`` results of float arrays hold the same numbers: equal bytes, or a NaN in both.  For the point kernels,
    whose NaN at a degenerate point of a normal comes with either sign from run to run (a NaN has no value to compare).  A
    buffer of bytes 0xFF is NaN in every element, so an element that a kernel left unwritten passes this under that
    pattern where the result is NaN too, and fails it under 0x5A, which is a finite number: the tests run both."""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        if a[:2] != b[:2]:
            return False
        if a[2] != b[2]:
            x, y = np.frombuffer(a[2], np.dtype(a[0])), np.frombuffer(b[2], np.dtype(b[0]))
            if not ((x.view(f"u{x.itemsize}") == y.view(f"u{y.itemsize}")) | (np.isnan(x) & np.isnan(y))).all():
                return False
    return True


def differing(got, want, pattern):
    """For a failure's message: per array of two ``bits_of`` results that differs, how many bytes differ, how many of
    those hold the poison ``pattern`` in ``got``, and where the first one is."""
    out = []

    def walk(a, b, at):
        if isinstance(a, tuple) and len(a) == 3 and isinstance(a[2], bytes):
            if a != b:
                if not (isinstance(b, tuple) and len(b) == 3 and isinstance(b[2], bytes) and len(a[2]) == len(b[2])):
                    out.append(f"{at}: {a[:2]} against {b[:2] if isinstance(b, tuple) else b}")
                    return
                x, y = np.frombuffer(a[2], np.uint8), np.frombuffer(b[2], np.uint8)
                bad = np.flatnonzero(x != y)
                item = np.dtype(a[0]).itemsize
                out.append(f"{at} {a[0]}{a[1]}: {len(bad)} of {len(x)} bytes differ, {int((x[bad] == pattern).sum())} of them are "
                           f"{pattern:#x}; elements {int(bad[0]) // item} .. {int(bad[-1]) // item}")
        elif isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b):
            for i, (u, v) in enumerate(zip(a, b)):
                walk(u, v, f"{at}[{i}]")
        elif a != b:
            out.append(f"{at}: {str(a)[:80]} against {str(b)[:80]}")
    walk(got, want, "result")
    return "; ".join(out)


@functools.lru_cache(maxsize=None)
def on_host(name):
    """Step (a): the host path's result, computed once a session."""
    return FAMILIES[name][0]("host")


def host_names(ran):
    """What the host path ran, under the device's names."""
    return [p[len("host "):] if p.startswith("host ") else p for p in ran]
