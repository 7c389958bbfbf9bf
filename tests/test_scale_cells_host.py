"""
The cell families away from unit scale, on the host path: zeros2 (roots2_flag / roots2_isolate / roots2_merge), zeros3
(roots3_*), project (project_seed / project_newton), contours (contour_flag / contour_march) and remove_knots (band_absmax /
band_absmax_line); DESIGN.md sections 17-21.  These are the CPU preconditions of tests/test_gpu_scale_cells.py, which runs
the functions of this module with path="device" and, for the batch calls, with path="cuda" (CUDA tensors in): what holds
here and fails there is the device path's fault.  The inputs are cases.cell_scale_cases, the transforms scale_ref.cell_*.

A. The scaling laws of scale_ref.cell_scaled, bit for bit, through the public batch calls: zeros, vertices, foot parameters
   and result knots x 2^kp; distances and result coefficients x 2^ks; offsets, status bytes, step counts, closed, field, the
   zero cells, the removed knots (``LAST_ROUNDS``) and what ``LAST_PATHS`` names unchanged.  Every threshold of the families
   is relative (S_d eps, tau_of, 2^-20 h, TRUST of the domain width, a tolerance relative to max |coefficient|) and every
   rounding commutes with a power of two, so there is nothing to tune.  Families moved off the bitwise law: none.
B. Shifted and stretched domains against the exact references: see the section below.
C. Locality and batch independence, no tolerance: one coefficient x 2^20 and x 2^40 leaves every zero, vertex and status
   byte of every cell whose B-spline window does not hold it bit for bit; a system, a field, a level, a slice of the points
   or a group of lines alone gives the bits it gives in the batch.
D. ``project`` squares coordinates and multiplies the squares.  Its drivers normalise by the power of two of
   max |coefficient| (``project.norm_exponent``), so the law of part A holds at kc = +-250, where the statement alone still
   keeps it, and at +-300 and +-500, where it does not: equal bits with kc = 0.
"""
import numpy as np
import pytest

import cases
import scale_ref as sr
from bspy_amd import Spline, contours, project, reduction, roots2, roots3
from bspy_amd.refinement import BandMap

CC = cases.cell_scale_cases()
CELLS_A = {family: {c.name: c for c in listed} for family, listed in CC["A"].items()}
ALL_KERNELS = set().union(*cases.CELL_KERNELS.values())
LOCAL_POWERS = (20, 40)
EPS = float(np.finfo(np.float64).eps)


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def on_path(a, path):
    """The array as the call takes it on ``path``: a CUDA tensor for "cuda", NumPy otherwise."""
    if a is None or path != "cuda":
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pin(path):
    """The ``_path`` argument: CUDA tensors choose the device path themselves."""
    return None if path == "cuda" else path


def named(ran, path, case):
    """The family's kernels among what ran, checked against the case: on the device exactly the declared ones and nothing
    of the host, on the host the same ones under their host names (remove_knots: the host driver has one name for both)."""
    assert ran, (case.name, "nothing ran")
    host = [p.startswith("host ") for p in ran]
    assert all(host) if path == "host" else not any(host), (case.name, path, ran)
    got = {p[len("host "):].split()[0] if h else p.split()[0] for p, h in zip(ran, host)} & ALL_KERNELS
    if path == "host" and case.family == "remove_knots":
        assert got == {"band_absmax"}, (case.name, ran)
    else:
        assert case.kernels <= got <= case.kernels | case.args.get("optional", set()), (case.name, path, ran)
    return list(ran)


def differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shapes {a.shape} / {b.shape}, types {a.dtype} / {b.dtype}"
    diff = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    return f"{int(diff.sum())} of {a.size} values differ"


def assert_bits(got, want, what):
    assert sr.same_bits(got, want), f"{what}: {differing(got, want)}"


# --------------------------------------------------------------------------------------------- the calls
def run_zeros(case, path, systems=None):
    """zeros2_batch / zeros3_batch of the case's systems (or of ``systems``, a slice of them)."""
    mod, call = (roots2, roots2.zeros2_batch) if case.family == "zeros2" else (roots3, roots3.zeros3_batch)
    coefs = case.coefs if systems is None else case.coefs[systems]
    n = len(case.order)
    spline = Spline(n, n, list(case.order), list(coefs.shape[2:]), case.knots, coefs[0])
    values, offsets, cells, status = call(spline, coefs=on_path(coefs, path), _path=pin(path))
    ran = named(mod.LAST_PATHS, path, case) if systems is None else list(mod.LAST_PATHS)
    assert path != "cuda" or (values.is_cuda and offsets.is_cuda and status.is_cuda)
    values, offsets, status = numpy_of(values), numpy_of(offsets), numpy_of(status)
    assert values.dtype == np.result_type(*(t.dtype for t in case.knots)) and status.shape[0] == len(coefs)
    return dict(values=values, offsets=offsets, cells=cells, status=status, ran=ran)


def run_project(case, path, guess=False, points=slice(None)):
    ndep = case.coefs.shape[0]
    spline = Spline(len(case.order), ndep, list(case.order), list(case.coefs.shape[1:]), case.knots, case.coefs)
    start = case.args["guess"][:, points] if guess else None
    out = project.project_batch(spline, on_path(case.args["points"][:, points], path), guess=on_path(start, path), _path=pin(path),
                                _chunk=case.args["chunk"])
    ran = list(project.LAST_PATHS)
    if points == slice(None):
        ran = named(ran, path, case.with_kernels({"project_newton"}) if guess else case)
    assert path != "cuda" or all(a.is_cuda for a in out)
    uvw, distance, status, steps = (numpy_of(a) for a in out)
    assert uvw.dtype == np.result_type(*(t.dtype for t in case.knots)) and distance.dtype == np.float64
    return dict(uvw=uvw, distance=distance, status=status, steps=steps, ran=ran)


def run_contours(case, path, split=None, fields=None):
    """trace_batch of the case's levels, or of its fields (B, n0, n1) (or of ``fields``, a slice of either)."""
    levels, coefs = case.args["levels"], case.coefs
    spline = Spline(2, 1, list(case.order), list(coefs.shape[1:]), case.knots, coefs[:1])
    if levels is not None:
        out = contours.trace_batch(spline, levels=levels if fields is None else levels[fields], depth=case.args["depth"], _path=pin(path),
                                   _split=split)
        assert path != "cuda", "levels come with the spline's own NumPy coefficients"
    else:
        out = contours.trace_batch(spline, coefs=on_path(coefs if fields is None else coefs[fields], path), depth=case.args["depth"],
                                   _path=pin(path), _split=split)
        assert path != "cuda" or (out[0].is_cuda and out[5].is_cuda)
    ran = named(contours.LAST_PATHS, path, case) if fields is None else list(contours.LAST_PATHS)
    vertices, offsets, closed, field, cells, status = (numpy_of(a) for a in out)
    assert vertices.dtype == np.result_type(*(t.dtype for t in case.knots))
    return dict(vertices=vertices, offsets=offsets, closed=closed, field=field, cells=cells, status=status, ran=ran)


_REFINED = {}


def refined(case):
    """The case's coarse spline with its knots inserted (host path) and its coefficients perturbed, as (knots, coefs): what
    remove_knots is given.  Cached per case and for its scaled copies formed by scale_ref.cell_scaled from the result."""
    if case.name not in _REFINED:
        ndep = case.coefs.shape[0]
        coarse = Spline(len(case.order), ndep, list(case.order), list(case.coefs.shape[1:]), case.knots, case.coefs)
        fine = coarse.insert_knots(case.args["new"], _path="host")
        noise = np.random.default_rng(case.args["seed"]).standard_normal(fine.coefs.shape)
        coefs = (fine.coefs * (1.0 + case.args["noise"] * noise)).astype(case.coefs.dtype)
        _REFINED[case.name] = cases.CellCase(case.name, case.family, case.order, [np.asarray(t) for t in fine.knots], coefs, case.kernels)
    return _REFINED[case.name]


def run_remove(case, path, tolerance):
    """remove_knots of an already refined case (``refined``)."""
    ndep = case.coefs.shape[0]
    s = Spline(len(case.order), ndep, list(case.order), list(case.coefs.shape[1:]), case.knots, case.coefs)
    r = s.remove_knots(tolerance, _path=path)
    ran = named(reduction.LAST_PATHS, path, case)
    assert r.coefs.dtype == case.coefs.dtype
    return dict(knots=[np.asarray(t) for t in r.knots], coefs=np.asarray(r.coefs), rounds=[list(map(list, v)) for v in reduction.LAST_ROUNDS], ran=ran)


# --------------------------------------------------------------------------------------------- A: the laws
def transforms(case):
    return sr.cell_transforms(case, CC["exponents"], CC["rows"])


def same_keys(got, base, keys, label):
    for key in keys:
        assert np.array_equal(got[key], base[key]), f"{label}: {key} changed"
    assert got["ran"] == base["ran"], f"{label}: {got['ran']} ran, unscaled {base['ran']}"


def check_zeros_law(case, path):
    base = run_zeros(case, path)
    assert len(base["values"]) > 0 and len(base["cells"]) == case.args.get("zero_cells", 0), case.name
    for label, ks, kp in transforms(case):
        got = run_zeros(sr.cell_scaled(case, ks, kp), path)
        label = f"{case.name} on {path} [{label}]"
        same_keys(got, base, ("offsets", "status"), label)
        assert_bits(sr.undo(got["values"], kp), base["values"], f"{label}: the zeros are not x 2^{kp}")
        assert np.array_equal(got["cells"][:, 0], base["cells"][:, 0]), label
        assert_bits(sr.undo(got["cells"][:, 1:], kp), base["cells"][:, 1:], f"{label}: the zero cells")
    return base


def project_transforms(case):
    """Those of the type, and for float64 the edge of the range in which the statement alone keeps the law."""
    return transforms(case) + ([(f"coefficients x 2^{k}", np.array(k), 0) for k in (250, -250)] if case.kind == "fp64" else [])


def check_project_law(case, path, guess, listed=None):
    base = run_project(case, path, guess)
    flagged = (base["status"] & project.STATUS_BOUND) != 0
    assert flagged.any() and not flagged.all() and np.isfinite(base["distance"]).all(), case.name
    for label, ks, kp in project_transforms(case) if listed is None else listed:
        got = run_project(sr.cell_scaled(case, ks, kp), path, guess)
        label = f"{case.name} on {path}, {'guess' if guess else 'seeded'} [{label}]"
        same_keys(got, base, ("status", "steps"), label)
        assert_bits(sr.undo(got["uvw"], kp), base["uvw"], f"{label}: the parameters are not x 2^{kp}")
        assert_bits(sr.undo(got["distance"], int(ks)), base["distance"], f"{label}: the distances are not x 2^{int(ks)}")
    return base


def check_contours_law(case, path):
    depth = case.args["depth"]
    first = None
    for split in range(depth + 1):
        base = run_contours(case, path, split)
        assert len(base["offsets"]) > 3 and len(base["vertices"]) > 50, case.name
        if first is not None:
            same_keys(base, first, ("offsets", "closed", "field", "status", "cells"), f"{case.name}: split {split}")
            assert_bits(base["vertices"], first["vertices"], f"{case.name} on {path}: split level {split} against 0")
        first = first or base
        for label, ks, kp in transforms(case):
            got = run_contours(sr.cell_scaled(case, ks, kp), path, split)
            label = f"{case.name} on {path}, split {split} [{label}]"
            same_keys(got, base, ("offsets", "closed", "field", "status"), label)
            assert_bits(sr.undo(got["vertices"], kp), base["vertices"], f"{label}: the vertices are not x 2^{kp}")
            assert np.array_equal(got["cells"][:, 0], base["cells"][:, 0]), label
            assert_bits(sr.undo(got["cells"][:, 1:], kp), base["cells"][:, 1:], f"{label}: the zero cells")
    return first


def check_remove_law(case, path):
    fine = refined(case)
    removed = []
    for tolerance in CC["tolerances"]:
        base = run_remove(fine, path, tolerance)
        removed.append(sum(len(r) for v in base["rounds"] for r in v))
        for label, ks, kp in transforms(fine):
            got = run_remove(sr.cell_scaled(fine, ks, kp), path, tolerance)
            label = f"{case.name} on {path}, tolerance {tolerance:g} [{label}]"
            assert got["rounds"] == base["rounds"], f"{label}: other knots are removed"
            assert got["ran"] == base["ran"], label
            for iv, (t2, t) in enumerate(zip(got["knots"], base["knots"])):
                assert_bits(sr.undo(t2, kp), t, f"{label}: result knots of variable {iv}")
            assert_bits(sr.undo_law(got["coefs"], ks), base["coefs"], f"{label}: the coefficients are not x 2^{ks.tolist()}")
    assert removed[0] <= removed[1] <= removed[2] and removed[1] > 0, (case.name, removed)
    if case.kind == "fp64":
        assert removed[0] < removed[1] < removed[2], (case.name, removed)      # the tolerances decide differently
    return removed


def absmax_cases():
    """(name, shape, axis, groups, nOut, K, kernel): band_absmax on a middle axis with scalar lanes, band_absmax_line on
    the last one, both over more than one group."""
    return [("rows (3, 37, 29)", (3, 37, 29), 1, 3, 41, 5, "band_absmax"), ("line (3, 29, 37)", (3, 29, 37), 2, 3, 43, 4, "band_absmax_line")]


ABSMAX = {c[0]: c for c in absmax_cases()}


def absmax_inputs(spec, dt):
    name, shape, axis, groups, n_out, K, kernel = spec
    rng = np.random.default_rng(len(name))
    first = np.sort(rng.integers(0, shape[axis] - K + 1, n_out)).astype(np.int32)
    out_shape = list(shape)
    out_shape[axis] = n_out
    return first, rng.standard_normal((n_out, K)), rng.standard_normal(shape).astype(dt), rng.standard_normal(out_shape).astype(dt)


def run_absmax(spec, first, w, data, minus, path):
    """reduction.absmax (device) or absmax_host: (groups, nOut) float64."""
    _, shape, axis, groups, _, _, kernel = spec
    with BandMap(first, w, shape[axis]) as band:
        if path == "host":
            return reduction.absmax_host(band, data, axis, groups, minus)
        import torch
        out = reduction.absmax(band, torch.from_numpy(data).cuda(), axis, groups, None if minus is None else torch.from_numpy(minus).cuda())
        assert reduction.LAST_PATHS == [kernel] and band.last_kernel() == kernel
        return out.cpu().numpy()


def check_absmax_law(spec, path):
    """The lines of group g x 2^ks[g] (and what is subtracted with them): the maxima of group g x 2^ks[g]."""
    groups = spec[3]
    for dt, kind in ((np.float64, "fp64"), (np.float32, "fp32")):
        first, w, data, minus = absmax_inputs(spec, dt)
        r = CC["rows"][kind]
        per_group = np.array(r)[np.arange(groups) % len(r)]
        assert groups == spec[1][0], "a group is an index of the first axis"
        lines = lambda a, ks: sr._p2(a, ks.reshape((-1,) + (1,) * (a.ndim - 1)))
        for m in (None, minus):
            base = run_absmax(spec, first, w, data, m, path)
            assert base.shape == (groups, spec[4]) and np.isfinite(base).all() and (base > 0).all()
            for ks in [np.full(groups, kc) for kc, _ in CC["exponents"][kind]] + [per_group]:
                got = run_absmax(spec, first, w, lines(data, ks), None if m is None else lines(m, ks), path)
                assert_bits(np.ldexp(got, -ks[:, None]), base, f"absmax {spec[0]} {kind} on {path}, groups x 2^{ks.tolist()}")


def check_project_beyond(case, path, guess):
    """Part D: kc = +-300 and +-500, far past where the squares of the statement overflow or vanish: the bits of kc = 0."""
    return check_project_law(case, path, guess, [(f"coefficients x 2^{k}", np.array(k), 0) for k in (300, -300, 500, -500)])


@pytest.mark.parametrize("name", sorted(CELLS_A["zeros2"]) + sorted(CELLS_A["zeros3"]))
def test_zeros_scaling_law_host(name):
    check_zeros_law({**CELLS_A["zeros2"], **CELLS_A["zeros3"]}[name], "host")


@pytest.mark.parametrize("guess", [False, True], ids=["seeded", "guess"])
@pytest.mark.parametrize("name", sorted(CELLS_A["project"]))
def test_project_scaling_law_host(name, guess):
    check_project_law(CELLS_A["project"][name], "host", guess)


@pytest.mark.parametrize("name", sorted(CELLS_A["contours"]))
def test_contours_scaling_law_host(name):
    check_contours_law(CELLS_A["contours"][name], "host")


@pytest.mark.parametrize("name", sorted(CELLS_A["remove_knots"]))
def test_remove_knots_scaling_law_host(name):
    check_remove_law(CELLS_A["remove_knots"][name], "host")


@pytest.mark.parametrize("name", sorted(ABSMAX))
def test_absmax_scaling_law_host(name):
    check_absmax_law(ABSMAX[name], "host")


@pytest.mark.parametrize("guess", [False, True], ids=["seeded", "guess"])
@pytest.mark.parametrize("name", sorted(n for n, c in CELLS_A["project"].items() if c.kind == "fp64"))
def test_project_beyond_the_range_of_its_squares_host(name, guess):
    check_project_beyond(CELLS_A["project"][name], "host", guess)


def test_project_normalisation_is_the_exact_power_of_two():
    assert project.norm_exponent(np.array([[0.5, -0.75]])) == 0 and project.norm_exponent(np.array([1.0])) == 1
    assert project.norm_exponent(np.array([3e300, 1.0])) == 999 and project.norm_exponent(np.array([-2.0 ** -1070])) == -1069
    assert project.norm_exponent(np.zeros(3)) == 0 and project.norm_exponent(np.array([np.inf, 1.0])) == 0
    assert project.norm_exponent(np.array([np.nan, 1.0])) == 0 and project.norm_exponent(np.array([2.5], np.float32)) == 2
    x = np.array([1.5, -3.0, 2.0 ** -600])
    for e, y in [(e, x) for e in (1, -1, 999, -1069)] + [(1024, x * 2.0 ** -100)]:          # 2^1024 itself is no double
        assert sr.same_bits(project._ldexp(y, e), np.ldexp(y, e))


def test_the_cases_are_what_the_laws_need():
    """Every order class of the kernels, candidates past a block of 64, a zero cell, the merge kernels; every kernel of the
    five families declared by a case of part A."""
    for family, n, classes in (("zeros2", 2, {(2, 2), (3, 4), (4, 4)}), ("zeros3", 3, {(2, 2, 2), (3, 3, 2), (4, 4, 4)})):
        listed = CELLS_A[family].values()
        assert {c.order for c in listed} >= classes and any(f"roots{n}_merge" in c.kernels for c in listed)
        assert any(c.args.get("zero_cells") for c in listed) and all(c.coefs.shape[0] == 3 for c in listed)
    assert {(c.order, c.coefs.shape[0]) for c in CELLS_A["project"].values()} >= {((6,), 2), ((2, 3), 3), ((4, 4), 3), ((6,), 3), ((4, 4), 2)}
    for c in CELLS_A["project"].values():
        plan = project.Plan(c.order, c.knots, c.order)
        assert -(-plan.nsamples // c.args["chunk"]) == 3 and c.args["points"].shape[1] == 300
    assert {(c.order, c.args["depth"], c.args["levels"] is None) for c in CELLS_A["contours"].values()} == {((4, 4), 4, False), ((2, 3), 2, True)}
    for family, kernels in cases.CELL_KERNELS.items():
        assert set().union(*(c.kernels for c in CELLS_A[family].values())) == kernels, family
        assert {c.kind for c in CELLS_A[family].values()} == {"fp64", "fp32"}, family
    assert {spec[6] for spec in ABSMAX.values()} == cases.CELL_KERNELS["remove_knots"]


# --------------------------------------------------------------------------------------------- C: locality
def local_system(family, dt=np.float64):
    """One system (or field) on 8 x 8 bicubic cells (zeros3: 4 x 3 x 3 cells of orders (3, 3, 2)) whose coefficients are at
    least 0.05 in size, so that none falls below S_d eps when one of them is x 2^40 (S_d grows with it: 2^40 x 4 eps is
    below 4e-3) and the zero-cell mask stays empty."""
    order, ncells = ((3, 3, 2), (4, 3, 3)) if family == "zeros3" else ((4, 4), (8, 8))
    rng = np.random.default_rng(5000 + len(family))
    knots = cases.cell_knots(rng, order, ncells, dt)
    ncoef = [len(t) - k for t, k in zip(knots, order)]
    lead = (1,) if family == "contours" else (1, len(order))
    raw = rng.standard_normal(lead + tuple(ncoef))
    coefs = (np.sign(raw) * (0.05 + np.abs(raw))).astype(dt)
    n = len(order)
    kernels = {"contours": {"contour_flag", "contour_march"}}.get(family, {f"roots{n}_flag", f"roots{n}_isolate"})
    # a zero next to a cell edge makes the merge kernel run, with one coefficient and not with another
    args = dict(levels=None, depth=2) if family == "contours" else dict(optional={f"roots{n}_merge"})
    return cases.CellCase(f"{family} locality {order}", family, order, knots, coefs, kernels, **args)


def windows(case, index):
    """Per axis the bool array over the cells: the B-spline window of the cell holds coefficient index[axis]."""
    plan = roots2.Plan2(case.order, case.knots) if len(case.order) == 2 else roots3.Plan3(case.order, case.knots)
    return plan, [(p.cell - k + 1 <= i) & (i <= p.cell) for p, k, i in zip(plan.axes, case.order, index)]


def clean_points(points, plan, hit):
    """The rows of ``points`` (n, nInd) none of whose cells - every cell whose closed box holds the point - has the
    multiplied coefficient in its window: on some axis no span that holds the coordinate is hit."""
    clean = np.zeros(len(points), bool)
    for a, (b, h) in enumerate(zip(plan.breaks, hit)):
        b = np.asarray(b, np.float64)
        u = points[:, a].astype(np.float64)[:, None]
        holds = (b[None, :-1] <= u) & (u <= b[None, 1:])
        clean |= ~(holds & h[None, :]).any(axis=1)
    return points[clean]


def rows_of(points):
    return sorted({row.tobytes() for row in points})


def check_cell_locality(family, path, index=None):
    case = local_system(family)
    run = (lambda c: run_contours(c, path)) if family == "contours" else (lambda c: run_zeros(c, path))
    key = "vertices" if family == "contours" else "values"
    base = run(case)
    n = len(case.order)
    at = (0,) * (case.coefs.ndim - n) + ((1,) * n if index is None else tuple(index))
    plan, hit = windows(case, at[-n:])
    touched = np.ones((), bool)
    for a, h in enumerate(hit):
        touched = touched & h.reshape([-1 if b == a else 1 for b in range(n)])
    assert 0 < touched.sum() < touched.size and len(base["cells"]) == 0
    want = rows_of(clean_points(base[key], plan, hit))
    assert len(want) >= (10 if family != "zeros3" else 1), (family, len(want))
    for power in LOCAL_POWERS:
        coefs = sr.multiplied(case.coefs, at, power)
        top = np.abs(coefs.astype(np.float64)).max()
        assert np.abs(coefs).min() >= top * EPS * 4 and top == abs(float(coefs[at])), "no coefficient may fall below S_d eps"
        got = run(case.replaced(coefs=coefs))
        assert len(got["cells"]) == 0
        assert rows_of(clean_points(got[key], plan, hit)) == want, (f"{case.name} on {path}: coefficient {at} x 2^{power} moves zeros or "
                                                                   f"vertices of cells whose window does not hold it")
        assert np.array_equal(got["status"][0][~touched], base["status"][0][~touched]), f"{case.name} on {path}: status bytes, x 2^{power}"
        assert rows_of(got[key]) != rows_of(base[key]), "the multiplied coefficient reaches nothing"
    return base


LOCAL_FAMILIES = ["zeros2", "zeros3", "contours"]


@pytest.mark.parametrize("family", LOCAL_FAMILIES)
def test_cell_locality_host(family):
    check_cell_locality(family, "host")


def check_absmax_locality(spec, path):
    """One element of the data x 2^20 and x 2^40: the maxima of the other groups, and of the rows of its own group whose
    window does not hold it, keep their bits; a group's lines alone give the group's maxima."""
    name, shape, axis, groups, n_out, K, _ = spec
    first, w, data, minus = absmax_inputs(spec, np.float64)
    base = run_absmax(spec, first, w, data, minus, path)
    for spot in ((0,) * len(shape), tuple(s - 1 for s in shape), tuple(s // 2 for s in shape)):
        touched = np.zeros((groups, n_out), bool)
        touched[spot[0], :] = (first <= spot[axis]) & (spot[axis] < first + K)
        assert touched.any() and not touched.all()
        for power in LOCAL_POWERS:
            got = run_absmax(spec, first, w, sr.multiplied(data, spot, power), minus, path)
            assert np.array_equal(got[~touched], base[~touched]), f"absmax {name} on {path}: element {spot} x 2^{power} moves maxima it has no weight on"
            assert (got[touched] != base[touched]).any()
    for g in range(groups):
        alone = run_absmax((name, (1,) + shape[1:], axis, 1, n_out, K, spec[6]), first, w, data[g:g + 1], minus[g:g + 1], path)
        assert np.array_equal(alone[0], base[g]), f"absmax {name} on {path}: group {g} alone"


@pytest.mark.parametrize("name", sorted(ABSMAX))
def test_absmax_locality_host(name):
    check_absmax_locality(ABSMAX[name], "host")


def independence_cases():
    """The part A cases whose batch is taken apart: the planted systems (the merge kernels run), a float64 project surface
    and curve, both contour cases (levels, and fields of their own)."""
    out = [c for f in ("zeros2", "zeros3") for c in CELLS_A[f].values() if "planted" in c.name and c.kind == "fp64"]
    out += [c for f in ("zeros2", "zeros3") for c in CELLS_A[f].values() if "zero cell" in c.name and c.kind == "fp64"]
    out += [c for c in CELLS_A["project"].values() if c.kind == "fp64" and c.order != (2, 3)]
    return out + [c for c in CELLS_A["contours"].values() if c.kind == "fp64"]


INDEPENDENT = {c.name: c for c in independence_cases()}


def check_independence(case, path):
    """A system, a field, a level or a slice of the points alone: the bits it has in the batch."""
    if case.family in ("zeros2", "zeros3"):
        whole = run_zeros(case, path)
        for b in range(len(case.coefs)):
            alone = run_zeros(case, path, systems=slice(b, b + 1))
            assert_bits(alone["values"], whole["values"][whole["offsets"][b]:whole["offsets"][b + 1]], f"{case.name} on {path}: system {b} alone")
            assert np.array_equal(alone["status"][0], whole["status"][b]) and (b > 0 or alone["ran"] == whole["ran"])
            assert np.array_equal(alone["cells"][:, 1:], whole["cells"][whole["cells"][:, 0] == b][:, 1:])
    elif case.family == "project":
        for guess in (False, True):
            whole = run_project(case, path, guess)
            for part in (slice(0, 1), slice(63, 129), slice(130, 300)):
                alone = run_project(case, path, guess, part)
                for key in ("uvw", "distance", "status", "steps"):
                    assert_bits(alone[key], whole[key][..., part], f"{case.name} on {path}: points {part} alone, {key}")
    else:
        whole = run_contours(case, path)
        count = len(case.coefs) if case.args["levels"] is None else len(case.args["levels"])
        for b in range(count):
            alone = run_contours(case, path, fields=slice(b, b + 1))
            mine = np.flatnonzero(whole["field"] == b)
            assert len(mine) == len(alone["field"]) and np.array_equal(alone["closed"], whole["closed"][mine])
            lo, hi = whole["offsets"][mine[0]], whole["offsets"][mine[-1] + 1]
            assert np.array_equal(alone["offsets"], whole["offsets"][mine[0]:mine[-1] + 2] - lo)
            assert_bits(alone["vertices"], whole["vertices"][lo:hi], f"{case.name} on {path}: field {b} alone")
            assert np.array_equal(alone["status"][0], whole["status"][b])


@pytest.mark.parametrize("name", sorted(INDEPENDENT))
def test_batch_independence_host(name):
    check_independence(INDEPENDENT[name], "host")


def test_part_c_declares_every_kernel():
    declared = set().union(*(c.kernels for c in INDEPENDENT.values())) | {spec[6] for spec in ABSMAX.values()}
    declared |= set().union(*(local_system(f).kernels for f in LOCAL_FAMILIES))
    assert declared == ALL_KERNELS



# =============================================================================================================
# B. Shifted and stretched domains against the exact references.  tests/golden/cell_scale.npz (made by
#    tests/golden/make_golden_cell_scale.py) holds systems of the families' own goldens moved to every domain of
#    cases.SCALE_DOMAINS (float32 knots: SCALE_DOMAINS_F32), with what zeros2_ref, zeros3_ref, project_ref and contours_ref
#    say is exactly true of the stored shifted values, in each family's own key layout.  So the families' own checks run
#    unchanged, with their own derived bars (which carry 4 eps max |domain end| / h, and one float32 spacing of the largest
#    domain end for float32 knots): test_roots2_host.check_golden, test_roots3_host.check_golden,
#    test_project_host.check_golden, the two golden tests of test_contours_host.py, and check_recovered / check_reduced of
#    test_remove_host.py (remove_ref certifies the error of the result in the test itself).  Counts, zero cells, status,
#    step counts and polyline structure equal the exact ones; every path of ``paths`` returns the bits of the first one.
#    remove_knots has no float32 case here: the suite has no bar for a float32 recovery, and part B adds none.
# =============================================================================================================
import contextlib
import os

import test_contours_host as tch
import test_project_host as tph
import test_remove_host as trm
import test_roots2_host as t2h
import test_roots3_host as t3h
from conftest import GOLDEN, observe

CELL_GOLD = np.load(os.path.join(GOLDEN, "cell_scale.npz"))
BANDS = {"band_apply", "band_apply_line"}


class Golden:
    """The entries of cell_scale.npz of one family, the family's prefix taken off: indexed like the family's own file."""

    def __init__(self, family):
        self.prefix = family + ":"
        self.files = [key[len(self.prefix):] for key in CELL_GOLD.files if key.startswith(self.prefix)]

    def __getitem__(self, key):
        return CELL_GOLD[self.prefix + key]


@contextlib.contextmanager
def golden_in(module, attribute, family):
    """The family's test module reads its goldens from a global: for the time of a check, that is the family's part of
    cell_scale.npz."""
    own = getattr(module, attribute)
    setattr(module, attribute, Golden(family))
    try:
        yield
    finally:
        setattr(module, attribute, own)


class ShiftedCase:
    def __init__(self, family, name, kernels):
        self.family, self.name, self.base, self.kernels = family, name, name.split("@")[0], set(kernels)


def shifted_kernels(family, base):
    """The family's kernels a moved system must run (asserted on every path)."""
    if family in ("zeros2", "zeros3"):
        n = family[-1]
        return {f"roots{n}_flag", f"roots{n}_isolate"} | ({f"roots{n}_merge"} if base.startswith("sep_knots") else set())
    if family == "remove":
        return {"band_absmax_line"} | ({"band_absmax"} if "surface" in base else set())
    return cases.CELL_KERNELS[family]


def shifted_cases():
    return [ShiftedCase(family, str(name), shifted_kernels(family, str(name).split("@")[0]))
            for family in ("zeros2", "zeros3", "project", "contours", "remove") for name in Golden(family)["names"]]


SHIFTED = {f"{c.family} {c.name}": c for c in shifted_cases()}


def launches(ran):
    """What ran without the band kernels of the extraction, under the device's names."""
    names = [p[len("host "):] if p.startswith("host ") else p for p in ran]
    return [p for p in names if p not in BANDS and p != "roots_extract"]


def check_launches(case, ran, paths):
    for path in paths:
        assert all(p.startswith("host ") for p in ran[path]) if path == "host" else not any(p.startswith("host ") for p in ran[path])
    if case.family == "remove":         # the host's data reduction has one name for both kernels and one for the band kernels
        assert len({len(ran[path]) for path in paths}) == 1, (case.name, ran)
        assert all(set(ran[path]) & ALL_KERNELS == case.kernels for path in paths if path != "host"), (case.name, ran)
        return
    first = launches(ran[paths[0]])
    assert all(launches(ran[path]) == first for path in paths), (case.name, ran)
    assert {p.split()[0] for p in first} & ALL_KERNELS == case.kernels, (case.name, first)


def check_shifted(case, paths):
    """One moved system on every path of ``paths``: the family's own check against the exact answer, the kernels that ran,
    and the bits of the first path on every other one."""
    label = f"scale cells B, {case.family} on"
    ran, bits = {}, {}
    if case.family in ("zeros2", "zeros3"):
        t, mod, call = (t2h, roots2, "zeros2") if case.family == "zeros2" else (t3h, roots3, "zeros3")
        with golden_in(t, "_GOLDEN", case.family):
            c = t.load_case(case.name)
        for path in paths:
            found = getattr(t.make_spline(c), call)(_path=path)
            ran[path] = list(mod.LAST_PATHS)
            t.check_golden(c, found, f"{label} {path}:")
            bits[path] = t.bits(found)
    elif case.family == "project":
        with golden_in(tph, "DATA", "project"):
            c = tph.load_case(case.name)
            spline = tph.make_spline(c)
            for path in paths:
                got = project.project_batch(spline, c["points"], samples=c["samples"], _path=path)
                ran[path] = list(project.LAST_PATHS)
                tph.check_golden(case.name, got[0], got[1], got[2], f"({label} {path})")
                assert got[3].tolist() == c["steps"].tolist(), f"{case.name} on {path}: other step counts than the statement's"
                bits[path] = [a.tobytes() for a in got]
    elif case.family == "contours":
        with golden_in(tch, "GOLD", "contours"):
            tch.test_keys_and_segments_equal_the_oracle(case.name)           # the host drivers and the public host call
            tch.test_vertices_within_the_derived_bar(case.name)
            s = tch.spline_of(case.name)
            level, depth = float(tch.GOLD[f"{case.name}/level"]), int(tch.GOLD[f"{case.name}/depth"])
        for path in ["host"] + [p for p in paths if p != "host"]:          # the checks above are the host's: every path has its bits
            out = contours.trace_batch(s, levels=None if level == 0.0 else [level], depth=depth, _path=path)
            ran[path] = list(contours.LAST_PATHS)
            bits[path] = [numpy_of(a).tobytes() for a in out]
        paths = ["host"] + [p for p in paths if p != "host"]
    else:
        g, p = Golden("remove"), case.name + "/"
        recover = case.base.startswith("recover")
        s = trm.spline_of(g, p, "in_knots", "in_coefs") if recover else trm.spline_of(g, p)
        tolerance = 1e-12 if recover else float(g[p + "tolerance"])
        for path in paths:
            r = s.remove_knots(tolerance, _path=path)
            ran[path] = list(reduction.LAST_PATHS)
            trm.check_rounds(s.order)
            if recover:
                err = trm.check_recovered(r, [g[f"{p}knots{iv}"] for iv in range(s.nInd)], g[p + "coefs"])
                observe(f"{label} {path}: recovery of inserted knots, coefficients", err, 1e-12)
                assert tuple(g[p + "ref_ncoef"]) == r.nCoef
            else:
                ratio = trm.check_reduced(s, r, tolerance, g[p + "ref_ncoef"])
                observe(f"{label} {path}: exact certified error / bound", ratio, 1.0)
            bits[path] = [r.coefs.tobytes()] + [t.tobytes() for t in r.knots] + [repr(reduction.LAST_ROUNDS)]
    check_launches(case, ran, paths)
    for path in paths[1:]:
        assert bits[path] == bits[paths[0]], f"{case.name}: {path} and {paths[0]} return different bits"


@pytest.mark.parametrize("name", sorted(SHIFTED))
def test_shifted_domain_host(name):
    check_shifted(SHIFTED[name], ["host"])


def test_part_b_moves_every_family_to_every_domain():
    ids = lambda doms: {f"{lo:g}+{w:g}" for lo, w in doms}
    for family in ("zeros2", "zeros3", "project", "contours", "remove"):
        listed = [c for c in SHIFTED.values() if c.family == family]
        per_base = {}
        for c in listed:
            per_base.setdefault(c.base, set()).add(c.name.split("@")[1])
        assert ids(CC["domains"]) in per_base.values(), family
        assert family == "remove" or ids(CC["domains_f32"]) in per_base.values(), family
        assert all(d in (ids(CC["domains"]), ids(CC["domains_f32"])) for d in per_base.values()), (family, per_base)
        assert set().union(*(c.kernels for c in listed)) == cases.CELL_KERNELS["remove_knots" if family == "remove" else family]
    assert os.path.getsize(os.path.join(GOLDEN, "cell_scale.npz")) < 1 << 20
