"""
What the cell families (``roots``, ``roots2``, ``roots3``, ``project``, ``contours``, ``isosurface``, ``mesh``, ``rays``, ``surfaces``) share, written
once: the host band loop, the per-axis Bezier plan (``JumpFreePlan``: the one of ``contours``, ``isosurface``, ``mesh`` and ``surfaces``, which refuses
a jump), the zero-cell table, and ``zeros2_batch`` / ``zeros3_batch`` whole, on the two backends of bspy_amd/_backend.py
(``Host``, ``Device``, the path switch: passed on under their names here).  The layer that ``rays`` and ``surfaces`` put on
top, one surface's tables and the passes of the pair search, is written once in bspy_amd/_pairs.py.

A driver is a function of a backend: it allocates with ``be.empty``, hands ``be.ptr(a)`` to ``be.call(name, ...)`` and uses
the backend's few array operations.  The families differ in their kernels and in the plain-Python statement that says what a
kernel computes.  ``project`` and ``contours`` keep their statements; the one of ``roots2`` and ``roots3``, the box walk that
``rays`` and ``surfaces`` stand on too, is written once for any number of variables in bspy_amd/_box.py, and the two modules
keep their Newton leaves.  ``zeros_batch`` (the checks and the path), ``tables``, ``isolate_cells`` (flag, isolate, merge),
``collect`` and ``zeros`` (the ``Spline.zerosN`` wrapper) are ``zeros2_batch`` and ``zeros3_batch``: each takes the family's
module, which supplies the number of variables, the entry-point prefix, the slots, the order checks and the path knobs.

The front of a call that takes a coefficient net is here too, once for every family that has one: ``coefs_arg`` (what a
``coefs`` argument may be, and the path it pins: all of ``roots``, ``zeros2`` / ``zeros3``, ``contours``, ``isosurface`` and
``mesh``), ``bezier_rows`` (upload, widen to float64, extract: everyone but ``roots``, which keeps float32 rows),
``field_scale`` and ``zero_table``.  ``level_batch`` (the checks, the path by leaf count, the tables, the run and the
zero-cell table), ``level_tables``, ``depth_of`` and ``split_of`` are ``contours.trace_batch`` and
``isosurface.extract_batch`` up to their tails, for any number of axes: each takes the family's module as ``zeros_batch``
does.  ``weld`` turns the key triples of ``isosurface`` and ``mesh`` into indexed triangles, member by member.
"""
import math

import numpy as np

from . import _native as nv
from . import refinement
from ._backend import Device, Host, is_torch, pick_path          # the cell families and the tools take them from here

EPS = float(np.finfo(np.float64).eps)


def band_host(data, steps, log):
    """NumPy (M, ...) float64 through band steps [(axis, first, w)] in the order the device path takes them, each summed as
    the band kernels sum it (``bsk_roots_extract_host`` on the lines of that axis); ``log`` receives one entry per step."""
    L = nv.lib()
    for axis, first, w in refinement._ordered(steps, data.shape):
        first, w = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(w, np.float64)
        lines = np.ascontiguousarray(np.moveaxis(data, axis, -1))
        out = np.empty(lines.shape[:-1] + (len(first),), np.float64)
        nv.check(L.bsk_roots_extract_host(w.shape[1], lines.shape[-1], len(first), first.ctypes.data, w.ctypes.data,
                                          lines.ctypes.data, lines.size // lines.shape[-1], out.ctypes.data))
        log.append(L.bsk_roots_last_kernel().decode())
        data = np.ascontiguousarray(np.moveaxis(out, -1, axis))
    return data


# ------------------------------------------------------------------------------------------ the coefficient argument
def coefs_arg(name, coefs, path, tail, text):
    """What ``name`` (the caller, for the messages) takes as ``coefs``: a float32 / float64 torch CUDA tensor, which pins
    the device path, or anything NumPy makes an array of; ``tail`` is the shape behind the batch axis (an int per axis, or
    a range of them) and ``text`` says it.  -> (coefs, on_device, path)."""
    on_device = is_torch(coefs)
    if on_device:
        import torch
        if not coefs.is_cuda or coefs.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{name} takes the coefficients as a float32 or float64 torch CUDA tensor")
        if path == "host":
            raise ValueError("coefficients on the device take the device path")
        path = "device"
    else:
        coefs = np.asarray(coefs)
    if coefs.ndim != len(tail) + 1 or not all(m in (want if isinstance(want, range) else (want,)) for m, want in zip(coefs.shape[1:], tail)):
        raise ValueError(f"coefs must have the shape {text}")
    return coefs, on_device, path


def backend_of(coefs):
    """Where the result of a call lives that computes nothing (B == 0): with its coefficients."""
    return Device(coefs.device) if is_torch(coefs) else Host()


def to_host(be, res):
    """A driver's dict of results with the backend's arrays brought to the host."""
    return {name: be.get(a) if is_torch(a) else a for name, a in res.items()}


def bezier_rows(coefs, path, plan, log, finite=None):
    """coefs (..., *nCoef), NumPy or a torch CUDA tensor of any strides, on the backend of ``path`` -> (be, data, rows):
    data = coefs in float64 (float32 is widened BEFORE the extraction; a float64 CUDA tensor is not copied) and rows =
    data through ``plan.steps``, the backend's contiguous array (..., *rowlen); ``log`` receives what ran.  ``finite``: the
    caller's name, which refuses coefficients that are not finite."""
    if path == "device":
        import torch
        data = (coefs if is_torch(coefs) else torch.from_numpy(np.ascontiguousarray(coefs)).cuda()).double()
        be, ok = Device(data.device), finite is None or bool(torch.isfinite(data).all())
    else:
        data = np.asarray(coefs).astype(np.float64)
        be, ok = Host(), finite is None or np.isfinite(data).all()
    if not ok:
        raise ValueError(f"{finite}: the coefficients must be finite")
    rows = data
    if plan.steps:
        rows = data.reshape((-1,) + tuple(data.shape[-plan.nind:]))
        if path == "device":
            rows, ran = refinement.run_device(rows, plan.steps)
            log.extend(ran)
        else:
            rows = band_host(rows, plan.steps, log)
        rows = rows.reshape(tuple(data.shape[:-plan.nind]) + tuple(plan.rowlen))
    return be, data, (rows.contiguous() if path == "device" else np.ascontiguousarray(rows))


def field_scale(be, data, levels=None):
    """S of every field, float64 (B): max |coefficient| of data (B, ...), or max |coefficient of field 0 - levels[b]|."""
    fields = data if levels is None else data[0][None] - levels[(slice(None),) + (None,) * (data.ndim - 1)]
    return be.amax(abs(fields), tuple(range(1, data.ndim)))


# ------------------------------------------------------------------------------------------ plans and tables
class BezierPlan:
    """Bezier extraction of one variable: ``steps`` (band steps on axis 1; empty when the knots are in Bezier form
    already), ``breaks`` (the distinct knots of the domain, in the knots' dtype), ``first`` (where span s starts in the
    extracted row), ``rowlen``, and ``cell`` (the knot cell of span s in the spline's own knots)."""

    def __init__(self, order, knots):
        k, t = int(order), knots
        n = len(t) - k
        lo, hi = t[k - 1], t[n]
        # merged knots as refinement.merged_knots forms them (new knots behind old ones of the same value), vectorised:
        # every distinct knot of the domain is raised to K - 1, the two ends to K
        values, counts = np.unique(t, return_counts=True)
        want = np.where((values == lo) | (values == hi), k, np.maximum(k - 1, counts))
        add = np.where((values >= lo) & (values <= hi), want - counts, 0)
        merged, origin = t, np.arange(len(t))
        if add.any():
            both = np.concatenate((t, np.repeat(values, add)))
            rank = np.argsort(both, kind="stable")
            merged, origin = both[rank], np.where(rank < len(t), rank, -1)
        row0 = int(np.searchsorted(merged, lo))
        row1 = int(np.searchsorted(merged, hi))
        self.steps = []
        if merged is not t or (row0, row1) != (0, n):
            self.steps = [(1, *refinement.refine_map(t, k, merged, 0, rows=slice(row0, row1), origin=origin))]
        bezier = merged[row0:row1 + k]
        self.order = k
        self.breaks = np.unique(bezier)
        self.nspans = len(self.breaks) - 1
        self.first = (np.searchsorted(bezier, self.breaks[:-1], "right") - k).astype(np.int32)
        self.rowlen = len(bezier) - k
        self.cell = np.clip(np.searchsorted(t, self.breaks[:-1], "right") - 1, k - 1, n - 1)
        self.margin = math.sqrt(EPS) * (float(hi) - float(lo))


class TensorPlan:
    """Bezier extraction of every variable: one ``BezierPlan`` per axis and the band steps on the axes 1 .. nInd of a
    tensor (M, *nCoef)."""

    def __init__(self, order, knots):
        self.nind = len(order)
        self.axes = [BezierPlan(order[d], knots[d]) for d in range(self.nind)]
        self.order = tuple(int(k) for k in order)
        self.steps = [(d + 1, first, w) for d in range(self.nind) for _, first, w in self.axes[d].steps]
        self.breaks = [p.breaks for p in self.axes]
        self.first = [p.first for p in self.axes]
        self.rowlen = [p.rowlen for p in self.axes]
        self.ncells = [p.nspans for p in self.axes]


class JumpFreePlan(TensorPlan):
    """``TensorPlan`` that refuses a jump: an interior knot of multiplicity >= K.  A subclass sets ``who``,
    the caller's name, and ``what``, the thing that cannot cross the knot (``contours``: a contour; ``surfaces``: a curve; ``isosurface``: a surface; ``mesh``: a mesh)."""
    who = what = None

    def __init__(self, order, knots):
        for d in range(len(order)):
            k, t = int(order[d]), np.asarray(knots[d])
            values, counts = np.unique(t, return_counts=True)
            inside = (values > t[k - 1]) & (values < t[len(t) - k]) & (counts >= k)
            if inside.any():
                raise ValueError(f"{self.who}: the knot {float(values[inside][0])} of variable {d} has multiplicity {int(counts[inside][0])}"
                                 f" >= order {k} (a jump: no {self.what} crosses it; trim the spline there)")
        super().__init__(order, knots)


def zero_cells(small, plan):
    """small: bool (B, nDep, *nCoef), |coefficient| < S_d eps.  -> bool (B, *ncells): all K0 x ... coefficients of the cell
    are small, for any component."""
    total = small.astype(np.int64)
    for a, K in enumerate(plan.order):                                   # windowed sums, one axis at a time
        run = np.concatenate((np.zeros_like(np.take(total, [0], axis=a + 2)), np.cumsum(total, axis=a + 2)), axis=a + 2)
        hi = plan.axes[a].cell + 1
        total = np.take(run, hi, axis=a + 2) - np.take(run, hi - K, axis=a + 2)
    return (total == int(np.prod(plan.order))).any(axis=1)


def zero_table(zero, plan):
    """zero: NumPy (B, *ncells), nonzero on a zero cell.  -> float64 (k, 2 nInd + 1): one row (member, u0, u1, v0, v1, ...)
    per zero cell, in index order."""
    at = np.argwhere(zero)
    cols = [at[:, 0].astype(np.float64)]
    for a, b in enumerate(plan.breaks):
        b = np.asarray(b, np.float64)
        cols += [b[at[:, a + 1]], b[at[:, a + 1] + 1]]
    return np.stack(cols, axis=1).reshape(-1, 2 * plan.nind + 1)


def system_tables(be, data, plan):
    """data: the backend's float64 (B, n, *nCoef).  -> (mask NumPy uint8 (B, *ncells), the zero cells; scale (B, n), the
    backend's, max |coefficient| of every component).  One byte per coefficient is read back on the device."""
    n = plan.nind
    wide = abs(data)
    scale = be.amax(wide, tuple(range(2, n + 2)))
    each = (...,) + (None,) * n
    small = be.get((wide < (scale * EPS)[each]) | (scale == 0.0)[each])
    return zero_cells(small, plan).astype(np.uint8), scale


# ------------------------------------------------------------------------------------------ the drivers of zeros2 and zeros3
def isolate_cells(be, prefix, rows, plan, mask, scale, R, log):
    """Flag the cells, isolate the zeros of the candidates, merge the ones near a cell boundary: the entry points
    ``prefix`` + ``_flag``, ``_isolate``, ``_merge`` for a plan of any number of axes n.  rows: float64 in Bezier form,
    the backend's contiguous array; mask: NumPy (B, *ncells); scale: float64 (B, n), the backend's; R: the slots per cell.
    -> dict of flags, cand, roots (ncand, R, n), near, count, status, nodes, keep, the backend's arrays; ``log`` receives
    what ran.  No candidates: the last two launches are skipped; no zero near a boundary: the last one is."""
    last = getattr(nv.lib(), prefix + "_last_kernel")

    def run(name, *args):
        be.call(prefix + name, *args)
        log.append(last().decode())

    B = mask.shape[0]
    if int(np.prod(rows.shape)) != B * plan.nind * int(np.prod(plan.rowlen)):
        raise ValueError(f"the rows must hold {plan.nind} components per system of the mask")
    with be:
        first = [be.put(f, np.int32) for f in plan.first]
        grid = plan.order + (be.ptr(rows), B) + tuple(plan.rowlen) + tuple(plan.ncells) + tuple(be.ptr(f) for f in first)
        mask = be.put(mask, np.uint8)
        flags = be.empty(mask.shape, np.uint8)
        run("_flag", *grid, be.ptr(mask), be.ptr(flags))
        cand = be.nonzero(flags)
        n = len(cand)
        out = dict(flags=flags, cand=cand, roots=be.empty((n, R, plan.nind), np.float64), near=be.empty((n, R), np.uint8),
                   count=be.empty(n, np.int32), status=be.empty(n, np.uint8), nodes=be.empty(n, np.int32))
        if n:
            breaks = [be.put(b, np.float64) for b in plan.breaks]
            run("_isolate", *grid, *map(be.ptr, breaks), be.ptr(scale), be.ptr(cand), n, be.ptr(out["roots"]), be.ptr(out["near"]),
                be.ptr(out["count"]), be.ptr(out["status"]), be.ptr(out["nodes"]))
        keep = be.cast(~be.isnan(out["roots"][:, :, 0]), np.uint8)
        which = be.nonzero(out["near"])
        if len(which):
            table = be.cumsum(flags.reshape(-1)) - 1
            run("_merge", R, be.ptr(out["roots"]), B, *plan.ncells, *map(be.ptr, breaks), be.ptr(cand), n, be.ptr(flags), be.ptr(table),
                be.ptr(which), len(which), be.ptr(keep))
        out["keep"] = keep
    return out


def collect(be, plan, kdtype, B, R=0, res=None, mask=None, numpy_out=True):
    """The result of ``zeros2_batch`` / ``zeros3_batch`` from what ``isolate_cells`` returned: (values, offsets, cells,
    status).  The kept zeros sorted by (system, u, v, ...) and rounded to ``kdtype``, where each system starts, one row
    (system, u0, u1, v0, v1, ...) per zero cell of ``mask`` and the status bits per cell; ``numpy_out`` brings the backend's
    arrays to the host.  B == 0: the empty result."""
    n, nc = plan.nind, tuple(plan.ncells)
    if B == 0:
        return be.empty((0, n), kdtype), be.zeros(1, np.int64), np.empty((0, 2 * n + 1)), be.zeros((0,) + nc, np.uint8)
    ncell = int(np.prod(nc))
    kept = be.cast(res["keep"].reshape(-1), bool)
    system = be.repeat(res["cand"] // ncell, R)[kept]
    values = res["roots"].reshape(-1, n)[kept]
    order = be.lexsort([values[:, a] for a in reversed(range(n))] + [system])
    values = be.cast(values[order], kdtype)
    offsets = be.searchsorted(system[order], B + 1)
    status = be.zeros(B * ncell, np.uint8)
    status[res["cand"]] = res["status"]
    status = status.reshape((B,) + nc)
    if numpy_out:
        values, offsets, status = be.get(values), be.get(offsets), be.get(status)
    return values, offsets, zero_table(mask, plan), status


def run_host(family, rows, plan, mask, scale):
    """``isolate_cells`` on the host: rows NumPy float64 (B, n, R0, ...) in Bezier form, mask uint8 (B, *ncells), scale
    float64 (B, n)."""
    rows, scale = np.ascontiguousarray(rows, np.float64), np.ascontiguousarray(scale, np.float64)
    return isolate_cells(Host(), family.PREFIX, rows, plan, mask, scale, family.slots(*plan.order), family.LAST_PATHS)


def tables(family, spline, coefs=None):
    """The host path's tables of a system: (plan, rows (B, n, R0, ...), mask (B, *ncells), scale (B, n)), all NumPy."""
    n = family.NIND
    plan = TensorPlan(spline.order, spline.knots)
    data = np.asarray(spline.coefs if coefs is None else coefs)
    be, data, rows = bezier_rows(data.reshape((-1, n) + data.shape[-n:]), "host", plan, family.LAST_PATHS)
    return (plan, rows) + system_tables(be, data, plan)


def zeros_batch(family, spline, coefs, _path):
    """``zeros2_batch`` and ``zeros3_batch``.  ``family``, the module, supplies NIND, WORD, PREFIX, ``_check_spline``,
    ``slots``, the orders the kernels cover (DEVICE_MIN_K, DEVICE_MAX_K), DEVICE_MIN_CELLS, FORCE_PATH and LAST_PATHS."""
    n, name = family.NIND, f"zeros{family.NIND}_batch"
    del family.LAST_PATHS[:]
    path = pick_path(_path, family.FORCE_PATH)
    family._check_spline(spline)
    K = tuple(int(k) for k in spline.order)
    ncoef = tuple(len(spline.knots[d]) - spline.order[d] for d in range(n))
    if coefs is None:
        if spline.nDep != n:
            raise ValueError(f"{name} takes {family.WORD} dependent variables, or coefs (B, {n}, {', '.join(f'n{d}' for d in range(n))})")
        coefs = spline.coefs[None]
    coefs, on_device, path = coefs_arg(name, coefs, path, (n,) + ncoef, f"(B, {n}, {', '.join(str(m) for m in ncoef)})")
    B = int(coefs.shape[0])
    plan = TensorPlan(spline.order, spline.knots)
    kdtype = np.result_type(*(spline.knots[d].dtype for d in range(n)))
    covered = family.DEVICE_MIN_K <= min(K) and max(K) <= family.DEVICE_MAX_K
    if path is None:
        path = "device" if covered and B * int(np.prod(plan.ncells)) >= family.DEVICE_MIN_CELLS else "host"
    if path == "device" and not covered:
        raise ValueError(f"the device path covers orders from {family.DEVICE_MIN_K} to {family.DEVICE_MAX_K}")

    if B == 0:
        return collect(backend_of(coefs), plan, kdtype, 0)
    be, data, rows = bezier_rows(coefs, path, plan, family.LAST_PATHS)
    mask, scale = system_tables(be, data, plan)
    res = isolate_cells(be, family.PREFIX, rows, plan, mask, scale, family.slots(*K), family.LAST_PATHS)
    return collect(be, plan, kdtype, B, family.slots(*K), res, mask, numpy_out=not on_device)


def zeros(family, spline, _path):
    """``Spline.zeros2`` and ``Spline.zeros3``: the zeros and the zero cells of one system in one list, sorted by (u, v,
    ...); a status bit of any cell raises ValueError."""
    n = family.NIND
    if not (spline.nInd == spline.nDep):
        raise ValueError("The number of independent variables (nInd) must match the number of dependent variables (nDep).")
    family._check_spline(spline)
    values, _, cells, status = zeros_batch(family, spline, None, _path)
    if status.any():
        at = tuple(int(x) for x in np.argwhere(status)[0])
        bits = int(status[at])
        breaks = TensorPlan(spline.order, spline.knots).breaks
        why = ", ".join(text for bit, text in family.STATUS_TEXT.items() if bits & bit)
        box = " x ".join(f"[{float(b[i])}, {float(b[i + 1])}]" for b, i in zip(breaks, at[1:]))
        raise ValueError(f"zeros{n}: {why} in the cell {box}")
    found = [(tuple(float(x) for x in r), r) for r in values]
    for row in cells.astype(values.dtype):
        lo, hi = tuple(row[1::2]), tuple(row[2::2])
        found.append((tuple(float(x) for x in lo), (lo, hi)))
    found.sort(key=lambda item: item[0])
    return [item[1] for item in found]


# ------------------------------------------------------------------------------------------ the drivers of contours and isosurface
def depth_of(family, tolerance, plan):
    """The depth that ``tolerance`` asks for (the family's statement says why): DEFAULT_DEPTH without one, at most MAX_DEPTH."""
    if tolerance is None:
        return family.DEFAULT_DEPTH
    if not tolerance > 0.0:
        raise ValueError("tolerance must be positive")
    breaks = [np.asarray(b, np.float64) for b in plan.breaks]
    h = max(float(np.diff(b).max()) for b in breaks)
    L = max(float(b[-1] - b[0]) for b in breaks)
    for d in range(family.MAX_DEPTH + 1):
        if (h * 2.0 ** -d) ** 2 <= tolerance * L:
            return d
    return family.MAX_DEPTH


def split_of(nind, fill, ncand, depth):
    """The split level P of a walk over ``nind`` axes: the smallest that gives ``fill`` walkers, at most depth."""
    P = 0
    while P < depth and (ncand << (nind * P)) < fill:
        P += 1
    return P


def level_tables(family, spline, levels=None, coefs=None):
    """The host path's tables of a level family: (plan, rows (nrows, *rowlen), levels or None, scale (B)), all NumPy float64."""
    plan = family.Plan(spline.order, spline.knots)
    data = np.asarray(spline.coefs if coefs is None else coefs)
    be, data, rows = bezier_rows(data.reshape((-1,) + data.shape[-plan.nind:]), "host", plan, family.LAST_PATHS)
    if levels is not None:
        levels = np.ascontiguousarray(levels, np.float64).reshape(-1)
    return plan, rows, levels, field_scale(be, data, levels)


def level_batch(family, spline, levels, coefs, depth, _path, _split):
    """``trace_batch`` and ``extract_batch`` up to their tails: the checks, the path, the tables on its backend, the run and
    the zero-cell table.  ``family``, the module, supplies NIND, BATCH (its name in the messages), ``_check_batch``, ``Plan``,
    DEFAULT_DEPTH, MAX_DEPTH, ``_check_keys`` (what the lattice's keys can hold), DEVICE_MIN_LEAVES, FORCE_PATH, LAST_PATHS
    and ``_run``.  -> (be, on_device, plan, B, res, cells): the backend, whether the caller's coefficients live on it, what
    ``_run`` returned (the backend's arrays; None for B == 0, which runs nothing) and ``zero_table`` of its zero cells."""
    n, name = family.NIND, family.BATCH
    del family.LAST_PATHS[:]
    path = pick_path(_path, family.FORCE_PATH)
    family._check_batch(spline)
    ncoef = tuple(len(spline.knots[d]) - spline.order[d] for d in range(n))
    if levels is not None and coefs is not None:
        raise ValueError(f"{name} takes levels or coefs, not both")
    if coefs is None:
        if spline.nDep != 1:
            raise ValueError(f"{name} takes one dependent variable, or coefs (B, {', '.join(f'n{d}' for d in range(n))})")
        coefs = spline.coefs
    coefs, on_device, path = coefs_arg(name, coefs, path, ncoef, f"(B, {', '.join(str(m) for m in ncoef)})")
    if levels is not None:
        levels = np.ascontiguousarray(levels, np.float64).reshape(-1)
    B = int(coefs.shape[0]) if levels is None else len(levels)
    plan = family.Plan(spline.order, spline.knots)
    nc = tuple(plan.ncells)
    depth = family.DEFAULT_DEPTH if depth is None else int(depth)
    if not 0 <= depth <= family.MAX_DEPTH:
        raise ValueError(f"depth must be in 0 .. {family.MAX_DEPTH}")
    if _split is not None and not 0 <= int(_split) <= depth:
        raise ValueError("_split must be in 0 .. depth")
    family._check_keys(plan, depth, max(B, 1))
    if path is None:
        path = "device" if (B * int(np.prod(nc))) << (n * depth) >= family.DEVICE_MIN_LEAVES else "host"
    if B == 0:
        return backend_of(coefs), on_device, plan, 0, None, zero_table(np.zeros((0,) + nc, np.uint8), plan)
    be, data, rows = bezier_rows(coefs, path, plan, family.LAST_PATHS)
    if levels is not None:
        levels = be.put(levels, np.float64)
    res = family._run(be, rows, plan, levels, field_scale(be, data, levels), depth, _split)
    return be, on_device, plan, B, res, zero_table(be.get(res["zero"]), plan)


# ------------------------------------------------------------------------------------------ the weld of isosurface and mesh
def weld(be, tris, tstart):
    """tris: the backend's int64 (m, 3), triangles as triples of vertex keys, member by member; tstart: where the B
    members start among them (B + 1 ints).  A member's vertices are its sorted unique keys.  -> (keys (n), members (n),
    the member of every vertex, triangles (m, 3), indices into keys, vertex_offsets (B + 1)), the backend's int64."""
    keys, members, triangles, vstart = [], [], [], [0]
    for b in range(len(tstart) - 1):
        unique, inverse = be.unique(tris[tstart[b]:tstart[b + 1]].reshape(-1))
        triangles.append(inverse.reshape(-1, 3) + vstart[-1])
        keys.append(unique)
        members.append(be.zeros(len(unique), np.int64) + b)
        vstart.append(vstart[-1] + len(unique))
    return be.cat(keys), be.cat(members), be.cat(triangles), be.put(vstart, np.int64)
