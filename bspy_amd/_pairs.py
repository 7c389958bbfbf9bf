"""
What ``rays`` (rays against a surface) and ``surfaces`` (lattice lines of one surface against another) share on top of
bspy_amd/_cells.py and bspy_amd/_box.py, written once: the rows and tables of one surface on a backend, the statement's
``box_of`` and ``pair_kind``, the pass driver of the pair search and the outputs of an isolate launch.  Its C++ side is
bspy_amd/csrc/bsk_pairs.hpp.  The families keep their lanes (frames, line segments), kernels and what follows the walk.
"""
import numpy as np

from . import _box
from . import _cells
from . import _native as nv
from . import refinement

EPS = _cells.EPS


# ------------------------------------------------------------------------------------------ the statement
def box_of(window):
    """(lo0, hi0, lo1, hi1, lo2, hi2) of a window [component][K0 rows of K1 floats]."""
    out = []
    for comp in window:
        flat = [x for row in comp for x in row]
        out += [min(flat), max(flat)]
    return out


def pair_kind(cell, S, inbox):
    """0: no pair; 1: a candidate; 2: a flat pair.  cell: (orders, [component]) of ``_box``; S: the scale per component.  A
    component below S eps on the whole window, or S = 0: flat when ``inbox``, else no pair; then the sign test decides."""
    if any(all(abs(x) < scale * EPS for x in comp) or scale == 0.0 for comp, scale in zip(cell[1], S)):
        return 2 if inbox else 0
    return 0 if _box.excluded(cell) else 1


# ------------------------------------------------------------------------------------------ one surface on a backend
def surface_rows(be, spline, plan, log):
    """The rows of one surface on a backend: ((3, R0, R1) float64 in Bezier form, contiguous, the backend's; cmax (3), NumPy:
    the largest |coefficient| per component of the widened coefficients).  ``log`` receives the band steps that ran."""
    if be.__class__ is _cells.Host:
        rows = np.asarray(spline.coefs).astype(np.float64)                 # float32 is widened BEFORE the extraction
        cmax = np.abs(rows).max(axis=(1, 2))
        return (_cells.band_host(rows, plan.steps, log) if plan.steps else np.ascontiguousarray(rows)), cmax
    rows = be.torch.from_numpy(np.ascontiguousarray(spline.coefs)).to(be.dev).double()     # widened BEFORE the extraction
    cmax = rows.abs().amax(dim=(1, 2)).cpu().numpy()
    if plan.steps:
        rows, ran = refinement.run_device(rows, plan.steps)
        log.extend(ran)
    return rows.contiguous(), cmax


class Tables:
    """One surface on a backend: the plan, the extracted rows (3, R0, R1), cmax (3, NumPy), first and breaks per axis, the
    boxes (ncell, 6) (``bsk_rays_boxes``, logged into ``log``) and ``surface``, the table's arguments of every entry point."""

    def __init__(self, be, plan, rows, cmax, log):
        self.be, self.plan, self.rows, self.cmax = be, plan, rows, np.asarray(cmax, np.float64)
        (self.K0, self.K1), (self.nc0, self.nc1) = plan.order, plan.ncells
        self.ncell = self.nc0 * self.nc1
        with be:
            self.first = [be.put(f, np.int32) for f in plan.first]
            self.breaks = [be.put(b, np.float64) for b in plan.breaks]
            self.boxes = be.empty((self.ncell, 6), np.float64)
            self.surface = plan.order + (be.ptr(rows),) + tuple(plan.rowlen) + tuple(plan.ncells) + tuple(be.ptr(f) for f in self.first)
            be.call("bsk_rays_boxes", *self.surface, be.ptr(self.boxes))
            log.append(nv.lib().bsk_rays_last_kernel().decode())


# ------------------------------------------------------------------------------------------ the pair search
def chunks(ncell, chunk):
    """The chunks of the pair search over ``ncell`` cells: gridDim.y of the count and emit launches."""
    nchunks = -(-ncell // chunk)
    if nchunks > 65535:
        raise ValueError("_chunk is too small: more than 65535 chunks")
    return nchunks


def passes(be, lo, hi, per_pass, limit, count, empty=False):
    """The lanes [lo, hi) in passes of at most ``per_pass`` lanes and ``limit`` pairs (None: any number).  ``count(lo, hi)``
    launches the count of a pass and returns (partial (hi - lo, nchunks) int32, whatever the caller wants back).  Yields
    (lo, hi, that, offset, npairs) per pass; offset: the exclusive sums of partial, where emit writes the pairs of (lane,
    chunk).  One number leaves the backend per pass.  A pass above ``limit`` is halved and its count launched again on the
    halves; one lane alone is never split.  A pass without a pair (offset None) is dropped unless ``empty``.  The caller
    has entered ``be``."""
    for begin in range(lo, hi, per_pass):
        end = min(begin + per_pass, hi)
        partial, back = count(begin, end)
        ends = be.cumsum(partial.reshape(-1))
        npairs = int(ends[-1])
        if limit is not None and npairs > limit and end - begin > 1:
            yield from passes(be, begin, end, (end - begin + 1) // 2, limit, count, empty)
        elif npairs:
            yield begin, end, back, ends - partial.reshape(-1), npairs
        elif empty:
            yield begin, end, back, None, 0


def isolate_outputs(be, npairs, R, n):
    """What an isolate launch writes per pair: roots (npairs, R, n), near (npairs, R), count, status, nodes (npairs)."""
    return dict(roots=be.empty((npairs, R, n), np.float64), near=be.empty((npairs, R), np.uint8), count=be.empty(npairs, np.int32),
                status=be.empty(npairs, np.uint8), nodes=be.empty(npairs, np.int32))
