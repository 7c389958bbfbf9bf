"""
Timings of Spline.contours / contours.trace_batch (DESIGN.md section 21 holds the table of its --quick run on an MI355X,
from which contours.DEVICE_MIN_LEAVES is read; the full run has not been made).

    python tools/contours_time.py [--quick] [--out contours_time.json]

  kernels    for bicubic float64 fields of B x (cells x cells) at depth 4: contour_flag, contour_march count and
             contour_march emit, each timed on its own, HIP events around `--launches` back-to-back calls after a warm-up.
             contour_flag reads its rows once: its bytes and the time of a device-to-device copy of as many bytes are given
             (fraction = copy / kernel).  The march launches are arithmetic: candidate cells, lanes, leaves of the lattice
             and segments per second are given, at the split level the host would choose and at P = 0.
  calls      the whole call, NumPy to polylines (linking on the host included), on both paths: the host / device crossover
             table behind contours.DEVICE_MIN_LEAVES.  The parent commit has no contours, so
             the host driver is the baseline.
Every figure is the range over `--repeats` runs.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bspy_amd import Spline, _cells, contours  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from refine_time import device_time, wall  # noqa: E402
from roots_time import copy_floor  # noqa: E402


def make(rng, ncells, B=1, order=(4, 4)):
    knots = [np.concatenate((k * [0.0], np.sort(rng.random(ncells - 1)), k * [1.0])) for k in order]
    ncoef = [len(t) - k for t, k in zip(knots, order)]
    coefs = rng.uniform(-1.0, 1.0, (B, *ncoef))
    return Spline(2, 1, list(order), ncoef, knots, coefs[:1]), coefs


def kernel_rows(name, s, coefs, depth, launches, repeats):
    out = []
    B = coefs.shape[0]
    plan = contours.Plan(s.order, s.knots)
    nc0, nc1 = plan.ncells
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    be, data, rows = _cells.bezier_rows(coefs, "device", plan, [])
    L = nv.lib()

    def row(kernel, t, **more):
        out.append(dict(case=name, kernel=kernel, seconds=t, **more))
        print(json.dumps(out[-1]), flush=True)

    first0, first1 = (torch.from_numpy(f).cuda() for f in plan.first)
    scale = _cells.field_scale(be, data)
    grid = contours._grid(plan, rows, lambda a: a.data_ptr(), None, B, scale, first0, first1)
    cand = torch.empty((B, nc0, nc1), dtype=torch.uint8, device="cuda")
    zero = torch.empty_like(cand)
    t = device_time(lambda: nv.check(L.bsk_contour_flag(*grid, cand.data_ptr(), zero.data_ptr(), stream)), launches, repeats)
    nbytes = rows.numel() * 8 + 2 * B * nc0 * nc1
    tc = copy_floor(nbytes, launches, repeats)
    row("contour_flag", t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc, fraction_of_copy=tc[0] / t[0], cells=B * nc0 * nc1)

    idx = torch.nonzero(cand.reshape(-1)).reshape(-1)
    n = int(idx.numel())
    breaks0, breaks1 = (torch.from_numpy(np.ascontiguousarray(b, np.float64)).cuda() for b in plan.breaks)
    for P in sorted({contours.split_of(n, depth), 0}):
        lanes = n << (2 * P)
        counts = torch.empty(lanes, dtype=torch.int32, device="cuda")
        lane_status = torch.empty(lanes, dtype=torch.uint8, device="cuda")
        march = grid + (breaks0.data_ptr(), breaks1.data_ptr(), idx.data_ptr(), n, depth, P)
        t = device_time(lambda: nv.check(L.bsk_contour_march(*march, 0, None, 0, counts.data_ptr(), lane_status.data_ptr(), None, None,
                                                             stream)), launches, repeats)
        leaves = n << (2 * depth)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(ends[-1])
        row("contour_march count", t, split=P, candidates=n, lanes=lanes, leaves=leaves, leaves_per_s=leaves / t[0], segments=total)
        if total:
            offsets = (ends - counts).contiguous()
            keys = torch.empty((total, 2), dtype=torch.int64, device="cuda")
            xy = torch.empty((total, 4), dtype=torch.float64, device="cuda")
            t = device_time(lambda: nv.check(L.bsk_contour_march(*march, 1, offsets.data_ptr(), total, None, None, keys.data_ptr(),
                                                                 xy.data_ptr(), stream)), launches, repeats)
            row("contour_march emit", t, split=P, candidates=n, lanes=lanes, segments=total, segments_per_s=total / t[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(kernels=[], calls=[])
    for ncells, B in ([(1, 1), (16, 1)] if a.quick else [(1, 1), (16, 1), (64, 1), (8, 256)]):
        s, coefs = make(rng, ncells, B)
        depth = 8 if ncells == 1 else 4
        results["kernels"] += kernel_rows(f"bicubic, {B} x {ncells} x {ncells} cells, depth {depth}", s, coefs, depth, a.launches, a.repeats)
    for ncells, B in [(2, 1), (4, 1), (8, 1), (16, 1), (32, 1)] + ([] if a.quick else [(64, 1), (8, 64)]):
        s, coefs = make(rng, ncells, B)
        row = dict(call=f"trace_batch, bicubic, {B} x {ncells} x {ncells} cells, depth 4, NumPy to polylines",
                   leaves=(B * ncells * ncells) << 8, polylines=int(len(contours.trace_batch(s, coefs=coefs, _path="host")[1]) - 1),
                   host=wall(lambda: contours.trace_batch(s, coefs=coefs, _path="host"), a.repeats),
                   device=wall(lambda: contours.trace_batch(s, coefs=coefs, _path="device"), a.repeats))
        results["calls"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
