"""
Timings of Spline.zeros3 / roots3.zeros3_batch.

    python tools/roots3_time.py [--quick] [--out roots3_time.json]

  kernels    for tricubic float64 systems of B x (cells x cells x cells): roots3_flag, roots3_isolate and roots3_merge and the
             band launches of the extraction, each timed on its own, HIP events around `--launches` back-to-back calls after
             a warm-up.  roots3_flag reads its rows once: its bytes and the time of a device-to-device copy of as many bytes
             are given (fraction = copy / kernel).  roots3_isolate is arithmetic and lane moves: candidates, zeros and
             visited nodes per second are given.
  calls      the whole call, NumPy to arrays, on both paths: the host / device crossover table behind
             roots3.DEVICE_MIN_CELLS.  The parent commit has no zeros3, so the host driver is the baseline.
  surface    last, the largest size: a whole ``zeros3`` call on both paths for a 32 x 32-coefficient bicubic surface against
             a 64-coefficient cubic curve (``surface.subtract(curve)``: 29 x 29 x 61 cells).
Every figure is the range over `--repeats` runs.  The reference's time on the same systems is not taken here: the reference is
not part of this repository; tests/golden/make_golden_roots3.py, which runs where it is importable, records its seconds per
golden case (``ref_seconds``).
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
from bspy_amd import Spline, refinement, roots3  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from refine_time import device_time, wall  # noqa: E402
from roots_time import copy_floor  # noqa: E402


def make(rng, ncells, B=1, order=(4, 4, 4)):
    knots = [np.concatenate((k * [0.0], np.sort(rng.random(ncells - 1)), k * [1.0])) for k in order]
    ncoef = [len(t) - k for t, k in zip(knots, order)]
    coefs = rng.standard_normal((B, 3, *ncoef))
    return Spline(3, 3, list(order), ncoef, knots, coefs[0]), coefs


def surface_and_curve(rng):
    ks = [np.concatenate((4 * [0.0], np.sort(rng.random(28)), 4 * [1.0])) for _ in range(2)]
    kc = np.concatenate((4 * [0.0], np.sort(rng.random(60)), 4 * [1.0]))
    gu, gv = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), indexing="ij")
    surface = np.stack([gu, gv, 0.3 * np.sin(5.0 * gu) * np.cos(4.0 * gv)]) + 0.01 * rng.standard_normal((3, 32, 32))
    t = np.linspace(0, 1, 64)
    curve = np.stack([0.5 + 0.4 * np.cos(9.0 * t) * t, 0.5 + 0.4 * np.sin(9.0 * t) * t, 0.5 * np.cos(14.0 * t)])
    return Spline(2, 3, [4, 4], [32, 32], ks, surface), Spline(1, 3, [4], [64], [kc], curve)


def kernel_rows(name, s, coefs, launches, repeats):
    out = []
    K = tuple(int(k) for k in s.order)
    R = roots3.slots(*K)
    B = coefs.shape[0]
    plan = roots3.Plan3(s.order, s.knots)
    nc = plan.ncells
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    data = torch.from_numpy(coefs).cuda().reshape(3 * B, *coefs.shape[2:])
    rows, _ = refinement.run_device(data, plan.steps)
    rows = rows.contiguous()
    L = nv.lib()

    def row(kernel, t, **more):
        out.append(dict(case=name, kernel=kernel, seconds=t, **more))
        print(json.dumps(out[-1]), flush=True)

    row("band launches of the extraction", device_time(lambda: refinement.run_device(data, plan.steps), launches, repeats), steps=len(plan.steps))
    first = [torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda() for f in plan.first]
    grid = K + (rows.data_ptr(), B) + tuple(plan.rowlen) + tuple(nc) + tuple(f.data_ptr() for f in first)
    mask = torch.zeros((B, *nc), dtype=torch.uint8, device="cuda")
    flags = torch.empty_like(mask)
    t = device_time(lambda: nv.check(L.bsk_roots3_flag(*grid, mask.data_ptr(), flags.data_ptr(), stream)), launches, repeats)
    nbytes = rows.numel() * 8 + 2 * mask.numel()
    tc = copy_floor(nbytes, launches, repeats)
    row("roots3_flag", t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc, fraction_of_copy=tc[0] / t[0], cells=mask.numel())

    cand = torch.nonzero(flags.reshape(-1)).reshape(-1)
    n = int(cand.numel())
    found = torch.empty((n, R, 3), dtype=torch.float64, device="cuda")
    near = torch.empty((n, R), dtype=torch.uint8, device="cuda")
    count, nodes = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    breaks = [torch.from_numpy(np.ascontiguousarray(b, np.float64)).cuda() for b in plan.breaks]
    scale = torch.from_numpy(np.ascontiguousarray(np.abs(coefs).max(axis=(2, 3, 4)))).cuda()
    t = device_time(lambda: nv.check(L.bsk_roots3_isolate(*grid, *(b.data_ptr() for b in breaks), scale.data_ptr(), cand.data_ptr(), n,
                                                          found.data_ptr(), near.data_ptr(), count.data_ptr(), status.data_ptr(),
                                                          nodes.data_ptr(), stream)), launches, repeats)
    visited = int(nodes.sum().item())
    row("roots3_isolate", t, candidates=n, zeros=int(count.sum().item()), nodes=visited, nodes_per_s=visited / t[0],
        largest_walk=int(nodes.max().item()), flagged_status=int((status != 0).sum().item()))

    which = torch.nonzero(near.reshape(-1)).reshape(-1)
    if int(which.numel()):
        keep = torch.ones((n, R), dtype=torch.uint8, device="cuda")
        table = torch.cumsum(flags.reshape(-1), 0, dtype=torch.int64) - 1
        t = device_time(lambda: nv.check(L.bsk_roots3_merge(R, found.data_ptr(), B, *nc, *(b.data_ptr() for b in breaks), cand.data_ptr(), n,
                                                            flags.data_ptr(), table.data_ptr(), which.data_ptr(), int(which.numel()),
                                                            keep.data_ptr(), stream)), launches, repeats)
        row("roots3_merge", t, near=int(which.numel()))
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
    results = dict(kernels=[], surface=[], calls=[])

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    for ncells, B in ([(4, 1), (8, 1)] if a.quick else [(4, 1), (8, 1), (16, 1), (4, 64)]):
        s, coefs = make(rng, ncells, B)
        results["kernels"] += kernel_rows(f"tricubic, {B} x {ncells}^3 cells", s, coefs, a.launches, a.repeats)
        flush()
    for ncells, B in [(2, 1), (3, 1), (4, 1), (6, 1), (8, 1), (2, 64)] + ([] if a.quick else [(12, 1), (16, 1)]):
        s, coefs = make(rng, ncells, B)
        row = dict(call=f"zeros3_batch, tricubic, {B} x {ncells}^3 cells, NumPy to arrays", cells=B * ncells ** 3,
                   zeros=int(len(roots3.zeros3_batch(s, coefs=coefs, _path="host")[0])),
                   host=wall(lambda: roots3.zeros3_batch(s, coefs=coefs, _path="host"), a.repeats),
                   device=wall(lambda: roots3.zeros3_batch(s, coefs=coefs, _path="device"), a.repeats))
        results["calls"].append(row)
        print(json.dumps(row), flush=True)
        flush()

    surface, curve = surface_and_curve(rng)
    system = surface.subtract(curve)
    cells = int(np.prod(roots3.Plan3(system.order, system.knots).ncells))
    row = dict(call="zeros3 of a 32 x 32 bicubic surface minus a 64-coefficient cubic curve", cells=cells,
               zeros=len(system.zeros3(_path="device")), device=wall(lambda: system.zeros3(_path="device"), a.repeats),
               host=wall(lambda: system.zeros3(_path="host"), max(1, a.repeats // 2)))
    results["surface"].append(row)
    print(json.dumps(row), flush=True)
    flush()


if __name__ == "__main__":
    main()
