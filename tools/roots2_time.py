"""
Timings of Spline.zeros2 / roots2.zeros2_batch.  NOBODY HAS RUN THIS ON AN MI355X YET: until someone
does, roots2.DEVICE_MIN_CELLS is an estimate.

    python tools/roots2_time.py [--quick] [--out roots2_time.json]

  kernels    for bicubic float64 systems of B x (cells x cells): roots2_flag, roots2_isolate and roots2_merge, each timed on
             its own, HIP events around `--launches` back-to-back calls after a warm-up.  roots2_flag reads its rows once:
             its bytes and the time of a device-to-device copy of as many bytes are given (fraction = copy / kernel).  The
             other two are arithmetic and pointer chasing: candidates, zeros and visited nodes per second are given.
  calls      the whole call, NumPy to arrays, on both paths: the host / device crossover table that is to replace the
             estimate in roots2.DEVICE_MIN_CELLS.  The parent commit has no zeros2, so the host driver is the baseline.
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
from bspy_amd import Spline, refinement, roots2  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from refine_time import device_time, wall  # noqa: E402
from roots_time import copy_floor  # noqa: E402


def make(rng, ncells, B=1, order=(4, 4)):
    knots = [np.concatenate((k * [0.0], np.sort(rng.random(ncells - 1)), k * [1.0])) for k in order]
    ncoef = [len(t) - k for t, k in zip(knots, order)]
    coefs = rng.standard_normal((B, 2, *ncoef))
    return Spline(2, 2, list(order), ncoef, knots, coefs[0]), coefs


def kernel_rows(name, s, coefs, launches, repeats):
    out = []
    K0, K1 = s.order
    R = roots2.slots(K0, K1)
    B = coefs.shape[0]
    plan = roots2.Plan2(s.order, s.knots)
    nc0, nc1 = plan.ncells
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, _ = refinement.run_device(torch.from_numpy(coefs).cuda().reshape(2 * B, *coefs.shape[2:]), plan.steps)
    rows = rows.contiguous()
    L = nv.lib()

    def row(kernel, t, **more):
        out.append(dict(case=name, kernel=kernel, seconds=t, **more))
        print(json.dumps(out[-1]), flush=True)

    first0, first1 = (torch.from_numpy(f).cuda() for f in plan.first)
    grid = (K0, K1, rows.data_ptr(), B, plan.rowlen[0], plan.rowlen[1], nc0, nc1, first0.data_ptr(), first1.data_ptr())
    mask = torch.zeros((B, nc0, nc1), dtype=torch.uint8, device="cuda")
    flags = torch.empty_like(mask)
    t = device_time(lambda: nv.check(L.bsk_roots2_flag(*grid, mask.data_ptr(), flags.data_ptr(), stream)), launches, repeats)
    nbytes = rows.numel() * 8 + 2 * B * nc0 * nc1
    tc = copy_floor(nbytes, launches, repeats)
    row("roots2_flag", t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc, fraction_of_copy=tc[0] / t[0], cells=B * nc0 * nc1)

    cand = torch.nonzero(flags.reshape(-1)).reshape(-1)
    n = int(cand.numel())
    found = torch.empty((n, R, 2), dtype=torch.float64, device="cuda")
    near = torch.empty((n, R), dtype=torch.uint8, device="cuda")
    count, nodes = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    breaks0, breaks1 = (torch.from_numpy(np.ascontiguousarray(b, np.float64)).cuda() for b in plan.breaks)
    scale = torch.from_numpy(np.ascontiguousarray(np.abs(coefs).max(axis=(2, 3)))).cuda()
    t = device_time(lambda: nv.check(L.bsk_roots2_isolate(*grid, breaks0.data_ptr(), breaks1.data_ptr(), scale.data_ptr(), cand.data_ptr(), n,
                                                          found.data_ptr(), near.data_ptr(), count.data_ptr(), status.data_ptr(),
                                                          nodes.data_ptr(), stream)), launches, repeats)
    visited = int(nodes.sum().item())
    row("roots2_isolate", t, candidates=n, zeros=int(count.sum().item()), nodes=visited, nodes_per_s=visited / t[0],
        largest_walk=int(nodes.max().item()), flagged_status=int((status != 0).sum().item()))

    which = torch.nonzero(near.reshape(-1)).reshape(-1)
    if int(which.numel()):
        keep = torch.ones((n, R), dtype=torch.uint8, device="cuda")
        table = torch.cumsum(flags.reshape(-1), 0, dtype=torch.int64) - 1
        t = device_time(lambda: nv.check(L.bsk_roots2_merge(R, found.data_ptr(), B, nc0, nc1, breaks0.data_ptr(), breaks1.data_ptr(),
                                                            cand.data_ptr(), n, flags.data_ptr(), table.data_ptr(), which.data_ptr(),
                                                            int(which.numel()), keep.data_ptr(), stream)), launches, repeats)
        row("roots2_merge", t, near=int(which.numel()))
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
    for ncells, B in ([(16, 1), (64, 1)] if a.quick else [(16, 1), (64, 1), (256, 1), (8, 1024)]):
        s, coefs = make(rng, ncells, B)
        results["kernels"] += kernel_rows(f"bicubic, {B} x {ncells} x {ncells} cells", s, coefs, a.launches, a.repeats)
    for ncells, B in [(4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (4, 64)] + ([] if a.quick else [(128, 1), (8, 1024)]):
        s, coefs = make(rng, ncells, B)
        row = dict(call=f"zeros2_batch, bicubic, {B} x {ncells} x {ncells} cells, NumPy to arrays", cells=B * ncells * ncells,
                   zeros=int(len(roots2.zeros2_batch(s, coefs=coefs, _path="host")[0])),
                   host=wall(lambda: roots2.zeros2_batch(s, coefs=coefs, _path="host"), a.repeats),
                   device=wall(lambda: roots2.zeros2_batch(s, coefs=coefs, _path="device"), a.repeats))
        results["calls"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
