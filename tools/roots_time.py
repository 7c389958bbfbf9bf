"""
Timings of Spline.zeros / roots.zeros_batch.

    python tools/roots_time.py [--quick] [--reference DIR] [--out roots_time.json]

  kernels    for order-4 float64 curves of 10^4, 10^5 and 10^6 coefficients (one component) and of 256 components x 4096
             coefficients: the extraction launch (band_apply_line), roots_flag and roots_isolate, each timed on its own, HIP
             events around `--launches` back-to-back calls after a warm-up, with the bytes the launch reads and writes and
             the time of a device-to-device copy of the same byte count in the same process: the floor for the first two,
             which read their input once and write their output once.  fraction = copy time / kernel time.  roots_isolate
             is arithmetic, not traffic; its fraction is given for scale only.
  calls      the whole call, NumPy to list / arrays, on both paths (plans, tables, upload, launches, download): the
             crossover that is to replace the estimate in roots.DEVICE_MIN_SPANS.
  reference  with --reference DIR (a checkout of the reference that imports): its zeros() on this machine's CPU at 10^3 and
             4 * 10^3 coefficients, for the ratio.
Every figure is the range over `--repeats` runs.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bspy_amd import Spline, refinement, roots  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from refine_time import device_time, wall  # noqa: E402

EPS = float(np.finfo(np.float64).eps)


def make(rng, ncoef, ncomp=1, order=4):
    t = np.concatenate((order * [0.0], np.sort(rng.random(ncoef - order)), order * [1.0]))
    return Spline(1, ncomp, [order], [ncoef], [t], rng.standard_normal((ncomp, ncoef)))


def copy_floor(nbytes, launches, repeats):
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return device_time(lambda: dst.copy_(src), launches, repeats)


def kernel_rows(name, s, launches, repeats):
    out = []
    k, nDep = s.order[0], s.nDep
    plan = roots.BezierPlan(k, s.knots[0])
    data = torch.from_numpy(s.coefs).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def row(kernel, t, nbytes, **more):
        tc = copy_floor(nbytes, launches, repeats)
        out.append(dict(case=name, kernel=kernel, seconds=t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc,
                        fraction_of_copy=tc[0] / t[0], **more))
        print(json.dumps(out[-1]), flush=True)

    _, first, w = plan.steps[0]
    band = refinement.BandMap(first, w, data.shape[1])
    t = device_time(lambda: band.apply_device(data, nDep, 1), launches, repeats)
    row(band.last_kernel(), t, nDep * (band.nIn + band.nOut) * 8, nIn=band.nIn, nOut=band.nOut)
    rows = band.apply_device(data, nDep, 1).reshape(nDep, band.nOut)
    band.close()

    mask = np.zeros((nDep, plan.nspans), np.uint8)
    mask[:, -1] = roots.MASK_LAST
    d_first, d_mask = torch.from_numpy(plan.first).cuda(), torch.from_numpy(mask).cuda()
    flags = torch.empty((nDep, plan.nspans), dtype=torch.uint8, device="cuda")
    L = nv.lib()
    t = device_time(lambda: nv.check(L.bsk_roots_flag(nv.BSK_F64, k, rows.data_ptr(), nDep, plan.rowlen, plan.nspans, d_first.data_ptr(),
                                                      d_mask.data_ptr(), flags.data_ptr(), stream)), launches, repeats)
    row("roots_flag", t, nDep * plan.rowlen * 8 + 2 * nDep * plan.nspans + 4 * plan.nspans, spans=nDep * plan.nspans)

    cand = torch.nonzero(flags.reshape(-1)).reshape(-1)
    ncand = int(cand.numel())
    found = torch.empty((ncand, k - 1), dtype=torch.float64, device="cuda")
    count = torch.empty(ncand, dtype=torch.int32, device="cuda")
    breaks = torch.from_numpy(np.ascontiguousarray(plan.breaks, np.float64)).cuda()
    scale = torch.from_numpy(np.abs(s.coefs).max(axis=1)).cuda()
    t = device_time(lambda: nv.check(L.bsk_roots_isolate(nv.BSK_F64, k, rows.data_ptr(), nDep, plan.rowlen, plan.nspans,
                                                         d_first.data_ptr(), d_mask.data_ptr(), breaks.data_ptr(), scale.data_ptr(),
                                                         plan.margin, cand.data_ptr(), ncand, found.data_ptr(), count.data_ptr(), stream)),
                    launches, repeats)
    row("roots_isolate", t, ncand * (8 + k * 8 + 16 + (k - 1) * 8 + 4), candidates=ncand, roots=int(count.sum().item()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(kernels=[], calls=[], reference=[])

    shapes = [(10 ** 4, 1), (10 ** 5, 1)] if a.quick else [(10 ** 4, 1), (10 ** 5, 1), (10 ** 6, 1), (4096, 256)]
    for ncoef, ncomp in shapes:
        s = make(rng, ncoef, ncomp)
        results["kernels"] += kernel_rows(f"order 4, {ncomp} x {ncoef} coefficients", s, a.launches, a.repeats)
    for ncoef, ncomp in [(10 ** 3, 1), (4 * 10 ** 3, 1), (16 * 10 ** 3, 1), (64 * 10 ** 3, 1)] + ([] if a.quick else [(10 ** 6, 1), (4096, 256)]):
        s = make(rng, ncoef, ncomp)
        row = dict(call=f"zeros_batch, order 4, {ncomp} x {ncoef} coefficients, NumPy to arrays", spans=ncomp * (ncoef - 3),
                   roots=int(len(roots.zeros_batch(s, _path="host")[0])),
                   host=wall(lambda: roots.zeros_batch(s, _path="host"), a.repeats),
                   device=wall(lambda: roots.zeros_batch(s, _path="device"), a.repeats))
        results["calls"].append(row)
        print(json.dumps(row), flush=True)
    if a.reference:
        sys.path.insert(0, a.reference)
        import bspy
        for ncoef in (10 ** 3, 4 * 10 ** 3):
            s = make(np.random.default_rng(ncoef), ncoef)
            ref = bspy.Spline(1, 1, s.order, s.nCoef, s.knots, s.coefs)
            t0 = time.perf_counter()
            found = ref.zeros()
            row = dict(call=f"the reference's zeros(), order 4, {ncoef} coefficients", seconds=time.perf_counter() - t0, roots=len(found),
                       ours=len(s.zeros(_path="host")))
            results["reference"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
