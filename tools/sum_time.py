"""
Timings of integrate and add.

    python tools/sum_time.py [--quick] [--out sum_time.json]

  kernels    for a 2048 x 2048 x 3 float64 surface integrated in its first and in its last variable, a 256^3 x 3 volume
             integrated likewise, and Su + Sv of two such surfaces with different knots (the band launches of the common
             basis, then sum_bcast): every device call is timed on its own, HIP events around `--launches` back-to-back
             calls after a warm-up, bytes in + bytes out, and the time of a device-to-device copy of the same byte count
             (half read, half written) in the same process: the floor for a kernel that reads its input once and writes
             its output once.  fraction = copy time / kernel time.  A running sum cut into segments is two launches and
             reads its input twice; it is timed as one call, with the segment count the library chose and, beside it,
             with one segment (one launch).
  calls      the whole Spline.integrate and Spline.add calls, NumPy to NumPy (operators, upload, kernels, download).
  crossover  host drivers against device path (with the copies in and out) for the whole calls over surface sizes: what
             is to replace the estimate in sums.DEVICE_MIN_ELEMENTS.
Every figure is the range over `--repeats` runs.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bspy_amd import refinement, sums  # noqa: E402
from refine_time import device_time, make, wall  # noqa: E402


def copy_floor(nbytes, launches, repeats):
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return device_time(lambda: dst.copy_(src), launches, repeats)


def scan_rows(name, s, iv, launches, repeats):
    rows = []
    scan = sums.ScanMap(sums.integral_weights(s.knots[iv], s.order[iv]))
    data = torch.from_numpy(s.coefs).cuda()
    shape = data.shape
    outer, inner = int(np.prod(shape[:iv + 1])), int(np.prod(shape[iv + 2:]))
    nbytes = outer * inner * (2 * scan.n + 1) * data.element_size()
    tc = copy_floor(nbytes, launches, repeats)
    for segments, label in ((0, "segments chosen by the library"), (1, "one segment, one launch")):
        t = device_time(lambda: scan.apply_device(data, outer, inner, segments), launches, repeats)
        rows.append(dict(case=f"{name}: integrate variable {iv}, {label}", kernel=scan.last_kernel(), n=scan.n, outer=outer,
                         inner=inner, seconds=t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc,
                         fraction_of_copy=tc[0] / t[0]))
        print(json.dumps(rows[-1]), flush=True)
    scan.close()
    return rows


def add_rows(name, a, b, launches, repeats):
    """The launches of a + b over the common variables: the band kernels of both operands, then sum_bcast."""
    rows = []
    pairs = [(iv, iv) for iv in range(a.nInd)]
    tensors = []
    for s, (_, _, stages) in zip((a, b), sums._basis_plans((a, b), pairs)):
        data = torch.from_numpy(s.coefs).cuda()
        for stage in stages:
            for axis, first, w in refinement._ordered(stage, data.shape):
                band = refinement.BandMap(first, w, data.shape[axis])
                outer, inner = int(np.prod(data.shape[:axis])), int(np.prod(data.shape[axis + 1:]))
                t = device_time(lambda: band.apply_device(data, outer, inner), launches, repeats)
                nbytes = outer * inner * (band.nIn + band.nOut) * data.element_size()
                tc = copy_floor(nbytes, launches, repeats)
                rows.append(dict(case=f"{name}: common basis", kernel=band.last_kernel(), K=band.K, nIn=band.nIn, nOut=band.nOut,
                                 outer=outer, inner=inner, seconds=t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9,
                                 copy_seconds=tc, fraction_of_copy=tc[0] / t[0]))
                print(json.dumps(rows[-1]), flush=True)
                data = refinement._apply(band, data, axis)
                band.close()
        tensors.append(data)
    x, y = tensors
    t = device_time(lambda: sums.add_tensors(x, y, 1), launches, repeats)
    nbytes = 3 * x.numel() * x.element_size()
    tc = copy_floor(nbytes, launches, repeats)
    rows.append(dict(case=f"{name}: the sum (two reads, one write; the copy moves the same bytes)", kernel=sums.LAST_PATHS[0],
                     shape=list(x.shape), seconds=t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc,
                     fraction_of_copy=tc[0] / t[0]))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def crossover(repeats, quick):
    rng = np.random.default_rng(3)
    rows = []
    for n in (16, 32, 64, 128, 256, 512) if quick else (16, 32, 64, 96, 128, 192, 256, 384, 512, 1024):
        a, b = make(rng, (n, n)), make(rng, (n, n))
        row = dict(shape=[3, n, n], elements=3 * n * n,
                   integrate_host=wall(lambda: a.integrate(0, _path="host"), repeats),
                   integrate_device=wall(lambda: a.integrate(0, _path="device"), repeats),
                   add_result_elements=3 * (2 * n - 4) ** 2,
                   add_host=wall(lambda: a.add(b, [0, 1], _path="host"), repeats),
                   add_device=wall(lambda: a.add(b, [0, 1], _path="device"), repeats))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(kernels=[], calls=[], crossover=[])

    shapes = [(1024, 1024)] if a.quick else [(2048, 2048), (256, 256, 256)]
    for shape in shapes:
        s = make(rng, shape)
        label = " x ".join(map(str, shape)) + " x 3"
        for iv in (0, len(shape) - 1):
            results["kernels"] += scan_rows(label, s, iv, a.launches, a.repeats)
            row = dict(call=f"{label}: Spline.integrate({iv}), NumPy to NumPy", seconds=wall(lambda: s.integrate(iv, _path="device"), a.repeats))
            results["calls"].append(row)
            print(json.dumps(row), flush=True)
        if len(shape) == 2:
            other = make(rng, shape)
            results["kernels"] += add_rows(f"{label}: Su + Sv, different knots", s, other, a.launches, a.repeats)
            row = dict(call=f"{label}: Su + Sv, NumPy to NumPy", seconds=wall(lambda: s + other, min(a.repeats, 2)))
            results["calls"].append(row)
            print(json.dumps(row), flush=True)
            del other
        del s

    results["crossover"] = crossover(a.repeats, a.quick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
