"""
Timings of insert_knots / elevate / trim.

    python tools/refine_time.py [--quick] [--out refine_time.json] [--reference-dir DIR]

  kernels    for a 2048 x 2048 x 3 float64 surface and a 256^3 x 3 volume: (a) insertion that doubles the knots of one
             variable, the first and the last; (b) elevation by 1 in every variable; (c) trim to the middle half.  Every
             kernel launch of the call is timed on its own: HIP events around `--launches` back-to-back launches after
             a warm-up, bytes in + bytes out, and the time of a device-to-device copy of the same byte count (half read,
             half written) in the same process: the floor for a kernel that reads its input once and writes its output
             once.  fraction = copy time / kernel time.
  calls      the whole Spline.insert_knots call, NumPy to NumPy (operator construction, upload, kernels, download), for
             the large surface and for a 512 x 512 x 3 surface with 200 + 200 new knots; with --reference-dir (a
             checkout of the reference) the reference's time for the small one on this machine's CPU.
  crossover  host driver against device path (with the copies in and out) for the whole call over surface sizes: where
             refinement.DEVICE_MIN_ELEMENTS comes from.
Every figure is the range over `--repeats` runs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bspy_amd import Spline, refinement  # noqa: E402


def jittered_knots(rng, order, ncoef):
    interior = np.linspace(0.0, 1.0, ncoef - order + 2)[1:-1]
    interior += (rng.random(ncoef - order) - 0.5) * 0.6 / (ncoef - order + 1)
    return np.concatenate((order * [0.0], interior, order * [1.0]))


def make(rng, shape, order=4, dtype=np.float64):
    knots = [jittered_knots(rng, order, n) for n in shape]
    return Spline(len(shape), 3, len(shape) * [order], shape, knots, rng.standard_normal((3, *shape)).astype(dtype))


def midpoints(knots, order):
    t = knots[order - 1:len(knots) - order + 1]
    return list(0.5 * (t[1:] + t[:-1]))


def wall(f, repeats):
    f()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return [min(out), max(out)]


def device_time(f, launches, repeats):
    """Seconds per launch: events around `launches` back-to-back launches."""
    for _ in range(3):
        f()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            f()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / launches)
    return [min(out), max(out)]


def captured(call):
    """Run `call` on the device path and return the launches it made: (first, w, nIn, shape, axis, dtype)."""
    steps, keep = [], refinement.BandMap.along

    def spy(band, be, tensor, axis, fused=False):
        steps.append((band.first.copy(), band.w.copy(), band.nIn, tuple(tensor.shape), axis, tensor.dtype))
        return keep(band, be, tensor, axis, fused)

    refinement.BandMap.along = spy
    try:
        call()
    finally:
        refinement.BandMap.along = keep
    return steps


def kernels(name, call, launches, repeats):
    rows = []
    for first, w, n_in, shape, axis, dtype in captured(call):
        band = refinement.BandMap(first, w, n_in)
        data = torch.randn(shape, dtype=dtype, device="cuda")
        outer, inner = int(np.prod(shape[:axis])), int(np.prod(shape[axis + 1:]))
        t = device_time(lambda: band.apply_device(data, outer, inner), launches, repeats)
        nbytes = outer * inner * (band.nIn + band.nOut) * data.element_size()
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        tc = device_time(lambda: dst.copy_(src), launches, repeats)
        rows.append(dict(case=name, kernel=band.last_kernel(), K=band.K, nIn=band.nIn, nOut=band.nOut, outer=outer, inner=inner,
                         seconds=t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc,
                         fraction_of_copy=tc[0] / t[0]))
        print(json.dumps(rows[-1]), flush=True)
        band.close()
        del data, src, dst
    return rows


def crossover(repeats, quick):
    rng = np.random.default_rng(3)
    rows = []
    for n in (16, 32, 64, 128, 256, 512) if quick else (16, 32, 64, 96, 128, 192, 256, 384, 512, 1024):
        s = make(rng, (n, n))
        new = [list(rng.random(n // 4)), list(rng.random(n // 4))]
        row = dict(shape=[3, n, n], elements=3 * n * n,
                   host=wall(lambda: s.insert_knots(new, _path="host"), repeats),
                   device=wall(lambda: s.insert_knots(new, _path="device"), repeats))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def reference_seconds(directory, s, new):
    sys.path.insert(0, directory)
    import bspy
    r = bspy.Spline(s.nInd, s.nDep, s.order, s.nCoef, s.knots, s.coefs)
    t0 = time.perf_counter()
    r.insert_knots(new)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference-dir", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(kernels=[], calls=[], crossover=[])

    shapes = [(1024, 1024)] if a.quick else [(2048, 2048), (256, 256, 256)]
    for shape in shapes:
        s = make(rng, shape)
        label = " x ".join(map(str, shape)) + " x 3"
        nind = len(shape)
        empty = [[] for _ in shape]
        for iv in (0, nind - 1):
            new = list(empty)
            new[iv] = midpoints(s.knots[iv], 4)
            results["kernels"] += kernels(f"{label}: insert, variable {iv} doubled", lambda: s.insert_knots(new, _path="device"),
                                          a.launches, a.repeats)
        results["kernels"] += kernels(f"{label}: elevate by 1", lambda: s.elevate(nind * [1], _path="device"), a.launches, a.repeats)
        results["kernels"] += kernels(f"{label}: trim to the middle half", lambda: s.trim(nind * [[0.25, 0.75]], _path="device"),
                                      a.launches, a.repeats)
        if nind == 2:
            new = [midpoints(k, 4) for k in s.knots]
            row = dict(call=f"{label}: Spline.insert_knots, both variables doubled, NumPy to NumPy",
                       seconds=wall(lambda: s.insert_knots(new, _path="device"), a.repeats))
            results["calls"].append(row)
            print(json.dumps(row), flush=True)
        del s

    s = make(rng, (512, 512))
    new = [list(rng.random(200)), list(rng.random(200))]
    row = dict(call="512 x 512 x 3: Spline.insert_knots, 200 + 200 knots, NumPy to NumPy",
               seconds=wall(lambda: s.insert_knots(new, _path="device"), a.repeats),
               host_path_seconds=wall(lambda: s.insert_knots(new, _path="host"), a.repeats))
    if a.reference_dir:
        row["reference_seconds"] = reference_seconds(a.reference_dir, s, new)
    results["calls"].append(row)
    print(json.dumps(row), flush=True)

    results["crossover"] = crossover(a.repeats, a.quick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
