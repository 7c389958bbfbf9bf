"""
Timings of remove_knots.

    python tools/remove_time.py [--quick] [--out remove_time.json]
    python tools/remove_time.py --reference-dir DIR          (no GPU needed: the reference's times only)

  kernels    band_absmax and band_absmax_line (each with its fold launch) with the residual operator of an order-4
             variable on a 2048 x 2048 x 3 float64 tensor, first and last variable: HIP events around `--launches`
             back-to-back calls after a warm-up, against a device-to-device copy of the same input bytes in the same
             process (the floor for a kernel that reads its input once and writes next to nothing).
  calls      a whole Spline.remove_knots call, NumPy to NumPy, on both paths: a 1024 x 1024 x 3 surface made from
             768 x 768 by inserting 256 + 256 knots, tolerance 1e-12 (the call takes them out again).
  crossover  host path against device path for the whole call over surface sizes: where
             reduction.DEVICE_MIN_ELEMENTS comes from.
  reference  with --reference-dir (a checkout of the reference): the reference's remove_knots on the two-component
             order-4 curve of tests/golden/make_golden_remove.py at tolerance 1e-5, doubling the coefficients from 120
             until a run takes more than a minute (that run is abandoned), next to the host path's time for the same
             input.
Every figure is the range over `--repeats` runs.
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bspy_amd import Spline, reduction  # noqa: E402
from bspy_amd.refinement import BandMap  # noqa: E402


def jittered_knots(rng, order, ncoef):
    interior = np.linspace(0.0, 1.0, ncoef - order + 2)[1:-1]
    interior += (rng.random(ncoef - order) - 0.5) * 0.6 / (ncoef - order + 1)
    return np.concatenate((order * [0.0], interior, order * [1.0]))


def refined_surface(rng, n, extra, order=4):
    knots = [jittered_knots(rng, order, n) for _ in range(2)]
    s = Spline(2, 3, [order, order], [n, n], knots, rng.standard_normal((3, n, n)))
    return s.insert_knots([list(0.01 + 0.98 * rng.random(extra)) for _ in range(2)], _path="host")


def wall(f, repeats, sync):
    f()
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        out.append(time.perf_counter() - t0)
    return [min(out), max(out)]


def device_time(torch, f, launches, repeats):
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


def kernels(torch, n, launches, repeats):
    rng = np.random.default_rng(0)
    rows = []
    data = torch.randn((3, n, n), dtype=torch.float64, device="cuda")
    src = torch.empty(data.numel() * data.element_size(), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    tc = device_time(torch, lambda: dst.copy_(src), launches, repeats)
    _, first, v = reduction.residual_map(jittered_knots(rng, 4, n), 4)
    band = BandMap(first, v, n)
    for axis in (1, 2):
        t = device_time(torch, lambda: reduction.absmax(band, data, axis, 3), launches, repeats)
        rows.append(dict(case=f"3 x {n} x {n} float64, order 4, variable {axis - 1}", kernel=band.last_kernel(), K=band.K, nOut=band.nOut,
                         seconds=t, input_bytes=src.numel(), gbytes_per_s=src.numel() / t[0] * 1e-9, copy_seconds=tc,
                         copy_gbytes_per_s_read=src.numel() / tc[0] * 1e-9))
        print(json.dumps(rows[-1]), flush=True)
    band.close()
    return rows


def calls(torch, n, extra, repeats):
    s = refined_surface(np.random.default_rng(1), n, extra)
    row = dict(call=f"{s.nCoef[0]} x {s.nCoef[1]} x 3 from {n} x {n}: Spline.remove_knots(1e-12), NumPy to NumPy")
    for path in ("device", "host"):
        row[path + "_seconds"] = wall(lambda: s.remove_knots(1e-12, _path=path), repeats, torch.cuda.synchronize)
        row[path + "_ncoef"] = list(s.remove_knots(1e-12, _path=path).nCoef)
        row[path + "_rounds"] = [len(v) for v in reduction.LAST_ROUNDS]
    print(json.dumps(row), flush=True)
    return [row]


def crossover(torch, repeats, quick):
    rows = []
    for n in (24, 48, 96, 192) if quick else (24, 48, 72, 96, 144, 192, 288, 384):
        s = refined_surface(np.random.default_rng(n), n, n // 3)
        row = dict(shape=[3, *s.nCoef], elements=int(s.coefs.size),
                   host=wall(lambda: s.remove_knots(1e-12, _path="host"), repeats, torch.cuda.synchronize),
                   device=wall(lambda: s.remove_knots(1e-12, _path="device"), repeats, torch.cuda.synchronize))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


class _TooLong(Exception):
    pass


def reference(directory, limit):
    from bspy_amd import _native
    _native.lib()                                   # before the reference's viewer modules are stubbed out
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import load_reference
    from make_golden_remove import greville, shape_functions, uniform_knots
    sys.path.insert(0, directory)
    bspy = load_reference()

    def alarm(*_):
        raise _TooLong()

    signal.signal(signal.SIGALRM, alarm)
    rows, n = [], 120
    while True:
        t = uniform_knots(4, n)
        coefs = np.stack(shape_functions(greville(t, 4)))
        ours = Spline(1, 2, [4], [n], [t], coefs)
        t0 = time.perf_counter()
        r = ours.remove_knots(1e-5, _path="host")
        row = dict(ncoef=n, host_path_seconds=time.perf_counter() - t0, host_path_ncoef=r.nCoef[0])
        ref = bspy.Spline(1, 2, [4], [n], [t], coefs)
        signal.alarm(int(limit))
        try:
            t0 = time.perf_counter()
            back = ref.remove_knots(1e-5)
            row.update(reference_seconds=time.perf_counter() - t0, reference_ncoef=int(back.nCoef[0]))
        except _TooLong:
            row.update(reference_seconds=None, note=f"abandoned after {limit} s")
        finally:
            signal.alarm(0)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if row["reference_seconds"] is None:
            return rows
        n *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference-dir", default=None)
    ap.add_argument("--reference-limit", type=float, default=60.0)
    a = ap.parse_args()
    if a.reference_dir:
        results = dict(reference=reference(a.reference_dir, a.reference_limit))
    else:
        import torch
        torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
        results = dict(kernels=kernels(torch, 512 if a.quick else 2048, a.launches, a.repeats),
                       calls=calls(torch, *((192, 64) if a.quick else (768, 256)), a.repeats),
                       crossover=crossover(torch, a.repeats, a.quick))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
