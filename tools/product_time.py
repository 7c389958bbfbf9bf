"""
Timings of Spline.multiply.

    python tools/product_time.py [--quick] [--out product_time.json] [--reference-seconds S]

  kernels    band_product_tile on the 512 x 512 x 3 bicubic Su x Sv ('C') and Su . Su ('D'); band_product_line on 4096
             planes of order-4 x order-4 curves with 1024 coefficients.  HIP events around `--launches` back-to-back
             launches after a warm-up; bytes in + out; the fp64 FMA count of the kernel's own scheme; and the time of a
             device-to-device copy of the same byte count (half read, half written) in the same process.
  calls      the whole NumPy-to-NumPy call for the same surfaces, and the 64 x 64 x 3 bicubic 'D' with both variables
             mapped, next to --reference-seconds (the reference's time for that call on the machine's CPU, measured
             apart: this tool does not import the reference).
  crossover  host driver against device path (with the copies in and out) for the whole call over surface sizes: what
             product.DEVICE_MIN_ELEMENTS is to be set from.
MI355X_MICROARCH.md gives the fp32 vector peak (157.3 TFLOPS) and no fp64 vector figure; the FMA rate is printed
against half of the fp32 figure, labelled as an assumption.
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
from bspy_amd import Spline, product  # noqa: E402

ASSUMED_FP64_FLOPS = 157.3e12 / 2


def jittered_knots(rng, order, ncoef):
    interior = np.linspace(0.0, 1.0, ncoef - order + 2)[1:-1]
    interior += (rng.random(ncoef - order) - 0.5) * 0.6 / (ncoef - order + 1)
    return np.concatenate((order * [0.0], interior, order * [1.0]))


def make(rng, shape, order=4, ndep=3):
    knots = [jittered_knots(rng, order, n) for n in shape]
    return Spline(len(shape), ndep, len(shape) * [order], shape, knots, rng.standard_normal((ndep, *shape)))


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


def fmas_per_output(maps, terms):
    """The kernels' own scheme, per output and term."""
    k1v, k2v = maps.k1[-1], maps.k2[-1]
    if maps.M == 1:
        per = k1v * k2v + k2v
    else:
        k1u, k2u = maps.k1[0], maps.k2[0]
        per = k1u * k1v * k2v + k1u * k2u * (k2v + 1)
    return per * terms.shape[1] + terms.shape[1]


def kernel_row(name, maps, terms, planes_a, planes_b, launches, repeats):
    a = torch.randn((planes_a, *maps.nIn1), dtype=torch.float64, device="cuda")
    b = torch.randn((planes_b, *maps.nIn2), dtype=torch.float64, device="cuda")
    t = device_time(lambda: maps.apply_device(a, b, terms), launches, repeats)
    outputs = terms.shape[0] * int(np.prod(maps.nOut))
    nbytes = 8 * (a.numel() + b.numel() + outputs)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    tc = device_time(lambda: dst.copy_(src), launches, repeats)
    fma = outputs * fmas_per_output(maps, terms)
    row = dict(case=name, kernel=maps.last_kernel(), nOut=maps.nOut, planes=int(terms.shape[0]), terms=int(terms.shape[1]),
               seconds=t, bytes=nbytes, gbytes_per_s=nbytes / t[0] * 1e-9, copy_seconds=tc, fraction_of_copy=tc[0] / t[0],
               fp64_fma=fma, tflops=2 * fma / t[0] * 1e-12, fraction_of_assumed_fp64_peak=2 * fma / t[0] / ASSUMED_FP64_FLOPS)
    print(json.dumps(row), flush=True)
    return row


def surface_maps(su, sv):
    return product.ProductMap.from_knots([(su.knots[v], su.order[v], sv.knots[v], sv.order[v]) for v in range(2)])[0]


def crossover(repeats, quick):
    rng = np.random.default_rng(3)
    rows = []
    for n in (8, 16, 32, 64) if quick else (6, 8, 12, 16, 24, 32, 48, 64, 96, 128):
        s = make(rng, (n, n))
        r = s.multiply(s, [0, 1], "D", _path="host")
        row = dict(shape=[3, n, n], result_elements=int(r.coefs.size),
                   host=wall(lambda: s.multiply(s, [0, 1], "D", _path="host"), repeats),
                   device=wall(lambda: s.multiply(s, [0, 1], "D", _path="device"), repeats))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference-seconds", type=float, default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(kernels=[], calls=[], crossover=[])

    n = 256 if a.quick else 512
    s = make(rng, (n, n))
    su, sv = s.differentiate(0), s.differentiate(1)
    maps = surface_maps(su, sv)
    terms = product.plane_table(product.dependent_terms("C", 3, 3))
    results["kernels"].append(kernel_row(f"{n} x {n} x 3 bicubic: Su x Sv", maps, terms, 3, 3, a.launches, a.repeats))
    maps.close()
    maps = surface_maps(su, su)
    terms = product.plane_table(product.dependent_terms("D", 3, 3))
    results["kernels"].append(kernel_row(f"{n} x {n} x 3 bicubic: Su . Su", maps, terms, 3, 3, a.launches, a.repeats))
    maps.close()
    planes = 1024 if a.quick else 4096
    t = jittered_knots(rng, 4, 1024)
    maps = product.ProductMap.from_knots([(t, 4, jittered_knots(rng, 4, 1024), 4)])[0]
    terms = product.plane_table(product.dependent_terms("S", 1, 1), planes, 1)
    results["kernels"].append(kernel_row(f"{planes} planes of order 4 x order 4 curves, 1024 coefficients", maps, terms, planes, 1,
                                         a.launches, a.repeats))
    maps.close()

    for label, f in ((f"{n} x {n} x 3: Su.cross(Sv), NumPy to NumPy", lambda: su.cross(sv, _path="device")),
                     (f"{n} x {n} x 3: Su.dot(Su), NumPy to NumPy", lambda: su.dot(su, _path="device"))):
        row = dict(call=label, seconds=wall(f, a.repeats))
        results["calls"].append(row)
        print(json.dumps(row), flush=True)
    small = make(rng, (64, 64))
    row = dict(call="64 x 64 x 3 bicubic: s.multiply(s, [0, 1], 'D'), NumPy to NumPy",
               device_seconds=wall(lambda: small.multiply(small, [0, 1], "D", _path="device"), a.repeats),
               host_seconds=wall(lambda: small.multiply(small, [0, 1], "D", _path="host"), a.repeats),
               reference_seconds=a.reference_seconds)
    results["calls"].append(row)
    print(json.dumps(row), flush=True)

    results["crossover"] = crossover(a.repeats, a.quick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
