"""Spline.integral on the GPU: per case the adaptive driver's rounds, final region count and nodes evaluated, the
device time of the quadrature kernels (HIP events around every bsk_integral launch, bsk_debug_stage_times) and the
wall time per call after a warm-up call.

    python tools/integral_time.py [--reps N] [--json FILE]

The numbers are quoted in DESIGN.md section 11, next to the times of BSpy's own integral on a CPU.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import cases  # noqa: E402
from bspy_amd import Spline  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from bspy_amd import integral as iq  # noqa: E402
from test_gpu_integral import affine, cfg2_surface, spline_of  # noqa: E402
from test_integral_host import annulus, golden_cases, quarter_arc  # noqa: E402


def case_list():
    bicubic8 = next(c[1] for c in golden_cases() if c[0] == "bicubic8")
    nind, ndep, order, ncoef, knots, coefs, dt = cases.bench_spline(2)
    rng = np.random.default_rng(3)
    g3 = np.meshgrid(*[np.linspace(0, 1, 5)] * 3, indexing="ij")
    g12 = np.meshgrid(np.linspace(0, 1, 12), np.linspace(0, 1, 12), indexing="ij")
    z12 = 0.2 * np.random.default_rng(8).standard_normal((12, 12))
    return [
        ("quarter arc, length", quarter_arc(), None),
        ("quarter arc, x moment (callable)", quarter_arc(), lambda x: x[0]),
        ("annulus (5,2), area", annulus(), None),
        ("annulus (5,2), x moment (callable)", annulus(), lambda x: x[0]),
        ("random bicubic 8x8, area", bicubic8, None),
        ("cfg2 height field 64x64, area", cfg2_surface(), None),
        ("cfg2 all-random 64x64, area", Spline(nind, ndep, order, ncoef, knots, coefs), None),
        ("trivariate affine (3,2,4), volume", affine((3, 2, 4), (4, 3, 5), [[2, .3, 0], [.1, 1.5, -.4], [0, .2, .7]],
                                                      [1, 0, -1], 0.0, 2.0), None),
        ("trivariate order 3 5^3, volume", spline_of((3, 3, 3), (5, 5, 5), np.stack(g3) + 0.05 * rng.standard_normal((3, 5, 5, 5))), None),
        ("bicubic 12x12 fp32, area", spline_of((4, 4), (12, 12), np.stack([g12[0], g12[1], z12]).astype(np.float32),
                                                dtype=np.float32), None),
    ]


def measure(spline, integrand, reps):
    tables = spline.device_tables()
    lib, handle = nv.lib(), tables._handle
    kernel_ms = [0.0]
    plain = tables.integral_regions

    def timed(lo_hi, span, nodes=False):
        lib.bsk_debug_stage_times(handle, 1, None, None, 0, None)
        out = plain(lo_hi, span, nodes)
        ms, names, count = (ctypes.c_float * 4)(), (ctypes.c_char_p * 4)(), ctypes.c_int(0)
        lib.bsk_debug_stage_times(handle, 0, ms, names, 4, ctypes.byref(count))
        kernel_ms[0] += sum(ms[i] for i in range(count.value))
        return out

    stats = {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        value = iq.integral(spline, integrand, stats=stats)             # warm-up
        tables.integral_regions = timed
        try:
            iq.integral(spline, integrand)
        finally:
            del tables.integral_regions
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            again = iq.integral(spline, integrand)
            walls.append(time.perf_counter() - t0)
    assert np.float64(again).tobytes() == np.float64(value).tobytes()
    note = str(caught[0].message) if caught else ""
    return dict(value=value, kernel_ms=kernel_ms[0], wall_ms=1e3 * min(walls), warning=note, **stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", help="also write the rows to this file")
    args = ap.parse_args()
    rows = []
    print(f"{'case':<38s} {'value':>22s} {'rounds':>6s} {'regions':>8s} {'nodes':>11s} {'kernels ms':>10s} {'wall ms':>9s}")
    for name, s, f in case_list():
        r = measure(s, f, args.reps)
        rows.append(dict(case=name, **r))
        print(f"{name:<38s} {r['value']:>22.16g} {r['rounds']:>6d} {r['regions']:>8d} {r['nodes']:>11d} "
              f"{r['kernel_ms']:>10.3f} {r['wall_ms']:>9.2f}" + (f"   [{r['warning']}]" if r["warning"] else ""), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1, default=lambda v: v if not isinstance(v, float) or math.isfinite(v) else None)


if __name__ == "__main__":
    main()
