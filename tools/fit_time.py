"""
Timings of Spline.least_squares.

    python tools/fit_time.py [--quick] [--out fit_time.json]

  cases      whole-call wall time (data resident on the device, and from host memory), the device time of each
             variable's sweep (HIP events around bsk_fit_sweep), the bytes each sweep has to move (rows read, columns
             written, read and written again by the back-substitution; a turned sweep moves its input and output twice
             more) as a fraction of 8 TB/s, a torch.clone of the same bytes as the practical floor, and tests/fit_ref.py
             (NumPy, dense) on the same machine as the baseline
  crossover  host plan against the kernel over line counts 1 ... 10^6 for one 1024 x 260 system of order 4: kernel on
             resident data, kernel with the copy of host data in and the result out, host plan
Every figure is the range over `--repeats` runs after a warm-up.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fit_ref  # noqa: E402
from bspy_amd import Spline, collocation_matrix, fitting  # noqa: E402

PEAK = 8.0e12


def franke(x, y):
    return (0.75 * np.exp(-((9 * x - 2) ** 2 + (9 * y - 2) ** 2) / 4) + 0.75 * np.exp(-((9 * x + 1) ** 2) / 49 - (9 * y + 1) / 10)
            + 0.5 * np.exp(-((9 * x - 7) ** 2 + (9 * y - 3) ** 2) / 4) - 0.2 * np.exp(-((9 * x - 4) ** 2 + (9 * y - 7) ** 2)))


def spread(f, repeats, sync=True):
    f()
    out = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        if sync:
            torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return [min(out), max(out)]


def device_spread(f, repeats):
    f()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return [min(out), max(out)]


def sweeps(us, data, order, knots, repeats):
    """Per variable: device time of the sweep, its bytes, the clone of as many bytes."""
    rows = []
    cur, shape = data, list(data.shape)
    for iv, u in enumerate(us):
        first, values = collocation_matrix(knots[iv], order[iv], u, dense=False)
        ncols = len(knots[iv]) - order[iv]
        plan = fitting.Plan(first, values, ncols)
        outer, inner = int(np.prod(shape[:iv + 1])), int(np.prod(shape[iv + 2:]))
        lines = outer * inner
        t = device_spread(lambda: plan.sweep(cur, outer, inner), repeats)
        nbytes = lines * (shape[iv + 1] * cur.element_size() + 3 * ncols * 8)
        if plan.last_kernel() == "fit_sweep turned":
            nbytes += lines * (shape[iv + 1] * (cur.element_size() + 8) + 2 * ncols * 8)
        blob = torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")        # clone reads and writes: half each
        tc = device_spread(lambda: blob.clone(), repeats)
        rows.append(dict(variable=iv, kernel=plan.last_kernel(), lines=lines, nrows=shape[iv + 1], ncols=ncols, seconds=t,
                         bytes=nbytes, roofline_fraction=nbytes / PEAK / t[0], clone_seconds=tc))
        cur = plan.sweep(cur, outer, inner)
        shape[iv + 1] = ncols
        del blob
    return rows


def case(name, us, data, repeats, baseline=True, **kw):
    order = kw.pop("order", [4] * len(us))
    arg = us if len(us) > 1 else us[0]
    td = torch.as_tensor(data, device="cuda")
    out = dict(name=name, shape=list(data.shape))
    out["wall_resident"] = spread(lambda: Spline.least_squares(arg, td, order, **kw), repeats)
    s = Spline.least_squares(arg, td, order, **kw)
    out["paths"], out["ncoef"] = list(fitting.LAST_PATHS), list(s.nCoef)
    out["wall_from_host"] = spread(lambda: Spline.least_squares(arg, data, order, **kw), repeats)
    if kw.get("tolerance") is None and all(p.startswith("fit_sweep") for p in out["paths"]):
        out["sweeps"] = sweeps(us, td, order, s.knots, repeats)
    if baseline:
        out["numpy_baseline"] = spread(lambda: fit_ref.fit(us, data, order, compression=kw.get("compression", 0.0),
                                                           tolerance=kw.get("tolerance")), 1, sync=False)
    print(json.dumps(out), flush=True)
    return out


def crossover(repeats, quick):
    rng = np.random.default_rng(1)
    u = np.linspace(0.0, 1.0, 1024)
    knots = fitting.auto_knots(u, 4, 0.75)
    first, values = collocation_matrix(knots, 4, u, dense=False)
    plan = fitting.Plan(first, values, len(knots) - 4)
    rows = []
    for lines in (1, 4, 16, 64, 256, 1024, 4096, 16384, 65536, 262144, 1000000):
        if quick and lines > 65536:
            break
        b = rng.standard_normal((1, 1024, lines))
        tb = torch.as_tensor(b, device="cuda")
        row = dict(lines=lines, kernel_resident=device_spread(lambda: plan.sweep(tb, 1, lines), repeats),
                   kernel_with_copies=spread(lambda: plan.sweep(torch.from_numpy(b).cuda(), 1, lines).cpu(), repeats))
        if lines <= 16384:
            row["host_plan"] = spread(lambda: plan.solve_host(b, 1, lines), min(repeats, 3), sync=False)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(cases=[], crossover=[])
    for n in (1024,) if a.quick else (1024, 2048):
        u = np.linspace(0.0, 1.0, n)
        f = franke(u[:, None], u[None, :])
        data = np.stack([f, 2.0 * f.T, 1.0 - f]) + 0.01 * rng.standard_normal((3, n, n))
        results["cases"].append(case(f"{n}^2 x 3, compression 0.75", [u, u], data, a.repeats, compression=0.75))
    if not a.quick:
        u = np.linspace(0.0, 1.0, 256)
        g = np.meshgrid(u, u, u, indexing="ij")
        vol = (np.sin(5 * g[0]) * np.cos(3 * g[1]) + g[2] ** 2)[None] + 0.01 * rng.standard_normal((1, 256, 256, 256))
        results["cases"].append(case("256^3 x 1, compression 0.75", [u, u, u], vol, a.repeats, compression=0.75))
        uc = np.sort(rng.random(1_000_000))
        curve = np.stack([np.sin(20 * uc), np.cos(13 * uc), uc ** 2]) + 0.01 * rng.standard_normal((3, 1_000_000))
        results["cases"].append(case("10^6-point curve, nDep 3, compression 0.75", [uc], curve, 2, baseline=False, compression=0.75))
    u = np.linspace(0.0, 1.0, 101)
    results["cases"].append(case("Franke 101 x 101, tolerance 1e-4", [u, u], franke(u[:, None], u[None, :])[None], a.repeats, tolerance=1e-4))
    results["crossover"] = crossover(a.repeats, a.quick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
