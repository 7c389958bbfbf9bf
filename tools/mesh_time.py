"""
Timings of Spline.triangulate / mesh.triangulate_batch (DESIGN.md section 26 holds the tables of a run on an MI355X, from
which mesh.DEVICE_MIN_WORK is read).

    python tools/mesh_time.py [--quick] [--out mesh_time.json]

  kernels    for a bump on a plate (bicubic, 16 x 16 cells, tolerance 1e-4) and for the 64 x 64 bicubic bench surface
             (tolerance 1e-2): every launch of the driver (mesh_bound, mesh_count, mesh_emit, mesh_vertex), each timed on its
             own through the driver itself, HIP events around `--launches` back-to-back calls after a warm-up.  The
             launches write the same bytes every time.
  calls      the whole call, NumPy to mesh, on both paths, for bicubic surfaces of 2 x 2 .. 64 x 64 cells: the host /
             device crossover behind mesh.DEVICE_MIN_WORK.
  uniform    the triangles of the adaptive mesh against the uniform grid that the same bound certifies (every cell at the
             largest levels of the surface), and ``evaluate_grid_device`` of the same spline on that grid's nodes.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
from bspy_amd import Spline, _cells, mesh  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from refine_time import device_time, wall  # noqa: E402


def plate(ncells, height=0.2, width=0.08, order=(4, 4)):
    """(u, v, a Gaussian bump of ``height`` in the middle of the unit square), sampled at the Greville abscissae."""
    knots = [np.concatenate(((k - 1) * [0.0], np.linspace(0.0, 1.0, ncells + 1), (k - 1) * [1.0])) for k in order]
    greville = [np.array([t[i + 1:i + k].mean() for i in range(len(t) - k)]) for t, k in zip(knots, order)]
    x, y = np.meshgrid(*greville, indexing="ij")
    z = height * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / (2.0 * width ** 2))
    return Spline(2, 3, list(order), list(z.shape), knots, np.stack([x, y, z]))


def bench_surface():
    nind, ndep, order, ncoef, knots, coefs, _ = cases.bench_spline(2)
    return Spline(nind, ndep, list(order), list(ncoef), knots, coefs)


class Timed(_cells.Device):
    """The device backend with every launch timed on its own."""

    def __init__(self, dev, launches, repeats):
        super().__init__(dev)
        self.launches, self.repeats, self.rows = launches, repeats, []

    def call(self, name, *args):
        t = device_time(lambda: _cells.Device.call(self, name, *args), self.launches, self.repeats)
        self.rows.append((nv.lib().bsk_mesh_last_kernel().decode(), t))


def kernel_rows(name, s, tolerance, launches, repeats):
    plan = mesh.Plan(s.order, s.knots)
    _, data, rows = _cells.bezier_rows(np.asarray(s.coefs)[None], "device", plan, [])
    be = Timed(data.device, launches, repeats)
    res = mesh._run(be, rows, plan, tolerance, mesh.DEFAULT_MAX_LEVEL, True, None, mesh.DEFAULT_MAX_TRIANGLES)
    torch.cuda.synchronize()
    out = []
    for kernel, t in be.rows:
        out.append(dict(case=name, kernel=kernel, seconds=t, cells=int(np.prod(plan.ncells)), quads=res["nquads"],
                        triangles=int(len(res["triangles"])), vertices=int(len(res["keys"]))))
        print(json.dumps(out[-1]), flush=True)
    return out


def uniform_row(name, s, tolerance, repeats):
    plan = mesh.Plan(s.order, s.knots)
    out = mesh.triangulate_batch(s, tolerance, _path="device")
    lev = out[5][0]
    a, b = int(lev[..., 0].max()), int(lev[..., 1].max())
    nc0, nc1 = (int(n) for n in plan.ncells)
    axes = []
    for breaks, level in zip(plan.breaks, (a, b)):
        breaks = np.asarray(breaks, np.float64)
        x = np.arange(1 << level) / (1 << level)
        axes.append(torch.from_numpy(np.concatenate([breaks[i] + x * (breaks[i + 1] - breaks[i]) for i in range(len(breaks) - 1)] + [breaks[-1:]])).cuda())
    tables = s.device_tables()
    grid = torch.empty((s.nDep,) + tuple(len(x) for x in axes), dtype=torch.float64, device="cuda")
    t = device_time(lambda: tables.evaluate_grid_device(axes, out=grid, check=False), 3, repeats)
    row = dict(case=name, tolerance=tolerance, adaptive_triangles=int(len(out[3])), adaptive_vertices=int(len(out[1])),
               uniform_levels=[a, b], uniform_triangles=2 * nc0 * nc1 << (a + b), uniform_nodes=int(len(axes[0]) * len(axes[1])),
               evaluate_grid_device=t, kernel=tables.last_kernel(), capped=int(np.count_nonzero(out[7])))
    print(json.dumps(row), flush=True)
    return row


def call_row(name, s, tolerance, repeats):
    host = mesh.triangulate_batch(s, tolerance, _path="host")
    device = mesh.triangulate_batch(s, tolerance, _path="device")
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(host, device))
    row = dict(call=f"triangulate_batch, {name}, NumPy to mesh", cells=int(np.prod(host[5].shape[1:3])), triangles=int(len(host[3])),
               host=wall(lambda: mesh.triangulate_batch(s, tolerance, _path="host"), repeats),
               device=wall(lambda: mesh.triangulate_batch(s, tolerance, _path="device"), repeats))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(kernels=[], calls=[], uniform=[])
    big = [("bump on a plate, bicubic, 16 x 16 cells", plate(16), 1e-4)]
    if not a.quick:
        big.append(("bench surface, bicubic, 64 x 64 coefficients", bench_surface(), 1e-2))
    for name, s, tolerance in big:
        results["kernels"] += kernel_rows(name, s, tolerance, a.launches, a.repeats)
        results["uniform"].append(uniform_row(name, s, tolerance, a.repeats))
        results["calls"].append(call_row(name, s, tolerance, a.repeats))
    for ncells in (2, 4, 8, 16, 32, 64):
        results["calls"].append(call_row(f"bump on a plate, bicubic, {ncells} x {ncells} cells, tolerance 1e-3", plate(ncells), 1e-3, a.repeats))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
