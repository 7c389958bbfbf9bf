"""
Timings of Spline.isosurface / isosurface.extract_batch (DESIGN.md section 25 holds the tables of a run on an MI355X, from
which isosurface.DEVICE_MIN_LEAVES is read).

    python tools/iso_time.py [--quick] [--out iso_time.json]

  kernels    for a tricubic float64 field (a wavy sphere: the surface meets a thin shell of the cells) on 1 cell at depth 6
             and on 16^3 and 32^3 cells at depth 3: every launch of the driver (iso_flag, iso_walk count / emit, iso_leaf
             count / emit, iso_vertex), each timed on its own through the driver itself, HIP events around `--launches`
             back-to-back calls after a warm-up.  The launches write the same bytes every time.
  calls      the whole call, NumPy to mesh, on both paths: the host / device crossover behind isosurface.DEVICE_MIN_LEAVES.
  dense      what the code needed before it could march at all: ``evaluate_grid_device`` of the same spline on all nodes
             of the same lattice (no marching, no vertices), events around the call.
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
from bspy_amd import Spline, _cells, isosurface  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from refine_time import device_time, wall  # noqa: E402


def make(ncells, order=(4, 4, 4)):
    """|x - c| - r with waves (r = 0.35; one cell: 0.6, what four coefficients an axis can hold), sampled at the Greville
    abscissae of uniform knots: close enough to a sphere."""
    knots = [np.concatenate(((k - 1) * [0.0], np.linspace(0.0, 1.0, ncells + 1), (k - 1) * [1.0])) for k in order]
    greville = [np.array([t[i + 1:i + k].mean() for i in range(len(t) - k)]) for t, k in zip(knots, order)]
    x, y, z = np.meshgrid(*greville, indexing="ij")
    coefs = np.sqrt((x - 0.47) ** 2 + (y - 0.52) ** 2 + (z - 0.49) ** 2) - (0.35 if ncells > 1 else 0.6) + 0.02 * np.sin(9.0 * x) * np.sin(7.0 * y) * np.sin(8.0 * z)
    return Spline(3, 1, list(order), list(coefs.shape), knots, coefs[None])


class Timed(_cells.Device):
    """The device backend with every launch timed on its own."""

    def __init__(self, dev, launches, repeats):
        super().__init__(dev)
        self.launches, self.repeats, self.rows = launches, repeats, []

    def call(self, name, *args):
        t = device_time(lambda: _cells.Device.call(self, name, *args), self.launches, self.repeats)
        self.rows.append((nv.lib().bsk_iso_last_kernel().decode(), t))


def kernel_rows(name, s, depth, launches, repeats):
    plan = isosurface.Plan(s.order, s.knots)
    _, data, rows = _cells.bezier_rows(s.coefs, "device", plan, [])
    be = Timed(data.device, launches, repeats)
    res = isosurface._run(be, rows, plan, None, _cells.field_scale(be, data), depth, None)
    torch.cuda.synchronize()
    out = []
    for kernel, t in be.rows:
        out.append(dict(case=name, kernel=kernel, seconds=t, split=res["split"], candidates=int(res["cand"].sum()), leaves=res["nleaves"],
                        triangles=int(len(res["triangles"])), vertices=int(len(res["keys"]))))
        print(json.dumps(out[-1]), flush=True)
    return out


def dense_row(name, s, depth, repeats):
    plan = isosurface.Plan(s.order, s.knots)
    G = 1 << depth
    axes = []
    for b in plan.breaks:
        b = np.asarray(b, np.float64)
        x = np.arange(G) / G
        axes.append(torch.from_numpy(np.concatenate([(1.0 - x) * b[i] + x * b[i + 1] for i in range(len(b) - 1)] + [b[-1:]])).cuda())
    tables = s.device_tables()
    out = torch.empty((1,) + tuple(len(a) for a in axes), dtype=torch.float64, device="cuda")
    t = device_time(lambda: tables.evaluate_grid_device(axes, out=out, check=False), 3, repeats)
    row = dict(case=name, kernel="evaluate_grid_device on all lattice nodes: " + tables.last_kernel(), seconds=t, nodes=int(out.numel()),
               bytes=int(out.numel()) * 8)
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
    results = dict(kernels=[], calls=[], dense=[])
    for ncells, depth in [(1, 6), (16, 3)] + ([] if a.quick else [(32, 3)]):
        s = make(ncells)
        name = f"tricubic, {ncells}^3 cells, depth {depth}"
        results["kernels"] += kernel_rows(name, s, depth, a.launches, a.repeats)
        results["dense"].append(dense_row(name, s, depth, a.repeats))
    for ncells, depth in [(1, 3), (2, 3), (4, 3), (8, 3), (1, 6), (16, 3)] + ([] if a.quick else [(32, 3)]):
        s = make(ncells)
        host = isosurface.extract_batch(s, depth=depth, _path="host")
        device = isosurface.extract_batch(s, depth=depth, _path="device")
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(host, device))
        row = dict(call=f"extract_batch, tricubic, {ncells}^3 cells, depth {depth}, NumPy to mesh", leaves=ncells ** 3 << (3 * depth),
                   triangles=int(len(host[3])),
                   host=wall(lambda: isosurface.extract_batch(s, depth=depth, _path="host"), a.repeats),
                   device=wall(lambda: isosurface.extract_batch(s, depth=depth, _path="device"), a.repeats))
        results["calls"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
