"""
Timings of Spline.project / project.project_batch.

    python tools/project_time.py [--quick] [--out project_time.json]

  calls      ``project_batch``, NumPy to arrays, on both paths over a small table of shapes, the bench surface (cfg2: 64 x 64
             bicubic, nDep 3) with 10^5 and 10^6 points among them: the host / device table behind project.DEVICE_MIN_WORK.
             The host path is skipped where points x samples is above 2 x 10^9 (minutes on one core).
  kernels    for the same shapes with everything on the device: project_seed and project_newton, each timed on its own
             (HIP events around `--launches` back-to-back calls after a warm-up), the share of each, the squared distances
             per second of the seed, and the mean and largest number of evaluations per point of the Newton kernel.
  yardstick  for the seed alone the obvious torch formulation on the same samples: ``torch.cdist(points, samples).argmin(1)``
             in float64, the points cut into blocks so that the distance matrix stays below 2 GiB.  Its indices are
             compared with the kernel's (cdist rounds differently, so equal distances may be told apart differently: the
             count of differing indices is printed, not asserted).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
from bspy_amd import Spline, project, refinement  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from refine_time import device_time, wall  # noqa: E402


def bench_surface():
    nind, ndep, order, ncoef, knots, coefs, _ = cases.bench_spline(2)
    return Spline(nind, ndep, order, ncoef, knots, coefs)


def smooth_surface(rng, n=32):
    knots = [np.concatenate((4 * [0.0], np.linspace(0, 1, n - 2)[1:-1], 4 * [1.0])) for _ in range(2)]
    gu, gv = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    coefs = np.stack([gu, gv, 0.3 * np.sin(5.0 * gu) * np.cos(4.0 * gv)]) + 0.01 * rng.standard_normal((3, n, n))
    return Spline(2, 3, [4, 4], [n, n], knots, coefs)


def curve(rng, n=64):
    knots = [np.concatenate((4 * [0.0], np.linspace(0, 1, n - 2)[1:-1], 4 * [1.0]))]
    t = np.linspace(0, 1, n)
    return Spline(1, 3, [4], [n], knots, np.stack([0.5 + 0.4 * np.cos(9.0 * t) * t, 0.5 + 0.4 * np.sin(9.0 * t) * t, 0.5 * np.cos(14.0 * t)]))


def points_for(s, rng, n):
    c = np.asarray(s.coefs, np.float64).reshape(s.nDep, -1)
    return c.mean(axis=1)[:, None] + 0.6 * c.std(axis=1)[:, None] * rng.standard_normal((s.nDep, n))


def yardstick(samples, pts):
    """argmin of torch.cdist over the same samples: samples (nDep, M), pts (nDep, N) on the device -> int64 (N)."""
    S, P = samples.t().contiguous(), pts.t().contiguous()
    block = max(1, (1 << 28) // S.shape[0])
    return torch.cat([torch.cdist(P[i:i + block], S).argmin(dim=1) for i in range(0, P.shape[0], block)])


def kernel_rows(name, s, pts, launches, repeats):
    plan = project.Plan(s.order, s.knots, tuple(int(k) for k in s.order))
    L = nv.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_pts = torch.from_numpy(pts).cuda()
    rows = torch.from_numpy(np.ascontiguousarray(s.coefs)).cuda().double()
    if plan.steps:
        rows, _ = refinement.run_device(rows, plan.steps)
    rows = rows.contiguous()
    grid = refinement.run_device(rows, plan.sample_steps)[0].contiguous()
    nDep, N = pts.shape
    M, chunk = plan.nsamples, project.SEED_CHUNK
    C = -(-M // chunk)
    d2 = torch.empty((C, N), dtype=torch.float64, device="cuda")
    idx = torch.empty((C, N), dtype=torch.int32, device="cuda")
    t_seed = device_time(lambda: nv.check(L.bsk_project_seed(nDep, grid.data_ptr(), M, d_pts.data_ptr(), N, chunk, d2.data_ptr(),
                                                             idx.data_ptr(), stream)), launches, repeats)
    tabs = [torch.from_numpy(t).cuda() for t in project._axis_tables(plan)]
    args = list(project._grid(plan, rows.data_ptr(), [t.data_ptr() for t in tabs]))
    args[3] = nDep
    uvw = torch.empty((plan.nind, N), dtype=torch.float64, device="cuda")
    dist = torch.empty(N, dtype=torch.float64, device="cuda")
    status = torch.empty(N, dtype=torch.uint8, device="cuda")
    steps = torch.empty(N, dtype=torch.int32, device="cuda")
    t_newton = device_time(lambda: nv.check(L.bsk_project_newton(*args, d_pts.data_ptr(), N, d2.data_ptr(), idx.data_ptr(), C, None,
                                                                 uvw.data_ptr(), dist.data_ptr(), status.data_ptr(), steps.data_ptr(),
                                                                 stream)), launches, repeats)
    flat = grid.reshape(nDep, M)
    t_torch = device_time(lambda: yardstick(flat, d_pts), max(1, launches // 5), repeats)
    best = torch.where(d2 == d2.min(dim=0).values[None], idx.long(), M).min(dim=0).values
    row = dict(case=name, points=N, samples=M, chunks=C, seed_seconds=t_seed, newton_seconds=t_newton,
               seed_share=t_seed[0] / (t_seed[0] + t_newton[0]), distances_per_s=N * M / t_seed[0],
               torch_cdist_argmin_seconds=t_torch, seed_over_torch=t_seed[0] / t_torch[0],
               indices_differing_from_torch=int((best != yardstick(flat, d_pts)).sum().item()),
               evaluations_mean=float(steps.float().mean().item()), evaluations_max=int(steps.max().item()),
               flagged=int(((status & project.WARN_BITS) != 0).sum().item()))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(calls=[], kernels=[])

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    shapes = [("cubic curve, 64 coefficients, nDep 3", curve(rng), [10 ** 3, 10 ** 5]),
              ("bicubic 32 x 32 smooth surface, nDep 3", smooth_surface(rng), [10 ** 3, 10 ** 5]),
              ("bench surface cfg2 (bicubic 64 x 64, nDep 3)", bench_surface(), [10 ** 3, 10 ** 4, 10 ** 5] + ([] if a.quick else [10 ** 6]))]
    for name, s, counts in shapes:
        for n in counts:
            pts = points_for(s, rng, n)
            M = project.Plan(s.order, s.knots, tuple(int(k) for k in s.order)).nsamples
            row = dict(call=f"project_batch, {name}, NumPy to arrays", points=n, samples=M,
                       device=wall(lambda: project.project_batch(s, pts, _path="device"), a.repeats))
            if n * M <= 2 * 10 ** 9:
                row["host"] = wall(lambda: project.project_batch(s, pts, _path="host"), max(1, a.repeats // 2))
            results["calls"].append(row)
            print(json.dumps(row), flush=True)
            results["kernels"].append(kernel_rows(name, s, pts, a.launches, a.repeats))
            flush()


if __name__ == "__main__":
    main()
