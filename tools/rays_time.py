"""
Timings of Spline.intersect_rays / rays.cast_batch.

    python tools/rays_time.py [--quick] [--out rays_time.json]

  calls      ``cast_batch`` (hits="first"), NumPy to arrays, on both paths: bicubic graph surfaces of 16 x 16 and 64 x 64 cells,
             N = 10^3 .. 10^6 rays from above (--quick: up to 10^5): the host / device table behind rays.DEVICE_MIN_WORK.  The
             host path is skipped where rays x cells is above 10^9.
  kernels    for the same shapes with everything on the device: ray_count, ray_emit, ray_isolate, ray_reduce, each timed on
             its own (HIP events around `--launches` back-to-back calls after a warm-up), the candidates per ray, and
             ray_count on the same rays moved off the surface, where every pair fails the box test: the box tests' share of
             ray_count (the rest is forming coefficients and the sign tests of the pairs that pass).
  baseline   the parent commit's only way: materialised systems (N, 2, n0, n1) through ``roots2.zeros2_batch`` on the device,
             at 1024 rays, against ``cast_batch(hits="all", tmin=-inf)`` on the same rays.
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
from bspy_amd import Spline, _cells, rays, refinement, roots2  # noqa: E402
from refine_time import device_time, wall  # noqa: E402


def surface(nc, rng):
    n = nc + 3
    knots = [np.concatenate((4 * [0.0], np.linspace(0, 1, nc + 1)[1:-1], 4 * [1.0])) for _ in range(2)]
    g = np.array([knots[0][i + 1:i + 4].mean() for i in range(n)])
    gu, gv = np.meshgrid(g, g, indexing="ij")
    return Spline(2, 3, [4, 4], [n, n], knots, np.stack([gu, gv, 0.2 * np.sin(5.0 * gu) * np.cos(4.0 * gv) + 0.002 * rng.standard_normal((n, n))]))


def rays_for(rng, N):
    target = np.stack([rng.uniform(0.0, 1.0, N), rng.uniform(0.0, 1.0, N), np.zeros(N)])
    d = np.stack([0.3 * rng.standard_normal(N), 0.3 * rng.standard_normal(N), -np.ones(N)])
    return target - 3.0 * d, d


def kernel_rows(name, s, o, d, launches, repeats):
    plan = rays.Plan(s.order, s.knots)
    rows = torch.from_numpy(np.ascontiguousarray(s.coefs)).cuda().double()
    cmax = rows.abs().amax(dim=(1, 2)).cpu().numpy()
    if plan.steps:
        rows, _ = refinement.run_device(rows, plan.steps)
    be = _cells.Device.current()
    tab = rays.Tables(be, plan, rows.contiguous(), cmax)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    away = d_o.clone()
    away[0] += 50.0
    N = o.shape[1]
    res = rays.run_pass(tab, d_o, d_d, 0.0, rays.INF)
    R = roots2.slots(*plan.order)
    nchunks = -(-tab.ncell // rays.CHUNK)
    with be:
        ray = (be.ptr(tab.dcmax), be.ptr(d_o), be.ptr(d_d), N)
        search = tab.surface + ray + (0.0, rays.INF, rays.CHUNK, 1, be.ptr(tab.boxes))
        miss = tab.surface + (be.ptr(tab.dcmax), be.ptr(away), be.ptr(d_d), N) + (0.0, rays.INF, rays.CHUNK, 1, be.ptr(tab.boxes))
        t_count = device_time(lambda: be.call("bsk_rays_count", *search, be.ptr(res["partial"]), be.ptr(res["skipped"])), launches, repeats)
        scratch = torch.empty_like(res["partial"])
        t_boxes = device_time(lambda: be.call("bsk_rays_count", *miss, be.ptr(scratch), be.ptr(res["skipped"])), launches, repeats)
        npairs = res["npairs"]
        ends = be.cumsum(res["partial"].reshape(-1))
        offset = ends - res["partial"].reshape(-1)
        pstart = torch.cat((offset.reshape(N, nchunks)[:, 0], ends[-1:]))
        t_emit = device_time(lambda: be.call("bsk_rays_emit", *search, be.ptr(offset), be.ptr(res["pair_ray"]), be.ptr(res["pair_cell"]), npairs),
                             launches, repeats)
        head = tab.surface + tuple(be.ptr(b) for b in tab.breaks) + ray
        t_isolate = device_time(lambda: be.call("bsk_rays_isolate", *head, be.ptr(res["pair_ray"]), be.ptr(res["pair_cell"]), npairs,
                                                be.ptr(res["roots"]), be.ptr(res["near"]), be.ptr(res["count"]), be.ptr(res["status"]),
                                                be.ptr(res["nodes"])), launches, repeats)
        t_reduce = device_time(lambda: be.call("bsk_rays_reduce", *head, 0.0, rays.INF, be.ptr(pstart), be.ptr(res["pair_cell"]), npairs,
                                               be.ptr(res["roots"]), be.ptr(res["near"]), be.ptr(res["count"]), be.ptr(res["status"]),
                                               be.ptr(res["skipped"]), 0, None, 0, be.ptr(res["uv"]), be.ptr(res["t"]), be.ptr(res["cell"]),
                                               be.ptr(res["hits"]), be.ptr(res["rstatus"])), launches, repeats)
    row = dict(case=name, rays=N, cells=tab.ncell, chunks=nchunks, slots=R, candidates_per_ray=npairs / N,
               count_seconds=t_count, count_all_boxes_missed_seconds=t_boxes, box_share_of_count=t_boxes[0] / t_count[0],
               emit_seconds=t_emit, isolate_seconds=t_isolate, reduce_seconds=t_reduce,
               box_tests_per_s=N * tab.ncell / t_count[0], nodes_mean=float(res["nodes"].float().mean().item()),
               nodes_max=int(res["nodes"].max().item()), hits=int((res["hits"] > 0).sum().item()),
               flagged=int((res["rstatus"] != 0).sum().item()))
    print(json.dumps(row), flush=True)
    return row


def baseline(name, s, o, d, repeats):
    """Materialised systems through zeros2_batch on the device, the parent's pipeline, against the fused family."""
    data = np.asarray(s.coefs, np.float64)
    cmax = np.abs(data).max(axis=(1, 2))
    g = np.empty((o.shape[1], 2) + data.shape[1:])
    for ray in range(o.shape[1]):
        fr = rays.frame(o[:, ray], d[:, ray], cmax)
        for k, (p, q, w0, w1) in enumerate(fr.terms):
            g[ray, k] = w0 * (data[p] - fr.o[p]) + w1 * (data[q] - fr.o[q])
    system = Spline(2, 2, list(s.order), list(s.nCoef), s.knots, np.zeros((2,) + tuple(s.nCoef)))
    d_g, d_o, d_d = torch.from_numpy(g).cuda(), torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    t_parent = wall(lambda: roots2.zeros2_batch(system, coefs=d_g, _path="device"), repeats)
    t_fused = wall(lambda: rays.cast_batch(s, d_o, d_d, tmin=-rays.INF, hits="all"), repeats)
    zeros = int(roots2.zeros2_batch(system, coefs=d_g, _path="device")[1][-1].item())
    hits = int(rays.cast_batch(s, d_o, d_d, tmin=-rays.INF, hits="all")[2][-1].item())
    row = dict(baseline=name, rays=o.shape[1], system_bytes=g.nbytes, zeros2_batch_device_seconds=t_parent, cast_batch_device_seconds=t_fused,
               parent_over_fused=t_parent[0] / t_fused[0], zeros=zeros, hits=hits)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(calls=[], kernels=[], baseline=[])

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    for nc in (16, 64):
        s = surface(nc, rng)
        name = f"bicubic graph surface, {nc} x {nc} cells"
        for N in [10 ** 3, 10 ** 4, 10 ** 5] + ([] if a.quick else [10 ** 6]):
            o, d = rays_for(rng, N)
            row = dict(call=f"cast_batch first, {name}, NumPy to arrays", rays=N, cells=nc * nc,
                       device=wall(lambda: rays.cast_batch(s, o, d, _path="device"), a.repeats))
            if N * nc * nc <= 10 ** 9:
                row["host"] = wall(lambda: rays.cast_batch(s, o, d, _path="host"), max(1, a.repeats // 2))
            results["calls"].append(row)
            print(json.dumps(row), flush=True)
            results["kernels"].append(kernel_rows(name, s, o, d, a.launches, a.repeats))
            flush()
        o, d = rays_for(rng, 1024)
        results["baseline"].append(baseline(name, s, o, d, a.repeats))
        flush()


if __name__ == "__main__":
    main()
