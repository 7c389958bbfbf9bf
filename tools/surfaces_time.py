"""
Timings of Spline.intersect_surface / surfaces.trace_pair.

    python tools/surfaces_time.py [--quick] [--out surfaces_time.json]

  calls      ``trace_pair``, NumPy to arrays, on both paths: two bicubic surfaces of 8 x 8, 16 x 16 and 32 x 32 cells against
             each other at depths 1 - 3 (--quick: 8 x 8 and 16 x 16, depths 1 and 2): the host / device table behind
             surfaces.DEVICE_MIN_WORK, with the tested pairs, the candidates, the walk nodes and the vertices.
  kernels    for the same shapes with everything on the device: ssx_count, ssx_emit and ssx_isolate of each of the four
             families, each timed on its own (HIP events around `--launches` back-to-back calls after a warm-up) and
             summed over the families: "back_to_back".  ssx_merge runs only where a zero lies near a cell face and is
             timed where it does.
  in a call  the launches of one live call by name, each single launch between two HIP events and right behind a host
             synchronisation, summed per name over the call ("kernels"), and what is left of the call's wall time
             ("outside_kernels"): the extraction, the boxes, cumsum, the readback of the counts, allocation, the linking
             on the host.  These hold the back-to-back figures against launch latency.
  baseline   the parent commit's only way: every line's system materialised in Bezier form (lines, 3, R, RY0, RY1) through
             ``roots3.zeros3_batch`` on the device, where that fits (8 x 8 and 16 x 16 cells at depth 1), against
             ``trace_pair`` on the device.  The materialisation itself (NumPy) is not timed.
Every figure is the range (fastest, slowest) over `--repeats` runs after one warm-up.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bspy_amd import Spline, _cells, refinement, roots, roots3, surfaces  # noqa: E402
from refine_time import device_time  # noqa: E402


def wall(f, repeats):
    f()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return [min(out), max(out)]


def pair(nc, rng):
    n = nc + 3
    knots = [np.concatenate((4 * [0.0], np.linspace(0, 1, nc + 1)[1:-1], 4 * [1.0])) for _ in range(2)]
    g = np.array([knots[0][i + 1:i + 4].mean() for i in range(n)])
    gu, gv = np.meshgrid(g, g, indexing="ij")
    a = np.stack([gu, gv, 0.2 * np.sin(5.0 * gu) * np.cos(4.0 * gv) + 0.002 * rng.standard_normal((n, n))])
    b = np.stack([0.03 + 0.9 * gu + 0.05 * gv, 0.02 - 0.04 * gu + 0.95 * gv, 0.05 + 0.1 * gu - 0.12 * gv + 0.15 * np.sin(3.0 * gu + 1.0) * np.cos(2.0 * gv)])
    return Spline(2, 3, [4, 4], [n, n], knots, a), Spline(2, 3, [4, 4], [n, n], knots, b)


def kernel_times(a, b, depth, repeats):
    """The device time of every launch of one call, summed per kernel name: (name -> [min, max] seconds, launches)."""
    plain = surfaces._run
    marks = []

    def timed(be, name, *args):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        plain(be, name, *args)
        stop.record()
        marks.append((surfaces.LAST_PATHS[-1], start, stop))

    sums, count = {}, {}
    surfaces._run = timed
    try:
        for rep in range(repeats + 1):
            del marks[:]
            surfaces.trace_pair(a, b, depth=depth, _path="device")
            torch.cuda.synchronize()
            if rep == 0:
                continue
            total = {}
            for name, start, stop in marks:
                total[name] = total.get(name, 0.0) + start.elapsed_time(stop) * 1e-3
                count[name] = count.get(name, 0) + 1
            for name, t in total.items():
                sums.setdefault(name, []).append(t)
    finally:
        surfaces._run = plain
    return {name: [min(t), max(t)] for name, t in sums.items()}, {name: c // repeats for name, c in count.items()}


def back_to_back(a, b, depth, launches, repeats):
    """Seconds per launch of ssx_count, ssx_emit, ssx_isolate (and ssx_merge where it runs), events around `launches`
    back-to-back launches, summed over the four families: name -> [min, max]."""
    be = _cells.Device.current()
    tabs = []
    for s in (a, b):
        plan = surfaces.Plan(s.order, s.knots)
        rows = torch.from_numpy(np.ascontiguousarray(s.coefs)).to(be.dev).double()
        cmax = rows.abs().amax(dim=(1, 2)).cpu().numpy()
        if plan.steps:
            rows, _ = refinement.run_device(rows, plan.steps)
        tabs.append(surfaces.Tables(be, plan, rows.contiguous(), cmax))
    scale = be.put(tabs[0].cmax + tabs[1].cmax, np.float64)
    G = 1 << depth
    total = {}

    def add(name, t):
        cur = total.setdefault(name, [0.0, 0.0])
        cur[0] += t[0]
        cur[1] += t[1]

    for fam in range(4):
        X, Y = (tabs[0], tabs[1]) if fam < 2 else (tabs[1], tabs[0])
        ax = fam & 1
        ncrun, ncfix = X.plan.ncells[1 - ax], X.plan.ncells[ax]
        nseg = (ncfix * G + 1) * ncrun
        R = roots3.slots(X.plan.order[1 - ax], *Y.plan.order)
        chunk = surfaces.chunk_of(nseg, Y.ncell)
        nchunks = -(-Y.ncell // chunk)
        side = X.surface + Y.surface + (ax, G)
        with be:
            search = side + (0, nseg, chunk, 1, be.ptr(Y.boxes), be.ptr(scale))
            partial = be.empty((nseg, nchunks), np.int32)
            add("ssx_count", device_time(lambda: be.call("bsk_ssx_count", *search, be.ptr(partial)), launches, repeats))
            ends = be.cumsum(partial.reshape(-1))
            npairs = int(ends[-1])
            if not npairs:
                continue
            offset = ends - partial.reshape(-1)
            seg, cell = be.empty(npairs, np.int32), be.empty(npairs, np.int32)
            add("ssx_emit", device_time(lambda: be.call("bsk_ssx_emit", *search, be.ptr(offset), be.ptr(seg), be.ptr(cell), npairs), launches, repeats))
            out = (be.empty((npairs, R, 3), np.float64), be.empty((npairs, R), np.uint8), be.empty(npairs, np.int32), be.empty(npairs, np.uint8),
                   be.empty(npairs, np.int32))
            add("ssx_isolate", device_time(lambda: be.call("bsk_ssx_isolate", *side, be.ptr(X.breaks[1 - ax]), be.ptr(Y.breaks[0]), be.ptr(Y.breaks[1]),
                                                           be.ptr(scale), be.ptr(seg), be.ptr(cell), npairs, *map(be.ptr, out)), launches, repeats))
            which = be.nonzero(out[1])
            if len(which):
                key = be.cast(seg, np.int64) * Y.ncell + be.cast(cell, np.int64)
                keep = be.cast(~be.isnan(out[0][:, :, 0]), np.uint8)
                add("ssx_merge", device_time(lambda: be.call("bsk_ssx_merge", R, be.ptr(out[0]), ncrun, *Y.plan.ncells, be.ptr(X.breaks[1 - ax]),
                                                             be.ptr(Y.breaks[0]), be.ptr(Y.breaks[1]), be.ptr(key), len(key), be.ptr(which), len(which),
                                                             be.ptr(keep)), launches, repeats))
    return total


def materialised(a, b, depth):
    """[(system spline, coefs (lines, 3, R, RY0, RY1))] per family: coefficient (i, j, k) = L_i - Y_jk in Bezier form."""
    G = 1 << depth
    tabs = [surfaces.host_tables(s) for s in (a, b)]
    out = []
    for fam in range(4):
        ax = fam & 1
        (planX, rowsX, _), (planY, rowsY, _) = (tabs[0], tabs[1]) if fam < 2 else (tabs[1], tabs[0])
        ncfix, KR = planX.ncells[ax], planX.order[1 - ax]
        lines = []
        for n in range(ncfix * G + 1):
            c, g = surfaces.line_owner(n, G, ncfix)
            x = float(g) / float(G)
            f = int(planX.first[ax][c])
            cols = np.moveaxis(rowsX, ax + 1, -1)[:, :, f:f + planX.order[ax]]
            L = np.array([[cols[d, r, 0] if x == 0.0 else (cols[d, r, -1] if x == 1.0 else roots.value([float(v) for v in cols[d, r]], x))
                           for r in range(cols.shape[1])] for d in range(3)])
            lines.append(L[:, :, None, None] - rowsY[:, None, :, :])

        def bezier(breaks, K):
            br = np.asarray(breaks, np.float64)
            return np.concatenate(([br[0]] * K, np.repeat(br[1:-1], K - 1), [br[-1]] * K))

        knots = [bezier(planX.breaks[1 - ax], KR), bezier(planY.breaks[0], planY.order[0]), bezier(planY.breaks[1], planY.order[1])]
        coefs = np.stack(lines)
        out.append((Spline(3, 3, [KR, *planY.order], list(coefs.shape[2:]), knots, coefs[0]), coefs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    results = dict(calls=[], baseline=[])

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    for nc in (8, 16) if a.quick else (8, 16, 32):
        sa, sb = pair(nc, rng)
        for depth in (1, 2) if a.quick else (1, 2, 3):
            res = surfaces.trace_pair(sa, sb, depth=depth, _path="device")
            info = res[4]
            row = dict(call=f"trace_pair, bicubic {nc} x {nc} cells against the same, depth {depth}", tested=info["tested"],
                       candidates=info["candidates"], nodes=info["nodes"], vertices=len(info["vertices"]), pieces=len(res[1]) - 1,
                       status_bits=res[3].bits, device=wall(lambda: surfaces.trace_pair(sa, sb, depth=depth, _path="device"), a.repeats))
            if info["tested"] <= 10 ** 8:
                row["host"] = wall(lambda: surfaces.trace_pair(sa, sb, depth=depth, _path="host"), max(1, a.repeats // 2))
            row["back_to_back"] = back_to_back(sa, sb, depth, a.launches, a.repeats)
            row["kernels"], row["launches"] = kernel_times(sa, sb, depth, a.repeats)
            row["outside_kernels"] = [row["device"][0] - sum(t[0] for t in row["kernels"].values()), row["device"][1] - sum(t[1] for t in row["kernels"].values())]
            results["calls"].append(row)
            print(json.dumps(row), flush=True)
            flush()
        if nc <= 16:
            systems = materialised(sa, sb, 1)
            on_device = [(system, torch.from_numpy(coefs).cuda()) for system, coefs in systems]
            parent = wall(lambda: [roots3.zeros3_batch(system, coefs=coefs, _path="device") for system, coefs in on_device], a.repeats)
            fused = wall(lambda: surfaces.trace_pair(sa, sb, depth=1, _path="device"), a.repeats)
            row = dict(baseline=f"bicubic {nc} x {nc} cells, depth 1", system_bytes=int(sum(c.nbytes for _, c in systems)),
                       zeros3_batch_device_seconds=parent, trace_pair_device_seconds=fused, parent_over_fused=parent[0] / fused[0],
                       zeros=int(sum(int(roots3.zeros3_batch(system, coefs=coefs, _path="device")[1][-1].item()) for system, coefs in on_device)))
            results["baseline"].append(row)
            print(json.dumps(row), flush=True)
            flush()


if __name__ == "__main__":
    main()
