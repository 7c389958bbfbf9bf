"""
Timings of Spline.fit_points / scatter.fit_batch.

    python tools/scatter_time.py [--quick] [--solves] [--out scatter_time.json]

  calls      ``fit_batch`` on both paths, NumPy in, for 10^4 .. 10^7 points on the bench surface's shape (cfg2: 64 x 64
             bicubic, nDep 3) and on a cubic curve of 64 coefficients, nDep 3: the host / device table behind
             scatter.DEVICE_MIN_WORK.  The host path is skipped above 10^6 points.
  stages     the assembly with everything on the device, each stage between HIP events on the stream: scatter_key, the sort
             (``be.lexsort`` and ``be.searchsorted``), scatter_gram, scatter_cell (all levels), scatter_fold; and, on the host,
             the solve.
  yardstick  the same stencil and right-hand side formed by ``torch.index_add_`` on the device from the same basis values
             (float atomics: not reproducible, the sums differ in the last bits); the largest difference from the kernels'
             stencil relative to its largest entry is printed, not asserted.
  solves     (``--solves``: this table alone) the banded solve of 16^2, 32^2, 64^2 and 128^2 bicubic coefficients, a 48 x 48
             surface of orders (3, 4) and cubic curves of 64 and 4096 coefficients, nDep 3, from 10^5 points:
             ``bsk_scatter_solve`` stage by stage between HIP events (``bsk_debug_scatter_solve``: the band expansion, the
             factorisation, the forward and the backward substitution) and whole, ``bsk_scatter_solve_host`` in the same run,
             and a robust call (Huber, 8 rounds, NumPy in, device path) with each solve.  The table behind
             scatter.SOLVE_MIN_WORK.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
from bspy_amd import _native as nv  # noqa: E402
from bspy_amd import scatter  # noqa: E402
from refine_time import wall  # noqa: E402


class Timed(scatter.Device):
    """``scatter.Device`` with HIP events around every entry point and around the sort."""

    def __init__(self, dev):
        super().__init__(dev)
        self.marks = []

    def _timed(self, name, f, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = f(*args)
        b.record()
        self.marks.append((name, a, b))
        return out

    def call(self, name, *args):
        return self._timed(name[len("bsk_"):], super().call, name, *args)

    def lexsort(self, columns):
        return self._timed("sort", super().lexsort, columns)

    def searchsorted(self, a, n):
        return self._timed("sort", super().searchsorted, a, n)

    def seconds(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.marks:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b) * 1e-3
        self.marks = []
        return out


def torch_basis(K, t, mu, u):
    """(N, K): Cox-de Boor on the device, vectorised over the points; t the knots, mu the spans (int64)."""
    b = [torch.ones_like(u)]
    for j in range(1, K):
        saved = torch.zeros_like(u)
        for r in range(j):
            tr, tl = t[mu + 1 + r], t[mu + 1 + r - j]
            temp = b[r] / (tr - tl)
            b[r] = saved + (tr - u) * temp
            saved = (u - tl) * temp
        b.append(saved)
    return torch.stack(b, dim=1)


def yardstick(sh, knots, uvw, pts, w, key, block=1 << 18):
    """The stencil and the right-hand side by torch.index_add_ (atomic adds), from the keys the kernels made; the points in
    blocks, so that the K x K products of a block stay below 1 GiB."""
    K0, K1 = sh.K01
    n0, n1 = sh.n01
    nc1 = n1 - K1 + 1
    S1, NS = 2 * K1 - 1, (2 * K0 - 1) * (2 * K1 - 1)
    stencil = torch.zeros(n0 * n1 * NS, dtype=torch.float64, device=key.device)
    rhs = torch.zeros((n0 * n1, pts.shape[0]), dtype=torch.float64, device=key.device)
    a0, a1 = torch.arange(K0, device=key.device), torch.arange(K1, device=key.device)
    for at in range(0, len(key), block):
        k, u, p = key[at:at + block], uvw[:, at:at + block], pts[:, at:at + block]
        c0, c1 = k // nc1, k % nc1
        B = torch_basis(K0, knots[0], c0 + K0 - 1, u[0])
        i0, i1 = c0[:, None] + a0[None], torch.zeros_like(c0)[:, None].expand(-1, K0)
        if sh.nind == 2:
            Bv = torch_basis(K1, knots[1], c1 + K1 - 1, u[1])
            B = (B[:, :, None] * Bv[:, None, :]).reshape(len(k), -1)
            i0 = (c0[:, None] + a0[None])[:, :, None].expand(-1, -1, K1).reshape(len(k), -1)
            i1 = (c1[:, None] + a1[None])[:, None, :].expand(-1, K0, -1).reshape(len(k), -1)
        T = w[at:at + block, None] * B
        e = (i0[:, None, :] - i0[:, :, None] + K0 - 1) * S1 + (i1[:, None, :] - i1[:, :, None] + K1 - 1)
        dest = ((i0 * n1 + i1)[:, :, None] * NS + e).reshape(-1)
        stencil.index_add_(0, dest, (T[:, :, None] * B[:, None, :]).reshape(-1))
        rhs.index_add_(0, (i0 * n1 + i1).reshape(-1), (T[:, :, None] * p.t()[:, None, :]).reshape(-1, pts.shape[0]))
    return stencil.reshape(n0 * n1, NS), rhs


def spread(rows):
    return {k: [min(r[k] for r in rows), max(r[k] for r in rows)] for k in rows[0]}


def clamped(order, ncoef):
    return [np.concatenate(((k - 1) * [0.0], np.linspace(0, 1, n - k + 2), (k - 1) * [1.0])) for k, n in zip(order, ncoef)]


def solves(repeats, out):
    """The table of the solves: one JSON line per shape."""
    import ctypes
    rng = np.random.default_rng(1)
    L = nv.lib()
    shapes = [(f"bicubic {m} x {m}", (4, 4), (m, m)) for m in (16, 32, 64, 128)]
    shapes += [("orders (3, 4), 48 x 48", (3, 4), (48, 48)), ("cubic curve, 64", (4,), (64,)), ("cubic curve, 4096", (4,), (4096,))]
    results = []
    for name, order, ncoef in shapes:
        knots = clamped(order, ncoef)
        sh = scatter.Shape(order, knots)
        n, nDep = 10 ** 5, 3
        uvw, pts = rng.random((len(order), n)), rng.standard_normal((nDep, n))
        be = scatter.Device.current()
        res = scatter.assemble(be, sh, *[torch.from_numpy(x).cuda() for x in (uvw, pts)], None)
        E = scatter.penalty_stencil(order, knots, 1)
        stencil = (res["stencil"] + torch.from_numpy(E).cuda() * 1e-6).contiguous()
        rhs = res["rhs"]
        hb = scatter.half_bandwidth(sh)
        row = dict(case=name, n=sh.n, hb=hb, work=sh.n * hb * hb)
        need = np.zeros(1, np.int64)
        nv.check(L.bsk_scatter_solve_work(sh.nind, *sh.K01, *sh.n01, nDep, need.ctypes.data_as(nv._i64p)))
        work = torch.empty(int(need[0]), dtype=torch.float64, device="cuda")
        coefs, bad = torch.empty((nDep, sh.n), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def stage(mask):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            nv.check(L.bsk_debug_scatter_solve(sh.nind, *sh.K01, *sh.n01, nDep, stencil.data_ptr(), rhs.data_ptr(), coefs.data_ptr(),
                                               work.data_ptr(), int(need[0]), bad.data_ptr(), mask, stream))
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3

        stage(15)
        runs = [dict(band=stage(1), factor=stage(2), forward=stage(4), backward=stage(8), device_solve=stage(15)) for _ in range(repeats)]
        assert int(bad.cpu()[0]) == -1
        row.update(spread(runs))
        hs, hr = stencil.cpu().numpy(), rhs.cpu().numpy()
        host = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            want = scatter.solve(sh, hs, hr)
            host.append(time.perf_counter() - t0)
        row["host_solve"] = [min(host), max(host)]
        row["same_bytes"] = bool(np.array_equal(want.view(np.int64), coefs.cpu().numpy().view(np.int64)))
        pts[:, ::10] += 50.0
        for where in ("device", "host"):
            row[f"robust_{where}_solve"] = wall(lambda: scatter.fit_batch(uvw, pts, order, knots, smoothing=1e-6, penalty=1, robust="huber",
                                                                         solve=where, _path="device"), repeats)
        results.append(row)
        print(json.dumps(row), flush=True)
        if out:
            with open(out, "w") as f:
                json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--solves", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.zeros(1 << 24, device="cuda").sum().item()                 # clocks up
    if a.solves:
        return solves(a.repeats, a.out)
    _, _, order2, ncoef2, knots2, _, _ = cases.bench_spline(2)
    curve_knots = [np.concatenate((4 * [0.0], np.linspace(0, 1, 62)[1:-1], 4 * [1.0]))]
    shapes = [("bench surface cfg2 (bicubic 64 x 64, nDep 3)", tuple(order2), [np.asarray(k, np.float64) for k in knots2]),
              ("cubic curve, 64 coefficients, nDep 3", (4,), curve_knots)]
    counts = [10 ** 4, 10 ** 5] + ([10 ** 6] if a.quick else [10 ** 6, 10 ** 7])
    results = []
    for name, order, knots in shapes:
        sh = scatter.Shape(order, knots)
        for n in counts:
            uvw = rng.random((len(order), n))
            pts = rng.standard_normal((3, n))
            w = rng.random(n)
            row = dict(case=name, points=n, device=wall(lambda: scatter.fit_batch(uvw, pts, order, knots, weights=w, _path="device"), a.repeats))
            if n <= 10 ** 6:
                row["host"] = wall(lambda: scatter.fit_batch(uvw, pts, order, knots, weights=w, _path="host"), max(1, a.repeats // 2))
            be = Timed(torch.device("cuda", torch.cuda.current_device()))
            d = [torch.from_numpy(x).cuda() for x in (uvw, pts, w)]
            scatter.assemble(be, sh, *d)
            be.seconds()
            stages = []
            for _ in range(a.repeats):
                res = scatter.assemble(be, sh, *d)
                stages.append(be.seconds())
            row["stages"] = spread(stages)
            stencil, rhs = res["stencil"].cpu().numpy(), res["rhs"].cpu().numpy()
            t0 = time.perf_counter()
            scatter.solve(sh, stencil, rhs)
            row["solve_host"] = time.perf_counter() - t0
            tk = [torch.from_numpy(k).cuda() for k in sh.knots]
            ok = res["key"] >= 0
            both = []
            for _ in range(a.repeats + 1):
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                ys, yr = yardstick(sh, tk, d[0][:, ok], d[1][:, ok], d[2][ok], res["key"][ok])
                s1.record()
                s1.synchronize()
                both.append(s0.elapsed_time(s1) * 1e-3)
            row["torch_index_add"] = [min(both[1:]), max(both[1:])]
            row["index_add_difference"] = float((ys - res["stencil"]).abs().max() / res["stencil"].abs().max())
            results.append(row)
            print(json.dumps(row), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
