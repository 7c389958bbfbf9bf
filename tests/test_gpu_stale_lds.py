"""
Results must not depend on what an earlier dispatch left in LDS.

Every kernel family that uses LDS runs the same call three times with device-resident inputs on torch's current stream:
once as it comes, once after bsk_debug_fill_lds has written 0xFFFFFFFF over the whole LDS of every CU (NaN in fp32 and
fp64), and once after 0x7F7F7F7F (finite and huge in both).  The three results must be bitwise equal (raw bytes: NaN
compares unequal to itself), and the first one matches the CPU oracle on a sample.  A kernel that reads a word of LDS it
never wrote - even one it multiplies by a zero weight - turns NaN or huge here.

The module starts with the positive control: a fill, then a dispatch that reads the whole LDS without writing it.  If a
later dispatch does not see what an earlier one left there, the sweep would prove nothing and the module is skipped
with that finding.
"""
import ctypes
import os

import numpy as np
import pytest

import cases
import oracle
import bspy_amd
from bspy_amd import DeviceSpline, Spline
from bspy_amd import _native as nv
from bspy_amd import integral as iq
from conftest import observe
from integral_ref import region_sums

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS = 0xFFFFFFFF          # NaN as fp32 and as fp64
HUGE_BITS = 0x7F7F7F7F         # 3.39e38 as fp32, 1.4e306 as fp64
CASES = {c.name: c for c in cases.parity_cases()}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fill(t, pattern):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, _stream()))


def _mismatches(t, pattern):
    miss = ctypes.c_int64(-1)
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 1, ctypes.byref(miss), _stream()))
    return miss.value


_CONTROL = {}


def _control():
    """(LDS survives between dispatches, what was seen)."""
    if not _CONTROL:
        t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
        seen = []
        for pattern in (0x5A5A5A5A, 0xA5A5A5A5):
            _fill(t, pattern)
            seen.append((pattern, _mismatches(t, pattern), _mismatches(t, pattern ^ 0xFFFFFFFF)))
        ok = all(same == 0 and other > 0 for _, same, other in seen)
        _CONTROL["result"] = (ok, "; ".join(f"fill {p:#010x}: {s} words differ on reading it back, {o} against its complement"
                                            for p, s, o in seen))
    return _CONTROL["result"]


@pytest.fixture(autouse=True)
def _lds_survives(request):
    ok, seen = _control()
    if not ok:
        pytest.skip(f"LDS does not survive between dispatches on this device ({seen}): the sweep would prove nothing")


def test_lds_fill_control():
    """Positive control: the words a dispatch reads without writing are the words the fill left (and the check counts
    every word that differs: a pattern's complement differs everywhere)."""
    ok, seen = _control()
    print("LDS control:", seen)
    assert ok, seen


def _kernel_ok(got, want):
    return got == want if not want.endswith("*") else want[:-1] in got


def _bytes(x):
    if isinstance(x, (tuple, list)):
        return b"".join(_bytes(v) for v in x)
    if torch.is_tensor(x):
        x = x.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(x).tobytes()


def _poisoned_runs(t, call, kernel, what):
    """call() three times: as it comes, after a NaN fill, after a huge fill of every CU's LDS; bitwise the same results.
    `kernel`: the family last_kernel() must name (a trailing * matches a part of it).  Returns the first result."""
    torch.cuda.synchronize()
    first = call()
    torch.cuda.synchronize()
    assert _kernel_ok(t.last_kernel(), kernel), (what, t.last_kernel())
    ref = _bytes(first)
    for pattern in (NAN_BITS, HUGE_BITS):
        _fill(t, pattern)
        out = call()
        torch.cuda.synchronize()
        assert _kernel_ok(t.last_kernel(), kernel), (what, t.last_kernel())
        got = _bytes(out)
        if got != ref:
            a = np.frombuffer(ref, np.uint8).reshape(-1, 4)
            b = np.frombuffer(got, np.uint8).reshape(-1, 4)
            nbad = int((a != b).any(axis=1).sum())
            pytest.fail(f"{what} [{t.last_kernel()}]: result changed after filling LDS with {pattern:#010x} "
                        f"({nbad} of {len(a)} 32-bit words differ)")
    return first


def _sample(n, rng, k=20_000):
    return np.unique(np.concatenate((np.arange(min(n, 2_000)), rng.integers(0, n, k), np.arange(max(0, n - 4_000), n))))


def _points(order, ncoef, knots, n, dt, rng):
    """Random points; every knot and +-1 ulp in random order at the front; a block of points in the LAST span of every
    variable, and the top corner of the domain, at the end (a read past a table's end happens only there)."""
    pts = []
    for k, o, c in zip(knots, order, ncoef):
        lo, hi = dt(k[o - 1]), dt(k[c])
        p = (lo + (hi - lo) * rng.random(n)).astype(dt)
        d = np.unique(k).astype(dt)
        e = np.concatenate((d, np.nextafter(d, dt(-np.inf)), np.nextafter(d, dt(np.inf)))).astype(dt)
        e = e[(e >= lo) & (e <= hi)]
        p[:len(e)] = rng.permutation(e)
        last_lo = dt(k[c - 1])
        p[n - 3_001: n - 1] = (last_lo + (hi - last_lo) * rng.random(3_000)).astype(dt)
        p[n - 1] = hi
        pts.append(np.clip(p, lo, hi).astype(dt))
    return pts


def _tol(dt):
    return 2e-5 if dt == np.float32 else 1e-12


def _scale(ref):
    return max(1.0, float(np.max(np.abs(ref))))


def _kind(dt):
    return "fp32" if dt == np.float32 else "fp64"


def _make(order, ncoef, knots, coefs, dt, monkeypatch=None, variant=None):
    if variant is not None:
        monkeypatch.setenv("BSK_VARIANT", variant)
    try:
        return DeviceSpline(order, ncoef, knots, coefs, dt)
    finally:
        if variant is not None:
            monkeypatch.delenv("BSK_VARIANT")


def _sweep_points(t, spec, pts, calls, label, rng):
    """calls: (kind, wrt, kernel) with kind in eval / jac / normal / curv; each through _poisoned_runs, then the oracle."""
    order, ncoef, knots, coefs, dt = spec
    tp = [torch.as_tensor(p, device="cuda") for p in pts]
    n = len(pts[0])
    idx = _sample(n, rng)
    sub = [p[idx] for p in pts]
    for kind, w, kernel in calls:
        if kind == "eval":
            f = lambda: t.evaluate_device(tp, list(w))                  # noqa: E731
        elif kind == "jac":
            f = lambda: t.jacobian_device(tp)                           # noqa: E731
        elif kind == "normal":
            f = lambda: t.normal_device(tp)                             # noqa: E731
        else:
            f = lambda: t.curvature_device(tp)                          # noqa: E731
        out = _poisoned_runs(t, f, kernel, f"{label}: {kind} {w}").cpu().numpy()
        if kind == "eval":
            ref, bad = oracle.c_evaluate(order, ncoef, knots, coefs, list(w), sub)
            got, bar = out[:, idx], _tol(dt)
        elif kind == "jac":
            ref, bad = oracle.c_jacobian(order, ncoef, knots, coefs, sub)
            got, bar = out[:, :, idx], _tol(dt)
        elif kind == "normal":                                          # unit normals: the bar of the normal tests
            ref, bad = oracle.c_normal(order, ncoef, knots, coefs, sub, True, False)
            got, bar = out[:, idx], 2e-5 if dt == np.float32 else 1e-10
        else:                                                           # curvature: the bar of the curvature tests
            ref, bad = oracle.c_curvature(order, ncoef, knots, coefs, sub)
            got, bar = out[idx], 2e-5 if dt == np.float32 else 1e-11
        assert bad == -1
        ok = np.isfinite(ref)
        assert ok.mean() > 0.9 and np.array_equal(ok, np.isfinite(got)), (label, kind)
        observe(f"stale LDS: {kernel.rstrip('*')} vs oracle, {kind}, {_kind(dt)}", np.abs(got[ok] - ref[ok]).max() / _scale(ref[ok]), bar)


def _spec(order, ncoef, ndep, dt, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    knots = [cases.nonuniform_knots(rng, o, c, dt, lo, hi) for o, c in zip(order, ncoef)]
    coefs = rng.standard_normal((ndep, *ncoef)).astype(dt)
    return (tuple(order), tuple(ncoef), knots, coefs, dt)


# ------------------------------------------------------------------------------------------ eval_slab2 (known bad first)
@pytest.mark.parametrize("order,ncoef,ndep,dt,n", [
    ((5, 3), (12, 40), 4, np.float32, (1 << 20) + 4_099),        # one slab, pad1 = 2
    ((6, 2), (9, 33), 2, np.float64, (1 << 20) + 4_099),         # one slab, pad1 = 4
    ((5, 3), (700, 40), 2, np.float64, (1 << 19) + 77_001),      # several passes, pad1 = 2 (448 KB table)
    ((4, 5), (900, 11), 3, np.float64, (1 << 19) + 7_001),       # the TomsNasty shape: several passes, pad0 = 1
])
def test_slab_kernel_ignores_stale_lds(order, ncoef, ndep, dt, n):
    """eval_slab2 with a second variable of lower order reads pad1 control points past a row's window (weight zero): on the
    last row of a slab, for a point in the last span of both variables, past the slab itself."""
    spec = _spec(order, ncoef, ndep, dt, sum(order) * 10 + ndep)
    rng = np.random.default_rng(5)
    pts = _points(order, ncoef, spec[2], n, dt, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("eval", (0, 0), "eval_slab2"), ("eval", (1, 1), "eval_slab2")],
                  f"eval_slab2 {order} {ncoef} nDep {ndep} {_kind(dt)}", rng)


# ------------------------------------------------------------------------------------------ LDS-resident point kernels
def test_uniform_knot_kernels_ignore_stale_lds():
    """eval_uni, jac_uni and the fused normal on the cfg2 bicubic."""
    nind, ndep, order, ncoef, knots, coefs, dt = cases.bench_spline(2)
    spec = (order, ncoef, knots, coefs, dt)
    rng = np.random.default_rng(11)
    pts = _points(order, ncoef, knots, 20_011, dt, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("eval", (0, 0), "eval_uni"), ("eval", (1, 2), "eval_uni"), ("jac", None, "jac_uni"),
                                 ("normal", None, "jac_uni")], "cfg2 bicubic", rng)


def test_rowrot_kernels_ignore_stale_lds():
    """eval_rowrot, jac_rowrot and curv_rowrot on the non-uniform cfg2 bicubic."""
    c = CASES["cfg2_bicubic_nonuniform"]
    spec = (c.order, c.nCoef, c.knots, c.coefs, np.float64)
    rng = np.random.default_rng(12)
    pts = _points(c.order, c.nCoef, c.knots, 20_011, np.float64, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("eval", (0, 0), "eval_rowrot"), ("eval", (2, 1), "eval_rowrot"), ("jac", None, "jac_rowrot"),
                                 ("curv", None, "curv_rowrot")], "cfg2 bicubic, non-uniform knots", rng)


def test_rec32_kernel_ignores_stale_lds():
    """eval_rec32: an fp32 bicubic with several spans in both variables."""
    spec = _spec((4, 4), (37, 16), 4, np.float32, 13, -2.0, 3.0)
    rng = np.random.default_rng(13)
    pts = _points(spec[0], spec[1], spec[2], 20_011, np.float32, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("eval", (0, 0), "eval_rec32"), ("eval", (1, 2), "eval_rec32")], "fp32 bicubic", rng)


def test_stream_kernels_ignore_stale_lds(monkeypatch):
    """eval_stream / jac_stream (BSK_VARIANT=4) and their uniform-knot forms eval_stream_uni / jac_stream_uni."""
    spec = _spec((3, 3, 3), (6, 7, 5), 2, np.float64, 14)
    rng = np.random.default_rng(14)
    pts = _points(spec[0], spec[1], spec[2], 20_011, np.float64, rng)
    t = _make(*spec, monkeypatch=monkeypatch, variant="4")
    _sweep_points(t, spec, pts, [("eval", (0, 0, 0), "eval_stream"), ("eval", (1, 0, 2), "eval_stream"),
                                 ("jac", None, "jac_stream")], "order 3 volume, BSK_VARIANT=4", rng)
    for order, ncoef, ndep in (((4,), (40,), 3), ((4, 4, 4), (8, 9, 10), 1)):
        knots = [cases.clamped_uniform_knots(o, nc) for o, nc in zip(order, ncoef)]
        coefs = rng.standard_normal((ndep, *ncoef))
        spec = (order, ncoef, knots, coefs, np.float64)
        pts = _points(order, ncoef, knots, 20_011, np.float64, rng)
        t = _make(*spec)
        _sweep_points(t, spec, pts, [("eval", (0,) * len(order), "eval_stream_uni"), ("eval", (2,) + (0,) * (len(order) - 1), "eval_stream_uni"),
                                     ("jac", None, "jac_stream_uni")], f"uniform knots {order}", rng)


def test_fixed_kernels_ignore_stale_lds(monkeypatch):
    """eval_fixed / jac_fixed (BSK_VARIANT=1)."""
    c = CASES["cfg2_bicubic_nonuniform"]
    spec = (c.order, c.nCoef, c.knots, c.coefs, np.float64)
    rng = np.random.default_rng(15)
    pts = _points(c.order, c.nCoef, c.knots, 20_011, np.float64, rng)
    t = _make(*spec, monkeypatch=monkeypatch, variant="1")
    _sweep_points(t, spec, pts, [("eval", (0, 0), "eval_fixed"), ("eval", (1, 1), "eval_fixed"), ("jac", None, "jac_fixed")],
                  "cfg2 bicubic non-uniform, BSK_VARIANT=1", rng)


def test_mixed_and_generic_kernels_ignore_stale_lds():
    """eval_mixed / jac_mixed (surface of orders 3 x 4; also curves up to order 12) and eval_generic, the dispatcher's
    last resort (a curve of order 14; it holds nothing in LDS, so this pins that it stays so)."""
    c = CASES["surface_o3x4"]
    spec = (c.order, c.nCoef, c.knots, c.coefs, np.float64)
    rng = np.random.default_rng(16)
    pts = _points(c.order, c.nCoef, c.knots, 20_011, np.float64, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("eval", (0, 0), "eval_mixed"), ("eval", (2, 1), "eval_mixed"), ("jac", None, "jac_mixed")],
                  "surface o3x4", rng)
    spec = _spec((14,), (24,), 2, np.float64, 16)
    pts = _points(spec[0], spec[1], spec[2], 20_011, np.float64, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("eval", (0,), "eval_generic"), ("eval", (3,), "eval_generic")], "curve order 14", rng)


# ------------------------------------------------------------------------------------------ large tables
def test_gather_kernel_ignores_stale_lds():
    """eval_gather: a table beyond LDS with a batch too small for the cell-order pipeline."""
    spec = _spec((4, 4), (200, 150), 2, np.float64, 17)
    rng = np.random.default_rng(17)
    pts = _points(spec[0], spec[1], spec[2], 20_011, np.float64, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("eval", (0, 0), "eval_gather*"), ("eval", (1, 0), "eval_gather*")], "200 x 150 table", rng)


@pytest.mark.parametrize("variant,kernel", [("0", "eval_cellsort, MFMA*"), ("12", "eval_cellsort, VALU*"), ("13", "eval_binned_lds*")])
def test_cell_order_pipeline_ignores_stale_lds(variant, kernel, monkeypatch):
    """The cell-order pipeline on the cfg5 shape: eval_cellsort (MFMA, VALU) and eval_binned_lds."""
    nind, ndep, order, ncoef, knots, coefs, dt = cases.bench_spline(5)
    spec = (order, ncoef, knots, coefs, dt)
    rng = np.random.default_rng(18)
    pts = _points(order, ncoef, knots, 400_003, dt, rng)
    t = _make(*spec, monkeypatch=monkeypatch, variant=variant)
    _sweep_points(t, spec, pts, [("eval", (0, 0, 0), kernel), ("eval", (1, 0, 2), kernel)], f"cfg5 shape, BSK_VARIANT={variant}", rng)


def test_fused_jacobian_ignores_stale_lds():
    """The fused fp32 jacobian of the cell-order pipeline (eval_cellsort<..., JAC>)."""
    spec = _spec((3, 3, 3), (38, 34, 40), 3, np.float32, 19, 0.0, 1.0)
    rng = np.random.default_rng(19)
    pts = _points(spec[0], spec[1], spec[2], 280_003, np.float32, rng)
    t = _make(*spec)
    _sweep_points(t, spec, pts, [("jac", None, "fused jacobian*")], "order 3 volume, fp32", rng)


# ------------------------------------------------------------------------------------------ grids and tessellation
def _grid_oracle(spec, axes, w):
    order, ncoef, knots, coefs, dt = spec
    mesh = np.meshgrid(*axes, indexing="ij")
    ref, bad = oracle.c_evaluate(order, ncoef, knots, coefs, list(w), [m.ravel() for m in mesh])
    assert bad == -1
    return ref.reshape(ref.shape[0], *[len(a) for a in axes])


@pytest.mark.parametrize("what", ["grid_rows vector", "grid_rows scalar", "grid_surface", "grid_generic"])
def test_grid_kernels_ignore_stale_lds(what):
    rng = np.random.default_rng(20)
    if what == "grid_generic":
        c = CASES["volume_o3x4x2"]
        spec, shape = (c.order, c.nCoef, c.knots, c.coefs, np.float64), (13, 17, 9)
    else:
        spec = _spec((4, 4), (20, 18), 3, np.float64, 21)
        shape = {"grid_rows vector": (40, 128), "grid_rows scalar": (40, 77), "grid_surface": (40, 40)}[what]
    order, ncoef, knots = spec[:3]
    axes = [np.sort((k[o - 1] + (k[nc] - k[o - 1]) * rng.random(m)))[::-1].copy() for k, o, nc, m in zip(knots, order, ncoef, shape)]
    t = _make(*spec)
    ta = [torch.as_tensor(a, device="cuda") for a in axes]
    w = [1] + [0] * (len(order) - 1)
    out = _poisoned_runs(t, lambda: t.evaluate_grid_device(ta, w), what.split()[0], what).cpu().numpy()
    ref = _grid_oracle(spec, axes, w)
    observe(f"stale LDS: {what.split()[0]} vs oracle, fp64", np.abs(out - ref).max() / _scale(ref), 1e-12)


def _tess_patches(order, ncoef, dt, seed, count=3):
    rng = np.random.default_rng(seed)
    knots = [cases.nonuniform_knots(rng, o, c, dt, 0.0, 1.0) for o, c in zip(order, ncoef)]
    return [(order, ncoef, knots, rng.standard_normal((3, *ncoef)).astype(dt)) for _ in range(count)]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["hoisted 512", "hoisted 256", "normals", "mixed"])
def test_tess_rows_ignores_stale_lds(form, dt, monkeypatch):
    order = (3, 4) if form == "mixed" else (4, 4)
    patches = _tess_patches(order, (9, 8), dt, 22)
    tabs = [DeviceSpline(o, c, k, cf, dt) for (o, c, k, cf) in patches]
    u = np.linspace(0.0, 1.0, 24, dtype=dt)
    v = np.linspace(0.0, 1.0, 128, dtype=dt)
    tu, tv = torch.as_tensor(u, device="cuda"), torch.as_tensor(v, device="cuda")
    if form == "hoisted 256":
        monkeypatch.setenv("BSK_TESS_T", "256")
    normals = form in ("normals", "mixed")
    out = _poisoned_runs(tabs[0], lambda: bspy_amd.tessellate_tables(tabs, (tu, tv), normals=normals, normalize=False),
                         f"tess_rows {form}", f"tess_rows {form} {_kind(dt)}")
    pos = (out[0] if normals else out).cpu().numpy()
    uu, vv = [m.ravel() for m in np.meshgrid(u, v, indexing="ij")]
    for p, (o, c, k, cf) in enumerate(patches):
        ref, bad = oracle.c_evaluate(o, c, k, cf, [0, 0], [uu, vv])
        assert bad == -1
        observe(f"stale LDS: tess_rows {form} positions vs oracle, {_kind(dt)}", np.abs(pos[p].reshape(3, -1) - ref).max() / _scale(ref), _tol(dt))
        if normals:
            ref, _ = oracle.c_normal(o, c, k, cf, [uu, vv], False, False)
            got = out[1][p].cpu().numpy().reshape(3, -1)
            observe(f"stale LDS: tess_rows {form} area normals vs oracle, {_kind(dt)}", np.abs(got - ref).max() / _scale(ref), _tol(dt))


# ------------------------------------------------------------------------------------------ quadrature
def test_integral_regions_ignores_stale_lds():
    """integral_regions: called from the host, one Gauss-Kronrod round per call - the fill precedes the call's only
    kernel here; inside Spline.integral it would precede the first round only."""
    rng = np.random.default_rng(23)
    order, ncoef = (3, 4), (7, 6)
    knots = [cases.clamped_uniform_knots(o, c) for o, c in zip(order, ncoef)]
    s = Spline(2, 3, order, ncoef, knots, rng.standard_normal((3, *ncoef)))
    lo_hi, span = iq.regions(s, iq.check_domain(s, None))
    lo_hi, span = iq.split(lo_hi, span)
    t = s.device_tables()
    out = _poisoned_runs(t, lambda: t.integral_regions(lo_hi, span), "integral_regions", "integral_regions")
    k, g = region_sums(s, lo_hi, span)
    observe("stale LDS: integral_regions vs CPU rule, fp64", max(np.abs(out[:, 0] - k).max(), np.abs(out[:, 1] - g).max()) / _scale(k), 1e-12)
