"""
Every device path on a side stream and on poisoned scratch memory ("The stream contract as tested").

include/bspy_amd.h promises that a BSK_DEVICE entry point "only enqueues work on `stream`", bspy_amd/_backend.py that
``Device`` runs "the kernels on the stream that is current on entry".  On the null stream neither can fail, because the null
stream orders everything, and ``torch.empty`` hands back the bytes of the last identical call, so that a kernel that leaves
part of its output unwritten still finds the right answer there.  Every test here runs one family's smallest case, the one
its own GPU test compares with the host path (tests/stream_families.py; the point kernels: the oracle at the bars of
tests/test_gpu_families.py, tests/test_gpu_shape.py and tests/test_gpu_stale_lds.py), in five steps:

  (a) the host path once (the oracle for the point kernels): the bytes to match;
  (b) one device call on the default stream, so that tables are uploaded and workspaces have grown;
  (c) the device call with every ``Device.empty`` buffer (every ``out=``) of bytes 0xFF, then 0x5A, on the default stream:
      the bytes of (a) and the launches of (b);
  (d) the same two calls inside ``torch.cuda.stream(side)``, the null stream kept busy by the gate (tests/stream_util.py)
      and the inputs copied to the device on the side stream after the gate is armed: the bytes of (a);
  (e) every gated entry point returned while the gate was still pending, unless ALLOWED names it; and at least one did.

A launch on stream 0, a workspace cleared or filled on the null stream, or a readback that is not ordered behind the side
stream lands behind the gate, and the consumer on the side stream reads poison in step (d).  Where the device path and the
host path may differ in the last bit (band, product and fit kernels) step (b) is held to the host path at the family's bar
and the bytes of (c) and (d) are those of (b).
"""
import numpy as np
import pytest

import bspy_amd
import cases
import oracle
import shape_ref as sh
import stream_families as sf
import test_gpu_families as fam
import test_gpu_shape as shp
import test_gpu_stale_lds as stale
from bspy_amd import DeviceSpline
from bspy_amd._backend import Device
from stream_util import Gate, GateLog, gated, kept_handles, poison_tensor, poisoned, side_stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PATTERNS = (0xFF, 0x5A)
OUT = [0x5A]               # the bytes of a poisoned ``out=``: the pattern of the step that runs (five_steps sets it)

# Entry points that include/bspy_amd.h permits to block on a host array: a blocking copy on the null stream returns only
# when the data has arrived (behind the gate), which is slow but correct.  Each with the header's sentence.
ALLOWED = {
    "bsk_product_apply": "`terms` is a host array.",
    "bsk_band_apply": "The operator's tables are uploaded by the first device call.",
    "bsk_band_absmax": "The operator's tables are uploaded by the first device call.",
    "bsk_fit_sweep": "The plan's tables are uploaded by the first device call",
    "bsk_scan_apply": "bsk_scan_create copies g and makes no HIP call.",
    # no host array, but a wait that the header states: the call returns when the kernels in front of it on `stream` have
    # run, and under the gate's products a large batch takes longer than a gate (the results are still held to their bytes)
    "bsk_domain_status": "Synchronise `stream` and report whether any BSK_DEVICE call on this handle since the",
}

# the kernels the family's own GPU test names (a launch is named by its kernel, some with a word behind it)
KERNELS = {
    "zeros": ["roots_flag", "roots_isolate"],
    "zeros2": ["roots2_flag", "roots2_isolate", "roots2_merge"],
    "zeros3": ["roots3_flag", "roots3_isolate", "roots3_merge"],
    "project seeded": ["project_seed", "project_newton"],
    "project guess": ["project_newton"],
    "contours": ["contour_flag", "contour_march"],
    "isosurface (3, 3, 3) on 2 x 2 x 2 cells": ["iso_flag", "iso_walk count", "iso_walk emit", "iso_leaf count", "iso_leaf emit", "iso_vertex"],
    "isosurface (4, 4, 4), 64 coefficients": ["iso_flag", "iso_walk count", "iso_walk emit", "iso_leaf count", "iso_leaf emit", "iso_vertex"],
    "mesh": ["mesh_bound", "mesh_count", "mesh_emit", "mesh_vertex"],
    "rays first": ["ray_boxes", "ray_count", "ray_emit", "ray_isolate", "ray_reduce"],
    "rays all": ["ray_boxes", "ray_count", "ray_emit", "ray_isolate", "ray_reduce", "ray_reduce all"],
    "surfaces": ["ray_boxes", "ssx_count", "ssx_emit", "ssx_isolate"],
    "scatter": ["scatter_key", "scatter_gram", "scatter_cell", "scatter_fold", "scatter_residual"],
    "scatter robust, device solve": ["scatter_key", "scatter_gram", "scatter_cell", "scatter_fold", "scatter_solve", "scatter_residual",
                                     "scatter_reweight"],
    "least_squares": ["fit_sweep", "fit_sweep turned"],
    "fit plan": ["fit_sweep", "fit_sweep turned"],
    "run_steps fp64": ["band_apply", "band_apply_line"],
    "run_steps fp32": ["band_apply", "band_apply_line"],
    "sums": ["scan_apply", "scan_line", "sum_bcast"],
    "product M = 1": ["band_product_line"],
    "product M = 2": ["band_product_tile"],
    "remove_knots": ["band_absmax", "band_absmax_line"],
}


@pytest.fixture(scope="module")
def gate():
    g = Gate()
    yield g
    g.drain()


@pytest.fixture(scope="module")
def side():
    return side_stream()


def five_steps(name, run, want, exact, gate, side, check_first=None, same=lambda got, want: got == want):
    """Steps (b) to (e) for ``run() -> Result``; ``want``: the Result of step (a), or None where ``check_first`` holds the
    first device run to its reference itself; ``same``: when two results are the same (the bytes; the point kernels:
    ``stream_families.same_numbers``).  Returns the launches named."""
    torch.cuda.synchronize()
    with kept_handles():
        first = run()                                                                  # (b)
        torch.cuda.synchronize()
        assert first.ran and not all(p.startswith("host") for p in first.ran), (name, first.ran)
        if check_first is not None:
            check_first(first)
        elif exact:
            if first.bits != want.bits:
                pytest.fail(f"{name}: the device path on the default stream differs from the host path: {sf.differing(first.bits, want.bits, 0)}")
        else:
            sf.near(name, first, want)
        for pattern in PATTERNS:                                                       # (c)
            OUT[0] = pattern
            with poisoned(pattern):
                got = run()
            torch.cuda.synchronize()
            assert got.ran == first.ran, (name, hex(pattern), got.ran, first.ran)
            if not same(got.bits, first.bits):
                pytest.fail(f"{name}: other bytes on scratch memory of bytes {pattern:#x} (default stream): "
                            f"{sf.differing(got.bits, first.bits, pattern)}")
        side.wait_stream(torch.cuda.default_stream())                                  # (d)
        try:
            with torch.cuda.stream(side), gated(Device, gate) as log:
                for pattern in PATTERNS:
                    OUT[0] = pattern
                    gate.ensure()                                                      # the inputs go over behind an armed gate
                    with poisoned(pattern):
                        got = run(log)
                    side.synchronize()
                    assert got.ran == first.ran, (name, hex(pattern), got.ran, first.ran)
                    if not same(got.bits, first.bits):
                        pytest.fail(f"{name}: other bytes on the side stream (scratch memory of bytes {pattern:#x}), something is "
                                    f"not ordered with the call's stream: {sf.differing(got.bits, first.bits, pattern)}")
        finally:
            side.synchronize()                                                         # the handles go back to the default stream
            gate.drain()
            torch.cuda.synchronize()
    late = log.check(ALLOWED)                                                          # (e)
    print(f"{name}: {len(log.calls)} gated calls, {gate.armed} gates so far, behind a finished gate (allowed): {late}")
    return first.ran


def test_the_helpers_do_what_they_say(gate, side):
    be = Device.current()
    for pattern in PATTERNS:
        with poisoned(pattern):
            for dtype in (np.float64, np.float32, np.int32, np.uint8, np.int64):
                a = be.empty((3, 5), dtype)
                assert (a.view(-1).view(torch.uint8) == pattern).all() and not be.zeros((3, 5), dtype).any()
            assert be.empty((0, 4), np.float64).shape == (0, 4)
    assert torch.isnan(poison_tensor((2, 3), torch.float64, 0xFF)).all()
    torch.cuda.synchronize()
    assert not gate.pending()
    gate.arm()
    assert gate.pending(), "the gate is over before the call that armed it returns"
    with torch.cuda.stream(side):                             # work on the side stream does not wait for the gate
        x = torch.ones(1000, device="cuda").sum().item()
    assert x == 1000.0 and gate.pending(), "the side stream waited for the null stream: the gate orders it, and would hide every bug"
    log = GateLog(gate)
    log.run("late", gate.drain)
    with pytest.raises(AssertionError, match="late returned behind a finished gate"):
        log.check(ALLOWED)
    with pytest.raises(AssertionError, match="proved nothing"):
        log.check({"late": "for this check"})
    assert float(gate.a[0, 0]) == 1.0 / gate.a.shape[0], "the chain of products left its fixed point"


@pytest.mark.parametrize("name", sorted(sf.FAMILIES))
def test_family_on_a_side_stream_and_poisoned_scratch(name, gate, side):
    run, exact = sf.FAMILIES[name]
    want = sf.on_host(name)                                                            # (a)
    ran = five_steps(name, lambda log=None: run("device"), want, exact, gate, side)
    for kernel in KERNELS[name]:
        assert any(p == kernel or p.startswith(kernel + " ") for p in ran), (name, kernel, ran)


def test_every_family_is_listed():
    assert set(KERNELS) == set(sf.FAMILIES)
    named = {k.split()[0] for listed in KERNELS.values() for k in listed}
    for family in ("zeros2", "zeros3", "project", "contours", "remove_knots"):
        assert cases.CELL_KERNELS[family] <= named, family


# ------------------------------------------------------------------------------------------ the point kernels
def _direct(log, name, call):
    """A DeviceSpline call, which does not go through ``Device.call``: gated by hand where a log is given."""
    return call() if log is None else log.run(name, call)


def _rung(name):
    """The spline, the points and the oracle's values of one rung of tests/test_gpu_families.py, drawn as there."""
    dt, order, ncoef, ndep, kind, n, eval_family, jac_family = fam.RUNGS[name]
    rng = np.random.default_rng(sorted(fam.RUNGS).index(name))
    if kind == "uniform":
        knots = [cases.clamped_uniform_knots(o, c, dt) for o, c in zip(order, ncoef)]
    else:
        knots = [cases.nonuniform_knots(rng, o, c, dt, 0.0, 1.0) for o, c in zip(order, ncoef)]
    coefs = rng.standard_normal((ndep, *ncoef)).astype(dt)
    pts = [rng.random(n).astype(dt) for _ in order]
    first = [1] + [0] * (len(order) - 1)
    refs = [oracle.c_evaluate(order, ncoef, knots, coefs, w, pts) for w in ([0] * len(order), first)]
    refs.append(oracle.c_jacobian(order, ncoef, knots, coefs, pts))
    assert all(bad == -1 for _, bad in refs)
    return DeviceSpline(order, ncoef, knots, coefs, dt), pts, first, [r for r, _ in refs]


@pytest.mark.parametrize("name", sorted(fam.RUNGS))
def test_point_rung_on_a_side_stream_and_poisoned_out(name, gate, side):
    """evaluate_device, one first derivative and jacobian_device of every rung into a poisoned ``out=``; fp32 and fp64 are
    the rungs' own types (rec32 and cell_order_fused are the fp32 ones)."""
    dt, order, ncoef, ndep, kind, n, eval_family, jac_family = fam.RUNGS[name]
    t, pts, first, refs = _rung(name)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    tol = 2e-5 if dt == np.float32 else 1e-12

    def run(log=None):
        tp = [torch.from_numpy(p).cuda() for p in pts]
        out, ran = [], []
        for w in ([0] * len(order), first):
            o = poison_tensor((ndep, n), tdt, OUT[0])
            out.append(_direct(log, "bsk_evaluate", lambda: t.evaluate_device(tp, w, out=o, check=False)))
            ran.append(t.last_kernel())
        o = poison_tensor((ndep, len(order), n), tdt, OUT[0])
        out.append(_direct(log, "bsk_jacobian", lambda: t.jacobian_device(tp, out=o, check=False)))
        ran.append(t.last_kernel())
        _direct(log, "bsk_domain_status", t.domain_status)
        return sf.Result(sf.bits_of(out), tuple(ran))

    def against_the_oracle(got):
        assert list(got.ran) == [eval_family, eval_family, jac_family], (name, got.ran)
        for (dtype, shape, raw), ref in zip(got.bits, refs):
            value = np.frombuffer(raw, np.dtype(dtype)).reshape(ref.shape)
            err = np.abs(value - ref).max() / max(1.0, np.abs(ref).max())
            assert err <= tol, (name, err)

    five_steps(name, run, None, True, gate, side, check_first=against_the_oracle, same=sf.same_numbers)
    t.close()


def _shape_cases():
    """One case of tests/test_gpu_shape.py per kernel it names: the one with the fewest points."""
    best = {}
    for name in shp.FAMILY_CASES:
        c = shp.CASES[name]
        if c.zero:
            continue
        key = (c.kind, c.kernel, c.type)
        if key not in best or (c.n, c.name) < (best[key].n, best[key].name):
            best[key] = c
    return {c.name: c for c in best.values()}


SHAPE_CASES = _shape_cases()


@pytest.mark.parametrize("name", sorted(SHAPE_CASES))
def test_normal_and_curvature_on_a_side_stream_and_poisoned_out(name, gate, side, monkeypatch):
    case = SHAPE_CASES[name]
    ref = sh.reference(case)
    t = shp._make(case, monkeypatch)
    pts = case.points()
    tdt = torch.float32 if case.dt == np.float32 else torch.float64
    shape = (case.n,) if case.kind == "curvature" else (max(case.nInd, case.nDep), case.n)
    q = "curvature" if case.kind == "curvature" else "unit normal"

    def run(log=None):
        tp = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pts]
        o = poison_tensor(shape, tdt, OUT[0])
        entry = "bsk_curvature" if case.kind == "curvature" else "bsk_normal"
        got = _direct(log, entry, lambda: shp._device_call(t, case, tp, q, out=o, check=False))
        ran = (t.last_kernel(),)
        _direct(log, "bsk_domain_status", t.domain_status)
        return sf.Result(sf.bits_of([got]), ran)

    def against_the_reference(got):
        assert shp._kernel_ok(got.ran[0], case.kernel), (name, got.ran, case.kernel)
        dtype, _, raw = got.bits[0]
        value = np.frombuffer(raw, np.dtype(dtype)).reshape(shape)
        ratio, _, share = ref.compare(q, value[..., ref.idx])
        assert share >= sh.KEEP and ratio <= 1.0, (name, ratio, share)

    five_steps(name, run, None, True, gate, side, check_first=against_the_reference, same=sf.same_numbers)
    t.close()


GRIDS = {"grid_rows vector": (40, 128), "grid_rows scalar": (40, 77), "grid_surface": (40, 40), "grid_generic": (13, 17, 9)}


@pytest.mark.parametrize("what", sorted(GRIDS))
def test_grid_on_a_side_stream_and_poisoned_out(what, gate, side):
    """The grid kernels on the cases of tests/test_gpu_stale_lds.py, against the oracle on the grid's points."""
    rng = np.random.default_rng(20)
    if what == "grid_generic":
        c = stale.CASES["volume_o3x4x2"]
        spec = (c.order, c.nCoef, c.knots, c.coefs, np.float64)
    else:
        spec = stale._spec((4, 4), (20, 18), 3, np.float64, 21)
    order, ncoef, knots = spec[:3]
    axes = [np.sort((k[o - 1] + (k[nc] - k[o - 1]) * rng.random(m)))[::-1].copy() for k, o, nc, m in zip(knots, order, ncoef, GRIDS[what])]
    w = [1] + [0] * (len(order) - 1)
    ref = stale._grid_oracle(spec, axes, w)
    t = stale._make(*spec)

    def run(log=None):
        ta = [torch.from_numpy(a).cuda() for a in axes]
        o = poison_tensor(ref.shape, torch.float64, OUT[0])
        got = _direct(log, "bsk_evaluate_grid", lambda: t.evaluate_grid_device(ta, w, out=o, check=False))
        ran = (t.last_kernel(),)
        _direct(log, "bsk_domain_status", t.domain_status)
        return sf.Result(sf.bits_of([got]), ran)

    def against_the_oracle(got):
        assert stale._kernel_ok(got.ran[0], what.split()[0]), (what, got.ran)
        value = np.frombuffer(got.bits[0][2], np.float64).reshape(ref.shape)
        assert np.abs(value - ref).max() / stale._scale(ref) <= 1e-12, what

    five_steps(what, run, None, True, gate, side, check_first=against_the_oracle, same=sf.same_numbers)
    t.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("form", ["positions", "normals", "mixed"])
def test_tessellate_on_a_side_stream_and_poisoned_out(form, dt, gate, side):
    """tess_rows on the patches of tests/test_gpu_stale_lds.py: positions alone, with area normals, and mixed orders."""
    patches = stale._tess_patches((3, 4) if form == "mixed" else (4, 4), (9, 8), dt, 22)
    tabs = [DeviceSpline(o, c, k, cf, dt) for (o, c, k, cf) in patches]
    u, v = np.linspace(0.0, 1.0, 24, dtype=dt), np.linspace(0.0, 1.0, 128, dtype=dt)
    uu, vv = [m.ravel() for m in np.meshgrid(u, v, indexing="ij")]
    normals = form != "positions"
    tdt = torch.float32 if dt == np.float32 else torch.float64
    shape = (len(tabs), 3, len(u), len(v))
    refs = [(oracle.c_evaluate(o, c, k, cf, [0, 0], [uu, vv])[0], oracle.c_normal(o, c, k, cf, [uu, vv], False, False)[0])
            for (o, c, k, cf) in patches]

    def run(log=None):
        tu, tv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
        out = (poison_tensor(shape, tdt, OUT[0]), poison_tensor(shape, tdt, OUT[0]) if normals else None)
        got = _direct(log, "bsk_tessellate", lambda: bspy_amd.tessellate_tables(tabs, (tu, tv), normals=normals, normalize=False, out=out,
                                                                               check=False))
        ran = (tabs[0].last_kernel(),)
        _direct(log, "bsk_domain_status", tabs[0].domain_status)
        return sf.Result(sf.bits_of(list(got) if normals else [got]), ran)

    def against_the_oracle(got):
        assert stale._kernel_ok(got.ran[0], "tess_rows*"), (form, got.ran)
        for which, (dtype, _, raw) in enumerate(got.bits):
            value = np.frombuffer(raw, np.dtype(dtype)).reshape(shape)
            for p, ref in enumerate(refs):
                err = np.abs(value[p].reshape(3, -1) - ref[which]).max() / stale._scale(ref[which])
                assert err <= stale._tol(dt), (form, which, p, err)

    five_steps(f"tessellate {form}", run, None, True, gate, side, check_first=against_the_oracle, same=sf.same_numbers)
    for t in tabs:
        t.close()
