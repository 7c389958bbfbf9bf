"""
Normal and curvature on every kernel family, batch path and chunk.  (CPU preconditions: tests/test_shape_host.py; inputs:
cases.shape_cases; yardstick and bars: tests/shape_ref.py.)

Spline.normal is dispatch_jac (whatever family the shape and the batch size select) and normal_epilogue, Spline.curvature two
or five dispatch_eval passes, a normal and curvature_curve / curvature_surface; only surfaces in 3-D on the LDS image take
fused kernels.  Every case runs the device call on its whole batch and compares 200 sample points with the
extended-precision restatement of the reference, as max |got - ref| / bar(p) <= 1 (observed under one label per quantity and
type): the unit normal, the area-scaled normal and its negation, or the curvature.  NaN results have to sit where the
reference's do, at most 10 % of a sample may be ill-conditioned, a polyline's curvature is exactly 0.0.  The derivative values
that enter are held to the delta the bar is built from (label "shape: derivative values / delta").

Kernel asserted by last_kernel() (an epilogue is unnamed: the family's name stays) and form of the bar, per family:
  jac_uni (fused normal)              cfg2                                           part-B form
  jac_rowrot (fused normal)           cfg2 non-uniform; order (2, 2) fp32            K eps
  jac_stream                          order (3, 3) fp64 / fp32; (3, 3, 3) nDep 2, 4  K eps
  jac_stream_uni                      order (3, 3) uniform; cubic curve uniform      part-B form
  jac_fixed                           cfg2 non-uniform, BSK_VARIANT=1; (6, 6); (5, 5, 5) nDep 4; L2-resident, n < 2^18   K eps
  jac_mixed                           surface_o3x4; (3, 4, 2) nDep 2                 K eps
  eval_mixed (derivative passes)      four variables; curve order 12                 K eps
  eval_generic (derivative passes)    curve order 14                                 K eps
  cell-order pipeline / eval_slab2    L2-resident surface, n 270 001 / 530 003 (derivative passes)   K eps
  fused cell-order jacobian           cfg5 fp32, n 280 003                           K eps
  curv_rowrot                         order (2, 2), (4, 4), bicubic fp32, cfg2 non-uniform   K eps
  five passes + normal + epilogue     (3, 3) fp64 / fp32 / uniform (part-B form), surface_o3x4, cfg2 under BSK_VARIANT=1,
                                      L2-resident at three sizes                     K eps
  two passes + curvature_curve        cubic uniform (signed, both orientations; part-B form), order 6, 12, 14,
                                      2 500 coefficients nDep 4 (L2-resident gather), polylines (exactly 0.0)   K eps
Families moved off the tight bar: none.

Batch paths, bit for bit wherever the same kernels run (the jac_stream surface, the fused cfg2 surface, the L2-resident
surface): device call against the small host call; device tensors and out= views 8 bytes past a 16-byte boundary; the staged
host path in one chunk; the pipelined host path (sample against the bar, the front against a call on the front alone, the
earlier of two offenders in different chunks); the staged host path in several chunks (child process: the limits are read
once); the 2^22 device chunk loop of curvature (tail against a call on the tail alone, sample against the bar, the call's flat
index of the first offender); stale workspaces; and the Python boundary (broadcasting, indices=, negateNormal, the reference's
ValueError from CUDA inputs, a wrong out=).
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import cases
import oracle
import bspy_amd
import scale_ref as sr
import shape_ref as sh
from bspy_amd import DeviceSpline, Spline
from conftest import ROOT, observe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = cases.shape_cases()
PATH_SIZES = (cases.SHAPE_STAGED, cases.SHAPE_PIPED, cases.SHAPE_DEVICE_CHUNKS)
FAMILY_CASES = sorted(n for n, c in CASES.items() if c.n not in PATH_SIZES)
N33, NFUSED, NL2 = "normal: general LDS, order (3, 3)", "normal: fused, cfg2 non-uniform", "normal: L2-resident surface"
C33, CFUSED, CL2 = "curvature: non-fused surface, order (3, 3)", "curvature: fused, cfg2 non-uniform", "curvature: non-fused surface, L2-resident"
PATH_CASES = [N33, NFUSED, NL2, C33, CFUSED, CL2]
QUANTITIES = {"unit normal": (True, False), "area normal": (False, False), "area normal, negated": (False, True)}


def _kernel_ok(got, want):
    return got == want if not want.endswith("*") else want[:-1] in got


def _make(case, monkeypatch):
    if case.variant is not None:
        monkeypatch.setenv("BSK_VARIANT", case.variant)
    try:
        return DeviceSpline(case.order, case.nCoef, case.knots, case.coefs, case.dt)
    finally:
        if case.variant is not None:
            monkeypatch.delenv("BSK_VARIANT")


def _np(x):
    return x.detach().cpu().numpy()


def _dev(pts):
    return [torch.as_tensor(p, device="cuda") for p in pts]


def _device_call(t, case, tp, q="unit normal", **kw):
    if case.kind == "curvature":
        return t.curvature_device(tp, **kw)
    return t.normal_device(tp, *QUANTITIES[q], **kw)


def _host_call(t, case, pts, q="unit normal"):
    return t.curvature(pts) if case.kind == "curvature" else t.normal(pts, *QUANTITIES[q])


def _quantities(case):
    return ["curvature"] if case.kind == "curvature" else list(QUANTITIES)


def _label(case, q):
    return f"shape: {q}, {case.type}{', uniform families' if case.uniform else ''}"


def _against_bar(case, q, got_at_sample):
    """The sample of one result against the bar; the ratio is printed, observed and asserted."""
    ref = sh.reference(case)
    ratio, units, share = ref.compare(q, got_at_sample)
    print(f"{case.name}: {q}: error / bar {ratio:.3f} ({units:.2f} units), kept {share:.3f}")
    assert share >= (1.0 if q.startswith("area") else sh.KEEP), (case.name, q, share)
    observe(_label(case, q), ratio, 1.0)


def _out_of_domain(case, pts, at):
    """pts with the last parameter of the points `at` beyond the top of the domain."""
    bad = [p.copy() for p in pts]
    k, o, c = case.knots[-1], case.order[-1], case.nCoef[-1]
    bad[-1][list(at)] = k[c] + (k[c] - k[o - 1])
    return bad


# ------------------------------------------------------------------------------------------ every family
@pytest.mark.parametrize("name", FAMILY_CASES)
def test_family_against_the_reference(name, monkeypatch):
    case = CASES[name]
    ref = sh.reference(case)
    t = _make(case, monkeypatch)
    pts = case.points()
    tp = _dev(pts)
    named = []
    # the derivative values the quantity is made of, against the delta its bar is built from
    for w, ext, delta in zip(ref.wrts, ref.D, ref.delta):
        got = _np(t.evaluate_device(tp, list(w)))[:, ref.idx]          # on the whole batch: the family the batch size selects
        assert np.array_equal(np.isnan(got).any(0), np.isnan(np.asarray(ext, np.float64)).any(0)), (name, w)
        err = float(np.abs(got[:, ref.finite].astype(ext.dtype) - ext[:, ref.finite]).max())
        print(f"{name}: derivative {w}: error / delta {err / delta:.3f}")
        observe(f"shape: derivative values / delta, {case.type}{', uniform families' if case.uniform else ''}", err / delta, 1.0)
    for q in _quantities(case):
        got = _np(_device_call(t, case, tp, q))
        named.append(t.last_kernel())
        assert got.shape == ((case.n,) if case.kind == "curvature" else (max(case.nInd, case.nDep), case.n))
        at = got[..., ref.idx]
        if case.zero:
            orc, bad = oracle.c_curvature(case.order, case.nCoef, case.knots, case.coefs, pts)
            assert bad == -1 and np.array_equal(np.isfinite(got), np.isfinite(orc)), name
            assert (got[np.isfinite(got)] == 0.0).all(), f"{name}: the second derivative of a polyline is identically zero"
            continue
        _against_bar(case, q, at)
    if name.endswith("cubic uniform nDep 2"):
        # the sign, both orientations: the reversed curve at the mirrored parameters has the opposite curvature
        back = CASES[name + ", reversed"]
        ext, _, bar = ref.q["curvature"]
        lo, hi = case.knots[0][case.order[0] - 1], case.knots[0][case.nCoef[0]]
        mirrored = _np(_make(back, monkeypatch).curvature_device(_dev([(lo + hi) - ref.pts[0]])))
        clear = ref.finite & (np.abs(np.asarray(ext[0], np.float64)) > 4.0 * bar[0])
        assert clear.sum() > 150
        assert np.array_equal(np.sign(at[clear]), np.sign(np.asarray(ext[0], np.float64))[clear])
        assert np.array_equal(np.sign(mirrored[clear]), -np.sign(at[clear]))
    assert all(_kernel_ok(k, case.kernel) for k in named), (name, named, case.kernel)


# ------------------------------------------------------------------------------------------ batch paths
@pytest.mark.parametrize("name", PATH_CASES)
def test_device_small_host_views_and_staged(name, monkeypatch):
    """(a) the device call against the small-call host call, (b) device tensors and out= views that start 8 bytes past a
    16-byte boundary, (c) the staged host path in one chunk against the device call: the same kernels, the same bytes."""
    case = CASES[name]
    t = _make(case, monkeypatch)
    pts = case.points()
    tp = _dev(pts)
    for q in _quantities(case)[:2]:
        dev = _device_call(t, case, tp, q)
        kernel = t.last_kernel()
        assert _kernel_ok(kernel, case.kernel), (name, kernel)
        host = _host_call(t, case, pts, q)
        assert t.last_kernel() == kernel, (name, "small host call", t.last_kernel(), kernel)
        assert sr.same_bits(host, _np(dev)), f"{name}: {q}: the small host call differs from the device call"
        shifted = []
        for p in tp:
            buf = torch.empty(case.n + 2, dtype=p.dtype, device="cuda")
            assert buf.data_ptr() % 16 == 0
            view = buf[1:case.n + 1]
            view.copy_(p)
            shifted.append(view)
        obuf = torch.empty(dev.numel() + 2, dtype=dev.dtype, device="cuda")
        out = obuf[1:1 + dev.numel()]
        assert out.data_ptr() % 16 == 8 and all(v.data_ptr() % 16 == 8 for v in shifted)
        obuf.fill_(7.0)
        back = _device_call(t, case, shifted, q, out=out)
        assert back.data_ptr() == out.data_ptr() and t.last_kernel() == kernel
        assert sr.same_bits(_np(out).reshape(dev.shape), _np(dev)), f"{name}: {q}: views 8 bytes past a 16-byte boundary differ"
        assert float(obuf[0]) == 7.0 and float(obuf[-1]) == 7.0, f"{name}: {q}: wrote outside the out= view"
    big = CASES[f"{name}, n {cases.SHAPE_STAGED}"]
    pts = big.points()
    dev = _np(_device_call(t, big, _dev(pts)))
    kernel = t.last_kernel()
    host = _host_call(t, big, pts)
    assert t.last_kernel() == kernel, (name, "staged host call", t.last_kernel(), kernel)
    assert sr.same_bits(host, dev), f"{name}: the staged host call differs from the device call"
    _against_bar(big, _quantities(big)[0], host[..., sh.reference(big).idx])


@pytest.mark.parametrize("name", [N33, NFUSED, NL2])
def test_pipelined_host_normal(name, monkeypatch):
    """(d) 2^21 + 5 points: three chunks of 2^20 through run_piped (curvature never takes this path)."""
    case = CASES[f"{name}, n {cases.SHAPE_PIPED}"]
    t = _make(case, monkeypatch)
    pts = case.points()
    got = t.normal(pts)
    t.normal_device(_dev([p[:1 << 20] for p in pts]))
    whole = t.last_kernel()                                  # of a full chunk (the ragged last one has five points)
    _against_bar(case, "unit normal", got[:, sh.reference(case).idx])
    front = t.normal([p[:cases.SHAPE_N] for p in pts])
    if t.last_kernel() == whole:
        assert sr.same_bits(got[:, :cases.SHAPE_N], front), f"{name}: the front of the pipelined call differs from a call on the front alone"
    else:
        # the family differs by batch size (the L2-resident surface: cell-order passes above 2^18 points a chunk, jac_fixed
        # below): both against the bar, on the points of the sample that lie in the front
        print(f"{name}: {whole} for chunks of 2^20 points, {t.last_kernel()} for {cases.SHAPE_N}: compared by the bar")
        ref = sh.reference(case)
        sub = np.where(ref.idx < cases.SHAPE_N, ref.idx, 0)
        at = np.where(ref.idx < cases.SHAPE_N, front[:, sub], got[:, ref.idx])
        _against_bar(case, "unit normal", at)
    second, third = (1 << 20) + 77_777, (1 << 21) + 2
    with pytest.raises(bspy_amd.DomainError) as e:
        t.normal(_out_of_domain(case, pts, (second, third)))
    assert e.value.index == second
    assert sr.same_bits(t.normal([p[:cases.SHAPE_N] for p in pts]), front), "a domain error left something behind"


CHILD = """
    import sys, numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import cases, bspy_amd
    C = cases.shape_cases()
    out = {}
    for key, name in (("surface", "normal: general LDS, order (3, 3)"), ("curve", "curvature: curve, order 12 nDep 2")):
        c = C[name].sized(150_001)
        t = bspy_amd.DeviceSpline(c.order, c.nCoef, c.knots, c.coefs, c.dt)
        pts = c.points()
        out[key + " normal"] = t.normal(pts)
        out[key + " curvature"] = t.curvature(pts)
        k, o, m = c.knots[-1], c.order[-1], c.nCoef[-1]
        bad = [p.copy() for p in pts]
        bad[-1][[47_123, 130_001]] = k[m] + (k[m] - k[o - 1])
        for what, fn in (("normal", t.normal), ("curvature", t.curvature)):
            try:
                fn(bad); print(key, what, "no error")
            except bspy_amd.DomainError as e:
                print(key, what, "bad", e.index)
    np.savez(sys.argv[1], **out)
"""


def test_staged_host_path_in_several_chunks(tmp_path):
    """(e) BSK_HOST_CHUNK=40000, BSK_SMALL_POINTS=1000 and BSK_RR_CHUNK=4096 in a child process (the limits are read once):
    150 001 points in four chunks against the same child without the limits, bit for bit; offenders in chunks 1 and 3."""
    code = textwrap.dedent(CHILD) % (ROOT, os.path.join(ROOT, "tests"))
    outs = []
    for env_extra in ({}, {"BSK_HOST_CHUNK": "40000", "BSK_SMALL_POINTS": "1000", "BSK_RR_CHUNK": "4096"}):
        f = str(tmp_path / f"chunks_{len(outs)}.npz")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        for line in ("surface normal bad 47123", "surface curvature bad 47123", "curve normal bad 47123", "curve curvature bad 47123"):
            assert line in r.stdout, r.stdout
        outs.append(np.load(f))
    for key in outs[0].files:
        assert sr.same_bits(outs[0][key], outs[1][key]), f"{key}: four chunks of 40 000 differ from the whole batch"


@pytest.mark.parametrize("name", [CFUSED, C33])
def test_curvature_device_chunk_loop(name, monkeypatch):
    """(f) 2^22 + 4 099 points on the device: two chunks.  The non-fused run takes 0.6 GB of curv_ws and 0.2 GB of aux_ws."""
    case = CASES[f"{name}, n {cases.SHAPE_DEVICE_CHUNKS}"]
    cut = 1 << 22
    t = _make(case, monkeypatch)
    try:
        pts = case.points()
        tp = _dev(pts)
        got = _np(t.curvature_device(tp))
        _against_bar(case, "curvature", got[sh.reference(case).idx])
        tail = _np(t.curvature_device([p[cut:] for p in tp]))
        assert sr.same_bits(got[cut:], tail), f"{name}: the second chunk differs from a call on the tail alone"
        for at, want in (((600, cut + 500), 600), ((cut + 500,), cut + 500)):
            with pytest.raises(bspy_amd.DomainError) as e:
                t.curvature_device(_dev(_out_of_domain(case, pts, at)))
            assert e.value.index == want, (name, at, e.value.index)
        assert sr.same_bits(_np(t.curvature_device([p[cut:] for p in tp])), tail), "a domain error left a record behind"
    finally:
        t.close()
        torch.cuda.empty_cache()


def test_stale_workspaces(monkeypatch):
    """(g) a large curvature, a small normal, a mid-sized curvature and a one-point normal on ONE handle: each the same bytes
    as on a fresh handle."""
    case = CASES[CL2]
    pts = case.sized(530_003).points()
    calls = [("curvature", 530_003), ("normal", 257), ("curvature", cases.SHAPE_N), ("normal", 1)]
    one = _make(case, monkeypatch)
    try:
        for what, n in calls:
            tp = _dev([p[:n] for p in pts])
            fresh = _make(case, monkeypatch)
            fn = (lambda t: t.curvature_device(tp)) if what == "curvature" else (lambda t: t.normal_device(tp))
            want = _np(fn(fresh))
            fresh.close()
            assert sr.same_bits(_np(fn(one)), want), f"{what} of {n} points after the calls before it differs from a fresh handle's"
    finally:
        one.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ Python boundary
def test_python_boundary():
    """(h) Spline.normal / Spline.curvature: broadcast NumPy and CUDA inputs, indices=, negateNormal, the reference's error."""
    c = CASES[N33]
    s = Spline(c.nInd, c.nDep, c.order, c.nCoef, c.knots, c.coefs)
    rng = np.random.default_rng(9)
    dom = [(k[o - 1], k[m]) for k, o, m in zip(c.knots, c.order, c.nCoef)]
    u = dom[0][0] + (dom[0][1] - dom[0][0]) * rng.random(37)
    v = dom[1][0] + (dom[1][1] - dom[1][0]) * rng.random(41)
    U, V = (a.ravel() for a in np.broadcast_arrays(u[:, None], v[None, :]))
    flat_n, flat_c = s.normal([U, V]), s.curvature([U, V])
    assert flat_n.shape == (3, 37 * 41) and flat_c.shape == (37 * 41,)
    for mk in (lambda a: a, lambda a: torch.as_tensor(a, device="cuda")):
        n2, c2 = s.normal([mk(u)[:, None], mk(v)[None, :]]), s.curvature([mk(u)[:, None], mk(v)[None, :]])
        assert tuple(n2.shape) == (3, 37, 41) and tuple(c2.shape) == (37, 41)
        n2, c2 = (_np(x) if torch.is_tensor(x) else x for x in (n2, c2))
        assert sr.same_bits(n2.reshape(3, -1), flat_n) and sr.same_bits(c2.reshape(-1), flat_c)
    # indices= on a non-fused spline: the selected cofactors, divided by the norm of THAT vector (reference :234-244)
    area = s.normal([U, V], False)
    for indices in ([0, 2], [1]):
        want = area[indices] / np.sqrt((area[indices] ** 2).sum(0))
        for got in (s.normal([U, V], True, indices), _np(s.normal([torch.as_tensor(U, device="cuda"), torch.as_tensor(V, device="cuda")], True, indices))):
            assert got.shape == want.shape and np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps
        assert sr.same_bits(s.normal([U, V], False, indices), area[indices])
        one = oracle.py_normal(c.order, c.nCoef, c.knots, c.coefs, [U[5], V[5]], True, False, indices)
        assert np.abs(s.normal([U[5], V[5]], True, indices) - one).max() <= 1e-12
    flipped = Spline(c.nInd, c.nDep, c.order, c.nCoef, c.knots, c.coefs, {"negateNormal": True})
    assert sr.same_bits(flipped.normal([U, V]), -flat_n) and sr.same_bits(flipped.normal([U, V], False), -area)
    # an outside point: the reference's ValueError, from NumPy and from CUDA inputs alike
    Ub = U.copy()
    Ub[123] = dom[0][1] + 1.0
    text = f"Spline evaluation outside domain: {np.atleast_1d([float(Ub[123]), float(V[123])])}"
    for mk in (lambda a: a, lambda a: torch.as_tensor(a, device="cuda")):
        for fn in (s.normal, s.curvature):
            with pytest.raises(ValueError) as e:
                fn([mk(Ub), mk(V)])
            assert type(e.value) is ValueError and str(e.value) == text, (fn.__name__, str(e.value))


def test_curvature_device_rejects_a_wrong_out():
    """A wrong dtype, size or a non-contiguous out= raises before any launch (no kernel ever sees the buffer)."""
    c = CASES[C33]
    t = DeviceSpline(c.order, c.nCoef, c.knots, c.coefs, c.dt)
    tp = _dev([p[:100] for p in c.points()])
    good = t.curvature_device(tp, out=torch.empty(100, dtype=torch.float64, device="cuda"))
    before = t.last_kernel()
    t.evaluate_device(tp)
    marker = t.last_kernel()
    assert marker != before
    for out in (torch.empty(100, dtype=torch.float32, device="cuda"), torch.empty(99, dtype=torch.float64, device="cuda"),
                torch.empty(101, dtype=torch.float64, device="cuda"), torch.empty(200, dtype=torch.float64, device="cuda")[::2]):
        with pytest.raises(ValueError):
            t.curvature_device(tp, out=out)
        assert t.last_kernel() == marker, "a launch happened before the check"
    assert sr.same_bits(_np(t.curvature_device(tp)), _np(good))
