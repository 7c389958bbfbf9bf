"""
Parity away from unit scale.  (CPU preconditions: tests/test_scale_host.py; inputs: cases.scale_cases; yardstick and
transforms: tests/scale_ref.py.)

A. Exact scaling laws, one case per kernel family (the enumeration of tests/test_gpu_stale_lds.py).  Coefficients
   x 2^kc and knots / parameters x 2^kp change derivative(w) by exactly 2^(kc - kp |w|) in the reference's arithmetic -
   every rounding commutes with a power of two, whatever the summation order or FMA contraction - and the C oracle is
   bitwise so on these very inputs (host module).  A kernel that is not contains an absolute constant, a
   magnitude-dependent branch or a denormal flush.  Asserted bit for bit after undoing the scale: one scale for all
   coefficients (both signs), one per dependent row, the parameter scale for the value, a first and the highest
   non-zero derivative, the unit normal (unchanged), NaN positions and the out-of-domain index (unchanged), and the
   kernel named before and after.
   Families moved off the bitwise law: none.

B. Shifted and stretched domains against the extended-precision restatement of the reference.  d_gpu and d_orc are the
   distances of the GPU result and of the fp64 (fp32) oracle from it, relative to max |result| (no floor of 1: a value
   scale of 1e-6 gets no free pass); d_gpu <= max(4 d_orc, 1e-12) (fp32: max(4 d_orc32, 2e-5)), and the contract's
   1e-10 unconditionally.  The domains near the acceptance edge of the table-free uniform-knot kernels are the point.

C. Ill-scaled coefficient fields on the unclamping paths: the outermost control-point layer x 2^20 per end and variable
   and on all ends; the whole sample against the global scale (bar B), and the points whose support holds no multiplied
   control point against the scale of the UNmultiplied spline, on the uniform kernels and on the general ones.
"""
import numpy as np
import pytest

import cases
import oracle
import bspy_amd
import scale_ref as sr
from bspy_amd import DeviceSpline, Spline
from bspy_amd import integral as iq
from conftest import observe
from test_scale_host import uniform_path_expected

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SC = cases.scale_cases()
FAMILIES = {f.name: f for f in SC["families"]}
POINT_FAMILIES = sorted(n for n, f in FAMILIES.items() if f.n)
GRID_FAMILIES = sorted(n for n, f in FAMILIES.items() if f.grid is not None)
BAD_AT = sr.NAN_AT + 12          # the out-of-domain parameter of the domain-error run


def _kernel_ok(got, want):
    return got == want if not want.endswith("*") else want[:-1] in got


def _make(order, ncoef, knots, coefs, dt, monkeypatch, variant=None):
    if variant is not None:
        monkeypatch.setenv("BSK_VARIANT", variant)
    try:
        return DeviceSpline(order, ncoef, knots, coefs, dt)
    finally:
        if variant is not None:
            monkeypatch.delenv("BSK_VARIANT")


def _np(x):
    return x.detach().cpu().numpy()


def _differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"shapes {a.shape} / {b.shape}"
    nan = np.isnan(a) | np.isnan(b)
    diff = (a != b) & ~nan
    return (f"{int(diff.sum())} of {a.size} values differ, NaN masks {'equal' if np.array_equal(np.isnan(a), np.isnan(b)) else 'DIFFER'}, "
            f"largest relative difference {float(np.max(np.abs(a[diff] - b[diff]) / np.abs(b[diff]), initial=0.0)):.2e}")


def _assert_law(base, runs, fam, what):
    """runs: (label, kcs, kp, uniform, results); results and base: {(kind, wrt): array}."""
    for label, kcs, kp, uniform, res in runs:
        for (kind, w), got in res.items():
            e = sr.call_exponent(kind, w, kcs, kp, fam.nInd, uniform)
            if e is None:
                continue
            back = sr.undo_law(got, e)
            assert sr.same_bits(back, base[(kind, w)]), \
                f"{what}: {kind} {w} under [{label}] is not the unscaled result x 2^{np.unique(e)}: {_differing(back, base[(kind, w)])}"


# ------------------------------------------------------------------------------------------ A: point kernels
def _run_points(fam, spec, monkeypatch):
    order, ncoef, knots, coefs, pts = spec
    t = _make(order, ncoef, knots, coefs, fam.dt, monkeypatch, fam.variant)
    tp = [torch.as_tensor(p, device="cuda") for p in pts]
    out = {}
    for kind, w, kernel in fam.calls:
        if kind == "eval":
            r = t.evaluate_device(tp, list(w))
        elif kind == "jac":
            r = t.jacobian_device(tp)
        elif kind == "normal":
            r = t.normal_device(tp)
        else:
            r = t.curvature_device(tp)
        torch.cuda.synchronize()
        assert _kernel_ok(t.last_kernel(), kernel), (fam.name, kind, w, t.last_kernel())
        out[(kind, w)] = _np(r)
    # the out-of-domain index: one parameter beyond the top of the domain (it scales with the knots)
    bad = [p.copy() for p in pts]
    top = knots[-1][ncoef[-1]]
    bad[-1][BAD_AT] = top + (top - knots[-1][order[-1] - 1])
    with pytest.raises(bspy_amd.DomainError) as e:
        t.evaluate_device([torch.as_tensor(p, device="cuda") for p in bad])
    assert e.value.index == BAD_AT, (fam.name, e.value.index)
    return out


@pytest.mark.parametrize("name", POINT_FAMILIES)
def test_scaling_law_point_kernels(name, monkeypatch):
    fam = FAMILIES[name]
    spec = (fam.order, fam.nCoef, fam.knots, fam.coefs, sr.family_points(fam))
    base = _run_points(fam, spec, monkeypatch)
    # the unscaled run is the function: value and first derivative at its front (knot points, NaN parameters) against
    # the oracle at the usual bar (higher derivatives: bitwise below, their accuracy is test_gpu_parity.py's subject)
    m = 8_000
    for (kind, w), got in base.items():
        if kind != "eval" or sum(w) > 1:
            continue
        ref, _ = oracle.c_evaluate(fam.order, fam.nCoef, fam.knots, fam.coefs, list(w), [p[:m] for p in spec[4]])
        assert np.array_equal(np.isnan(got[:, :m]), np.isnan(ref)), (name, w)
        ok = ~np.isnan(ref)
        observe(f"scale A: {name} vs oracle, unscaled, {fam.kind}", np.abs(got[:, :m][ok] - ref[ok]).max() / max(1.0, np.abs(ref[ok]).max()),
                2e-5 if fam.dt == np.float32 else 1e-12)
    for label, kcs, kp, uniform in sr.family_transforms(fam, SC["exponents"], SC["rows"]):
        _assert_law(base, [(label, kcs, kp, uniform, _run_points(fam, sr.transformed(spec, kcs, kp), monkeypatch))], fam, name)


@pytest.mark.parametrize("path,n", [("small", 20_011), ("staged", 150_001), ("pipelined", (1 << 21) + 5)])
def test_scaling_law_host_paths(path, n):
    """The cfg2 spline through the three host paths (NumPy in, NumPy out): the same law, bit for bit."""
    fam = FAMILIES["eval_uni / jac_uni"]
    pts = sr.sample_points(fam.order, fam.nCoef, fam.knots, n, fam.dt, np.random.default_rng(n))
    pts[0][sr.NAN_AT] = np.nan
    spec = (fam.order, fam.nCoef, fam.knots, fam.coefs, pts)

    def run(spec):
        order, ncoef, knots, coefs, pts = spec
        t = DeviceSpline(order, ncoef, knots, coefs, fam.dt)
        out = {}
        for w in ((0, 0), (0, 1), (3, 0)):
            out[("eval", w)] = t.evaluate(pts, list(w)).copy()
            assert t.last_kernel() == "eval_uni"
        out[("jac", None)] = t.jacobian(pts).copy()
        assert t.last_kernel() == "jac_uni"
        bad = [p.copy() for p in pts]
        bad[0][n - 3] = knots[0][-1] * 2 + 1
        with pytest.raises(bspy_amd.DomainError) as e:
            t.evaluate(bad)
        assert e.value.index == n - 3
        return out
    base = run(spec)
    for label, kcs, kp, u in sr.family_transforms(fam, SC["exponents"], SC["rows"]):
        _assert_law(base, [(label, kcs, kp, u, run(sr.transformed(spec, kcs, kp)))], fam, f"cfg2, {path} host path")


# ------------------------------------------------------------------------------------------ A: grids, tessellation
def _run_grid(fam, spec, axes, monkeypatch):
    order, ncoef, knots, coefs, _ = spec
    t = _make(order, ncoef, knots, coefs, fam.dt, monkeypatch, fam.variant)
    ta = [torch.as_tensor(a, device="cuda") for a in axes]
    out = {}
    for kind, w, kernel in fam.calls:
        if kind == "grid":
            r = t.evaluate_grid_device(ta, list(w))
            torch.cuda.synchronize()
            assert _kernel_ok(t.last_kernel(), kernel), (fam.name, t.last_kernel())
            out[(kind, w)] = _np(r)
        else:
            for key, value in fam.env.items():
                monkeypatch.setenv(key, value)
            try:
                r = bspy_amd.tessellate_tables([t], ta, normals=kind == "tessn", normalize=True)
            finally:
                for key in fam.env:
                    monkeypatch.delenv(key)
            torch.cuda.synchronize()
            assert t.last_kernel() == kernel, (fam.name, t.last_kernel())
            if kind == "tessn":
                out[("tess", None)], out[("tessn", None)] = _np(r[0])[0], _np(r[1])[0]
            else:
                out[("tess", None)] = _np(r)[0]
    return out


@pytest.mark.parametrize("name", GRID_FAMILIES)
def test_scaling_law_grid_kernels(name, monkeypatch):
    fam = FAMILIES[name]
    axes = sr.family_axes(fam)
    spec = (fam.order, fam.nCoef, fam.knots, fam.coefs, axes)           # the axes ride in the points' slot: they scale alike
    base = _run_grid(fam, spec, axes, monkeypatch)
    mesh = [m.ravel() for m in np.meshgrid(*axes, indexing="ij")]
    key = ("grid", fam.calls[0][1]) if fam.calls[0][0] == "grid" else ("tess", None)
    ref, bad = oracle.c_evaluate(fam.order, fam.nCoef, fam.knots, fam.coefs, [0] * fam.nInd, mesh)
    assert bad == -1
    observe(f"scale A: {name.split(',')[0]} vs oracle, unscaled, {fam.kind}", np.abs(base[key].reshape(ref.shape) - ref).max() / max(1.0, np.abs(ref).max()),
            2e-5 if fam.dt == np.float32 else 1e-12)
    runs = []
    for label, kcs, kp, uniform in sr.family_transforms(fam, SC["exponents"], SC["rows"]):
        tspec = sr.transformed(spec, kcs, kp)
        runs.append((label, kcs, kp, uniform, _run_grid(fam, tspec, tspec[4], monkeypatch)))
    _assert_law(base, runs, fam, name)


# ------------------------------------------------------------------------------------------ A: quadrature, fits
def test_scaling_law_integral_regions():
    """One Gauss-Kronrod round in MEASURE mode (not the adaptive driver: its absolute tolerance legitimately changes
    its path): Kronrod and Gauss sums x 2^(nInd kc), the parameter scale cancels."""
    fam = FAMILIES["integral_regions"]

    def run(knots, coefs):
        s = Spline(fam.nInd, fam.nDep, fam.order, fam.nCoef, knots, coefs)
        lo_hi, span = iq.split(*iq.regions(s, iq.check_domain(s, None)))
        t = s.device_tables()
        out = t.integral_regions(lo_hi, span)
        assert t.last_kernel() == "integral_regions"
        return {("integral", None): out}
    base = run(fam.knots, fam.coefs)
    assert np.isfinite(base[("integral", None)]).all() and (base[("integral", None)] > 0).all()
    runs = []
    for label, kcs, kp, uniform in sr.family_transforms(fam, SC["exponents"], SC["rows"]):
        if uniform:
            _, _, knots, coefs, _ = sr.transformed((fam.order, fam.nCoef, fam.knots, fam.coefs, []), kcs, kp)
            runs.append((label, kcs, kp, uniform, run(knots, coefs)))
    _assert_law(base, runs, fam, "integral_regions")


@pytest.mark.parametrize("system", SC["fit"][0], ids=lambda s: f"order{s[0]}-{s[3]}x{s[4]}")
def test_scaling_law_fit_kernels(system):
    """fit_sweep / fit_sweep turned / fit_residual: data x 2^k gives coefficients x 2^k and residual sums x 2^2k."""
    plan, first, values, b = sr.fit_system(*system)
    outer, inner = system[3], system[4]
    turned = inner == 1 and outer > 1

    def run(b):
        tb = torch.as_tensor(b, device="cuda")
        x = plan.sweep(tb, outer, inner)
        assert plan.last_kernel() == ("fit_sweep turned" if turned else "fit_sweep")
        rows = plan.residual_rows(tb, x, outer, inner)
        assert plan.last_kernel() == ("fit_residual turned" if turned else "fit_residual")
        return _np(x), rows
    x0, r0 = run(b)
    want = plan.solve_host(b, outer, inner)
    observe("scale A: fit_sweep vs host plan, unscaled", np.abs(x0 - want).max() / np.abs(want).max(), 1e-10)
    for k in SC["fit"][1]:
        xk, rk = run(np.ldexp(b, k))
        assert sr.same_bits(np.ldexp(xk, -k), x0), f"fit_sweep{' turned' if turned else ''}, data x 2^{k}: {_differing(np.ldexp(xk, -k), x0)}"
        assert sr.same_bits(np.ldexp(rk, -2 * k), r0), f"fit_residual{' turned' if turned else ''}, data x 2^{k}: {_differing(np.ldexp(rk, -2 * k), r0)}"


# ------------------------------------------------------------------------------------------ B: shifted domains
def _bars(dt):
    return (2e-5, None) if dt == np.float32 else (1e-12, 1e-10)


def _yardstick_check(label, t, spec, kernels, dt, y, sel=None, scales=None, check_kernel=True):
    """Evaluate every multi-index of y and the jacobian on the device; each distance from the extended result printed,
    then asserted: the contract's bar, then max(4 d_orc, floor).  sel: the points to judge; scales: per multi-index
    scale to judge against (default: y's own).  Returns the worst d_gpu."""
    order, ncoef, knots, coefs, pts = spec
    floor, contract = _bars(dt)
    tp = [torch.as_tensor(p, device="cuda") for p in pts]
    sel = slice(None) if sel is None else sel
    worst = 0.0
    firsts = [tuple(int(i == j) for i in range(len(order))) for j in range(len(order))]
    jac = _np(t.jacobian_device(tp))
    if check_kernel:
        assert t.last_kernel() == kernels[1], (label, t.last_kernel(), kernels)
    results = [(w, "".join(map(str, w)), None) for w in y] + [(w, "jacobian column " + str(j), jac[:, j]) for j, w in enumerate(firsts)]
    for w, what, got in results:
        ext, orc, scale, _ = y[w]
        scale = scale if scales is None else scales[w]
        if got is None:
            got = _np(t.evaluate_device(tp, list(w)))
            if check_kernel:
                assert t.last_kernel() == kernels[0], (label, w, t.last_kernel(), kernels)
        assert np.isfinite(got).all(), (label, what)
        d_orc = sr.distance(orc[:, sel], ext[:, sel], scale)
        d_gpu = sr.distance(got[:, sel], ext[:, sel], scale)
        print(f"{label}: {what}: d_gpu {d_gpu:.2e}  d_orc {d_orc:.2e}  scale {scale:.2e}")
        worst = max(worst, d_gpu)
        if contract is not None:
            observe(f"{label}, contract", d_gpu, contract)
        observe(label, d_gpu, max(4.0 * d_orc, floor))
    return worst


def _domain_id(d):
    return f"{d[0]:g}+{d[1]:g}"


def _shifted(spl, lo, width):
    spec = sr.shifted(spl, lo, width, SC["sample"])
    took, dev = uniform_path_expected(spl, lo, width)
    kernels = spl.uni if took else spl.general
    label = f"scale B: {kernels[0]} / {kernels[1]}, {spl.name}, [{lo:g}, {lo:g} + {width:g}]"
    y = sr.yardstick(spec, sr.yardstick_wrts(spl.order), oracle.c_evaluate)
    t = DeviceSpline(spl.order, spl.nCoef, spec[2], spec[3], spl.dt)
    _yardstick_check(label, t, spec, kernels, spl.dt, y)


@pytest.mark.parametrize("dom", SC["domains"], ids=_domain_id)
@pytest.mark.parametrize("name", [s.name for s in SC["splines"]])
def test_shifted_domain(name, dom):
    _shifted({s.name: s for s in SC["splines"]}[name], *dom)


@pytest.mark.parametrize("dom", SC["domains_f32"], ids=_domain_id)
@pytest.mark.parametrize("name", [s.name for s in SC["splines_f32"]])
def test_shifted_domain_fp32(name, dom):
    _shifted({s.name: s for s in SC["splines_f32"]}[name], *dom)


# ------------------------------------------------------------------------------------------ C: ill-scaled layers
@pytest.mark.parametrize("name", [s.name for s in SC["illscaled"]])
def test_illscaled_boundary_layers(name, monkeypatch):
    spl = {s.name: s for s in SC["illscaled"]}[name]
    order, ncoef, knots, coefs, pts = sr.shifted(spl, 0.0, 1.0, SC["sample"])
    nind = len(order)
    wrts = sr.yardstick_wrts(order)[:1 + nind]                      # value and first derivatives (= the jacobian)
    y0 = sr.yardstick((order, ncoef, knots, coefs, pts), wrts, oracle.c_evaluate)
    scales0 = {w: v[2] for w, v in y0.items()}
    ix = sr.span_indices(order, knots, pts)
    ends = [(iv, e) for iv in range(nind) for e in (0, 1)]
    general = "9" if spl.general[0] == "eval_rowrot" else "4"
    for which in [[e] for e in ends] + [ends]:
        c2, mask = sr.multiply_layers(coefs, which)
        spec = (order, ncoef, knots, c2, pts)
        clean = sr.support_is_clean(order, mask, ix)
        assert 0.2 < clean.mean() < 1.0, (name, which, clean.mean())
        y2 = sr.yardstick(spec, wrts, oracle.c_evaluate)
        tag = "all ends" if len(which) > 1 else f"variable {which[0][0]} {'low' if which[0][1] == 0 else 'high'} end"
        t = DeviceSpline(order, ncoef, knots, c2, spl.dt)
        _yardstick_check(f"scale C: {spl.uni[0]} / {spl.uni[1]}, {name}, layer x 2^20 at {tag}, whole sample", t, spec, spl.uni, spl.dt, y2)
        _yardstick_check(f"scale C: {spl.uni[0]} / {spl.uni[1]}, {name}, layer x 2^20 at {tag}, clean supports", t, spec, spl.uni, spl.dt, y2,
                         sel=clean, scales=scales0)
        tg = _make(order, ncoef, knots, c2, spl.dt, monkeypatch, general)
        _yardstick_check(f"scale C: {spl.general[0]} / {spl.general[1]}, {name}, layer x 2^20 at {tag}, clean supports", tg, spec, spl.general,
                         spl.dt, y2, sel=clean, scales=scales0)
