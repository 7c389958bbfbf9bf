"""
One case per rung of the two point-path ladders (dispatch_eval / dispatch_jac in bspy_amd/csrc/bsk_api.hip and the
large-table units behind them): each case evaluates, takes one first derivative and the jacobian, and asserts

  * the family ``last_kernel()`` names after each call, against the table below - recorded by running this test at
    the commit before the ladders were rewritten on one shape classifier, so a shape that moves to another rung fails here;
  * the values against ``oracle.c_evaluate`` / ``oracle.c_jacobian`` at the bars of test_gpu_parity.py: 1e-12 (fp64) and
    2e-5 (fp32) of the result scale.

Shapes are the smallest that reach the rung: 3000 points (no multiple of a tile, several workgroups), about ten
control points per variable for the LDS-resident rungs, a 180000-byte table (fp64, nDep 1, 150 x 150: just beyond the
160 KiB of LDS) for the large-table rungs.  The cell-order pipeline asks for 2^18 points and eval_slab2 for 2^19: those
three cases take 2^18 + 37 and 2^19 + 37.
"""
import numpy as np
import pytest

import cases
import oracle
from bspy_amd import DeviceSpline

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
N = 3000
N_CELL = (1 << 18) + 37
N_SLAB = (1 << 19) + 37

# name: (dtype, order, ncoef, nDep, knots, points, family of evaluate and of the derivative, family of the jacobian)
RUNGS = {
    "curve_order7":      (F64, (7,), (12,), 2, "general", N, "eval_stream", "jac_stream"),
    "curve_order10":     (F64, (10,), (14,), 2, "general", N, "eval_mixed", "eval_mixed"),                 # derivative passes
    "stream":            (F64, (3, 3), (10, 9), 3, "general", N, "eval_stream", "jac_stream"),
    "stream_uniform":    (F64, (3, 3), (10, 9), 3, "uniform", N, "eval_stream_uni", "jac_stream_uni"),
    "rowrot":            (F64, (4, 4), (10, 9), 3, "general", N, "eval_rowrot", "jac_rowrot"),
    "uniform":           (F64, (4, 4), (10, 9), 3, "uniform", N, "eval_uni", "jac_uni"),
    "rec32":             (F32, (4, 4), (10, 9), 3, "general", N, "eval_rec32", "jac_rowrot"),
    "fixed":             (F64, (6, 6), (12, 13), 3, "general", N, "eval_fixed", "jac_fixed"),
    "mixed":             (F64, (3, 4), (10, 9), 3, "general", N, "eval_mixed", "jac_mixed"),
    "volume_order5":     (F64, (5, 5, 5), (10, 10, 11), 2, "general", N, "eval_stream", "jac_fixed"),     # the jacobian's exception
    "generic":           (F64, (5, 5, 5, 5), (6, 6, 6, 6), 1, "general", N, "eval_generic", "eval_generic"),   # derivative passes
    "gather":            (F64, (4, 4), (150, 150), 1, "general", N, "eval_gather", "jac_fixed"),
    "slab":              (F64, (4, 4), (150, 150), 1, "general", N_SLAB, "eval_slab2", "eval_slab2"),       # derivative passes
    "cell_order":        (F64, (3, 3, 3), (42, 40, 44), 2, "general", N_CELL,
                          "cell-order pipeline (eval_cellsort, VALU)", "cell-order pipeline (eval_cellsort, VALU)"),   # derivative passes
    "cell_order_fused":  (F32, (3, 3, 3), (42, 40, 44), 2, "general", N_CELL,
                          "cell-order pipeline (eval_cellsort, MFMA)", "cell-order pipeline (eval_cellsort, MFMA, fused jacobian)"),
}


@pytest.mark.parametrize("name", sorted(RUNGS))
def test_rung_family_and_values(name):
    dt, order, ncoef, ndep, kind, n, eval_family, jac_family = RUNGS[name]
    rng = np.random.default_rng(sorted(RUNGS).index(name))
    if kind == "uniform":
        knots = [cases.clamped_uniform_knots(o, c, dt) for o, c in zip(order, ncoef)]
    else:
        knots = [cases.nonuniform_knots(rng, o, c, dt, 0.0, 1.0) for o, c in zip(order, ncoef)]
    coefs = rng.standard_normal((ndep, *ncoef)).astype(dt)
    pts = [rng.random(n).astype(dt) for _ in order]
    tol = 2e-5 if dt == F32 else 1e-12
    t = DeviceSpline(order, ncoef, knots, coefs, dt)
    first = [1] + [0] * (len(order) - 1)
    for w in ([0] * len(order), first):
        out = t.evaluate(pts, w)
        family = t.last_kernel()
        ref, bad = oracle.c_evaluate(order, ncoef, knots, coefs, w, pts)
        assert bad == -1
        err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
        print(f"{name} wrt {w}: {family}, error {err:.2e} of the scale (bar {tol:g})")
        assert family == eval_family, (name, w, family)
        assert err <= tol, (name, w, err)
    jac = t.jacobian(pts)
    family = t.last_kernel()
    ref, bad = oracle.c_jacobian(order, ncoef, knots, coefs, pts)
    assert bad == -1 and jac.shape == ref.shape == (ndep, len(order), n)
    err = np.abs(jac - ref).max() / max(1.0, np.abs(ref).max())
    print(f"{name} jacobian: {family}, error {err:.2e} of the scale (bar {tol:g})")
    assert family == jac_family, (name, family)
    assert err <= tol, (name, err)
