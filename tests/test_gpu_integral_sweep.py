"""
The device half of the integral sweep: every instantiation of ``integral_regions<T, NIND, OMAX>`` (18: fp32 / fp64 x nInd 1 - 3
x order bucket 4 / 8 / 16) through ``DeviceSpline.integral_regions`` - the kernel without the adaptive driver - on the cases
of tests/integral_sweep.py, one test id per case (dtype, nInd, bucket, orders, nDep, measure branch lt / eq / gt, kind and
staging side DG / DG+1 are in the id).  Every case runs both modes:

    NODES      x, wK mu and wG mu of every node against the longdouble reference at the counted bars
    MEASURE    K and G against ``math.fsum`` of the same call's NODES columns at the summation bar, and against the reference
    bytes      a second MEASURE call, the batch reversed, the batch concatenated with itself (both modes), and the x column
               of a dependent against the one-dependent spline made from it (first and last dependent of the first and of the
               second stage): the same instruction sequences, no tolerance
    degenerate finite, 0 <= wK mu <= bar; exactly 0 where an order-1 variable makes a zero column and nDep >= nInd

Every observed / bar ratio is recorded per instantiation (``conftest.observe``).  J itself is not an output of the kernel:
its bars are held on the CPU (the oracle) and enter here through mu.
"""
import numpy as np
import pytest

import integral_sweep as isw
from bspy_amd.device_spline import DeviceSpline
from conftest import observe

pytestmark = pytest.mark.gpu


def run(b, coefs, fn):
    ds = DeviceSpline(b.order, b.nCoef, b.knots, coefs, b.case.dtype)
    try:
        return fn(ds)
    finally:
        ds.close()


@pytest.mark.parametrize("case", isw.CASES, ids=isw.CASE_IDS)
def test_integral_regions_case(case):
    b = isw.build(case)
    ref = isw.reference(b)
    R, NN = len(b.lo_hi), isw.GK_N ** case.nInd
    back = slice(None, None, -1)
    lo_hi2, span2 = np.concatenate([b.lo_hi, b.lo_hi]), np.concatenate([b.span, b.span])

    def calls(ds):
        sums = ds.integral_regions(b.lo_hi, b.span)
        nodes = ds.integral_regions(b.lo_hi, b.span, nodes=True)
        assert isw.bits(ds.integral_regions(b.lo_hi, b.span)) == isw.bits(sums), "two MEASURE calls differ"
        for mode, base in ((False, sums), (True, nodes)):
            assert isw.bits(ds.integral_regions(b.lo_hi[back], b.span[back], nodes=mode)[back]) == isw.bits(base), ("reversed", mode)
            twice = ds.integral_regions(lo_hi2, span2, nodes=mode)
            assert isw.bits(twice[:R]) == isw.bits(base) and isw.bits(twice[R:]) == isw.bits(base), ("doubled", mode)
        return sums, nodes

    sums, nodes = run(b, b.coefs, calls)
    assert sums.shape == (R, 2) and nodes.shape == (R, NN, case.nDep + 2) and sums.dtype == nodes.dtype == np.float64
    assert np.isfinite(sums).all() and np.isfinite(nodes).all()
    for d in isw.bitwise_dependents(case):
        alone = run(b, b.coefs[d:d + 1], lambda ds: ds.integral_regions(b.lo_hi, b.span, nodes=True))
        assert isw.bits(alone[:, :, 0]) == isw.bits(nodes[:, :, d]), f"x of dependent {d} differs from the one-dependent spline"
    fk, fg = nodes[:, :, -2], nodes[:, :, -1]
    assert (fk >= 0).all() and (fg >= 0).all() and (sums >= 0).all()
    if isw.is_exact_zero(case):
        assert not fk.any() and not fg.any() and not sums.any()
    if isw.is_degenerate(case):
        assert (fk.astype(isw.LD) <= ref.bar_fk).all() and (fg.astype(isw.LD) <= ref.bar_fg).all()
    per_node = isw.node_ratios(ref, nodes)
    against_nodes = isw.measure_against_nodes(case.nInd, sums, nodes)
    against_ref = isw.measure_ratios(ref, sums)
    label = isw.instance_label(case)
    failed = []
    for name, value in (("x", per_node["x"]), ("mu", per_node["mu"]), ("mu (wG)", per_node["muG"]), ("K", against_ref["K"]),
                        ("G", against_ref["G"]), ("K against fsum of NODES", against_nodes["K"]),
                        ("G against fsum of NODES", against_nodes["G"])):
        try:
            observe(f"{label} {name}", value, 1.0)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed
