"""
The CPU half of the integral sweep (tests/integral_sweep.py; the device half is tests/test_gpu_integral_sweep.py).

    coverage    the generated case table reaches every instantiation of ``integral_regions`` (the dispatch is restated:
                dtype, nInd, bucket of the highest order), every order tuple, measure branch, staging side, degenerate
                case and knot pattern of the list in ``test_every_instantiation_and_branch_is_listed``
    constants   W, CAP, DG, BLOCK and the Gauss-Kronrod tables restated in integral_sweep.py are the sources', by text
    reference   the longdouble reference agrees with ``fractions.Fraction`` arithmetic on a sample of nodes of every case
                to 2^-60 of sum |c| B (knots are dyadic, coefficients are eighths)
    precondition mu >= 0.1 prod ||v|| at every node of every non-degenerate case (the bars are as sharp as that)
    oracle      the bars hold for the reference alone: ``oracle.c_evaluate`` / ``c_jacobian`` lie within the per-node bars
                of x and J, ``integral_ref.region_sums`` within the per-region bars of K and G, on every case.  With fp32
                knots and coefficients the oracle evaluates x and J in fp32; ``region_sums`` then forms the measure, the
                weights and the sums in fp64 whatever the spline's type is, so against the fp32 bars of mu, K and G it
                tests the jacobian's share only.
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import integral_sweep as isw
import oracle
from bspy_amd import integral as iq
from conftest import ROOT, observe
from integral_ref import ORACLE_NDEP, region_sums

CSRC = os.path.join(ROOT, "bspy_amd", "csrc")


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_restated_constants_are_the_sources():
    for name, lines in isw.SOURCE_TEXT.items():
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for line in lines:
            assert text.count(line) == 1, (name, line)
        if name == "bsk_integral.hpp":
            for key, want in (("GK_X", isw.GK_X), ("GK_WK", isw.GK_WK), ("GK_WG", isw.GK_WG)):
                body = re.search(rf"__constant__ double {key}\[GK_N\] = \{{(.*?)\}};", text, re.S).group(1)
                assert [float(v) for v in body.split(",")] == want.tolist() == getattr(iq, key).tolist(), key
    assert [isw.staging((B,) * n)[2] for n in (1, 2, 3) for B in isw.BUCKETS] == [512, 256, 128, 128, 32, 8, 32, 4, 1]
    assert [isw.block_of(n) for n in (1, 2, 3)] == [64, 256, 256]
    for orders in isw.NODIV.values():
        W, CAP, DG = isw.staging(orders)
        assert CAP % W != 0 and DG == CAP // W


def test_every_instantiation_and_branch_is_listed():
    assert len(isw.INSTANCES) == 18 and len(set(isw.CASE_IDS)) == len(isw.CASES)
    for inst in isw.INSTANCES:
        # the dispatch of bsk_integral_tu.hip restated: dtype, nInd, bucket of the highest order
        mine = [c for c in isw.CASES if (c.dtype, c.nInd, next(b for b in (4, 8, 16) if max(c.orders) <= b)) == inst]
        assert mine and all(c.bucket == inst.bucket for c in mine)
        n, B = inst.nInd, inst.bucket
        tuples = {c.orders for c in mine}
        assert (B,) * n in tuples
        assert any(max(t) == isw.LOWEST_MAX[B] for t in tuples)
        for p in range(n if n > 1 else 0):
            assert any(t[p] == B and all(v < B for i, v in enumerate(t) if i != p) and 2 in t for t in tuples), (inst, p)
        if B == 4:
            assert any(1 in t for t in tuples)
            assert any(isw.is_exact_zero(c) for c in mine)
        branches = {isw.branch(c) for c in mine}
        assert branches >= ({"eq", "gt"} if n == 1 else {"lt", "eq", "gt"}), inst
        if n == 3:
            assert {1, 2} <= {c.nDep for c in mine}
        DG = isw.staging((B,) * n)[2]
        assert {(c.nDep, c.stage) for c in mine if c.kind == "allmax"} == {(DG, "DG"), (DG + 1, "DG+1")}
    for dt in isw.DTYPES:
        for n in (1, 2, 3):
            mine = [c for c in isw.CASES if c.dtype == dt and c.nInd == n]
            DG = isw.staging(isw.NODIV[n])[2]
            assert {(c.orders, c.nDep) for c in mine if c.kind == "nodiv"} == {(isw.NODIV[n], DG), (isw.NODIV[n], DG + 1)}
            if n >= 2:
                assert {"line", "equal"} <= {c.kind for c in mine}
                assert {isw.branch(c) for c in mine if c.kind == "line"} == ({"eq", "gt"} if n == 2 else {"lt", "eq", "gt"})
            # knots: a negative domain start and one above 1, a double knot, multiplicity order - 1 and multiplicity order
            los = {isw.domain_lo(c, i) for c in mine for i in range(n)}
            assert min(los) < 0 and max(los) > 1
            mults = [isw.multiplicities(o) for c in mine for o in c.orders]
            assert any(m[2] == 2 and m[2] < m[0] for m in mults) and all(m[3] == max(m[0] - 1, 1) and m[4] == m[0] for m in mults)
    # every case is both a MEASURE and a NODES case in the device half; none is marked
    assert all(isinstance(i, str) for i in isw.CASE_IDS)


def check_geometry(case, b):
    n = case.nInd
    R = len(b.lo_hi)
    assert R >= 3 and b.lo_hi.dtype == np.dtype(case.dtype) and b.span.shape == (R, n)
    assert (b.lo_hi[:, :, 0] < b.lo_hi[:, :, 1]).all()                                     # also the deep child, in T
    for i in range(n):
        k, o = b.knots[i], b.order[i]
        assert k.dtype == np.dtype(case.dtype) and (k.astype(np.float64) * 4 == np.rint(k.astype(np.float64) * 4)).all()
        assert (np.diff(k) >= 0).all() and (k[:o] == k[0]).all() and (k[-o:] == k[-1]).all()
        sp = b.span[:, i]
        assert (sp >= o).all() and (sp <= b.nCoef[i]).all()
        assert (k[sp - 1] <= b.lo_hi[:, i, 0]).all() and (b.lo_hi[:, i, 1] <= k[sp]).all() and (k[sp - 1] < k[sp]).all()
        lo, hi, span = iq.cells(isw.spline_of(b), iq.check_domain(isw.spline_of(b), None))[i]
        assert list(span) == list(np.cumsum(isw.multiplicities(o))[:5]) and list(lo) == list(b.breaks[i][:5])
    assert (b.span == np.array(b.nCoef)).all(axis=1).sum() >= 2                            # the last cell and its deep child
    depth = isw.DEEP[np.dtype(case.dtype)]
    width = (b.lo_hi[:, :, 1] - b.lo_hi[:, :, 0]).astype(np.float64)
    assert any((width[r] == np.array([isw.WIDTHS[4]] * n) * 2.0 ** -depth).all() for r in range(R))
    full = 8 + 2 ** n
    if R == full:
        for i in range(n):
            assert set(b.span[:, i]) == set(np.cumsum(isw.multiplicities(b.order[i]))[:5])
    assert (b.c8 == np.rint(b.coefs.astype(np.float64) * 8)).all()                             # eighths, exact in T


def check_exact(case, b):
    """x and J of the longdouble reference against Fraction arithmetic on a sample of nodes, to 2^-60 of the sums of
    absolute values."""
    W = isw.staging(case.orders)[0]
    nodes = [1, 13] if W > 512 else [0, 7, 13]
    deps = sorted({0, case.nDep - 1})
    worst = 0.0
    for r in ([0] if W > 512 else [0, 1]):
        _, x, J, Sx, SJ, _ = isw.values_and_jacobian(b, r, isw.LD(0), nodes, deps)
        ex, eJ = isw.values_and_jacobian(b, r, Fraction(0), nodes, deps)
        pairs = [(x, ex, Sx)] + [(J[i], eJ[i], SJ[i]) for i in range(case.nInd)]
        for got, want, S in pairs:
            for g, w, s in zip(got.ravel(), want.ravel(), S.ravel()):
                hi = float(g)
                err = abs(Fraction(hi) + Fraction(float(g - isw.LD(hi))) - w)
                bar = Fraction(float(s)) / 2 ** 60
                assert err <= bar, (isw.case_id(case), r, float(err), float(bar))
                if err:
                    worst = max(worst, float(err / bar))
    observe(f"integral sweep reference: {isw.tag(case.dtype)}, longdouble against exact / (2^-60 sum |c| B)", worst, 1.0)


def check_oracle(case, b, ref):
    n, R = case.nInd, len(b.lo_hi)
    jgrid = np.indices((isw.GK_N,) * n).reshape(n, -1)
    pts = [np.ascontiguousarray(ref.u[:, i, :][:, jgrid[i]].reshape(-1)) for i in range(n)]
    xs, js = [], []
    for d in range(0, case.nDep, ORACLE_NDEP):
        part = b.coefs[d:d + ORACLE_NDEP]
        x, bad = oracle.c_evaluate(b.order, b.nCoef, b.knots, part, [0] * n, pts)
        j, bad2 = oracle.c_jacobian(b.order, b.nCoef, b.knots, part, pts)
        assert bad == -1 and bad2 == -1 and x.dtype == j.dtype == np.dtype(case.dtype)
        xs.append(x)
        js.append(j)
    x = np.concatenate(xs).reshape(case.nDep, R, -1).transpose(1, 2, 0)
    J = np.concatenate(js).reshape(case.nDep, n, R, -1).transpose(2, 3, 0, 1)
    label = isw.instance_label(case).replace("sweep:", "sweep oracle:")
    observe(label + " x", isw.ratio(x, ref.x, ref.bar_x), 1.0)
    observe(label + " J", isw.ratio(J, ref.J, ref.bar_J), 1.0)
    K, G = region_sums(isw.spline_of(b), b.lo_hi, b.span)
    observe(label + " K", isw.ratio(K, ref.K, ref.bar_K), 1.0)
    observe(label + " G", isw.ratio(G, ref.G, ref.bar_G), 1.0)


@pytest.mark.parametrize("case", isw.CASES, ids=isw.CASE_IDS)
def test_case_reference_precondition_and_oracle(case):
    b = isw.build(case)
    check_geometry(case, b)
    check_exact(case, b)
    ref = isw.reference(b)
    assert all(np.isfinite(np.asarray(a, np.float64)).all() for a in ref)
    if isw.is_exact_zero(case):
        assert (ref.mu == 0).all() and (ref.K == 0).all() and (ref.G == 0).all()
    if isw.is_degenerate(case):
        assert (ref.mu <= ref.bar_mu).all()                                                # 0 in exact arithmetic
    else:
        assert (ref.mu >= 0.1 * ref.norms).all(), float((ref.mu / ref.norms).min())
    check_oracle(case, b, ref)
