"""
Spline.zeros and roots.zeros_batch on the GPU (roots_flag, roots_isolate, band_apply_line for the extraction): every golden
of tests/golden/roots.npz through ``_path="device"`` (bars of tests/test_roots_host.py) with the kernels that ran asserted
from ``roots.LAST_PATHS`` and ``bsk_roots_last_kernel``, bit-equal to the host path and on a second run; then the layouts
of both kernels through ``zeros_batch`` on CUDA tensors against the host drivers, which run the same functions of
bsk_roots.hpp: bit for bit.  Neither kernel uses LDS, so the family has no stale-LDS test.
"""
import os
import sys

import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import roots
from test_roots_host import EPS, NAMES, check_golden, load_case, make_spline

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def bits(found):
    return [np.asarray(r).tobytes() for r in found]


def curve(rng, order, nspans, ncomp, dtype=np.float64, double_every=0, jump_every=0):
    """A clamped curve of `ncomp` components on `nspans` spans; interior knots are simple, but every `double_every`-th is
    double and every `jump_every`-th has full multiplicity (a jump)."""
    interior = np.sort(rng.random(nspans - 1))
    reps = np.ones(nspans - 1, int)
    if double_every and order > 2:
        reps[::double_every] = 2
    if jump_every:
        reps[1::jump_every] = order
    t = np.concatenate((order * [0.0], np.repeat(interior, reps), order * [1.0]))
    n = len(t) - order
    return bspy_amd.Spline(1, ncomp, [order], [n], [t], rng.standard_normal((ncomp, n)).astype(dtype))


def on_device(s):
    return torch.from_numpy(np.ascontiguousarray(s.coefs)).cuda()


def same_as_host(s, coefs=None, want_isolate=None):
    """zeros_batch on a CUDA tensor against the host drivers on the same numbers: equal bits, and the same launches: the
    second one runs exactly when the host path found a candidate (``want_isolate`` pins what the case is built for)."""
    d = on_device(s) if coefs is None else coefs
    values, offsets, intervals = roots.zeros_batch(s, coefs=d)
    ran = list(roots.LAST_PATHS)
    last = nv.lib().bsk_roots_last_kernel().decode()
    assert values.is_cuda and offsets.is_cuda
    host = bspy_amd.Spline(1, s.nDep, s.order, s.nCoef, s.knots, d.cpu().numpy())
    h_values, h_offsets, h_intervals = roots.zeros_batch(host, _path="host")
    isolates = "host roots_isolate" in roots.LAST_PATHS
    assert want_isolate is None or isolates == want_isolate
    plan = roots.BezierPlan(s.order[0], s.knots[0])
    assert ran == (["band_apply_line"] if plan.steps else []) + ["roots_flag"] + (["roots_isolate"] if isolates else [])
    assert last == ran[-1]
    assert offsets.cpu().numpy().tolist() == h_offsets.tolist()
    assert values.cpu().numpy().tobytes() == h_values.tobytes()
    assert intervals.tobytes() == h_intervals.tobytes()
    return h_values, h_offsets


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", NAMES)
def test_golden_device(name):
    c = load_case(name)
    host = make_spline(c).zeros(_path="host")
    isolates = "host roots_isolate" in roots.LAST_PATHS
    found = make_spline(c).zeros(_path="device")
    ran = list(roots.LAST_PATHS)
    plan = roots.BezierPlan(c["order"], make_spline(c).knots[0])
    assert ran == (["band_apply_line"] if plan.steps else []) + ["roots_flag"] + (["roots_isolate"] if isolates else [])
    assert nv.lib().bsk_roots_last_kernel().decode() == ran[-1]
    check_golden(c, found, "roots device")
    assert bits(found) == bits(host), "the device path and the host path differ"
    assert bits(make_spline(c).zeros(_path="device")) == bits(found), "two runs differ"


def test_goldens_reach_every_launch():
    ran = set()
    for name in NAMES:
        make_spline(load_case(name)).zeros(_path="device")
        ran |= set(roots.LAST_PATHS)
    assert ran == {"band_apply_line", "roots_flag", "roots_isolate"}


# ------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [2, 3, 4, 6, 8])
def test_layouts(order, dtype):
    """The smallest shapes at which the indexing of either kernel can go wrong: one span, one lane short of a wave, a wave, one
    more, more than a workgroup, many workgroups with a ragged end; one, few and an odd number of components.  float32
    rows reach the kernels as they are where no extraction is needed (order 2, one span) and widened elsewhere."""
    rng = np.random.default_rng(100 * order + np.dtype(dtype).itemsize)
    total = 0
    for nspans in (1, 63, 64, 65, 257, 1030):
        for ncomp in (1, 3, 37):
            s = curve(rng, order, nspans, ncomp, dtype)
            values, offsets = same_as_host(s)
            assert len(offsets) == ncomp + 1
            total += len(values)
    assert total > 1000


@pytest.mark.parametrize("order", [3, 4, 8])
def test_layouts_mixed_multiplicities(order):
    """Double knots and jumps: the span windows step by K - 1 and by K in one row."""
    rng = np.random.default_rng(order)
    for nspans, ncomp in ((65, 3), (257, 2)):
        same_as_host(curve(rng, order, nspans, ncomp, double_every=3, jump_every=7))


def test_misaligned_and_strided_input():
    rng = np.random.default_rng(9)
    for order, dtype in ((2, np.float32), (4, np.float64), (4, np.float32)):
        s = curve(rng, order, 130, 3, dtype)
        n = s.nCoef[0]
        base = torch.zeros(3 * n + 1, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
        base[1:] = on_device(s).reshape(-1)
        shifted = base[1:].view(3, n)                               # one element past the allocation's alignment
        assert shifted.data_ptr() % 16 != 0
        want, _ = same_as_host(s, shifted)
        wide = torch.zeros((3, n + 5), dtype=base.dtype, device="cuda")
        wide[:, 2:n + 2] = on_device(s)
        got, _ = same_as_host(s, wide[:, 2:n + 2])                  # rows that are not contiguous
        assert got.tobytes() == want.tobytes()


def test_no_candidates_skips_the_second_launch():
    rng = np.random.default_rng(3)
    s = curve(rng, 4, 300, 5)
    s.coefs[...] = np.abs(s.coefs) + 0.1
    values, offsets = same_as_host(s, want_isolate=False)
    assert len(values) == 0 and offsets.tolist() == [0] * 6
    assert s.nDep == 5 and bspy_amd.Spline(1, 1, s.order, s.nCoef, s.knots, s.coefs[:1]).zeros(_path="device") == []
    assert roots.LAST_PATHS == ["band_apply_line", "roots_flag"]


def test_every_span_is_a_candidate():
    rng = np.random.default_rng(4)
    s = curve(rng, 2, 1030, 3)
    s.coefs[...] = (np.abs(s.coefs) + 0.1) * (-1.0) ** np.arange(s.nCoef[0])
    values, offsets = same_as_host(s, want_isolate=True)
    assert offsets.tolist() == [0, 1030, 2060, 3090]
    breaks = np.unique(s.knots[0])
    for d in range(3):
        r = values[offsets[d]:offsets[d + 1]]
        assert np.all(r > breaks[:-1]) and np.all(r < breaks[1:])      # one root inside every span


def test_full_house_in_every_span():
    """K - 1 simple roots in each of 300 spans: the shifted Chebyshev polynomial T5 in Bernstein form, span after span
    (mirrored in every other span, so that the ends meet), on C0 knots."""
    c = load_case("chebyshev_o6")
    cheb = c["coefs"]
    assert cheb[0] == -1.0 and cheb[-1] == 1.0
    nspans, k = 300, 6
    row = [cheb[0]]
    for s_ in range(nspans):
        row += list(cheb[1:]) if s_ % 2 == 0 else list(cheb[::-1][1:])
    breaks = np.arange(nspans + 1) / nspans
    t = np.concatenate(([0.0], np.repeat(breaks, k - 1), [1.0]))
    s = bspy_amd.Spline(1, 1, [k], [len(row)], [t], [row])
    values, offsets = same_as_host(s, want_isolate=True)
    assert len(values) == (k - 1) * nspans
    x = np.sort(0.5 * (1.0 + np.cos((2 * np.arange(1, 6) - 1) * np.pi / 10)))      # the roots of T5(2 x - 1)
    want = (breaks[:-1, None] + x[None, :] / nspans).ravel()
    # delta of test_roots_host.py in the span's own parameter, scaled by the span's width: |d T5(2 x - 1) / dx| >= 10 at
    # the roots; plus 4 eps for the mapping and 4 eps for `want` itself (cos, the sum)
    bar = 8 * k * EPS * float(np.abs(cheb).max()) / 10.0 / nspans + 8 * EPS
    assert np.abs(values - want).max() <= bar
    listed = s.zeros(_path="device")
    assert np.array(listed).tobytes() == values.tobytes()


# ------------------------------------------------------------------------------------------ one realistic call
def test_closest_points_of_a_planar_curve():
    """Closest-point candidates of a cubic planar curve c for 257 query points p: the roots of c . c' - p . c', one component
    per query, built from differentiate, @, transform and subtract alone; one launch sequence for all queries.  For every
    query the best candidate (or a domain end) is at least as close as the best of 20 001 uniformly sampled parameters."""
    import oracle
    rng = np.random.default_rng(21)
    k, n, m = 4, 40, 257
    t = np.concatenate((k * [0.0], np.sort(rng.random(n - k)), k * [1.0]))
    angle = np.linspace(0.0, 1.5 * np.pi, n)
    ctrl = np.stack([np.cos(angle), np.sin(angle)]) * (1.0 + 0.3 * rng.standard_normal((1, n)))
    c = bspy_amd.Spline(1, 2, [k], [n], [t], ctrl)
    queries = 1.5 * rng.standard_normal((m, 2))
    dc = c.differentiate()
    g = (c @ dc).transform(np.ones((m, 1))) - dc.transform(queries)          # component q: c . c' - p_q . c'
    assert g.nDep == m and g.order == (6,)
    values, offsets, intervals = roots.zeros_batch(g, coefs=on_device(g))
    assert "roots_flag" in roots.LAST_PATHS and "roots_isolate" in roots.LAST_PATHS and len(intervals) == 0
    values, offsets = values.cpu().numpy(), offsets.cpu().numpy()

    def points(u):
        out, bad = oracle.c_evaluate(c.order, c.nCoef, c.knots, c.coefs, [0], [np.ascontiguousarray(u, np.float64)])
        assert bad == -1
        return out                                                    # (2, len(u))

    samples = points(np.linspace(0.0, 1.0, 20001))
    sampled = np.sqrt(((samples[:, None, :] - queries.T[:, :, None]) ** 2).sum(axis=0)).min(axis=1)       # (m,)
    at_roots = points(values)
    ends = points(np.array([0.0, 1.0]))
    # both distances are evaluated in fp64 from coefficients of size <= S: each carries a rounding of a few K eps S
    slack = 16 * k * EPS * float(np.abs(ctrl).max() + np.abs(queries).max())
    for q in range(m):
        own = at_roots[:, offsets[q]:offsets[q + 1]]
        cand = np.concatenate((own, ends), axis=1)
        best = np.sqrt(((cand - queries[q][:, None]) ** 2).sum(axis=0)).min()
        assert best <= sampled[q] + slack, f"query {q}: candidates {best}, samples {sampled[q]}"
