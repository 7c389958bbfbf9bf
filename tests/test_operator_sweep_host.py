"""
The CPU half of the operator sweep (tests/operator_sweep.py holds the cases): no GPU.

    lists          the three parametrisations are the built instantiation sets, derived from the modules' device ranges:
                   band apply 42, band absmax 42, product 100; the geometry constants restated in operator_sweep.py are the
                   ones in the kernels' sources; the cases land on the edges they are made for (staged / in place, NL, NP,
                   a second tile of one row, more units than ABSMAX_PARTS)
    preconditions  of the exact cases: the sum of the absolute values of the elementary products, times the weights'
                   denominator, is an integer below 2^24 for float32 (2^53 for float64), so every partial sum in any order is
                   exact and every output is a value of the data's type
    host drivers   ``apply_host``, ``apply_fma_host``, ``absmax_host`` and ``ProductMap.apply_host`` equal the exact values
                   byte for byte on every edge case of every instantiation: a host-side staging bug shows without a GPU
    fused twin     ``apply_fma_host`` on real data lies within K 2^-53 sum_t |w x| of the exact rational row (one rounding
                   per fma; float32: plus 2^-24 |exact| for the rounding to the data's type)
    product bar    ``ProductMap.apply_host`` on real data lies within the counted bar of (d), see ``PRODUCT_BAR``: the bar
                   is reachable by the reference alone

The device twin is tests/test_gpu_operator_sweep.py; it imports ``PRODUCT_BAR`` and the helpers from here.
"""
import os
import re

import numpy as np
import pytest

import operator_sweep as ops
from bspy_amd import product, reduction, refinement
from conftest import ROOT, observe

PRODUCT_BAR = """
The counted bar of the product kernels, per output element:

    |got - exact| <= n 2^-52 sum |W1| |W2| |A| |B|      (float32: + 2^-24 |exact|)

n is counted from the sum order stated in bsk_product.hpp for UNFUSED evaluation (every product and every sum rounds), so it
holds whether or not the compiler contracts.  Widening the data to fp64 is exact, a term's sign is a factor of +-1, and the
first sum onto an accumulator that holds 0.0 is exact.

    line   an elementary product W[a][b] A[a] B[b] passes through: the product A[a] W[a][b] (1), the k1 - 1 further sums into
           V[b], the product V[b] B[b] (1), the k2 - 1 further sums over b, the T - 1 further sums over the terms:
           k1 + k2 + T - 1 roundings of 2^-53 each.  The bar takes n = k1 + k2 + T + 1 units of 2^-52: more than twice the
           count, which covers the second-order terms of (1 + 2^-53)^n - 1 and the factor 1 + 2^-24 on the error for float32.
    tile   the last variable as above gives k1v + k2v roundings up to s = sum_b2 V[b2] B[b1][b2]; then the product
           W1[a1][b1] s (1), the k1u k2u - 1 further sums over (a1, b1), the T - 1 further sums over the terms:
           k1v + k2v + k1u k2u + T - 1 roundings.  The bar takes n = k1v + k2v + k1u k2u + T + 2 units of 2^-52.

The host driver (``ProductMap::contract``) forms the same sums in the same order and is held to the same bar here.
"""

BAND_IDS = [ops.band_id(i) for i in ops.BAND_INSTANCES]
PRODUCT_IDS = [ops.product_id(i) for i in ops.PRODUCT_INSTANCES]


def band_of(case, w=None):
    return refinement.BandMap(case.first, ops.band_weights(case) if w is None else w, case.nIn)


def absmax_runs(case):
    """(groups, with minus) of a case: groups 1 and outer, without and with a subtrahend.  A case whose scalar lanes come
    from a misaligned subtrahend alone has no run without one; the shape with many units runs once."""
    if case.only_absmax:
        return [(1, True)]
    runs = [(1, False), (case.outer, True), (1, True), (case.outer, False)]
    if case.how == "minus_offset":
        runs = [r for r in runs if r[1]]
    return list(dict.fromkeys(runs))


# ------------------------------------------------------------------------------------------ lists and geometry
def built_band():
    ks = range(refinement.DEVICE_MIN_K, refinement.DEVICE_MAX_K + 1)
    return [(np.dtype(dt).name, K, lanes) for dt in (np.float32, np.float64) for K in ks for lanes in ("wide", "scalar", "line")]


def test_band_apply_list_is_the_built_set():
    assert [(np.dtype(i.dtype).name, i.K, i.lanes) for i in ops.BAND_INSTANCES] == built_band()
    assert len(ops.BAND_INSTANCES) == len(set(BAND_IDS)) == 42 and "f64-K7-scalar" in BAND_IDS


def test_band_absmax_list_is_the_built_set():
    """band_absmax and band_absmax_line are instantiated over the set of band_apply and band_apply_line (bsk_refine_tu.hip)."""
    assert sorted((np.dtype(i.dtype).name, i.K, i.lanes) for i in ops.BAND_INSTANCES) == sorted(built_band())
    assert len(built_band()) == 42 and reduction.BandMap is refinement.BandMap


def test_product_list_is_the_built_set():
    ks = range(product.DEVICE_MIN_K, product.DEVICE_MAX_K + 1)
    built = [(np.dtype(dt).name, k1, k2, kernel) for dt in (np.float32, np.float64) for k1 in ks for k2 in ks for kernel in ("line", "tile")]
    assert [(np.dtype(i.dtype).name, i.k1, i.k2, i.kernel) for i in ops.PRODUCT_INSTANCES] == built
    assert len(built) == len(set(PRODUCT_IDS)) == 100 and "f32-k5x2-tile" in PRODUCT_IDS
    assert (product.DEVICE_MIN_K, product.DEVICE_MAX_K, product.DEVICE_MAX_M) == (2, 6, 2)


def test_restated_constants_are_the_sources():
    for name, constants in ops.HEADER_CONSTANTS.items():
        with open(os.path.join(ROOT, "bspy_amd", "csrc", name)) as f:
            text = f.read()
        for key, value in constants.items():
            found = re.findall(rf"constexpr (?:int|long long) (?:[A-Z0-9_]+ = \d+, )*{key} = (\d+)", text)
            assert found == [str(value)], (name, key, found)


@pytest.mark.parametrize("K", ops.BAND_KS)
def test_band_cases_land_on_their_edges(K):
    for V in (2, 4):
        for lanes in ("wide", "scalar"):
            cases = ops.band_cases(K, lanes, V)
            seen = {"LX": set(), "outer": set(), "tiles": set(), "kinds": set()}
            for c in cases:
                assert c.nIn == c.first[-1] + K and np.all(np.diff(c.first) >= 0) and c.inner > 1
                eligible = c.inner % V == 0
                assert eligible == (lanes == "wide" or c.how != "plain")
                LX, LY, tiles = ops.rows_geometry(c.inner, V if lanes == "wide" else 1)
                if c.only_absmax:
                    units = -(-c.outer // LY) * tiles
                    assert units > ops.ABSMAX_PARTS and units % 2 == 1
                    continue
                seen["LX"].add(LX), seen["tiles"].add(tiles), seen["kinds"].add(c.name.split("-")[2])
                seen["outer"].add((LX, c.outer - LY))
                steps = np.diff(c.first)
                if "-jumps-" in c.name and len(c.first) > 2:
                    assert K in steps[:ops.BAND_ROWS - 1] and K + 3 in steps[:ops.BAND_ROWS - 1]
                if "-boundary-" in c.name:
                    assert steps[ops.BAND_ROWS - 1] == K + 3
            assert {c.name.split("-")[1] for c in cases if not c.only_absmax} == {"n1", "n31", "n32", "n33", "n65"}
            assert seen["kinds"] == set(ops.ROWS_PATTERNS) and seen["tiles"] == {1, 2}
            assert seen["LX"] >= ({1, 4, 256} if lanes == "wide" else {4, 256})
            for LX in seen["LX"]:
                LY = ops.BAND_BLOCK // LX
                assert {d for lx, d in seen["outer"] if lx == LX} == {1 - LY, -1, 1} - {-LY}
    line = ops.band_cases(K, "line", 2)
    assert {c.name.split("-")[1] for c in line[:-3]} == {"n1", "n3", "n64", "n255", "n256", "n257"}
    for c in line[:-3]:
        R, G, staged, NL0, NL = ops.line_geometry(c.first, K, c.outer)
        assert staged and c.outer - NL0 in (-1, 0, 1) or c.outer == 1
    assert {(len(c.first), c.outer - ops.line_geometry(c.first, K, c.outer)[3]) for c in line[:-3] if c.outer > 1 or len(c.first) > 3} >= {
        (n, d) for n in (64, 255, 256, 257) for d in (-1, 0, 1)}
    assert ops.line_geometry(line[0].first, K, 1)[:2] == (1, 256) and ops.BAND_BLOCK % 3 == 1
    exact, plus, many = line[-3:]
    assert ops.max_span(exact.first, K, 2) == ops.BAND_LINE_LDS and ops.line_geometry(exact.first, K, exact.outer)[2:] == (True, 1, 1)
    assert ops.max_span(plus.first, K, 2) == ops.BAND_LINE_LDS + 1
    assert ops.line_geometry(plus.first, K, plus.outer)[2:] == (False, 128, 128) and plus.outer == 129
    assert many.only_absmax and ops.line_geometry(many.first, K, many.outer)[4] == 1 and many.outer == ops.ABSMAX_PARTS + 1


@pytest.mark.parametrize("k1,k2", [(a, b) for a in ops.PROD_KS for b in ops.PROD_KS])
def test_product_cases_land_on_their_edges(k1, k2):
    line = ops.product_cases(k1, k2, "line")
    assert {(len(c.variables[0][0]), c.terms.shape[1]) for c in line[:-4]} == {(1, 1), (3, 3), (64, 2), (255, 1), (256, 3), (257, 2)}
    for c in line[:-4]:
        f, g, W8, n1, n2 = c.variables[0]
        P, T = c.terms.shape[:2]
        R, G, staged, NP0, NP = ops.product_line_geometry(f, g, k1, k2, T, P)
        assert staged and P in (1, NP0, NP0 + 1) and W8.shape[1:] == (k1, k2)
        if len(f) > 3:
            sa, sb = ops.max_span(f, k1, R), ops.max_span(g, k2, R)
            assert max(sa, sb) >= 1.5 * min(sa, sb) and not np.array_equal(f, g)
        assert c.terms[:, :, 2].tolist() == [[1, -1] if T == 2 else [1] * T] * P
    want = {"line-lds-exact-a": (True, ops.PROD_LINE_LDS), "line-lds-exact-b": (True, ops.PROD_LINE_LDS),
            "line-lds-plus-one-a": (False, ops.PROD_LINE_LDS + 1), "line-lds-plus-one-b": (False, ops.PROD_LINE_LDS + 1)}
    for c in line[-4:]:
        f, g, _, _, _ = c.variables[0]
        T = c.terms.shape[1]
        assert (ops.product_line_geometry(f, g, k1, k2, T, 3)[2], T * max(ops.max_span(f, k1, 2), ops.max_span(g, k2, 2))) == want[c.name]
    tile = ops.product_cases(k1, k2, "tile")
    shapes = [(len(c.variables[0][0]), len(c.variables[1][0])) + c.variables[0][2].shape[1:] for c in tile[:-3]]
    assert shapes == [(1, 1, k2, k1), (15, 63, k2, k1), (16, 64, k2, k1), (17, 65, k2, k1), (17, 65, 2, 6)]
    assert [c.terms.shape[1] for c in tile] == [1, 3, 2, 1, 3, 2, 3, 1]
    assert all(ops.tile_staged(c.variables)[0] and c.variables[1][2].shape[1:] == (k1, k2) for c in tile[:-3])
    assert ops.tile_staged(tile[-3].variables) == (True, (ops.TILE_LDS, (k1 + 1) * (k2 + 1)))
    assert ops.tile_staged(tile[-2].variables)[0] is False and ops.tile_staged(tile[-2].variables)[1][0] == ops.TILE_LDS + 1
    assert ops.tile_staged(tile[-1].variables)[0] is False and ops.tile_staged(tile[-1].variables)[1][1] == ops.TILE_LDS + 1


# ------------------------------------------------------------------------------------------ (a) exact cases on the host
@pytest.mark.parametrize("inst", ops.BAND_INSTANCES, ids=BAND_IDS)
def test_band_host_drivers_equal_the_exact_values(inst):
    limit = 2 ** 24 if inst.dtype == np.float32 else 2 ** 53
    for case in ops.band_cases(inst.K, inst.lanes, ops.lane_width(inst.dtype)):
        x, minus = ops.band_int_data(case, inst.dtype)
        assert np.array_equal(x, np.rint(x)) and np.all(np.abs(case.w8) <= 8) and (np.any(case.w8 == 0) or case.w8.size < 24)
        assert ops.band_eval(case.first, np.abs(case.w8), np.abs(x.astype(np.int64))).max() < limit
        with band_of(case) as band:
            if not case.only_absmax:
                want = ops.band_exact(case, x)
                assert np.array_equal(want.astype(np.float64) * 8, ops.band_exact8(case, x))
                assert ops.bits(band.apply_host(x, case.outer, case.inner)) == ops.bits(want), case.name
                assert ops.bits(reduction.apply_fma_host(band, x, 1)) == ops.bits(want), case.name
            for groups, with_minus in absmax_runs(case):
                m = minus if with_minus else None
                got = reduction.absmax_host(band, x, 1, groups, m)
                assert ops.bits(got) == ops.bits(ops.absmax_exact(case, x, groups, m)), (case.name, groups, with_minus)


@pytest.mark.parametrize("inst", ops.PRODUCT_INSTANCES, ids=PRODUCT_IDS)
def test_product_host_driver_equals_the_exact_values(inst):
    limit = 2 ** 24 if inst.dtype == np.float32 else 2 ** 53
    for case in ops.product_cases(inst.k1, inst.k2, inst.kernel):
        a, b = ops.product_int_data(case, inst.dtype)
        exact, absolute = ops.product_exact_scaled(case, a, b)
        assert absolute.max() < limit and np.all(np.abs(exact) <= absolute), case.name
        assert all(np.any(v[2] == 0) or v[2].size < 24 for v in case.variables)
        want = ops.product_exact(case, a, b)
        assert np.array_equal(want.astype(np.float64) * ops.product_denominator(case), exact)
        with product.ProductMap(ops.product_weights(case)) as maps:
            assert maps.covered() and maps.M == (1 if inst.kernel == "line" else 2)
            assert ops.bits(maps.apply_host(a, b, case.terms)) == ops.bits(want), case.name


# ------------------------------------------------------------------------------------------ (b) the fused twin
@pytest.mark.parametrize("inst", ops.BAND_INSTANCES, ids=BAND_IDS)
def test_fused_twin_within_one_rounding_per_fma(inst):
    """At most 4 x 8 lines of every edge case (the host driver treats every line alike)."""
    for case in ops.band_cases(inst.K, inst.lanes, ops.lane_width(inst.dtype)):
        if case.only_absmax:
            continue
        w, x, _ = ops.band_real_case(case, inst.dtype)
        x = np.ascontiguousarray(x[:4, :, :8])
        with band_of(case, w) as band:
            got = reduction.apply_fma_host(band, x, 1)
        exact, S = ops.band_real_exact(case.first, w, x)
        bars = ops.counted_bars(inst.K, 2.0 ** -53, S, exact, inst.dtype)
        observe(f"operator sweep, fused host twin {ops.tag(inst.dtype)}, |error| / (K 2^-53 sum |w x|)", ops.worst_ratio(got, exact, bars), 1.0)


# ------------------------------------------------------------------------------------------ (d) the product's counted bar
def check_product_bar(inst, got, reference, who):
    """``got`` against the exact bilinear form at the counted bar (``PRODUCT_BAR``); reference = (exact, S, n)."""
    exact, S, n = reference
    bars = ops.counted_bars(n, 2.0 ** -52, S, exact, inst.dtype)
    kernel = "band_product_" + inst.kernel
    observe(f"operator sweep, {who} {kernel} {ops.tag(inst.dtype)}, |error| / counted bar", ops.worst_ratio(got, exact, bars), 1.0)


def product_real_reference(inst):
    variables, a, b, terms, n = ops.product_real_case(inst)
    exact, S = ops.product_real_exact(variables, a, b, terms)
    return variables, a, b, terms, (exact, S, n)


@pytest.mark.parametrize("inst", ops.PRODUCT_INSTANCES, ids=PRODUCT_IDS)
def test_product_host_driver_within_the_counted_bar(inst):
    variables, a, b, terms, reference = product_real_reference(inst)
    T = terms.shape[1]
    if inst.kernel == "line":
        assert len(variables[0][0]) == 257 and reference[2] == inst.k1 + inst.k2 + T + 1
    else:
        assert (len(variables[0][0]), len(variables[1][0])) == (17, 65)
        assert reference[2] == inst.k1 + inst.k2 + inst.k1 * inst.k2 + T + 2 and variables[0][2].shape[1:] == (inst.k2, inst.k1)
    assert T == 2 and terms[:, :, 2].tolist() == [[1, -1]] * len(terms)
    with product.ProductMap(variables) as maps:
        got = maps.apply_host(a, b, terms)
    check_product_bar(inst, got, reference, "host driver")
