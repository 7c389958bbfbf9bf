"""
The device half of the operator sweep: every instantiation of band_apply<T, K, V> / band_apply_line<T, K> (42), of
band_absmax<T, K, V> / band_absmax_line<T, K> (42) and of band_product_line<T, K1, K2> / band_product_tile<T, K1V, K2V> (100),
one test each, on the edge shapes of tests/operator_sweep.py (the smallest that cross BAND_ROWS, LX / LY, R and G, NL, NP,
LINE_LDS, TILE_R1 x TILE_R2, TILE_LDS and ABSMAX_PARTS from both sides; the host half asserts that they do).

    (a) exact pin   multiples of 2^-3 on small integers: the device output equals BYTE FOR BYTE the int64 evaluation of the
                    operator and the host drivers ``apply_host``, ``apply_fma_host``, ``absmax_host``, ``ProductMap.apply_host``
    (b) fused chain standard-normal data, random real weights: ``refinement.apply`` equals ``reduction.apply_fma_host`` byte for
                    byte (DESIGN.md sections 16 and 18: the kernels' sums are the chain acc = fma(w[t], x[t], acc)); a second
                    run gives the same bytes
    (c) absmax      ``reduction.absmax`` equals ``reduction.absmax_host`` (``np.array_equal``) on the same real data, groups 1
                    and outer, without and with a subtrahend
    (d) product     one real-valued case per instantiation against the exact bilinear form at the counted bar
                    (``test_operator_sweep_host.PRODUCT_BAR``), observed / bar recorded per kernel and dtype

``last_kernel()`` does not name the lane width, so the launcher's rule is restated (``wide_lanes``) and asserted on the
pointers of every launch: scalar lanes come from an odd inner extent and from a 16-byte-misaligned view of a wide-eligible
shape (for absmax also from a misaligned subtrahend alone).
"""
import numpy as np
import pytest

import operator_sweep as ops
from bspy_amd import product, reduction, refinement
from test_operator_sweep_host import (BAND_IDS, PRODUCT_IDS, absmax_runs, band_of, check_product_bar, product_real_reference)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

APPLY = {"wide": "band_apply", "scalar": "band_apply", "line": "band_apply_line"}
ABSMAX = {"wide": "band_absmax", "scalar": "band_absmax", "line": "band_absmax_line"}


def on_device(a, misaligned=False):
    """The array as a contiguous CUDA tensor, on request one element off the allocation's 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misaligned:
        out = t.cuda()
        assert out.data_ptr() % 16 == 0
        return out
    flat = torch.empty(a.size + 1, dtype=t.dtype, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    out = flat[1:].view(a.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def wide_lanes(inner, V, *tensors):
    """The launchers' rule (``run`` and ``run_absmax`` of bsk_refine_tu.hip): 16-byte lanes when V divides inner and every
    pointer is 16-byte aligned (a result is a fresh allocation: aligned); inner == 1 is the line kernel."""
    return inner % V == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def check_lanes(inst, case, *tensors):
    if inst.lanes == "line":
        assert case.inner == 1
    else:
        assert case.inner > 1 and wide_lanes(case.inner, ops.lane_width(inst.dtype), *tensors) == (inst.lanes == "wide"), case.name


def device_apply(inst, case, band, x):
    t = on_device(x, case.how != "plain")
    check_lanes(inst, case, t)
    del refinement.LAST_PATHS[:]
    got = refinement.apply(band, t, 1)
    assert refinement.LAST_PATHS == [APPLY[inst.lanes]] and band.last_kernel() == APPLY[inst.lanes]
    assert got.is_cuda and tuple(got.shape) == (case.outer, len(case.first), case.inner)
    return t, got.cpu().numpy()


@pytest.mark.parametrize("inst", ops.BAND_INSTANCES, ids=BAND_IDS)
def test_band_apply_instantiation(inst):
    for case in ops.band_cases(inst.K, inst.lanes, ops.lane_width(inst.dtype)):
        if case.only_absmax:
            continue
        # (a) the exact pin
        x, _ = ops.band_int_data(case, inst.dtype)
        want = ops.bits(ops.band_exact(case, x))
        with band_of(case) as band:
            _, got = device_apply(inst, case, band, x)
            assert got.dtype == x.dtype and ops.bits(got) == want, case.name
            assert ops.bits(band.apply_host(x, case.outer, case.inner)) == want, case.name
            assert ops.bits(reduction.apply_fma_host(band, x, 1)) == want, case.name
        # (b) the fused chain
        w, x, _ = ops.band_real_case(case, inst.dtype)
        with band_of(case, w) as band:
            t, got = device_apply(inst, case, band, x)
            assert ops.bits(got) == ops.bits(reduction.apply_fma_host(band, x, 1)), case.name
            assert ops.bits(refinement.apply(band, t, 1).cpu().numpy()) == ops.bits(got), "two runs differ"


@pytest.mark.parametrize("inst", ops.BAND_INSTANCES, ids=BAND_IDS)
def test_band_absmax_instantiation(inst):
    for case in ops.band_cases(inst.K, inst.lanes, ops.lane_width(inst.dtype)):
        w_real, x_real, minus_real = ops.band_real_case(case, inst.dtype)
        x_int, minus_int = ops.band_int_data(case, inst.dtype)
        for exact, w, x, minus in ((True, None, x_int, minus_int), (False, w_real, x_real, minus_real)):
            t = on_device(x, case.how == "offset")
            tm = on_device(minus, case.how in ("offset", "minus_offset"))
            with band_of(case, w) as band:
                for groups, with_minus in absmax_runs(case):
                    m, sub = (minus, tm) if with_minus else (None, None)
                    check_lanes(inst, case, t, sub)
                    del reduction.LAST_PATHS[:]
                    got = reduction.absmax(band, t, 1, groups, sub)
                    assert reduction.LAST_PATHS == [ABSMAX[inst.lanes]] and band.last_kernel() == ABSMAX[inst.lanes]
                    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (groups, len(case.first))
                    got = got.cpu().numpy()
                    # (c) the host driver, exact and real data alike
                    assert np.array_equal(got, reduction.absmax_host(band, x, 1, groups, m)), (case.name, groups, with_minus, exact)
                    if exact:                                                              # (a) the exact pin
                        assert ops.bits(got) == ops.bits(ops.absmax_exact(case, x, groups, m)), (case.name, groups, with_minus)


def device_product(inst, maps, a, b, terms):
    kernel = "band_product_" + inst.kernel
    del product.LAST_PATHS[:]
    got = product.apply(maps, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), terms)
    assert product.LAST_PATHS == [kernel] and maps.last_kernel() == kernel
    assert got.is_cuda and tuple(got.shape) == (len(terms), *maps.nOut)
    got = got.cpu().numpy()
    assert got.dtype == a.dtype
    return got


@pytest.mark.parametrize("inst", ops.PRODUCT_INSTANCES, ids=PRODUCT_IDS)
def test_product_instantiation(inst):
    # (a) the exact pin on every edge
    for case in ops.product_cases(inst.k1, inst.k2, inst.kernel):
        a, b = ops.product_int_data(case, inst.dtype)
        want = ops.bits(ops.product_exact(case, a, b))
        with product.ProductMap(ops.product_weights(case)) as maps:
            assert (maps.k1[-1], maps.k2[-1]) == (inst.k1, inst.k2)
            assert ops.bits(device_product(inst, maps, a, b, case.terms)) == want, case.name
            assert ops.bits(maps.apply_host(a, b, case.terms)) == want, case.name
    # (d) the exact bilinear form at the counted bar
    variables, a, b, terms, reference = product_real_reference(inst)
    with product.ProductMap(variables) as maps:
        got = device_product(inst, maps, a, b, terms)
        assert ops.bits(device_product(inst, maps, a, b, terms)) == ops.bits(got), "two runs differ"
    check_product_bar(inst, got, reference, "device")
