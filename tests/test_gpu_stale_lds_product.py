"""
The product kernels must not depend on what an earlier dispatch left in LDS (pattern of tests/test_gpu_stale_lds.py,
tests/test_gpu_stale_lds_fit.py and tests/test_gpu_stale_lds_refine.py): band_product_line (the staged pieces of both
operands for every term of a block of planes: many short lines per workgroup, tiles of long lines, a ragged last tile)
and band_product_tile (the staged 2-D pieces, restaged per term) give the same bits as they come, after
bsk_debug_fill_lds has written 0xFFFFFFFF (NaN in fp32 and fp64) over the whole LDS of every CU, and after 0x7F7F7F7F
(finite and huge).

This file sorts between tests/test_gpu_stale_lds_fit.py and tests/test_gpu_stale_lds_refine.py on purpose: like those
it leaves every CU's LDS filled with a pattern while it runs, and no test of another module may run on LDS poisoned by
this one.  The last thing the test does, pass or fail, is to fill LDS with zeros.
"""
import ctypes

import numpy as np
import pytest

from bspy_amd import DeviceSpline, product
from bspy_amd import _native as nv
from test_gpu_product import KERNEL, some_map

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS, HUGE_BITS = 0xFFFFFFFF, 0x7F7F7F7F


def _fill(t, pattern, stream):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, stream))


def test_product_kernels_ignore_stale_lds():
    t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        miss = ctypes.c_int64(-1)
        _fill(t, 0x5A5A5A5A, stream)
        nv.check(nv.lib().bsk_debug_fill_lds(t._handle, 0x5A5A5A5A, 1, ctypes.byref(miss), stream))
        if miss.value != 0:
            pytest.skip("LDS does not survive between dispatches on this device: the fills would prove nothing")
        rng = np.random.default_rng(9)
        calls = [([(91, 60)], 4, 4, "S", 1, 1000), ([(91, 60)], 3, 5, "C", 3, 5), ([(1000, 700)], 4, 4, "D", 3, 1),
                 ([(7, 9)], 2, 6, "S", 1, 1), ([(40, 33), (37, 41)], 4, 4, "C", 3, 2), ([(9, 10), (11, 8)], 6, 6, "D", 2, 1),
                 ([(120, 120), (5, 6)], 3, 5, "S", 1, 3)]
        for shapes, k1, k2, ptype, nDep, U in calls:
            maps = some_map(shapes, k1, k2)
            terms = product.plane_table(product.dependent_terms(ptype, nDep, nDep), U, 1)
            for dtype in (np.float64, np.float32):
                a = rng.standard_normal((nDep * U, *maps.nIn1)).astype(dtype)
                b = rng.standard_normal((nDep, *maps.nIn2)).astype(dtype)
                ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()

                def call():
                    x = product.apply(maps, ta, tb, terms)
                    assert maps.last_kernel() == KERNEL[maps.M]
                    return x.cpu().numpy().tobytes()

                ref = call()
                want = maps.apply_host(a, b, terms)
                got = np.frombuffer(ref, dtype).reshape(want.shape)
                bar = 1e-12 if dtype == np.float64 else 2.0 ** -23
                assert np.abs(got.astype(np.float64) - want).max() <= bar * terms.shape[1] * np.abs(a).max() * np.abs(b).max()
                for pattern in (NAN_BITS, HUGE_BITS):
                    _fill(t, pattern, stream)
                    assert call() == ref, (f"result changed after filling LDS with {pattern:#010x} "
                                           f"(shapes {shapes}, orders {k1} x {k2}, {ptype}, {np.dtype(dtype).name})")
    finally:
        _fill(t, 0, stream)
