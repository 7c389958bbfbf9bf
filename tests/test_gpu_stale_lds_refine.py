"""
The band kernels must not depend on what an earlier dispatch left in LDS (pattern of tests/test_gpu_stale_lds.py and
tests/test_gpu_stale_lds_fit.py): band_apply (staged weights and first columns) and band_apply_line (the staged piece of
the lines: many short lines per workgroup, tiles of long lines, a ragged last tile) give the same bits as they come,
after bsk_debug_fill_lds has written 0xFFFFFFFF (NaN in fp32 and fp64) over the whole LDS of every CU, and after
0x7F7F7F7F (finite and huge).

This file sorts behind tests/test_gpu_stale_lds_fit.py on purpose: like that one it leaves every CU's LDS filled with
a pattern while it runs, and no test of another module may run on LDS poisoned by this one.  The last thing the test
does, pass or fail, is to fill LDS with zeros.
"""
import ctypes

import numpy as np
import pytest

from bspy_amd import DeviceSpline, refinement
from bspy_amd import _native as nv
from test_gpu_refine import some_band

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS, HUGE_BITS = 0xFFFFFFFF, 0x7F7F7F7F


def _fill(t, pattern, stream):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, stream))


def test_band_kernels_ignore_stale_lds():
    t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        miss = ctypes.c_int64(-1)
        _fill(t, 0x5A5A5A5A, stream)
        nv.check(nv.lib().bsk_debug_fill_lds(t._handle, 0x5A5A5A5A, 1, ctypes.byref(miss), stream))
        if miss.value != 0:
            pytest.skip("LDS does not survive between dispatches on this device: the fills would prove nothing")
        rng = np.random.default_rng(8)
        for order, m, n_in, inserted in ((4, 0, 91, 23), (7, 1, 91, 7), (3, 0, 1000, 301)):
            band = some_band(rng, order, n_in, m, inserted)
            for dtype in (np.float64, np.float32):
                for outer, inner in ((1000, 1), (3, 37), (1, 1), (2, 1024)):
                    a = rng.standard_normal((outer, n_in, inner)).astype(dtype)
                    ta = torch.from_numpy(a).cuda()

                    def call():
                        x = refinement.apply(band, ta, 1)
                        assert band.last_kernel() == ("band_apply_line" if inner == 1 else "band_apply")
                        return x.cpu().numpy().tobytes()

                    ref = call()
                    want = band.apply_host(a, outer, inner)
                    got = np.frombuffer(ref, dtype).reshape(want.shape)
                    bar = 1e-12 if dtype == np.float64 else 2.0 ** -23
                    assert np.abs(got.astype(np.float64) - want).max() <= bar * np.abs(want).max()
                    for pattern in (NAN_BITS, HUGE_BITS):
                        _fill(t, pattern, stream)
                        assert call() == ref, (f"result changed after filling LDS with {pattern:#010x} "
                                               f"(order {order}, outer {outer}, inner {inner}, {np.dtype(dtype).name})")
            band.close()
    finally:
        _fill(t, 0, stream)
