"""
The maxima kernels of remove_knots must not depend on what an earlier dispatch left in LDS (pattern of
tests/test_gpu_stale_lds_refine.py): band_absmax (staged weights and first columns, the per-wave words of the workgroup
reduction), band_absmax_line (the staged piece of the lines, the words that combine the line groups) and the second
launch band_absmax_fold give the same bits as they come, after bsk_debug_fill_lds has written 0xFFFFFFFF (NaN in fp32 and
fp64) over the whole LDS of every CU, and after 0x7F7F7F7F (finite and huge: it would win any maximum).

This file sorts behind tests/test_gpu_stale_lds_refine.py on purpose: like that one it leaves every CU's LDS filled with
a pattern while it runs, and no test of another module may run on LDS poisoned by this one.  The last thing the test
does, pass or fail, is to fill LDS with zeros.
"""
import ctypes

import numpy as np
import pytest

from bspy_amd import DeviceSpline, reduction
from bspy_amd import _native as nv
from bspy_amd.refinement import BandMap
from test_remove_host import some_map

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS, HUGE_BITS = 0xFFFFFFFF, 0x7F7F7F7F


def _fill(t, pattern, stream):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, stream))


def test_absmax_kernels_ignore_stale_lds():
    t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        miss = ctypes.c_int64(-1)
        _fill(t, 0x5A5A5A5A, stream)
        nv.check(nv.lib().bsk_debug_fill_lds(t._handle, 0x5A5A5A5A, 1, ctypes.byref(miss), stream))
        if miss.value != 0:
            pytest.skip("LDS does not survive between dispatches on this device: the fills would prove nothing")
        rng = np.random.default_rng(18)
        for K, n_in, n_out in ((5, 91, 114), (8, 40, 45), (4, 700, 1001)):
            first, w = some_map(rng, K, n_in, n_out)
            band = BandMap(first, w, n_in)
            for dtype in (np.float64, np.float32):
                # many short lines per workgroup and a ragged last tile, lanes along inner, one line, 16-byte lanes
                for outer, inner, groups in ((1000, 1, 4), (3, 37, 3), (1, 1, 1), (2, 1024, 2)):
                    a = rng.standard_normal((outer, n_in, inner)).astype(dtype)
                    minus = rng.standard_normal((outer, n_out, inner)).astype(dtype)
                    ta, tm = torch.from_numpy(a).cuda(), torch.from_numpy(minus).cuda()
                    for m, tmm in ((None, None), (minus, tm)):

                        def call():
                            x = reduction.absmax(band, ta, 1, groups, tmm)
                            assert band.last_kernel() == ("band_absmax_line" if inner == 1 else "band_absmax")
                            return x.cpu().numpy().tobytes()

                        ref = call()
                        want = reduction.absmax_host(band, a, 1, groups, m)
                        assert ref == want.tobytes()
                        for pattern in (NAN_BITS, HUGE_BITS):
                            _fill(t, pattern, stream)
                            assert call() == ref, (f"result changed after filling LDS with {pattern:#010x} "
                                                   f"(K {K}, outer {outer}, inner {inner}, {np.dtype(dtype).name})")
            band.close()
    finally:
        _fill(t, 0, stream)
