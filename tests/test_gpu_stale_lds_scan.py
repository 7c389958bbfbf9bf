"""
scan_line must not depend on what an earlier dispatch left in LDS (pattern of tests/test_gpu_stale_lds_refine.py): the
staged products of its tile and the chunk totals (many short lines per workgroup, one long line cut into segments, ragged
last chunks and a ragged last block of lines, both launches of the two-launch path) give the same bits as they come,
after bsk_debug_fill_lds has written 0xFFFFFFFF (NaN in fp32 and fp64) over the whole LDS of every CU, and after
0x7F7F7F7F (finite and huge).  scan_apply and sum_bcast stage nothing in LDS; scan_apply runs here once as a control.

This file sorts behind tests/test_gpu_stale_lds_refine.py on purpose: like that one it leaves every CU's LDS filled with
a pattern while it runs, and no test of another module may run on LDS poisoned by this one.  The last thing the test
does, pass or fail, is to fill LDS with zeros.
"""
import ctypes

import numpy as np
import pytest

from bspy_amd import DeviceSpline, sums
from bspy_amd import _native as nv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS, HUGE_BITS = 0xFFFFFFFF, 0x7F7F7F7F


def _fill(t, pattern, stream):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, stream))


def test_scan_kernels_ignore_stale_lds():
    t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        miss = ctypes.c_int64(-1)
        _fill(t, 0x5A5A5A5A, stream)
        nv.check(nv.lib().bsk_debug_fill_lds(t._handle, 0x5A5A5A5A, 1, ctypes.byref(miss), stream))
        if miss.value != 0:
            pytest.skip("LDS does not survive between dispatches on this device: the fills would prove nothing")
        rng = np.random.default_rng(9)
        for n, outer, inner, segments in ((7, 1000, 1, 0), (33, 131, 1, 0), (300, 3, 1, 2), (4500, 1, 1, 0), (1000, 5, 1, 5),
                                          (95, 3, 37, 2)):
            scan = sums.ScanMap(rng.random(n) + 0.05)
            for dtype in (np.float64, np.float32):
                a = rng.standard_normal((outer, n, inner)).astype(dtype)
                ta = torch.from_numpy(a).cuda()

                def call():
                    x = sums.scan(scan, ta, 1, _segments=segments)
                    assert scan.last_kernel() == ("scan_line" if inner == 1 else "scan_apply")
                    return x.cpu().numpy().tobytes()

                ref = call()
                assert ref == scan.apply_host(a, outer, inner).tobytes()
                for pattern in (NAN_BITS, HUGE_BITS):
                    _fill(t, pattern, stream)
                    assert call() == ref, (f"result changed after filling LDS with {pattern:#010x} "
                                           f"(n {n}, outer {outer}, inner {inner}, segments {segments}, {np.dtype(dtype).name})")
            scan.close()
    finally:
        _fill(t, 0, stream)
