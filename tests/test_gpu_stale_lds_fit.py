"""
The fit kernels must not depend on what an earlier dispatch left in LDS (pattern of tests/test_gpu_stale_lds.py):
fit_sweep (staged rotations), fit_transpose (tile) and fit_residual (reduction tree) give the same bits as they come,
after bsk_debug_fill_lds has written 0xFFFFFFFF (NaN in fp32 and fp64) over the whole LDS of every CU, and after
0x7F7F7F7F (finite and huge).

This file sorts behind tests/test_gpu_stale_lds.py on purpose: like that one it leaves every CU's LDS filled with a
pattern while it runs, and no test of another module may run on LDS poisoned by this one.  The last thing the test
does, pass or fail, is to fill LDS with zeros.
"""
import ctypes

import numpy as np
import pytest

from bspy_amd import DeviceSpline
from bspy_amd import _native as nv
from test_gpu_fit import _system

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS, HUGE_BITS = 0xFFFFFFFF, 0x7F7F7F7F


def _fill(t, pattern, stream):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, stream))


def test_fit_kernels_ignore_stale_lds():
    t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        miss = ctypes.c_int64(-1)
        _fill(t, 0x5A5A5A5A, stream)
        nv.check(nv.lib().bsk_debug_fill_lds(t._handle, 0x5A5A5A5A, 1, ctypes.byref(miss), stream))
        if miss.value != 0:
            pytest.skip("LDS does not survive between dispatches on this device: the fills would prove nothing")
        rng = np.random.default_rng(8)
        for order in (4, 7):
            plan, first, values = _system(order, 91, 23, 7)
            for outer, inner in ((1000, 1), (3, 37), (1, 1)):
                tb = torch.as_tensor(rng.standard_normal((outer, 91, inner)), device="cuda")

                def call():
                    x = plan.sweep(tb, outer, inner)
                    assert plan.last_kernel() == ("fit_sweep turned" if inner == 1 and outer > 1 else "fit_sweep")
                    return x.cpu().numpy().tobytes() + plan.residual_rows(tb, x, outer, inner).tobytes()

                ref = call()
                want = plan.solve_host(tb.cpu().numpy(), outer, inner)
                got = np.frombuffer(ref, np.float64)[:want.size].reshape(want.shape)
                assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
                for pattern in (NAN_BITS, HUGE_BITS):
                    _fill(t, pattern, stream)
                    assert call() == ref, (f"result changed after filling LDS with {pattern:#010x} "
                                           f"(order {order}, outer {outer}, inner {inner})")
    finally:
        _fill(t, 0, stream)
