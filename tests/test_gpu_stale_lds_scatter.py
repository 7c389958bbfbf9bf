"""
The scatter kernels must not depend on what an earlier dispatch left in LDS (pattern of tests/test_gpu_stale_lds.py and
tests/test_gpu_stale_lds_rays.py).  scatter_gram declares ``__shared__ double tile[64 * ROW]``; a batch of cnt < 64 points
writes the rows of the lanes below cnt only, and the strands read the rows j < cnt: a wrong bound on either side reads what
the last dispatch left.  The cases k2, k33 and k44 of tests/golden/orders_scatter.npz (Q = 32, 4 and 4) hold batches of 1,
Q - 1 and 65 = 64 + 1 points: ``assemble(..., keep=True)`` on the device gives the host path's bytes as it comes, after
bsk_debug_fill_lds has written 0xFFFFFFFF (NaN in fp64) over the whole LDS of every CU, and after 0x7F7F7F7F (finite and
huge).

Like the other files of its name it leaves every CU's LDS filled with a pattern while it runs; the last thing the test does,
pass or fail, is to fill LDS with zeros.
"""
import ctypes

import numpy as np
import pytest

from bspy_amd import DeviceSpline
from bspy_amd import _native as nv
from test_gpu_scatter_orders import CASES, TABLES, device_tables, same_tables
from test_scatter_orders_host import bits, host

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS, HUGE_BITS = 0xFFFFFFFF, 0x7F7F7F7F


def _fill(t, pattern, stream):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, stream))


def test_scatter_kernels_ignore_stale_lds():
    t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        miss = ctypes.c_int64(-1)
        _fill(t, 0x5A5A5A5A, stream)
        nv.check(nv.lib().bsk_debug_fill_lds(t._handle, 0x5A5A5A5A, 1, ctypes.byref(miss), stream))
        if miss.value != 0:
            pytest.skip("LDS does not survive between dispatches on this device: the fills would prove nothing")
        for name in ("k2", "k33", "k44"):
            counts = CASES[name]["counts"].tolist()
            assert 1 in counts and 65 in counts and 2 * 256 + 5 in counts
            want = host(name, 4)[2]
            ref = device_tables(CASES[name], 4)
            same_tables(ref, want)
            for pattern in (NAN_BITS, HUGE_BITS):
                _fill(t, pattern, stream)
                have = device_tables(CASES[name], 4)
                for what in TABLES:
                    assert bits(have[what].reshape(-1)) == bits(np.asarray(want[what]).reshape(-1)), \
                        f"{name}: {what} changed after filling LDS with {pattern:#010x}"
    finally:
        _fill(t, 0, stream)
