"""
The ray kernels must not depend on what an earlier dispatch left in LDS (pattern of tests/test_gpu_stale_lds.py and
tests/test_gpu_stale_lds_product.py).  No kernel of the family declares LDS, but the compiler places a small private array
of the walk in LDS in ray_isolate (2048 bytes per block in the resource log, as in roots2_isolate): ``cast_batch`` gives the
same bytes as it comes, after bsk_debug_fill_lds has written 0xFFFFFFFF (NaN in fp64) over the whole LDS of every CU, and
after 0x7F7F7F7F (finite and huge).

Like the other files of its name it leaves every CU's LDS filled with a pattern while it runs; the last thing the test does,
pass or fail, is to fill LDS with zeros.
"""
import ctypes

import numpy as np
import pytest

from bspy_amd import DeviceSpline, rays
from bspy_amd import _native as nv
from test_rays_host import across_rays, arch_surface, down_rays, graph_surface, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_BITS, HUGE_BITS = 0xFFFFFFFF, 0x7F7F7F7F


def _fill(t, pattern, stream):
    nv.check(nv.lib().bsk_debug_fill_lds(t._handle, pattern, 0, None, stream))


def test_ray_kernels_ignore_stale_lds():
    t = DeviceSpline((2,), (3,), [np.array((0.0, 0.0, 0.5, 1.0, 1.0))], np.zeros((1, 3)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        miss = ctypes.c_int64(-1)
        _fill(t, 0x5A5A5A5A, stream)
        nv.check(nv.lib().bsk_debug_fill_lds(t._handle, 0x5A5A5A5A, 1, ctypes.byref(miss), stream))
        if miss.value != 0:
            pytest.skip("LDS does not survive between dispatches on this device: the fills would prove nothing")
        rng = np.random.default_rng(6)
        for s, (o, d) in ((arch_surface(bezier=False), across_rays(rng, 300)), (graph_surface((4, 4), (9, 7), seed=5), down_rays(rng, 300)),
                          (graph_surface((2, 2), (3, 2), seed=6), down_rays(rng, 65))):
            for hits in ("first", "all"):
                ref = rays.cast_batch(s, o, d, hits=hits, _path="device")
                assert "ray_isolate" in rays.LAST_PATHS and same(ref, rays.cast_batch(s, o, d, hits=hits, _path="host"))
                for pattern in (NAN_BITS, HUGE_BITS):
                    _fill(t, pattern, stream)
                    assert same(ref, rays.cast_batch(s, o, d, hits=hits, _path="device")), f"result changed after filling LDS with {pattern:#010x}"
    finally:
        _fill(t, 0, stream)
