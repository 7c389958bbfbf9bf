"""
The host path of every cell family and line-operator family on scratch memory that is not zero: ``Host.empty`` hands out
buffers of bytes 0xFF (NaN in every float, -1 in every integer) and 0x5A (a finite 4.6e127, an integer far past every
array), and every result has to keep the bytes of the run on plain ``np.empty``.  A host driver that reads what it did not
write cannot pass both.  The cases are those of tests/stream_families.py, which tests/test_gpu_side_stream.py runs on the
device against these same host results.  ("The stream contract as tested", lists the ``np.empty`` sites that do
not go through ``Host.empty``.)
"""
import numpy as np
import pytest

import stream_families as sf
from bspy_amd._backend import Host
from stream_util import poisoned

PATTERNS = (0xFF, 0x5A)


def test_poisoned_empty_is_poison_and_zeros_is_zero():
    be = Host()
    for pattern in PATTERNS:
        with poisoned(pattern):
            for dtype in (np.float64, np.float32, np.int32, np.uint8, np.int64):
                a = be.empty((3, 5), dtype)
                assert a.dtype == dtype and a.shape == (3, 5) and (a.view(np.uint8) == pattern).all()
                assert not be.zeros((3, 5), dtype).any()
            assert be.empty((0, 4), np.float64).shape == (0, 4)
        assert Host.empty(be, 4, np.uint8).shape == (4,), "the wrap is taken off again"
    with poisoned(0xFF):
        assert np.isnan(be.empty(7, np.float64)).all() and (be.empty(7, np.int32) == -1).all()


@pytest.mark.parametrize("name", sorted(set(sf.FAMILIES) - sf.HOST_NEEDS_GPU))
def test_host_path_reads_nothing_it_did_not_write(name):
    run, _ = sf.FAMILIES[name]
    want = sf.on_host(name)
    assert want.ran and all(p.startswith("host") for p in want.ran), (name, want.ran)
    for pattern in PATTERNS:
        with poisoned(pattern):
            got = run("host")
        assert got.ran == want.ran, (name, hex(pattern), got.ran)
        assert got.bits == want.bits, f"{name}: the host path on scratch memory of bytes {pattern:#x} returns other bytes"
