"""
The result pool of the NumPy call path (bspy_amd/result_pool.py) when a lease's finalizer runs inside ``empty()``: the
garbage collector may free a dead lease during one of ``empty()``'s own allocations, on the same thread, while the pool's
lock is held; ``_give_back`` then takes that lock again.  With a plain lock the thread waits for itself.
"""
import gc

import numpy as np

from bspy_amd.result_pool import MIN_BYTES, ResultPool


def test_give_back_may_run_while_empty_holds_the_lock():
    pool = ResultPool()
    with pool._lock:
        again = pool._lock.acquire(blocking=False)              # what _give_back needs on this thread; never waits
        assert again, "the pool's lock is not reentrant: a finalizer inside empty() would wait for its own thread"
        pool._lock.release()
        pool._give_back(np.empty(MIN_BYTES, np.uint8))
    assert len(pool._free) == 1


def test_a_lease_in_a_cycle_is_recycled_by_the_collector():
    pool = ResultPool()
    a = pool.empty((MIN_BYTES,), np.uint8)
    holder = [a]
    holder.append(holder)                                       # only the cycle collector frees it
    del a, holder
    gc.collect()
    assert len(pool._free) == 1
    b = pool.empty((MIN_BYTES,), np.uint8)
    assert pool.recycled == 1 and b.nbytes == MIN_BYTES
