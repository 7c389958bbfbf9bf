"""
Every instantiation of the ``bsk_scatter_*`` kernels on the device: scatter_gram<K0, K1, NDEP> is built 48 times (K0 2 .. 4,
K1 1 .. 4 with 1 a curve, NDEP 1 .. 4), each with its own LDS row stride (K + 1 + NDEP) | 1, strand count Q and idle lanes;
scatter_residual<K0, K1> 12 times.  The 12 cases of tests/golden/orders_scatter.npz, each with its first d = 1 .. 4 channels,
run all 48, and every case holds cells with 3, 0, 1, Q - 1, Q + 1, 63, 65, SEG, SEG + 1 and 2 SEG + 5 points: the strand
deal, the batch of 64 and the unit of SEG points from both sides.

Per (K0, K1, nDep): ``_path="device"`` (on the runs with d = 4 also CUDA tensors in) with the six kernel names asserted from
``info["paths"]`` and ``bsk_scatter_last_kernel``; key, status, counts, unit slabs, cell slabs, stencil and right-hand side
BYTE FOR BYTE those of the host path, then the coefficients and the residuals; a second run gives the same bytes.  The host
path itself is held to the exact oracle in tests/test_scatter_orders_host.py, whose cached host results are used here.
Per order tuple also its points on every knot and on the domain ends (``on_the_knots``), byte for byte the host path's.
"""
import numpy as np
import pytest

import orders_util as ou
from bspy_amd import _native as nv
from bspy_amd import scatter
from test_scatter_orders_host import CASES, TRIPLES, arrays, bits, host, name_of, on_the_knots, triple_id

pytestmark = pytest.mark.gpu

KERNELS = ["scatter_key", "scatter_gram", "scatter_cell", "scatter_fold", "host scatter_solve", "scatter_residual"]
TABLES = ("key", "status", "counts", "units", "cells", "stencil", "rhs")


def device_tables(case, d):
    import torch
    be = scatter.Device.current()
    put = [None if a is None else torch.from_numpy(a).to(be.dev) for a in arrays(case, d)]
    del scatter.LAST_PATHS[:]
    res = scatter.assemble(be, scatter.Shape(case["order"], case["knots"]), *put, keep=True)
    assert scatter.LAST_PATHS == KERNELS[:4]                                     # one scatter_cell level: at most 3 units per cell
    return {k: v.cpu().numpy() for k, v in res.items()}


def same_tables(have, want):
    for what in TABLES:
        assert have[what].shape == np.asarray(want[what]).shape, what
        assert bits(have[what].reshape(-1)) == bits(np.asarray(want[what]).reshape(-1)), what


def test_every_triple_appears_once():
    top, deps = scatter.DEVICE_MAX_K, scatter.DEVICE_MAX_NDEP
    built = [(k0, k1, d) for k0 in range(2, top + 1) for k1 in range(1, top + 1) for d in range(1, deps + 1)]
    assert sorted(TRIPLES) == built and len(built) == 48
    ids = [triple_id(t) for t in TRIPLES]
    assert len(set(ids)) == 48 and "k43-d2" in ids and "k3-d1" in ids
    assert {name_of(t) for t in TRIPLES} == {ou.case_id(o) for o in ou.dispatched("scatter")}


@pytest.mark.parametrize("triple", TRIPLES, ids=triple_id)
def test_instantiation_equals_the_host_path_byte_for_byte(triple):
    name, d = name_of(triple), triple[2]
    case = CASES[name]
    coefs, hinfo, want = host(name, d)
    uvw, pts, w = arrays(case, d)
    first = device_tables(case, d)
    same_tables(first, want)
    s, info = scatter.fit_batch(uvw, pts, case["order"], case["knots"], weights=w, _path="device")
    assert info["paths"] == KERNELS and scatter.LAST_PATHS == KERNELS           # a host assembly cannot pass as a GPU result
    assert nv.lib().bsk_scatter_last_kernel().decode() == "scatter_residual"
    assert bits(s.coefs.reshape(d, -1)) == bits(coefs)
    assert bits(info["residual"]) == bits(hinfo["residual"]) and bits(info["status"]) == bits(hinfo["status"])
    assert info["objective"] == hinfo["objective"] and info["empty"] == hinfo["empty"] == 1
    # twice: the same bytes
    again = device_tables(case, d)
    for what in TABLES:
        assert bits(again[what].reshape(-1)) == bits(first[what].reshape(-1)), what
    if d == scatter.DEVICE_MAX_NDEP:
        import torch
        t = [None if a is None else torch.from_numpy(a).cuda() for a in (uvw, pts, w)]
        s, info = scatter.fit_batch(t[0], t[1], case["order"], case["knots"], weights=t[2])
        assert info["paths"] == KERNELS and info["status"].is_cuda and info["residual"].is_cuda
        assert nv.lib().bsk_scatter_last_kernel().decode() == "scatter_residual"
        assert bits(s.coefs.reshape(d, -1)) == bits(coefs)
        assert bits(info["residual"].cpu().numpy()) == bits(hinfo["residual"]) and not info["status"].any()


@pytest.mark.parametrize("order", ou.dispatched("scatter"), ids=ou.case_id)
def test_points_on_the_knots_and_the_domain_ends(order):
    case, key = on_the_knots(order)
    have = device_tables(case, 4)
    assert have["key"].tolist() == key.tolist() and not have["status"].any()
    want = scatter.assemble(scatter.Host(), scatter.Shape(case["order"], case["knots"]), *arrays(case, 4), keep=True)
    same_tables(have, want)
