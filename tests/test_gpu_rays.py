"""
Spline.intersect_rays and rays.cast_batch on the GPU (ray_boxes, ray_count, ray_emit, ray_isolate, ray_reduce, the band
kernels for the extraction): every golden of tests/golden/rays.npz through ``_path="device"`` (bars of
tests/test_rays_host.py) with the kernels that ran asserted from ``rays.LAST_PATHS`` and ``bsk_rays_last_kernel``, bit-equal
to the host path and on a second run; then the layouts of the kernels against the host drivers, which run the same
functions of bsk_rays.hpp: bit for bit.  No kernel of the family declares LDS; the compiler keeps a small private array of the
walk there in ray_isolate, as in roots2_isolate, and tests/test_gpu_stale_lds_rays.py is the stale-LDS test that goes with it.
"""
import warnings

import numpy as np
import pytest

import bspy_amd
from bspy_amd import _native as nv
from bspy_amd import rays, roots2
from test_rays_host import (NAMES, across_rays, arch_surface, check_golden, compare_with_parent, down_rays, graph_surface, load_case,
                            make_spline, parent_pipeline_case, run_both, same)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BANDS = {"band_apply", "band_apply_line"}
INF = float("inf")


def launches(ran):
    return [p for p in ran if p not in BANDS]


def expected(host_ran):
    """The launches of the device path from those of the host path on the same numbers."""
    return [p[len("host "):] for p in host_ran if p.startswith("host ray_")]


def numpy_of(result):
    return tuple(a.cpu().numpy() if torch.is_tensor(a) else a for a in result)


@pytest.mark.parametrize("name", NAMES)
def test_golden_device(name):
    c = load_case(name)
    s = make_spline(c)
    host = run_both(s, c, _path="host")
    host_ran = list(rays.LAST_PATHS)
    every, first = run_both(s, c, _path="device")
    assert launches(rays.LAST_PATHS) == expected(host_ran) and launches(rays.LAST_PATHS)[0] == "ray_boxes"
    assert nv.lib().bsk_rays_last_kernel().decode() == launches(rays.LAST_PATHS)[-1]
    check_golden(c, every, first, "device")
    assert same(every, host[0]) and same(first, host[1])
    again = run_both(s, c, _path="device")
    assert same(every, again[0]) and same(first, again[1])


@pytest.mark.parametrize("order", [(2, 2), (3, 4), (4, 4), (4, 2)])
@pytest.mark.parametrize("ncells", [(1, 1), (3, 2), (9, 7)])
def test_layouts_against_the_host_drivers(order, ncells):
    """N in {1, 63, 65, 300} with a NaN ray in the middle of a wave; 1, 2 and 3 chunks of the cells; passes of 64 rays; both
    ``hits`` modes."""
    rng = np.random.default_rng(sum(order) * 100 + sum(ncells))
    s = graph_surface(order, ncells, seed=sum(order) + ncells[0])
    o, d = down_rays(rng, 300)
    o[1, 37] = np.nan
    ncell = ncells[0] * ncells[1]
    for N in (1, 63, 65, 300):
        for hits in ("first", "all"):
            host = rays.cast_batch(s, o[:, :N], d[:, :N], hits=hits, _path="host")
            dev = rays.cast_batch(s, o[:, :N], d[:, :N], hits=hits, _path="device")
            assert same(host, dev), (N, hits)
    host = rays.cast_batch(s, o, d, hits="all", _path="host")
    assert host[3][37] == 8 and host[2][-1] > 200
    for nchunks in (2, 3):
        chunk = -(-ncell // nchunks)
        assert same(host, rays.cast_batch(s, o, d, hits="all", _path="device", _chunk=chunk)), nchunks
    assert same(host, rays.cast_batch(s, o, d, hits="all", _path="device", _pass=64))
    assert rays.LAST_PATHS.count("ray_count") == 5
    assert same(host, rays.cast_batch(s, o, d, hits="all", _path="device", _prefilter=False))


def test_no_candidates_and_all_candidates():
    s = graph_surface((4, 4), (3, 2), seed=21)
    rng = np.random.default_rng(3)
    o, d = down_rays(rng, 130)
    away = o.copy()
    away[0] += 50.0                                        # every ray misses every box: the launches behind the count are skipped
    uv, t, cell, count, status = rays.cast_batch(s, away, d, _path="device")
    assert launches(rays.LAST_PATHS) == ["ray_boxes", "ray_count"]
    assert np.isnan(uv).all() and np.isnan(t).all() and (cell == -1).all() and not count.any() and not status.any()
    assert same((uv, t, cell, count, status), rays.cast_batch(s, away, d, _path="host"))
    assert rays.cast_batch(s, away, d, hits="all", _path="device")[2].tolist() == [0] * 131
    down = np.stack([rng.uniform(0.05, 0.95, 130), rng.uniform(0.1, 1.9, 130), np.full(130, 3.0)])
    straight = np.zeros((3, 130))
    straight[2] = -2.0
    first = rays.cast_batch(s, down, straight, _path="device")
    assert launches(rays.LAST_PATHS) == ["ray_boxes", "ray_count", "ray_emit", "ray_isolate", "ray_reduce"]
    assert (first[3] == 1).all() and same(first, rays.cast_batch(s, down, straight, _path="host"))
    every = rays.cast_batch(s, down, straight, hits="all", _path="device")
    assert launches(rays.LAST_PATHS)[-2:] == ["ray_reduce", "ray_reduce all"] and every[2].tolist() == list(range(131))


def test_cuda_tensors():
    s = arch_surface(bezier=False)
    rng = np.random.default_rng(4)
    o, d = across_rays(rng, 200)
    host = rays.cast_batch(s, o, d, _path="host")
    dev = rays.cast_batch(s, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    assert all(torch.is_tensor(a) and a.is_cuda for a in dev) and launches(rays.LAST_PATHS)[-1] == "ray_reduce"
    assert same(host, numpy_of(dev))
    wide = torch.from_numpy(np.concatenate((o, d))).cuda()                             # rows 0:3 and 3:6 of one tensor, every 2nd ray
    view = rays.cast_batch(s, wide[:3, ::2], wide[3:, ::2], hits="all")
    assert not wide[:3, ::2].is_contiguous() and same(rays.cast_batch(s, o[:, ::2], d[:, ::2], hits="all", _path="host"), numpy_of(view))
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    dev32 = rays.cast_batch(s, torch.from_numpy(o32).cuda(), torch.from_numpy(d32).cuda())
    assert same(rays.cast_batch(s, o32, d32, _path="host"), numpy_of(dev32))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        uv, t = s.intersect_rays(torch.from_numpy(o.reshape(3, 10, 20)).cuda(), torch.from_numpy(d.reshape(3, 10, 20)).cuda())
    assert uv.shape == (2, 10, 20) and t.shape == (10, 20) and uv.is_cuda and same((host[0], host[1]), (uv.reshape(2, 200).cpu().numpy(), t.reshape(200).cpu().numpy()))
    with pytest.raises(ValueError, match="device path"):
        rays.cast_batch(s, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), _path="host")
    with pytest.raises(TypeError):
        rays.cast_batch(s, torch.from_numpy(o).cuda(), d)


@pytest.mark.parametrize("k,m", [(-40, 3), (20, -7), (40, 11)])
def test_scale_law_on_cuda_tensors(k, m):
    rng = np.random.default_rng(14)
    s = graph_surface((4, 4), (3, 2), seed=15)
    o, d = down_rays(rng, 200)
    big = bspy_amd.Spline(2, 3, list(s.order), list(s.nCoef), s.knots, np.asarray(s.coefs) * 2.0 ** k)
    for hits in ("first", "all"):
        a = numpy_of(rays.cast_batch(s, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), tmin=1.5, tmax=40.0, hits=hits))
        b = numpy_of(rays.cast_batch(big, torch.from_numpy(o * 2.0 ** k).cuda(), torch.from_numpy(d * 2.0 ** m).cuda(),
                                     tmin=1.5 * 2.0 ** (k - m), tmax=40.0 * 2.0 ** (k - m), hits=hits))
        assert same([a[0], a[1] * 2.0 ** (k - m)] + list(a[2:]), b) and np.isfinite(a[1]).sum() > 50


def test_against_zeros2_batch_on_the_device():
    s, o, d, system, g = parent_pipeline_case("bicubic")
    uv, t, mine, status = rays.cast_batch(s, o, d, tmin=-INF, hits="all", _path="device")
    values, offsets, cells, zstatus = roots2.zeros2_batch(system, coefs=torch.from_numpy(g).cuda(), _path="device")
    assert not status.any() and not zstatus.any() and mine[-1] == int(offsets[-1]) and mine[-1] >= 150
    compare_with_parent(s, o, d, values.cpu().numpy(), offsets.cpu().numpy(), uv, mine)


def test_device_entry_points_refuse_what_the_host_twins_refuse():
    L = nv.lib()
    rows = torch.zeros((3, 2, 2), dtype=torch.float64, device="cuda")
    first = torch.zeros(1, dtype=torch.int32, device="cuda")
    boxes = torch.zeros((1, 6), dtype=torch.float64, device="cuda")
    assert L.bsk_rays_boxes(5, 2, rows.data_ptr(), 2, 2, 1, 1, first.data_ptr(), first.data_ptr(), boxes.data_ptr(), None) == nv.BSK_ERR_UNSUPPORTED
    assert L.bsk_last_error().decode() == "bsk_rays_boxes: order above 4"
    assert L.bsk_rays_boxes(2, 2, rows.data_ptr(), 2, 2, 1, 1, first.data_ptr(), first.data_ptr(), None, None) == nv.BSK_ERR_INVALID
    assert L.bsk_rays_boxes(2, 2, rows.data_ptr(), 2, 2, 1, 1, first.data_ptr(), first.data_ptr(), boxes.data_ptr(), None) == nv.BSK_OK
    torch.cuda.synchronize()
    assert boxes.cpu().numpy().tolist() == [[0.0] * 6] and L.bsk_rays_last_kernel().decode() == "ray_boxes"
