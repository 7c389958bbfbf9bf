"""
Every order tuple of the six cell families whose orders are template constants, on the GPU: the cases of
tests/golden/orders_<family>.npz (one per tuple that ``with_range<2, MAX_K>`` dispatches; tests/test_orders_host.py holds
the host path on them to the exact oracles) through ``_path="device"`` and, where the family takes CUDA tensors, through
those.  The device result is byte-equal to the host path on the same case and byte-equal on a second run; the launches are
those of the host path under the device's names (``LAST_PATHS``) and ``bsk_<family>_last_kernel`` names the last one.  Most of
the arithmetic is shared host/device code, so equality alone would not notice a wrong stride: the oracle in the host test
does.  What equality adds is each tuple's own kernel: its launch shape, its wave primitives against ``HostWave``.
surfaces: ``info["families"]`` shows that each of the four line families walked a pair that holds a vertex, so the
(KR; K1, K2) kernels of the parametrized pair really ran.
"""
import pytest

import orders_util as ou
import test_orders_host as host

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RUNS = [(family, name, path) for family, name in host.CASES for path in ("device", "cuda") if path == "device" or host.has_cuda_path(family)]


def run_id(family, name, path):
    """A surface pair is named by the (KR, K1, K2) of its four line families as well."""
    triples = "-" + "+".join(ou.case_id(t) for t in ou.triples_of(*host.tuple_of(name))) if family == "surfaces" else ""
    return f"{family}-{name}{triples}-{path}"


@pytest.mark.parametrize("family,name,path", RUNS, ids=[run_id(*r) for r in RUNS])
def test_every_order_tuple_equals_the_host_path(family, name, path):
    on_host = host.run(family, name, "host", check=False)
    got = host.run(family, name, path, check=False)
    ran = host.launches(got["ran"])
    assert ran == host.launches(on_host["ran"]), (got["ran"], on_host["ran"])
    assert host.kernels(got["ran"]) <= ou.KERNELS[family] | {"ray_boxes"} and ran[0] == {"zeros2": "roots2_flag", "zeros3": "roots3_flag", "contours": "contour_flag",
                                                                        "project": "project_seed", "rays": "ray_boxes", "surfaces": "ray_boxes"}[family]
    assert got["last"] == [p for p in ran if family != "surfaces" or p.startswith("ssx_")][-1]
    assert got["bits"] == on_host["bits"], f"{family} {name}: the {path} path and the host path differ"
    assert host.run(family, name, path, check=False)["bits"] == got["bits"], f"{family} {name}: two runs on the {path} path differ"


def test_every_tuple_appears_once_per_family_and_path():
    for family in ou.FAMILIES:
        listed = [host.tuple_of(n) for f, n, p in RUNS if f == family and p == "device"]
        if family == "surfaces":
            listed = sorted(set().union(*(ou.triples_of(*pair) for pair in listed)))
        assert listed == ou.dispatched(family), family
