"""
What the order sweep shares (tests/golden/make_golden_orders.py, tests/test_orders_host.py, tests/test_gpu_orders.py): the
order tuples each cell family turns into template constants, read from the family's own range constants, the kernels the
family's resource guard (bspy_amd/csrc/check_spills.py) names, and the fixtures tests/golden/orders_<family>.npz.
"""
import itertools
import os

import numpy as np

FAMILIES = ("zeros2", "zeros3", "contours", "project", "rays", "surfaces")
KERNELS = {"zeros2": {"roots2_flag", "roots2_isolate", "roots2_merge"}, "zeros3": {"roots3_flag", "roots3_isolate", "roots3_merge"},
           "contours": {"contour_flag", "contour_march"}, "project": {"project_seed", "project_newton"},
           "rays": {"ray_boxes", "ray_count", "ray_emit", "ray_isolate", "ray_reduce"},
           "surfaces": {"ssx_count", "ssx_emit", "ssx_isolate", "ssx_merge"}}
# the template of a search kernel is launched twice, under two names: the guard knows the template
SEARCH = {"ray_count": "ray_search", "ray_emit": "ray_search", "ssx_count": "ssx_search", "ssx_emit": "ssx_search"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dispatched(family):
    """The sorted order tuples the family's ``with_range<2, MAX_K>`` dispatch builds a kernel for, from the range constants of
    the family's Python module.  project: pairs are surfaces, singles are curves.  surfaces: (KR, K1, K2), the order of the
    running variable of a lattice line and the orders of the other surface."""
    from bspy_amd import contours, project, rays, roots2, roots3, surfaces
    span = lambda lo, hi, n: sorted(itertools.product(range(lo, hi + 1), repeat=n))
    if family == "zeros2":
        return span(roots2.DEVICE_MIN_K, roots2.DEVICE_MAX_K, 2)
    if family == "zeros3":
        return span(roots3.MIN_K, roots3.MAX_K, 3)
    if family == "contours":
        return span(contours.DEVICE_MIN_K, contours.DEVICE_MAX_K, 2)
    if family == "project":
        return span(2, project.SURFACE_MAX_K, 2) + span(2, project.CURVE_MAX_K, 1)
    if family == "rays":
        return span(rays.MIN_K, rays.MAX_K, 2)
    if family == "surfaces":
        return span(surfaces.MIN_K, surfaces.MAX_K, 3)
    if family == "scatter":
        from bspy_amd import scatter
        return span(2, scatter.DEVICE_MAX_K, 1) + span(2, scatter.DEVICE_MAX_K, 2)
    raise KeyError(family)


def scatter_triples():
    """The (K0, K1, nDep) scatter_gram is built for: K1 = 1 is a curve.  ("scatter" is not one of FAMILIES: its fixture
    orders_scatter.npz has the layout of scatter.npz and its tests are tests/test_scatter_orders_host.py and
    tests/test_gpu_scatter_orders.py.)"""
    from bspy_amd import scatter
    return [((tuple(order) + (1,))[:2]) + (d,) for order in dispatched("scatter") for d in range(1, scatter.DEVICE_MAX_NDEP + 1)]


def triples_of(oa, ob):
    """The (KR, K1, K2) of the four line families of the pair (a, b): family f < 2 walks a's lines with variable f fixed
    against b's cells, f >= 2 b's lines against a's; the running variable is the other one."""
    return [(oa[1], *ob), (oa[0], *ob), (ob[1], *oa), (ob[0], *oa)]


def case_id(order):
    return "k" + "".join(str(int(k)) for k in order)


def path_of(family):
    return os.path.join(GOLDEN, f"orders_{family}.npz")


class Golden:
    """orders_<family>.npz, indexed like the family's own fixture (the family's key layout is kept)."""

    def __init__(self, family):
        self.data = np.load(path_of(family))
        self.files = self.data.files

    def __getitem__(self, key):
        return self.data[key]


def guarded_kernels():
    """The kernel names of the six families in check_spills.py's list."""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "bspy_amd", "csrc", "check_spills.py")).read()
    prefixes = ("roots2_", "roots3_", "contour_", "project_", "ray_", "ssx_")
    import re
    listed = set(re.findall(r'"([a-z0-9_]+)"', text.split("any(k in name for k in (", 1)[1].split("))", 1)[0]))
    return {k for k in listed if k.startswith(prefixes)}
