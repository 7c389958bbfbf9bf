"""
Every order tuple of the six cell families whose orders are template constants, on the host path (no GPU), against the
exact oracles: tests/golden/orders_<family>.npz (made by tests/golden/make_golden_orders.py) holds one small fp64 case per
tuple that ``with_range<2, MAX_K>`` dispatches for zeros2, zeros3, contours, project, rays and surfaces, in each family's own
key layout.  So every case goes through the family's batch entry point and then through the family's own check, with the
bars as they are derived there and nothing added:
    zeros2, zeros3   test_roots2_host.check_golden, test_roots3_host.check_golden (per system of the B = 2 batch)
    rays             test_rays_host.check_golden (hits="all" and "first")
    project          test_project_host.check_golden, and the step counts of the statement
    contours         test_keys_and_segments_equal_the_oracle and test_vertices_within_the_derived_bar of test_contours_host
    surfaces         test_counts_bars_segments_and_components_are_the_exact_ones of test_surfaces_host
Every case is checked, counts are exact, no status bit is set, and ``observe`` records the worst error / bar per family and
tuple.  ``run`` is also what tests/test_gpu_orders.py calls with path="device" and path="cuda".

Two checks need no oracle of their own.  Transposition: the case of every (K0, K1) with its two variables swapped must give
the same counts, and its answers are held to the oracle's values, swapped, by the same check.  Completeness: the tuples in
the fixtures are the tuples the families dispatch today, and every kernel the resource guard knows is launched by the sweep
or named by a GPU test.
"""
import contextlib
import glob
import os

import numpy as np
import pytest

import orders_util as ou
import surfaces_util
import test_contours_host as tch
import test_project_host as tph
import test_rays_host as trh
import test_roots2_host as t2h
import test_roots3_host as t3h
import test_surfaces_host as tsh
import zeros3_ref
from bspy_amd import _native as nv
from bspy_amd import contours, project, rays, roots2, roots3, surfaces
from conftest import observe

GOLD = {family: ou.Golden(family) for family in ou.FAMILIES}
BANDS = {"band_apply", "band_apply_line", "roots_extract"}


def names(family):
    return [str(n) for n in GOLD[family]["names"]]


def tuple_of(name):
    """The orders of a case id: "k234" -> (2, 3, 4); a surface pair "k23_k44" -> ((2, 3), (4, 4))."""
    parts = [tuple(int(ch) for ch in part[1:]) for part in name.split("_")]
    return parts[0] if len(parts) == 1 else tuple(parts)


CASES = [(family, name) for family in ou.FAMILIES for name in names(family)]
IDS = [f"{family}-{name}" for family, name in CASES]


class Table:
    """Entries indexed like an .npz file: a family's fixture with the transposed cases next to it."""

    def __init__(self, base, extra):
        self.entries = {**{key: base[key] for key in base.files}, **extra}
        self.files = list(self.entries)

    def __getitem__(self, key):
        return self.entries[key]


@contextlib.contextmanager
def golden_in(module, attribute, table):
    """A family's test module reads its goldens from a global: for the time of a check, that is ``table``."""
    own = getattr(module, attribute)
    setattr(module, attribute, table)
    try:
        yield
    finally:
        setattr(module, attribute, own)


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def on_path(a, path):
    """The array as the call takes it on ``path``: a CUDA tensor for "cuda", NumPy otherwise."""
    if path != "cuda":
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pin(path):
    return None if path == "cuda" else path


def launches(ran):
    """What ran without the extraction's band kernels, under the device's names."""
    stripped = [p[len("host "):] if p.startswith("host ") else p for p in ran]
    return [p for p in stripped if p not in BANDS]


def kernels(ran):
    """The kernels among the launches (a launch may say what it was for: "contour_march count")."""
    return {p.split()[0] for p in launches(ran)}


def on_the_right_side(ran, path):
    assert ran and all(p.startswith("host ") == (path == "host") for p in ran), (path, ran)


# --------------------------------------------------------------------------------------------- the six calls
def zeros_systems(family, name, table=None):
    t = t2h if family == "zeros2" else t3h
    with golden_in(t, "_GOLDEN", table or GOLD[family]):
        systems = [t.load_case(f"{name}.{b}") for b in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(systems[0]["knots"], systems[1]["knots"])), "B = 2 systems on shared knots"
    return t, systems


def run_zeros(family, name, path, check=True, systems=None):
    t, systems = zeros_systems(family, name) if systems is None else (t2h if family == "zeros2" else t3h, systems)
    mod, call, last = (roots2, roots2.zeros2_batch, "bsk_roots2_last_kernel") if family == "zeros2" else (roots3, roots3.zeros3_batch, "bsk_roots3_last_kernel")
    coefs = np.stack([c["coefs"] for c in systems])
    values, offsets, cells, status = call(t.make_spline(systems[0]), coefs=on_path(coefs, path), _path=pin(path))
    ran, last = list(mod.LAST_PATHS), getattr(nv.lib(), last)().decode()
    on_the_right_side(ran, path)
    assert path != "cuda" or (values.is_cuda and offsets.is_cuda and status.is_cuda)
    values, offsets, cells, status = (numpy_of(a) for a in (values, offsets, cells, status))
    assert not status.any() and len(cells) == 0 and offsets[0] == 0 and offsets[-1] == len(values), name
    worst = 0.0
    if check:
        for b, c in enumerate(systems):
            worst = max(worst, t.check_golden(c, list(values[offsets[b]:offsets[b + 1]]), f"orders {family} {tuple(c['order'])} {path}"))
    return dict(bits=[a.tobytes() for a in (values, offsets, cells, status)], ran=ran, last=last, values=values, offsets=offsets, worst=worst)


def run_rays(name, path, check=True, case=None):
    if case is None:
        with golden_in(trh, "_GOLDEN", GOLD["rays"]):
            case = trh.load_case(name)
    c = case
    s = trh.make_spline(c)
    o, d = on_path(c["origins"], path), on_path(c["directions"], path)
    every = rays.cast_batch(s, o, d, c["tmin"], c["tmax"], hits="all", _path=pin(path))
    ran = list(rays.LAST_PATHS)
    first = rays.cast_batch(s, o, d, c["tmin"], c["tmax"], _path=pin(path))
    ran += list(rays.LAST_PATHS)
    last = nv.lib().bsk_rays_last_kernel().decode()
    on_the_right_side(ran, path)
    assert path != "cuda" or all(a.is_cuda for a in every + first)
    every, first = tuple(numpy_of(a) for a in every), tuple(numpy_of(a) for a in first)
    assert not every[3].any(), (name, "a ray carries a status bit")
    if check:
        trh.check_golden(c, every, first, f"orders {tuple(c['order'])} {path}")
    return dict(bits=[a.tobytes() for a in every + first], ran=ran, last=last, every=every)


def run_project(name, path, check=True, table=None):
    with golden_in(tph, "DATA", table or GOLD["project"]):
        c = tph.load_case(name)
        spline = tph.make_spline(c)
        got = project.project_batch(spline, on_path(c["points"], path), samples=c["samples"], _path=pin(path))
        ran, last = list(project.LAST_PATHS), nv.lib().bsk_project_last_kernel().decode()
        on_the_right_side(ran, path)
        assert path != "cuda" or all(a.is_cuda for a in got)
        got = tuple(numpy_of(a) for a in got)
        if check:
            tph.check_golden(name, got[0], got[1], got[2], f"orders {tuple(c['order'])} {path}")
    return dict(bits=[a.tobytes() for a in got], ran=ran, last=last, got=got, case=c)


def run_contours(name, path, check=True, table=None):
    with golden_in(tch, "GOLD", table or GOLD["contours"]):
        if check:                                               # the host drivers and the public host call against the oracle
            tch.test_keys_and_segments_equal_the_oracle(name)
            tch.test_vertices_within_the_derived_bar(name)
        s = tch.spline_of(name)
        depth = int(tch.GOLD[f"{name}/depth"])
    if path == "cuda":
        out = contours.trace_batch(s, coefs=on_path(np.asarray(s.coefs), path), depth=depth)
    else:
        out = contours.trace_batch(s, depth=depth, _path=path)
    ran, last = list(contours.LAST_PATHS), nv.lib().bsk_contour_last_kernel().decode()
    on_the_right_side(ran, path)
    out = tuple(numpy_of(a) for a in out)
    assert not out[5].any() and len(out[4]) == 0, (name, "a status bit or a zero cell")
    return dict(bits=[a.tobytes() for a in out], ran=ran, last=last, out=out)


def surface_bits(res):
    return [np.asarray(a).tobytes() for a in (res[0], res[1], res[2], res[3].segments, res[3].leaves)] + \
           [np.asarray(res[4]["families"][f][k]).tobytes() for f in range(4) for k in surfaces_util.PER_PAIR]


def run_surfaces(name, path, check=True):
    with golden_in(surfaces_util, "GOLD", GOLD["surfaces"]):
        c = surfaces_util.load_case(name)
        a, b = surfaces_util.make(c)
        res = surfaces.trace_pair(a, b, depth=c["depth"], _path=path)
        ran, last = list(surfaces.LAST_PATHS), nv.lib().bsk_ssx_last_kernel().decode()
        on_the_right_side(ran, path)
        assert res[3].bits == 0 and len(res[3].leaves) == 0, (name, "a status bit")
        walked = [int((np.asarray(f["count"]) > 0).sum()) for f in res[4]["families"]]
        assert min(walked) >= 1, (name, "a line family walked no pair that holds a vertex", walked)
        if check:
            tsh.test_counts_bars_segments_and_components_are_the_exact_ones(name)
            rows, _, _ = tsh.vertex_rows(name)
            triples = ou.triples_of(*tuple_of(name))
            assert {r["F"][0].shape for r in rows} == set(triples), (name, "a triple of the pair holds no vertex")
            for r in rows:                                      # the same figure per (KR, K1, K2): the check above records it per pair
                assert r["F"][0].shape == triples[r["fam"]]
                observe(f"orders surfaces {r['F'][0].shape} zero / bar", float(zeros3_ref.error_bound(r["F"], r["cert"], r["local"])) / r["bar"], 1.0)
    return dict(bits=surface_bits(res), ran=ran, last=last, res=res)


def run(family, name, path, check=True):
    """One recorded case through the family's batch entry point on ``path`` ("host", "device" or "cuda"): dict(bits, ran,
    last, ...).  check: held to the family's own check against the exact oracle."""
    if family in ("zeros2", "zeros3"):
        return run_zeros(family, name, path, check)
    return {"rays": run_rays, "project": run_project, "contours": run_contours, "surfaces": run_surfaces}[family](name, path, check)


def has_cuda_path(family):
    return family != "surfaces"                                # trace_pair takes two splines: there is no tensor to hand over


# --------------------------------------------------------------------------------------------- against the oracles
@pytest.mark.parametrize("family,name", CASES, ids=IDS)
def test_every_order_tuple_against_the_exact_oracle_host(family, name):
    got = run(family, name, "host")
    assert kernels(got["ran"]) <= ou.KERNELS[family] | ({"ray_boxes"} if family == "surfaces" else set()), got["ran"]
    assert got["last"] == [p for p in got["ran"] if p[len("host "):] not in BANDS and (family != "surfaces" or "ssx_" in p)][-1]
    if family == "project":
        assert got["got"][3].tolist() == got["case"]["steps"].tolist(), f"{name}: other step counts than the statement's"
    again = run(family, name, "host", check=False)
    assert again["bits"] == got["bits"], "two runs differ"


# --------------------------------------------------------------------------------------------- transposition
def by_rows(points):
    return points[np.lexsort(points.T[::-1])]


def transposed_zeros2(c):
    uv = c["exact_uv"][:, ::-1]
    perm = np.lexsort((uv[:, 1], uv[:, 0]))
    t = dict(c, name=c["name"] + "^T", order=c["order"][::-1], knots0=c["knots1"], knots1=c["knots0"], knots=c["knots"][::-1],
             coefs=np.ascontiguousarray(c["coefs"].transpose(0, 2, 1)), exact_uv=np.ascontiguousarray(uv[perm]),
             cert_cell=c["cert_cell"][perm][:, ::-1], cert_xy=c["cert_xy"][perm][:, ::-1], cert_radius=c["cert_radius"][perm],
             cert_Y=c["cert_Y"][perm][:, ::-1, :])              # Y's rows are the variables
    return t


def transposed_rays(c):
    nc0, nc1 = (len(np.unique(k)) - 1 for k in c["knots"])
    i, j = np.divmod(c["hit_cell"], nc1)
    return dict(c, name=c["name"] + "^T", order=c["order"][::-1], knots0=c["knots1"], knots1=c["knots0"], knots=c["knots"][::-1],
                coefs=np.ascontiguousarray(c["coefs"].transpose(0, 2, 1)), hit_u=c["hit_v"], hit_v=c["hit_u"], hit_x=c["hit_y"], hit_y=c["hit_x"],
                hit_cell=j * nc0 + i, hit_Y=c["hit_Y"][:, ::-1, :])


def transposed_project(name):
    g, t = GOLD["project"], name + "T"
    extra = {f"{t}.{key}": g[f"{name}.{key}"] for key in ("samples", "points", "dist_lo", "dist_hi", "gap", "hinv", "jmax", "hmin", "steps")}
    extra.update({f"{t}.order": g[f"{name}.order"][::-1], f"{t}.knots0": g[f"{name}.knots1"], f"{t}.knots1": g[f"{name}.knots0"],
                  f"{t}.coefs": np.ascontiguousarray(g[f"{name}.coefs"].transpose(0, 2, 1))})
    extra.update({f"{t}.{key}": np.ascontiguousarray(g[f"{name}.{key}"][::-1]) for key in ("u", "radius", "free")})
    return t, Table(g, extra)


def transposed_key(keys, NI, NJ):
    """The lattice-edge keys ((I NJ + J) << 1) | dir of a field with the variables swapped: edge (J, I, 1 - dir)."""
    keys = np.asarray(keys, np.int64)
    node, direction = keys >> 1, keys & 1
    I, J = np.divmod(node, NJ)
    return ((J * NI + I) << 1) | (1 - direction)


def transposed_contours(name):
    g, t = GOLD["contours"], name + "T"
    G = 1 << int(g[f"{name}/depth"])
    NI, NJ = ((len(np.unique(g[f"{name}/knots{a}"])) - 1) * G + 1 for a in range(2))
    edge = g[f"{name}/vedge"]
    extra = {f"{t}/{key}": g[f"{name}/{key}"] for key in ("depth", "level", "kind", "vslope")}
    extra.update({f"{t}/order": g[f"{name}/order"][::-1], f"{t}/knots0": g[f"{name}/knots1"], f"{t}/knots1": g[f"{name}/knots0"],
                  f"{t}/coefs": np.ascontiguousarray(g[f"{name}/coefs"].T), f"{t}/vkeys": transposed_key(g[f"{name}/vkeys"], NI, NJ),
                  f"{t}/vedge": np.stack([edge[:, 1], edge[:, 0], 1 - edge[:, 2]], axis=1)})
    extra.update({f"{t}/{key}": np.ascontiguousarray(g[f"{name}/{key}"][:, ::-1]) for key in ("vmid_hi", "vmid_lo", "vwidth")})
    return t, Table(g, extra), (NI, NJ)


PAIRS = [(family, name) for family in ("zeros2", "contours", "rays", "project") for name in names(family) if len(tuple_of(name)) == 2]


@pytest.mark.parametrize("family,name", PAIRS, ids=[f"{f}-{n}" for f, n in PAIRS])
def test_swapping_the_two_variables_swaps_the_answer(family, name):
    """Transposed coefficients, swapped knots and orders: the (K1, K0) kernel on the same geometry.  The counts are those of
    the recorded case and every answer is within its own bar of the oracle's value, swapped; where the bytes are the same as
    the recorded case's, swapped, that is said (printed), not required."""
    if family == "zeros2":
        _, systems = zeros_systems(family, name)
        base = run_zeros(family, name, "host", check=False)
        got = run_zeros(family, name, "host", systems=[transposed_zeros2(c) for c in systems])
        assert got["offsets"].tolist() == base["offsets"].tolist()
        back = np.concatenate([by_rows(got["values"][a:b][:, ::-1]) for a, b in zip(got["offsets"][:-1], got["offsets"][1:])])
        same = back.tobytes() == base["values"].tobytes()
    elif family == "rays":
        with golden_in(trh, "_GOLDEN", GOLD["rays"]):
            c = trh.load_case(name)
        base = run_rays(name, "host", check=False)
        got = run_rays(name, "host", case=transposed_rays(c))
        assert got["every"][2].tolist() == base["every"][2].tolist()           # the offsets: hits per ray
        same = got["every"][0][::-1].tobytes() == base["every"][0].tobytes() and got["every"][1].tobytes() == base["every"][1].tobytes()
    elif family == "project":
        t, table = transposed_project(name)
        base = run_project(name, "host", check=False)
        got = run_project(t, "host", table=table)
        assert got["got"][2].tolist() == base["got"][2].tolist()               # status: the same points sit on a bound
        same = got["got"][0][::-1].tobytes() == base["got"][0].tobytes() and got["got"][1].tobytes() == base["got"][1].tobytes()
    else:
        t, table, (NI, NJ) = transposed_contours(name)
        base = run_contours(name, "host", check=False)
        with golden_in(tch, "GOLD", table):
            tch.test_vertices_within_the_derived_bar(t)                        # every vertex against the oracle's, swapped
            keys = tch.raw(t)[4]["keys"]
            got = run_contours(t, "host", check=False, table=table)
        want = {frozenset(int(k) for k in transposed_key(seg, NI, NJ)) for seg in GOLD["contours"][f"{name}/segments"]}
        assert {frozenset(int(k) for k in seg) for seg in keys} == want and len(keys) == len(want), (name, "segments")
        assert sorted(np.diff(got["out"][1]).tolist()) == sorted(np.diff(base["out"][1]).tolist())      # the components' lengths
        assert sorted(got["out"][2].tolist()) == sorted(base["out"][2].tolist())                        # and how many are closed
        same = by_rows(got["out"][0][:, ::-1]).tobytes() == by_rows(base["out"][0]).tobytes()
    print(f"orders {family} {name}: the transposed case gives {'the same bytes, swapped' if same else 'other bytes, within its bars'}")


# --------------------------------------------------------------------------------------------- completeness
def test_the_fixtures_hold_every_dispatched_tuple():
    for family in ou.FAMILIES:
        want = ou.dispatched(family)
        if family == "surfaces":
            pairs = [tuple_of(n) for n in names(family)]
            assert sorted(set().union(*(ou.triples_of(*p) for p in pairs))) == want and len(want) == len(set(want))
            assert 4 * len(pairs) < len(want) + 4 * 3, "no more pairs than the triples need"
            doubles = [n for n in names(family) if any(len(np.unique(GOLD[family][f"{n}/{s}_knots0"])) + 2 * (int(GOLD[family][f"{n}/{s}_order"][0]) - 1)
                                                    < len(GOLD[family][f"{n}/{s}_knots0"]) for s in "ab")]
        else:
            assert [tuple_of(n) for n in names(family)] == want, family
            key = {"project": "{}.knots0", "zeros2": "{}.0/knots0", "zeros3": "{}.0/knots0"}.get(family, "{}/knots0")
            doubles = [n for n in names(family) if len(np.unique(GOLD[family][key.format(n)])) + 2 * (tuple_of(n)[0] - 1) < len(GOLD[family][key.format(n)])]
        assert doubles, (family, "no case with a double interior knot")
        assert os.path.getsize(ou.path_of(family)) < 1 << 18


def test_the_range_constants_are_those_of_the_dispatch():
    """``dispatched`` reads the Python modules' range constants; the kernels are built for ``with_range<2, *_MAX_K>`` of the
    translation units' constants.  The two are the same numbers, so raising one of them alone fails here, and raising both
    fails ``test_the_fixtures_hold_every_dispatched_tuple`` until the generator has run."""
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bspy_amd", "csrc")
    text = "".join(open(p).read() for p in glob.glob(os.path.join(csrc, "bsk_*.h*")))
    built = {name: int(value) for name, value in re.findall(r"\b([A-Z0-9_]+_MAX_K) = (\d+)", text)}
    want = {"ROOTS2_DEVICE_MAX_K": roots2.DEVICE_MAX_K, "ROOTS3_MAX_K": roots3.MAX_K, "CONTOUR_MAX_K": contours.DEVICE_MAX_K,
            "PROJECT_CURVE_MAX_K": project.CURVE_MAX_K, "PROJECT_SURFACE_MAX_K": project.SURFACE_MAX_K, "RAYS_MAX_K": rays.MAX_K,
            "SSX_MAX_K": surfaces.MAX_K}
    assert {name: built.get(name) for name in want} == want
    assert roots2.DEVICE_MIN_K == roots3.MIN_K == contours.DEVICE_MIN_K == rays.MIN_K == surfaces.MIN_K == 2


def test_every_guarded_kernel_is_launched_by_the_sweep_or_named_by_a_gpu_test():
    """The resource guard's list (check_spills.py) is the list of kernels.  The GPU sweep asserts the host path's launches of
    every case under the device's names, so what the host path launches here is what the sweep launches there; a kernel the
    transversal cases never need (the merge kernels: no zero lies on a cell's edge) must be named by another GPU test."""
    guarded = ou.guarded_kernels()
    known = set().union(*ou.KERNELS.values())
    assert {ou.SEARCH.get(k, k) for k in known} == guarded, (guarded, known)
    swept = set()
    for family, name in CASES:
        swept |= kernels(run(family, name, "host", check=False)["ran"])
    assert swept >= known - {"roots2_merge", "roots3_merge", "ssx_merge"}, known - swept
    here = os.path.dirname(os.path.abspath(__file__))
    text = "".join(open(p).read() for p in glob.glob(os.path.join(here, "test_gpu_*.py")))
    assert all(k in text for k in known - swept), known - swept
