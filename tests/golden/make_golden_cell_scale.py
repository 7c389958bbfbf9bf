"""
Writes tests/golden/cell_scale.npz: part B of the cell families' scale tests (tests/test_scale_cells_host.py).  Systems of
the families' own goldens (roots2.npz, roots3.npz, project.npz, contours.npz, remove.npz: well conditioned by their
generators' rules) are moved to every domain of cases.SCALE_DOMAINS (float32 knots: cases.SCALE_DOMAINS_F32) by
scale_ref.map_axis, and what is exactly true of the STORED shifted values is computed anew by the project's rational
references: zeros2_ref, zeros3_ref and zeros_ref, project_ref, contours_ref, and refine_ref for the refined input of a
recovery (remove_ref judges the result in the test itself).  Nothing here needs the reference checkout: the entries that
record what the reference returned say that it was not asked (ref_complete False, ref_count -1), and the reference's
coefficient counts of the data reduction, which do not depend on the domain (knot removal commutes with an affine map of
the parameter), are taken over from remove.npz.

Every case is certified on every domain or the generator stops: none is left out.  Run on the CPU from the repository
root, three to four minutes:

    python tests/golden/make_golden_cell_scale.py

Keys: ``<family>:`` in front of the family's own key layout, the case called ``<its name>@<lo>+<width>``; per family
``<family>:names``.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
import scale_ref as sr  # noqa: E402
import refine_ref  # noqa: E402
import make_golden_roots2 as g2  # noqa: E402
import make_golden_roots3 as g3  # noqa: E402
import make_golden_project as gp  # noqa: E402
import make_golden_contours as gc  # noqa: E402
import test_roots2_host as t2  # noqa: E402
import test_roots3_host as t3  # noqa: E402
import test_project_host as tp  # noqa: E402
import test_contours_host as tc  # noqa: E402
from bspy_amd import project  # noqa: E402

# the systems moved, per family: on the float64 domains, on the float32 domains (their knots are float32)
BASES = {"zeros2": (["rand_34", "rand_44", "sep_knots_22", "zero_one_cell"], ["f32_knots_34"]),
         "zeros3": (["rand_222", "rand_333", "sep_knots_222", "zero_one_cell"], ["f32_knots_233"]),
         "project": (["curve_k6", "surface_k24_mixed", "surface_k44_uniform"], ["curve_k4_float32", "surface_k43_float32"]),
         "contours": (["random_34", "random_44"], ["float32"]),
         "remove": (["recover/curve_o4", "recover/surface_o43", "reduce/curve_40_1e-03"], [])}


def domain_id(dom):
    return f"{dom[0]:g}+{dom[1]:g}"


def moved(knots, order, dom):
    return [sr.map_axis(t, int(k), dom[0], dom[1], t.dtype.type) for t, k in zip(knots, order)]


def runs(family):
    wide, narrow = BASES[family]
    return [(b, d) for b in wide for d in cases.SCALE_DOMAINS] + [(b, d) for b in narrow for d in cases.SCALE_DOMAINS_F32]


def zeros_records(nind):
    g, t = (g2, t2) if nind == 2 else (g3, t3)
    out, names = {}, []
    for base, dom in runs(f"zeros{nind}"):
        c = t.load_case(base)
        kdtype = c["knots"][0].dtype
        assert (kdtype == np.float32) == (dom in cases.SCALE_DOMAINS_F32 and base.startswith("f32_knots")), base
        c = dict(kind=c["kind"], order=c["order"], knots=moved(c["knots"], c["order"], dom), coefs=c["coefs"],
                 lines=[(c["order"][a], None, c.get(f"{p}_coefs")) for a, p in enumerate("uvw"[:nind])])
        assert all(len(np.unique(k)) == len(np.unique(b)) for k, b in zip(c["knots"], t.load_case(base)["knots"])), "knots merged by the rounding"
        if c["kind"] in ("coupled", "zero"):
            assert g.certified(c["order"], c["knots"], c["coefs"]) is not None, f"{base} on {dom}: not certified, or not as well conditioned"
        elif c["kind"] == "separable":
            c["lines"] = [(k, knots, line) for (k, _, line), knots in zip(c["lines"], c["knots"])]
            for k, knots, line in c["lines"]:                       # every 1-D factor decided exactly, its roots simple
                exact = g.one_d("x", k, knots, line)[0]
                assert len(exact["x_lo"]) >= 1 and np.all(exact["x_fprime"] != 0.0), f"{base} on {dom}"
        else:
            raise AssertionError(f"{base}: no rule for the kind {c['kind']}")
        exact, extra = g.exact_of(c)
        name = f"{base}@{domain_id(dom)}"
        rec = dict(order=np.array(c["order"], np.int32), coefs=c["coefs"], kind=np.array(c["kind"]), ref_roots=np.empty((0, nind)),
                   ref_complete=np.array(False), ref_dev=np.float64("nan"), **{f"knots{a}": k for a, k in enumerate(c["knots"])}, **extra)
        rec["exact_uv" if nind == 2 else "exact_uvw"] = exact
        names.append(name)
        for key, val in rec.items():
            out[f"{name}/{key}"] = val
        print(f"zeros{nind} {name}: {len(exact)} zeros, {len(extra['exact_cells'])} zero cells", flush=True)
    out["names"] = np.array(names)
    return out


def project_records():
    out, names = {}, []
    for base, dom in runs("project"):
        c = tp.load_case(base)
        case = dict(order=c["order"], knots=moved(c["knots"], c["order"], dom), coefs=c["coefs"], samples=c["samples"])
        spline = gp.spline_of(case)
        tables = project.host_tables(spline, case["samples"])
        rows = [gp.record(case, spline, tables, p) for p in c["points"].T]
        assert all(r is not None for r in rows), f"{base} on {dom}: a point is not certified"
        name = f"{base}@{domain_id(dom)}"
        names.append(name)
        out[name + ".order"] = np.array(case["order"], np.int32)
        for a, k in enumerate(case["knots"]):
            out[f"{name}.knots{a}"] = k
        out[name + ".coefs"] = case["coefs"]
        out[name + ".samples"] = np.array(0 if case["samples"] is None else case["samples"], np.int32)
        out[name + ".points"] = c["points"]
        for key in ("u", "radius", "free"):
            out[f"{name}.{key}"] = np.array([r[key] for r in rows]).T
        for key in ("dist_lo", "dist_hi", "gap", "hinv", "jmax", "hmin", "steps"):
            out[f"{name}.{key}"] = np.array([r[key] for r in rows])
        assert np.all(out[name + ".gap"] > gp.MARGIN)
        print(f"project {name}: {len(rows)} points", flush=True)
    out["names"], out["margin"] = np.array(names), np.array(gp.MARGIN)
    return out


def contour_records():
    out, names = {}, []
    for base, dom in runs("contours"):
        order = tc.GOLD[f"{base}/order"]
        knots = moved([tc.GOLD[f"{base}/knots0"], tc.GOLD[f"{base}/knots1"]], order, dom)
        case = dict(order=order, knots=knots, coefs=tc.GOLD[f"{base}/coefs"], depth=int(tc.GOLD[f"{base}/depth"]),
                    level=float(tc.GOLD[f"{base}/level"]), kind=str(tc.GOLD[f"{base}/kind"]))
        why = []
        rec = gc.decide(case, why)
        assert rec is not None, f"{base} on {dom} breaks an assumption of the bars: {why}"
        for key in ("segments", "saddles", "zero", "closed", "lengths", "first_keys", "vkeys"):     # the structure of [0, 1]
            assert np.array_equal(rec[key], tc.GOLD[f"{base}/{key}"]), f"{base} on {dom}: {key} differs from the unit domain's"
        name = f"{base}@{domain_id(dom)}"
        names.append(name)
        for key, value in dict(order=order, knots0=knots[0], knots1=knots[1], coefs=case["coefs"], depth=case["depth"], level=case["level"],
                               kind=case["kind"], ref_count=-1, **rec).items():
            out[f"{name}/{key}"] = value
        print(f"contours {name}: {len(rec['closed'])} components, {len(rec['vkeys'])} vertices", flush=True)
    out["names"] = np.array(names)
    return out


def remove_records():
    out, names = {}, []
    with np.load(os.path.join(HERE, "remove.npz")) as g:
        for base, dom in runs("remove"):
            p = base + "/"
            order = [int(k) for k in g[p + "order"]]
            old = [g[f"{p}knots{iv}"] for iv in range(len(order))]
            knots = moved(old, order, dom)
            q = f"{base}@{domain_id(dom)}/"
            names.append(q[:-1])
            out[q + "order"], out[q + "coefs"], out[q + "ref_ncoef"] = g[p + "order"], g[p + "coefs"], g[p + "ref_ncoef"]
            for iv, t in enumerate(knots):
                out[f"{q}knots{iv}"] = t
            if base.startswith("reduce"):
                out[q + "tolerance"] = g[p + "tolerance"]
                continue
            assert tuple(g[p + "ref_ncoef"]) == g[p + "coefs"].shape[1:], "the reference recovers the case"
            fine = []
            for iv, (t, k) in enumerate(zip(knots, order)):
                new = np.array(sr.map_axis(old[iv], k, dom[0], dom[1], np.float64, values=list(g[f"{p}new{iv}"])))
                fine.append(np.sort(np.concatenate((t, new))))
                assert len(np.unique(np.concatenate((t[k:-k], new)))) == len(t) - 2 * k + len(new), "an inserted knot met another one"
                out[f"{q}new{iv}"], out[f"{q}in_knots{iv}"] = new, fine[-1]
            exact, mask = refine_ref.change_basis(tuple(order), knots, g[p + "coefs"], order, fine)
            assert mask.all()
            out[q + "in_coefs"] = np.asarray(exact, g[p + "coefs"].dtype)
            print(f"remove {q[:-1]}: nCoef {g[p + 'coefs'].shape[1:]} -> {exact.shape[1:]}", flush=True)
    out["names"] = np.array(names)
    return out


def main():
    started = time.time()
    store = {}
    for family, records in (("zeros2", zeros_records(2)), ("zeros3", zeros_records(3)), ("project", project_records()),
                            ("contours", contour_records()), ("remove", remove_records())):
        for key, val in records.items():
            store[f"{family}:{key}"] = val
    store["generator_seconds"] = np.float64(time.time() - started)
    path = os.path.join(HERE, "cell_scale.npz")
    np.savez_compressed(path, **store)
    print(f"{path}: {os.path.getsize(path)} bytes in {time.time() - started:.0f} s")


if __name__ == "__main__":
    main()
