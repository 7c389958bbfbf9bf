"""
The operator families away from unit scale, on the GPU: band_apply / band_apply_line, band_product_line / band_product_tile,
scan_apply / scan_line / sum_bcast and roots_flag / roots_isolate (DESIGN.md sections 13-16).  The cases, the checks and
their reasons are those of tests/test_scale_host.py (section "operator families": CPU preconditions, the trim rule, the
bars), run here with path="device"; every result is tied to the kernels that made it (``LAST_PATHS`` and the
``*_last_kernel`` functions, asserted in run_op / run_roots before and after every transform).

A. Exact scaling laws, bit for bit after undoing the power of two: coefficients, result knots, roots, intervals; offsets,
   candidates and counts unchanged.  Families moved off the bitwise law: none.
B. Shifted and stretched domains against the exact references on the stored shifted values; the host path's distance is
   printed and recorded alongside.
C. Locality under one ill-scaled coefficient: outputs with an exact weight of zero keep their bits.
"""
import numpy as np
import pytest

import cases
import test_scale_host as host
from bspy_amd import refinement, roots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OC = host.OC


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", sorted(host.OPS_A))
def test_operator_scaling_law(name):
    host.check_op_law(host.OPS_A[name], "device")


@pytest.mark.parametrize("name", sorted(host.ROOT_SPECS))
def test_roots_scaling_law(name, monkeypatch):
    spec = host.ROOT_SPECS[name]
    if not (roots.DEVICE_MIN_K <= spec[0][0] <= roots.DEVICE_MAX_K):
        with pytest.raises(ValueError, match="device path covers orders"):
            host.run_roots(spec, "device", monkeypatch)
        return
    base = host.check_roots_law(spec, "device", monkeypatch, name)
    on_host = host.run_roots(spec, "host", monkeypatch)
    assert base["values"].tobytes() == on_host["values"].tobytes() and base["offsets"].tolist() == on_host["offsets"].tolist()
    if name.startswith("257"):
        assert "roots_isolate" in base["ran"] and len(base["cand"]) > 256, "more than one workgroup of candidates"


def test_every_kernel_is_named_by_every_part():
    """The cases declare their kernels and run_op / run_roots assert them on every device run, so the declarations are
    what ran: every kernel of the four families in part A, in part B and in part C."""
    parts = {"A": list(host.OPS_A.values()), "B": list(host.OPS_B.values()), "C": [c for c, _ in host.locality_cases()]}
    for part, listed in parts.items():
        named = set().union(*(c.kernels for c in listed))
        assert named == host.ALL_KERNELS - cases.OPERATOR_KERNELS["roots"], (part, named)
    # the roots tests of the three parts: test_roots_scaling_law, test_roots_shifted_domain, test_roots_locality
    ran = set()
    for spec in (host.ROOT_SPECS["golden chebyshev_o6"], OC["roots_curves"][np.float64], host.shifted_root_spec(np.float64, OC["domains"][1])):
        (k,), (t,), coefs = spec
        roots.zeros_batch(host.Spline(1, coefs.shape[0], [k], [coefs.shape[1]], [t], coefs), _path="device")
        assert set(roots.LAST_PATHS) >= cases.OPERATOR_KERNELS["roots"], roots.LAST_PATHS
        ran |= set(roots.LAST_PATHS)
    assert ran == cases.OPERATOR_KERNELS["roots"] | {"band_apply_line"}


# ------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("dom", OC["domains"], ids=host.domain_id)
@pytest.mark.parametrize("family", ["band", "product", "sum"])
def test_operator_shifted_domain(family, dom):
    host.check_shifted_family(family, "fp64", dom, ["device", "host"])


@pytest.mark.parametrize("dom", OC["domains_f32"], ids=host.domain_id)
@pytest.mark.parametrize("family", ["band", "product", "sum"])
def test_operator_shifted_domain_fp32(family, dom):
    host.check_shifted_family(family, "fp32", dom, ["device", "host"])


@pytest.mark.parametrize("dt,dom", host.ROOT_DOMAINS, ids=[host.root_domain_id(p) for p in host.ROOT_DOMAINS])
def test_roots_shifted_domain(dt, dom, monkeypatch):
    host.check_shifted_roots(dt, dom, ["device", "host"], monkeypatch)


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("name", sorted(host.LOCALITY))
def test_locality(name):
    host.check_locality(*host.LOCALITY[name], "device")


def test_extraction_locality():
    def extract(coefs, plan):
        out, ran = refinement.run_device(torch.from_numpy(np.ascontiguousarray(coefs)).cuda(), plan.steps)
        assert ran == ["band_apply_line"]
        return out.cpu().numpy()
    host.check_extraction_locality(extract)


def test_roots_locality(monkeypatch):
    host.check_roots_locality("device", monkeypatch)
