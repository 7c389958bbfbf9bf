"""
The sweep behind tests/test_gpu_solve.py (``bsk_scatter_solve`` against ``bsk_scatter_solve_host`` through the C ABI, byte
for byte) and tests/test_solve_host.py (the same generators and laws on the CPU: the host solve against the plain-float
statement ``scatter.solve_statement``).  A solver is a function (system, stencil (n, S), rhs (n, nDep)) -> (coefs (nDep, n)
or None, bad_row); ``compare`` and the laws take two of them, or one.

Systems (NB = 32 rows to a panel of the device solve, hb the half bandwidth min((K0 - 1) n1 + K1 - 1, n - 1)):
    curves      orders 2, 3, 4 with n = K, NB - 1, NB, NB + 1, 2 NB + 1
    full        4 x 4 bicubic: hb = n - 1, the band is the whole matrix
    edge        orders (2, 2), n1 = 30, 31, 32: hb = 31, 32, 33, just below, at and above NB
    panels      10 x 10 bicubic: three panels and a remainder of 4 rows
    holes       n1 = K1: (3, 3) 7 x 3 and (4, 4) 9 x 4
    mixed       orders (2, 4), (4, 2), (3, 4), (4, 4) at 5 x 4, 9 x 7, 13 x 11
Stencils:
    assembled   by the host path from random points, without and with smoothing E
    integer     64 U^T D U for a unit upper U with entries +-1/8 at the offsets the stencil holds and D in {16, 32}: symmetric,
                strictly diagonally dominant, all integers, and every value of the factorisation and of both substitutions is
                a small dyadic number, so the solve is exact: rhs = N x for integer x gives back x itself
"""
import functools

import numpy as np

from bspy_amd import _native as nv
from bspy_amd import scatter

NB = 32


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64).tolist()


class System:
    def __init__(self, name, order, ncoef):
        self.name, self.order, self.ncoef = name, tuple(order), tuple(ncoef)
        self.nind = len(order)
        self.K01, self.n01 = (self.order + (1,))[:2], (self.ncoef + (1,))[:2]
        self.n = int(np.prod(ncoef))
        self.S = (2 * self.K01[0] - 1) * (2 * self.K01[1] - 1)
        self.hb = min((self.K01[0] - 1) * self.n01[1] + self.K01[1] - 1, self.n - 1)
        self.knots = [np.concatenate((np.zeros(k - 1), np.linspace(0.0, 1.0, n - k + 2), np.ones(k - 1))) for k, n in zip(order, ncoef)]
        self.head = (self.nind,) + self.K01 + self.n01

    def __repr__(self):
        return self.name


def systems():
    out = []
    for K in (2, 3, 4):
        for n in (K, NB - 1, NB, NB + 1, 2 * NB + 1):
            out.append(System(f"curve{K}_n{n}", (K,), (n,)))
    out.append(System("full_4x4", (4, 4), (4, 4)))
    for n1 in (30, 31, 32):
        out.append(System(f"edge_2x2_4x{n1}", (2, 2), (4, n1)))
    out.append(System("panels_10x10", (4, 4), (10, 10)))
    out.append(System("holes_3x3_7x3", (3, 3), (7, 3)))
    out.append(System("holes_4x4_9x4", (4, 4), (9, 4)))
    for order in ((2, 4), (4, 2), (3, 4), (4, 4)):
        for ncoef in ((5, 4), (9, 7), (13, 11)):
            out.append(System(f"mixed_{order[0]}{order[1]}_{ncoef[0]}x{ncoef[1]}", order, ncoef))
    return out


SYSTEMS = systems()
BY_NAME = {s.name: s for s in SYSTEMS}
REFUSALS = ("curve4_n65", "panels_10x10")                                   # n = 65 and 100: a first, a later and a last panel


# ------------------------------------------------------------------------------------------ stencils
@functools.lru_cache(maxsize=None)
def assembled(name, smoothing):
    """(stencil, rhs (n, 4)) of random points on the system, by the host path."""
    sy = BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    N = 40 * sy.n + 50
    uvw = rng.random((sy.nind, N))
    uvw[:, :2] = [[0.0, 1.0]] * sy.nind                                      # both domain ends
    points = rng.standard_normal((4, N))
    sh = scatter.Shape(sy.order, sy.knots)
    res = scatter.assemble(scatter.Host(), sh, uvw, points, rng.random(N) + 0.25)
    stencil = res["stencil"]
    if smoothing:
        stencil = stencil + smoothing * scatter.penalty_stencil(sy.order, sy.knots, 1)
    return np.ascontiguousarray(stencil), np.ascontiguousarray(res["rhs"])


def offsets(sy):
    """The (d0, d1) at which U of the integer family has entries."""
    if sy.nind == 1:
        return [(1, 0)] + ([(2, 0)] if sy.K01[0] >= 3 else [])
    return [(0, 1), (1, 0)]


def integer(sy, pivots=None):
    """(stencil, rhs (n, 4), x (4, n)) of the integer family; ``pivots`` {row: D} replaces pivots (0.0, a negative one)."""
    rng = np.random.default_rng(sy.n + 7 * sy.hb)
    n, (n0, n1), (K0, K1) = sy.n, sy.n01, sy.K01
    D = rng.choice([16.0, 32.0], n)
    for row, value in (pivots or {}).items():
        D[row] = value
    U = np.eye(n)
    for i0 in range(n0):
        for i1 in range(n1):
            for d0, d1 in offsets(sy):
                if i0 + d0 < n0 and i1 + d1 < n1:
                    U[i0 * n1 + i1, (i0 + d0) * n1 + i1 + d1] = rng.choice([-0.125, 0.125])
    dense = 64.0 * (U.T @ (D[:, None] * U))                                 # exact: small dyadic numbers
    stencil = np.zeros((n, 2 * K0 - 1, 2 * K1 - 1))
    seen = np.zeros_like(dense, bool)
    for i0 in range(n0):
        for i1 in range(n1):
            for e0 in range(2 * K0 - 1):
                for e1 in range(2 * K1 - 1):
                    j0, j1 = i0 + e0 - (K0 - 1), i1 + e1 - (K1 - 1)
                    if 0 <= j0 < n0 and 0 <= j1 < n1:
                        stencil[i0 * n1 + i1, e0, e1] = dense[i0 * n1 + i1, j0 * n1 + j1]
                        seen[i0 * n1 + i1, j0 * n1 + j1] = True
    assert not dense[~seen].any()                                           # the stencil holds every entry of the matrix
    x = rng.integers(-8, 9, (4, n)).astype(np.float64)
    return stencil.reshape(n, -1), np.ascontiguousarray((dense @ x.T)), x, dense


def cases(sy):
    """name -> (stencil, rhs (n, 4)) of a system."""
    out = {"assembled": assembled(sy.name, 0.0), "smoothed": assembled(sy.name, 0.03125)}
    out["integer"] = integer(sy)[:2]
    return out


# ------------------------------------------------------------------------------------------ solvers
def host_solver(sy, stencil, rhs):
    stencil, rhs = np.ascontiguousarray(stencil, np.float64), np.ascontiguousarray(rhs, np.float64)
    ndep = rhs.shape[1]
    coefs, bad = np.empty((ndep, sy.n)), np.full(1, 77, np.int64)
    st = nv.lib().bsk_scatter_solve_host(*sy.head, ndep, stencil.ctypes.data, rhs.ctypes.data, coefs.ctypes.data, bad.ctypes.data_as(nv._i64p))
    assert (st == nv.BSK_OK) == (bad[0] == -1)
    return (coefs if st == nv.BSK_OK else None), int(bad[0])


def statement_solver(sy, stencil, rhs):
    coefs, bad = scatter.solve_statement(sy.order, sy.ncoef, np.asarray(stencil).tolist(), np.asarray(rhs).tolist())
    return (None if coefs is None else np.array(coefs)), bad


# ------------------------------------------------------------------------------------------ the checks
def compare(one, two, sy, stencil, rhs):
    a, bad_a = one(sy, stencil, rhs)
    b, bad_b = two(sy, stencil, rhs)
    assert bad_a == bad_b, (sy, bad_a, bad_b)
    if bad_a == -1:
        assert bits(a) == bits(b), sy
    return a


def sweep(one, two, names=None, kinds=("assembled", "smoothed", "integer")):
    """Every system and stencil, ndep 4, byte for byte; the integer family gives back its x."""
    for sy in SYSTEMS:
        if names is not None and sy.name not in names:
            continue
        mine = cases(sy)
        for kind in kinds:
            got = compare(one, two, sy, *mine[kind])
            if kind == "integer":
                assert bits(got) == bits(integer(sy)[2]), sy


def law_channels(solver, sy):
    """coefs[:d] of the ndep = 4 solve are the bits of the ndep = d solve."""
    stencil, rhs = cases(sy)["assembled"]
    whole, _ = solver(sy, stencil, rhs)
    for d in (1, 2, 3):
        part, bad = solver(sy, stencil, np.ascontiguousarray(rhs[:, :d]))
        assert bad == -1 and bits(part) == bits(whole[:d]), (sy, d)


def law_scale(solver, sy):
    """Stencil and rhs x 2^k keep every bit."""
    stencil, rhs = cases(sy)["smoothed"]
    want, _ = solver(sy, stencil, rhs)
    for k in (1, -1, 37, -37):
        got, bad = solver(sy, np.ldexp(stencil, k), np.ldexp(rhs, k))
        assert bad == -1 and bits(got) == bits(want), (sy, k)


def law_twice(solver, sy):
    stencil, rhs = cases(sy)["assembled"]
    assert bits(solver(sy, stencil, rhs)[0]) == bits(solver(sy, stencil, rhs)[0])


def refusals(sy):
    """name -> (stencil, rhs, the bad row): a zero, a negative and a NaN pivot in the first panel, a later one and the last
    row; two bad rows."""
    n, out = sy.n, {}
    centre = (sy.S - 1) // 2
    for where, row in (("first", 3), ("later", NB + 8), ("last", n - 1)):
        for what, value in (("zero", 0.0), ("negative", -16.0)):
            stencil, rhs = integer(sy, {row: value})[:2]
            out[f"{what}_{where}"] = (stencil, rhs, row)
        stencil, rhs = (a.copy() for a in cases(sy)["assembled"])
        stencil[row, centre] = np.nan
        out[f"nan_{where}"] = (stencil, rhs, row)
    stencil, rhs = integer(sy, {NB + 8: 0.0, n - 2: -16.0})[:2]
    out["two"] = (stencil, rhs, NB + 8)
    return out


def check_refusals(one, two, sy):
    for name, (stencil, rhs, row) in refusals(sy).items():
        for solver in (one, two):
            coefs, bad = solver(sy, stencil, rhs)
            assert bad == row, (sy, name, bad, row)
