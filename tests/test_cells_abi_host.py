"""
The argument contract of the cell families' C entry points (no GPU): bsk_roots_*, bsk_roots2_*, bsk_roots3_*,
bsk_project_*, bsk_contour_*, bsk_rays_* and bsk_ssx_*, twenty-one ``x_host`` / ``x`` pairs.  Every entry gets one rejected call per failure branch
of its checks, held to the status AND to the exact text of ``bsk_last_error()``; every ``x_host`` entry gets one accepted
call, held to ``bsk_<family>_last_kernel()`` and to what it wrote.  A device twin checks its arguments before it touches HIP, so its rejected
calls need no device: they pass a null stream.

The inputs are the smallest there are: one system, one cell, orders 2 (rays: a 1 x 1 bilinear cell and one ray; ssx: two
1 x 1 bilinear surfaces with G = 1).  Every rejected call differs from the valid one in one fault alone, so the order of
the checks is not pinned.  A rejected call reads none of its arrays, so the
extents that make it "too large" stand for no memory.

Where the twins differ, the difference is pinned as it is: the device twins take fewer orders (roots 8 of 16, roots2 4
of 6) and say where the others go; ``bsk_roots_isolate`` refuses more candidates than spans where its host twin runs them;
``bsk_project_newton`` and ``bsk_contour_march`` refuse what one launch cannot hold, which the host twins would loop over
(those two are therefore called on the device twin only).  ``bsk_project_seed`` has the same launch bound, but "array too
large" refuses every such call first (npts <= 5e11 < 2^31 blocks of 256), on both twins: no call reaches it.
"""
import numpy as np
import pytest

from bspy_amd import _native as nv

INVALID, UNSUPPORTED = nv.BSK_ERR_INVALID, nv.BSK_ERR_UNSUPPORTED
NULL = "NULL argument"
LARGE = "array too large"
ONE_CELL2 = "the rows must hold one cell (R0 >= K0, R1 >= K1)"


def twins(entry):
    """(name, trailing arguments, is the device twin) of a pair."""
    return ((entry + "_host", (), False), (entry, (None,), True))


def ptr(a):
    return a.ctypes.data


class Entry:
    """One entry point on valid arguments (a dict in the order of the C signature; the arrays are kept alive in it)."""

    def __init__(self, name_, tail_, arrays_, **args):
        self.name, self.tail, self.arrays, self.args = name_, tail_, arrays_, args

    def call(self, **change):
        args = dict(self.args, **change)
        assert set(args) == set(self.args), sorted(set(args) - set(self.args))
        return getattr(nv.lib(), self.name)(*args.values(), *self.tail)

    def rejects(self, want_, text_, **change):
        assert self.call(**change) == want_, (self.name, change)
        assert nv.lib().bsk_last_error().decode() == f"{self.name}: {text_}", (self.name, change)

    def null(self, *keys, text=NULL):
        for key in keys:
            self.rejects(INVALID, text, **{key: None})

    def accepts(self, last_, kernel_, **change):
        assert self.call(**change) == nv.BSK_OK, (self.name, nv.lib().bsk_last_error())
        assert last_().decode() == kernel_


# ------------------------------------------------------------------------------------------------------------ roots
def roots_arrays():
    a = dict(rows=np.array([[-1.0, 1.0]]), first=np.zeros(1, np.int32), mask=np.zeros(1, np.uint8), flags=np.zeros(1, np.uint8),
             breaks=np.array([0.0, 1.0]), scale=np.ones(1), cand=np.zeros(2, np.int64), roots=np.full((2, 1), -1.0),
             count=np.full(2, -1, np.int32))
    grid = dict(dtype=nv.BSK_F64, order=2, rows=ptr(a["rows"]), ncomp=1, rowlen=2, nspans=1, first=ptr(a["first"]), mask=ptr(a["mask"]))
    return a, grid


def roots_call_checks(e, device):
    e.null("rows", "first", "mask")
    e.rejects(INVALID, "dtype must be BSK_F32 or BSK_F64", dtype=2)
    e.rejects(INVALID, "order must be >= 2", order=1)
    if device:
        e.rejects(UNSUPPORTED, "order above 8 (the host driver takes it)", order=9, rowlen=9)
    else:
        e.rejects(UNSUPPORTED, "order above 16", order=17, rowlen=17)
    e.rejects(INVALID, "ncomp and nspans must be >= 1", ncomp=0)
    e.rejects(INVALID, "ncomp and nspans must be >= 1", nspans=0)
    e.rejects(INVALID, "rowlen must be >= order", rowlen=1)
    e.rejects(INVALID, LARGE, ncomp=10 ** 12)
    e.rejects(INVALID, LARGE, rowlen=10 ** 16)


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots_flag"))
def test_roots_flag(name, tail, device):
    a, grid = roots_arrays()
    e = Entry(name, tail, a, **grid, flags=ptr(a["flags"]))
    roots_call_checks(e, device)
    e.null("flags")
    if not device:
        e.accepts(nv.lib().bsk_roots_last_kernel, "host roots_flag")
        assert a["flags"].tolist() == [1]
        e.accepts(nv.lib().bsk_roots_last_kernel, "host roots_flag", dtype=nv.BSK_F32, rows=ptr(a["rows"].astype(np.float32)))


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots_isolate"))
def test_roots_isolate(name, tail, device):
    a, grid = roots_arrays()
    e = Entry(name, tail, a, **grid, breaks=ptr(a["breaks"]), scale=ptr(a["scale"]), margin=0.0, cand=ptr(a["cand"]), ncand=1,
              roots=ptr(a["roots"]), count=ptr(a["count"]))
    roots_call_checks(e, device)
    e.null("breaks", "scale", "cand", "roots", "count")
    e.rejects(INVALID, "ncand must be >= 1 (no candidates: no call)", ncand=0)
    for margin in (-1.0, float("nan"), float("inf")):
        e.rejects(INVALID, "margin must be finite and >= 0", margin=margin)
    if device:
        e.rejects(INVALID, "more candidates than spans", ncand=2)
    else:
        e.accepts(nv.lib().bsk_roots_last_kernel, "host roots_isolate")
        assert a["count"].tolist() == [1, -1] and a["roots"].ravel().tolist() == [0.5, -1.0]
        e.accepts(nv.lib().bsk_roots_last_kernel, "host roots_isolate", ncand=2)       # the host twin runs the span twice
        assert a["count"].tolist() == [1, 1] and a["roots"].ravel().tolist() == [0.5, 0.5]


# ------------------------------------------------------------------------------------------------------------ roots2
def roots2_arrays():
    f = np.array([[-0.5, -0.5], [0.5, 0.5]])
    a = dict(rows=np.ascontiguousarray(np.stack([f, f.T])[None]), first0=np.zeros(1, np.int32), first1=np.zeros(1, np.int32),
             mask=np.zeros(1, np.uint8), flags=np.zeros(1, np.uint8), breaks0=np.array([0.0, 1.0]), breaks1=np.array([0.0, 1.0]),
             scale=np.full((1, 2), 0.5), cand=np.zeros(1, np.int64), roots=np.full((1, 2, 2), -1.0), near=np.zeros((1, 2), np.uint8),
             count=np.zeros(1, np.int32), status=np.zeros(1, np.uint8), nodes=np.zeros(1, np.int32), table=np.zeros(1, np.int64),
             which=np.zeros(1, np.int64), keep=np.zeros((1, 2), np.uint8))
    grid = dict(K0=2, K1=2, rows=ptr(a["rows"]), nsys=1, R0=2, R1=2, nc0=1, nc1=1, first0=ptr(a["first0"]), first1=ptr(a["first1"]))
    return a, grid


def roots2_call_checks(e, device):
    e.null("rows", "first0", "first1")
    for key in ("K0", "K1"):
        e.rejects(INVALID, "orders must be >= 2", **{key: 1})
        if device:
            e.rejects(UNSUPPORTED, "order above 4 (the host driver takes orders up to 6)", **{key: 5})
        else:
            e.rejects(UNSUPPORTED, "order above 6", **{key: 7})
    for key in ("nsys", "nc0", "nc1"):
        e.rejects(INVALID, "nsys, nc0 and nc1 must be >= 1", **{key: 0})
    for key in ("R0", "R1"):
        e.rejects(INVALID, ONE_CELL2, **{key: 1})
    e.rejects(INVALID, LARGE, nsys=10 ** 12)
    e.rejects(INVALID, LARGE, R0=10 ** 16)


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots2_flag"))
def test_roots2_flag(name, tail, device):
    a, grid = roots2_arrays()
    e = Entry(name, tail, a, **grid, mask=ptr(a["mask"]), flags=ptr(a["flags"]))
    roots2_call_checks(e, device)
    e.null("mask", "flags")
    if not device:
        e.accepts(nv.lib().bsk_roots2_last_kernel, "host roots2_flag")
        assert a["flags"].tolist() == [1]


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots2_isolate"))
def test_roots2_isolate(name, tail, device):
    a, grid = roots2_arrays()
    e = Entry(name, tail, a, **grid, breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]), scale=ptr(a["scale"]), cand=ptr(a["cand"]),
              ncand=1, roots=ptr(a["roots"]), near=ptr(a["near"]), count=ptr(a["count"]), status=ptr(a["status"]), nodes=ptr(a["nodes"]))
    roots2_call_checks(e, device)
    e.null("status", "breaks0", "breaks1", "scale", "cand", "roots", "near", "count", "nodes")
    e.rejects(INVALID, "ncand must be >= 1 (no candidates: no call)", ncand=0)
    e.rejects(INVALID, "more candidates than cells", ncand=2)
    if not device:
        e.accepts(nv.lib().bsk_roots2_last_kernel, "host roots2_isolate")
        assert a["count"].tolist() == [1] and a["roots"][0, 0].tolist() == [0.5, 0.5]


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots2_merge"))
def test_roots2_merge(name, tail, device):
    a, _ = roots2_arrays()
    a["roots"][:] = [[0.5, 0.5], [np.nan, np.nan]]
    a["flags"][:] = 1
    e = Entry(name, tail, a, R=2, roots=ptr(a["roots"]), nsys=1, nc0=1, nc1=1, breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]),
              cand=ptr(a["cand"]), ncand=1, flags=ptr(a["flags"]), table=ptr(a["table"]), which=ptr(a["which"]), nnear=1, keep=ptr(a["keep"]))
    e.null("roots", "breaks0", "breaks1", "cand", "flags", "table", "which", "keep")
    for R in (1, 51):
        e.rejects(INVALID, "R must be 2 (K0 - 1)(K1 - 1) of covered orders", R=R)
    for key in ("nsys", "nc0", "nc1"):
        e.rejects(INVALID, "nsys, nc0 and nc1 must be >= 1", **{key: 0})
    e.rejects(INVALID, LARGE, nsys=10 ** 12)
    for ncand in (0, 2):
        e.rejects(INVALID, "ncand must be in [1, cells]", ncand=ncand)
    for nnear in (0, 3):
        e.rejects(INVALID, "nnear must be in [1, ncand R] (no root near an edge: no call)", nnear=nnear)
    if not device:
        e.accepts(nv.lib().bsk_roots2_last_kernel, "host roots2_merge")
        assert a["keep"].tolist() == [[1, 0]]


# ------------------------------------------------------------------------------------------------------------ roots3
def roots3_arrays():
    f = np.broadcast_to(np.array([-0.5, 0.5])[:, None, None], (2, 2, 2))
    a = dict(rows=np.ascontiguousarray(np.stack([f, f.transpose(1, 0, 2), f.transpose(2, 1, 0)])[None]), mask=np.zeros(1, np.uint8),
             flags=np.zeros(1, np.uint8), scale=np.full((1, 3), 0.5), cand=np.zeros(1, np.int64), roots=np.full((1, 6, 3), -1.0),
             near=np.zeros((1, 6), np.uint8), count=np.zeros(1, np.int32), status=np.zeros(1, np.uint8), nodes=np.zeros(1, np.int32),
             table=np.zeros(1, np.int64), which=np.zeros(1, np.int64), keep=np.zeros((1, 6), np.uint8))
    for d in range(3):
        a[f"first{d}"], a[f"breaks{d}"] = np.zeros(1, np.int32), np.array([0.0, 1.0])
    grid = dict(K0=2, K1=2, K2=2, rows=ptr(a["rows"]), nsys=1, R0=2, R1=2, R2=2, nc0=1, nc1=1, nc2=1, first0=ptr(a["first0"]),
                first1=ptr(a["first1"]), first2=ptr(a["first2"]))
    return a, grid


def roots3_call_checks(e):
    e.null("rows", "first0", "first1", "first2")
    for key in ("K0", "K1", "K2"):
        e.rejects(INVALID, "orders must be >= 2", **{key: 1})
        e.rejects(UNSUPPORTED, "order above 4 (one wave holds 64 coefficients)", **{key: 5})
    for key in ("nsys", "nc0", "nc1", "nc2"):
        e.rejects(INVALID, "nsys, nc0, nc1 and nc2 must be >= 1", **{key: 0})
    for key in ("R0", "R1", "R2"):
        e.rejects(INVALID, "the rows must hold one cell (R0 >= K0, R1 >= K1, R2 >= K2)", **{key: 1})
    e.rejects(INVALID, LARGE, nsys=10 ** 12)
    e.rejects(INVALID, LARGE, R0=10 ** 16)


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots3_flag"))
def test_roots3_flag(name, tail, device):
    a, grid = roots3_arrays()
    e = Entry(name, tail, a, **grid, mask=ptr(a["mask"]), flags=ptr(a["flags"]))
    roots3_call_checks(e)
    e.null("mask", "flags")
    if not device:
        e.accepts(nv.lib().bsk_roots3_last_kernel, "host roots3_flag")
        assert a["flags"].tolist() == [1]


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots3_isolate"))
def test_roots3_isolate(name, tail, device):
    a, grid = roots3_arrays()
    e = Entry(name, tail, a, **grid, breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]), breaks2=ptr(a["breaks2"]), scale=ptr(a["scale"]),
              cand=ptr(a["cand"]), ncand=1, roots=ptr(a["roots"]), near=ptr(a["near"]), count=ptr(a["count"]), status=ptr(a["status"]),
              nodes=ptr(a["nodes"]))
    roots3_call_checks(e)
    e.null("status", "breaks0", "breaks1", "breaks2", "scale", "cand", "roots", "near", "count", "nodes")
    e.rejects(INVALID, "ncand must be >= 1 (no candidates: no call)", ncand=0)
    e.rejects(INVALID, "more candidates than cells", ncand=2)
    e.rejects(INVALID, "more candidates than one launch takes (2^31 - 1)", nsys=2 ** 31, ncand=2 ** 31)       # on both twins
    if not device:
        e.accepts(nv.lib().bsk_roots3_last_kernel, "host roots3_isolate")
        assert a["count"].tolist() == [1] and a["roots"][0, 0].tolist() == [0.5, 0.5, 0.5]


@pytest.mark.parametrize("name,tail,device", twins("bsk_roots3_merge"))
def test_roots3_merge(name, tail, device):
    a, _ = roots3_arrays()
    a["roots"][:] = np.nan
    a["roots"][0, 0] = 0.5
    a["flags"][:] = 1
    e = Entry(name, tail, a, R=6, roots=ptr(a["roots"]), nsys=1, nc0=1, nc1=1, nc2=1, breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]),
              breaks2=ptr(a["breaks2"]), cand=ptr(a["cand"]), ncand=1, flags=ptr(a["flags"]), table=ptr(a["table"]), which=ptr(a["which"]),
              nnear=1, keep=ptr(a["keep"]))
    e.null("roots", "breaks0", "breaks1", "breaks2", "cand", "flags", "table", "which", "keep")
    for R in (5, 33):
        e.rejects(INVALID, "R must be min(6 (K0 - 1)(K1 - 1)(K2 - 1), 32) of covered orders", R=R)
    for key in ("nsys", "nc0", "nc1", "nc2"):
        e.rejects(INVALID, "nsys, nc0, nc1 and nc2 must be >= 1", **{key: 0})
    e.rejects(INVALID, LARGE, nsys=10 ** 12)
    for ncand in (0, 2):
        e.rejects(INVALID, "ncand must be in [1, cells]", ncand=ncand)
    for nnear in (0, 7):
        e.rejects(INVALID, "nnear must be in [1, ncand R] (no zero near a face: no call)", nnear=nnear)
    if not device:
        e.accepts(nv.lib().bsk_roots3_last_kernel, "host roots3_merge")
        assert a["keep"].tolist() == [[1, 0, 0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------------------------ project
def project_arrays():
    """The segment (0, 0) - (1, 0) as a curve of order 2, one sample (its middle), the point (0.25, 1)."""
    return dict(rows=np.array([[0.0, 1.0], [0.0, 0.0]]), samples=np.array([[0.5], [0.0]]), points=np.array([[0.25], [1.0]]),
                part_d2=np.zeros((1, 1)), part_idx=np.zeros((1, 1), np.int32), first0=np.zeros(1, np.int32), first1=np.zeros(1, np.int32),
                breaks0=np.array([0.0, 1.0]), breaks1=np.array([0.0, 1.0]), guess=np.full((1, 1), 0.5), uvw=np.zeros((1, 1)),
                distance=np.zeros(1), status=np.zeros(1, np.uint8), steps=np.zeros(1, np.int32))


@pytest.mark.parametrize("name,tail,device", twins("bsk_project_seed"))
def test_project_seed(name, tail, device):
    a = project_arrays()
    e = Entry(name, tail, a, ndep=2, samples=ptr(a["samples"]), nsamples=1, points=ptr(a["points"]), npts=1, chunk=1,
              part_d2=ptr(a["part_d2"]), part_idx=ptr(a["part_idx"]))
    e.null("samples", "points", "part_d2", "part_idx")
    for key in ("nsamples", "npts", "chunk"):
        e.rejects(INVALID, "nsamples, npts and chunk must be >= 1", **{key: 0})
    for ndep in (1, 4):
        e.rejects(UNSUPPORTED, "ndep must be 2 or 3", ndep=ndep)
    e.rejects(INVALID, "more than 2^31 - 1 samples", nsamples=2 ** 31, chunk=2 ** 31)
    e.rejects(INVALID, "more than 65535 chunks", nsamples=65536)
    e.rejects(INVALID, LARGE, npts=10 ** 12)
    e.rejects(INVALID, LARGE, npts=6 * 10 ** 11)                       # 2^31 blocks and more: refused here, on both twins
    if not device:
        e.accepts(nv.lib().bsk_project_last_kernel, "host project_seed")
        assert a["part_d2"].tolist() == [[0.0625 + 1.0]] and a["part_idx"].tolist() == [[0]]


@pytest.mark.parametrize("name,tail,device", twins("bsk_project_newton"))
def test_project_newton(name, tail, device):
    a = project_arrays()
    a["part_d2"][:] = 1.0625
    e = Entry(name, tail, a, nind=1, K0=2, K1=1, ndep=2, rows=ptr(a["rows"]), R0=2, R1=1, nc0=1, nc1=1, first0=ptr(a["first0"]),
              first1=ptr(a["first1"]), breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]), g0=1, g1=1, points=ptr(a["points"]), npts=1,
              part_d2=ptr(a["part_d2"]), part_idx=ptr(a["part_idx"]), nchunks=1, guess=None, uvw=ptr(a["uvw"]), distance=ptr(a["distance"]),
              status=ptr(a["status"]), steps=ptr(a["steps"]))
    surface = dict(nind=2, K1=2, R1=2)                              # passes the checks up to the orders; never run
    e.null("rows", "first0", "first1", "breaks0", "breaks1", "points", "uvw", "distance", "status", "steps")
    e.null("part_d2", "part_idx", text="neither a guess nor the partials of the seed")
    e.rejects(INVALID, "nchunks must be >= 1", nchunks=0)
    for key in ("npts", "nc0", "nc1"):
        e.rejects(INVALID, "npts, nc0 and nc1 must be >= 1", **{key: 0})
    for nind in (0, 3):
        e.rejects(UNSUPPORTED, "nind must be 1 (curves) or 2 (surfaces)", nind=nind)
    for ndep in (1, 4):
        e.rejects(UNSUPPORTED, "ndep must be 2 or 3", ndep=ndep)
    for change in (dict(K1=2), dict(R1=2), dict(nc1=2), dict(g1=2)):
        e.rejects(INVALID, "a curve has K1 = R1 = nc1 = g1 = 1", **change)
    e.rejects(INVALID, "orders must be >= 2", K0=1)
    e.rejects(INVALID, "orders must be >= 2", **dict(surface, K1=1))
    e.rejects(UNSUPPORTED, "curves of order 2 to 6", K0=7, R0=7)
    for key in ("K0", "K1"):
        e.rejects(UNSUPPORTED, "surfaces of orders 2 to 4", **dict(surface, R0=5, R1=5, **{key: 5}))
    for change in (dict(g0=0), dict(g0=9), dict(surface, g1=0), dict(surface, g1=9)):
        e.rejects(INVALID, "1 to 8 samples per cell and axis", **change)
    e.rejects(INVALID, ONE_CELL2, R0=1)
    e.rejects(INVALID, ONE_CELL2, **dict(surface, R1=1))
    e.rejects(INVALID, "more than 2^31 - 1 samples", nc0=2 ** 31)
    e.rejects(INVALID, LARGE, R0=10 ** 16)
    e.rejects(INVALID, LARGE, npts=10 ** 12)
    e.rejects(INVALID, LARGE, npts=10 ** 6, nchunks=10 ** 6)
    if device:
        e.rejects(INVALID, "too many points for one launch", npts=2 * 10 ** 11)      # 2^31 blocks of 64 and more
    else:
        last = nv.lib().bsk_project_last_kernel
        e.accepts(last, "host project_newton")
        assert a["uvw"].tolist() == [[0.25]] and a["distance"].tolist() == [1.0]
        a["uvw"][:] = -1.0
        e.accepts(last, "host project_newton", guess=ptr(a["guess"]), part_d2=None, part_idx=None, nchunks=0)
        assert a["uvw"].tolist() == [[0.25]]


# ------------------------------------------------------------------------------------------------------------ contour
def contour_arrays():
    """The field 2 u - 1 on one bilinear cell: its zero level is the line u = 1/2."""
    a = dict(rows=np.array([[[-1.0, -1.0], [1.0, 1.0]]]), first0=np.zeros(1, np.int32), first1=np.zeros(1, np.int32), scale=np.ones(1),
             levels=np.zeros(1), flag=np.zeros(1, np.uint8), zero=np.zeros(1, np.uint8), breaks0=np.array([0.0, 1.0]),
             breaks1=np.array([0.0, 1.0]), cand=np.zeros(1, np.int64), offsets=np.zeros(1, np.int64), counts=np.zeros(1, np.int32),
             lane_status=np.zeros(1, np.uint8), keys=np.zeros((2, 2), np.int64), xy=np.zeros((2, 4)))
    grid = dict(K0=2, K1=2, rows=ptr(a["rows"]), nrows=1, R0=2, R1=2, nc0=1, nc1=1, first0=ptr(a["first0"]), first1=ptr(a["first1"]),
                levels=None, nfields=1, scale=ptr(a["scale"]))
    return a, grid


def contour_call_checks(e, a):
    e.null("rows", "first0", "first1", "scale")
    for key in ("K0", "K1"):
        e.rejects(INVALID, "orders must be >= 2", **{key: 1})
        e.rejects(UNSUPPORTED, "orders above 4 are not covered", **{key: 5})
    for key in ("nfields", "nrows", "nc0", "nc1"):
        e.rejects(INVALID, "nfields, nrows, nc0 and nc1 must be >= 1", **{key: 0})
    e.rejects(INVALID, "the rows hold one field with levels and nfields fields without", nrows=2)
    e.rejects(INVALID, "the rows hold one field with levels and nfields fields without", nrows=2, nfields=2, levels=ptr(a["levels"]))
    for key in ("R0", "R1"):
        e.rejects(INVALID, ONE_CELL2, **{key: 1})
    e.rejects(INVALID, LARGE, nc0=2 * 10 ** 9)
    e.rejects(INVALID, LARGE, R0=10 ** 16)


@pytest.mark.parametrize("name,tail,device", twins("bsk_contour_flag"))
def test_contour_flag(name, tail, device):
    a, grid = contour_arrays()
    e = Entry(name, tail, a, **grid, cand=ptr(a["flag"]), zero=ptr(a["zero"]))
    contour_call_checks(e, a)
    e.null("cand", "zero")
    if not device:
        e.accepts(nv.lib().bsk_contour_last_kernel, "host contour_flag")
        assert a["flag"].tolist() == [1] and a["zero"].tolist() == [0]
        e.accepts(nv.lib().bsk_contour_last_kernel, "host contour_flag", levels=ptr(a["levels"]))


@pytest.mark.parametrize("name,tail,device", twins("bsk_contour_march"))
def test_contour_march(name, tail, device):
    a, grid = contour_arrays()
    e = Entry(name, tail, a, **grid, breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]), cand=ptr(a["cand"]), ncand=1, depth=1, split=0,
              emit=0, offsets=None, total=0, counts=ptr(a["counts"]), lane_status=ptr(a["lane_status"]), keys=None, xy=None)
    emit = dict(emit=1, offsets=ptr(a["offsets"]), total=2, counts=None, lane_status=None, keys=ptr(a["keys"]), xy=ptr(a["xy"]))
    contour_call_checks(e, a)
    e.null("breaks0", "breaks1", "cand")
    for depth in (-1, 9):
        e.rejects(INVALID, "depth must be in [0, 8]", depth=depth)
    for split in (-1, 2):
        e.rejects(INVALID, "the split level must be in [0, depth]", split=split)
    e.rejects(INVALID, "ncand must be >= 1 (no candidates: no call)", ncand=0)
    e.rejects(INVALID, "more candidates than cells", ncand=2)
    e.null("counts", "lane_status", text="count takes counts and lane_status")
    for change in (dict(offsets=None), dict(keys=None), dict(xy=None), dict(total=0)):
        e.rejects(INVALID, "emit takes offsets, keys, xy and total >= 1 (no segments: no call)", **dict(emit, **change))
    if device:
        e.rejects(INVALID, "too many lanes", nc0=2 ** 22, ncand=2 ** 22, depth=8, split=8)      # 2^38 lanes: 2^32 blocks of 64
    else:
        last = nv.lib().bsk_contour_last_kernel
        e.accepts(last, "host contour_march count")
        assert a["counts"].tolist() == [2] and a["lane_status"].tolist() == [0]      # depth 1: the line crosses two leaves
        e.accepts(last, "host contour_march emit", **emit)
        assert a["xy"][:, [0, 2]].tolist() == [[0.5, 0.5]] * 2


# ------------------------------------------------------------------------------------------------------------ the surface table
SURFACE_KEYS = ("K0", "K1", "rows", "R0", "R1", "nc0", "nc1", "first0", "first1")


def surface_checks(e, tag=""):
    """The six checks of one surface table (bsk_rays_* has one, bsk_ssx_* two: ``tag`` X and Y)."""
    e.null(*(key + tag for key in ("rows", "first0", "first1")))
    for key in ("K0", "K1"):
        e.rejects(INVALID, "orders must be >= 2", **{key + tag: 1})
        e.rejects(UNSUPPORTED, "order above 4", **{key + tag: 5})
    for key in ("nc0", "nc1"):
        e.rejects(INVALID, "nc0 and nc1 must be >= 1", **{key + tag: 0})
    for key in ("R0", "R1"):
        e.rejects(INVALID, ONE_CELL2, **{key + tag: 1})
    e.rejects(INVALID, LARGE, **{"nc0" + tag: 3 * 10 ** 9})
    e.rejects(INVALID, LARGE, **{"R0" + tag: 10 ** 16})


def same(a, want):
    return np.array_equal(a, np.array(want, a.dtype), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ rays
NAN = float("nan")


def rays_arrays():
    """The cell (u, v, 0) on the unit square and the ray from (1/4, 1/2, 1) straight down: one hit, (1/4, 1/2) at t = 1.
    The arrays an entry writes start from values it never writes; the ones a later entry reads hold what the earlier wrote."""
    a = dict(rows=np.array([[[0.0, 0.0], [1.0, 1.0]], [[0.0, 1.0], [0.0, 1.0]], [[0.0, 0.0], [0.0, 0.0]]]), first0=np.zeros(1, np.int32),
             first1=np.zeros(1, np.int32), breaks0=np.array([0.0, 1.0]), breaks1=np.array([0.0, 1.0]), cmax=np.array([1.0, 1.0, 0.0]),
             origins=np.array([[0.25], [0.5], [1.0]]), dirs=np.array([[0.0], [0.0], [-1.0]]), boxes=np.array([[0.0, 1.0, 0.0, 1.0, 0.0, 0.0]]),
             zero=np.zeros(1, np.int32), offset=np.zeros(1, np.int64), found=np.array([[[0.25, 0.5], [NAN, NAN]]]),
             found_near=np.zeros((1, 2), np.uint8), found_count=np.ones(1, np.int32), found_status=np.zeros(1, np.uint8),
             pstart=np.array([0, 1], np.int64), hit_off=np.array([0, 1], np.int64),
             out_boxes=np.full((1, 6), -1.0), partial=np.full(1, -1, np.int32), skipped=np.full(1, 255, np.uint8),
             pair_ray=np.full(1, -1, np.int32), pair_cell=np.full(1, -1, np.int32), roots=np.full((1, 2, 2), -1.0),
             near=np.full((1, 2), 255, np.uint8), count=np.full(1, -1, np.int32), status=np.full(1, 255, np.uint8),
             nodes=np.full(1, -1, np.int32), uv=np.full((2, 1), -1.0), t=np.full(1, -1.0), cell=np.full(1, -7, np.int32),
             hits=np.full(1, -1, np.int32), rstatus=np.full(1, 255, np.uint8))
    surface = dict(K0=2, K1=2, rows=ptr(a["rows"]), R0=2, R1=2, nc0=1, nc1=1, first0=ptr(a["first0"]), first1=ptr(a["first1"]))
    rays = dict(cmax=ptr(a["cmax"]), origins=ptr(a["origins"]), dirs=ptr(a["dirs"]), nrays=1)
    return a, surface, rays


def rays_checks(e):
    e.null("cmax", "origins", "dirs")
    for nrays in (0, 2 * 10 ** 9 + 1):
        e.rejects(INVALID, "nrays must be in [1, 2e9] (the driver walks the rays in passes)", nrays=nrays)


def search_checks(e, nc0):
    """The checks that the count and emit entries of bsk_rays_* and bsk_ssx_* share; ``nc0`` names the searched surface's."""
    e.rejects(INVALID, "chunk must be >= 1", chunk=0)
    e.rejects(INVALID, "more than 65535 chunks", **{nc0: 65536})
    if "npairs" in e.args:
        e.rejects(INVALID, "npairs must be >= 1 (no pairs: no call)", npairs=0)


@pytest.mark.parametrize("name,tail,device", twins("bsk_rays_boxes"))
def test_rays_boxes(name, tail, device):
    a, surface, _ = rays_arrays()
    e = Entry(name, tail, a, **surface, boxes=ptr(a["out_boxes"]))
    surface_checks(e)
    e.null("boxes")
    if not device:
        e.accepts(nv.lib().bsk_rays_last_kernel, "host ray_boxes")
        assert same(a["out_boxes"], a["boxes"])


@pytest.mark.parametrize("name,tail,device", twins("bsk_rays_count"))
def test_rays_count(name, tail, device):
    a, surface, rays = rays_arrays()
    e = Entry(name, tail, a, **surface, **rays, tmin=0.0, tmax=float("inf"), chunk=1, prefilter=1, boxes=ptr(a["boxes"]),
              partial=ptr(a["partial"]), skipped=ptr(a["skipped"]))
    surface_checks(e)
    rays_checks(e)
    e.null("boxes", "partial", "skipped")
    search_checks(e, "nc0")
    if not device:
        e.accepts(nv.lib().bsk_rays_last_kernel, "host ray_count")
        assert same(a["partial"], [1]) and same(a["skipped"], [0])
        e.accepts(nv.lib().bsk_rays_last_kernel, "host ray_count", prefilter=0)
        assert same(a["partial"], [1]) and same(a["skipped"], [0])


@pytest.mark.parametrize("name,tail,device", twins("bsk_rays_emit"))
def test_rays_emit(name, tail, device):
    a, surface, rays = rays_arrays()
    e = Entry(name, tail, a, **surface, **rays, tmin=0.0, tmax=float("inf"), chunk=1, prefilter=1, boxes=ptr(a["boxes"]),
              offset=ptr(a["offset"]), pair_ray=ptr(a["pair_ray"]), pair_cell=ptr(a["pair_cell"]), npairs=1)
    surface_checks(e)
    rays_checks(e)
    e.null("boxes", "offset", "pair_ray", "pair_cell")
    search_checks(e, "nc0")
    if not device:
        e.accepts(nv.lib().bsk_rays_last_kernel, "host ray_emit")
        assert same(a["pair_ray"], [0]) and same(a["pair_cell"], [0])


@pytest.mark.parametrize("name,tail,device", twins("bsk_rays_isolate"))
def test_rays_isolate(name, tail, device):
    a, surface, rays = rays_arrays()
    e = Entry(name, tail, a, **surface, breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]), **rays, pair_ray=ptr(a["zero"]),
              pair_cell=ptr(a["zero"]), npairs=1, roots=ptr(a["roots"]), near=ptr(a["near"]), count=ptr(a["count"]), status=ptr(a["status"]),
              nodes=ptr(a["nodes"]))
    surface_checks(e)
    rays_checks(e)
    e.null("breaks0", "breaks1", "pair_ray", "pair_cell", "roots", "near", "count", "status", "nodes")
    e.rejects(INVALID, "npairs must be >= 1 (no pairs: no call)", npairs=0)
    if not device:
        e.accepts(nv.lib().bsk_rays_last_kernel, "host ray_isolate")
        assert same(a["roots"], a["found"]) and same(a["near"], a["found_near"]) and same(a["count"], a["found_count"])
        assert same(a["status"], a["found_status"]) and same(a["nodes"], [283])        # the nodes that rays.statement visits


@pytest.mark.parametrize("name,tail,device", twins("bsk_rays_reduce"))
def test_rays_reduce(name, tail, device):
    a, surface, rays = rays_arrays()
    e = Entry(name, tail, a, **surface, breaks0=ptr(a["breaks0"]), breaks1=ptr(a["breaks1"]), **rays, tmin=0.0, tmax=float("inf"),
              pstart=ptr(a["pstart"]), pair_cell=ptr(a["zero"]), npairs=1, roots=ptr(a["found"]), near=ptr(a["found_near"]),
              count=ptr(a["found_count"]), pstatus=ptr(a["found_status"]), skipped=ptr(a["found_status"]), all=0, hit_off=None, nhits=0,
              uv=ptr(a["uv"]), t=ptr(a["t"]), cell=ptr(a["cell"]), hits=ptr(a["hits"]), status=ptr(a["rstatus"]))
    every = dict(all=1, hit_off=ptr(a["hit_off"]), nhits=1, hits=None, status=None)
    surface_checks(e)
    rays_checks(e)
    e.null("breaks0", "breaks1", "pstart", "pair_cell", "roots", "near", "count", "pstatus", "skipped", "uv", "t", "cell", "hits", "status")
    e.rejects(INVALID, NULL, **dict(every, hit_off=None))
    e.rejects(INVALID, "npairs must be >= 1 (no pairs: no call)", npairs=0)
    e.rejects(INVALID, "nhits must be >= 1 (no hits: no call)", **dict(every, nhits=0))
    if not device:
        e.accepts(nv.lib().bsk_rays_last_kernel, "host ray_reduce")
        assert same(a["uv"], [[0.25], [0.5]]) and same(a["t"], [1.0]) and same(a["cell"], [0]) and same(a["hits"], [1])
        assert same(a["rstatus"], [0])
        a["uv"][:], a["t"][:], a["cell"][:] = -1.0, -1.0, -7
        e.accepts(nv.lib().bsk_rays_last_kernel, "host ray_reduce all", **every)            # uv is (nhits, 2) here
        assert same(a["uv"].reshape(1, 2), [[0.25, 0.5]]) and same(a["t"], [1.0]) and same(a["cell"], [0])


# ------------------------------------------------------------------------------------------------------------ ssx
def ssx_arrays():
    """X = (u, v, 0) and Y = (s - 1/4, 1/4 + s / 2, t - 3/4) on unit squares, G = 1, the lines of X with u fixed: the line
    u = 0, segment 0, meets Y at (w, s, t) = (3/8, 1/4, 3/4); the line u = 1, segment 1, misses Y's box."""
    a = dict(rowsX=np.array([[[0.0, 0.0], [1.0, 1.0]], [[0.0, 1.0], [0.0, 1.0]], [[0.0, 0.0], [0.0, 0.0]]]),
             rowsY=np.array([[[-0.25, -0.25], [0.75, 0.75]], [[0.25, 0.25], [0.75, 0.75]], [[-0.75, 0.25], [-0.75, 0.25]]]),
             first=np.zeros(1, np.int32), breaks=np.array([0.0, 1.0]), boxes=np.array([[-0.25, 0.75, 0.25, 0.75, -0.75, 0.25]]),
             scale=np.array([1.75, 1.75, 0.75]), zero=np.zeros(1, np.int32), offset=np.array([0, 1], np.int64), key=np.zeros(1, np.int64),
             which=np.zeros(1, np.int64), found=np.full((1, 6, 3), NAN),
             partial=np.full((2, 1), -1, np.int32), pair_seg=np.full(1, -1, np.int32), pair_cell=np.full(1, -1, np.int32),
             roots=np.full((1, 6, 3), -1.0), near=np.full((1, 6), 255, np.uint8), count=np.full(1, -1, np.int32),
             status=np.full(1, 255, np.uint8), nodes=np.full(1, -1, np.int32), keep=np.full((1, 6), 7, np.uint8))
    a["found"][0, 0] = [0.375, 0.25, 0.75]
    side = {}
    for tag in "XY":
        side.update({"K0" + tag: 2, "K1" + tag: 2, "rows" + tag: ptr(a["rows" + tag]), "R0" + tag: 2, "R1" + tag: 2, "nc0" + tag: 1,
                     "nc1" + tag: 1, "first0" + tag: ptr(a["first"]), "first1" + tag: ptr(a["first"])})
    side.update(ax=0, G=1)
    return a, side


def side_checks(e):
    surface_checks(e, "X")
    surface_checks(e, "Y")
    for ax in (-1, 2):
        e.rejects(INVALID, "ax must be 0 or 1", ax=ax)
    for G in (0, 65):
        e.rejects(INVALID, "G must be in [1, 64]", G=G)
    e.rejects(INVALID, "more than 2e9 line segments", nc0X=40000, nc1X=40000, G=2)         # 1.6e9 cells, 3.2e9 segments


def ssx_search_checks(e):
    e.null("boxes", "scale")
    search_checks(e, "nc0Y")
    for change in (dict(seg0=-1), dict(nseg=0), dict(nseg=3), dict(seg0=2)):
        e.rejects(INVALID, "the segments seg0 .. seg0 + nseg - 1 must be segments of the family", **change)


@pytest.mark.parametrize("name,tail,device", twins("bsk_ssx_count"))
def test_ssx_count(name, tail, device):
    a, side = ssx_arrays()
    e = Entry(name, tail, a, **side, seg0=0, nseg=2, chunk=1, prefilter=1, boxes=ptr(a["boxes"]), scale=ptr(a["scale"]),
              partial=ptr(a["partial"]))
    side_checks(e)
    ssx_search_checks(e)
    e.null("partial")
    if not device:
        e.accepts(nv.lib().bsk_ssx_last_kernel, "host ssx_count")
        assert same(a["partial"], [[1], [0]])
        a["partial"][:] = -1
        e.accepts(nv.lib().bsk_ssx_last_kernel, "host ssx_count", prefilter=0)
        assert same(a["partial"], [[1], [0]])


@pytest.mark.parametrize("name,tail,device", twins("bsk_ssx_emit"))
def test_ssx_emit(name, tail, device):
    a, side = ssx_arrays()
    e = Entry(name, tail, a, **side, seg0=0, nseg=2, chunk=1, prefilter=1, boxes=ptr(a["boxes"]), scale=ptr(a["scale"]),
              offset=ptr(a["offset"]), pair_seg=ptr(a["pair_seg"]), pair_cell=ptr(a["pair_cell"]), npairs=1)
    side_checks(e)
    ssx_search_checks(e)
    e.null("offset", "pair_seg", "pair_cell")
    if not device:
        e.accepts(nv.lib().bsk_ssx_last_kernel, "host ssx_emit")
        assert same(a["pair_seg"], [0]) and same(a["pair_cell"], [0])


@pytest.mark.parametrize("name,tail,device", twins("bsk_ssx_isolate"))
def test_ssx_isolate(name, tail, device):
    a, side = ssx_arrays()
    e = Entry(name, tail, a, **side, breaks_run=ptr(a["breaks"]), breaksY0=ptr(a["breaks"]), breaksY1=ptr(a["breaks"]), scale=ptr(a["scale"]),
              pair_seg=ptr(a["zero"]), pair_cell=ptr(a["zero"]), npairs=1, roots=ptr(a["roots"]), near=ptr(a["near"]), count=ptr(a["count"]),
              status=ptr(a["status"]), nodes=ptr(a["nodes"]))
    side_checks(e)
    e.null("breaks_run", "breaksY0", "breaksY1", "scale", "pair_seg", "pair_cell", "roots", "near", "count", "status", "nodes")
    e.rejects(INVALID, "npairs must be >= 1 (no pairs: no call)", npairs=0)
    e.rejects(INVALID, "more pairs than one launch takes (2^31 - 1)", npairs=2 ** 31)      # on both twins
    if not device:
        e.accepts(nv.lib().bsk_ssx_last_kernel, "host ssx_isolate")
        assert same(a["roots"], a["found"]) and same(a["near"], np.zeros((1, 6))) and same(a["count"], [1]) and same(a["status"], [0])
        assert same(a["nodes"], [402])                                                 # the nodes that surfaces.statement_family visits


@pytest.mark.parametrize("name,tail,device", twins("bsk_ssx_merge"))
def test_ssx_merge(name, tail, device):
    a, _ = ssx_arrays()
    e = Entry(name, tail, a, R=6, roots=ptr(a["found"]), ncrun=1, ncY0=1, ncY1=1, breaks_run=ptr(a["breaks"]), breaksY0=ptr(a["breaks"]),
              breaksY1=ptr(a["breaks"]), pair_key=ptr(a["key"]), npairs=1, which=ptr(a["which"]), nnear=1, keep=ptr(a["keep"]))
    e.null("roots", "breaks_run", "breaksY0", "breaksY1", "pair_key", "which", "keep")
    for R in (5, 33):
        e.rejects(INVALID, "R must be min(6 (KR - 1)(K1 - 1)(K2 - 1), 32) of covered orders", R=R)
    for key in ("ncrun", "ncY0", "ncY1"):
        e.rejects(INVALID, "ncrun, ncy0 and ncy1 must be >= 1", **{key: 0})
    e.rejects(INVALID, LARGE, ncY0=3 * 10 ** 9)
    e.rejects(INVALID, "npairs must be >= 1", npairs=0)
    for nnear in (0, 7):
        e.rejects(INVALID, "nnear must be in [1, npairs R] (no zero near a face: no call)", nnear=nnear)
    if not device:
        e.accepts(nv.lib().bsk_ssx_last_kernel, "host ssx_merge")
        assert same(a["keep"], [[1, 7, 7, 7, 7, 7]])                                       # the lane of ``which`` alone writes
