"""
Sums of splines: ``common_basis``, ``add``, ``subtract``, ``translate``, the ``+`` and ``-`` operators, ``integrate`` and
``contract`` (reference bspy/spline.py:85-147, :149, :308, :567, :1290, :2199, :2335, bspy/_spline_operations.py:14, :184,
:290, :795 and bspy/_spline_domain.py:43).

``add`` is a change of basis followed by a sum.  The mapped variables of both splines are brought to one order and one
knot vector (``common_basis``: clamp, then one ``elevate_and_insert_knots`` per spline, the band operators of
refinement.py, exact to a few ulp), and the two coefficient tensors, which then agree in the mapped variables, are added
with the unmapped variables of each broadcast over the other's.  ``integrate`` is a weighted running sum of the
coefficients along one variable (``ScanMap``); ``contract`` is, per fixed variable, a band operator with one output row
that holds the B-spline values at the fixed parameter, followed by dropping that axis.

    device path   common_basis steps by ``bsk_band_apply`` with the intermediates on the device, then one ``sum_bcast``
                  launch (``bsk_sum_apply``); ``integrate``: ``bsk_scan_apply`` (scan_apply or scan_line, one launch, or
                  two when a line is cut into segments); ``contract``: the band kernels
    host path     the same sums on the CPU (``bsk_band_apply_host``, ``bsk_sum_apply_host``, ``bsk_scan_apply_host``), for
                  small results, operands of two dtypes and what the band kernels do not cover

The running sum has ONE association, whatever the path and the launch geometry (``ScanMap.apply_line`` states it in
NumPy): products g[i] * c[i] rounded to fp64; chunks of ``SCAN_CHUNK`` rows; left to right inside a chunk; chunk totals
left to right into the carry; output = carry + running sum of the chunk, rounded once.

``_path="device" | "host"`` (or ``sums.FORCE_PATH``) pins the path; ``sums.LAST_PATHS`` lists what the last call ran
("band_apply", "band_apply_line", "host band", "sum_bcast", "host sum", "scan_apply", "scan_line", "host scan").
"""
import ctypes

import numpy as np

from . import _native as nv
from . import refinement
from ._backend import FLOATS, Device, Handle, Host, choose, is_torch as _is_torch, lines, pick_path

# Elements of the result from which the device path is taken.  AN ESTIMATE, not a measurement: refinement's threshold
#  carried over; tools/sum_time.py prints the host / device crossover table that is to replace it.
DEVICE_MIN_ELEMENTS = 1 << 16
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []
SCAN_CHUNK = 32            # rows per chunk of the running sum's association (bsk_sum.hpp)
SUM_MAX_RANK = 8
RANK_UNCOVERED = f"the device path covers a rank of at most {SUM_MAX_RANK} after merging"


# ------------------------------------------------------------------------------------------ the running sum
class ScanMap(Handle):
    """out[0] = 0, out[j + 1] = sum_{i <= j} g[i] * in[i] (``bsk_scan`` handle).  g: (n,) float64."""
    prefix = "bsk_scan"

    def __init__(self, g):
        self.g = np.ascontiguousarray(g, np.float64)
        self.n = len(self.g)
        self._open(self.n, self.g.ctypes.data)

    def apply_line(self, x):
        """One line in NumPy, the statement of what the library computes on every path: fp64 products, each rounded;
        chunks of SCAN_CHUNK rows; inside a chunk the products are added left to right from 0.0; the chunk totals are
        added left to right from 0.0 into the chunk's carry; an output is carry + running sum, rounded once."""
        x = np.asarray(x)
        p = self.g * x.astype(np.float64)
        out = np.zeros(self.n + 1, np.float64)
        carry = np.float64(0.0)
        for r0 in range(0, self.n, SCAN_CHUNK):
            local = np.float64(0.0)
            for r in range(r0, min(self.n, r0 + SCAN_CHUNK)):
                local = local + p[r]
                out[r + 1] = carry + local
            carry = carry + local
        return out.astype(x.dtype)

    def apply(self, be, a, outer, inner, segments=0):
        """The launch: a, the entered backend's contiguous float32 / float64 array of outer * n * inner values ->
        (outer, n + 1, inner), same type.  segments: pieces the kernels cut a line into (0: the library chooses)."""
        code = be.code(a)
        out = be.empty((outer, self.n + 1, inner), FLOATS[code])
        cut = (int(segments),) if isinstance(be, Device) else ()            # the host entry point has no such argument
        be.call("bsk_scan_apply", self._handle, code, be.ptr(a), outer, inner, be.ptr(out), *cut)
        return out

    def apply_host(self, a, outer, inner):
        """a: NumPy float32 / float64 of outer * n * inner values -> (outer, n + 1, inner), same dtype."""
        return self.apply(Host(), np.ascontiguousarray(a), outer, inner)

    def apply_device(self, a, outer, inner, segments=0):
        """a: contiguous torch CUDA tensor of outer * n * inner float32 / float64 -> (outer, n + 1, inner), same dtype."""
        with Device(a.device) as be:
            return self.apply(be, a, outer, inner, segments)


def integral_weights(knots, order):
    """g[i] = (t[i + k] - t[i]) / k in the knots' own precision, as the reference forms it."""
    k = int(order)
    return (knots[k:] - knots[:len(knots) - k]) / k


def scan(scan_map, tensor, axis, _segments=None):
    """The running sum ``scan_map`` along ``axis`` of a torch CUDA tensor (float32 / float64); returns a new CUDA tensor
    whose extent along ``axis`` is n + 1.  For pipelines that stay on the device.  ``LAST_PATHS`` holds this call's
    kernel."""
    import torch
    if not (_is_torch(tensor) and tensor.is_cuda):
        raise TypeError("sums.scan takes a torch CUDA tensor")
    if tensor.dtype not in (torch.float32, torch.float64):
        raise TypeError("sums.scan takes float32 or float64")
    axis = axis % tensor.dim()
    shape = list(tensor.shape)
    outer, inner = lines(shape, axis, scan_map.n)
    shape[axis] += 1
    if outer * inner == 0:
        LAST_PATHS[:] = []
        return torch.empty(shape, dtype=tensor.dtype, device=tensor.device)
    out = scan_map.apply_device(tensor.contiguous(), outer, inner, _segments or 0).reshape(shape)
    LAST_PATHS[:] = [scan_map.last_kernel()]
    return out


def integrate(self, with_respect_to=0, _path=None, _segments=None):
    del LAST_PATHS[:]
    path = pick_path(_path, FORCE_PATH)
    if not (0 <= with_respect_to < self.nInd):
        raise ValueError("Invalid with_respect_to")
    iv = with_respect_to
    t, k = self.knots[iv], self.order[iv]
    order, knots = list(self.order), list(self.knots)
    order[iv] = k + 1
    knots[iv] = np.concatenate((t[:1], t, t[-1:]))
    shape = list(self.coefs.shape)
    outer, inner = lines(shape, iv + 1, shape[iv + 1])
    shape[iv + 1] += 1
    if outer * inner == 0:
        return type(self)(self.nInd, self.nDep, order, shape[1:], knots, np.empty(shape, self.coefs.dtype), self.metadata)
    path = choose(path, True, outer * inner * shape[iv + 1] >= DEVICE_MIN_ELEMENTS, None)
    be = Device.current() if path == "device" else Host()
    with ScanMap(integral_weights(t, k)) as scan_map, be:
        coefs = be.get(scan_map.apply(be, be.put(self.coefs, self.coefs.dtype), outer, inner, _segments or 0)).reshape(shape)
        LAST_PATHS.append(scan_map.last_kernel())
    return type(self)(self.nInd, self.nDep, order, shape[1:], knots, coefs, self.metadata)


# ------------------------------------------------------------------------------------------ the broadcast sum
def _strides(a):
    return [int(s) for s in a.stride()] if _is_torch(a) else [int(s) // a.itemsize for s in a.strides]


def sum_layout(a, b):
    """a, b: arrays or tensors of one rank whose extents agree or are 1.  Returns (shape of the sum, dim, strideA,
    strideB): the extents and the strides in elements after extents of 1 are dropped and adjacent axes that both
    operands walk as one are merged; a stride of 0 broadcasts."""
    if a.ndim != b.ndim:
        raise ValueError("the operands must have the same rank")
    shape, axes = [], []
    for da, db, sa, sb in zip(a.shape, b.shape, _strides(a), _strides(b)):
        if da != db and 1 not in (da, db):
            raise ValueError(f"extents {da} and {db} do not broadcast")
        d = db if da == 1 else da
        shape.append(int(d))
        if d != 1:
            axes.append([int(d), sa if da != 1 else 0, sb if db != 1 else 0])
    merged = []
    for d, sa, sb in axes:
        if merged and merged[-1][1] == d * sa and merged[-1][2] == d * sb:
            merged[-1] = [merged[-1][0] * d, sa, sb]
        else:
            merged.append([d, sa, sb])
    if not merged:
        merged = [[1, 0, 0]]
    dim, sa, sb = (list(v) for v in zip(*merged))
    return shape, dim, sa, sb


def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def _add(be, a, b, sign):
    """a + sign * b, the entered backend's arrays of one float type and one rank, any non-negative strides -> the
    backend's contiguous array.  One launch; above ``SUM_MAX_RANK`` the host peels the leading axis in Python."""
    shape, dim, sa, sb = sum_layout(a, b)
    if len(dim) > SUM_MAX_RANK and isinstance(be, Device):
        raise ValueError(RANK_UNCOVERED)
    out = be.empty(shape, FLOATS[be.code(a)])
    if 0 in shape:
        return out
    if len(dim) > SUM_MAX_RANK:                       # more axes than one call takes: the leading axis in Python
        at = next(i for i, d in enumerate(shape) if d != 1)
        for i in range(shape[at]):
            take = lambda x: x if x.shape[at] == 1 else np.take(x, [i], axis=at)
            index = (slice(None),) * at + (slice(i, i + 1),)
            out[index] = _add(be, take(a), take(b), sign)
        return out
    be.call("bsk_sum_apply", be.code(a), len(dim), _i64(dim), be.ptr(a), _i64(sa), be.ptr(b), _i64(sb), int(sign), be.ptr(out))
    return out


def add_tensors(a, b, sign=1):
    """a + sign * b for torch CUDA tensors of one type (float32 / float64) and one rank whose extents agree or are 1
    (broadcast); any non-negative strides (views made by permute and expand need no copy).  One ``sum_bcast`` launch;
    returns a new contiguous CUDA tensor.  For pipelines that stay on the device.  ``LAST_PATHS`` holds the kernel."""
    import torch
    if not (_is_torch(a) and _is_torch(b) and a.is_cuda and b.is_cuda):
        raise TypeError("sums.add_tensors takes torch CUDA tensors")
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.float64):
        raise TypeError("sums.add_tensors takes two float32 or two float64 tensors")
    if sign not in (1, -1):
        raise ValueError("sign must be 1 or -1")
    with Device(a.device) as be:
        out = _add(be, a, b, sign)
    LAST_PATHS[:] = [nv.lib().bsk_sum_last_kernel().decode()] if out.numel() else []
    return out


def _add_host(a, b, sign):
    """NumPy arrays of one float type, any non-negative strides."""
    return _add(Host(), a, b, sign)


def _placed(x, sources):
    """View of x (component axis, then its variables) with, behind the component axis, one axis per entry of
    ``sources``: x's variable of that number, or an axis of extent 1 for None.  NumPy arrays and torch tensors."""
    perm = [0] + [1 + s for s in sources if s is not None]
    y = x.permute(perm) if _is_torch(x) else np.transpose(x, perm)
    return y[(slice(None),) + tuple(slice(None) if s is not None else None for s in sources)]


# ------------------------------------------------------------------------------------------ common basis
def _basis_plans(splines, indMap):
    """What ``common_basis`` does to every spline, from orders and knots alone: [(orders, knots, [band steps per
    stage])], in the reference's order of checks."""
    if indMap is None:
        indMap = [len(splines) * [iv] for iv in range(splines[0].nInd)]
    state = []
    for s in splines:
        every = tuple(range(s.nInd))
        plan = refinement.trim_plan(s.order, s.knots, refinement.clamp_box(s.order, s.knots, every, every)) if s.nInd else None
        knots, steps = plan if plan is not None else (list(s.knots), [])
        state.append([list(s.order), list(knots), [steps] if steps else []])

    def domain_knots(at, ind):
        order, knots = state[at][0][ind], state[at][1][ind]
        return order, knots[order - 1:len(knots) - order + 1]

    # per aligned variable: the largest order, and per distinct knot the largest multiplicity once every spline is elevated
    orders = []
    for mapping in indMap:
        if len(mapping) != len(splines):
            raise ValueError("Invalid map")
        orders.append(max(state[at][0][ind] for at, ind in enumerate(mapping)))
    merged = []
    for mapping, order in zip(indMap, orders):
        _, first = domain_knots(0, mapping[0])
        multiplicity = {}                                           # value -> [the knot as first met, multiplicity]
        for at, ind in enumerate(mapping):
            k, piece = domain_knots(at, ind)
            if not (piece[0] == first[0]) or not (piece[-1] == first[-1]):
                raise ValueError("Spline domains don't match")
            for knot, count in zip(*np.unique(piece, return_counts=True)):
                entry = multiplicity.setdefault(float(knot), [knot, 0])
                entry[1] = max(entry[1], int(count) + order - k)
        merged.append(multiplicity)

    for at, (order, knots, stages) in enumerate(state):
        m = len(order) * [0]
        new = [[] for _ in order]
        for mapping, common, multiplicity in zip(indMap, orders, merged):
            ind = mapping[at]
            k, piece = domain_knots(at, ind)
            m[ind] = common - k
            own = dict(zip((float(v) for v in np.unique(piece)), np.unique(piece, return_counts=True)[1]))
            for value in sorted(multiplicity):
                knot, times = multiplicity[value]
                new[ind] += (times - int(own.get(value, 0))) * [knot]
        plan = refinement.elevate_plan(order, knots, m, new)
        if plan is not None:
            state[at][0], state[at][1], clamp_steps, steps = plan
            stages += [stage for stage in (clamp_steps, steps) if stage]
    return [tuple(entry) for entry in state]


def _run_stages(coefs, stages, path):
    """NumPy -> NumPy through refinement's own dispatch, stage by stage; returns (coefs, what ran)."""
    ran = []
    for steps in stages:
        coefs = refinement._run(coefs, steps, path)
        ran += refinement.LAST_PATHS
    return coefs, ran


def _staged(be, coefs, stages):
    """NumPy coefs through the stages on the entered backend (``refinement.run_steps``); returns the backend's array.  The host
    keeps an array that no stage touches as it is, strides and all: the sum takes any strides."""
    if not stages and isinstance(be, Host):
        return coefs
    data = be.put(coefs, coefs.dtype)
    for steps in stages:
        data = refinement.run_steps(be, data, steps, LAST_PATHS)
    return data


def _rebuilt(s, order, knots, coefs):
    return type(s)(s.nInd, s.nDep, order, coefs.shape[1:], knots, coefs, s.metadata)


def common_basis(splines, indMap=None, _path=None):
    del LAST_PATHS[:]
    path = pick_path(_path, FORCE_PATH)
    splines = tuple(splines)
    out = []
    for s, (order, knots, stages) in zip(splines, _basis_plans(splines, indMap)):
        if not stages:
            out.append(s)                              # clamped, of the common order, with every common knot: itself
            continue
        coefs, ran = _run_stages(s.coefs, stages, path)
        LAST_PATHS.extend(ran)
        out.append(_rebuilt(s, order, knots, coefs))
    return tuple(out)


# ------------------------------------------------------------------------------------------ add, subtract, translate
def add(self, other, indMap=None, _path=None, _sign=1):
    del LAST_PATHS[:]
    path = pick_path(_path, FORCE_PATH)
    if not (self.nDep == other.nDep):
        raise ValueError("self and other must have same nDep")
    if indMap is None:
        pairs = []                                     # the outer sum: nothing is aligned, nothing is clamped
        plans = [(list(s.order), list(s.knots), []) for s in (self, other)]
    else:
        pairs = [(m, m) if np.isscalar(m) else m for m in indMap]
        plans = _basis_plans((self, other), pairs)
    (order1, knots1, stages1), (order2, knots2, stages2) = plans
    target = {p[1]: p[0] for p in pairs}
    free2 = [iv for iv in range(other.nInd) if iv not in target]
    order = [*order1] + [order2[iv] for iv in free2]
    knots = [*knots1] + [knots2[iv] for iv in free2]
    nCoef = [len(t) - k for t, k in zip(knots, order)]
    shape2 = [len(t) - k for t, k in zip(knots2, order2)]
    for iv, at in target.items():
        if shape2[iv] != nCoef[at]:
            raise ValueError("Invalid map")
    # where other's variables stand in the result: self's variables in place, then other's unmapped ones
    source = [None] * len(order)
    for iv in range(other.nInd):
        source[target[iv] if iv in target else self.nInd + free2.index(iv)] = iv
    own = list(range(self.nInd)) + [None] * len(free2)

    dtype = self.coefs.dtype
    one_type = other.coefs.dtype == dtype
    steps = [s for stage in stages1 + stages2 for s in stage]
    size = self.nDep * int(np.prod(nCoef, dtype=np.int64))
    if size == 0:
        return type(self)(len(order), self.nDep, order, nCoef, knots, np.empty((self.nDep, *nCoef), dtype), self.metadata)
    rank = len(sum_layout(_placed(np.empty((self.nDep, *nCoef[:self.nInd]), np.int8), own),
                          _placed(np.empty((other.nDep, *shape2), np.int8), source))[1])
    why = ("the device path takes two splines of one coefficient dtype" if not one_type else
           refinement.UNCOVERED if not refinement.steps_covered(steps) else RANK_UNCOVERED)
    path = choose(path, one_type and refinement.steps_covered(steps) and rank <= SUM_MAX_RANK, size >= DEVICE_MIN_ELEMENTS, why)
    with (Device.current() if path == "device" else Host()) as be:
        a, b = _staged(be, self.coefs, stages1), _staged(be, other.coefs, stages2)
        if not one_type:                                    # host only: summed in float64, rounded to self's
            common = np.result_type(a.dtype, b.dtype)
            a, b = a.astype(common, copy=False), b.astype(common, copy=False)
        coefs = be.get(_add(be, _placed(a, own), _placed(b, source), _sign)).astype(dtype, copy=False)
    LAST_PATHS.append(nv.lib().bsk_sum_last_kernel().decode())
    return type(self)(len(order), self.nDep, order, nCoef, knots, coefs, self.metadata)


def subtract(self, other, indMap=None, _path=None):
    return add(self, other, indMap, _path, -1)


def translate(self, translationVector):
    vector = np.atleast_1d(translationVector)
    if not (len(vector) == self.nDep):
        raise ValueError("Invalid translationVector")
    coefs = np.array(self.coefs)
    for i in range(self.nDep):
        coefs[i] += vector[i]
    return type(self)(self.nInd, self.nDep, self.order, self.nCoef, self.knots, coefs, self.metadata)


# ------------------------------------------------------------------------------------------ contract
def basis_row(knots, order, u):
    """(first, w) of the band operator with one output row that evaluates in one variable: w (1, order) are the B-spline
    values at u (the value ``bspline_values`` returns, here from the de Boor recurrence of refinement.py with every
    argument equal to u, in extended precision where the platform has it, rounded once) and first = ix - order, ix the
    reference's knot index: the cell to the right of an interior knot, the last cell at the right end of the domain."""
    k = int(order)
    u = knots.dtype.type(u)
    t = np.asarray(knots, np.float64)
    first = refinement.knot_cell(t, k, np.array([np.float64(u)])) - k + 1
    args = np.full((1, k - 1), u, np.longdouble)
    w = refinement.blossom_weights(t.astype(np.longdouble), k, first, args)
    return first.astype(np.int32), w.astype(np.float64)


def contract(self, uvw, _path=None):
    del LAST_PATHS[:]
    pick_path(_path, FORCE_PATH)
    domain = self.domain()
    steps, fixed, dtype = [], [], self.coefs.dtype
    for iv in range(self.nInd):
        if uvw[iv] is None:
            continue
        if uvw[iv] < domain[iv][0] or uvw[iv] > domain[iv][1]:
            raise ValueError(f"Spline evaluation outside domain: {uvw}")
        first, values = basis_row(self.knots[iv], self.order[iv], uvw[iv])
        dtype = np.result_type(dtype, self.knots[iv].dtype)          # the reference multiplies by values of the knots' type
        steps.append((iv + 1, first, values))
        fixed.append(iv)
    if not fixed:
        return self
    kept = [iv for iv in range(self.nInd) if iv not in fixed]
    coefs = refinement._run(self.coefs.astype(dtype, copy=False), steps, _path)
    LAST_PATHS.extend(refinement.LAST_PATHS)
    nCoef = [self.nCoef[iv] for iv in kept]
    return type(self)(len(kept), self.nDep, [self.order[iv] for iv in kept], nCoef, [self.knots[iv] for iv in kept],
                      np.ascontiguousarray(coefs).reshape((self.nDep, *nCoef)), self.metadata)
