"""
Products of splines: ``multiply`` (scalar, dot and cross products of the dependent variables), ``dot``, ``cross``,
``scale``, ``transform`` and the ``*``, ``@``, unary ``-`` and ``/`` operators (reference bspy/spline.py:97-147, :1585 and
bspy/_spline_operations.py:225, :268, :318, :767, :788).

For one pair of mapped variables (variable ind1 of self: order k1, knots t; variable ind2 of other: order k2, knots s)
the product is a spline of order p = k1 + k2 - 1 on the knots tbar (``product_knots``: the reference's rule, bit for
bit), and its coefficients are a small banded BILINEAR operator on the two coefficient lines, the same for every line:

    c[j] = sum_{a < k1} sum_{b < k2} W[j, a, b] * A[f[j] + a] * B[g[j] + b]                     (``product_map``)

Coefficient j is the blossom of the polynomial piece of the product on one cell inside the support of basis function j
at tbar[j + 1 .. j + p - 1]; the blossom of a product of polynomials of degrees k1 - 1 and k2 - 1 is the mean, over the
(k1 - 1)-subsets S of its arguments, of the first factor's blossom at S times the second factor's at the complement, and
each factor's blossom is the multi-affine de Boor recurrence of refinement.py on its own cell.  Every W[j] sums to one and
has no negative entry: a product coefficient is a convex combination of products A[i] * B[l].  Several mapped variables:
the tensor product of the per-variable operators.  Nothing of the size of the outer product of the two coefficient
tensors is ever formed (the reference forms it over all variables, mapped ones included).

    device path   ``bsk_product_apply``: band_product_line (one mapped variable) or band_product_tile (two), one launch
                  for the whole result
    host path     ``bsk_product_apply_host``: the same sums on the CPU, for small results, three mapped variables and
                  orders outside 2 .. 6
    no mapped variable: a plain outer product in NumPy, no kernel

``_path="device" | "host"`` (or ``product.FORCE_PATH``) pins the path; ``product.LAST_PATHS`` lists what the last call
ran ("band_product_line", "band_product_tile", "host product", "outer").
"""
import ctypes
import math

import numpy as np

from . import _native as nv
from ._backend import FLOATS, Device, Handle, Host, choose, is_torch as _is_torch, pick_path
from .refinement import knot_cell, support_cell

# Elements of the result from which the device path is taken.  AN ESTIMATE, not a measurement: refinement's threshold
# carried over.  tools/product_time.py prints the host / device crossover table that is to replace it; the first table
#  puts the crossover of a surface dot product near 500 elements.
DEVICE_MIN_ELEMENTS = 1 << 16
DEVICE_MIN_K, DEVICE_MAX_K = 2, 6
DEVICE_MAX_M, HOST_MAX_M = 2, 3
UNCOVERED = f"the device path covers one or two mapped variables of orders {DEVICE_MIN_K} to {DEVICE_MAX_K}"
FORCE_PATH = None          # None, "device" or "host"
LAST_PATHS = []


# ------------------------------------------------------------------------------------------ the operator
def product_knots(knots1, order1, knots2, order2, ind1=0, ind2=0):
    """Knots of the product in one mapped variable (the reference's rule): the distinct knots of both domains, an
    interior one with multiplicity m1 + k2 - 1, m2 + k1 - 1 or the larger of both where the operands share it, the ends
    with multiplicity k1 + k2 - 1.  Always clamped; dtype of knots1."""
    k1, k2 = int(order1), int(order2)
    d1, m1 = np.unique(knots1[k1 - 1:len(knots1) - k1 + 1], return_counts=True)
    d2, m2 = np.unique(knots2[k2 - 1:len(knots2) - k2 + 1], return_counts=True)
    if not (d1[0] == d2[0] and d1[-1] == d2[-1]):
        raise ValueError(f"self[{ind1}] domain doesn't match other[{ind2}]")
    values = np.union1d(d1, d2)
    mult = np.zeros(len(values), np.int64)
    at1, at2 = np.searchsorted(values, d1), np.searchsorted(values, d2)
    mult[at1] = m1 + k2 - 1
    mult[at2] = np.maximum(mult[at2], m2 + k1 - 1)
    mult[0] = mult[-1] = k1 + k2 - 1
    return np.repeat(values, mult).astype(knots1.dtype)


def product_map(knots1, order1, knots2, order2, newKnots):
    """(f, g, W) of one mapped variable: W (nOut, k1, k2) float64, f and g (nOut,) int32, nOut = len(newKnots) - p.
    The cell is refine_map's choice: the non-empty new cell nearest the middle of the support, the lower of two."""
    t, s, tb = (np.asarray(a, np.float64) for a in (knots1, knots2, newKnots))
    k1, k2 = int(order1), int(order2)
    n = k1 + k2 - 2                                 # arguments of the product's blossom
    nOut = len(tb) - n - 1
    j = np.arange(nOut)
    cell = support_cell(tb, j, n)
    x = 0.5 * (tb[cell] + tb[cell + 1])
    f = knot_cell(t, k1, np.clip(x, t[k1 - 1], t[len(t) - k1])) - k1 + 1
    g = knot_cell(s, k2, np.clip(x, s[k2 - 1], s[len(s) - k2])) - k2 + 1

    # extended precision where the platform has it, rounded once to double (as refine_map)
    t, s, tb = t.astype(np.longdouble), s.astype(np.longdouble), tb.astype(np.longdouble)
    # The sum over the C(n, k1 - 1) subsets collapses: E[i, l] is the sum, over all ways to hand i of the first i + l
    # arguments to the first factor, of (weights of factor 1) x (weights of factor 2), each factor's recurrence run from
    # its top level downwards (_descend), so a factor's state after i arguments is a vector of i + 1 weights and the next
    # argument, whichever it is, takes the next level: the blossom is symmetric in its arguments.
    E = {(0, 0): np.ones((nOut, 1, 1), np.longdouble)}
    for m in range(n):
        u = tb[j + 1 + m]
        nxt = {}
        for (i, l), e in E.items():
            if i < k1 - 1:
                step = np.moveaxis(_descend(t, k1, f, i, u, np.moveaxis(e, 1, -1)), -1, 1)
                nxt[i + 1, l] = nxt[i + 1, l] + step if (i + 1, l) in nxt else step
            if l < k2 - 1:
                step = _descend(s, k2, g, l, u, e)
                nxt[i, l + 1] = nxt[i, l + 1] + step if (i, l + 1) in nxt else step
        E = nxt
    W = E[k1 - 1, k2 - 1] / math.comb(n, k1 - 1)
    return f.astype(np.int32), g.astype(np.int32), W.astype(np.float64)


def _descend(knots, order, first, done, u, state):
    """One level of the de Boor recurrence, read from the top: ``state`` (rows, ..., done + 1) holds weights on the
    level-r values d_p^r, p = r .. k - 1, r = k - 1 - done; since d_p^r = (1 - a_p) d_{p-1}^{r-1} + a_p d_p^{r-1} with
    a_p = (u - t[first + p]) / (t[first + p + k - r] - t[first + p]), the weights on level r - 1 (one entry more) follow."""
    k = order
    r = k - 1 - done
    p = np.arange(r, k)
    left, right = knots[first[:, None] + p], knots[first[:, None] + p + k - r]
    a = (u[:, None] - left) / (right - left)                                  # (rows, done + 1)
    a = a.reshape((a.shape[0],) + (1,) * (state.ndim - 2) + (a.shape[1],))
    out = np.zeros(state.shape[:-1] + (done + 2,), state.dtype)
    out[..., 1:] += a * state
    out[..., :-1] += (1 - a) * state
    return out


class ProductMap(Handle):
    """The operators of M >= 1 mapped variables (``bsk_product`` handle).  variables: [(f, g, W, nIn1, nIn2)]."""
    prefix = "bsk_product"

    def __init__(self, variables):
        self.M = len(variables)
        self.f = [np.ascontiguousarray(v[0], np.int32) for v in variables]
        self.g = [np.ascontiguousarray(v[1], np.int32) for v in variables]
        self.W = [np.ascontiguousarray(v[2], np.float64) for v in variables]
        self.nIn1 = [int(v[3]) for v in variables]
        self.nIn2 = [int(v[4]) for v in variables]
        self.nOut = [w.shape[0] for w in self.W]
        self.k1 = [w.shape[1] for w in self.W]
        self.k2 = [w.shape[2] for w in self.W]
        i32 = lambda values: (ctypes.c_int32 * self.M)(*values)
        i32p = ctypes.POINTER(ctypes.c_int32)
        self._open(self.M, i32(self.nIn1), i32(self.nIn2), i32(self.nOut), i32(self.k1), i32(self.k2),
                   (i32p * self.M)(*[a.ctypes.data_as(i32p) for a in self.f]), (i32p * self.M)(*[a.ctypes.data_as(i32p) for a in self.g]),
                   nv.ptr_array([w.ctypes.data for w in self.W]))

    @classmethod
    def from_knots(cls, pairs):
        """pairs: [(knots1, order1, knots2, order2)] -> (ProductMap, [knots of the product])."""
        variables, knots = [], []
        for knots1, k1, knots2, k2 in pairs:
            tbar = product_knots(knots1, k1, knots2, k2)
            knots.append(tbar)
            variables.append((*product_map(knots1, k1, knots2, k2, tbar), len(knots1) - k1, len(knots2) - k2))
        return cls(variables), knots

    def covered(self):
        """Whether the device path has kernels for this map."""
        return self.M <= DEVICE_MAX_M and all(DEVICE_MIN_K <= k <= DEVICE_MAX_K for k in self.k1 + self.k2)

    def apply_line(self, a, b):
        """One line of one mapped variable in NumPy, the statement of what the library computes in the last variable:
        V[b] = sum_a A[a] W[a][b] in the order of a, then sum_b V[b] B[b] in the order of b, fp64, rounded once."""
        assert self.M == 1
        a, b = np.asarray(a), np.asarray(b)
        V = np.zeros((self.nOut[0], self.k2[0]), np.float64)
        for i in range(self.k1[0]):
            V += a[self.f[0] + i].astype(np.float64)[:, None] * self.W[0][:, i, :]
        acc = np.zeros(self.nOut[0], np.float64)
        for l in range(self.k2[0]):
            acc += V[:, l] * b[self.g[0] + l].astype(np.float64)
        return acc.astype(a.dtype)

    def apply(self, be, a, b, terms):
        """The launch: a (PA, *nIn1) and b (PB, *nIn2), the entered backend's contiguous arrays of one float32 / float64
        type; terms (P, T, 3): NumPy plane table -> (P, *nOut) of that type."""
        if tuple(a.shape[1:]) != tuple(self.nIn1) or tuple(b.shape[1:]) != tuple(self.nIn2):
            raise ValueError(f"the map takes a of shape (PA, {self.nIn1}) and b of shape (PB, {self.nIn2})")
        terms = np.ascontiguousarray(terms, np.int32)
        if terms.ndim != 3 or terms.shape[2] != 3 or terms.size == 0:
            raise ValueError("terms must have shape (P, T, 3) with P, T >= 1")
        code = be.code(a)
        out = be.empty((terms.shape[0], *self.nOut), FLOATS[code])
        be.call("bsk_product_apply", self._handle, code, be.ptr(a), a.shape[0], be.ptr(b), b.shape[0],
                terms.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), terms.shape[0], terms.shape[1], be.ptr(out))
        return out

    def apply_host(self, a, b, terms):
        """a: NumPy (PA, *nIn1), b: (PB, *nIn2), the same float32 / float64 type; terms (P, T, 3) -> (P, *nOut)."""
        return self.apply(Host(), np.ascontiguousarray(a), np.ascontiguousarray(b), terms)

    def apply_device(self, a, b, terms):
        """a, b: contiguous torch CUDA tensors of one float type -> CUDA tensor (P, *nOut) of that type."""
        with Device(a.device) as be:
            return self.apply(be, a, b, terms)


# ------------------------------------------------------------------------------------------ the plane table
def dependent_terms(productType, nDep1, nDep2):
    """Per dependent variable of the result its terms [(component of self, component of other, sign)]: scalar product
    with broadcast of a one-component operand, dot product, cross product in 3-D (three components) and 2-D (one)."""
    if productType == "D":
        return [[(d, d, 1) for d in range(nDep1)]]
    if productType == "C":
        if nDep1 == 3:
            return [[(1, 2, 1), (2, 1, -1)], [(2, 0, 1), (0, 2, -1)], [(0, 1, 1), (1, 0, -1)]]
        return [[(0, 1, 1), (1, 0, -1)]]
    return [[(d if nDep1 > 1 else 0, d if nDep2 > 1 else 0, 1)] for d in range(max(nDep1, nDep2))]


def plane_table(dep_terms, UA=1, UB=1):
    """terms (P, T, 3) int32 for operands stored as a[(component, ua)] and b[(component, ub)], ua < UA and ub < UB the
    flat unmapped variables: output plane ((d * UA) + ua) * UB + ub."""
    dep = np.array(dep_terms, np.int64)                               # (D, T, 3)
    D, T, _ = dep.shape
    ua = np.arange(UA, dtype=np.int64)[None, :, None, None]
    ub = np.arange(UB, dtype=np.int64)[None, None, :, None]
    terms = np.empty((D, UA, UB, T, 3), np.int64)
    terms[..., 0] = dep[:, None, None, :, 0] * UA + ua
    terms[..., 1] = dep[:, None, None, :, 1] * UB + ub
    terms[..., 2] = dep[:, None, None, :, 2]
    if terms.max() > np.iinfo(np.int32).max:
        raise ValueError("too many planes for one call")
    return terms.reshape(D * UA * UB, T, 3).astype(np.int32)


# ------------------------------------------------------------------------------------------ application
def apply(maps, a, b, terms):
    """The product operator ``maps`` (a ProductMap) on torch CUDA tensors a (PA, *nIn1) and b (PB, *nIn2) of one type
    (float32 / float64), mapped variables last; ``terms`` (P, T, 3): NumPy plane table.  Returns a new CUDA tensor
    (P, *nOut).  For pipelines that stay on the device.  ``LAST_PATHS`` holds this call's kernel."""
    import torch
    if not (_is_torch(a) and _is_torch(b) and a.is_cuda and b.is_cuda):
        raise TypeError("product.apply takes torch CUDA tensors")
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.float64):
        raise TypeError("product.apply takes two float32 or two float64 tensors")
    if not maps.covered():
        raise ValueError(UNCOVERED)
    out = maps.apply_device(a.contiguous(), b.contiguous(), terms)
    LAST_PATHS[:] = [maps.last_kernel()]
    return out


def _run(maps, a, b, terms, path):
    """a, b: NumPy in the canonical layout, one dtype.  Returns NumPy (P, *nOut)."""
    size = terms.shape[0] * int(np.prod(maps.nOut, dtype=np.int64))
    path = choose(path if path is not None else FORCE_PATH, maps.covered(), size >= DEVICE_MIN_ELEMENTS, UNCOVERED)
    with (Device.current() if path == "device" else Host()) as be:
        out = be.get(maps.apply(be, be.put(a, a.dtype), be.put(b, b.dtype), terms))
    LAST_PATHS.append(maps.last_kernel())
    return out


def _canonical(coefs, mapped):
    """(nDep, *nCoef) -> contiguous (nDep * unmapped, *mapped extents), and the unmapped extents."""
    moved = np.moveaxis(coefs, [m + 1 for m in mapped], range(coefs.ndim - len(mapped), coefs.ndim))
    rest = moved.shape[1:coefs.ndim - len(mapped)]
    tail = moved.shape[coefs.ndim - len(mapped):]
    return np.ascontiguousarray(moved).reshape((coefs.shape[0] * int(np.prod(rest, dtype=np.int64)), *tail)), rest


def multiply(self, other, indMap=None, productType="S", _path=None):
    del LAST_PATHS[:]
    pick_path(_path, None)
    if productType not in ("C", "D", "S"):
        raise ValueError("productType must be 'C', 'D' or 'S'")
    if productType == "D" and self.nDep != other.nDep:
        raise ValueError("Mismatched dimensions")
    if productType == "C" and not (self.nDep == other.nDep and 2 <= self.nDep <= 3):
        raise ValueError("Mismatched dimensions")
    if productType == "S" and not (self.nDep == 1 or other.nDep == 1 or self.nDep == other.nDep):
        raise ValueError("Mismatched dimensions")

    pairs = [] if indMap is None else [(m, m) if np.isscalar(m) else (m[0], m[1]) for m in indMap]
    # the reference's checks, in its order: it takes the pairs from the last one backwards
    tbar = {}
    for at in range(len(pairs) - 1, -1, -1):
        ind1, ind2 = pairs[at]
        tbar[at] = product_knots(self.knots[ind1], self.order[ind1], other.knots[ind2], other.order[ind2], ind1, ind2)
        if any(i2 == ind2 for _, i2 in pairs[:at]) or any(i1 == ind1 for i1, _ in pairs[:at]):
            raise ValueError("You can't map the same independent variable to multiple others.")
    M = len(pairs)
    if M > HOST_MAX_M:
        raise NotImplementedError(f"multiply maps {M} pairs of variables; at most {HOST_MAX_M} are covered (deliberate scope)")

    dtype = np.result_type(self.coefs.dtype, other.coefs.dtype)
    if self.nDep == 0 or other.nDep == 0:
        raise ValueError("Mismatched dimensions")
    dep = dependent_terms(productType, self.nDep, other.nDep)
    mapped1, mapped2 = [p[0] for p in pairs], [p[1] for p in pairs]
    free1 = [i for i in range(self.nInd) if i not in mapped1]
    free2 = [i for i in range(other.nInd) if i not in mapped2]

    if M == 0:
        # no variable in common: the outer product, one broadcast multiplication per term
        a = self.coefs.astype(dtype, copy=False).reshape(self.coefs.shape + (1,) * other.nInd)
        b = other.coefs.astype(dtype, copy=False).reshape((other.nDep,) + (1,) * self.nInd + other.coefs.shape[1:])
        coefs = np.stack([sum(sign * a[da] * b[db] for da, db, sign in rows) for rows in dep])
        LAST_PATHS.append("outer")
        order, knots = [*self.order, *other.order], [*self.knots, *other.knots]
        return type(self)(len(order), len(dep), order, coefs.shape[1:], knots, coefs, self.metadata)

    a, rest1 = _canonical(self.coefs.astype(dtype, copy=False), mapped1)
    b, rest2 = _canonical(other.coefs.astype(dtype, copy=False), mapped2)
    variables = []
    for at, (ind1, ind2) in enumerate(pairs):
        f, g, W = product_map(self.knots[ind1], self.order[ind1], other.knots[ind2], other.order[ind2], tbar[at])
        variables.append((f, g, W, self.nCoef[ind1], other.nCoef[ind2]))
    UA, UB = int(np.prod(rest1, dtype=np.int64)), int(np.prod(rest2, dtype=np.int64))
    with ProductMap(variables) as maps:
        if a.size == 0 or b.size == 0:
            out = np.empty((len(dep) * UA * UB, *maps.nOut), dtype)
        else:
            out = _run(maps, a, b, plane_table(dep, UA, UB), _path)

    # (component, unmapped of self, unmapped of other, mapped) -> self's variables with the mapped ones in place, then other's
    out = out.reshape((len(dep), *rest1, *rest2, *maps.nOut))
    source = {v: 1 + n for n, v in enumerate(free1)}
    source.update({v: 1 + len(free1) + len(free2) + n for n, v in enumerate(mapped1)})
    axes = [0] + [source[v] for v in range(self.nInd)] + [1 + len(free1) + n for n in range(len(free2))]
    coefs = np.ascontiguousarray(out.transpose(axes))
    order = [self.order[v] for v in range(self.nInd)] + [other.order[v] for v in free2]
    knots = [self.knots[v] for v in range(self.nInd)] + [other.knots[v] for v in free2]
    for at, (ind1, ind2) in enumerate(pairs):
        order[ind1] = self.order[ind1] + other.order[ind2] - 1
        knots[ind1] = tbar[at]
    return type(self)(len(order), len(dep), order, coefs.shape[1:], knots, coefs, self.metadata)


# ------------------------------------------------------------------------------------------ the thin forms
def _common(self, other):
    return [(ix, ix) for ix in range(min(self.nInd, other.nInd))]


def _same_knots(self, nDep, coefs):
    return type(self)(self.nInd, nDep, self.order, self.nCoef, self.knots, coefs, self.metadata)


def dot(self, vector, **kwargs):
    if isinstance(vector, type(self)):
        return multiply(self, vector, _common(self, vector), "D", **kwargs)
    if len(vector) != self.nDep:
        raise ValueError("Invalid vector")
    coefs = vector[0] * self.coefs[0]
    for i in range(1, self.nDep):
        coefs = coefs + vector[i] * self.coefs[i]
    return _same_knots(self, 1, coefs[None])


def cross(self, vector, **kwargs):
    if isinstance(vector, type(self)):
        return multiply(self, vector, _common(self, vector), "C", **kwargs)
    c = self.coefs
    if self.nDep == 3:
        if len(vector) != 3:
            raise ValueError("Invalid vector")
        coefs = np.stack([vector[2] * c[1] - vector[1] * c[2], vector[0] * c[2] - vector[2] * c[0], vector[1] * c[0] - vector[0] * c[1]])
        return _same_knots(self, 3, coefs.astype(c.dtype, copy=False))
    if self.nDep != 2:
        raise ValueError("Invalid nDep")
    if len(vector) != 2:
        raise ValueError("Invalid vector")
    return _same_knots(self, 1, (vector[1] * c[0] - vector[0] * c[1]).astype(c.dtype, copy=False)[None])


def scale(self, multiplier, **kwargs):
    if isinstance(multiplier, type(self)):
        return multiply(self, multiplier, _common(self, multiplier), "S", **kwargs)
    if np.isscalar(multiplier):
        return _same_knots(self, self.nDep, multiplier * self.coefs)
    if len(multiplier) == self.nDep:
        column = np.asarray(multiplier).reshape((self.nDep,) + (1,) * self.nInd)
        return _same_knots(self, self.nDep, (self.coefs * column).astype(self.coefs.dtype, copy=False))
    if self.nDep == 1:
        column = np.asarray(multiplier).reshape((len(multiplier),) + (1,) * self.nInd)
        return _same_knots(self, len(multiplier), (column * self.coefs).astype(self.coefs.dtype, copy=False))
    raise ValueError("Invalid multiplier")


def transform(self, matrix):
    matrix = np.asarray(matrix)
    if not (matrix.ndim == 2 and matrix.shape[1] == self.nDep):
        raise ValueError("Invalid matrix")
    return _same_knots(self, matrix.shape[0], np.tensordot(matrix, self.coefs, axes=(1, 0)))
