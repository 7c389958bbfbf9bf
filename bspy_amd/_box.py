"""
The tensor-product Bernstein box and its walk in plain Python floats, written once for any number of axes: the statement of
what the kernels of ``roots2`` (n = 2) and ``roots3`` (n = 3) compute, bit for bit, and through them of ``rays`` and
``surfaces``, which form cells of their own and walk them unchanged.

A cell is ``(dims, [component, ...])``: dims = (K0, ..., K(n-1)) and a component is the flat list of its K0 ... K(n-1)
floats, the last index fastest.  A FAMILY is the module of a cell family.  It supplies what the families do not share: the
Newton leaf ``_leaf(cell, lo, t0, h, S, out, near, R)``, ``slots(*dims)``, ``DEPTH`` (halvings per axis), ``WALK`` (nodes a
walk may visit), ``STATUS_WALK`` and ``SAME`` (the merge radius); their docstrings say what the numbers mean.
"""
import itertools
import math

import numpy as np

from . import roots


def _one_sign(comp):
    return all(x > 0.0 for x in comp) or all(x < 0.0 for x in comp)


def excluded(cell):
    return any(_one_sign(comp) for comp in cell[1])


def _along(dims, comp, axis, f):
    """f on every line of a component along ``axis``; f returns a tuple of lines -> a tuple of components."""
    stride = math.prod(dims[axis + 1:])
    K = dims[axis]
    outs = None
    for start in range(len(comp)):
        if (start // stride) % K:
            continue
        res = f([comp[start + e * stride] for e in range(K)])
        if outs is None:
            outs = [list(comp) for _ in res]
        for which, line in enumerate(res):
            for e in range(len(line)):
                outs[which][start + e * stride] = line[e]
    return tuple(outs)


def halve(cell, axis):
    """(left, right) halves of a cell along ``axis``."""
    dims, comps = cell
    parts = [_along(dims, comp, axis, lambda line: roots.split(line, 0.5)) for comp in comps]
    return (dims, [p[0] for p in parts]), (dims, [p[1] for p in parts])


def restrict_box(cell, lo, w):
    """The cell on the box [lo, lo + w] per axis: ``roots.restrict`` along axis 0, then axis 1, ..."""
    dims, comps = cell
    out = []
    for comp in comps:
        for axis in range(len(dims)):
            comp = _along(dims, comp, axis, lambda line: (roots.restrict(line, lo[axis], w[axis]),))[0]
        out.append(comp)
    return dims, out


def eval1(c, x):
    """Value and derivative of the Bernstein coefficients c at x."""
    b = list(c)
    K = len(b)
    s = 1.0 - x
    for r in range(1, K - 1):
        for i in range(K - r):
            b[i] = s * b[i] + x * b[i + 1]
    return s * b[0] + x * b[1], float(K - 1) * (b[1] - b[0])


def node_box(depth, path, n):
    """(corner, widths) of node (depth, path) of the walk in n variables: depth d splits axis d mod n, exact."""
    at, w = [0] * n, [1.0] * n
    for k in range(depth):
        bit = (path >> (depth - 1 - k)) & 1
        at[k % n], w[k % n] = 2 * at[k % n] + bit, 0.5 * w[k % n]
    return [float(at[a]) * w[a] for a in range(n)], w


def flag_cell(cell, mask):
    """What the ``_flag`` kernel of a family writes for one cell."""
    return 0 if mask or excluded(cell) else 1


def _outside(x, lo, w):
    if x != x:
        return float("inf")
    return max(0.0, lo - x, x - (lo + w))


def isolate_cell(family, cell, t0, t1, S, walk=None):
    """What the ``_isolate`` kernel of a family returns for one candidate cell on [t0, t1] per axis with the scales S:
    (zeros [tuple], near bytes, status, nodes visited)."""
    dims, comps = cell
    n = len(dims)
    R = family.slots(*dims)
    cell = (dims, [[float(x) for x in comp] for comp in comps])
    h = [t1[a] - t0[a] for a in range(n)]
    out, near = [], []
    cur, depth, path = cell, 0, 0
    live, done = True, False
    status = nodes = 0
    for _ in range(family.WALK if walk is None else walk):
        nodes += 1
        if not live:
            while path & 1:
                path >>= 1
                depth -= 1
            if depth == 0:
                done = True
                break
            path |= 1
            cur = restrict_box(cell, *node_box(depth, path, n))
            live = not excluded(cur)
        elif depth == n * family.DEPTH:
            status |= family._leaf(cell, node_box(depth, path, n)[0], t0, h, S, out, near, R)
            live = False
        else:
            left, right = halve(cur, depth % n)
            if not excluded(left):
                cur, path, depth = left, path << 1, depth + 1
            elif not excluded(right):
                cur, path, depth = right, (path << 1) | 1, depth + 1
            else:
                live = False
    if not done:
        status |= family.STATUS_WALK
    return out, near, status, nodes


def merge_keep(found, flags, cand, breaks, same):
    """The keep bytes of the ``_merge`` kernel of a family: found = the (zeros, near) pairs of the candidates, in their
    order.  The neighbours are the cells that precede a cell in flat index, the lower half of the 3^n around it."""
    nc = flags.shape[1:]
    n = len(nc)
    slot_of = {int(at): m for m, at in enumerate(cand)}
    before = list(itertools.product((-1, 0, 1), repeat=n))[:(3 ** n - 1) // 2]
    keep = []
    for m, (zeros, near) in enumerate(found):
        b, *at = np.unravel_index(int(cand[m]), flags.shape)
        tol = [same * (float(breaks[a][at[a] + 1]) - float(breaks[a][at[a]])) for a in range(n)]
        row = []
        for z, close in zip(zeros, near):
            k = 1
            if close:
                for delta in before:
                    other = tuple(at[a] + delta[a] for a in range(n))
                    if any(other[a] < 0 or other[a] >= nc[a] for a in range(n)) or not flags[(b,) + other]:
                        continue
                    for zz in found[slot_of[int(np.ravel_multi_index((b,) + other, flags.shape))]][0]:
                        if all(abs(zz[a] - z[a]) <= tol[a] for a in range(n)):
                            k = 0
            row.append(k)
        keep.append(row)
    return keep


def statement(family, rows, plan, mask, scale, walk=None):
    """flags, candidates, zeros (NaN padded), near, count, status, nodes and keep of the extracted rows (B, n, R0, ...),
    from the functions above: what the host drivers and the kernels of a family return, bit for bit."""
    n = plan.nind
    R = family.slots(*plan.order)

    def cell_of(b, *at):
        window = tuple(slice(plan.first[a][i], plan.first[a][i] + plan.order[a]) for a, i in enumerate(at))
        return plan.order, [[float(x) for x in rows[(b, d) + window].reshape(-1)] for d in range(n)]

    flags = np.zeros(mask.shape, np.uint8)
    for where in np.ndindex(*mask.shape):
        flags[where] = flag_cell(cell_of(*where), int(mask[where]))
    cand = np.flatnonzero(flags).astype(np.int64)
    out = np.full((len(cand), R, n), np.nan)
    near = np.zeros((len(cand), R), np.uint8)
    count, status, nodes = np.zeros(len(cand), np.int32), np.zeros(len(cand), np.uint8), np.zeros(len(cand), np.int32)
    found = []
    for m, flat in enumerate(cand):
        b, *at = np.unravel_index(int(flat), mask.shape)
        t0 = [float(plan.breaks[a][i]) for a, i in enumerate(at)]
        t1 = [float(plan.breaks[a][i + 1]) for a, i in enumerate(at)]
        zeros, close, status[m], nodes[m] = isolate_cell(family, cell_of(b, *at), t0, t1, [float(s) for s in scale[b]], walk)
        found.append((zeros, close))
        count[m] = len(zeros)
        out[m, :len(zeros)] = np.array(zeros).reshape(-1, n)
        near[m, :len(zeros)] = close
    keep = np.zeros((len(cand), R), np.uint8)
    for m, row in enumerate(merge_keep(found, flags, cand, plan.breaks, family.SAME)):
        keep[m, :len(row)] = row
    return dict(flags=flags, cand=cand, roots=out, near=near, count=count, status=status, nodes=nodes, keep=keep)
