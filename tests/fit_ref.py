"""
NumPy statement of Spline.least_squares for the tests and tools/fit_time.py: dense collocation matrices from a plain
Cox - de Boor recursion, one Householder QR (numpy.linalg.qr) per variable, the tolerance loop.  No GPU, no library.
"""
import numpy as np


def span_of(knots, order, u):
    """"Rightmost knot of the segment": searchsorted right, clamped to [order, len(knots) - order]."""
    return int(min(max(np.searchsorted(knots, u, "right"), order), len(knots) - order))


def basis_row(knots, order, u, derivative=0, ix=None):
    """(ix, values): the `order` B-splines (or their derivative) that are non-zero on segment ix at u."""
    knots = np.asarray(knots, np.float64)
    if ix is None:
        ix = span_of(knots, order, u)
    if derivative > order - 1:
        return ix, np.zeros(order)
    row = np.zeros(order + 1)                                 # row[j]: B-spline ix - order + j; row[order] stays 0
    row[order - 1] = 1.0
    for degree in range(1, order):
        lifted = np.zeros(order + 1)
        differentiate = degree > order - 1 - derivative
        for j in range(order - degree - 1, order):
            i = ix - order + j
            left_gap = knots[i + degree] - knots[i]
            right_gap = knots[i + degree + 1] - knots[i + 1]
            if differentiate:
                left = degree / left_gap if left_gap > 0 else 0.0
                right = -degree / right_gap if right_gap > 0 else 0.0
            else:
                left = (u - knots[i]) / left_gap if left_gap > 0 else 0.0
                right = (knots[i + degree + 1] - u) / right_gap if right_gap > 0 else 0.0
            lifted[j] = left * row[j] + right * row[j + 1]
        row = lifted
    return ix, row[:order]


def derivative_orders(u):
    d = np.zeros(len(u), int)
    for i in range(1, len(u)):
        if u[i] == u[i - 1]:
            d[i] = d[i - 1] + 1
    return d


def banded_matrix(knots, order, u):
    """(first, values): first column and `order` entries of every row; repeated parameters give derivative rows."""
    d = derivative_orders(u)
    first = np.empty(len(u), np.int32)
    values = np.empty((len(u), order))
    for r, (ur, dr) in enumerate(zip(u, d)):
        ix, values[r] = basis_row(knots, order, ur, int(dr))
        first[r] = ix - order
    return first, values


def dense_matrix(knots, order, u):
    first, values = banded_matrix(knots, order, u)
    A = np.zeros((len(u), len(knots) - order))
    for r in range(len(u)):
        A[r, first[r]:first[r] + order] = values[r]
    return A


def auto_knots(u, order, compression):
    u = np.asarray(u, np.float64)
    n = len(u)
    count = int((n - order) * (1.0 - compression) + 0.9999999999)
    spots = np.linspace(0.0, n - 1.0, count + 2)[1:-1]
    cells = spots.astype(int)
    alpha = spots - cells
    interior = (1.0 - alpha) * u[cells] + alpha * u[np.minimum(cells + 1, n - 1)]
    return np.sort(np.concatenate((np.full(order, u.min()), interior, np.full(order, u.max()))))


def qr_solve(A, b):
    Q, R = np.linalg.qr(A)
    return np.linalg.solve(R, Q.T @ b)


def fit(uValues, data, order, knots=None, compression=0.0, tolerance=None, matrix=dense_matrix, trace=None):
    """(knots, coefs) of the gridded fit; data (nDep, N0, ...).  `matrix(knots, order, u)` builds A; `trace`, a list,
    receives the row norms of every tolerance iteration."""
    data = np.asarray(data, np.float64)
    uValues = [np.asarray(u, np.float64) for u in uValues]
    nInd = len(uValues)
    if tolerance is not None:
        compression = 1.0
    if knots is None:
        knots = [auto_knots(u, o, compression) for u, o in zip(uValues, order)]
    knots = [np.array(k, np.float64) for k in knots]
    for iv in range(nInd):
        u = uValues[iv]
        b = np.moveaxis(data, iv + 1, 0)
        tail = b.shape[1:]
        b = b.reshape(len(u), -1)
        while True:
            A = matrix(knots[iv], order[iv], u)
            x = qr_solve(A, b)
            if tolerance is None:
                break
            norms = np.sqrt(np.sum((b - A @ x) ** 2, axis=1))
            if trace is not None:
                trace.append(norms)
            worst = int(np.argmax(norms))
            if norms[worst] <= tolerance / nInd:
                break
            k = knots[iv]
            ix = min(int(np.searchsorted(k, u[worst], "right")), A.shape[1])
            knots[iv] = np.sort(np.append(k, 0.5 * (k[ix - 1] + k[ix])))
        data = np.moveaxis(x.reshape((A.shape[1],) + tail), 0, iv + 1)
    return knots, np.ascontiguousarray(data)
