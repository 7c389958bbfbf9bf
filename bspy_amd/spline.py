"""
``bspy_amd.Spline``: drop-in for the evaluation path of the reference's ``bspy.Spline``
(bspy/spline.py) - same constructor, attributes, call conventions, return types and
error messages for

    Spline(nInd, nDep, order, nCoef, knots, coefs, metadata={})   spline.py:46-76
    s(*uvw) / s.evaluate(*uvw)                                    spline.py:78-79, :904-949
    s.derivative(with_respect_to, *uvw)                           spline.py:720-770
    s.jacobian(uvw) / s.tangent_space(uvw)                        spline.py:1354-1377, :2238-2252
    s.domain()                                                    spline.py:794-808
    s.normal(uvw, normalize=True, indices=None)                   spline.py:1648-1682
    s.integral(integrand=None, domain=None)                       spline.py:1249 (nInd 1 - 3)
    Spline.bspline_values(knot, knots, splineOrder, u, ...)       spline.py:207-252
    Spline.least_squares(uValues, dataPoints, order, knots, ...)  spline.py:1402 (gridded data; not Spline-valued data)
    s.insert_knots(newKnots) / s.trim(newDomain) / s.clamp(l, r)  spline.py:1219, :2386, :282
    s.elevate(m) / s.elevate_and_insert_knots(m, newKnots)        spline.py:845-902
    s.differentiate(with_respect_to=0)                            spline.py:772
    s.remove_knot(iKnot, nLeft, nRight) / s.remove_knots(tol)     spline.py:1812, :1848 (its own statement: reduction.py)
    s.range_bounds()                                              spline.py:1794
    s.multiply(other, indMap, productType) / dot / cross / scale  spline.py:1585, :821, :641, :2028
    s.transform(matrix), s * x, x * s, s @ x, x @ s, -s, s / x    spline.py:2307, :97-147
    Spline.common_basis(splines, indMap) / s.add / s.subtract     spline.py:308, :149, :2199
    s.translate(vector), s + x, x + s, s - x, x - s               spline.py:2335, :85-95, :132-143
    s.integrate(with_respect_to=0) / s.contract(uvw)              spline.py:1290, :567
    s.zeros() (curves: nInd == nDep == 1)                         spline.py:2470
    s.zeros2() (the same call for nInd == nDep == 2)              spline.py:2470
    to_dict / from_dict / load / save (JSON, as an input format)   spline.py:1099-1125, :1542-1583, :1998-2026, :2254-2267

The arithmetic runs on the GPU (bspy_amd/_spline_evaluation.py -> libbspy_amd.so); the
rest of the reference's Spline API (the other fitting calls - fit, contour, solve_ode, ... -, zeros for nInd > 2,
intersect, contours, CSG, viewer) is out of scope.

Documented deviations from the reference:
  * all-integer knots / coefs are promoted to float64 (the reference keeps int64 and
    silently truncates, e.g. Spline(1,1,[4],[4],[[0,0,0,0,1,1,1,1]],[[0.,1,2,3]])(0.5) -> 0);
  * batched calls with nDep == 1 and N-D inputs return the full broadcast shape (the
    reference returns only column 0 of each row);
  * of the ufunc keyword arguments of the reference's np.frompyfunc wrapper, where= and out= are
    honoured (out= also takes float arrays); the others (casting=, order=, ...) raise TypeError;
  * mixed float32/float64 inputs are computed in float64;
  * differentiate() of a spline with an interior knot of full multiplicity raises ValueError (the reference
    divides by the zero knot gap and returns inf / nan coefficients);
  * remove_knot() raises ValueError where an operator weight is not finite (a fixed unknown, nLeft / nRight, whose
    pivot is zero; the reference returns inf / nan); remove_knots() follows the statement of bspy_amd/reduction.py,
    not the reference's serial loop, and always returns a new spline;
  * CUDA/HIP torch tensors are accepted as parameters (results stay on the GPU) and
    jacobian() accepts arrays of points (the reference's is single-point).
"""
import numpy as np

from . import _spline_evaluation as _ev


def _as_float_array(a):
    a = np.array(a)
    if not np.issubdtype(a.dtype, np.floating):
        a = a.astype(np.float64)
    elif a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return a


class Spline:
    """Tensor-product B-spline with nInd independent and nDep dependent variables
    (constructor semantics of the reference, bspy/spline.py:46-76)."""

    def __init__(self, nInd, nDep, order, nCoef, knots, coefs, metadata={}):
        # argument checks in the reference's order, with its messages (spline.py:47-69)
        def need(ok, message):
            if not ok:
                raise ValueError(message)

        need(nInd >= 0, "nInd < 0")
        need(nDep >= 0, "nDep < 0")
        self.nInd, self.nDep = int(nInd), int(nDep)
        need(len(order) == self.nInd, "len(order) != nInd")
        need(len(nCoef) == self.nInd, "len(nCoef) != nInd")
        self.order = tuple(map(int, order))
        self.nCoef = tuple(map(int, nCoef))
        need(len(knots) == nInd, "len(knots) != nInd")
        for variable, (kv, o, n) in enumerate(zip(knots, self.order, self.nCoef)):
            need(len(kv) == o + n, f"Knots array for variable {variable} should have length {o + n}")
        self.knots = tuple(_as_float_array(kv) for kv in knots)
        for kv, o, n in zip(self.knots, self.order, self.nCoef):
            # non-decreasing over the first nCoef + 1 knots, and every basis function has support
            # (knots[i + order] > knots[i]), reference spline.py:61-64
            proper = n == 0 or (bool(np.all(np.diff(kv[:n + 1]) >= 0)) and bool(np.all(kv[o:o + n] > kv[:n])))
            need(proper, "Improper knot order or multiplicity")
        points = int(np.prod(self.nCoef, dtype=np.int64)) if self.nCoef else 1
        need(len(coefs) in (points, self.nDep), f"Length of coefs should be {points} or {self.nDep}")
        table = _as_float_array(coefs)
        canonical = (self.nDep, *self.nCoef)
        if table.shape != canonical:
            if len(table) == points:
                # flat "list of points" form: nDep fastest, then the FIRST variable (spline.py:72-73)
                table = table.reshape((*reversed(self.nCoef), self.nDep)).T
            else:
                # one array per dependent variable, each stored last-variable-first (spline.py:74-75)
                table = np.stack([np.transpose(component) for component in table]).reshape(canonical)
        self.coefs = table
        self.metadata = dict(metadata)

    def __call__(self, *uvw, **kwargs):
        return self.evaluate(*uvw, **kwargs)

    def __repr__(self):
        return f"Spline({self.nInd}, {self.nDep}, {self.order}, {self.nCoef}, ...)"

    # ------------------------------------------------------------------ evaluation
    @staticmethod
    def bspline_values(knot, knots, splineOrder, u, derivativeOrder=0, taylorCoefs=False):
        """B-spline (derivative) basis values of one segment; reference spline.py:207-252."""
        return _ev.bspline_values(knot, knots, splineOrder, u, derivativeOrder, taylorCoefs)

    def _batched_masked(self, with_respect_to, uvw, where, out, device):
        """The ufunc keyword arguments the reference's np.frompyfunc call honours (bspy/spline.py:943-947):
        ``where`` - only the selected points are evaluated (an out-of-domain value under a False entry does not
        raise); unselected results are NaN, or what ``out`` held; ``out`` - nDep arrays of the broadcast shape
        (one array when nDep == 1) that receive the results (object arrays as np.frompyfunc needs, or float
        arrays).  Returns new arrays in the coefficients' dtype, as the reference does."""
        arrays = [np.asarray(a) for a in uvw]
        mask = np.asarray(True if where is None else where, dtype=bool)
        shape = np.broadcast_shapes(mask.shape, *[a.shape for a in arrays])
        outs = None
        if out is not None:
            outs = (out,) if not isinstance(out, (tuple, list)) else tuple(out)
            if len(outs) != self.nDep:
                raise ValueError(f"out must hold {self.nDep} arrays")
            shape = np.broadcast_shapes(shape, *[o.shape for o in outs])
            for o in outs:
                if o.shape != shape:
                    raise ValueError("non-broadcastable output operand")
        sel = np.broadcast_to(mask, shape)
        res = np.full((self.nDep, *shape), np.nan, _ev.compute_dtype(self))
        if outs is not None:
            for d, o in enumerate(outs):
                res[d] = np.asarray(o, dtype=res.dtype)
        pts = [np.broadcast_to(a, shape)[sel] for a in arrays]
        if pts[0].size:
            try:
                res[:, sel] = _ev.evaluate_batch(self, with_respect_to, pts, device=device)
            except ValueError as e:
                raise ValueError(str(e)) from None
        if outs is not None:
            for d, o in enumerate(outs):
                o[...] = res[d]
        res = res.astype(self.coefs.dtype, copy=False)
        return tuple(res[d] for d in range(self.nDep)) if self.nDep > 1 else res[0]

    def _batched(self, with_respect_to, uvw, kwargs):
        device = kwargs.pop("device", None)
        check = kwargs.pop("check", True)
        where = kwargs.pop("where", None)
        out = kwargs.pop("out", None)
        if kwargs:
            raise TypeError("ufunc keyword arguments other than where= / out= are not supported by bspy_amd: " + ", ".join(sorted(kwargs)))
        if where is not None or out is not None:
            if any(_ev._is_torch(a) for a in uvw):
                raise TypeError("where= / out= take NumPy arrays")
            return self._batched_masked(with_respect_to, uvw, where, out, device)
        out = _ev.evaluate_batch(self, with_respect_to, uvw, device=device, check=check)
        if _ev._is_torch(out):
            import torch
            tdt = torch.float32 if self.coefs.dtype == np.float32 else torch.float64
            out = out.to(tdt)
            return tuple(out[d] for d in range(self.nDep)) if self.nDep > 1 else out[0]
        out = out.astype(self.coefs.dtype, copy=False)
        return tuple(out[d] for d in range(self.nDep)) if self.nDep > 1 else out[0]

    def evaluate(self, *uvw, **kwargs):
        """Value of the spline; dispatch of the reference (spline.py:935-949):
        s(u, v) with scalars or s([u, v]) -> ndarray (nDep,);
        s(uArray, vArray) (broadcast, ufunc style) -> tuple of nDep arrays (one array when nDep == 1)."""
        if len(uvw) == 0 and self.nInd == 0:
            return self.coefs
        elif _isscalar(uvw[0]):
            return _ev.evaluate(self, uvw)
        elif len(uvw) > 1 or len(uvw[0]) > self.nInd:
            return self._batched(None, uvw, kwargs)
        else:
            return _ev.evaluate(self, *uvw)

    def derivative(self, with_respect_to, *uvw, **kwargs):
        """Derivative of the spline, with_respect_to[i] = derivative order in variable i;
        same dispatch as evaluate (reference spline.py:757-770)."""
        if len(uvw) == 0 and self.nInd == 0:
            return np.zeros(self.nDep, self.coefs.dtype)
        elif _isscalar(uvw[0]):
            return _ev.derivative(self, with_respect_to, uvw)
        elif len(uvw) > 1 or len(uvw[0]) > self.nInd:
            return self._batched(with_respect_to, uvw, kwargs)
        else:
            return _ev.derivative(self, with_respect_to, *uvw)

    def jacobian(self, uvw, **kwargs):
        """(nDep, nInd) matrix of first partial derivatives at one point (reference
        spline.py:1354-1377).  Extension: nInd arrays of points -> (nDep, nInd, *shape)."""
        if len(uvw) == self.nInd and self.nInd > 0 and not _isscalar(uvw[0]) and _ndim(uvw[0]) > 0:
            out = _ev.jacobian_batch(self, uvw, device=kwargs.pop("device", None), check=kwargs.pop("check", True))
            if _ev._is_torch(out):
                return out
            return out.astype(self.coefs.dtype, copy=False)
        return _ev.jacobian(self, uvw)

    def normal(self, uvw, normalize=True, indices=None):
        """Normal of the spline (|nInd - nDep| must be 1; reference spline.py:1648-1682): unit
        length by default, else the area-scaled cofactor vector; `metadata["negateNormal"]`
        flips it.  Extension: nInd arrays of points -> (len(normal), *shape)."""
        return _ev.normal(self, uvw, normalize, indices)

    def curvature(self, uv):
        """Curvature of a curve (nDep >= 2) or Gaussian curvature of a surface in 3-D
        (reference spline.py `curvature` -> _spline_evaluation.py:80-107); arrays of points
        give an array of curvatures."""
        return _ev.curvature(self, uv)

    def integral(self, integrand=None, domain=None):
        """Integral over ``domain`` (nInd x 2, default the spline's domain) of integrand(x) dA, where dA is the
        measure of the map (product of the singular values of the jacobian): arc length, area or volume when
        ``integrand`` is None, moments with e.g. ``lambda x: x[0]`` (reference spline.py:1249).  Returns a float.

        Every knot cell inside the domain is integrated by a tensor Gauss-Kronrod 7/15 rule on the GPU, split
        adaptively until each region's Kronrod / Gauss difference is within its share of max(tol, tol |I|),
        tol = 1e-13 / nInd (the reference's request); float32 splines evaluate their nodes in float32 (sums in
        float64) with tol = 1e-6.  A callable integrand is called once per quadrature node with x (ndarray, nDep)
        and must return a scalar.  After 40 rounds or 2^22 regions the current sum is returned with a
        RuntimeWarning that gives the estimated error.  Results are bitwise reproducible.
        nInd 1 to 3 only: nInd >= 4 raises NotImplementedError (deliberate scope)."""
        from . import integral as _integral
        return _integral.integral(self, integrand, domain)

    @staticmethod
    def least_squares(uValues, dataPoints, order=None, knots=None, compression=0.0, tolerance=None, fixEnds=False,
                      metadata={}, **kwargs):
        """Least-squares fit of a spline to gridded data (reference spline.py:1402, its signature, defaults, checks
        and ValueError messages).  Returns a Spline with float64 knots and coefficients.

        uValues: the parameter values, one array (nInd 1) or nInd arrays, each non-decreasing; a repeated value
        means the next derivative at that parameter (Hermite data).  dataPoints: shape (nDep, N0, ..., N_{nInd-1}),
        NumPy float32 / float64 or a torch CUDA tensor of those types, which is used where it is (float32 is read
        as float32 and computed in float64).  order defaults to min(4, N_i) per variable; knots default to the
        reference's rule: clamped ends and int((N_i - order)(1 - compression) + 0.9999999999) interior knots.
        tolerance: fit to tolerance - start without interior knots, and while the largest 2-norm of a residual
        row exceeds tolerance / nInd insert the midpoint knot of that row's span and solve again.

        Each variable is one banded Givens QR (no normal equations), factored once on the host and applied to all
        lines of the data by a GPU kernel; few lines (curves) and orders above 8 apply it on the host.  Results are
        bitwise reproducible.  Deliberate scope: fixEnds=True and rank-deficient systems are solved on the host with
        the reference's dense algebra (correct, not fast); dataPoints made of Spline objects raises
        NotImplementedError.  ``_path="device"`` / ``"host"`` pins the path (tests, measurements)."""
        from . import fitting as _fitting
        return _fitting.least_squares(uValues, dataPoints, order, knots, compression, tolerance, fixEnds, metadata, **kwargs)

    @staticmethod
    def fit_points(uvw, points, order, knots, weights=None, smoothing=0.0, penalty=None, correct=0, metadata={}, robust=None,
                   iterations=8, solve=None, **kwargs):
        """Least-squares fit of a spline to scattered data (an extension beyond the reference's API; the gridded call is
        ``least_squares``).  uvw: (nInd, N) parameters, or (N,) for a curve; points: (nDep, N); NumPy float32 / float64 or
        torch CUDA tensors of those types (float32 is widened first).  order and knots are required.  weights: (N,), all
        >= 0, or None.  Returns the Spline (float64) that minimises

            sum_i w_i |S(u_i) - p_i|^2 + smoothing E_m(S),

        E_m the energy of derivative order m = ``penalty`` (default min(2, min(order) - 1)): int |S'|^2 or int |S''|^2 for
        a curve, membrane or thin plate for a surface.  ``correct=n`` runs n rounds of parameter correction (nDep 2 or 3):
        uvw <- s.project(points, guess=uvw), then the fit again on the same knots.

        The normal equations are assembled on the GPU without atomics (a key per point, a stable sort, per-cell Gram
        slabs in a stated association, a gather) and solved by a banded Cholesky factorisation on the host; few points,
        orders 5 and 6 and nDep > 4 are assembled on the host by the same functions.  Results are bitwise reproducible.
        A point outside the domain, with a NaN or infinite value or a negative weight is excluded with one
        RuntimeWarning (``scatter.fit_batch`` returns the status bits, residuals and objective values).  smoothing == 0
        with a coefficient that has no data in its support raises ValueError, as does a matrix that is not positive
        definite.  Curves and surfaces of orders 2 to 6; nInd 3 raises NotImplementedError (deliberate scope).

        ``robust="huber"`` / ``"tukey"`` / ``(name, c)`` makes the fit robust against gross outliers: behind the plain fit
        run exactly ``iterations`` reweighted rounds (residuals, sigma = 1.4826 x their lower median, the loss's weights
        times ``weights``, assemble, solve; fewer rounds only when sigma == 0.0; no convergence test, so the result is a
        function of the inputs alone).  c defaults to 1.345 (Huber) and 4.685 (Tukey).  Tukey gives a point beyond
        c sigma the weight 0.0 and can so take all weight from under a coefficient: that raises the ValueError of a matrix
        that is not positive definite.  ``solve="host"`` / ``"device"`` pins the banded solve; None is the host solve for a
        plain fit and, for a robust fit on the device path, the device solve (``bsk_scatter_solve``: the host's bytes) once
        the system is large enough for it (``scatter.SOLVE_MIN_WORK``).
        ``_path="device"`` / ``"host"`` pins the path (tests, measurements)."""
        from . import scatter as _scatter
        return _scatter.fit_points(uvw, points, order, knots, weights=weights, smoothing=smoothing, penalty=penalty, correct=correct,
                                   metadata=metadata, robust=robust, iterations=iterations, solve=solve, **kwargs)

    # ------------------------------------------------------------------ spline to spline (bspy_amd/refinement.py)
    def insert_knots(self, newKnots, **kwargs):
        """Insert knots: newKnots holds per independent variable an iterable of knots or (knot, multiplicity) pairs
        (reference spline.py:1219, its checks and ValueError messages).  Returns a Spline of the same function on the
        refined knots, coefficients in this spline's dtype.  Per variable the insertion is one banded operator built
        on the host and applied to all lines of the coefficients by a GPU kernel (small tensors: on the host);
        ``_path="device"`` / ``"host"`` pins the path."""
        from . import refinement as _refinement
        return _refinement.insert_knots(self, newKnots, **kwargs)

    def elevate(self, m, **kwargs):
        """Raise the order of variable i by m[i] (reference spline.py:845)."""
        from . import refinement as _refinement
        return _refinement.elevate(self, m, **kwargs)

    def elevate_and_insert_knots(self, m, newKnots, **kwargs):
        """Raise the order by m and insert the knots newKnots (plain values) in one step (reference spline.py:872);
        returns self when there is nothing to do.  The spline is clamped on the left first; the resulting knots follow
        the reference's rule.  The operator is built by blossoming, not by differentiating and integrating back."""
        from . import refinement as _refinement
        return _refinement.elevate_and_insert_knots(self, m, newKnots, **kwargs)

    def trim(self, newDomain, **kwargs):
        """Restrict the spline to newDomain (nInd x 2; None / nan keeps a bound; reference spline.py:2386): full
        multiplicity knots at the bounds, which snap to a knot within eps.  Returns self when nothing changes."""
        from . import refinement as _refinement
        return _refinement.trim(self, newDomain, **kwargs)

    def clamp(self, left, right, **kwargs):
        """Full multiplicity at the domain's left / right end of the listed variables (reference spline.py:282)."""
        from . import refinement as _refinement
        return _refinement.clamp(self, left, right, **kwargs)

    def differentiate(self, with_respect_to=0, **kwargs):
        """The spline of the derivative with respect to one variable (reference spline.py:772)."""
        from . import refinement as _refinement
        return _refinement.differentiate(self, with_respect_to, **kwargs)

    # ------------------------------------------------------------------ data reduction (bspy_amd/reduction.py)
    def range_bounds(self):
        """[[min, max]] of the coefficients per dependent variable, in the coefficients' dtype (reference
        _spline_evaluation.py:248)."""
        from . import reduction as _reduction
        return _reduction.range_bounds(self)

    def remove_knot(self, iKnot, nLeft=0, nRight=0):
        """Remove knot iKnot of a curve: (spline, residual) with the least-squares coefficients of the window and the
        per-component absolute residual (reference _spline_domain.py:452, its messages).  nLeft / nRight coefficients
        at the ends are kept by exact substitution.  Raises ValueError where an operator weight is not finite."""
        from . import reduction as _reduction
        return _reduction.remove_knot(self, iKnot, nLeft, nRight)

    def remove_knots(self, tolerance=1e-14, nLeft=0, nRight=0, **kwargs):
        """Remove as many knots as the tolerance (relative to max |coefficient| per dependent variable) allows, with a
        certified bound on the sup-norm error against this spline (the statement in bspy_amd/reduction.py; the
        reference's signature, spline.py:1848, not its serial loop).  Always returns a new spline.
        ``_path="device"`` / ``"host"`` pins the path."""
        from . import reduction as _reduction
        return _reduction.remove_knots(self, tolerance, nLeft, nRight, **kwargs)

    # ------------------------------------------------------------------ products (bspy_amd/product.py)
    def multiply(self, other, indMap=None, productType='S', **kwargs):
        """Product of two splines (reference spline.py:1585, its checks and ValueError messages).  indMap: indices n (variable
        n of self is variable n of other) or pairs (n, m); mapped variables must have the same domain, the others stay
        independent: the result has self's variables, the mapped ones in place, then other's unmapped ones.  productType
        'S' scalar product (nDep equal, or 1 on one side), 'D' dot product, 'C' cross product (nDep 2 or 3).  A mapped
        variable of orders k1 and k2 has order k1 + k2 - 1 and the reference's knots; the coefficients come from one
        banded bilinear operator per mapped variable, applied by one GPU kernel (small results, three mapped variables
        and orders outside 2 .. 6: on the host); more than three mapped variables raise NotImplementedError.
        ``_path="device"`` / ``"host"`` pins the path."""
        from . import product as _product
        return _product.multiply(self, other, indMap, productType, **kwargs)

    def dot(self, vector, **kwargs):
        """Dot product with a vector or, over the common variables, with a Spline (reference spline.py:821)."""
        from . import product as _product
        return _product.dot(self, vector, **kwargs)

    def cross(self, vector, **kwargs):
        """Cross product with a vector or, over the common variables, with a Spline (reference spline.py:641)."""
        from . import product as _product
        return _product.cross(self, vector, **kwargs)

    def scale(self, multiplier, **kwargs):
        """Scale by a scalar, by a vector (per component; nDep == 1 broadcasts) or by a Spline (reference spline.py:2028)."""
        from . import product as _product
        return _product.scale(self, multiplier, **kwargs)

    def transform(self, matrix):
        """Apply a matrix (rows x nDep) to the dependent variables (reference spline.py:2307)."""
        from . import product as _product
        return _product.transform(self, matrix)

    def _common(self, other):
        return [(ix, ix) for ix in range(min(self.nInd, other.nInd))]

    def __matmul__(self, other):
        if isinstance(other, Spline):
            return self.multiply(other, self._common(other), 'D')
        other = np.atleast_1d(other)
        return self.transform(other.T) if other.ndim > 1 else self.dot(other)

    def __rmatmul__(self, other):
        if isinstance(other, Spline):
            return other.multiply(self, self._common(other), 'D')
        other = np.atleast_1d(other)
        return self.transform(other) if other.ndim > 1 else self.dot(other)

    def __mul__(self, other):
        return self.multiply(other, self._common(other), 'S') if isinstance(other, Spline) else self.scale(other)

    def __rmul__(self, other):
        return other.multiply(self, self._common(other), 'S') if isinstance(other, Spline) else self.scale(other)

    def __neg__(self):
        return self.scale(-1.0)

    def __truediv__(self, other):
        if not np.isscalar(other):
            raise ValueError('Divisor must be a scalar')
        return self * (1.0 / other)

    # ------------------------------------------------------------------ sums (bspy_amd/sums.py)
    @staticmethod
    def common_basis(splines, indMap=None, **kwargs):
        """Align splines to one basis (reference spline.py:308): every spline is clamped in all its variables; per entry
        (i0, .., iN) of indMap the variables take the largest order and the merged knots (multiplicities raised with the
        order), by one elevate_and_insert_knots per spline.  indMap None aligns variable i of every spline.  A spline that
        needs nothing comes back itself."""
        from . import sums as _sums
        return _sums.common_basis(splines, indMap, **kwargs)

    def add(self, other, indMap=None, **kwargs):
        """Sum of two splines of one nDep (reference spline.py:149).  indMap: indices n or pairs (n, m) of variables that
        are the same variable; they are brought to a common basis first.  None: no variable in common (the outer sum,
        nothing is clamped).  The result has self's variables, the mapped ones in place, then other's unmapped ones, and
        self's metadata and coefficient dtype.  Large results: band kernels, then one broadcast-sum kernel, on the GPU.
        ``_path="device"`` / ``"host"`` pins the path."""
        from . import sums as _sums
        return _sums.add(self, other, indMap, **kwargs)

    def subtract(self, other, indMap=None, **kwargs):
        """self - other (reference spline.py:2199): ``add`` with the sign of other's coefficients turned."""
        from . import sums as _sums
        return _sums.subtract(self, other, indMap, **kwargs)

    def translate(self, translationVector):
        """Add a vector to the dependent variables (reference spline.py:2335)."""
        from . import sums as _sums
        return _sums.translate(self, translationVector)

    def integrate(self, with_respect_to=0, **kwargs):
        """Antiderivative in one variable that vanishes at the left end of the domain (reference spline.py:1290): order and
        coefficient count of that variable go up by one, both end knots are repeated once more, the coefficients are a
        weighted running sum (large tensors: on the GPU).  ``_path="device"`` / ``"host"`` pins the path."""
        from . import sums as _sums
        return _sums.integrate(self, with_respect_to, **kwargs)

    def contract(self, uvw, **kwargs):
        """Fix the variables whose entry of uvw is not None at that value (reference spline.py:567); the others stay the
        variables of the result, which may have none.  Returns self when nothing is fixed."""
        from . import sums as _sums
        return _sums.contract(self, uvw, **kwargs)

    # ------------------------------------------------------------------ roots (bspy_amd/roots.py)
    def zeros(self, epsilon=None, initialScale=None, **kwargs):
        """The real roots of a scalar curve (nInd == nDep == 1; reference spline.py:2470): a list, ascending, of scalars of
        the knots' dtype for isolated roots and of (left, right) tuples for intervals on which the spline is zero.
        ``epsilon`` and ``initialScale`` are accepted and ignored, as the reference's curve path ignores them.  Every knot
        span is brought to Bernstein form by one band operator; spans whose coefficients show no sign change are rejected
        by one kernel, the others are isolated by subdivision, one lane per span, and refined by bisection to adjacent
        doubles (few spans and orders above 8: the same arithmetic on the host).  What counts as a root (zero spans,
        roots at knots, touching roots, jumps) is stated in bspy_amd/roots.py.  Results are bitwise reproducible and the
        same on both paths.  nInd != nDep raises the reference's ValueError; nInd == nDep > 1 raises NotImplementedError
        (deliberate scope).  ``_path="device"`` / ``"host"`` pins the path.  ``bspy_amd.roots.zeros_batch`` does the same
        for every component of a curve with any nDep."""
        from . import roots as _roots
        return _roots.zeros(self, epsilon, initialScale, **kwargs)

    def zeros2(self, **kwargs):
        """The isolated common zeros of two scalar splines in two variables (nInd == nDep == 2; the reference reaches them
        through ``zeros``, whose name here stays with curves): a list, sorted by (u, v), of length-2 arrays (u, v) of the
        knots' dtype and, for every knot cell on which a component vanishes, a tuple ((u0, v0), (u1, v1)).  Both variables
        are brought to Bezier form by the band operator; cells whose coefficients exclude a zero are rejected by one kernel,
        the others are walked by dyadic subdivision, one lane per cell, and polished by Newton steps (few cells and orders 5
        and 6: the same arithmetic on the host).  What counts as a zero is stated in bspy_amd/roots2.py.  Results are bitwise
        reproducible and the same on both paths.  Raises the reference's ValueError for nInd != nDep, a ValueError that names
        the cell when zeros could not be isolated there or a zero is tangential, NotImplementedError for nInd != 2 or an
        order above 6.  ``_path="device"`` / ``"host"`` pins the path.  ``bspy_amd.roots2.zeros2_batch`` solves many systems
        on the same knots in one launch sequence."""
        from . import roots2 as _roots2
        return _roots2.zeros2(self, **kwargs)

    def zeros3(self, **kwargs):
        """The isolated common zeros of three scalar splines in three variables (nInd == nDep == 3, for example
        ``surface.subtract(curve)``; the reference reaches them through ``zeros``): a list, sorted by (u, v, w), of length-3
        arrays (u, v, w) of the knots' dtype and, for every knot cell on which a component vanishes, a tuple
        ((u0, v0, w0), (u1, v1, w1)).  The three variables are brought to Bezier form by the band operator; cells whose
        coefficients exclude a zero are rejected by one kernel, every other cell is walked by dyadic subdivision by one
        wave, a lane per coefficient, and its leaves are polished by Newton steps (few cells: the same arithmetic on the
        host).  What counts as a zero is stated in bspy_amd/roots3.py.  Results are bitwise reproducible and the same on
        both paths.  Raises the reference's ValueError for nInd != nDep, a ValueError that names the cell when zeros could
        not be isolated there or a zero is tangential, NotImplementedError for nInd != 3 or an order outside 2 .. 4.
        ``_path="device"`` / ``"host"`` pins the path.  ``bspy_amd.roots3.zeros3_batch`` solves many systems on the same
        knots in one launch sequence."""
        from . import roots3 as _roots3
        return _roots3.zeros3(self, **kwargs)

    def project(self, points, guess=None, samples=None, **kwargs):
        """The closest point of the spline to each of N query points (an extension: the reference has no counterpart).
        ``points``: (nDep, *shape), NumPy float32 / float64 or a torch CUDA tensor of those types.  Returns ``(uvw,
        distance)``: the parameters (nInd, *shape) in the knots' dtype and the Euclidean distances (*shape) in float64;
        CUDA in gives CUDA out.  Curves (nInd 1) of order 2 .. 6 and surfaces (nInd 2) of orders 2 .. 4, nDep 2 or 3;
        anything else raises NotImplementedError.  Every knot cell is sampled ``samples`` times per axis (default: the
        order of the axis; 1 .. 8), the nearest sample of a point is found by brute force, one lane per point, and refined
        by Newton steps on the squared distance; ``guess`` (nInd, *shape) takes the place of the search.  The result is the
        local minimiser reached from the nearest sample: the closest point whenever that sample lies in its basin; it is
        NOT certified global.  What is computed is stated in bspy_amd/project.py; results are bitwise reproducible and
        the same on both paths.  One RuntimeWarning when a point did not converge (bspy_amd.project.project_batch returns
        the status of every point).  ``_path="device"`` / ``"host"`` pins the path."""
        from . import project as _project
        return _project.project(self, points, guess=guess, samples=samples, **kwargs)

    def intersect_rays(self, origins, directions, tmin=0.0, tmax=float("inf"), **kwargs):
        """Where N rays o + t d hit this surface, and which hit comes first (an extension: the reference has no
        counterpart).  ``origins``, ``directions``: (3, *shape), NumPy float32 / float64 or torch CUDA tensors of those
        types; directions need not be normalised.  Returns ``(uv, t)``: the parameters (2, *shape) in the knots' dtype and
        t (*shape) in float64 with S(uv) = o + t d, for the hit of smallest t in [tmin, tmax]; NaN for a ray without a hit;
        CUDA in gives CUDA out.  Surfaces (nInd 2, nDep 3) of orders 2 .. 4; anything else raises NotImplementedError.  A
        hit is a common zero of the two planes of the ray on the surface: almost every (ray, knot cell) pair is discarded
        by a box test and the rest is isolated by the walk of ``zeros2``.  What is computed is stated in
        bspy_amd/rays.py; results are bitwise reproducible and the same on both paths.  A grazing hit (the ray
        tangent to the surface) may be missed silently: only transversal hits are promised.  One RuntimeWarning when a ray
        carries a status bit (a ray in the plane of a flat cell, a ray that is not finite, a walk that hit a bound);
        ``bspy_amd.rays.cast_batch`` returns the status, the cell and the number of hits of every ray and, with
        hits="all", every hit.  ``_path="device"`` / ``"host"`` pins the path."""
        from . import rays as _rays
        return _rays.intersect_rays(self, origins, directions, tmin=tmin, tmax=tmax, **kwargs)

    def intersect_surface(self, other, depth=None, tolerance=None, **kwargs):
        """The curves along which this surface meets another one (the reference's ``intersect`` of two surfaces; both
        nInd 2, nDep 3, orders 2 .. 4, anything else raises NotImplementedError): a list of ``(curve_on_self,
        curve_on_other)``, one pair per connected piece.  Both curves (nInd 1, nDep 2, on [0, 1], order <= 4) are fitted to
        the same chord-length parameters of one polyline, so ``self(*ca(t))`` is ``other(*cb(t))`` up to the resolution of
        the lattice; a closed piece has equal end points.  Each surface carries 2^depth lattice lines per knot cell and
        variable (depth 0 .. 6; default 2, or chosen from ``tolerance``, which is also the tolerance of the fit) and every
        vertex is a hit of a lattice line of one surface on the other: a ``zeros3`` system that is formed in registers,
        never stored, and walked by one wave.  The curve is decided on the two lattices: a piece inside one product leaf
        is missed without a flag, tangential contact and coincident regions give a status bit at best, and nothing is
        certified; what is computed is stated in bspy_amd/surfaces.py.  One RuntimeWarning when a status bit is set
        (``bspy_amd.surfaces.trace_pair`` returns the raw polylines and the status).  Results are bitwise reproducible
        and the same on both paths.  ``_path="device"`` / ``"host"`` pins the path of the trace; the fit
        (``Spline.least_squares``) needs the device on either path, ``surfaces.trace_pair`` does not."""
        from . import surfaces as _surfaces
        return _surfaces.intersect_surface(self, other, depth=depth, tolerance=tolerance, **kwargs)

    def contours(self, tolerance=None, depth=None, **kwargs):
        """The level curves {f = 0} of a scalar spline in two variables (nInd == 2, nDep == 1; reference spline.py
        ``contours``, whose other shapes are not built): a list of curves (nInd 1, nDep 2, on [0, 1], order 4, f >= 0 on
        their left), one per connected piece, a closed piece with equal end points, and a tuple ((u0, v0), (u1, v1)) for
        every knot cell on which f vanishes; sorted by their first vertex.  Every knot cell is marched on a lattice of
        2^depth x 2^depth leaves (depth 0 .. 8; default 4, or chosen from ``tolerance``, which is also the tolerance of the
        fit): the contour is decided on that lattice, features smaller than a leaf are missed without a flag and nothing is
        certified; what is computed is stated in bspy_amd/contours.py.  Results are bitwise reproducible and the same on
        both paths.  ``_path="device"`` / ``"host"`` pins the path.  ``bspy_amd.contours.trace_batch`` traces many fields
        or many levels of one field in one launch sequence and returns the raw polylines."""
        from . import contours as _contours
        return _contours.contours(self, tolerance=tolerance, depth=depth, **kwargs)

    def isosurface(self, level=0.0, tolerance=None, depth=None, normals=False, **kwargs):
        """The level surface {f = level} of a scalar spline in three variables (nInd == 3, nDep == 1, orders 2 .. 4; the
        reference has nothing for it): (vertices (n, 3) float64, triangles (m, 3) int64), the vertices parameter values
        (u, v, w), every triangle's right-hand normal pointing into f >= level; with ``normals=True`` a third array (n, 3),
        the normalised gradient at every vertex (from ``jacobian``; NaN where it vanishes).  Every knot cell carries a
        lattice of 2^depth leaves per axis (depth 0 .. 6; default 3, or chosen from ``tolerance``), every leaf is cut into
        six tetrahedra, and the surface is decided on that lattice: features smaller than a leaf are missed without a flag
        and nothing is certified; what is computed is stated in bspy_amd/isosurface.py.  Where no lattice node value is
        exactly zero the mesh is a consistently oriented 2-manifold, closed but for the domain boundary and zero cells.
        Results are bitwise reproducible and the same on both paths.  ``_path="device"`` / ``"host"`` pins the path.
        ``bspy_amd.isosurface.extract_batch`` extracts many fields or many levels of one field in one launch sequence."""
        from . import isosurface as _isosurface
        return _isosurface.isosurface(self, level=level, tolerance=tolerance, depth=depth, normals=normals, **kwargs)

    def triangulate(self, tolerance, parameters=False, normals=False, **kwargs):
        """A watertight triangle mesh of a surface (nInd == 2, nDep 1 .. 3, orders 2 .. 4; the reference has this only in
        its viewer's tessellation shaders): (xyz (n, nDep) float64, triangles (m, 3) int64, counter-clockwise in (u, v)),
        then the parameters uv (n, 2) with ``parameters=True`` and the unit normals (n, 3) with ``normals=True`` (nDep 3).
        Every knot cell carries 2^a x 2^b grid quads, the levels taken from bounds of its second derivatives so that every
        point of every triangle is within ``tolerance`` of the surface point with the same parameters (plus the counted
        rounding slack of bspy_amd/mesh.py), and every cell edge takes the larger level of its two cells, so the triangles
        tile the domain without cracks or T-junctions.  ``max_level`` (default 8, at most 10) caps the levels: a cell that
        needs more is meshed at the cap with one RuntimeWarning.  ``max_triangles`` (default 2^28) raises a ValueError
        before the triangles are written.  ``metadata['negateNormal']`` flips the triangles and the normals.  Seams and
        poles are not welded.  Results are bitwise reproducible and the same on both paths.  ``_path="device"`` / ``"host"``
        pins the path.  ``bspy_amd.mesh.triangulate_batch`` meshes many nets on the same knots in one launch sequence."""
        from . import mesh as _mesh
        return _mesh.triangulate(self, tolerance, parameters=parameters, normals=normals, **kwargs)

    def __add__(self, other):
        return self.add(other, self._common(other)) if isinstance(other, Spline) else self.translate(other)

    def __radd__(self, other):
        return other.add(self, self._common(other)) if isinstance(other, Spline) else self.translate(other)

    def __sub__(self, other):
        if isinstance(other, Spline):
            return self.subtract(other, self._common(other))
        return self.translate(-np.atleast_1d(other))

    def __rsub__(self, other):
        if isinstance(other, Spline):
            return other.subtract(self, self._common(other))
        return self.scale(-1.0).translate(other)

    # NumPy must hand `array @ spline` and `array * spline` to the methods above instead of broadcasting over the spline
    __array_ufunc__ = None

    def tangent_space(self, uvw):
        """Same as jacobian (reference spline.py:2238-2252)."""
        return _ev.jacobian(self, uvw)

    def domain(self):
        """nInd x 2 array of parameter bounds (reference spline.py:794-808)."""
        return _ev.domain(self)

    # ------------------------------------------------------------------ persistence (input format)
    def to_dict(self):
        """`dict` with the spline's data (reference spline.py:2254-2267)."""
        return {"type": "Spline", "nInd": self.nInd, "nDep": self.nDep, "order": self.order, "nCoef": self.nCoef,
                "knots": self.knots, "coefs": self.coefs, "metadata": self.metadata}

    @staticmethod
    def from_dict(dictionary):
        """Spline from a `dict` as written by `to_dict` / the reference's files, including the
        legacy "flipNormal" metadata key (reference spline.py:1099-1125)."""
        d = dictionary
        meta = dict(d.get("metadata", {}))
        if meta.pop("flipNormal", False):              # legacy name of negateNormal
            meta["negateNormal"] = True
        return Spline(d["nInd"], d["nDep"], d["order"], d["nCoef"], [np.asarray(k) for k in d["knots"]],
                      np.asarray(d["coefs"]), meta)

    @staticmethod
    def load(fileName):
        """List of splines from a JSON file in the reference's format: one object or a list of
        objects, nested `coefs` of shape (nDep, *nCoef) (reference spline.py:1542-1583; the
        legacy .npz branch is not supported)."""
        import json
        with open(fileName, "r", encoding="utf-8") as stream:
            content = json.load(stream)
        records = [content] if isinstance(content, dict) else content
        return [Spline.from_dict(r) for r in records if r.get("type", "Spline") == "Spline"]

    def save(self, fileName, *additional_splines):
        """Write this spline (and more) as JSON in the reference's format (spline.py:1998-2026):
        one object, or a list when more splines are given; arrays as nested lists, indent 4."""
        import json

        def plain(value):
            if isinstance(value, Spline):
                return plain(value.to_dict())
            if isinstance(value, np.ndarray):
                return value.tolist()
            if isinstance(value, dict):
                return {k: plain(v) for k, v in value.items()}
            if isinstance(value, (list, tuple)):
                return [plain(v) for v in value]
            if isinstance(value, np.generic):
                return value.item()
            return value

        document = plain(self) if not additional_splines else [plain(s) for s in (self, *additional_splines)]
        with open(fileName, "w", encoding="utf-8") as stream:
            json.dump(document, stream, indent=4)

    # ------------------------------------------------------------------ device tables
    def device_tables(self, device=None):
        """The cached DeviceSpline of this spline (explicit pinning: hold on to it and call
        its *_device methods to skip the per-call checksum of knots/coefs)."""
        return _ev.device_tables(self, device)


def _isscalar(x):
    return np.isscalar(x)


def _ndim(x):
    return x.ndim if hasattr(x, "ndim") else np.ndim(x)
