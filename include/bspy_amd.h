/*
 * bspy_amd.h - C ABI of libbspy_amd.so: MI355X (gfx950) batched B-spline evaluation.
 *
 * The reference (ericbrec/BSpy 5.0.1) is pure Python and has no FFI of its own; its
 * boundary for this path is the Python API.  Each entry point
 * below names the reference interface it replaces (paths relative to the reference
 * checkout).  The reference-side binding a maintainer would add is the ctypes stub
 * shown in INTEGRATION.md; bspy_amd/_native.py is that stub in full.
 *
 * Conventions
 *  - plain C types only; no exceptions, no Python objects, no torch types.
 *  - every function returns a bsk_status (0 = ok).  bsk_last_error() returns a
 *    thread-local, human readable message for the last non-zero status.
 *  - dtype: BSK_F32 or BSK_F64.  It is the arithmetic type of the whole call:
 *    knots, coefficients, parameters and results all have it (the Python layer
 *    promotes mixed inputs, see bspy_amd/spline.py).
 *  - parameter points are SoA: one pointer per independent variable, each to n
 *    contiguous values.  Results are SoA: out[d * n + i] (evaluate/derivative),
 *    out[(d * nInd + j) * n + i] (jacobian).
 *  - mem: BSK_HOST buffers are copied to/from the device by the library (PCIe in the
 *    call); BSK_DEVICE buffers are device pointers on the spline's device and the call
 *    only enqueues work on `stream` (a hipStream_t, NULL = default stream).
 *  - the caller owns every buffer it passes; the library owns the device tables
 *    behind a bsk_spline handle.  Handles are not thread safe; distinct handles are
 *    independent.
 *  - a handle also owns scratch workspaces (jacobian rows of a non-fused normal, derivative passes of a
 *    non-fused curvature, grid basis rows, the cell-order pipeline's records).  They are shared by every call
 *    on the handle, so ONE handle is used from ONE stream at a time (create a second handle for a second
 *    stream).  A workspace grows (free + allocate) only when a call needs more than any call before it; such
 *    growth cannot be recorded by a stream capture and returns BSK_ERR_INVALID with a message saying so - run
 *    the call once outside the capture.  With that, every BSK_DEVICE call only enqueues kernels on `stream`
 *    (the cell-order pipeline of large tables sizes its workspace per batch and declines under capture: the
 *    call then runs the gather kernel).
 */
#ifndef BSPY_AMD_H
#define BSPY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSK_VERSION 1

#define BSK_MAX_NIND 8     /* independent variables per spline */
#define BSK_MAX_ORDER 16   /* polynomial order (degree + 1) per variable */

typedef enum { BSK_F32 = 0, BSK_F64 = 1 } bsk_dtype;
typedef enum { BSK_HOST = 0, BSK_DEVICE = 1 } bsk_mem;

typedef enum {
    BSK_OK = 0,
    BSK_ERR_INVALID = 1,      /* bad argument (message says which) */
    BSK_ERR_DOMAIN = 2,       /* a parameter lies outside the spline's domain; *first_bad = its flat index */
    BSK_ERR_HIP = 3,          /* HIP runtime failure */
    BSK_ERR_NO_DEVICE = 4,    /* no usable gfx950 device */
    BSK_ERR_UNSUPPORTED = 5   /* nInd / order beyond BSK_MAX_* */
} bsk_status;

typedef struct bsk_spline_s *bsk_spline;

/* Library / device information. */
int bsk_version(void);
const char *bsk_last_error(void);
bsk_status bsk_device_count(int *count);

/*
 * Spline handle = the device-resident tables of one reference `Spline` object.
 * Replaces: Spline.__init__ storage, bspy/spline.py:46-76 (validation stays in Python).
 *   knots[iv]  : order[iv] + nCoef[iv] values, non-decreasing
 *   coefs      : C-contiguous (nDep, nCoef[0], ..., nCoef[nInd-1])
 * The data is copied; bsk_spline_update re-uploads after the Python object's
 * knots/coefs were mutated (same shapes).
 */
bsk_status bsk_spline_create(bsk_dtype dtype, int device, int nInd, int nDep,
                             const int *order, const int *nCoef,
                             const void *const *knots, const void *coefs,
                             bsk_spline *out);
bsk_status bsk_spline_update(bsk_spline s, const void *const *knots, const void *coefs);
bsk_status bsk_spline_destroy(bsk_spline s);

/*
 * Batched evaluate / derivative.
 * Replaces: Spline.evaluate / Spline.derivative batched through np.frompyfunc,
 *   bspy/spline.py:936-949 and :757-770, i.e. one call of
 *   bspy/_spline_evaluation.py:140-164 (evaluate) / :109-133 (derivative) per point,
 *   including its span search and de Boor recursion (:4-27).
 *   wrt        : nInd derivative orders, or NULL for plain evaluation
 *   uvw[iv]    : n parameter values of variable iv
 *   out        : nDep * n results, out[d * n + i]
 *   first_bad  : (may be NULL) receives -1, or the index of the first point outside
 *                the inclusive domain [knots[order-1], knots[nCoef]] (status
 *                BSK_ERR_DOMAIN; the reference raises ValueError for that point,
 *                _spline_evaluation.py:148-152).  NaN parameters pass, as there.
 * With mem == BSK_DEVICE the call is asynchronous and never reports BSK_ERR_DOMAIN
 * itself: use bsk_domain_status() after the work was enqueued.
 */
bsk_status bsk_evaluate(bsk_spline s, const int *wrt, const void *const *uvw, int64_t n,
                        bsk_mem mem, void *out, void *stream, int64_t *first_bad);

/*
 * Batched jacobian: all first partial derivatives in one pass.
 * Replaces: Spline.jacobian / tangent_space, bspy/_spline_evaluation.py:205-213
 *   (nInd calls of derivative per point; single point only in the reference).
 *   out        : nDep * nInd * n results, out[(d * nInd + j) * n + i]
 */
bsk_status bsk_jacobian(bsk_spline s, const void *const *uvw, int64_t n,
                        bsk_mem mem, void *out, void *stream, int64_t *first_bad);

/*
 * Batched normal (next row of the scope table).
 * Replaces: Spline.normal, bspy/spline.py:1648-1682 -> bspy/_spline_evaluation.py:215-246
 *   (single point in the reference).  Needs |nInd - nDep| == 1 and max(nInd, nDep) <= 4.
 *   normalize  : unit length (the reference's default) or area-scaled cofactor vector
 *   negate     : the reference's metadata["negateNormal"]
 *   out        : max(nInd, nDep) * n values, out[i * n + p]
 */
bsk_status bsk_normal(bsk_spline s, const void *const *uvw, int64_t n, bsk_mem mem, int normalize, int negate,
                      void *out, void *stream, int64_t *first_bad);

/*
 * Batched curvature (next row).
 * Replaces: Spline.curvature, bspy/_spline_evaluation.py:80-107 (single point there).
 *   curves (nInd 1, nDep >= 2): signed curvature in 2-D, unsigned otherwise;
 *   surfaces in 3-D (nInd 2, nDep 3): Gaussian curvature.
 *   out : n values
 */
bsk_status bsk_curvature(bsk_spline s, const void *const *uvw, int64_t n, bsk_mem mem, void *out, void *stream,
                         int64_t *first_bad);

/*
 * Tensor-product grid evaluation: parameters are the outer product of per-variable
 * vectors (the reference's broadcast call s(u[:, None], v[None, :]), bspy/spline.py:941-945).
 *   grid[iv]   : ngrid[iv] values of variable iv
 *   out        : nDep * prod(ngrid) results, C order (d, i0, i1, ...)
 *   first_bad  : flat index into the broadcast shape (i0, i1, ...) of the first offender
 */
bsk_status bsk_evaluate_grid(bsk_spline s, const int *wrt, const void *const *grid, const int64_t *ngrid,
                             bsk_mem mem, void *out, void *stream, int64_t *first_bad);

/*
 * Tessellation of a BATCH of surface patches in 3-D on one parameter grid: positions and, optionally,
 * normals of every patch from one launch (next row).
 * Replaces: per patch the broadcast call s(u[:, None], v[None, :]) (bspy/spline.py:941-945) and
 *   Spline.normal at every grid point (bspy/spline.py:1648-1682 -> bspy/_spline_evaluation.py:215-246);
 *   it is the compute-side counterpart of the reference's GLSL tessellation shaders
 *   (bspy/splineOpenGLFrame.py:671-714), e.g. for the 32 patches of examples/teapot.py.
 *   splines    : count handles with nInd 2, nDep 3 that share dtype, device, orders, nCoef and knots
 *   grid[iv]   : ngrid[iv] values of variable iv (the grid is shared by all patches)
 *   positions  : count * 3 * n0 * n1 values, positions[((p * 3 + d) * n0 + i0) * n1 + i1]
 *   normals    : NULL, or the same shape: cross product of the two partial derivatives
 *                (normalize / negate as in bsk_normal)
 *   first_bad  : flat index i0 * n1 + i1 of the first grid point outside the domain
 */
bsk_status bsk_tessellate(const bsk_spline *splines, int count, const void *const *grid, const int64_t *ngrid,
                          bsk_mem mem, int normalize, int negate, void *positions, void *normals, void *stream,
                          int64_t *first_bad);

/*
 * One round of the adaptive quadrature behind Spline.integral: a tensor-product Gauss-Kronrod 7/15 rule over each
 * of nreg boxes ("regions"), each inside one knot cell.  The adaptive driver (which regions to split) is the caller's.
 * Replaces: the nested scipy.integrate.quad of composed_integral, bspy/_spline_evaluation.py:29-73 (bspy/spline.py:1249).
 *   The integrated measure is mu(u) = product of the singular values of the nDep x nInd jacobian:
 *   |det J| (nDep == nInd), sqrt(det(J^T J)) (nDep > nInd), sqrt(det(J J^T)) (nDep < nInd), determinants clamped at 0.
 *   mode    : BSK_INTEGRAL_MEASURE - out[2 r] = Kronrod sum K_r of mu, out[2 r + 1] = embedded Gauss sum G_r;
 *             BSK_INTEGRAL_NODES   - per node q of region r (15^nInd nodes, first variable slowest):
 *               out[(r * 15^nInd + q) * (nDep + 2) + d] = x_d (d < nDep), then wK * mu and wG * mu, the node's
 *               Kronrod / Gauss weight (box volume included, wG = 0 off the Gauss nodes) times the measure
 *   lo_hi   : nreg * nInd * 2 values in the spline's dtype, lo_hi[(r * nInd + iv) * 2 + {0, 1}] = bounds of region r
 *   span    : nreg * nInd span indices of the cell each region lies in ("rightmost knot of the segment":
 *             knots[iv][span - 1] <= lo < hi <= knots[iv][span], order <= span <= nCoef)
 *   out     : fp64 for both dtypes (fp32 splines evaluate their nodes in fp32 and sum in fp64)
 * Host buffers; the call synchronises `stream`.  Sums run in a fixed order (no atomics): bitwise reproducible.
 * nInd outside 1 - 3 returns BSK_ERR_UNSUPPORTED.
 */
typedef enum { BSK_INTEGRAL_MEASURE = 0, BSK_INTEGRAL_NODES = 1 } bsk_integral_mode;
bsk_status bsk_integral(bsk_spline s, int mode, const void *lo_hi, const int32_t *span, int64_t nreg, void *out,
                        void *stream);

/*
 * Least-squares fit of gridded data, one variable at a time (Spline.least_squares, bspy_amd/fitting.py).
 * Replaces: the dense matrix + numpy.linalg.lstsq of least_squares, bspy/_spline_fitting.py:736-770 (bspy/spline.py:1402).
 * A bsk_fit handle, the "plan", holds the banded QR of one collocation matrix A (nrows x ncols, `order` non-zeros per row):
 * row-sequential Givens rotations, recorded once on the host, then applied to any number of right-hand sides.
 *   first[r]   : column of the first non-zero of row r, non-decreasing, 0 <= first[r] <= ncols - order
 *   values     : nrows * order matrix entries, values[r * order + t] = A[r][first[r] + t]
 * bsk_fit_create makes no HIP call.  bsk_fit_info reports ncols, the rank indicator min |R_jj| / max |R_jj| (0 when R is
 * singular: the solve calls then return BSK_ERR_INVALID) and, when r_band is not NULL, the ncols * order band of R,
 * r_band[j * order + t] = R[j][j + t].  Any of the three pointers may be NULL.
 * The data of a solve is viewed as b[outer][nrows][inner] (dtype BSK_F32 or BSK_F64, computed in fp64); the result is
 * x[outer][ncols][inner], fp64: one "line" per (outer, inner) pair.
 *   bsk_fit_solve_host : host buffers, the plan applied on the CPU (few lines; also the statement of what the kernel
 *                        computes).  Any order up to BSK_MAX_ORDER.
 *   bsk_fit_sweep      : device buffers on the current device, kernels enqueued on `stream` (fit_sweep: one lane per
 *                        line; lines that are contiguous in memory, inner == 1, are turned through an LDS tile first).
 *                        Orders above 8 return BSK_ERR_UNSUPPORTED.  The plan's tables are uploaded by the first device
 *                        call; a workspace of the plan grows when a call needs more than any call before it.
 *   bsk_fit_residual   : device b and x as above; sumsq (host, nrows values) receives for every row the sum over all
 *                        lines of (b - A x)^2, summed in a fixed order (no atomics).  Synchronises `stream`.
 *   bsk_fit_last_kernel: "fit_sweep", "fit_sweep turned", "fit_residual", "fit_residual turned" or "host plan": the
 *                        path the most recent solve / residual call on this plan took.
 * A plan is used from one thread and one stream at a time.
 */
typedef struct bsk_fit_s *bsk_fit;
bsk_status bsk_fit_create(int nrows, int ncols, int order, const int32_t *first, const double *values, bsk_fit *out);
bsk_status bsk_fit_destroy(bsk_fit p);
bsk_status bsk_fit_info(bsk_fit p, int *ncols, double *rank_indicator, double *r_band);
bsk_status bsk_fit_solve_host(bsk_fit p, bsk_dtype dtype, const void *b, int64_t outer, int64_t inner, double *x);
bsk_status bsk_fit_sweep(bsk_fit p, bsk_dtype dtype, const void *b, int64_t outer, int64_t inner, double *x, void *stream);
bsk_status bsk_fit_residual(bsk_fit p, bsk_dtype dtype, const void *b, const double *x, int64_t outer, int64_t inner,
                            double *sumsq, void *stream);
const char *bsk_fit_last_kernel(bsk_fit p);

/*
 * Banded linear operators on coefficient tensors (Spline.insert_knots, elevate, elevate_and_insert_knots, trim, clamp,
 * differentiate; bspy_amd/refinement.py).
 * Replaces: the per-knot numpy.insert loop of insert_knots (bspy/_spline_domain.py:341), the derivative-and-integrate
 * elevation (:110), the slicing of trim (:610) and the coefficient loop of differentiate (bspy/_spline_operations.py:244).
 * A bsk_band handle holds one operator of one independent variable:
 *   out[j] = sum over t < K of w[j * K + t] * in[first[j] + t],   j < nOut
 *   first[j] : non-decreasing, 0 <= first[j] <= nIn - K
 * bsk_band_create copies first and w and makes no HIP call.  The data of a call is viewed as in[outer][nIn][inner]
 * (dtype BSK_F32 or BSK_F64); the result is out[outer][nOut][inner] in the same type.  The products of a row are added
 * in fp64 in the order t = 0 .. K - 1 and rounded once; there are no atomics, results are bitwise reproducible.
 *   bsk_band_apply_host : host buffers, the operator applied on the CPU (small tensors; also the statement of what the
 *                         kernels compute).  Any K up to BSK_MAX_ORDER.
 *   bsk_band_apply      : device buffers on the current device, one kernel enqueued on `stream`: band_apply (inner > 1,
 *                         lanes along inner) or band_apply_line (inner == 1, lines staged through LDS).  in and out must
 *                         not overlap.  K outside [2, 8] returns BSK_ERR_UNSUPPORTED.  The operator's tables are
 *                         uploaded by the first device call.
 *   bsk_band_last_kernel: "band_apply", "band_apply_line" or "host band": the path of the most recent call on this map.
 * A map is used from one thread and one stream at a time.
 */
typedef struct bsk_band_s *bsk_band;
bsk_status bsk_band_create(int nIn, int nOut, int K, const int32_t *first, const double *w, bsk_band *out);
bsk_status bsk_band_destroy(bsk_band p);
bsk_status bsk_band_apply_host(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out);
bsk_status bsk_band_apply(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out, void *stream);
const char *bsk_band_last_kernel(bsk_band p);

/*
 * Maxima of a band operator over all lines (Spline.remove_knots: the residual of every interior knot and the error
 * certificate of a removal; bspy_amd/reduction.py).
 * Replaces: the trial removal of one knot at a time on a folded spline, each a Givens solve in Python, of
 * bspy/_spline_domain.py:518.
 * The data is viewed as in[outer][nIn][inner] as for bsk_band_apply; `groups` divides `outer` and the group of a line is
 * the leading part of its outer index, g = o / (outer / groups).  minus is null or a buffer of the operator's result
 * shape [outer][nOut][inner] in the same dtype.  out[groups][nOut] is fp64:
 *   out[g][j] = max over the lines (o, i) of group g of | round_dtype(sum_t w[j][t] * in[o][first[j] + t][i]) - minus[o][j][i] |
 * The sum is the chain acc = fma(w[j][t], in[..], acc) from 0 in the order of t in fp64, rounded once to dtype; the
 * difference and the maximum are taken in fp64.  A NaN anywhere in a row's lines gives +inf for that row.  A maximum is
 * exact, so the result does not depend on the launch geometry and the host driver and the kernels give the same bits.
 *   bsk_band_absmax        : device buffers (in, minus, out) on the current device, two launches enqueued on `stream`:
 *                            band_absmax (inner > 1) or band_absmax_line (inner == 1) write one partial maximum per
 *                            (workgroup, group, row) into a workspace the handle owns, band_absmax_fold folds them.  No
 *                            atomics; no workgroup waits for another.  K outside [2, 8] returns BSK_ERR_UNSUPPORTED.
 *   bsk_band_absmax_host   : host buffers, the same values on the CPU, any K.
 *   bsk_band_apply_fma_host: bsk_band_apply_host with the sums formed as the fused chain above: the bits of
 *                            bsk_band_apply (bsk_band_apply_host rounds every product and can differ in the last bit).
 * bsk_band_last_kernel additionally reports "band_absmax", "band_absmax_line" or "host band_absmax".
 */
bsk_status bsk_band_absmax(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, int64_t groups,
                           const void *minus, double *out, void *stream);
bsk_status bsk_band_absmax_host(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, int64_t groups,
                                const void *minus, double *out);
bsk_status bsk_band_apply_fma_host(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out);

/*
 * Products of splines (Spline.multiply, dot, cross, scale by a spline, the * and @ operators; bspy_amd/product.py).
 * Replaces: multiplyAndConvolve's outer product over all variables followed by per-segment Taylor expansions
 * (bspy/_spline_operations.py:318).
 * A bsk_product handle holds, for each of M mapped pairs of variables (variable v: order k1[v], nIn1[v] coefficients
 * of the first spline; order k2[v], nIn2[v] coefficients of the second), one banded bilinear operator
 *   c[j] = sum over a < k1, b < k2 of W[(j * k1 + a) * k2 + b] * A[f[j] + a] * B[g[j] + b],   j < nOut[v]
 *   f, g : non-decreasing, 0 <= f[j] <= nIn1 - k1, 0 <= g[j] <= nIn2 - k2
 * The operator of several mapped variables is the tensor product of these.  bsk_product_create copies the tables and
 * makes no HIP call.
 * Data of a call (dtype BSK_F32 or BSK_F64, mapped variables last, contiguous):
 *   a[PA][nIn1[0]]..[nIn1[M-1]],  b[PB][nIn2[0]]..[nIn2[M-1]]  ->  out[P][nOut[0]]..[nOut[M-1]]
 *   terms : host array int32 [P][T][3]: output plane p is the sum over its T terms (planeA, planeB, sign = +1 / -1) of
 *           sign * product(a[planeA], b[planeB]).  The table carries the dependent-variable rule (scalar, dot, cross)
 *           and the unmapped variables of both splines.
 * Arithmetic: data widened to fp64, fp64 weights and accumulation, rounded once to dtype.  Per term and output the sums
 * run over the first mapped variable outermost, a before b; in the last variable V[b] = sum_a A[a] W[a][b] is formed
 * first and then sum_b V[b] B[b].  Terms are added in table order.  No atomics; results are bitwise reproducible.
 *   bsk_product_apply_host : host buffers, the sums above in plain C++, M = 1 .. 3, any order up to BSK_MAX_ORDER.
 *   bsk_product_apply      : device buffers on the current device, one kernel enqueued on `stream`:
 *                            band_product_line (M = 1) or band_product_tile (M = 2).  `terms` is a host array.  Orders of
 *                            the mapped variables outside [2, 6] or M > 2 return BSK_ERR_UNSUPPORTED.  out must not
 *                            overlap a or b.
 *   bsk_product_last_kernel: "band_product_line", "band_product_tile" or "host product".
 * A handle is used from one thread and one stream at a time.
 */
typedef struct bsk_product_s *bsk_product;
bsk_status bsk_product_create(int M, const int32_t *nIn1, const int32_t *nIn2, const int32_t *nOut, const int32_t *k1,
                              const int32_t *k2, const int32_t *const *f, const int32_t *const *g, const double *const *W,
                              bsk_product *out);
bsk_status bsk_product_destroy(bsk_product p);
bsk_status bsk_product_apply_host(bsk_product p, bsk_dtype dtype, const void *a, int64_t PA, const void *b, int64_t PB,
                                  const int32_t *terms, int64_t P, int T, void *out);
bsk_status bsk_product_apply(bsk_product p, bsk_dtype dtype, const void *a, int64_t PA, const void *b, int64_t PB,
                             const int32_t *terms, int64_t P, int T, void *out, void *stream);
const char *bsk_product_last_kernel(bsk_product p);

/*
 * Running sums and broadcast sums of coefficient tensors (Spline.integrate, add, subtract and the + and - operators;
 * bspy_amd/sums.py).
 * Replaces: the row-by-row coefficient loop of integrate (bspy/_spline_operations.py:290) and the zero-filled,
 * transposed in-place additions of add (:14).
 * A bsk_scan handle holds the weights g[0 .. n - 1] of one independent variable:
 *   out[0] = 0,   out[j + 1] = sum over i <= j of g[i] * in[i],   j < n
 * bsk_scan_create copies g and makes no HIP call.  The data of a call is viewed as in[outer][n][inner] (dtype BSK_F32
 * or BSK_F64); the result is out[outer][n + 1][inner] in the same type.  The association is one, for every path and
 * every launch geometry: each product g[i] * in[i] is rounded to fp64; rows are taken in chunks of 32; inside a chunk
 * the products are added left to right from 0; the chunk totals are added left to right from 0 into the chunk's carry;
 * an output is carry + the chunk's running sum, rounded once to dtype.  No atomics; results are bitwise reproducible
 * and the host driver and the kernels give the same bits.
 *   bsk_scan_apply_host : host buffers, the sums above in plain C++.
 *   bsk_scan_apply      : device buffers on the current device, enqueued on `stream`: scan_apply (inner > 1, lanes
 *                         along inner) or scan_line (inner == 1, tiles of lines staged through LDS).  A line is cut into
 *                         `segments` pieces of whole chunks (0: the library chooses; the count is rounded to what whole
 *                         chunks allow); more than one piece takes two launches: chunk totals into a workspace the
 *                         handle owns, then every workgroup forms its carry from the totals in front of it.  No
 *                         workgroup waits for another.  in and out must not overlap.
 *   bsk_scan_last_kernel: "scan_apply", "scan_line" or "host scan": the path of the most recent call on this map.
 * A map is used from one thread and one stream at a time.
 *
 * bsk_sum_apply(_host): out[idx] = a[idx . strideA] + sign * b[idx . strideB] over the contiguous result out of extents
 * dim[0 .. rank - 1], 1 <= rank <= 8 (BSK_ERR_UNSUPPORTED above: merge adjacent axes first).  Strides are in elements and
 * not negative; 0 broadcasts the operand along that axis.  sign is +1 or -1.  Both operands and the result have type
 * dtype; the sum is formed in fp64 and rounded once.
 *   bsk_sum_apply_host  : host buffers.
 *   bsk_sum_apply       : device buffers on the current device, one kernel (sum_bcast) enqueued on `stream`; out must not
 *                         overlap a or b.
 *   bsk_sum_last_kernel : "sum_bcast" or "host sum": the most recent call of this thread.
 */
typedef struct bsk_scan_s *bsk_scan;
bsk_status bsk_scan_create(int n, const double *g, bsk_scan *out);
bsk_status bsk_scan_destroy(bsk_scan p);
bsk_status bsk_scan_apply_host(bsk_scan p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out);
bsk_status bsk_scan_apply(bsk_scan p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out, int segments,
                          void *stream);
const char *bsk_scan_last_kernel(bsk_scan p);
bsk_status bsk_sum_apply_host(bsk_dtype dtype, int rank, const int64_t *dim, const void *a, const int64_t *strideA,
                              const void *b, const int64_t *strideB, int sign, void *out);
bsk_status bsk_sum_apply(bsk_dtype dtype, int rank, const int64_t *dim, const void *a, const int64_t *strideA, const void *b,
                         const int64_t *strideB, int sign, void *out, void *stream);
const char *bsk_sum_last_kernel(void);

/*
 * Real roots of scalar spline curves (Spline.zeros, bspy_amd.roots.zeros_batch; bspy_amd/roots.py).
 * Replaces: the recursive interval Newton iteration of bspy/_spline_intersection.py:12, which trims and reparametrizes
 * a spline object per step.
 * The caller brings every component to Bezier form first (one bsk_band_apply): rows[ncomp][rowlen] (dtype BSK_F32 or
 * BSK_F64) holds, for span s of the nspans knot spans, the `order` Bernstein coefficients of the piece on
 * [breaks[s], breaks[s + 1]] at rows[d][first[s] .. first[s] + order - 1].  mask[ncomp][nspans] (bytes): bit 0 the span
 * is skipped (it lies in a run of zero spans), bit 1 / bit 2 the span to the left / right is a zero span (a root within
 * `margin` of that end is dropped), bit 3 the last span (it owns the right end of the domain).
 * Arithmetic: fp64 whatever dtype, every product and sum rounded on its own; de Casteljau steps are
 * (1 - t) * a + t * b.  No atomics, no waiting between lanes; every loop has a compile-time bound.  Results are bitwise
 * reproducible and the host drivers and the kernels give the same bits.
 *   bsk_roots_flag(_host)   : flags[ncomp][nspans] (bytes) = the sign variations of the span's coefficients, zeros
 *                             skipped, + 1 for a first coefficient that is exactly 0, + 1 for a last coefficient that is
 *                             exactly 0 in the last span; 0 for a skipped span.  Device: one kernel (roots_flag), no LDS.
 *   bsk_roots_isolate(_host): cand[ncand] (int64, flat indices d * nspans + s of the spans to work on, ncand >= 1: no
 *                             candidates means no call); scale[ncomp] = max |coefficient| of the component.  Per
 *                             candidate the roots inside the span, ascending, go to roots[ncand][order - 1] (doubles, NaN
 *                             behind the last one) and their number to count[ncand] (int32): sub-intervals are halved
 *                             (at most 50 times) while their control polygon has two or more sign variations; one
 *                             variation is a bracket, refined by at most 60 bisection steps on the span's own
 *                             coefficients; two or more at the depth limit is a touching root, reported at the
 *                             midpoint when |f| <= 4 order eps scale there.  A root x in [0, 1] is returned as
 *                             breaks[s] + x * (breaks[s + 1] - breaks[s]).  Device: one kernel (roots_isolate), one lane
 *                             per candidate, registers only.
 *   The device entry points take device buffers on the current device (first, mask, breaks, scale, cand included) and
 *   enqueue on `stream`; orders 2 .. 8 (BSK_ERR_UNSUPPORTED above; the host drivers take orders up to BSK_MAX_ORDER).
 *   bsk_roots_extract_host  : the Bezier extraction of the host path: out[ncomp][nOut] from in[ncomp][nIn] (doubles) by the
 *                             band operator out[j] = sum_t w[j][t] * in[first[j] + t], t < K, formed as the chain
 *                             acc = fma(w[j][t], in[first[j] + t], acc) from 0 in the order of t.  This is what the band
 *                             kernels compute on the device (their sums are fused); bsk_band_apply_host rounds every
 *                             product, so its rows differ from theirs in the last bit and the roots would too.
 *   bsk_roots_last_kernel   : "roots_flag", "roots_isolate", "host roots_extract", "host roots_flag" or
 *                             "host roots_isolate": the most recent call of this thread.
 */
bsk_status bsk_roots_extract_host(int K, int64_t nIn, int64_t nOut, const int32_t *first, const double *w, const double *in,
                                  int64_t ncomp, double *out);
bsk_status bsk_roots_flag_host(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                               const int32_t *first, const uint8_t *mask, uint8_t *flags);
bsk_status bsk_roots_flag(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                          const int32_t *first, const uint8_t *mask, uint8_t *flags, void *stream);
bsk_status bsk_roots_isolate_host(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                                  const int32_t *first, const uint8_t *mask, const double *breaks, const double *scale,
                                  double margin, const int64_t *cand, int64_t ncand, double *roots, int32_t *count);
bsk_status bsk_roots_isolate(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                             const int32_t *first, const uint8_t *mask, const double *breaks, const double *scale,
                             double margin, const int64_t *cand, int64_t ncand, double *roots, int32_t *count, void *stream);
const char *bsk_roots_last_kernel(void);

/*
 * Isolated common zeros of two scalar splines in two variables (Spline.zeros2; the statement of what a zero is and of the
 * arithmetic is in bspy_amd/roots2.py and DESIGN.md section 17).  The family keeps no handle.  The caller brings both
 * variables to Bezier form with the band operator: rows[nsys][2][R0][R1] (doubles) holds nsys systems of two components
 * on the same knots, and cell (i, j), i < nc0, j < nc1, is the K0 x K1 window of both components at first0[i], first1[j];
 * it covers [breaks0[i], breaks0[i + 1]] x [breaks1[j], breaks1[j + 1]].  A cell's flat index is
 * (system * nc0 + i) * nc1 + j.  A window that leaves the rows, or a flat index that is no cell, gives no zero instead of
 * a read out of bounds.
 *   bsk_roots2_flag(_host)   : flags[nsys][nc0][nc1] (bytes) = 1 unless mask (same shape; a zero cell) is set or a
 *                              component's K0 K1 Bernstein coefficients are all > 0 or all < 0.
 *   bsk_roots2_isolate(_host): cand[ncand] (int64, flat indices of the flagged cells, ncand >= 1: no candidates means no
 *                              call); scale[nsys][2] = max |coefficient| of the component.  Per candidate: the zeros go to
 *                              roots[ncand][R][2] as (u, v), R = 2 (K0 - 1)(K1 - 1), NaN behind the last one; near[ncand][R]
 *                              (bytes) = 1 for a zero within 2^-20 of an edge of its cell; count[ncand] (int32);
 *                              status[ncand] (bytes): bit 1 = the walk visited more than its bound of nodes (zeros not
 *                              isolated), bit 2 = more than R zeros, bit 4 = a tangential or singular zero, not reported;
 *                              nodes[ncand] (int32) = the boxes the walk visited.  One lane per candidate walks the dyadic
 *                              boxes of the cell depth first without a stack, 24 halvings per axis, dropping a box when a
 *                              component's coefficients are strictly of one sign, and polishes a leaf with at most 8
 *                              Newton steps.
 *   bsk_roots2_merge(_host)  : which[nnear] (int64, flat indices candidate * R + slot of the zeros with near set,
 *                              nnear >= 1); table[nsys][nc0][nc1] (int64) = cumsum(flags) - 1, the candidate of a flagged
 *                              cell.  keep[ncand][R] (bytes): a lane clears its own byte when a neighbouring cell of the
 *                              same system with a lower flat index holds a zero within 2^-20 of the lane's cell widths on
 *                              both axes, and sets it otherwise; no other byte is written.
 *   The device entry points take device buffers on the current device and enqueue on `stream`; K0, K1 in 2 .. 4
 *   (BSK_ERR_UNSUPPORTED above; the host drivers take 2 .. 6).  No atomics, no waiting, every loop has a compile-time
 *   bound; the host drivers and the kernels give the same bits.
 *   bsk_roots2_last_kernel   : "roots2_flag", "roots2_isolate", "roots2_merge" or the same behind "host ".
 */
bsk_status bsk_roots2_flag_host(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                const int32_t *first0, const int32_t *first1, const uint8_t *mask, uint8_t *flags);
bsk_status bsk_roots2_flag(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                           const int32_t *first0, const int32_t *first1, const uint8_t *mask, uint8_t *flags, void *stream);
bsk_status bsk_roots2_isolate_host(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                   int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                                   const double *breaks1, const double *scale, const int64_t *cand, int64_t ncand, double *roots,
                                   uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes);
bsk_status bsk_roots2_isolate(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                              const int32_t *first0, const int32_t *first1, const double *breaks0, const double *breaks1,
                              const double *scale, const int64_t *cand, int64_t ncand, double *roots, uint8_t *near,
                              int32_t *count, uint8_t *status, int32_t *nodes, void *stream);
bsk_status bsk_roots2_merge_host(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, const double *breaks0,
                                 const double *breaks1, const int64_t *cand, int64_t ncand, const uint8_t *flags,
                                 const int64_t *table, const int64_t *which, int64_t nnear, uint8_t *keep);
bsk_status bsk_roots2_merge(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, const double *breaks0,
                            const double *breaks1, const int64_t *cand, int64_t ncand, const uint8_t *flags, const int64_t *table,
                            const int64_t *which, int64_t nnear, uint8_t *keep, void *stream);
const char *bsk_roots2_last_kernel(void);

/*
 * Ray-surface hits (Spline.intersect_rays, bspy_amd.rays.cast_batch; the statement of what a hit is and of the arithmetic is
 * in bspy_amd/rays.py and DESIGN.md section 22).  The family keeps no handle.  The caller brings the surface (nInd 2,
 * nDep 3) to Bezier form with the band operator: rows[3][R0][R1] (doubles), and cell (i, j), flat index i * nc1 + j, is
 * the K0 x K1 window of the three components at first0[i], first1[j]; it covers [breaks0[i], breaks0[i + 1]] x
 * [breaks1[j], breaks1[j + 1]].  Rays: origins[3][nrays], dirs[3][nrays] (doubles), cmax[3] = max |coefficient| per
 * component.  A hit of ray r is a common zero of g_k = n_k . (S - o), k = 1, 2, the two planes of the ray's frame; a
 * cell's coefficients of g_k are formed from the window and the ray, never stored.  A window that leaves the rows, or an
 * index that is no cell, no ray or no pair, gives no hit instead of an access out of bounds.
 *   bsk_rays_boxes(_host)  : boxes[nc0 * nc1][6] = min and max of the window per component (lo0, hi0, lo1, hi1, lo2, hi2).
 *   bsk_rays_count(_host)  : the cells in chunks of `chunk`, nchunks = ceil(cells / chunk) <= 65535; partial[nrays][nchunks]
 *                            (int32) = the pairs (ray, cell) of the chunk that pass the slab test against the box on
 *                            [tmin, tmax] (prefilter != 0) and are flat or not of one sign in g_1 or g_2; skipped[nrays]
 *                            (bytes) = 8 for a ray with a non-finite entry or a zero direction, which has no pairs.
 *   bsk_rays_emit(_host)   : the same search; offset[nrays][nchunks] (int64) = the exclusive sums of partial in that order;
 *                            pair_ray, pair_cell[npairs] (int32), npairs >= 1: a ray's pairs are contiguous, cells ascending.
 *   bsk_rays_isolate(_host): per pair the walk of bsk_roots2_isolate on the formed cell, with the ray's S_1, S_2 as the
 *                            scale: roots[npairs][R][2] as (u, v), R = 2 (K0 - 1)(K1 - 1), NaN behind the last one;
 *                            near[npairs][R], count, status, nodes[npairs] as there; status bit 16 = the ray lies in the
 *                            plane of a flat cell (all K0 K1 values of a g_k below S_k eps): not walked.
 *   bsk_rays_reduce(_host) : pstart[nrays + 1] (int64) = where a ray's pairs start.  Per ray: a root near an edge of its
 *                            cell is dropped when a pair of the same ray on a neighbouring cell with a lower flat index
 *                            holds one within 2^-20 of the cell widths; t = (S_c(u, v) - o_c) / d_c on the dominant axis c;
 *                            a hit has tmin <= t <= tmax.  all == 0: uv[2][nrays], t, cell (-1: no hit), hits[nrays]
 *                            (int32), status[nrays] (bytes, the OR of skipped and the pairs' status) of the hit of smallest
 *                            t; all != 0: every hit of ray r at hit_off[r] + n, n < hits[r], in (cell, slot) order:
 *                            uv[nhits][2], t, cell[nhits]; hits and status are not written.
 *   The device entry points take device buffers on the current device and enqueue on `stream`; K0, K1 in 2 .. 4
 *   (BSK_ERR_UNSUPPORTED above) on both sides.  No atomics, no waiting, no declared LDS; the host drivers and the kernels give
 *   the same bits.
 *   bsk_rays_last_kernel   : "ray_boxes", "ray_count", "ray_emit", "ray_isolate", "ray_reduce", "ray_reduce all" or the
 *                            same behind "host ".
 */
bsk_status bsk_rays_boxes_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                               const int32_t *first0, const int32_t *first1,
                               double *boxes);
bsk_status bsk_rays_boxes(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                          const int32_t *first0, const int32_t *first1,
                          double *boxes,
                          void *stream);
bsk_status bsk_rays_count_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                               const int32_t *first0, const int32_t *first1,
                               const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                               double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                               int32_t *partial, uint8_t *skipped);
bsk_status bsk_rays_count(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                          const int32_t *first0, const int32_t *first1,
                          const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                          double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                          int32_t *partial, uint8_t *skipped,
                          void *stream);
bsk_status bsk_rays_emit_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                              const int32_t *first0, const int32_t *first1,
                              const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                              double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                              const int64_t *offset, int32_t *pair_ray, int32_t *pair_cell, int64_t npairs);
bsk_status bsk_rays_emit(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                         const int32_t *first0, const int32_t *first1,
                         const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                         double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                         const int64_t *offset, int32_t *pair_ray, int32_t *pair_cell, int64_t npairs,
                         void *stream);
bsk_status bsk_rays_isolate_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                 const int32_t *first0, const int32_t *first1,
                                 const double *breaks0, const double *breaks1,
                                 const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                 const int32_t *pair_ray, const int32_t *pair_cell, int64_t npairs, double *roots, uint8_t *near,
                                 int32_t *count, uint8_t *status, int32_t *nodes);
bsk_status bsk_rays_isolate(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                            const int32_t *first0, const int32_t *first1,
                            const double *breaks0, const double *breaks1,
                            const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                            const int32_t *pair_ray, const int32_t *pair_cell, int64_t npairs, double *roots, uint8_t *near,
                            int32_t *count, uint8_t *status, int32_t *nodes,
                            void *stream);
bsk_status bsk_rays_reduce_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                const int32_t *first0, const int32_t *first1,
                                const double *breaks0, const double *breaks1,
                                const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                double tmin, double tmax, const int64_t *pstart, const int32_t *pair_cell, int64_t npairs,
                                const double *roots, const uint8_t *near, const int32_t *count, const uint8_t *pstatus,
                                const uint8_t *skipped, int all, const int64_t *hit_off, int64_t nhits, double *uv, double *t,
                                int32_t *cell, int32_t *hits, uint8_t *status);
bsk_status bsk_rays_reduce(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                           const int32_t *first0, const int32_t *first1,
                           const double *breaks0, const double *breaks1,
                           const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                           double tmin, double tmax, const int64_t *pstart, const int32_t *pair_cell, int64_t npairs,
                           const double *roots, const uint8_t *near, const int32_t *count, const uint8_t *pstatus,
                           const uint8_t *skipped, int all, const int64_t *hit_off, int64_t nhits, double *uv, double *t,
                           int32_t *cell, int32_t *hits, uint8_t *status,
                           void *stream);
const char *bsk_rays_last_kernel(void);

/*
 * Surface-surface intersection (Spline.intersect_surface, bspy_amd.surfaces.trace_pair; the statement is in
 * bspy_amd/surfaces.py and DESIGN.md section 23).  The family keeps no handle.  Both surfaces (nInd 2, nDep 3) are brought
 * to Bezier form as for bsk_rays_*: X is (KX0, KX1, rowsX[3][RX0][RX1], ncX0, ncX1, firstX0, firstX1), Y likewise.  A call
 * serves one family of lattice lines: the lines of X with variable `ax` (0 or 1) fixed, G = 2^depth per knot cell
 * (1 <= G <= 64), against the cells of Y.  Line n, 0 <= n <= nc_ax G, is owned by cell c = min(n / G, nc_ax - 1) at the
 * local value (n - c G) / G; its segment on running cell e has the index n * ncrun + e, ncrun the cells of the other
 * variable, and is a Bezier curve of KR points (KR the order of the running variable).  The pair (segment, cell (p, q) of
 * Y) is the three-variable system with the Bernstein coefficients L_i - Y_jk, formed where it is needed and never stored.
 * scale[3] = max |coefficient of X| + max |coefficient of Y| per component.  An index that is no segment, no cell or no
 * pair, or a window that leaves the rows, gives nothing instead of an access out of bounds.
 *   bsk_ssx_count(_host)  : the segments seg0 .. seg0 + nseg - 1 against Y's cells in chunks of `chunk`, nchunks =
 *                           ceil(cells / chunk) <= 65535; boxes = bsk_rays_boxes of Y.  partial[nseg][nchunks] (int32) =
 *                           the pairs of the chunk that are flat (the boxes of the segment's points and of the cell are
 *                           not strictly disjoint and a component is below scale eps on the whole pair) or not strictly
 *                           of one sign in any component.  prefilter != 0 drops a pair with strictly disjoint boxes
 *                           before its window is read: the same result.
 *   bsk_ssx_emit(_host)   : the same search; offset[nseg][nchunks] (int64) = the exclusive sums of partial in that order;
 *                           pair_seg (the segment's index in the family), pair_cell[npairs] (int32), npairs >= 1, sorted by
 *                           (segment, cell).
 *   bsk_ssx_isolate(_host): per pair the walk of bsk_roots3_isolate on the formed system, one wave a pair:
 *                           roots[npairs][R][3] as (w, s, t), w the running parameter of X, (s, t) Y's;
 *                           R = min(6 (KR - 1)(KY0 - 1)(KY1 - 1), 32); near, count, status, nodes as there; status bit
 *                           16 = a flat pair: not walked.
 *   bsk_ssx_merge(_host)  : pair_key[npairs] (int64, ascending) = segment * ncY0 * ncY1 + cell over all pairs of the family;
 *                           which[nnear] = the flat indices (pair, slot) of the zeros with near set.  keep[npairs][R]
 *                           (bytes) of such a zero becomes 0 when one of the 13 pairs of the same line that precede it in
 *                           (e, p, q) holds a zero within 2^-20 of the cell widths on all three axes.
 *   The device entry points take device buffers on the current device and enqueue on `stream`; orders 2 .. 4
 *   (BSK_ERR_UNSUPPORTED above).  No atomics, no waiting, no LDS; the host drivers and the kernels give the same bits.
 *   bsk_ssx_last_kernel   : "ssx_count", "ssx_emit", "ssx_isolate", "ssx_merge" or the same behind "host ".
 */
bsk_status bsk_ssx_count_host(int KX0, int KX1, const double *rowsX, int64_t RX0, int64_t RX1, int64_t ncX0, int64_t ncX1,
                              const int32_t *firstX0, const int32_t *firstX1,
                              int KY0, int KY1, const double *rowsY, int64_t RY0, int64_t RY1, int64_t ncY0, int64_t ncY1,
                              const int32_t *firstY0, const int32_t *firstY1, int ax, int64_t G,
                              int64_t seg0, int64_t nseg, int64_t chunk, int prefilter, const double *boxes, const double *scale,
                              int32_t *partial);
bsk_status bsk_ssx_count(int KX0, int KX1, const double *rowsX, int64_t RX0, int64_t RX1, int64_t ncX0, int64_t ncX1,
                         const int32_t *firstX0, const int32_t *firstX1,
                         int KY0, int KY1, const double *rowsY, int64_t RY0, int64_t RY1, int64_t ncY0, int64_t ncY1,
                         const int32_t *firstY0, const int32_t *firstY1, int ax, int64_t G,
                         int64_t seg0, int64_t nseg, int64_t chunk, int prefilter, const double *boxes, const double *scale,
                         int32_t *partial,
                         void *stream);
bsk_status bsk_ssx_emit_host(int KX0, int KX1, const double *rowsX, int64_t RX0, int64_t RX1, int64_t ncX0, int64_t ncX1,
                             const int32_t *firstX0, const int32_t *firstX1,
                             int KY0, int KY1, const double *rowsY, int64_t RY0, int64_t RY1, int64_t ncY0, int64_t ncY1,
                             const int32_t *firstY0, const int32_t *firstY1, int ax, int64_t G,
                             int64_t seg0, int64_t nseg, int64_t chunk, int prefilter, const double *boxes, const double *scale,
                             const int64_t *offset, int32_t *pair_seg, int32_t *pair_cell, int64_t npairs);
bsk_status bsk_ssx_emit(int KX0, int KX1, const double *rowsX, int64_t RX0, int64_t RX1, int64_t ncX0, int64_t ncX1,
                        const int32_t *firstX0, const int32_t *firstX1,
                        int KY0, int KY1, const double *rowsY, int64_t RY0, int64_t RY1, int64_t ncY0, int64_t ncY1,
                        const int32_t *firstY0, const int32_t *firstY1, int ax, int64_t G,
                        int64_t seg0, int64_t nseg, int64_t chunk, int prefilter, const double *boxes, const double *scale,
                        const int64_t *offset, int32_t *pair_seg, int32_t *pair_cell, int64_t npairs,
                        void *stream);
bsk_status bsk_ssx_isolate_host(int KX0, int KX1, const double *rowsX, int64_t RX0, int64_t RX1, int64_t ncX0, int64_t ncX1,
                                const int32_t *firstX0, const int32_t *firstX1,
                                int KY0, int KY1, const double *rowsY, int64_t RY0, int64_t RY1, int64_t ncY0, int64_t ncY1,
                                const int32_t *firstY0, const int32_t *firstY1, int ax, int64_t G,
                                const double *breaks_run, const double *breaksY0, const double *breaksY1, const double *scale,
                                const int32_t *pair_seg, const int32_t *pair_cell, int64_t npairs, double *roots, uint8_t *near,
                                int32_t *count, uint8_t *status, int32_t *nodes);
bsk_status bsk_ssx_isolate(int KX0, int KX1, const double *rowsX, int64_t RX0, int64_t RX1, int64_t ncX0, int64_t ncX1,
                           const int32_t *firstX0, const int32_t *firstX1,
                           int KY0, int KY1, const double *rowsY, int64_t RY0, int64_t RY1, int64_t ncY0, int64_t ncY1,
                           const int32_t *firstY0, const int32_t *firstY1, int ax, int64_t G,
                           const double *breaks_run, const double *breaksY0, const double *breaksY1, const double *scale,
                           const int32_t *pair_seg, const int32_t *pair_cell, int64_t npairs, double *roots, uint8_t *near,
                           int32_t *count, uint8_t *status, int32_t *nodes,
                           void *stream);
bsk_status bsk_ssx_merge_host(int R, const double *roots, int64_t ncrun, int64_t ncY0, int64_t ncY1, const double *breaks_run,
                              const double *breaksY0, const double *breaksY1, const int64_t *pair_key, int64_t npairs,
                              const int64_t *which, int64_t nnear, uint8_t *keep);
bsk_status bsk_ssx_merge(int R, const double *roots, int64_t ncrun, int64_t ncY0, int64_t ncY1, const double *breaks_run,
                         const double *breaksY0, const double *breaksY1, const int64_t *pair_key, int64_t npairs,
                         const int64_t *which, int64_t nnear, uint8_t *keep,
                         void *stream);
const char *bsk_ssx_last_kernel(void);

/*
 * Isolated common zeros of three scalar splines in three variables (Spline.zeros3; the statement of what a zero is and of
 * the arithmetic is in bspy_amd/roots3.py and DESIGN.md section 19).  The family keeps no handle.  The caller brings the
 * three variables to Bezier form with the band operator: rows[nsys][3][R0][R1][R2] (doubles) holds nsys systems of three
 * components on the same knots, and cell (i, j, k) is the K0 x K1 x K2 window of the components at first0[i], first1[j],
 * first2[k]; it covers [breaks0[i], breaks0[i + 1]] x [breaks1[j], breaks1[j + 1]] x [breaks2[k], breaks2[k + 1]].  A
 * cell's flat index is ((system * nc0 + i) * nc1 + j) * nc2 + k.  A window that leaves the rows, or a flat index that is
 * no cell, gives no zero instead of a read out of bounds.
 *   bsk_roots3_flag(_host)   : flags[nsys][nc0][nc1][nc2] (bytes) = 1 unless mask (same shape; a zero cell) is set or a
 *                              component's K0 K1 K2 Bernstein coefficients are all > 0 or all < 0.
 *   bsk_roots3_isolate(_host): cand[ncand] (int64, flat indices of the flagged cells, 1 <= ncand < 2^31: no candidates
 *                              means no call); scale[nsys][3] = max |coefficient| of the component.  Per candidate: the
 *                              zeros go to roots[ncand][R][3] as (u, v, w), R = min(6 (K0 - 1)(K1 - 1)(K2 - 1), 32), NaN
 *                              behind the last one; near[ncand][R] (bytes) = 1 for a zero within 2^-20 of a face of its
 *                              cell; count[ncand] (int32); status[ncand] (bytes): bit 1 = the walk visited more than its
 *                              bound of nodes (zeros not isolated), bit 2 = more than R zeros, bit 4 = a tangential or
 *                              singular zero, not reported; nodes[ncand] (int32) = the boxes the walk visited.  One wave
 *                              (a workgroup of 64 lanes, lane = coefficient of the window) per candidate walks the dyadic
 *                              boxes of the cell depth first without a stack, 19 halvings per axis, dropping a box when a
 *                              component's coefficients are strictly of one sign, and polishes a leaf with at most 8
 *                              Newton steps.
 *   bsk_roots3_merge(_host)  : which[nnear] (int64, flat indices candidate * R + slot of the zeros with near set,
 *                              nnear >= 1); table[nsys][nc0][nc1][nc2] (int64) = cumsum(flags) - 1, the candidate of a
 *                              flagged cell.  keep[ncand][R] (bytes): a lane clears its own byte when one of the 13
 *                              neighbouring cells of the same system with a lower flat index holds a zero within 2^-20 of
 *                              the lane's cell widths on all axes, and sets it otherwise; no other byte is written.
 *   The device entry points take device buffers on the current device and enqueue on `stream`; K0, K1, K2 in 2 .. 4 on
 *   both sides (BSK_ERR_UNSUPPORTED above).  No atomics, no waiting, no LDS, every loop has a compile-time bound; the host
 *   drivers and the kernels give the same bits.
 *   bsk_roots3_last_kernel   : "roots3_flag", "roots3_isolate", "roots3_merge" or the same behind "host ".
 *   bsk_roots3_walk_bound    : the number of nodes a walk may visit before status bit 1 is set, as compiled.
 */
bsk_status bsk_roots3_flag_host(int K0, int K1, int K2, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t R2,
                                int64_t nc0, int64_t nc1, int64_t nc2, const int32_t *first0, const int32_t *first1,
                                const int32_t *first2, const uint8_t *mask, uint8_t *flags);
bsk_status bsk_roots3_flag(int K0, int K1, int K2, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t R2,
                           int64_t nc0, int64_t nc1, int64_t nc2, const int32_t *first0, const int32_t *first1,
                           const int32_t *first2, const uint8_t *mask, uint8_t *flags, void *stream);
bsk_status bsk_roots3_isolate_host(int K0, int K1, int K2, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t R2,
                                   int64_t nc0, int64_t nc1, int64_t nc2, const int32_t *first0, const int32_t *first1,
                                   const int32_t *first2, const double *breaks0, const double *breaks1, const double *breaks2,
                                   const double *scale, const int64_t *cand, int64_t ncand, double *roots, uint8_t *near,
                                   int32_t *count, uint8_t *status, int32_t *nodes);
bsk_status bsk_roots3_isolate(int K0, int K1, int K2, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t R2,
                              int64_t nc0, int64_t nc1, int64_t nc2, const int32_t *first0, const int32_t *first1,
                              const int32_t *first2, const double *breaks0, const double *breaks1, const double *breaks2,
                              const double *scale, const int64_t *cand, int64_t ncand, double *roots, uint8_t *near,
                              int32_t *count, uint8_t *status, int32_t *nodes, void *stream);
bsk_status bsk_roots3_merge_host(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, int64_t nc2,
                                 const double *breaks0, const double *breaks1, const double *breaks2, const int64_t *cand,
                                 int64_t ncand, const uint8_t *flags, const int64_t *table, const int64_t *which, int64_t nnear,
                                 uint8_t *keep);
bsk_status bsk_roots3_merge(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, int64_t nc2,
                            const double *breaks0, const double *breaks1, const double *breaks2, const int64_t *cand,
                            int64_t ncand, const uint8_t *flags, const int64_t *table, const int64_t *which, int64_t nnear,
                            uint8_t *keep, void *stream);
const char *bsk_roots3_last_kernel(void);
int bsk_roots3_walk_bound(void);

/*
 * Closest points on curves and surfaces (Spline.project; the statement of the seed, of the Newton iteration and of the
 * arithmetic is in bspy_amd/project.py and DESIGN.md section 20).  The family keeps no handle.  The caller brings every
 * variable to Bezier form with the band operator: rows[ndep][R0][R1] (doubles; a curve has R1 = K1 = nc1 = g1 = 1,
 * first1 = {0} and breaks1 = {0, 1}), cell (i, j) is the K0 x K1 window of every component at first0[i], first1[j] and
 * covers [breaks0[i], breaks0[i + 1]] x [breaks1[j], breaks1[j + 1]].  One more band step per variable gives the sample
 * grid samples[ndep][nsamples], nsamples = (nc0 g0)(nc1 g1): flat sample (i g0 + a)(nc1 g1) + (j g1 + b) lies at the local
 * coordinates ((a + 1/2) / g0, (b + 1/2) / g1) of cell (i, j).  points[ndep][npts] are the query points.
 *   seed   : the samples are cut into nchunks = ceil(nsamples / chunk) ranges of `chunk` samples, nchunks <= 65535.
 *            part_d2[nchunks][npts] (doubles) and part_idx[nchunks][npts] (int32) receive, per point and range, the
 *            smallest squared distance (summed in component order, every product and sum rounded on its own) and the flat
 *            index of the first sample that has it; +inf and -1 where no sample's squared distance is below +inf (a point
 *            with a NaN or an infinite coordinate).
 *   newton : per point the partials are reduced in range order by the same rule (guess == NULL), or the start is
 *            guess[nind][npts] clamped to the domain.  Then Newton on |S(u) - p|^2 / 2 as project.newton_point states it.
 *            uvw[nind][npts] and distance[npts] (doubles), status[npts] (bytes: 1 evaluation bound reached, 2 foot point
 *            on a domain bound, 4 singular step or a window that leaves the rows, 8 point not finite or no seed:
 *            not iterated, NaN out) and steps[npts] (int32, evaluations made).
 *   nind = 1: K0 in 2 .. 6, K1 = 1; nind = 2: K0, K1 in 2 .. 4; ndep = 2 or 3; anything else is BSK_ERR_UNSUPPORTED.
 *   The device entry points take device buffers on the current device and enqueue on `stream`.  No atomics, no waiting,
 *   every loop has a compile-time or launch-uniform bound; the host drivers and the kernels give the same bits.
 *   The name of the last call: "project_seed", "project_newton" or the same behind "host ".
 */
bsk_status bsk_project_seed_host(int ndep, const double *samples, int64_t nsamples, const double *points, int64_t npts,
                                 int64_t chunk, double *part_d2, int32_t *part_idx);
bsk_status bsk_project_seed(int ndep, const double *samples, int64_t nsamples, const double *points, int64_t npts, int64_t chunk,
                            double *part_d2, int32_t *part_idx, void *stream);
bsk_status bsk_project_newton_host(int nind, int K0, int K1, int ndep, const double *rows, int64_t R0, int64_t R1, int64_t nc0,
                                   int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                                   const double *breaks1, int g0, int g1, const double *points, int64_t npts,
                                   const double *part_d2, const int32_t *part_idx, int64_t nchunks, const double *guess,
                                   double *uvw, double *distance, uint8_t *status, int32_t *steps);
bsk_status bsk_project_newton(int nind, int K0, int K1, int ndep, const double *rows, int64_t R0, int64_t R1, int64_t nc0,
                              int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                              const double *breaks1, int g0, int g1, const double *points, int64_t npts, const double *part_d2,
                              const int32_t *part_idx, int64_t nchunks, const double *guess, double *uvw, double *distance,
                              uint8_t *status, int32_t *steps, void *stream);
const char *bsk_project_last_kernel(void);

/*
 * Level curves {f = 0} of scalar splines in two variables (Spline.contours; the statement of the lattice, the vertices
 * and the arithmetic is in bspy_amd/contours.py and DESIGN.md section 21).  The family keeps no handle.  The caller brings
 * both variables to Bezier form with the band operator: rows[nrows][R0][R1] (doubles), cell (i, j), i < nc0, j < nc1, is
 * the K0 x K1 window at first0[i], first1[j] and covers [breaks0[i], breaks0[i + 1]] x [breaks1[j], breaks1[j + 1]]; no
 * knot is a jump, so adjacent cells share their end row or column.  There are nfields fields: field b is rows[b]
 * (levels NULL, nrows == nfields) or rows[0] - levels[b] (nrows == 1); scale[nfields] = max |coefficient| of the field.
 * A cell's flat index is (field * nc0 + i) * nc1 + j.  A window that leaves the rows, or a flat index that is no cell,
 * gives no segment instead of a read out of bounds.
 *   bsk_contour_flag(_host) : zero[nfields][nc0][nc1] (bytes) = 1 where every coefficient of the cell is below scale eps;
 *                             cand (same shape) = 1 unless the cell is a zero cell or its coefficients are all above tau
 *                             or all below -tau, tau = 32 (K0 + K1) eps scale.
 *   bsk_contour_march(_host): cand[ncand] (int64, flat indices of the flagged cells, ncand >= 1).  Every cell carries
 *                             2^depth x 2^depth leaves, depth in 0 .. 8; lane = candidate * 4^split + top box, split in
 *                             0 .. depth.  emit == 0: counts[lanes] (int32) = the segments of the lane, lane_status[lanes]
 *                             (bytes): bit 1 = a leaf with four crossings.  emit != 0: offsets[lanes] (int64, the
 *                             exclusive sum of counts), total = the sum (>= 1: no segments means no call); segment n is
 *                             keys[n][2] (int64 lattice-edge keys of its two vertices, f >= 0 on the left from the first to
 *                             the second) and xy[n][4] = (u, v) of both.  Pointers of the other pass may be NULL.
 *   The device entry points take device buffers on the current device and enqueue on `stream`; K0, K1 in 2 .. 4
 *   (BSK_ERR_UNSUPPORTED above).  No atomics, no waiting, every loop has a compile-time bound; the host drivers and the
 *   kernels give the same bits, and the segments do not depend on split.
 *   bsk_contour_last_kernel : "contour_flag", "contour_march count", "contour_march emit" or the same behind "host ".
 */
bsk_status bsk_contour_flag_host(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                 int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                 int64_t nfields, const double *scale, uint8_t *cand, uint8_t *zero);
bsk_status bsk_contour_flag(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                            const int32_t *first0, const int32_t *first1, const double *levels, int64_t nfields,
                            const double *scale, uint8_t *cand, uint8_t *zero, void *stream);
bsk_status bsk_contour_march_host(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                  int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                  int64_t nfields, const double *scale, const double *breaks0, const double *breaks1,
                                  const int64_t *cand, int64_t ncand, int depth, int split, int emit, const int64_t *offsets,
                                  int64_t total, int32_t *counts, uint8_t *lane_status, int64_t *keys, double *xy);
bsk_status bsk_contour_march(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                             const int32_t *first0, const int32_t *first1, const double *levels, int64_t nfields,
                             const double *scale, const double *breaks0, const double *breaks1, const int64_t *cand,
                             int64_t ncand, int depth, int split, int emit, const int64_t *offsets, int64_t total,
                             int32_t *counts, uint8_t *lane_status, int64_t *keys, double *xy, void *stream);
const char *bsk_contour_last_kernel(void);

/*
 * Level surfaces {f = 0} of scalar splines in three variables (Spline.isosurface; the statement of the lattice, the
 * tetrahedra, the vertices and the arithmetic is in bspy_amd/isosurface.py and DESIGN.md section 25).  The family keeps no
 * handle.  The caller brings the three variables to Bezier form with the band operator: rows[nrows][R0][R1][R2] (doubles),
 * cell (i, j, k) is the K0 x K1 x K2 window at first0[i], first1[j], first2[k] and covers [breaks0[i], breaks0[i + 1]] x
 * [breaks1[j], breaks1[j + 1]] x [breaks2[k], breaks2[k + 1]]; no knot is a jump, so adjacent cells share their end plane.
 * There are nfields fields: field b is rows[b] (levels NULL, nrows == nfields) or rows[0] - levels[b] (nrows == 1);
 * scale[nfields] = max |coefficient| of the field.  A cell's flat index is ((field * nc0 + i) * nc1 + j) * nc2 + k; every
 * cell carries 2^depth leaves per axis, depth in 0 .. 6, and a leaf's flat index is ((field * NL0 + I) * NL1 + J) * NL2 + K
 * with NL = nc << depth.  A window that leaves the rows, or an index that is no cell, leaf or lattice edge, gives nothing
 * (a vertex: NaN) instead of a read out of bounds.
 *   bsk_iso_flag(_host)   : zero[nfields][nc0][nc1][nc2] (bytes) = 1 where every coefficient of the cell is below scale eps;
 *                           cand (same shape) = 1 unless the cell is a zero cell or its coefficients are all above tau or
 *                           all below -tau, tau = 32 (K0 + K1 + K2) eps scale.
 *   bsk_iso_walk(_host)   : cand[ncand] (int64, flat indices of the flagged cells, ncand >= 1); wave = candidate * 8^split +
 *                           top box, split in 0 .. depth.  emit == 0: counts[waves] (int32) = the leaves of the wave's box
 *                           that the sign test keeps.  emit != 0: offsets[waves] (int64, the exclusive sum of counts),
 *                           total = the sum (>= 1), leaves[total] (int64) = their flat indices in the order of the walk.
 *   bsk_iso_leaf(_host)   : leaves[nleaves] (int64, ascending).  emit == 0: counts[nleaves] (int32) = the triangles of the
 *                           leaf, and status[nfields][nc0][nc1][nc2] (bytes, zeroed by the caller) = 2 on the cell of a
 *                           leaf with a node value of exactly 0.0.  emit != 0: offsets[nleaves], total (>= 1) and
 *                           tris[total][3] (int64) = the lattice-edge keys of the triangles' vertices, the right-hand
 *                           normal into f >= 0.  Pointers of the other pass may be NULL.
 *   bsk_iso_vertex(_host) : keys[n], fields[n] (int64) -> xyz[n][3] = (u, v, w) of the crossed lattice edge.
 *   The device entry points take device buffers on the current device and enqueue on `stream`; K0, K1, K2 in 2 .. 4
 *   (BSK_ERR_UNSUPPORTED above).  No atomics, no waiting, every loop has a compile-time bound; the host drivers and the
 *   kernels give the same bits, and the triangles do not depend on split.
 *   bsk_iso_last_kernel   : "iso_flag", "iso_walk count", "iso_walk emit", "iso_leaf count", "iso_leaf emit", "iso_vertex"
 *                           or the same behind "host ".
 */
#define BSK_ISO_GRID                                                                                                          \
    int K0, int K1, int K2, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t R2, int64_t nc0, int64_t nc1,   \
        int64_t nc2, const int32_t *first0, const int32_t *first1, const int32_t *first2, const double *levels,               \
        int64_t nfields, const double *scale
bsk_status bsk_iso_flag_host(BSK_ISO_GRID, uint8_t *cand, uint8_t *zero);
bsk_status bsk_iso_flag(BSK_ISO_GRID, uint8_t *cand, uint8_t *zero, void *stream);
bsk_status bsk_iso_walk_host(BSK_ISO_GRID, const int64_t *cand, int64_t ncand, int depth, int split, int emit,
                             const int64_t *offsets, int64_t total, int32_t *counts, int64_t *leaves);
bsk_status bsk_iso_walk(BSK_ISO_GRID, const int64_t *cand, int64_t ncand, int depth, int split, int emit, const int64_t *offsets,
                        int64_t total, int32_t *counts, int64_t *leaves, void *stream);
bsk_status bsk_iso_leaf_host(BSK_ISO_GRID, const int64_t *leaves, int64_t nleaves, int depth, int emit, const int64_t *offsets,
                             int64_t total, int32_t *counts, uint8_t *status, int64_t *tris);
bsk_status bsk_iso_leaf(BSK_ISO_GRID, const int64_t *leaves, int64_t nleaves, int depth, int emit, const int64_t *offsets,
                        int64_t total, int32_t *counts, uint8_t *status, int64_t *tris, void *stream);
bsk_status bsk_iso_vertex_host(BSK_ISO_GRID, const double *breaks0, const double *breaks1, const double *breaks2,
                               const int64_t *keys, const int64_t *fields, int64_t n, int depth, double *xyz);
bsk_status bsk_iso_vertex(BSK_ISO_GRID, const double *breaks0, const double *breaks1, const double *breaks2, const int64_t *keys,
                          const int64_t *fields, int64_t n, int depth, double *xyz, void *stream);
#undef BSK_ISO_GRID
const char *bsk_iso_last_kernel(void);

/*
 * Triangle meshes of parametric surfaces within a tolerance (Spline.triangulate; the statement of the bounds, the levels,
 * the keys, the triangles and the vertices is in bspy_amd/mesh.py and DESIGN.md section 26).  The family keeps no handle.
 * The caller brings the two variables to Bezier form with the band operator: rows[nmem][ndep][R0][R1] (doubles, ndep in
 * 1 .. 3), cell (i, j) is the K0 x K1 window at first0[i], first1[j] and covers [breaks0[i], breaks0[i + 1]] x
 * [breaks1[j], breaks1[j + 1]].  A window that leaves the rows, or an index that is no cell, quad or key, gives nothing (a
 * vertex: NaN) instead of a read out of bounds.
 *   bsk_mesh_bound(_host) : per (member, cell): Q[.][3] = (Quu, Qvv, Quv), the squared bounds of the second derivatives
 *                           in the cell's own parameters; lev[.][2] (int32) = (a, b), the least levels in 0 .. max_level
 *                           (<= 10) with max(Quu, Quv) <= T 16^a and max(Qvv, Quv) <= T 16^b; status[.] (bytes) = 1
 *                           where there is none (the level is max_level then).  T = (2 tolerance)^2.
 *   bsk_mesh_count(_host) : qoff[ncells + 1] (int64) = the exclusive sums of 2^(a + b), ncells = nmem nc0 nc1; 2^steps >=
 *                           ncells; span >= 2^(the largest difference of two levels).  For the quads start .. start + n - 1
 *                           of nquads = qoff[ncells]: counts[quad] (int32) = 2, or the segments on its four sides.
 *   bsk_mesh_emit(_host)  : offsets[nquads] (int64, the exclusive sums of counts), total (>= 1), tris[total][3] (int64) =
 *                           the keys of the triangles' vertices, counter-clockwise in (u, v); key = (X << 31) | Y,
 *                           X = (i << 11) + the local coordinate in units of 2^-11 of the cell.
 *   bsk_mesh_vertex(_host): keys[n], members[n] (int64) -> uv[n][2], xyz[n][ndep] and, unless NULL (ndep 3 only),
 *                           normals[n][3] = S_u x S_v in the cell's own parameters, not normalised.
 *   The device entry points take device buffers on the current device and enqueue on `stream`; K0, K1 in 2 .. 4
 *   (BSK_ERR_UNSUPPORTED above).  No atomics, no waiting, no LDS, every loop has a compile-time or launch-uniform bound; the
 *   host drivers and the kernels give the same bits.
 *   bsk_mesh_last_kernel  : "mesh_bound", "mesh_count", "mesh_emit", "mesh_vertex" or the same behind "host ".
 */
#define BSK_MESH_NET                                                                                                          \
    int K0, int K1, const double *rows, int64_t nmem, int ndep, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,             \
        const int32_t *first0, const int32_t *first1
#define BSK_MESH_QUADS                                                                                                        \
    const int64_t *qoff, int64_t ncells, int64_t nc0, int64_t nc1, const int32_t *lev, int steps, int span, int64_t start,    \
        int64_t n, int64_t nquads
bsk_status bsk_mesh_bound_host(BSK_MESH_NET, double T, int max_level, double *Q, int32_t *lev, uint8_t *status);
bsk_status bsk_mesh_bound(BSK_MESH_NET, double T, int max_level, double *Q, int32_t *lev, uint8_t *status, void *stream);
bsk_status bsk_mesh_count_host(BSK_MESH_QUADS, int32_t *counts);
bsk_status bsk_mesh_count(BSK_MESH_QUADS, int32_t *counts, void *stream);
bsk_status bsk_mesh_emit_host(BSK_MESH_QUADS, const int64_t *offsets, int64_t total, int64_t *tris);
bsk_status bsk_mesh_emit(BSK_MESH_QUADS, const int64_t *offsets, int64_t total, int64_t *tris, void *stream);
bsk_status bsk_mesh_vertex_host(BSK_MESH_NET, const double *breaks0, const double *breaks1, const int64_t *keys,
                                const int64_t *members, int64_t n, double *uv, double *xyz, double *normals);
bsk_status bsk_mesh_vertex(BSK_MESH_NET, const double *breaks0, const double *breaks1, const int64_t *keys, const int64_t *members,
                           int64_t n, double *uv, double *xyz, double *normals, void *stream);
#undef BSK_MESH_NET
#undef BSK_MESH_QUADS
const char *bsk_mesh_last_kernel(void);

/*
 * Scattered least squares (Spline.fit_points; the statement of the key, the units, the Gram slabs, the trees, the fold
 * and the solve is in bspy_amd/scatter.py and DESIGN.md section 24).  The family keeps no handle.  Variable d has order
 * K_d, n_d coefficients and the n_d + K_d knots knots_d (doubles); a curve has nind = 1, K1 = n1 = 1, knots1 = {0, 1} and
 * top1 = 0.  Knot cell (c0, c1), c_d in 0 .. n_d - K_d, is the span c_d + K_d - 1; its flat index is c0 nc1 + c1,
 * nc_d = n_d - K_d + 1.  top_d is the last span of positive width.  uvw[nind][npts], points[ndep][npts], weights[npts]
 * or NULL (doubles).
 *   key      : key_out[npts] (int64) = the flat cell of the point, the last span whose left knot is <= u per variable
 *              (the right domain end belongs to span top); -1 and status[npts] (bytes) != 0 for an excluded point:
 *              1 a parameter outside the domain, 2 a parameter, coordinate or weight that is NaN or infinite,
 *              4 a negative weight.
 *   gram     : order[npts] (int64) is the stable sort of the points by key, offsets[ncells + 1] where the cells start in
 *              it.  A cell's points are cut into units of 256 points: unit_cell[nunits], unit_start[ncells] (the first
 *              unit of a cell).  slabs[nunits][K][K + ndep], K = K0 K1: row a = a0 K1 + a1 holds sum w B_a B_b, b < K,
 *              then sum w B_a p_d, summed as scatter.gram_unit states it.
 *   cell     : one level of the adjacent-pairs tree over the nodes of a cell, 16 to a node: out[nnodes][entries], node g
 *              of cell node_cell[g] is its node g - out_start[cell] and sums the inputs in_start[cell] + 16 k ..., at
 *              most in_count[cell] in all; no inputs: zeros.
 *   fold     : cells[ncells][K][K + ndep] -> stencil[n0 n1][2 K0 - 1][2 K1 - 1] (entry (i, j), j - i = (d0, d1) at
 *              [i][d0 + K0 - 1][d1 + K1 - 1]; 0 where j is no coefficient) and rhs[n0 n1][ndep]: per entry the cells that
 *              hold both coefficients, in increasing flat index; entry (a, b) of a slab is read with a <= b.
 *   residual : residual_out[npts] = |S(u) - p| for coefs[ndep][n0][n1], NaN where key_in is -1.
 *   solve    : host only.  The stencil of a symmetric positive definite matrix goes to upper band storage of half
 *              bandwidth (K0 - 1) n1 + K1 - 1 (at most 2^27 doubles) and is solved by a banded Cholesky factorisation:
 *              coefs[ndep][n0 n1].  A pivot that is not positive: *bad_row = its row, BSK_ERR_INVALID.
 *   The kernels cover K0, K1 in 2 .. 4 and ndep 1 .. 4 (gram) and K0, K1 in 2 .. 4 (residual), the host twins orders
 *   2 .. 6 and any ndep; anything else is BSK_ERR_UNSUPPORTED.  The device entry points take device buffers on the
 *   current device and enqueue on `stream`.  No atomics, no waiting; the host drivers and the kernels give the same bits.
 *   solve (device) : the twin of solve_host for ndep 1 .. 4 and half bandwidths hb = min((K0 - 1) n1 + K1 - 1, n - 1) up to
 *              4095 (anything else is BSK_ERR_UNSUPPORTED and stays with solve_host): stencil, rhs, coefs[ndep][n], work
 *              and the one int64 bad_row are device buffers; work holds at least the doubles that bsk_scatter_solve_work
 *              reports (2 n (hb + 1) + ndep n) and needs no contents.  The call enqueues launches and returns; coefs are
 *              the bytes of solve_host, and *bad_row is -1 or the first row whose pivot is not > 0 (coefs then hold
 *              nothing of use).
 *   reweight : the robust weights of a reweighted fit.  loss 0 (Huber): r <= s ? w0 : w0 (s / r); loss 1 (Tukey):
 *              r < s ? w0 (q q), q = 1 - (r / s)(r / s) : 0; r = residual[i], w0 = weights[i] (1.0 for NULL), s =
 *              threshold > 0; a point with key_in[i] < 0 keeps w0.
 *   The name of the last call: "scatter_key", "scatter_gram", "scatter_cell", "scatter_fold", "scatter_residual",
 *   "scatter_reweight" or the same behind "host ", or "host scatter_solve", or "scatter_solve".
 */
bsk_status bsk_scatter_key_host(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points,
                                const double *weights, int64_t npts, int64_t *key_out, uint8_t *status);
bsk_status bsk_scatter_key(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                           int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points, const double *weights,
                           int64_t npts, int64_t *key_out, uint8_t *status, void *stream);
bsk_status bsk_scatter_gram_host(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                 int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points,
                                 const double *weights, int64_t npts, const int64_t *order, const int64_t *offsets,
                                 const int64_t *unit_cell, const int64_t *unit_start, int64_t nunits, double *slabs);
bsk_status bsk_scatter_gram(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                            int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points, const double *weights,
                            int64_t npts, const int64_t *order, const int64_t *offsets, const int64_t *unit_cell,
                            const int64_t *unit_start, int64_t nunits, double *slabs, void *stream);
bsk_status bsk_scatter_cell_host(int64_t entries, const double *in, const int64_t *in_start, const int64_t *in_count,
                                 const int64_t *node_cell, const int64_t *out_start, int64_t nnodes, double *out);
bsk_status bsk_scatter_cell(int64_t entries, const double *in, const int64_t *in_start, const int64_t *in_count,
                            const int64_t *node_cell, const int64_t *out_start, int64_t nnodes, double *out, void *stream);
bsk_status bsk_scatter_fold_host(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *cells, double *stencil,
                                 double *rhs);
bsk_status bsk_scatter_fold(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *cells, double *stencil,
                            double *rhs, void *stream);
bsk_status bsk_scatter_residual_host(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                     int64_t top0, int64_t top1, int ndep, const double *coefs, const double *uvw,
                                     const double *points, const int64_t *key_in, int64_t npts, double *residual_out);
bsk_status bsk_scatter_residual(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                int64_t top0, int64_t top1, int ndep, const double *coefs, const double *uvw, const double *points,
                                const int64_t *key_in, int64_t npts, double *residual_out, void *stream);
bsk_status bsk_scatter_solve_host(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *stencil,
                                  const double *rhs, double *coefs, int64_t *bad_row);
/* the device solve and the robust weights (the parameter lists start on a line of their own) */
bsk_status bsk_scatter_solve_work(
    int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, int64_t *doubles);
bsk_status bsk_scatter_solve(
    int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *stencil, const double *rhs, double *coefs,
    double *work, int64_t work_doubles, int64_t *bad_row, void *stream);
bsk_status bsk_scatter_reweight_host(
    int loss, double threshold, const double *residual, const double *weights, const int64_t *key_in, int64_t npts,
    double *weights_out);
bsk_status bsk_scatter_reweight(
    int loss, double threshold, const double *residual, const double *weights, const int64_t *key_in, int64_t npts,
    double *weights_out, void *stream);
const char *bsk_scatter_last_kernel(void);

/*
 * Synchronise `stream` and report whether any BSK_DEVICE call on this handle since the
 * last bsk_domain_status() met an out-of-domain parameter (*first_bad = smallest such
 * index, else -1).  Resets the record.
 */
bsk_status bsk_domain_status(bsk_spline s, void *stream, int64_t *first_bad);

/*
 * Batched B-spline basis values (no spline object).
 * Replaces: Spline.bspline_values, bspy/spline.py:207-252 -> bspy/_spline_evaluation.py:4-27.
 *   knot_in    : NULL to search the span of every u (reference: knot=None), else n
 *                explicit span indices
 *   ix_out     : n span indices ("rightmost knot of the segment")
 *   basis_out  : n * order values, basis_out[i * order + k] multiplies coefficient
 *                ix_out[i] - order + k
 * Host buffers only (this is the low-rate public helper; the evaluation kernels have
 * the same recursion fused in).
 */
bsk_status bsk_bspline_values(bsk_dtype dtype, int device, const void *knots, int nknots, int order,
                              const void *u, int64_t n, int derivative_order, int taylor_coefs,
                              const int32_t *knot_in, int32_t *ix_out, void *basis_out);

/*
 * Multi-device evaluation in ONE process (north_star: "sharding the evaluation-point batch with an RCCL
 * all-gather of results"; the reference has no multi-device code).  A bsk_multi holds one
 * replica of the spline tables and one stream per device.  A call cuts the n points into contiguous shards
 * of ceil(n / ndev) points (bsk_multi_shard_plan: start[d] .. start[d + 1]), evaluates every shard on its
 * device through bsk_evaluate / bsk_jacobian, and exchanges results only on request:
 *   mem == BSK_HOST    uvw[iv] = n host values; out[0] = host (rows, n); every device copies its shard over
 *                      its own PCIe link; `gather` is ignored (the host holds the whole result).
 *   mem == BSK_DEVICE  uvw[d * nInd + iv] = device d's shard of variable iv (on device d);
 *     gather == 0      out[d] = device d's compact (rows, shard) block: no collective at all.
 *     gather != 0      out[d] = (rows, ndev * chunk) on device d, chunk = ceil(n / ndev): every device
 *                      receives every shard - one grouped RCCL exchange (ncclGroupStart, one ncclAllGather
 *                      per device and row, ncclGroupEnd); columns >= n of the last chunk are padding.
 *                      librccl.so is opened on first use; BSK_ERR_UNSUPPORTED when it cannot be loaded.
 *   rows = nDep (evaluate / derivative) or nDep * nInd (jacobian).
 *   first_bad = global index of the first out-of-domain point (BSK_ERR_DOMAIN), else -1.  The call returns
 *   when every device has finished.
 */
typedef struct bsk_multi_s *bsk_multi;
bsk_status bsk_multi_create(bsk_dtype dtype, int ndev, const int *devices /* NULL = 0 .. ndev-1 */, int nInd, int nDep,
                            const int *order, const int *nCoef, const void *const *knots, const void *coefs,
                            bsk_multi *out);
bsk_status bsk_multi_destroy(bsk_multi m);
bsk_status bsk_multi_shard_plan(bsk_multi m, int64_t n, int64_t *start /* ndev + 1 entries */);
bsk_status bsk_multi_stream(bsk_multi m, int d, void **stream /* hipStream_t of device slot d */);
bsk_status bsk_multi_evaluate(bsk_multi m, const int *wrt, const void *const *uvw, int64_t n, bsk_mem mem,
                              void *const *out, int gather, int64_t *first_bad);
bsk_status bsk_multi_jacobian(bsk_multi m, const void *const *uvw, int64_t n, bsk_mem mem, void *const *out,
                              int gather, int64_t *first_bad);

/*
 * Diagnostics (no reference counterpart; used by bench.py, tools/ and the tests).
 *   bsk_last_kernel : family name of the kernel the most recent point call on this handle launched
 *                     ("eval_uni", "eval_rowrot", "eval_stream", "cell-order pipeline (...)", ...), so
 *                     that measurements and tests name the kernel that actually ran.  bsk_evaluate_grid records its
 *                     grid kernel ("grid_rows", "grid_surface", "grid_generic"); bsk_tessellate records the form of
 *                     tess_rows it launched on the first patch's handle ("tess_rows hoisted 512", "tess_rows hoisted
 *                     256", "tess_rows normals", "tess_rows mixed", "tess_rows columns").
 */
const char *bsk_last_kernel(bsk_spline s);

/*
 * BSK_INTERNAL: measurement hooks of this repository's bench.py / tools/.  They are exported by the library but are
 * NOT part of the product ABI (no reference counterpart, no stability promise): a binding of the reference never
 * needs them, and they are only declared when the including file asks for them.
 *   bsk_debug_probe       : memory-side floor of the LDS-resident kernels' launch geometry: streams two fp64
 *                           parameter arrays in and three result arrays out with trivial arithmetic
 *                           (mode 0: 8 B per lane per access, mode 1: 16 B), `blocks_per_cu` workgroups of
 *                           `threads` lanes per CU with `lds_bytes` of LDS allocated.  tools/probe_stream.py.
 *   bsk_debug_stage_times : per-kernel durations of the cell-order pipeline (HIP events between its kernels on the
 *                           call's stream).  enable != 0 records the FOLLOWING calls on this handle; a call with
 *                           ms / names / count returns the stages of the last recorded call (names are static
 *                           strings, at most `cap` entries).
 *   bsk_debug_fill_lds    : LDS contents for the stale-LDS tests: 8 workgroups per CU of 1024 lanes, each with the whole
 *                           LDS of a CU.  mode 0 writes `pattern` over it; mode 1 (positive control) reads it without
 *                           writing it and adds the words that differ from `pattern` to *mismatches.  Synchronises
 *                           `stream` before it returns.
 *   bsk_debug_scatter_solve : bsk_scatter_solve stage by stage for tools/scatter_time.py: `stages` is a sum of 1 (the band
 *                           expansion), 2 (the factorisation), 4 (the forward substitution), 8 (the backward one).
 */
#ifdef BSK_INTERNAL
bsk_status bsk_debug_probe(bsk_spline s, int mode, int blocks_per_cu, int threads, int64_t lds_bytes,
                           const void *u, const void *v, int64_t n, void *out, void *stream);
bsk_status bsk_debug_stage_times(bsk_spline s, int enable, float *ms, const char **names, int cap, int *count);
bsk_status bsk_debug_fill_lds(bsk_spline s, uint32_t pattern, int mode, int64_t *mismatches, void *stream);
bsk_status bsk_debug_scatter_solve(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *stencil,
                                   const double *rhs, double *coefs, double *work, int64_t work_doubles, int64_t *bad_row,
                                   int stages, void *stream);
#endif

#ifdef __cplusplus
}
#endif
#endif /* BSPY_AMD_H */
