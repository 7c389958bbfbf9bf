// Spline.least_squares on the device (bsk_fit.hpp): the bsk_fit_* entry points.  The plan (banded Givens QR) is host
// work and makes no HIP call; its tables go to the device with the first device call on the handle.
// Instantiations: fit_sweep fp32 / fp64 input x order 1 - 8, fit_transpose and fit_residual fp32 / fp64 input.
#include "bsk_host.hpp"
#include "bsk_fit.hpp"

using namespace bskfit;

struct bsk_fit_s {
    FitPlan plan;
    int device = -1;                   // device the tables live on (-1: not uploaded)
    DevBuf d_first, d_avals, d_rot, d_R;
    DevBuf ws_in, ws_out, ws_part;     // turned copies of contiguous lines, residual partial sums
    const char *last_kernel = "";
};

static bsk_status upload(bsk_fit p)
{
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (p->device == dev) return BSK_OK;
    if (p->device >= 0) return fail(BSK_ERR_INVALID, "bsk_fit: the plan's tables live on another device");
    const FitPlan &q = p->plan;
    HIPCHK(p->d_first.reserve(sizeof(int) * q.first.size()));
    HIPCHK(p->d_avals.reserve(sizeof(double) * q.avals.size()));
    HIPCHK(p->d_rot.reserve(sizeof(double) * q.rot.size()));
    HIPCHK(p->d_R.reserve(sizeof(double) * q.R.size()));
    HIPCHK(hipMemcpy(p->d_first.p, q.first.data(), sizeof(int) * q.first.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_avals.p, q.avals.data(), sizeof(double) * q.avals.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_rot.p, q.rot.data(), sizeof(double) * q.rot.size(), hipMemcpyHostToDevice));
    std::vector<double> Rd(q.R);           // the kernel multiplies by 1 / R_jj
    for (int j = 0; j < q.ncols; ++j) Rd[(size_t)j * q.k] = 1.0 / Rd[(size_t)j * q.k];
    HIPCHK(hipMemcpy(p->d_R.p, Rd.data(), sizeof(double) * Rd.size(), hipMemcpyHostToDevice));
    p->device = dev;
    return BSK_OK;
}

static bsk_status check_shape(bsk_fit p, int64_t outer, int64_t inner, const char *who)
{
    if (!p) return fail(BSK_ERR_INVALID, std::string(who) + ": plan is NULL");
    if (outer < 1 || inner < 1) return fail(BSK_ERR_INVALID, std::string(who) + ": outer and inner must be >= 1");
    const double cells = (double)outer * (double)inner * (double)std::max(p->plan.nrows, p->plan.ncols);
    if (cells > 9.0e15) return fail(BSK_ERR_INVALID, std::string(who) + ": array too large");
    if ((double)outer * (double)inner > 1.0e11) return fail(BSK_ERR_INVALID, std::string(who) + ": too many lines");
    return BSK_OK;
}

template <typename TIN, int K>
static void launch_sweep(bsk_fit p, const TIN *b, double *x, long long inner, long long nlines, hipStream_t st)
{
    const unsigned grid = (unsigned)((nlines + FIT_BLOCK - 1) / FIT_BLOCK);
    hipLaunchKernelGGL((fit_sweep<TIN, K>), dim3(grid), dim3(FIT_BLOCK), 0, st, b, x,
                       static_cast<const double2 *>(p->d_rot.p), static_cast<const int *>(p->d_first.p),
                       static_cast<const double *>(p->d_R.p), p->plan.nrows, p->plan.ncols, inner, nlines);
}

template <typename TIN>
static void launch_sweep_k(bsk_fit p, const TIN *b, double *x, long long inner, long long nlines, hipStream_t st)
{
    switch (p->plan.k) {
    case 1: launch_sweep<TIN, 1>(p, b, x, inner, nlines, st); break;
    case 2: launch_sweep<TIN, 2>(p, b, x, inner, nlines, st); break;
    case 3: launch_sweep<TIN, 3>(p, b, x, inner, nlines, st); break;
    case 4: launch_sweep<TIN, 4>(p, b, x, inner, nlines, st); break;
    case 5: launch_sweep<TIN, 5>(p, b, x, inner, nlines, st); break;
    case 6: launch_sweep<TIN, 6>(p, b, x, inner, nlines, st); break;
    case 7: launch_sweep<TIN, 7>(p, b, x, inner, nlines, st); break;
    default: launch_sweep<TIN, 8>(p, b, x, inner, nlines, st); break;
    }
}

template <typename TIN>
static bsk_status transpose(const TIN *in, double *out, long long R, long long C, hipStream_t st)
{
    const long long tiles_c = (C + FIT_TILE - 1) / FIT_TILE, tiles_r = (R + FIT_TILE - 1) / FIT_TILE;
    if (tiles_c * tiles_r > 0x7fffffffLL) return fail(BSK_ERR_INVALID, "bsk_fit: array too large for fit_transpose");
    hipLaunchKernelGGL((fit_transpose<TIN>), dim3((unsigned)(tiles_c * tiles_r)), dim3(FIT_TILE, 8), 0, st, in, out, R, C,
                       tiles_c);
    HIPCHK(hipGetLastError());
    return BSK_OK;
}

template <typename TIN>
static bsk_status run_sweep(bsk_fit p, const TIN *b, long long outer, long long inner, double *x, hipStream_t st)
{
    const FitPlan &q = p->plan;
    const long long nlines = outer * inner;
    if ((nlines + FIT_BLOCK - 1) / FIT_BLOCK > 0x7fffffffLL) return fail(BSK_ERR_INVALID, "bsk_fit_sweep: too many lines");
    if (inner == 1 && outer > 1) {
        // contiguous lines: turn [lines, nrows] so that lanes run along the lines, sweep, turn the result back
        HIPCHK(p->ws_in.reserve(sizeof(double) * (size_t)nlines * q.nrows));
        HIPCHK(p->ws_out.reserve(sizeof(double) * (size_t)nlines * q.ncols));
        double *bt = static_cast<double *>(p->ws_in.p), *xt = static_cast<double *>(p->ws_out.p);
        bsk_status s = transpose<TIN>(b, bt, nlines, q.nrows, st);
        if (s != BSK_OK) return s;
        launch_sweep_k<double>(p, bt, xt, nlines, nlines, st);
        HIPCHK(hipGetLastError());
        s = transpose<double>(xt, x, q.ncols, nlines, st);
        if (s != BSK_OK) return s;
        p->last_kernel = "fit_sweep turned";
    } else {
        launch_sweep_k<TIN>(p, b, x, inner, nlines, st);
        HIPCHK(hipGetLastError());
        p->last_kernel = "fit_sweep";
    }
    return BSK_OK;
}

template <typename TIN>
static bsk_status run_residual(bsk_fit p, const TIN *b, const double *x, long long outer, long long inner, double *sumsq,
                               hipStream_t st)
{
    const FitPlan &q = p->plan;
    const long long nlines = outer * inner;
    const long long per = (long long)RES_BLOCK * RES_PER_LANE, nchunks = (nlines + per - 1) / per;
    if (nchunks * q.nrows > 0x7fffffffLL) return fail(BSK_ERR_INVALID, "bsk_fit_residual: too many rows x lines");
    const size_t part_off = (sizeof(double) * (size_t)q.nrows + 255) & ~(size_t)255;
    HIPCHK(p->ws_part.reserve(part_off + sizeof(double) * (size_t)nchunks * q.nrows));
    double *dsum = static_cast<double *>(p->ws_part.p);
    double *part = reinterpret_cast<double *>(static_cast<char *>(p->ws_part.p) + part_off);
    const int *first = static_cast<const int *>(p->d_first.p);
    const double *avals = static_cast<const double *>(p->d_avals.p);
    const unsigned grid = (unsigned)(nchunks * q.nrows);
    if (inner == 1 && outer > 1) {
        HIPCHK(p->ws_in.reserve(sizeof(double) * (size_t)nlines * q.nrows));
        HIPCHK(p->ws_out.reserve(sizeof(double) * (size_t)nlines * q.ncols));
        double *bt = static_cast<double *>(p->ws_in.p), *xt = static_cast<double *>(p->ws_out.p);
        bsk_status s = transpose<TIN>(b, bt, nlines, q.nrows, st);
        if (s != BSK_OK) return s;
        s = transpose<double>(x, xt, nlines, q.ncols, st);
        if (s != BSK_OK) return s;
        hipLaunchKernelGGL((fit_residual<double>), dim3(grid), dim3(RES_BLOCK), 0, st, bt, xt, avals, first, q.k, q.nrows,
                           q.ncols, nlines, nlines, nchunks, part);
        p->last_kernel = "fit_residual turned";
    } else {
        hipLaunchKernelGGL((fit_residual<TIN>), dim3(grid), dim3(RES_BLOCK), 0, st, b, x, avals, first, q.k, q.nrows,
                           q.ncols, inner, nlines, nchunks, part);
        p->last_kernel = "fit_residual";
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fit_residual_rows, dim3((unsigned)((q.nrows + 255) / 256)), dim3(256), 0, st, part, nchunks, q.nrows,
                       dsum);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sumsq, dsum, sizeof(double) * (size_t)q.nrows, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return BSK_OK;
}

extern "C" bsk_status bsk_fit_create(int nrows, int ncols, int order, const int32_t *first, const double *values,
                                     bsk_fit *out)
{
    if (!first || !values || !out) return fail(BSK_ERR_INVALID, "NULL argument");
    if (order < 1 || order > MAXO) return fail(BSK_ERR_UNSUPPORTED, "bsk_fit_create: order must be in [1, BSK_MAX_ORDER]");
    if (ncols < order) return fail(BSK_ERR_INVALID, "bsk_fit_create: fewer columns than the order");
    if (nrows < 1 || nrows > (1 << 26) || ncols > (1 << 26)) return fail(BSK_ERR_INVALID, "bsk_fit_create: nrows, ncols must be in [1, 2^26]");
    for (int r = 0; r < nrows; ++r) {
        if (first[r] < 0 || first[r] > ncols - order) return fail(BSK_ERR_INVALID, "bsk_fit_create: first column outside [0, ncols - order]");
        if (r && first[r] < first[r - 1]) return fail(BSK_ERR_INVALID, "bsk_fit_create: first columns must be non-decreasing");
    }
    for (size_t i = 0; i < (size_t)nrows * order; ++i)
        if (!std::isfinite(values[i])) return fail(BSK_ERR_INVALID, "bsk_fit_create: matrix entry is not finite");
    bsk_fit p = new bsk_fit_s;
    p->plan.nrows = nrows;
    p->plan.ncols = ncols;
    p->plan.k = order;
    p->plan.first.assign(first, first + nrows);
    p->plan.avals.assign(values, values + (size_t)nrows * order);
    p->plan.factor();
    *out = p;
    return BSK_OK;
}

extern "C" bsk_status bsk_fit_destroy(bsk_fit p)
{
    if (!p) return BSK_OK;
    p->d_first.release(); p->d_avals.release(); p->d_rot.release(); p->d_R.release();
    p->ws_in.release(); p->ws_out.release(); p->ws_part.release();
    delete p;
    return BSK_OK;
}

extern "C" bsk_status bsk_fit_info(bsk_fit p, int *ncols, double *rank_indicator, double *r_band)
{
    if (!p) return fail(BSK_ERR_INVALID, "plan is NULL");
    if (ncols) *ncols = p->plan.ncols;
    if (rank_indicator) *rank_indicator = p->plan.rmax > 0.0 ? p->plan.rmin / p->plan.rmax : 0.0;
    if (r_band) std::memcpy(r_band, p->plan.R.data(), sizeof(double) * p->plan.R.size());
    return BSK_OK;
}

extern "C" const char *bsk_fit_last_kernel(bsk_fit p) { return p ? p->last_kernel : ""; }

extern "C" bsk_status bsk_fit_solve_host(bsk_fit p, bsk_dtype dtype, const void *b, int64_t outer, int64_t inner, double *x)
{
    bsk_status s = check_shape(p, outer, inner, "bsk_fit_solve_host");
    if (s != BSK_OK) return s;
    if (!b || !x) return fail(BSK_ERR_INVALID, "NULL argument");
    if (dtype != BSK_F32 && dtype != BSK_F64) return fail(BSK_ERR_INVALID, "dtype must be BSK_F32 or BSK_F64");
    const FitPlan &q = p->plan;
    if (!(q.rmin > 0.0)) return fail(BSK_ERR_INVALID, "bsk_fit_solve_host: R is singular (see bsk_fit_info)");
    std::vector<double> d;
    for (int64_t o = 0; o < outer; ++o)
        for (int64_t i = 0; i < inner; ++i) {
            double *xl = x + o * q.ncols * inner + i;
            if (dtype == BSK_F32) q.solve_line(static_cast<const float *>(b) + o * q.nrows * inner + i, inner, xl, inner, d);
            else q.solve_line(static_cast<const double *>(b) + o * q.nrows * inner + i, inner, xl, inner, d);
        }
    p->last_kernel = "host plan";
    return BSK_OK;
}

extern "C" bsk_status bsk_fit_sweep(bsk_fit p, bsk_dtype dtype, const void *b, int64_t outer, int64_t inner, double *x,
                                    void *stream)
{
    bsk_status s = check_shape(p, outer, inner, "bsk_fit_sweep");
    if (s != BSK_OK) return s;
    if (!b || !x) return fail(BSK_ERR_INVALID, "NULL argument");
    if (dtype != BSK_F32 && dtype != BSK_F64) return fail(BSK_ERR_INVALID, "dtype must be BSK_F32 or BSK_F64");
    if (p->plan.k > FIT_KMAX) return fail(BSK_ERR_UNSUPPORTED, "bsk_fit_sweep: orders above 8 are solved by bsk_fit_solve_host");
    if (!(p->plan.rmin > 0.0)) return fail(BSK_ERR_INVALID, "bsk_fit_sweep: R is singular (see bsk_fit_info)");
    s = upload(p);
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == BSK_F32 ? run_sweep<float>(p, static_cast<const float *>(b), outer, inner, x, st)
                            : run_sweep<double>(p, static_cast<const double *>(b), outer, inner, x, st);
}

extern "C" bsk_status bsk_fit_residual(bsk_fit p, bsk_dtype dtype, const void *b, const double *x, int64_t outer,
                                       int64_t inner, double *sumsq, void *stream)
{
    bsk_status s = check_shape(p, outer, inner, "bsk_fit_residual");
    if (s != BSK_OK) return s;
    if (!b || !x || !sumsq) return fail(BSK_ERR_INVALID, "NULL argument");
    if (dtype != BSK_F32 && dtype != BSK_F64) return fail(BSK_ERR_INVALID, "dtype must be BSK_F32 or BSK_F64");
    s = upload(p);
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == BSK_F32 ? run_residual<float>(p, static_cast<const float *>(b), x, outer, inner, sumsq, st)
                            : run_residual<double>(p, static_cast<const double *>(b), x, outer, inner, sumsq, st);
}
