// Scattered least squares (bsk_scatter.hpp): the bsk_scatter_* entry points.  Like bsk_project_tu.hip the family keeps
// no handle, and each x_host / x pair is one function of DEVICE: the checks, the dispatch, then the host loop over the
// lanes or the launch.  bsk_scatter_solve_host, the banded Cholesky solve, is a loop of its own; bsk_scatter_solve is its
// device twin, a sequence of launches (scatter_band, scatter_panel and scatter_trail per panel, scatter_forward,
// scatter_backward) on the caller's workspace.
// Instantiations: scatter_gram for curves of order 2 .. 4 and surfaces of orders 2 .. 4, ndep 1 .. 4; scatter_residual for
// the same orders; the host drivers for orders 2 .. 6 and any ndep.
#include <cstdint>
#include <vector>

#include "bsk_host.hpp"
#include "bsk_scatter.hpp"

using namespace bskscatter;

static thread_local const char *g_scatter_kernel = "";

constexpr double SCATTER_MAX_BAND = 134217728.0;    // 2^27 doubles of band storage

struct Shape {
    int nind, K0, K1;
    long long n0, n1;
    const double *knots0, *knots1;
    long long top0, top1;
};

// `knots`: the call reads them (fold and solve take the orders and the sizes alone)
static bsk_status check_shape(const Shape &s, bool device, const std::string &w, bool knots = true)
{
    if (s.nind != 1 && s.nind != 2) return fail(BSK_ERR_UNSUPPORTED, w + ": nind must be 1 (curves) or 2 (surfaces)");
    if (knots && (!s.knots0 || !s.knots1)) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (s.nind == 1 && (s.K1 != 1 || s.n1 != 1 || s.top1 != 0)) return fail(BSK_ERR_INVALID, w + ": a curve has K1 = n1 = 1, top1 = 0");
    if (s.K0 < 2 || (s.nind == 2 && s.K1 < 2)) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    const int top = device ? SCATTER_DEVICE_MAX_K : SCATTER_MAX_K;
    if (s.K0 > top || s.K1 > top) return fail(BSK_ERR_UNSUPPORTED, w + (device ? ": orders 2 to 4" : ": orders 2 to 6"));
    if (s.n0 < s.K0 || s.n1 < s.K1) return fail(BSK_ERR_INVALID, w + ": fewer coefficients than the order");
    if (s.top0 < s.K0 - 1 || s.top0 > s.n0 - 1 || s.top1 < s.K1 - 1 || s.top1 > s.n1 - 1)
        return fail(BSK_ERR_INVALID, w + ": top must be a span, K - 1 .. n - 1");
    if ((double)s.n0 * (double)s.n1 > 1.0e9) return fail(BSK_ERR_INVALID, w + ": more than 10^9 coefficients");
    return BSK_OK;
}

static Grid grid_of(const Shape &s)
{
    Grid g;
    g.ax0 = Axis{s.knots0, s.n0, s.top0, bisection_trips(s.top0 - (s.K0 - 1))};
    g.ax1 = Axis{s.knots1, s.n1, s.top1, bisection_trips(s.top1 - (s.K1 - 1))};
    g.nc1 = s.n1 - s.K1 + 1;
    return g;
}

// f(<K0>, <K1>) behind check_shape: K1 = 1 is the curve
template <bool DEVICE, typename F>
static bsk_status by_orders(const Shape &s, F &&f)
{
    constexpr int TOP = DEVICE ? SCATTER_DEVICE_MAX_K : SCATTER_MAX_K;
    return with_range<2, TOP>(s.K0, [&](auto k0) { return with_range<1, TOP>(s.K1, [&](auto k1) { return f(k0, k1); }); });
}

static bool too_many(long long lanes, int block) { return (lanes + block - 1) / block > 0x7fffffffLL; }

// ------------------------------------------------------------------------------------------ key
template <bool DEVICE>
static bsk_status key(const Shape &s, int ndep, const double *uvw, const double *points, const double *weights, long long npts,
                      int64_t *out, uint8_t *status, hipStream_t st)
{
    const std::string w = DEVICE ? "bsk_scatter_key" : "bsk_scatter_key_host";
    bsk_status r = check_shape(s, false, w);
    if (r != BSK_OK) return r;
    if (!uvw || !points || !out || !status) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (npts < 1 || ndep < 1) return fail(BSK_ERR_INVALID, w + ": npts and ndep must be >= 1");
    if (DEVICE && too_many(npts, SCATTER_BLOCK)) return fail(BSK_ERR_INVALID, w + ": too many points for one launch");
    const Grid g = grid_of(s);
    if constexpr (DEVICE) {
        r = launch_lanes<SCATTER_BLOCK>(scatter_key, npts, st, s.nind, s.K0, s.K1, g, ndep, uvw, points, weights, npts, out, status);
        if (r != BSK_OK) return r;
    } else {
        for (long long lane = 0; lane < npts; ++lane) key_lane(s.nind, s.K0, s.K1, g, ndep, uvw, points, weights, npts, lane, out, status);
    }
    g_scatter_kernel = DEVICE ? "scatter_key" : "host scatter_key";
    return BSK_OK;
}

// ------------------------------------------------------------------------------------------ gram
template <bool DEVICE>
static bsk_status gram(const Shape &s, int ndep, const Units &U, long long nunits, double *slabs, hipStream_t st)
{
    const std::string w = DEVICE ? "bsk_scatter_gram" : "bsk_scatter_gram_host";
    bsk_status r = check_shape(s, DEVICE, w);
    if (r != BSK_OK) return r;
    if (!U.uvw || !U.points || !U.order || !U.offsets || !U.unit_cell || !U.unit_start || !slabs) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (U.npts < 1 || nunits < 1 || ndep < 1) return fail(BSK_ERR_INVALID, w + ": npts, nunits and ndep must be >= 1");
    if (DEVICE && ndep > SCATTER_DEVICE_MAX_NDEP) return fail(BSK_ERR_UNSUPPORTED, w + ": ndep 1 to 4");
    if (nunits > 0x7fffffffLL) return fail(BSK_ERR_INVALID, w + ": too many units for one launch");
    const Grid g = grid_of(s);
    r = by_orders<DEVICE>(s, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE) {
            return with_range<1, SCATTER_DEVICE_MAX_NDEP>(ndep, [&](auto nd) {
                hipLaunchKernelGGL((scatter_gram<K0, K1, decltype(nd)::value>), dim3((unsigned)nunits), dim3(SCATTER_WAVE), 0, st, g, U, slabs);
                HIPCHK(hipGetLastError());
                return BSK_OK;
            });
        } else {
            constexpr int K = K0 * K1, Q = strands(K);
            std::vector<double> work((size_t)(K + 1 + ndep) + (size_t)Q * K * (K + ndep) + Q);
            gram_host<K0, K1>(g, U, ndep, nunits, slabs, work.data());
            return BSK_OK;
        }
    });
    if (r == BSK_OK) g_scatter_kernel = DEVICE ? "scatter_gram" : "host scatter_gram";
    return r;
}

// ------------------------------------------------------------------------------------------ cell
template <bool DEVICE>
static bsk_status cell(const Level &L, hipStream_t st)
{
    const std::string w = DEVICE ? "bsk_scatter_cell" : "bsk_scatter_cell_host";
    if (!L.in || !L.in_start || !L.in_count || !L.node_cell || !L.out_start || !L.out) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (L.entries < 1 || L.nnodes < 1) return fail(BSK_ERR_INVALID, w + ": entries and nnodes must be >= 1");
    if ((double)L.entries * (double)L.nnodes > 5.0e11) return fail(BSK_ERR_INVALID, w + ": array too large");
    const long long lanes = L.entries * L.nnodes;
    if (DEVICE && too_many(lanes, SCATTER_BLOCK)) return fail(BSK_ERR_INVALID, w + ": too many entries for one launch");
    if constexpr (DEVICE) {
        bsk_status r = launch_lanes<SCATTER_BLOCK>(scatter_cell, lanes, st, L);
        if (r != BSK_OK) return r;
    } else {
        for (long long lane = 0; lane < lanes; ++lane) cell_lane(L, lane);
    }
    g_scatter_kernel = DEVICE ? "scatter_cell" : "host scatter_cell";
    return BSK_OK;
}

// ------------------------------------------------------------------------------------------ fold
template <bool DEVICE>
static bsk_status fold(int nind, const Fold &F, hipStream_t st)
{
    const std::string w = DEVICE ? "bsk_scatter_fold" : "bsk_scatter_fold_host";
    const Shape s{nind, F.K0, F.K1, F.n0, F.n1, nullptr, nullptr, F.n0 - 1, F.n1 - 1};
    bsk_status r = check_shape(s, false, w, false);
    if (r != BSK_OK) return r;
    if (!F.cells || !F.stencil || !F.rhs) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (F.ndep < 1) return fail(BSK_ERR_INVALID, w + ": ndep must be >= 1");
    const long long lanes = F.n0 * F.n1 * ((2 * F.K0 - 1) * (2 * F.K1 - 1) + F.ndep);
    if (DEVICE && too_many(lanes, SCATTER_BLOCK)) return fail(BSK_ERR_INVALID, w + ": too many entries for one launch");
    if constexpr (DEVICE) {
        r = launch_lanes<SCATTER_BLOCK>(scatter_fold, lanes, st, F, lanes);
        if (r != BSK_OK) return r;
    } else {
        for (long long lane = 0; lane < lanes; ++lane) fold_lane(F, lane);
    }
    g_scatter_kernel = DEVICE ? "scatter_fold" : "host scatter_fold";
    return BSK_OK;
}

// ------------------------------------------------------------------------------------------ residual
template <bool DEVICE>
static bsk_status residual(const Shape &s, int ndep, const double *coefs, const double *uvw, const double *points, const int64_t *keys,
                           long long npts, double *out, hipStream_t st)
{
    const std::string w = DEVICE ? "bsk_scatter_residual" : "bsk_scatter_residual_host";
    bsk_status r = check_shape(s, DEVICE, w);
    if (r != BSK_OK) return r;
    if (!coefs || !uvw || !points || !keys || !out) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (npts < 1 || ndep < 1) return fail(BSK_ERR_INVALID, w + ": npts and ndep must be >= 1");
    if (DEVICE && too_many(npts, SCATTER_BLOCK)) return fail(BSK_ERR_INVALID, w + ": too many points for one launch");
    const Grid g = grid_of(s);
    r = by_orders<DEVICE>(s, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE)
            return launch_lanes<SCATTER_BLOCK>(scatter_residual<K0, K1>, npts, st, g, ndep, coefs, uvw, points, keys, npts, out);
        else {
            for (long long lane = 0; lane < npts; ++lane) residual_lane<K0, K1>(g, ndep, coefs, uvw, points, keys, npts, lane, out);
            return BSK_OK;
        }
    });
    if (r == BSK_OK) g_scatter_kernel = DEVICE ? "scatter_residual" : "host scatter_residual";
    return r;
}

// ------------------------------------------------------------------------------------------ reweight
template <bool DEVICE>
static bsk_status reweight(int loss, double s, const double *residual, const double *weights, const int64_t *keys, long long npts,
                           double *out, hipStream_t st)
{
    const std::string w = DEVICE ? "bsk_scatter_reweight" : "bsk_scatter_reweight_host";
    if (loss != 0 && loss != 1) return fail(BSK_ERR_INVALID, w + ": loss must be 0 (Huber) or 1 (Tukey)");
    if (!(s > 0.0) || !is_finite(s)) return fail(BSK_ERR_INVALID, w + ": the threshold must be finite and > 0");
    if (!residual || !keys || !out) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (npts < 1) return fail(BSK_ERR_INVALID, w + ": npts must be >= 1");
    if (DEVICE && too_many(npts, SCATTER_BLOCK)) return fail(BSK_ERR_INVALID, w + ": too many points for one launch");
    if constexpr (DEVICE) {
        bsk_status r = launch_lanes<SCATTER_BLOCK>(scatter_reweight, npts, st, loss, s, residual, weights, keys, npts, out);
        if (r != BSK_OK) return r;
    } else {
        for (long long lane = 0; lane < npts; ++lane) reweight_lane(loss, s, residual, weights, keys, lane, out);
    }
    g_scatter_kernel = DEVICE ? "scatter_reweight" : "host scatter_reweight";
    return BSK_OK;
}

// ------------------------------------------------------------------------------------------ solve (device)
constexpr int STAGE_BAND = 1, STAGE_FACTOR = 2, STAGE_FORWARD = 4, STAGE_BACKWARD = 8;

// the checks of bsk_scatter_solve and the band it works on; *doubles: the workspace (A, Ub: n ld each; z: ndep n)
static bsk_status solve_plan(const Shape &s, int ndep, const std::string &w, Band &B, long long &doubles)
{
    bsk_status r = check_shape(s, false, w, false);
    if (r != BSK_OK) return r;
    if (ndep < 1 || ndep > SCATTER_DEVICE_MAX_NDEP) return fail(BSK_ERR_UNSUPPORTED, w + ": ndep 1 to 4");
    const long long n = s.n0 * s.n1, full = (long long)(s.K0 - 1) * s.n1 + s.K1 - 1, hb = full < n - 1 ? full : n - 1;
    if ((double)n * (double)(full + 1) > SCATTER_MAX_BAND) return fail(BSK_ERR_INVALID, w + ": the band storage n (half bandwidth + 1) exceeds 2^27 doubles");
    if (hb > SOLVE_RING - 1) return fail(BSK_ERR_UNSUPPORTED, w + ": half bandwidths up to " + std::to_string(SOLVE_RING - 1));
    B = Band{s.K0, s.K1, s.n1, n, hb, hb + 1};
    doubles = 2 * n * (hb + 1) + (long long)ndep * n;
    return BSK_OK;
}

static bsk_status solve_device(const Shape &s, int ndep, const double *stencil, const double *rhs, double *coefs, double *work,
                               long long work_doubles, int64_t *bad_row, int stages, hipStream_t st)
{
    const std::string w = "bsk_scatter_solve";
    Band B;
    long long need = 0;
    bsk_status r = solve_plan(s, ndep, w, B, need);
    if (r != BSK_OK) return r;
    if (!stencil || !rhs || !coefs || !work || !bad_row) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (work_doubles < need) return fail(BSK_ERR_INVALID, w + ": the workspace holds fewer than " + std::to_string(need) + " doubles");
    const long long n = B.n, hb = B.hb;
    double *A = work, *Ub = work + n * B.ld, *z = work + 2 * n * B.ld;
    if (stages & STAGE_BAND) {
        r = launch_lanes<SOLVE_BLOCK>(scatter_band, n * B.ld, st, B, stencil, A, bad_row);
        if (r != BSK_OK) return r;
    }
    if (stages & STAGE_FACTOR)
        for (long long k0 = 0; k0 < n; k0 += SOLVE_NB) {
            const long long behind = n - k0 - SOLVE_NB, cols = behind < hb ? behind : hb;     // columns and rows behind the panel
            hipLaunchKernelGGL(scatter_panel, dim3((unsigned)(cols > 0 ? (cols + SOLVE_BLOCK - 1) / SOLVE_BLOCK : 1)), dim3(SOLVE_BLOCK), 0, st,
                               B, k0, A, Ub, bad_row);
            HIPCHK(hipGetLastError());
            if (cols > 0) {
                hipLaunchKernelGGL(scatter_trail, dim3((unsigned)((cols + SOLVE_BLOCK - 1) / SOLVE_BLOCK), (unsigned)cols), dim3(SOLVE_BLOCK), 0, st,
                                   B, k0, A, Ub);
                HIPCHK(hipGetLastError());
            }
        }
    if (stages & STAGE_FORWARD) {
        hipLaunchKernelGGL(scatter_forward, dim3((unsigned)ndep), dim3(SOLVE_BLOCK), 0, st, B, ndep, Ub, rhs, z);
        HIPCHK(hipGetLastError());
    }
    if (stages & STAGE_BACKWARD) {
        hipLaunchKernelGGL(scatter_backward, dim3((unsigned)ndep), dim3(SCATTER_WAVE), 0, st, B, Ub, z, coefs);
        HIPCHK(hipGetLastError());
    }
    g_scatter_kernel = "scatter_solve";
    return BSK_OK;
}

// ------------------------------------------------------------------------------------------ the C ABI
extern "C" const char *bsk_scatter_last_kernel(void) { return g_scatter_kernel; }

#define SHAPE Shape{nind, K0, K1, n0, n1, knots0, knots1, top0, top1}

extern "C" bsk_status bsk_scatter_key_host(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                           int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points,
                                           const double *weights, int64_t npts, int64_t *key_out, uint8_t *status)
{
    return key<false>(SHAPE, ndep, uvw, points, weights, npts, key_out, status, nullptr);
}

extern "C" bsk_status bsk_scatter_key(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                      int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points,
                                      const double *weights, int64_t npts, int64_t *key_out, uint8_t *status, void *stream)
{
    return key<true>(SHAPE, ndep, uvw, points, weights, npts, key_out, status, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_scatter_gram_host(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                            int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points,
                                            const double *weights, int64_t npts, const int64_t *order, const int64_t *offsets,
                                            const int64_t *unit_cell, const int64_t *unit_start, int64_t nunits, double *slabs)
{
    return gram<false>(SHAPE, ndep, Units{uvw, points, weights, npts, order, offsets, unit_cell, unit_start}, nunits, slabs, nullptr);
}

extern "C" bsk_status bsk_scatter_gram(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                       int64_t top0, int64_t top1, int ndep, const double *uvw, const double *points,
                                       const double *weights, int64_t npts, const int64_t *order, const int64_t *offsets,
                                       const int64_t *unit_cell, const int64_t *unit_start, int64_t nunits, double *slabs, void *stream)
{
    return gram<true>(SHAPE, ndep, Units{uvw, points, weights, npts, order, offsets, unit_cell, unit_start}, nunits, slabs,
                      static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_scatter_cell_host(int64_t entries, const double *in, const int64_t *in_start, const int64_t *in_count,
                                            const int64_t *node_cell, const int64_t *out_start, int64_t nnodes, double *out)
{
    return cell<false>(Level{entries, in, in_start, in_count, node_cell, out_start, nnodes, out}, nullptr);
}

extern "C" bsk_status bsk_scatter_cell(int64_t entries, const double *in, const int64_t *in_start, const int64_t *in_count,
                                       const int64_t *node_cell, const int64_t *out_start, int64_t nnodes, double *out, void *stream)
{
    return cell<true>(Level{entries, in, in_start, in_count, node_cell, out_start, nnodes, out}, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_scatter_fold_host(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *cells,
                                            double *stencil, double *rhs)
{
    return fold<false>(nind, Fold{K0, K1, ndep, n0, n1, cells, stencil, rhs}, nullptr);
}

extern "C" bsk_status bsk_scatter_fold(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *cells, double *stencil,
                                       double *rhs, void *stream)
{
    return fold<true>(nind, Fold{K0, K1, ndep, n0, n1, cells, stencil, rhs}, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_scatter_residual_host(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0,
                                                const double *knots1, int64_t top0, int64_t top1, int ndep, const double *coefs,
                                                const double *uvw, const double *points, const int64_t *key_in, int64_t npts,
                                                double *residual_out)
{
    return residual<false>(SHAPE, ndep, coefs, uvw, points, key_in, npts, residual_out, nullptr);
}

extern "C" bsk_status bsk_scatter_residual(int nind, int K0, int K1, int64_t n0, int64_t n1, const double *knots0, const double *knots1,
                                           int64_t top0, int64_t top1, int ndep, const double *coefs, const double *uvw,
                                           const double *points, const int64_t *key_in, int64_t npts, double *residual_out, void *stream)
{
    return residual<true>(SHAPE, ndep, coefs, uvw, points, key_in, npts, residual_out, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_scatter_reweight_host(int loss, double threshold, const double *residual, const double *weights,
                                                const int64_t *key_in, int64_t npts, double *weights_out)
{
    return reweight<false>(loss, threshold, residual, weights, key_in, npts, weights_out, nullptr);
}

extern "C" bsk_status bsk_scatter_reweight(int loss, double threshold, const double *residual, const double *weights,
                                           const int64_t *key_in, int64_t npts, double *weights_out, void *stream)
{
    return reweight<true>(loss, threshold, residual, weights, key_in, npts, weights_out, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_scatter_solve_work(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, int64_t *doubles)
{
    if (!doubles) return fail(BSK_ERR_INVALID, "bsk_scatter_solve_work: NULL argument");
    Band B;
    long long need = 0;
    bsk_status r = solve_plan(Shape{nind, K0, K1, n0, n1, nullptr, nullptr, n0 - 1, n1 - 1}, ndep, "bsk_scatter_solve_work", B, need);
    if (r == BSK_OK) *doubles = need;
    return r;
}

extern "C" bsk_status bsk_scatter_solve(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *stencil,
                                        const double *rhs, double *coefs, double *work, int64_t work_doubles, int64_t *bad_row,
                                        void *stream)
{
    return solve_device(Shape{nind, K0, K1, n0, n1, nullptr, nullptr, n0 - 1, n1 - 1}, ndep, stencil, rhs, coefs, work, work_doubles,
                        bad_row, STAGE_BAND | STAGE_FACTOR | STAGE_FORWARD | STAGE_BACKWARD, static_cast<hipStream_t>(stream));
}

// measurement hook (tools/scatter_time.py): the stages of bsk_scatter_solve one by one, 1 band, 2 factor, 4 forward, 8 backward
extern "C" bsk_status bsk_debug_scatter_solve(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *stencil,
                                              const double *rhs, double *coefs, double *work, int64_t work_doubles,
                                              int64_t *bad_row, int stages, void *stream)
{
    return solve_device(Shape{nind, K0, K1, n0, n1, nullptr, nullptr, n0 - 1, n1 - 1}, ndep, stencil, rhs, coefs, work, work_doubles,
                        bad_row, stages, static_cast<hipStream_t>(stream));
}

// The stencil [n][2 K0 - 1][2 K1 - 1] of a symmetric positive definite matrix goes to upper band storage, column j at
// band[j (hb + 1) ..], entry (i, j) at hb + i - j, hb = (K0 - 1) n1 + K1 - 1; then the Cholesky factorisation without
// square roots, U^T D U = N with a unit upper U, column by column: v_i = N_ij - sum_{k < i} U_ki v_k (k increasing),
// U_ij = v_i / D_i, D_j = N_jj - U_ij v_i (i increasing); then U^T z = b forward, z / D, U x = z backward per right-hand
// side, the sums in increasing k.  No square root: N and b x 2^k give the same U and x, bit for bit.  A pivot D_j that is
// not > 0: *bad_row = j, BSK_ERR_INVALID.
extern "C" bsk_status bsk_scatter_solve_host(int nind, int K0, int K1, int64_t n0, int64_t n1, int ndep, const double *stencil,
                                             const double *rhs, double *coefs, int64_t *bad_row)
{
    const std::string w = "bsk_scatter_solve_host";
    if (bad_row) *bad_row = -1;
    const Shape s{nind, K0, K1, n0, n1, nullptr, nullptr, n0 - 1, n1 - 1};
    bsk_status r = check_shape(s, false, w, false);
    if (r != BSK_OK) return r;
    if (!stencil || !rhs || !coefs || !bad_row) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (ndep < 1) return fail(BSK_ERR_INVALID, w + ": ndep must be >= 1");
    const long long n = n0 * n1, full = (long long)(K0 - 1) * n1 + K1 - 1, hb = full < n - 1 ? full : n - 1, ld = hb + 1;
    if ((double)n * (double)(full + 1) > SCATTER_MAX_BAND) return fail(BSK_ERR_INVALID, w + ": the band storage n (half bandwidth + 1) exceeds 2^27 doubles");
    const int S1 = 2 * K1 - 1, NS = (2 * K0 - 1) * S1;
    std::vector<double> band((size_t)(n * ld), 0.0), y((size_t)n);
    for (long long i0 = 0; i0 < n0; ++i0)
        for (long long i1 = 0; i1 < n1; ++i1)
            for (int d0 = 0; d0 < K0; ++d0)
                for (int d1 = -(K1 - 1); d1 < K1; ++d1) {
                    const long long j0 = i0 + d0, j1 = i1 + d1, i = i0 * n1 + i1, j = j0 * n1 + j1;
                    if (j0 >= n0 || j1 < 0 || j1 >= n1 || j < i) continue;
                    band[(size_t)(j * ld + hb + i - j)] = stencil[i * NS + (d0 + K0 - 1) * S1 + d1 + K1 - 1];
                }
    std::vector<double> v((size_t)ld);
    for (long long j = 0; j < n; ++j) {
        const long long low = j > hb ? j - hb : 0;
        double *cj = band.data() + j * ld + hb - j;          // cj[i] = N_ij, then U_ij (i < j) and D_j
        for (long long i = low; i < j; ++i) {
            const double *ci = band.data() + i * ld + hb - i;
            double sum = cj[i];
            for (long long k = low; k < i; ++k) sum = sum - ci[k] * v[(size_t)(k - low)];
            v[(size_t)(i - low)] = sum;                      // D_i U_ij
        }
        double pivot = cj[j];
        for (long long i = low; i < j; ++i) {
            cj[i] = v[(size_t)(i - low)] / band[(size_t)(i * ld + hb)];
            pivot = pivot - cj[i] * v[(size_t)(i - low)];
        }
        if (!(pivot > 0.0)) {
            *bad_row = j;
            return fail(BSK_ERR_INVALID, w + ": the pivot of row " + std::to_string(j) + " is not positive");
        }
        cj[j] = pivot;
    }
    for (int d = 0; d < ndep; ++d) {
        for (long long j = 0; j < n; ++j) {
            const long long low = j > hb ? j - hb : 0;
            const double *cj = band.data() + j * ld + hb - j;
            double sum = rhs[j * ndep + d];
            for (long long k = low; k < j; ++k) sum = sum - cj[k] * y[(size_t)k];
            y[(size_t)j] = sum;
        }
        for (long long j = 0; j < n; ++j) y[(size_t)j] = y[(size_t)j] / band[(size_t)(j * ld + hb)];
        for (long long i = n - 1; i >= 0; --i) {
            const long long top = i + hb < n - 1 ? i + hb : n - 1;
            double sum = y[(size_t)i];
            for (long long k = i + 1; k <= top; ++k) sum = sum - band[(size_t)(k * ld + hb + i - k)] * y[(size_t)k];
            y[(size_t)i] = sum;
        }
        for (long long i = 0; i < n; ++i) coefs[d * n + i] = y[(size_t)i];
    }
    g_scatter_kernel = "host scatter_solve";
    return BSK_OK;
}
