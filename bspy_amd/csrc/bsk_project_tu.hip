// Closest points on curves and surfaces (bsk_project.hpp): the bsk_project_* entry points.  Like bsk_roots2_tu.hip the
// family keeps no handle, and each x_host / x pair is one function of DEVICE: the checks, the dispatch, then the host
// loop over the lanes (seed_host and newton_host of bsk_project.hpp) or the launch.
// Instantiations: project_seed for ndep = 2, 3; project_newton for curves of order 2 .. 6 and surfaces of orders 2 .. 4,
// ndep = 2, 3, on the device and on the host alike.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_project.hpp"

using namespace bskproject;

static thread_local const char *g_project_kernel = "";

constexpr int PROJECT_CURVE_MAX_K = 6, PROJECT_SURFACE_MAX_K = 4;
constexpr long long PROJECT_MAX_CHUNKS = 65535;     // gridDim.y

struct SeedCall {
    int ndep;
    const double *samples;
    long long nsamples;
    const double *points;
    long long npts, chunk;
    double *part_d2;
    int32_t *part_idx;
};

struct NewtonCall {
    int nind, K0, K1, ndep;
    Tables T;
    const double *points;
    long long npts;
    const double *part_d2;
    const int32_t *part_idx;
    long long nchunks;
    const double *guess;
    double *uvw, *distance;
    uint8_t *status;
    int32_t *steps;
};

static bsk_status check_seed(const SeedCall &c, const char *who)
{
    const std::string w(who);
    if (!c.samples || !c.points || !c.part_d2 || !c.part_idx) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.nsamples < 1 || c.npts < 1 || c.chunk < 1) return fail(BSK_ERR_INVALID, w + ": nsamples, npts and chunk must be >= 1");
    if (c.ndep != 2 && c.ndep != 3) return fail(BSK_ERR_UNSUPPORTED, w + ": ndep must be 2 or 3");
    if (c.nsamples > INT32_MAX) return fail(BSK_ERR_INVALID, w + ": more than 2^31 - 1 samples");
    if ((c.nsamples + c.chunk - 1) / c.chunk > PROJECT_MAX_CHUNKS) return fail(BSK_ERR_INVALID, w + ": more than 65535 chunks");
    if ((double)c.npts * (double)((c.nsamples + c.chunk - 1) / c.chunk) > 5.0e11) return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

static bsk_status check_newton(const NewtonCall &c, const char *who)
{
    const std::string w(who);
    const Tables &T = c.T;
    if (!T.rows || !T.first0 || !T.first1 || !T.breaks0 || !T.breaks1 || !c.points || !c.uvw || !c.distance || !c.status || !c.steps)
        return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (!c.guess && (!c.part_d2 || !c.part_idx)) return fail(BSK_ERR_INVALID, w + ": neither a guess nor the partials of the seed");
    if (!c.guess && c.nchunks < 1) return fail(BSK_ERR_INVALID, w + ": nchunks must be >= 1");
    if (c.npts < 1 || T.nc0 < 1 || T.nc1 < 1) return fail(BSK_ERR_INVALID, w + ": npts, nc0 and nc1 must be >= 1");
    if (c.nind != 1 && c.nind != 2) return fail(BSK_ERR_UNSUPPORTED, w + ": nind must be 1 (curves) or 2 (surfaces)");
    if (c.ndep != 2 && c.ndep != 3) return fail(BSK_ERR_UNSUPPORTED, w + ": ndep must be 2 or 3");
    if (c.nind == 1 && (c.K1 != 1 || T.R1 != 1 || T.nc1 != 1 || T.g1 != 1))
        return fail(BSK_ERR_INVALID, w + ": a curve has K1 = R1 = nc1 = g1 = 1");
    if (c.K0 < 2 || (c.nind == 2 && c.K1 < 2)) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    if (c.nind == 1 && c.K0 > PROJECT_CURVE_MAX_K) return fail(BSK_ERR_UNSUPPORTED, w + ": curves of order 2 to 6");
    if (c.nind == 2 && (c.K0 > PROJECT_SURFACE_MAX_K || c.K1 > PROJECT_SURFACE_MAX_K))
        return fail(BSK_ERR_UNSUPPORTED, w + ": surfaces of orders 2 to 4");
    if (T.g0 < 1 || T.g0 > PROJECT_MAX_SAMPLES || T.g1 < 1 || T.g1 > PROJECT_MAX_SAMPLES)
        return fail(BSK_ERR_INVALID, w + ": 1 to 8 samples per cell and axis");
    if (T.R0 < c.K0 || T.R1 < c.K1) return fail(BSK_ERR_INVALID, w + ": the rows must hold one cell (R0 >= K0, R1 >= K1)");
    if ((double)T.nc0 * T.g0 * (double)T.nc1 * T.g1 > (double)INT32_MAX) return fail(BSK_ERR_INVALID, w + ": more than 2^31 - 1 samples");
    if ((double)c.ndep * (double)T.R0 * (double)T.R1 > 9.0e15 || (double)c.npts * (double)(c.nchunks > 1 ? c.nchunks : 1) > 5.0e11)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

// f(<NIND>, <K0>, <K1>, <NDEP>) behind check_newton: curves of order 2 .. 6 (K1 = 1), surfaces of orders 2 .. 4
template <typename F>
static bsk_status by_shape(const NewtonCall &c, F &&f)
{
    auto dep = [&](auto ni, auto k0, auto k1) {
        return with_int<2, 3>(c.ndep, [&](auto nd) { return f(ni, k0, k1, nd); });
    };
    return with_int<1, 2>(c.nind, [&](auto ni) {
        if constexpr (decltype(ni)::value == 1)          // a curve has K1 = 1
            return with_range<2, PROJECT_CURVE_MAX_K>(c.K0, [&](auto k0) {
                return with_int<1>(c.K1, [&](auto k1) { return dep(ni, k0, k1); });
            });
        else
            return with_range<2, PROJECT_SURFACE_MAX_K>(c.K0, [&](auto k0) {
                return with_range<2, PROJECT_SURFACE_MAX_K>(c.K1, [&](auto k1) { return dep(ni, k0, k1); });
            });
    });
}

template <bool DEVICE>
static bsk_status seed(const SeedCall &c, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_project_seed" : "bsk_project_seed_host";
    bsk_status s = check_seed(c, who);
    if (s != BSK_OK) return s;
    const long long nchunks = (c.nsamples + c.chunk - 1) / c.chunk;
    // the bound of the launch's gridDim.x, on the device twin alone
    if constexpr (DEVICE)
        if ((c.npts + PROJECT_BLOCK - 1) / PROJECT_BLOCK > 0x7fffffffLL) return fail(BSK_ERR_INVALID, std::string(who) + ": too many points for one launch");
    s = with_int<2, 3>(c.ndep, [&](auto nd) {
        constexpr int NDEP = decltype(nd)::value;
        if constexpr (DEVICE)
            return launch_lanes<PROJECT_BLOCK>(project_seed<NDEP>, c.npts, nchunks, st, c.samples, c.nsamples, c.points, c.npts, c.chunk,
                                               c.part_d2, c.part_idx);
        else {
            seed_host<NDEP>(c.samples, c.nsamples, c.points, c.npts, c.chunk, nchunks, c.part_d2, c.part_idx);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_project_kernel = DEVICE ? "project_seed" : "host project_seed";
    return s;
}

template <bool DEVICE>
static bsk_status newton(const NewtonCall &c, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_project_newton" : "bsk_project_newton_host";
    bsk_status s = check_newton(c, who);
    if (s != BSK_OK) return s;
    // the bound of the launch's gridDim.x, on the device twin alone
    if constexpr (DEVICE)
        if ((c.npts + PROJECT_NEWTON_BLOCK - 1) / PROJECT_NEWTON_BLOCK > 0x7fffffffLL)
            return fail(BSK_ERR_INVALID, std::string(who) + ": too many points for one launch");
    s = by_shape(c, [&](auto ni, auto k0, auto k1, auto nd) {
        constexpr int NIND = decltype(ni)::value, K0 = decltype(k0)::value, K1 = decltype(k1)::value, NDEP = decltype(nd)::value;
        if constexpr (DEVICE)
            return launch_lanes<PROJECT_NEWTON_BLOCK>(project_newton<NIND, K0, K1, NDEP>, c.npts, st, c.T, c.points, c.npts, c.part_d2,
                                                      c.part_idx, c.nchunks, c.guess, c.uvw, c.distance, c.status, c.steps);
        else {
            newton_host<NIND, K0, K1, NDEP>(c.T, c.points, c.npts, c.part_d2, c.part_idx, c.nchunks, c.guess, c.uvw, c.distance, c.status,
                                            c.steps);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_project_kernel = DEVICE ? "project_newton" : "host project_newton";
    return s;
}

static NewtonCall newton_call(int nind, int K0, int K1, int ndep, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                              const int32_t *first0, const int32_t *first1, const double *breaks0, const double *breaks1, int g0, int g1,
                              const double *points, int64_t npts, const double *part_d2, const int32_t *part_idx, int64_t nchunks,
                              const double *guess, double *uvw, double *distance, uint8_t *status, int32_t *steps)
{
    const Tables T{rows, R0, R1, nc0, nc1, first0, first1, breaks0, breaks1, nc0 >= 1 ? bisection_trips(nc0) : 0,
                   nc1 >= 1 ? bisection_trips(nc1) : 0, g0, g1};
    return NewtonCall{nind, K0, K1, ndep, T, points, npts, part_d2, part_idx, nchunks, guess, uvw, distance, status, steps};
}

extern "C" const char *bsk_project_last_kernel(void) { return g_project_kernel; }

extern "C" bsk_status bsk_project_seed_host(int ndep, const double *samples, int64_t nsamples, const double *points, int64_t npts,
                                            int64_t chunk, double *part_d2, int32_t *part_idx)
{
    return seed<false>(SeedCall{ndep, samples, nsamples, points, npts, chunk, part_d2, part_idx}, nullptr);
}

extern "C" bsk_status bsk_project_seed(int ndep, const double *samples, int64_t nsamples, const double *points, int64_t npts,
                                       int64_t chunk, double *part_d2, int32_t *part_idx, void *stream)
{
    return seed<true>(SeedCall{ndep, samples, nsamples, points, npts, chunk, part_d2, part_idx}, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_project_newton_host(int nind, int K0, int K1, int ndep, const double *rows, int64_t R0, int64_t R1,
                                              int64_t nc0, int64_t nc1, const int32_t *first0, const int32_t *first1,
                                              const double *breaks0, const double *breaks1, int g0, int g1, const double *points,
                                              int64_t npts, const double *part_d2, const int32_t *part_idx, int64_t nchunks,
                                              const double *guess, double *uvw, double *distance, uint8_t *status, int32_t *steps)
{
    return newton<false>(newton_call(nind, K0, K1, ndep, rows, R0, R1, nc0, nc1, first0, first1, breaks0, breaks1, g0, g1, points, npts,
                                     part_d2, part_idx, nchunks, guess, uvw, distance, status, steps),
                         nullptr);
}

extern "C" bsk_status bsk_project_newton(int nind, int K0, int K1, int ndep, const double *rows, int64_t R0, int64_t R1, int64_t nc0,
                                         int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                                         const double *breaks1, int g0, int g1, const double *points, int64_t npts,
                                         const double *part_d2, const int32_t *part_idx, int64_t nchunks, const double *guess,
                                         double *uvw, double *distance, uint8_t *status, int32_t *steps, void *stream)
{
    return newton<true>(newton_call(nind, K0, K1, ndep, rows, R0, R1, nc0, nc1, first0, first1, breaks0, breaks1, g0, g1, points, npts,
                                    part_d2, part_idx, nchunks, guess, uvw, distance, status, steps),
                        static_cast<hipStream_t>(stream));
}
