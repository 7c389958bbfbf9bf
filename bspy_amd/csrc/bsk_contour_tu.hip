// Level curves of scalar splines in two variables (bsk_contour.hpp): the bsk_contour_* entry points.  Like
// bsk_roots2_tu.hip the family keeps no handle: a call takes the extracted rows and the per-cell tables and enqueues one
// launch.  Instantiations: contour_flag and contour_march (count and emit) for K0, K1 = 2 .. 4 on fp64 rows; the host
// drivers run the same functions for the same orders.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_contour.hpp"

using namespace bskcontour;

static thread_local const char *g_contour_kernel = "";

constexpr int CONTOUR_MAX_K = 4;

struct ContourCall {
    int K0, K1;
    Grid g;
};

static bsk_status check_call(const ContourCall &c, const char *who)
{
    const std::string w(who);
    if (!c.g.rows || !c.g.first0 || !c.g.first1 || !c.g.scale) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.K0 < 2 || c.K1 < 2) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    if (c.K0 > CONTOUR_MAX_K || c.K1 > CONTOUR_MAX_K) return fail(BSK_ERR_UNSUPPORTED, w + ": orders above 4 are not covered");
    if (c.g.nfields < 1 || c.g.nrows < 1 || c.g.nc0 < 1 || c.g.nc1 < 1) return fail(BSK_ERR_INVALID, w + ": nfields, nrows, nc0 and nc1 must be >= 1");
    if (c.g.levels ? c.g.nrows != 1 : c.g.nrows != c.g.nfields)
        return fail(BSK_ERR_INVALID, w + ": the rows hold one field with levels and nfields fields without");
    if (c.g.R0 < c.K0 || c.g.R1 < c.K1) return fail(BSK_ERR_INVALID, w + ": the rows must hold one cell (R0 >= K0, R1 >= K1)");
    // a lattice index times the lattice width must fit a key: cells x 2^16 x 2 < 2^62
    if ((double)c.g.nfields * (double)c.g.nc0 * (double)c.g.nc1 > 1.0e9 || (double)c.g.nrows * (double)c.g.R0 * (double)c.g.R1 > 9.0e15)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

template <typename F>
static bsk_status by_order(int order, F &&f)
{
    switch (order) {
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    default: break;
    }
    return fail(BSK_ERR_UNSUPPORTED, "bsk_contour: order not covered");
}

extern "C" const char *bsk_contour_last_kernel(void) { return g_contour_kernel; }

extern "C" bsk_status bsk_contour_flag_host(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                            int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                            int64_t nfields, const double *scale, uint8_t *cand, uint8_t *zero)
{
    const ContourCall c{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}};
    bsk_status s = check_call(c, "bsk_contour_flag_host");
    if (s != BSK_OK) return s;
    if (!cand || !zero) return fail(BSK_ERR_INVALID, "bsk_contour_flag_host: NULL argument");
    s = by_order(K0, [&](auto k0) {
        return by_order(K1, [&](auto k1) {
            for (long long at = 0; at < nfields * nc0 * nc1; ++at) flag_lane<decltype(k0)::value, decltype(k1)::value>(c.g, at, cand, zero);
            return BSK_OK;
        });
    });
    if (s == BSK_OK) g_contour_kernel = "host contour_flag";
    return s;
}

extern "C" bsk_status bsk_contour_flag(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                       int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                       int64_t nfields, const double *scale, uint8_t *cand, uint8_t *zero, void *stream)
{
    const ContourCall c{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}};
    bsk_status s = check_call(c, "bsk_contour_flag");
    if (s != BSK_OK) return s;
    if (!cand || !zero) return fail(BSK_ERR_INVALID, "bsk_contour_flag: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long lanes = nfields * nc0 * nc1;
    const long long blocks = (lanes + CONTOUR_BLOCK - 1) / CONTOUR_BLOCK;
    s = by_order(K0, [&](auto k0) {
        return by_order(K1, [&](auto k1) {
            hipLaunchKernelGGL((contour_flag<decltype(k0)::value, decltype(k1)::value>), dim3((unsigned)blocks), dim3(CONTOUR_BLOCK), 0, st,
                               c.g, cand, zero);
            HIPCHK(hipGetLastError());
            return BSK_OK;
        });
    });
    if (s == BSK_OK) g_contour_kernel = "contour_flag";
    return s;
}

static bsk_status check_march(const ContourCall &c, const double *breaks0, const double *breaks1, const int64_t *cand, int64_t ncand,
                              int depth, int split, int emit, const int64_t *offsets, int64_t total, const int32_t *counts,
                              const uint8_t *lane_status, const int64_t *keys, const double *xy, const char *who)
{
    const std::string w(who);
    if (!breaks0 || !breaks1 || !cand) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (depth < 0 || depth > CONTOUR_MAX_DEPTH) return fail(BSK_ERR_INVALID, w + ": depth must be in [0, 8]");
    if (split < 0 || split > depth) return fail(BSK_ERR_INVALID, w + ": the split level must be in [0, depth]");
    if (ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (ncand > c.g.nfields * c.g.nc0 * c.g.nc1) return fail(BSK_ERR_INVALID, w + ": more candidates than cells");
    if (emit ? (!offsets || !keys || !xy || total < 1) : (!counts || !lane_status))
        return fail(BSK_ERR_INVALID, w + (emit ? ": emit takes offsets, keys, xy and total >= 1 (no segments: no call)" : ": count takes counts and lane_status"));
    return BSK_OK;
}

extern "C" bsk_status bsk_contour_march_host(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                             int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                             int64_t nfields, const double *scale, const double *breaks0, const double *breaks1,
                                             const int64_t *cand, int64_t ncand, int depth, int split, int emit,
                                             const int64_t *offsets, int64_t total, int32_t *counts, uint8_t *lane_status,
                                             int64_t *keys, double *xy)
{
    const ContourCall c{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}};
    bsk_status s = check_call(c, "bsk_contour_march_host");
    if (s != BSK_OK) return s;
    s = check_march(c, breaks0, breaks1, cand, ncand, depth, split, emit, offsets, total, counts, lane_status, keys, xy, "bsk_contour_march_host");
    if (s != BSK_OK) return s;
    const long long lanes = (long long)ncand << (2 * split);
    s = by_order(K0, [&](auto k0) {
        return by_order(K1, [&](auto k1) {
            constexpr int k0v = decltype(k0)::value, k1v = decltype(k1)::value;
            for (long long lane = 0; lane < lanes; ++lane) {
                if (emit) march_lane<k0v, k1v, true>(c.g, breaks0, breaks1, cand, ncand, depth, split, lane, offsets, total, counts, lane_status, keys, xy);
                else march_lane<k0v, k1v, false>(c.g, breaks0, breaks1, cand, ncand, depth, split, lane, offsets, total, counts, lane_status, keys, xy);
            }
            return BSK_OK;
        });
    });
    if (s == BSK_OK) g_contour_kernel = emit ? "host contour_march emit" : "host contour_march count";
    return s;
}

extern "C" bsk_status bsk_contour_march(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                        int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                        int64_t nfields, const double *scale, const double *breaks0, const double *breaks1,
                                        const int64_t *cand, int64_t ncand, int depth, int split, int emit, const int64_t *offsets,
                                        int64_t total, int32_t *counts, uint8_t *lane_status, int64_t *keys, double *xy, void *stream)
{
    const ContourCall c{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}};
    bsk_status s = check_call(c, "bsk_contour_march");
    if (s != BSK_OK) return s;
    s = check_march(c, breaks0, breaks1, cand, ncand, depth, split, emit, offsets, total, counts, lane_status, keys, xy, "bsk_contour_march");
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long lanes = (long long)ncand << (2 * split);
    const long long blocks = (lanes + CONTOUR_MARCH_BLOCK - 1) / CONTOUR_MARCH_BLOCK;
    if (blocks > 0x7fffffffll) return fail(BSK_ERR_INVALID, "bsk_contour_march: too many lanes");
    s = by_order(K0, [&](auto k0) {
        return by_order(K1, [&](auto k1) {
            constexpr int k0v = decltype(k0)::value, k1v = decltype(k1)::value;
            if (emit)
                hipLaunchKernelGGL((contour_march<k0v, k1v, true>), dim3((unsigned)blocks), dim3(CONTOUR_MARCH_BLOCK), 0, st, c.g, breaks0,
                                   breaks1, cand, (long long)ncand, depth, split, offsets, (long long)total, counts, lane_status, keys, xy);
            else
                hipLaunchKernelGGL((contour_march<k0v, k1v, false>), dim3((unsigned)blocks), dim3(CONTOUR_MARCH_BLOCK), 0, st, c.g, breaks0,
                                   breaks1, cand, (long long)ncand, depth, split, offsets, (long long)total, counts, lane_status, keys, xy);
            HIPCHK(hipGetLastError());
            return BSK_OK;
        });
    });
    if (s == BSK_OK) g_contour_kernel = emit ? "contour_march emit" : "contour_march count";
    return s;
}
