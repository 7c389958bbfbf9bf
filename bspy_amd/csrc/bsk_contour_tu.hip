// Level curves of scalar splines in two variables (bsk_contour.hpp): the bsk_contour_* entry points.  Like
// bsk_roots2_tu.hip the family keeps no handle, and each x_host / x pair is one function of DEVICE: the checks, the
// dispatch, then the host loop over the lanes or the launch.
// Instantiations: contour_flag and contour_march (count and emit) for K0, K1 = 2 .. 4 on fp64 rows; the host drivers run
// the same functions for the same orders.
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

struct ContourMarch {
    const double *breaks0, *breaks1;
    const int64_t *cand;
    long long ncand;
    int depth, split, emit;
    const int64_t *offsets;
    long long total;
    int32_t *counts;
    uint8_t *lane_status;
    int64_t *keys;
    double *xy;
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

static bsk_status check_march(const ContourCall &c, const ContourMarch &m, const char *who)
{
    const std::string w(who);
    if (!m.breaks0 || !m.breaks1 || !m.cand) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (m.depth < 0 || m.depth > CONTOUR_MAX_DEPTH) return fail(BSK_ERR_INVALID, w + ": depth must be in [0, 8]");
    if (m.split < 0 || m.split > m.depth) return fail(BSK_ERR_INVALID, w + ": the split level must be in [0, depth]");
    if (m.ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (m.ncand > c.g.nfields * c.g.nc0 * c.g.nc1) return fail(BSK_ERR_INVALID, w + ": more candidates than cells");
    if (m.emit ? (!m.offsets || !m.keys || !m.xy || m.total < 1) : (!m.counts || !m.lane_status))
        return fail(BSK_ERR_INVALID, w + (m.emit ? ": emit takes offsets, keys, xy and total >= 1 (no segments: no call)" : ": count takes counts and lane_status"));
    return BSK_OK;
}

// f(<K0>, <K1>) behind check_call
template <typename F>
static bsk_status by_orders(const ContourCall &c, F &&f)
{
    return with_range<2, CONTOUR_MAX_K>(c.K0, [&](auto k0) {
        return with_range<2, CONTOUR_MAX_K>(c.K1, [&](auto k1) { return f(k0, k1); });
    });
}

template <bool DEVICE>
static bsk_status flag(const ContourCall &c, uint8_t *cand, uint8_t *zero, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_contour_flag" : "bsk_contour_flag_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    if (!cand || !zero) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    const long long lanes = c.g.nfields * c.g.nc0 * c.g.nc1;
    s = by_orders(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE) return launch_lanes<CONTOUR_BLOCK>(contour_flag<K0, K1>, lanes, st, c.g, cand, zero);
        else {
            for (long long at = 0; at < lanes; ++at) flag_lane<K0, K1>(c.g, at, cand, zero);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_contour_kernel = DEVICE ? "contour_flag" : "host contour_flag";
    return s;
}

template <bool DEVICE>
static bsk_status march(const ContourCall &c, const ContourMarch &m, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_contour_march" : "bsk_contour_march_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    s = check_march(c, m, who);
    if (s != BSK_OK) return s;
    const long long lanes = m.ncand << (2 * m.split);
    // the bound of the launch's gridDim.x, on the device twin alone
    if constexpr (DEVICE)
        if ((lanes + CONTOUR_MARCH_BLOCK - 1) / CONTOUR_MARCH_BLOCK > 0x7fffffffLL) return fail(BSK_ERR_INVALID, std::string(who) + ": too many lanes");
    s = by_orders(c, [&](auto k0, auto k1) {
        return with_bool(m.emit != 0, [&](auto emit) {
            constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
            constexpr bool EMIT = decltype(emit)::value;
            if constexpr (DEVICE)
                return launch_lanes<CONTOUR_MARCH_BLOCK>(contour_march<K0, K1, EMIT>, lanes, st, c.g, m.breaks0, m.breaks1, m.cand, m.ncand,
                                                         m.depth, m.split, m.offsets, m.total, m.counts, m.lane_status, m.keys, m.xy);
            else {
                for (long long lane = 0; lane < lanes; ++lane)
                    march_lane<K0, K1, EMIT>(c.g, m.breaks0, m.breaks1, m.cand, m.ncand, m.depth, m.split, lane, m.offsets, m.total, m.counts,
                                             m.lane_status, m.keys, m.xy);
                return BSK_OK;
            }
        });
    });
    if (s != BSK_OK) return s;
    if constexpr (DEVICE) g_contour_kernel = m.emit ? "contour_march emit" : "contour_march count";
    else g_contour_kernel = m.emit ? "host contour_march emit" : "host contour_march count";
    return BSK_OK;
}

extern "C" const char *bsk_contour_last_kernel(void) { return g_contour_kernel; }

extern "C" bsk_status bsk_contour_flag_host(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                            int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                            int64_t nfields, const double *scale, uint8_t *cand, uint8_t *zero)
{
    return flag<false>(ContourCall{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}}, cand, zero, nullptr);
}

extern "C" bsk_status bsk_contour_flag(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                       int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                       int64_t nfields, const double *scale, uint8_t *cand, uint8_t *zero, void *stream)
{
    return flag<true>(ContourCall{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}}, cand, zero,
                      static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_contour_march_host(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                             int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                             int64_t nfields, const double *scale, const double *breaks0, const double *breaks1,
                                             const int64_t *cand, int64_t ncand, int depth, int split, int emit,
                                             const int64_t *offsets, int64_t total, int32_t *counts, uint8_t *lane_status,
                                             int64_t *keys, double *xy)
{
    return march<false>(ContourCall{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}},
                        ContourMarch{breaks0, breaks1, cand, ncand, depth, split, emit, offsets, total, counts, lane_status, keys, xy}, nullptr);
}

extern "C" bsk_status bsk_contour_march(int K0, int K1, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t nc0,
                                        int64_t nc1, const int32_t *first0, const int32_t *first1, const double *levels,
                                        int64_t nfields, const double *scale, const double *breaks0, const double *breaks1,
                                        const int64_t *cand, int64_t ncand, int depth, int split, int emit, const int64_t *offsets,
                                        int64_t total, int32_t *counts, uint8_t *lane_status, int64_t *keys, double *xy, void *stream)
{
    return march<true>(ContourCall{K0, K1, Grid{rows, nrows, R0, R1, nc0, nc1, first0, first1, levels, nfields, scale}},
                       ContourMarch{breaks0, breaks1, cand, ncand, depth, split, emit, offsets, total, counts, lane_status, keys, xy},
                       static_cast<hipStream_t>(stream));
}
