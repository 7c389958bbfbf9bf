// Isolated zeros of 2-variable systems (bsk_roots2.hpp): the bsk_roots2_* entry points.  Like bsk_roots_tu.hip the family
// keeps no handle, and each x_host / x pair is one function of DEVICE: the checks, the dispatch, then the host loop over
// the lanes or the launch.
// Instantiations: roots2_flag and roots2_isolate for K0, K1 = 2 .. 4 on fp64 rows; the host drivers run K0, K1 = 2 .. 6.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_roots2.hpp"

using namespace bskroots2;

static thread_local const char *g_roots2_kernel = "";

constexpr int ROOTS2_DEVICE_MAX_K = 4, ROOTS2_HOST_MAX_K = 6;

struct Roots2Call {
    int K0, K1;
    Grid g;
};

struct Roots2Isolate {
    const double *breaks0, *breaks1, *scale;
    const int64_t *cand;
    long long ncand;
    double *roots;
    uint8_t *near;
    int32_t *count;
    uint8_t *status;
    int32_t *nodes;
};

struct Roots2Merge {
    int R;
    const double *roots;
    long long nsys, nc0, nc1;
    const double *breaks0, *breaks1;
    const int64_t *cand;
    long long ncand;
    const uint8_t *flags;
    const int64_t *table, *which;
    long long nnear;
    uint8_t *keep;
};

static bsk_status check_call(const Roots2Call &c, int max_order, const uint8_t *mask, const uint8_t *flags, const char *who)
{
    const std::string w(who);
    if (!c.g.rows || !c.g.first0 || !c.g.first1 || !mask || !flags) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.K0 < 2 || c.K1 < 2) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    if (c.K0 > max_order || c.K1 > max_order)
        return fail(BSK_ERR_UNSUPPORTED, w + ": order above " + std::to_string(max_order) +
                                             (max_order == ROOTS2_DEVICE_MAX_K ? " (the host driver takes orders up to 6)" : ""));
    if (c.g.nsys < 1 || c.g.nc0 < 1 || c.g.nc1 < 1) return fail(BSK_ERR_INVALID, w + ": nsys, nc0 and nc1 must be >= 1");
    if (c.g.R0 < c.K0 || c.g.R1 < c.K1) return fail(BSK_ERR_INVALID, w + ": the rows must hold one cell (R0 >= K0, R1 >= K1)");
    if ((double)c.g.nsys * (double)c.g.nc0 * (double)c.g.nc1 > 5.0e11 || 2.0 * (double)c.g.nsys * (double)c.g.R0 * (double)c.g.R1 > 9.0e15)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

static bsk_status check_isolate(const Roots2Call &c, const Roots2Isolate &a, const char *who)
{
    const std::string w(who);
    if (!a.breaks0 || !a.breaks1 || !a.scale || !a.cand || !a.roots || !a.near || !a.count || !a.nodes)
        return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (a.ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (a.ncand > c.g.nsys * c.g.nc0 * c.g.nc1) return fail(BSK_ERR_INVALID, w + ": more candidates than cells");
    return BSK_OK;
}

static bsk_status check_merge(const Roots2Merge &m, const char *who)
{
    const std::string w(who);
    if (!m.roots || !m.breaks0 || !m.breaks1 || !m.cand || !m.flags || !m.table || !m.which || !m.keep)
        return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (m.R < 2 || m.R > slots(ROOTS2_HOST_MAX_K, ROOTS2_HOST_MAX_K)) return fail(BSK_ERR_INVALID, w + ": R must be 2 (K0 - 1)(K1 - 1) of covered orders");
    if (m.nsys < 1 || m.nc0 < 1 || m.nc1 < 1) return fail(BSK_ERR_INVALID, w + ": nsys, nc0 and nc1 must be >= 1");
    if ((double)m.nsys * (double)m.nc0 * (double)m.nc1 > 5.0e11) return fail(BSK_ERR_INVALID, w + ": array too large");
    if (m.ncand < 1 || m.ncand > m.nsys * m.nc0 * m.nc1) return fail(BSK_ERR_INVALID, w + ": ncand must be in [1, cells]");
    if (m.nnear < 1 || m.nnear > m.ncand * m.R) return fail(BSK_ERR_INVALID, w + ": nnear must be in [1, ncand R] (no root near an edge: no call)");
    return BSK_OK;
}

// f(<K0>, <K1>) behind check_call: the device launches exist for K0, K1 = 2 .. 4 only
template <bool DEVICE, typename F>
static bsk_status by_orders(const Roots2Call &c, F &&f)
{
    constexpr int MAX_K = DEVICE ? ROOTS2_DEVICE_MAX_K : ROOTS2_HOST_MAX_K;
    return with_range<2, MAX_K>(c.K0, [&](auto k0) {
        return with_range<2, MAX_K>(c.K1, [&](auto k1) { return f(k0, k1); });
    });
}

template <bool DEVICE>
static bsk_status flag(const Roots2Call &c, const uint8_t *mask, uint8_t *flags, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_roots2_flag" : "bsk_roots2_flag_host";
    bsk_status s = check_call(c, DEVICE ? ROOTS2_DEVICE_MAX_K : ROOTS2_HOST_MAX_K, mask, flags, who);
    if (s != BSK_OK) return s;
    const long long lanes = c.g.nsys * c.g.nc0 * c.g.nc1;
    s = by_orders<DEVICE>(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE) return launch_lanes<ROOTS2_BLOCK>(roots2_flag<K0, K1>, lanes, st, c.g, mask, flags);
        else {
            for (long long at = 0; at < lanes; ++at) flag_lane<K0, K1>(c.g, at, mask, flags);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_roots2_kernel = DEVICE ? "roots2_flag" : "host roots2_flag";
    return s;
}

template <bool DEVICE>
static bsk_status isolate(const Roots2Call &c, const Roots2Isolate &a, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_roots2_isolate" : "bsk_roots2_isolate_host";
    const uint8_t dummy = 0;
    bsk_status s = check_call(c, DEVICE ? ROOTS2_DEVICE_MAX_K : ROOTS2_HOST_MAX_K, &dummy, a.status, who);
    if (s != BSK_OK) return s;
    s = check_isolate(c, a, who);
    if (s != BSK_OK) return s;
    s = by_orders<DEVICE>(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE)
            return launch_lanes<ROOTS2_ISOLATE_BLOCK>(roots2_isolate<K0, K1>, a.ncand, st, c.g, a.breaks0, a.breaks1, a.scale, a.cand, a.ncand,
                                                      a.roots, a.near, a.count, a.status, a.nodes);
        else {
            for (long long lane = 0; lane < a.ncand; ++lane)
                isolate_lane<K0, K1>(c.g, lane, a.breaks0, a.breaks1, a.scale, a.cand, a.roots, a.near, a.count, a.status, a.nodes);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_roots2_kernel = DEVICE ? "roots2_isolate" : "host roots2_isolate";
    return s;
}

template <bool DEVICE>
static bsk_status merge(const Roots2Merge &m, hipStream_t st)
{
    bsk_status s = check_merge(m, DEVICE ? "bsk_roots2_merge" : "bsk_roots2_merge_host");
    if (s != BSK_OK) return s;
    if constexpr (DEVICE) {
        s = launch_lanes<ROOTS2_BLOCK>(roots2_merge, m.nnear, st, m.R, m.roots, m.nsys, m.nc0, m.nc1, m.breaks0, m.breaks1, m.cand, m.ncand,
                                       m.flags, m.table, m.which, m.nnear, m.keep);
        if (s != BSK_OK) return s;
    } else {
        for (long long lane = 0; lane < m.nnear; ++lane)
            merge_lane(lane, m.R, m.roots, m.nsys, m.nc0, m.nc1, m.breaks0, m.breaks1, m.cand, m.ncand, m.flags, m.table, m.which, m.keep);
    }
    g_roots2_kernel = DEVICE ? "roots2_merge" : "host roots2_merge";
    return BSK_OK;
}

extern "C" const char *bsk_roots2_last_kernel(void) { return g_roots2_kernel; }

extern "C" bsk_status bsk_roots2_flag_host(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                           int64_t nc1, const int32_t *first0, const int32_t *first1, const uint8_t *mask,
                                           uint8_t *flags)
{
    return flag<false>(Roots2Call{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}}, mask, flags, nullptr);
}

extern "C" bsk_status bsk_roots2_flag(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                      int64_t nc1, const int32_t *first0, const int32_t *first1, const uint8_t *mask, uint8_t *flags,
                                      void *stream)
{
    return flag<true>(Roots2Call{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}}, mask, flags, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_roots2_isolate_host(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                              int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                                              const double *breaks1, const double *scale, const int64_t *cand, int64_t ncand,
                                              double *roots, uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes)
{
    return isolate<false>(Roots2Call{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}},
                          Roots2Isolate{breaks0, breaks1, scale, cand, ncand, roots, near, count, status, nodes}, nullptr);
}

extern "C" bsk_status bsk_roots2_isolate(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                         int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                                         const double *breaks1, const double *scale, const int64_t *cand, int64_t ncand, double *roots,
                                         uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes, void *stream)
{
    return isolate<true>(Roots2Call{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}},
                         Roots2Isolate{breaks0, breaks1, scale, cand, ncand, roots, near, count, status, nodes},
                         static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_roots2_merge_host(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, const double *breaks0,
                                            const double *breaks1, const int64_t *cand, int64_t ncand, const uint8_t *flags,
                                            const int64_t *table, const int64_t *which, int64_t nnear, uint8_t *keep)
{
    return merge<false>(Roots2Merge{R, roots, nsys, nc0, nc1, breaks0, breaks1, cand, ncand, flags, table, which, nnear, keep}, nullptr);
}

extern "C" bsk_status bsk_roots2_merge(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, const double *breaks0,
                                       const double *breaks1, const int64_t *cand, int64_t ncand, const uint8_t *flags,
                                       const int64_t *table, const int64_t *which, int64_t nnear, uint8_t *keep, void *stream)
{
    return merge<true>(Roots2Merge{R, roots, nsys, nc0, nc1, breaks0, breaks1, cand, ncand, flags, table, which, nnear, keep},
                       static_cast<hipStream_t>(stream));
}
