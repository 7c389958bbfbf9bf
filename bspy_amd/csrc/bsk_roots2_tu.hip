// Isolated zeros of 2-variable systems (bsk_roots2.hpp): the bsk_roots2_* entry points.  Like bsk_roots_tu.hip the family
// keeps no handle: a call takes the extracted rows and the per-cell tables and enqueues one launch.
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

template <typename F>
static bsk_status by_order(int order, int max_order, F &&f)
{
    if (order <= max_order) switch (order) {
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        case 6: return f(std::integral_constant<int, 6>());
        default: break;
        }
    return fail(BSK_ERR_UNSUPPORTED, "bsk_roots2: order not covered");
}

// the device launches exist for K0, K1 = 2 .. 4 only: keep the kernels of higher orders out of the code object
template <int K0, int K1, bool DEVICE = (K0 <= ROOTS2_DEVICE_MAX_K && K1 <= ROOTS2_DEVICE_MAX_K)>
struct Launch {
    static bsk_status flag(const Grid &g, const uint8_t *mask, uint8_t *flags, hipStream_t st)
    {
        const long long lanes = g.nsys * g.nc0 * g.nc1;
        const long long blocks = (lanes + ROOTS2_BLOCK - 1) / ROOTS2_BLOCK;
        hipLaunchKernelGGL((roots2_flag<K0, K1>), dim3((unsigned)blocks), dim3(ROOTS2_BLOCK), 0, st, g, mask, flags);
        HIPCHK(hipGetLastError());
        return BSK_OK;
    }
    static bsk_status isolate(const Grid &g, const double *breaks0, const double *breaks1, const double *scale, const int64_t *cand,
                              long long ncand, double *roots, uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes,
                              hipStream_t st)
    {
        const long long blocks = (ncand + ROOTS2_ISOLATE_BLOCK - 1) / ROOTS2_ISOLATE_BLOCK;
        hipLaunchKernelGGL((roots2_isolate<K0, K1>), dim3((unsigned)blocks), dim3(ROOTS2_ISOLATE_BLOCK), 0, st, g, breaks0, breaks1,
                           scale, cand, ncand, roots, near, count, status, nodes);
        HIPCHK(hipGetLastError());
        return BSK_OK;
    }
};
template <int K0, int K1>
struct Launch<K0, K1, false> {
    static bsk_status flag(const Grid &, const uint8_t *, uint8_t *, hipStream_t) { return fail(BSK_ERR_UNSUPPORTED, "bsk_roots2: order not covered"); }
    static bsk_status isolate(const Grid &, const double *, const double *, const double *, const int64_t *, long long, double *,
                              uint8_t *, int32_t *, uint8_t *, int32_t *, hipStream_t)
    {
        return fail(BSK_ERR_UNSUPPORTED, "bsk_roots2: order not covered");
    }
};

extern "C" const char *bsk_roots2_last_kernel(void) { return g_roots2_kernel; }

extern "C" bsk_status bsk_roots2_flag_host(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                           int64_t nc1, const int32_t *first0, const int32_t *first1, const uint8_t *mask,
                                           uint8_t *flags)
{
    const Roots2Call c{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}};
    bsk_status s = check_call(c, ROOTS2_HOST_MAX_K, mask, flags, "bsk_roots2_flag_host");
    if (s != BSK_OK) return s;
    s = by_order(K0, ROOTS2_HOST_MAX_K, [&](auto k0) {
        return by_order(K1, ROOTS2_HOST_MAX_K, [&](auto k1) {
            for (long long at = 0; at < nsys * nc0 * nc1; ++at) flag_lane<decltype(k0)::value, decltype(k1)::value>(c.g, at, mask, flags);
            return BSK_OK;
        });
    });
    if (s == BSK_OK) g_roots2_kernel = "host roots2_flag";
    return s;
}

extern "C" bsk_status bsk_roots2_flag(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                      int64_t nc1, const int32_t *first0, const int32_t *first1, const uint8_t *mask, uint8_t *flags,
                                      void *stream)
{
    const Roots2Call c{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}};
    bsk_status s = check_call(c, ROOTS2_DEVICE_MAX_K, mask, flags, "bsk_roots2_flag");
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = by_order(K0, ROOTS2_DEVICE_MAX_K, [&](auto k0) {
        return by_order(K1, ROOTS2_DEVICE_MAX_K, [&](auto k1) { return Launch<decltype(k0)::value, decltype(k1)::value>::flag(c.g, mask, flags, st); });
    });
    if (s == BSK_OK) g_roots2_kernel = "roots2_flag";
    return s;
}

static bsk_status check_isolate(const Roots2Call &c, const double *breaks0, const double *breaks1, const double *scale,
                                const int64_t *cand, int64_t ncand, const double *roots, const uint8_t *near, const int32_t *count,
                                const int32_t *nodes, const char *who)
{
    const std::string w(who);
    if (!breaks0 || !breaks1 || !scale || !cand || !roots || !near || !count || !nodes) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (ncand > c.g.nsys * c.g.nc0 * c.g.nc1) return fail(BSK_ERR_INVALID, w + ": more candidates than cells");
    return BSK_OK;
}

extern "C" bsk_status bsk_roots2_isolate_host(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                              int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                                              const double *breaks1, const double *scale, const int64_t *cand, int64_t ncand,
                                              double *roots, uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes)
{
    const Roots2Call c{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}};
    const uint8_t dummy = 0;
    bsk_status s = check_call(c, ROOTS2_HOST_MAX_K, &dummy, status, "bsk_roots2_isolate_host");
    if (s != BSK_OK) return s;
    s = check_isolate(c, breaks0, breaks1, scale, cand, ncand, roots, near, count, nodes, "bsk_roots2_isolate_host");
    if (s != BSK_OK) return s;
    s = by_order(K0, ROOTS2_HOST_MAX_K, [&](auto k0) {
        return by_order(K1, ROOTS2_HOST_MAX_K, [&](auto k1) {
            for (long long lane = 0; lane < ncand; ++lane)
                isolate_lane<decltype(k0)::value, decltype(k1)::value>(c.g, lane, breaks0, breaks1, scale, cand, roots, near, count, status,
                                                                       nodes);
            return BSK_OK;
        });
    });
    if (s == BSK_OK) g_roots2_kernel = "host roots2_isolate";
    return s;
}

extern "C" bsk_status bsk_roots2_isolate(int K0, int K1, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t nc0,
                                         int64_t nc1, const int32_t *first0, const int32_t *first1, const double *breaks0,
                                         const double *breaks1, const double *scale, const int64_t *cand, int64_t ncand, double *roots,
                                         uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes, void *stream)
{
    const Roots2Call c{K0, K1, Grid{rows, nsys, R0, R1, nc0, nc1, first0, first1}};
    const uint8_t dummy = 0;
    bsk_status s = check_call(c, ROOTS2_DEVICE_MAX_K, &dummy, status, "bsk_roots2_isolate");
    if (s != BSK_OK) return s;
    s = check_isolate(c, breaks0, breaks1, scale, cand, ncand, roots, near, count, nodes, "bsk_roots2_isolate");
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = by_order(K0, ROOTS2_DEVICE_MAX_K, [&](auto k0) {
        return by_order(K1, ROOTS2_DEVICE_MAX_K, [&](auto k1) {
            return Launch<decltype(k0)::value, decltype(k1)::value>::isolate(c.g, breaks0, breaks1, scale, cand, ncand, roots, near, count,
                                                                             status, nodes, st);
        });
    });
    if (s == BSK_OK) g_roots2_kernel = "roots2_isolate";
    return s;
}

static bsk_status check_merge(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, const double *breaks0,
                              const double *breaks1, const int64_t *cand, int64_t ncand, const uint8_t *flags, const int64_t *table,
                              const int64_t *which, int64_t nnear, const uint8_t *keep, const char *who)
{
    const std::string w(who);
    if (!roots || !breaks0 || !breaks1 || !cand || !flags || !table || !which || !keep) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (R < 2 || R > slots(ROOTS2_HOST_MAX_K, ROOTS2_HOST_MAX_K)) return fail(BSK_ERR_INVALID, w + ": R must be 2 (K0 - 1)(K1 - 1) of covered orders");
    if (nsys < 1 || nc0 < 1 || nc1 < 1) return fail(BSK_ERR_INVALID, w + ": nsys, nc0 and nc1 must be >= 1");
    if ((double)nsys * (double)nc0 * (double)nc1 > 5.0e11) return fail(BSK_ERR_INVALID, w + ": array too large");
    if (ncand < 1 || ncand > nsys * nc0 * nc1) return fail(BSK_ERR_INVALID, w + ": ncand must be in [1, cells]");
    if (nnear < 1 || nnear > ncand * R) return fail(BSK_ERR_INVALID, w + ": nnear must be in [1, ncand R] (no root near an edge: no call)");
    return BSK_OK;
}

extern "C" bsk_status bsk_roots2_merge_host(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, const double *breaks0,
                                            const double *breaks1, const int64_t *cand, int64_t ncand, const uint8_t *flags,
                                            const int64_t *table, const int64_t *which, int64_t nnear, uint8_t *keep)
{
    bsk_status s = check_merge(R, roots, nsys, nc0, nc1, breaks0, breaks1, cand, ncand, flags, table, which, nnear, keep, "bsk_roots2_merge_host");
    if (s != BSK_OK) return s;
    for (long long lane = 0; lane < nnear; ++lane) merge_lane(lane, R, roots, nsys, nc0, nc1, breaks0, breaks1, cand, ncand, flags, table, which, keep);
    g_roots2_kernel = "host roots2_merge";
    return BSK_OK;
}

extern "C" bsk_status bsk_roots2_merge(int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, const double *breaks0,
                                       const double *breaks1, const int64_t *cand, int64_t ncand, const uint8_t *flags,
                                       const int64_t *table, const int64_t *which, int64_t nnear, uint8_t *keep, void *stream)
{
    bsk_status s = check_merge(R, roots, nsys, nc0, nc1, breaks0, breaks1, cand, ncand, flags, table, which, nnear, keep, "bsk_roots2_merge");
    if (s != BSK_OK) return s;
    const long long blocks = (nnear + ROOTS2_BLOCK - 1) / ROOTS2_BLOCK;
    hipLaunchKernelGGL(roots2_merge, dim3((unsigned)blocks), dim3(ROOTS2_BLOCK), 0, static_cast<hipStream_t>(stream), R, roots, (long long)nsys,
                       (long long)nc0, (long long)nc1, breaks0, breaks1, cand, (long long)ncand, flags, table, which, (long long)nnear, keep);
    HIPCHK(hipGetLastError());
    g_roots2_kernel = "roots2_merge";
    return BSK_OK;
}
