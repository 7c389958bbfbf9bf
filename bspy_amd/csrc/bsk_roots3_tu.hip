// Isolated zeros of 3-variable systems (bsk_roots3.hpp): the bsk_roots3_* entry points.  Like bsk_roots2_tu.hip the family
// keeps no handle: a call takes the extracted rows and the per-cell tables and enqueues one launch.
// Instantiations: roots3_flag and roots3_isolate for K0, K1, K2 = 2 .. 4 on fp64 rows; the host drivers run the same orders.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_roots3.hpp"

using namespace bskroots3;

static thread_local const char *g_roots3_kernel = "";

constexpr int ROOTS3_MAX_K = 4;

struct Roots3Call {
    int K0, K1, K2;
    Grid g;
};

static bsk_status check_call(const Roots3Call &c, const uint8_t *mask, const uint8_t *flags, const char *who)
{
    const std::string w(who);
    if (!c.g.rows || !c.g.first0 || !c.g.first1 || !c.g.first2 || !mask || !flags) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.K0 < 2 || c.K1 < 2 || c.K2 < 2) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    if (c.K0 > ROOTS3_MAX_K || c.K1 > ROOTS3_MAX_K || c.K2 > ROOTS3_MAX_K)
        return fail(BSK_ERR_UNSUPPORTED, w + ": order above " + std::to_string(ROOTS3_MAX_K) + " (one wave holds 64 coefficients)");
    if (c.g.nsys < 1 || c.g.nc0 < 1 || c.g.nc1 < 1 || c.g.nc2 < 1) return fail(BSK_ERR_INVALID, w + ": nsys, nc0, nc1 and nc2 must be >= 1");
    if (c.g.R0 < c.K0 || c.g.R1 < c.K1 || c.g.R2 < c.K2)
        return fail(BSK_ERR_INVALID, w + ": the rows must hold one cell (R0 >= K0, R1 >= K1, R2 >= K2)");
    if ((double)c.g.nsys * (double)c.g.nc0 * (double)c.g.nc1 * (double)c.g.nc2 > 5.0e11 ||
        3.0 * (double)c.g.nsys * (double)c.g.R0 * (double)c.g.R1 * (double)c.g.R2 > 9.0e15)
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
    return fail(BSK_ERR_UNSUPPORTED, "bsk_roots3: order not covered");
}

template <typename F>
static bsk_status by_orders(const Roots3Call &c, F &&f)
{
    return by_order(c.K0, [&](auto k0) {
        return by_order(c.K1, [&](auto k1) {
            return by_order(c.K2, [&](auto k2) { return f(k0, k1, k2); });
        });
    });
}

#define ROOTS3_GRID_ARGS                                                                                                        \
    int K0, int K1, int K2, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t R2, int64_t nc0, int64_t nc1,      \
        int64_t nc2, const int32_t *first0, const int32_t *first1, const int32_t *first2
#define ROOTS3_CALL Roots3Call{K0, K1, K2, Grid{rows, nsys, R0, R1, R2, nc0, nc1, nc2, first0, first1, first2}}

extern "C" const char *bsk_roots3_last_kernel(void) { return g_roots3_kernel; }

// the node bound the drivers and the kernels were compiled with: roots3.WALK must say the same (tests hold it to that)
extern "C" int bsk_roots3_walk_bound(void) { return ROOTS3_WALK; }

extern "C" bsk_status bsk_roots3_flag_host(ROOTS3_GRID_ARGS, const uint8_t *mask, uint8_t *flags)
{
    const Roots3Call c = ROOTS3_CALL;
    bsk_status s = check_call(c, mask, flags, "bsk_roots3_flag_host");
    if (s != BSK_OK) return s;
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        for (long long at = 0; at < nsys * nc0 * nc1 * nc2; ++at)
            flag_lane<decltype(k0)::value, decltype(k1)::value, decltype(k2)::value>(c.g, at, mask, flags);
        return BSK_OK;
    });
    if (s == BSK_OK) g_roots3_kernel = "host roots3_flag";
    return s;
}

extern "C" bsk_status bsk_roots3_flag(ROOTS3_GRID_ARGS, const uint8_t *mask, uint8_t *flags, void *stream)
{
    const Roots3Call c = ROOTS3_CALL;
    bsk_status s = check_call(c, mask, flags, "bsk_roots3_flag");
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        const long long lanes = c.g.nsys * c.g.nc0 * c.g.nc1 * c.g.nc2;
        const long long blocks = (lanes + ROOTS3_BLOCK - 1) / ROOTS3_BLOCK;
        hipLaunchKernelGGL((roots3_flag<decltype(k0)::value, decltype(k1)::value, decltype(k2)::value>), dim3((unsigned)blocks),
                           dim3(ROOTS3_BLOCK), 0, st, c.g, mask, flags);
        HIPCHK(hipGetLastError());
        return BSK_OK;
    });
    if (s == BSK_OK) g_roots3_kernel = "roots3_flag";
    return s;
}

static bsk_status check_isolate(const Roots3Call &c, const Breaks &br, const double *scale, const int64_t *cand, int64_t ncand,
                                const double *roots, const uint8_t *near, const int32_t *count, const int32_t *nodes, const char *who)
{
    const std::string w(who);
    if (!br.b0 || !br.b1 || !br.b2 || !scale || !cand || !roots || !near || !count || !nodes) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (ncand > c.g.nsys * c.g.nc0 * c.g.nc1 * c.g.nc2) return fail(BSK_ERR_INVALID, w + ": more candidates than cells");
    if (ncand > 0x7fffffffLL) return fail(BSK_ERR_INVALID, w + ": more candidates than one launch takes (2^31 - 1)");
    return BSK_OK;
}

extern "C" bsk_status bsk_roots3_isolate_host(ROOTS3_GRID_ARGS, const double *breaks0, const double *breaks1, const double *breaks2,
                                              const double *scale, const int64_t *cand, int64_t ncand, double *roots, uint8_t *near,
                                              int32_t *count, uint8_t *status, int32_t *nodes)
{
    const Roots3Call c = ROOTS3_CALL;
    const Breaks br{breaks0, breaks1, breaks2};
    const uint8_t dummy = 0;
    bsk_status s = check_call(c, &dummy, status, "bsk_roots3_isolate_host");
    if (s != BSK_OK) return s;
    s = check_isolate(c, br, scale, cand, ncand, roots, near, count, nodes, "bsk_roots3_isolate_host");
    if (s != BSK_OK) return s;
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        const HostWave wave;
        for (long long slot = 0; slot < ncand; ++slot)
            isolate_wave<HostWave, decltype(k0)::value, decltype(k1)::value, decltype(k2)::value>(wave, c.g, slot, br, scale, cand, roots,
                                                                                                 near, count, status, nodes);
        return BSK_OK;
    });
    if (s == BSK_OK) g_roots3_kernel = "host roots3_isolate";
    return s;
}

extern "C" bsk_status bsk_roots3_isolate(ROOTS3_GRID_ARGS, const double *breaks0, const double *breaks1, const double *breaks2,
                                         const double *scale, const int64_t *cand, int64_t ncand, double *roots, uint8_t *near,
                                         int32_t *count, uint8_t *status, int32_t *nodes, void *stream)
{
    const Roots3Call c = ROOTS3_CALL;
    const Breaks br{breaks0, breaks1, breaks2};
    const uint8_t dummy = 0;
    bsk_status s = check_call(c, &dummy, status, "bsk_roots3_isolate");
    if (s != BSK_OK) return s;
    s = check_isolate(c, br, scale, cand, ncand, roots, near, count, nodes, "bsk_roots3_isolate");
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        hipLaunchKernelGGL((roots3_isolate<decltype(k0)::value, decltype(k1)::value, decltype(k2)::value>), dim3((unsigned)ncand),
                           dim3(ROOTS3_WAVE), 0, st, c.g, br, scale, cand, (long long)ncand, roots, near, count, status, nodes);
        HIPCHK(hipGetLastError());
        return BSK_OK;
    });
    if (s == BSK_OK) g_roots3_kernel = "roots3_isolate";
    return s;
}

#define ROOTS3_MERGE_ARGS                                                                                                       \
    int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, int64_t nc2, const double *breaks0, const double *breaks1, \
        const double *breaks2, const int64_t *cand, int64_t ncand, const uint8_t *flags, const int64_t *table,                  \
        const int64_t *which, int64_t nnear, uint8_t *keep

static bsk_status check_merge(ROOTS3_MERGE_ARGS, const char *who)
{
    const std::string w(who);
    if (!roots || !breaks0 || !breaks1 || !breaks2 || !cand || !flags || !table || !which || !keep)
        return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (R < 6 || R > ROOTS3_MAX_SLOTS) return fail(BSK_ERR_INVALID, w + ": R must be min(6 (K0 - 1)(K1 - 1)(K2 - 1), 32) of covered orders");
    if (nsys < 1 || nc0 < 1 || nc1 < 1 || nc2 < 1) return fail(BSK_ERR_INVALID, w + ": nsys, nc0, nc1 and nc2 must be >= 1");
    if ((double)nsys * (double)nc0 * (double)nc1 * (double)nc2 > 5.0e11) return fail(BSK_ERR_INVALID, w + ": array too large");
    if (ncand < 1 || ncand > nsys * nc0 * nc1 * nc2) return fail(BSK_ERR_INVALID, w + ": ncand must be in [1, cells]");
    if (nnear < 1 || nnear > ncand * R) return fail(BSK_ERR_INVALID, w + ": nnear must be in [1, ncand R] (no zero near a face: no call)");
    return BSK_OK;
}

extern "C" bsk_status bsk_roots3_merge_host(ROOTS3_MERGE_ARGS)
{
    bsk_status s = check_merge(R, roots, nsys, nc0, nc1, nc2, breaks0, breaks1, breaks2, cand, ncand, flags, table, which, nnear, keep,
                               "bsk_roots3_merge_host");
    if (s != BSK_OK) return s;
    const Breaks br{breaks0, breaks1, breaks2};
    for (long long lane = 0; lane < nnear; ++lane) merge_lane(lane, R, roots, nsys, nc0, nc1, nc2, br, cand, ncand, flags, table, which, keep);
    g_roots3_kernel = "host roots3_merge";
    return BSK_OK;
}

extern "C" bsk_status bsk_roots3_merge(ROOTS3_MERGE_ARGS, void *stream)
{
    bsk_status s = check_merge(R, roots, nsys, nc0, nc1, nc2, breaks0, breaks1, breaks2, cand, ncand, flags, table, which, nnear, keep,
                               "bsk_roots3_merge");
    if (s != BSK_OK) return s;
    const Breaks br{breaks0, breaks1, breaks2};
    const long long blocks = (nnear + ROOTS3_BLOCK - 1) / ROOTS3_BLOCK;
    hipLaunchKernelGGL(roots3_merge, dim3((unsigned)blocks), dim3(ROOTS3_BLOCK), 0, static_cast<hipStream_t>(stream), R, roots,
                       (long long)nsys, (long long)nc0, (long long)nc1, (long long)nc2, br, cand, (long long)ncand, flags, table, which,
                       (long long)nnear, keep);
    HIPCHK(hipGetLastError());
    g_roots3_kernel = "roots3_merge";
    return BSK_OK;
}
