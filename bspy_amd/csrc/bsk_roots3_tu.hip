// Isolated zeros of 3-variable systems (bsk_roots3.hpp): the bsk_roots3_* entry points.  Like bsk_roots2_tu.hip the family
// keeps no handle, and each x_host / x pair is one function of DEVICE: the checks, the dispatch, then the host loop over
// the lanes (flag_host and isolate_host of bsk_roots3.hpp, the latter over the cells on a HostWave) or the launch.
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

struct Roots3Isolate {
    Breaks br;
    const double *scale;
    const int64_t *cand;
    long long ncand;
    double *roots;
    uint8_t *near;
    int32_t *count;
    uint8_t *status;
    int32_t *nodes;
};

struct Roots3Merge {
    int R;
    const double *roots;
    long long nsys, nc0, nc1, nc2;
    Breaks br;
    const int64_t *cand;
    long long ncand;
    const uint8_t *flags;
    const int64_t *table, *which;
    long long nnear;
    uint8_t *keep;
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

static bsk_status check_isolate(const Roots3Call &c, const Roots3Isolate &a, const char *who)
{
    const std::string w(who);
    if (!a.br.b0 || !a.br.b1 || !a.br.b2 || !a.scale || !a.cand || !a.roots || !a.near || !a.count || !a.nodes)
        return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (a.ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (a.ncand > c.g.nsys * c.g.nc0 * c.g.nc1 * c.g.nc2) return fail(BSK_ERR_INVALID, w + ": more candidates than cells");
    // one workgroup a candidate; the host twin keeps the bound of the launch
    if (a.ncand > 0x7fffffffLL) return fail(BSK_ERR_INVALID, w + ": more candidates than one launch takes (2^31 - 1)");
    return BSK_OK;
}

static bsk_status check_merge(const Roots3Merge &m, const char *who)
{
    const std::string w(who);
    if (!m.roots || !m.br.b0 || !m.br.b1 || !m.br.b2 || !m.cand || !m.flags || !m.table || !m.which || !m.keep)
        return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (m.R < 6 || m.R > ROOTS3_MAX_SLOTS) return fail(BSK_ERR_INVALID, w + ": R must be min(6 (K0 - 1)(K1 - 1)(K2 - 1), 32) of covered orders");
    if (m.nsys < 1 || m.nc0 < 1 || m.nc1 < 1 || m.nc2 < 1) return fail(BSK_ERR_INVALID, w + ": nsys, nc0, nc1 and nc2 must be >= 1");
    if ((double)m.nsys * (double)m.nc0 * (double)m.nc1 * (double)m.nc2 > 5.0e11) return fail(BSK_ERR_INVALID, w + ": array too large");
    if (m.ncand < 1 || m.ncand > m.nsys * m.nc0 * m.nc1 * m.nc2) return fail(BSK_ERR_INVALID, w + ": ncand must be in [1, cells]");
    if (m.nnear < 1 || m.nnear > m.ncand * m.R) return fail(BSK_ERR_INVALID, w + ": nnear must be in [1, ncand R] (no zero near a face: no call)");
    return BSK_OK;
}

// f(<K0>, <K1>, <K2>) behind check_call
template <typename F>
static bsk_status by_orders(const Roots3Call &c, F &&f)
{
    return with_range<2, ROOTS3_MAX_K>(c.K0, [&](auto k0) {
        return with_range<2, ROOTS3_MAX_K>(c.K1, [&](auto k1) {
            return with_range<2, ROOTS3_MAX_K>(c.K2, [&](auto k2) { return f(k0, k1, k2); });
        });
    });
}

template <bool DEVICE>
static bsk_status flag(const Roots3Call &c, const uint8_t *mask, uint8_t *flags, hipStream_t st)
{
    bsk_status s = check_call(c, mask, flags, DEVICE ? "bsk_roots3_flag" : "bsk_roots3_flag_host");
    if (s != BSK_OK) return s;
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
        if constexpr (DEVICE)
            return launch_lanes<ROOTS3_BLOCK>(roots3_flag<K0, K1, K2>, c.g.nsys * c.g.nc0 * c.g.nc1 * c.g.nc2, st, c.g, mask, flags);
        else {
            flag_host<K0, K1, K2>(c.g, mask, flags);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_roots3_kernel = DEVICE ? "roots3_flag" : "host roots3_flag";
    return s;
}

template <bool DEVICE>
static bsk_status isolate(const Roots3Call &c, const Roots3Isolate &a, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_roots3_isolate" : "bsk_roots3_isolate_host";
    const uint8_t dummy = 0;
    bsk_status s = check_call(c, &dummy, a.status, who);
    if (s != BSK_OK) return s;
    s = check_isolate(c, a, who);
    if (s != BSK_OK) return s;
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
        if constexpr (DEVICE)            // one wave a workgroup, one cell a wave
            return launch_lanes<ROOTS3_WAVE>(roots3_isolate<K0, K1, K2>, a.ncand * ROOTS3_WAVE, st, c.g, a.br, a.scale, a.cand, a.ncand, a.roots,
                                             a.near, a.count, a.status, a.nodes);
        else {
            isolate_host<K0, K1, K2>(c.g, a.br, a.scale, a.cand, a.ncand, a.roots, a.near, a.count, a.status, a.nodes);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_roots3_kernel = DEVICE ? "roots3_isolate" : "host roots3_isolate";
    return s;
}

template <bool DEVICE>
static bsk_status merge(const Roots3Merge &m, hipStream_t st)
{
    bsk_status s = check_merge(m, DEVICE ? "bsk_roots3_merge" : "bsk_roots3_merge_host");
    if (s != BSK_OK) return s;
    if constexpr (DEVICE) {
        s = launch_lanes<ROOTS3_BLOCK>(roots3_merge, m.nnear, st, m.R, m.roots, m.nsys, m.nc0, m.nc1, m.nc2, m.br, m.cand, m.ncand, m.flags,
                                       m.table, m.which, m.nnear, m.keep);
        if (s != BSK_OK) return s;
    } else {
        for (long long lane = 0; lane < m.nnear; ++lane)
            merge_lane(lane, m.R, m.roots, m.nsys, m.nc0, m.nc1, m.nc2, m.br, m.cand, m.ncand, m.flags, m.table, m.which, m.keep);
    }
    g_roots3_kernel = DEVICE ? "roots3_merge" : "host roots3_merge";
    return BSK_OK;
}

#define ROOTS3_GRID_ARGS                                                                                                        \
    int K0, int K1, int K2, const double *rows, int64_t nsys, int64_t R0, int64_t R1, int64_t R2, int64_t nc0, int64_t nc1,      \
        int64_t nc2, const int32_t *first0, const int32_t *first1, const int32_t *first2
#define ROOTS3_CALL Roots3Call{K0, K1, K2, Grid{rows, nsys, R0, R1, R2, nc0, nc1, nc2, first0, first1, first2}}
#define ROOTS3_MERGE_ARGS                                                                                                       \
    int R, const double *roots, int64_t nsys, int64_t nc0, int64_t nc1, int64_t nc2, const double *breaks0, const double *breaks1, \
        const double *breaks2, const int64_t *cand, int64_t ncand, const uint8_t *flags, const int64_t *table,                  \
        const int64_t *which, int64_t nnear, uint8_t *keep

extern "C" const char *bsk_roots3_last_kernel(void) { return g_roots3_kernel; }

// the node bound the drivers and the kernels were compiled with: roots3.WALK must say the same (tests hold it to that)
extern "C" int bsk_roots3_walk_bound(void) { return ROOTS3_WALK; }

extern "C" bsk_status bsk_roots3_flag_host(ROOTS3_GRID_ARGS, const uint8_t *mask, uint8_t *flags)
{
    return flag<false>(ROOTS3_CALL, mask, flags, nullptr);
}

extern "C" bsk_status bsk_roots3_flag(ROOTS3_GRID_ARGS, const uint8_t *mask, uint8_t *flags, void *stream)
{
    return flag<true>(ROOTS3_CALL, mask, flags, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_roots3_isolate_host(ROOTS3_GRID_ARGS, const double *breaks0, const double *breaks1, const double *breaks2,
                                              const double *scale, const int64_t *cand, int64_t ncand, double *roots, uint8_t *near,
                                              int32_t *count, uint8_t *status, int32_t *nodes)
{
    return isolate<false>(ROOTS3_CALL, Roots3Isolate{Breaks{breaks0, breaks1, breaks2}, scale, cand, ncand, roots, near, count, status, nodes},
                          nullptr);
}

extern "C" bsk_status bsk_roots3_isolate(ROOTS3_GRID_ARGS, const double *breaks0, const double *breaks1, const double *breaks2,
                                         const double *scale, const int64_t *cand, int64_t ncand, double *roots, uint8_t *near,
                                         int32_t *count, uint8_t *status, int32_t *nodes, void *stream)
{
    return isolate<true>(ROOTS3_CALL, Roots3Isolate{Breaks{breaks0, breaks1, breaks2}, scale, cand, ncand, roots, near, count, status, nodes},
                         static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_roots3_merge_host(ROOTS3_MERGE_ARGS)
{
    return merge<false>(Roots3Merge{R, roots, nsys, nc0, nc1, nc2, Breaks{breaks0, breaks1, breaks2}, cand, ncand, flags, table, which, nnear, keep},
                        nullptr);
}

extern "C" bsk_status bsk_roots3_merge(ROOTS3_MERGE_ARGS, void *stream)
{
    return merge<true>(Roots3Merge{R, roots, nsys, nc0, nc1, nc2, Breaks{breaks0, breaks1, breaks2}, cand, ncand, flags, table, which, nnear, keep},
                       static_cast<hipStream_t>(stream));
}
