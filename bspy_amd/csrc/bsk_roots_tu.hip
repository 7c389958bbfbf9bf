// Real roots of scalar spline curves (bsk_roots.hpp): the bsk_roots_* entry points.  The family keeps no handle: a
// call takes the extracted rows and the per-span tables and enqueues one launch.  Each x_host / x pair is one function
// of DEVICE: the checks, the dispatch, then the host loop or the launch.
// Instantiations: roots_flag and roots_isolate, fp32 / fp64 x K = 2 .. 8; the host drivers run K = 2 .. BSK_MAX_ORDER.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_roots.hpp"

using namespace bskroots;

static thread_local const char *g_roots_kernel = "";

constexpr int ROOTS_DEVICE_MAX_K = 8;

struct RootsCall {
    bsk_dtype dtype;
    int order;
    const void *rows;
    long long ncomp, rowlen, nspans;
    const int32_t *first;
    const uint8_t *mask;
};

struct RootsIsolate {
    const double *breaks, *scale;
    double margin;
    const int64_t *cand;
    long long ncand;
    double *roots;
    int32_t *count;
};

static bsk_status check_call(const RootsCall &c, int max_order, const char *who)
{
    const std::string w(who);
    if (!c.rows || !c.first || !c.mask) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.dtype != BSK_F32 && c.dtype != BSK_F64) return fail(BSK_ERR_INVALID, w + ": dtype must be BSK_F32 or BSK_F64");
    if (c.order < 2) return fail(BSK_ERR_INVALID, w + ": order must be >= 2");
    if (c.order > max_order)
        return fail(BSK_ERR_UNSUPPORTED, w + ": order above " + std::to_string(max_order) +
                                             (max_order == ROOTS_DEVICE_MAX_K ? " (the host driver takes it)" : ""));
    if (c.ncomp < 1 || c.nspans < 1) return fail(BSK_ERR_INVALID, w + ": ncomp and nspans must be >= 1");
    if (c.rowlen < c.order) return fail(BSK_ERR_INVALID, w + ": rowlen must be >= order");
    if ((double)c.ncomp * (double)c.nspans > 5.0e11 || (double)c.ncomp * (double)c.rowlen > 9.0e15)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

static bsk_status check_isolate(const RootsIsolate &a, const char *who)
{
    const std::string w(who);
    if (!a.breaks || !a.scale || !a.cand || !a.roots || !a.count) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (a.ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (!(a.margin >= 0.0) || !std::isfinite(a.margin)) return fail(BSK_ERR_INVALID, w + ": margin must be finite and >= 0");
    return BSK_OK;
}

// f(<K>, <T>) behind check_call: the device launches exist for K = 2 .. 8 only
template <bool DEVICE, typename F>
static bsk_status by_kind(const RootsCall &c, F &&f)
{
    return with_range<2, DEVICE ? ROOTS_DEVICE_MAX_K : BSK_MAX_ORDER>(c.order, [&](auto k) {
        return with_dtype(c.dtype, [&](auto t) { return f(k, t); });
    });
}

template <bool DEVICE>
static bsk_status flag(const RootsCall &c, uint8_t *flags, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_roots_flag" : "bsk_roots_flag_host";
    bsk_status s = check_call(c, DEVICE ? ROOTS_DEVICE_MAX_K : BSK_MAX_ORDER, who);
    if (s != BSK_OK) return s;
    if (!flags) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    s = by_kind<DEVICE>(c, [&](auto k, auto t) {
        using T = decltype(t);
        constexpr int K = decltype(k)::value;
        const T *rows = static_cast<const T *>(c.rows);
        if constexpr (DEVICE)
            return launch_lanes<ROOTS_BLOCK>(roots_flag<T, K>, c.ncomp * c.nspans, st, rows, c.ncomp, c.rowlen, c.nspans, c.first, c.mask, flags);
        else {
            flag_host<T, K>(rows, c.ncomp, c.rowlen, c.nspans, c.first, c.mask, flags);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_roots_kernel = DEVICE ? "roots_flag" : "host roots_flag";
    return s;
}

template <bool DEVICE>
static bsk_status isolate(const RootsCall &c, const RootsIsolate &a, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_roots_isolate" : "bsk_roots_isolate_host";
    bsk_status s = check_call(c, DEVICE ? ROOTS_DEVICE_MAX_K : BSK_MAX_ORDER, who);
    if (s != BSK_OK) return s;
    s = check_isolate(a, who);
    if (s != BSK_OK) return s;
    // the device twin alone refuses this; the host twin runs every candidate it is given
    if constexpr (DEVICE)
        if (a.ncand > c.ncomp * c.nspans) return fail(BSK_ERR_INVALID, std::string(who) + ": more candidates than spans");
    s = by_kind<DEVICE>(c, [&](auto k, auto t) {
        using T = decltype(t);
        constexpr int K = decltype(k)::value;
        const T *rows = static_cast<const T *>(c.rows);
        if constexpr (DEVICE)
            return launch_lanes<ROOTS_BLOCK>(roots_isolate<T, K>, a.ncand, st, rows, c.ncomp, c.rowlen, c.nspans, c.first, c.mask, a.breaks,
                                             a.scale, a.margin, a.cand, a.ncand, a.roots, a.count);
        else {
            isolate_host<T, K>(rows, c.ncomp, c.rowlen, c.nspans, c.first, c.mask, a.breaks, a.scale, a.margin, a.cand, a.ncand, a.roots,
                               a.count);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_roots_kernel = DEVICE ? "roots_isolate" : "host roots_isolate";
    return s;
}

extern "C" const char *bsk_roots_last_kernel(void) { return g_roots_kernel; }

extern "C" bsk_status bsk_roots_extract_host(int K, int64_t nIn, int64_t nOut, const int32_t *first, const double *w,
                                             const double *in, int64_t ncomp, double *out)
{
    if (!first || !w || !in || !out) return fail(BSK_ERR_INVALID, "bsk_roots_extract_host: NULL argument");
    if (K < 1 || K > BSK_MAX_ORDER) return fail(BSK_ERR_INVALID, "bsk_roots_extract_host: K must be in [1, BSK_MAX_ORDER]");
    if (nIn < K || nOut < 1 || ncomp < 1) return fail(BSK_ERR_INVALID, "bsk_roots_extract_host: nIn >= K, nOut >= 1 and ncomp >= 1");
    for (int64_t j = 0; j < nOut; ++j)
        if (first[j] < 0 || (int64_t)first[j] + K > nIn) return fail(BSK_ERR_INVALID, "bsk_roots_extract_host: a row reaches outside the input");
    extract_host(in, ncomp, nIn, nOut, K, first, w, out);
    g_roots_kernel = "host roots_extract";
    return BSK_OK;
}

extern "C" bsk_status bsk_roots_flag_host(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen,
                                          int64_t nspans, const int32_t *first, const uint8_t *mask, uint8_t *flags)
{
    return flag<false>(RootsCall{dtype, order, rows, ncomp, rowlen, nspans, first, mask}, flags, nullptr);
}

extern "C" bsk_status bsk_roots_flag(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                                     const int32_t *first, const uint8_t *mask, uint8_t *flags, void *stream)
{
    return flag<true>(RootsCall{dtype, order, rows, ncomp, rowlen, nspans, first, mask}, flags, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_roots_isolate_host(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen,
                                             int64_t nspans, const int32_t *first, const uint8_t *mask, const double *breaks,
                                             const double *scale, double margin, const int64_t *cand, int64_t ncand,
                                             double *roots, int32_t *count)
{
    return isolate<false>(RootsCall{dtype, order, rows, ncomp, rowlen, nspans, first, mask},
                          RootsIsolate{breaks, scale, margin, cand, ncand, roots, count}, nullptr);
}

extern "C" bsk_status bsk_roots_isolate(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                                        const int32_t *first, const uint8_t *mask, const double *breaks, const double *scale,
                                        double margin, const int64_t *cand, int64_t ncand, double *roots, int32_t *count,
                                        void *stream)
{
    return isolate<true>(RootsCall{dtype, order, rows, ncomp, rowlen, nspans, first, mask},
                         RootsIsolate{breaks, scale, margin, cand, ncand, roots, count}, static_cast<hipStream_t>(stream));
}
