// Real roots of scalar spline curves (bsk_roots.hpp): the bsk_roots_* entry points.  The family keeps no handle: a
// call takes the extracted rows and the per-span tables and enqueues one launch.
// Instantiations: roots_flag and roots_isolate, fp32 / fp64 x K = 2 .. 8; the host drivers run K = 2 .. BSK_MAX_ORDER.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_roots.hpp"

using namespace bskroots;

static thread_local const char *g_roots_kernel = "";

struct RootsCall {
    bsk_dtype dtype;
    int order;
    const void *rows;
    long long ncomp, rowlen, nspans;
    const int32_t *first;
    const uint8_t *mask;
};

static bsk_status check_call(const RootsCall &c, int max_order, const char *who)
{
    const std::string w(who);
    if (!c.rows || !c.first || !c.mask) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.dtype != BSK_F32 && c.dtype != BSK_F64) return fail(BSK_ERR_INVALID, w + ": dtype must be BSK_F32 or BSK_F64");
    if (c.order < 2) return fail(BSK_ERR_INVALID, w + ": order must be >= 2");
    if (c.order > max_order)
        return fail(BSK_ERR_UNSUPPORTED, w + ": order above " + std::to_string(max_order) + (max_order == 8 ? " (the host driver takes it)" : ""));
    if (c.ncomp < 1 || c.nspans < 1) return fail(BSK_ERR_INVALID, w + ": ncomp and nspans must be >= 1");
    if (c.rowlen < c.order) return fail(BSK_ERR_INVALID, w + ": rowlen must be >= order");
    if ((double)c.ncomp * (double)c.nspans > 5.0e11 || (double)c.ncomp * (double)c.rowlen > 9.0e15)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

template <typename F>
static bsk_status by_order(int order, int max_order, F &&f)
{
    switch (order) {
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
    default: break;
    }
    if (max_order > 8) switch (order) {
        case 9: return f(std::integral_constant<int, 9>());
        case 10: return f(std::integral_constant<int, 10>());
        case 11: return f(std::integral_constant<int, 11>());
        case 12: return f(std::integral_constant<int, 12>());
        case 13: return f(std::integral_constant<int, 13>());
        case 14: return f(std::integral_constant<int, 14>());
        case 15: return f(std::integral_constant<int, 15>());
        case 16: return f(std::integral_constant<int, 16>());
        default: break;
        }
    return fail(BSK_ERR_UNSUPPORTED, "bsk_roots: order not covered");
}

// the device launches exist for K = 2 .. 8 only: keep the kernels of higher orders out of the code object
template <int K, bool DEVICE = (K <= 8)>
struct Launch {
    template <typename T>
    static bsk_status flag(const RootsCall &c, uint8_t *flags, hipStream_t st)
    {
        const long long lanes = c.ncomp * c.nspans;
        const long long blocks = (lanes + ROOTS_BLOCK - 1) / ROOTS_BLOCK;
        hipLaunchKernelGGL((roots_flag<T, K>), dim3((unsigned)blocks), dim3(ROOTS_BLOCK), 0, st, static_cast<const T *>(c.rows), c.ncomp,
                           c.rowlen, c.nspans, c.first, c.mask, flags);
        HIPCHK(hipGetLastError());
        return BSK_OK;
    }
    template <typename T>
    static bsk_status isolate(const RootsCall &c, const double *breaks, const double *scale, double margin, const int64_t *cand,
                              long long ncand, double *roots, int32_t *count, hipStream_t st)
    {
        const long long blocks = (ncand + ROOTS_BLOCK - 1) / ROOTS_BLOCK;
        hipLaunchKernelGGL((roots_isolate<T, K>), dim3((unsigned)blocks), dim3(ROOTS_BLOCK), 0, st, static_cast<const T *>(c.rows),
                           c.ncomp, c.rowlen, c.nspans, c.first, c.mask, breaks, scale, margin, cand, ncand, roots, count);
        HIPCHK(hipGetLastError());
        return BSK_OK;
    }
};
template <int K>
struct Launch<K, false> {
    template <typename T>
    static bsk_status flag(const RootsCall &, uint8_t *, hipStream_t) { return fail(BSK_ERR_UNSUPPORTED, "bsk_roots: order not covered"); }
    template <typename T>
    static bsk_status isolate(const RootsCall &, const double *, const double *, double, const int64_t *, long long, double *,
                              int32_t *, hipStream_t)
    {
        return fail(BSK_ERR_UNSUPPORTED, "bsk_roots: order not covered");
    }
};

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
    const RootsCall c{dtype, order, rows, ncomp, rowlen, nspans, first, mask};
    bsk_status s = check_call(c, BSK_MAX_ORDER, "bsk_roots_flag_host");
    if (s != BSK_OK) return s;
    if (!flags) return fail(BSK_ERR_INVALID, "bsk_roots_flag_host: NULL argument");
    s = by_order(order, BSK_MAX_ORDER, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (dtype == BSK_F32) flag_host<float, K>(static_cast<const float *>(rows), ncomp, rowlen, nspans, first, mask, flags);
        else flag_host<double, K>(static_cast<const double *>(rows), ncomp, rowlen, nspans, first, mask, flags);
        return BSK_OK;
    });
    if (s == BSK_OK) g_roots_kernel = "host roots_flag";
    return s;
}

extern "C" bsk_status bsk_roots_flag(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                                     const int32_t *first, const uint8_t *mask, uint8_t *flags, void *stream)
{
    const RootsCall c{dtype, order, rows, ncomp, rowlen, nspans, first, mask};
    bsk_status s = check_call(c, 8, "bsk_roots_flag");
    if (s != BSK_OK) return s;
    if (!flags) return fail(BSK_ERR_INVALID, "bsk_roots_flag: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = by_order(order, 8, [&](auto k) {
        constexpr int K = decltype(k)::value;
        return dtype == BSK_F32 ? Launch<K>::template flag<float>(c, flags, st) : Launch<K>::template flag<double>(c, flags, st);
    });
    if (s == BSK_OK) g_roots_kernel = "roots_flag";
    return s;
}

static bsk_status check_isolate(const double *breaks, const double *scale, double margin, const int64_t *cand, int64_t ncand,
                                const double *roots, const int32_t *count, const char *who)
{
    const std::string w(who);
    if (!breaks || !scale || !cand || !roots || !count) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(BSK_ERR_INVALID, w + ": margin must be finite and >= 0");
    return BSK_OK;
}

extern "C" bsk_status bsk_roots_isolate_host(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen,
                                             int64_t nspans, const int32_t *first, const uint8_t *mask, const double *breaks,
                                             const double *scale, double margin, const int64_t *cand, int64_t ncand,
                                             double *roots, int32_t *count)
{
    const RootsCall c{dtype, order, rows, ncomp, rowlen, nspans, first, mask};
    bsk_status s = check_call(c, BSK_MAX_ORDER, "bsk_roots_isolate_host");
    if (s != BSK_OK) return s;
    s = check_isolate(breaks, scale, margin, cand, ncand, roots, count, "bsk_roots_isolate_host");
    if (s != BSK_OK) return s;
    s = by_order(order, BSK_MAX_ORDER, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (dtype == BSK_F32)
            isolate_host<float, K>(static_cast<const float *>(rows), ncomp, rowlen, nspans, first, mask, breaks, scale, margin, cand,
                                   ncand, roots, count);
        else
            isolate_host<double, K>(static_cast<const double *>(rows), ncomp, rowlen, nspans, first, mask, breaks, scale, margin, cand,
                                    ncand, roots, count);
        return BSK_OK;
    });
    if (s == BSK_OK) g_roots_kernel = "host roots_isolate";
    return s;
}

extern "C" bsk_status bsk_roots_isolate(bsk_dtype dtype, int order, const void *rows, int64_t ncomp, int64_t rowlen, int64_t nspans,
                                        const int32_t *first, const uint8_t *mask, const double *breaks, const double *scale,
                                        double margin, const int64_t *cand, int64_t ncand, double *roots, int32_t *count,
                                        void *stream)
{
    const RootsCall c{dtype, order, rows, ncomp, rowlen, nspans, first, mask};
    bsk_status s = check_call(c, 8, "bsk_roots_isolate");
    if (s != BSK_OK) return s;
    s = check_isolate(breaks, scale, margin, cand, ncand, roots, count, "bsk_roots_isolate");
    if (s != BSK_OK) return s;
    if (ncand > c.ncomp * c.nspans) return fail(BSK_ERR_INVALID, "bsk_roots_isolate: more candidates than spans");
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = by_order(order, 8, [&](auto k) {
        constexpr int K = decltype(k)::value;
        return dtype == BSK_F32 ? Launch<K>::template isolate<float>(c, breaks, scale, margin, cand, ncand, roots, count, st)
                                : Launch<K>::template isolate<double>(c, breaks, scale, margin, cand, ncand, roots, count, st);
    });
    if (s == BSK_OK) g_roots_kernel = "roots_isolate";
    return s;
}
