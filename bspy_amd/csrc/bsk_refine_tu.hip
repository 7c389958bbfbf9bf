// Banded operators on coefficient tensors (bsk_refine.hpp): the bsk_band_* entry points.  A band map is host data and
// bsk_band_create makes no HIP call; its tables go to the device with the first device call on the handle.
// Instantiations: band_apply fp32 / fp64 x K 2 - 8 x (16-byte lanes, scalar lanes), band_apply_line fp32 / fp64 x K 2 - 8,
// and the same sets of band_absmax and band_absmax_line (bsk_band_absmax: two launches, the second one band_absmax_fold).
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_refine.hpp"

using namespace bskband;

struct bsk_band_s {
    BandMap map;
    int device = -1;                   // device the tables live on (-1: not uploaded)
    DevBuf d_first, d_w;
    DevBuf d_part;                     // partial maxima of bsk_band_absmax: [groups][P][nOut] doubles
    const char *last_kernel = "";
};

static bsk_status upload(bsk_band p)
{
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (p->device == dev) return BSK_OK;
    if (p->device >= 0) return fail(BSK_ERR_INVALID, "bsk_band: the map's tables live on another device");
    const BandMap &q = p->map;
    HIPCHK(p->d_first.reserve(sizeof(int) * q.first.size()));
    HIPCHK(p->d_w.reserve(sizeof(double) * q.w.size()));
    HIPCHK(hipMemcpy(p->d_first.p, q.first.data(), sizeof(int) * q.first.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_w.p, q.w.data(), sizeof(double) * q.w.size(), hipMemcpyHostToDevice));
    p->device = dev;
    return BSK_OK;
}

static bsk_status check_call(bsk_band p, bsk_dtype dtype, const void *in, void *out, int64_t outer, int64_t inner,
                             const char *who)
{
    if (!p) return fail(BSK_ERR_INVALID, std::string(who) + ": map is NULL");
    if (!in || !out) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    if (dtype != BSK_F32 && dtype != BSK_F64) return fail(BSK_ERR_INVALID, std::string(who) + ": dtype must be BSK_F32 or BSK_F64");
    if (outer < 1 || inner < 1) return fail(BSK_ERR_INVALID, std::string(who) + ": outer and inner must be >= 1");
    const double cells = (double)outer * (double)inner * (double)std::max(p->map.nIn, p->map.nOut);
    if (cells > 9.0e15) return fail(BSK_ERR_INVALID, std::string(who) + ": array too large");
    return BSK_OK;
}

template <typename T, int K, int V>
static bsk_status launch_rows(bsk_band p, const T *in, T *out, long long outer, long long inner, hipStream_t st)
{
    const BandMap &q = p->map;
    const long long lanes_i = inner / V;
    int LX = 1;
    while (LX < BAND_BLOCK && LX < lanes_i) LX *= 2;
    const long long LY = BAND_BLOCK / LX;
    const long long tiles_i = (lanes_i + LX - 1) / LX, row_blocks = (q.nOut + BAND_ROWS - 1) / BAND_ROWS;
    const long long blocks_o = (outer + LY - 1) / LY;
    if ((double)tiles_i * (double)row_blocks * (double)blocks_o > 2147483647.0)
        return fail(BSK_ERR_INVALID, "bsk_band_apply: array too large for one launch");
    hipLaunchKernelGGL((band_apply<T, K, V>), dim3((unsigned)(tiles_i * row_blocks * blocks_o)), dim3(BAND_BLOCK), 0, st, in, out,
                       static_cast<const int *>(p->d_first.p), static_cast<const double *>(p->d_w.p), q.nIn, q.nOut, outer,
                       inner, LX, tiles_i, row_blocks);
    HIPCHK(hipGetLastError());
    p->last_kernel = "band_apply";
    return BSK_OK;
}

template <typename T, int K>
static bsk_status launch_line(bsk_band p, const T *in, T *out, long long nlines, hipStream_t st)
{
    const BandMap &q = p->map;
    const int R = std::min(q.nOut, BAND_BLOCK);
    const int G = BAND_BLOCK / R;
    const long long span = q.max_span(R);
    const int staged = span <= LINE_LDS;
    // lines per workgroup: what LDS holds, at most 16 per line group (the weights of a row are read once per workgroup)
    long long NL = staged ? std::min<long long>(LINE_LDS / span, 16LL * G) : G;
    NL = std::max<long long>(1, std::min(NL, nlines));
    const long long tiles = (q.nOut + R - 1) / R, line_blocks = (nlines + NL - 1) / NL;
    if ((double)tiles * (double)line_blocks > 2147483647.0)
        return fail(BSK_ERR_INVALID, "bsk_band_apply: array too large for one launch");
    hipLaunchKernelGGL((band_apply_line<T, K>), dim3((unsigned)(tiles * line_blocks)), dim3(BAND_BLOCK), 0, st, in, out,
                       static_cast<const int *>(p->d_first.p), static_cast<const double *>(p->d_w.p), q.nIn, q.nOut, nlines, R,
                       (int)NL, tiles, staged);
    HIPCHK(hipGetLastError());
    p->last_kernel = "band_apply_line";
    return BSK_OK;
}

template <typename T>
static bsk_status run(bsk_band p, const T *in, T *out, long long outer, long long inner, hipStream_t st)
{
    constexpr int V = 16 / sizeof(T);
    const bool wide = inner % V == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    return with_int<2, 3, 4, 5, 6, 7, 8>(p->map.K, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (inner == 1) return launch_line<T, K>(p, in, out, outer, st);
        if (wide) return launch_rows<T, K, V>(p, in, out, outer, inner, st);
        return launch_rows<T, K, 1>(p, in, out, outer, inner, st);
    });
}

extern "C" bsk_status bsk_band_create(int nIn, int nOut, int K, const int32_t *first, const double *w, bsk_band *out)
{
    if (!first || !w || !out) return fail(BSK_ERR_INVALID, "NULL argument");
    if (K < 1 || K > MAXO) return fail(BSK_ERR_UNSUPPORTED, "bsk_band_create: K must be in [1, BSK_MAX_ORDER]");
    if (nIn < K || nIn > (1 << 26)) return fail(BSK_ERR_INVALID, "bsk_band_create: nIn must be in [K, 2^26]");
    if (nOut < 1 || nOut > (1 << 26)) return fail(BSK_ERR_INVALID, "bsk_band_create: nOut must be in [1, 2^26]");
    for (int j = 0; j < nOut; ++j) {
        if (first[j] < 0 || first[j] > nIn - K) return fail(BSK_ERR_INVALID, "bsk_band_create: first column outside [0, nIn - K]");
        if (j && first[j] < first[j - 1]) return fail(BSK_ERR_INVALID, "bsk_band_create: first columns must be non-decreasing");
    }
    for (size_t i = 0; i < (size_t)nOut * K; ++i)
        if (!std::isfinite(w[i])) return fail(BSK_ERR_INVALID, "bsk_band_create: weight is not finite");
    bsk_band p = new bsk_band_s;
    p->map.nIn = nIn;
    p->map.nOut = nOut;
    p->map.K = K;
    p->map.first.assign(first, first + nOut);
    p->map.w.assign(w, w + (size_t)nOut * K);
    *out = p;
    return BSK_OK;
}

extern "C" bsk_status bsk_band_destroy(bsk_band p)
{
    if (!p) return BSK_OK;
    p->d_first.release();
    p->d_w.release();
    p->d_part.release();
    delete p;
    return BSK_OK;
}

extern "C" const char *bsk_band_last_kernel(bsk_band p) { return p ? p->last_kernel : ""; }

extern "C" bsk_status bsk_band_apply_host(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out)
{
    bsk_status s = check_call(p, dtype, in, out, outer, inner, "bsk_band_apply_host");
    if (s != BSK_OK) return s;
    if (dtype == BSK_F32) p->map.apply_host(static_cast<const float *>(in), outer, inner, static_cast<float *>(out));
    else p->map.apply_host(static_cast<const double *>(in), outer, inner, static_cast<double *>(out));
    p->last_kernel = "host band";
    return BSK_OK;
}

extern "C" bsk_status bsk_band_apply(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out,
                                     void *stream)
{
    bsk_status s = check_call(p, dtype, in, out, outer, inner, "bsk_band_apply");
    if (s != BSK_OK) return s;
    if (p->map.K < 2 || p->map.K > BAND_KMAX)
        return fail(BSK_ERR_UNSUPPORTED, "bsk_band_apply: K outside [2, 8] is applied by bsk_band_apply_host");
    s = upload(p);
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == BSK_F32 ? run<float>(p, static_cast<const float *>(in), static_cast<float *>(out), outer, inner, st)
                            : run<double>(p, static_cast<const double *>(in), static_cast<double *>(out), outer, inner, st);
}

// ---------------------------------------------------------------------------------------------- bsk_band_absmax
constexpr long long ABSMAX_PARTS = 1024;       // partials per (group, row) at most: the fold's loop stays short

static bsk_status check_absmax(bsk_band p, bsk_dtype dtype, const void *in, double *out, int64_t outer, int64_t inner,
                               int64_t groups, const char *who)
{
    bsk_status s = check_call(p, dtype, in, out, outer, inner, who);
    if (s != BSK_OK) return s;
    if (groups < 1 || outer % groups != 0) return fail(BSK_ERR_INVALID, std::string(who) + ": groups must divide outer");
    return BSK_OK;
}

static bsk_status fold(bsk_band p, long long groups, long long P, double *out, hipStream_t st)
{
    const long long jblocks = (p->map.nOut + 63) / 64;
    if ((double)jblocks * (double)groups > 2147483647.0) return fail(BSK_ERR_INVALID, "bsk_band_absmax: array too large for one launch");
    hipLaunchKernelGGL(band_absmax_fold, dim3((unsigned)(jblocks * groups)), dim3(BAND_BLOCK), 0, st,
                       static_cast<const double *>(p->d_part.p), out, p->map.nOut, P, jblocks);
    HIPCHK(hipGetLastError());
    return BSK_OK;
}

template <typename T, int K, int V>
static bsk_status absmax_rows(bsk_band p, const T *in, const T *minus, double *out, long long outer, long long inner,
                              long long groups, hipStream_t st)
{
    const BandMap &q = p->map;
    const long long og = outer / groups;
    const long long lanes_i = inner / V;
    int LX = 1;
    while (LX < BAND_BLOCK && LX < lanes_i) LX *= 2;
    const long long LY = BAND_BLOCK / LX;
    const long long tiles_i = (lanes_i + LX - 1) / LX, row_blocks = (q.nOut + BAND_ROWS - 1) / BAND_ROWS;
    const long long units = ((og + LY - 1) / LY) * tiles_i;
    const long long upw = (units + ABSMAX_PARTS - 1) / ABSMAX_PARTS;
    const long long P = (units + upw - 1) / upw;
    if ((double)P * (double)row_blocks * (double)groups > 2147483647.0 || upw > 2147483647LL)
        return fail(BSK_ERR_INVALID, "bsk_band_absmax: array too large for one launch");
    HIPCHK(p->d_part.reserve(sizeof(double) * (size_t)(groups * P * q.nOut)));
    hipLaunchKernelGGL((band_absmax<T, K, V>), dim3((unsigned)(P * row_blocks * groups)), dim3(BAND_BLOCK), 0, st, in, minus,
                       static_cast<double *>(p->d_part.p), static_cast<const int *>(p->d_first.p),
                       static_cast<const double *>(p->d_w.p), q.nIn, q.nOut, og, inner, LX, tiles_i, row_blocks, units, (int)upw, P);
    HIPCHK(hipGetLastError());
    p->last_kernel = "band_absmax";
    return fold(p, groups, P, out, st);
}

template <typename T, int K>
static bsk_status absmax_line(bsk_band p, const T *in, const T *minus, double *out, long long nlines, long long groups,
                              hipStream_t st)
{
    const BandMap &q = p->map;
    const long long lg = nlines / groups;
    const int R = std::min(q.nOut, BAND_BLOCK);
    const int G = BAND_BLOCK / R;
    const long long span = q.max_span(R);
    const int staged = span <= LINE_LDS;
    long long NL = staged ? std::min<long long>(LINE_LDS / span, 16LL * G) : G;
    NL = std::max<long long>(1, std::min(NL, lg));
    const long long tiles = (q.nOut + R - 1) / R, lblocks = (lg + NL - 1) / NL;
    const long long lbw = (lblocks + ABSMAX_PARTS - 1) / ABSMAX_PARTS;
    const long long P = (lblocks + lbw - 1) / lbw;
    if ((double)tiles * (double)P * (double)groups > 2147483647.0 || lbw > 2147483647LL)
        return fail(BSK_ERR_INVALID, "bsk_band_absmax: array too large for one launch");
    HIPCHK(p->d_part.reserve(sizeof(double) * (size_t)(groups * P * q.nOut)));
    hipLaunchKernelGGL((band_absmax_line<T, K>), dim3((unsigned)(tiles * P * groups)), dim3(BAND_BLOCK), 0, st, in, minus,
                       static_cast<double *>(p->d_part.p), static_cast<const int *>(p->d_first.p),
                       static_cast<const double *>(p->d_w.p), q.nIn, q.nOut, lg, R, (int)NL, tiles, staged, lblocks, (int)lbw, P);
    HIPCHK(hipGetLastError());
    p->last_kernel = "band_absmax_line";
    return fold(p, groups, P, out, st);
}

template <typename T>
static bsk_status run_absmax(bsk_band p, const T *in, const T *minus, double *out, long long outer, long long inner,
                             long long groups, hipStream_t st)
{
    constexpr int V = 16 / sizeof(T);
    const bool wide = inner % V == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(minus) % 16 == 0;
    return with_int<2, 3, 4, 5, 6, 7, 8>(p->map.K, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (inner == 1) return absmax_line<T, K>(p, in, minus, out, outer, groups, st);
        if (wide) return absmax_rows<T, K, V>(p, in, minus, out, outer, inner, groups, st);
        return absmax_rows<T, K, 1>(p, in, minus, out, outer, inner, groups, st);
    });
}

extern "C" bsk_status bsk_band_apply_fma_host(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out)
{
    bsk_status s = check_call(p, dtype, in, out, outer, inner, "bsk_band_apply_fma_host");
    if (s != BSK_OK) return s;
    if (dtype == BSK_F32) p->map.apply_fma_host(static_cast<const float *>(in), outer, inner, static_cast<float *>(out));
    else p->map.apply_fma_host(static_cast<const double *>(in), outer, inner, static_cast<double *>(out));
    p->last_kernel = "host band";
    return BSK_OK;
}

extern "C" bsk_status bsk_band_absmax_host(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner,
                                           int64_t groups, const void *minus, double *out)
{
    bsk_status s = check_absmax(p, dtype, in, out, outer, inner, groups, "bsk_band_absmax_host");
    if (s != BSK_OK) return s;
    if (dtype == BSK_F32)
        p->map.absmax_host(static_cast<const float *>(in), outer, inner, groups, static_cast<const float *>(minus), out);
    else p->map.absmax_host(static_cast<const double *>(in), outer, inner, groups, static_cast<const double *>(minus), out);
    p->last_kernel = "host band_absmax";
    return BSK_OK;
}

extern "C" bsk_status bsk_band_absmax(bsk_band p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, int64_t groups,
                                      const void *minus, double *out, void *stream)
{
    bsk_status s = check_absmax(p, dtype, in, out, outer, inner, groups, "bsk_band_absmax");
    if (s != BSK_OK) return s;
    if (p->map.K < 2 || p->map.K > BAND_KMAX)
        return fail(BSK_ERR_UNSUPPORTED, "bsk_band_absmax: K outside [2, 8] is covered by bsk_band_absmax_host");
    s = upload(p);
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == BSK_F32 ? run_absmax<float>(p, static_cast<const float *>(in), static_cast<const float *>(minus), out, outer, inner, groups, st)
                            : run_absmax<double>(p, static_cast<const double *>(in), static_cast<const double *>(minus), out, outer, inner, groups, st);
}
