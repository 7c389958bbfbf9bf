// Running sums and broadcast sums of coefficient tensors (bsk_sum.hpp): the bsk_scan_* and bsk_sum_* entry points.
// A scan map is host data and bsk_scan_create makes no HIP call; its weights go to the device with the first device
// call on the handle, and the handle owns the workspace of the two-launch path.
// Instantiations: scan_apply fp32 / fp64 x (16-byte lanes, scalar lanes) x (totals, write), scan_line fp32 / fp64 x
// (totals, write), sum_bcast fp32 / fp64 x (16-byte lanes, scalar lanes).
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_sum.hpp"

using namespace bsksum;

struct bsk_scan_s {
    ScanMap map;
    int device = -1;                   // device the weights live on (-1: not uploaded)
    DevBuf d_g, ws;
    const char *last_kernel = "";
};

static thread_local const char *g_sum_kernel = "";

static bsk_status upload(bsk_scan p)
{
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (p->device == dev) return BSK_OK;
    if (p->device >= 0) return fail(BSK_ERR_INVALID, "bsk_scan: the map's weights live on another device");
    HIPCHK(p->d_g.reserve(sizeof(double) * p->map.g.size()));
    HIPCHK(hipMemcpy(p->d_g.p, p->map.g.data(), sizeof(double) * p->map.g.size(), hipMemcpyHostToDevice));
    p->device = dev;
    return BSK_OK;
}

static bsk_status check_call(bsk_scan p, bsk_dtype dtype, const void *in, void *out, int64_t outer, int64_t inner,
                             const char *who)
{
    if (!p) return fail(BSK_ERR_INVALID, std::string(who) + ": map is NULL");
    if (!in || !out) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    if (dtype != BSK_F32 && dtype != BSK_F64) return fail(BSK_ERR_INVALID, std::string(who) + ": dtype must be BSK_F32 or BSK_F64");
    if (outer < 1 || inner < 1) return fail(BSK_ERR_INVALID, std::string(who) + ": outer and inner must be >= 1");
    if ((double)outer * (double)inner * ((double)p->map.n + 1.0) > 9.0e15)
        return fail(BSK_ERR_INVALID, std::string(who) + ": array too large");
    return BSK_OK;
}

static inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// inner > 1.  segments: 0 = choose, else the wanted number of segments (rounded to whole chunks).
template <typename T, int V>
static bsk_status launch_rows(bsk_scan p, const T *in, T *out, long long outer, long long inner, int segments, hipStream_t st)
{
    const int n = p->map.n;
    const int nchunks = (int)ceil_div(n, SCAN_CHUNK);
    const long long lanes = outer * (inner / V);
    long long want = segments > 0 ? segments : std::min<long long>(SCAN_MAX_SEGMENTS, ceil_div(SCAN_LANES_WANTED, lanes));
    want = std::max<long long>(1, std::min<long long>(want, nchunks));
    const int cps = (int)ceil_div(nchunks, want);
    const int nseg = (int)ceil_div(nchunks, cps);
    const long long blocks = ceil_div(lanes, SCAN_BLOCK);
    if (blocks > 2147483647LL || nseg > 65535) return fail(BSK_ERR_INVALID, "bsk_scan_apply: array too large for one launch");
    const double *g = static_cast<const double *>(p->d_g.p);
    double *ws = nullptr;
    if (nseg > 1) {
        HIPCHK(p->ws.reserve(sizeof(double) * (size_t)outer * (size_t)nchunks * (size_t)inner));
        ws = static_cast<double *>(p->ws.p);
        hipLaunchKernelGGL((scan_apply<T, V, true>), dim3((unsigned)blocks, (unsigned)(nseg - 1)), dim3(SCAN_BLOCK), 0, st, in, out,
                           g, ws, n, outer, inner, nchunks, cps);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL((scan_apply<T, V, false>), dim3((unsigned)blocks, (unsigned)nseg), dim3(SCAN_BLOCK), 0, st, in, out, g, ws, n,
                       outer, inner, nchunks, cps);
    HIPCHK(hipGetLastError());
    p->last_kernel = "scan_apply";
    return BSK_OK;
}

template <typename T>
static bsk_status launch_line(bsk_scan p, const T *in, T *out, long long nlines, int segments, hipStream_t st)
{
    const int n = p->map.n;
    const int nchunks = (int)ceil_div(n, SCAN_CHUNK);
    int cps;
    if (segments > 0) {
        cps = (int)std::min<long long>(LINE_BLOCK, ceil_div(nchunks, std::min(segments, nchunks)));
    } else {
        // whole tiles; lines too few to fill the device are split further, down to 8 chunks a segment
        cps = std::min(nchunks, LINE_BLOCK);
        while (cps > 8 && ceil_div(nlines, std::max(1, LINE_BLOCK / cps)) * ceil_div(nchunks, cps) < LINE_WG_WANTED) cps = (cps + 1) / 2;
    }
    const int nseg = (int)ceil_div(nchunks, cps);
    const int NL = (int)std::max<long long>(1, std::min<long long>(LINE_BLOCK / cps, nlines));
    const long long blocks = ceil_div(nlines, NL) * nseg;
    if (blocks > 2147483647LL) return fail(BSK_ERR_INVALID, "bsk_scan_apply: array too large for one launch");
    const double *g = static_cast<const double *>(p->d_g.p);
    double *ws = nullptr;
    if (nseg > 1) {
        HIPCHK(p->ws.reserve(sizeof(double) * (size_t)nlines * (size_t)nchunks));
        ws = static_cast<double *>(p->ws.p);
        hipLaunchKernelGGL((scan_line<T, true>), dim3((unsigned)blocks), dim3(LINE_BLOCK), 0, st, in, out, g, ws, n, nlines, nchunks,
                           cps, NL, nseg);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL((scan_line<T, false>), dim3((unsigned)blocks), dim3(LINE_BLOCK), 0, st, in, out, g, ws, n, nlines, nchunks, cps,
                       NL, nseg);
    HIPCHK(hipGetLastError());
    p->last_kernel = "scan_line";
    return BSK_OK;
}

template <typename T>
static bsk_status run_scan(bsk_scan p, const T *in, T *out, long long outer, long long inner, int segments, hipStream_t st)
{
    constexpr int V = 16 / sizeof(T);
    if (inner == 1) return launch_line<T>(p, in, out, outer, segments, st);
    const bool wide = inner % V == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (wide) return launch_rows<T, V>(p, in, out, outer, inner, segments, st);
    return launch_rows<T, 1>(p, in, out, outer, inner, segments, st);
}

extern "C" bsk_status bsk_scan_create(int n, const double *g, bsk_scan *out)
{
    if (!g || !out) return fail(BSK_ERR_INVALID, "NULL argument");
    if (n < 1 || n > (1 << 26)) return fail(BSK_ERR_INVALID, "bsk_scan_create: n must be in [1, 2^26]");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(g[i])) return fail(BSK_ERR_INVALID, "bsk_scan_create: weight is not finite");
    bsk_scan p = new bsk_scan_s;
    p->map.n = n;
    p->map.g.assign(g, g + n);
    *out = p;
    return BSK_OK;
}

extern "C" bsk_status bsk_scan_destroy(bsk_scan p)
{
    if (!p) return BSK_OK;
    p->d_g.release();
    p->ws.release();
    delete p;
    return BSK_OK;
}

extern "C" const char *bsk_scan_last_kernel(bsk_scan p) { return p ? p->last_kernel : ""; }

extern "C" bsk_status bsk_scan_apply_host(bsk_scan p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out)
{
    bsk_status s = check_call(p, dtype, in, out, outer, inner, "bsk_scan_apply_host");
    if (s != BSK_OK) return s;
    if (dtype == BSK_F32) p->map.apply_host(static_cast<const float *>(in), outer, inner, static_cast<float *>(out));
    else p->map.apply_host(static_cast<const double *>(in), outer, inner, static_cast<double *>(out));
    p->last_kernel = "host scan";
    return BSK_OK;
}

extern "C" bsk_status bsk_scan_apply(bsk_scan p, bsk_dtype dtype, const void *in, int64_t outer, int64_t inner, void *out,
                                     int segments, void *stream)
{
    bsk_status s = check_call(p, dtype, in, out, outer, inner, "bsk_scan_apply");
    if (s != BSK_OK) return s;
    if (segments < 0) return fail(BSK_ERR_INVALID, "bsk_scan_apply: segments must be >= 0");
    s = upload(p);
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == BSK_F32 ? run_scan<float>(p, static_cast<const float *>(in), static_cast<float *>(out), outer, inner, segments, st)
                            : run_scan<double>(p, static_cast<const double *>(in), static_cast<double *>(out), outer, inner, segments, st);
}

// ------------------------------------------------------------------------------------------ broadcast sum
static bsk_status sum_desc(int rank, const int64_t *dim, const int64_t *sa, const int64_t *sb, int sign, const void *a,
                           const void *b, void *out, bsk_dtype dtype, const char *who, SumDesc &d)
{
    if (!dim || !sa || !sb || !a || !b || !out) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    if (dtype != BSK_F32 && dtype != BSK_F64) return fail(BSK_ERR_INVALID, std::string(who) + ": dtype must be BSK_F32 or BSK_F64");
    if (rank < 1) return fail(BSK_ERR_INVALID, std::string(who) + ": rank must be >= 1");
    if (rank > SUM_MAX_RANK) return fail(BSK_ERR_UNSUPPORTED, std::string(who) + ": rank above 8 (merge adjacent axes first)");
    if (sign != 1 && sign != -1) return fail(BSK_ERR_INVALID, std::string(who) + ": sign must be +1 or -1");
    double total = 1.0;
    const int pad = SUM_MAX_RANK - rank;
    for (int ax = 0; ax < SUM_MAX_RANK; ++ax) {
        d.dim[ax] = ax < pad ? 1 : dim[ax - pad];
        d.sa[ax] = ax < pad ? 0 : sa[ax - pad];
        d.sb[ax] = ax < pad ? 0 : sb[ax - pad];
        if (d.dim[ax] < 1 || d.sa[ax] < 0 || d.sb[ax] < 0)
            return fail(BSK_ERR_INVALID, std::string(who) + ": extents must be >= 1 and strides >= 0");
        total *= (double)d.dim[ax];
    }
    if (total > 9.0e15) return fail(BSK_ERR_INVALID, std::string(who) + ": array too large");
    return BSK_OK;
}

template <typename T>
static bsk_status run_sum(const T *a, const T *b, T *out, const SumDesc &d, double sign, hipStream_t st)
{
    constexpr int V = 16 / sizeof(T);
    constexpr int L = SUM_MAX_RANK - 1;
    long long rows = 1;
    for (int ax = 0; ax < L; ++ax) rows *= d.dim[ax];
    if (rows > 4294967295LL) return fail(BSK_ERR_INVALID, "bsk_sum_apply: array too large for one launch");
    auto fits = [&](const T *p, const long long *s) {
        if (s[L] == 0) return true;
        if (s[L] != 1 || reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
        for (int ax = 0; ax < L; ++ax)
            if (d.dim[ax] > 1 && s[ax] % V != 0) return false;
        return true;
    };
    const bool wide = d.dim[L] % V == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 && fits(a, d.sa) && fits(b, d.sb);
    const long long lanes_last = wide ? d.dim[L] / V : d.dim[L];
    const long long lanes = rows * lanes_last;
    const long long blocks = (lanes + SUM_BLOCK - 1) / SUM_BLOCK;
    if (blocks > 2147483647LL) return fail(BSK_ERR_INVALID, "bsk_sum_apply: array too large for one launch");
    if (wide)
        hipLaunchKernelGGL((sum_bcast<T, V>), dim3((unsigned)blocks), dim3(SUM_BLOCK), 0, st, a, b, out, d, sign, lanes_last, lanes);
    else
        hipLaunchKernelGGL((sum_bcast<T, 1>), dim3((unsigned)blocks), dim3(SUM_BLOCK), 0, st, a, b, out, d, sign, lanes_last, lanes);
    HIPCHK(hipGetLastError());
    g_sum_kernel = "sum_bcast";
    return BSK_OK;
}

extern "C" const char *bsk_sum_last_kernel(void) { return g_sum_kernel; }

extern "C" bsk_status bsk_sum_apply_host(bsk_dtype dtype, int rank, const int64_t *dim, const void *a, const int64_t *strideA,
                                         const void *b, const int64_t *strideB, int sign, void *out)
{
    SumDesc d;
    bsk_status s = sum_desc(rank, dim, strideA, strideB, sign, a, b, out, dtype, "bsk_sum_apply_host", d);
    if (s != BSK_OK) return s;
    if (dtype == BSK_F32) sum_host(static_cast<const float *>(a), static_cast<const float *>(b), static_cast<float *>(out), d, (double)sign);
    else sum_host(static_cast<const double *>(a), static_cast<const double *>(b), static_cast<double *>(out), d, (double)sign);
    g_sum_kernel = "host sum";
    return BSK_OK;
}

extern "C" bsk_status bsk_sum_apply(bsk_dtype dtype, int rank, const int64_t *dim, const void *a, const int64_t *strideA,
                                    const void *b, const int64_t *strideB, int sign, void *out, void *stream)
{
    SumDesc d;
    bsk_status s = sum_desc(rank, dim, strideA, strideB, sign, a, b, out, dtype, "bsk_sum_apply", d);
    if (s != BSK_OK) return s;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == BSK_F32 ? run_sum<float>(static_cast<const float *>(a), static_cast<const float *>(b), static_cast<float *>(out), d, (double)sign, st)
                            : run_sum<double>(static_cast<const double *>(a), static_cast<const double *>(b), static_cast<double *>(out), d, (double)sign, st);
}
