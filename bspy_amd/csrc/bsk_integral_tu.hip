// Spline.integral on the device (bsk_integral.hpp): one Gauss-Kronrod round over a batch of regions.  The adaptive
// driver (which regions to split) runs in Python, bspy_amd/integral.py.  18 instantiations: fp32 / fp64 x nInd 1 - 3
// x order bucket 4 / 8 / 16 (per-variable orders are run-time values up to the bucket).
#include "bsk_host.hpp"
#include "bsk_integral.hpp"

template <typename T, int NIND, int OMAX>
static void launch_integral(bsk_spline s, const T *lo_hi, const int *span, long long nreg, int mode, double *out,
                            hipStream_t st)
{
    hipLaunchKernelGGL((integral_regions<T, NIND, OMAX>), dim3((unsigned)nreg), dim3(IntegralShape<NIND>::BLOCK), 0, st,
                       desc_of<T>(s), static_cast<const T *>(s->tab), static_cast<const T *>(s->coef), lo_hi, span, mode,
                       out);
}

template <typename T, int NIND>
static void launch_integral_nind(bsk_spline s, int omax, const T *lo_hi, const int *span, long long nreg, int mode,
                                 double *out, hipStream_t st)
{
    if (omax <= 4) launch_integral<T, NIND, 4>(s, lo_hi, span, nreg, mode, out, st);
    else if (omax <= 8) launch_integral<T, NIND, 8>(s, lo_hi, span, nreg, mode, out, st);
    else launch_integral<T, NIND, 16>(s, lo_hi, span, nreg, mode, out, st);
}

template <typename T>
static bsk_status run_integral(bsk_spline s, int mode, const void *lo_hi, const int32_t *span, long long nreg, void *out,
                               hipStream_t st)
{
    const int nInd = s->nInd;
    int omax = 0;
    for (int iv = 0; iv < nInd; ++iv) omax = std::max(omax, s->order[iv]);
    const long long nn = nInd == 1 ? GK_N : nInd == 2 ? GK_N * GK_N : GK_N * GK_N * GK_N;
    const size_t bounds_bytes = sizeof(T) * (size_t)nreg * nInd * 2;
    const size_t span_off = (bounds_bytes + 255) & ~(size_t)255;
    const size_t in_bytes = span_off + sizeof(int32_t) * (size_t)nreg * nInd;
    const size_t out_bytes = sizeof(double) * (size_t)nreg * (mode == IQ_NODES ? nn * (s->nDep + 2) : 2);
    HIPCHK(s->in_ws.reserve(in_bytes));
    HIPCHK(s->out_ws.reserve(out_bytes));
    char *in = static_cast<char *>(s->in_ws.p);
    HIPCHK(hipMemcpyAsync(in, lo_hi, bounds_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + span_off, span, sizeof(int32_t) * (size_t)nreg * nInd, hipMemcpyHostToDevice, st));
    const T *dlh = reinterpret_cast<const T *>(in);
    const int *dsp = reinterpret_cast<const int *>(in + span_off);
    double *dout = static_cast<double *>(s->out_ws.p);
    stage_mark(s, st, "start", true);
    if (nInd == 1) launch_integral_nind<T, 1>(s, omax, dlh, dsp, nreg, mode, dout, st);
    else if (nInd == 2) launch_integral_nind<T, 2>(s, omax, dlh, dsp, nreg, mode, dout, st);
    else launch_integral_nind<T, 3>(s, omax, dlh, dsp, nreg, mode, dout, st);
    HIPCHK(hipGetLastError());
    stage_mark(s, st, "integral_regions");
    s->last_kernel = "integral_regions";
    HIPCHK(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return BSK_OK;
}

extern "C" bsk_status bsk_integral(bsk_spline s, int mode, const void *lo_hi, const int32_t *span, int64_t nreg, void *out,
                                   void *stream)
{
    if (!s) return fail(BSK_ERR_INVALID, "spline is NULL");
    if (s->nInd < 1 || s->nInd > 3) return fail(BSK_ERR_UNSUPPORTED, "bsk_integral: nInd must be 1, 2 or 3");
    if (mode != BSK_INTEGRAL_MEASURE && mode != BSK_INTEGRAL_NODES) return fail(BSK_ERR_INVALID, "bsk_integral: unknown mode");
    if (nreg < 0 || nreg > 0x7fffffffLL) return fail(BSK_ERR_INVALID, "bsk_integral: region count outside [0, 2^31)");
    if (nreg == 0) return BSK_OK;
    if (!lo_hi || !span || !out) return fail(BSK_ERR_INVALID, "NULL argument");
    // every window the kernel reads lies inside the coefficient table: order <= span <= nCoef
    for (int64_t r = 0; r < nreg; ++r)
        for (int iv = 0; iv < s->nInd; ++iv) {
            const int32_t ix = span[r * s->nInd + iv];
            if (ix < s->order[iv] || ix > s->ncoef[iv])
                return fail(BSK_ERR_INVALID, "bsk_integral: span index outside [order, nCoef]");
        }
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    return s->dtype == BSK_F32 ? run_integral<float>(s, mode, lo_hi, span, nreg, out, st)
                               : run_integral<double>(s, mode, lo_hi, span, nreg, out, st);
}
