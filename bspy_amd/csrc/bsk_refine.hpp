// Spline to spline (bspy_amd/refinement.py): knot insertion, degree elevation, trim and differentiation of one variable
// are each one banded linear operator, the same for every line of the coefficient tensor along that variable.
//
//   BandMap          host: out[j] = sum_t w[j][t] * in[first[j] + t], j < nOut, t < K; first is non-decreasing and
//                    first[j] + K <= nIn.  The operator is built by the caller (refinement.py builds it by blossoming)
//                    and does not depend on the data.  apply_line is one line on the host and states what the kernels
//                    compute: the K products are added in the order t = 0 .. K - 1 in fp64 and rounded once.
//   band_apply       device, inner > 1: data viewed as [outer, nIn, inner] -> [outer, nOut, inner], lanes run along
//                    `inner` (V elements = 16 bytes per lane where the alignment allows), a workgroup owns BAND_ROWS
//                    output rows of BAND_BLOCK / LX values of `outer`.  Rows are independent: no serial walk over the
//                    whole line, only a rolling register window of K input values while the block's rows advance.
//                    first and w of the block are wave-uniform: staged in LDS once, read at uniform addresses.
//   band_apply_line  device, inner == 1 (the last variable: lines are contiguous): a workgroup stages the piece
//                    in[first[j0] .. first[j1 - 1] + K - 1] of NL lines in LDS with coalesced reads, then lane j
//                    produces output row j of its lines from LDS addresses first[j] - first[j0] + t, near-consecutive
//                    across lanes.  A lane keeps the K weights of its row in registers over its lines.  No transposes.
//
// Input fp32 or fp64, weights and accumulation fp64, output in the input's type.  No atomics: a result does not depend
// on the launch geometry's timing, and the sum order is the one of apply_line for every path.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace bskband {

constexpr int BAND_KMAX = 8;       // largest K with a device instantiation (as FIT_KMAX)
constexpr int BAND_BLOCK = 256;    // lanes per workgroup of both kernels
constexpr int BAND_ROWS = 32;      // output rows per workgroup of band_apply: enough workgroups to fill the CUs at 2048^2
constexpr int LINE_LDS = 4096;     // elements of the input type staged per workgroup of band_apply_line

struct BandMap {
    int nIn = 0, nOut = 0, K = 0;
    std::vector<int> first;        // nOut
    std::vector<double> w;         // nOut * K

    // in[row * istride] -> out[row * ostride]
    template <typename T>
    void apply_line(const T *in, long long istride, T *out, long long ostride) const
    {
        for (int j = 0; j < nOut; ++j) {
            const T *p = in + (long long)first[j] * istride;
            double acc = 0.0;
            for (int t = 0; t < K; ++t) acc += w[(size_t)j * K + t] * (double)p[(long long)t * istride];
            out[(long long)j * ostride] = (T)acc;
        }
    }

    // host driver over [outer, nIn, inner] -> [outer, nOut, inner]
    template <typename T>
    void apply_host(const T *in, long long outer, long long inner, T *out) const
    {
        for (long long o = 0; o < outer; ++o)
            for (long long i = 0; i < inner; ++i) apply_line(in + o * nIn * inner + i, inner, out + o * nOut * inner + i, inner);
    }

    // Largest number of input rows under a tile of `rows` consecutive output rows (band_apply_line stages that piece).
    long long max_span(int rows) const
    {
        long long m = 0;
        for (int j0 = 0; j0 < nOut; j0 += rows) {
            const int j1 = j0 + rows < nOut ? j0 + rows : nOut;
            const long long s = (long long)first[j1 - 1] + K - first[j0];
            if (s > m) m = s;
        }
        return m;
    }
};

#ifdef __HIPCC__
template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

// in: [outer, nIn, inner], out: [outer, nOut, inner].  Workgroup = (outer block, inner tile, row block); lane =
// (outer within the block, inner within the tile): LX lanes (a power of two) along inner, BAND_BLOCK / LX along outer.
// V divides inner and both pointers are V * sizeof(T) aligned when V > 1 (the launcher checks).
// Every lane walks the same rows, so the window moves under wave-uniform control; lanes past the end of outer or
// inner load and store nothing.  Reads stay in bounds because first[j] + K <= nIn for every row (bsk_band_create).
template <typename T, int K, int V>
__global__ __launch_bounds__(BAND_BLOCK) void band_apply(const T *__restrict__ in, T *__restrict__ out,
                                                         const int *__restrict__ first, const double *__restrict__ w,
                                                         int nIn, int nOut, long long outer, long long inner, int LX,
                                                         long long tiles_i, long long row_blocks)
{
    __shared__ double sw[BAND_ROWS * K];
    __shared__ int sfirst[BAND_ROWS];
    const int tid = threadIdx.x;
    const long long rb = blockIdx.x % row_blocks;
    const long long rest = blockIdx.x / row_blocks;
    const long long it = rest % tiles_i, ob = rest / tiles_i;
    const int j0 = (int)rb * BAND_ROWS;
    const int rows = nOut - j0 < BAND_ROWS ? nOut - j0 : BAND_ROWS;

    // stage the block's weights and first columns; every word is written (zeros / the last row's column past the end)
    for (int idx = tid; idx < BAND_ROWS * K; idx += BAND_BLOCK) sw[idx] = idx < rows * K ? w[(long long)j0 * K + idx] : 0.0;
    if (tid < BAND_ROWS) sfirst[tid] = first[j0 + (tid < rows ? tid : rows - 1)];
    __syncthreads();

    const int LY = BAND_BLOCK / LX;
    const long long o = ob * LY + tid / LX;
    const long long ii = (it * LX + tid % LX) * V;
    const bool live = o < outer && ii < inner;
    const T *src = in + (live ? o * nIn * inner + ii : 0);
    T *dst = out + (live ? o * nOut * inner + ii : 0);
    using P = Pack<T, V>;

    P win[K];
    int f = sfirst[0];
#pragma unroll
    for (int t = 0; t < K; ++t)
        if (live) win[t] = *reinterpret_cast<const P *>(src + (long long)(f + t) * inner);
    for (int q = 0; q < rows; ++q) {
        const int fj = __builtin_amdgcn_readfirstlane(sfirst[q]);
        while (f < fj) {                               // uniform: the window moves one input row on
#pragma unroll
            for (int t = 0; t + 1 < K; ++t) win[t] = win[t + 1];
            if (live) win[K - 1] = *reinterpret_cast<const P *>(src + (long long)(f + K) * inner);
            ++f;
        }
        double acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const double wt = sw[q * K + t];
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += wt * (double)win[t].v[e];
        }
        P r;
#pragma unroll
        for (int e = 0; e < V; ++e) r.v[e] = (T)acc[e];
        if (live) *reinterpret_cast<P *>(dst + (long long)(j0 + q) * inner) = r;
    }
}

// in: [nlines, nIn], out: [nlines, nOut].  Workgroup = (line block of NL lines, tile of R output rows); lane =
// (line group g = tid / R, row r = tid % R), G = BAND_BLOCK / R line groups; group g takes lines g, g + G, ... < NL.
// The piece of the NL lines under the tile is staged in LDS when staged != 0 (the launcher guarantees NL * span <=
// LINE_LDS for every tile then); otherwise (a band map whose rows jump far) the lanes read the input where it is.
// An LDS word is read only for a line < nlines and a column < span: exactly the words the staging loop writes.
template <typename T, int K>
__global__ __launch_bounds__(BAND_BLOCK) void band_apply_line(const T *__restrict__ in, T *__restrict__ out,
                                                              const int *__restrict__ first, const double *__restrict__ w,
                                                              int nIn, int nOut, long long nlines, int R, int NL,
                                                              long long tiles, int staged)
{
    __shared__ T piece[LINE_LDS];
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x % tiles, lb = blockIdx.x / tiles;
    const int j0 = (int)tile * R;
    const int rows = nOut - j0 < R ? nOut - j0 : R;
    const long long line0 = lb * NL;
    const int base = first[j0];
    const int span = first[j0 + rows - 1] + K - base;
    const int nl = nlines - line0 < NL ? (int)(nlines - line0) : NL;

    if (staged) {
        const int total = nl * span;
        for (int idx = tid; idx < total; idx += BAND_BLOCK) {
            const int l = idx / span, c = idx - l * span;
            piece[idx] = in[(line0 + l) * nIn + base + c];
        }
        __syncthreads();
    }
    const int G = BAND_BLOCK / R;
    const int g = tid / R, r = tid - g * R;
    if (g >= G || r >= rows) return;
    const int j = j0 + r;
    const int off = first[j] - base;
    double wt[K];
#pragma unroll
    for (int t = 0; t < K; ++t) wt[t] = w[(long long)j * K + t];
    for (int l = g; l < nl; l += G) {
        double acc = 0.0;
        if (staged) {
            const T *p = piece + l * span + off;
#pragma unroll
            for (int t = 0; t < K; ++t) acc += wt[t] * (double)p[t];
        } else {
            const T *p = in + (line0 + l) * nIn + base + off;
#pragma unroll
            for (int t = 0; t < K; ++t) acc += wt[t] * (double)p[t];
        }
        out[(line0 + l) * nOut + j] = (T)acc;
    }
}
#endif

}  // namespace bskband
