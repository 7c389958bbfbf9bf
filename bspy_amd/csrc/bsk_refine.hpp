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
//   band_absmax      device, inner > 1 (bspy_amd/reduction.py): the operator is applied as in band_apply, but no result is
//                    written: per output row j and group g (the leading part of `outer`) the kernel keeps
//                    max | round_T(sum_t w[j][t] in[first[j] + t]) - minus |.  A lane folds the rows of its block over
//                    its share of (outer, inner tiles) in BAND_ROWS registers; then a wave reduction by lane exchange,
//                    one LDS word per (wave, row), and one plain store of a partial per (workgroup, group, row).
//   band_absmax_line device, inner == 1: band_apply_line's staging; lane (g, r) keeps the maximum of row r over its
//                    lines, the line groups are combined through LDS, one partial per (workgroup, group, row).
//   band_absmax_fold the second launch: out[g][j] = max over the partials of (g, j).  A maximum is exact and a NaN is
//                    turned into +inf where it arises, so the result does not depend on the launch geometry.
//
// Input fp32 or fp64, weights and accumulation fp64, output in the input's type.  No atomics: a result does not depend
// on the launch geometry's timing, and the sum order is the one of apply_line for every path.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
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

    // The statement of the band kernels' arithmetic on the host: the chain acc = fma(w[t], x[t], acc) from 0 in the
    // order of t (the kernels' sums are fused), rounded once to T.
    template <typename T>
    double fma_row(int j, const T *p, long long istride) const
    {
        double acc = 0.0;
        for (int t = 0; t < K; ++t) acc = std::fma(w[(size_t)j * K + t], (double)p[(long long)t * istride], acc);
        return acc;
    }

    template <typename T>
    void apply_fma_host(const T *in, long long outer, long long inner, T *out) const
    {
        for (long long o = 0; o < outer; ++o)
            for (int j = 0; j < nOut; ++j)
                for (long long i = 0; i < inner; ++i)
                    out[(o * nOut + j) * inner + i] = (T)fma_row(j, in + (o * nIn + first[j]) * inner + i, inner);
    }

    // |x| for a maximum: a NaN counts as +inf
    static double magnitude(double x)
    {
        const double a = std::fabs(x);
        return a <= DBL_MAX ? a : HUGE_VAL;
    }

    // out[g][j] = max over the lines of group g of | round_T(row j) - minus |; minus may be null
    template <typename T>
    void absmax_host(const T *in, long long outer, long long inner, long long groups, const T *minus, double *out) const
    {
        const long long og = outer / groups;
        for (long long g = 0; g < groups; ++g)
            for (int j = 0; j < nOut; ++j) {
                double m = 0.0;
                for (long long o = g * og; o < (g + 1) * og; ++o)
                    for (long long i = 0; i < inner; ++i) {
                        double r = (double)(T)fma_row(j, in + (o * nIn + first[j]) * inner + i, inner);
                        if (minus) r -= (double)minus[(o * nOut + j) * inner + i];
                        const double a = magnitude(r);
                        m = a > m ? a : m;
                    }
                out[g * nOut + j] = m;
            }
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
// ---------------------------------------------------------------------------------------------- maxima of a band operator
__device__ __forceinline__ double band_magnitude(double x)
{
    const double a = fabs(x);
    return a <= DBL_MAX ? a : HUGE_VAL;       // NaN -> +inf
}

// band_apply's geometry inside one group of `og` values of outer: a unit is (outer block, inner tile), workgroup p of
// the group takes the units p * upw .. and walks its BAND_ROWS rows for each.  part: [groups][P][nOut].
// minus: null or [outer, nOut, inner]; V-aligned like in when V > 1 (the launcher checks).
template <typename T, int K, int V>
__global__ __launch_bounds__(BAND_BLOCK) void band_absmax(const T *__restrict__ in, const T *__restrict__ minus,
                                                          double *__restrict__ part, const int *__restrict__ first,
                                                          const double *__restrict__ w, int nIn, int nOut, long long og,
                                                          long long inner, int LX, long long tiles_i, long long row_blocks,
                                                          long long units, int upw, long long P)
{
    __shared__ double sw[BAND_ROWS * K];
    __shared__ int sfirst[BAND_ROWS];
    __shared__ double sred[BAND_BLOCK / 64][BAND_ROWS];
    const int tid = threadIdx.x;
    const long long rb = blockIdx.x % row_blocks;
    const long long rest = blockIdx.x / row_blocks;
    const long long p = rest % P, g = rest / P;
    const int j0 = (int)rb * BAND_ROWS;
    const int rows = nOut - j0 < BAND_ROWS ? nOut - j0 : BAND_ROWS;

    for (int idx = tid; idx < BAND_ROWS * K; idx += BAND_BLOCK) sw[idx] = idx < rows * K ? w[(long long)j0 * K + idx] : 0.0;
    if (tid < BAND_ROWS) sfirst[tid] = first[j0 + (tid < rows ? tid : rows - 1)];
    __syncthreads();

    const int LY = BAND_BLOCK / LX;
    using Pk = Pack<T, V>;
    double rmax[BAND_ROWS];
#pragma unroll
    for (int q = 0; q < BAND_ROWS; ++q) rmax[q] = 0.0;

    const long long u1 = (p + 1) * upw < units ? (p + 1) * upw : units;
    for (long long u = p * upw; u < u1; ++u) {
        // the weights are read from LDS where they are used: hoisted out of this loop they would take 2 K BAND_ROWS registers
        asm volatile("" ::: "memory");
        const long long it = u % tiles_i, ob = u / tiles_i;
        const long long ol = ob * LY + tid / LX;
        const long long ii = (it * LX + tid % LX) * V;
        const bool live = ol < og && ii < inner;
        const long long o = g * og + ol;
        const T *src = in + (live ? o * nIn * inner + ii : 0);
        const T *sub = minus ? minus + (live ? o * nOut * inner + ii : 0) : nullptr;

        Pk win[K];
        int f = sfirst[0];
#pragma unroll
        for (int t = 0; t < K; ++t) {
#pragma unroll
            for (int e = 0; e < V; ++e) win[t].v[e] = (T)0;
            if (live) win[t] = *reinterpret_cast<const Pk *>(src + (long long)(f + t) * inner);
        }
#pragma unroll
        for (int q = 0; q < BAND_ROWS; ++q) {
            if (q < rows) {                                    // uniform
                const int fj = __builtin_amdgcn_readfirstlane(sfirst[q]);
                while (f < fj) {
#pragma unroll
                    for (int t = 0; t + 1 < K; ++t) win[t] = win[t + 1];
                    if (live) win[K - 1] = *reinterpret_cast<const Pk *>(src + (long long)(f + K) * inner);
                    ++f;
                }
                double acc[V];
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] = 0.0;
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    const double wt = sw[q * K + t];
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] = fma(wt, (double)win[t].v[e], acc[e]);
                }
                if (live) {
                    Pk m;
#pragma unroll
                    for (int e = 0; e < V; ++e) m.v[e] = (T)0;
                    if (sub) m = *reinterpret_cast<const Pk *>(sub + (long long)(j0 + q) * inner);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const double a = band_magnitude((double)(T)acc[e] - (double)m.v[e]);
                        rmax[q] = a > rmax[q] ? a : rmax[q];
                    }
                }
            }
        }
    }

    // wave reduction by lane exchange, then one LDS word per (wave, row); every word of sred is written
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < BAND_ROWS; ++q) {
        double v = rmax[q];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const double other = __shfl_xor(v, s, 64);
            v = other > v ? other : v;
        }
        if (lane == 0) sred[wave][q] = v;
    }
    __syncthreads();
    if (tid < rows) {
        double v = sred[0][tid];
#pragma unroll
        for (int s = 1; s < BAND_BLOCK / 64; ++s) v = sred[s][tid] > v ? sred[s][tid] : v;
        part[(g * P + p) * nOut + j0 + tid] = v;
    }
}

// band_apply_line's geometry inside one group of `lg` lines: workgroup p of the group takes the line blocks
// p * lbw .. (NL lines each) of its tile of R rows.  minus: null or [nlines, nOut].  part: [groups][P][nOut].
template <typename T, int K>
__global__ __launch_bounds__(BAND_BLOCK) void band_absmax_line(const T *__restrict__ in, const T *__restrict__ minus,
                                                               double *__restrict__ part, const int *__restrict__ first,
                                                               const double *__restrict__ w, int nIn, int nOut, long long lg,
                                                               int R, int NL, long long tiles, int staged, long long lblocks,
                                                               int lbw, long long P)
{
    __shared__ T piece[LINE_LDS];
    __shared__ double sred[BAND_BLOCK];
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x % tiles, rest = blockIdx.x / tiles;
    const long long p = rest % P, grp = rest / P;
    const int j0 = (int)tile * R;
    const int rows = nOut - j0 < R ? nOut - j0 : R;
    const int base = first[j0];
    const int span = first[j0 + rows - 1] + K - base;

    const int G = BAND_BLOCK / R;
    const int g = tid / R, r = tid - g * R;
    const bool active = g < G && r < rows;
    const int j = j0 + (active ? r : 0);
    const int off = first[j] - base;
    double wt[K];
#pragma unroll
    for (int t = 0; t < K; ++t) wt[t] = w[(long long)j * K + t];

    double m = 0.0;
    const long long lb1 = (p + 1) * lbw < lblocks ? (p + 1) * lbw : lblocks;
    for (long long lb = p * lbw; lb < lb1; ++lb) {
        const long long local0 = lb * NL;
        const int nl = lg - local0 < NL ? (int)(lg - local0) : NL;
        const long long line0 = grp * lg + local0;
        if (staged) {
            __syncthreads();                                   // the piece of the block before this one has been read
            const int total = nl * span;
            for (int idx = tid; idx < total; idx += BAND_BLOCK) {
                const int l = idx / span, c = idx - l * span;
                piece[idx] = in[(line0 + l) * nIn + base + c];
            }
            __syncthreads();
        }
        if (active)
            for (int l = g; l < nl; l += G) {
                const T *q = staged ? piece + l * span + off : in + (line0 + l) * nIn + base + off;
                double acc = 0.0;
#pragma unroll
                for (int t = 0; t < K; ++t) acc = fma(wt[t], (double)q[t], acc);
                double x = (double)(T)acc;
                if (minus) x -= (double)minus[(line0 + l) * nOut + j];
                const double a = band_magnitude(x);
                m = a > m ? a : m;
            }
    }
    sred[tid] = active ? m : 0.0;                              // every word is written
    __syncthreads();
    if (tid < rows) {                                          // line group 0, row tid
        double v = sred[tid];
        for (int s = 1; s < G; ++s) v = sred[s * R + tid] > v ? sred[s * R + tid] : v;
        part[(grp * P + p) * nOut + j0 + tid] = v;
    }
}

// out[g][j] = max over p < P of part[g][p][j]: 64 rows x 4 lanes along p per workgroup
__global__ __launch_bounds__(BAND_BLOCK) void band_absmax_fold(const double *__restrict__ part, double *__restrict__ out,
                                                               int nOut, long long P, long long jblocks)
{
    __shared__ double sm[BAND_BLOCK];
    const int tid = threadIdx.x;
    const int jl = tid & 63, pl = tid >> 6;
    const long long g = blockIdx.x / jblocks;
    const long long j = (blockIdx.x % jblocks) * 64 + jl;
    double m = 0.0;
    if (j < nOut)
        for (long long p = pl; p < P; p += BAND_BLOCK / 64) {
            const double v = part[(g * P + p) * nOut + j];
            m = v > m ? v : m;
        }
    sm[tid] = m;
    __syncthreads();
    if (pl == 0 && j < nOut) {
#pragma unroll
        for (int s = 1; s < BAND_BLOCK / 64; ++s) m = sm[s * 64 + jl] > m ? sm[s * 64 + jl] : m;
        out[g * nOut + j] = m;
    }
}
#endif

}  // namespace bskband
