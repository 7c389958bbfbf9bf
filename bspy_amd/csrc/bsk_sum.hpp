// Sums of splines (bspy_amd/sums.py): the two operators that the band kernels of bsk_refine.hpp cannot express.
//
//   ScanMap      host: the weighted running sum of one variable (Spline.integrate),
//                    out[0] = 0,  out[j + 1] = sum over i <= j of g[i] * in[i],   j < n.
//                THE ASSOCIATION, the same for the host driver and both kernels whatever the launch geometry:
//                    p[i] = g[i] * in[i]                    one fp64 product, rounded (never contracted into the sum)
//                    chunk q = rows SCAN_CHUNK * q .. SCAN_CHUNK * (q + 1) - 1 (the last one may be short)
//                    local[i] = the sum of p over the chunk's rows up to i, left to right, from 0.0
//                    total[q] = local of the chunk's last row
//                    carry[q] = the sum of total[0 .. q - 1], left to right, from 0.0
//                    out[i + 1] = carry[q(i)] + local[i], rounded once to the data type
//                apply_line is that statement in plain C++ (sums.ScanMap.apply_line states it in NumPy).
//   scan_apply   device, inner > 1: data viewed as [outer, n, inner] -> [outer, n + 1, inner], lanes run along `inner`
//                (V elements = 16 bytes per lane where the alignment allows).  A lane walks the chunks of one segment
//                (whole chunks; blockIdx.y) of its column; loads of a chunk are independent, only the adds are serial.
//   scan_line    device, inner == 1 (lines are contiguous): a workgroup stages the products of one segment (at most
//                LINE_BLOCK chunks) of NL lines in LDS with coalesced reads, lane = one chunk of one line.  A lane sums
//                its chunk from LDS into registers, the chunk totals meet in LDS, every lane adds the totals in front
//                of it (left to right), writes carry + local back and the tile leaves with coalesced stores.
//                LDS layout: chunk slot s at doubles LINE_PAD * s .. , LINE_PAD = SCAN_CHUNK + 1: lane s reads byte
//                address 8 * (33 s + i), bank (2 s + 2 i) mod 64 for the 64-bit read: the 32 lanes of a half wave
//                (the read's lane group) hit 32 different even banks.  Unpadded, every lane would sit on one bank.
//   Segments     A line is split into segments of whole chunks so that few long lines still fill the device.  More
//                than one segment takes two launches on one stream: the TOTALS instantiation writes total[q] of the
//                chunks (scan_apply leaves the last segment out) into a workspace [outer, nchunks, inner] (doubles), then the
//                writing instantiation forms its carry from the workspace totals in front of its segment, in order.
//                No workgroup waits for another: no flags, no look-back.  The totals of the first launch and the
//                local sums of the second are the same instruction sequence on the same data: the same bits.
//   sum_bcast    device: out[idx] = a[idx . strideA] + sign * b[idx . strideB] over a contiguous result of rank <= 8;
//                a stride of 0 broadcasts.  Lanes run along the last axis, 16 bytes per lane where the last strides
//                are 1 or 0 and the pointers and row strides are aligned.  Widened to fp64, rounded once.
//
// No atomics anywhere: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

// products and sums stay separate roundings in this translation unit, on the host and on the device (see ScanMap)
#pragma clang fp contract(off)

namespace bsksum {

constexpr int SCAN_CHUNK = 32;                  // rows per chunk of the association
constexpr int SCAN_BLOCK = 256;                 // lanes per workgroup of scan_apply
constexpr int SCAN_UNROLL = 8;                  // independent loads in flight per lane of scan_apply
constexpr int SCAN_MAX_SEGMENTS = 32;           // automatic split: the carry loop reads at most this many chunk groups
constexpr long long SCAN_LANES_WANTED = 131072; // lanes from which scan_apply stops splitting (2 workgroups per CU)
constexpr int LINE_BLOCK = 128;                 // lanes per workgroup of scan_line = chunks of its tile
constexpr int LINE_PAD = SCAN_CHUNK + 1;        // doubles per chunk slot in LDS
constexpr int LINE_UNROLL = 8;                  // independent loads in flight per lane while scan_line stages its tile
constexpr int LINE_WG_WANTED = 512;             // workgroups from which scan_line stops splitting
constexpr int SUM_BLOCK = 256;
constexpr int SUM_MAX_RANK = 8;

struct ScanMap {
    int n = 0;
    std::vector<double> g;             // n

    // in[row * istride], n rows -> out[row * ostride], n + 1 rows
    template <typename T>
    void apply_line(const T *in, long long istride, T *out, long long ostride) const
    {
        out[0] = (T)0.0;
        double carry = 0.0;
        for (int r0 = 0; r0 < n; r0 += SCAN_CHUNK) {
            const int r1 = r0 + SCAN_CHUNK < n ? r0 + SCAN_CHUNK : n;
            double local = 0.0;
            for (int r = r0; r < r1; ++r) {
                const double p = g[r] * (double)in[(long long)r * istride];
                local = local + p;
                out[(long long)(r + 1) * ostride] = (T)(carry + local);
            }
            carry = carry + local;
        }
    }

    // host driver over [outer, n, inner] -> [outer, n + 1, inner]
    template <typename T>
    void apply_host(const T *in, long long outer, long long inner, T *out) const
    {
        for (long long o = 0; o < outer; ++o)
            for (long long i = 0; i < inner; ++i) apply_line(in + o * n * inner + i, inner, out + o * (n + 1) * inner + i, inner);
    }
};

// out is contiguous with extents dim[0 .. 7] (leading extents 1 fill the rank up); sa, sb: strides in elements, 0 = broadcast
struct SumDesc {
    long long dim[SUM_MAX_RANK], sa[SUM_MAX_RANK], sb[SUM_MAX_RANK];
};

template <typename T>
inline void sum_host(const T *a, const T *b, T *out, const SumDesc &d, double sign)
{
    long long idx[SUM_MAX_RANK] = {};
    long long total = 1;
    for (int ax = 0; ax < SUM_MAX_RANK; ++ax) total *= d.dim[ax];
    long long oa = 0, ob = 0;
    for (long long at = 0; at < total; ++at) {
        out[at] = (T)((double)a[oa] + sign * (double)b[ob]);
        for (int ax = SUM_MAX_RANK - 1; ax >= 0; --ax) {            // odometer
            oa += d.sa[ax];
            ob += d.sb[ax];
            if (++idx[ax] < d.dim[ax]) break;
            oa -= idx[ax] * d.sa[ax];
            ob -= idx[ax] * d.sb[ax];
            idx[ax] = 0;
        }
    }
}

#ifdef __HIPCC__
template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

// in: [outer, n, inner], out: [outer, n + 1, inner], ws: [outer, nchunks, inner] doubles (read or written only when
// the launch has more than one segment).  Lane = (outer index, V consecutive inner indices), gid < outer * (inner / V);
// blockIdx.y = segment of cps chunks, so the row a wave works on is uniform and g[row] is a scalar operand.
// V divides inner and in, out and ws are V * sizeof aligned when V > 1 (the launcher checks).
// TOTALS: write total[q] of the segment's chunks into ws, nothing into out.  Otherwise: carry = the totals in front of
// the segment (from ws, in order), then the segment's rows are written; segment 0 also writes the zero row.
template <typename T, int V, bool TOTALS>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_apply(const T *__restrict__ in, T *__restrict__ out,
                                                         const double *__restrict__ g, double *__restrict__ ws, int n,
                                                         long long outer, long long inner, int nchunks, int cps)
{
    using P = Pack<T, V>;
    using D = Pack<double, V>;
    const long long lanes_i = inner / V;
    const long long gid = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (gid >= outer * lanes_i) return;
    const long long o = gid / lanes_i, ii = (gid - o * lanes_i) * V;
    const int seg = blockIdx.y;
    const int q0 = seg * cps;
    const int q1 = q0 + cps < nchunks ? q0 + cps : nchunks;
    const T *src = in + o * n * inner + ii;
    T *dst = out + o * ((long long)n + 1) * inner + ii;
    const long long ws_at = o * nchunks * inner + ii;

    double carry[V];
#pragma unroll
    for (int e = 0; e < V; ++e) carry[e] = 0.0;
    if (!TOTALS) {
        for (int q = 0; q < q0; ++q) {
            const D t = *reinterpret_cast<const D *>(ws + ws_at + (long long)q * inner);
#pragma unroll
            for (int e = 0; e < V; ++e) carry[e] = carry[e] + t.v[e];
        }
        if (seg == 0) {
            P z;
#pragma unroll
            for (int e = 0; e < V; ++e) z.v[e] = (T)0.0;
            *reinterpret_cast<P *>(dst) = z;
        }
    }
    for (int q = q0; q < q1; ++q) {
        const int r0 = q * SCAN_CHUNK;
        const int cnt = n - r0 < SCAN_CHUNK ? n - r0 : SCAN_CHUNK;
        double local[V];
#pragma unroll
        for (int e = 0; e < V; ++e) local[e] = 0.0;
        auto row = [&](int r) {
            const P x = *reinterpret_cast<const P *>(src + (long long)r * inner);
            const double gr = g[r];
            P y;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double p = gr * (double)x.v[e];
                local[e] = local[e] + p;
                y.v[e] = (T)(carry[e] + local[e]);
            }
            if (!TOTALS) *reinterpret_cast<P *>(dst + (long long)(r + 1) * inner) = y;
        };
        if (cnt == SCAN_CHUNK) {
#pragma unroll SCAN_UNROLL
            for (int i = 0; i < SCAN_CHUNK; ++i) row(r0 + i);
        } else {
            for (int i = 0; i < cnt; ++i) row(r0 + i);
        }
        if (TOTALS) {
            D t;
#pragma unroll
            for (int e = 0; e < V; ++e) t.v[e] = local[e];
            *reinterpret_cast<D *>(ws + ws_at + (long long)q * inner) = t;
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) carry[e] = carry[e] + local[e];
        }
    }
}

// Position (line l, column c) inside a tile of lines of `span` columns, for the flat index tid, tid + LINE_BLOCK, ...
// One division at the start; a step needs another only where lines are shorter than the workgroup.
struct TileWalk {
    int l, c;
    __device__ TileWalk(int tid, int span) : l(tid / span), c(tid - (tid / span) * span) {}
    __device__ void next(int span)
    {
        c += LINE_BLOCK;
        if (span >= LINE_BLOCK) {
            if (c >= span) {
                c -= span;
                ++l;
            }
        } else {
            const int d = c / span;
            l += d;
            c -= d * span;
        }
    }
};

// in: [nlines, n], out: [nlines, n + 1], ws: [nlines, nchunks] doubles (used only when nseg > 1).
// Workgroup = (block of NL lines, segment of cps <= LINE_BLOCK chunks), NL * cps <= LINE_BLOCK; lane tid = chunk slot
// (line tid / cps, chunk tid % cps of the segment).  An LDS word is read only where the staging loop of this dispatch
// wrote it: slot < nl * cps with the chunk inside the segment, and i < cnt rows of that chunk.
template <typename T, bool TOTALS>
__global__ __launch_bounds__(LINE_BLOCK) void scan_line(const T *__restrict__ in, T *__restrict__ out,
                                                        const double *__restrict__ g, double *__restrict__ ws, int n,
                                                        long long nlines, int nchunks, int cps, int NL, int nseg)
{
    __shared__ double sp[LINE_BLOCK * LINE_PAD];
    __shared__ double stot[LINE_BLOCK];
    const int tid = threadIdx.x;
    const int seg = blockIdx.x % nseg;
    const long long line0 = (long long)(blockIdx.x / nseg) * NL;
    const int nl = nlines - line0 < NL ? (int)(nlines - line0) : NL;
    const int q0 = seg * cps;
    const int nq = nchunks - q0 < cps ? nchunks - q0 : cps;
    const int col0 = q0 * SCAN_CHUNK;
    const int span = n - col0 < nq * SCAN_CHUNK ? n - col0 : nq * SCAN_CHUNK;
    const int total = nl * span;

    // staging: LINE_UNROLL independent loads per lane in flight, then the products go to LDS
    {
        TileWalk at(tid, span);
        for (int base = tid; base < total; base += LINE_UNROLL * LINE_BLOCK) {
            T v[LINE_UNROLL];
            double gv[LINE_UNROLL];
            int slot[LINE_UNROLL];
#pragma unroll
            for (int u = 0; u < LINE_UNROLL; ++u) {
                slot[u] = -1;
                if (base + u * LINE_BLOCK < total) {
                    v[u] = in[(line0 + at.l) * n + col0 + at.c];
                    gv[u] = g[col0 + at.c];
                    slot[u] = (at.l * cps + at.c / SCAN_CHUNK) * LINE_PAD + at.c % SCAN_CHUNK;
                }
                at.next(span);
            }
#pragma unroll
            for (int u = 0; u < LINE_UNROLL; ++u)
                if (slot[u] >= 0) sp[slot[u]] = gv[u] * (double)v[u];
        }
    }
    __syncthreads();

    const int l = tid / cps, q = tid - l * cps;
    const bool live = l < nl && q < nq;
    const int cnt = !live ? 0 : (span - q * SCAN_CHUNK < SCAN_CHUNK ? span - q * SCAN_CHUNK : SCAN_CHUNK);
    double *mine = sp + tid * LINE_PAD;
    double loc[SCAN_CHUNK];
    double local = 0.0;
#pragma unroll
    for (int i = 0; i < SCAN_CHUNK; ++i) {
        loc[i] = 0.0;
        if (i < cnt) {
            local = local + mine[i];
            loc[i] = local;
        }
    }
    if (TOTALS) {
        if (live) ws[(line0 + l) * nchunks + q0 + q] = local;
        return;
    }
    if (live) stot[tid] = local;
    __syncthreads();
    if (live) {
        double carry = 0.0;
        const double *front = ws + (line0 + l) * nchunks;         // read only for q0 > 0, i.e. nseg > 1
        for (int j = 0; j < q0; ++j) carry = carry + front[j];
#pragma unroll 8
        for (int j = 0; j < q; ++j) carry = carry + stot[l * cps + j];
#pragma unroll
        for (int i = 0; i < SCAN_CHUNK; ++i)
            if (i < cnt) mine[i] = carry + loc[i];
    }
    __syncthreads();
    {
        TileWalk at(tid, span);
        for (int idx = tid; idx < total; idx += LINE_BLOCK) {
            out[(line0 + at.l) * ((long long)n + 1) + 1 + col0 + at.c] =
                (T)sp[(at.l * cps + at.c / SCAN_CHUNK) * LINE_PAD + at.c % SCAN_CHUNK];
            at.next(span);
        }
    }
    if (seg == 0 && tid < nl) out[(line0 + tid) * ((long long)n + 1)] = (T)0.0;
}

// Lane = V consecutive entries of the last axis of one row of out; rows = the product of the other extents (< 2^32,
// the launcher checks).  V > 1: the last extent is a multiple of V, an operand whose last stride is 1 has its pointer
// and its other strides V * sizeof(T) aligned, one whose last stride is 0 is read as one value.
template <typename T, int V>
__global__ __launch_bounds__(SUM_BLOCK) void sum_bcast(const T *__restrict__ a, const T *__restrict__ b, T *__restrict__ out,
                                                       SumDesc d, double sign, long long lanes_last, long long lanes)
{
    using P = Pack<T, V>;
    const long long gid = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x;
    if (gid >= lanes) return;
    unsigned row = (unsigned)(gid / lanes_last);
    const long long c = (gid - (long long)row * lanes_last) * V;
    long long oa = c * d.sa[SUM_MAX_RANK - 1], ob = c * d.sb[SUM_MAX_RANK - 1];
#pragma unroll
    for (int ax = SUM_MAX_RANK - 2; ax >= 0; --ax) {
        if (d.dim[ax] > 1) {                              // uniform: extents of 1 cost nothing
            const unsigned ext = (unsigned)d.dim[ax];
            const unsigned nxt = row / ext;
            const long long at = row - nxt * ext;
            row = nxt;
            oa += at * d.sa[ax];
            ob += at * d.sb[ax];
        }
    }
    P x, y, r;
    if (V > 1 && d.sa[SUM_MAX_RANK - 1] != 0) x = *reinterpret_cast<const P *>(a + oa);
    else {
        const T s = a[oa];
#pragma unroll
        for (int e = 0; e < V; ++e) x.v[e] = s;
    }
    if (V > 1 && d.sb[SUM_MAX_RANK - 1] != 0) y = *reinterpret_cast<const P *>(b + ob);
    else {
        const T s = b[ob];
#pragma unroll
        for (int e = 0; e < V; ++e) y.v[e] = s;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = (T)((double)x.v[e] + sign * (double)y.v[e]);
    *reinterpret_cast<P *>(out + gid * V) = r;
}
#endif

}  // namespace bsksum
