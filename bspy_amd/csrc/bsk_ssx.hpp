// Surface-surface intersection (bspy_amd/surfaces.py): the bsk_ssx_* family.  Two surfaces (nInd 2, nDep 3, orders 2 .. 4).
//
// The caller has brought both variables of both surfaces to Bezier form (the band operator of bsk_refine.hpp, once per
// axis): rows is [3, R0, R1] in fp64 and cell (i, j), flat index i nc1 + j, is the K0 x K1 window of the three components
// at first0[i], first1[j].  A launch serves one FAMILY of lattice lines: the isoparametric lines of surface X with the
// variable `ax` fixed, G = 2^depth of them per knot cell, against the cells of the other surface Y.  Line n is owned by
// cell c = min(n / G, nc - 1) of the fixed variable at the local value x = (n - c G) / G, a dyadic number; on the running
// cell e it is a Bezier curve of KR points, each the de Casteljau value at x of one column (ax = 0) or row (ax = 1) of the
// window (x = 0 and x = 1 copy the first and the last one).  Segment n ncrun + e against cell (p, q) of Y is the system
// F(w, s, t) = L(w) - Y(s, t) with the Bernstein coefficients F_ijk = L_i - Y_jk: a bskroots3 system of orders
// (KR, KY0, KY1) that is never stored.
//
//   ssx_search    lane = line segment with its KR points and their box in registers; grid = (segment blocks, chunks of
//                 Y's cells).  The boxes (bsk_rays_boxes of Y) are read through wave-uniform addresses (kernel arguments,
//                 blockIdx, the loop counter): scalar loads in the built code.  Y's windows have uniform addresses too, but
//                 they are read behind the lanes' own box test, and the compiler makes them vector loads.  inbox: the box
//                 of the segment's OWN points and the box of Y's cell are not strictly disjoint in any component, an
//                 exact comparison.  A pair is flat when
//                 inbox holds and all KR KY0 KY1 values of a component are below S_d eps (or S_d is 0), else it is a
//                 candidate unless a component is strictly of one sign.  A pair with disjoint boxes is strictly of one
//                 sign in that component (a difference of two distinct doubles is not 0), so PREFILTER, which drops it
//                 before its window is read, changes no byte.  Flat pairs and candidates are counted (EMIT = false:
//                 partial[lane, chunk]) or written (EMIT = true: pair_seg, pair_cell at offset[lane, chunk] + n, cells
//                 ascending).
//   ssx_isolate   ONE WAVE = one pair, block 64: a flat pair sets status bit 16 and reports nothing; any other pair is
//                 walked by bskroots3::isolate_cell on a PairCell, which gives lane (i0, i1, i2) the value L_i0 - Y_i1i2;
//                 every lane forms its own L_i0 by the lerps of its column.
//   ssx_merge     lane = one zero with near set: the rule of roots3_merge among the pairs of the same line.  It is
//                 dropped when one of the 13 neighbours (e + de, p + dp, q + dq) that precede it holds a zero within
//                 2^-20 h on all three axes.  The pairs are sorted by key = segment ncellY + cell, so a neighbour is found
//                 by a binary search of 64 steps at most; no table over lines x cells exists.
//
// fp64, no contraction, bskroots::lerp's association, one text for the host drivers and the kernels; surfaces.py states
// it in Python floats.  No atomics, no waiting, no LDS, and every loop has a compile-time or an argument bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#define BSK_ROOTS3_FUNCTIONS_ONLY
#include "bsk_pairs.hpp"
#include "bsk_roots3.hpp"

#pragma clang fp contract(off)

namespace bskssx {

using bskpairs::Surface;                            // one surface with its orders (bsk_pairs.hpp)
using bskpairs::window;
using bskroots::lerp;
using bskroots::ROOTS_EPS;
using bskroots3::ROOTS3_SAME;
using bskroots3::slots;

constexpr int SSX_SEARCH_BLOCK = 64;                // few segments: one wave a workgroup spreads them over the device
constexpr int SSX_BLOCK = 256;                      // ssx_merge
constexpr int SSX_WAVE = 64;                        // ssx_isolate: one wave a workgroup, one pair a wave
constexpr int SSX_MAX_K = 4;
constexpr unsigned STATUS_FLAT = 16;

// one family: the lines of X with variable ax fixed, G per knot cell, against Y
struct Side {
    Surface X, Y;
    int ax;
    long long G;
};

BSK_HD long long ncrun(const Side &s) { return s.ax == 0 ? s.X.nc1 : s.X.nc0; }
BSK_HD long long ncfix(const Side &s) { return s.ax == 0 ? s.X.nc0 : s.X.nc1; }
BSK_HD int order_run(const Side &s) { return s.ax == 0 ? s.X.K1 : s.X.K0; }

// A line on one running cell: component d of point i is the value at x of the KF doubles q[r sf], q = p + d sd + i sr.
struct LineRef {
    const double *p;
    long long sd, sf, sr;
    int KF;
    double x;
};

BSK_HD double line_point(const LineRef &l, int d, int i)
{
    const double *q = l.p + d * l.sd + i * l.sr;
    if (l.x == 0.0) return q[0];
    if (l.x == 1.0) return q[(l.KF - 1) * l.sf];
    double b[SSX_MAX_K];
#pragma unroll
    for (int r = 0; r < SSX_MAX_K; ++r) b[r] = r < l.KF ? q[r * l.sf] : 0.0;
    const double s = 1.0 - l.x;
#pragma unroll
    for (int r = 1; r < SSX_MAX_K; ++r)
#pragma unroll
        for (int e = 0; e < SSX_MAX_K - r; ++e)
            if (r < l.KF && e < l.KF - r) b[e] = lerp(s, l.x, b[e], b[e + 1]);
    return b[0];
}

// segment seg = n ncrun + e of the family; false: no such segment, or its window leaves the rows
BSK_HD bool line_ref(const Side &s, long long seg, LineRef &l, long long &e)
{
    const long long nr = ncrun(s), nf = ncfix(s);
    if (s.G < 1 || seg < 0 || seg >= (nf * s.G + 1) * nr) return false;
    const long long n = seg / nr;
    e = seg - n * nr;
    long long c = n / s.G;
    if (c > nf - 1) c = nf - 1;
    const long long g = n - c * s.G;
    const long long i = s.ax == 0 ? c : e, j = s.ax == 0 ? e : c;
    const long long f0 = s.X.first0[i], f1 = s.X.first1[j];
    if (f0 < 0 || f0 + s.X.K0 > s.X.R0 || f1 < 0 || f1 + s.X.K1 > s.X.R1) return false;
    l.p = s.X.rows + f0 * s.X.R1 + f1;
    l.sd = s.X.R0 * s.X.R1;
    l.sf = s.ax == 0 ? s.X.R1 : 1;
    l.sr = s.ax == 0 ? 1 : s.X.R1;
    l.KF = s.ax == 0 ? s.X.K0 : s.X.K1;
    l.x = (double)g / (double)s.G;
    return true;
}

// the points of a segment: L[d][i], i < KR (0 behind)
BSK_HD void line_points(const LineRef &l, int KR, double (*L)[SSX_MAX_K])
{
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int i = 0; i < SSX_MAX_K; ++i) L[d][i] = i < KR ? line_point(l, d, i) : 0.0;
}

// 0: no pair; 1: a candidate; 2: a flat pair.  w: Y's window, component d, entry (j, k) at w[d sd + j si + k].
BSK_HD int pair_kind(const double (*L)[SSX_MAX_K], int KR, const double *w, long long sd, long long si, int K1, int K2, const double *S,
                     bool inbox)
{
    bool flat = false, ex = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        bool pos = true, neg = true, small = true;
        const double tiny = S[d] * ROOTS_EPS;
        for (int j = 0; j < K1; ++j)
            for (int k = 0; k < K2; ++k) {
                const double y = w[d * sd + j * si + k];
#pragma unroll
                for (int i = 0; i < SSX_MAX_K; ++i)
                    if (i < KR) {
                        const double f = L[d][i] - y;
                        pos = pos && f > 0.0;
                        neg = neg && f < 0.0;
                        small = small && fabs(f) < tiny;
                    }
            }
        flat = flat || small || S[d] == 0.0;               // as roots3's zero-cell rule: a scale of 0 is a zero field
        ex = ex || pos || neg;
    }
    if (flat) return inbox ? 2 : 0;
    return ex ? 0 : 1;
}

// One pair seen as a cell of bskroots3: lane (i0, i1, i2) holds L_i0 - Y_i1i2.
struct PairCell {
    LineRef l;
    const double *w;
    long long sd, si;
    BSK_HD double at(int d, int i0, int i1, int i2) const { return line_point(l, d, i0) - w[d * sd + i1 * si + i2]; }
};

// partial: [nseg, nchunks]; offset: [nseg, nchunks] (exclusive sums of partial); pair_*: [npairs].  The launch serves the
// segments seg0 .. seg0 + nseg - 1 of the family; pair_seg holds the segment's index in the family.
struct Search {
    long long seg0, nseg, chunk, nchunks;
    const double *boxes, *scale;
    int32_t *partial;
    const int64_t *offset;
    int32_t *pair_seg, *pair_cell;
    long long npairs;
};

template <bool PREFILTER, bool EMIT>
BSK_HD void search_lane(const Side &s, const Search &a, long long ch, long long lane)
{
    LineRef l;
    long long e = 0;
    const long long seg = a.seg0 + lane;
    const bool ok = line_ref(s, seg, l, e);
    const int KR = order_run(s);
    const long long ncell = s.Y.nc0 * s.Y.nc1;
    const long long begin = ch * a.chunk, end = begin + a.chunk < ncell ? begin + a.chunk : ncell;
    const long long base = EMIT ? a.offset[lane * a.nchunks + ch] : 0;
    long long n = 0;
    if (ok) {
        double L[3][SSX_MAX_K], lo[3], hi[3];
        line_points(l, KR, L);
        const double S[3] = {a.scale[0], a.scale[1], a.scale[2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = hi[d] = L[d][0];
#pragma unroll
            for (int i = 1; i < SSX_MAX_K; ++i)
                if (i < KR) {
                    lo[d] = L[d][i] < lo[d] ? L[d][i] : lo[d];
                    hi[d] = L[d][i] > hi[d] ? L[d][i] : hi[d];
                }
        }
        for (long long cell = begin; cell < end; ++cell) {
            const double *box = a.boxes + 6 * cell;
            bool inbox = true;
#pragma unroll
            for (int d = 0; d < 3; ++d) inbox = inbox && !(hi[d] < box[2 * d] || lo[d] > box[2 * d + 1]);
            if (PREFILTER && !inbox) continue;
            const double *w;
            long long p, q;
            if (!window(s.Y, s.Y.K0, s.Y.K1, cell, w, p, q)) continue;
            if (pair_kind(L, KR, w, s.Y.R0 * s.Y.R1, s.Y.R1, s.Y.K0, s.Y.K1, S, inbox) == 0) continue;
            if (EMIT && base + n >= 0 && base + n < a.npairs) {
                a.pair_seg[base + n] = (int32_t)seg;
                a.pair_cell[base + n] = (int32_t)cell;
            }
            ++n;
        }
    }
    if (!EMIT) a.partial[lane * a.nchunks + ch] = (int32_t)n;
}

// brun: the breaks of X's running variable; by0, by1: Y's.  roots: [npairs, R, 3] as (w, s, t); near: [npairs, R];
// count, status, nodes: [npairs]
struct Isolate {
    const double *brun, *by0, *by1, *scale;
    const int32_t *pair_seg, *pair_cell;
    long long npairs;
    double *roots;
    uint8_t *near;
    int32_t *count;
    uint8_t *status;
    int32_t *nodes;
};

template <class W, int KR, int K1, int K2>
BSK_HD void isolate_wave(const W &wave, const Side &s, const Isolate &a, long long slot)
{
    constexpr int R = slots(KR, K1, K2);
    double *out = a.roots + slot * 3 * R;
    PairCell pc;
    long long e = 0, p = 0, q = 0;
    bool walk = line_ref(s, a.pair_seg[slot], pc.l, e) && window(s.Y, s.Y.K0, s.Y.K1, a.pair_cell[slot], pc.w, p, q);
    unsigned status = 0;
    if (walk) {
        pc.sd = s.Y.R0 * s.Y.R1;
        pc.si = s.Y.R1;
        const double S[3] = {a.scale[0], a.scale[1], a.scale[2]};
        double L[3][SSX_MAX_K];
        line_points(pc.l, KR, L);
        if (pair_kind(L, KR, pc.w, pc.sd, pc.si, K1, K2, S, true) == 2) {
            walk = false;
            status = STATUS_FLAT;
        } else {
            const double t0[3] = {a.brun[e], a.by0[p], a.by1[q]};
            const double t1[3] = {a.brun[e + 1], a.by0[p + 1], a.by1[q + 1]};
            bskroots3::isolate_cell<W, KR, K1, K2>(wave, pc, t0, t1, S, out, a.near + slot * R, a.count + slot, a.status + slot,
                                                   a.nodes + slot);
        }
    }
    if (!walk && wave.first()) {
        for (int r = 0; r < R; ++r) {
            out[3 * r] = __builtin_nan("");
            out[3 * r + 1] = __builtin_nan("");
            out[3 * r + 2] = __builtin_nan("");
            a.near[slot * R + r] = 0;
        }
        a.count[slot] = 0;
        a.status[slot] = (uint8_t)status;
        a.nodes[slot] = 0;
    }
}

// pair_key: [npairs] ascending, segment ncellY + cell; which: [nnear] flat (pair, slot); keep: [npairs, R]
struct Merge {
    int R;
    const double *roots;
    long long ncrun, ncy0, ncy1;
    const double *brun, *by0, *by1;
    const int64_t *pair_key;
    long long npairs;
    const int64_t *which;
    long long nnear;
    uint8_t *keep;
};

BSK_HD void merge_lane(const Merge &m, long long lane)
{
    const long long at = m.which[lane];
    if (at < 0 || at >= m.npairs * m.R) return;
    const long long pair = at / m.R;
    const long long ncell = m.ncy0 * m.ncy1;
    const long long key = m.pair_key[pair];
    if (key < 0) return;
    const long long seg = key / ncell, cell = key - seg * ncell;
    const long long e = seg % m.ncrun, p = cell / m.ncy1, q = cell - p * m.ncy1;
    const double u = m.roots[3 * at], v = m.roots[3 * at + 1], w = m.roots[3 * at + 2];
    const double tolu = ROOTS3_SAME * (m.brun[e + 1] - m.brun[e]), tolv = ROOTS3_SAME * (m.by0[p + 1] - m.by0[p]);
    const double tolw = ROOTS3_SAME * (m.by1[q + 1] - m.by1[q]);
    uint8_t kept = (u == u) ? 1 : 0;
    for (int n = 0; n < 13; ++n) {                             // the 13 of the 26 neighbours that precede (e, p, q)
        const long long de = n / 9 - 1, ne = e + de, np = p + (n / 3) % 3 - 1, nq = q + n % 3 - 1;
        if (ne < 0 || np < 0 || nq < 0 || ne >= m.ncrun || np >= m.ncy0 || nq >= m.ncy1) continue;
        const long long want = (seg + de) * ncell + np * m.ncy1 + nq;
        long long lo = 0, hi = m.npairs;                       // the first pair with key >= want
        for (int step = 0; step < 64; ++step) {
            if (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (m.pair_key[mid] < want) lo = mid + 1;
                else hi = mid;
            }
        }
        if (lo >= m.npairs || m.pair_key[lo] != want) continue;
        for (int r = 0; r < m.R; ++r) {
            const double *z = m.roots + 3 * (lo * m.R + r);
            if (fabs(z[0] - u) <= tolu && fabs(z[1] - v) <= tolv && fabs(z[2] - w) <= tolw) kept = 0;
        }
    }
    m.keep[at] = kept;
}

#ifdef __HIPCC__
template <bool PREFILTER, bool EMIT>
__global__ __launch_bounds__(SSX_SEARCH_BLOCK) void ssx_search(Side s, Search a)
{
    const long long gid = (long long)blockIdx.x * SSX_SEARCH_BLOCK + threadIdx.x;
    if (gid >= a.nseg) return;
    search_lane<PREFILTER, EMIT>(s, a, (long long)blockIdx.y, gid);
}

// one workgroup = one wave = one pair: every lane of the wave takes every branch together
template <int KR, int K1, int K2>
__global__ __launch_bounds__(SSX_WAVE) void ssx_isolate(Side s, Isolate a)
{
    const long long slot = blockIdx.x;
    if (slot >= a.npairs) return;
    const bskroots3::LaneWave wave{(int)threadIdx.x};
    isolate_wave<bskroots3::LaneWave, KR, K1, K2>(wave, s, a, slot);
}

__global__ __launch_bounds__(SSX_BLOCK) void ssx_merge(Merge m)
{
    const long long gid = (long long)blockIdx.x * SSX_BLOCK + threadIdx.x;
    if (gid >= m.nnear) return;
    merge_lane(m, gid);
}
#endif

}  // namespace bskssx
