// Level curves of a scalar spline in two variables (bspy_amd/contours.py): the bsk_contour_* family.
//
// The caller has brought both variables to Bezier form (the band operator of bsk_refine.hpp, once per axis): rows is
// [nrows, R0, R1] in fp64 and cell (i, j) is the K0 x K1 window at first0[i], first1[j].  Field b reads rows[b], or, with
// levels, rows[0] with levels[b] subtracted from every coefficient as it is loaded (one extraction for all fields).
// Adjacent cells share their end row / column of the rows (no knot of the caller's is a jump), so the two cells next to a
// knot line hold the same floats on it.
//
// Every cell carries a lattice of G x G leaves, G = 2^depth.  Lattice node (I, J) = cell (i, j), local (a, b), I = i G + a.
//   node value     the cell with the lowest flat index that contains the node owns it: io = (I - 1) / G for I > 0, else 0,
//                  a = I - io G (so a = G on the far side), the same for J.  value = de Casteljau of the owner's
//                  coefficients, every row at y = b / G, then the K0 results at x = a / G.  Its sign: v >= 0 is positive.
//   edge           (I, J, dir): from node (I, J) to (I + 1, J) (dir 0) or (I, J + 1) (dir 1); key = ((I NJ + J) << 1) | dir
//                  with NJ = nc1 G + 1.  It is crossed when the signs of its two nodes differ.
//   vertex         of a crossed edge, a function of the edge alone: the owner cell of the lattice line (the lowest flat
//                  index again) is restricted to the line by one de Casteljau per row (column) in the fixed variable, that
//                  polynomial to the edge's interval (bskroots::restrict_to), and the sign bisection of roots_isolate on
//                  [0, 1] (at most 60 steps, midpoint an end or value 0.0) from the sign of node (I, J) gives s; the moving
//                  coordinate is x = a / G + s / G, and a local x becomes lerp(1 - x, x, t0, t1) of the cell's knots.
//   leaf           its perimeter is walked counter-clockwise (bottom, right, top, left).  A crossing from + to - starts a
//                  segment, one from - to + ends it (f >= 0 lies on the left).  2 crossings: one segment.  4 crossings: the
//                  centre value (the leaf's own cell at ((2a + 1) / 2G, (2b + 1) / 2G)) pairs a start with the next end
//                  when it is positive, with the previous one when not; the lane's status gets bit 1.
//
//   contour_flag   lane = (field, cell): zero = every coefficient is below S eps in magnitude (or S is 0);
//                  cand = not zero and not (all coefficients > tau or all < -tau), tau = 32 (K0 + K1) eps S.
//   contour_march  lane = (candidate cell, top box q of the 4^P boxes of its cell), block 64.  The lane restricts the
//                  cell's coefficients to its box and walks the 2 (depth - P) binary levels below it (axis 0 first) depth
//                  first without a stack, as roots2_isolate does: a live node is halved, a child is dropped when its
//                  coefficients are all > tau or all < -tau, the left live child is walked next, else the right one;
//                  otherwise the walk strips the trailing 1 bits, sets bit 0 and restricts the cell's own coefficients,
//                  read again, to that box.  tau bounds the rounding of a restriction plus that of a node value
//                  (contours.py derives it), so a dropped box holds no crossed edge and dropping changes the cost only.
//                  EMIT = false counts the segments of the lane; EMIT = true writes segment n of the lane at
//                  offsets[lane] + n: keys (a, b) and xy (ua, va, ub, vb), plain vector stores.
//
// fp64, no contraction, lerp(s, t, a, b) = s a + t b: one association for the host drivers and the kernels.  No LDS, no
// atomics, no waiting, every loop has a compile-time trip bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsk_box2.hpp"
#include "bsk_roots.hpp"

#pragma clang fp contract(off)

namespace bskcontour {

using bskbox2::halve;
using bskbox2::restrict_box;
using bskroots::lerp;
using bskroots::restrict_to;
using bskroots::value;

constexpr int CONTOUR_BLOCK = 256;                  // contour_flag
constexpr int CONTOUR_MARCH_BLOCK = 64;             // one wave: the walk may use the whole register file
constexpr int CONTOUR_MAX_DEPTH = 8;
constexpr int CONTOUR_BISECT = bskroots::ROOTS_BISECT;
// trips of a walk: at most 2^16 leaves, as many inner nodes and as many steps back below one top box
constexpr int CONTOUR_WALK = 1 << 18;
constexpr double CONTOUR_TAU = 32.0;                // tau = CONTOUR_TAU (K0 + K1) eps S
constexpr double CONTOUR_EPS = 0x1p-52;
constexpr unsigned STATUS_SADDLE = 1;

// The tables of a launch.  rows: [nrows, R0, R1]; first0: [nc0]; first1: [nc1]; levels: [nfields] or null; scale: [nfields].
struct Grid {
    const double *rows;
    long long nrows, R0, R1, nc0, nc1;
    const int32_t *first0, *first1;
    const double *levels;
    long long nfields;
    const double *scale;
};

// the coefficients of cell (i, j) of field b, the level subtracted; false: not a cell, or its window leaves the rows
template <int K0, int K1>
BSK_HD bool load_cell(const Grid &g, long long b, long long i, long long j, double *c)
{
    if (b < 0 || b >= g.nfields || i < 0 || i >= g.nc0 || j < 0 || j >= g.nc1) return false;
    const long long rb = g.levels ? 0 : b;
    if (rb >= g.nrows) return false;
    const long long f0 = g.first0[i], f1 = g.first1[j];
    if (f0 < 0 || f0 + K0 > g.R0 || f1 < 0 || f1 + K1 > g.R1) return false;
    const double lev = g.levels ? g.levels[b] : 0.0;
    const double *p = g.rows + (rb * g.R0 + f0) * g.R1 + f1;
#pragma unroll
    for (int r = 0; r < K0; ++r)
#pragma unroll
        for (int s = 0; s < K1; ++s) c[r * K1 + s] = p[r * g.R1 + s] - lev;
    return true;
}

template <int N>
BSK_HD bool one_side(const double *c, double tau)
{
    bool pos = true, neg = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pos = pos && c[i] > tau;
        neg = neg && c[i] < -tau;
    }
    return pos || neg;
}

template <int K0, int K1>
BSK_HD double tau_of(double S)
{
    return CONTOUR_TAU * (double)(K0 + K1) * CONTOUR_EPS * S;
}

// every row at y, then the K0 results at x
template <int K0, int K1>
BSK_HD double value2(const double *c, double x, double y)
{
    double p[K0];
#pragma unroll
    for (int r = 0; r < K0; ++r) p[r] = value<K1>(c + r * K1, y);
    return value<K0>(p, x);
}

// owner and local index of the lattice coordinate I: the lowest cell that contains it
BSK_HD void owner_of(long long I, int depth, long long &cell, long long &a)
{
    cell = I > 0 ? (I - 1) >> depth : 0;
    a = I - (cell << depth);
}

template <int K0, int K1>
BSK_HD double node_value(const Grid &g, long long b, long long I, long long J, int depth)
{
    const double inv = 1.0 / (double)(1 << depth);
    long long io, a, jo, bb;
    owner_of(I, depth, io, a);
    owner_of(J, depth, jo, bb);
    double c[K0 * K1];
    if (!load_cell<K0, K1>(g, b, io, jo, c)) return __builtin_nan("");
    return value2<K0, K1>(c, (double)a * inv, (double)bb * inv);
}

// the sign bisection of bsk_roots.hpp on [0, 1]: pos is the sign at 0
template <int K>
BSK_HD double bisect(const double *e, bool pos)
{
    double a = 0.0, b = 1.0;
    for (int step = 0; step < CONTOUR_BISECT; ++step) {
        const double m = 0.5 * (a + b);
        if (m == a || m == b) break;
        const double f = value<K>(e, m);
        if (f == 0.0) {
            a = m;
            b = m;
            break;
        }
        if ((f > 0.0) == pos) a = m;
        else b = m;
    }
    return 0.5 * (a + b);
}

// the vertex of the crossed edge (I, J, dir) of field b; pos: the sign of node (I, J)
template <int K0, int K1>
BSK_HD void vertex(const Grid &g, const double *breaks0, const double *breaks1, long long b, long long I, long long J, int dir,
                   int depth, bool pos, double &u, double &v)
{
    const double inv = 1.0 / (double)(1 << depth);
    long long i, a, j, bb;
    if (dir == 0) {
        i = I >> depth;
        a = I - (i << depth);
        owner_of(J, depth, j, bb);
    } else {
        owner_of(I, depth, i, a);
        j = J >> depth;
        bb = J - (j << depth);
    }
    double c[K0 * K1];
    u = __builtin_nan("");
    v = __builtin_nan("");
    if (!load_cell<K0, K1>(g, b, i, j, c)) return;
    double x = (double)a * inv, y = (double)bb * inv;
    if (dir == 0) {
        double p[K0], e[K0];
#pragma unroll
        for (int r = 0; r < K0; ++r) p[r] = value<K1>(c + r * K1, y);
        restrict_to<K0>(p, x, inv, e);
        x = x + bisect<K0>(e, pos) * inv;
    } else {
        double q[K1], e[K1];
#pragma unroll
        for (int s = 0; s < K1; ++s) {
            double col[K0];
#pragma unroll
            for (int r = 0; r < K0; ++r) col[r] = c[r * K1 + s];
            q[s] = value<K0>(col, x);
        }
        restrict_to<K1>(q, y, inv, e);
        y = y + bisect<K1>(e, pos) * inv;
    }
    u = lerp(1.0 - x, x, breaks0[i], breaks0[i + 1]);
    v = lerp(1.0 - y, y, breaks1[j], breaks1[j + 1]);
}

// Leaf (a, bb) of cell (i, j) of field b.  count: the segments of the lane so far; EMIT: segment n goes to base + n.
template <int K0, int K1, bool EMIT>
BSK_HD void leaf(const Grid &g, const double *breaks0, const double *breaks1, long long b, long long i, long long j, long long a,
                 long long bb, int depth, long long &count, unsigned &status, long long base, long long total, int64_t *keys,
                 double *xy)
{
    const long long I = (i << depth) + a, J = (j << depth) + bb;
    const long long NJ = (g.nc1 << depth) + 1;
    const bool s00 = node_value<K0, K1>(g, b, I, J, depth) >= 0.0;
    const bool s10 = node_value<K0, K1>(g, b, I + 1, J, depth) >= 0.0;
    const bool s11 = node_value<K0, K1>(g, b, I + 1, J + 1, depth) >= 0.0;
    const bool s01 = node_value<K0, K1>(g, b, I, J + 1, depth) >= 0.0;
    // +1: a segment starts on the edge (from + to - counter-clockwise), -1: one ends, 0: not crossed
    const int t0 = (int)s00 - (int)s10, t1 = (int)s10 - (int)s11, t2 = (int)s11 - (int)s01, t3 = (int)s01 - (int)s00;
    const int ncross = (t0 != 0) + (t1 != 0) + (t2 != 0) + (t3 != 0);
    if (ncross == 0) return;
    bool cpos = false;
    if (ncross == 4) {
        const double inv = 1.0 / (double)(1 << depth);
        double c[K0 * K1];
        double vc = __builtin_nan("");
        if (load_cell<K0, K1>(g, b, i, j, c)) vc = value2<K0, K1>(c, (double)(2 * a + 1) * (0.5 * inv), (double)(2 * bb + 1) * (0.5 * inv));
        cpos = vc >= 0.0;
        status |= STATUS_SADDLE;
    }
    const int last = t0 < 0 ? 0 : (t1 < 0 ? 1 : (t2 < 0 ? 2 : 3));         // the end of the one segment of 2 crossings
#pragma nounroll
    for (int k = 0; k < 4; ++k) {
        const int tk = k == 0 ? t0 : (k == 1 ? t1 : (k == 2 ? t2 : t3));
        if (tk <= 0) continue;
        if (EMIT) {
            const int e = ncross == 2 ? last : ((k + (cpos ? 1 : 3)) & 3);
            long long key[2];
            double pt[4];
#pragma nounroll
            for (int w = 0; w < 2; ++w) {
                const int n = w == 0 ? k : e;
                // bottom (I, J, 0) from n00; right (I + 1, J, 1) from n10; top (I, J + 1, 0) from n01; left (I, J, 1) from n00
                const long long EI = n == 1 ? I + 1 : I, EJ = n == 2 ? J + 1 : J;
                const int dir = n & 1;
                const bool pos = n == 1 ? s10 : (n == 2 ? s01 : s00);
                double u, v;
                vertex<K0, K1>(g, breaks0, breaks1, b, EI, EJ, dir, depth, pos, u, v);
                if (w == 0) {
                    key[0] = ((EI * NJ + EJ) << 1) | dir;
                    pt[0] = u;
                    pt[1] = v;
                } else {
                    key[1] = ((EI * NJ + EJ) << 1) | dir;
                    pt[2] = u;
                    pt[3] = v;
                }
            }
            const long long at = base + count;
            if (at >= 0 && at < total) {
                keys[2 * at] = key[0];
                keys[2 * at + 1] = key[1];
                xy[4 * at] = pt[0];
                xy[4 * at + 1] = pt[1];
                xy[4 * at + 2] = pt[2];
                xy[4 * at + 3] = pt[3];
            }
        }
        ++count;
    }
}

// One step down from a live node: cur becomes its left live child, else its right live one (0, 1), or stays (-1).
template <int K0, int K1, int AXIS>
BSK_HD int descend(double *cur, double tau)
{
    constexpr int N = K0 * K1;
    double left[N], right[N];
    halve<1, K0, K1, AXIS>(cur, left, right);
    const bool liveL = !one_side<N>(left, tau), liveR = !one_side<N>(right, tau);
#pragma unroll
    for (int e = 0; e < N; ++e) cur[e] = liveL ? left[e] : (liveR ? right[e] : cur[e]);
    return liveL ? 0 : (liveR ? 1 : -1);
}

// node (depth, path) below a top box: index and halvings per axis, axis 0 first
BSK_HD void node_index(int depth, unsigned path, unsigned &i0, int &h0, unsigned &i1, int &h1)
{
    i0 = 0;
    i1 = 0;
    h0 = 0;
    h1 = 0;
    for (int k = 0; k < 2 * CONTOUR_MAX_DEPTH; ++k)
        if (k < depth) {
            const unsigned bit = (path >> (depth - 1 - k)) & 1u;
            if ((k & 1) == 0) {
                i0 = 2 * i0 + bit;
                ++h0;
            } else {
                i1 = 2 * i1 + bit;
                ++h1;
            }
        }
}

template <int K0, int K1>
BSK_HD void flag_lane(const Grid &g, long long at, uint8_t *cand, uint8_t *zero)
{
    const long long ncell = g.nc0 * g.nc1;
    const long long b = at / ncell, cell = at - b * ncell;
    const long long i = cell / g.nc1, j = cell - i * g.nc1;
    double c[K0 * K1];
    uint8_t f = 0, z = 0;
    if (load_cell<K0, K1>(g, b, i, j, c)) {
        const double S = g.scale[b];
        const double small = S * CONTOUR_EPS;
        bool all = true;
#pragma unroll
        for (int e = 0; e < K0 * K1; ++e) all = all && fabs(c[e]) < small;
        z = (all || S == 0.0) ? 1 : 0;
        f = (!z && !one_side<K0 * K1>(c, tau_of<K0, K1>(S))) ? 1 : 0;
    }
    cand[at] = f;
    zero[at] = z;
}

// cand: [ncand] flat (field, cell) indices; lanes = ncand << 2P.  EMIT = false writes counts[lane] and lane_status[lane];
// EMIT = true reads offsets[lane] and writes keys [total, 2] and xy [total, 4].
template <int K0, int K1, bool EMIT>
BSK_HD void march_lane(const Grid &g, const double *breaks0, const double *breaks1, const int64_t *cand, long long ncand, int depth,
                       int P, long long lane, const int64_t *offsets, long long total, int32_t *counts, uint8_t *lane_status,
                       int64_t *keys, double *xy)
{
    constexpr int N = K0 * K1;
    const long long n = lane >> (2 * P);
    const unsigned q = (unsigned)(lane & ((1ll << (2 * P)) - 1));
    const unsigned qi = q >> P, qj = q & ((1u << P) - 1u);
    const int D = depth - P;
    long long count = 0;
    unsigned status = 0;
    const long long base = EMIT ? offsets[lane] : 0;
    const long long ncell = g.nc0 * g.nc1;
    const long long at = n < ncand ? cand[n] : -1;
    const long long b = at >= 0 ? at / ncell : -1;
    const long long cell = at - b * ncell;
    const long long i = cell / g.nc1, j = cell - i * g.nc1;
    double cur[N];
    bool live = false, done = true;
    double tau = 0.0;
    {
        double own[N];
        if (at >= 0 && load_cell<K0, K1>(g, b, i, j, own)) {
            tau = tau_of<K0, K1>(g.scale[b]);
            const double w = 1.0 / (double)(1 << P);
            if (P > 0) {
                restrict_box<1, K0, K1>(own, (double)qi * w, w, (double)qj * w, w, cur);
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e) cur[e] = own[e];
            }
            live = !one_side<N>(cur, tau);
            done = false;
        }
    }
    int depth_now = 0;
    unsigned path = 0;
    for (int it = 0; it < CONTOUR_WALK && !done; ++it) {
        if (!live) {
            for (int k = 0; k < 2 * CONTOUR_MAX_DEPTH; ++k)
                if (path & 1u) {
                    path >>= 1;
                    --depth_now;
                }
            if (depth_now == 0) {
                done = true;
            } else {
                path |= 1u;
                unsigned i0, i1;
                int h0, h1;
                node_index(depth_now, path, i0, h0, i1, h1);
                const double w0 = 1.0 / (double)(1 << (P + h0)), w1 = 1.0 / (double)(1 << (P + h1));
                double own[N];
                load_cell<K0, K1>(g, b, i, j, own);            // the cell's own coefficients, read again
                restrict_box<1, K0, K1>(own, (double)((qi << h0) + i0) * w0, w0, (double)((qj << h1) + i1) * w1, w1, cur);
                live = !one_side<N>(cur, tau);
            }
        } else if (depth_now == 2 * D) {
            unsigned i0, i1;
            int h0, h1;
            node_index(depth_now, path, i0, h0, i1, h1);
            leaf<K0, K1, EMIT>(g, breaks0, breaks1, b, i, j, (long long)((qi << D) + i0), (long long)((qj << D) + i1), depth, count,
                               status, base, total, keys, xy);
            live = false;
        } else {
            const int child = (depth_now & 1) ? descend<K0, K1, 1>(cur, tau) : descend<K0, K1, 0>(cur, tau);
            if (child < 0) {
                live = false;
            } else {
                path = (path << 1) | (unsigned)child;
                ++depth_now;
            }
        }
    }
    if (!EMIT) {
        counts[lane] = (int32_t)count;
        lane_status[lane] = (uint8_t)status;
    }
}

#ifdef __HIPCC__
template <int K0, int K1>
__global__ __launch_bounds__(CONTOUR_BLOCK) void contour_flag(Grid g, uint8_t *__restrict__ cand, uint8_t *__restrict__ zero)
{
    const long long gid = (long long)blockIdx.x * CONTOUR_BLOCK + threadIdx.x;
    if (gid >= g.nfields * g.nc0 * g.nc1) return;
    flag_lane<K0, K1>(g, gid, cand, zero);
}

template <int K0, int K1, bool EMIT>
__global__ __launch_bounds__(CONTOUR_MARCH_BLOCK) void contour_march(Grid g, const double *__restrict__ breaks0,
                                                                    const double *__restrict__ breaks1,
                                                                    const int64_t *__restrict__ cand, long long ncand, int depth,
                                                                    int P, const int64_t *__restrict__ offsets, long long total,
                                                                    int32_t *__restrict__ counts, uint8_t *__restrict__ lane_status,
                                                                    int64_t *__restrict__ keys, double *__restrict__ xy)
{
    const long long gid = (long long)blockIdx.x * CONTOUR_MARCH_BLOCK + threadIdx.x;
    if (gid >= (ncand << (2 * P))) return;
    march_lane<K0, K1, EMIT>(g, breaks0, breaks1, cand, ncand, depth, P, gid, offsets, total, counts, lane_status, keys, xy);
}
#endif

}  // namespace bskcontour
