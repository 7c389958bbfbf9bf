// Level surfaces of a scalar spline in three variables (bspy_amd/isosurface.py): the bsk_iso_* family.
//
// The caller has brought all three variables to Bezier form (the band operator of bsk_refine.hpp, once per axis): rows is
// [nrows, R0, R1, R2] in fp64 and cell (i, j, k) is the K0 x K1 x K2 window at first0[i], first1[j], first2[k].  Field b
// reads rows[b], or, with levels, rows[0] with levels[b] subtracted from every coefficient as it is loaded.  No knot of
// the caller's is a jump, so the two cells next to a knot plane hold the same floats on it.
//
// Every cell carries a lattice of G x G x G leaves, G = 2^depth.  Node (I, J, K) = cell (i, j, k), local (a0, a1, a2).
//   node value   the cell with the lowest flat index that contains the node owns it: per axis io = (I - 1) / G for I > 0,
//                else 0, a = I - io G.  value = de Casteljau of the owner's coefficients along axis 2 at a2 / G, then
//                along axis 1, then along axis 0 (eval3).  v >= 0 is positive.
//   tetrahedra   a leaf cube is cut into the 6 Kuhn tetrahedra along its diagonal (0,0,0) - (1,1,1): tetrahedron t belongs
//                to the t-th permutation (a, b, c) of the axes in lexicographic order and has the corners v0 = (0,0,0),
//                v1 = v0 + e_a, v2 = v1 + e_b, v3 = (1,1,1).  A corner is the 3-bit number 4 c0 + 2 c1 + c2.
//   edge         from node (I, J, K) in direction d = 4 d0 + 2 d1 + d2, d in 1 .. 7; key = (((I NJ + J) NK + K) << 3) | d
//                with NJ = nc1 G + 1, NK = nc2 G + 1.  Every edge of a tetrahedron runs from its lower corner to its higher
//                one.  It is crossed when the signs of its two nodes differ.
//   vertex       of a crossed edge, a function of (field, key): the owner of the edge is, per axis, the cell I / G of a
//                moving axis and the owner of I of a fixed one.  Its coefficients are reduced in the fixed axes (2, then 1,
//                then 0: de Casteljau at a / G); f(s) = eval3 of what is left at a / G + s / G in the moving axes; s = the
//                sign bisection of roots_isolate on [0, 1] from the sign of the node value of (I, J, K): at most 60 steps,
//                until the midpoint is an end or f is 0.0.  A local x of cell i becomes lerp(1 - x, x, t_i, t_{i+1}).
//   triangles    of a tetrahedron with corners m = 0 .. 3: one corner p apart from q < r < s: (pq, pr, ps); two negative
//                p < q and two positive r < s: the quad (pr, ps, qs, qr) cut along pr - qs: (pr, ps, qs), (pr, qs, qr).
//                The parity of (p, q, r, s), the sign of the permutation (a, b, c) and which side is positive decide
//                whether the last two vertices of every triangle are exchanged (the quad: reversed), so that the right-hand
//                normal points into f >= 0.
//
//   iso_flag     lane = (field, cell): zero = every coefficient is below S eps in magnitude (or S is 0); cand = not zero
//                and not (all coefficients > tau or all < -tau), tau = 32 (K0 + K1 + K2) eps S.
//   iso_walk     ONE WAVE = one (candidate cell, top box of the 8^P boxes of its cell); lane (i0 K1 + i1) K2 + i2 holds
//                coefficient (i0, i1, i2): one double for the box that is walked and one for the cell's own coefficient
//                (the wave of bsk_wave3.hpp with one component).  The wave restricts the cell to its top box and walks the
//                3 (depth - P) binary levels below it (axis 0, 1, 2 in turn) depth first without a stack: a half is
//                dropped when it is on one side of tau (one_side); backing up strips the trailing 1 bits of the path
//                and restricts the cell's own coefficients again.  EMIT = false counts the leaves that survive;
//                EMIT = true writes their flat indices ((b NL0 + I) NL1 + J) NL2 + K, NL = nc G, at offsets[wave] + n
//                in the order of the walk.  Lane 0 alone writes.
//   iso_leaf     lane = one surviving leaf (the caller has sorted them).  The 8 canonical node values come from the owners'
//                coefficients, read again from global memory when the owner changes; the 6 tetrahedra are classified on the
//                8 sign bits.  EMIT = false counts the triangles and stores 2 into the status byte of the leaf's cell when
//                a node value is exactly 0.0 (every lane that stores there stores the same byte); EMIT = true writes
//                the triangles as key triples at offsets[lane] + n, plain vector stores.
//   iso_vertex   lane = one unique crossed edge (field, key): (u, v, w) as above.
//
// fp64, no contraction, lerp(s, t, a, b) = s a + t b: one association for the host drivers and the kernels; the walk is
// written once over the LaneWave and the HostWave of bsk_wave3.hpp.  No LDS, no atomics, no waiting, every loop has a
// compile-time trip bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsk_roots.hpp"
#include "bsk_wave3.hpp"

#pragma clang fp contract(off)

namespace bskiso {

using bskroots::lerp;
using bskroots::value;
using bskwave3::one_side;                           // all coefficients > tau or all < -tau

constexpr int ISO_BLOCK = 256;                      // iso_flag, iso_leaf, iso_vertex
constexpr int ISO_WAVE = 64;                        // iso_walk: one wave a workgroup
constexpr int ISO_MAX_DEPTH = 6;
constexpr int ISO_BISECT = bskroots::ROOTS_BISECT;
// trips of a walk below one top box: at most 2^18 leaves, fewer inner nodes and as many steps back
constexpr int ISO_WALK = 1 << 20;
constexpr double ISO_TAU = 32.0;                    // tau = ISO_TAU (K0 + K1 + K2) eps S
constexpr double ISO_EPS = 0x1p-52;
constexpr unsigned STATUS_ZERO_NODE = 2;
// corners v1 and v2 of tetrahedron t (3 bits each) and the sign of its permutation (bit t: even)
constexpr unsigned TET_V1 = 4u | (4u << 3) | (2u << 6) | (2u << 9) | (1u << 12) | (1u << 15);
constexpr unsigned TET_V2 = 6u | (5u << 3) | (6u << 6) | (3u << 9) | (5u << 12) | (3u << 15);
constexpr unsigned TET_EVEN = 0x19;

// The tables of a launch.  rows: [nrows, R0, R1, R2]; first_a: [nc_a]; levels: [nfields] or null; scale: [nfields].
struct Grid {
    const double *rows;
    long long nrows, R0, R1, R2, nc0, nc1, nc2;
    const int32_t *first0, *first1, *first2;
    const double *levels;
    long long nfields;
    const double *scale;
};

struct Breaks {
    const double *b0, *b1, *b2;
};

// where cell (i, j, k) of field b starts in the rows, and its level; false: not a cell, or its window leaves the rows
template <int K0, int K1, int K2>
BSK_HD bool cell_at(const Grid &g, long long b, long long i, long long j, long long k, const double *&p, double &lev)
{
    if (b < 0 || b >= g.nfields || i < 0 || i >= g.nc0 || j < 0 || j >= g.nc1 || k < 0 || k >= g.nc2) return false;
    const long long rb = g.levels ? 0 : b;
    if (rb >= g.nrows) return false;
    const long long f0 = g.first0[i], f1 = g.first1[j], f2 = g.first2[k];
    if (f0 < 0 || f0 + K0 > g.R0 || f1 < 0 || f1 + K1 > g.R1 || f2 < 0 || f2 + K2 > g.R2) return false;
    lev = g.levels ? g.levels[b] : 0.0;
    p = g.rows + ((rb * g.R0 + f0) * g.R1 + f1) * g.R2 + f2;
    return true;
}

template <int K0, int K1, int K2>
BSK_HD bool load_cell(const Grid &g, long long b, long long i, long long j, long long k, double *c)
{
    const double *p = nullptr;
    double lev = 0.0;
    if (!cell_at<K0, K1, K2>(g, b, i, j, k, p, lev)) return false;
#pragma unroll
    for (int r = 0; r < K0; ++r)
#pragma unroll
        for (int s = 0; s < K1; ++s)
#pragma unroll
            for (int t = 0; t < K2; ++t) c[(r * K1 + s) * K2 + t] = p[(r * g.R1 + s) * g.R2 + t] - lev;
    return true;
}

template <int K0, int K1, int K2>
BSK_HD double tau_of(double S)
{
    return ISO_TAU * (double)(K0 + K1 + K2) * ISO_EPS * S;
}

// de Casteljau at x along axis AX of an N0 x N1 x N2 array: out is the array with one entry on that axis
template <int N0, int N1, int N2, int AX>
BSK_HD void reduce(const double *in, double x, double *out)
{
    constexpr int K = AX == 0 ? N0 : (AX == 1 ? N1 : N2);
    constexpr int S = AX == 0 ? N1 * N2 : (AX == 1 ? N2 : 1);
    constexpr int O0 = AX == 0 ? 1 : N0, O1 = AX == 1 ? 1 : N1, O2 = AX == 2 ? 1 : N2;
#pragma unroll
    for (int o0 = 0; o0 < O0; ++o0)
#pragma unroll
        for (int o1 = 0; o1 < O1; ++o1)
#pragma unroll
            for (int o2 = 0; o2 < O2; ++o2) {
                double line[K];
#pragma unroll
                for (int e = 0; e < K; ++e) line[e] = in[(o0 * N1 + o1) * N2 + o2 + e * S];
                out[(o0 * O1 + o1) * O2 + o2] = value<K>(line, x);
            }
}

// axis 2, then 1, then 0
template <int N0, int N1, int N2>
BSK_HD double eval3(const double *c, double x0, double x1, double x2)
{
    double a[N0 * N1], b[N0], r[1];
    reduce<N0, N1, N2, 2>(c, x2, a);
    reduce<N0, N1, 1, 1>(a, x1, b);
    reduce<N0, 1, 1, 0>(b, x0, r);
    return r[0];
}

// owner and local index of the lattice coordinate I: the lowest cell that contains it
BSK_HD void owner_of(long long I, int depth, long long &cell, long long &a)
{
    cell = I > 0 ? (I - 1) >> depth : 0;
    a = I - (cell << depth);
}

template <int K0, int K1, int K2>
BSK_HD double node_value(const Grid &g, long long b, long long I, long long J, long long K, int depth)
{
    const double inv = 1.0 / (double)(1 << depth);
    long long i, a0, j, a1, k, a2;
    owner_of(I, depth, i, a0);
    owner_of(J, depth, j, a1);
    owner_of(K, depth, k, a2);
    double c[K0 * K1 * K2];
    if (!load_cell<K0, K1, K2>(g, b, i, j, k, c)) return __builtin_nan("");
    return eval3<K0, K1, K2>(c, (double)a0 * inv, (double)a1 * inv, (double)a2 * inv);
}

// s of the crossed edge of direction D from the local point (x0, x1, x2) of the cell c; pos: the sign at s = 0
template <int K0, int K1, int K2, int D>
BSK_HD double edge_root(const double *c, double x0, double x1, double x2, double inv, bool pos)
{
    constexpr bool m0 = (D & 4) != 0, m1 = (D & 2) != 0, m2 = (D & 1) != 0;
    constexpr int M0 = m0 ? K0 : 1, M1 = m1 ? K1 : 1, M2 = m2 ? K2 : 1;
    double a[K0 * K1 * M2], b[K0 * M1 * M2], r[M0 * M1 * M2];
    if (m2) {
#pragma unroll
        for (int e = 0; e < K0 * K1 * K2; ++e) a[e] = c[e];
    } else {
        reduce<K0, K1, K2, 2>(c, x2, a);
    }
    if (m1) {
#pragma unroll
        for (int e = 0; e < K0 * K1 * M2; ++e) b[e] = a[e];
    } else {
        reduce<K0, K1, M2, 1>(a, x1, b);
    }
    if (m0) {
#pragma unroll
        for (int e = 0; e < K0 * M1 * M2; ++e) r[e] = b[e];
    } else {
        reduce<K0, M1, M2, 0>(b, x0, r);
    }
    double lo = 0.0, hi = 1.0;
    for (int step = 0; step < ISO_BISECT; ++step) {
        const double m = 0.5 * (lo + hi);
        if (m == lo || m == hi) break;
        const double t = m * inv;
        const double f = eval3<M0, M1, M2>(r, m0 ? x0 + t : x0, m1 ? x1 + t : x1, m2 ? x2 + t : x2);
        if (f == 0.0) {
            lo = m;
            hi = m;
            break;
        }
        if ((f > 0.0) == pos) lo = m;
        else hi = m;
    }
    return 0.5 * (lo + hi);
}

template <int K0, int K1, int K2>
BSK_HD void flag_lane(const Grid &g, long long at, uint8_t *cand, uint8_t *zero)
{
    const long long ncell = g.nc0 * g.nc1 * g.nc2;
    const long long b = at / ncell, cell = at - b * ncell;
    const long long i = cell / (g.nc1 * g.nc2), j = (cell / g.nc2) % g.nc1, k = cell % g.nc2;
    double c[K0 * K1 * K2];
    uint8_t f = 0, z = 0;
    if (load_cell<K0, K1, K2>(g, b, i, j, k, c)) {
        const double S = g.scale[b];
        const double small = S * ISO_EPS;
        bool all = true;
#pragma unroll
        for (int e = 0; e < K0 * K1 * K2; ++e) all = all && fabs(c[e]) < small;
        z = (all || S == 0.0) ? 1 : 0;
        f = (!z && !one_side<K0 * K1 * K2>(c, tau_of<K0, K1, K2>(S))) ? 1 : 0;
    }
    cand[at] = f;
    zero[at] = z;
}

// ------------------------------------------------------------------------------------------ the walk, once for both waves
// The wave (bsk_wave3.hpp) with one component; the sign tests take the threshold tau.
using bskwave3::descend;
using bskwave3::restrict_axis;
using HostWave = bskwave3::HostWave<1>;
#ifdef __HIPCC__
using LaneWave = bskwave3::LaneWave<1>;
#endif

// One cell of the rows with the level subtracted as it is read: coefficient (i0, i1, i2) is p[i0 s0 + i1 s1 + i2] - lev.
struct LevelCell {
    const double *p;
    long long s0, s1;
    double lev;
    BSK_HD double at(int, int i0, int i1, int i2) const { return p[i0 * s0 + i1 * s1 + i2] - lev; }
};

// box (depth, path) below a top box: index and halvings per axis, axis 0 first
BSK_HD void node_index(int depth, unsigned path, unsigned *at, int *h)
{
    at[0] = at[1] = at[2] = 0;
    h[0] = h[1] = h[2] = 0;
    for (int k = 0; k < 3 * ISO_MAX_DEPTH; k += 3)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (k + a < depth) {
                at[a] = 2 * at[a] + ((path >> (depth - 1 - k - a)) & 1u);
                ++h[a];
            }
}

// cand: [ncand] flat (field, cell) indices; waves = ncand << 3P, wave = (candidate << 3P) | (q0 << 2P) | (q1 << P) | q2.
// EMIT = false writes counts[wave]; EMIT = true reads offsets[wave] and writes leaves [total].
template <class W, int K0, int K1, int K2, bool EMIT>
BSK_HD void walk_wave(const W &wave, const Grid &g, const int64_t *cand, long long ncand, int depth, int P, long long slot,
                      const int64_t *offsets, long long total, int32_t *counts, int64_t *leaves)
{
    constexpr int N = K0 * K1 * K2;
    const long long n = slot >> (3 * P);
    const unsigned mask = (1u << P) - 1u;
    const unsigned q = (unsigned)(slot & ((1ll << (3 * P)) - 1));
    const unsigned top[3] = {(q >> (2 * P)) & mask, (q >> P) & mask, q & mask};
    const int D = depth - P;
    const long long ncell = g.nc0 * g.nc1 * g.nc2;
    const long long at = n < ncand ? cand[n] : -1;
    const long long b = at >= 0 ? at / ncell : -1;
    const long long cell = at - b * ncell;
    const long long i = cell / (g.nc1 * g.nc2), j = (cell / g.nc2) % g.nc1, k = cell % g.nc2;
    const long long NL1 = g.nc1 << depth, NL2 = g.nc2 << depth;
    const long long base = EMIT ? offsets[slot] : 0;
    long long count = 0;
    typename W::V own, cur;
    const double *p = nullptr;
    double lev = 0.0, tau = 0.0;
    bool live = false, done = true;
    if (at >= 0 && cell_at<K0, K1, K2>(g, b, i, j, k, p, lev)) {
        wave.template load<K0, K1, K2>(LevelCell{p, g.R1 * g.R2, g.R2, lev}, &own);
        tau = tau_of<K0, K1, K2>(g.scale[b]);
        cur = own;
        if (P > 0) {
            const double w = 1.0 / (double)(1 << P);
            restrict_axis<W, K0, K1 * K2>(wave, &cur, (double)top[0] * w, w);
            restrict_axis<W, K1, K2>(wave, &cur, (double)top[1] * w, w);
            restrict_axis<W, K2, 1>(wave, &cur, (double)top[2] * w, w);
        }
        live = !wave.template one_side<N>(&cur, tau);
        done = false;
    } else {
        wave.clear(own);                                          // not a cell: nothing is walked
        wave.clear(cur);
    }
    int depth_now = 0;
    unsigned path = 0;
    for (int it = 0; it < ISO_WALK && !done; ++it) {
        if (!live) {
            for (int s = 0; s < 3 * ISO_MAX_DEPTH; ++s)
                if (path & 1u) {
                    path >>= 1;
                    --depth_now;
                }
            if (depth_now == 0) {
                done = true;
            } else {
                path |= 1u;
                unsigned idx[3];
                int h[3];
                node_index(depth_now, path, idx, h);
                cur = own;
                const double w0 = 1.0 / (double)(1 << (P + h[0])), w1 = 1.0 / (double)(1 << (P + h[1])), w2 = 1.0 / (double)(1 << (P + h[2]));
                restrict_axis<W, K0, K1 * K2>(wave, &cur, (double)((top[0] << h[0]) + idx[0]) * w0, w0);
                restrict_axis<W, K1, K2>(wave, &cur, (double)((top[1] << h[1]) + idx[1]) * w1, w1);
                restrict_axis<W, K2, 1>(wave, &cur, (double)((top[2] << h[2]) + idx[2]) * w2, w2);
                live = !wave.template one_side<N>(&cur, tau);
            }
        } else if (depth_now == 3 * D) {
            unsigned idx[3];
            int h[3];
            node_index(depth_now, path, idx, h);
            if (EMIT) {
                const long long I = (i << depth) + (long long)((top[0] << D) + idx[0]);
                const long long J = (j << depth) + (long long)((top[1] << D) + idx[1]);
                const long long K = (k << depth) + (long long)((top[2] << D) + idx[2]);
                const long long where = base + count;
                if (wave.first() && where >= 0 && where < total) leaves[where] = ((b * (g.nc0 << depth) + I) * NL1 + J) * NL2 + K;
            }
            ++count;
            live = false;
        } else {
            const int axis = depth_now % 3;
            const int child = axis == 0 ? descend<W, 1, K0, K1, K2, 0>(wave, &cur, tau)
                                        : (axis == 1 ? descend<W, 1, K0, K1, K2, 1>(wave, &cur, tau)
                                                     : descend<W, 1, K0, K1, K2, 2>(wave, &cur, tau));
            if (child < 0) {
                live = false;
            } else {
                path = (path << 1) | (unsigned)child;
                ++depth_now;
            }
        }
    }
    if (!EMIT && wave.first()) counts[slot] = (int32_t)count;
}

// ------------------------------------------------------------------------------------------ leaves and vertices
// the key of the edge between the corners m1 and m2 of a tetrahedron (corners: 4 x 3 bits) of the leaf at node (I, J, K)
BSK_HD long long edge_key(unsigned corners, int m1, int m2, long long I, long long J, long long K, long long NJ, long long NK)
{
    const int lo = m1 < m2 ? m1 : m2, hi = m1 < m2 ? m2 : m1;
    const unsigned c1 = (corners >> (3 * lo)) & 7u, c2 = (corners >> (3 * hi)) & 7u;
    const long long node = ((I + (long long)(c1 >> 2)) * NJ + J + (long long)((c1 >> 1) & 1u)) * NK + K + (long long)(c1 & 1u);
    return (node << 3) | (long long)(c1 ^ c2);
}

// leaves: [nleaves] flat leaf indices.  EMIT = false writes counts[lane] and, for a node value 0.0, status[cell] = 2;
// EMIT = true reads offsets[lane] and writes tris [total, 3].
template <int K0, int K1, int K2, bool EMIT>
BSK_HD void leaf_lane(const Grid &g, const int64_t *leaves, int depth, long long lane, const int64_t *offsets, long long total,
                      int32_t *counts, uint8_t *status, int64_t *tris)
{
    const long long NL0 = g.nc0 << depth, NL1 = g.nc1 << depth, NL2 = g.nc2 << depth;
    const long long NJ = NL1 + 1, NK = NL2 + 1;
    const long long at = leaves[lane];
    const double inv = 1.0 / (double)(1 << depth);
    long long count = 0;
    const long long base = EMIT ? offsets[lane] : 0;
    if (at >= 0 && at < g.nfields * NL0 * NL1 * NL2) {
        const long long K = at % NL2, J = (at / NL2) % NL1, I = (at / (NL1 * NL2)) % NL0, b = at / (NL0 * NL1 * NL2);
        double c[K0 * K1 * K2];
        long long ci = -1, cj = -1, ck = -1;
        unsigned signs = 0;
        bool zero = false, ok = true;
#pragma nounroll
        for (int n = 0; n < 8; ++n) {
            long long i, a0, j, a1, k, a2;
            owner_of(I + ((n >> 2) & 1), depth, i, a0);
            owner_of(J + ((n >> 1) & 1), depth, j, a1);
            owner_of(K + (n & 1), depth, k, a2);
            if (i != ci || j != cj || k != ck) {
                ok = load_cell<K0, K1, K2>(g, b, i, j, k, c) && ok;
                ci = i;
                cj = j;
                ck = k;
            }
            const double v = ok ? eval3<K0, K1, K2>(c, (double)a0 * inv, (double)a1 * inv, (double)a2 * inv) : __builtin_nan("");
            signs |= (v >= 0.0 ? 1u : 0u) << n;
            zero = zero || v == 0.0;
        }
        if (ok) {
            if (!EMIT && zero) status[((b * g.nc0 + (I >> depth)) * g.nc1 + (J >> depth)) * g.nc2 + (K >> depth)] = (uint8_t)STATUS_ZERO_NODE;
#pragma nounroll
            for (int t = 0; t < 6; ++t) {
                const unsigned v1 = (TET_V1 >> (3 * t)) & 7u, v2 = (TET_V2 >> (3 * t)) & 7u;
                const unsigned corners = (v1 << 3) | (v2 << 6) | (7u << 9);
                const unsigned s4 = (signs & 1u) | (((signs >> v1) & 1u) << 1) | (((signs >> v2) & 1u) << 2) | (((signs >> 7) & 1u) << 3);
                const int npos = __builtin_popcount(s4);
                if (npos == 0 || npos == 4) continue;
                const bool even = ((TET_EVEN >> t) & 1u) != 0;
                long long key[4];
                bool good;
                if (npos == 2) {
                    const unsigned neg = ~s4 & 15u;
                    const int p = __builtin_ctz(neg), q = 31 - __builtin_clz(neg), r = __builtin_ctz(s4), s = 31 - __builtin_clz(s4);
                    const int inversions = (p > r) + (p > s) + (q > r) + (q > s);
                    good = ((inversions & 1) == 0) == even;
                    key[0] = edge_key(corners, p, r, I, J, K, NJ, NK);
                    key[1] = edge_key(corners, p, s, I, J, K, NJ, NK);
                    key[2] = edge_key(corners, q, s, I, J, K, NJ, NK);
                    key[3] = edge_key(corners, q, r, I, J, K, NJ, NK);
                } else {
                    const int p = __builtin_ctz(npos == 1 ? s4 : (~s4 & 15u));
                    const int q = p == 0 ? 1 : 0, r = p <= 1 ? 2 : 1, s = p <= 2 ? 3 : 2;
                    good = (((p & 1) == 0) == even) != (npos == 1);
                    key[0] = edge_key(corners, p, q, I, J, K, NJ, NK);
                    key[1] = edge_key(corners, p, r, I, J, K, NJ, NK);
                    key[2] = edge_key(corners, p, s, I, J, K, NJ, NK);
                    key[3] = 0;
                }
                if (EMIT) {
                    const long long where = base + count;
                    if (where >= 0 && where < total) {
                        tris[3 * where] = key[0];
                        tris[3 * where + 1] = good ? key[1] : (npos == 2 ? key[3] : key[2]);
                        tris[3 * where + 2] = npos == 2 ? key[2] : (good ? key[2] : key[1]);
                    }
                    if (npos == 2 && where + 1 >= 0 && where + 1 < total) {
                        tris[3 * where + 3] = key[0];
                        tris[3 * where + 4] = key[2];
                        tris[3 * where + 5] = good ? key[3] : key[1];
                    }
                }
                count += npos == 2 ? 2 : 1;
            }
        }
    }
    if (!EMIT) counts[lane] = (int32_t)count;
}

// keys, fields: [n]; xyz: [n, 3].  A key that is no edge of the lattice gives NaN.
template <int K0, int K1, int K2>
BSK_HD void vertex_lane(const Grid &g, const Breaks &br, const int64_t *keys, const int64_t *fields, int depth, long long lane, double *xyz)
{
    const long long NL[3] = {g.nc0 << depth, g.nc1 << depth, g.nc2 << depth};
    const long long NJ = NL[1] + 1, NK = NL[2] + 1;
    const long long key = keys[lane], b = fields[lane];
    const int d = (int)(key & 7);
    const long long node = key >> 3;
    const long long at[3] = {node / (NJ * NK), (node / NK) % NJ, node % NK};
    const double inv = 1.0 / (double)(1 << depth);
    double out[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    bool ok = key >= 0 && d != 0;
    long long cell[3] = {0, 0, 0}, a[3] = {0, 0, 0};
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const bool moving = ((d >> (2 - x)) & 1) != 0;
        ok = ok && at[x] + (moving ? 1 : 0) <= NL[x];
        if (moving) {
            cell[x] = at[x] >> depth;
            a[x] = at[x] - (cell[x] << depth);
        } else {
            owner_of(at[x], depth, cell[x], a[x]);
        }
    }
    double c[K0 * K1 * K2];
    if (ok && load_cell<K0, K1, K2>(g, b, cell[0], cell[1], cell[2], c)) {
        const bool pos = node_value<K0, K1, K2>(g, b, at[0], at[1], at[2], depth) >= 0.0;
        const double x0 = (double)a[0] * inv, x1 = (double)a[1] * inv, x2 = (double)a[2] * inv;
        double s;
        switch (d) {
        case 1: s = edge_root<K0, K1, K2, 1>(c, x0, x1, x2, inv, pos); break;
        case 2: s = edge_root<K0, K1, K2, 2>(c, x0, x1, x2, inv, pos); break;
        case 3: s = edge_root<K0, K1, K2, 3>(c, x0, x1, x2, inv, pos); break;
        case 4: s = edge_root<K0, K1, K2, 4>(c, x0, x1, x2, inv, pos); break;
        case 5: s = edge_root<K0, K1, K2, 5>(c, x0, x1, x2, inv, pos); break;
        case 6: s = edge_root<K0, K1, K2, 6>(c, x0, x1, x2, inv, pos); break;
        default: s = edge_root<K0, K1, K2, 7>(c, x0, x1, x2, inv, pos); break;
        }
        const double t = s * inv;
        const double y0 = (d & 4) ? x0 + t : x0, y1 = (d & 2) ? x1 + t : x1, y2 = (d & 1) ? x2 + t : x2;
        out[0] = lerp(1.0 - y0, y0, br.b0[cell[0]], br.b0[cell[0] + 1]);
        out[1] = lerp(1.0 - y1, y1, br.b1[cell[1]], br.b1[cell[1] + 1]);
        out[2] = lerp(1.0 - y2, y2, br.b2[cell[2]], br.b2[cell[2] + 1]);
    }
    xyz[3 * lane] = out[0];
    xyz[3 * lane + 1] = out[1];
    xyz[3 * lane + 2] = out[2];
}

#ifdef __HIPCC__
template <int K0, int K1, int K2>
__global__ __launch_bounds__(ISO_BLOCK) void iso_flag(Grid g, uint8_t *__restrict__ cand, uint8_t *__restrict__ zero)
{
    const long long gid = (long long)blockIdx.x * ISO_BLOCK + threadIdx.x;
    if (gid >= g.nfields * g.nc0 * g.nc1 * g.nc2) return;
    flag_lane<K0, K1, K2>(g, gid, cand, zero);
}

// one workgroup = one wave = one top box: every lane of the wave takes every branch together
template <int K0, int K1, int K2, bool EMIT>
__global__ __launch_bounds__(ISO_WAVE) void iso_walk(Grid g, const int64_t *__restrict__ cand, long long ncand, int depth, int P,
                                                    const int64_t *__restrict__ offsets, long long total,
                                                    int32_t *__restrict__ counts, int64_t *__restrict__ leaves)
{
    const long long slot = blockIdx.x;
    if (slot >= (ncand << (3 * P))) return;
    const LaneWave wave{(int)threadIdx.x};
    walk_wave<LaneWave, K0, K1, K2, EMIT>(wave, g, cand, ncand, depth, P, slot, offsets, total, counts, leaves);
}

template <int K0, int K1, int K2, bool EMIT>
__global__ __launch_bounds__(ISO_BLOCK) void iso_leaf(Grid g, const int64_t *__restrict__ leaves, long long nleaves, int depth,
                                                     const int64_t *__restrict__ offsets, long long total,
                                                     int32_t *__restrict__ counts, uint8_t *status, int64_t *__restrict__ tris)
{
    const long long gid = (long long)blockIdx.x * ISO_BLOCK + threadIdx.x;
    if (gid >= nleaves) return;
    leaf_lane<K0, K1, K2, EMIT>(g, leaves, depth, gid, offsets, total, counts, status, tris);
}

template <int K0, int K1, int K2>
__global__ __launch_bounds__(ISO_BLOCK) void iso_vertex(Grid g, Breaks br, const int64_t *__restrict__ keys,
                                                       const int64_t *__restrict__ fields, long long n, int depth,
                                                       double *__restrict__ xyz)
{
    const long long gid = (long long)blockIdx.x * ISO_BLOCK + threadIdx.x;
    if (gid >= n) return;
    vertex_lane<K0, K1, K2>(g, br, keys, fields, depth, gid, xyz);
}
#endif

}  // namespace bskiso
