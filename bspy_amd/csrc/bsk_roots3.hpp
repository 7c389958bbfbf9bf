// Isolated common zeros of three scalar splines in three variables (bspy_amd/roots3.py): the bsk_roots3_* family.
//
// The caller has brought all three variables to Bezier form (the band operator of bsk_refine.hpp, once per axis): rows is
// [nsys, 3, R0, R1, R2] in fp64 and cell (i, j, k) of system b is the K0 x K1 x K2 window of the three components at
// first0[i], first1[j], first2[k].
//
//   roots3_flag     lane = (system, cell), the last cell index fastest: adjacent lanes read adjacent windows of the
//                   innermost axis.  1 unless the cell is masked (a zero cell) or a component's K0 K1 K2 Bernstein
//                   coefficients are all > 0 or all < 0.  A lane keeps two booleans per component, no array.
//   roots3_isolate  ONE WAVE = one flagged (system, cell); lane (i0 K1 + i1) K2 + i2 holds coefficient (i0, i1, i2) of the
//                   three components: three doubles for the node that is walked (cur) and three for the cell's own
//                   coefficients (own).  The two bivariate arrays of roots2_isolate (the node and its halves) would be
//                   3 x 192 doubles a lane here.  The wave, its halves along an axis (left_part, right_part) and its sign
//                   test (one_side, here with the threshold Zero: strictly of one sign) are bsk_wave3.hpp's.
//                   The walk is that of roots2_isolate: a stackless depth-first walk of the binary tree of dyadic boxes
//                   of the unit cell, depth d splits axis d mod 3, ROOTS3_DEPTH = 19 halvings per axis, a node is
//                   (depth << 57) | path in one 64-bit integer (6 + 57 bits: 19 is the most that fits).
//                     live node, not a leaf   the left half along the axis (a compile-time axis of the step); when a
//                                             component of it is strictly of one sign, the right half; the first live
//                                             one is walked next with the halved coefficients; none: not live
//                     otherwise               strip the trailing 1 bits (back up), set bit 0 (the right sibling) and
//                                             restrict the cell's OWN coefficients to that box: axis 0, then 1, then 2,
//                                             each the right part at lo and then the left part at w / (1 - lo)
//                     depth 0 after stripping: the walk is complete.
//                   Every trip of the loop is one visited node; more than ROOTS3_WALK of them set status bit 1.
//                   A leaf (width w = 2^-19 on all axes): Newton on the cell's polynomial from the centre, value and
//                   3 x 3 Jacobian by trivariate de Casteljau (axis 2, then 1, then 0; the results sit in lane 0 and are
//                   broadcast), Cramer's rule with IEEE division, at most ROOTS3_NEWTON steps; convergence, leaving the
//                   box and a zero determinant as in roots2_isolate.  A converged x inside the cell grown by 2^-44 is
//                   clamped and mapped; it is dropped when the cell already holds a zero within 2^-20 h on all axes, it
//                   sets status bit 2 when the R = min(6 (K0 - 1)(K1 - 1)(K2 - 1), 32) slots are full.  An unconverged
//                   leaf whose three centre values are within 4 (K0 + K1 + K2) w^2 S_d (= c (K0 + K1 + K2) eps S_d with
//                   c = 2^18: what a zero of second order leaves at the centre of a box of width w) sets status bit 4.
//                   Lane 0 alone writes: the slots, the near bytes, the count, the status and the node count.
//   roots3_merge    lane = one zero with near set.  It is dropped (keep = 0) when one of the 13 neighbouring cells of the
//                   same system with a lower flat index holds a zero within 2^-20 h on all axes, h the widths of the
//                   lane's own cell.  The neighbour's slots are found through table = cumsum(flags) - 1.  A lane writes
//                   its own keep byte and nothing else.
//
// The arithmetic is that of bsk_roots.hpp (fp64, no contraction, lerp(s, t, a, b) = s a + t b), one association for the
// host drivers and the kernels: the walk is written once, over the LaneWave and the HostWave of bsk_wave3.hpp.
// roots3.flag_cell and roots3.isolate_cell state it in Python.
// No atomics, no waiting, no LDS, and every loop has a compile-time trip bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsk_roots.hpp"
#include "bsk_wave3.hpp"

#pragma clang fp contract(off)

namespace bskroots3 {

using bskroots::lerp;

constexpr int ROOTS3_BLOCK = 256;                   // roots3_flag, roots3_merge
constexpr int ROOTS3_WAVE = 64;                     // roots3_isolate: one wave a workgroup, one cell a wave
constexpr int ROOTS3_DEPTH = 19;                    // halvings per axis: 3 x 19 path bits + 6 bits of depth = 63
constexpr int ROOTS3_NEWTON = 8;
// nodes a walk may visit: 4 x 4065, the largest count on the recorded cases, rounded up to a power of two
constexpr int ROOTS3_WALK = 16384;
constexpr double ROOTS3_LEAF_W = 0x1p-19;
constexpr double ROOTS3_GROW = 0x1p-44;
constexpr double ROOTS3_SAME = 0x1p-20;
constexpr double ROOTS3_SMALL_STEP = 0x1p-40;
constexpr double ROOTS3_TANGENT = 0x1p-36;          // 4 w^2 = 2^18 eps
constexpr int ROOTS3_MAX_SLOTS = 32;
constexpr int ROOTS3_PATH_BITS = 57;
constexpr unsigned STATUS_WALK = 1, STATUS_SLOTS = 2, STATUS_TANGENT = 4;

constexpr int slots(int K0, int K1, int K2)
{
    return 6 * (K0 - 1) * (K1 - 1) * (K2 - 1) < ROOTS3_MAX_SLOTS ? 6 * (K0 - 1) * (K1 - 1) * (K2 - 1) : ROOTS3_MAX_SLOTS;
}

// One cell of one system in the extracted rows: component d, coefficient (i0, i1, i2) at p[d * sd + i0 * s0 + i1 * s1 + i2].
// A cell is anything with at(d, i0, i1, i2): CellRef reads its coefficients, bsk_ssx.hpp's PairCell forms them.
struct CellRef {
    const double *p;
    long long sd, s0, s1;
    BSK_HD double at(int d, int i0, int i1, int i2) const { return p[d * sd + i0 * s0 + i1 * s1 + i2]; }
};

// ------------------------------------------------------------------------------------------ the walk, once for both waves
// The wave (bsk_wave3.hpp) with three components; the sign tests take the threshold Zero.
using bskwave3::descend;
using bskwave3::restrict_axis;
using bskwave3::Zero;
using HostWave = bskwave3::HostWave<3>;
#ifdef __HIPCC__
using LaneWave = bskwave3::LaneWave<3>;
#endif

// the box of node (depth, path): corners and widths per axis, exact
BSK_HD void node_box(int depth, uint64_t path, double *lo, double *w)
{
    uint64_t at[3] = {0, 0, 0};
    w[0] = w[1] = w[2] = 1.0;
    for (int k = 0; k < 3 * ROOTS3_DEPTH; k += 3)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (k + a < depth) {
                at[a] = 2 * at[a] + ((path >> (depth - 1 - k - a)) & 1u);
                w[a] = 0.5 * w[a];
            }
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = (double)at[a] * w[a];
}

BSK_HD double outside(double x, double lo, double w)
{
    const double below = lo - x, above = x - (lo + w);
    double d = 0.0;
    if (below > d) d = below;
    if (above > d) d = above;
    if (!(x == x)) d = __builtin_inf();
    return d;
}

BSK_HD double det3(double a00, double a01, double a02, double a10, double a11, double a12, double a20, double a21, double a22)
{
    const double m0 = a11 * a22 - a12 * a21;
    const double m1 = a10 * a22 - a12 * a20;
    const double m2 = a10 * a21 - a11 * a20;
    return (a00 * m0 - a01 * m1) + a02 * m2;
}

// F[d] and J[d][0 .. 2] of the cell's own coefficients at x
template <class W, int K0, int K1, int K2>
BSK_HD void eval3(const W &wave, const typename W::V *own, const double *x, double *F, double (*J)[3])
{
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        typename W::V p, q, pv, pd, qv, f, f0, f1, f2, unused;
        wave.template eval_axis<K2, 1>(own[d], x[2], p, q);
        wave.template eval_axis<K1, K2>(p, x[1], pv, pd);
        wave.template eval_axis<K1, K2>(q, x[1], qv, unused);
        wave.template eval_axis<K0, K1 * K2>(pv, x[0], f, f0);
        wave.template eval_axis<K0, K1 * K2>(pd, x[0], f1, unused);
        wave.template eval_axis<K0, K1 * K2>(qv, x[0], f2, unused);
        F[d] = wave.get0(f);
        J[d][0] = wave.get0(f0);
        J[d][1] = wave.get0(f1);
        J[d][2] = wave.get0(f2);
    }
}

// The leaf box with corner lo: at most one zero into out, see the head of this file.  t0, h: the cell; S: the scales.
template <class W, int K0, int K1, int K2>
BSK_HD void leaf(const W &wave, const typename W::V *own, const double *lo, const double *t0, const double *h, const double *S,
                 double *out, uint8_t *near, int &count, unsigned &status)
{
    constexpr int R = slots(K0, K1, K2);
    const double w = ROOTS3_LEAF_W;
    double x[3] = {lo[0] + 0.5 * w, lo[1] + 0.5 * w, lo[2] + 0.5 * w};
    double prev = __builtin_inf(), last = __builtin_inf(), fc[3] = {0.0, 0.0, 0.0};
    bool conv = false, ended = false;
    for (int step = 0; step < ROOTS3_NEWTON && !ended; ++step) {
        double F[3], J[3][3];
        eval3<W, K0, K1, K2>(wave, own, x, F, J);
        if (step == 0) {
            fc[0] = F[0];
            fc[1] = F[1];
            fc[2] = F[2];
        }
        const double det = det3(J[0][0], J[0][1], J[0][2], J[1][0], J[1][1], J[1][2], J[2][0], J[2][1], J[2][2]);
        if (det == 0.0) {
            ended = true;
        } else {
            const double d0 = det3(F[0], J[0][1], J[0][2], F[1], J[1][1], J[1][2], F[2], J[2][1], J[2][2]) / det;
            const double d1 = det3(J[0][0], F[0], J[0][2], J[1][0], F[1], J[1][2], J[2][0], F[2], J[2][2]) / det;
            const double d2 = det3(J[0][0], J[0][1], F[0], J[1][0], J[1][1], F[1], J[2][0], J[2][1], F[2]) / det;
            const double n0 = x[0] - d0, n1 = x[1] - d1, n2 = x[2] - d2;
            double far = outside(n0, lo[0], w);
            const double far1 = outside(n1, lo[1], w), far2 = outside(n2, lo[2], w);
            if (far1 > far) far = far1;
            if (far2 > far) far = far2;
            if (!(far <= 2.0 * w)) {
                ended = true;
            } else {
                x[0] = n0;
                x[1] = n1;
                x[2] = n2;
                last = fabs(d0);
                if (fabs(d1) > last) last = fabs(d1);
                if (fabs(d2) > last) last = fabs(d2);
                if (!(last < prev)) {
                    conv = true;
                    ended = true;
                }
                prev = last;
            }
        }
    }
    if (!ended && last <= ROOTS3_SMALL_STEP) conv = true;      // every step shrank and the last one is far below w
    if (!conv) {
        const double tol = (double)(K0 + K1 + K2) * ROOTS3_TANGENT;
        if (fabs(fc[0]) <= tol * S[0] && fabs(fc[1]) <= tol * S[1] && fabs(fc[2]) <= tol * S[2]) status |= STATUS_TANGENT;
        return;
    }
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) in = in && x[a] >= -ROOTS3_GROW && x[a] <= 1.0 + ROOTS3_GROW;
    if (!in) return;
    double u[3], tol[3];
    bool close = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        x[a] = x[a] < 0.0 ? 0.0 : (x[a] > 1.0 ? 1.0 : x[a]);
        u[a] = t0[a] + x[a] * h[a];
        tol[a] = ROOTS3_SAME * h[a];
        close = close || x[a] <= ROOTS3_SAME || x[a] >= 1.0 - ROOTS3_SAME;
    }
    int seen = 0;
    if (wave.first())                                          // lane 0 reads what lane 0 wrote
        for (int q = 0; q < R; ++q)
            if (q < count && fabs(out[3 * q] - u[0]) <= tol[0] && fabs(out[3 * q + 1] - u[1]) <= tol[1] &&
                fabs(out[3 * q + 2] - u[2]) <= tol[2])
                seen = 1;
    seen = wave.bcast(seen);
    if (seen) return;
    if (count >= R) {
        status |= STATUS_SLOTS;
        return;
    }
    if (wave.first()) {
        out[3 * count] = u[0];
        out[3 * count + 1] = u[1];
        out[3 * count + 2] = u[2];
        near[count] = close ? 1 : 0;
    }
    ++count;
}

// out: R x 3 slots (the zeros in front, NaN behind), near: R bytes.  The cell is a candidate (roots3_flag said 1).
template <class W, int K0, int K1, int K2, class Ref>
BSK_HD void isolate_cell(const W &wave, const Ref &ref, const double *t0, const double *t1, const double *S, double *out,
                         uint8_t *near, int32_t *count_out, uint8_t *status_out, int32_t *nodes_out)
{
    constexpr int R = slots(K0, K1, K2);
    constexpr int N = K0 * K1 * K2;
    const double h[3] = {t1[0] - t0[0], t1[1] - t0[1], t1[2] - t0[2]};
    if (wave.first())
        for (int q = 0; q < R; ++q) {
            out[3 * q] = __builtin_nan("");
            out[3 * q + 1] = __builtin_nan("");
            out[3 * q + 2] = __builtin_nan("");
            near[q] = 0;
        }
    typename W::V own[3], cur[3];
    wave.template load<K0, K1, K2>(ref, own);
#pragma unroll
    for (int d = 0; d < 3; ++d) cur[d] = own[d];
    uint64_t node = 0;                                         // (depth << 57) | path
    const uint64_t PATH = (1ull << ROOTS3_PATH_BITS) - 1;
    bool live = true, done = false;
    int count = 0, nodes = 0;
    unsigned status = 0;
    for (int it = 0; it < ROOTS3_WALK && !done; ++it) {
        ++nodes;
        int depth = (int)(node >> ROOTS3_PATH_BITS);
        uint64_t path = node & PATH;
        if (!live) {
            const int ones = __builtin_ctzll(~path);           // the trailing 1 bits: at most depth of them
            path >>= ones;
            depth -= ones;
            if (depth <= 0) {
                done = true;
            } else {
                path |= 1u;
                double lo[3], w[3];
                node_box(depth, path, lo, w);
#pragma unroll
                for (int d = 0; d < 3; ++d) cur[d] = own[d];
                restrict_axis<W, K0, K1 * K2>(wave, cur, lo[0], w[0]);
                restrict_axis<W, K1, K2>(wave, cur, lo[1], w[1]);
                restrict_axis<W, K2, 1>(wave, cur, lo[2], w[2]);
                live = !wave.template one_side<N>(cur, Zero{});
            }
        } else if (depth == 3 * ROOTS3_DEPTH) {
            double lo[3], w[3];
            node_box(depth, path, lo, w);
            leaf<W, K0, K1, K2>(wave, own, lo, t0, h, S, out, near, count, status);
            live = false;
        } else {
            const int axis = depth % 3;
            const int child = axis == 0 ? descend<W, 3, K0, K1, K2, 0>(wave, cur, Zero{})
                                        : (axis == 1 ? descend<W, 3, K0, K1, K2, 1>(wave, cur, Zero{})
                                                     : descend<W, 3, K0, K1, K2, 2>(wave, cur, Zero{}));
            if (child < 0) {
                live = false;
            } else {
                path = (path << 1) | (uint64_t)child;
                ++depth;
            }
        }
        node = ((uint64_t)depth << ROOTS3_PATH_BITS) | path;
    }
    if (!done) status |= STATUS_WALK;
    if (wave.first()) {
        *count_out = count;
        *status_out = (uint8_t)status;
        *nodes_out = nodes;
    }
}

// ------------------------------------------------------------------------------------------ the tables of a launch
// rows: [nsys, 3, R0, R1, R2]; first_a: [nc_a]; breaks_a: [nc_a + 1].
struct Grid {
    const double *rows;
    long long nsys, R0, R1, R2, nc0, nc1, nc2;
    const int32_t *first0, *first1, *first2;
};

struct Breaks {
    const double *b0, *b1, *b2;
};

// the cell of flat index `at` (system, i, j, k); false: not a cell, or its window leaves the rows
template <int K0, int K1, int K2>
BSK_HD bool cell_ref(const Grid &g, long long at, CellRef &ref, long long &b, long long *ijk)
{
    const long long ncell = g.nc0 * g.nc1 * g.nc2;
    if (at < 0 || at >= g.nsys * ncell) return false;
    b = at / ncell;
    const long long cell = at - b * ncell;
    ijk[0] = cell / (g.nc1 * g.nc2);
    ijk[1] = (cell / g.nc2) % g.nc1;
    ijk[2] = cell % g.nc2;
    const long long f0 = g.first0[ijk[0]], f1 = g.first1[ijk[1]], f2 = g.first2[ijk[2]];
    if (f0 < 0 || f0 + K0 > g.R0 || f1 < 0 || f1 + K1 > g.R1 || f2 < 0 || f2 + K2 > g.R2) return false;
    ref.s1 = g.R2;
    ref.s0 = g.R1 * g.R2;
    ref.sd = g.R0 * ref.s0;
    ref.p = g.rows + b * 3 * ref.sd + f0 * ref.s0 + f1 * ref.s1 + f2;
    return true;
}

template <int K0, int K1, int K2>
BSK_HD void flag_lane(const Grid &g, long long at, const uint8_t *mask, uint8_t *flags)
{
    CellRef ref;
    long long b, ijk[3];
    int f = 0;
    if (!mask[at] && cell_ref<K0, K1, K2>(g, at, ref, b, ijk)) {
        bool ex = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            bool pos = true, neg = true;
#pragma unroll
            for (int i0 = 0; i0 < K0; ++i0)
#pragma unroll
                for (int i1 = 0; i1 < K1; ++i1)
#pragma unroll
                    for (int i2 = 0; i2 < K2; ++i2) {
                        const double v = ref.p[d * ref.sd + i0 * ref.s0 + i1 * ref.s1 + i2];
                        pos = pos && v > 0.0;
                        neg = neg && v < 0.0;
                    }
            ex = ex || pos || neg;
        }
        f = ex ? 0 : 1;
    }
    flags[at] = (uint8_t)f;
}

// candidate `slot` of the launch, by one wave
template <class W, int K0, int K1, int K2>
BSK_HD void isolate_wave(const W &wave, const Grid &g, long long slot, const Breaks &br, const double *scale, const int64_t *cand,
                         double *roots, uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes)
{
    constexpr int R = slots(K0, K1, K2);
    CellRef ref;
    long long b, ijk[3];
    double *out = roots + slot * 3 * R;
    if (!cell_ref<K0, K1, K2>(g, cand[slot], ref, b, ijk)) {
        if (wave.first()) {
            for (int q = 0; q < R; ++q) {
                out[3 * q] = __builtin_nan("");
                out[3 * q + 1] = __builtin_nan("");
                out[3 * q + 2] = __builtin_nan("");
                near[slot * R + q] = 0;
            }
            count[slot] = 0;
            status[slot] = 0;
            nodes[slot] = 0;
        }
        return;
    }
    const double t0[3] = {br.b0[ijk[0]], br.b1[ijk[1]], br.b2[ijk[2]]};
    const double t1[3] = {br.b0[ijk[0] + 1], br.b1[ijk[1] + 1], br.b2[ijk[2] + 1]};
    const double S[3] = {scale[3 * b], scale[3 * b + 1], scale[3 * b + 2]};
    isolate_cell<W, K0, K1, K2, CellRef>(wave, ref, t0, t1, S, out, near + slot * R, count + slot, status + slot, nodes + slot);
}

// roots: [ncand, R, 3]; cand: [ncand]; flags, table: [nsys, nc0, nc1, nc2]; which: [nnear] flat (candidate, slot); keep: [ncand, R]
BSK_HD void merge_lane(long long lane, int R, const double *roots, long long nsys, long long nc0, long long nc1, long long nc2,
                       const Breaks &br, const int64_t *cand, long long ncand, const uint8_t *flags, const int64_t *table,
                       const int64_t *which, uint8_t *keep)
{
    const long long at = which[lane];
    if (at < 0 || at >= ncand * R) return;
    const long long slot = at / R;
    const long long cellat = cand[slot];
    const long long ncell = nc0 * nc1 * nc2;
    if (cellat < 0 || cellat >= nsys * ncell) return;
    const long long b = cellat / ncell, cell = cellat - b * ncell;
    const long long i = cell / (nc1 * nc2), j = (cell / nc2) % nc1, k = cell % nc2;
    const double u = roots[3 * at], v = roots[3 * at + 1], w = roots[3 * at + 2];
    const double tolu = ROOTS3_SAME * (br.b0[i + 1] - br.b0[i]), tolv = ROOTS3_SAME * (br.b1[j + 1] - br.b1[j]);
    const double tolw = ROOTS3_SAME * (br.b2[k + 1] - br.b2[k]);
    uint8_t kept = (u == u) ? 1 : 0;
    for (int n = 0; n < 13; ++n) {                             // the 13 of the 26 neighbours that precede (i, j, k)
        const long long ni = i + n / 9 - 1, nj = j + (n / 3) % 3 - 1, nk = k + n % 3 - 1;
        if (ni < 0 || nj < 0 || nk < 0 || ni >= nc0 || nj >= nc1 || nk >= nc2) continue;
        const long long nat = b * ncell + (ni * nc1 + nj) * nc2 + nk;
        if (!flags[nat]) continue;
        const long long ns = table[nat];
        if (ns < 0 || ns >= ncand) continue;
        for (int q = 0; q < R; ++q) {
            const double *z = roots + 3 * (ns * R + q);
            if (fabs(z[0] - u) <= tolu && fabs(z[1] - v) <= tolv && fabs(z[2] - w) <= tolw) kept = 0;
        }
    }
    keep[at] = kept;
}

// The host drivers' loops over flag_lane and isolate_wave (bsk_roots3_tu.hip): out of line and on a 64-byte boundary, so
// that where their instructions lie does not depend on the dispatcher that calls them.  Host functions: the device pass
// emits nothing for them.
template <int K0, int K1, int K2>
__attribute__((noinline, aligned(64))) void flag_host(const Grid &g, const uint8_t *mask, uint8_t *flags)
{
    const long long lanes = g.nsys * g.nc0 * g.nc1 * g.nc2;
    for (long long at = 0; at < lanes; ++at) flag_lane<K0, K1, K2>(g, at, mask, flags);
}

template <int K0, int K1, int K2>
__attribute__((noinline, aligned(64))) void isolate_host(const Grid &g, const Breaks &br, const double *scale, const int64_t *cand,
                                                         long long ncand, double *roots, uint8_t *near, int32_t *count, uint8_t *status,
                                                         int32_t *nodes)
{
    const HostWave wave;
    for (long long slot = 0; slot < ncand; ++slot)
        isolate_wave<HostWave, K0, K1, K2>(wave, g, slot, br, scale, cand, roots, near, count, status, nodes);
}

// BSK_ROOTS3_FUNCTIONS_ONLY: a unit that takes the walk for cells of its own (bsk_ssx.hpp) leaves the kernels to bsk_roots3_tu.hip
#if defined(__HIPCC__) && !defined(BSK_ROOTS3_FUNCTIONS_ONLY)
template <int K0, int K1, int K2>
__global__ __launch_bounds__(ROOTS3_BLOCK) void roots3_flag(Grid g, const uint8_t *__restrict__ mask, uint8_t *__restrict__ flags)
{
    const long long gid = (long long)blockIdx.x * ROOTS3_BLOCK + threadIdx.x;
    if (gid >= g.nsys * g.nc0 * g.nc1 * g.nc2) return;
    flag_lane<K0, K1, K2>(g, gid, mask, flags);
}

// one workgroup = one wave = one candidate: every lane of the wave takes every branch together
template <int K0, int K1, int K2>
__global__ __launch_bounds__(ROOTS3_WAVE) void roots3_isolate(Grid g, Breaks br, const double *__restrict__ scale,
                                                             const int64_t *__restrict__ cand, long long ncand, double *roots,
                                                             uint8_t *near, int32_t *__restrict__ count,
                                                             uint8_t *__restrict__ status, int32_t *__restrict__ nodes)
{
    const long long slot = blockIdx.x;
    if (slot >= ncand) return;
    const LaneWave wave{(int)threadIdx.x};
    isolate_wave<LaneWave, K0, K1, K2>(wave, g, slot, br, scale, cand, roots, near, count, status, nodes);
}

__global__ __launch_bounds__(ROOTS3_BLOCK) void roots3_merge(int R, const double *__restrict__ roots, long long nsys, long long nc0,
                                                            long long nc1, long long nc2, Breaks br,
                                                            const int64_t *__restrict__ cand, long long ncand,
                                                            const uint8_t *__restrict__ flags, const int64_t *__restrict__ table,
                                                            const int64_t *__restrict__ which, long long nnear,
                                                            uint8_t *__restrict__ keep)
{
    const long long gid = (long long)blockIdx.x * ROOTS3_BLOCK + threadIdx.x;
    if (gid >= nnear) return;
    merge_lane(gid, R, roots, nsys, nc0, nc1, nc2, br, cand, ncand, flags, table, which, keep);
}
#endif

}  // namespace bskroots3
