// Isolated common zeros of two scalar splines in two variables (bspy_amd/roots2.py): the bsk_roots2_* family.
//
// The caller has brought both variables to Bezier form (the band operator of bsk_refine.hpp, once per axis): rows is
// [nsys, 2, R0, R1] in fp64 and cell (i, j) of system b is the K0 x K1 window of both components at first0[i], first1[j].
//
//   roots2_flag     lane = (system, cell): 1 unless the cell is masked (a zero cell) or a component's K0 K1 Bernstein
//                   coefficients are all > 0 or all < 0.
//   roots2_isolate  lane = one flagged (system, cell).  A stackless depth-first walk of the binary tree of dyadic boxes
//                   of the unit cell: depth d splits axis d mod 2, ROOTS2_DEPTH halvings per axis.  A node is
//                   (depth << 48) | path in one 64-bit integer, the newest choice in bit 0 of the path; the corner of its
//                   box is a sum of powers of two, computed exactly from the bits.
//                     live node, not a leaf   halve along the axis (lerp at 1/2: the sign a hull has never flips); a child
//                                             is dropped when either component's coefficients are strictly of one sign;
//                                             the left live child is walked next, else the right one, and it keeps the
//                                             halved coefficients
//                     otherwise               strip the trailing 1 bits (back up), set bit 0 (the right sibling) and
//                                             restrict the cell's OWN coefficients, read again from global memory, to that
//                                             box (bskroots::restrict_to per column, then per row); test it as above
//                     depth 0 after stripping: the walk is complete.
//                   Every trip of the loop is one visited node; more than ROOTS2_WALK of them set status bit 1.
//                   A leaf (width w = 2^-24 on both axes): Newton on the cell's polynomial from the centre, value and
//                   Jacobian by bivariate de Casteljau, Cramer's rule with IEEE division, at most ROOTS2_NEWTON steps.
//                   An iterate farther than 2 w (max-norm) from the box, or a determinant of 0, ends it unconverged.  It has
//                   converged when a step is not smaller than the one before, or when the last step is <= 2^-40.  A
//                   converged x inside the cell grown by 2^-44 is clamped to the cell and becomes (t0 + x h) per axis;
//                   it is dropped when the lane has already written a root within 2^-20 h of it on both axes, it sets
//                   status bit 2 when the R = 2 (K0 - 1)(K1 - 1) slots are full.  An unconverged leaf whose centre
//                   values are both within 4 (K0 + K1) eps S_d sets status bit 4 (a tangential or singular zero); any other
//                   one is a near miss.  near[slot] = 1 for a root within 2^-20 of an edge of the unit cell.
//   roots2_merge    lane = one root with near set.  It is dropped (keep = 0) when a neighbouring cell of the same system
//                   with a lower flat index (i - 1, j - 1), (i - 1, j), (i - 1, j + 1), (i, j - 1) holds a root within
//                   2^-20 h on both axes, h the widths of the lane's own cell.  The neighbour's slots are found through
//                   table[system, cell] = cumsum(flags) - 1.  A lane writes its own keep byte and nothing else.
//
// The arithmetic is that of bsk_roots.hpp (fp64, no contraction, lerp(s, t, a, b) = s a + t b), one association for the
// host drivers and the kernels; roots2.flag_cell and roots2.isolate_cell state it in Python.  No atomics, no waiting, and
// every loop has a compile-time trip bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsk_box2.hpp"
#include "bsk_roots.hpp"

#pragma clang fp contract(off)

namespace bskroots2 {

using bskbox2::halve;
using bskbox2::restrict_box;
using bskroots::lerp;

constexpr int ROOTS2_BLOCK = 256;                   // roots2_flag, roots2_merge
constexpr int ROOTS2_ISOLATE_BLOCK = 64;            // one wave: the walk may use the whole register file
constexpr int ROOTS2_DEPTH = 24;                    // halvings per axis
constexpr int ROOTS2_NEWTON = 8;
// nodes a walk may visit: 4 x 5052, the largest count on the recorded cases, rounded up to a power of two
constexpr int ROOTS2_WALK = 32768;
constexpr double ROOTS2_LEAF_W = 0x1p-24;
constexpr double ROOTS2_GROW = 0x1p-44;
constexpr double ROOTS2_SAME = 0x1p-20;
constexpr double ROOTS2_SMALL_STEP = 0x1p-40;
constexpr double ROOTS2_EPS = 0x1p-52;
constexpr unsigned STATUS_WALK = 1, STATUS_SLOTS = 2, STATUS_TANGENT = 4;

constexpr int slots(int K0, int K1) { return 2 * (K0 - 1) * (K1 - 1); }

// One cell of one system in the extracted rows: component d, row i, column j at p[d * sd + i * si + j].
struct CellRef {
    const double *p;
    long long sd, si;
};

template <int K0, int K1>
BSK_HD void load_cell(const CellRef &ref, double *c)
{
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int i = 0; i < K0; ++i)
#pragma unroll
            for (int j = 0; j < K1; ++j) c[(d * K0 + i) * K1 + j] = ref.p[d * ref.sd + i * ref.si + j];
}

template <int N>
BSK_HD bool one_sign(const double *c)
{
    bool pos = true, neg = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pos = pos && c[i] > 0.0;
        neg = neg && c[i] < 0.0;
    }
    return pos || neg;
}

template <int K0, int K1>
BSK_HD bool excluded(const double *c)
{
    return one_sign<K0 * K1>(c) || one_sign<K0 * K1>(c + K0 * K1);
}

// One step down from a live node: cur becomes its left live child, else its right live one (0, 1), or stays (-1: both
// children are dropped).  The halves are locals of the step and cur is written once, in index order.
template <int K0, int K1, int AXIS>
BSK_HD int descend(double *cur)
{
    constexpr int N = 2 * K0 * K1;
    double left[N], right[N];
    halve<2, K0, K1, AXIS>(cur, left, right);
    const bool liveL = !excluded<K0, K1>(left), liveR = !excluded<K0, K1>(right);
#pragma unroll
    for (int e = 0; e < N; ++e) cur[e] = liveL ? left[e] : (liveR ? right[e] : cur[e]);
    return liveL ? 0 : (liveR ? 1 : -1);
}

// value and derivative of K Bernstein coefficients at x
template <int K>
BSK_HD void eval1(const double *c, double x, double &val, double &der)
{
    double b[K];
    const double s = 1.0 - x;
#pragma unroll
    for (int i = 0; i < K; ++i) b[i] = c[i];
#pragma unroll
    for (int r = 1; r < K - 1; ++r)
#pragma unroll
        for (int i = 0; i < K - r; ++i) b[i] = lerp(s, x, b[i], b[i + 1]);
    der = (double)(K - 1) * (b[1] - b[0]);
    val = lerp(s, x, b[0], b[1]);
}

// one component (K0 x K1) at (x0, x1): value, d/dx0, d/dx1
template <int K0, int K1>
BSK_HD void eval2(const double *c, double x0, double x1, double &f, double &f0, double &f1)
{
    double p[K0], q[K0];
#pragma unroll
    for (int i = 0; i < K0; ++i) eval1<K1>(c + i * K1, x1, p[i], q[i]);
    eval1<K0>(p, x0, f, f0);
    f1 = bskroots::value<K0>(q, x0);
}

// the box of node (depth, path): corner and widths, exact
BSK_HD void node_box(int depth, uint64_t path, double &lo0, double &w0, double &lo1, double &w1)
{
    uint64_t i0 = 0, i1 = 0;
    w0 = 1.0;
    w1 = 1.0;
    for (int k = 0; k < 2 * ROOTS2_DEPTH; ++k)
        if (k < depth) {
            const uint64_t bit = (path >> (depth - 1 - k)) & 1u;
            if ((k & 1) == 0) {
                i0 = 2 * i0 + bit;
                w0 = 0.5 * w0;
            } else {
                i1 = 2 * i1 + bit;
                w1 = 0.5 * w1;
            }
        }
    lo0 = (double)i0 * w0;
    lo1 = (double)i1 * w1;
}

template <int K0, int K1>
BSK_HD int flag_cell(const double *c, unsigned mask)
{
    if (mask) return 0;
    return excluded<K0, K1>(c) ? 0 : 1;
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

// The leaf box with corner (lo0, lo1): at most one root into out, see the head of this file.  Ref: where the cell's own
// coefficients come from, load_cell<K0, K1>(ref, c): CellRef reads them, bsk_rays.hpp's RayCell forms them.
template <int K0, int K1, class Ref>
BSK_HD void leaf(const Ref &ref, double lo0, double lo1, double t0u, double hu, double t0v, double hv, double S0, double S1,
                 double *out, uint8_t *near, int &count, unsigned &status)
{
    constexpr int R = slots(K0, K1);
    const double w = ROOTS2_LEAF_W;
    double x0 = lo0 + 0.5 * w, x1 = lo1 + 0.5 * w;
    double prev = __builtin_inf(), last = __builtin_inf(), fc0 = 0.0, fc1 = 0.0;
    bool conv = false, ended = false;
    for (int step = 0; step < ROOTS2_NEWTON && !ended; ++step) {
        double c[2 * K0 * K1];
        load_cell<K0, K1>(ref, c);
        double f, fu, fv, g, gu, gv;
        eval2<K0, K1>(c, x0, x1, f, fu, fv);
        eval2<K0, K1>(c + K0 * K1, x0, x1, g, gu, gv);
        if (step == 0) {
            fc0 = f;
            fc1 = g;
        }
        const double det = fu * gv - fv * gu;
        if (det == 0.0) {
            ended = true;
        } else {
            const double du = (f * gv - fv * g) / det;
            const double dv = (fu * g - f * gu) / det;
            const double n0 = x0 - du, n1 = x1 - dv;
            const double far0 = outside(n0, lo0, w), far1 = outside(n1, lo1, w);
            if (!((far0 > far1 ? far0 : far1) <= 2.0 * w)) {
                ended = true;
            } else {
                x0 = n0;
                x1 = n1;
                const double a0 = fabs(du), a1 = fabs(dv);
                last = a0 > a1 ? a0 : a1;
                if (!(last < prev)) {
                    conv = true;
                    ended = true;
                }
                prev = last;
            }
        }
    }
    if (!ended && last <= ROOTS2_SMALL_STEP) conv = true;      // every step shrank and the last one is far below w
    if (!conv) {
        const double tol = 4.0 * (K0 + K1) * ROOTS2_EPS;
        if (fabs(fc0) <= tol * S0 && fabs(fc1) <= tol * S1) status |= STATUS_TANGENT;
        return;
    }
    if (!(x0 >= -ROOTS2_GROW && x0 <= 1.0 + ROOTS2_GROW && x1 >= -ROOTS2_GROW && x1 <= 1.0 + ROOTS2_GROW)) return;
    x0 = x0 < 0.0 ? 0.0 : (x0 > 1.0 ? 1.0 : x0);
    x1 = x1 < 0.0 ? 0.0 : (x1 > 1.0 ? 1.0 : x1);
    const double u = t0u + x0 * hu, v = t0v + x1 * hv;
    const double tolu = ROOTS2_SAME * hu, tolv = ROOTS2_SAME * hv;
    bool seen = false;
    for (int q = 0; q < R; ++q)
        if (q < count && fabs(out[2 * q] - u) <= tolu && fabs(out[2 * q + 1] - v) <= tolv) seen = true;
    if (seen) return;
    if (count >= R) {
        status |= STATUS_SLOTS;
        return;
    }
    out[2 * count] = u;
    out[2 * count + 1] = v;
    near[count] = (x0 <= ROOTS2_SAME || x0 >= 1.0 - ROOTS2_SAME || x1 <= ROOTS2_SAME || x1 >= 1.0 - ROOTS2_SAME) ? 1 : 0;
    ++count;
}

// out: R x 2 slots (the roots in front, NaN behind), near: R bytes.  The cell is a candidate (roots2_flag said 1).
template <int K0, int K1, class Ref>
BSK_HD void isolate_cell(const Ref &ref, double t0u, double t1u, double t0v, double t1v, double S0, double S1, double *out,
                         uint8_t *near, int32_t *count_out, uint8_t *status_out, int32_t *nodes_out)
{
    constexpr int R = slots(K0, K1);
    constexpr int N = 2 * K0 * K1;
    const double hu = t1u - t0u, hv = t1v - t0v;
    for (int q = 0; q < R; ++q) {
        out[2 * q] = __builtin_nan("");
        out[2 * q + 1] = __builtin_nan("");
        near[q] = 0;
    }
    double cur[N];
    load_cell<K0, K1>(ref, cur);
    uint64_t node = 0;                                         // (depth << 48) | path
    const uint64_t PATH = (1ull << 48) - 1;
    bool live = true, done = false;
    int count = 0, nodes = 0;
    unsigned status = 0;
    for (int it = 0; it < ROOTS2_WALK && !done; ++it) {
        ++nodes;
        int depth = (int)(node >> 48);
        uint64_t path = node & PATH;
        if (!live) {
            for (int k = 0; k < 2 * ROOTS2_DEPTH; ++k)
                if (path & 1u) {
                    path >>= 1;
                    --depth;
                }
            if (depth == 0) {
                done = true;
            } else {
                path |= 1u;
                double lo0, w0, lo1, w1;
                node_box(depth, path, lo0, w0, lo1, w1);
                double own[N];
                load_cell<K0, K1>(ref, own);                   // the cell's own coefficients, read again
                restrict_box<2, K0, K1>(own, lo0, w0, lo1, w1, cur);
                live = !excluded<K0, K1>(cur);
            }
        } else if (depth == 2 * ROOTS2_DEPTH) {
            double lo0, w0, lo1, w1;
            node_box(depth, path, lo0, w0, lo1, w1);
            leaf<K0, K1>(ref, lo0, lo1, t0u, hu, t0v, hv, S0, S1, out, near, count, status);
            live = false;
        } else {
            const int child = (depth & 1) ? descend<K0, K1, 1>(cur) : descend<K0, K1, 0>(cur);
            if (child < 0) {
                live = false;
            } else {
                path = (path << 1) | (uint64_t)child;
                ++depth;
            }
        }
        node = ((uint64_t)depth << 48) | path;
    }
    if (!done) status |= STATUS_WALK;
    *count_out = count;
    *status_out = (uint8_t)status;
    *nodes_out = nodes;
}

// The tables of a launch.  rows: [nsys, 2, R0, R1]; first0: [nc0]; first1: [nc1]; breaks0: [nc0 + 1]; breaks1: [nc1 + 1].
struct Grid {
    const double *rows;
    long long nsys, R0, R1, nc0, nc1;
    const int32_t *first0, *first1;
};

// the cell of flat index `at` (system, i, j); false: not a cell, or its window leaves the rows
template <int K0, int K1>
BSK_HD bool cell_ref(const Grid &g, long long at, CellRef &ref, long long &b, long long &i, long long &j)
{
    const long long ncell = g.nc0 * g.nc1;
    if (at < 0 || at >= g.nsys * ncell) return false;
    b = at / ncell;
    const long long cell = at - b * ncell;
    i = cell / g.nc1;
    j = cell - i * g.nc1;
    const long long f0 = g.first0[i], f1 = g.first1[j];
    if (f0 < 0 || f0 + K0 > g.R0 || f1 < 0 || f1 + K1 > g.R1) return false;
    ref.sd = g.R0 * g.R1;
    ref.si = g.R1;
    ref.p = g.rows + b * 2 * ref.sd + f0 * ref.si + f1;
    return true;
}

template <int K0, int K1>
BSK_HD void flag_lane(const Grid &g, long long at, const uint8_t *mask, uint8_t *flags)
{
    CellRef ref;
    long long b, i, j;
    int f = 0;
    if (!mask[at] && cell_ref<K0, K1>(g, at, ref, b, i, j)) {
        double c[2 * K0 * K1];
        load_cell<K0, K1>(ref, c);
        f = flag_cell<K0, K1>(c, 0);
    }
    flags[at] = (uint8_t)f;
}

template <int K0, int K1>
BSK_HD void isolate_lane(const Grid &g, long long lane, const double *breaks0, const double *breaks1, const double *scale,
                         const int64_t *cand, double *roots, uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes)
{
    constexpr int R = slots(K0, K1);
    CellRef ref;
    long long b, i, j;
    double *out = roots + lane * 2 * R;
    if (!cell_ref<K0, K1>(g, cand[lane], ref, b, i, j)) {
        for (int q = 0; q < R; ++q) {
            out[2 * q] = __builtin_nan("");
            out[2 * q + 1] = __builtin_nan("");
            near[lane * R + q] = 0;
        }
        count[lane] = 0;
        status[lane] = 0;
        nodes[lane] = 0;
        return;
    }
    isolate_cell<K0, K1>(ref, breaks0[i], breaks0[i + 1], breaks1[j], breaks1[j + 1], scale[2 * b], scale[2 * b + 1], out,
                         near + lane * R, count + lane, status + lane, nodes + lane);
}

// roots: [ncand, R, 2]; cand: [ncand]; flags, table: [nsys, nc0, nc1]; which: [nnear] flat (candidate, slot); keep: [ncand, R]
BSK_HD void merge_lane(long long lane, int R, const double *roots, long long nsys, long long nc0, long long nc1,
                       const double *breaks0, const double *breaks1, const int64_t *cand, long long ncand, const uint8_t *flags,
                       const int64_t *table, const int64_t *which, uint8_t *keep)
{
    const long long at = which[lane];
    if (at < 0 || at >= ncand * R) return;
    const long long slot = at / R;
    const long long cellat = cand[slot];
    const long long ncell = nc0 * nc1;
    if (cellat < 0 || cellat >= nsys * ncell) return;
    const long long b = cellat / ncell, cell = cellat - b * ncell;
    const long long i = cell / nc1, j = cell - i * nc1;
    const double u = roots[2 * at], v = roots[2 * at + 1];
    const double tolu = ROOTS2_SAME * (breaks0[i + 1] - breaks0[i]), tolv = ROOTS2_SAME * (breaks1[j + 1] - breaks1[j]);
    uint8_t k = (u == u) ? 1 : 0;
    for (int n = 0; n < 4; ++n) {
        const long long ni = i + (n < 3 ? -1 : 0), nj = j + (n < 3 ? n - 1 : -1);
        if (ni < 0 || nj < 0 || nj >= nc1) continue;
        const long long nat = b * ncell + ni * nc1 + nj;
        if (!flags[nat]) continue;
        const long long ns = table[nat];
        if (ns < 0 || ns >= ncand) continue;
        for (int q = 0; q < R; ++q) {
            const double uu = roots[2 * (ns * R + q)], vv = roots[2 * (ns * R + q) + 1];
            if (fabs(uu - u) <= tolu && fabs(vv - v) <= tolv) k = 0;
        }
    }
    keep[at] = k;
}

// BSK_ROOTS2_FUNCTIONS_ONLY: a unit that takes the walk for cells of its own (bsk_rays.hpp) leaves the kernels to bsk_roots2_tu.hip
#if defined(__HIPCC__) && !defined(BSK_ROOTS2_FUNCTIONS_ONLY)
template <int K0, int K1>
__global__ __launch_bounds__(ROOTS2_BLOCK) void roots2_flag(Grid g, const uint8_t *__restrict__ mask, uint8_t *__restrict__ flags)
{
    const long long gid = (long long)blockIdx.x * ROOTS2_BLOCK + threadIdx.x;
    if (gid >= g.nsys * g.nc0 * g.nc1) return;
    flag_lane<K0, K1>(g, gid, mask, flags);
}

template <int K0, int K1>
__global__ __launch_bounds__(ROOTS2_ISOLATE_BLOCK) void roots2_isolate(Grid g, const double *__restrict__ breaks0,
                                                                      const double *__restrict__ breaks1,
                                                                      const double *__restrict__ scale,
                                                                      const int64_t *__restrict__ cand, long long ncand,
                                                                      double *roots, uint8_t *__restrict__ near,
                                                                      int32_t *__restrict__ count, uint8_t *__restrict__ status,
                                                                      int32_t *__restrict__ nodes)
{
    const long long gid = (long long)blockIdx.x * ROOTS2_ISOLATE_BLOCK + threadIdx.x;
    if (gid >= ncand) return;
    isolate_lane<K0, K1>(g, gid, breaks0, breaks1, scale, cand, roots, near, count, status, nodes);
}

__global__ __launch_bounds__(ROOTS2_BLOCK) void roots2_merge(int R, const double *__restrict__ roots, long long nsys, long long nc0,
                                                            long long nc1, const double *__restrict__ breaks0,
                                                            const double *__restrict__ breaks1, const int64_t *__restrict__ cand,
                                                            long long ncand, const uint8_t *__restrict__ flags,
                                                            const int64_t *__restrict__ table, const int64_t *__restrict__ which,
                                                            long long nnear, uint8_t *__restrict__ keep)
{
    const long long gid = (long long)blockIdx.x * ROOTS2_BLOCK + threadIdx.x;
    if (gid >= nnear) return;
    merge_lane(gid, R, roots, nsys, nc0, nc1, breaks0, breaks1, cand, ncand, flags, table, which, keep);
}
#endif

}  // namespace bskroots2
