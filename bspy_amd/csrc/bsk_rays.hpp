// Ray-surface hits (bspy_amd/rays.py): the bsk_rays_* family.  N lines o + t d against one surface (nInd 2, nDep 3).
//
// The caller has brought both variables to Bezier form (the band operator of bsk_refine.hpp, once per axis): rows is
// [3, R0, R1] in fp64 and cell (i, j), flat index i nc1 + j, is the K0 x K1 window of the three components at first0[i],
// first1[j].  A ray is the intersection of two planes, so a hit is a common zero of g_k(u, v) = n_k . (S(u, v) - o),
// k = 1, 2: a bskroots2 system whose cell coefficients are never stored but formed from the window and the ray's frame.
//
//   frame         c = the axis of the largest |d| (the highest index on ties), a < b the other two; n1 = e_a x d,
//                 n2 = e_b x d: one entry of each is 0 and the others are +- components of d, so g_k of a control point P is
//                 w_k0 (P_p - o_p) + w_k1 (P_q - o_q), p < q the two axes where n_k is not 0: two differences, two products,
//                 one sum, each rounded on its own.  S_k = |w_k0| (C_p + |o_p|) + |w_k1| (C_q + |o_q|), C = max |coefficient|
//                 per component, bounds |g_k| and takes the place of bskroots2's S_d.  A ray with a non-finite entry or
//                 d = 0 is skipped (status bit 8).
//   ray_boxes     lane = cell: min and max of the window per component, boxes [ncell, 6] = lo0, hi0, lo1, hi1, lo2, hi2.
//   ray_search    lane = ray with its frame in registers; grid = (ray blocks, chunks of the cells).  The boxes and the rows
//                 are read through wave-uniform addresses (kernel arguments, blockIdx, the loop counter).  A pair
//                 (ray, cell) passes the slab test unless the line on [tmin, tmax] misses the box: per axis with d != 0 the
//                 two parameters (lo - o) (1 / d), (hi - o) (1 / d) carry three roundings, below 2 eps relative, and are
//                 pushed outward by 4 eps |t| + 2^-1070; an axis with d = 0 compares o with the box exactly; a NaN or an
//                 infinity keeps the pair.  A passing pair is flat when all K0 K1 values of g_1 or of g_2 are below
//                 S_k eps (or S_k is 0), else it is a candidate unless g_1 or g_2 is strictly of one sign.  Flat pairs and candidates are
//                 counted (EMIT = false: partial[ray, chunk]) or written (EMIT = true: pair_ray, pair_cell at
//                 offset[ray, chunk] + n, cells ascending).  PREFILTER = false sends every pair to the sign test; the slab
//                 test then decides the flat rule alone.
//   ray_isolate   lane = pair, block 64: a flat pair sets status bit 16 and reports nothing; any other pair is walked by
//                 bskroots2::isolate_cell on a RayCell, which forms the coefficients wherever bskroots2 reads them again.
//   ray_reduce    lane = ray: the rule of roots2_merge among the ray's own pairs (they are sorted by cell), t of a kept root
//                 = (S_c(x) - o_c) / d_c with S_c by bskroots2::eval2 at x = ((u - t0u) / hu, (v - t0v) / hv), and the range
//                 tmin <= t <= tmax.  ALL = false: the kept hit of smallest t (ties: lowest cell, then slot), the number of
//                 hits and the OR of the status bytes; ALL = true: every hit at hit_off[ray] + n in (cell, slot) order.
//
// fp64, no contraction, one association for the host drivers and the kernels; rays.py states it in Python floats.  No
// atomics, no waiting, no LDS of its own (the compiler keeps a private array of the walk there in ray_isolate, as in roots2_isolate),
// and every loop has a compile-time or an argument bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#define BSK_ROOTS2_FUNCTIONS_ONLY
#include "bsk_pairs.hpp"
#include "bsk_roots2.hpp"

#pragma clang fp contract(off)

namespace bskroots2 {

// One cell of the surface seen from one ray: component m of the window at p[m * sd + i * si + j].
struct RayCell {
    const double *p;
    long long sd, si;
    int p1, q1, p2, q2;                        // the axes of the two terms of g_1 and of g_2
    double w10, w11, w20, w21;                 // their weights
    double o10, o11, o20, o21;                 // the origin's entries on those axes
};

BSK_HD double pick(int axis, double x, double y, double z) { return axis == 0 ? x : (axis == 1 ? y : z); }

template <int K0, int K1>
BSK_HD void load_cell(const RayCell &rc, double *c)
{
#pragma unroll
    for (int i = 0; i < K0; ++i)
#pragma unroll
        for (int j = 0; j < K1; ++j) {
            const double x = rc.p[i * rc.si + j], y = rc.p[rc.sd + i * rc.si + j], z = rc.p[2 * rc.sd + i * rc.si + j];
            const double a0 = rc.w10 * (pick(rc.p1, x, y, z) - rc.o10), a1 = rc.w11 * (pick(rc.q1, x, y, z) - rc.o11);
            const double b0 = rc.w20 * (pick(rc.p2, x, y, z) - rc.o20), b1 = rc.w21 * (pick(rc.q2, x, y, z) - rc.o21);
            c[i * K1 + j] = a0 + a1;
            c[(K0 + i) * K1 + j] = b0 + b1;
        }
}

}  // namespace bskroots2

namespace bskrays {

using bskpairs::Surface;                            // the tables of a launch (bsk_pairs.hpp); K0, K1 are template constants here
using bskpairs::window;
using bskroots2::RayCell;
using bskroots2::ROOTS2_EPS;
using bskroots2::ROOTS2_SAME;
using bskroots2::slots;

constexpr int RAYS_BLOCK = 256;                     // ray_boxes, ray_search, ray_reduce
constexpr int RAYS_ISOLATE_BLOCK = 64;              // one wave: the walk may use the whole register file
constexpr unsigned STATUS_SKIPPED = 8, STATUS_FLAT = 16;
constexpr double RAYS_TINY = 0x1p-1070;

// origins, dirs: [3, nrays]; cmax: [3]
struct Rays {
    const double *origins, *dirs, *cmax;
    long long nrays;
};

struct Frame {
    double o[3], d[3];
    int c;                                     // the dominant axis
    double S1, S2;
    bool skipped;
    int p1, q1, p2, q2;
    double w10, w11, w20, w21;
};

BSK_HD bool finite(double x) { return x - x == 0.0; }

BSK_HD Frame make_frame(const Rays &r, long long ray)
{
    Frame f;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        f.o[m] = r.origins[m * r.nrays + ray];
        f.d[m] = r.dirs[m * r.nrays + ray];
    }
    const double a0 = fabs(f.d[0]), a1 = fabs(f.d[1]), a2 = fabs(f.d[2]);
    bool ok = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) ok = ok && finite(f.o[m]) && finite(f.d[m]);
    f.skipped = !ok || (a0 == 0.0 && a1 == 0.0 && a2 == 0.0);
    f.c = (a2 >= a0 && a2 >= a1) ? 2 : (a1 >= a0 ? 1 : 0);
    const double dx = f.d[0], dy = f.d[1], dz = f.d[2];
    // e_x x d = (0, -dz, dy), e_y x d = (dz, 0, -dx), e_z x d = (-dy, dx, 0)
    if (f.c == 2) {                            // a = 0, b = 1
        f.p1 = 1, f.q1 = 2, f.w10 = -dz, f.w11 = dy;
        f.p2 = 0, f.q2 = 2, f.w20 = dz, f.w21 = -dx;
    } else if (f.c == 1) {                     // a = 0, b = 2
        f.p1 = 1, f.q1 = 2, f.w10 = -dz, f.w11 = dy;
        f.p2 = 0, f.q2 = 1, f.w20 = -dy, f.w21 = dx;
    } else {                                   // a = 1, b = 2
        f.p1 = 0, f.q1 = 2, f.w10 = dz, f.w11 = -dx;
        f.p2 = 0, f.q2 = 1, f.w20 = -dy, f.w21 = dx;
    }
    const double c0 = r.cmax[0] + fabs(f.o[0]), c1 = r.cmax[1] + fabs(f.o[1]), c2 = r.cmax[2] + fabs(f.o[2]);
    using bskroots2::pick;
    f.S1 = fabs(f.w10) * pick(f.p1, c0, c1, c2) + fabs(f.w11) * pick(f.q1, c0, c1, c2);
    f.S2 = fabs(f.w20) * pick(f.p2, c0, c1, c2) + fabs(f.w21) * pick(f.q2, c0, c1, c2);
    return f;
}

BSK_HD RayCell ray_cell(const Frame &f, const double *p, long long sd, long long si)
{
    using bskroots2::pick;
    RayCell rc;
    rc.p = p, rc.sd = sd, rc.si = si;
    rc.p1 = f.p1, rc.q1 = f.q1, rc.p2 = f.p2, rc.q2 = f.q2;
    rc.w10 = f.w10, rc.w11 = f.w11, rc.w20 = f.w20, rc.w21 = f.w21;
    rc.o10 = pick(f.p1, f.o[0], f.o[1], f.o[2]), rc.o11 = pick(f.q1, f.o[0], f.o[1], f.o[2]);
    rc.o20 = pick(f.p2, f.o[0], f.o[1], f.o[2]), rc.o21 = pick(f.q2, f.o[0], f.o[1], f.o[2]);
    return rc;
}

template <int K0, int K1>
BSK_HD void boxes_lane(const Surface &s, long long cell, double *boxes)
{
    const double *p;
    long long i, j;
    const bool ok = window(s, K0, K1, cell, p, i, j);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        double lo = __builtin_inf(), hi = -__builtin_inf();      // no window: lo > hi; search_lane drops the pair by the same window test
        if (ok) {
#pragma unroll
            for (int a = 0; a < K0; ++a)
#pragma unroll
                for (int b = 0; b < K1; ++b) {
                    const double x = p[m * s.R0 * s.R1 + a * s.R1 + b];
                    lo = x < lo ? x : lo;
                    hi = x > hi ? x : hi;
                }
        }
        boxes[6 * cell + 2 * m] = lo;
        boxes[6 * cell + 2 * m + 1] = hi;
    }
}

// false: the line on [tmin, tmax] misses the box
BSK_HD bool slab_test(const Frame &f, const double *inv, const double *box, double tmin, double tmax)
{
    double enter = tmin, leave = tmax;
    bool hit = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const double lo = box[2 * m], hi = box[2 * m + 1];
        if (f.d[m] == 0.0) {
            hit = hit && !(f.o[m] < lo || f.o[m] > hi);
        } else {
            const double ta = (lo - f.o[m]) * inv[m], tb = (hi - f.o[m]) * inv[m];
            double near = inv[m] > 0.0 ? ta : tb, far = inv[m] > 0.0 ? tb : ta;
            near = near - (4.0 * ROOTS2_EPS * fabs(near) + RAYS_TINY);
            far = far + (4.0 * ROOTS2_EPS * fabs(far) + RAYS_TINY);
            if (!(near == near)) near = -__builtin_inf();
            if (!(far == far)) far = __builtin_inf();
            enter = near > enter ? near : enter;
            leave = far < leave ? far : leave;
        }
    }
    return hit && !(enter > leave);
}

// 0: no pair; 1: a candidate; 2: a flat pair (the slab test passed and g_1 or g_2 is below S_k eps on the whole window)
template <int K0, int K1>
BSK_HD int pair_kind(const RayCell &rc, double S1, double S2, bool inbox)
{
    constexpr int N = K0 * K1;
    double c[2 * N];
    bskroots2::load_cell<K0, K1>(rc, c);
    bool small1 = true, small2 = true;
    const double e1 = S1 * ROOTS2_EPS, e2 = S2 * ROOTS2_EPS;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        small1 = small1 && fabs(c[e]) < e1;
        small2 = small2 && fabs(c[N + e]) < e2;
    }
    small1 = small1 || S1 == 0.0;                          // as roots2's zero-cell rule: a scale of 0 is a zero field
    small2 = small2 || S2 == 0.0;
    if (small1 || small2) return inbox ? 2 : 0;
    return bskroots2::excluded<K0, K1>(c) ? 0 : 1;
}

// partial: [nrays, nchunks]; skipped: [nrays]; offset: [nrays, nchunks] (exclusive sums of partial); pair_*: [npairs]
struct Search {
    double tmin, tmax;
    long long chunk, nchunks;
    const double *boxes;
    int32_t *partial;
    uint8_t *skipped;
    const int64_t *offset;
    int32_t *pair_ray, *pair_cell;
    long long npairs;
};

template <int K0, int K1, bool PREFILTER, bool EMIT>
BSK_HD void search_lane(const Surface &s, const Rays &r, const Search &a, long long ch, long long ray)
{
    const Frame f = make_frame(r, ray);
    const long long ncell = s.nc0 * s.nc1;
    const long long begin = ch * a.chunk, end = begin + a.chunk < ncell ? begin + a.chunk : ncell;
    long long n = 0;
    const long long base = EMIT ? a.offset[ray * a.nchunks + ch] : 0;
    if (!f.skipped) {
        double inv[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) inv[m] = 1.0 / f.d[m];
        for (long long cell = begin; cell < end; ++cell) {
            const bool inbox = slab_test(f, inv, a.boxes + 6 * cell, a.tmin, a.tmax);
            if (PREFILTER && !inbox) continue;
            const double *p;
            long long i, j;
            if (!window(s, K0, K1, cell, p, i, j)) continue;
            const RayCell rc = ray_cell(f, p, s.R0 * s.R1, s.R1);
            if (pair_kind<K0, K1>(rc, f.S1, f.S2, inbox) == 0) continue;
            if (EMIT && base + n >= 0 && base + n < a.npairs) {
                a.pair_ray[base + n] = (int32_t)ray;
                a.pair_cell[base + n] = (int32_t)cell;
            }
            ++n;
        }
    }
    if (!EMIT) {
        a.partial[ray * a.nchunks + ch] = (int32_t)n;
        if (ch == 0) a.skipped[ray] = f.skipped ? (uint8_t)STATUS_SKIPPED : (uint8_t)0;
    }
}

// roots: [npairs, R, 2]; near: [npairs, R]; count, status, nodes: [npairs]
struct Isolate {
    const double *breaks0, *breaks1;
    const int32_t *pair_ray, *pair_cell;
    long long npairs;
    double *roots;
    uint8_t *near;
    int32_t *count;
    uint8_t *status;
    int32_t *nodes;
};

template <int K0, int K1>
BSK_HD void isolate_lane(const Surface &s, const Rays &r, const Isolate &a, long long lane)
{
    constexpr int R = slots(K0, K1);
    double *out = a.roots + lane * 2 * R;
    const long long ray = a.pair_ray[lane];
    const double *p = nullptr;
    long long i = 0, j = 0;
    bool walk = ray >= 0 && ray < r.nrays && window(s, K0, K1, a.pair_cell[lane], p, i, j);
    unsigned status = 0;
    if (walk) {
        const Frame f = make_frame(r, ray);
        const RayCell rc = ray_cell(f, p, s.R0 * s.R1, s.R1);
        if (f.skipped) walk = false;
        else if (pair_kind<K0, K1>(rc, f.S1, f.S2, true) == 2) {
            walk = false;
            status = STATUS_FLAT;
        } else {
            bskroots2::isolate_cell<K0, K1>(rc, a.breaks0[i], a.breaks0[i + 1], a.breaks1[j], a.breaks1[j + 1], f.S1, f.S2, out,
                                            a.near + lane * R, a.count + lane, a.status + lane, a.nodes + lane);
        }
    }
    if (!walk) {
        for (int q = 0; q < R; ++q) {
            out[2 * q] = __builtin_nan("");
            out[2 * q + 1] = __builtin_nan("");
            a.near[lane * R + q] = 0;
        }
        a.count[lane] = 0;
        a.status[lane] = (uint8_t)status;
        a.nodes[lane] = 0;
    }
}

// pstart: [nrays + 1], the pairs of a ray; hit_off: [nrays + 1] (ALL).  ALL = false: uv [2, nrays], t, cell, hits, status
// [nrays]; ALL = true: uv [nhits, 2], t, cell [nhits].
struct Reduce {
    const double *breaks0, *breaks1;
    double tmin, tmax;
    const int64_t *pstart;
    const int32_t *pair_cell;
    long long npairs;
    const double *roots;
    const uint8_t *near;
    const int32_t *count;
    const uint8_t *pstatus, *skipped;
    const int64_t *hit_off;
    long long nhits;
    double *uv, *t;
    int32_t *cell, *hits;
    uint8_t *status;
};

template <int K0, int K1, bool ALL>
BSK_HD void reduce_lane(const Surface &s, const Rays &r, const Reduce &a, long long ray)
{
    constexpr int R = slots(K0, K1);
    const Frame f = make_frame(r, ray);
    long long p0 = a.pstart[ray], p1 = a.pstart[ray + 1];
    if (p0 < 0 || p1 > a.npairs || p1 < p0) p0 = p1 = 0;
    const double oc = bskroots2::pick(f.c, f.o[0], f.o[1], f.o[2]), dc = bskroots2::pick(f.c, f.d[0], f.d[1], f.d[2]);
    double bu = __builtin_nan(""), bv = __builtin_nan(""), bt = __builtin_nan("");
    int32_t bcell = -1, n = 0;
    unsigned status = a.skipped[ray];
    const long long hbase = ALL ? a.hit_off[ray] : 0;
    for (long long p = p0; p < p1; ++p) {
        status |= a.pstatus[p];
        const double *w;
        long long i, j;
        const long long cell = a.pair_cell[p];
        if (!window(s, K0, K1, cell, w, i, j)) continue;
        const double t0u = a.breaks0[i], t0v = a.breaks1[j];
        const double hu = a.breaks0[i + 1] - t0u, hv = a.breaks1[j + 1] - t0v;
        const double tolu = ROOTS2_SAME * hu, tolv = ROOTS2_SAME * hv;
        for (int q = 0; q < R; ++q) {
            if (q >= a.count[p]) continue;
            const double u = a.roots[2 * (p * R + q)], v = a.roots[2 * (p * R + q) + 1];
            bool keep = u == u;
            if (a.near[p * R + q]) {
                for (long long pp = p0; pp < p; ++pp) {
                    const long long other = a.pair_cell[pp];
                    const long long oi = other / s.nc1, oj = other - oi * s.nc1;
                    const bool nb = (oi == i - 1 && (oj == j - 1 || oj == j || oj == j + 1)) || (oi == i && oj == j - 1);
                    if (!nb) continue;
                    for (int k = 0; k < R; ++k) {
                        const double uu = a.roots[2 * (pp * R + k)], vv = a.roots[2 * (pp * R + k) + 1];
                        if (fabs(uu - u) <= tolu && fabs(vv - v) <= tolv) keep = false;
                    }
                }
            }
            if (!keep) continue;
            double c[K0 * K1];
#pragma unroll
            for (int e0 = 0; e0 < K0; ++e0)
#pragma unroll
                for (int e1 = 0; e1 < K1; ++e1) c[e0 * K1 + e1] = w[f.c * s.R0 * s.R1 + e0 * s.R1 + e1];
            double val, du, dv;
            bskroots2::eval2<K0, K1>(c, (u - t0u) / hu, (v - t0v) / hv, val, du, dv);
            const double t = (val - oc) / dc;
            if (!(t >= a.tmin && t <= a.tmax)) continue;
            if (ALL) {
                const long long at = hbase + n;
                if (at >= 0 && at < a.nhits) {
                    a.uv[2 * at] = u;
                    a.uv[2 * at + 1] = v;
                    a.t[at] = t;
                    a.cell[at] = (int32_t)cell;
                }
            } else if (n == 0 || t < bt) {
                bu = u, bv = v, bt = t, bcell = (int32_t)cell;
            }
            ++n;
        }
    }
    if (!ALL) {
        a.uv[ray] = bu;
        a.uv[r.nrays + ray] = bv;
        a.t[ray] = bt;
        a.cell[ray] = bcell;
        a.hits[ray] = n;
        a.status[ray] = (uint8_t)status;
    }
}

#ifdef __HIPCC__
template <int K0, int K1>
__global__ __launch_bounds__(RAYS_BLOCK) void ray_boxes(Surface s, double *__restrict__ boxes)
{
    const long long gid = (long long)blockIdx.x * RAYS_BLOCK + threadIdx.x;
    if (gid >= s.nc0 * s.nc1) return;
    boxes_lane<K0, K1>(s, gid, boxes);
}

template <int K0, int K1, bool PREFILTER, bool EMIT>
__global__ __launch_bounds__(RAYS_BLOCK) void ray_search(Surface s, Rays r, Search a)
{
    const long long gid = (long long)blockIdx.x * RAYS_BLOCK + threadIdx.x;
    if (gid >= r.nrays) return;
    search_lane<K0, K1, PREFILTER, EMIT>(s, r, a, (long long)blockIdx.y, gid);
}

template <int K0, int K1>
__global__ __launch_bounds__(RAYS_ISOLATE_BLOCK) void ray_isolate(Surface s, Rays r, Isolate a)
{
    const long long gid = (long long)blockIdx.x * RAYS_ISOLATE_BLOCK + threadIdx.x;
    if (gid >= a.npairs) return;
    isolate_lane<K0, K1>(s, r, a, gid);
}

template <int K0, int K1, bool ALL>
__global__ __launch_bounds__(RAYS_BLOCK) void ray_reduce(Surface s, Rays r, Reduce a)
{
    const long long gid = (long long)blockIdx.x * RAYS_BLOCK + threadIdx.x;
    if (gid >= r.nrays) return;
    reduce_lane<K0, K1, ALL>(s, r, a, gid);
}
#endif

}  // namespace bskrays
