// Scattered least squares (bspy_amd/scatter.py): the bsk_scatter_* family.  The normal equations of
//     sum_i w_i |S(u_i) - p_i|^2  over N scattered points (u_i, p_i)
// are formed without atomics: a key per point, a stable sort by key (the caller's), a Gram slab per unit of at most
// SCATTER_SEG points of one knot cell, a pairwise tree over the units of a cell, and a gather into the stencil.
//
// A curve is a surface with K1 = n1 = 1 and knots1 = {0, 1}.  Knot cell (c0, c1), c_d in 0 .. n_d - K_d, is the span
// mu_d = c_d + K_d - 1 of variable d; its K = K0 K1 basis functions are the coefficients (c0 + a0, c1 + a1), local flat
// index a = a0 K1 + a1.  Flat cell index c0 nc1 + c1, nc_d = n_d - K_d + 1; cells of zero width exist and stay empty.
//
//   scatter_key       lane = one point.  Excluded (key -1, a status bit): a parameter outside the domain (1), a parameter,
//                     coordinate or weight that is NaN or infinite (2), a negative weight (4).  Otherwise per variable the
//                     last span in K - 1 .. top whose left knot is <= u, by a bisection with a launch-uniform trip count;
//                     top is the last span of positive width, so the right domain end belongs to it.
//   scatter_gram      one wave per unit.  The unit's points come in batches of 64, one point per lane: the lane forms
//                     Bu, Bv by the Cox-de Boor recursion (basis<K>) and writes B_a = Bu_a0 Bv_a1, w and p to LDS.  Then
//                     lane (a, q) = a Q + q, Q = strands(K), adds the points j = q (mod Q) of the batch, in increasing j,
//                     to row a of its strand's slab: t = w B_a, G_ab = G_ab + t B_b, r_ad = r_ad + t p_d, K + ndep
//                     accumulators from 0.  The Q strands are combined by an adjacent-pairs tree (a butterfly of lane
//                     exchanges: IEEE addition commutes, every lane of a row ends with the same bits) and lane (a, 0)
//                     stores row a: slab [K][K + ndep] per unit.
//   scatter_cell      lane = (node, entry): one level of the adjacent-pairs tree over the units of a cell, SCATTER_FAN
//                     inputs to a node (pair_tree: pairs (0, 1), (2, 3), ..., an odd last one is carried up).  Aligned
//                     blocks of 2^m leaves are subtrees of that tree, so the levels compose to the tree over all units.
//                     A cell without units gives zeros.
//   scatter_fold      lane = one destination entry of the stencil [n][2 K0 - 1][2 K1 - 1] or of the right-hand side
//                     [n][ndep]: the sum, from 0 and in increasing flat cell index, over the cells that hold both basis
//                     functions.  Entry (i, j) reads slab entry (a, b) of the cell with a <= b (the other triangle is
//                     stored and not read), so the stencil is symmetric bit for bit.
//   scatter_residual  lane = one point: |S(u) - p| with S_d = sum_a B_a c_d, a increasing, NaN for an excluded point.
//
// fp64, no contraction, every product and sum rounded on its own: one association for the host drivers and the
// kernels; scatter.py states it in Python.  No atomics, no waiting, every loop has a launch-uniform or data-size bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsk_roots.hpp"

#pragma clang fp contract(off)

namespace bskscatter {

constexpr int SCATTER_SEG = 256;                    // points per unit: a constant of the statement, not a launch shape
constexpr int SCATTER_FAN = 16;                     // inputs per node and level of scatter_cell: a power of two
constexpr int SCATTER_BLOCK = 256;                  // scatter_key, scatter_cell, scatter_fold, scatter_residual
constexpr int SCATTER_WAVE = 64;                    // scatter_gram: one wave per unit
constexpr int SCATTER_MAX_K = 6;                    // per variable, host drivers; the kernels cover 2 .. SCATTER_DEVICE_MAX_K
constexpr int SCATTER_DEVICE_MAX_K = 4;
constexpr int SCATTER_DEVICE_MAX_NDEP = 4;
constexpr unsigned STATUS_OUTSIDE = 1, STATUS_NONFINITE = 2, STATUS_WEIGHT = 4;

// strands of a unit: the largest power of two with Q K <= 64, at least 1
constexpr int strands(int K)
{
    int q = 1;
    while (2 * q * K <= 64) q *= 2;
    return q;
}

BSK_HD bool is_finite(double x) { return fabs(x) < __builtin_inf(); }

// One variable: n + K knots, spans K - 1 .. top are searched, trips = bit length of top - (K - 1).
struct Axis {
    const double *knots;
    long long n, top;
    int trips;
};

// The grid of a call: a curve has K1 = 1, ax1 = {{0, 1}, 1, 0, 0}.
struct Grid {
    Axis ax0, ax1;
    long long nc1;          // cells of variable 1
};

BSK_HD int bisection_trips(long long width)
{
    int trips = 0;
    for (long long n = width; n > 0; n >>= 1) ++trips;
    return trips;
}

// the last span in lo .. top whose left knot is <= u (lo for a u below it)
BSK_HD long long find_span(const Axis &ax, long long lo, double u)
{
    long long hi = ax.top;
    for (int t = 0; t < ax.trips; ++t) {
        const long long mid = (lo + hi + 1) >> 1;
        if (ax.knots[mid] <= u) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The K basis functions of order K that live on span mu at u, by the Cox-de Boor recursion on the 2 K local knots
// local[l] = knots[mu - K + 1 + l]: b[r] multiplies coefficient mu - K + 1 + r.
template <int K>
BSK_HD void basis(const double *knots, long long mu, double u, double *b)
{
    double local[2 * K];
#pragma unroll
    for (int l = 0; l < 2 * K; ++l) local[l] = knots[mu - K + 1 + l];
    b[0] = 1.0;
#pragma unroll
    for (int j = 1; j < K; ++j) {
        double saved = 0.0;
#pragma unroll
        for (int r = 0; r < j; ++r) {
            const double tr = local[K + r], tl = local[K + r - j];
            const double temp = b[r] / (tr - tl);
            b[r] = saved + (tr - u) * temp;
            saved = (u - tl) * temp;
        }
        b[j] = saved;
    }
}

// ------------------------------------------------------------------------------------------ key
// uvw: [nind, npts]; points: [ndep, npts]; weights: [npts] or NULL
BSK_HD void key_lane(int nind, int K0, int K1, const Grid &g, int ndep, const double *uvw, const double *points,
                     const double *weights, long long npts, long long lane, int64_t *key, uint8_t *status)
{
    unsigned st = 0;
    const double u0 = uvw[lane], u1 = nind == 2 ? uvw[npts + lane] : 0.0;
    bool finite = is_finite(u0) && is_finite(u1);
    for (int d = 0; d < ndep; ++d) finite = finite && is_finite(points[d * npts + lane]);
    if (weights) {
        const double w = weights[lane];
        finite = finite && is_finite(w);
        if (w < 0.0) st |= STATUS_WEIGHT;
    }
    if (!finite) st |= STATUS_NONFINITE;
    if (u0 < g.ax0.knots[K0 - 1] || u0 > g.ax0.knots[g.ax0.n]) st |= STATUS_OUTSIDE;
    if (nind == 2 && (u1 < g.ax1.knots[K1 - 1] || u1 > g.ax1.knots[g.ax1.n])) st |= STATUS_OUTSIDE;
    long long k = -1;
    if (!st) {
        const long long c0 = find_span(g.ax0, K0 - 1, u0) - (K0 - 1);
        const long long c1 = nind == 2 ? find_span(g.ax1, K1 - 1, u1) - (K1 - 1) : 0;
        k = c0 * g.nc1 + c1;
    }
    key[lane] = k;
    status[lane] = (uint8_t)st;
}

// ------------------------------------------------------------------------------------------ gram
// The point tables of a call and the units: order [npts] (the stable sort by key), offsets [ncells + 1] (where the cells
// start in the sorted order), unit_cell [nunits], unit_start [ncells] (the first unit of a cell).
struct Units {
    const double *uvw, *points, *weights;
    long long npts;
    const int64_t *order, *offsets, *unit_cell, *unit_start;
};

// B_a, w and p of point j in the cell (c0, c1): row[0 .. K), row[K], row[K + 1 .. K + 1 + NDEP)
template <int K0, int K1>
BSK_HD void point_row(const Grid &g, const Units &U, int ndep, long long c0, long long c1, long long j, double *row)
{
    double bu[K0], bv[K1];
    basis<K0>(g.ax0.knots, c0 + K0 - 1, U.uvw[j], bu);
    if constexpr (K1 > 1) basis<K1>(g.ax1.knots, c1 + K1 - 1, U.uvw[U.npts + j], bv);
    else bv[0] = 1.0;
#pragma unroll
    for (int a0 = 0; a0 < K0; ++a0)
#pragma unroll
        for (int a1 = 0; a1 < K1; ++a1) row[a0 * K1 + a1] = K1 > 1 ? bu[a0] * bv[a1] : bu[a0];
    row[K0 * K1] = U.weights ? U.weights[j] : 1.0;
    for (int d = 0; d < ndep; ++d) row[K0 * K1 + 1 + d] = U.points[d * U.npts + j];
}

// pairs (0, 1), (2, 3), ... of the cnt <= N live entries of x, an odd last one carried up, level by level; N a power of two
template <int N>
BSK_HD double pair_tree(double *x, int cnt)
{
#pragma unroll
    for (int width = N; width > 1; width >>= 1) {
#pragma unroll
        for (int i = 0; i < width / 2; ++i) x[i] = 2 * i + 1 < cnt ? x[2 * i] + x[2 * i + 1] : x[2 * i];
        cnt = (cnt + 1) >> 1;
    }
    return x[0];
}

// the same for any count, in place (host)
inline double pair_tree_any(double *x, long long cnt)
{
    if (cnt < 1) return 0.0;
    while (cnt > 1) {
        for (long long i = 0; 2 * i < cnt; ++i) x[i] = 2 * i + 1 < cnt ? x[2 * i] + x[2 * i + 1] : x[2 * i];
        cnt = (cnt + 1) >> 1;
    }
    return x[0];
}

// the begin and end of a unit in the sorted order
BSK_HD void unit_range(const Units &U, long long unit, long long &cell, long long &begin, long long &end)
{
    cell = U.unit_cell[unit];
    const long long stop = U.offsets[cell + 1];
    begin = U.offsets[cell] + (unit - U.unit_start[cell]) * SCATTER_SEG;
    end = begin + SCATTER_SEG < stop ? begin + SCATTER_SEG : stop;
}

// The host driver of scatter_gram: the strands' slabs one after the other, then the tree.  slabs: [nunits][K][K + ndep].
template <int K0, int K1>
__attribute__((noinline)) void gram_host(const Grid &g, const Units &U, int ndep, long long nunits, double *slabs, double *work)
{
    constexpr int K = K0 * K1, Q = strands(K);
    const int W = K + ndep;
    double *row = work;                  // K + 1 + ndep
    double *acc = work + K + 1 + ndep;   // [Q][K][W]
    double *leaf = acc + (long long)Q * K * W;   // Q
    for (long long unit = 0; unit < nunits; ++unit) {
        long long cell, begin, end;
        unit_range(U, unit, cell, begin, end);
        const long long c0 = cell / g.nc1, c1 = cell - c0 * g.nc1;
        for (long long e = 0; e < (long long)Q * K * W; ++e) acc[e] = 0.0;
        for (long long at = begin; at < end; ++at) {
            const int q = (int)((at - begin) % Q);
            point_row<K0, K1>(g, U, ndep, c0, c1, U.order[at], row);
            for (int a = 0; a < K; ++a) {
                const double t = row[K] * row[a];
                double *mine = acc + ((long long)q * K + a) * W;
                for (int b = 0; b < K; ++b) mine[b] = mine[b] + t * row[b];
                for (int d = 0; d < ndep; ++d) mine[K + d] = mine[K + d] + t * row[K + 1 + d];
            }
        }
        for (int e = 0; e < K * W; ++e) {
            for (int q = 0; q < Q; ++q) leaf[q] = acc[(long long)q * K * W + e];
            slabs[unit * K * W + e] = pair_tree_any(leaf, Q);
        }
    }
}

// ------------------------------------------------------------------------------------------ cell
// One level: node `node` of the output sums at most SCATTER_FAN nodes of its cell in the input.  in: [*][entries];
// in_start, in_count, out_start: [ncells]; node_cell: [nnodes]; out: [nnodes][entries].
struct Level {
    long long entries;
    const double *in;
    const int64_t *in_start, *in_count, *node_cell, *out_start;
    long long nnodes;
    double *out;
};

BSK_HD void cell_lane(const Level &L, long long lane)
{
    const long long node = lane / L.entries, e = lane - node * L.entries;
    const long long cell = L.node_cell[node];
    const long long k = node - L.out_start[cell];
    const long long first = L.in_start[cell] + k * SCATTER_FAN;
    long long cnt = L.in_count[cell] - k * SCATTER_FAN;
    cnt = cnt < 0 ? 0 : (cnt > SCATTER_FAN ? SCATTER_FAN : cnt);
    double x[SCATTER_FAN];
#pragma unroll
    for (int i = 0; i < SCATTER_FAN; ++i) x[i] = i < cnt ? L.in[(first + i) * L.entries + e] : 0.0;
    L.out[lane] = pair_tree<SCATTER_FAN>(x, (int)cnt);
}

// ------------------------------------------------------------------------------------------ fold
// cells: [nc0 nc1][K][K + ndep]; stencil: [n0 n1][2 K0 - 1][2 K1 - 1]; rhs: [n0 n1][ndep]
struct Fold {
    int K0, K1, ndep;
    long long n0, n1;
    const double *cells;
    double *stencil, *rhs;
};

BSK_HD void fold_lane(const Fold &F, long long lane)
{
    const int K0 = F.K0, K1 = F.K1, K = K0 * K1, W = K + F.ndep, S1 = 2 * K1 - 1, NS = (2 * K0 - 1) * S1;
    const long long nc0 = F.n0 - K0 + 1, nc1 = F.n1 - K1 + 1;
    const long long i = lane / (NS + F.ndep);
    const int e = (int)(lane - i * (NS + F.ndep));
    const long long i0 = i / F.n1, i1 = i - i0 * F.n1;
    long long j0 = i0, j1 = i1;
    if (e < NS) {
        j0 = i0 + e / S1 - (K0 - 1);
        j1 = i1 + e % S1 - (K1 - 1);
    }
    double acc = 0.0;
    if (j0 >= 0 && j0 < F.n0 && j1 >= 0 && j1 < F.n1) {
        const long long top0 = i0 < j0 ? i0 : j0, top1 = i1 < j1 ? i1 : j1;
        const long long low0 = (i0 > j0 ? i0 : j0) - (K0 - 1), low1 = (i1 > j1 ? i1 : j1) - (K1 - 1);
        for (long long c0 = low0 < 0 ? 0 : low0; c0 <= top0 && c0 < nc0; ++c0)
            for (long long c1 = low1 < 0 ? 0 : low1; c1 <= top1 && c1 < nc1; ++c1) {
                const int a = (int)((i0 - c0) * K1 + (i1 - c1)), b = (int)((j0 - c0) * K1 + (j1 - c1));
                const double *slab = F.cells + (c0 * nc1 + c1) * K * W;
                const int col = e < NS ? (a < b ? b : a) : K + (e - NS);
                acc = acc + slab[(e < NS && b < a ? b : a) * W + col];
            }
    }
    if (e < NS) F.stencil[i * NS + e] = acc;
    else F.rhs[i * F.ndep + (e - NS)] = acc;
}

// ------------------------------------------------------------------------------------------ residual
// coefs: [ndep][n0][n1]; key: [npts] as scatter_key wrote it; residual: [npts]
template <int K0, int K1>
BSK_HD void residual_lane(const Grid &g, int ndep, const double *coefs, const double *uvw, const double *points,
                          const int64_t *key, long long npts, long long lane, double *residual)
{
    const long long cell = key[lane];
    const long long ncells = (g.ax0.n - K0 + 1) * g.nc1;
    if (cell < 0 || cell >= ncells) {
        residual[lane] = __builtin_nan("");
        return;
    }
    const long long c0 = cell / g.nc1, c1 = cell - c0 * g.nc1, n1 = g.ax1.n;
    double bu[K0], bv[K1];
    basis<K0>(g.ax0.knots, c0 + K0 - 1, uvw[lane], bu);
    if constexpr (K1 > 1) basis<K1>(g.ax1.knots, c1 + K1 - 1, uvw[npts + lane], bv);
    else bv[0] = 1.0;
    double d2 = 0.0;
    for (int d = 0; d < ndep; ++d) {
        const double *c = coefs + (d * g.ax0.n + c0) * n1 + c1;
        double s = 0.0;
#pragma unroll
        for (int a0 = 0; a0 < K0; ++a0)
#pragma unroll
            for (int a1 = 0; a1 < K1; ++a1) s = s + (K1 > 1 ? bu[a0] * bv[a1] : bu[a0]) * c[a0 * n1 + a1];
        const double r = s - points[d * npts + lane];
        d2 = d2 + r * r;
    }
    residual[lane] = sqrt(d2);
}

// ------------------------------------------------------------------------------------------ reweight
// The robust weight of one point: residual r >= 0, the caller's weight w0, the threshold s = c sigma > 0.  Huber (loss 0)
// and Tukey (loss 1); an excluded point (key < 0) keeps w0.  Every operation rounded on its own.
BSK_HD double reweight_value(int loss, double r, double w0, long long key, double s)
{
    if (key < 0) return w0;
    if (loss == 0) return r <= s ? w0 : w0 * (s / r);
    if (r < s) {
        const double t = r / s;
        const double q = 1.0 - t * t;
        return w0 * (q * q);
    }
    return 0.0;
}

BSK_HD void reweight_lane(int loss, double s, const double *residual, const double *weights, const int64_t *key, long long lane,
                          double *out)
{
    out[lane] = reweight_value(loss, residual[lane], weights ? weights[lane] : 1.0, key[lane], s);
}

// ------------------------------------------------------------------------------------------ solve
// The device twin of bsk_scatter_solve_host: U^T D U = N in band storage, the host's operations on the host's operands
// in the host's order, reached from the right.  Once row k is final (v_kj = D_k U_kj), every entry (i, j), k < i <= j <=
// k + hb, subtracts U_ki v_kj; an entry takes its updates in increasing k, the product rounded, then the difference, so
// it ends with the host's bits (the host's column j sums the same products over k = low .. i - 1, low = max(0, j - hb)).
// Rows outside low .. are never touched: a product with a stored zero inside the band is formed, one outside is not.
//
// Storage is by rows: entry (i, i + d), d in 0 .. hb, at [i ld + d], ld = hb + 1.  Two arrays of n ld doubles: A holds
// the running entries and, behind the sweep, v; Ub holds U and D on d = 0.  z: [ndep][n].
//
//   scatter_band      lane = one stored entry: the stencil's entry of (i, i + d) or 0.0, by the host loop's index rule.
//   scatter_panel     SOLVE_NB rows k0 .. : wave 0 of every workgroup factors the panel's diagonal triangle in registers,
//                     lane = column, one row after the other, the finished row handed round by lane exchanges; the
//                     triangle's U and D go to LDS.  Then lane = one column k0 + NB .. k0 + NB - 1 + hb: the column's
//                     NB entries in registers take the panel's rows in increasing k.  Workgroup 0 stores the triangle.
//   scatter_trail     lane = one entry of the window behind the panel, rows and columns k0 + NB .. k0 + NB - 1 + hb:
//                     the panel's NB rows in increasing k.
//   scatter_forward   one workgroup per right-hand side, panel by panel: U^T z = b as a column sweep (z_k final: every
//                     later row subtracts U_kj z_k), wave 0 the triangle, lane = one row of the window; then z / D.
//   scatter_backward  one wave per right-hand side: row i sums k = i + 1 .. top in increasing k, a serial chain (its
//                     first term finished last, so no two rows overlap); the lanes form 64 products at a time and put
//                     them in LDS, every lane runs the chain on them.  x lives in an LDS ring of SOLVE_RING doubles.
constexpr int SOLVE_NB = 32;                        // rows of a panel: a launch shape, no bit depends on it
constexpr int SOLVE_BLOCK = 256;                    // scatter_band, scatter_panel, scatter_trail, scatter_forward
constexpr int SOLVE_RING = 4096;                    // scatter_backward's window of x: half bandwidths up to SOLVE_RING - 1

struct Band {
    int K0, K1;
    long long n1, n, hb, ld;
};

// entry (i, i + d) of the normal matrix in the stencil [n][2 K0 - 1][2 K1 - 1], 0.0 where the stencil has none
BSK_HD double band_entry(const Band &B, const double *stencil, long long i, long long d)
{
    const long long j = i + d;
    if (j >= B.n) return 0.0;
    const long long i0 = i / B.n1, i1 = i - i0 * B.n1, j0 = j / B.n1, j1 = j - j0 * B.n1;
    const long long d0 = j0 - i0, d1 = j1 - i1;
    if (d0 >= B.K0 || d1 <= -B.K1 || d1 >= B.K1) return 0.0;
    const int S1 = 2 * B.K1 - 1;
    return stencil[i * ((2 * B.K0 - 1) * S1) + (d0 + B.K0 - 1) * S1 + d1 + B.K1 - 1];
}

// ------------------------------------------------------------------------------------------ kernels
#ifdef __HIPCC__
__global__ __launch_bounds__(SCATTER_BLOCK) void scatter_reweight(int loss, double s, const double *__restrict__ residual,
                                                                 const double *__restrict__ weights, const int64_t *__restrict__ key,
                                                                 long long npts, double *__restrict__ out)
{
    const long long gid = (long long)blockIdx.x * SCATTER_BLOCK + threadIdx.x;
    if (gid >= npts) return;
    reweight_lane(loss, s, residual, weights, key, gid, out);
}

__global__ __launch_bounds__(SOLVE_BLOCK) void scatter_band(Band B, const double *__restrict__ stencil, double *__restrict__ A,
                                                           int64_t *__restrict__ bad_row)
{
    const long long gid = (long long)blockIdx.x * SOLVE_BLOCK + threadIdx.x;
    if (gid == 0) *bad_row = -1;
    if (gid >= B.n * B.ld) return;
    const long long i = gid / B.ld;
    A[gid] = band_entry(B, stencil, i, gid - i * B.ld);
}

__global__ __launch_bounds__(SOLVE_BLOCK) void scatter_panel(Band B, long long k0, double *A, double *__restrict__ Ub, int64_t *bad_row)
{
    constexpr int NB = SOLVE_NB;
    __shared__ double tri[NB][NB + 1];              // tri[r][i] = U of (k0 + r, k0 + i), r < i; tri[r][r] = D
    const int tid = threadIdx.x;
    const long long n = B.n, hb = B.hb, ld = B.ld;
    if (tid < 64) {
        const int t = tid;                          // column k0 + t of the triangle
        const bool col = t < NB && k0 + t < n;
        double a[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) a[i] = col && i <= t && t - i <= hb ? A[(k0 + i) * ld + (t - i)] : 1.0;
        long long bad = -1;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const double D = __shfl(a[r], r, 64);   // lane r holds the pivot of row k0 + r
            if (k0 + r < n && bad < 0 && !(D > 0.0)) bad = k0 + r;
            const bool live = col && t > r && t - r <= hb;
            const double u = a[r] / D;
            if (col && t >= r && t - r <= hb) {
                const double keep = t == r ? D : u;
                tri[r][t] = keep;
                if (blockIdx.x == 0) Ub[(k0 + r) * ld + (t - r)] = keep;
            }
#pragma unroll
            for (int i = r + 1; i < NB; ++i) {
                const double ui = __shfl(u, i, 64);
                if (live && i <= t) a[i] = a[i] - ui * a[r];
            }
        }
        if (blockIdx.x == 0 && t == 0 && bad >= 0 && *bad_row < 0) *bad_row = bad;
    }
    __syncthreads();
    const long long c = NB + (long long)blockIdx.x * SOLVE_BLOCK + tid, j = k0 + c;
    if (c >= hb + NB || j >= n) return;
    double a[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) a[i] = c - i <= hb ? A[(k0 + i) * ld + (c - i)] : 0.0;
#pragma unroll
    for (int r = 0; r < NB; ++r)
        if (c - r <= hb) {
#pragma unroll
            for (int i = r + 1; i < NB; ++i) a[i] = a[i] - tri[r][i] * a[r];
        }
#pragma unroll
    for (int r = 0; r < NB; ++r)
        if (c - r <= hb) {
            A[(k0 + r) * ld + (c - r)] = a[r];
            Ub[(k0 + r) * ld + (c - r)] = a[r] / tri[r][r];
        }
}

__global__ __launch_bounds__(SOLVE_BLOCK) void scatter_trail(Band B, long long k0, double *A, const double *__restrict__ Ub)
{
    constexpr int NB = SOLVE_NB;
    const long long n = B.n, hb = B.hb, ld = B.ld;
    const long long i = k0 + NB + blockIdx.y, d = (long long)blockIdx.x * SOLVE_BLOCK + threadIdx.x, j = i + d;
    const long long top = k0 + NB - 1 + hb < n - 1 ? k0 + NB - 1 + hb : n - 1;
    if (i > top || j > top) return;
    double acc = A[i * ld + d];
#pragma unroll 8
    for (int r = 0; r < NB; ++r) {
        const long long k = k0 + r;
        if (j - k <= hb) acc = acc - Ub[k * ld + (i - k)] * A[k * ld + (j - k)];
    }
    A[i * ld + d] = acc;
}

__global__ __launch_bounds__(SOLVE_BLOCK) void scatter_forward(Band B, int ndep, const double *__restrict__ Ub,
                                                              const double *__restrict__ rhs, double *z)
{
    constexpr int NB = SOLVE_NB;
    __shared__ double zs[NB];
    const int tid = threadIdx.x;
    const long long n = B.n, hb = B.hb, ld = B.ld;
    const int dep = blockIdx.x;
    double *zd = z + dep * n;
    for (long long j = tid; j < n; j += SOLVE_BLOCK) zd[j] = rhs[j * ndep + dep];
    __syncthreads();
    for (long long k0 = 0; k0 < n; k0 += NB) {
        if (tid < 64) {
            const int t = tid;
            const bool col = t < NB && k0 + t < n;
            double zt = col ? zd[k0 + t] : 0.0;
            double u[NB];
#pragma unroll
            for (int r = 0; r < NB; ++r) u[r] = col && r < t && t - r <= hb ? Ub[(k0 + r) * ld + (t - r)] : 0.0;
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                const double zr = __shfl(zt, r, 64);
                if (col && r < t && t - r <= hb) zt = zt - u[r] * zr;
            }
            if (col) {
                zs[t] = zt;
                zd[k0 + t] = zt;
            }
        }
        __syncthreads();
        const long long top = k0 + NB - 1 + hb < n - 1 ? k0 + NB - 1 + hb : n - 1;
        for (long long j = k0 + NB + tid; j <= top; j += SOLVE_BLOCK) {
            double acc = zd[j];
#pragma unroll 8
            for (int r = 0; r < NB; ++r) {
                const long long k = k0 + r;
                if (j - k <= hb) acc = acc - Ub[k * ld + (j - k)] * zs[r];
            }
            zd[j] = acc;
        }
        __syncthreads();
    }
    for (long long j = tid; j < n; j += SOLVE_BLOCK) zd[j] = zd[j] / Ub[j * ld];
}

__global__ __launch_bounds__(SCATTER_WAVE) __attribute__((amdgpu_waves_per_eu(1, 1))) void scatter_backward(Band B, const double *__restrict__ Ub, const double *__restrict__ z,
                                                                double *__restrict__ coefs)
{
    __shared__ double ring[SOLVE_RING], prod[SCATTER_WAVE];
    const int lane = threadIdx.x;
    const long long n = B.n, hb = B.hb, ld = B.ld;
    const double *y = z + blockIdx.x * n;
    double *x = coefs + blockIdx.x * n;
    // U of row ii at the offsets base .. base + 63, one per lane: loaded one step ahead of its use
    auto load = [&](long long ii, long long base) {
        const long long kk = base + lane, mm = hb < n - 1 - ii ? hb : n - 1 - ii;
        return ii >= 0 && kk <= mm ? Ub[ii * ld + kk] : 0.0;
    };
    double unext = load(n - 1, 1), ynext = y[n - 1];
    for (long long i = n - 1; i >= 0; --i) {
        const long long m = hb < n - 1 - i ? hb : n - 1 - i;      // the terms k = i + 1 .. i + m
        double sum = ynext;
        if (i > 0) ynext = y[i - 1];
        long long base = 1;
        do {
            const double u = unext;
            unext = base + 64 <= m ? load(i, base + 64) : load(i - 1, 1);
            const long long kk = base + lane;
            const double p = kk <= m ? u * ring[(i + kk) & (SOLVE_RING - 1)] : 0.0;
            const long long cnt = m - base + 1;
            __builtin_amdgcn_wave_barrier();        // one wave: its LDS accesses complete in program order
            prod[lane] = p;
            __builtin_amdgcn_wave_barrier();
            if (cnt >= 64) {
                double q[SCATTER_WAVE];                // all 64 reads in flight, then the chain
#pragma unroll
                for (int l = 0; l < 64; ++l) q[l] = prod[l];
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int l = 0; l < 64; ++l) sum = sum - q[l];
            } else {
                for (int l = 0; l < (int)cnt; ++l) sum = sum - prod[l];
            }
            base += 64;
        } while (base <= m);
        __builtin_amdgcn_wave_barrier();
        ring[i & (SOLVE_RING - 1)] = sum;           // every lane writes the same value
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) x[i] = sum;
    }
}

__global__ __launch_bounds__(SCATTER_BLOCK) void scatter_key(int nind, int K0, int K1, Grid g, int ndep,
                                                            const double *__restrict__ uvw, const double *__restrict__ points,
                                                            const double *__restrict__ weights, long long npts,
                                                            int64_t *__restrict__ key, uint8_t *__restrict__ status)
{
    const long long gid = (long long)blockIdx.x * SCATTER_BLOCK + threadIdx.x;
    if (gid >= npts) return;
    key_lane(nind, K0, K1, g, ndep, uvw, points, weights, npts, gid, key, status);
}

template <int K0, int K1, int NDEP>
__global__ __launch_bounds__(SCATTER_WAVE) void scatter_gram(Grid g, Units U, double *__restrict__ slabs)
{
    constexpr int K = K0 * K1, Q = strands(K), W = K + NDEP, ROW = (K + 1 + NDEP) | 1;   // an odd row: the strands' reads spread over the banks
    __shared__ double tile[SCATTER_WAVE * ROW];
    const int lane = threadIdx.x, a = lane / Q, q = lane % Q;
    long long cell, begin, end;
    unit_range(U, (long long)blockIdx.x, cell, begin, end);
    const long long c0 = cell / g.nc1, c1 = cell - c0 * g.nc1;
    double acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.0;
    for (long long base = begin; base < end; base += SCATTER_WAVE) {
        const int cnt = (int)(end - base < SCATTER_WAVE ? end - base : SCATTER_WAVE);
        if (lane < cnt) {
            double row[K + 1 + NDEP];
            point_row<K0, K1>(g, U, NDEP, c0, c1, U.order[base + lane], row);
#pragma unroll
            for (int e = 0; e < K + 1 + NDEP; ++e) tile[lane * ROW + e] = row[e];
        }
        __syncthreads();
        if (a < K)
            for (int j = q; j < cnt; j += Q) {
                const double *row = tile + j * ROW;
                const double t = row[K] * row[a];
#pragma unroll
                for (int b = 0; b < K; ++b) acc[b] = acc[b] + t * row[b];
#pragma unroll
                for (int d = 0; d < NDEP; ++d) acc[K + d] = acc[K + d] + t * row[K + 1 + d];
            }
        __syncthreads();
    }
#pragma unroll
    for (int m = 1; m < Q; m <<= 1)
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] = acc[e] + __shfl_xor(acc[e], m, SCATTER_WAVE);
    if (a < K && q == 0) {
        double *out = slabs + ((long long)blockIdx.x * K + a) * W;
#pragma unroll
        for (int e = 0; e < W; ++e) out[e] = acc[e];
    }
}

__global__ __launch_bounds__(SCATTER_BLOCK) void scatter_cell(Level L)
{
    const long long gid = (long long)blockIdx.x * SCATTER_BLOCK + threadIdx.x;
    if (gid >= L.nnodes * L.entries) return;
    cell_lane(L, gid);
}

__global__ __launch_bounds__(SCATTER_BLOCK) void scatter_fold(Fold F, long long lanes)
{
    const long long gid = (long long)blockIdx.x * SCATTER_BLOCK + threadIdx.x;
    if (gid >= lanes) return;
    fold_lane(F, gid);
}

template <int K0, int K1>
__global__ __launch_bounds__(SCATTER_BLOCK) void scatter_residual(Grid g, int ndep, const double *__restrict__ coefs,
                                                                 const double *__restrict__ uvw, const double *__restrict__ points,
                                                                 const int64_t *__restrict__ key, long long npts,
                                                                 double *__restrict__ residual)
{
    const long long gid = (long long)blockIdx.x * SCATTER_BLOCK + threadIdx.x;
    if (gid >= npts) return;
    residual_lane<K0, K1>(g, ndep, coefs, uvw, points, key, npts, gid, residual);
}
#endif

}  // namespace bskscatter
