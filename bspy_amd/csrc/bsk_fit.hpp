// Spline.least_squares (bspy_amd/fitting.py): min |A x - b| for one variable of gridded data, A = banded collocation
// matrix (`order` non-zeros per row, first columns non-decreasing), b = every line of the data along that variable.
//
//   FitPlan        host: row-sequential Givens QR of the band.  Row r (first column f) meets R rows f .. f + k - 1 in
//                  turn; no earlier row reaches past column f + k - 1, so the row is zero after k rotations and R keeps
//                  bandwidth k.  The plan records (c, s) of every rotation and the final R: everything that does not
//                  depend on the right-hand sides.
//   fit_sweep      device: one lane = one line.  Forward: walk the rows, rotate b[row] into a register window of k
//                  partly rotated entries of Q^T b, store an entry when the window's first column moves past it.
//                  Backward: back-substitution over R with a register window of k - 1 solved values.  (c, s), first
//                  columns and R are the same for all lanes: staged in LDS per row block, read at uniform addresses.
//                  Data is viewed as [outer, nRows, inner], lanes run along `inner`.
//   fit_transpose  device: [R, C] -> [C, R] through a padded LDS tile; a line that is contiguous in memory (inner == 1)
//                  is turned so that the sweep always reads and writes along lanes.
//   fit_residual   device: squared residual b - A x summed over the lines of each row in a fixed order (per-lane
//                  partial sums, an LDS tree, then the workgroup partials of a row in index order): no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

namespace bskfit {

constexpr int FIT_BLOCK = 64;      // lanes (= lines) per workgroup of fit_sweep: few lines still spread over many CUs
constexpr int FIT_ROWS = 16;       // rows per staged block of fit_sweep
constexpr int FIT_KMAX = 8;        // largest order with a device instantiation
constexpr int FIT_TILE = 32;       // fit_transpose tile edge
constexpr int RES_BLOCK = 256;     // fit_residual: lanes per workgroup ...
constexpr int RES_PER_LANE = 4;    // ... and lines per lane

struct FitPlan {
    int nrows = 0, ncols = 0, k = 0;
    std::vector<int> first;        // nrows
    std::vector<double> avals;     // nrows * k, the band of A
    std::vector<double> rot;       // nrows * k * 2: (c, s) of the rotation of row r against R row first[r] + t
    std::vector<double> R;         // ncols * k: R[j][j + t]
    double rmin = 0.0, rmax = 0.0; // min / max |R_jj|

    void factor()
    {
        R.assign((size_t)ncols * k, 0.0);
        rot.assign((size_t)nrows * k * 2, 0.0);
        std::vector<double> w(k);
        for (int r = 0; r < nrows; ++r) {
            const int f = first[r];
            for (int t = 0; t < k; ++t) w[t] = avals[(size_t)r * k + t];
            for (int t = 0; t < k; ++t) {
                double *Rj = &R[(size_t)(f + t) * k];       // columns f + t .. : Rj[u] pairs with w[t + u]
                const double a = Rj[0], bq = w[t];
                const double h = std::hypot(a, bq);
                double c = 1.0, s = 0.0;
                if (h > 0.0 && bq != 0.0) {
                    c = a / h;
                    s = bq / h;
                    for (int u = 0; t + u < k; ++u) {
                        const double ru = Rj[u], wu = w[t + u];
                        Rj[u] = c * ru + s * wu;
                        w[t + u] = c * wu - s * ru;
                    }
                    Rj[0] = h;
                }
                rot[((size_t)r * k + t) * 2] = c;
                rot[((size_t)r * k + t) * 2 + 1] = s;
            }
        }
        rmin = rmax = std::fabs(R[0]);
        for (int j = 0; j < ncols; ++j) {
            const double v = std::fabs(R[(size_t)j * k]);
            rmin = std::min(rmin, v);
            rmax = std::max(rmax, v);
        }
    }

    // One line on the host, the statement of what fit_sweep computes: b[row * bstride] -> x[col * xstride].
    template <typename TIN>
    void solve_line(const TIN *b, long long bstride, double *x, long long xstride, std::vector<double> &d) const
    {
        d.assign(ncols, 0.0);
        for (int r = 0; r < nrows; ++r) {
            double beta = (double)b[(long long)r * bstride];
            const int f = first[r];
            for (int t = 0; t < k; ++t) {
                const double c = rot[((size_t)r * k + t) * 2], s = rot[((size_t)r * k + t) * 2 + 1];
                const double dj = d[f + t];
                d[f + t] = c * dj + s * beta;
                beta = c * beta - s * dj;
            }
        }
        for (int j = ncols - 1; j >= 0; --j) {
            double acc = d[j];
            for (int t = 1; t < k && j + t < ncols; ++t) acc -= R[(size_t)j * k + t] * d[j + t];
            d[j] = acc * (1.0 / R[(size_t)j * k]);
        }
        for (int j = 0; j < ncols; ++j) x[(long long)j * xstride] = d[j];
    }
};

#ifdef __HIPCC__
// b: [outer, nrows, inner] (TIN), x: [outer, ncols, inner] (fp64); line L = o * inner + i.  One wave per workgroup.
// The walk is latency bound (a line is one dependent chain), so nothing on it may wait for memory: the rotations
// (and R on the way back) of FIT_ROWS rows are staged in LDS, fetched into registers one block ahead, and read at
// wave-uniform addresses (broadcast); the right-hand side values are fetched one block ahead too.  Every word of the
// staging area is written before the block that reads it (identity rotations / zeros past the end).
// Rd = R with R_jj replaced by 1 / R_jj.
template <typename TIN, int K>
__global__ __launch_bounds__(FIT_BLOCK) void fit_sweep(const TIN *__restrict__ b, double *__restrict__ x,
                                                       const double2 *__restrict__ rot, const int *__restrict__ first,
                                                       const double *__restrict__ Rd, int nrows, int ncols,
                                                       long long inner, long long nlines)
{
    constexpr int PER = (FIT_ROWS * K + FIT_BLOCK - 1) / FIT_BLOCK;      // staged entries per lane
    __shared__ double2 srot[FIT_ROWS * K];
    __shared__ double sR[FIT_ROWS * K];
    __shared__ int sfirst[FIT_ROWS];
    const int lane = threadIdx.x;
    long long L = (long long)blockIdx.x * FIT_BLOCK + lane;
    const bool live = L < nlines;          // idle lanes of the last wave keep staging; they load and store no data
    if (!live) L = nlines - 1;
    const long long o = L / inner, ii = L - o * inner;
    const TIN *bl = b + o * nrows * inner + ii;
    double *xl = x + o * ncols * inner + ii;

    // ---- forward: d[t] = partly rotated entry of Q^T b at column f + t
    double d[K];
#pragma unroll
    for (int t = 0; t < K; ++t) d[t] = 0.0;
    int f = 0;
    double2 pre[PER];
    int prefirst = 0;
    double bb[FIT_ROWS], bnext[FIT_ROWS];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int idx = p * FIT_BLOCK + lane;
            const long long g = (long long)r0 * K + idx;
            pre[p] = idx < FIT_ROWS * K && g < (long long)nrows * K ? rot[g] : make_double2(1.0, 0.0);
        }
        prefirst = lane < FIT_ROWS && r0 + lane < nrows ? first[r0 + lane] : 0;
#pragma unroll
        for (int q = 0; q < FIT_ROWS; ++q) bnext[q] = live && r0 + q < nrows ? (double)bl[(long long)(r0 + q) * inner] : 0.0;
    };
    fetch(0);
    for (int r0 = 0; r0 < nrows; r0 += FIT_ROWS) {
        __syncthreads();                   // the previous block's reads of the staging area are done
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int idx = p * FIT_BLOCK + lane;
            if (idx < FIT_ROWS * K) srot[idx] = pre[p];
        }
        if (lane < FIT_ROWS) sfirst[lane] = prefirst;
#pragma unroll
        for (int q = 0; q < FIT_ROWS; ++q) bb[q] = bnext[q];
        __syncthreads();
        if (r0 + FIT_ROWS < nrows) fetch(r0 + FIT_ROWS);
        // the staged values of row q + 1 are read while row q's chain runs
        double2 cs[K], csn[K];
        int frn = sfirst[0];
#pragma unroll
        for (int t = 0; t < K; ++t) csn[t] = srot[t];
#pragma unroll
        for (int q = 0; q < FIT_ROWS; ++q) {
            const int row = r0 + q;
            const int fr = __builtin_amdgcn_readfirstlane(frn);
#pragma unroll
            for (int t = 0; t < K; ++t) cs[t] = csn[t];
            if (q + 1 < FIT_ROWS) {
                frn = sfirst[q + 1];
#pragma unroll
                for (int t = 0; t < K; ++t) csn[t] = srot[(q + 1) * K + t];
            }
            if (row < nrows) {
                while (f < fr) {                     // uniform: column f is finished
                    if (live) xl[(long long)f * inner] = d[0];
#pragma unroll
                    for (int t = 0; t + 1 < K; ++t) d[t] = d[t + 1];
                    d[K - 1] = 0.0;
                    ++f;
                }
                double beta = bb[q];
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    const double dj = d[t];
                    d[t] = cs[t].x * dj + cs[t].y * beta;
                    beta = cs[t].x * beta - cs[t].y * dj;
                }
            }
        }
    }
    while (f < ncols) {
        if (live) xl[(long long)f * inner] = d[0];
#pragma unroll
        for (int t = 0; t + 1 < K; ++t) d[t] = d[t + 1];
        d[K - 1] = 0.0;
        ++f;
    }

    // ---- backward: xs[t] = x at column j + 1 + t (zero past the last column, where R holds zeros too); blocks of
    // FIT_ROWS columns from the last one down, block entry q = column j0 - q
    constexpr int W = K > 1 ? K - 1 : 1;
    double xs[W];
#pragma unroll
    for (int t = 0; t < W; ++t) xs[t] = 0.0;
    double rpre[PER];
    auto fetch_back = [&](int j0) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int idx = p * FIT_BLOCK + lane;            // entry (q, t) = (idx / K, idx % K)
            const int j = j0 - idx / K;
            rpre[p] = idx < FIT_ROWS * K && j >= 0 ? Rd[(long long)j * K + idx % K] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < FIT_ROWS; ++q) bnext[q] = live && j0 - q >= 0 ? xl[(long long)(j0 - q) * inner] : 0.0;
    };
    fetch_back(ncols - 1);
    for (int j0 = ncols - 1; j0 >= 0; j0 -= FIT_ROWS) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int idx = p * FIT_BLOCK + lane;
            if (idx < FIT_ROWS * K) sR[idx] = rpre[p];
        }
#pragma unroll
        for (int q = 0; q < FIT_ROWS; ++q) bb[q] = bnext[q];
        __syncthreads();
        if (j0 - FIT_ROWS >= 0) fetch_back(j0 - FIT_ROWS);
        double rr[K], rn[K];
#pragma unroll
        for (int t = 0; t < K; ++t) rn[t] = sR[t];
#pragma unroll
        for (int q = 0; q < FIT_ROWS; ++q) {
            const int j = j0 - q;
#pragma unroll
            for (int t = 0; t < K; ++t) rr[t] = rn[t];
            if (q + 1 < FIT_ROWS) {
#pragma unroll
                for (int t = 0; t < K; ++t) rn[t] = sR[(q + 1) * K + t];
            }
            if (j >= 0) {
                double acc = bb[q];
#pragma unroll
                for (int t = 1; t < K; ++t) acc -= rr[t] * xs[t - 1];
                const double xj = acc * rr[0];
#pragma unroll
                for (int t = W - 1; t > 0; --t) xs[t] = xs[t - 1];
                xs[0] = xj;
                if (live) xl[(long long)j * inner] = xj;
            }
        }
    }
}

// in: [R, C] (TIN) -> out: [C, R] (fp64).  Workgroup (FIT_TILE, 8), one tile each; a word of the tile is read only
// under the condition it was written under.
template <typename TIN>
__global__ __launch_bounds__(FIT_TILE * 8) void fit_transpose(const TIN *__restrict__ in, double *__restrict__ out,
                                                              long long R, long long C, long long tiles_c)
{
    __shared__ double tile[FIT_TILE][FIT_TILE + 1];
    const long long by = blockIdx.x / tiles_c, bx = blockIdx.x - by * tiles_c;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long long c = bx * FIT_TILE + tx;
    for (int i = ty; i < FIT_TILE; i += 8) {
        const long long r = by * FIT_TILE + i;
        if (r < R && c < C) tile[i][tx] = (double)in[r * C + c];
    }
    __syncthreads();
    const long long r2 = by * FIT_TILE + tx;
    for (int i = ty; i < FIT_TILE; i += 8) {
        const long long c2 = bx * FIT_TILE + i;
        if (r2 < R && c2 < C) out[c2 * R + r2] = tile[tx][i];
    }
}

// partial[row * nchunks + chunk] = sum over the chunk's lines of (b - A x)^2; workgroup = (row, chunk).
template <typename TIN>
__global__ __launch_bounds__(RES_BLOCK) void fit_residual(const TIN *__restrict__ b, const double *__restrict__ x,
                                                          const double *__restrict__ avals, const int *__restrict__ first,
                                                          int k, int nrows, int ncols, long long inner, long long nlines,
                                                          long long nchunks, double *__restrict__ partial)
{
    __shared__ double red[RES_BLOCK];
    const long long row = blockIdx.x / nchunks, chunk = blockIdx.x - row * nchunks;
    const int f = first[row];
    double acc = 0.0;
    for (int m = 0; m < RES_PER_LANE; ++m) {
        const long long L = (chunk * RES_PER_LANE + m) * RES_BLOCK + threadIdx.x;
        if (L < nlines) {
            const long long o = L / inner, ii = L - o * inner;
            double r = (double)b[(o * nrows + row) * inner + ii];
            const double *xl = x + (o * ncols + f) * inner + ii;
            for (int t = 0; t < k; ++t) r -= avals[row * k + t] * xl[(long long)t * inner];
            acc += r * r;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = RES_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// sumsq[row] = partial[row][0] + partial[row][1] + ... in index order
__global__ void fit_residual_rows(const double *__restrict__ partial, long long nchunks, int nrows, double *__restrict__ sumsq)
{
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    double acc = 0.0;
    for (long long c = 0; c < nchunks; ++c) acc += partial[row * nchunks + c];
    sumsq[row] = acc;
}
#endif

}  // namespace bskfit
