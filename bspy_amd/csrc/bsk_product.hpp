// Products of splines (bspy_amd/product.py): for one pair of mapped variables the coefficients of self * other are a
// banded BILINEAR operator on the two coefficient lines, the same for every line, as section 13's operators are linear:
//
//   c[j] = sum_{a < k1} sum_{b < k2} W[j][a][b] * A[f[j] + a] * B[g[j] + b],   j < nOut
//
// f and g are non-decreasing, f[j] + k1 <= nIn1, g[j] + k2 <= nIn2.  Several mapped variables: the tensor product.
//
//   ProductMap         host: the tables of M variables and apply_host, the statement of what the kernels compute.
//   band_product_line  device, M = 1: a[PA][n], b[PB][m] -> out[P][N].  A workgroup owns a tile of R output rows of NP
//                      output planes; it stages the pieces a[f[j0] .. f[j1 - 1] + k1 - 1] and b[g[j0] .. g[j1 - 1] + k2 - 1]
//                      of every term of its planes in LDS with coalesced reads; lane = output row, with the row's
//                      k1 * k2 weights in registers (read coalesced from the transposed table Wt[a][b][j]) over its planes.
//   band_product_tile  device, M = 2: a[PA][n1][n2], b[PB][m1][m2] -> out[P][N1][N2].  A workgroup owns TILE_R1 x TILE_R2
//                      outputs of one plane; per term it stages the 2-D pieces of a and b under the tile in LDS.  Lane =
//                      output column (variable 2) with that column's weights W2 in registers; a wave walks rows, so the
//                      row's f1, g1 and W1 are wave-uniform.  Per output and term, for each a1: V[b2] = sum_a2 A[a1][a2] W2[a2][b2]
//                      (A's row is read once and kept over b1), then for each b1: acc += W1[a1][b1] * sum_b2 V[b2] B[b1][b2]:
//                      k1u k1v k2v + k1u k2u (k2v + 1) FMAs.
//
// A plane table terms[P][T][3] = (planeA, planeB, sign) says which planes of a and b make output plane p: it carries the
// dependent-variable rule (scalar 1 term, dot nDep terms, cross 2 signed terms) and the unmapped variables.
//
// Data fp32 or fp64 widened to fp64, weights and accumulation fp64, rounded once.  Sum order, every path: terms in table
// order; within a term variable 1 outermost, a before b; in the last variable V[b] = sum_a A[a] W[a][b], then sum_b V[b] B[b].
// No atomics.  A map whose rows jump so far that a tile's piece does not fit LDS is read in place (staged == 0).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace bskprod {

constexpr int PROD_KMIN = 2, PROD_KMAX = 6;   // orders with a device instantiation
constexpr int PROD_MAXM = 3;                  // mapped variables of the host driver
constexpr int PROD_BLOCK = 256;
constexpr int LINE_LDS = 2048;                // elements of the data type staged per operand, band_product_line
constexpr int TILE_R1 = 16, TILE_R2 = 64;     // output tile of band_product_tile (rows of variable 1 x columns of variable 2)
constexpr int TILE_LDS = 2560;                // elements staged per operand, band_product_tile

struct ProductVar {
    int nIn1 = 0, nIn2 = 0, nOut = 0, k1 = 0, k2 = 0;
    std::vector<int> f, g;          // nOut
    std::vector<double> W;          // nOut * k1 * k2

    // largest pieces of the two operands under a tile of `rows` consecutive output rows
    void max_span(int rows, long long &sa, long long &sb) const
    {
        sa = sb = 0;
        for (int j0 = 0; j0 < nOut; j0 += rows) {
            const int j1 = j0 + rows < nOut ? j0 + rows : nOut;
            const long long a = (long long)f[j1 - 1] + k1 - f[j0], b = (long long)g[j1 - 1] + k2 - g[j0];
            if (a > sa) sa = a;
            if (b > sb) sb = b;
        }
    }
};

struct ProductMap {
    int M = 0;
    ProductVar v[PROD_MAXM];

    // One output of one term: variables lvl .. M - 1 of the planes at a and b (strides sa[], sb[] in elements).
    template <typename T>
    double contract(int lvl, const T *a, const T *b, const long long *sa, const long long *sb, const int *j) const
    {
        const ProductVar &q = v[lvl];
        const int jj = j[lvl];
        const T *pa = a + (long long)q.f[jj] * sa[lvl];
        const T *pb = b + (long long)q.g[jj] * sb[lvl];
        const double *w = q.W.data() + (size_t)jj * q.k1 * q.k2;
        double acc = 0.0;
        if (lvl == M - 1) {
            double V[16];
            for (int bb = 0; bb < q.k2; ++bb) V[bb] = 0.0;
            for (int aa = 0; aa < q.k1; ++aa) {
                const double x = (double)pa[aa * sa[lvl]];
                for (int bb = 0; bb < q.k2; ++bb) V[bb] += x * w[aa * q.k2 + bb];
            }
            for (int bb = 0; bb < q.k2; ++bb) acc += V[bb] * (double)pb[bb * sb[lvl]];
            return acc;
        }
        for (int aa = 0; aa < q.k1; ++aa)
            for (int bb = 0; bb < q.k2; ++bb)
                acc += w[aa * q.k2 + bb] * contract(lvl + 1, pa + aa * sa[lvl], pb + bb * sb[lvl], sa, sb, j);
        return acc;
    }

    template <typename T>
    void apply_host(const T *a, const T *b, const int32_t *terms, long long P, int Tn, T *out) const
    {
        long long sa[PROD_MAXM], sb[PROD_MAXM], so[PROD_MAXM], na = 1, nb = 1, no = 1;
        for (int l = M - 1; l >= 0; --l) {
            sa[l] = na, sb[l] = nb, so[l] = no;
            na *= v[l].nIn1, nb *= v[l].nIn2, no *= v[l].nOut;
        }
        for (long long p = 0; p < P; ++p)
            for (long long o = 0; o < no; ++o) {
                int j[PROD_MAXM];
                for (int l = 0; l < M; ++l) j[l] = (int)(o / so[l] % v[l].nOut);
                double acc = 0.0;
                for (int t = 0; t < Tn; ++t) {
                    const int32_t *e = terms + (p * Tn + t) * 3;
                    acc += (double)e[2] * contract(0, a + e[0] * na, b + e[1] * nb, sa, sb, j);
                }
                out[p * no + o] = (T)acc;
            }
    }
};

#ifdef __HIPCC__
// One row of the last variable: V[b] = sum_a A[a] W[a][b], then sum_b V[b] B[b].  A, B: LDS or global.
template <typename T, int K1, int K2>
__device__ __forceinline__ double row_product(const T *pa, const T *pb, const double (&w)[K1 * K2])
{
    double V[K2];
#pragma unroll
    for (int b = 0; b < K2; ++b) V[b] = 0.0;
#pragma unroll
    for (int a = 0; a < K1; ++a) {
        const double x = (double)pa[a];
#pragma unroll
        for (int b = 0; b < K2; ++b) V[b] += x * w[a * K2 + b];
    }
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < K2; ++b) s += V[b] * (double)pb[b];
    return s;
}

// a: [PA][nIn1], b: [PB][nIn2], out: [P][nOut].  Workgroup = (block of NP planes, tile of R output rows); lane = (plane
// group g = tid / R, row r = tid % R); group g takes planes g, g + G, ... < NP of the block, G = PROD_BLOCK / R.
// staged: the launcher guarantees NP * T * span <= LINE_LDS for both operands and every tile.  An LDS word is read only for
// a plane-term < np * T and a column < span: exactly the words the staging loops write.
// Global reads stay in bounds: f[j] + K1 <= nIn1, g[j] + K2 <= nIn2 (bsk_product_create), planes < PA, PB (checked per call).
template <typename T, int K1, int K2>
__global__ __launch_bounds__(PROD_BLOCK) void band_product_line(const T *__restrict__ a, const T *__restrict__ b,
                                                                T *__restrict__ out, const int *__restrict__ f,
                                                                const int *__restrict__ g, const double *__restrict__ wt,
                                                                const int *__restrict__ terms, int nIn1, int nIn2, int nOut,
                                                                long long P, int Tn, int R, int NP, long long tiles, int staged)
{
    __shared__ T sA[LINE_LDS];
    __shared__ T sB[LINE_LDS];
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x % tiles, pblock = blockIdx.x / tiles;
    const int j0 = (int)tile * R;
    const int rows = nOut - j0 < R ? nOut - j0 : R;
    const long long p0 = pblock * NP;
    const int np = P - p0 < NP ? (int)(P - p0) : NP;
    const int baseA = f[j0], baseB = g[j0];
    const int spanA = f[j0 + rows - 1] + K1 - baseA, spanB = g[j0 + rows - 1] + K2 - baseB;

    if (staged) {
        for (int idx = tid; idx < np * Tn * spanA; idx += PROD_BLOCK) {
            const int q = idx / spanA, c = idx - q * spanA;
            sA[idx] = a[(long long)terms[(p0 * Tn + q) * 3] * nIn1 + baseA + c];
        }
        for (int idx = tid; idx < np * Tn * spanB; idx += PROD_BLOCK) {
            const int q = idx / spanB, c = idx - q * spanB;
            sB[idx] = b[(long long)terms[(p0 * Tn + q) * 3 + 1] * nIn2 + baseB + c];
        }
        __syncthreads();
    }
    const int G = PROD_BLOCK / R;
    const int grp = tid / R, r = tid - grp * R;
    if (grp >= G || r >= rows) return;
    const int j = j0 + r;
    const int offA = f[j] - baseA, offB = g[j] - baseB;
    double w[K1 * K2];
#pragma unroll
    for (int i = 0; i < K1 * K2; ++i) w[i] = wt[(long long)i * nOut + j];
    for (int l = grp; l < np; l += G) {
        double acc = 0.0;
        for (int t = 0; t < Tn; ++t) {
            const int *e = terms + ((p0 + l) * Tn + t) * 3;
            const double sign = (double)e[2];
            if (staged) acc += sign * row_product<T, K1, K2>(sA + (l * Tn + t) * spanA + offA, sB + (l * Tn + t) * spanB + offB, w);
            else acc += sign * row_product<T, K1, K2>(a + (long long)e[0] * nIn1 + baseA + offA, b + (long long)e[1] * nIn2 + baseB + offB, w);
        }
        out[(p0 + l) * nOut + j] = (T)acc;
    }
}

// One output of one term in band_product_tile.  pa, pb: the first window rows of the output's row (LDS or global), lda, ldb
// their row strides; w1 (wave-uniform): W1[a1][b1] of the output row.
template <typename T, int K1V, int K2V>
__device__ __forceinline__ double tile_product(const T *pa, int lda, const T *pb, int ldb, const double *__restrict__ w1, int k1u,
                                               int k2u, const double (&w2)[K1V * K2V])
{
    double acc = 0.0;
    for (int a1 = 0; a1 < k1u; ++a1) {
        double V[K2V];
#pragma unroll
        for (int b = 0; b < K2V; ++b) V[b] = 0.0;
#pragma unroll
        for (int a2 = 0; a2 < K1V; ++a2) {
            const double x = (double)pa[a1 * lda + a2];
#pragma unroll
            for (int b = 0; b < K2V; ++b) V[b] += x * w2[a2 * K2V + b];
        }
        for (int b1 = 0; b1 < k2u; ++b1) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < K2V; ++b) s += V[b] * (double)pb[b1 * ldb + b];
            acc += w1[a1 * k2u + b1] * s;
        }
    }
    return acc;
}

struct TileArgs {
    const int *f1, *g1, *f2, *g2;      // variable 1 (rows) and variable 2 (columns)
    const double *w1;                  // [N1][k1u][k2u]
    const double *wt2;                 // transposed: [K1V * K2V][N2]
    const int *terms;
    int n1, n2, m1, m2, N1, N2, k1u, k2u, Tn;
    long long tiles1, tiles2;
    int staged;
};

// a: [PA][n1][n2], b: [PB][m1][m2], out: [P][N1][N2].  Workgroup = (plane, tile of TILE_R1 rows, tile of TILE_R2 columns);
// lane = (row group rg = tid / TILE_R2 = its wave, column c = tid % TILE_R2); wave rg takes rows rg, rg + 4, ... of the tile.
// staged: the launcher guarantees (rows of a piece) * (columns of a piece) <= TILE_LDS for both operands and every tile.  The
// pieces are stored with their own row length; an LDS word is read only at a row < rowsA and a column < colsA of the
// piece (f1[i] - baseA1 + a1 < rowsA, f2[j] - baseA2 + a2 < colsA by the definition of the spans): the words written.
// Every lane of the workgroup reaches both barriers of every term: no early return before the term loop ends.
template <typename T, int K1V, int K2V>
__global__ __launch_bounds__(PROD_BLOCK) void band_product_tile(const T *__restrict__ a, const T *__restrict__ b, T *__restrict__ out,
                                                                const TileArgs q)
{
    constexpr int RG = PROD_BLOCK / TILE_R2;          // row groups = waves
    constexpr int RPT = TILE_R1 / RG;                 // rows per lane
    __shared__ T sA[TILE_LDS];
    __shared__ T sB[TILE_LDS];
    const int tid = threadIdx.x;
    const long long t2 = blockIdx.x % q.tiles2, rest = blockIdx.x / q.tiles2;
    const long long t1 = rest % q.tiles1, p = rest / q.tiles1;
    const int i0 = (int)t1 * TILE_R1, c0 = (int)t2 * TILE_R2;
    const int rows = q.N1 - i0 < TILE_R1 ? q.N1 - i0 : TILE_R1;
    const int cols = q.N2 - c0 < TILE_R2 ? q.N2 - c0 : TILE_R2;
    const int baseA1 = q.f1[i0], baseB1 = q.g1[i0], baseA2 = q.f2[c0], baseB2 = q.g2[c0];
    const int rowsA = q.f1[i0 + rows - 1] + q.k1u - baseA1, rowsB = q.g1[i0 + rows - 1] + q.k2u - baseB1;
    const int colsA = q.f2[c0 + cols - 1] + K1V - baseA2, colsB = q.g2[c0 + cols - 1] + K2V - baseB2;

    const int rg = tid / TILE_R2, c = tid - rg * TILE_R2;
    const bool live = c < cols;
    const int j = c0 + (live ? c : 0);
    const int offA2 = q.f2[j] - baseA2, offB2 = q.g2[j] - baseB2;
    double w2[K1V * K2V];
#pragma unroll
    for (int i = 0; i < K1V * K2V; ++i) w2[i] = q.wt2[(long long)i * q.N2 + j];

    double acc[RPT];
#pragma unroll
    for (int s = 0; s < RPT; ++s) acc[s] = 0.0;
    for (int t = 0; t < q.Tn; ++t) {
        const int *e = q.terms + (p * q.Tn + t) * 3;
        const T *ga = a + ((long long)e[0] * q.n1 + baseA1) * q.n2 + baseA2;
        const T *gb = b + ((long long)e[1] * q.m1 + baseB1) * q.m2 + baseB2;
        const double sign = (double)e[2];
        if (q.staged) {
            if (t) __syncthreads();                  // the previous term's pieces have been read
            for (int idx = tid; idx < rowsA * colsA; idx += PROD_BLOCK) {
                const int rr = idx / colsA, cc = idx - rr * colsA;
                sA[idx] = ga[(long long)rr * q.n2 + cc];
            }
            for (int idx = tid; idx < rowsB * colsB; idx += PROD_BLOCK) {
                const int rr = idx / colsB, cc = idx - rr * colsB;
                sB[idx] = gb[(long long)rr * q.m2 + cc];
            }
            __syncthreads();
        }
#pragma unroll
        for (int s = 0; s < RPT; ++s) {
            const int r = rg + s * RG;               // wave-uniform
            if (r < rows && live) {
                const int i = i0 + r;
                const int ra = q.f1[i] - baseA1, rb = q.g1[i] - baseB1;
                const double *w1 = q.w1 + (long long)i * q.k1u * q.k2u;
                if (q.staged)
                    acc[s] += sign * tile_product<T, K1V, K2V>(sA + ra * colsA + offA2, colsA, sB + rb * colsB + offB2, colsB, w1, q.k1u, q.k2u, w2);
                else
                    acc[s] += sign * tile_product<T, K1V, K2V>(ga + (long long)ra * q.n2 + offA2, q.n2, gb + (long long)rb * q.m2 + offB2, q.m2, w1,
                                                               q.k1u, q.k2u, w2);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < RPT; ++s) {
        const int r = rg + s * RG;
        if (r < rows && live) out[(p * q.N1 + i0 + r) * q.N2 + j] = (T)acc[s];
    }
}
#endif

}  // namespace bskprod
