// Gauss-Kronrod 7/15 quadrature of f(S(u)) * mu(u) over boxes ("regions") inside one knot cell each
// (Spline.integral; reference bspy/_spline_evaluation.py:29-73 integrates the same measure with nested quad).
//
// mu(u) = product of the singular values of the nDep x nInd jacobian J:
//   |det J| (nDep == nInd), sqrt(det JtJ) (nDep > nInd), sqrt(det J Jt) (nDep < nInd); determinants clamped at 0.
//
// One workgroup per region.  A region lies inside one knot cell, so its span indices come with it (no span
// search) and every node shares one control-point window: the window is staged in LDS once, and the value and
// first-derivative bases are computed once per axis node (15 per variable) into LDS.  Each lane then contracts
// the window for its tensor nodes; dependents are visited one at a time (the Gram matrix JtJ is accumulated over
// them), so LDS holds order^nInd values per staged dependent whatever nDep is.
//   mode MEASURE : out[2 r] = K_r, out[2 r + 1] = G_r (fp64), the Kronrod / embedded Gauss sums of mu.
//   mode NODES   : per node q of region r, out[(r * NN + q) * (nDep + 2) + ...] = x[nDep], wK * mu, wG * mu (fp64).
// Sums run in a fixed lane order (per-lane partials, wave shuffles, waves through LDS): no atomics, results are
// bitwise reproducible.
#pragma once
#include "bsk_device.hpp"

namespace bsk {

constexpr int GK_N = 15;

// Kronrod 15-point nodes on [-1, 1], ascending; the 7 Gauss-Legendre nodes are those of odd index.
__constant__ double GK_X[GK_N] = {
    -0.99145537112081264, -0.94910791234275852, -0.86486442335976907, -0.74153118559939444, -0.58608723546769113,
    -0.40584515137739717, -0.20778495500789847, 0.0, 0.20778495500789847, 0.40584515137739717,
    0.58608723546769113, 0.74153118559939444, 0.86486442335976907, 0.94910791234275852, 0.99145537112081264};
__constant__ double GK_WK[GK_N] = {
    0.022935322010529225, 0.063092092629978553, 0.10479001032225018, 0.14065325971552592, 0.16900472663926790,
    0.19035057806478541, 0.20443294007529889, 0.20948214108472783, 0.20443294007529889, 0.19035057806478541,
    0.16900472663926790, 0.14065325971552592, 0.10479001032225018, 0.063092092629978553, 0.022935322010529225};
// Gauss 7-point weights at the same 15 positions (0 at the Kronrod-only nodes).
__constant__ double GK_WG[GK_N] = {
    0.0, 0.12948496616886969, 0.0, 0.27970539148927667, 0.0, 0.38183005050511894, 0.0, 0.41795918367346939,
    0.0, 0.38183005050511894, 0.0, 0.27970539148927667, 0.0, 0.12948496616886969, 0.0};

enum { IQ_MEASURE = 0, IQ_NODES = 1 };

template <int NIND>
struct IntegralShape {
    static constexpr int NN = NIND == 1 ? GK_N : NIND == 2 ? GK_N * GK_N : GK_N * GK_N * GK_N;   // nodes per region
    static constexpr int BLOCK = NIND == 1 ? 64 : 256;
};

template <int NIND, int OMAX>
struct IntegralLds {
    static constexpr int WIN = NIND == 1 ? OMAX : NIND == 2 ? OMAX * OMAX : OMAX * OMAX * OMAX;
    static constexpr int CAP = WIN > 2048 ? WIN : 2048;     // coefficient slots: CAP / window dependents per stage
};

template <typename T>
__device__ __forceinline__ T det3(const T (&m)[3][3])
{
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// Fixed-order sum over the workgroup (lane partials -> wave shuffles -> waves in index order); lane 0 returns it.
template <int BLOCK>
__device__ __forceinline__ double block_sum(double v, double *red)
{
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    constexpr int NW = BLOCK / WAVE;
    if (NW == 1) return v;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    __syncthreads();                                        // red may still be read by an earlier sum
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NW; ++w) t += red[w];
    return t;
}

// tab: the spline's axis table (Desc), coef: (nDep, nCoef...) as Desc describes.  lo_hi: nreg x NIND x 2 region
// bounds, span: nreg x NIND span indices ("rightmost knot of the segment", validated by the host).  Orders are the
// spline's own (<= OMAX), read from the descriptor.
template <typename T, int NIND, int OMAX>
__global__ void __launch_bounds__(IntegralShape<NIND>::BLOCK)
integral_regions(Desc<T> d, const T *__restrict__ tab, const T *__restrict__ coef, const T *__restrict__ lo_hi,
                 const int *__restrict__ span, int mode, double *__restrict__ out)
{
    constexpr int NN = IntegralShape<NIND>::NN;
    constexpr int BLOCK = IntegralShape<NIND>::BLOCK;
    constexpr int CAP = IntegralLds<NIND, OMAX>::CAP;
    __shared__ T sb[NIND][GK_N][2][OMAX];     // value / first-derivative basis per axis node, right aligned
    __shared__ T sc[CAP];                     // control-point windows of the staged dependents
    __shared__ double red[BLOCK / WAVE];
    const long long r = blockIdx.x;
    const int tid = threadIdx.x;
    const int nDep = d.nDep;

    int o[NIND], base[NIND];
    double half[NIND];
    double vol = 1.0;
    int W = 1;
#pragma unroll
    for (int i = 0; i < NIND; ++i) {
        const double lo = double(lo_hi[(r * NIND + i) * 2]), hi = double(lo_hi[(r * NIND + i) * 2 + 1]);
        o[i] = d.order[i];
        base[i] = span[r * NIND + i] - o[i];
        half[i] = 0.5 * (hi - lo);
        vol *= half[i];
        W *= o[i];
        if (tid / GK_N == i) {                  // lanes i * 15 .. i * 15 + 14 build the bases of variable i
            const int j = tid % GK_N;
            const T u = T(0.5 * (lo + hi) + half[i] * GK_X[j]);
            T b[OMAX], db[OMAX];
            basis_bounded<T, OMAX>(tab + d.off[i], d.nk[i], o[i], base[i] + o[i], u, 0, b);
            basis_bounded<T, OMAX>(tab + d.off[i], d.nk[i], o[i], base[i] + o[i], u, 1, db);
#pragma unroll
            for (int m = 0; m < OMAX; ++m) {
                sb[i][j][0][m] = b[m];
                sb[i][j][1][m] = db[m];
            }
        }
    }
    const int DG = CAP / W;                     // dependents per stage (>= 1: W <= OMAX^NIND <= CAP)
    const bool once = nDep <= DG;

    double accK = 0.0, accG = 0.0;
    for (int q0 = 0; q0 < NN; q0 += BLOCK) {
        const int q = q0 + tid;
        const bool active = q < NN;
        int j[NIND];
        {
            int t = active ? q : 0;
#pragma unroll
            for (int i = NIND - 1; i >= 0; --i) { j[i] = t % GK_N; t /= GK_N; }
        }
        T gram[NIND][NIND];
        T rows[3][NIND];                         // the first rows of J (nDep <= nInd)
#pragma unroll
        for (int a = 0; a < NIND; ++a) {
#pragma unroll
            for (int b = 0; b < NIND; ++b) gram[a][b] = T(0);
#pragma unroll
            for (int e = 0; e < 3; ++e) rows[e][a] = T(0);
        }
        for (int dg0 = 0; dg0 < nDep; dg0 += DG) {
            const int ng = min(DG, nDep - dg0);
            if (!once || q0 == 0) {
                __syncthreads();                 // earlier readers of sc are done (and the bases are written)
                for (int e = tid; e < ng * W; e += BLOCK) {
                    const int g = e / W;
                    int rest = e - g * W;
                    long long gi = (long long)(dg0 + g) * d.cstride[0];
#pragma unroll
                    for (int i = NIND - 1; i >= 0; --i) {
                        const int k = rest % o[i];
                        rest /= o[i];
                        gi += (long long)(base[i] + k) * d.cstride[i + 1];
                    }
                    sc[e] = coef[gi];
                }
                __syncthreads();
            }
            if (!active) continue;
            for (int g = 0; g < ng; ++g) {
                const T *c = sc + g * W;
                T x = T(0), dx[NIND];
#pragma unroll
                for (int i = 0; i < NIND; ++i) dx[i] = T(0);
                const T *B0 = &sb[0][j[0]][0][OMAX - o[0]], *D0 = &sb[0][j[0]][1][OMAX - o[0]];
                if constexpr (NIND == 1) {
                    for (int a = 0; a < o[0]; ++a) {
                        x += c[a] * B0[a];
                        dx[0] += c[a] * D0[a];
                    }
                } else if constexpr (NIND == 2) {
                    const T *B1 = &sb[1][j[1]][0][OMAX - o[1]], *D1 = &sb[1][j[1]][1][OMAX - o[1]];
                    for (int a = 0; a < o[0]; ++a) {
                        T t = T(0), td = T(0);
                        for (int k = 0; k < o[1]; ++k) {
                            const T cv = c[a * o[1] + k];
                            t += cv * B1[k];
                            td += cv * D1[k];
                        }
                        x += t * B0[a];
                        dx[0] += t * D0[a];
                        dx[1] += td * B0[a];
                    }
                } else {
                    const T *B1 = &sb[1][j[1]][0][OMAX - o[1]], *D1 = &sb[1][j[1]][1][OMAX - o[1]];
                    const T *B2 = &sb[2][j[2]][0][OMAX - o[2]], *D2 = &sb[2][j[2]][1][OMAX - o[2]];
                    for (int a = 0; a < o[0]; ++a) {
                        T s = T(0), s1 = T(0), s2 = T(0);
                        for (int k = 0; k < o[1]; ++k) {
                            T t = T(0), td = T(0);
                            for (int m = 0; m < o[2]; ++m) {
                                const T cv = c[(a * o[1] + k) * o[2] + m];
                                t += cv * B2[m];
                                td += cv * D2[m];
                            }
                            s += t * B1[k];
                            s1 += t * D1[k];
                            s2 += td * B1[k];
                        }
                        x += s * B0[a];
                        dx[0] += s * D0[a];
                        dx[1] += s1 * B0[a];
                        dx[2] += s2 * B0[a];
                    }
                }
                // dx: jacobian row of this dependent in the spline's own parameters (the [-1, 1] -> [lo, hi]
                // scaling of the rule is in the weights: vol)
                const int dep = dg0 + g;
                if (mode == IQ_NODES) out[((r * NN + q) * (nDep + 2)) + dep] = double(x);
#pragma unroll
                for (int a = 0; a < NIND; ++a)
#pragma unroll
                    for (int b = 0; b < NIND; ++b) gram[a][b] += dx[a] * dx[b];
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (dep == e)
#pragma unroll
                        for (int a = 0; a < NIND; ++a) rows[e][a] = dx[a];
            }
        }
        if (!active) continue;
        T mu;
        if (nDep == NIND) {
            if constexpr (NIND == 1) mu = fabs(rows[0][0]);
            else if constexpr (NIND == 2) mu = fabs(rows[0][0] * rows[1][1] - rows[0][1] * rows[1][0]);
            else {
                T m[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) m[a][b] = rows[a][b % NIND];
                mu = fabs(det3(m));
            }
        } else if (nDep > NIND) {
            T det;
            if constexpr (NIND == 1) det = gram[0][0];
            else if constexpr (NIND == 2) det = gram[0][0] * gram[1][1] - gram[0][1] * gram[1][0];
            else {
                T m[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) m[a][b] = gram[a % NIND][b % NIND];
                det = det3(m);
            }
            mu = sqrt(fmax(det, T(0)));
        } else {                                 // nDep < nInd (so nInd >= 2, nDep <= 2): det(J Jt)
            T g00 = T(0), g01 = T(0), g11 = T(0);
#pragma unroll
            for (int a = 0; a < NIND; ++a) {
                g00 += rows[0][a] * rows[0][a];
                g01 += rows[0][a] * rows[1][a];
                g11 += rows[1][a] * rows[1][a];
            }
            mu = nDep == 1 ? sqrt(g00) : sqrt(fmax(g00 * g11 - g01 * g01, T(0)));
        }
        double wK = vol, wG = vol;
#pragma unroll
        for (int i = 0; i < NIND; ++i) {
            wK *= GK_WK[j[i]];
            wG *= GK_WG[j[i]];
        }
        const double fk = wK * double(mu), fg = wG * double(mu);
        if (mode == IQ_NODES) {
            double *p = out + (r * NN + q) * (nDep + 2) + nDep;
            p[0] = fk;
            p[1] = fg;
        } else {
            accK += fk;
            accG += fg;
        }
    }
    if (mode == IQ_MEASURE) {
        const double k = block_sum<BLOCK>(accK, red);
        const double g = block_sum<BLOCK>(accG, red);
        if (tid == 0) {
            out[2 * r] = k;
            out[2 * r + 1] = g;
        }
    }
}

}  // namespace bsk
