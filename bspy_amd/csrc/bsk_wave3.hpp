// One wave per trivariate Bernstein cell, one lane per coefficient: the wave of roots3_isolate (bsk_roots3.hpp, three
// components, threshold 0), of ssx_isolate (bsk_ssx.hpp, through bsk_roots3.hpp) and of iso_walk (bsk_iso.hpp, one
// component, threshold tau).
//
// Lane (i0 K1 + i1) K2 + i2 holds coefficient (i0, i1, i2) of the NC components; K0 K1 K2 <= 64 and the lanes behind are
// loaded with 0 and masked out of the ballots.  A value is V[NC], V one double per lane.
//   de Casteljau along an axis is K - 1 rounds of "fetch the neighbour STRIDE lanes away, lerp":
//     left part at t    round r: lanes with e >= r take lerp(1 - t, t, x[e - 1], x[e])   (e the lane's
//     right part at t   round r: lanes with e < K - r take lerp(1 - t, t, x[e], x[e + 1])  index on the axis)
//   which leave in lane e exactly the entry e of bskroots::split's left and right.
//   A component is on one side of the threshold when the ballot of (x > tau) or of (x < -tau) covers the live lanes; the
//   threshold is a double, or Zero: x > 0.0 and x < 0.0.
// Everything is written once over a `wave` that is 64 lanes on the device (LaneWave: a double per lane, shuffles, two
// ballots) and an array of 64 doubles per value on the host (HostWave: loops), which makes the host path the yardstick of
// the device path.  The families keep their walks, leaves and constants.  The arithmetic is bsk_roots.hpp's (fp64, no
// contraction, lerp(s, t, a, b) = s a + t b).
#pragma once
#include <hip/hip_runtime.h>

#include "bsk_roots.hpp"

#pragma clang fp contract(off)

namespace bskwave3 {

using bskroots::lerp;

constexpr int WAVE = 64;

// the threshold 0 as a type: the comparisons are x > 0.0 and x < 0.0
struct Zero {};
BSK_HD bool above(double x, Zero) { return x > 0.0; }
BSK_HD bool below(double x, Zero) { return x < 0.0; }
BSK_HD bool above(double x, double tau) { return x > tau; }
BSK_HD bool below(double x, double tau) { return x < -tau; }

// N coefficients that are all above tau or all below -tau
template <int N, class T>
BSK_HD bool one_side(const double *c, T tau)
{
    bool pos = true, neg = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pos = pos && above(c[i], tau);
        neg = neg && below(c[i], tau);
    }
    return pos || neg;
}

// ------------------------------------------------------------------------------------------ the two waves
// Both offer: first, bcast, get0, clear, load, left_part, right_part, one_side, eval_axis.  A cell is anything with
// at(d, i0, i1, i2).
template <int NC>
struct HostWave {
    struct V {
        double a[WAVE];
    };
    bool first() const { return true; }
    int bcast(int x) const { return x; }
    double get0(const V &x) const { return x.a[0]; }
    void clear(V &c) const
    {
        for (int l = 0; l < WAVE; ++l) c.a[l] = 0.0;
    }

    template <int K0, int K1, int K2, class Cell>
    void load(const Cell &cell, V *c) const
    {
        for (int d = 0; d < NC; ++d)
            for (int l = 0; l < WAVE; ++l) {
                const int i0 = l / (K1 * K2), i1 = (l / K2) % K1, i2 = l % K2;
                c[d].a[l] = l < K0 * K1 * K2 ? cell.at(d, i0, i1, i2) : 0.0;
            }
    }
    template <int K, int STRIDE>
    void left_part(V *x, double s, double t) const
    {
        for (int r = 1; r < K; ++r)
            for (int d = 0; d < NC; ++d) {
                const V old = x[d];
                for (int l = 0; l < WAVE; ++l) {
                    const double below = l >= STRIDE ? old.a[l - STRIDE] : old.a[l];
                    if ((l / STRIDE) % K >= r) x[d].a[l] = lerp(s, t, below, old.a[l]);
                }
            }
    }
    template <int K, int STRIDE>
    void right_part(V *x, double s, double t) const
    {
        for (int r = 1; r < K; ++r)
            for (int d = 0; d < NC; ++d) {
                const V old = x[d];
                for (int l = 0; l < WAVE; ++l) {
                    const double above = l + STRIDE < WAVE ? old.a[l + STRIDE] : old.a[l];
                    if ((l / STRIDE) % K < K - r) x[d].a[l] = lerp(s, t, old.a[l], above);
                }
            }
    }
    // a component whose N live coefficients are all above tau or all below -tau
    template <int N, class T>
    bool one_side(const V *x, T tau) const
    {
        // NC = 1 through the unrolled test, more components in a rolled loop: what the host builds of the families had, and
        // either is 0.5 - 3 % slower on the host in the other's form
        if constexpr (NC == 1) {
            return bskwave3::one_side<N>(x[0].a, tau);
        } else {
            bool one = false;
            for (int d = 0; d < NC; ++d) {
                bool pos = true, neg = true;
                for (int l = 0; l < N; ++l) {
                    pos = pos && above(x[d].a[l], tau);
                    neg = neg && below(x[d].a[l], tau);
                }
                one = one || pos || neg;
            }
            return one;
        }
    }
    // value and derivative at x of the lines of one component along one axis; the results of a line sit in its lane e = 0
    template <int K, int STRIDE>
    void eval_axis(const V &c, double x, V &val, V &der) const
    {
        V b = c;
        const double s = 1.0 - x;
        for (int r = 1; r < K - 1; ++r) {
            const V old = b;
            for (int l = 0; l < WAVE; ++l) {
                const double above = l + STRIDE < WAVE ? old.a[l + STRIDE] : old.a[l];
                if ((l / STRIDE) % K < K - r) b.a[l] = lerp(s, x, old.a[l], above);
            }
        }
        for (int l = 0; l < WAVE; ++l) {
            const double above = l + STRIDE < WAVE ? b.a[l + STRIDE] : b.a[l];
            der.a[l] = (double)(K - 1) * (above - b.a[l]);
            val.a[l] = lerp(s, x, b.a[l], above);
        }
    }
};

#ifdef __HIPCC__
template <int NC>
struct LaneWave {
    using V = double;
    int lane;
    __device__ bool first() const { return lane == 0; }
    __device__ int bcast(int x) const { return __shfl(x, 0); }
    __device__ double get0(const V &x) const { return __shfl(x, 0); }
    __device__ void clear(V &c) const { c = 0.0; }

    template <int K0, int K1, int K2, class Cell>
    __device__ void load(const Cell &cell, V *c) const
    {
        const int i0 = lane / (K1 * K2), i1 = (lane / K2) % K1, i2 = lane % K2;
#pragma unroll
        for (int d = 0; d < NC; ++d) c[d] = lane < K0 * K1 * K2 ? cell.at(d, i0, i1, i2) : 0.0;
    }
    template <int K, int STRIDE>
    __device__ void left_part(V *x, double s, double t) const
    {
        const int e = (lane / STRIDE) % K;
#pragma unroll
        for (int r = 1; r < K; ++r)
#pragma unroll
            for (int d = 0; d < NC; ++d) {
                const double below = __shfl_up(x[d], STRIDE);
                const double n = lerp(s, t, below, x[d]);
                x[d] = e >= r ? n : x[d];
            }
    }
    template <int K, int STRIDE>
    __device__ void right_part(V *x, double s, double t) const
    {
        const int e = (lane / STRIDE) % K;
#pragma unroll
        for (int r = 1; r < K; ++r)
#pragma unroll
            for (int d = 0; d < NC; ++d) {
                const double above = __shfl_down(x[d], STRIDE);
                const double n = lerp(s, t, x[d], above);
                x[d] = e < K - r ? n : x[d];
            }
    }
    template <int N, class T>
    __device__ bool one_side(const V *x, T tau) const
    {
        constexpr unsigned long long live = N >= 64 ? ~0ull : ((1ull << (N & 63)) - 1ull);
        bool one = false;
#pragma unroll
        for (int d = 0; d < NC; ++d) {
            const unsigned long long pos = __ballot(above(x[d], tau)) & live, neg = __ballot(below(x[d], tau)) & live;
            one = one || pos == live || neg == live;
        }
        return one;
    }
    template <int K, int STRIDE>
    __device__ void eval_axis(const V &c, double x, V &val, V &der) const
    {
        const int e = (lane / STRIDE) % K;
        double b = c;
        const double s = 1.0 - x;
#pragma unroll
        for (int r = 1; r < K - 1; ++r) {
            const double above = __shfl_down(b, STRIDE);
            const double n = lerp(s, x, b, above);
            b = e < K - r ? n : b;
        }
        const double above = __shfl_down(b, STRIDE);
        der = (double)(K - 1) * (above - b);
        val = lerp(s, x, b, above);
    }
};
#endif

// ------------------------------------------------------------------------------------------ the steps, once for both waves
// One step down from a live box along AXIS: cur becomes its left live half, else its right live one (0, 1), or stays
// (-1: both halves are dropped).  The split axis is a compile-time one.
template <class W, int NC, int K0, int K1, int K2, int AXIS, class T>
BSK_HD int descend(const W &wave, typename W::V *cur, T tau)
{
    constexpr int K = AXIS == 0 ? K0 : (AXIS == 1 ? K1 : K2);
    constexpr int STRIDE = AXIS == 0 ? K1 * K2 : (AXIS == 1 ? K2 : 1);
    typename W::V half[NC];
#pragma unroll
    for (int d = 0; d < NC; ++d) half[d] = cur[d];
    wave.template left_part<K, STRIDE>(half, 0.5, 0.5);
    int child = 0;
    if (wave.template one_side<K0 * K1 * K2>(half, tau)) {
#pragma unroll
        for (int d = 0; d < NC; ++d) half[d] = cur[d];
        wave.template right_part<K, STRIDE>(half, 0.5, 0.5);
        child = wave.template one_side<K0 * K1 * K2>(half, tau) ? -1 : 1;
    }
    if (child >= 0) {
#pragma unroll
        for (int d = 0; d < NC; ++d) cur[d] = half[d];
    }
    return child;
}

// x on [lo, lo + w] of one axis: the right part at lo, then the left part at w / (1 - lo)
template <class W, int K, int STRIDE>
BSK_HD void restrict_axis(const W &wave, typename W::V *x, double lo, double w)
{
    wave.template right_part<K, STRIDE>(x, 1.0 - lo, lo);
    const double t = w / (1.0 - lo);
    wave.template left_part<K, STRIDE>(x, 1.0 - t, t);
}

}  // namespace bskwave3
