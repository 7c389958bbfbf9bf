// The bivariate tensor-product Bernstein box of NC components, c[(d * K0 + i) * K1 + j]: its halves along an axis and its
// restriction to a sub-box.  bsk_roots2.hpp walks boxes of two components (and bsk_rays.hpp through it), bsk_contour.hpp
// of one; each keeps its own descend, sign predicate and walk.  The arithmetic is bsk_roots.hpp's (fp64, no contraction).
#pragma once
#include "bsk_roots.hpp"

#pragma clang fp contract(off)

namespace bskbox2 {

// the halves of cur along AXIS (a compile-time axis: the two axes never store to one array under a run-time index)
template <int NC, int K0, int K1, int AXIS>
BSK_HD void halve(const double *cur, double *left, double *right)
{
    constexpr int K = AXIS == 0 ? K0 : K1, LINES = AXIS == 0 ? K1 : K0;
    constexpr int STEP = AXIS == 0 ? K1 : 1, LINE = AXIS == 0 ? 1 : K1;
#pragma unroll
    for (int d = 0; d < NC; ++d)
#pragma unroll
        for (int n = 0; n < LINES; ++n) {
            const int base = d * K0 * K1 + n * LINE;
            double line[K], l[K], r[K];
#pragma unroll
            for (int e = 0; e < K; ++e) line[e] = cur[base + e * STEP];
            bskroots::split<K>(line, 0.5, l, r);
#pragma unroll
            for (int e = 0; e < K; ++e) {
                left[base + e * STEP] = l[e];
                right[base + e * STEP] = r[e];
            }
        }
}

// one component c on the box [lo0, lo0 + w0] x [lo1, lo1 + w1]: every column, then every row (always inline: the host
// build then has one restrict_box with all components in it, as it had)
template <int K0, int K1>
BSK_HD __attribute__((always_inline)) void restrict_component(const double *c, double lo0, double w0, double lo1, double w1, double *out)
{
#pragma unroll
    for (int j = 0; j < K1; ++j) {
        double col[K0], res[K0];
#pragma unroll
        for (int i = 0; i < K0; ++i) col[i] = c[i * K1 + j];
        bskroots::restrict_to<K0>(col, lo0, w0, res);
#pragma unroll
        for (int i = 0; i < K0; ++i) out[i * K1 + j] = res[i];
    }
#pragma unroll
    for (int i = 0; i < K0; ++i) {
        double row[K1], res[K1];
#pragma unroll
        for (int j = 0; j < K1; ++j) row[j] = out[i * K1 + j];
        bskroots::restrict_to<K1>(row, lo1, w1, res);
#pragma unroll
        for (int j = 0; j < K1; ++j) out[i * K1 + j] = res[j];
    }
}

// every component in turn (NC = 1 without a loop around it: that keeps bsk_contour.hpp's register allocation as it was)
template <int NC, int K0, int K1>
BSK_HD void restrict_box(const double *c, double lo0, double w0, double lo1, double w1, double *out)
{
    if constexpr (NC == 1) {
        restrict_component<K0, K1>(c, lo0, w0, lo1, w1, out);
    } else {
#pragma unroll
        for (int d = 0; d < NC; ++d) restrict_component<K0, K1>(c + d * K0 * K1, lo0, w0, lo1, w1, out + d * K0 * K1);
    }
}

}  // namespace bskbox2
