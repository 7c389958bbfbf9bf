// What the two pair-search families share (bsk_rays.hpp: rays against a surface; bsk_ssx.hpp: lattice lines of one surface
// against another): the table of one surface in Bezier form, the window of a cell, and the host-side checks of the table
// and of a count / emit launch.  The kernels' loops stay in their families.
#pragma once
#include <cstdint>
#include <string>

#include "bsk_host.hpp"
#include "bsk_roots.hpp"

namespace bskpairs {

// One surface: rows [3, R0, R1] in fp64, Bezier form on both axes; cell (i, j), flat index i nc1 + j, is the K0 x K1 window
// of the three components at first0[i], first1[j].  first0: [nc0]; first1: [nc1].
struct Surface {
    int K0, K1;
    const double *rows;
    long long R0, R1, nc0, nc1;
    const int32_t *first0, *first1;
};

// the window of cell (i, j); false: it leaves the rows.  K0, K1: the surface's orders, which bsk_rays.hpp passes as
// compile-time constants
BSK_HD bool window(const Surface &s, int K0, int K1, long long cell, const double *&p, long long &i, long long &j)
{
    if (cell < 0 || cell >= s.nc0 * s.nc1) return false;
    i = cell / s.nc1;
    j = cell - i * s.nc1;
    const long long f0 = s.first0[i], f1 = s.first1[j];
    if (f0 < 0 || f0 + K0 > s.R0 || f1 < 0 || f1 + K1 > s.R1) return false;
    p = s.rows + f0 * s.R1 + f1;
    return true;
}

inline bsk_status check_surface(const Surface &s, int max_k, const std::string &w)
{
    if (!s.rows || !s.first0 || !s.first1) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (s.K0 < 2 || s.K1 < 2) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    if (s.K0 > max_k || s.K1 > max_k) return fail(BSK_ERR_UNSUPPORTED, w + ": order above " + std::to_string(max_k));
    if (s.nc0 < 1 || s.nc1 < 1) return fail(BSK_ERR_INVALID, w + ": nc0 and nc1 must be >= 1");
    if (s.R0 < s.K0 || s.R1 < s.K1) return fail(BSK_ERR_INVALID, w + ": the rows must hold one cell (R0 >= K0, R1 >= K1)");
    if ((double)s.nc0 * (double)s.nc1 > 2.0e9 || 3.0 * (double)s.R0 * (double)s.R1 > 9.0e15)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

// A count (emit = false) or emit launch over the cells of `s` in chunks of `chunk`; nchunks receives their number.
inline bsk_status check_search(const Surface &s, long long chunk, bool emit, long long npairs, long long &nchunks, const std::string &w)
{
    if (chunk < 1) return fail(BSK_ERR_INVALID, w + ": chunk must be >= 1");
    if (emit && npairs < 1) return fail(BSK_ERR_INVALID, w + ": npairs must be >= 1 (no pairs: no call)");
    nchunks = (s.nc0 * s.nc1 + chunk - 1) / chunk;
    if (nchunks > 65535) return fail(BSK_ERR_INVALID, w + ": more than 65535 chunks");
    return BSK_OK;
}

}  // namespace bskpairs
