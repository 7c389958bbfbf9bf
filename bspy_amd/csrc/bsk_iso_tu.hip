// Level surfaces of scalar splines in three variables (bsk_iso.hpp): the bsk_iso_* entry points.  Like bsk_contour_tu.hip
// the family keeps no handle, and each x_host / x pair is one function of DEVICE: the checks, the dispatch, then the host
// loop over the lanes (the waves of iso_walk on a HostWave) or the launch.
// Instantiations: iso_flag, iso_walk and iso_leaf (count and emit) and iso_vertex for K0, K1, K2 = 2 .. 4 on fp64 rows; the
// host drivers run the same functions for the same orders.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_iso.hpp"

using namespace bskiso;

static thread_local const char *g_iso_kernel = "";

constexpr int ISO_MAX_K = 4;

struct IsoCall {
    int K0, K1, K2;
    Grid g;
};

struct IsoWalk {
    const int64_t *cand;
    long long ncand;
    int depth, split, emit;
    const int64_t *offsets;
    long long total;
    int32_t *counts;
    int64_t *leaves;
};

struct IsoLeaf {
    const int64_t *leaves;
    long long nleaves;
    int depth, emit;
    const int64_t *offsets;
    long long total;
    int32_t *counts;
    uint8_t *status;
    int64_t *tris;
};

static bsk_status check_call(const IsoCall &c, const char *who)
{
    const std::string w(who);
    if (!c.g.rows || !c.g.first0 || !c.g.first1 || !c.g.first2 || !c.g.scale) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.K0 < 2 || c.K1 < 2 || c.K2 < 2) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    if (c.K0 > ISO_MAX_K || c.K1 > ISO_MAX_K || c.K2 > ISO_MAX_K)
        return fail(BSK_ERR_UNSUPPORTED, w + ": order above " + std::to_string(ISO_MAX_K) + " (one wave holds 64 coefficients)");
    if (c.g.nfields < 1 || c.g.nrows < 1 || c.g.nc0 < 1 || c.g.nc1 < 1 || c.g.nc2 < 1)
        return fail(BSK_ERR_INVALID, w + ": nfields, nrows, nc0, nc1 and nc2 must be >= 1");
    if (c.g.levels ? c.g.nrows != 1 : c.g.nrows != c.g.nfields)
        return fail(BSK_ERR_INVALID, w + ": the rows hold one field with levels and nfields fields without");
    if (c.g.R0 < c.K0 || c.g.R1 < c.K1 || c.g.R2 < c.K2)
        return fail(BSK_ERR_INVALID, w + ": the rows must hold one cell (R0 >= K0, R1 >= K1, R2 >= K2)");
    // a flat leaf index, and so a key, must fit 62 bits at depth 6: fields x cells x 2^18 x 2^3 x (the nodes' one more per axis)
    if ((double)c.g.nfields * (double)(c.g.nc0 + 1) * (double)(c.g.nc1 + 1) * (double)(c.g.nc2 + 1) > 0x1p40 ||
        (double)c.g.nrows * (double)c.g.R0 * (double)c.g.R1 * (double)c.g.R2 > 9.0e15)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

static bsk_status check_depth(int depth, const char *who)
{
    if (depth < 0 || depth > ISO_MAX_DEPTH) return fail(BSK_ERR_INVALID, std::string(who) + ": depth must be in [0, 6]");
    return BSK_OK;
}

static bsk_status check_walk(const IsoCall &c, const IsoWalk &m, const char *who)
{
    const std::string w(who);
    bsk_status s = check_depth(m.depth, who);
    if (s != BSK_OK) return s;
    if (!m.cand) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (m.split < 0 || m.split > m.depth) return fail(BSK_ERR_INVALID, w + ": the split level must be in [0, depth]");
    if (m.ncand < 1) return fail(BSK_ERR_INVALID, w + ": ncand must be >= 1 (no candidates: no call)");
    if (m.ncand > c.g.nfields * c.g.nc0 * c.g.nc1 * c.g.nc2) return fail(BSK_ERR_INVALID, w + ": more candidates than cells");
    // one workgroup a wave; the host twin keeps the bound of the launch
    if ((m.ncand << (3 * m.split)) > 0x7fffffffLL) return fail(BSK_ERR_INVALID, w + ": more waves than one launch takes (2^31 - 1)");
    if (m.emit ? (!m.offsets || !m.leaves || m.total < 1) : !m.counts)
        return fail(BSK_ERR_INVALID, w + (m.emit ? ": emit takes offsets, leaves and total >= 1 (no leaves: no call)" : ": count takes counts"));
    return BSK_OK;
}

static bsk_status check_leaf(const IsoLeaf &m, const char *who)
{
    const std::string w(who);
    bsk_status s = check_depth(m.depth, who);
    if (s != BSK_OK) return s;
    if (!m.leaves) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (m.nleaves < 1) return fail(BSK_ERR_INVALID, w + ": nleaves must be >= 1 (no leaves: no call)");
    if ((m.nleaves + ISO_BLOCK - 1) / ISO_BLOCK > 0x7fffffffLL) return fail(BSK_ERR_INVALID, w + ": too many leaves");
    if (m.emit ? (!m.offsets || !m.tris || m.total < 1) : (!m.counts || !m.status))
        return fail(BSK_ERR_INVALID, w + (m.emit ? ": emit takes offsets, tris and total >= 1 (no triangles: no call)" : ": count takes counts and status"));
    return BSK_OK;
}

// f(<K0>, <K1>, <K2>) behind check_call
template <typename F>
static bsk_status by_orders(const IsoCall &c, F &&f)
{
    return with_range<2, ISO_MAX_K>(c.K0, [&](auto k0) {
        return with_range<2, ISO_MAX_K>(c.K1, [&](auto k1) {
            return with_range<2, ISO_MAX_K>(c.K2, [&](auto k2) { return f(k0, k1, k2); });
        });
    });
}

template <bool DEVICE>
static bsk_status flag(const IsoCall &c, uint8_t *cand, uint8_t *zero, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_iso_flag" : "bsk_iso_flag_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    if (!cand || !zero) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    const long long lanes = c.g.nfields * c.g.nc0 * c.g.nc1 * c.g.nc2;
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
        if constexpr (DEVICE) return launch_lanes<ISO_BLOCK>(iso_flag<K0, K1, K2>, lanes, st, c.g, cand, zero);
        else {
            for (long long at = 0; at < lanes; ++at) flag_lane<K0, K1, K2>(c.g, at, cand, zero);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_iso_kernel = DEVICE ? "iso_flag" : "host iso_flag";
    return s;
}

template <bool DEVICE>
static bsk_status walk(const IsoCall &c, const IsoWalk &m, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_iso_walk" : "bsk_iso_walk_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    s = check_walk(c, m, who);
    if (s != BSK_OK) return s;
    const long long waves = m.ncand << (3 * m.split);
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        return with_bool(m.emit != 0, [&](auto emit) {
            constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
            constexpr bool EMIT = decltype(emit)::value;
            if constexpr (DEVICE)            // one wave a workgroup, one top box a wave
                return launch_lanes<ISO_WAVE>(iso_walk<K0, K1, K2, EMIT>, waves * ISO_WAVE, st, c.g, m.cand, m.ncand, m.depth, m.split,
                                              m.offsets, m.total, m.counts, m.leaves);
            else {
                const HostWave wave;
                for (long long slot = 0; slot < waves; ++slot)
                    walk_wave<HostWave, K0, K1, K2, EMIT>(wave, c.g, m.cand, m.ncand, m.depth, m.split, slot, m.offsets, m.total, m.counts,
                                                          m.leaves);
                return BSK_OK;
            }
        });
    });
    if (s != BSK_OK) return s;
    if constexpr (DEVICE) g_iso_kernel = m.emit ? "iso_walk emit" : "iso_walk count";
    else g_iso_kernel = m.emit ? "host iso_walk emit" : "host iso_walk count";
    return BSK_OK;
}

template <bool DEVICE>
static bsk_status leaf(const IsoCall &c, const IsoLeaf &m, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_iso_leaf" : "bsk_iso_leaf_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    s = check_leaf(m, who);
    if (s != BSK_OK) return s;
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        return with_bool(m.emit != 0, [&](auto emit) {
            constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
            constexpr bool EMIT = decltype(emit)::value;
            if constexpr (DEVICE)
                return launch_lanes<ISO_BLOCK>(iso_leaf<K0, K1, K2, EMIT>, m.nleaves, st, c.g, m.leaves, m.nleaves, m.depth, m.offsets, m.total,
                                               m.counts, m.status, m.tris);
            else {
                for (long long lane = 0; lane < m.nleaves; ++lane)
                    leaf_lane<K0, K1, K2, EMIT>(c.g, m.leaves, m.depth, lane, m.offsets, m.total, m.counts, m.status, m.tris);
                return BSK_OK;
            }
        });
    });
    if (s != BSK_OK) return s;
    if constexpr (DEVICE) g_iso_kernel = m.emit ? "iso_leaf emit" : "iso_leaf count";
    else g_iso_kernel = m.emit ? "host iso_leaf emit" : "host iso_leaf count";
    return BSK_OK;
}

template <bool DEVICE>
static bsk_status vertex(const IsoCall &c, const Breaks &br, const int64_t *keys, const int64_t *fields, long long n, int depth, double *xyz,
                         hipStream_t st)
{
    const char *who = DEVICE ? "bsk_iso_vertex" : "bsk_iso_vertex_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    s = check_depth(depth, who);
    if (s != BSK_OK) return s;
    if (!br.b0 || !br.b1 || !br.b2 || !keys || !fields || !xyz) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    if (n < 1) return fail(BSK_ERR_INVALID, std::string(who) + ": n must be >= 1 (no vertices: no call)");
    if ((n + ISO_BLOCK - 1) / ISO_BLOCK > 0x7fffffffLL) return fail(BSK_ERR_INVALID, std::string(who) + ": too many vertices");
    s = by_orders(c, [&](auto k0, auto k1, auto k2) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
        if constexpr (DEVICE) return launch_lanes<ISO_BLOCK>(iso_vertex<K0, K1, K2>, n, st, c.g, br, keys, fields, n, depth, xyz);
        else {
            for (long long lane = 0; lane < n; ++lane) vertex_lane<K0, K1, K2>(c.g, br, keys, fields, depth, lane, xyz);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_iso_kernel = DEVICE ? "iso_vertex" : "host iso_vertex";
    return s;
}

#define ISO_GRID_ARGS                                                                                                           \
    int K0, int K1, int K2, const double *rows, int64_t nrows, int64_t R0, int64_t R1, int64_t R2, int64_t nc0, int64_t nc1,     \
        int64_t nc2, const int32_t *first0, const int32_t *first1, const int32_t *first2, const double *levels, int64_t nfields, \
        const double *scale
#define ISO_CALL IsoCall{K0, K1, K2, Grid{rows, nrows, R0, R1, R2, nc0, nc1, nc2, first0, first1, first2, levels, nfields, scale}}
#define ISO_WALK_ARGS const int64_t *cand, int64_t ncand, int depth, int split, int emit, const int64_t *offsets, int64_t total, int32_t *counts, int64_t *leaves
#define ISO_LEAF_ARGS const int64_t *leaves, int64_t nleaves, int depth, int emit, const int64_t *offsets, int64_t total, int32_t *counts, uint8_t *status, int64_t *tris
#define ISO_VERTEX_ARGS const double *breaks0, const double *breaks1, const double *breaks2, const int64_t *keys, const int64_t *fields, int64_t n, int depth, double *xyz

extern "C" const char *bsk_iso_last_kernel(void) { return g_iso_kernel; }

extern "C" bsk_status bsk_iso_flag_host(ISO_GRID_ARGS, uint8_t *cand, uint8_t *zero) { return flag<false>(ISO_CALL, cand, zero, nullptr); }

extern "C" bsk_status bsk_iso_flag(ISO_GRID_ARGS, uint8_t *cand, uint8_t *zero, void *stream)
{
    return flag<true>(ISO_CALL, cand, zero, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_iso_walk_host(ISO_GRID_ARGS, ISO_WALK_ARGS)
{
    return walk<false>(ISO_CALL, IsoWalk{cand, ncand, depth, split, emit, offsets, total, counts, leaves}, nullptr);
}

extern "C" bsk_status bsk_iso_walk(ISO_GRID_ARGS, ISO_WALK_ARGS, void *stream)
{
    return walk<true>(ISO_CALL, IsoWalk{cand, ncand, depth, split, emit, offsets, total, counts, leaves}, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_iso_leaf_host(ISO_GRID_ARGS, ISO_LEAF_ARGS)
{
    return leaf<false>(ISO_CALL, IsoLeaf{leaves, nleaves, depth, emit, offsets, total, counts, status, tris}, nullptr);
}

extern "C" bsk_status bsk_iso_leaf(ISO_GRID_ARGS, ISO_LEAF_ARGS, void *stream)
{
    return leaf<true>(ISO_CALL, IsoLeaf{leaves, nleaves, depth, emit, offsets, total, counts, status, tris}, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_iso_vertex_host(ISO_GRID_ARGS, ISO_VERTEX_ARGS)
{
    return vertex<false>(ISO_CALL, Breaks{breaks0, breaks1, breaks2}, keys, fields, n, depth, xyz, nullptr);
}

extern "C" bsk_status bsk_iso_vertex(ISO_GRID_ARGS, ISO_VERTEX_ARGS, void *stream)
{
    return vertex<true>(ISO_CALL, Breaks{breaks0, breaks1, breaks2}, keys, fields, n, depth, xyz, static_cast<hipStream_t>(stream));
}
