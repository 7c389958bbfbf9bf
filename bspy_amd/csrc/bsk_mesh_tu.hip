// Triangle meshes of parametric surfaces within a tolerance (bsk_mesh.hpp): the bsk_mesh_* entry points.  Like
// bsk_iso_tu.hip the family keeps no handle, and each x_host / x pair is one function of DEVICE: the checks, the dispatch,
// then the host loop over the lanes or the launch.
// Instantiations: mesh_bound for K0, K1 = 2 .. 4 (9), mesh_count and mesh_emit (1 each: they do not see the orders) and
// mesh_vertex for K0, K1 = 2 .. 4 with and without normals (18): 29 kernels; the host drivers run the same functions.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_mesh.hpp"

using namespace bskmesh;

static thread_local const char *g_mesh_kernel = "";

constexpr int MESH_MAX_K = 4;

struct MeshCall {
    int K0, K1;
    Net g;
};

static bsk_status check_call(const MeshCall &c, const char *who)
{
    const std::string w(who);
    if (!c.g.rows || !c.g.first0 || !c.g.first1) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (c.K0 < 2 || c.K1 < 2) return fail(BSK_ERR_INVALID, w + ": orders must be >= 2");
    if (c.K0 > MESH_MAX_K || c.K1 > MESH_MAX_K) return fail(BSK_ERR_UNSUPPORTED, w + ": order above " + std::to_string(MESH_MAX_K));
    if (c.g.ndep < 1 || c.g.ndep > MESH_MAX_DEP) return fail(BSK_ERR_INVALID, w + ": ndep must be in [1, 3]");
    if (c.g.nmem < 1 || c.g.nc0 < 1 || c.g.nc1 < 1) return fail(BSK_ERR_INVALID, w + ": nmem, nc0 and nc1 must be >= 1");
    if (c.g.R0 < c.K0 || c.g.R1 < c.K1) return fail(BSK_ERR_INVALID, w + ": the rows must hold one cell (R0 >= K0, R1 >= K1)");
    // a key holds 31 bits per axis, 11 of them below the cell
    if (c.g.nc0 >= (1LL << 20) || c.g.nc1 >= (1LL << 20)) return fail(BSK_ERR_INVALID, w + ": more than 2^20 - 1 cells per axis");
    if ((double)c.g.nmem * (double)c.g.nc0 * (double)c.g.nc1 > 0x1p40 || (double)c.g.nmem * 3.0 * (double)c.g.R0 * (double)c.g.R1 > 9.0e15)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    return BSK_OK;
}

static bsk_status check_quads(const Quads &q, long long start, long long n, long long nquads, const char *who)
{
    const std::string w(who);
    if (!q.qoff || !q.lev) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (q.nc0 < 1 || q.nc1 < 1 || q.ncells < 1 || q.ncells % (q.nc0 * q.nc1) != 0)
        return fail(BSK_ERR_INVALID, w + ": ncells must be a positive multiple of nc0 nc1");
    if (q.steps < 0 || q.steps > 62 || (q.steps < 62 && (1LL << q.steps) < q.ncells))
        return fail(BSK_ERR_INVALID, w + ": 2^steps must reach ncells");
    if (q.span < 1 || q.span > (1 << MESH_MAX_LEVEL)) return fail(BSK_ERR_INVALID, w + ": span must be in [1, 1024]");
    if (start < 0 || n < 1 || nquads < 1 || start > nquads - n) return fail(BSK_ERR_INVALID, w + ": the quads [start, start + n) must lie in [0, nquads)");
    if ((n + MESH_BLOCK - 1) / MESH_BLOCK > 0x7fffffffLL) return fail(BSK_ERR_INVALID, w + ": more quads than one launch takes");
    return BSK_OK;
}

template <typename F>
static bsk_status by_orders(const MeshCall &c, F &&f)
{
    return with_range<2, MESH_MAX_K>(c.K0, [&](auto k0) { return with_range<2, MESH_MAX_K>(c.K1, [&](auto k1) { return f(k0, k1); }); });
}

template <bool DEVICE>
static bsk_status bound(const MeshCall &c, double T, int max_level, double *Q, int32_t *lev, uint8_t *status, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_mesh_bound" : "bsk_mesh_bound_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    if (!Q || !lev || !status) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    if (!(T > 0.0) || !std::isfinite(T)) return fail(BSK_ERR_INVALID, std::string(who) + ": T must be finite and > 0");
    if (max_level < 0 || max_level > MESH_MAX_LEVEL) return fail(BSK_ERR_INVALID, std::string(who) + ": max_level must be in [0, 10]");
    const long long lanes = c.g.nmem * c.g.nc0 * c.g.nc1;
    s = by_orders(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE) return launch_lanes<MESH_BLOCK>(mesh_bound<K0, K1>, lanes, st, c.g, T, max_level, Q, lev, status);
        else {
            for (long long at = 0; at < lanes; ++at) bound_lane<K0, K1>(c.g, at, T, max_level, Q, lev, status);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_mesh_kernel = DEVICE ? "mesh_bound" : "host mesh_bound";
    return s;
}

template <bool DEVICE>
static bsk_status count(const Quads &q, long long start, long long n, long long nquads, int32_t *counts, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_mesh_count" : "bsk_mesh_count_host";
    bsk_status s = check_quads(q, start, n, nquads, who);
    if (s != BSK_OK) return s;
    if (!counts) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    if constexpr (DEVICE) {
        s = launch_lanes<MESH_BLOCK>(mesh_count, n, st, q, start, n, counts);
        if (s != BSK_OK) return s;
    } else {
        for (long long lane = 0; lane < n; ++lane) quad_lane<false>(q, start + lane, nullptr, 0, counts, nullptr);
    }
    g_mesh_kernel = DEVICE ? "mesh_count" : "host mesh_count";
    return BSK_OK;
}

template <bool DEVICE>
static bsk_status emit(const Quads &q, long long start, long long n, long long nquads, const int64_t *offsets, long long total, int64_t *tris,
                       hipStream_t st)
{
    const char *who = DEVICE ? "bsk_mesh_emit" : "bsk_mesh_emit_host";
    bsk_status s = check_quads(q, start, n, nquads, who);
    if (s != BSK_OK) return s;
    if (!offsets || !tris || total < 1) return fail(BSK_ERR_INVALID, std::string(who) + ": emit takes offsets, tris and total >= 1");
    if constexpr (DEVICE) {
        s = launch_lanes<MESH_BLOCK>(mesh_emit, n, st, q, start, n, offsets, total, tris);
        if (s != BSK_OK) return s;
    } else {
        for (long long lane = 0; lane < n; ++lane) quad_lane<true>(q, start + lane, offsets, total, nullptr, tris);
    }
    g_mesh_kernel = DEVICE ? "mesh_emit" : "host mesh_emit";
    return BSK_OK;
}

template <bool DEVICE>
static bsk_status vertex(const MeshCall &c, const double *breaks0, const double *breaks1, const int64_t *keys, const int64_t *members,
                         long long n, double *uv, double *xyz, double *normals, hipStream_t st)
{
    const char *who = DEVICE ? "bsk_mesh_vertex" : "bsk_mesh_vertex_host";
    bsk_status s = check_call(c, who);
    if (s != BSK_OK) return s;
    if (!breaks0 || !breaks1 || !keys || !members || !uv || !xyz) return fail(BSK_ERR_INVALID, std::string(who) + ": NULL argument");
    if (n < 1) return fail(BSK_ERR_INVALID, std::string(who) + ": n must be >= 1 (no vertices: no call)");
    if ((n + MESH_BLOCK - 1) / MESH_BLOCK > 0x7fffffffLL) return fail(BSK_ERR_INVALID, std::string(who) + ": too many vertices");
    if (normals && c.g.ndep != 3) return fail(BSK_ERR_INVALID, std::string(who) + ": normals take three dependent variables");
    s = by_orders(c, [&](auto k0, auto k1) {
        return with_bool(normals != nullptr, [&](auto nrm) {
            constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
            constexpr bool NORMALS = decltype(nrm)::value;
            if constexpr (DEVICE)
                return launch_lanes<MESH_BLOCK>(mesh_vertex<K0, K1, NORMALS>, n, st, c.g, breaks0, breaks1, keys, members, n, uv, xyz, normals);
            else {
                for (long long lane = 0; lane < n; ++lane) vertex_lane<K0, K1, NORMALS>(c.g, breaks0, breaks1, keys, members, lane, uv, xyz, normals);
                return BSK_OK;
            }
        });
    });
    if (s == BSK_OK) g_mesh_kernel = DEVICE ? "mesh_vertex" : "host mesh_vertex";
    return s;
}

#define MESH_NET_ARGS \
    int K0, int K1, const double *rows, int64_t nmem, int ndep, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1, const int32_t *first0, const int32_t *first1
#define MESH_CALL MeshCall{K0, K1, Net{rows, nmem, R0, R1, nc0, nc1, first0, first1, ndep}}
#define MESH_QUAD_ARGS const int64_t *qoff, int64_t ncells, int64_t nc0, int64_t nc1, const int32_t *lev, int steps, int span, int64_t start, int64_t n, int64_t nquads
#define MESH_QUADS Quads{qoff, ncells, nc0, nc1, lev, steps, span}
#define MESH_VERTEX_ARGS const double *breaks0, const double *breaks1, const int64_t *keys, const int64_t *members, int64_t n, double *uv, double *xyz, double *normals

extern "C" const char *bsk_mesh_last_kernel(void) { return g_mesh_kernel; }

extern "C" bsk_status bsk_mesh_bound_host(MESH_NET_ARGS, double T, int max_level, double *Q, int32_t *lev, uint8_t *status)
{
    return bound<false>(MESH_CALL, T, max_level, Q, lev, status, nullptr);
}

extern "C" bsk_status bsk_mesh_bound(MESH_NET_ARGS, double T, int max_level, double *Q, int32_t *lev, uint8_t *status, void *stream)
{
    return bound<true>(MESH_CALL, T, max_level, Q, lev, status, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_mesh_count_host(MESH_QUAD_ARGS, int32_t *counts) { return count<false>(MESH_QUADS, start, n, nquads, counts, nullptr); }

extern "C" bsk_status bsk_mesh_count(MESH_QUAD_ARGS, int32_t *counts, void *stream)
{
    return count<true>(MESH_QUADS, start, n, nquads, counts, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_mesh_emit_host(MESH_QUAD_ARGS, const int64_t *offsets, int64_t total, int64_t *tris)
{
    return emit<false>(MESH_QUADS, start, n, nquads, offsets, total, tris, nullptr);
}

extern "C" bsk_status bsk_mesh_emit(MESH_QUAD_ARGS, const int64_t *offsets, int64_t total, int64_t *tris, void *stream)
{
    return emit<true>(MESH_QUADS, start, n, nquads, offsets, total, tris, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_mesh_vertex_host(MESH_NET_ARGS, MESH_VERTEX_ARGS)
{
    return vertex<false>(MESH_CALL, breaks0, breaks1, keys, members, n, uv, xyz, normals, nullptr);
}

extern "C" bsk_status bsk_mesh_vertex(MESH_NET_ARGS, MESH_VERTEX_ARGS, void *stream)
{
    return vertex<true>(MESH_CALL, breaks0, breaks1, keys, members, n, uv, xyz, normals, static_cast<hipStream_t>(stream));
}
