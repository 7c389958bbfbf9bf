// Ray-surface hits (bsk_rays.hpp): the bsk_rays_* entry points.  Like bsk_roots2_tu.hip the family keeps no handle, and
// each x_host / x pair is one function of DEVICE: the checks, the dispatch, then the host loop over the lanes or the launch.
// Instantiations: ray_boxes, ray_search (count and emit, with and without the prefilter), ray_isolate and ray_reduce (first
// and all) for K0, K1 = 2 .. 4 on fp64 rows, on both sides.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_rays.hpp"

using namespace bskrays;

static thread_local const char *g_rays_kernel = "";

constexpr int RAYS_MAX_K = 4;

static bsk_status check_rays(const Rays &r, const std::string &w)
{
    if (!r.origins || !r.dirs || !r.cmax) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (r.nrays < 1 || r.nrays > 2000000000ll) return fail(BSK_ERR_INVALID, w + ": nrays must be in [1, 2e9] (the driver walks the rays in passes)");
    return BSK_OK;
}

template <typename F>
static bsk_status by_orders(const Surface &s, F &&f)
{
    return with_range<2, RAYS_MAX_K>(s.K0, [&](auto k0) {
        return with_range<2, RAYS_MAX_K>(s.K1, [&](auto k1) { return f(k0, k1); });
    });
}

template <bool DEVICE>
static bsk_status boxes_of(const Surface &c, double *out, hipStream_t st)
{
    const std::string who = DEVICE ? "bsk_rays_boxes" : "bsk_rays_boxes_host";
    bsk_status s = bskpairs::check_surface(c, RAYS_MAX_K, who);
    if (s != BSK_OK) return s;
    if (!out) return fail(BSK_ERR_INVALID, who + ": NULL argument");
    const long long lanes = c.nc0 * c.nc1;
    s = by_orders(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE) return launch_lanes<RAYS_BLOCK>(ray_boxes<K0, K1>, lanes, st, c, out);
        else {
            for (long long cell = 0; cell < lanes; ++cell) boxes_lane<K0, K1>(c, cell, out);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_rays_kernel = DEVICE ? "ray_boxes" : "host ray_boxes";
    return s;
}

template <bool DEVICE, bool EMIT>
static bsk_status search(const Surface &c, const Rays &r, Search a, int prefilter, hipStream_t st)
{
    const std::string who = std::string(EMIT ? "bsk_rays_emit" : "bsk_rays_count") + (DEVICE ? "" : "_host");
    bsk_status s = bskpairs::check_surface(c, RAYS_MAX_K, who);
    if (s != BSK_OK) return s;
    s = check_rays(r, who);
    if (s != BSK_OK) return s;
    if (!a.boxes || (EMIT ? (!a.offset || !a.pair_ray || !a.pair_cell) : (!a.partial || !a.skipped)))
        return fail(BSK_ERR_INVALID, who + ": NULL argument");
    s = bskpairs::check_search(c, a.chunk, EMIT, a.npairs, a.nchunks, who);
    if (s != BSK_OK) return s;
    s = by_orders(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        return with_bool(prefilter != 0, [&](auto pf) {
            constexpr bool PF = decltype(pf)::value;
            if constexpr (DEVICE) return launch_lanes<RAYS_BLOCK>(ray_search<K0, K1, PF, EMIT>, r.nrays, a.nchunks, st, c, r, a);
            else {
                for (long long ch = 0; ch < a.nchunks; ++ch)
                    for (long long ray = 0; ray < r.nrays; ++ray) search_lane<K0, K1, PF, EMIT>(c, r, a, ch, ray);
                return BSK_OK;
            }
        });
    });
    if (s == BSK_OK) g_rays_kernel = EMIT ? (DEVICE ? "ray_emit" : "host ray_emit") : (DEVICE ? "ray_count" : "host ray_count");
    return s;
}

template <bool DEVICE>
static bsk_status isolate(const Surface &c, const Rays &r, const Isolate &a, hipStream_t st)
{
    const std::string who = DEVICE ? "bsk_rays_isolate" : "bsk_rays_isolate_host";
    bsk_status s = bskpairs::check_surface(c, RAYS_MAX_K, who);
    if (s != BSK_OK) return s;
    s = check_rays(r, who);
    if (s != BSK_OK) return s;
    if (!a.breaks0 || !a.breaks1 || !a.pair_ray || !a.pair_cell || !a.roots || !a.near || !a.count || !a.status || !a.nodes)
        return fail(BSK_ERR_INVALID, who + ": NULL argument");
    if (a.npairs < 1) return fail(BSK_ERR_INVALID, who + ": npairs must be >= 1 (no pairs: no call)");
    s = by_orders(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        if constexpr (DEVICE) return launch_lanes<RAYS_ISOLATE_BLOCK>(ray_isolate<K0, K1>, a.npairs, st, c, r, a);
        else {
            for (long long lane = 0; lane < a.npairs; ++lane) isolate_lane<K0, K1>(c, r, a, lane);
            return BSK_OK;
        }
    });
    if (s == BSK_OK) g_rays_kernel = DEVICE ? "ray_isolate" : "host ray_isolate";
    return s;
}

template <bool DEVICE>
static bsk_status reduce(const Surface &c, const Rays &r, const Reduce &a, int all, hipStream_t st)
{
    const std::string who = DEVICE ? "bsk_rays_reduce" : "bsk_rays_reduce_host";
    bsk_status s = bskpairs::check_surface(c, RAYS_MAX_K, who);
    if (s != BSK_OK) return s;
    s = check_rays(r, who);
    if (s != BSK_OK) return s;
    if (!a.breaks0 || !a.breaks1 || !a.pstart || !a.pair_cell || !a.roots || !a.near || !a.count || !a.pstatus || !a.skipped || !a.uv ||
        !a.t || !a.cell || (all ? !a.hit_off : (!a.hits || !a.status)))
        return fail(BSK_ERR_INVALID, who + ": NULL argument");
    if (a.npairs < 1) return fail(BSK_ERR_INVALID, who + ": npairs must be >= 1 (no pairs: no call)");
    if (all && a.nhits < 1) return fail(BSK_ERR_INVALID, who + ": nhits must be >= 1 (no hits: no call)");
    s = by_orders(c, [&](auto k0, auto k1) {
        constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
        return with_bool(all != 0, [&](auto every) {
            constexpr bool ALL = decltype(every)::value;
            if constexpr (DEVICE) return launch_lanes<RAYS_BLOCK>(ray_reduce<K0, K1, ALL>, r.nrays, st, c, r, a);
            else {
                for (long long ray = 0; ray < r.nrays; ++ray) reduce_lane<K0, K1, ALL>(c, r, a, ray);
                return BSK_OK;
            }
        });
    });
    if (s == BSK_OK) g_rays_kernel = all ? (DEVICE ? "ray_reduce all" : "host ray_reduce all") : (DEVICE ? "ray_reduce" : "host ray_reduce");
    return s;
}

extern "C" const char *bsk_rays_last_kernel(void) { return g_rays_kernel; }

extern "C" bsk_status bsk_rays_boxes_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                          const int32_t *first0, const int32_t *first1,
                                          double *boxes)
{
    return boxes_of<false>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, boxes, nullptr);
}

extern "C" bsk_status bsk_rays_boxes(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                     const int32_t *first0, const int32_t *first1,
                                     double *boxes,
                                     void *stream)
{
    return boxes_of<true>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, boxes, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_rays_count_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                          const int32_t *first0, const int32_t *first1,
                                          const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                          double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                                          int32_t *partial, uint8_t *skipped)
{
    return search<false, false>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                                Search{tmin, tmax, chunk, 0, boxes, partial, skipped, nullptr, nullptr, nullptr, 0}, prefilter, nullptr);
}

extern "C" bsk_status bsk_rays_count(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                     const int32_t *first0, const int32_t *first1,
                                     const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                     double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                                     int32_t *partial, uint8_t *skipped,
                                     void *stream)
{
    return search<true, false>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                               Search{tmin, tmax, chunk, 0, boxes, partial, skipped, nullptr, nullptr, nullptr, 0}, prefilter, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_rays_emit_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                         const int32_t *first0, const int32_t *first1,
                                         const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                         double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                                         const int64_t *offset, int32_t *pair_ray, int32_t *pair_cell, int64_t npairs)
{
    return search<false, true>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                               Search{tmin, tmax, chunk, 0, boxes, nullptr, nullptr, offset, pair_ray, pair_cell, npairs}, prefilter, nullptr);
}

extern "C" bsk_status bsk_rays_emit(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                    const int32_t *first0, const int32_t *first1,
                                    const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                    double tmin, double tmax, int64_t chunk, int prefilter, const double *boxes,
                                    const int64_t *offset, int32_t *pair_ray, int32_t *pair_cell, int64_t npairs,
                                    void *stream)
{
    return search<true, true>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                              Search{tmin, tmax, chunk, 0, boxes, nullptr, nullptr, offset, pair_ray, pair_cell, npairs}, prefilter, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_rays_isolate_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                            const int32_t *first0, const int32_t *first1,
                                            const double *breaks0, const double *breaks1,
                                            const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                            const int32_t *pair_ray, const int32_t *pair_cell, int64_t npairs, double *roots, uint8_t *near,
                                            int32_t *count, uint8_t *status, int32_t *nodes)
{
    return isolate<false>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                          Isolate{breaks0, breaks1, pair_ray, pair_cell, npairs, roots, near, count, status, nodes}, nullptr);
}

extern "C" bsk_status bsk_rays_isolate(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                       const int32_t *first0, const int32_t *first1,
                                       const double *breaks0, const double *breaks1,
                                       const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                       const int32_t *pair_ray, const int32_t *pair_cell, int64_t npairs, double *roots, uint8_t *near,
                                       int32_t *count, uint8_t *status, int32_t *nodes,
                                       void *stream)
{
    return isolate<true>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                         Isolate{breaks0, breaks1, pair_ray, pair_cell, npairs, roots, near, count, status, nodes}, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_rays_reduce_host(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                           const int32_t *first0, const int32_t *first1,
                                           const double *breaks0, const double *breaks1,
                                           const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                           double tmin, double tmax, const int64_t *pstart, const int32_t *pair_cell, int64_t npairs,
                                           const double *roots, const uint8_t *near, const int32_t *count, const uint8_t *pstatus,
                                           const uint8_t *skipped, int all, const int64_t *hit_off, int64_t nhits, double *uv, double *t,
                                           int32_t *cell, int32_t *hits, uint8_t *status)
{
    return reduce<false>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                         Reduce{breaks0, breaks1, tmin, tmax, pstart, pair_cell, npairs, roots, near, count, pstatus, skipped, hit_off, nhits, uv, t, cell,
                                 hits, status}, all, nullptr);
}

extern "C" bsk_status bsk_rays_reduce(int K0, int K1, const double *rows, int64_t R0, int64_t R1, int64_t nc0, int64_t nc1,
                                      const int32_t *first0, const int32_t *first1,
                                      const double *breaks0, const double *breaks1,
                                      const double *cmax, const double *origins, const double *dirs, int64_t nrays,
                                      double tmin, double tmax, const int64_t *pstart, const int32_t *pair_cell, int64_t npairs,
                                      const double *roots, const uint8_t *near, const int32_t *count, const uint8_t *pstatus,
                                      const uint8_t *skipped, int all, const int64_t *hit_off, int64_t nhits, double *uv, double *t,
                                      int32_t *cell, int32_t *hits, uint8_t *status,
                                      void *stream)
{
    return reduce<true>(Surface{K0, K1, rows, R0, R1, nc0, nc1, first0, first1}, Rays{origins, dirs, cmax, nrays},
                        Reduce{breaks0, breaks1, tmin, tmax, pstart, pair_cell, npairs, roots, near, count, pstatus, skipped, hit_off, nhits, uv, t, cell,
                                 hits, status}, all, static_cast<hipStream_t>(stream));
}
