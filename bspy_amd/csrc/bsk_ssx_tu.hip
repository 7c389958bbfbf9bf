// Surface-surface intersection (bsk_ssx.hpp): the bsk_ssx_* entry points.  Like bsk_rays_tu.hip the family keeps no handle,
// and each x_host / x pair is one function of DEVICE: the checks, the dispatch, then the host loop over the lanes (the
// isolate one over the pairs on a HostWave) or the launch.
// Instantiations: ssx_search (count and emit, with and without the prefilter; the orders are arguments), ssx_isolate for
// KR, K1, K2 = 2 .. 4 and ssx_merge, on fp64 rows, on both sides.
#include <cstdint>

#include "bsk_host.hpp"
#include "bsk_ssx.hpp"

using namespace bskssx;

static thread_local const char *g_ssx_kernel = "";

static bsk_status check_side(const Side &s, const std::string &w)
{
    bsk_status st = bskpairs::check_surface(s.X, SSX_MAX_K, w);
    if (st != BSK_OK) return st;
    st = bskpairs::check_surface(s.Y, SSX_MAX_K, w);
    if (st != BSK_OK) return st;
    if (s.ax != 0 && s.ax != 1) return fail(BSK_ERR_INVALID, w + ": ax must be 0 or 1");
    if (s.G < 1 || s.G > 64) return fail(BSK_ERR_INVALID, w + ": G must be in [1, 64]");
    if ((double)(ncfix(s) * s.G + 1) * (double)ncrun(s) > 2.0e9) return fail(BSK_ERR_INVALID, w + ": more than 2e9 line segments");
    return BSK_OK;
}

template <bool DEVICE, bool EMIT>
static bsk_status search(const Side &s, Search a, int prefilter, hipStream_t st)
{
    const std::string who = std::string(EMIT ? "bsk_ssx_emit" : "bsk_ssx_count") + (DEVICE ? "" : "_host");
    bsk_status r = check_side(s, who);
    if (r != BSK_OK) return r;
    if (!a.boxes || !a.scale || (EMIT ? (!a.offset || !a.pair_seg || !a.pair_cell) : !a.partial)) return fail(BSK_ERR_INVALID, who + ": NULL argument");
    if (a.seg0 < 0 || a.nseg < 1 || a.seg0 + a.nseg > (ncfix(s) * s.G + 1) * ncrun(s))
        return fail(BSK_ERR_INVALID, who + ": the segments seg0 .. seg0 + nseg - 1 must be segments of the family");
    r = bskpairs::check_search(s.Y, a.chunk, EMIT, a.npairs, a.nchunks, who);
    if (r != BSK_OK) return r;
    r = with_bool(prefilter != 0, [&](auto pf) {
        constexpr bool PF = decltype(pf)::value;
        if constexpr (DEVICE) return launch_lanes<SSX_SEARCH_BLOCK>(ssx_search<PF, EMIT>, a.nseg, a.nchunks, st, s, a);
        else {
            for (long long ch = 0; ch < a.nchunks; ++ch)
                for (long long lane = 0; lane < a.nseg; ++lane) search_lane<PF, EMIT>(s, a, ch, lane);
            return BSK_OK;
        }
    });
    if (r == BSK_OK) g_ssx_kernel = EMIT ? (DEVICE ? "ssx_emit" : "host ssx_emit") : (DEVICE ? "ssx_count" : "host ssx_count");
    return r;
}

template <bool DEVICE>
static bsk_status isolate(const Side &s, const Isolate &a, hipStream_t st)
{
    const std::string who = DEVICE ? "bsk_ssx_isolate" : "bsk_ssx_isolate_host";
    bsk_status r = check_side(s, who);
    if (r != BSK_OK) return r;
    if (!a.brun || !a.by0 || !a.by1 || !a.scale || !a.pair_seg || !a.pair_cell || !a.roots || !a.near || !a.count || !a.status || !a.nodes)
        return fail(BSK_ERR_INVALID, who + ": NULL argument");
    if (a.npairs < 1) return fail(BSK_ERR_INVALID, who + ": npairs must be >= 1 (no pairs: no call)");
    // one workgroup a pair; the host twin keeps the bound of the launch
    if (a.npairs > 0x7fffffffLL) return fail(BSK_ERR_INVALID, who + ": more pairs than one launch takes (2^31 - 1)");
    r = with_range<2, SSX_MAX_K>(order_run(s), [&](auto kr) {
        return with_range<2, SSX_MAX_K>(s.Y.K0, [&](auto k1) {
            return with_range<2, SSX_MAX_K>(s.Y.K1, [&](auto k2) {
                constexpr int KR = decltype(kr)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
                if constexpr (DEVICE) return launch_lanes<SSX_WAVE>(ssx_isolate<KR, K1, K2>, a.npairs * SSX_WAVE, st, s, a);
                else {
                    const bskroots3::HostWave wave;
                    for (long long slot = 0; slot < a.npairs; ++slot) isolate_wave<bskroots3::HostWave, KR, K1, K2>(wave, s, a, slot);
                    return BSK_OK;
                }
            });
        });
    });
    if (r == BSK_OK) g_ssx_kernel = DEVICE ? "ssx_isolate" : "host ssx_isolate";
    return r;
}

template <bool DEVICE>
static bsk_status merge(const Merge &m, hipStream_t st)
{
    const std::string who = DEVICE ? "bsk_ssx_merge" : "bsk_ssx_merge_host";
    if (!m.roots || !m.brun || !m.by0 || !m.by1 || !m.pair_key || !m.which || !m.keep) return fail(BSK_ERR_INVALID, who + ": NULL argument");
    if (m.R < 6 || m.R > bskroots3::ROOTS3_MAX_SLOTS) return fail(BSK_ERR_INVALID, who + ": R must be min(6 (KR - 1)(K1 - 1)(K2 - 1), 32) of covered orders");
    if (m.ncrun < 1 || m.ncy0 < 1 || m.ncy1 < 1) return fail(BSK_ERR_INVALID, who + ": ncrun, ncy0 and ncy1 must be >= 1");
    if ((double)m.ncy0 * (double)m.ncy1 > 2.0e9) return fail(BSK_ERR_INVALID, who + ": array too large");
    if (m.npairs < 1) return fail(BSK_ERR_INVALID, who + ": npairs must be >= 1");
    if (m.nnear < 1 || m.nnear > m.npairs * m.R) return fail(BSK_ERR_INVALID, who + ": nnear must be in [1, npairs R] (no zero near a face: no call)");
    if constexpr (DEVICE) {
        const bsk_status r = launch_lanes<SSX_BLOCK>(ssx_merge, m.nnear, st, m);
        if (r != BSK_OK) return r;
    } else {
        for (long long lane = 0; lane < m.nnear; ++lane) merge_lane(m, lane);
    }
    g_ssx_kernel = DEVICE ? "ssx_merge" : "host ssx_merge";
    return BSK_OK;
}

#define SSX_SIDE_ARGS                                                                                                           \
    int KX0, int KX1, const double *rowsX, int64_t RX0, int64_t RX1, int64_t ncX0, int64_t ncX1, const int32_t *firstX0,          \
        const int32_t *firstX1, int KY0, int KY1, const double *rowsY, int64_t RY0, int64_t RY1, int64_t ncY0, int64_t ncY1,      \
        const int32_t *firstY0, const int32_t *firstY1, int ax, int64_t G
#define SSX_SIDE                                                                                                                \
    Side{Surface{KX0, KX1, rowsX, RX0, RX1, ncX0, ncX1, firstX0, firstX1}, Surface{KY0, KY1, rowsY, RY0, RY1, ncY0, ncY1, firstY0, firstY1}, ax, G}
#define SSX_SEARCH_ARGS int64_t seg0, int64_t nseg, int64_t chunk, int prefilter, const double *boxes, const double *scale
#define SSX_ISOLATE_ARGS                                                                                                        \
    const double *breaks_run, const double *breaksY0, const double *breaksY1, const double *scale, const int32_t *pair_seg,      \
        const int32_t *pair_cell, int64_t npairs, double *roots, uint8_t *near, int32_t *count, uint8_t *status, int32_t *nodes
#define SSX_ISOLATE Isolate{breaks_run, breaksY0, breaksY1, scale, pair_seg, pair_cell, npairs, roots, near, count, status, nodes}
#define SSX_MERGE_ARGS                                                                                                          \
    int R, const double *roots, int64_t ncrun, int64_t ncY0, int64_t ncY1, const double *breaks_run, const double *breaksY0,     \
        const double *breaksY1, const int64_t *pair_key, int64_t npairs, const int64_t *which, int64_t nnear, uint8_t *keep
#define SSX_MERGE Merge{R, roots, ncrun, ncY0, ncY1, breaks_run, breaksY0, breaksY1, pair_key, npairs, which, nnear, keep}

extern "C" const char *bsk_ssx_last_kernel(void) { return g_ssx_kernel; }

extern "C" bsk_status bsk_ssx_count_host(SSX_SIDE_ARGS, SSX_SEARCH_ARGS, int32_t *partial)
{
    return search<false, false>(SSX_SIDE, Search{seg0, nseg, chunk, 0, boxes, scale, partial, nullptr, nullptr, nullptr, 0}, prefilter, nullptr);
}

extern "C" bsk_status bsk_ssx_count(SSX_SIDE_ARGS, SSX_SEARCH_ARGS, int32_t *partial, void *stream)
{
    return search<true, false>(SSX_SIDE, Search{seg0, nseg, chunk, 0, boxes, scale, partial, nullptr, nullptr, nullptr, 0}, prefilter,
                               static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_ssx_emit_host(SSX_SIDE_ARGS, SSX_SEARCH_ARGS, const int64_t *offset, int32_t *pair_seg, int32_t *pair_cell,
                                        int64_t npairs)
{
    return search<false, true>(SSX_SIDE, Search{seg0, nseg, chunk, 0, boxes, scale, nullptr, offset, pair_seg, pair_cell, npairs}, prefilter,
                               nullptr);
}

extern "C" bsk_status bsk_ssx_emit(SSX_SIDE_ARGS, SSX_SEARCH_ARGS, const int64_t *offset, int32_t *pair_seg, int32_t *pair_cell,
                                   int64_t npairs, void *stream)
{
    return search<true, true>(SSX_SIDE, Search{seg0, nseg, chunk, 0, boxes, scale, nullptr, offset, pair_seg, pair_cell, npairs}, prefilter,
                              static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_ssx_isolate_host(SSX_SIDE_ARGS, SSX_ISOLATE_ARGS) { return isolate<false>(SSX_SIDE, SSX_ISOLATE, nullptr); }

extern "C" bsk_status bsk_ssx_isolate(SSX_SIDE_ARGS, SSX_ISOLATE_ARGS, void *stream)
{
    return isolate<true>(SSX_SIDE, SSX_ISOLATE, static_cast<hipStream_t>(stream));
}

extern "C" bsk_status bsk_ssx_merge_host(SSX_MERGE_ARGS) { return merge<false>(SSX_MERGE, nullptr); }

extern "C" bsk_status bsk_ssx_merge(SSX_MERGE_ARGS, void *stream) { return merge<true>(SSX_MERGE, static_cast<hipStream_t>(stream)); }
