// eval_slab2 (bsk_slab.hpp) in its own translation unit: 176 instantiations (fp32 / fp64 x one common order 1 - 6 or mixed
// orders up to 2 - 6 x nDep 1 - 4 x with / without derivative branches) compile beside bsk_gather_tu.hip instead of
// behind it.  Entry: slab2_any<T>.
#include "bsk_host.hpp"
#include "bsk_tile.hpp"
#include "bsk_gather.hpp"
#include "bsk_binned.hpp"
#include "bsk_slab.hpp"

// Surfaces whose table can be streamed through LDS once per chunk of 8192 points (bsk_slab.hpp): no global sort.
// (tools/mixed_small.py on the TomsNasty shape: a launch takes 53 us for any batch up to 1.2 M points - every slab staged by every
//  workgroup - against 14 - 34 us of the gather kernel up to 300 k points; even at 600 k: 54 against 65 us)
constexpr long long SLAB_MIN_POINTS = 1 << 19;

template <typename T, int O, bool MIXED>
static bsk_status launch_eval_slab2(bsk_spline s, const Params<T> &prm, long long n, T *out, long long ostride, const Wrt &w,
                                    hipStream_t st)
{
    if (s->nInd != 2 || s->nDep > 4 || !s->coef_aos || n < SLAB_MIN_POINTS) return BSK_ERR_UNSUPPORTED;
    if (s->variant == 7 || s->variant == 13 || s->variant == 14) return BSK_ERR_UNSUPPORTED;     // pinned to the other large-table paths
    const Desc<T> &d = desc_of<T>(s);
    const TileDesc<T> &td = tile_of<T>(s);
    if ((size_t)d.coef_len * sizeof(T) > SLAB_MAX_TABLE || s->ncoef[0] > 65535) return BSK_ERR_UNSUPPORTED;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    SlabPlan sp;
    size_t off = up16(sizeof(T) * (size_t)d.nk[1] * s->order[1]);
    sp.off_lut = (unsigned)off;
    off += up16(4 * (size_t)td.lut_len);
    sp.off_wcnt = (unsigned)off;
    off += up16(4 * (size_t)SLAB_WAVES * SLAB_MAX_PASS);
    sp.off_pstart = (unsigned)off;
    off += up16(4 * (size_t)(SLAB_MAX_PASS + 1) * (1 + SLAB_ROUND));   // pass starts of the chunk being ordered + of every chunk of the round
    sp.off_tab0 = (unsigned)off;
    const size_t lds_wg = s->lds_max;                             // one workgroup per CU
    if (off + 4096 > lds_wg) return BSK_ERR_UNSUPPORTED;
    // a pass of spp spans needs (spp + order0 - 1) table rows and order0 x (spp + order0) axis-table entries
    const size_t rowbytes = (size_t)s->ncoef[1] * s->nDep * sizeof(T), slicebytes = (size_t)s->order[0] * sizeof(T);
    const int S0 = s->ncoef[0] - s->order[0] + 1;
    const long long room = (long long)lds_wg - (long long)off - 256 - (long long)(s->order[0] - 1) * (long long)rowbytes -
                           (long long)s->order[0] * (long long)slicebytes;
    int spp = (int)std::min<long long>(room / (long long)(rowbytes + slicebytes), S0);
    if (spp < 1) return BSK_ERR_UNSUPPORTED;
    sp.npass = (S0 + spp - 1) / spp;
    if (sp.npass > SLAB_MAX_PASS) return BSK_ERR_UNSUPPORTED;
    spp = (S0 + sp.npass - 1) / sp.npass;                         // even passes
    sp.spp = spp;
    sp.rows = spp + s->order[0] - 1;
    sp.snk = spp + s->order[0];
    sp.off_slab = (unsigned)(off + up16((size_t)sp.snk * slicebytes));
    // behind the slab: O - 1 control points of zeros (a mixed-order window row reads up to pad1 of them past the slab's
    // last row; eval_slab2 zeroes them at kernel start).  At most 160 bytes: inside the 256 bytes `room` keeps free.
    sp.off_tail = (unsigned)(sp.off_slab + (size_t)sp.rows * rowbytes);
    sp.total = (unsigned)(sp.off_slab + up16((size_t)sp.rows * rowbytes + (size_t)(O - 1) * s->nDep * sizeof(T)));
    if (sp.total > lds_wg) return BSK_ERR_UNSUPPORTED;
    // chunk-private scratch of the order: batch position | span of every point
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return BSK_ERR_UNSUPPORTED;                               // the workspace may have to be (re)allocated
    }
    HIPCHK(s->bin_ws.reserve(4 * (size_t)n + 256));
    SlabPt<T> *spts = nullptr;                                    // (the points are read again from the caller's arrays)
    unsigned *sidx = reinterpret_cast<unsigned *>(s->bin_ws.p);
    // one slab (no ordering phase): chunks may be as short as 1024 points, so that a small batch still reaches two chunks per CU
    sp.chunk = SLAB_CHUNK;
    // (an LDS-resident table has eval_mixed as well: within 15 % either way up to 1 M points, this form 1.4 x faster at 10 M)
    if (sp.npass == 1 && s->aos_small && n < (1ll << 20)) return BSK_ERR_UNSUPPORTED;
    if (sp.npass == 1 && MIXED)
        sp.chunk = (int)std::max<long long>(1024, std::min<long long>(SLAB_CHUNK, ((n + 2 * s->num_cu - 1) / (2 * s->num_cu) + 1023) / 1024 * 1024));
    const long long nchunks = (n + sp.chunk - 1) / sp.chunk;
    int grid = persistent_grid(s, nchunks, 1);
    if (const char *g = getenv("BSK_SLAB_GRID")) grid = std::max(1, std::min(grid, atoi(g)));          // test knob: few workgroups = several rounds each
    static const int slab_dbg = getenv("BSK_SLAB_DBG") ? atoi(getenv("BSK_SLAB_DBG")) : 0;     // timing-only switches (tools/)
    const T *tab = static_cast<const T *>(s->tab);
    const T *aos = static_cast<const T *>(s->coef_aos);
    bool deriv = false;
    for (int iv = 0; iv < 2; ++iv) deriv |= w.w[iv] != 0;
    // DERIV false = plain evaluation: the recursions without their derivative branches (nDep <= 4: checked above)
    return with_range<1, 4>(s->nDep, [&](auto nd) {
        return with_bool(deriv, [&](auto dv) {
            return launch(s, "eval_slab2", eval_slab2<T, O, decltype(nd)::value, MIXED, decltype(dv)::value>, dim3(grid),
                          dim3(SLAB_BLOCK), sp.total, st, d, td, sp, tab, s->lut, aos, prm, n, 0ll, spts, sidx, out, ostride, w,
                          s->bad, slab_dbg);
        });
    });
}

// One common order 1..6, or mixed orders whose largest is 2..6 (`mixed` is the caller's: see gather_or_binned_any)
template <typename T>
bsk_status slab2_any(bsk_spline s, bool mixed, const Params<T> &prm, long long n, T *out, long long ostride, const Wrt &w,
                     hipStream_t st)
{
    const int omax = max_order(s);
    if (s->nInd != 2 || omax < (mixed ? 2 : 1) || omax > 6) return BSK_ERR_UNSUPPORTED;
    auto go = [&](auto o, auto mx) {
        return launch_eval_slab2<T, decltype(o)::value, decltype(mx)::value>(s, prm, n, out, ostride, w, st);
    };
    if (mixed) return with_range<2, 6>(omax, [&](auto o) { return go(o, std::true_type{}); });
    return with_range<1, 6>(omax, [&](auto o) { return go(o, std::false_type{}); });
}

template bsk_status slab2_any<float>(bsk_spline, bool, const Params<float> &, long long, float *, long long, const Wrt &, hipStream_t);
template bsk_status slab2_any<double>(bsk_spline, bool, const Params<double> &, long long, double *, long long, const Wrt &, hipStream_t);
