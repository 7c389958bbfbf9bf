// Products of splines (bsk_product.hpp): the bsk_product_* entry points.  A product map is host data and
// bsk_product_create makes no HIP call; its tables go to the device with the first device call on the handle, the plane
// table of a call with that call.
// Instantiations: band_product_line and band_product_tile, fp32 / fp64 x (k1, k2) of the last variable in 2 - 6.
#include <cstdint>
#include <cstring>

#include "bsk_host.hpp"
#include "bsk_product.hpp"

using namespace bskprod;

struct bsk_product_s {
    ProductMap map;
    int device = -1;                   // device the tables live on (-1: not uploaded)
    DevBuf d_f[2], d_g[2], d_w1, d_wt, d_terms;
    std::vector<int32_t> terms;        // what d_terms holds
    const char *last_kernel = "";
};

static bsk_status upload(bsk_product p)
{
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (p->device == dev) return BSK_OK;
    if (p->device >= 0) return fail(BSK_ERR_INVALID, "bsk_product: the map's tables live on another device");
    const ProductMap &m = p->map;
    for (int l = 0; l < m.M; ++l) {
        const ProductVar &q = m.v[l];
        HIPCHK(p->d_f[l].reserve(sizeof(int) * q.nOut));
        HIPCHK(p->d_g[l].reserve(sizeof(int) * q.nOut));
        HIPCHK(hipMemcpy(p->d_f[l].p, q.f.data(), sizeof(int) * q.nOut, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_g[l].p, q.g.data(), sizeof(int) * q.nOut, hipMemcpyHostToDevice));
    }
    // the last variable's weights transposed, Wt[a * k2 + b][j]: a lane's reads are coalesced
    const ProductVar &last = m.v[m.M - 1];
    const int kk = last.k1 * last.k2;
    std::vector<double> wt((size_t)kk * last.nOut);
    for (int j = 0; j < last.nOut; ++j)
        for (int i = 0; i < kk; ++i) wt[(size_t)i * last.nOut + j] = last.W[(size_t)j * kk + i];
    HIPCHK(p->d_wt.reserve(sizeof(double) * wt.size()));
    HIPCHK(hipMemcpy(p->d_wt.p, wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice));
    if (m.M == 2) {
        HIPCHK(p->d_w1.reserve(sizeof(double) * m.v[0].W.size()));
        HIPCHK(hipMemcpy(p->d_w1.p, m.v[0].W.data(), sizeof(double) * m.v[0].W.size(), hipMemcpyHostToDevice));
    }
    p->device = dev;
    return BSK_OK;
}

// The plane table of this call on the device.  The buffer may still be read by the handle's previous launch: it is
// rewritten only when the table differs, and then after the stream has drained.
static bsk_status upload_terms(bsk_product p, const int32_t *terms, size_t count, hipStream_t st)
{
    if (p->terms.size() == count && std::memcmp(p->terms.data(), terms, sizeof(int32_t) * count) == 0) return BSK_OK;
    HIPCHK(hipStreamSynchronize(st));
    p->terms.clear();
    HIPCHK(p->d_terms.reserve(sizeof(int32_t) * count));
    HIPCHK(hipMemcpy(p->d_terms.p, terms, sizeof(int32_t) * count, hipMemcpyHostToDevice));
    p->terms.assign(terms, terms + count);
    return BSK_OK;
}

static bsk_status check_call(bsk_product p, bsk_dtype dtype, const void *a, int64_t PA, const void *b, int64_t PB,
                             const int32_t *terms, int64_t P, int T, const void *out, const char *who)
{
    const std::string w(who);
    if (!p) return fail(BSK_ERR_INVALID, w + ": map is NULL");
    if (!a || !b || !terms || !out) return fail(BSK_ERR_INVALID, w + ": NULL argument");
    if (dtype != BSK_F32 && dtype != BSK_F64) return fail(BSK_ERR_INVALID, w + ": dtype must be BSK_F32 or BSK_F64");
    if (PA < 1 || PB < 1 || P < 1) return fail(BSK_ERR_INVALID, w + ": PA, PB and P must be >= 1");
    if (T < 1 || T > 64) return fail(BSK_ERR_INVALID, w + ": T must be in [1, 64]");
    double na = 1, nb = 1, no = 1;
    for (int l = 0; l < p->map.M; ++l) na *= p->map.v[l].nIn1, nb *= p->map.v[l].nIn2, no *= p->map.v[l].nOut;
    if (na * (double)PA > 9.0e15 || nb * (double)PB > 9.0e15 || no * (double)P > 9.0e15 || (double)P * T > 7.0e8)
        return fail(BSK_ERR_INVALID, w + ": array too large");
    for (int64_t i = 0; i < P * T; ++i) {
        const int32_t *e = terms + i * 3;
        if (e[0] < 0 || e[0] >= PA || e[1] < 0 || e[1] >= PB) return fail(BSK_ERR_INVALID, w + ": term names a plane outside a or b");
        if (e[2] != 1 && e[2] != -1) return fail(BSK_ERR_INVALID, w + ": a term's sign must be +1 or -1");
    }
    return BSK_OK;
}

template <typename T, int K1, int K2>
static bsk_status launch_line(bsk_product p, const T *a, const T *b, T *out, long long P, int Tn, hipStream_t st)
{
    const ProductVar &q = p->map.v[0];
    const int R = std::min(q.nOut, PROD_BLOCK);
    const int G = PROD_BLOCK / R;
    long long sa, sb;
    q.max_span(R, sa, sb);
    const long long per_plane = (long long)Tn * std::max(sa, sb);
    const int staged = per_plane <= LINE_LDS;
    // planes per workgroup: what LDS holds, at most 16 per plane group (the weights of a row are read once per workgroup)
    long long NP = staged ? std::min<long long>(LINE_LDS / per_plane, 16LL * G) : G;
    NP = std::max<long long>(1, std::min(NP, P));
    const long long tiles = (q.nOut + R - 1) / R, blocks = (P + NP - 1) / NP;
    if ((double)tiles * (double)blocks > 2147483647.0) return fail(BSK_ERR_INVALID, "bsk_product_apply: array too large for one launch");
    hipLaunchKernelGGL((band_product_line<T, K1, K2>), dim3((unsigned)(tiles * blocks)), dim3(PROD_BLOCK), 0, st, a, b, out,
                       static_cast<const int *>(p->d_f[0].p), static_cast<const int *>(p->d_g[0].p),
                       static_cast<const double *>(p->d_wt.p), static_cast<const int *>(p->d_terms.p), q.nIn1, q.nIn2, q.nOut, P, Tn,
                       R, (int)NP, tiles, staged);
    HIPCHK(hipGetLastError());
    p->last_kernel = "band_product_line";
    return BSK_OK;
}

template <typename T, int K1V, int K2V>
static bsk_status launch_tile(bsk_product p, const T *a, const T *b, T *out, long long P, int Tn, hipStream_t st)
{
    const ProductVar &u = p->map.v[0], &v = p->map.v[1];
    long long ua, ub, va, vb;
    u.max_span(TILE_R1, ua, ub);
    v.max_span(TILE_R2, va, vb);
    TileArgs q;
    q.f1 = static_cast<const int *>(p->d_f[0].p), q.g1 = static_cast<const int *>(p->d_g[0].p);
    q.f2 = static_cast<const int *>(p->d_f[1].p), q.g2 = static_cast<const int *>(p->d_g[1].p);
    q.w1 = static_cast<const double *>(p->d_w1.p), q.wt2 = static_cast<const double *>(p->d_wt.p);
    q.terms = static_cast<const int *>(p->d_terms.p);
    q.n1 = u.nIn1, q.n2 = v.nIn1, q.m1 = u.nIn2, q.m2 = v.nIn2, q.N1 = u.nOut, q.N2 = v.nOut;
    q.k1u = u.k1, q.k2u = u.k2, q.Tn = Tn;
    q.tiles1 = (u.nOut + TILE_R1 - 1) / TILE_R1, q.tiles2 = (v.nOut + TILE_R2 - 1) / TILE_R2;
    q.staged = ua * va <= TILE_LDS && ub * vb <= TILE_LDS;
    if ((double)q.tiles1 * (double)q.tiles2 * (double)P > 2147483647.0)
        return fail(BSK_ERR_INVALID, "bsk_product_apply: array too large for one launch");
    hipLaunchKernelGGL((band_product_tile<T, K1V, K2V>), dim3((unsigned)(q.tiles1 * q.tiles2 * P)), dim3(PROD_BLOCK), 0, st, a, b, out, q);
    HIPCHK(hipGetLastError());
    p->last_kernel = "band_product_tile";
    return BSK_OK;
}

template <typename T>
static bsk_status run(bsk_product p, const T *a, const T *b, T *out, long long P, int Tn, hipStream_t st)
{
    const ProductVar &last = p->map.v[p->map.M - 1];
    const bool line = p->map.M == 1;
    return with_int<2, 3, 4, 5, 6>(last.k1, [&](auto k1) {
        return with_int<2, 3, 4, 5, 6>(last.k2, [&](auto k2) {
            constexpr int K1 = decltype(k1)::value, K2 = decltype(k2)::value;
            return line ? launch_line<T, K1, K2>(p, a, b, out, P, Tn, st) : launch_tile<T, K1, K2>(p, a, b, out, P, Tn, st);
        });
    });
}

extern "C" bsk_status bsk_product_create(int M, const int32_t *nIn1, const int32_t *nIn2, const int32_t *nOut, const int32_t *k1,
                                         const int32_t *k2, const int32_t *const *f, const int32_t *const *g,
                                         const double *const *W, bsk_product *out)
{
    if (!nIn1 || !nIn2 || !nOut || !k1 || !k2 || !f || !g || !W || !out) return fail(BSK_ERR_INVALID, "NULL argument");
    if (M < 1 || M > PROD_MAXM) return fail(BSK_ERR_UNSUPPORTED, "bsk_product_create: M must be in [1, 3]");
    for (int l = 0; l < M; ++l) {
        if (!f[l] || !g[l] || !W[l]) return fail(BSK_ERR_INVALID, "NULL argument");
        if (k1[l] < 1 || k1[l] > MAXO || k2[l] < 1 || k2[l] > MAXO)
            return fail(BSK_ERR_UNSUPPORTED, "bsk_product_create: orders must be in [1, BSK_MAX_ORDER]");
        if (nIn1[l] < k1[l] || nIn1[l] > (1 << 26) || nIn2[l] < k2[l] || nIn2[l] > (1 << 26))
            return fail(BSK_ERR_INVALID, "bsk_product_create: nIn must be in [order, 2^26]");
        if (nOut[l] < 1 || nOut[l] > (1 << 26)) return fail(BSK_ERR_INVALID, "bsk_product_create: nOut must be in [1, 2^26]");
        for (int j = 0; j < nOut[l]; ++j) {
            if (f[l][j] < 0 || f[l][j] > nIn1[l] - k1[l] || g[l][j] < 0 || g[l][j] > nIn2[l] - k2[l])
                return fail(BSK_ERR_INVALID, "bsk_product_create: first column outside [0, nIn - order]");
            if (j && (f[l][j] < f[l][j - 1] || g[l][j] < g[l][j - 1]))
                return fail(BSK_ERR_INVALID, "bsk_product_create: first columns must be non-decreasing");
        }
        for (size_t i = 0; i < (size_t)nOut[l] * k1[l] * k2[l]; ++i)
            if (!std::isfinite(W[l][i])) return fail(BSK_ERR_INVALID, "bsk_product_create: weight is not finite");
    }
    bsk_product p = new bsk_product_s;
    p->map.M = M;
    for (int l = 0; l < M; ++l) {
        ProductVar &q = p->map.v[l];
        q.nIn1 = nIn1[l], q.nIn2 = nIn2[l], q.nOut = nOut[l], q.k1 = k1[l], q.k2 = k2[l];
        q.f.assign(f[l], f[l] + nOut[l]);
        q.g.assign(g[l], g[l] + nOut[l]);
        q.W.assign(W[l], W[l] + (size_t)nOut[l] * k1[l] * k2[l]);
    }
    *out = p;
    return BSK_OK;
}

extern "C" bsk_status bsk_product_destroy(bsk_product p)
{
    if (!p) return BSK_OK;
    for (int l = 0; l < 2; ++l) p->d_f[l].release(), p->d_g[l].release();
    p->d_w1.release();
    p->d_wt.release();
    p->d_terms.release();
    delete p;
    return BSK_OK;
}

extern "C" const char *bsk_product_last_kernel(bsk_product p) { return p ? p->last_kernel : ""; }

extern "C" bsk_status bsk_product_apply_host(bsk_product p, bsk_dtype dtype, const void *a, int64_t PA, const void *b, int64_t PB,
                                             const int32_t *terms, int64_t P, int T, void *out)
{
    bsk_status s = check_call(p, dtype, a, PA, b, PB, terms, P, T, out, "bsk_product_apply_host");
    if (s != BSK_OK) return s;
    if (dtype == BSK_F32) p->map.apply_host(static_cast<const float *>(a), static_cast<const float *>(b), terms, P, T, static_cast<float *>(out));
    else p->map.apply_host(static_cast<const double *>(a), static_cast<const double *>(b), terms, P, T, static_cast<double *>(out));
    p->last_kernel = "host product";
    return BSK_OK;
}

extern "C" bsk_status bsk_product_apply(bsk_product p, bsk_dtype dtype, const void *a, int64_t PA, const void *b, int64_t PB,
                                        const int32_t *terms, int64_t P, int T, void *out, void *stream)
{
    bsk_status s = check_call(p, dtype, a, PA, b, PB, terms, P, T, out, "bsk_product_apply");
    if (s != BSK_OK) return s;
    if (p->map.M > 2) return fail(BSK_ERR_UNSUPPORTED, "bsk_product_apply: M > 2 is applied by bsk_product_apply_host");
    for (int l = 0; l < p->map.M; ++l) {
        const ProductVar &q = p->map.v[l];
        if (q.k1 < PROD_KMIN || q.k1 > PROD_KMAX || q.k2 < PROD_KMIN || q.k2 > PROD_KMAX)
            return fail(BSK_ERR_UNSUPPORTED, "bsk_product_apply: orders outside [2, 6] are applied by bsk_product_apply_host");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = upload(p);
    if (s != BSK_OK) return s;
    s = upload_terms(p, terms, (size_t)P * T * 3, st);
    if (s != BSK_OK) return s;
    return dtype == BSK_F32 ? run<float>(p, static_cast<const float *>(a), static_cast<const float *>(b), static_cast<float *>(out), P, T, st)
                            : run<double>(p, static_cast<const double *>(a), static_cast<const double *>(b), static_cast<double *>(out), P, T, st);
}
