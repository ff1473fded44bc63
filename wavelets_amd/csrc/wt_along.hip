// The 1-D transform along an axis of an array that is not its last one (wt_along): every pixel's light curve of a
// (T, H, W) movie, every pixel's spectrum of a (lambda, Y, X) raster.  The reference transforms a signal in its 1-D
// branch (watroo/wavelets.py:65-69 under :408-444); the signal unit (wt_signals) takes signals whose samples are
// contiguous, so such data had to be transposed on the host, twice.  This unit views the array as (O, N, I) - N
// samples I elements apart - and runs a tile of TI neighbouring signals per workgroup with the scales in LDS
// (wt_along_kernels.h): the device layout is the host layout, and every signal gets the bits of the signal unit.
// The host text it shares with the signal unit (wt_signals.hip) is wt_lines_host.h, the device text wt_signal_common.h.
//
// The LDS budget is the signal unit's 64 KiB (WT_SIGNALS_LDS_BYTES) for the two buffers of N x TI elements - CHOSEN,
// not a measured optimum: TI = the largest power of two with 2 * N * TI * itemsize <= 64 KiB, at most 256, and runs of
// at least 64 bytes (TI * itemsize >= 64), which admits N <= 512 in float32 and in float64.
//
// Device memory of a wt_along of `cap` signals of N samples:  in (cap * N) | medians (cap) | with planes:
// planes ((max_level + 1) * cap * N) | without: sum (cap * N) and the threshold table (cap * 2 * max_level doubles).
// A chunk (oc, N, ic), oc * ic <= cap, lies dense at the head of each; its planes are (level + 1, oc, N, ic).
#include <algorithm>
#include <cstring>
#include <vector>

#include "wt_lines_host.h"
#include "wt_along_kernels.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

struct wt_along {
    wt_ctx *ctx = nullptr;
    int64_t cap = 0;                     // signals
    int N = 0, TI = 0, lg = 0, family = WT_B3SPLINE, max_level = 0, itemsize = 4, with_planes = 1;
    int oc = 0, ic = 0;                  // the chunk of the last wt_along_upload
    int level = 0;                       // scales of the last wt_along_decompose (layout of `planes`)
    void *in = nullptr, *planes = nullptr, *sum = nullptr, *medians = nullptr;
    double *d_tab = nullptr;
    std::vector<double> h_tab;
    bool has_sum = false;
};

/* the tile rule: the largest power of two TI <= 256 with 2 * N * TI * itemsize <= WT_SIGNALS_LDS_BYTES; 0: none */
static int along_tile(int64_t N, int itemsize)
{
    if (N < 1 || N > WT_SIGNALS_LDS_BYTES) return 0;
    int ti = WT_ALONG_MAX_TILE;
    while (ti > 0 && 2 * N * ti * itemsize > WT_SIGNALS_LDS_BYTES) ti >>= 1;
    return ti;
}

/* host logic, no device needed: 1 when signals of n_samples samples, n_inner >= 2 elements apart, of `itemsize` bytes
 * (4: float, 8: double) of `family` over `level` scales run on a wt_along - a built-in family, 1 .. 24 scales, and a
 * tile with runs of at least 64 bytes within the LDS budget (n_samples <= 512 in either type); else 0 */
extern "C" int wt_along_ok(int family, int64_t n_samples, int64_t n_inner, int level, int itemsize)
{
    if (family != WT_B3SPLINE && family != WT_TRIANGLE) return 0;
    if (itemsize != 4 && itemsize != 8) return 0;
    if (level < 1 || level > 24 || n_samples < 1 || n_inner < 2 || n_inner > (int64_t)1 << 30) return 0;
    return (int64_t)along_tile(n_samples, itemsize) * itemsize >= WT_ALONG_MIN_RUN_BYTES ? 1 : 0;
}

static void along_free(wt_along *b, int *bad) { lines_free({b->in, b->planes, b->sum, b->medians, b->d_tab}, bad); }

extern "C" int wt_along_create(wt_ctx *ctx, int64_t n_signals, int n_samples, int family, int max_level, int itemsize, int with_planes, wt_along **out)
{
    WtGuard guard_(ctx);
    if (!ctx || !out) WT_FAIL("wt_along_create: null pointer");
    *out = nullptr;
    if (n_signals < 1 || n_signals > (int64_t)1 << 30) WT_FAIL("wt_along_create: %lld signals", (long long)n_signals);
    if (!wt_along_ok(family, n_samples, 2, max_level, itemsize))
        WT_FAIL("wt_along_create: %d samples of %d bytes, family %d, %d scales are not an axis stack (wt_along_ok)", n_samples, itemsize, family, max_level);
    wt_along *b = new wt_along;
    b->ctx = ctx;
    b->cap = n_signals;
    b->N = n_samples;
    b->TI = along_tile(n_samples, itemsize);
    while ((1 << b->lg) < b->TI) ++b->lg;
    b->family = family;
    b->max_level = max_level;
    b->itemsize = itemsize;
    b->with_planes = with_planes ? 1 : 0;
    const size_t block = (size_t)n_signals * n_samples * itemsize;
    hipError_t e = hipMalloc(&b->in, block);
    if (e == hipSuccess) e = hipMalloc(&b->medians, (size_t)n_signals * itemsize);
    if (with_planes) {
        if (e == hipSuccess) e = hipMalloc(&b->planes, block * (max_level + 1));
    } else {
        if (e == hipSuccess) e = hipMalloc(&b->sum, block);
        if (e == hipSuccess) e = hipMalloc((void **)&b->d_tab, (size_t)n_signals * 2 * max_level * sizeof(double));
    }
    return lines_created(b, out, e, "wt_along_create", along_free);
}

extern "C" int wt_along_destroy(wt_along *b) { return lines_destroy(b, "wt_along_destroy", along_free); }

extern "C" int wt_along_info(wt_along *b, int64_t *info)
{
    if (!b || !info) WT_FAIL("wt_along_info: null pointer");
    const int64_t v[8] = {b->cap, b->N, b->TI, b->family, b->max_level, b->itemsize, b->with_planes, b->level};
    memcpy(info, v, sizeof v);
    return 0;
}

// oc * N rows of ic elements between a host block (rows `pitch` elements apart) and the dense device block
static int along_copy(wt_along *b, void *dev, void *host, int64_t pitch, bool up)
{
    const size_t w = (size_t)b->ic * b->itemsize;
    return lines_copy(b->ctx->stream, dev, w, host, (size_t)pitch * b->itemsize, w, (size_t)b->oc * b->N, up);
}

static int along_loaded(const wt_along *b, const char *who)
{
    if (!b) WT_FAIL("%s: null axis stack", who);
    if (b->oc < 1) WT_FAIL("%s: no chunk in the stack (wt_along_upload first)", who);
    return 0;
}

extern "C" int wt_along_upload(wt_along *b, int n_outer, int n_inner, const void *host, int64_t pitch)
{
    if (!b || !host) WT_FAIL("wt_along_upload: null pointer");
    if (n_outer < 1 || n_inner < 1 || (int64_t)n_outer * n_inner > b->cap)
        WT_FAIL("wt_along_upload: a chunk of %d x %d signals outside the stack of %lld", n_outer, n_inner, (long long)b->cap);
    if (pitch < n_inner) WT_FAIL("wt_along_upload: pitch %lld below the %d elements of a row", (long long)pitch, n_inner);
    WtGuard guard_(b->ctx);
    b->oc = n_outer;
    b->ic = n_inner;
    b->level = 0;
    b->has_sum = false;
    WT_TRY(along_copy(b, b->in, const_cast<void *>(host), pitch, true));
    WT_HIP(hipStreamSynchronize(b->ctx->stream));          // the caller's block is free when this returns
    return 0;
}

static WtAlongArgs along_args(const wt_along *b, void *out)
{
    WtAlongArgs a{};
    a.in = b->in;
    a.out = out;
    a.plane = (int64_t)b->oc * b->N * b->ic;
    a.N = b->N;
    a.ic = b->ic;
    a.tiles = (b->ic + b->TI - 1) / b->TI;
    a.TI = b->TI;
    a.lg = b->lg;
    a.k5 = b->family == WT_B3SPLINE;
    return a;
}
// one workgroup per (outer index, tile); oc * tiles <= cap <= 2^30
static dim3 along_grid(const wt_along *b, const WtAlongArgs &a) { return dim3((unsigned)((int64_t)b->oc * a.tiles)); }
static size_t along_lds(const wt_along *b) { return 2 * (size_t)b->N * b->TI * b->itemsize; }

extern "C" int wt_along_decompose(wt_along *b, int level)
{
    WT_TRY(along_loaded(b, "wt_along_decompose"));
    if (!b->with_planes) WT_FAIL("wt_along_decompose: a stack without planes (wt_along_create)");
    if (level < 1 || level > b->max_level) WT_FAIL("wt_along_decompose: %d scales outside [1, %d]", level, b->max_level);
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    WtAlongArgs a = along_args(b, b->planes);
    a.level = level;
    const size_t lds = along_lds(b);
    if (lds > WT_SIGNALS_LDS_BYTES) WT_FAIL("wt_along_decompose: %zu bytes of LDS per tile", lds);
    const dim3 grid = along_grid(b, a), block(WT_ALONG_THREADS);
    ProfScope ps(c, b->itemsize == 8 ? "wt_along_decompose_kernel<double>" : "wt_along_decompose_kernel<float>");
    lines_by_type_family(b->itemsize, b->family, [&](auto t, auto k) {
        hipLaunchKernelGGL((wt_along_decompose_kernel<decltype(t), decltype(k)::value>), grid, block, lds, c->stream, a);
    });
    WT_HIP(hipGetLastError());
    b->level = level;
    return 0;
}

static int along_abs_median(wt_along *b, void *medians, int flags, const char *who)
{
    WT_TRY(along_loaded(b, who));
    WT_TRY(lines_flags(flags, who));
    if (!medians) WT_FAIL("%s: null pointer", who);
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    WtAlongArgs a = along_args(b, b->medians);
    a.n2 = 1;
    while (a.n2 < b->N) a.n2 <<= 1;
    const size_t lds = along_lds(b);
    if (lds > WT_SIGNALS_LDS_BYTES || (size_t)a.n2 * b->TI * b->itemsize > lds) WT_FAIL("%s: %zu bytes of LDS per tile", who, lds);
    {
        ProfScope ps(c, b->itemsize == 8 ? "wt_along_abs_median_kernel<double>" : "wt_along_abs_median_kernel<float>");
        lines_by_type(b->itemsize, [&](auto t) {
            typedef decltype(t) T;
            if (flags & WT_LINES_ANSCOMBE) hipLaunchKernelGGL((wt_along_abs_median_kernel<T, true>), along_grid(b, a), dim3(WT_ALONG_THREADS), lds, c->stream, a);
            else hipLaunchKernelGGL((wt_along_abs_median_kernel<T, false>), along_grid(b, a), dim3(WT_ALONG_THREADS), lds, c->stream, a);
        });
    }
    WT_HIP(hipGetLastError());
    // all medians of the chunk in one host round trip
    WT_HIP(hipMemcpyAsync(medians, b->medians, (size_t)b->oc * b->ic * b->itemsize, hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int wt_along_abs_median(wt_along *b, void *medians) { return along_abs_median(b, medians, 0, "wt_along_abs_median"); }
extern "C" int wt_along_abs_median_ex(wt_along *b, void *medians, int flags) { return along_abs_median(b, medians, flags, "wt_along_abs_median_ex"); }

static int along_denoise(wt_along *b, int level, int n_den, const double *tau, const double *wgt, int soft, int flags, const char *who)
{
    WT_TRY(along_loaded(b, who));
    WT_TRY(lines_flags(flags, who));
    if (b->with_planes) WT_FAIL("%s: a stack with planes (wt_along_create)", who);
    if (level < 1 || level > b->max_level) WT_FAIL("%s: %d scales outside [1, %d]", who, level, b->max_level);
    if (level + 1 > WT_MAX_SUM_PLANES) WT_FAIL("%s: %d planes (at most %d)", who, level + 1, WT_MAX_SUM_PLANES);
    if (n_den < 0 || n_den > level) WT_FAIL("%s: n_den %d outside [0,%d]", who, n_den, level);
    if (n_den > 0 && (!tau || !wgt)) WT_FAIL("%s: null tau / wgt", who);
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    const bool f64 = b->itemsize == 8;
    const int64_t count = (int64_t)b->oc * b->ic;
    if (n_den) {
        const double *src = tau;
        if (f64) {
            // rows of {tau, 1 / tau}
            b->h_tab.resize((size_t)count * 2 * n_den);
            for (int64_t f = 0; f < count; ++f) {
                double *row = b->h_tab.data() + (size_t)f * 2 * n_den;
                for (int k = 0; k < n_den; ++k) {
                    const double t = tau[(size_t)f * n_den + k];
                    row[k] = t;
                    row[n_den + k] = lines_inv_tau(t);
                }
            }
            src = b->h_tab.data();
        }
        WT_HIP(hipMemcpyAsync(b->d_tab, src, (size_t)count * (f64 ? 2 : 1) * n_den * sizeof(double), hipMemcpyHostToDevice, c->stream));
        WT_HIP(hipStreamSynchronize(c->stream));           // the caller's table (and the staging block) are free
    }
    WtAlongArgs a = along_args(b, b->sum);
    a.tab = b->d_tab;
    a.level = level;
    a.n_den = n_den;
    a.soft = soft;
    for (int k = 0; k < n_den; ++k) a.wgt[k] = wgt[k];
    const size_t lds = along_lds(b);
    if (lds > WT_SIGNALS_LDS_BYTES) WT_FAIL("%s: %zu bytes of LDS per tile", who, lds);
    const dim3 grid = along_grid(b, a), block(WT_ALONG_THREADS);
    ProfScope ps(c, f64 ? "wt_along_denoise_kernel<double>" : "wt_along_denoise_kernel<float>");
    lines_by_type_family(b->itemsize, b->family, [&](auto t, auto k) {
        typedef decltype(t) T;
        constexpr int K = decltype(k)::value;
        if (flags & WT_LINES_ANSCOMBE) hipLaunchKernelGGL((wt_along_denoise_kernel<T, K, true>), grid, block, lds, c->stream, a);
        else hipLaunchKernelGGL((wt_along_denoise_kernel<T, K, false>), grid, block, lds, c->stream, a);
    });
    WT_HIP(hipGetLastError());
    b->has_sum = true;
    return 0;
}
extern "C" int wt_along_denoise(wt_along *b, int level, int n_den, const double *tau, const double *wgt, int soft)
{
    return along_denoise(b, level, n_den, tau, wgt, soft, 0, "wt_along_denoise");
}
extern "C" int wt_along_denoise_ex(wt_along *b, int level, int n_den, const double *tau, const double *wgt, int soft, int flags)
{
    return along_denoise(b, level, n_den, tau, wgt, soft, flags, "wt_along_denoise_ex");
}

extern "C" int wt_along_download_planes(wt_along *b, void *host, int64_t pitch, int64_t plane_stride)
{
    WT_TRY(along_loaded(b, "wt_along_download_planes"));
    if (!host) WT_FAIL("wt_along_download_planes: null pointer");
    if (b->level < 1) WT_FAIL("wt_along_download_planes: no transform in the stack (wt_along_decompose first)");
    if (pitch < b->ic || plane_stride < 0) WT_FAIL("wt_along_download_planes: pitch %lld, plane stride %lld", (long long)pitch, (long long)plane_stride);
    WtGuard guard_(b->ctx);
    const size_t plane = (size_t)b->oc * b->N * b->ic * b->itemsize;
    for (int s = 0; s <= b->level; ++s)
        WT_TRY(along_copy(b, (char *)b->planes + plane * s, (char *)host + (size_t)plane_stride * s * b->itemsize, pitch, false));
    WT_HIP(hipStreamSynchronize(b->ctx->stream));          // the caller's block is filled when this returns
    return 0;
}

extern "C" int wt_along_download_sum(wt_along *b, void *host, int64_t pitch)
{
    WT_TRY(along_loaded(b, "wt_along_download_sum"));
    if (!host) WT_FAIL("wt_along_download_sum: null pointer");
    if (!b->has_sum) WT_FAIL("wt_along_download_sum: no sum in the stack (wt_along_denoise first)");
    if (pitch < b->ic) WT_FAIL("wt_along_download_sum: pitch %lld below the %d elements of a row", (long long)pitch, b->ic);
    WtGuard guard_(b->ctx);
    WT_TRY(along_copy(b, b->sum, host, pitch, false));
    WT_HIP(hipStreamSynchronize(b->ctx->stream));
    return 0;
}
