// Stacks of 1-D signals of one length (wt_signals): spectra, light curves, detector rows.  The reference transforms
// a signal in its 1-D branch (watroo/wavelets.py:65-69 under :408-444); the per-signal call of this library runs it
// as a 1 x N image, one launch per scale.  This unit runs M signals in one launch, a workgroup per signal, the scales
// in LDS (wt_signals_kernels.h), and gives every signal the bits of the per-signal call.
// The host text it shares with the axis unit (wt_along.hip) is wt_lines_host.h, the device text wt_signal_common.h.
//
// Device memory of a wt_signals for M signals of N samples over `max_level` scales, Np = N rounded up to the
// 16-byte group:  in (M, Np) | planes (M, max_level + 1, Np) | sum (M, Np) | medians (M) | the threshold table.
// A call with fewer scales packs its planes (signal, level + 1, Np) at the head of `planes`.
// Only a stack that runs wow (wt_signals_moments / wt_signals_wow_sum) also holds, from its first such call on, the
// moments (M, max_level + 1, 2) and the wow tables (M, 2 * max_level + 1) of doubles: 4 * max_level + 3 doubles per signal.
#include <algorithm>
#include <cstring>
#include <vector>

#include "wt_lines_host.h"
#include "wt_signals_kernels.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

struct wt_signals {
    wt_ctx *ctx = nullptr;
    int n = 0, N = 0, Np = 0, family = WT_B3SPLINE, max_level = 0, itemsize = 4;
    int level = 0;                       // scales of the last wt_signals_decompose (layout of `planes`)
    void *in = nullptr, *planes = nullptr, *sum = nullptr, *medians = nullptr;
    double *d_tab = nullptr, *h_tab = nullptr;      // [signal][3 * WT_MAX_SUM_PLANES]
    void *h_med = nullptr;
    double *d_mom = nullptr, *h_mom = nullptr;      // wow: [signal][max_level + 1][2], allocated by the first wt_signals_moments
    double *d_wow = nullptr, *h_wow = nullptr;      // wow: tau [signal][level] | factor [signal][level + 1], by the first wt_signals_wow_sum
};

static inline int signals_pitch(int64_t N, int itemsize) { return (int)((N + 16 / itemsize - 1) / (16 / itemsize) * (16 / itemsize)); }

/* host logic, no device needed: 1 when M signals of n_samples samples of `itemsize` bytes (4: float, 8: double) of
 * `family` over `level` scales run on a wt_signals - a built-in family, 1 .. 24 scales, and the two LDS buffers of a
 * signal within WT_SIGNALS_LDS_BYTES (n_samples <= 8192 floats, <= 4096 doubles); else 0 */
extern "C" int wt_signals_ok(int family, int64_t n_samples, int level, int itemsize)
{
    if (family != WT_B3SPLINE && family != WT_TRIANGLE) return 0;
    if (itemsize != 4 && itemsize != 8) return 0;
    if (level < 1 || level > 24 || n_samples < 1 || n_samples > WT_SIGNALS_LDS_BYTES) return 0;
    return 2 * (int64_t)signals_pitch(n_samples, itemsize) * itemsize <= WT_SIGNALS_LDS_BYTES ? 1 : 0;
}

static void signals_free(wt_signals *b, int *bad)
{
    lines_free({b->in, b->planes, b->sum, b->medians, b->d_tab, b->d_mom, b->d_wow}, bad);
    for (void *q : {(void *)b->h_tab, b->h_med, (void *)b->h_mom, (void *)b->h_wow})
        if (q && hipHostFree(q) != hipSuccess) *bad = 1;
}

extern "C" int wt_signals_create(wt_ctx *ctx, int n_signals, int n_samples, int family, int max_level, int itemsize, wt_signals **out)
{
    WtGuard guard_(ctx);
    if (!ctx || !out) WT_FAIL("wt_signals_create: null pointer");
    *out = nullptr;
    if (n_signals < 1) WT_FAIL("wt_signals_create: %d signals", n_signals);
    if (!wt_signals_ok(family, n_samples, max_level, itemsize))
        WT_FAIL("wt_signals_create: %d samples of %d bytes, family %d, %d scales are not a signal stack (wt_signals_ok)", n_samples, itemsize, family,
                max_level);
    wt_signals *b = new wt_signals;
    b->ctx = ctx;
    b->n = n_signals;
    b->N = n_samples;
    b->Np = signals_pitch(n_samples, itemsize);
    b->family = family;
    b->max_level = max_level;
    b->itemsize = itemsize;
    const size_t row = (size_t)b->Np * itemsize, tab = (size_t)n_signals * 3 * WT_MAX_SUM_PLANES * sizeof(double);
    hipError_t e = hipMalloc(&b->in, row * n_signals);
    if (e == hipSuccess) e = hipMalloc(&b->planes, row * n_signals * (max_level + 1));
    if (e == hipSuccess) e = hipMalloc(&b->sum, row * n_signals);
    if (e == hipSuccess) e = hipMalloc(&b->medians, (size_t)n_signals * itemsize);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_tab, tab);
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_tab, tab, 0);
    if (e == hipSuccess) e = hipHostMalloc(&b->h_med, (size_t)n_signals * itemsize, 0);
    // (the padding of every row is read by the 16-byte loads and by the thresholded sum, never handed out: finite from the start)
    if (e == hipSuccess) e = hipMemsetAsync(b->in, 0, row * n_signals, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->planes, 0, row * n_signals * (max_level + 1), ctx->stream);
    return lines_created(b, out, e, "wt_signals_create", signals_free);
}

extern "C" int wt_signals_destroy(wt_signals *b) { return lines_destroy(b, "wt_signals_destroy", signals_free); }

extern "C" int wt_signals_info(wt_signals *b, int64_t *info)
{
    if (!b || !info) WT_FAIL("wt_signals_info: null pointer");
    const int64_t v[6] = {b->n, b->N, b->Np, b->family, b->max_level, b->itemsize};
    memcpy(info, v, sizeof v);
    return 0;
}

static int signals_check(const wt_signals *b, int first, int count, const char *who)
{
    if (!b) WT_FAIL("%s: null signal stack", who);
    if (first < 0 || count < 1 || (int64_t)first + count > b->n) WT_FAIL("%s: signals [%d, %d) outside the stack of %d", who, first, first + count, b->n);
    return 0;
}

// rows of N elements between a host block (pitch N) and device rows (pitch Np)
static int signals_copy(wt_signals *b, void *dev, void *host, size_t rows, bool up)
{
    const size_t w = (size_t)b->N * b->itemsize;
    WT_TRY(lines_copy(b->ctx->stream, dev, (size_t)b->Np * b->itemsize, host, w, w, rows, up));
    WT_HIP(hipStreamSynchronize(b->ctx->stream));          // the caller's block is free (or filled) when this returns
    return 0;
}

extern "C" int wt_signals_upload(wt_signals *b, int first, int count, const void *host)
{
    WT_TRY(signals_check(b, first, count, "wt_signals_upload"));
    if (!host) WT_FAIL("wt_signals_upload: null pointer");
    WtGuard guard_(b->ctx);
    return signals_copy(b, (char *)b->in + (size_t)first * b->Np * b->itemsize, const_cast<void *>(host), (size_t)count, true);
}

static int signals_decompose(wt_signals *b, int count, int level, int flags, const char *who)
{
    WT_TRY(signals_check(b, 0, count, who));
    WT_TRY(lines_flags(flags, who));
    if (level < 1 || level > b->max_level) WT_FAIL("%s: %d scales outside [1, %d]", who, level, b->max_level);
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    const size_t lds = 2 * (size_t)b->Np * b->itemsize;
    if (lds > WT_SIGNALS_LDS_BYTES) WT_FAIL("%s: %zu bytes of LDS per signal", who, lds);
    const dim3 grid((unsigned)count), block(WT_SIGNALS_THREADS);
    ProfScope ps(c, b->itemsize == 8 ? "wt_signals_decompose_kernel<double>" : "wt_signals_decompose_kernel<float>");
    lines_by_type_family(b->itemsize, b->family, [&](auto t, auto k) {
        typedef decltype(t) T;
        constexpr int K = decltype(k)::value;
        if (flags & WT_LINES_ANSCOMBE)
            hipLaunchKernelGGL((wt_signals_decompose_kernel<T, K, true>), grid, block, lds, c->stream, (const T *)b->in, (T *)b->planes, b->N, b->Np, level);
        else
            hipLaunchKernelGGL((wt_signals_decompose_kernel<T, K, false>), grid, block, lds, c->stream, (const T *)b->in, (T *)b->planes, b->N, b->Np, level);
    });
    WT_HIP(hipGetLastError());
    b->level = level;
    return 0;
}
extern "C" int wt_signals_decompose(wt_signals *b, int count, int level) { return signals_decompose(b, count, level, 0, "wt_signals_decompose"); }
extern "C" int wt_signals_decompose_ex(wt_signals *b, int count, int level, int flags) { return signals_decompose(b, count, level, flags, "wt_signals_decompose_ex"); }

extern "C" int wt_signals_abs_median(wt_signals *b, int count, void *medians)
{
    WT_TRY(signals_check(b, 0, count, "wt_signals_abs_median"));
    if (!medians) WT_FAIL("wt_signals_abs_median: null pointer");
    if (b->level < 1) WT_FAIL("wt_signals_abs_median: no transform in the stack (wt_signals_decompose first)");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    int n2 = 1;
    while (n2 < b->N) n2 <<= 1;
    const size_t lds = (size_t)n2 * b->itemsize;
    const int64_t stride = (int64_t)(b->level + 1) * b->Np;         // plane 0 of one signal to plane 0 of the next
    {
        ProfScope ps(c, b->itemsize == 8 ? "wt_signals_abs_median_kernel<double>" : "wt_signals_abs_median_kernel<float>");
        lines_by_type(b->itemsize, [&](auto t) {
            typedef decltype(t) T;
            hipLaunchKernelGGL(wt_signals_abs_median_kernel<T>, dim3((unsigned)count), dim3(WT_SIGNALS_THREADS), lds, c->stream, (const T *)b->planes, stride, b->N, n2,
                               (T *)b->medians);
        });
    }
    WT_HIP(hipGetLastError());
    // all medians in one host round trip
    WT_HIP(hipMemcpyAsync(b->h_med, b->medians, (size_t)count * b->itemsize, hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));
    memcpy(medians, b->h_med, (size_t)count * b->itemsize);
    return 0;
}

static int signals_denoise_sum(wt_signals *b, int count, int n_den, const double *tau, const double *wgt, int soft, int flags, const char *who)
{
    WT_TRY(signals_check(b, 0, count, who));
    WT_TRY(lines_flags(flags, who));
    if (b->level < 1) WT_FAIL("%s: no transform in the stack (wt_signals_decompose first)", who);
    const int n = b->level + 1;
    if (n > WT_MAX_SUM_PLANES) WT_FAIL("%s: %d planes (at most %d)", who, n, WT_MAX_SUM_PLANES);
    if (n_den < 0 || n_den > n) WT_FAIL("%s: n_den %d outside [0,%d]", who, n_den, n);
    if (n_den > 0 && (!tau || !wgt)) WT_FAIL("%s: null tau / wgt", who);
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    const bool f64 = b->itemsize == 8;
    const int per = f64 ? 3 : 2;
    // (the table of the previous call may still be read: the staging block is reused only behind the stream)
    WT_HIP(hipStreamSynchronize(c->stream));
    for (int f = 0; f < count; ++f) {
        double *row = b->h_tab + (size_t)f * per * n_den;
        for (int k = 0; k < n_den; ++k) {
            const double t = tau[(size_t)f * n_den + k];
            row[k] = t;
            if (f64) {
                row[n_den + k] = lines_inv_tau(t);
                row[2 * n_den + k] = wgt[(size_t)f * n_den + k];
            } else {
                row[n_den + k] = wgt[(size_t)f * n_den + k];
            }
        }
    }
    if (n_den) WT_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, (size_t)count * per * n_den * sizeof(double), hipMemcpyHostToDevice, c->stream));
    WtSignalsSumArgs a{};
    a.planes = b->planes;
    a.dst = b->sum;
    a.tab = b->d_tab;
    a.g = b->Np / (16 / b->itemsize);
    a.groups = (int64_t)count * a.g;
    a.Np = b->Np;
    a.n = n;
    a.n_den = n_den;
    a.soft = soft;
    const unsigned grid = (unsigned)std::min<int64_t>((a.groups + WT_SIGNALS_THREADS - 1) / WT_SIGNALS_THREADS, (int64_t)c->num_cus * 32);
    ProfScope ps(c, f64 ? "wt_signals_denoise_sum_kernel<double>" : "wt_signals_denoise_sum_kernel<float>");
    lines_by_type(b->itemsize, [&](auto t) {
        typedef decltype(t) T;
        if (flags & WT_LINES_ANSCOMBE) hipLaunchKernelGGL((wt_signals_denoise_sum_kernel<T, true>), dim3(grid), dim3(WT_SIGNALS_THREADS), 0, c->stream, a);
        else hipLaunchKernelGGL((wt_signals_denoise_sum_kernel<T, false>), dim3(grid), dim3(WT_SIGNALS_THREADS), 0, c->stream, a);
    });
    WT_HIP(hipGetLastError());
    return 0;
}
extern "C" int wt_signals_denoise_sum(wt_signals *b, int count, int n_den, const double *tau, const double *wgt, int soft)
{
    return signals_denoise_sum(b, count, n_den, tau, wgt, soft, 0, "wt_signals_denoise_sum");
}
extern "C" int wt_signals_denoise_sum_ex(wt_signals *b, int count, int n_den, const double *tau, const double *wgt, int soft, int flags)
{
    return signals_denoise_sum(b, count, n_den, tau, wgt, soft, flags, "wt_signals_denoise_sum_ex");
}

// a device block and its page-locked twin of `bytes` bytes, allocated on first use
static int signals_pair(double **dev, double **host, size_t bytes)
{
    if (!*dev) WT_HIP(hipMalloc((void **)dev, bytes));
    if (!*host) WT_HIP(hipHostMalloc((void **)host, bytes, 0));
    return 0;
}

extern "C" int wt_signals_moments(wt_signals *b, int count, double *moments)
{
    WT_TRY(signals_check(b, 0, count, "wt_signals_moments"));
    if (!moments) WT_FAIL("wt_signals_moments: null pointer");
    if (b->level < 1) WT_FAIL("wt_signals_moments: no transform in the stack (wt_signals_decompose first)");
    const int64_t blocks = (int64_t)count * (b->level + 1);
    if (blocks > 0x7fffffff) WT_FAIL("wt_signals_moments: %lld planes in one launch", (long long)blocks);
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    WT_TRY(signals_pair(&b->d_mom, &b->h_mom, (size_t)b->n * (b->max_level + 1) * 2 * sizeof(double)));
    {
        ProfScope ps(c, b->itemsize == 8 ? "wt_signals_moments_kernel<double>" : "wt_signals_moments_kernel<float>");
        lines_by_type(b->itemsize, [&](auto t) {
            typedef decltype(t) T;
            hipLaunchKernelGGL(wt_signals_moments_kernel<T>, dim3((unsigned)blocks), dim3(WT_SIGNALS_THREADS), 0, c->stream, (const T *)b->planes, b->N, b->Np,
                               b->d_mom);
        });
    }
    WT_HIP(hipGetLastError());
    // all moments in one host round trip
    WT_HIP(hipMemcpyAsync(b->h_mom, b->d_mom, (size_t)blocks * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));
    memcpy(moments, b->h_mom, (size_t)blocks * 2 * sizeof(double));
    return 0;
}

extern "C" int wt_signals_wow_sum(wt_signals *b, int count, int n_scales, const double *tau, const double *factor, int whitening, int soft, int write_planes)
{
    WT_TRY(signals_check(b, 0, count, "wt_signals_wow_sum"));
    if (b->level < 1) WT_FAIL("wt_signals_wow_sum: no transform in the stack (wt_signals_decompose first)");
    if (n_scales != b->level) WT_FAIL("wt_signals_wow_sum: %d scales, the stack holds a transform over %d", n_scales, b->level);
    if (!tau || !factor) WT_FAIL("wt_signals_wow_sum: null tau / factor");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    const int L = b->level;
    const size_t lds = whitening ? 2 * (size_t)b->Np * b->itemsize : 0;
    if (lds > WT_SIGNALS_LDS_BYTES) WT_FAIL("wt_signals_wow_sum: %zu bytes of LDS per signal", lds);
    WT_TRY(signals_pair(&b->d_wow, &b->h_wow, (size_t)b->n * (2 * b->max_level + 1) * sizeof(double)));
    // (the tables of the previous call may still be read: the staging block is reused only behind the stream)
    WT_HIP(hipStreamSynchronize(c->stream));
    const size_t nt = (size_t)count * L, nf = (size_t)count * (L + 1);
    memcpy(b->h_wow, tau, nt * sizeof(double));
    memcpy(b->h_wow + nt, factor, nf * sizeof(double));
    WT_HIP(hipMemcpyAsync(b->d_wow, b->h_wow, (nt + nf) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    WtSignalsWowArgs a{};
    a.planes = b->planes;
    a.sum = b->sum;
    a.tau = b->d_wow;
    a.factor = b->d_wow + nt;
    a.N = b->N;
    a.Np = b->Np;
    a.level = L;
    a.soft = soft;
    a.write_planes = write_planes;
    const dim3 grid((unsigned)count), block(WT_SIGNALS_THREADS);
    ProfScope ps(c, b->itemsize == 8 ? "wt_signals_wow_kernel<double>" : "wt_signals_wow_kernel<float>");
    lines_by_type_family(b->itemsize, b->family, [&](auto t, auto k) {
        typedef decltype(t) T;
        constexpr int K = decltype(k)::value;
        if (whitening) hipLaunchKernelGGL((wt_signals_wow_kernel<T, K, true>), grid, block, lds, c->stream, a);
        else hipLaunchKernelGGL((wt_signals_wow_kernel<T, K, false>), grid, block, 0, c->stream, a);
    });
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_signals_download_planes(wt_signals *b, int first, int count, void *host)
{
    WT_TRY(signals_check(b, first, count, "wt_signals_download_planes"));
    if (!host) WT_FAIL("wt_signals_download_planes: null pointer");
    if (b->level < 1) WT_FAIL("wt_signals_download_planes: no transform in the stack (wt_signals_decompose first)");
    WtGuard guard_(b->ctx);
    const size_t rows = (size_t)(b->level + 1);
    return signals_copy(b, (char *)b->planes + (size_t)first * rows * b->Np * b->itemsize, host, (size_t)count * rows, false);
}

extern "C" int wt_signals_download_sum(wt_signals *b, int first, int count, void *host)
{
    WT_TRY(signals_check(b, first, count, "wt_signals_download_sum"));
    if (!host) WT_FAIL("wt_signals_download_sum: null pointer");
    WtGuard guard_(b->ctx);
    return signals_copy(b, (char *)b->sum + (size_t)first * b->Np * b->itemsize, host, (size_t)count, false);
}
