// libwatroo_hip.so - host side of the C ABI, unit 3 of 4: the pointwise operators (plane sum, thresholds, wow
// update, gamma blend, Anscombe), cubes, the support of richardson_lucy (small-PSF correlation, FFT products, the
// tap-list operator and the tiled axis filters), the exact median and the reductions.  gfx950 only.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "wt_host.h"
#include "wt_kernels_common.h"
#include "wt_kernels_apps.h"
#include "wt_fft.h"
#include "wt_axis.h"
#include "wt_rng.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

// =============================================================================================
// pointwise ops
// =============================================================================================
extern "C" int wt_plane_sum(wt_plan *p, int first, int count, int dst)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_plane_sum: null plan");
    if (count < 1 || count > WT_MAX_SUM_PLANES) WT_FAIL("wt_plane_sum: count %d out of range [1,%d]", count, WT_MAX_SUM_PLANES);
    if (first < 0 || first + count - 1 > p->max_level) WT_FAIL("wt_plane_sum: planes [%d,%d) outside [0,%d]", first, first + count, p->max_level);
    const float *planes[WT_MAX_SUM_PLANES];
    for (int i = 0; i < count; ++i) {
        float *b = nullptr;
        WT_TRY(plane_base(p, first + i, &b));
        planes[i] = b;
    }
    float *o = nullptr;
    WT_TRY(plane_base(p, dst, &o));
    return launch_plane_sum(p->ctx, planes, count, o, plan_n4(p));
}

// (wt_plane_sum and wt_batch_plane_sum: n4 float4 groups of contiguous planes, summed in plane order)
int launch_plane_sum(wt_ctx *c, const float *const *planes, int count, float *out, int64_t n4)
{
    SumArgs a{};
    a.n = count;
    for (int i = 0; i < count; ++i) a.p[i] = planes[i];
    ProfScope ps(c, "wt_plane_sum_kernel");
    static const int64_t sum_grid = getenv("WT_SUM_GRID") ? atoll(getenv("WT_SUM_GRID")) : ((int64_t)1 << 30);
    const int grid = (int)std::min<int64_t>((n4 + 255) / 256, sum_grid);
    hipLaunchKernelGGL(wt_plane_sum_kernel, dim3(grid), dim3(256), 0, c->stream, a, out, n4);
    WT_HIP(hipGetLastError());
    return 0;
}

// np.sum(coefficients, axis=0) in two parts (round 5).  In wow() behind a bilateral transform (watroo/utils.py:174-205)
// the whitened planes of the first scales are final long before the last scales of the transform have run:
// wt_plane_sum_early puts planes [0, count) into dst on the SIDE stream, behind the updates queued there and beside
// the bilateral kernels still running (they are bound by instruction issue and leave two thirds of the memory
// bandwidth idle); wt_plane_sum_resume finishes dst = dst + planes [first, first + count) on the main stream.  The
// additions happen in plane order either way (a sequential sum interrupted and resumed): identical bits.
// *done = 0: the plan is not in the overlapped state (nothing queued: the caller sums in one piece).
static int plane_sum_launch(wt_plan *p, const float *acc, int first, int count, float *o)
{
    SumArgs a{};
    a.n = 0;
    if (acc) a.p[a.n++] = const_cast<float *>(acc);
    for (int i = 0; i < count; ++i) {
        float *b = nullptr;
        WT_TRY(plane_base(p, first + i, &b));
        a.p[a.n++] = b;
    }
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_plane_sum_kernel");
    hipLaunchKernelGGL(wt_plane_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, p->ctx->stream, a, o, n4);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_plane_sum_early(wt_plan *p, int count, int dst, int *done)
{
    WtGuard guard_(ctx_of(p));
    if (!p || !done) WT_FAIL("wt_plane_sum_early: null pointer");
    *done = 0;
    if (count < 1 || count > WT_MAX_SUM_PLANES || count - 1 > p->max_level) WT_FAIL("wt_plane_sum_early: %d planes outside [1,%d]", count, p->max_level + 1);
    if (dst >= 0) WT_FAIL("wt_plane_sum_early: dst must not be a coefficient plane");
    const bool side = g_opt_wow_overlap && wt_side_ok(p) && count <= p->overlap_scales && p->nranks == 1 && p->ctx->side_pending;
    if (!side) return 0;
    WtSideScope side_scope(p->ctx, p->scale_ev[count - 1], true);
    if (!side_scope.ok()) return 2;
    float *o = nullptr;
    WT_TRY(plane_base(p, dst, &o));
    WT_TRY(plane_sum_launch(p, nullptr, 0, count, o));
    *done = 1;
    return 0;
}

extern "C" int wt_plane_sum_resume(wt_plan *p, int first, int count, int dst)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_plane_sum_resume: null plan");
    if (count < 1 || count + 1 > WT_MAX_SUM_PLANES || first < 0 || first + count - 1 > p->max_level)
        WT_FAIL("wt_plane_sum_resume: planes [%d,%d) outside [0,%d]", first, first + count, p->max_level);
    if (dst >= 0) WT_FAIL("wt_plane_sum_resume: dst must not be a coefficient plane");
    float *o = nullptr;
    WT_TRY(plane_base(p, dst, &o));                 // (a main-stream access: joins the side stream)
    return plane_sum_launch(p, o, first, count, o);  // in place: every thread reads its own group before writing it
}

static int noise_ptr(wt_plan *p, int noise_plane, float **np_);

extern "C" int wt_denoise_sum(wt_plan *p, int first, int count, int dst, int n_den, const double *tau,
                              const double *wgt, int soft, int noise_plane, int write_back)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_denoise_sum: null plan");
    if (count < 1 || count > WT_MAX_SUM_PLANES) WT_FAIL("wt_denoise_sum: count %d out of range [1,%d]", count, WT_MAX_SUM_PLANES);
    if (first < 0 || first + count - 1 > p->max_level) WT_FAIL("wt_denoise_sum: planes [%d,%d) outside [0,%d]", first, first + count, p->max_level);
    if (n_den < 0 || n_den > count) WT_FAIL("wt_denoise_sum: n_den %d outside [0,%d]", n_den, count);
    if (n_den > 0 && (!tau || !wgt)) WT_FAIL("wt_denoise_sum: null tau/wgt");
    DenoiseSumArgs a{};
    a.n = count; a.n_den = n_den; a.soft = soft; a.write_back = write_back;
    for (int i = 0; i < count; ++i) {
        float *b = nullptr;
        WT_TRY(plane_base(p, first + i, &b));
        a.p[i] = b;
        a.tau[i] = i < n_den ? tau[i] : 0.0;
        a.wgt[i] = i < n_den ? (float)wgt[i] : 1.f;
    }
    float *o = nullptr, *nz = nullptr;
    WT_TRY(plane_base(p, dst, &o));
    WT_TRY(noise_ptr(p, noise_plane, &nz));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_denoise_sum_kernel");
    hipLaunchKernelGGL(wt_denoise_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, p->ctx->stream, a, nz, o, n4);
    WT_HIP(hipGetLastError());
    return 0;
}

// wt_denoise_sum over the strip-local rows [r0, r1) of planes 0 .. count-1 (planes are contiguous with
// pitch P: a row range is a flat range); planes are not written back
int denoise_sum_rows(wt_plan *p, int count, int dst, int n_den, const double *tau, const double *wgt, int soft, int r0, int r1)
{
    if (r1 <= r0) return 0;
    DenoiseSumArgs a{};
    a.n = count; a.n_den = n_den; a.soft = soft; a.write_back = 0;
    const size_t off = (size_t)r0 * p->g.P;
    for (int i = 0; i < count; ++i) {
        float *b = nullptr;
        WT_TRY(plane_base(p, i, &b));
        a.p[i] = b + off;
        a.tau[i] = i < n_den ? tau[i] : 0.0;
        a.wgt[i] = i < n_den ? (float)wgt[i] : 1.f;
    }
    float *o = nullptr;
    WT_TRY(plane_base(p, dst, &o));
    const int64_t n4 = (int64_t)(r1 - r0) * p->g.P / 4;
    ProfScope ps(p->ctx, "wt_denoise_sum_kernel");
    hipLaunchKernelGGL(wt_denoise_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, p->ctx->stream, a, (const float *)nullptr, o + off, n4);
    WT_HIP(hipGetLastError());
    return 0;
}

static int noise_ptr(wt_plan *p, int noise_plane, float **np_)
{
    *np_ = nullptr;
    if (noise_plane == WT_PLANE_NONE) return 0;
    return plane_base(p, noise_plane, np_);
}

extern "C" int wt_significance(wt_plan *p, int plane, int dst, double tau, int soft, int noise_plane)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_significance: null plan");
    if (!(tau > 0.0)) WT_FAIL("wt_significance: tau must be positive (the sigma==0 / noise==0 short-circuits of wavelets.py:130-143 are host-side)");
    float *c = nullptr, *d = nullptr, *nz = nullptr;
    WT_TRY(plane_base(p, plane, &c));
    WT_TRY(plane_base(p, dst, &d));
    WT_TRY(noise_ptr(p, noise_plane, &nz));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_signif_kernel");
    hipLaunchKernelGGL(wt_signif_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, c, nz, d, n4, tau, 1.f, soft, 0);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_denoise(wt_plan *p, int plane, double tau, double wgt, int soft, int noise_plane)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_denoise: null plan");
    if (!(tau > 0.0)) WT_FAIL("wt_denoise: tau must be positive");
    float *c = nullptr, *nz = nullptr;
    WT_TRY(plane_base(p, plane, &c));
    WT_TRY(noise_ptr(p, noise_plane, &nz));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_signif_kernel");
    hipLaunchKernelGGL(wt_signif_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, c, nz, c, n4, tau, (float)wgt, soft, 1);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_wow_update(wt_plan *p, int plane, int power_plane, double tau, int soft, int noise_plane, float factor, int gamma_plane)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_wow_update: null plan");
    float *c = nullptr, *pw = nullptr, *nz = nullptr, *gm = nullptr;
    WT_TRY(plane_base(p, plane, &c));
    if (power_plane != WT_PLANE_NONE) WT_TRY(plane_base(p, power_plane, &pw));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(plane_base(p, gamma_plane, &gm));
    WT_TRY(noise_ptr(p, noise_plane, &nz));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_wow_kernel");
    hipLaunchKernelGGL(wt_wow_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, c, pw, nz, gm, n4, tau, soft, factor);
    WT_HIP(hipGetLastError());
    return 0;
}

// Fused wow per-scale update: local power conv_s(c^2) (watroo/utils.py:194) is formed inside
// the kernel that applies wt_wow_update's pointwise step, and the result is written to a spare
// plane whose pointer is then swapped with the coefficient plane ("in place" at pointer level:
// the neighbours' taps still need the old values while the kernel runs).
extern "C" int wt_wow_scale(wt_plan *p, int plane, int s, double tau, int soft, int noise_plane,
                            float factor, int gamma_plane, int flags)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_wow_scale: null plan");
    if (plane < 0 || plane > p->max_level) WT_FAIL("wt_wow_scale: plane %d is not a coefficient plane", plane);
    WT_TRY(check_scale(p, s, "wt_wow_scale"));
    const int spare = WT_PLANE_SCRATCH(3);
    // Right behind a bilateral transform the update of w_s only needs scale s of it (its event): it runs on the
    // side stream, beside the bilateral kernels of the later scales (plain mode: no maps to order against)
    const bool side = g_opt_wow_overlap && wt_side_ok(p) && plane < p->overlap_scales && noise_plane == WT_PLANE_NONE &&
                      gamma_plane == WT_PLANE_NONE && p->nranks == 1 && !p->ntaps;
    WtSideScope side_scope(p->ctx, side ? p->scale_ev[plane] : nullptr, side);
    if (!side_scope.ok()) return 2;
    float *c = nullptr, *t = nullptr, *nz = nullptr, *gm = nullptr;
    WT_TRY(plane_base(p, plane, &c));
    WT_TRY(plane_base(p, spare, &t));
    WT_TRY(noise_ptr(p, noise_plane, &nz));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(plane_base(p, gamma_plane, &gm));
    WT_TRY(maybe_exchange(p, plane, scale_halo(p, s), flags));
    ChainArgs a{};
    a.in = c; a.out_c = t; a.out_w = nullptr; a.aux = nullptr;
    a.noise = nz; a.gamma = gm; a.tau = tau; a.factor = factor; a.soft = soft; a.whiten = 1;
    // (no per-pixel noise map, no gamma accumulator: the instantiation without conditional loads)
    WT_TRY(launch_chain_mode(p, !nz && !gm ? MODE_WOW_PLAIN : (!nz ? MODE_WOW_GAMMA : MODE_WOW), a, s, "wt_chain_kernel<wow>"));
    std::swap(p->coef[plane], p->scratch[3]);     // both are "first margin row" pointers
    return 0;
}

extern "C" int wt_gamma_blend(wt_plan *p, int recon, int gamma_plane, float gmin, float gmax, float inv_gamma, float h)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_gamma_blend: null plan");
    float *r = nullptr, *g = nullptr;
    WT_TRY(plane_base(p, recon, &r));
    WT_TRY(plane_base(p, gamma_plane, &g));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_gamma_kernel");
    hipLaunchKernelGGL(wt_gamma_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, r, g, n4, gmin, gmax - gmin, inv_gamma, h);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_anscombe(wt_plan *p, int src, int dst, float alpha, float g, float sigma, int inverse)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_anscombe: null plan");
    if (alpha == 0.f) WT_FAIL("wt_anscombe: alpha must be non-zero");
    float *s = nullptr, *d = nullptr;
    WT_TRY(plane_base(p, src, &s));
    WT_TRY(plane_base(p, dst, &d));
    return launch_anscombe(p->ctx, s, d, plan_n4(p), alpha, g, sigma, inverse);
}

// (wt_anscombe and wt_batch_anscombe: n4 float4 groups of contiguous planes)
int launch_anscombe(wt_ctx *c, const float *s, float *d, int64_t n4, float alpha, float g, float sigma, int inverse)
{
    // scalar terms are formed in double like the python floats of wavelets.py:17,19
    const double a = alpha, gg = g, sg = sigma;
    float c1, c2, c3;
    if (inverse) { c1 = (float)(a * gg); c2 = (float)(sg * sg); c3 = (float)(3.0 * a / 8.0); }
    else { c1 = (float)(3.0 * a * a / 8.0); c2 = (float)(sg * sg); c3 = (float)(a * gg); }
    ProfScope ps(c, "wt_anscombe_kernel");
    hipLaunchKernelGGL(wt_anscombe_kernel, dim3(flat_grid(n4)), dim3(256), 0, c->stream, s, d, n4, alpha, c1, c2, c3, inverse);
    WT_HIP(hipGetLastError());
    return 0;
}

// =============================================================================================
// 3-D cubes: a (Z, Y, X) cube is a (Z*Y) x X image on the plan
// =============================================================================================
extern "C" int wt_binary(wt_plan *p, int op, int a, int b, int dst);
static int conv3d_planes(wt_plan *p, float *in, float *tmp, float *out, int s, int depth)
{
    const Geo whole = p->g;
    const int Y = whole.H / depth;
    if (p->ntaps) {      // user-defined taps: rows -> scratch 15, axis 1 -> scratch 12, axis 0 -> out
        float *t2 = nullptr;
        WT_TRY(plane_base(p, WT_PLANE_SCRATCH(12), &t2));
        if (in == t2 || out == t2 || tmp == t2) WT_FAIL("3-D filter: scratch plane 12 is used internally for user-defined taps");
        const CustomTaps t = plan_taps(p);
        dim3 grid((whole.W + 255) / 256, (unsigned)std::min(whole.H, 32768)), block(256);
        ProfScope ps(p->ctx, "wt_custom_kernels");
        hipLaunchKernelGGL(wt_custom_rows_kernel, grid, block, 0, p->ctx->stream, (const float *)in, tmp, whole, 1 << s, t, 0);
        hipLaunchKernelGGL(wt_custom_axis_kernel, grid, block, 0, p->ctx->stream, (const float *)tmp, t2, whole.W, whole.P, Y, depth,
                           1 << s, whole.border, t, 1);
        hipLaunchKernelGGL(wt_custom_axis_kernel, grid, block, 0, p->ctx->stream, (const float *)t2, out, whole.W, whole.P, Y, depth,
                           1 << s, whole.border, t, 0);
        WT_HIP(hipGetLastError());
        return 0;
    }
    // per-slice 2-D filter: the single-scale kernels run on each Y x X slice as its own image
    p->g.H = Y;
    p->g.nrows = Y;
    int rc = 0;
    for (int z = 0; z < depth && !rc; ++z) {
        const size_t off = (size_t)z * Y * whole.P;
        {
            ChainArgs ca{};
            ca.in = in + off; ca.out_c = tmp + off;
            ca.f1 = 1.f; ca.f2 = 1.f;
            rc = launch_chain_mode(p, MODE_SMOOTH, ca, s, "wt_chain_kernel<smooth>");
        }
    }
    p->g = whole;
    if (rc) return rc;
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_zfilter_kernel");
    if (p->family == WT_B3SPLINE)
        hipLaunchKernelGGL((wt_zfilter_kernel<5>), dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, tmp, out, n4, whole.P / 4, Y, depth, 1 << s, whole.border);
    else
        hipLaunchKernelGGL((wt_zfilter_kernel<3>), dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, tmp, out, n4, whole.P / 4, Y, depth, 1 << s, whole.border);
    WT_HIP(hipGetLastError());
    return 0;
}

static int check3d(const wt_plan *p, int depth, int s, const char *who)
{
    if (p->nranks != 1 || (p->g.border != 0 && p->g.border != 1))
        WT_FAIL("%s: single-GPU plans with the symmetric border (whole cube or polyphase) only", who);
    if (depth < 1 || p->g.H % depth) WT_FAIL("%s: plan height %d is not a multiple of depth %d", who, p->g.H, depth);
    if (s < 0 || s > 20) WT_FAIL("%s: scale %d out of range", who, s);
    return 0;
}

extern "C" int wt_smooth3d(wt_plan *p, int src, int dst, int s, int depth)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_smooth3d: null plan");
    WT_TRY(check3d(p, depth, s, "wt_smooth3d"));
    const int tmpid = WT_PLANE_SCRATCH(15);
    if (src == dst || src == tmpid || dst == tmpid) WT_FAIL("wt_smooth3d: src, dst and scratch 15 must differ");
    float *in = nullptr, *tmp = nullptr, *out = nullptr;
    WT_TRY(plane_base(p, src, &in));
    WT_TRY(plane_base(p, tmpid, &tmp));
    WT_TRY(plane_base(p, dst, &out));
    return conv3d_planes(p, in, tmp, out, s, depth);
}

// sdev_loc(..., variance=True) * f1 * f2 of a cube (watroo/wavelets.py:24-32, :434-436) into `dst`
extern "C" int wt_local_variance3d(wt_plan *p, int src, int dst, int s, int depth, float f1, float f2)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_local_variance3d: null plan");
    WT_TRY(check3d(p, depth, s, "wt_local_variance3d"));
    const int tmpid = WT_PLANE_SCRATCH(15), sqid = WT_PLANE_SCRATCH(14), mid = WT_PLANE_SCRATCH(13);
    if (src == dst || src == tmpid || src == sqid || src == mid || dst == tmpid || dst == sqid || dst == mid)
        WT_FAIL("wt_local_variance3d: src / dst must differ from each other and from scratch 13-15");
    float *in = nullptr, *tmp = nullptr, *sq = nullptr, *mean = nullptr, *out = nullptr;
    WT_TRY(plane_base(p, src, &in));
    WT_TRY(plane_base(p, tmpid, &tmp));
    WT_TRY(plane_base(p, sqid, &sq));
    WT_TRY(plane_base(p, mid, &mean));
    WT_TRY(plane_base(p, dst, &out));
    WT_TRY(conv3d_planes(p, in, tmp, mean, s, depth));          // conv(I)
    WT_TRY(wt_binary(p, WT_OP_MUL, src, src, sqid));            // I^2
    WT_TRY(conv3d_planes(p, sq, tmp, out, s, depth));           // conv(I^2)
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_var_moments_kernel");
    hipLaunchKernelGGL(wt_var_moments_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, (const float *)mean,
                       (const float *)out, out, n4, f1, f2);
    WT_HIP(hipGetLastError());
    return 0;
}

// atrous_convolution(cube, 3-D kernel, bilateral_variance=var, s) - watroo/wavelets.py:74-105
extern "C" int wt_bilateral3d_conv(wt_plan *p, int src, int var, int dst, int s, int depth)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_bilateral3d_conv: null plan");
    WT_TRY(check3d(p, depth, s, "wt_bilateral3d_conv"));
    if (src == dst || var == dst) WT_FAIL("wt_bilateral3d_conv: dst must differ from src and var");
    float *in = nullptr, *v = nullptr, *out = nullptr;
    WT_TRY(plane_base(p, src, &in));
    WT_TRY(plane_base(p, var, &v));
    WT_TRY(plane_base(p, dst, &out));
    const int Y = p->g.H / depth;
    dim3 grid((p->g.W + 255) / 256, (unsigned)std::min(p->g.H, 32768)), block(256);
    if (p->ntaps) {
        ProfScope ps(p->ctx, "wt_bilateral_custom_kernel");
        hipLaunchKernelGGL(wt_bilateral_custom_kernel, grid, block, 0, p->ctx->stream, (const float *)in, (const float *)v, out,
                           (float *)nullptr, p->g, Y, depth, 1 << s, plan_taps(p), 0);
        WT_HIP(hipGetLastError());
        return 0;
    }
    ProfScope ps(p->ctx, "wt_bilateral3d_kernel");
    if (p->family == WT_B3SPLINE)
        hipLaunchKernelGGL((wt_bilateral3d_kernel<5>), grid, block, 0, p->ctx->stream, (const float *)in, (const float *)v, out,
                           p->g.W, p->g.P, Y, depth, 1 << s, p->g.border);
    else
        hipLaunchKernelGGL((wt_bilateral3d_kernel<3>), grid, block, 0, p->ctx->stream, (const float *)in, (const float *)v, out,
                           p->g.W, p->g.P, Y, depth, 1 << s, p->g.border);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_decompose3d(wt_plan *p, int src, int level, int depth)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_decompose3d: null plan");
    WT_TRY(check3d(p, depth, 0, "wt_decompose3d"));
    if (level < 0 || level > p->max_level) WT_FAIL("wt_decompose3d: level %d exceeds plan max_level %d", level, p->max_level);
    if (src >= 0 && src <= level) WT_FAIL("wt_decompose3d: src plane %d is one of the output planes", src);
    if (level == 0) return wt_copy_plane(p, src, 0);
    int cur = src;
    for (int s = 0; s < level; ++s) {
        const int nxt = (s == level - 1) ? level : WT_PLANE_SCRATCH(s & 1);
        if (cur == nxt) WT_FAIL("wt_decompose3d: scratch planes 0/1 are used internally");
        float *in = nullptr, *tmp = nullptr, *oc = nullptr;
        WT_TRY(plane_base(p, cur, &in));
        WT_TRY(plane_base(p, WT_PLANE_SCRATCH(15), &tmp));
        WT_TRY(plane_base(p, nxt, &oc));
        WT_TRY(conv3d_planes(p, in, tmp, oc, s, depth));
        WT_TRY(wt_binary(p, WT_OP_SUB, cur, nxt, s));        // w_s = c_s - c_{s+1}   (wavelets.py:442)
        cur = nxt;
    }
    return 0;
}

// =============================================================================================
// Richardson-Lucy support
// =============================================================================================
extern "C" int wt_filter2d_ex(wt_plan *p, int src, int dst, const float *kernel, int kh, int kw, int ay, int ax,
                             int border, int flags)
{
    WtGuard guard_(ctx_of(p));
    if (!p || !kernel) WT_FAIL("wt_filter2d: null pointer");
    if (kh < 1 || kw < 1 || (int64_t)kh * kw > (1 << 22)) WT_FAIL("wt_filter2d: kernel %d x %d unsupported (up to 2^22 taps)", kh, kw);
    if (ay < 0 || ay >= kh || ax < 0 || ax >= kw) WT_FAIL("wt_filter2d: anchor (%d, %d) outside the %d x %d kernel", ay, ax, kh, kw);
    if (src == dst) WT_FAIL("wt_filter2d: src and dst must differ");
    if (border != WT_BORDER_SYMMETRIC && border != WT_BORDER_PERIODIC) WT_FAIL("wt_filter2d: border %d unsupported (symmetric or periodic)", border);
    if (p->g.border) WT_FAIL("wt_filter2d ignores the plan's border mode; reset it to symmetric first");
    const bool wrap = border == WT_BORDER_PERIODIC;
    if (wrap && (p->nranks > 1 || p->g.row0 != 0 || p->g.nrows != p->g.H))
        WT_FAIL("wt_filter2d: the periodic border needs a whole-image plan");
    const int reach = std::max(ay, kh - 1 - ay);
    if (p->nranks > 1 && reach > p->g.halo) WT_FAIL("wt_filter2d: kernel needs %d halo rows, plan has %d", reach, p->g.halo);
    wt_ctx *c = p->ctx;
    float *in = nullptr, *o = nullptr;
    WT_TRY(plane_base(p, src, &in));
    WT_TRY(plane_base(p, dst, &o));
    WT_TRY(maybe_exchange(p, src, reach, flags));
    const size_t ntaps = (size_t)kh * kw;
    // the taps come from caller-owned memory: drain the stream (the previous PSF may still be read),
    // copy synchronously (small PSFs through the pinned scratch, as before)
    WT_HIP(hipStreamSynchronize(c->stream));
    if (ntaps > c->d_psf_cap) {
        (void)hipFree(c->d_psf);
        c->d_psf = nullptr;
        c->d_psf_cap = 0;
        WT_HIP(hipMalloc(&c->d_psf, ntaps * sizeof(float)));
        c->d_psf_cap = ntaps;
    }
    if (ntaps * sizeof(float) <= 65536) {
        memcpy(c->h_pinned, kernel, ntaps * sizeof(float));
        WT_HIP(hipMemcpyAsync(c->d_psf, c->h_pinned, ntaps * sizeof(float), hipMemcpyHostToDevice, c->stream));
    } else {
        WT_HIP(hipMemcpy(c->d_psf, kernel, ntaps * sizeof(float), hipMemcpyHostToDevice));
    }
    dim3 grid((p->g.W + WT_F2D_TW - 1) / WT_F2D_TW, (p->g.nrows + WT_F2D_TH - 1) / WT_F2D_TH), block(64, 4);
    if (grid.y > 65535u) WT_FAIL("wt_filter2d: strip too tall");
    // Bands (round 3: the reference has no PSF size limit, watroo/utils.py:245-257): a launch takes a
    // window of at most 4096 taps whose LDS tile fits 96 KB; the windows tile the PSF and every launch
    // after the first accumulates.  A PSF that fits is one launch, as before.
    const int bw = std::min(kw, 512);
    int bh = std::max(1, std::min(kh, 4096 / bw));
    while (bh > 1 && (size_t)(WT_F2D_TW + bw - 1) * (WT_F2D_TH + bh - 1) * sizeof(float) > 96 * 1024) --bh;
    const size_t lds = (size_t)(WT_F2D_TW + bw - 1) * (WT_F2D_TH + bh - 1) * sizeof(float);
    ProfScope ps(c, "wt_filter2d_kernel");
    bool first = true;
    for (int i0 = 0; i0 < kh; i0 += bh) {
        for (int j0 = 0; j0 < kw; j0 += bw) {
            const int h = std::min(bh, kh - i0), w = std::min(bw, kw - j0);
            const float *sub = c->d_psf + (size_t)i0 * kw + j0;
            #define WT_F2D_LAUNCH(WRAP, ACC)                                                                                        \
                do {                                                                                                                 \
                    if (lds > 64 * 1024)                                                                                             \
                        WT_HIP(hipFuncSetAttribute((const void *)wt_filter2d_kernel<WRAP, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                    hipLaunchKernelGGL((wt_filter2d_kernel<WRAP, ACC>), grid, block, lds, c->stream, (const float *)in, o, p->g, sub, kw, h, w, ay - i0, ax - j0); \
                } while (0)
            if (wrap) { if (first) WT_F2D_LAUNCH(true, false); else WT_F2D_LAUNCH(true, true); }
            else { if (first) WT_F2D_LAUNCH(false, false); else WT_F2D_LAUNCH(false, true); }
            #undef WT_F2D_LAUNCH
            first = false;
        }
    }
    WT_HIP(hipGetLastError());
    return 0;
}

// ---- circular products through the FFT (wt_fft.h; watroo/utils.py:245-254, 284)
extern "C" int wt_fft_supported(int64_t H, int64_t W, int *ok)
{
    if (!ok) WT_FAIL("wt_fft_supported: null pointer");
    *ok = (H <= WT_FFT_MAX_N && W <= WT_FFT_MAX_N && wt_fft_size_ok((int)H, (int)W)) ? 1 : 0;
    return 0;
}

static int fft_plan_check(const wt_plan *p, const char *who)
{
    if (p->nranks != 1 || p->g.row0 != 0 || p->g.nrows != p->g.H) WT_FAIL("%s: whole-image plans only", who);
    if (!wt_fft_size_ok(p->g.H, p->g.W)) WT_FAIL("%s: a side of the %d x %d image has a prime factor above 5 (or lies outside 2 .. %d)", who, p->g.H, p->g.W, WT_FFT_MAX_N);
    return 0;
}

extern "C" int wt_fft_spectrum(wt_plan *p, int src)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_fft_spectrum: null plan");
    WT_TRY(fft_plan_check(p, "wt_fft_spectrum"));
    float *s = nullptr;
    WT_TRY(plane_base(p, src, &s));
    const size_t before = p->raw_allocs.size();
    WT_TRY(wt_fft_prepare<float>(p->ctx, p->fft, p->g.H, p->g.W, p->raw_allocs));
    if (p->raw_allocs.size() != before) p->raw_bytes += (size_t)3 * p->g.H * p->g.W * sizeof(float2) + (size_t)(p->g.H + p->g.W) / 2 * sizeof(float2);
    return wt_fft_set_spectrum<float>(p->ctx, p->fft, s, p->g.P);
}

extern "C" int wt_fft_apply(wt_plan *p, int src, int dst, int conj)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_fft_apply: null plan");
    WT_TRY(fft_plan_check(p, "wt_fft_apply"));
    float *s = nullptr, *d = nullptr;
    WT_TRY(plane_base(p, src, &s));
    WT_TRY(plane_base(p, dst, &d));
    return wt_fft_apply_t<float>(p->ctx, p->fft, s, d, p->g.P, conj);
}

// the same float kernels for the frames of a wt_batch (wt_batch_fft_spectrum / wt_batch_fft_apply, wt_batch.hip)
int wt_fft32_prepare(wt_ctx *c, WtFftState &f, int H, int W, std::vector<void *> &owner, int nframes)
{
    return wt_fft_prepare<float>(c, f, H, W, owner, nframes);
}
int wt_fft32_spectrum(wt_ctx *c, WtFftState &f, const float *src, int P) { return wt_fft_set_spectrum<float>(c, f, src, P); }
int wt_fft32_apply(wt_ctx *c, WtFftState &f, const float *src, float *dst, int P, int conj, int nf, int64_t fstride)
{
    return wt_fft_apply_t<float>(c, f, src, dst, P, conj, nf, fstride);
}

extern "C" int wt_filter2d(wt_plan *p, int src, int dst, const float *kernel, int kh, int kw, int flags)
{
    WtGuard guard_(ctx_of(p));
    return wt_filter2d_ex(p, src, dst, kernel, kh, kw, kh / 2, kw / 2, WT_BORDER_SYMMETRIC, flags);
}

extern "C" int wt_taps_conv(wt_plan *p, int src, int var, int dst, const int32_t *offsets, const float *weights, int ntaps,
                            float center_weight, int has_center, int depth, int pad_mode, float fill_value)
{
    WtGuard guard_(ctx_of(p));
    if (pad_mode > WT_PAD_CONSTANT) WT_FAIL("wt_taps_conv: unknown pad mode %d (the polyphase modes take a dilation: wt_taps_conv_ex)", pad_mode);
    return wt_taps_conv_ex(p, src, var, dst, offsets, weights, ntaps, center_weight, has_center, depth, pad_mode, fill_value, 1);
}

extern "C" int wt_variance_from_moments(wt_plan *p, int mean, int meansq, int dst, float f1, float f2, int take_sqrt)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_variance_from_moments: null plan");
    float *m = nullptr, *q = nullptr, *d = nullptr;
    WT_TRY(plane_base(p, mean, &m));
    WT_TRY(plane_base(p, meansq, &q));
    WT_TRY(plane_base(p, dst, &d));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_var_moments_kernel");
    hipLaunchKernelGGL(wt_var_moments_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, (const float *)m, (const float *)q, d, n4, f1, f2,
                       take_sqrt);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_taps_conv_ex(wt_plan *p, int src, int var, int dst, const int32_t *offsets, const float *weights, int ntaps,
                               float center_weight, int has_center, int depth, int pad_mode, float fill_value, int dilation)
{
    WtGuard guard_(ctx_of(p));
    if (!p || (ntaps > 0 && (!offsets || !weights))) WT_FAIL("wt_taps_conv: null pointer");
    if (dilation < 1) WT_FAIL("wt_taps_conv: dilation %d must be positive", dilation);
    if (p->nranks > 1) WT_FAIL("wt_taps_conv: the generic operator is single-GPU (whole images)");
    if (src == dst || var == dst) WT_FAIL("wt_taps_conv: dst must differ from src and var");
    if (pad_mode < WT_PAD_SYMMETRIC || pad_mode > WT_PAD_POLY_MIRROR) WT_FAIL("wt_taps_conv: unknown pad mode %d", pad_mode);
    if (depth < 0 || (depth > 0 && p->g.nrows % depth)) WT_FAIL("wt_taps_conv: %d rows are not a multiple of depth %d", p->g.nrows, depth);
    float *in = nullptr, *o = nullptr, *v = nullptr;
    WT_TRY(plane_base(p, src, &in));
    WT_TRY(plane_base(p, dst, &o));
    if (var != WT_PLANE_NONE) WT_TRY(plane_base(p, var, &v));
    const int32_t *d_offs = nullptr;
    const float *d_wts = nullptr;
    WT_TRY(upload_taplist<float>(p->ctx, offsets, weights, ntaps, &d_offs, &d_wts));
    const int Z = depth > 0 ? depth : 1, Y = p->g.nrows / Z;
    ProfScope ps(p->ctx, "wt_taps_kernel");
    hipLaunchKernelGGL(wt_taps_kernel<float>, dim3((p->g.W + 255) / 256, (unsigned)std::min(p->g.nrows, 32768)), dim3(256), 0, p->ctx->stream,
                       (const float *)in, (const float *)v, o, p->g.W, p->g.P, Y, Z, d_offs, d_wts, ntaps, center_weight, has_center, pad_mode,
                       fill_value, dilation);
    WT_HIP(hipGetLastError());
    return 0;
}

int g_opt_axis_filter = getenv("WT_NO_AXIS_FILTER") ? 0 : 1;

/* K-tap filter along ONE axis of plane src -> dst: out[i] = sum_j weights[j] * in[pad(i + offsets[j])] along axis
 * 2 (x), 1 (y, inside every slice of a cube) or 0 (z, across the `depth` slices); border rule pad_mode / fill /
 * dilation as wt_taps_conv_ex.  The separable form of the scaling functions the tuned kernels do not take
 * (watroo/wavelets.py:152-197: any coefficients_1d) on the tiled kernels of wt_axis.h; tap sets they do not
 * take (more than 33 taps, irregular offsets along y / z, an x reach beyond 2048 pixels) run on the tap-list
 * operator - same bits either way. */
extern "C" int wt_axis_filter(wt_plan *p, int src, int dst, int axis, const int32_t *offsets, const float *weights, int ntaps, int depth,
                              int pad_mode, float fill_value, int dilation)
{
    WtGuard guard_(ctx_of(p));
    if (!p || !offsets || !weights) WT_FAIL("wt_axis_filter: null pointer");
    if (ntaps < 1 || ntaps > 4096) WT_FAIL("wt_axis_filter: %d taps unsupported", ntaps);
    if (axis < 0 || axis > 2) WT_FAIL("wt_axis_filter: axis %d (2 = x, 1 = y, 0 = z)", axis);
    if (dilation < 1) WT_FAIL("wt_axis_filter: dilation %d must be positive", dilation);
    if (p->nranks > 1) WT_FAIL("wt_axis_filter: the generic operator is single-GPU (whole images)");
    if (src == dst) WT_FAIL("wt_axis_filter: dst must differ from src");
    if (pad_mode < WT_PAD_SYMMETRIC || pad_mode > WT_PAD_POLY_MIRROR) WT_FAIL("wt_axis_filter: unknown pad mode %d", pad_mode);
    if (depth < 0 || (depth > 0 && p->g.nrows % depth)) WT_FAIL("wt_axis_filter: %d rows are not a multiple of depth %d", p->g.nrows, depth);
    if (axis == 0 && depth == 0) WT_FAIL("wt_axis_filter: axis 0 needs a cube (depth > 0)");
    float *in = nullptr, *o = nullptr;
    WT_TRY(plane_base(p, src, &in));
    WT_TRY(plane_base(p, dst, &o));
    const int rc = wt_axis_filter_launch<float>(p->ctx, in, o, p->g.W, p->g.P, p->g.nrows, depth, axis, offsets, weights, ntaps, pad_mode,
                                                fill_value, dilation);
    if (rc >= 0) return rc;
    std::vector<int32_t> o3((size_t)ntaps * 3, 0);
    for (int j = 0; j < ntaps; ++j) o3[(size_t)3 * j + axis] = offsets[j];
    return wt_taps_conv_ex(p, src, WT_PLANE_NONE, dst, o3.data(), weights, ntaps, 0.f, 0, depth, pad_mode, fill_value, dilation);
}

extern "C" int wt_binary(wt_plan *p, int op, int a, int b, int dst)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_binary: null plan");
    if (op < 0 || op > WT_OP_ADD_DIV) WT_FAIL("wt_binary: unknown op %d", op);
    float *pa = nullptr, *pb = nullptr, *pd = nullptr;
    WT_TRY(plane_base(p, a, &pa));
    WT_TRY(plane_base(p, b, &pb));
    WT_TRY(plane_base(p, dst, &pd));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_binary_kernel");
    hipLaunchKernelGGL(wt_binary_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, pa, pb, pd, n4, op);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_mrs_update(wt_plan *p, int plane, int mrs_plane, double tau, int soft, int noise_plane,
                             int persistent, float inv_pow)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_mrs_update: null plan");
    if (plane == mrs_plane) WT_FAIL("wt_mrs_update: plane and mrs_plane must differ");
    float *c = nullptr, *m = nullptr, *nz = nullptr;
    WT_TRY(plane_base(p, plane, &c));
    WT_TRY(plane_base(p, mrs_plane, &m));
    WT_TRY(noise_ptr(p, noise_plane, &nz));
    const int64_t n4 = plan_n4(p);
    ProfScope ps(p->ctx, "wt_mrs_kernel");
    hipLaunchKernelGGL(wt_mrs_kernel, dim3(flat_grid(n4)), dim3(256), 0, p->ctx->stream, c, m, nz, n4, tau, soft, persistent, inv_pow);
    WT_HIP(hipGetLastError());
    return 0;
}

// plane <- standard normal deviates (wt_rng.h: Philox4x32-10 keyed by seed, counter (x >> 2, y, trial, 0))
extern "C" int wt_fill_normal(wt_plan *p, int plane, uint64_t seed, uint32_t trial)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_fill_normal: null plan");
    float *d = nullptr;
    WT_TRY(plane_base(p, plane, &d));
    return wt_launch_fill_normal(p->ctx, d, p->g, p->g.nrows, 1, 0, seed, trial);
}

// =============================================================================================
// reductions / selection (host-synchronous: they return values)
// =============================================================================================
extern "C" int wt_reduce(wt_plan *p, int plane, double out[4])
{
    WtGuard guard_(ctx_of(p));
    if (!p || !out) WT_FAIL("wt_reduce: null pointer");
    wt_ctx *c = p->ctx;
    float *b = nullptr;
    WT_TRY(plane_base(p, plane, &b));
    // (work items: (row, chunk of 4096 pixels) pairs)
    const int blocks = (int)std::min<int64_t>((int64_t)p->g.nrows * ((p->g.W + 4095) / 4096), c->partial_blocks);
    double *dout = c->d_partials + (size_t)c->partial_blocks * 4;
    {
        ProfScope ps(c, "wt_reduce_kernel");
        hipLaunchKernelGGL(wt_reduce_kernel, dim3(blocks), dim3(256), 0, c->stream, b, p->g.nrows, p->g.P / 4, p->g.W, c->d_partials);
        hipLaunchKernelGGL(wt_reduce_final_kernel, dim3(1), dim3(256), 0, c->stream, c->d_partials, blocks, dout);
    }
    WT_HIP(hipGetLastError());
    if (p->nranks > 1) {
        if (!c->comm) WT_FAIL("wt_reduce: multi-rank plan without communicator");
        WT_NCCL(g_rccl.AllReduce(dout, dout, 2, NCCL_FLOAT64, NCCL_SUM, c->comm, c->stream));
        WT_NCCL(g_rccl.AllReduce(dout + 2, dout + 2, 1, NCCL_FLOAT64, NCCL_MIN, c->comm, c->stream));
        WT_NCCL(g_rccl.AllReduce(dout + 3, dout + 3, 1, NCCL_FLOAT64, NCCL_MAX, c->comm, c->stream));
    }
    WT_HIP(hipMemcpyAsync(c->h_pinned, dout, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));
    memcpy(out, c->h_pinned, 4 * sizeof(double));
    return 0;
}

// One histogram pass of the radix select + the device-side step that folds the selected bin into
// the state (no host round trip: the three passes chain on the stream).
static int select_pass(wt_plan *p, const float *b, WtSelectState *st, uint32_t prefix_mask, int shift, uint32_t bin_mask, int last,
                       bool have_hist = false)
{
    wt_ctx *c = p->ctx;
    if (!have_hist) {
        ProfScope ps(c, "wt_hist_kernel");
        // first level (no prefix yet): every element is binned - four interleaved LDS copies;
        // 4 blocks per CU (32 KB of LDS each) against 8 for the later levels
        const int X4 = (p->g.W + 3) / 4, nchunk = (X4 + 256 * WT_HIST_UNROLL - 1) / (256 * WT_HIST_UNROLL);
        const int64_t nitems = (int64_t)p->g.nrows * nchunk;
        if (prefix_mask == 0u)
            hipLaunchKernelGGL(wt_hist_kernel<4>, dim3((unsigned)std::min<int64_t>(nitems, 4 * c->num_cus)), dim3(256), 0, c->stream, b,
                               p->g.nrows, p->g.P / 4, p->g.W, prefix_mask, (const WtSelectState *)st, shift, bin_mask, c->d_hist);
        else
            hipLaunchKernelGGL(wt_hist_kernel<1>, dim3((unsigned)std::min<int64_t>(nitems, 8 * c->num_cus)), dim3(256), 0, c->stream, b,
                               p->g.nrows, p->g.P / 4, p->g.W, prefix_mask, (const WtSelectState *)st, shift, bin_mask, c->d_hist);
    }
    WT_HIP(hipGetLastError());
    if (p->nranks > 1) {
        if (!c->comm) WT_FAIL("wt_abs_median: multi-rank plan without communicator");
        WT_NCCL(g_rccl.AllReduce(c->d_hist, c->d_hist, WT_HIST_BINS, NCCL_UINT32, NCCL_SUM, c->comm, c->stream));
    }
    hipLaunchKernelGGL(wt_select_step_kernel, dim3(1), dim3(256), 0, c->stream, c->d_hist, st, (int)bin_mask + 1, shift, last);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_abs_median(wt_plan *p, int plane, float *median)
{
    WtGuard guard_(ctx_of(p));
    if (!p || !median) WT_FAIL("wt_abs_median: null pointer");
    wt_ctx *c = p->ctx;
    // MAD of a detail plane right behind a bilateral transform: beside the scales still queued (side stream)
    const bool side = g_opt_wow_overlap && wt_side_ok(p) && plane >= 0 && plane < p->overlap_scales && p->nranks == 1;
    WtSideScope side_scope(c, side ? p->scale_ev[plane] : nullptr, side);
    if (!side_scope.ok()) return 2;
    // a fused pass has histogrammed the first level of this plane (flag bit4 of wt_decompose /
    // wt_decompose_pass) and nothing has touched the plane or the bins since: one pass less over it
    const bool pre = c->prehist_plan == p && c->prehist_plane == plane;
    c->prehist_plan = nullptr;
    float *b = nullptr;
    WT_TRY(plane_base(p, plane, &b));
    const int64_t N = (int64_t)p->g.H * p->g.W;   // global element count
    const int64_t klo = (N - 1) / 2;
    // state on the device (behind the histogram and the upper-median word); initialised from pinned memory
    WtSelectState *st = (WtSelectState *)(c->d_hist + WT_HIST_BINS + 4);
    WtSelectState *hst = (WtSelectState *)c->h_pinned;
    hst->k = (unsigned long long)klo; hst->cum_le = 0; hst->prefix = 0; hst->failed = 0;
    const bool windowed = pre && c->prehist_windowed;
    c->prehist_windowed = false;
    WtSelectState res_st{};
    auto run = [&](bool have_hist, bool window) -> int {
        WT_HIP(hipMemcpyAsync(st, hst, sizeof(WtSelectState), hipMemcpyHostToDevice, c->stream));
        if (!have_hist) WT_HIP(hipMemsetAsync(c->d_hist, 0, WT_HIST_BINS * sizeof(uint32_t), c->stream));
        if (window) {
            // the riding histogram sits in a predicted window of 21-bit keys: its step fixes 21 bits at once
            hipLaunchKernelGGL(wt_select_window_step_kernel, dim3(1), dim3(256), 0, c->stream, c->d_hist, st, (const uint32_t *)hist_base_word(c));
            WT_HIP(hipGetLastError());
        } else {
            WT_TRY(select_pass(p, b, st, 0u, 20, 0x7ffu, 0, have_hist));
            WT_TRY(select_pass(p, b, st, 0x7ff00000u, 10, 0x3ffu, 0));
        }
        WT_TRY(select_pass(p, b, st, 0x7ffffc00u, 0, 0x3ffu, 1));
        WT_HIP(hipMemcpyAsync((char *)c->h_pinned + 64, st, sizeof(WtSelectState), hipMemcpyDeviceToHost, c->stream));
        WT_HIP(hipStreamSynchronize(c->stream));             // the one host round trip of the select
        res_st = *(const WtSelectState *)((const char *)c->h_pinned + 64);
        return 0;
    };
    // No riding histogram (a plane of a bilateral / recursive / generic transform, or an edited one):
    // the same window, placed from a 4096-sample of the plane itself, lets ONE pass bin the top 21 bits
    // - two passes over the plane instead of three.
    bool window = windowed;
    if (!pre && g_opt_hist_window && p->nranks == 1 && N >= ((int64_t)1 << 20) && p->g.H >= 64 && p->g.W >= 64) {
        WT_HIP(hipMemsetAsync(c->d_hist, 0, WT_HIST_BINS * sizeof(uint32_t), c->stream));
        uint32_t *keys = (uint32_t *)c->d_partials;          // 16 KB of the reduction scratch (stream-ordered use)
        {
            ProfScope ps(c, "wt_median_window_kernel");
            hipLaunchKernelGGL(wt_plane_sample_kernel<float>, dim3(64), dim3(64), 0, c->stream, (const float *)b, p->g.nrows, p->g.W, p->g.P, keys);
            hipLaunchKernelGGL(wt_median_window_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t *)keys, hist_base_word(c));
        }
        {
            ProfScope ps(c, "wt_hist_kernel");
            const int X4 = (p->g.W + 3) / 4, nchunk = (X4 + 256 * WT_HIST_UNROLL - 1) / (256 * WT_HIST_UNROLL);
            const int64_t nitems = (int64_t)p->g.nrows * nchunk;
            hipLaunchKernelGGL((wt_hist_kernel<4, true>), dim3((unsigned)std::min<int64_t>(nitems, 4 * c->num_cus)), dim3(256), 0, c->stream,
                               (const float *)b, p->g.nrows, p->g.P / 4, p->g.W, 0u, (const WtSelectState *)st, 10, 0x7ffu, c->d_hist,
                               (const uint32_t *)hist_base_word(c));
        }
        WT_HIP(hipGetLastError());
        window = true;
    }
    WT_TRY(run(pre || window, window));
    if (window && res_st.failed == 3) WT_TRY(run(false, false));      // the window missed the median: the ordinary three passes
    if (res_st.failed) WT_FAIL("wt_abs_median: rank %lld not found (NaN input?)", (long long)klo);
    const int64_t cum_le = (int64_t)res_st.cum_le;           // elements <= v_lo
    const uint32_t ulo = res_st.prefix;
    uint32_t uhi = ulo;
    if ((N & 1) == 0 && cum_le < klo + 2) {
        // the upper median is the smallest element strictly greater than v_lo
        uint32_t *res = c->d_hist + WT_HIST_BINS;
        WT_HIP(hipMemsetAsync(res, 0xff, sizeof(uint32_t), c->stream));
        {
            ProfScope ps(c, "wt_min_greater_kernel");
            hipLaunchKernelGGL(wt_min_greater_kernel, dim3(std::min(p->g.nrows, 2048)), dim3(256), 0, c->stream, b, p->g.nrows, p->g.P / 4, p->g.W, ulo, res);
        }
        WT_HIP(hipGetLastError());
        if (p->nranks > 1) WT_NCCL(g_rccl.AllReduce(res, res, 1, NCCL_UINT32, NCCL_MIN, c->comm, c->stream));
        WT_HIP(hipMemcpyAsync(c->h_pinned, res, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        WT_HIP(hipStreamSynchronize(c->stream));
        uhi = *(const uint32_t *)c->h_pinned;
        if (uhi == 0xffffffffu) WT_FAIL("wt_abs_median: upper median not found");
    }
    float lo, hi;
    memcpy(&lo, &ulo, 4);
    memcpy(&hi, &uhi, 4);
    // np.median on float32: mean of the two middle values in float32
    *median = (N & 1) ? lo : (lo + hi) / 2.0f;
    return 0;
}

