// Batched float32 engine (wt_batch): N frames of the same H x W go through each fused pass in ONE launch,
// the frame index a grid dimension (blockIdx.z, wt_fused.h), instead of one API call per frame.
//
// Layout: every plane of the batch is one allocation of N frames back to back, frame f at f * H * P floats
// (P = the pitch of a wt_plan of the same width).  A plane is therefore also ONE tall image of N * H rows:
// pointwise work (transfers, Anscombe, the fused thresholds + plane sum) runs once over the whole stack.
// Only the fused passes see frames: each frame is its own image there (row reflection at the frame's
// borders), so a frame's bits are those of the per-frame call on a wt_plan of the same shape.
// The MAD median is a per-frame radix select (three histogram levels, 11 + 10 + 10 bits of |x|, the
// levels of wt_abs_median) over all frames at once, two ranks per frame for the upper median of an
// even pixel count: N medians for one host round trip.
// wow (watroo/utils.py:105-219) runs on a batch too: its per-scale update is the batched stencil of
// wt_stencil32_batch.hip (the frame's tau and factor from a small device table), the pointwise update, the
// {sum, sumsq, min, max} moments (one host round trip for all frames), the gamma blend, the fill and the plane
// sum run once over the stack, each frame with its own parameters and the bits of the per-frame call.
// richardson_lucy (watroo/utils.py:222-290) runs on a batch as well: the PSF correlation of all frames is one launch
// (wt_batch_filter2d_kernel, the frame as grid z, the two operands resident in the batch), the binary ops run once
// over the stack, the support update takes the frame's threshold from a device table.  With fft=True and a large PSF
// the two products of an iteration are wt_fft.h's six launches over all frames against one kernel spectrum
// (wt_batch_fft_spectrum / wt_batch_fft_apply).
// What lives where: this file has the float32 kernels and launch lines, the median select, the fused schedule and the
// FFT entry points.  The host side both engines share is wt_batch_core.h (planes, checks, tables, transfers, the
// loops of the transform) and wt_batch_rl.h (richardson_lucy's planes, PSFs and entry points); wt_rl_point.h has the
// correlation's tile body.  The three threshold sums are shells around one body (wt_batch_threshold_sum), the two
// pointwise wow kernels around another (wt_batch_wow_frame).
#include <algorithm>
#include <cstring>
#include <vector>

#include "wt_batch_rl.h"
#include "wt_reduce.h"
#include "wt_rng.h"
#include "wt_stencil_launch.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

struct WtBatchSel {                 // select state of one rank of one frame
    unsigned long long k;           // rank still to find among the keys matching `prefix`
    uint32_t prefix;                // key bits fixed so far
    uint32_t nan;                   // NaN pixels of the frame (counted by the first level)
};

struct wt_batch : WtBatchRl<float> {            // (richardson_lucy's planes and PSFs: wt_batch_rl.h; this batch's from its creation)
    wt_batch() : WtBatchRl<float>("wt_batch") {}
    wt_plan geo;                    // ONE frame's geometry, context and family: what the fused launches read (no planes)
    uint32_t *d_hist = nullptr;     // [n][2 ranks][WT_HIST_BINS]
    WtBatchSel *d_sel = nullptr;    // [n][2 ranks]
    WtBatchSel *h_sel = nullptr;    // pinned copy
    // (d_tau: [n][2 * WT_MAX_SUM_PLANES], the thresholds of wt_batch_denoise_sum; wt_batch_enhance_sum: then the weights)
    // richardson_lucy(fft=True): two complex work arrays of n frames, ONE kernel spectrum and the twiddle tables
    // (wt_fft.h), allocated by the first wt_batch_fft_spectrum
    WtFftState fft;
    std::vector<void *> fft_allocs;
};

// ------------------------------------------------------------------------------------------------ kernels
// One radix level of the per-frame select: bins of (key >> shift) & bmask over the keys of frame blockIdx.y
// that match a rank's prefix (key = magnitude bits of a float: their order is the order of |x|).
__global__ __launch_bounds__(256) void wt_batch_hist_kernel(const float *p, int H, int P, int W, int64_t fstride, uint32_t mask, int shift,
                                                            uint32_t bmask, WtBatchSel *st, uint32_t *hist)
{
    __shared__ uint32_t lh[2][WT_HIST_BINS];
    __shared__ uint32_t lnan;
    const int f = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * WT_HIST_BINS; i += 256) lh[i / WT_HIST_BINS][i % WT_HIST_BINS] = 0;
    if (threadIdx.x == 0) lnan = 0;
    __syncthreads();
    const uint32_t pre0 = st[2 * f].prefix, pre1 = st[2 * f + 1].prefix;
    const float *fp = p + (int64_t)f * fstride;
    const int W4 = (W + 3) / 4;
    const int64_t items = (int64_t)H * W4;
    uint32_t nan = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i / W4), c4 = (int)(i % W4);
        const float4 v = *reinterpret_cast<const float4 *>(fp + (int64_t)row * P + 4 * c4);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * c4 + j >= W) continue;
            const uint32_t key = __float_as_uint(e[j]) & 0x7fffffffu;
            nan += key > 0x7f800000u;
            if ((key & mask) == pre0) atomicAdd(&lh[0][(key >> shift) & bmask], 1u);
            if ((key & mask) == pre1) atomicAdd(&lh[1][(key >> shift) & bmask], 1u);
        }
    }
    if (nan) atomicAdd(&lnan, nan);
    __syncthreads();
    uint32_t *gh = hist + (int64_t)f * 2 * WT_HIST_BINS;
    for (int i = threadIdx.x; i < 2 * WT_HIST_BINS; i += 256) {
        const uint32_t c = lh[i / WT_HIST_BINS][i % WT_HIST_BINS];
        if (c) atomicAdd(&gh[i], c);
    }
    if (threadIdx.x == 0 && lnan && shift == 20) atomicAdd(&st[2 * f].nan, lnan);
}

// The bin of one rank (block = frame * 2 + rank): fixes bmask's bits of the prefix, leaves the bins cleared.
__global__ __launch_bounds__(256) void wt_batch_select_kernel(uint32_t *hist, WtBatchSel *st, int nbins, int shift)
{
    __shared__ unsigned long long part[256];
    __shared__ int sel_t;
    __shared__ unsigned long long sel_before;
    uint32_t *h = hist + (int64_t)blockIdx.x * WT_HIST_BINS;
    const int per = nbins / 256;
    unsigned long long s = 0;
    for (int i = 0; i < per; ++i) s += h[threadIdx.x * per + i];
    part[threadIdx.x] = s;
    __syncthreads();
    WtBatchSel &S = st[blockIdx.x];
    if (threadIdx.x == 0) {
        unsigned long long cum = 0;
        int t = 255;
        for (int i = 0; i < 256; ++i) {
            if (cum + part[i] > S.k) { t = i; break; }
            cum += part[i];
        }
        sel_t = t;
        sel_before = cum;
    }
    __syncthreads();
    if (threadIdx.x == sel_t) {
        unsigned long long cum = sel_before;
        int b = threadIdx.x * per + per - 1;
        for (int i = 0; i < per; ++i) {
            const uint32_t c = h[threadIdx.x * per + i];
            if (cum + c > S.k) { b = threadIdx.x * per + i; break; }
            cum += c;
        }
        S.prefix |= (uint32_t)b << shift;
        S.k -= cum;
    }
    __syncthreads();
    for (int i = 0; i < per; ++i) h[threadIdx.x * per + i] = 0;
}

// (`block`: blockDim.x, read by the shells - only inside a kernel does the compiler fold it to the one load the
//  launch bound allows - and handed to the shared bodies below)
// wt_denoise_sum_kernel (wt_kernels_apps.h) over the frames as one flat range, the frame from the flat index and its
// row of the table: ft[k] = the threshold of plane k.  Same arithmetic, contraction off: the bits of the per-frame call.
//   NOISE   nn comes from the batch's noise plane at the same flat index, as wt_denoise_sum_kernel reads its noise
//           plane (Coefficients.significance with an ndarray noise, watroo/wavelets.py:133-141; a frame whose noise is
//           a scalar has ones in its slot: tauf * 1.f and t * 1.0 are exact); else nn = 1
//   ROW_WGT the weight is the frame's too (utils.enhance per channel, watroo/utils.py:60-78): rows of 2 * n_den,
//           ft[n_den + k] a double rounded to float here as wt_denoise_sum rounds it on the host; else a.wgt[k]
struct BatchDenoiseArgs {
    float *p[WT_MAX_SUM_PLANES];
    float wgt[WT_MAX_SUM_PLANES];
    int n, n_den, soft, write_back;
};
struct BatchEnhanceArgs {
    float *p[WT_MAX_SUM_PLANES];
    int n, n_den, soft, write_back;
};
template <bool NOISE, bool ROW_WGT, typename Args>
__device__ __forceinline__ void wt_batch_threshold_sum(const Args &a, const double *tab, const float *noise, float *out, int64_t n4, int64_t f4,
                                                       unsigned block)
{
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * block + threadIdx.x; i < n4; i += (int64_t)gridDim.x * block) {
        const double *ft = tab + (ROW_WGT ? (i / f4) * 2 * a.n_den : (i / f4) * a.n_den);
        float nn[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (NOISE) {
            const float4 nz = reinterpret_cast<const float4 *>(noise)[i];
            nn[0] = nz.x; nn[1] = nz.y; nn[2] = nz.z; nn[3] = nz.w;
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.n; ++k) {
            const float4 v = reinterpret_cast<const float4 *>(a.p[k])[i];
            float c[4] = {v.x, v.y, v.z, v.w};
            if (k < a.n_den) {
                const double t = ft[k];
                const float tauf = (float)t;
                float wgt;
                if constexpr (ROW_WGT) wgt = (float)ft[a.n_den + k];
                else wgt = a.wgt[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sgn = t > 0.0 ? wt_sig(c[j], tauf * nn[j], t * (double)nn[j], a.soft) : 1.f;
                    c[j] = c[j] * (wgt * sgn);
                }
                if (a.write_back) reinterpret_cast<float4 *>(a.p[k])[i] = make_float4(c[0], c[1], c[2], c[3]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = k == 0 ? c[j] : acc[j] + c[j];
        }
        reinterpret_cast<float4 *>(out)[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}
__global__ __launch_bounds__(256) void wt_batch_denoise_sum_kernel(BatchDenoiseArgs a, const double *tau, float *out, int64_t n4, int64_t f4)
{
    wt_batch_threshold_sum<false, false>(a, tau, nullptr, out, n4, f4, blockDim.x);
}
__global__ __launch_bounds__(256) void wt_batch_denoise_sum_map_kernel(BatchDenoiseArgs a, const double *tau, const float *noise, float *out,
                                                                       int64_t n4, int64_t f4)
{
    wt_batch_threshold_sum<true, false>(a, tau, noise, out, n4, f4, blockDim.x);
}
__global__ __launch_bounds__(256) void wt_batch_enhance_sum_kernel(BatchEnhanceArgs a, const double *tab, float *out, int64_t n4, int64_t f4)
{
    wt_batch_threshold_sum<false, true>(a, tab, nullptr, out, n4, f4, blockDim.x);
}

// wt_wow_kernel (wt_kernels_apps.h) with the frame as grid y: no power plane, the frame's {tau, factor} (wow's last
// plane, whitening=False, h >= 1 - watroo/utils.py:185-203).  NOISE: nn[k] from the frame's slot of the batch's noise
// plane, as wt_wow_kernel reads its noise plane (watroo/utils.py:199 on an ndarray noise, wavelets.py:133-141); else
// nn = 1.  Same wt_wow_point: the bits of the per-frame call.
template <bool NOISE>
__device__ __forceinline__ void wt_batch_wow_frame(float *c, const float *noise, float *gamma, int64_t f4, const double *ptab, int soft, unsigned block)
{
    const int f = blockIdx.y;
    const double tau = ptab[2 * f];
    const float tauf = (float)tau, factor = (float)ptab[2 * f + 1];
    float4 *cf = reinterpret_cast<float4 *>(c) + (int64_t)f * f4;
    const float4 *nf4 = NOISE ? reinterpret_cast<const float4 *>(noise) + (int64_t)f * f4 : nullptr;
    float4 *gf = gamma ? reinterpret_cast<float4 *>(gamma) + (int64_t)f * f4 : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * block + threadIdx.x; i < f4; i += (int64_t)gridDim.x * block) {
        const float4 v = cf[i];
        float nn[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (NOISE) {
            const float4 nz = nf4[i];
            nn[0] = nz.x; nn[1] = nz.y; nn[2] = nz.z; nn[3] = nz.w;
        }
        float4 gm = make_float4(0, 0, 0, 0);
        if (gf) gm = gf[i];
        float in[4] = {v.x, v.y, v.z, v.w};
        float gg[4] = {gm.x, gm.y, gm.z, gm.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) in[k] = wt_wow_point(in[k], 1.f, false, nn[k], tau, tauf, soft, factor, gg[k]);
        cf[i] = make_float4(in[0], in[1], in[2], in[3]);
        if (gf) gf[i] = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
}
__global__ __launch_bounds__(256) void wt_batch_wow_kernel(float *c, float *gamma, int64_t f4, const double *ptab, int soft)
{
    wt_batch_wow_frame<false>(c, nullptr, gamma, f4, ptab, soft, blockDim.x);
}
__global__ __launch_bounds__(256) void wt_batch_wow_map_kernel(float *c, const float *noise, float *gamma, int64_t f4, const double *ptab, int soft)
{
    wt_batch_wow_frame<true>(c, noise, gamma, f4, ptab, soft, blockDim.x);
}

// wt_gamma_kernel (wt_kernels_apps.h, watroo/utils.py:212-217) with the frame as grid y and its own {gmin, gmax}
__global__ __launch_bounds__(256) void wt_batch_gamma_kernel(float *recon, float *gamma, int64_t f4, const double *ptab, float inv_gamma, float h)
{
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const float gmin = (float)ptab[2 * f], gmax = (float)ptab[2 * f + 1];
    const float range = gmax - gmin;            // (wt_gamma_blend: the same float subtraction on the host)
    const float omh = 1.f - h;
    float4 *rf = reinterpret_cast<float4 *>(recon) + (int64_t)f * f4;
    float4 *gf = reinterpret_cast<float4 *>(gamma) + (int64_t)f * f4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 r = rf[i];
        const float4 gq = gf[i];
        const float rr[4] = {r.x, r.y, r.z, r.w};
        float gg[4] = {gq.x, gq.y, gq.z, gq.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = (gg[k] - gmin) / range;
            t = t < 0.f ? 0.f : t;
            t = t > 1.f ? 1.f : t;
            t = powf(t, inv_gamma);
            gg[k] = t;
            o[k] = omh * rr[k] + h * t;
        }
        rf[i] = make_float4(o[0], o[1], o[2], o[3]);
        gf[i] = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
}

__global__ __launch_bounds__(256) void wt_batch_fill_kernel(float *d, int64_t n4, float value)
{
    batch_fill_groups(reinterpret_cast<float4 *>(d), n4, make_float4(value, value, value, value), blockDim.x);
}
__global__ __launch_bounds__(256) void wt_batch_replicate_kernel(float *d, int64_t f4)
{
    batch_replicate_groups(reinterpret_cast<float4 *>(d), f4, blockDim.x);
}

// wt_filter2d_kernel (wt_kernels_apps.h) for the frames of a batch: wt_f2d_batch_tile (wt_rl_point.h).  !SKEW is the
// one wt_batch_filter2d launches; SKEW (measured slower) only on request.
template <bool WRAP, bool SKEW>
__global__ __launch_bounds__(256) void wt_batch_filter2d_kernel(const float *in, float *out, Geo g, int64_t fstride, const float *__restrict__ psf,
                                                                int kh, int kw, int ay, int ax)
{
    extern __shared__ float tile[];
    wt_f2d_batch_tile<WRAP, SKEW>(tile, in, out, g, fstride, psf, kh, kw, ay, ax);
}

// wt_mrs_kernel (wt_kernels_apps.h) with the frame as grid y and its own tau (ptab[2 * f]; <= 0: significance one);
// no noise map - richardson_lucy's noise is the data's MAD estimate.  Same wt_mrs_point: the bits of the per-frame call.
__global__ __launch_bounds__(256) void wt_batch_mrs_kernel(float *c, float *mrs, int64_t f4, const double *ptab, int soft, int persistent,
                                                           float inv_pow)
{
    const int f = blockIdx.y;
    const double tau = ptab[2 * f];
    const float tauf = (float)tau;
    float4 *cf = reinterpret_cast<float4 *>(c) + (int64_t)f * f4;
    float4 *mf = reinterpret_cast<float4 *>(mrs) + (int64_t)f * f4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = cf[i];
        const float4 m4 = mf[i];
        float cc[4] = {v.x, v.y, v.z, v.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) wt_mrs_point(cc[k], mm[k], 1.f, tau, tauf, soft, persistent, inv_pow);
        cf[i] = make_float4(cc[0], cc[1], cc[2], cc[3]);
        mf[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    }
}

// wt_binary_kernel (wt_kernels_apps.h) over the active frames, one flat range (wt_binary_point4)
__global__ __launch_bounds__(256) void wt_batch_binary_kernel(const float *a, const float *b, float *dst, int64_t n4, int op)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<float4 *>(dst)[i] = wt_binary_point4(reinterpret_cast<const float4 *>(a)[i], reinterpret_cast<const float4 *>(b)[i], op);
}

// wt_reduce_kernel + wt_reduce_final_kernel per frame (grid y / the final block = the frame): the per-frame
// work split (gridDim.x blocks) and fold order of wt_reduce.h, i.e. the doubles of the per-frame call
#define WT_REDUCE_KERNEL_NAME wt_batch_reduce_kernel
#define WT_REDUCE_KERNEL_BATCH 1
#include "wt_reduce_rows.h"
#undef WT_REDUCE_KERNEL_NAME
#undef WT_REDUCE_KERNEL_BATCH
__global__ __launch_bounds__(256) void wt_batch_reduce_final_kernel(const double *partials, int nblocks, double *out)
{
    wt_reduce_final_block(partials + (int64_t)blockIdx.x * nblocks * 4, nblocks, out + (int64_t)blockIdx.x * 4);
}

// ------------------------------------------------------------------------------------------------ host
// the fused schedule of `level` scales, or an error: the passes with a sum run fused kernels only; `single`: a
// single-scale pass without a fused kernel runs the batched MODE_DECOMP stencil (as wt_decompose_pass on a plan)
static int batch_schedule(wt_batch *b, int level, int32_t *tr, int *np, const char *who, bool single)
{
    if (level < 1 || level > b->max_level) WT_FAIL("%s: level %d outside [1, %d]", who, level, b->max_level);
    WT_TRY(wt_schedule(b->family, level, 1, tr, 32, np));
    for (int i = 0; i < *np; ++i)
        if (!wt_fused_has_pass(tr[3 * i], tr[3 * i + 1], b->family) && !(single && tr[3 * i + 1] == 1))
            WT_FAIL("%s: %d scales have no all-fused schedule (wt_plan_fused_ok): not a batch case", who, level);
    return 0;
}

static int batch_pass(wt_batch *b, int nf, int cur, int nxt, int s0, int ns, int acc, int sum_plane, bool first)
{
    float *in = nullptr, *oc = nullptr, *ps = nullptr, *ow[WT_FUSED_MAX_SCALES] = {nullptr};
    WT_TRY(batch_pass_planes(b, cur, nxt, s0, ns, acc, sum_plane, first, &in, &oc, ow, &ps));
    FusedRows rows;
    rows.frames = nf;
    rows.fstride = b->fstride;
    return wt_fused_launch(&b->geo, in, oc, ow, s0, ns, acc, first ? nullptr : ps, ps, rows);
}

static int batch_run(wt_batch *b, int nf, int src, int level, bool with_sum, int dst, const char *who)
{
    return batch_schedule_run(
        b, nf, src, level, with_sum, dst, who,
        [b](int lv, bool sum, int32_t *tr, int *np, const char *w) { return batch_schedule(b, lv, tr, np, w, !sum); },
        [b](int frames, int cur, int nxt, int s0, int ns, int acc, int sum_plane, bool first) {
            return batch_pass(b, frames, cur, nxt, s0, ns, acc, sum_plane, first);
        });
}

// every buffer of the batch back to the runtime: the core's and the float32 engine's own
static void batch_free(wt_batch *b, int *bad)
{
    batch_release(b, bad);
    auto f = [&](void *q) { if (q && hipFree(q) != hipSuccess) *bad = 1; };
    f(b->d_hist);
    f(b->d_sel);
    batch_rl_release(b, bad);
    for (void *q : b->fft_allocs) f(q);
    if (b->h_sel && hipHostFree(b->h_sel) != hipSuccess) *bad = 1;
}

extern "C" int wt_batch_create(wt_ctx *ctx, int n, int H, int W, int family, int max_level, wt_batch **out)
{
    WtGuard guard_(ctx);
    WT_TRY(batch_check_create(ctx, out, n, H, W, family, max_level, "wt_batch_create"));
    wt_batch *b = new wt_batch;
    batch_init(b, ctx, n, H, W, (W + 3) / 4 * 4, family, max_level);
    b->geo.ctx = ctx;
    b->geo.family = family;
    b->geo.max_level = max_level;
    b->geo.g = b->g;
    batch_rl_own_planes(b);
    if (!wt_fused_supported(&b->geo)) {
        delete b;
        WT_FAIL("wt_batch_create: rows of %d pixels are too wide for the fused passes", W);
    }
    hipError_t e = hipMalloc((void **)&b->d_hist, (size_t)n * 2 * WT_HIST_BINS * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_sel, (size_t)n * 2 * sizeof(WtBatchSel));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_tau, (size_t)n * 2 * WT_MAX_SUM_PLANES * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_sel, (size_t)n * 2 * sizeof(WtBatchSel), 0);
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_tau, (size_t)n * 2 * WT_MAX_SUM_PLANES * sizeof(double), 0);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_hist, 0, (size_t)n * 2 * WT_HIST_BINS * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) {
        int bad = 0;
        batch_free(b, &bad);
        delete b;
        wt_set_error("wt_batch_create: HIP error %d (%s)", (int)e, hipGetErrorString(e));
        return 2;
    }
    *out = b;
    return 0;
}

extern "C" int wt_batch_destroy(wt_batch *b)
{
    if (!b) return 0;
    WtGuard guard_(b->ctx);
    (void)hipStreamSynchronize(b->ctx->stream);
    int bad = 0;
    batch_free(b, &bad);
    delete b;
    if (bad) WT_FAIL("wt_batch_destroy: a device buffer could not be released");
    return 0;
}

extern "C" int wt_batch_info(wt_batch *b, int64_t *info)
{
    return batch_info(b, info, "wt_batch_info");
}

wt_ctx *wt_batch_ctx(wt_batch *b) { return b->ctx; }

extern "C" int wt_batch_plane_ptr(wt_batch *b, int plane, void **ptr, int64_t *frame_stride)
{
    return batch_plane_ptr(b, plane, ptr, frame_stride, "wt_batch_plane_ptr");
}

extern "C" int wt_batch_upload(wt_batch *b, int plane, int f0, int nf, const float *host, int64_t host_frame_stride)
{
    return batch_copy(b, plane, f0, nf, const_cast<float *>(host), host_frame_stride, true, "wt_batch_upload");
}

extern "C" int wt_batch_download(wt_batch *b, int plane, int f0, int nf, float *host, int64_t host_frame_stride)
{
    return batch_copy(b, plane, f0, nf, host, host_frame_stride, false, "wt_batch_download");
}

extern "C" int wt_batch_decompose(wt_batch *b, int nf, int src, int level, int flags)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_decompose"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose: a batch runs the fused passes (flags bit0)");
    if (level == 0) {
        float *s = nullptr;
        if (src == 0) WT_FAIL("wt_batch_decompose: src plane 0 is the output plane");
        WT_TRY(batch_plane(b, src, &s));
        return batch_copy_to_plane0(b, nf, s);
    }
    return batch_run(b, nf, src, level, false, WT_PLANE_NONE, "wt_batch_decompose");
}

// wt_decompose_bilateral (wt_transform.hip) for the active frames: batch_decompose_bilateral's loop on the batched
// march of wt_bilateral32_batch.hip; no two-kernel form, no side-stream overlap.
extern "C" int wt_batch_decompose_bilateral(wt_batch *b, int nf, int src, int level, const double *sigma_b, int bilateral_scaling, int flags)
{
    (void)flags;
    WT_TRY(batch_check_frames(b, nf, "wt_batch_decompose_bilateral"));
    WtGuard guard_(b->ctx);
    return batch_decompose_bilateral(
        b, nf, src, level, sigma_b, bilateral_scaling, "wt_batch_decompose_bilateral", [] { return 0; },
        [b](const ChainArgs &a, int s, const WtFrames &fr) {
            return wt32_bilateral_batch_launch(batch_stencil_ctx(b), a, s, g_opt_bilateral_paired != 0, fr);
        });
}

extern "C" int wt_batch_decompose_sum(wt_batch *b, int nf, int src, int level, int dst, int flags)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_decompose_sum"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose_sum: a batch runs the fused passes (flags bit0)");
    return batch_run(b, nf, src, level, true, dst, "wt_batch_decompose_sum");
}

extern "C" int wt_batch_decompose_pass(wt_batch *b, int nf, int cur, int nxt, int s0, int ns, int flags)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_decompose_pass"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose_pass: a batch runs the fused passes (flags bit0)");
    return batch_pass(b, nf, cur, nxt, s0, ns, 0, WT_PLANE_NONE, false);
}

extern "C" int wt_batch_decompose_pass_sum(wt_batch *b, int nf, int cur, int nxt, int s0, int ns, int flags, int sum_plane, int first,
                                           int last)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_decompose_pass_sum"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose_pass_sum: a batch runs the fused passes (flags bit0)");
    return batch_pass(b, nf, cur, nxt, s0, ns, last ? 2 : 1, sum_plane, first != 0);
}

extern "C" int wt_batch_abs_median(wt_batch *b, int nf, int plane, float *medians)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_abs_median"));
    if (!medians) WT_FAIL("wt_batch_abs_median: null pointer");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    float *q = nullptr;
    WT_TRY(batch_plane(b, plane, &q));
    const Geo &g = b->geo.g;
    const int64_t N = (int64_t)g.H * g.W;
    const unsigned long long klo = (unsigned long long)((N - 1) / 2);
    for (int f = 0; f < nf; ++f)
        for (int r = 0; r < 2; ++r) b->h_sel[2 * f + r] = WtBatchSel{klo + ((N & 1) == 0 && r == 1 ? 1ull : 0ull), 0u, 0u};
    WT_HIP(hipMemcpyAsync(b->d_sel, b->h_sel, (size_t)nf * 2 * sizeof(WtBatchSel), hipMemcpyHostToDevice, c->stream));
    const int64_t items = (int64_t)g.H * ((g.W + 3) / 4);
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>((items + 2047) / 2048, std::max(1, 8 * c->num_cus / nf)));
    const uint32_t masks[3] = {0u, 0x7ff00000u, 0x7ffffc00u};
    const int shifts[3] = {20, 10, 0};
    const uint32_t bmasks[3] = {0x7ffu, 0x3ffu, 0x3ffu};
    for (int lv = 0; lv < 3; ++lv) {
        {
            ProfScope ps(c, "wt_batch_hist_kernel");
            hipLaunchKernelGGL(wt_batch_hist_kernel, dim3(bx, nf), dim3(256), 0, c->stream, (const float *)q, g.H, g.P, g.W, b->fstride, masks[lv],
                               shifts[lv], bmasks[lv], b->d_sel, b->d_hist);
        }
        {
            ProfScope ps(c, "wt_batch_select_kernel");
            hipLaunchKernelGGL(wt_batch_select_kernel, dim3(2 * nf), dim3(256), 0, c->stream, b->d_hist, b->d_sel, (int)bmasks[lv] + 1, shifts[lv]);
        }
        WT_HIP(hipGetLastError());
    }
    WT_HIP(hipMemcpyAsync(b->h_sel, b->d_sel, (size_t)nf * 2 * sizeof(WtBatchSel), hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));               // the one host round trip for all nf medians
    for (int f = 0; f < nf; ++f)
        if (b->h_sel[2 * f].nan) WT_FAIL("wt_batch_abs_median: frame %d holds %u NaN pixels", f, b->h_sel[2 * f].nan);
    for (int f = 0; f < nf; ++f) {
        float lo, hi;
        memcpy(&lo, &b->h_sel[2 * f].prefix, 4);
        memcpy(&hi, &b->h_sel[2 * f + 1].prefix, 4);
        // np.median on float32: mean of the two middle values in float32 (as wt_abs_median)
        medians[f] = (N & 1) ? lo : (lo + hi) / 2.0f;
    }
    return 0;
}

// wt_batch_denoise_sum / wt_batch_denoise_sum_map: noise_plane == WT_PLANE_NONE runs the kernel without a map
static int batch_denoise_sum(wt_batch *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft, int write_back,
                             int noise_plane, const char *who)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    WT_TRY(batch_check_sum(b, count, dst, n_den, 0, tau, wgt, who));
    if (noise_plane != WT_PLANE_NONE && (noise_plane == dst || (noise_plane >= 0 && noise_plane < count)))
        WT_FAIL("%s: the noise plane %d is a plane of the sum", who, noise_plane);
    BatchDenoiseArgs a{};
    float *o = nullptr, *nz = nullptr;
    WT_TRY(batch_sum_args(b, count, dst, n_den, soft, write_back, &a, &o));
    for (int i = 0; i < count; ++i) a.wgt[i] = i < n_den ? (float)wgt[i] : 1.f;
    if (noise_plane != WT_PLANE_NONE) WT_TRY(batch_plane(b, noise_plane, &nz));
    // rows of n_den thresholds (one 0.0 when no plane is thresholded)
    const int nt = std::max(n_den, 1);
    WT_TRY(batch_sum_table(b, nf, nt, [&](int f, double *r) {
        for (int k = 0; k < nt; ++k) r[k] = n_den ? tau[f * nt + k] : 0.0;
    }));
    const int64_t n4 = (int64_t)nf * b->fstride / 4;
    if (nz) {
        ProfScope ps(b->ctx, "wt_batch_denoise_sum_map_kernel");
        hipLaunchKernelGGL(wt_batch_denoise_sum_map_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, b->ctx->stream, a,
                           (const double *)b->d_tau, (const float *)nz, o, n4, b->fstride / 4);
    } else {
        ProfScope ps(b->ctx, "wt_batch_denoise_sum_kernel");
        hipLaunchKernelGGL(wt_batch_denoise_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, b->ctx->stream, a,
                           (const double *)b->d_tau, o, n4, b->fstride / 4);
    }
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch_denoise_sum(wt_batch *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft,
                                    int write_back)
{
    return batch_denoise_sum(b, nf, count, dst, n_den, tau, wgt, soft, write_back, WT_PLANE_NONE, "wt_batch_denoise_sum");
}

extern "C" int wt_batch_denoise_sum_map(wt_batch *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft,
                                        int write_back, int noise_plane)
{
    if (noise_plane == WT_PLANE_NONE) WT_FAIL("wt_batch_denoise_sum_map: no noise plane (wt_batch_denoise_sum is the call without a map)");
    return batch_denoise_sum(b, nf, count, dst, n_den, tau, wgt, soft, write_back, noise_plane, "wt_batch_denoise_sum_map");
}

extern "C" int wt_batch_enhance_sum(wt_batch *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft,
                                    int write_back)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_enhance_sum"));
    WtGuard guard_(b->ctx);
    WT_TRY(batch_check_sum(b, count, dst, n_den, 1, tau, wgt, "wt_batch_enhance_sum"));
    BatchEnhanceArgs a{};
    float *o = nullptr;
    WT_TRY(batch_sum_args(b, count, dst, n_den, soft, write_back, &a, &o));
    // rows of n_den thresholds, then n_den weights (nf <= n, n_den <= WT_MAX_SUM_PLANES: within the tables)
    WT_TRY(batch_sum_table(b, nf, 2 * n_den, [&](int f, double *r) {
        for (int k = 0; k < n_den; ++k) {
            r[k] = tau[f * n_den + k];
            r[n_den + k] = wgt[f * n_den + k];
        }
    }));
    const int64_t n4 = (int64_t)nf * b->fstride / 4;
    ProfScope ps(b->ctx, "wt_batch_enhance_sum_kernel");
    hipLaunchKernelGGL(wt_batch_enhance_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, b->ctx->stream, a, (const double *)b->d_tau,
                       o, n4, b->fstride / 4);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch_anscombe(wt_batch *b, int nf, int src, int dst, float alpha, float g, float sigma, int inverse)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_anscombe"));
    WtGuard guard_(b->ctx);
    if (alpha == 0.f) WT_FAIL("wt_batch_anscombe: alpha must be non-zero");
    float *s = nullptr, *d = nullptr;
    WT_TRY(batch_plane(b, src, &s));
    WT_TRY(batch_plane(b, dst, &d));
    return launch_anscombe(b->ctx, s, d, (int64_t)nf * b->fstride / 4, alpha, g, sigma, inverse);
}

// ------------------------------------------------------------------------------------------------ wow
extern "C" int wt_batch_fill(wt_batch *b, int nf, int plane, float value)
{
    return batch_fill(b, nf, plane, "wt_batch_fill", [&](float *d) {
        const int64_t n4 = (int64_t)nf * b->fstride / 4;
        ProfScope ps(b->ctx, "wt_batch_fill_kernel");
        hipLaunchKernelGGL(wt_batch_fill_kernel, dim3(flat_grid(n4)), dim3(256), 0, b->ctx->stream, d, n4, value);
    });
}

extern "C" int wt_batch_replicate(wt_batch *b, int nf, int plane)
{
    return batch_replicate(b, nf, plane, "wt_batch_replicate", [&](float *d) {
        const int64_t f4 = b->fstride / 4;
        ProfScope ps(b->ctx, "wt_batch_replicate_kernel");
        hipLaunchKernelGGL(wt_batch_replicate_kernel, dim3(batch_frame_blocks(f4, nf), nf - 1), dim3(256), 0, b->ctx->stream, d, f4);
    });
}

// frame f of the plane <- the field wt_fill_normal(seed, first_trial + f) gives a wt_plan of the frame's shape
extern "C" int wt_batch_fill_normal(wt_batch *b, int nf, int plane, uint64_t seed, uint32_t first_trial)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_fill_normal"));
    WtGuard guard_(b->ctx);
    float *d = nullptr;
    WT_TRY(batch_plane(b, plane, &d));
    return wt_launch_fill_normal(b->ctx, d, b->geo.g, b->geo.g.H, nf, b->fstride, seed, first_trial);
}

// wt_batch_wow_update / wt_batch_wow_update_map: noise_plane == WT_PLANE_NONE runs the kernel without a map
static int batch_wow_update(wt_batch *b, int nf, int plane, const double *tau, int soft, const float *factor, int gamma_plane, int noise_plane,
                            const char *who)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    float *c = nullptr, *gm = nullptr, *nz = nullptr;
    const double *dt = nullptr;
    WT_TRY(batch_wow_update_args(b, nf, plane, tau, factor, gamma_plane, noise_plane, who, &c, &gm, &nz, &dt));
    if (nz) {
        ProfScope ps(b->ctx, "wt_batch_wow_map_kernel");
        hipLaunchKernelGGL(wt_batch_wow_map_kernel, dim3(batch_frame_blocks(b->fstride / 4, nf), nf), dim3(256), 0, b->ctx->stream, c, (const float *)nz, gm,
                           b->fstride / 4, dt, soft);
    } else {
        ProfScope ps(b->ctx, "wt_batch_wow_kernel");
        hipLaunchKernelGGL(wt_batch_wow_kernel, dim3(batch_frame_blocks(b->fstride / 4, nf), nf), dim3(256), 0, b->ctx->stream, c, gm, b->fstride / 4, dt, soft);
    }
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch_wow_update(wt_batch *b, int nf, int plane, const double *tau, int soft, const float *factor, int gamma_plane)
{
    return batch_wow_update(b, nf, plane, tau, soft, factor, gamma_plane, WT_PLANE_NONE, "wt_batch_wow_update");
}

extern "C" int wt_batch_wow_update_map(wt_batch *b, int nf, int plane, const double *tau, int soft, const float *factor, int gamma_plane,
                                       int noise_plane)
{
    if (noise_plane == WT_PLANE_NONE) WT_FAIL("wt_batch_wow_update_map: no noise plane (wt_batch_wow_update is the call without a map)");
    return batch_wow_update(b, nf, plane, tau, soft, factor, gamma_plane, noise_plane, "wt_batch_wow_update_map");
}

// wt_batch_wow_scale / wt_batch_wow_scale_map: noise_plane == WT_PLANE_NONE runs the instantiations without a map
static int batch_wow_scale(wt_batch *b, int nf, int plane, int s, const double *tau, int soft, const float *factor, int gamma_plane, int noise_plane,
                           const char *who)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    WT_TRY(batch_check_wow_scale(b, plane, s, who));
    return batch_wow_scale_run(b, nf, plane, s, tau, soft, factor, gamma_plane, noise_plane, who);
}

extern "C" int wt_batch_wow_scale(wt_batch *b, int nf, int plane, int s, const double *tau, int soft, const float *factor, int gamma_plane)
{
    return batch_wow_scale(b, nf, plane, s, tau, soft, factor, gamma_plane, WT_PLANE_NONE, "wt_batch_wow_scale");
}

extern "C" int wt_batch_wow_scale_map(wt_batch *b, int nf, int plane, int s, const double *tau, int soft, const float *factor, int gamma_plane,
                                      int noise_plane)
{
    if (noise_plane == WT_PLANE_NONE) WT_FAIL("wt_batch_wow_scale_map: no noise plane (wt_batch_wow_scale is the call without a map)");
    return batch_wow_scale(b, nf, plane, s, tau, soft, factor, gamma_plane, noise_plane, "wt_batch_wow_scale_map");
}

extern "C" int wt_batch_reduce(wt_batch *b, int nf, int plane, double *out)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_reduce"));
    if (!out) WT_FAIL("wt_batch_reduce: null pointer");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    float *q = nullptr;
    WT_TRY(batch_plane(b, plane, &q));
    const Geo &g = b->geo.g;
    // (wt_reduce's work items: (row, chunk of 4096 pixels) pairs over at most partial_blocks blocks, per frame)
    const int blocks = (int)std::min<int64_t>((int64_t)g.H * ((g.W + 4095) / 4096), c->partial_blocks);
    WT_TRY(batch_reduce_buffers(b, blocks, false));
    {
        ProfScope ps(c, "wt_batch_reduce_kernel");
        hipLaunchKernelGGL(wt_batch_reduce_kernel, dim3(blocks, nf), dim3(256), 0, c->stream, (const float *)q, g.H, g.P / 4, g.W, b->fstride, b->d_red);
        hipLaunchKernelGGL(wt_batch_reduce_final_kernel, dim3(nf), dim3(256), 0, c->stream, (const double *)b->d_red, blocks, batch_reduce_results(b));
    }
    return batch_reduce_fetch(b, nf, out);
}

extern "C" int wt_batch_gamma_blend(wt_batch *b, int nf, int recon, int gamma_plane, const float *gmin, const float *gmax, float inv_gamma,
                                    float h)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_gamma_blend"));
    if (!gmin || !gmax) WT_FAIL("wt_batch_gamma_blend: null gmin / gmax");
    WtGuard guard_(b->ctx);
    if (recon == gamma_plane) WT_FAIL("wt_batch_gamma_blend: recon and gamma planes must differ");
    float *r = nullptr, *g = nullptr;
    WT_TRY(batch_plane(b, recon, &r));
    WT_TRY(batch_plane(b, gamma_plane, &g));
    const double *dt = nullptr;
    WT_TRY(batch_pairs(b, nf, gmin, gmax, &dt));
    ProfScope ps(b->ctx, "wt_batch_gamma_kernel");
    hipLaunchKernelGGL(wt_batch_gamma_kernel, dim3(batch_frame_blocks(b->fstride / 4, nf), nf), dim3(256), 0, b->ctx->stream, r, g, b->fstride / 4, dt, inv_gamma, h);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch_plane_sum(wt_batch *b, int nf, int first, int count, int dst)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_plane_sum"));
    WtGuard guard_(b->ctx);
    const float *planes[WT_MAX_SUM_PLANES];
    float *o = nullptr;
    WT_TRY(batch_plane_sum_planes(b, first, count, dst, WT_MAX_SUM_PLANES, "wt_batch_plane_sum", planes, &o));
    // the frames back to back are one flat range: wt_plane_sum_kernel over all of them
    return launch_plane_sum(b->ctx, planes, count, o, (int64_t)nf * b->fstride / 4);
}

// ------------------------------------------------------------------------------------------------ richardson_lucy
// (wt_batch_rl.h; the planes of richardson_lucy are this batch's from its creation on)
extern "C" int wt_batch_psf_ok(int kh, int kw, int *ok)
{
    return batch_psf_ok<float>(kh, kw, ok, "wt_batch_psf_ok");
}

extern "C" int wt_batch_set_psf(wt_batch *b, int slot, const float *kernel, int kh, int kw)
{
    return batch_set_psf(b, slot, kernel, kh, kw, "wt_batch_set_psf");
}

// (measured, tools/bench_rl_stack.py: the per-image tap loop is about twice as fast as the row-skewed one at every
//  shape - 10 to 18 against 5 to 10 TFMA/s - so the skewed loop runs only on request, for that measurement)
static int g_batch_f2d_plain = getenv("WT_BATCH_F2D_SKEW") ? 0 : 1;
extern "C" int wt_batch_filter2d(wt_batch *b, int nf, int src, int dst, int slot, int ay, int ax, int border)
{
    return batch_filter2d(b, nf, src, dst, slot, ay, ax, border, "wt_batch_filter2d", "wt_batch_filter2d_kernel", [](bool periodic) {
        if (periodic) return g_batch_f2d_plain ? wt_batch_filter2d_kernel<true, false> : wt_batch_filter2d_kernel<true, true>;
        return g_batch_f2d_plain ? wt_batch_filter2d_kernel<false, false> : wt_batch_filter2d_kernel<false, true>;
    });
}

extern "C" int wt_batch_binary(wt_batch *b, int nf, int op, int a, int b2, int dst)
{
    return batch_binary(b, nf, op, a, b2, dst, "wt_batch_binary", [&](const float *pa, const float *pb, float *pd) {
        const int64_t n4 = (int64_t)nf * b->fstride / 4;
        ProfScope ps(b->ctx, "wt_batch_binary_kernel");
        hipLaunchKernelGGL(wt_batch_binary_kernel, dim3(flat_grid(n4)), dim3(256), 0, b->ctx->stream, pa, pb, pd, n4, op);
    });
}

extern "C" int wt_batch_mrs_update(wt_batch *b, int nf, int plane, int mrs_plane, const double *tau, int soft, int persistent, float inv_pow)
{
    return batch_mrs_update(b, nf, plane, mrs_plane, tau, "wt_batch_mrs_update", [&](float *c, float *m, const double *dt) {
        const int64_t f4 = b->fstride / 4;
        ProfScope ps(b->ctx, "wt_batch_mrs_kernel");
        hipLaunchKernelGGL(wt_batch_mrs_kernel, dim3(batch_frame_blocks(f4, nf), nf), dim3(256), 0, b->ctx->stream, c, m, f4, dt, soft, persistent, inv_pow);
    });
}

// ---- the circular products of richardson_lucy(fft=True) through the FFT (wt_fft.h; watroo/utils.py:245-254, 284)
// host logic: *ok = 1 when a batch of H x W frames takes them - wt_fft_supported's rule on the frame shape
extern "C" int wt_batch_fft_ok(int64_t H, int64_t W, int *ok)
{
    if (!ok) WT_FAIL("wt_batch_fft_ok: null pointer");
    return wt_fft_supported(H, W, ok);
}

// The kernel spectrum of the batch <- FFT2 of FRAME 0 of plane `src` (fft_psf of watroo/utils.py:246-251: the caller
// uploads the periodically placed PSF there), once per call of the stack function: every chunk multiplies by it.
extern "C" int wt_batch_fft_spectrum(wt_batch *b, int src)
{
    if (!b) WT_FAIL("wt_batch_fft_spectrum: null batch");
    WtGuard guard_(b->ctx);
    const Geo &g = b->geo.g;
    int ok = 0;
    WT_TRY(wt_fft_supported(g.H, g.W, &ok));
    if (!ok) WT_FAIL("wt_batch_fft_spectrum: a side of the %d x %d frames has a prime factor above 5 (or lies outside 2 .. 8192)", g.H, g.W);
    float *s = nullptr;
    WT_TRY(batch_plane(b, src, &s));
    b->fft.have_spec = false;
    WT_TRY(wt_fft32_prepare(b->ctx, b->fft, g.H, g.W, b->fft_allocs, b->n));
    return wt_fft32_spectrum(b->ctx, b->fft, s, g.P);
}

// wt_fft_apply per frame (watroo/utils.py:254: irfft2(rfft2(psi) * fft_psf); conj, utils.py:284: * conj(fft_psf)) with
// the batch's one kernel spectrum: six launches for all active frames, no stream drain, no host round trip
extern "C" int wt_batch_fft_apply(wt_batch *b, int nf, int src, int dst, int conj)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch_fft_apply"));
    WtGuard guard_(b->ctx);
    if (src == dst) WT_FAIL("wt_batch_fft_apply: src and dst must differ");
    float *s = nullptr, *d = nullptr;
    WT_TRY(batch_plane(b, src, &s));
    WT_TRY(batch_plane(b, dst, &d));
    if (!b->fft.have_spec) WT_FAIL("wt_batch_fft_apply: the batch has no kernel spectrum (wt_batch_fft_spectrum first)");
    return wt_fft32_apply(b->ctx, b->fft, s, d, b->geo.g.P, conj, nf, b->fstride);
}
