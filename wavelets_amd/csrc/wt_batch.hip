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
#include <algorithm>
#include <cstring>
#include <vector>

#include "wt_host.h"
#include "wt_fused_decl.h"
#include "wt_reduce.h"
#include "wt_rl_point.h"
#include "wt_rng.h"
#include "wt_stencil_launch.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

struct WtBatchSel {                 // select state of one rank of one frame
    unsigned long long k;           // rank still to find among the keys matching `prefix`
    uint32_t prefix;                // key bits fixed so far
    uint32_t nan;                   // NaN pixels of the frame (counted by the first level)
};

struct wt_batch {
    wt_ctx *ctx = nullptr;
    wt_plan geo;                    // ONE frame's geometry, context and family: what the fused launches read (no planes)
    int n = 0, max_level = 0;
    int64_t fstride = 0;            // floats from one frame to the next (H * P)
    std::vector<float *> coef;      // planes 0 .. max_level
    float *input = nullptr, *out = nullptr, *scr[2] = {nullptr, nullptr};
    uint32_t *d_hist = nullptr;     // [n][2 ranks][WT_HIST_BINS]
    WtBatchSel *d_sel = nullptr;    // [n][2 ranks]
    WtBatchSel *h_sel = nullptr;    // pinned copy
    double *d_tau = nullptr;        // [n][2 * WT_MAX_SUM_PLANES]: thresholds of wt_batch_denoise_sum; wt_batch_enhance_sum: then the weights
    double *h_tau = nullptr;        // pinned staging of the table
    // wow: WT_PLANE_SCRATCH(3) = the output plane of wt_batch_wow_scale (swapped with the coefficient plane, as
    // wt_wow_scale does), WT_PLANE_SCRATCH(4) = the gamma accumulator (utils.wow's plane ids)
    float *spare = nullptr, *gamma = nullptr;
    float *noise = nullptr;         // WT_PLANE_SCRATCH(5): the per-pixel noise maps of the frames (Coefficients' noise plane id)
    // richardson_lucy: WT_PLANE_SCRATCH(6 .. 10) = data, psi, phi, residual, correlation; WT_PLANE_SCRATCH(16 + s) = the
    // support plane of scale s (utils.richardson_lucy's plane ids); the forward / backward PSF of wt_batch_set_psf
    float *rl[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<float *> mrs;       // max_level entries
    float *d_psf[2] = {nullptr, nullptr};
    size_t psf_cap[2] = {0, 0};
    int psf_kh[2] = {0, 0}, psf_kw[2] = {0, 0};
    // richardson_lucy(fft=True): two complex work arrays of n frames, ONE kernel spectrum and the twiddle tables
    // (wt_fft.h), allocated by the first wt_batch_fft_spectrum
    WtFftState fft;
    std::vector<void *> fft_allocs;
    // per-frame parameter pairs of one launch ({tau, factor}, {gmin, gmax}): a ring of table slots [n][2], pinned
    // staging + device copy; a slot is refilled only after the copy that last read it has completed (its event)
    static constexpr int kTabSlots = 16;
    double *d_ptab = nullptr, *h_ptab = nullptr;
    hipEvent_t ptab_ev[kTabSlots] = {};
    int ptab_next = 0;
    // wt_batch_reduce: [n][red_blocks][4] partials + [n][4] results on the device, [n][4] pinned
    double *d_red = nullptr, *h_red = nullptr;
    int red_blocks = 0;
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

// wt_denoise_sum_kernel (wt_kernels_apps.h) with one threshold row per frame: tau[frame * n_den + k], the frame
// from the flat index.  Same arithmetic (no noise plane: nn = 1), contraction off: the bits of the per-frame call.
struct BatchDenoiseArgs {
    float *p[WT_MAX_SUM_PLANES];
    float wgt[WT_MAX_SUM_PLANES];
    int n, n_den, soft, write_back;
};
__global__ __launch_bounds__(256) void wt_batch_denoise_sum_kernel(BatchDenoiseArgs a, const double *tau, float *out, int64_t n4, int64_t f4)
{
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const double *ft = tau + (i / f4) * a.n_den;
        const float nn[4] = {1.f, 1.f, 1.f, 1.f};
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.n; ++k) {
            const float4 v = reinterpret_cast<const float4 *>(a.p[k])[i];
            float c[4] = {v.x, v.y, v.z, v.w};
            if (k < a.n_den) {
                const double t = ft[k];
                const float tauf = (float)t;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sgn = t > 0.0 ? wt_sig(c[j], tauf * nn[j], t * (double)nn[j], a.soft) : 1.f;
                    c[j] = c[j] * (a.wgt[k] * sgn);
                }
                if (a.write_back) reinterpret_cast<float4 *>(a.p[k])[i] = make_float4(c[0], c[1], c[2], c[3]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = k == 0 ? c[j] : acc[j] + c[j];
        }
        reinterpret_cast<float4 *>(out)[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// wt_batch_denoise_sum_kernel with a per-pixel noise map (Coefficients.significance with an ndarray noise,
// watroo/wavelets.py:133-141): nn comes from the batch's noise plane at the same flat index, as wt_denoise_sum_kernel
// reads its noise plane.  A frame whose noise is a scalar has ones in its slot of the plane (tauf * 1.f and
// t * 1.0 are exact).  Same arithmetic, contraction off: the bits of the per-frame call.
__global__ __launch_bounds__(256) void wt_batch_denoise_sum_map_kernel(BatchDenoiseArgs a, const double *tau, const float *noise, float *out,
                                                                       int64_t n4, int64_t f4)
{
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const double *ft = tau + (i / f4) * a.n_den;
        const float4 nz = reinterpret_cast<const float4 *>(noise)[i];
        const float nn[4] = {nz.x, nz.y, nz.z, nz.w};
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.n; ++k) {
            const float4 v = reinterpret_cast<const float4 *>(a.p[k])[i];
            float c[4] = {v.x, v.y, v.z, v.w};
            if (k < a.n_den) {
                const double t = ft[k];
                const float tauf = (float)t;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sgn = t > 0.0 ? wt_sig(c[j], tauf * nn[j], t * (double)nn[j], a.soft) : 1.f;
                    c[j] = c[j] * (a.wgt[k] * sgn);
                }
                if (a.write_back) reinterpret_cast<float4 *>(a.p[k])[i] = make_float4(c[0], c[1], c[2], c[3]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = k == 0 ? c[j] : acc[j] + c[j];
        }
        reinterpret_cast<float4 *>(out)[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// wt_batch_denoise_sum_kernel with one WEIGHT row per frame as well (utils.enhance per channel, watroo/utils.py:60-78):
// tab[frame * 2 * n_den + k] = tau, tab[frame * 2 * n_den + n_den + k] = the weight (a double, rounded to float here as
// wt_denoise_sum rounds it on the host), the frame from the flat index.  Same arithmetic, contraction off: the bits of
// the per-frame call.
struct BatchEnhanceArgs {
    float *p[WT_MAX_SUM_PLANES];
    int n, n_den, soft, write_back;
};
__global__ __launch_bounds__(256) void wt_batch_enhance_sum_kernel(BatchEnhanceArgs a, const double *tab, float *out, int64_t n4, int64_t f4)
{
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const double *ft = tab + (i / f4) * 2 * a.n_den;
        const float nn[4] = {1.f, 1.f, 1.f, 1.f};
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.n; ++k) {
            const float4 v = reinterpret_cast<const float4 *>(a.p[k])[i];
            float c[4] = {v.x, v.y, v.z, v.w};
            if (k < a.n_den) {
                const double t = ft[k];
                const float tauf = (float)t, wgt = (float)ft[a.n_den + k];
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

// wt_wow_kernel (wt_kernels_apps.h) with the frame as grid y: no power plane, no noise map, the frame's {tau, factor}
// (wow's last plane, whitening=False, h >= 1 - watroo/utils.py:185-203).  Same wt_wow_point: the bits of the per-frame call.
__global__ __launch_bounds__(256) void wt_batch_wow_kernel(float *c, float *gamma, int64_t f4, const double *ptab, int soft)
{
    const int f = blockIdx.y;
    const double tau = ptab[2 * f];
    const float tauf = (float)tau, factor = (float)ptab[2 * f + 1];
    float4 *cf = reinterpret_cast<float4 *>(c) + (int64_t)f * f4;
    float4 *gf = gamma ? reinterpret_cast<float4 *>(gamma) + (int64_t)f * f4 : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = cf[i];
        float4 gm = make_float4(0, 0, 0, 0);
        if (gf) gm = gf[i];
        float in[4] = {v.x, v.y, v.z, v.w};
        float gg[4] = {gm.x, gm.y, gm.z, gm.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) in[k] = wt_wow_point(in[k], 1.f, false, 1.f, tau, tauf, soft, factor, gg[k]);
        cf[i] = make_float4(in[0], in[1], in[2], in[3]);
        if (gf) gf[i] = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
}

// wt_batch_wow_kernel with a per-pixel noise map (watroo/utils.py:199 on an ndarray noise, wavelets.py:133-141): nn[k]
// from the frame's slot of the batch's noise plane, as wt_wow_kernel reads its noise plane.  Same wt_wow_point.
__global__ __launch_bounds__(256) void wt_batch_wow_map_kernel(float *c, const float *noise, float *gamma, int64_t f4, const double *ptab, int soft)
{
    const int f = blockIdx.y;
    const double tau = ptab[2 * f];
    const float tauf = (float)tau, factor = (float)ptab[2 * f + 1];
    float4 *cf = reinterpret_cast<float4 *>(c) + (int64_t)f * f4;
    const float4 *nf4 = reinterpret_cast<const float4 *>(noise) + (int64_t)f * f4;
    float4 *gf = gamma ? reinterpret_cast<float4 *>(gamma) + (int64_t)f * f4 : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = cf[i];
        const float4 nz = nf4[i];
        float4 gm = make_float4(0, 0, 0, 0);
        if (gf) gm = gf[i];
        float in[4] = {v.x, v.y, v.z, v.w};
        const float nn[4] = {nz.x, nz.y, nz.z, nz.w};
        float gg[4] = {gm.x, gm.y, gm.z, gm.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) in[k] = wt_wow_point(in[k], 1.f, false, nn[k], tau, tauf, soft, factor, gg[k]);
        cf[i] = make_float4(in[0], in[1], in[2], in[3]);
        if (gf) gf[i] = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
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
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<float4 *>(d)[i] = make_float4(value, value, value, value);
}

// frame 0 of a plane -> frames 1 .. gridDim.y (a noise map shared by the frames of a chunk crosses PCIe once)
__global__ __launch_bounds__(256) void wt_batch_replicate_kernel(float *d, int64_t f4)
{
    const float4 *src = reinterpret_cast<const float4 *>(d);
    float4 *dst = reinterpret_cast<float4 *>(d) + (int64_t)(blockIdx.y + 1) * f4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f4; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// wt_filter2d_kernel (wt_kernels_apps.h) for the frames of a batch: grid z = the frame, each its own image (the
// border rules act at the frame's borders).  Staging, tile geometry and the chain of fmaf per output are
// wt_rl_point.h's; !SKEW is the per-image tap loop (one LDS read per FMA), the one wt_batch_filter2d launches; SKEW
// walks every staged row once for the four output rows of a thread (wt_f2d_taps_skewed: one LDS read per four FMAs,
// measured slower) - identical bits either way.
template <bool WRAP, bool SKEW>
__global__ __launch_bounds__(256) void wt_batch_filter2d_kernel(const float *in, float *out, Geo g, int64_t fstride, const float *__restrict__ psf,
                                                                int kh, int kw, int ay, int ax)
{
    extern __shared__ float tile[];
    in += (int64_t)blockIdx.z * fstride;
    out += (int64_t)blockIdx.z * fstride;
    const int tw = WT_F2D_TW + kw - 1, th = WT_F2D_TH + kh - 1;
    const int x0 = blockIdx.x * WT_F2D_TW, ly0 = blockIdx.y * WT_F2D_TH;
    wt_f2d_stage<WRAP>(tile, in, g, x0, ly0, tw, th, ay, ax);
    __syncthreads();
    const int x = x0 + threadIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (SKEW) wt_f2d_taps_skewed(tile, tw, psf, kh, kw, acc);
    else wt_f2d_taps(tile, tw, psf, kw, kh, kw, acc);
    if (x < g.W) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ly = ly0 + threadIdx.y * 4 + r;
            if (ly < g.H) out[(int64_t)ly * g.P + x] = acc[r];
        }
    }
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
static int bplane(wt_batch *b, int id, float **out)
{
    float **slot = nullptr;
    if (id >= 0 && id <= b->max_level) slot = &b->coef[id];
    else if (id == WT_PLANE_INPUT) slot = &b->input;
    else if (id == WT_PLANE_OUT) slot = &b->out;
    else if (id == WT_PLANE_SCRATCH(0)) slot = &b->scr[0];
    else if (id == WT_PLANE_SCRATCH(1)) slot = &b->scr[1];
    else if (id == WT_PLANE_SCRATCH(3)) slot = &b->spare;
    else if (id == WT_PLANE_SCRATCH(4)) slot = &b->gamma;
    else if (id == WT_PLANE_SCRATCH(5)) slot = &b->noise;
    else if (id <= WT_PLANE_SCRATCH(6) && id >= WT_PLANE_SCRATCH(10)) slot = &b->rl[WT_PLANE_SCRATCH(6) - id];
    else if (id <= WT_PLANE_SCRATCH(16) && id > WT_PLANE_SCRATCH(16) - (int)b->mrs.size()) slot = &b->mrs[WT_PLANE_SCRATCH(16) - id];
    if (!slot)
        WT_FAIL("wt_batch: plane %d is not a plane of a batch (0..%d, input, out, scratch 0/1/3/4/5, 6..10, 16..%d)", id, b->max_level,
                15 + (int)b->mrs.size());
    if (!*slot) WT_HIP(hipMalloc((void **)slot, (size_t)b->n * (size_t)b->fstride * sizeof(float)));
    *out = *slot;
    return 0;
}

static int check_frames(const wt_batch *b, int nf, const char *who)
{
    if (!b) WT_FAIL("%s: null batch", who);
    if (nf < 1 || nf > b->n) WT_FAIL("%s: %d active frames (batch of %d)", who, nf, b->n);
    return 0;
}

// the fused schedule of `level` scales, or an error: the passes with a sum run fused kernels only; `single`: a
// single-scale pass without a fused kernel runs the batched MODE_DECOMP stencil (as wt_decompose_pass on a plan)
static int batch_schedule(wt_batch *b, int level, int32_t *tr, int *np, const char *who, bool single = false)
{
    if (level < 1 || level > b->max_level) WT_FAIL("%s: level %d outside [1, %d]", who, level, b->max_level);
    WT_TRY(wt_schedule(b->geo.family, level, 1, tr, 32, np));
    for (int i = 0; i < *np; ++i)
        if (!wt_fused_has_pass(tr[3 * i], tr[3 * i + 1], b->geo.family) && !(single && tr[3 * i + 1] == 1))
            WT_FAIL("%s: %d scales have no all-fused schedule (wt_plan_fused_ok): not a batch case", who, level);
    return 0;
}

// the frames of a batched stencil launch on the batch's stream
static StencilCtx batch_stencil_ctx(const wt_batch *b)
{
    return StencilCtx{b->ctx, b->ctx->stream, b->geo.g, b->geo.family};
}

// one single-scale pass of the transform on the batched MODE_DECOMP stencil (decompose_pass_impl's per-scale branch)
static int batch_stencil_pass(wt_batch *b, int nf, int cur, int nxt, int s0)
{
    if (s0 < 0 || s0 > 24 || s0 > b->max_level) WT_FAIL("wt_batch_decompose: scale %d outside the batch (max_level %d)", s0, b->max_level);
    if (cur == nxt || cur == s0 || nxt == s0) WT_FAIL("wt_batch_decompose: input/output planes alias the detail plane of the pass");
    float *in = nullptr, *oc = nullptr, *ow = nullptr;
    WT_TRY(bplane(b, cur, &in));
    WT_TRY(bplane(b, nxt, &oc));
    WT_TRY(bplane(b, s0, &ow));
    ChainArgs a{};
    a.in = in; a.out_c = oc; a.out_w = ow; a.aux = nullptr;
    a.f1 = 1.f; a.f2 = 1.f; a.take_sqrt = 0;
    WtFrames fr;
    fr.n = nf;
    fr.fstride = b->fstride;
    return wt32_stencil_batch_launch(batch_stencil_ctx(b), MODE_DECOMP, a, s0, "wt_chain_batch_kernel<decomp>", fr);
}

// per-frame parameter pairs (pairs[2 * f], pairs[2 * f + 1]) -> a device table slot, stream-ordered (*dev)
static int batch_table(wt_batch *b, int nf, const double *pairs, const double **dev)
{
    wt_ctx *c = b->ctx;
    if (!b->d_ptab) {
        WT_HIP(hipMalloc((void **)&b->d_ptab, (size_t)wt_batch::kTabSlots * b->n * 2 * sizeof(double)));
        WT_HIP(hipHostMalloc((void **)&b->h_ptab, (size_t)wt_batch::kTabSlots * b->n * 2 * sizeof(double), 0));
    }
    const int slot = b->ptab_next;
    b->ptab_next = (slot + 1) % wt_batch::kTabSlots;
    if (b->ptab_ev[slot]) WT_HIP(hipEventSynchronize(b->ptab_ev[slot]));    // (the copy of kTabSlots calls ago)
    else WT_HIP(hipEventCreateWithFlags(&b->ptab_ev[slot], hipEventDisableTiming));
    double *h = b->h_ptab + (size_t)slot * b->n * 2, *d = b->d_ptab + (size_t)slot * b->n * 2;
    memcpy(h, pairs, (size_t)nf * 2 * sizeof(double));
    WT_HIP(hipMemcpyAsync(d, h, (size_t)nf * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    WT_HIP(hipEventRecord(b->ptab_ev[slot], c->stream));
    *dev = d;
    return 0;
}

// x blocks per frame of the batched pointwise kernels (grid y = the frame): about flat_grid's 2048 in all
static unsigned batch_flat_blocks(const wt_batch *b, int nf)
{
    const int64_t f4 = b->fstride / 4;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((f4 + 255) / 256, (2048 + nf - 1) / nf));
}

static int batch_pass(wt_batch *b, int nf, int cur, int nxt, int s0, int ns, int acc, int sum_plane, bool first)
{
    if (ns < 1 || ns > WT_FUSED_MAX_SCALES || s0 < 0 || s0 + ns - 1 > b->max_level)
        WT_FAIL("wt_batch_decompose_pass: scales [%d,%d) outside the batch (max_level %d)", s0, s0 + ns, b->max_level);
    if (cur == nxt || (cur >= s0 && cur < s0 + ns) || (nxt >= s0 && nxt < s0 + ns))
        WT_FAIL("wt_batch_decompose_pass: input/output planes alias the detail planes of the pass");
    if (!wt_fused_has_pass(s0, ns, b->geo.family)) WT_FAIL("wt_batch_decompose_pass: no fused kernel for first scale %d x %d scales", s0, ns);
    if (acc && first != (s0 == 0))
        WT_FAIL("wt_batch_decompose_pass_sum: first must be set for the pass that starts at scale 0 and only for it (got first=%d, s0=%d)", (int)first, s0);
    float *in = nullptr, *oc = nullptr, *ps = nullptr;
    WT_TRY(bplane(b, cur, &in));
    WT_TRY(bplane(b, nxt, &oc));
    float *ow[WT_FUSED_MAX_SCALES] = {nullptr};
    for (int k = 0; k < ns; ++k) WT_TRY(bplane(b, s0 + k, &ow[k]));
    if (acc) {
        if (sum_plane == cur || sum_plane == nxt || (sum_plane >= s0 && sum_plane < s0 + ns))
            WT_FAIL("wt_batch_decompose_pass_sum: the sum plane aliases a plane of the pass");
        WT_TRY(bplane(b, sum_plane, &ps));
    }
    FusedRows rows;
    rows.frames = nf;
    rows.fstride = b->fstride;
    return wt_fused_launch(&b->geo, in, oc, ow, s0, ns, acc, first ? nullptr : ps, ps, rows);
}

static int batch_schedule_run(wt_batch *b, int nf, int src, int level, bool with_sum, int dst, const char *who)
{
    if (src >= 0 && src <= level) WT_FAIL("%s: src plane %d is one of the output planes", who, src);
    if (src == WT_PLANE_SCRATCH(0) || src == WT_PLANE_SCRATCH(1)) WT_FAIL("%s: scratch planes 0/1 are used internally", who);
    if (with_sum && ((dst >= 0 && dst <= level) || dst == src || dst == WT_PLANE_SCRATCH(0) || dst == WT_PLANE_SCRATCH(1)))
        WT_FAIL("%s: dst plane %d is an input / output / internal plane of the transform", who, dst);
    int32_t tr[3 * 32];
    int np = 0;
    WT_TRY(batch_schedule(b, level, tr, &np, who, !with_sum));
    int cur = src;
    for (int i = 0; i < np; ++i) {
        const int s0 = tr[3 * i], ns = tr[3 * i + 1];
        const bool last = s0 + ns == level;
        const int nxt = last ? level : WT_PLANE_SCRATCH(i & 1);
        if (!with_sum && ns == 1 && !wt_fused_has_pass(s0, 1, b->geo.family)) WT_TRY(batch_stencil_pass(b, nf, cur, nxt, s0));
        else WT_TRY(batch_pass(b, nf, cur, nxt, s0, ns, with_sum ? (last ? 2 : 1) : 0, dst, i == 0));
        cur = nxt;
    }
    return 0;
}

extern "C" int wt_batch_create(wt_ctx *ctx, int n, int H, int W, int family, int max_level, wt_batch **out)
{
    WtGuard guard_(ctx);
    if (!ctx || !out) WT_FAIL("wt_batch_create: null pointer");
    *out = nullptr;
    if (n < 1 || n > 65535) WT_FAIL("wt_batch_create: %d frames (1..65535 per batch)", n);
    if (H < 1 || W < 1) WT_FAIL("wt_batch_create: frame %d x %d", H, W);
    if (family != WT_B3SPLINE && family != WT_TRIANGLE) WT_FAIL("wt_batch_create: family %d (built-in families only)", family);
    if (max_level < 0 || max_level > 30) WT_FAIL("wt_batch_create: max_level %d", max_level);
    wt_batch *b = new wt_batch;
    b->ctx = ctx;
    b->n = n;
    b->max_level = max_level;
    b->geo.ctx = ctx;
    b->geo.family = family;
    b->geo.max_level = max_level;
    b->geo.g = Geo{W, (W + 3) / 4 * 4, H, 0, H, 0, 0};
    b->fstride = (int64_t)H * b->geo.g.P;
    b->coef.assign(max_level + 1, nullptr);
    b->mrs.assign(std::min(max_level, WT_NUM_SCRATCH - 16), nullptr);
    if (!wt_fused_supported(&b->geo)) {
        delete b;
        WT_FAIL("wt_batch_create: rows of %d pixels are too wide for the fused passes", W);
    }
    auto fail = [&](hipError_t e) -> int {
        (void)hipFree(b->d_hist);
        (void)hipFree(b->d_sel);
        (void)hipFree(b->d_tau);
        (void)hipHostFree(b->h_sel);
        (void)hipHostFree(b->h_tau);
        delete b;
        wt_set_error("wt_batch_create: HIP error %d (%s)", (int)e, hipGetErrorString(e));
        return 2;
    };
    hipError_t e = hipMalloc((void **)&b->d_hist, (size_t)n * 2 * WT_HIST_BINS * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_sel, (size_t)n * 2 * sizeof(WtBatchSel));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_tau, (size_t)n * 2 * WT_MAX_SUM_PLANES * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_sel, (size_t)n * 2 * sizeof(WtBatchSel), 0);
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_tau, (size_t)n * 2 * WT_MAX_SUM_PLANES * sizeof(double), 0);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_hist, 0, (size_t)n * 2 * WT_HIST_BINS * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) return fail(e);
    *out = b;
    return 0;
}

extern "C" int wt_batch_destroy(wt_batch *b)
{
    if (!b) return 0;
    WtGuard guard_(b->ctx);
    (void)hipStreamSynchronize(b->ctx->stream);
    int bad = 0;
    auto f = [&](void *q) { if (q && hipFree(q) != hipSuccess) bad = 1; };
    for (float *q : b->coef) f(q);
    f(b->input);
    f(b->out);
    f(b->scr[0]);
    f(b->scr[1]);
    f(b->d_hist);
    f(b->d_sel);
    f(b->d_tau);
    f(b->spare);
    f(b->gamma);
    f(b->noise);
    for (float *q : b->rl) f(q);
    for (float *q : b->mrs) f(q);
    f(b->d_psf[0]);
    f(b->d_psf[1]);
    for (void *q : b->fft_allocs) f(q);
    f(b->d_ptab);
    f(b->d_red);
    if (b->h_sel && hipHostFree(b->h_sel) != hipSuccess) bad = 1;
    if (b->h_tau && hipHostFree(b->h_tau) != hipSuccess) bad = 1;
    if (b->h_ptab && hipHostFree(b->h_ptab) != hipSuccess) bad = 1;
    if (b->h_red && hipHostFree(b->h_red) != hipSuccess) bad = 1;
    for (hipEvent_t e : b->ptab_ev)
        if (e && hipEventDestroy(e) != hipSuccess) bad = 1;
    delete b;
    if (bad) WT_FAIL("wt_batch_destroy: a device buffer could not be released");
    return 0;
}

extern "C" int wt_batch_info(wt_batch *b, int64_t *info)
{
    if (!b || !info) WT_FAIL("wt_batch_info: null pointer");
    const Geo &g = b->geo.g;
    const int64_t v[7] = {b->n, g.H, g.W, g.P, b->fstride, b->max_level, b->geo.family};
    memcpy(info, v, sizeof v);
    return 0;
}

extern "C" int wt_batch_plane_ptr(wt_batch *b, int plane, void **ptr, int64_t *frame_stride)
{
    if (!b || !ptr || !frame_stride) WT_FAIL("wt_batch_plane_ptr: null pointer");
    WtGuard guard_(b->ctx);
    float *q = nullptr;
    WT_TRY(bplane(b, plane, &q));
    *ptr = q;
    *frame_stride = b->fstride;
    return 0;
}

// frames [f0, f0 + nf) of a plane <-> host frames `hstride` floats apart (rows of W floats back to back within a frame)
static int batch_copy(wt_batch *b, int plane, int f0, int nf, float *host, int64_t hstride, bool up, const char *who)
{
    if (!b || !host) WT_FAIL("%s: null pointer", who);
    if (f0 < 0 || nf < 1 || f0 + nf > b->n) WT_FAIL("%s: frames [%d, %d) outside the batch of %d", who, f0, f0 + nf, b->n);
    const Geo &g = b->geo.g;
    const int64_t fpx = (int64_t)g.H * g.W;
    if (hstride == 0) hstride = fpx;
    if (hstride < fpx) WT_FAIL("%s: host frame stride %lld below the %lld pixels of a frame", who, (long long)hstride, (long long)fpx);
    WtGuard guard_(b->ctx);
    WT_TRY(wt_side_join(b->ctx));
    float *q = nullptr;
    WT_TRY(bplane(b, plane, &q));
    float *dev = q + (int64_t)f0 * b->fstride;
    const size_t span = ((size_t)(nf - 1) * (size_t)hstride + (size_t)fpx) * 4;
    const bool pinned = try_pin(host, span);     // (no-op for page-locked blocks: _lib.host_empty)
    hipError_t e = hipSuccess;
    // contiguous frames are one tall image of nf * H rows; else one 2-D copy per frame
    const int pieces = hstride == fpx ? 1 : nf;
    const size_t rows = (size_t)g.H * (size_t)(hstride == fpx ? nf : 1);
    for (int i = 0; i < pieces && e == hipSuccess; ++i) {
        float *d = dev + (int64_t)i * b->fstride, *h = host + (int64_t)i * hstride;
        e = up ? hipMemcpy2DAsync(d, (size_t)g.P * 4, h, (size_t)g.W * 4, (size_t)g.W * 4, rows, hipMemcpyHostToDevice, b->ctx->stream)
               : hipMemcpy2DAsync(h, (size_t)g.W * 4, d, (size_t)g.P * 4, (size_t)g.W * 4, rows, hipMemcpyDeviceToHost, b->ctx->stream);
    }
    hipError_t e2 = hipStreamSynchronize(b->ctx->stream);
    if (e == hipSuccess) e = e2;
    if (pinned) (void)hipHostUnregister(host);
    WT_HIP(e);
    return 0;
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
    WT_TRY(check_frames(b, nf, "wt_batch_decompose"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose: a batch runs the fused passes (flags bit0)");
    if (level == 0) {
        float *s = nullptr, *d = nullptr;
        if (src == 0) WT_FAIL("wt_batch_decompose: src plane 0 is the output plane");
        WT_TRY(bplane(b, src, &s));
        WT_TRY(bplane(b, 0, &d));
        WT_HIP(hipMemcpyAsync(d, s, (size_t)nf * (size_t)b->fstride * 4, hipMemcpyDeviceToDevice, b->ctx->stream));
        return 0;
    }
    return batch_schedule_run(b, nf, src, level, false, WT_PLANE_NONE, "wt_batch_decompose");
}

// wt_decompose_bilateral (wt_transform.hip, watroo/wavelets.py:433-442) for the active frames: scale s reads `cur`,
// writes c_{s+1} to a scratch plane (the two ping-pong; plane `level` on the last scale) and w_s to plane s, the
// variance formed in the march with f1 = sigma_b[s]^2, f2 = s + 1 under bilateral_scaling.  One launch per scale for
// all frames (wt_bilateral32_batch.hip); no two-kernel form, no side-stream overlap.
extern "C" int wt_batch_decompose_bilateral(wt_batch *b, int nf, int src, int level, const double *sigma_b, int bilateral_scaling, int flags)
{
    (void)flags;
    WT_TRY(check_frames(b, nf, "wt_batch_decompose_bilateral"));
    WtGuard guard_(b->ctx);
    if (!sigma_b) WT_FAIL("wt_batch_decompose_bilateral: null pointer");
    if (level < 0 || level > b->max_level) WT_FAIL("wt_batch_decompose_bilateral: level %d exceeds the batch's max_level %d", level, b->max_level);
    if (src >= 0 && src <= level) WT_FAIL("wt_batch_decompose_bilateral: src plane %d is one of the output planes", src);
    if (src == WT_PLANE_SCRATCH(0) || src == WT_PLANE_SCRATCH(1)) WT_FAIL("wt_batch_decompose_bilateral: scratch planes 0/1 are used internally");
    if (level > 25) WT_FAIL("wt_batch_decompose_bilateral: scale %d out of range", level - 1);
    float *in = nullptr;
    WT_TRY(bplane(b, src, &in));
    if (level == 0) {
        float *d = nullptr;
        WT_TRY(bplane(b, 0, &d));
        WT_HIP(hipMemcpyAsync(d, in, (size_t)nf * (size_t)b->fstride * 4, hipMemcpyDeviceToDevice, b->ctx->stream));
        return 0;
    }
    WtFrames fr;
    fr.n = nf;
    fr.fstride = b->fstride;
    for (int s = 0; s < level; ++s) {
        const int nxt = (s == level - 1) ? level : WT_PLANE_SCRATCH(s & 1);
        float *oc = nullptr, *ow = nullptr;
        WT_TRY(bplane(b, nxt, &oc));
        WT_TRY(bplane(b, s, &ow));
        ChainArgs a{};
        a.in = in; a.out_c = oc; a.out_w = ow;
        // variance = sdev_loc(c_s)^2-form * sigma_b[s]**2 (* (s+1))   watroo/wavelets.py:434-436
        a.f1 = (float)(sigma_b[s] * sigma_b[s]);
        a.f2 = bilateral_scaling ? (float)(s + 1) : 1.f;
        WT_TRY(wt32_bilateral_batch_launch(batch_stencil_ctx(b), a, s, g_opt_bilateral_paired != 0, fr));
        in = oc;
    }
    return 0;
}

extern "C" int wt_batch_decompose_sum(wt_batch *b, int nf, int src, int level, int dst, int flags)
{
    WT_TRY(check_frames(b, nf, "wt_batch_decompose_sum"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose_sum: a batch runs the fused passes (flags bit0)");
    return batch_schedule_run(b, nf, src, level, true, dst, "wt_batch_decompose_sum");
}

extern "C" int wt_batch_decompose_pass(wt_batch *b, int nf, int cur, int nxt, int s0, int ns, int flags)
{
    WT_TRY(check_frames(b, nf, "wt_batch_decompose_pass"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose_pass: a batch runs the fused passes (flags bit0)");
    return batch_pass(b, nf, cur, nxt, s0, ns, 0, WT_PLANE_NONE, false);
}

extern "C" int wt_batch_decompose_pass_sum(wt_batch *b, int nf, int cur, int nxt, int s0, int ns, int flags, int sum_plane, int first,
                                           int last)
{
    WT_TRY(check_frames(b, nf, "wt_batch_decompose_pass_sum"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch_decompose_pass_sum: a batch runs the fused passes (flags bit0)");
    return batch_pass(b, nf, cur, nxt, s0, ns, last ? 2 : 1, sum_plane, first != 0);
}

extern "C" int wt_batch_abs_median(wt_batch *b, int nf, int plane, float *medians)
{
    WT_TRY(check_frames(b, nf, "wt_batch_abs_median"));
    if (!medians) WT_FAIL("wt_batch_abs_median: null pointer");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    float *q = nullptr;
    WT_TRY(bplane(b, plane, &q));
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
    WT_TRY(check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    if (count < 1 || count > WT_MAX_SUM_PLANES || count - 1 > b->max_level)
        WT_FAIL("%s: count %d out of range [1,%d]", who, count, std::min(WT_MAX_SUM_PLANES, b->max_level + 1));
    if (n_den < 0 || n_den > count) WT_FAIL("%s: n_den %d outside [0,%d]", who, n_den, count);
    if (n_den > 0 && (!tau || !wgt)) WT_FAIL("%s: null tau/wgt", who);
    if (dst >= 0 && dst < count) WT_FAIL("%s: dst plane %d is one of the summed planes", who, dst);
    if (noise_plane != WT_PLANE_NONE && (noise_plane == dst || (noise_plane >= 0 && noise_plane < count)))
        WT_FAIL("%s: the noise plane %d is a plane of the sum", who, noise_plane);
    BatchDenoiseArgs a{};
    a.n = count; a.n_den = n_den; a.soft = soft; a.write_back = write_back;
    for (int i = 0; i < count; ++i) {
        WT_TRY(bplane(b, i, &a.p[i]));
        a.wgt[i] = i < n_den ? (float)wgt[i] : 1.f;
    }
    float *o = nullptr, *nz = nullptr;
    WT_TRY(bplane(b, dst, &o));
    if (noise_plane != WT_PLANE_NONE) WT_TRY(bplane(b, noise_plane, &nz));
    const int nt = std::max(n_den, 1);
    // (the table goes up stream-ordered from pinned staging: the previous call's kernel may still read d_tau)
    WT_HIP(hipStreamSynchronize(b->ctx->stream));
    for (int i = 0; i < nf * nt; ++i) b->h_tau[i] = n_den ? tau[i] : 0.0;
    WT_HIP(hipMemcpyAsync(b->d_tau, b->h_tau, (size_t)nf * nt * sizeof(double), hipMemcpyHostToDevice, b->ctx->stream));
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
    WT_TRY(check_frames(b, nf, "wt_batch_enhance_sum"));
    WtGuard guard_(b->ctx);
    if (count < 1 || count > WT_MAX_SUM_PLANES || count - 1 > b->max_level)
        WT_FAIL("wt_batch_enhance_sum: count %d out of range [1,%d]", count, std::min(WT_MAX_SUM_PLANES, b->max_level + 1));
    if (n_den < 1 || n_den > count) WT_FAIL("wt_batch_enhance_sum: n_den %d outside [1,%d]", n_den, count);
    if (!tau || !wgt) WT_FAIL("wt_batch_enhance_sum: null tau/wgt");
    if (dst >= 0 && dst < count) WT_FAIL("wt_batch_enhance_sum: dst plane %d is one of the summed planes", dst);
    BatchEnhanceArgs a{};
    a.n = count; a.n_den = n_den; a.soft = soft; a.write_back = write_back;
    for (int i = 0; i < count; ++i) WT_TRY(bplane(b, i, &a.p[i]));
    float *o = nullptr;
    WT_TRY(bplane(b, dst, &o));
    // (the table goes up stream-ordered from pinned staging: the previous call's kernel may still read d_tau)
    WT_HIP(hipStreamSynchronize(b->ctx->stream));
    const int row = 2 * n_den;                              // nf <= n, n_den <= WT_MAX_SUM_PLANES: within the tables
    for (int f = 0; f < nf; ++f)
        for (int k = 0; k < n_den; ++k) {
            b->h_tau[f * row + k] = tau[f * n_den + k];
            b->h_tau[f * row + n_den + k] = wgt[f * n_den + k];
        }
    WT_HIP(hipMemcpyAsync(b->d_tau, b->h_tau, (size_t)nf * row * sizeof(double), hipMemcpyHostToDevice, b->ctx->stream));
    const int64_t n4 = (int64_t)nf * b->fstride / 4;
    ProfScope ps(b->ctx, "wt_batch_enhance_sum_kernel");
    hipLaunchKernelGGL(wt_batch_enhance_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, b->ctx->stream, a, (const double *)b->d_tau,
                       o, n4, b->fstride / 4);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch_anscombe(wt_batch *b, int nf, int src, int dst, float alpha, float g, float sigma, int inverse)
{
    WT_TRY(check_frames(b, nf, "wt_batch_anscombe"));
    WtGuard guard_(b->ctx);
    if (alpha == 0.f) WT_FAIL("wt_batch_anscombe: alpha must be non-zero");
    float *s = nullptr, *d = nullptr;
    WT_TRY(bplane(b, src, &s));
    WT_TRY(bplane(b, dst, &d));
    return launch_anscombe(b->ctx, s, d, (int64_t)nf * b->fstride / 4, alpha, g, sigma, inverse);
}

// ------------------------------------------------------------------------------------------------ wow
extern "C" int wt_batch_fill(wt_batch *b, int nf, int plane, float value)
{
    WT_TRY(check_frames(b, nf, "wt_batch_fill"));
    WtGuard guard_(b->ctx);
    float *d = nullptr;
    WT_TRY(bplane(b, plane, &d));
    const int64_t n4 = (int64_t)nf * b->fstride / 4;
    ProfScope ps(b->ctx, "wt_batch_fill_kernel");
    hipLaunchKernelGGL(wt_batch_fill_kernel, dim3(flat_grid(n4)), dim3(256), 0, b->ctx->stream, d, n4, value);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch_replicate(wt_batch *b, int nf, int plane)
{
    WT_TRY(check_frames(b, nf, "wt_batch_replicate"));
    WtGuard guard_(b->ctx);
    float *d = nullptr;
    WT_TRY(bplane(b, plane, &d));
    if (nf == 1) return 0;
    const int64_t f4 = b->fstride / 4;
    ProfScope ps(b->ctx, "wt_batch_replicate_kernel");
    hipLaunchKernelGGL(wt_batch_replicate_kernel, dim3(batch_flat_blocks(b, nf), nf - 1), dim3(256), 0, b->ctx->stream, d, f4);
    WT_HIP(hipGetLastError());
    return 0;
}

// frame f of the plane <- the field wt_fill_normal(seed, first_trial + f) gives a wt_plan of the frame's shape
extern "C" int wt_batch_fill_normal(wt_batch *b, int nf, int plane, uint64_t seed, uint32_t first_trial)
{
    WT_TRY(check_frames(b, nf, "wt_batch_fill_normal"));
    WtGuard guard_(b->ctx);
    float *d = nullptr;
    WT_TRY(bplane(b, plane, &d));
    return wt_launch_fill_normal(b->ctx, d, b->geo.g, b->geo.g.H, nf, b->fstride, seed, first_trial);
}

static int wow_pairs(wt_batch *b, int nf, const double *tau, const float *factor, const double **dev, const char *who)
{
    if (!tau || !factor) WT_FAIL("%s: null tau / factor", who);
    std::vector<double> pairs((size_t)nf * 2);
    for (int f = 0; f < nf; ++f) {
        pairs[2 * f] = tau[f];
        pairs[2 * f + 1] = (double)factor[f];
    }
    return batch_table(b, nf, pairs.data(), dev);
}

// wt_batch_wow_update / wt_batch_wow_update_map: noise_plane == WT_PLANE_NONE runs the kernel without a map
static int batch_wow_update(wt_batch *b, int nf, int plane, const double *tau, int soft, const float *factor, int gamma_plane, int noise_plane,
                            const char *who)
{
    WT_TRY(check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    if (gamma_plane == plane) WT_FAIL("%s: the gamma plane is the updated plane", who);
    if (noise_plane != WT_PLANE_NONE && (noise_plane == plane || noise_plane == gamma_plane)) WT_FAIL("%s: the noise plane aliases a plane of the update", who);
    float *c = nullptr, *gm = nullptr, *nz = nullptr;
    WT_TRY(bplane(b, plane, &c));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(bplane(b, gamma_plane, &gm));
    if (noise_plane != WT_PLANE_NONE) WT_TRY(bplane(b, noise_plane, &nz));
    const double *dt = nullptr;
    WT_TRY(wow_pairs(b, nf, tau, factor, &dt, who));
    if (nz) {
        ProfScope ps(b->ctx, "wt_batch_wow_map_kernel");
        hipLaunchKernelGGL(wt_batch_wow_map_kernel, dim3(batch_flat_blocks(b, nf), nf), dim3(256), 0, b->ctx->stream, c, (const float *)nz, gm,
                           b->fstride / 4, dt, soft);
    } else {
        ProfScope ps(b->ctx, "wt_batch_wow_kernel");
        hipLaunchKernelGGL(wt_batch_wow_kernel, dim3(batch_flat_blocks(b, nf), nf), dim3(256), 0, b->ctx->stream, c, gm, b->fstride / 4, dt, soft);
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
    WT_TRY(check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    if (plane < 0 || plane > b->max_level) WT_FAIL("%s: plane %d is not a coefficient plane", who, plane);
    if (s < 0 || s > 24) WT_FAIL("%s: scale %d out of range", who, s);
    if (gamma_plane == plane || gamma_plane == WT_PLANE_SCRATCH(3)) WT_FAIL("%s: the gamma plane aliases a plane of the update", who);
    if (noise_plane != WT_PLANE_NONE && (noise_plane == plane || noise_plane == WT_PLANE_SCRATCH(3) || noise_plane == gamma_plane))
        WT_FAIL("%s: the noise plane aliases a plane of the update", who);
    float *c = nullptr, *t = nullptr, *gm = nullptr, *nz = nullptr;
    WT_TRY(bplane(b, plane, &c));
    WT_TRY(bplane(b, WT_PLANE_SCRATCH(3), &t));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(bplane(b, gamma_plane, &gm));
    if (noise_plane != WT_PLANE_NONE) WT_TRY(bplane(b, noise_plane, &nz));
    const double *dt = nullptr;
    WT_TRY(wow_pairs(b, nf, tau, factor, &dt, who));
    // (wt_wow_scale's arguments and its choice of instantiation; tau and factor come from the frame's row of the table)
    ChainArgs a{};
    a.in = c; a.out_c = t; a.out_w = nullptr; a.aux = nullptr;
    a.noise = nz; a.gamma = gm; a.soft = soft; a.whiten = 1;
    WtFrames fr;
    fr.n = nf;
    fr.fstride = b->fstride;
    fr.ftab = dt;
    WT_TRY(wt32_stencil_batch_launch(batch_stencil_ctx(b), nz ? MODE_WOW : (gm ? MODE_WOW_GAMMA : MODE_WOW_PLAIN), a, s, "wt_chain_batch_kernel<wow>", fr));
    std::swap(b->coef[plane], b->spare);          // (wt_wow_scale: "in place" at pointer level)
    return 0;
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
    WT_TRY(check_frames(b, nf, "wt_batch_reduce"));
    if (!out) WT_FAIL("wt_batch_reduce: null pointer");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    float *q = nullptr;
    WT_TRY(bplane(b, plane, &q));
    const Geo &g = b->geo.g;
    // (wt_reduce's work items: (row, chunk of 4096 pixels) pairs over at most partial_blocks blocks, per frame)
    const int blocks = (int)std::min<int64_t>((int64_t)g.H * ((g.W + 4095) / 4096), c->partial_blocks);
    if (!b->d_red || b->red_blocks != blocks) {
        (void)hipFree(b->d_red);
        (void)hipHostFree(b->h_red);
        b->d_red = nullptr;
        b->h_red = nullptr;
        WT_HIP(hipMalloc((void **)&b->d_red, (size_t)b->n * ((size_t)blocks + 1) * 4 * sizeof(double)));
        WT_HIP(hipHostMalloc((void **)&b->h_red, (size_t)b->n * 4 * sizeof(double), 0));
        b->red_blocks = blocks;
    }
    double *dout = b->d_red + (size_t)b->n * blocks * 4;
    {
        ProfScope ps(c, "wt_batch_reduce_kernel");
        hipLaunchKernelGGL(wt_batch_reduce_kernel, dim3(blocks, nf), dim3(256), 0, c->stream, (const float *)q, g.H, g.P / 4, g.W, b->fstride, b->d_red);
        hipLaunchKernelGGL(wt_batch_reduce_final_kernel, dim3(nf), dim3(256), 0, c->stream, (const double *)b->d_red, blocks, dout);
    }
    WT_HIP(hipGetLastError());
    WT_HIP(hipMemcpyAsync(b->h_red, dout, (size_t)nf * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));               // the one host round trip for all nf frames
    memcpy(out, b->h_red, (size_t)nf * 4 * sizeof(double));
    return 0;
}

extern "C" int wt_batch_gamma_blend(wt_batch *b, int nf, int recon, int gamma_plane, const float *gmin, const float *gmax, float inv_gamma,
                                    float h)
{
    WT_TRY(check_frames(b, nf, "wt_batch_gamma_blend"));
    if (!gmin || !gmax) WT_FAIL("wt_batch_gamma_blend: null gmin / gmax");
    WtGuard guard_(b->ctx);
    if (recon == gamma_plane) WT_FAIL("wt_batch_gamma_blend: recon and gamma planes must differ");
    float *r = nullptr, *g = nullptr;
    WT_TRY(bplane(b, recon, &r));
    WT_TRY(bplane(b, gamma_plane, &g));
    std::vector<double> pairs((size_t)nf * 2);
    for (int f = 0; f < nf; ++f) {
        pairs[2 * f] = gmin[f];
        pairs[2 * f + 1] = gmax[f];
    }
    const double *dt = nullptr;
    WT_TRY(batch_table(b, nf, pairs.data(), &dt));
    ProfScope ps(b->ctx, "wt_batch_gamma_kernel");
    hipLaunchKernelGGL(wt_batch_gamma_kernel, dim3(batch_flat_blocks(b, nf), nf), dim3(256), 0, b->ctx->stream, r, g, b->fstride / 4, dt, inv_gamma, h);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch_plane_sum(wt_batch *b, int nf, int first, int count, int dst)
{
    WT_TRY(check_frames(b, nf, "wt_batch_plane_sum"));
    WtGuard guard_(b->ctx);
    if (count < 1 || count > WT_MAX_SUM_PLANES) WT_FAIL("wt_batch_plane_sum: count %d out of range [1,%d]", count, WT_MAX_SUM_PLANES);
    if (first < 0 || first + count - 1 > b->max_level) WT_FAIL("wt_batch_plane_sum: planes [%d,%d) outside [0,%d]", first, first + count, b->max_level);
    if (dst >= first && dst < first + count) WT_FAIL("wt_batch_plane_sum: dst plane %d is one of the summed planes", dst);
    const float *planes[WT_MAX_SUM_PLANES];
    for (int i = 0; i < count; ++i) {
        float *q = nullptr;
        WT_TRY(bplane(b, first + i, &q));
        planes[i] = q;
    }
    float *o = nullptr;
    WT_TRY(bplane(b, dst, &o));
    // the frames back to back are one flat range: wt_plane_sum_kernel over all of them
    return launch_plane_sum(b->ctx, planes, count, o, (int64_t)nf * b->fstride / 4);
}

// ------------------------------------------------------------------------------------------------ richardson_lucy
// host logic: *ok = 1 when wt_batch_set_psf takes a kh x kw PSF - one wt_filter2d_ex applies in ONE launch
extern "C" int wt_batch_psf_ok(int kh, int kw, int *ok)
{
    if (!ok) WT_FAIL("wt_batch_psf_ok: null pointer");
    *ok = wt_f2d_single_launch(kh, kw) ? 1 : 0;
    return 0;
}

// One of the two PSF operands of a richardson_lucy call (slot 0: forward, watroo/utils.py:257; slot 1: backward,
// utils.py:286) -> device memory of the batch, once per call: the iterations then correlate without a stream drain
// and without a PSF copy (wt_filter2d_ex does both on every call - its kernel comes from caller-owned memory).
extern "C" int wt_batch_set_psf(wt_batch *b, int slot, const float *kernel, int kh, int kw)
{
    if (!b || !kernel) WT_FAIL("wt_batch_set_psf: null pointer");
    WtGuard guard_(b->ctx);
    if (slot < 0 || slot > 1) WT_FAIL("wt_batch_set_psf: slot %d (0: forward, 1: backward)", slot);
    if (!wt_f2d_single_launch(kh, kw))
        WT_FAIL("wt_batch_set_psf: a %d x %d PSF is not applied in one launch (at most %d taps, rows of at most %d, an LDS tile of at most %d KB)",
                kh, kw, WT_F2D_MAX_TAPS, WT_F2D_MAX_KW, WT_F2D_MAX_LDS / 1024);
    const size_t ntaps = (size_t)kh * kw;
    // a launch on the stream may still read the slot, and `kernel` is the caller's: drain, then copy synchronously
    WT_HIP(hipStreamSynchronize(b->ctx->stream));
    if (ntaps > b->psf_cap[slot]) {
        (void)hipFree(b->d_psf[slot]);
        b->d_psf[slot] = nullptr;
        b->psf_cap[slot] = 0;
        b->psf_kh[slot] = b->psf_kw[slot] = 0;
        WT_HIP(hipMalloc((void **)&b->d_psf[slot], ntaps * sizeof(float)));
        b->psf_cap[slot] = ntaps;
    }
    WT_HIP(hipMemcpy(b->d_psf[slot], kernel, ntaps * sizeof(float), hipMemcpyHostToDevice));
    b->psf_kh[slot] = kh;
    b->psf_kw[slot] = kw;
    return 0;
}

// wt_filter2d_ex per frame (watroo/utils.py:257,286; periodic: the circular products of utils.py:245-254,284) with
// the PSF of `slot`: one launch for all active frames
// (measured, tools/bench_rl_stack.py: the per-image tap loop is about twice as fast as the row-skewed one at every
//  shape - 10 to 18 against 5 to 10 TFMA/s - so the skewed loop runs only on request, for that measurement)
static int g_batch_f2d_plain = getenv("WT_BATCH_F2D_SKEW") ? 0 : 1;
extern "C" int wt_batch_filter2d(wt_batch *b, int nf, int src, int dst, int slot, int ay, int ax, int border)
{
    WT_TRY(check_frames(b, nf, "wt_batch_filter2d"));
    WtGuard guard_(b->ctx);
    if (slot < 0 || slot > 1 || !b->d_psf[slot] || !b->psf_kh[slot]) WT_FAIL("wt_batch_filter2d: PSF slot %d is not set (wt_batch_set_psf)", slot);
    const int kh = b->psf_kh[slot], kw = b->psf_kw[slot];
    if (!wt_f2d_single_launch(kh, kw)) WT_FAIL("wt_batch_filter2d: a %d x %d PSF is not applied in one launch", kh, kw);
    if (ay < 0 || ay >= kh || ax < 0 || ax >= kw) WT_FAIL("wt_batch_filter2d: anchor (%d, %d) outside the %d x %d kernel", ay, ax, kh, kw);
    if (src == dst) WT_FAIL("wt_batch_filter2d: src and dst must differ");
    if (border != WT_BORDER_SYMMETRIC && border != WT_BORDER_PERIODIC) WT_FAIL("wt_batch_filter2d: border %d unsupported (symmetric or periodic)", border);
    const Geo &g = b->geo.g;
    dim3 grid((g.W + WT_F2D_TW - 1) / WT_F2D_TW, (g.H + WT_F2D_TH - 1) / WT_F2D_TH, nf), block(64, 4);
    if (grid.y > 65535u) WT_FAIL("wt_batch_filter2d: frames of %d rows are too tall (%u row tiles, at most 65535)", g.H, grid.y);
    if (grid.z > 65535u) WT_FAIL("wt_batch_filter2d: %d frames in one launch (at most 65535)", nf);
    float *in = nullptr, *o = nullptr;
    WT_TRY(bplane(b, src, &in));
    WT_TRY(bplane(b, dst, &o));
    const size_t lds = wt_f2d_lds_bytes(kh, kw);
    ProfScope ps(b->ctx, "wt_batch_filter2d_kernel");
    #define WT_BF2D_LAUNCH(WRAP, SKEW)                                                                                               \
        do {                                                                                                                         \
            if (lds > 64 * 1024)                                                                                                     \
                WT_HIP(hipFuncSetAttribute((const void *)wt_batch_filter2d_kernel<WRAP, SKEW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            hipLaunchKernelGGL((wt_batch_filter2d_kernel<WRAP, SKEW>), grid, block, lds, b->ctx->stream, (const float *)in, o, g, b->fstride, \
                               (const float *)b->d_psf[slot], kh, kw, ay, ax);                                                       \
        } while (0)
    if (border == WT_BORDER_PERIODIC) { if (g_batch_f2d_plain) WT_BF2D_LAUNCH(true, false); else WT_BF2D_LAUNCH(true, true); }
    else { if (g_batch_f2d_plain) WT_BF2D_LAUNCH(false, false); else WT_BF2D_LAUNCH(false, true); }
    #undef WT_BF2D_LAUNCH
    WT_HIP(hipGetLastError());
    return 0;
}

// wt_binary over the active frames (watroo/utils.py:259,280-281,288)
extern "C" int wt_batch_binary(wt_batch *b, int nf, int op, int a, int b2, int dst)
{
    WT_TRY(check_frames(b, nf, "wt_batch_binary"));
    WtGuard guard_(b->ctx);
    if (op < 0 || op > WT_OP_ADD_DIV) WT_FAIL("wt_batch_binary: unknown op %d", op);
    float *pa = nullptr, *pb = nullptr, *pd = nullptr;
    WT_TRY(bplane(b, a, &pa));
    WT_TRY(bplane(b, b2, &pb));
    WT_TRY(bplane(b, dst, &pd));
    const int64_t n4 = (int64_t)nf * b->fstride / 4;
    ProfScope ps(b->ctx, "wt_batch_binary_kernel");
    hipLaunchKernelGGL(wt_batch_binary_kernel, dim3(flat_grid(n4)), dim3(256), 0, b->ctx->stream, (const float *)pa, (const float *)pb, pd, n4, op);
    WT_HIP(hipGetLastError());
    return 0;
}

// wt_mrs_update per frame (watroo/utils.py:263-276) with the frame's tau[f]; scalar noise only
extern "C" int wt_batch_mrs_update(wt_batch *b, int nf, int plane, int mrs_plane, const double *tau, int soft, int persistent, float inv_pow)
{
    WT_TRY(check_frames(b, nf, "wt_batch_mrs_update"));
    WtGuard guard_(b->ctx);
    if (!tau) WT_FAIL("wt_batch_mrs_update: null tau");
    if (plane == mrs_plane) WT_FAIL("wt_batch_mrs_update: plane and mrs_plane must differ");
    float *c = nullptr, *m = nullptr;
    WT_TRY(bplane(b, plane, &c));
    WT_TRY(bplane(b, mrs_plane, &m));
    std::vector<double> pairs((size_t)nf * 2, 0.0);
    for (int f = 0; f < nf; ++f) pairs[2 * f] = tau[f];
    const double *dt = nullptr;
    WT_TRY(batch_table(b, nf, pairs.data(), &dt));
    ProfScope ps(b->ctx, "wt_batch_mrs_kernel");
    hipLaunchKernelGGL(wt_batch_mrs_kernel, dim3(batch_flat_blocks(b, nf), nf), dim3(256), 0, b->ctx->stream, c, m, b->fstride / 4, dt, soft, persistent,
                       inv_pow);
    WT_HIP(hipGetLastError());
    return 0;
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
    WT_TRY(bplane(b, src, &s));
    b->fft.have_spec = false;
    WT_TRY(wt_fft32_prepare(b->ctx, b->fft, g.H, g.W, b->fft_allocs, b->n));
    return wt_fft32_spectrum(b->ctx, b->fft, s, g.P);
}

// wt_fft_apply per frame (watroo/utils.py:254: irfft2(rfft2(psi) * fft_psf); conj, utils.py:284: * conj(fft_psf)) with
// the batch's one kernel spectrum: six launches for all active frames, no stream drain, no host round trip
extern "C" int wt_batch_fft_apply(wt_batch *b, int nf, int src, int dst, int conj)
{
    WT_TRY(check_frames(b, nf, "wt_batch_fft_apply"));
    WtGuard guard_(b->ctx);
    if (src == dst) WT_FAIL("wt_batch_fft_apply: src and dst must differ");
    float *s = nullptr, *d = nullptr;
    WT_TRY(bplane(b, src, &s));
    WT_TRY(bplane(b, dst, &d));
    if (!b->fft.have_spec) WT_FAIL("wt_batch_fft_apply: the batch has no kernel spectrum (wt_batch_fft_spectrum first)");
    return wt_fft32_apply(b->ctx, b->fft, s, d, b->geo.g.P, conj, nf, b->fstride);
}
