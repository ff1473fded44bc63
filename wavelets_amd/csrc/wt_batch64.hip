// Batched float64 engine (wt_batch64): the float64 counterpart of wt_batch (wt_batch.hip) for stacks the reference
// computes in float64 - native float64 frames, and the integer / big-endian frames it recasts to float64
// (watroo/wavelets.py:297, 319-320).  N frames of the same H x W go through each fused pass in ONE launch, the frame
// index a grid dimension (wt_fused_batch_kernel<double, ...>, the units fused_f64_k*_batch_acc*).
//
// Layout: every plane is one allocation of N frames back to back, frame f at f * H * P doubles (P = the pitch of a
// wt_plan64 of the same width, even).  A plane is therefore also ONE tall image of N * H rows: transfers, the
// widening of integer frames, Anscombe and the thresholds + plane sum run once over the whole stack.  Only the fused
// passes see frames: each frame is its own image there, with the per-frame float64 schedule, kernel choice and
// geometry (the batch's wt_plan64 `geo` is the one a wt_plan64 of that shape has), so a frame's bits are those of
// the per-frame call.
// The MAD median is a per-frame radix select over the 63 magnitude bits of a double (six histogram levels of
// 11 / 11 / 11 / 11 / 11 / 8 bits, the levels of wt64_abs_median), two ranks per frame for an even pixel count:
// N exact medians for one host round trip.
// wow (watroo/utils.py:105-219) runs on the same planes: schedules beyond the fused passes (from 9 scales on) take the
// batched per-scale stencil for their single-scale passes, the fused update of a scale is ONE launch of that stencil
// for all frames (wt_stencil64_batch.hip), and the pointwise update, the gamma blend, the moments and the plane sum
// are the per-frame kernels' texts (wt_wow64.h) with the frame as a grid dimension.
// richardson_lucy (watroo/utils.py:222-290) runs on the same planes plus its own (data, psi, phi, residual,
// correlation, one support plane per scale): the PSF correlation of all frames is ONE launch of the tiled kernel
// (wt_batch64_filter2d_kernel: wt_rl_point.h's 64 x 16 tile staged in LDS as doubles, the two operands resident in
// the batch), the binary ops run once over the frames as a flat range, the support update has the frame as grid y.
// What lives where: this file has the float64 kernels and launch lines, the median select, the widening upload and
// the shape rules of the float64 schedules.  The host side both engines share is wt_batch_core.h and wt_batch_rl.h
// (see wt_batch.hip); what this engine does differently there stays here, in the open: richardson_lucy's planes become
// planes of the batch at the first wt_batch64_set_psf, and wt_batch64_binary renumbers the op for wt64_binary_point.
// The three threshold sums are shells around one body in the float64 arithmetic (wt_batch64_threshold_sum).
#include <algorithm>
#include <cstring>
#include <vector>

#include "wt_batch_rl.h"
#include "wt_math64.h"
#include "wt_reduce.h"
#include "wt_wow64.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

struct WtBatch64Sel {               // select state of one rank of one frame
    unsigned long long k;           // rank still to find among the keys matching `prefix`
    unsigned long long prefix;      // key bits fixed so far
    uint32_t failed, pad;           // failed: the rank lies beyond the frame's keys (never, with every key counted)
};

// (richardson_lucy's planes and PSFs: wt_batch_rl.h.  The planes belong to a batch from its first wt_batch64_set_psf
//  on: a batch without a PSF keeps the plane list every other stack function sees.)
struct wt_batch64 : WtBatchRl<double> {
    wt_batch64() : WtBatchRl<double>("wt_batch64") {}
    wt_plan64 geo;                  // ONE frame's geometry, context and taps: what the fused launches read (no planes)
    void *istage = nullptr;         // frames of another element type on their way into a plane
    size_t istage_cap = 0;
    uint32_t *d_hist = nullptr;     // [n][2 ranks][WT_HIST_BINS] (allocated by the first median)
    WtBatch64Sel *d_sel = nullptr;  // [n][2 ranks]
    WtBatch64Sel *h_sel = nullptr;  // pinned copy
    // (d_tau: [n][3 * WT_MAX_SUM_PLANES], the thresholds of wt_batch64_denoise_sum, then 1 / tau; wt_batch64_enhance_sum: then the weights)
};

// ------------------------------------------------------------------------------------------------ kernels
// One radix level of the per-frame select: bins of (key >> shift) & bmask over the keys of frame blockIdx.y that
// match a rank's prefix (key = the magnitude bits of a double: their order is the order of |x|; NaN keys order
// above infinity and are counted, as wt64_hist_kernel counts them).
__global__ __launch_bounds__(256) void wt_batch64_hist_kernel(const double *p, int H, int P, int W, int64_t fstride, unsigned long long mask,
                                                              int shift, uint32_t bmask, const WtBatch64Sel *st, uint32_t *hist)
{
    __shared__ uint32_t lh[2][WT_HIST_BINS];
    const int f = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * WT_HIST_BINS; i += 256) lh[i / WT_HIST_BINS][i % WT_HIST_BINS] = 0;
    __syncthreads();
    const unsigned long long pre0 = st[2 * f].prefix & mask, pre1 = st[2 * f + 1].prefix & mask;
    const double *fp = p + (int64_t)f * fstride;
    const int X2 = (W + 1) / 2;                          // double2 groups per row (P even: 16-byte aligned rows)
    const int64_t items = (int64_t)H * X2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i / X2), c2 = (int)(i % X2);
        const double2 v = *reinterpret_cast<const double2 *>(fp + (int64_t)row * P + 2 * c2);
        const double e[2] = {v.x, v.y};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (2 * c2 + j >= W) continue;
            const unsigned long long key = (unsigned long long)__double_as_longlong(e[j]) & 0x7fffffffffffffffull;
            const uint32_t bin = (uint32_t)(key >> shift) & bmask;
            if ((key & mask) == pre0) atomicAdd(&lh[0][bin], 1u);
            if ((key & mask) == pre1) atomicAdd(&lh[1][bin], 1u);
        }
    }
    __syncthreads();
    uint32_t *gh = hist + (int64_t)f * 2 * WT_HIST_BINS;
    for (int i = threadIdx.x; i < 2 * WT_HIST_BINS; i += 256) {
        const uint32_t c = lh[i / WT_HIST_BINS][i % WT_HIST_BINS];
        if (c) atomicAdd(&gh[i], c);
    }
}

// The bin of one rank (block = frame * 2 + rank): fixes bmask's bits of the prefix, leaves the bins cleared.
__global__ __launch_bounds__(256) void wt_batch64_select_kernel(uint32_t *hist, WtBatch64Sel *st, int nbins, int shift)
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
    WtBatch64Sel &S = st[blockIdx.x];
    if (threadIdx.x == 0) {
        unsigned long long cum = 0;
        int t = -1;
        for (int i = 0; i < 256; ++i) {
            if (cum + part[i] > S.k) { t = i; break; }
            cum += part[i];
        }
        if (t < 0) S.failed = 1;
        sel_t = t;
        sel_before = cum;
    }
    __syncthreads();
    if ((int)threadIdx.x == sel_t) {
        unsigned long long cum = sel_before;
        int b = threadIdx.x * per + per - 1;
        for (int i = 0; i < per; ++i) {
            const uint32_t c = h[threadIdx.x * per + i];
            if (cum + c > S.k) { b = threadIdx.x * per + i; break; }
            cum += c;
        }
        S.prefix |= (unsigned long long)b << shift;
        S.k -= cum;
    }
    __syncthreads();
    for (int i = 0; i < per; ++i) h[threadIdx.x * per + i] = 0;
}

// wt64_denoise_sum_kernel (wt_kernels_f64.h) over the frames as one flat range, the frame from the flat index and its
// row of the table: ft[k] = tau, ft[n_den + k] = 1 / tau (the host's IEEE division, as wt64_denoise_sum).  Same
// expressions and accesses: the bits of the per-frame call.
//   MAP     rows of 2 * n_den + 1, ft[2 * n_den] = 1.0 for a frame with a per-pixel noise map (Coefficients.significance
//           with an ndarray noise, watroo/wavelets.py:133-141): such a frame thresholds at tau * nz by the quotient
//           (wt_sig64), as the per-frame kernel does with a noise plane; a frame whose noise is a scalar keeps the
//           reciprocal form of the map-free kernel (wt_sig64_inv) - the two differ by a rounding, so each frame takes
//           the form its per-frame call takes
//   ROW_WGT rows of 3 * n_den, ft[2 * n_den + k] = the frame's weight (utils.enhance per channel,
//           watroo/utils.py:60-78); else a.wgt[k]
struct Batch64DenoiseArgs {
    double *p[WT_MAX_SUM_PLANES];
    double wgt[WT_MAX_SUM_PLANES];
    int n, n_den, soft, write_back;
};
struct Batch64EnhanceArgs {
    double *p[WT_MAX_SUM_PLANES];
    int n, n_den, soft, write_back;
};
typedef double wt_b64_ntd2 __attribute__((ext_vector_type(2)));
template <bool MAP, bool ROW_WGT, typename Args>
__device__ __forceinline__ void wt_batch64_threshold_sum(const Args &a, const double *tab, const double *noise, double *dst, int64_t n2, int64_t f2)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
        const double *ft = tab + (ROW_WGT ? (i / f2) * 3 * a.n_den : MAP ? (i / f2) * (2 * a.n_den + 1) : (i / f2) * 2 * a.n_den);
        bool mapped = false;
        double2 nz = make_double2(1.0, 1.0);
        if constexpr (MAP) {
            mapped = ft[2 * a.n_den] != 0.0;
            nz = reinterpret_cast<const double2 *>(noise)[i];
        }
        double2 acc = make_double2(0.0, 0.0);
        for (int k = 0; k < a.n; ++k) {
            const wt_b64_ntd2 raw = __builtin_nontemporal_load(reinterpret_cast<const wt_b64_ntd2 *>(a.p[k]) + i);   // (read exactly once)
            double2 v = make_double2(raw.x, raw.y);
            if (k < a.n_den) {
                const double tau = ft[k], inv_tau = ft[a.n_den + k];
                double wgt;
                if constexpr (ROW_WGT) wgt = ft[2 * a.n_den + k];
                else wgt = a.wgt[k];
                double2 sg = make_double2(1.0, 1.0);
                if (tau > 0.0) {
                    if (mapped) sg = make_double2(wt_sig64(v.x, tau * nz.x, a.soft), wt_sig64(v.y, tau * nz.y, a.soft));
                    else sg = make_double2(wt_sig64_inv(v.x, tau, inv_tau, a.soft), wt_sig64_inv(v.y, tau, inv_tau, a.soft));
                }
                v = make_double2(v.x * (wgt * sg.x), v.y * (wgt * sg.y));
                if (a.write_back) reinterpret_cast<double2 *>(a.p[k])[i] = v;
            }
            acc = k == 0 ? v : make_double2(acc.x + v.x, acc.y + v.y);
        }
        __builtin_nontemporal_store((wt_b64_ntd2){acc.x, acc.y}, reinterpret_cast<wt_b64_ntd2 *>(dst) + i);
    }
}
__global__ __launch_bounds__(256) void wt_batch64_denoise_sum_kernel(Batch64DenoiseArgs a, const double *tab, double *dst, int64_t n2, int64_t f2)
{
    wt_batch64_threshold_sum<false, false>(a, tab, nullptr, dst, n2, f2);
}
__global__ __launch_bounds__(256) void wt_batch64_denoise_sum_map_kernel(Batch64DenoiseArgs a, const double *tab, const double *noise, double *dst,
                                                                         int64_t n2, int64_t f2)
{
    wt_batch64_threshold_sum<true, false>(a, tab, noise, dst, n2, f2);
}
__global__ __launch_bounds__(256) void wt_batch64_enhance_sum_kernel(Batch64EnhanceArgs a, const double *tab, double *dst, int64_t n2, int64_t f2)
{
    wt_batch64_threshold_sum<false, true>(a, tab, nullptr, dst, n2, f2);
}

// plane <- value over the active frames, pitch padding included (the noise plane before the maps go up: no lane
// computes on what hipMalloc left there); frame 0 of a plane -> frames 1 .. gridDim.y
__global__ __launch_bounds__(256) void wt_batch64_fill_kernel(double *d, int64_t n2, double value)
{
    batch_fill_groups(reinterpret_cast<double2 *>(d), n2, make_double2(value, value), 256u);
}
__global__ __launch_bounds__(256) void wt_batch64_replicate_kernel(double *d, int64_t f2)
{
    batch_replicate_groups(reinterpret_cast<double2 *>(d), f2, 256u);
}

// generalized_anscombe (watroo/wavelets.py:14-21) over the frames as one tall image: wt64_anscombe_kernel's expressions
__global__ __launch_bounds__(256) void wt_batch64_anscombe_kernel(const double *src, double *dst, int W, int P, int nrows, double alpha, double g,
                                                                  double sigma, int inverse)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < nrows; y += gridDim.y) {
        const int64_t o = (int64_t)y * P + x;
        const double v = src[o];
        double r;
        if (inverse) {
            const double h = alpha * v / 2.0;
            r = (h * h + alpha * g - sigma * sigma - 3.0 * alpha / 8.0) / alpha;
        } else {
            double dum = alpha * v + 3.0 * alpha * alpha / 8.0 + sigma * sigma - alpha * g;
            if (dum <= 0.0) dum = 0.0;
            r = 2.0 * sqrt(dum) / alpha;
        }
        dst[o] = r;
    }
}

// frames of another element type -> double planes (wt64_upload_int's widening: one element per thread from the
// tightly packed staging copy, SWAP = the other byte order); the frames are one tall image of nrows = nf * H rows
template <int N> struct WtB64Uint;
template <> struct WtB64Uint<1> { typedef uint8_t T; };
template <> struct WtB64Uint<2> { typedef uint16_t T; };
template <> struct WtB64Uint<4> { typedef uint32_t T; };
template <> struct WtB64Uint<8> { typedef uint64_t T; };
__device__ __forceinline__ uint8_t wt_b64_bswap(uint8_t v) { return v; }
__device__ __forceinline__ uint16_t wt_b64_bswap(uint16_t v) { return __builtin_bswap16(v); }
__device__ __forceinline__ uint32_t wt_b64_bswap(uint32_t v) { return __builtin_bswap32(v); }
__device__ __forceinline__ uint64_t wt_b64_bswap(uint64_t v) { return __builtin_bswap64(v); }
template <typename I, bool SWAP>
__global__ __launch_bounds__(256) void wt_batch64_widen_kernel(const I *src, double *dst, int W, int P, int nrows)
{
    typedef typename WtB64Uint<sizeof(I)>::T U;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < nrows; y += gridDim.y) {
        U raw = reinterpret_cast<const U *>(src)[(int64_t)y * W + x];
        if (SWAP) raw = wt_b64_bswap(raw);
        dst[(int64_t)y * P + x] = (double)__builtin_bit_cast(I, raw);
    }
}

// wt64_wow_kernel (wt_kernels_f64.h) with the frame as grid z: no power plane, the frame's {tau, factor} (wow's last
// plane, whitening=False, h >= 1 - watroo/utils.py:185-203); `noise`: the batch's noise plane (a frame with a scalar
// level has ones there: tau * 1.0 is tau) or null.  Same wt64_wow_point: the bits of the per-frame call.
__global__ __launch_bounds__(256) void wt_batch64_wow_kernel(double *c, const double *noise, double *gamma, int W, int P, int nrows, int64_t fstride,
                                                             const double *ptab, int soft)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int f = blockIdx.z;
    const double tau = ptab[2 * f], factor = ptab[2 * f + 1];
    const int64_t fo = (int64_t)f * fstride;
    c += fo;
    if (noise) noise += fo;
    if (gamma) gamma += fo;
    for (int y = blockIdx.y; y < nrows; y += gridDim.y) {
        const int64_t o = (int64_t)y * P + x;
        c[o] = wt64_wow_point(c[o], false, 0.0, noise, gamma, o, tau, soft, factor);
    }
}

// wt64_gamma_kernel (wt_kernels_f64.h, watroo/utils.py:212-217) with the frame as grid z and its own {gmin, gmax}
__global__ __launch_bounds__(256) void wt_batch64_gamma_kernel(double *recon, const double *gamma, int W, int P, int nrows, int64_t fstride,
                                                               const double *ptab, double inv_gamma, double h)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int f = blockIdx.z;
    const double gmin = ptab[2 * f];
    const double range = ptab[2 * f + 1] - gmin;        // (wt64_gamma_blend: the same subtraction on the host)
    recon += (int64_t)f * fstride;
    gamma += (int64_t)f * fstride;
    for (int y = blockIdx.y; y < nrows; y += gridDim.y) {
        const int64_t o = (int64_t)y * P + x;
        recon[o] = wt64_gamma_point(recon[o], gamma[o], gmin, range, inv_gamma, h);
    }
}

// wt64_reduce_kernel + wt_reduce_final_kernel per frame (grid y / the final block = the frame): the per-frame split
// into gridDim.x row-strided blocks and the fold order of wt64_reduce, i.e. the doubles of the per-frame call
__global__ __launch_bounds__(256) void wt_batch64_reduce_kernel(const double *p, int nrows, int P, int W, int64_t fstride, double *partials)
{
    wt64_reduce_rows_block(p + (int64_t)blockIdx.y * fstride, nrows, P, W, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}
__global__ __launch_bounds__(256) void wt_batch64_reduce_final_kernel(const double *partials, int nblocks, double *out)
{
    wt_reduce_final_block(partials + (int64_t)blockIdx.x * nblocks * 4, nblocks, out + (int64_t)blockIdx.x * 4);
}

// wt64_plane_sum_kernel over the frames back to back (one flat range): the additions in plane order
__global__ __launch_bounds__(256) void wt_batch64_plane_sum_kernel(Sum64Args a, double *dst, int64_t n2)
{
    wt64_plane_sum_groups(a, dst, n2);
}

// wt64_filter2d_kernel (wt_kernels_f64.h) for the frames of a batch, tiled: wt_f2d_batch_tile (wt_rl_point.h) with
// T = double - the (64 + kw - 1) x (16 + kh - 1) window of a 64 x 16 output tile in dynamic LDS, four output rows per
// thread, taps as wave-uniform loads from the batch's device copy.  Every output is the chain
// acc = fma(psf[i * kw + j], v, acc) from 0.0, i outer, j inner, over the same samples (wt_refl / a true modulo
// pick the sample the per-frame kernel reads): the bits of wt64_filter2d on that frame.
template <bool WRAP>
__global__ __launch_bounds__(256) void wt_batch64_filter2d_kernel(const double *in, double *out, Geo g, int64_t fstride,
                                                                  const double *__restrict__ psf, int kh, int kw, int ay, int ax)
{
    extern __shared__ double tile64[];
    wt_f2d_batch_tile<WRAP, false>(tile64, in, out, g, fstride, psf, kh, kw, ay, ax);
}

// wt64_binary_kernel (wt_kernels_f64.h) over the active frames, one flat range of 16-byte groups (wt64_binary_point;
// op in wt64_binary's numbering)
__global__ __launch_bounds__(256) void wt_batch64_binary_kernel(const double *a, const double *b, double *dst, int64_t n2, int op)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
        const double2 u = reinterpret_cast<const double2 *>(a)[i], v = reinterpret_cast<const double2 *>(b)[i];
        reinterpret_cast<double2 *>(dst)[i] = make_double2(wt64_binary_point(u.x, v.x, op), wt64_binary_point(u.y, v.y, op));
    }
}

// wt64_mrs_kernel (wt_kernels_f64.h) with the frame as grid y and its own tau (ptab[2 * f]; <= 0: significance one);
// no noise map - richardson_lucy's noise is the data's MAD estimate.  Same wt64_mrs_point: the bits of the per-frame call.
__global__ __launch_bounds__(256) void wt_batch64_mrs_kernel(double *c, double *mrs, int64_t f2, const double *ptab, int soft, int persistent,
                                                             double inv_pow)
{
    const int f = blockIdx.y;
    const double tau = ptab[2 * f];
    double2 *cf = reinterpret_cast<double2 *>(c) + (int64_t)f * f2;
    double2 *mf = reinterpret_cast<double2 *>(mrs) + (int64_t)f * f2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < f2; i += (int64_t)gridDim.x * 256) {
        double2 v = cf[i], m = mf[i];
        wt64_mrs_point(v.x, m.x, tau, tau, soft, persistent, inv_pow);
        wt64_mrs_point(v.y, m.y, tau, tau, soft, persistent, inv_pow);
        cf[i] = v;
        mf[i] = m;
    }
}

// ------------------------------------------------------------------------------------------------ host
// fused64_ok (wt_f64.h) for one frame of this shape: an image (H >= 2) whose rows the fused passes take at 8 bytes
// per pixel and whose float64 schedule of `level` scales is fused passes only
static bool batch64_all_fused(int family, int64_t H, int64_t W, int level, int32_t *tr, int *np)
{
    if ((family != WT_B3SPLINE && family != WT_TRIANGLE) || H < 2 || W < 1 || level < 1) return false;
    if (!wt_fused_supported_bytes((W + 1) / 2 * 2 * 8)) return false;
    if (wt_schedule(family, level, 1, tr, 32, np)) return false;
    for (int i = 0; i < *np; ++i)
        if (!wt_fused_has_pass(tr[3 * i], tr[3 * i + 1], family)) return false;
    return true;
}

extern "C" int wt_batch64_fused_ok(int family, int64_t H, int64_t W, int level, int *ok)
{
    if (!ok) WT_FAIL("wt_batch64_fused_ok: null pointer");
    int32_t tr[3 * 32];
    int np = 0;
    *ok = batch64_all_fused(family, H, W, level, tr, &np) ? 1 : 0;
    return 0;
}

// The wider condition of wow's transform: `level` in 1..24 whose float64 schedule holds, besides fused passes,
// single-scale passes for the batched per-scale stencil - what fused64_run (wt_f64.h) gives one frame on the
// per-frame stencil - and the option "stencil64" on: with it off the per-frame call takes the two generic kernels
// per scale, for the passes and for wt64_wow_scale (stencil64_ok), whose bits differ.
static bool batch64_wow_shape_ok(int family, int64_t H, int64_t W, int level, int32_t *tr, int *np)
{
    if ((family != WT_B3SPLINE && family != WT_TRIANGLE) || H < 2 || W < 1 || H > INT32_MAX || W > INT32_MAX) return false;
    if (level < 1 || level > 24) return false;
    if (!wt_fused_supported_bytes((W + 1) / 2 * 2 * 8)) return false;
    if (!wt_get_stencil64()) return false;
    if (wt_schedule(family, level, 1, tr, 32, np)) return false;
    for (int i = 0; i < *np; ++i)
        if (!wt_fused_has_pass(tr[3 * i], tr[3 * i + 1], family) && tr[3 * i + 1] != 1) return false;
    return true;
}

extern "C" int wt_batch64_wow_ok(int family, int64_t H, int64_t W, int level, int *ok)
{
    if (!ok) WT_FAIL("wt_batch64_wow_ok: null pointer");
    int32_t tr[3 * 32];
    int np = 0;
    *ok = batch64_wow_shape_ok(family, H, W, level, tr, &np) ? 1 : 0;
    return 0;
}

static int batch64_pass(wt_batch64 *b, int nf, int cur, int nxt, int s0, int ns, int acc, int sum_plane, bool first)
{
    double *in = nullptr, *oc = nullptr, *ps = nullptr, *ow[WT_FUSED_MAX_SCALES] = {nullptr};
    WT_TRY(batch_pass_planes(b, cur, nxt, s0, ns, acc, sum_plane, first, &in, &oc, ow, &ps));
    // (the arguments of fused64_pass, wt_f64.h)
    FusedArgsT<double> a{};
    a.in = in;
    a.out_c = oc;
    for (int k = 0; k < 3; ++k) a.out_w[k] = ow[k];
    a.out_w3 = ow[3];
    a.g = b->geo.g;
    a.p_out = ps;
    a.p_in = first ? nullptr : ps;
    FusedRows rows;
    rows.frames = nf;
    rows.fstride = b->fstride;
    const bool b3 = b->family == WT_B3SPLINE;
    if (acc == 2) return b3 ? wt_fused_tu_f64_k5_batch_acc2(&b->geo, a, s0, ns, rows) : wt_fused_tu_f64_k3_batch_acc2(&b->geo, a, s0, ns, rows);
    if (acc == 1) return b3 ? wt_fused_tu_f64_k5_batch_acc1(&b->geo, a, s0, ns, rows) : wt_fused_tu_f64_k3_batch_acc1(&b->geo, a, s0, ns, rows);
    return b3 ? wt_fused_tu_f64_k5_batch_acc0(&b->geo, a, s0, ns, rows) : wt_fused_tu_f64_k3_batch_acc0(&b->geo, a, s0, ns, rows);
}

static int batch64_run(wt_batch64 *b, int nf, int src, int level, bool with_sum, int dst, const char *who)
{
    // (this engine refuses the level before it looks at the planes)
    if (level < 1 || level > b->max_level) WT_FAIL("%s: level %d outside [1, %d]", who, level, b->max_level);
    return batch_schedule_run(
        b, nf, src, level, with_sum, dst, who,
        // (the passes with a sum run fused kernels only; a transform alone also takes single-scale stencil passes)
        [b](int lv, bool sum, int32_t *tr, int *np, const char *w) -> int {
            if (!batch64_all_fused(b->family, b->geo.g.H, b->geo.g.W, lv, tr, np) &&
                (sum || !batch64_wow_shape_ok(b->family, b->geo.g.H, b->geo.g.W, lv, tr, np)))
                WT_FAIL("%s: %d scales have no %s float64 schedule for %d x %d frames (%s): not a batch case", w, lv, sum ? "all-fused" : "batched",
                        b->geo.g.H, b->geo.g.W, sum ? "wt64_plan_fused_ok" : "wt_batch64_wow_ok");
            return 0;
        },
        [b](int frames, int cur, int nxt, int s0, int ns, int acc, int sum_plane, bool first) {
            return batch64_pass(b, frames, cur, nxt, s0, ns, acc, sum_plane, first);
        });
}

// every buffer of the batch back to the runtime: the core's and the float64 engine's own
static void batch64_free(wt_batch64 *b, int *bad)
{
    batch_release(b, bad);
    auto f = [&](void *q) { if (q && hipFree(q) != hipSuccess) *bad = 1; };
    f(b->istage);
    f(b->d_hist);
    f(b->d_sel);
    batch_rl_release(b, bad);
    if (b->h_sel && hipHostFree(b->h_sel) != hipSuccess) *bad = 1;
}

extern "C" int wt_batch64_create(wt_ctx *ctx, int n, int H, int W, int family, int max_level, wt_batch64 **out)
{
    WtGuard guard_(ctx);
    WT_TRY(batch_check_create(ctx, out, n, H, W, family, max_level, "wt_batch64_create"));
    if (H < 2) WT_FAIL("wt_batch64_create: frames of one row are signals for the float64 engine (no fused passes)");
    if (!wt_fused_supported_bytes((int64_t)(W + 1) / 2 * 2 * 8)) WT_FAIL("wt_batch64_create: rows of %d pixels are too wide for the fused float64 passes", W);
    wt_batch64 *b = new wt_batch64;
    batch_init(b, ctx, n, H, W, (W + 1) / 2 * 2, family, max_level);
    // the geometry and taps a wt_plan64 of this shape has (wt64_plan_create)
    static const double b3[5] = {1. / 16, 1. / 4, 3. / 8, 1. / 4, 1. / 16}, tri[3] = {1. / 4, 1. / 2, 1. / 4};
    b->geo.ctx = ctx;
    b->geo.g = b->g;
    b->geo.max_level = max_level;
    b->geo.ntaps = family == WT_B3SPLINE ? 5 : 3;
    for (int i = 0; i < b->geo.ntaps; ++i) b->geo.taps[i] = family == WT_B3SPLINE ? b3[i] : tri[i];
    hipError_t e = hipMalloc((void **)&b->d_sel, (size_t)n * 2 * sizeof(WtBatch64Sel));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_tau, (size_t)n * 3 * WT_MAX_SUM_PLANES * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_sel, (size_t)n * 2 * sizeof(WtBatch64Sel), 0);
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_tau, (size_t)n * 3 * WT_MAX_SUM_PLANES * sizeof(double), 0);
    if (e != hipSuccess) {
        int bad = 0;
        batch64_free(b, &bad);
        delete b;
        wt_set_error("wt_batch64_create: HIP error %d (%s)", (int)e, hipGetErrorString(e));
        return 2;
    }
    *out = b;
    return 0;
}

extern "C" int wt_batch64_destroy(wt_batch64 *b)
{
    if (!b) return 0;
    WtGuard guard_(b->ctx);
    (void)hipStreamSynchronize(b->ctx->stream);
    int bad = 0;
    batch64_free(b, &bad);
    delete b;
    if (bad) WT_FAIL("wt_batch64_destroy: a device buffer could not be released");
    return 0;
}

extern "C" int wt_batch64_info(wt_batch64 *b, int64_t *info)
{
    return batch_info(b, info, "wt_batch64_info");
}

wt_ctx *wt_batch64_ctx(wt_batch64 *b) { return b->ctx; }

extern "C" int wt_batch64_plane_ptr(wt_batch64 *b, int plane, void **ptr, int64_t *frame_stride)
{
    return batch_plane_ptr(b, plane, ptr, frame_stride, "wt_batch64_plane_ptr");
}

extern "C" int wt_batch64_upload(wt_batch64 *b, int plane, int f0, int nf, const double *host, int64_t host_frame_stride)
{
    return batch_copy(b, plane, f0, nf, const_cast<double *>(host), host_frame_stride, true, "wt_batch64_upload");
}

extern "C" int wt_batch64_download(wt_batch64 *b, int plane, int f0, int nf, double *host, int64_t host_frame_stride)
{
    return batch_copy(b, plane, f0, nf, host, host_frame_stride, false, "wt_batch64_download");
}

template <typename I>
static void batch64_widen_launch(wt_batch64 *b, double *dst, int nrows, bool swap)
{
    const Geo &g = b->geo.g;
    const dim3 grid((g.W + 255) / 256, (unsigned)std::min(nrows, 32768)), block(256);
    if (swap) hipLaunchKernelGGL((wt_batch64_widen_kernel<I, true>), grid, block, 0, b->ctx->stream, (const I *)b->istage, dst, g.W, g.P, nrows);
    else hipLaunchKernelGGL((wt_batch64_widen_kernel<I, false>), grid, block, 0, b->ctx->stream, (const I *)b->istage, dst, g.W, g.P, nrows);
}

// wt64_upload_int for frames [f0, f0 + nf): a C-contiguous (nf, H, W) block of elements of type `dtype` crosses PCIe
// as it is and is widened (byte-swapped) into the plane by one kernel over the nf * H rows
extern "C" int wt_batch64_upload_elems(wt_batch64 *b, int plane, int f0, int nf, const void *host, int dtype)
{
    if (!b || !host) WT_FAIL("wt_batch64_upload_elems: null pointer");
    WT_TRY(batch_check_range(b, f0, nf, "wt_batch64_upload_elems"));
    WtGuard guard_(b->ctx);
    static const int isz[11] = {0, 1, 1, 2, 2, 4, 4, 8, 8, 4, 8};
    const bool swap = (dtype & WT_BYTESWAPPED) != 0;
    const int base = dtype & ~WT_BYTESWAPPED;
    if (base < WT_INT8 || base > WT_FLOAT64) WT_FAIL("wt_batch64_upload_elems: unknown element type %d", dtype);
    const Geo &g = b->geo.g;
    const int64_t nrows64 = (int64_t)nf * g.H;
    if (nrows64 > INT32_MAX) WT_FAIL("wt_batch64_upload_elems: %lld rows in one upload", (long long)nrows64);
    const int nrows = (int)nrows64;
    const size_t need = (size_t)nrows * (size_t)g.W * isz[base];
    WT_TRY(wt_side_join(b->ctx));
    double *q = nullptr;
    WT_TRY(batch_plane(b, plane, &q));
    if (b->istage_cap < need) {
        WT_HIP(hipStreamSynchronize(b->ctx->stream));
        if (b->istage) (void)hipFree(b->istage);
        b->istage = nullptr;
        b->istage_cap = 0;
        WT_HIP(hipMalloc(&b->istage, need));
        b->istage_cap = need;
    }
    const bool pinned = try_pin(host, need);
    hipError_t e = hipMemcpyAsync(b->istage, host, need, hipMemcpyHostToDevice, b->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->ctx->stream);      // (the host frames are free again)
    if (pinned) (void)hipHostUnregister(const_cast<void *>(host));
    WT_HIP(e);
    double *dst = q + (int64_t)f0 * b->fstride;
    switch (base) {
        case WT_INT8: batch64_widen_launch<int8_t>(b, dst, nrows, false); break;
        case WT_UINT8: batch64_widen_launch<uint8_t>(b, dst, nrows, false); break;
        case WT_INT16: batch64_widen_launch<int16_t>(b, dst, nrows, swap); break;
        case WT_UINT16: batch64_widen_launch<uint16_t>(b, dst, nrows, swap); break;
        case WT_INT32: batch64_widen_launch<int32_t>(b, dst, nrows, swap); break;
        case WT_UINT32: batch64_widen_launch<uint32_t>(b, dst, nrows, swap); break;
        case WT_INT64: batch64_widen_launch<int64_t>(b, dst, nrows, swap); break;
        case WT_UINT64: batch64_widen_launch<uint64_t>(b, dst, nrows, swap); break;
        case WT_FLOAT32: batch64_widen_launch<float>(b, dst, nrows, swap); break;
        default: batch64_widen_launch<double>(b, dst, nrows, swap); break;
    }
    WT_HIP(hipGetLastError());
    WT_HIP(hipStreamSynchronize(b->ctx->stream));          // (as wt64_upload_int: the staging copy is free again)
    return 0;
}

extern "C" int wt_batch64_decompose(wt_batch64 *b, int nf, int src, int level, int flags)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_decompose"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch64_decompose: a batch runs the fused passes (flags bit0)");
    if (level == 0) {
        double *s = nullptr;
        if (src == 0) WT_FAIL("wt_batch64_decompose: src plane 0 is the output plane");
        WT_TRY(batch_plane(b, src, &s));
        return batch_copy_to_plane0(b, nf, s);
    }
    return batch64_run(b, nf, src, level, false, WT_PLANE_NONE, "wt_batch64_decompose");
}

// When a frame of this shape takes the float64 bilateral march per frame (wt64_decompose_bilateral's `tiled`:
// stencil64_ok of a wt_plan64 of that shape - the option, a built-in family, an image), so that the batched march
// gives the per-frame call's bits; with the option off the per-frame call runs the generic three-kernel form.
static bool batch64_bilateral_shape_ok(int family, int64_t H, int64_t W, int level)
{
    if (family != WT_B3SPLINE && family != WT_TRIANGLE) return false;
    if (H < 2 || W < 1 || H > INT32_MAX || W > INT32_MAX) return false;
    if (!wt_fused_supported_bytes((W + 1) / 2 * 2 * 8)) return false;      // (the rows wt_batch64_create accepts)
    if (level < 1 || level > 25) return false;
    return wt_get_stencil64() != 0;
}

extern "C" int wt_batch64_bilateral_ok(int family, int64_t H, int64_t W, int level, int *ok)
{
    if (!ok) WT_FAIL("wt_batch64_bilateral_ok: null pointer");
    *ok = batch64_bilateral_shape_ok(family, H, W, level) ? 1 : 0;
    return 0;
}

// wt64_decompose_bilateral (wt_f64.h) for the active frames: batch_decompose_bilateral's loop on the batched march of
// wt_bilateral64_batch.hip; no three-kernel form, no side stream, no scale events.
extern "C" int wt_batch64_decompose_bilateral(wt_batch64 *b, int nf, int src, int level, const double *sigma_b, int bilateral_scaling, int flags)
{
    (void)flags;
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_decompose_bilateral"));
    WtGuard guard_(b->ctx);
    return batch_decompose_bilateral(
        b, nf, src, level, sigma_b, bilateral_scaling, "wt_batch64_decompose_bilateral",
        [b, level]() -> int {
            if (!batch64_bilateral_shape_ok(b->family, b->geo.g.H, b->geo.g.W, level))
                WT_FAIL("wt_batch64_decompose_bilateral: %d x %d frames do not take the float64 march per frame (wt_batch64_bilateral_ok): not a batch case",
                        b->geo.g.H, b->geo.g.W);
            return 0;
        },
        [b](const ChainArgsT<double> &a, int s, const WtFrames &fr) { return wt64_bilateral_batch_launch(batch_stencil_ctx(b), a, s, fr); });
}

extern "C" int wt_batch64_decompose_sum(wt_batch64 *b, int nf, int src, int level, int dst, int flags)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_decompose_sum"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch64_decompose_sum: a batch runs the fused passes (flags bit0)");
    return batch64_run(b, nf, src, level, true, dst, "wt_batch64_decompose_sum");
}

extern "C" int wt_batch64_decompose_pass(wt_batch64 *b, int nf, int cur, int nxt, int s0, int ns, int flags)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_decompose_pass"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch64_decompose_pass: a batch runs the fused passes (flags bit0)");
    return batch64_pass(b, nf, cur, nxt, s0, ns, 0, WT_PLANE_NONE, false);
}

extern "C" int wt_batch64_decompose_pass_sum(wt_batch64 *b, int nf, int cur, int nxt, int s0, int ns, int flags, int sum_plane, int first,
                                             int last)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_decompose_pass_sum"));
    WtGuard guard_(b->ctx);
    if (!(flags & 1)) WT_FAIL("wt_batch64_decompose_pass_sum: a batch runs the fused passes (flags bit0)");
    return batch64_pass(b, nf, cur, nxt, s0, ns, last ? 2 : 1, sum_plane, first != 0);
}

extern "C" int wt_batch64_abs_median(wt_batch64 *b, int nf, int plane, double *medians)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_abs_median"));
    if (!medians) WT_FAIL("wt_batch64_abs_median: null pointer");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    double *q = nullptr;
    WT_TRY(batch_plane(b, plane, &q));
    if (!b->d_hist) {
        WT_HIP(hipMalloc((void **)&b->d_hist, (size_t)b->n * 2 * WT_HIST_BINS * sizeof(uint32_t)));
        WT_HIP(hipMemsetAsync(b->d_hist, 0, (size_t)b->n * 2 * WT_HIST_BINS * sizeof(uint32_t), c->stream));
    }
    const Geo &g = b->geo.g;
    const int64_t N = (int64_t)g.H * g.W;
    const unsigned long long klo = (unsigned long long)((N - 1) / 2);
    for (int f = 0; f < nf; ++f)
        for (int r = 0; r < 2; ++r) b->h_sel[2 * f + r] = WtBatch64Sel{klo + ((N & 1) == 0 && r == 1 ? 1ull : 0ull), 0ull, 0u, 0u};
    WT_HIP(hipMemcpyAsync(b->d_sel, b->h_sel, (size_t)nf * 2 * sizeof(WtBatch64Sel), hipMemcpyHostToDevice, c->stream));
    const int64_t items = (int64_t)g.H * ((g.W + 1) / 2);
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>((items + 2047) / 2048, std::max(1, 8 * c->num_cus / nf)));
    // the radix levels of wt64_abs_median: 11 bits five times, then the last 8 (63 magnitude bits)
    const int shifts[6] = {52, 41, 30, 19, 8, 0};
    const int bits[6] = {11, 11, 11, 11, 11, 8};
    unsigned long long mask = 0;
    for (int lv = 0; lv < 6; ++lv) {
        const uint32_t bmask = (1u << bits[lv]) - 1u;
        {
            ProfScope ps(c, "wt_batch64_hist_kernel");
            hipLaunchKernelGGL(wt_batch64_hist_kernel, dim3(bx, nf), dim3(256), 0, c->stream, (const double *)q, g.H, g.P, g.W, b->fstride, mask,
                               shifts[lv], bmask, (const WtBatch64Sel *)b->d_sel, b->d_hist);
        }
        {
            ProfScope ps(c, "wt_batch64_select_kernel");
            hipLaunchKernelGGL(wt_batch64_select_kernel, dim3(2 * nf), dim3(256), 0, c->stream, b->d_hist, b->d_sel, (int)bmask + 1, shifts[lv]);
        }
        WT_HIP(hipGetLastError());
        mask |= (unsigned long long)bmask << shifts[lv];
    }
    WT_HIP(hipMemcpyAsync(b->h_sel, b->d_sel, (size_t)nf * 2 * sizeof(WtBatch64Sel), hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));               // the one host round trip for all nf medians
    for (int f = 0; f < nf; ++f)
        if (b->h_sel[2 * f].failed || b->h_sel[2 * f + 1].failed) WT_FAIL("wt_batch64_abs_median: rank %llu of frame %d not found", klo, f);
    for (int f = 0; f < nf; ++f) {
        double lo, hi;
        memcpy(&lo, &b->h_sel[2 * f].prefix, 8);
        memcpy(&hi, &b->h_sel[2 * f + 1].prefix, 8);
        // np.median of float64: the mean of the two middle values of an even count (as wt64_abs_median)
        medians[f] = (N & 1) ? lo : (lo + hi) / 2.0;
    }
    return 0;
}

// the head of a frame's row of the threshold table: tau, then 1 / tau (the host's IEEE division: wt64_denoise_sum's inv_tau)
static void batch64_tau_row(double *r, const double *tau, int n_den)
{
    for (int k = 0; k < n_den; ++k) {
        r[k] = tau[k];
        r[n_den + k] = tau[k] > 0.0 ? 1.0 / tau[k] : 0.0;
    }
}

// x blocks of the flat kernels over n2 16-byte groups (not wt_host.h's flat_grid: that one stops at 2048 blocks)
static dim3 batch64_flat_grid(int64_t n2)
{
    return dim3((unsigned)std::min<int64_t>((n2 + 255) / 256, 256 * 16 * 8));
}

// wt_batch64_denoise_sum / wt_batch64_denoise_sum_map (map: with the noise plane and the frames' has_map flags)
static int batch64_denoise_sum(wt_batch64 *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft, int write_back,
                               bool map, int noise_plane, const int *has_map, const char *who)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    WT_TRY(batch_check_sum(b, count, dst, n_den, 0, tau, wgt, who));
    if (map && noise_plane == WT_PLANE_NONE) WT_FAIL("%s: no noise plane (wt_batch64_denoise_sum is the call without a map)", who);
    if (map && (noise_plane == dst || (noise_plane >= 0 && noise_plane < count))) WT_FAIL("%s: the noise plane %d is a plane of the sum", who, noise_plane);
    Batch64DenoiseArgs a{};
    double *o = nullptr, *nz = nullptr;
    WT_TRY(batch_sum_args(b, count, dst, n_den, soft, write_back, &a, &o));
    for (int i = 0; i < count; ++i) a.wgt[i] = i < n_den ? wgt[i] : 1.0;
    if (map) WT_TRY(batch_plane(b, noise_plane, &nz));
    // rows of {tau, 1 / tau} (two 0.0 when no plane is thresholded); with a map: then 1.0 for a frame that has one
    // (nf <= n, n_den <= WT_MAX_SUM_PLANES: within the tables)
    const int row = map ? 2 * n_den + 1 : 2 * std::max(n_den, 1);
    WT_TRY(batch_sum_table(b, nf, row, [&](int f, double *r) {
        batch64_tau_row(r, tau + f * n_den, n_den);
        if (map) r[2 * n_den] = (!has_map || has_map[f]) ? 1.0 : 0.0;
        else if (n_den == 0) r[0] = r[1] = 0.0;
    }));
    const int64_t n2 = (int64_t)nf * b->fstride / 2;
    if (map) {
        ProfScope ps(b->ctx, "wt_batch64_denoise_sum_map_kernel");
        hipLaunchKernelGGL(wt_batch64_denoise_sum_map_kernel, batch64_flat_grid(n2), dim3(256), 0, b->ctx->stream, a, (const double *)b->d_tau,
                           (const double *)nz, o, n2, b->fstride / 2);
    } else {
        ProfScope ps(b->ctx, "wt_batch64_denoise_sum_kernel");
        hipLaunchKernelGGL(wt_batch64_denoise_sum_kernel, batch64_flat_grid(n2), dim3(256), 0, b->ctx->stream, a, (const double *)b->d_tau, o, n2,
                           b->fstride / 2);
    }
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch64_denoise_sum(wt_batch64 *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft,
                                      int write_back)
{
    return batch64_denoise_sum(b, nf, count, dst, n_den, tau, wgt, soft, write_back, false, WT_PLANE_NONE, nullptr, "wt_batch64_denoise_sum");
}

extern "C" int wt_batch64_denoise_sum_map(wt_batch64 *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft,
                                          int write_back, int noise_plane, const int *has_map)
{
    return batch64_denoise_sum(b, nf, count, dst, n_den, tau, wgt, soft, write_back, true, noise_plane, has_map, "wt_batch64_denoise_sum_map");
}

extern "C" int wt_batch64_fill(wt_batch64 *b, int nf, int plane, double value)
{
    return batch_fill(b, nf, plane, "wt_batch64_fill", [&](double *d) {
        const int64_t n2 = (int64_t)nf * b->fstride / 2;
        ProfScope ps(b->ctx, "wt_batch64_fill_kernel");
        hipLaunchKernelGGL(wt_batch64_fill_kernel, batch64_flat_grid(n2), dim3(256), 0, b->ctx->stream, d, n2, value);
    });
}

extern "C" int wt_batch64_replicate(wt_batch64 *b, int nf, int plane)
{
    return batch_replicate(b, nf, plane, "wt_batch64_replicate", [&](double *d) {
        const int64_t f2 = b->fstride / 2;
        ProfScope ps(b->ctx, "wt_batch64_replicate_kernel");
        hipLaunchKernelGGL(wt_batch64_replicate_kernel, dim3(batch_frame_blocks(f2, nf), nf - 1), dim3(256), 0, b->ctx->stream, d, f2);
    });
}

extern "C" int wt_batch64_enhance_sum(wt_batch64 *b, int nf, int count, int dst, int n_den, const double *tau, const double *wgt, int soft,
                                      int write_back)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_enhance_sum"));
    WtGuard guard_(b->ctx);
    WT_TRY(batch_check_sum(b, count, dst, n_den, 1, tau, wgt, "wt_batch64_enhance_sum"));
    Batch64EnhanceArgs a{};
    double *o = nullptr;
    WT_TRY(batch_sum_args(b, count, dst, n_den, soft, write_back, &a, &o));
    // rows of {tau, 1 / tau, the weights} (nf <= n, n_den <= WT_MAX_SUM_PLANES: within the tables)
    WT_TRY(batch_sum_table(b, nf, 3 * n_den, [&](int f, double *r) {
        batch64_tau_row(r, tau + f * n_den, n_den);
        for (int k = 0; k < n_den; ++k) r[2 * n_den + k] = wgt[f * n_den + k];
    }));
    const int64_t n2 = (int64_t)nf * b->fstride / 2;
    ProfScope ps(b->ctx, "wt_batch64_enhance_sum_kernel");
    hipLaunchKernelGGL(wt_batch64_enhance_sum_kernel, batch64_flat_grid(n2), dim3(256), 0, b->ctx->stream, a, (const double *)b->d_tau, o, n2,
                       b->fstride / 2);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch64_anscombe(wt_batch64 *b, int nf, int src, int dst, double alpha, double g, double sigma, int inverse)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_anscombe"));
    WtGuard guard_(b->ctx);
    if (alpha == 0.0) WT_FAIL("wt_batch64_anscombe: alpha must be non-zero");
    double *s = nullptr, *d = nullptr;
    WT_TRY(batch_plane(b, src, &s));
    WT_TRY(batch_plane(b, dst, &d));
    const Geo &geo = b->geo.g;
    const int64_t nrows64 = (int64_t)nf * geo.H;
    if (nrows64 > INT32_MAX) WT_FAIL("wt_batch64_anscombe: %lld rows", (long long)nrows64);
    const int nrows = (int)nrows64;
    ProfScope ps(b->ctx, "wt_batch64_anscombe_kernel");
    hipLaunchKernelGGL(wt_batch64_anscombe_kernel, dim3((geo.W + 255) / 256, (unsigned)std::min(nrows, 32768)), dim3(256), 0, b->ctx->stream,
                       (const double *)s, d, geo.W, geo.P, nrows, alpha, g, sigma, inverse);
    WT_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ wow
// grid of the batched pointwise kernels: wt64's (x blocks, rows) per frame, the frame as grid z
static dim3 batch64_point_grid(const wt_batch64 *b, int nf)
{
    const Geo &g = b->geo.g;
    return dim3((g.W + 255) / 256, (unsigned)std::max(1, std::min(g.H, (4096 + nf - 1) / nf)), (unsigned)nf);
}

// wt_batch64_wow_update / wt_batch64_wow_update_map: noise_plane == WT_PLANE_NONE runs without a map
static int batch64_wow_update(wt_batch64 *b, int nf, int plane, const double *tau, int soft, const double *factor, int gamma_plane, int noise_plane,
                              const char *who)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    double *c = nullptr, *gm = nullptr, *nz = nullptr;
    const double *dt = nullptr;
    WT_TRY(batch_wow_update_args(b, nf, plane, tau, factor, gamma_plane, noise_plane, who, &c, &gm, &nz, &dt));
    const Geo &g = b->geo.g;
    ProfScope ps(b->ctx, nz ? "wt_batch64_wow_map_kernel" : "wt_batch64_wow_kernel");
    hipLaunchKernelGGL(wt_batch64_wow_kernel, batch64_point_grid(b, nf), dim3(256), 0, b->ctx->stream, c, (const double *)nz, gm, g.W, g.P, g.H,
                       b->fstride, dt, soft);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch64_wow_update(wt_batch64 *b, int nf, int plane, const double *tau, int soft, const double *factor, int gamma_plane)
{
    return batch64_wow_update(b, nf, plane, tau, soft, factor, gamma_plane, WT_PLANE_NONE, "wt_batch64_wow_update");
}

extern "C" int wt_batch64_wow_update_map(wt_batch64 *b, int nf, int plane, const double *tau, int soft, const double *factor, int gamma_plane,
                                         int noise_plane)
{
    if (noise_plane == WT_PLANE_NONE) WT_FAIL("wt_batch64_wow_update_map: no noise plane (wt_batch64_wow_update is the call without a map)");
    return batch64_wow_update(b, nf, plane, tau, soft, factor, gamma_plane, noise_plane, "wt_batch64_wow_update_map");
}

// wt_batch64_wow_scale / wt_batch64_wow_scale_map: noise_plane == WT_PLANE_NONE runs the instantiations without a map
static int batch64_wow_scale(wt_batch64 *b, int nf, int plane, int s, const double *tau, int soft, const double *factor, int gamma_plane,
                             int noise_plane, const char *who)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    WT_TRY(batch_check_wow_scale(b, plane, s, who));
    if (!wt_get_stencil64()) WT_FAIL("%s: option stencil64 is off (the per-frame call runs the generic kernels): not a batch case", who);
    return batch_wow_scale_run(b, nf, plane, s, tau, soft, factor, gamma_plane, noise_plane, who);
}

extern "C" int wt_batch64_wow_scale(wt_batch64 *b, int nf, int plane, int s, const double *tau, int soft, const double *factor, int gamma_plane)
{
    return batch64_wow_scale(b, nf, plane, s, tau, soft, factor, gamma_plane, WT_PLANE_NONE, "wt_batch64_wow_scale");
}

extern "C" int wt_batch64_wow_scale_map(wt_batch64 *b, int nf, int plane, int s, const double *tau, int soft, const double *factor, int gamma_plane,
                                        int noise_plane)
{
    if (noise_plane == WT_PLANE_NONE) WT_FAIL("wt_batch64_wow_scale_map: no noise plane (wt_batch64_wow_scale is the call without a map)");
    return batch64_wow_scale(b, nf, plane, s, tau, soft, factor, gamma_plane, noise_plane, "wt_batch64_wow_scale_map");
}

extern "C" int wt_batch64_reduce(wt_batch64 *b, int nf, int plane, double *out)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_reduce"));
    if (!out) WT_FAIL("wt_batch64_reduce: null pointer");
    WtGuard guard_(b->ctx);
    wt_ctx *c = b->ctx;
    double *q = nullptr;
    WT_TRY(batch_plane(b, plane, &q));
    const Geo &g = b->geo.g;
    // (wt64_reduce's split: row-strided blocks, at most partial_blocks of them, per frame)
    const int blocks = std::min(g.H, c->partial_blocks);
    WT_TRY(batch_reduce_buffers(b, blocks, true));
    {
        ProfScope ps(c, "wt_batch64_reduce_kernel");
        hipLaunchKernelGGL(wt_batch64_reduce_kernel, dim3(blocks, nf), dim3(256), 0, c->stream, (const double *)q, g.H, g.P, g.W, b->fstride, b->d_red);
        hipLaunchKernelGGL(wt_batch64_reduce_final_kernel, dim3(nf), dim3(256), 0, c->stream, (const double *)b->d_red, blocks, batch_reduce_results(b));
    }
    return batch_reduce_fetch(b, nf, out);
}

extern "C" int wt_batch64_gamma_blend(wt_batch64 *b, int nf, int recon, int gamma_plane, const double *gmin, const double *gmax, double inv_gamma,
                                      double h)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_gamma_blend"));
    if (!gmin || !gmax) WT_FAIL("wt_batch64_gamma_blend: null gmin / gmax");
    WtGuard guard_(b->ctx);
    if (recon == gamma_plane) WT_FAIL("wt_batch64_gamma_blend: recon and gamma planes must differ");
    double *r = nullptr, *g = nullptr;
    WT_TRY(batch_plane(b, recon, &r));
    WT_TRY(batch_plane(b, gamma_plane, &g));
    const double *dt = nullptr;
    WT_TRY(batch_pairs(b, nf, gmin, gmax, &dt));
    const Geo &geo = b->geo.g;
    ProfScope ps(b->ctx, "wt_batch64_gamma_kernel");
    hipLaunchKernelGGL(wt_batch64_gamma_kernel, batch64_point_grid(b, nf), dim3(256), 0, b->ctx->stream, r, (const double *)g, geo.W, geo.P, geo.H,
                       b->fstride, dt, inv_gamma, h);
    WT_HIP(hipGetLastError());
    return 0;
}

extern "C" int wt_batch64_plane_sum(wt_batch64 *b, int nf, int first, int count, int dst)
{
    WT_TRY(batch_check_frames(b, nf, "wt_batch64_plane_sum"));
    WtGuard guard_(b->ctx);
    Sum64Args a{};
    a.n = count;
    double *o = nullptr;
    WT_TRY(batch_plane_sum_planes(b, first, count, dst, 32, "wt_batch64_plane_sum", a.p, &o));
    // the frames back to back are one flat range: wt64_plane_sum_kernel's groups over all of them
    const int64_t n2 = (int64_t)nf * b->fstride / 2;
    ProfScope ps(b->ctx, "wt_batch64_plane_sum_kernel");
    hipLaunchKernelGGL(wt_batch64_plane_sum_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, b->ctx->stream, a, o, n2);
    WT_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ richardson_lucy
// (wt_batch_rl.h with T = double: the LDS tile holds doubles, so fewer PSFs go in one launch than in float32)
extern "C" int wt_batch64_psf_ok(int kh, int kw, int *ok)
{
    return batch_psf_ok<double>(kh, kw, ok, "wt_batch64_psf_ok");
}

// The first PSF makes richardson_lucy's planes planes of this batch.
extern "C" int wt_batch64_set_psf(wt_batch64 *b, int slot, const double *kernel, int kh, int kw)
{
    WT_TRY(batch_set_psf(b, slot, kernel, kh, kw, "wt_batch64_set_psf"));
    batch_rl_own_planes(b);
    return 0;
}

extern "C" int wt_batch64_filter2d(wt_batch64 *b, int nf, int src, int dst, int slot, int ay, int ax, int border)
{
    return batch_filter2d(b, nf, src, dst, slot, ay, ax, border, "wt_batch64_filter2d", "wt_batch64_filter2d_kernel",
                          [](bool periodic) { return periodic ? wt_batch64_filter2d_kernel<true> : wt_batch64_filter2d_kernel<false>; });
}

// op: wt_batch_binary's numbering (WT_OP_*); wt64_binary_point counts add, sub, ...
extern "C" int wt_batch64_binary(wt_batch64 *b, int nf, int op, int a, int b2, int dst)
{
    return batch_binary(b, nf, op, a, b2, dst, "wt_batch64_binary", [&](const double *pa, const double *pb, double *pd) {
        const int op64 = op == WT_OP_SUB ? 1 : op == WT_OP_ADD ? 0 : op;
        const int64_t n2 = (int64_t)nf * b->fstride / 2;
        ProfScope ps(b->ctx, "wt_batch64_binary_kernel");
        hipLaunchKernelGGL(wt_batch64_binary_kernel, batch64_flat_grid(n2), dim3(256), 0, b->ctx->stream, pa, pb, pd, n2, op64);
    });
}

extern "C" int wt_batch64_mrs_update(wt_batch64 *b, int nf, int plane, int mrs_plane, const double *tau, int soft, int persistent, double inv_pow)
{
    return batch_mrs_update(b, nf, plane, mrs_plane, tau, "wt_batch64_mrs_update", [&](double *c, double *m, const double *dt) {
        const int64_t f2 = b->fstride / 2;
        ProfScope ps(b->ctx, "wt_batch64_mrs_kernel");
        hipLaunchKernelGGL(wt_batch64_mrs_kernel, dim3(batch_frame_blocks(f2, nf), nf), dim3(256), 0, b->ctx->stream, c, m, f2, dt, soft, persistent, inv_pow);
    });
}
