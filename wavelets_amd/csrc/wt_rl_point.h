// Richardson-Lucy support shared by the per-image kernels (wt_kernels_apps.h) and the batched ones (wt_batch.hip,
// wt_batch64.hip): the PSF correlation's tile geometry, staging, border rules and the batched tile body, and the
// pointwise arithmetic of the binary ops and
// of the multiresolution-support update.  One text for both, so a frame of a batch gets the bits of the per-image
// call (watroo/utils.py:222-290).
#pragma once
#include <hip/hip_runtime.h>

#include "wt_internal.h"
#include "wt_device.h"
#include "wt_stencil.h"

// cv2.filter2D(src, -1, kernel, dst, (-1,-1), 0, BORDER_REFLECT) with an arbitrary small PSF
// (watroo/utils.py:257,286): correlation, anchor = kernel centre (k/2), symmetric border.
// 64 x 16 output tile + halo staged in LDS; the PSF taps are wave-uniform scalar loads.
#define WT_F2D_TW 64
#define WT_F2D_TH 16
// a PSF the correlation applies in ONE launch without bands: at most 4096 taps in rows of at most 512, and an LDS
// tile of at most 96 KB (wt_filter2d_ex's band rule; wt_batch_filter2d takes these PSFs only)
#define WT_F2D_MAX_TAPS 4096
#define WT_F2D_MAX_KW 512
#define WT_F2D_MAX_LDS (96 * 1024)
// (elem: bytes of a staged sample - floats, or the doubles of wt_batch64_filter2d_kernel)
static inline size_t wt_f2d_lds_bytes(int kh, int kw, size_t elem = sizeof(float))
{
    return (size_t)(WT_F2D_TW + kw - 1) * (WT_F2D_TH + kh - 1) * elem;
}
static inline bool wt_f2d_single_launch(int kh, int kw, size_t elem = sizeof(float))
{
    return kh >= 1 && kw >= 1 && kw <= WT_F2D_MAX_KW && (int64_t)kh * kw <= WT_F2D_MAX_TAPS && wt_f2d_lds_bytes(kh, kw, elem) <= WT_F2D_MAX_LDS;
}
// (the float64 batch asks with elem = sizeof(double): the same tile geometry at twice the bytes, wt_batch_rl.h)

// WRAP: periodic border (the circular convolution of the reference's rFFT path,
// watroo/utils.py:245-254,284), whole-image plans only; (ay, ax) = anchor of the correlation.
__device__ __forceinline__ int wt_wrap(int i, int n)
{
    const int m = i % n;
    return m < 0 ? m + n : m;
}

// the (WT_F2D_TW + kw - 1) x (WT_F2D_TH + kh - 1) input window of the output tile at (x0, local row ly0) -> LDS,
// by the 256 threads of the block (T: float, or double for the float64 batch)
template <bool WRAP, typename T>
__device__ __forceinline__ void wt_f2d_stage(T *tile, const T *in, const Geo &g, int x0, int ly0, int tw, int th, int ay, int ax)
{
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < tw * th; i += 256) {
        const int ty = i / tw, tx = i - ty * tw;
        if (WRAP) {
            const T *row = in + (int64_t)wt_wrap(ly0 + ty - ay, g.H) * g.P;
            tile[i] = row[wt_wrap(x0 + tx - ax, g.W)];
        } else {
            const T *row = wt_row(in, g, g.row0 + ly0 + ty - ay);
            tile[i] = row[wt_refl(x0 + tx - ax, g.W)];
        }
    }
}

// the four output rows threadIdx.y * 4 + r of column threadIdx.x: acc[r] = fmaf(k[i][j], v, acc[r]), i outer, j inner
// (T = double: fma, the chain of wt64_filter2d_kernel)
__device__ __forceinline__ float wt_f2d_fma(float k, float v, float acc) { return fmaf(k, v, acc); }
__device__ __forceinline__ double wt_f2d_fma(double k, double v, double acc) { return fma(k, v, acc); }
template <typename T>
__device__ __forceinline__ void wt_f2d_taps(const T *tile, int tw, const T *psf, int psf_pitch, int kh, int kw, T acc[4])
{
    for (int i = 0; i < kh; ++i)
        for (int j = 0; j < kw; ++j) {
            const T k = psf[i * psf_pitch + j];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[r] = wt_f2d_fma(k, tile[(threadIdx.y * 4 + r + i) * tw + threadIdx.x + j], acc[r]);
        }
}

// wt_f2d_taps with the loops skewed: the staged row t = i + r is walked once, and each value read from LDS feeds the
// FMAs of all the output rows r that have a tap row i = t - r there (up to four) - one LDS read per four FMAs in
// the steady rows instead of one per FMA.  Every acc[r] still sees its taps with i ascending and j inside: the
// same chain of fmaf, the same bits.  Measured on MI355X it is about half as fast as wt_f2d_taps:
// four scalar tap loads per step and the edge rows' branches cost more than the LDS reads save; kept for that
// measurement only (WT_BATCH_F2D_SKEW).
__device__ __forceinline__ void wt_f2d_taps_skewed(const float *tile, int tw, const float *__restrict__ psf, int kh, int kw, float acc[4])
{
    const float *col = tile + threadIdx.y * 4 * tw + threadIdx.x;
    for (int t = 0; t < kh + 3; ++t) {
        const float *row = col + t * tw;
        const float *k0 = psf + t * kw;            // tap row of r = 0; r's is r rows above
        if (t >= 3 && t < kh) {
            for (int j = 0; j < kw; ++j) {
                const float v = row[j];
                acc[0] = fmaf(k0[j], v, acc[0]);
                acc[1] = fmaf(k0[j - kw], v, acc[1]);
                acc[2] = fmaf(k0[j - 2 * kw], v, acc[2]);
                acc[3] = fmaf(k0[j - 3 * kw], v, acc[3]);
            }
        } else {
            for (int j = 0; j < kw; ++j) {
                const float v = row[j];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t - r >= 0 && t - r < kh) acc[r] = fmaf(k0[j - r * kw], v, acc[r]);
            }
        }
    }
}

// One 64 x 16 output tile of the batched correlation (wt_batch_filter2d_kernel, wt_batch64_filter2d_kernel: block
// (64, 4), grid z = the frame, each frame its own image - the border rules act at the frame's borders): the window
// staged in `tile` (dynamic LDS), then per output the chain of fma from 0, i outer, j inner.  !SKEW is the per-image
// tap loop (one LDS read per FMA); SKEW (float only) walks every staged row once for the four output rows of a
// thread - identical bits either way.
template <bool WRAP, bool SKEW, typename T>
__device__ __forceinline__ void wt_f2d_batch_tile(T *tile, const T *in, T *out, const Geo &g, int64_t fstride, const T *__restrict__ psf, int kh,
                                                  int kw, int ay, int ax)
{
    in += (int64_t)blockIdx.z * fstride;
    out += (int64_t)blockIdx.z * fstride;
    const int tw = WT_F2D_TW + kw - 1, th = WT_F2D_TH + kh - 1;
    const int x0 = blockIdx.x * WT_F2D_TW, ly0 = blockIdx.y * WT_F2D_TH;
    wt_f2d_stage<WRAP>(tile, in, g, x0, ly0, tw, th, ay, ax);
    __syncthreads();
    const int x = x0 + threadIdx.x;
    T acc[4] = {0, 0, 0, 0};
    if constexpr (SKEW) wt_f2d_taps_skewed(tile, tw, psf, kh, kw, acc);
    else wt_f2d_taps(tile, tw, psf, kw, kh, kw, acc);
    if (x < g.W) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ly = ly0 + threadIdx.y * 4 + r;
            if (ly < g.H) out[(int64_t)ly * g.P + x] = acc[r];
        }
    }
}

// elementwise binary ops of the RL iteration (watroo/utils.py:259,280-281,288)
enum { WT_OP_SUB = 0, WT_OP_ADD = 1, WT_OP_MUL = 2, WT_OP_DIV = 3, WT_OP_ADD_DIV = 4 };
__device__ __forceinline__ float4 wt_binary_point4(float4 u, float4 v, int op)
{
#pragma clang fp contract(off)
    const float x[4] = {u.x, u.y, u.z, u.w}, y[4] = {v.x, v.y, v.z, v.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        switch (op) {
            case WT_OP_SUB: o[k] = x[k] - y[k]; break;
            case WT_OP_ADD: o[k] = x[k] + y[k]; break;
            case WT_OP_MUL: o[k] = x[k] * y[k]; break;
            case WT_OP_DIV: o[k] = x[k] / y[k]; break;
            default: o[k] = (x[k] + y[k]) / y[k]; break;   // res += phi; res /= phi
        }
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

// ... and of the float64 engine (wt64_binary_kernel, wt_batch64_binary_kernel); op in wt64_binary's numbering:
// 0 add, 1 sub, 2 mul, 3 div, 4 (u + v) / v
__device__ __forceinline__ double wt64_binary_point(double u, double v, int op)
{
    return op == 0 ? u + v : op == 1 ? u - v : op == 2 ? u * v : op == 3 ? u / v : (u + v) / v;
}

// multiresolution-support update of one residual value (watroo/utils.py:263-276):
//   sig = significance(c);  hard: mrs = persistent ? max(mrs, sig) : sig ;  c *= mrs
//                           soft: mrs = persistent ? mrs * sig   : sig ;  c *= mrs ** inv_pow
__device__ __forceinline__ void wt_mrs_point(float &cc, float &mm, float nn, double tau, float tauf, int soft, int persistent, float inv_pow)
{
    const float sg = tau > 0.0 ? wt_sig(cc, tauf * nn, tau * (double)nn, soft) : 1.f;
    if (soft) {
        mm = persistent ? mm * sg : sg;
        cc = cc * powf(mm, inv_pow);
    } else {
        mm = persistent ? fmaxf(mm, sg) : sg;
        cc = cc * mm;
    }
}

// ... in float64 (wt64_mrs_kernel, wt_batch64_mrs_kernel): tt = the threshold of this sample (tau, or tau * its noise);
// the significance is the quotient form wt_sig64 (wt_sig64_inv differs by a rounding)
__device__ __forceinline__ void wt64_mrs_point(double &cc, double &mm, double tau, double tt, int soft, int persistent, double inv_pow)
{
    const double v = cc;
    double sg = 1.0;
    if (tau > 0.0) sg = wt_sig64(v, tt, soft);
    double m = mm;
    if (soft) {
        m = persistent ? m * sg : sg;
        cc = v * pow(m, inv_pow);
    } else {
        m = persistent ? fmax(m, sg) : sg;
        cc = v * m;
    }
    mm = m;
}
