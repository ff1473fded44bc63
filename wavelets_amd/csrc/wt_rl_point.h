// Richardson-Lucy support shared by the per-image kernels (wt_kernels_apps.h) and the batched ones (wt_batch.hip):
// the PSF correlation's tile geometry, staging and border rules, and the pointwise arithmetic of the binary ops and
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
static inline size_t wt_f2d_lds_bytes(int kh, int kw)
{
    return (size_t)(WT_F2D_TW + kw - 1) * (WT_F2D_TH + kh - 1) * sizeof(float);
}
static inline bool wt_f2d_single_launch(int kh, int kw)
{
    return kh >= 1 && kw >= 1 && kw <= WT_F2D_MAX_KW && (int64_t)kh * kw <= WT_F2D_MAX_TAPS && wt_f2d_lds_bytes(kh, kw) <= WT_F2D_MAX_LDS;
}

// WRAP: periodic border (the circular convolution of the reference's rFFT path,
// watroo/utils.py:245-254,284), whole-image plans only; (ay, ax) = anchor of the correlation.
__device__ __forceinline__ int wt_wrap(int i, int n)
{
    const int m = i % n;
    return m < 0 ? m + n : m;
}

// the (WT_F2D_TW + kw - 1) x (WT_F2D_TH + kh - 1) input window of the output tile at (x0, local row ly0) -> LDS,
// by the 256 threads of the block
template <bool WRAP>
__device__ __forceinline__ void wt_f2d_stage(float *tile, const float *in, const Geo &g, int x0, int ly0, int tw, int th, int ay, int ax)
{
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < tw * th; i += 256) {
        const int ty = i / tw, tx = i - ty * tw;
        if (WRAP) {
            const float *row = in + (int64_t)wt_wrap(ly0 + ty - ay, g.H) * g.P;
            tile[i] = row[wt_wrap(x0 + tx - ax, g.W)];
        } else {
            const float *row = wt_row(in, g, g.row0 + ly0 + ty - ay);
            tile[i] = row[wt_refl(x0 + tx - ax, g.W)];
        }
    }
}

// the four output rows threadIdx.y * 4 + r of column threadIdx.x: acc[r] = fmaf(k[i][j], v, acc[r]), i outer, j inner
__device__ __forceinline__ void wt_f2d_taps(const float *tile, int tw, const float *psf, int psf_pitch, int kh, int kw, float acc[4])
{
    for (int i = 0; i < kh; ++i)
        for (int j = 0; j < kw; ++j) {
            const float k = psf[i * psf_pitch + j];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[r] = fmaf(k, tile[(threadIdx.y * 4 + r + i) * tw + threadIdx.x + j], acc[r]);
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
