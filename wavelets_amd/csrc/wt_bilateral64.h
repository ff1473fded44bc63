// K10 in float64: the bilateral (range-weighted) dilated convolution of watroo/wavelets.py:74-105 on
// double planes - what AtrousTransform(bilateral=...) / wow(bilateral=...) run for float64 and integer
// (FITS) images, which the reference computes in float64 (wavelets.py:297,319-320).
//
//   out = (k_c I + sum_t k_t e_t I_t) / (k_c + sum_t k_t e_t),   e_t = exp(-((I - I_t)^2) / var / 2)   (:97)
//
// The march of wt_bilateral2_kernel (wt_kernels_transform.h) with ONE pixel per thread: a thread owns a column and
// one chunk of one polyphase row chain and keeps the K x K dilated neighbourhood in a register window of
// K x K doubles (the float kernel's K x K float2), every input row is fetched once per chain through K
// coalesced 8-byte loads at x + j d.  Full K x K tap set (not separable): VALU-bound, K*K - 1 exponentials
// per pixel, and there is no double-precision exponential instruction - per tap
//   k_t exp(-delta^2 / (2 var)) = 2^(delta^2 * (-log2(e) / (2 var)) + log2(k_t))
// with the per-pixel factor formed once: u = fma(delta^2, s / 64, 1 + log2 k_t / 64) clamped to [0, 1] by the FMA's
// own output modifier, the range reduction by the 1.5 * 2^37 trick, 2^(j / 512) from a 512-entry table in LDS, a degree-3
// polynomial, the exponent added as an integer (wt_math64.h, table form).  12 double-precision operations (5 of them
// FMAs) + 4 integer operations + 1 LDS read per tap, ~305 double-precision operations per pixel with the variance
// and the two divisions.  The kernel is bound by its double-precision issue at the clock the chip holds under it
// (DESIGN.md section 3.6): the first version (a degree-10 polynomial, 12 FMAs per tap at the SAME instruction count)
// took 1.20 ms per scale of 8192^2, the 64-entry table 1.08, this one 1.05 (round 6: buffer loads, see below) -
// against 0.34 ms for the float kernel whose taps are packed-FP32 pairs around a hardware v_exp_f32.
// Differences from the reference's operation order (exp of a quotient; IEEE divisions) are a few ulp of
// the weight: the float64 parity bound of the tests is 1e-12 * max|input|.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wt_stencil.h"

template <int K>
__device__ __forceinline__ constexpr double wt_tap_log2_d(int i)
{
    // log2 of the taps: 1/4, 1/2 (Triangle); 1/16, 1/4, 3/8 (B3spline)
    if (K == 3) return i == 1 ? -1.0 : -2.0;
    return (i == 2) ? -1.4150374992788438 : ((i == 1 || i == 3) ? -2.0 : -4.0);
}

typedef unsigned int wt_du2 __attribute__((ext_vector_type(2)));
// 8-byte store of one pixel through a raw buffer descriptor of the row (see wt_storev)
__device__ __forceinline__ void wt_store1d(double *row, int x, int P, double v)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(wt_du2, v), wt_row_rsrc(row, P), (unsigned)x * 8u, 0, 0);
}

#define WT_BIL_NAME(base) base##_kernel
#define WT_BIL_PARAM(type, name) type name
#define WT_BIL_FRAME(name)
#include "wt_bilateral64_march.h"
#undef WT_BIL_NAME
#undef WT_BIL_PARAM
#undef WT_BIL_FRAME
// (templates: instantiated only where a batched launch names them - wt_bilateral64_batch.hip; in-kernel variance only)
#define WT_BIL_NAME(base) base##_batch_kernel
#define WT_BIL_PARAM(type, name) WtFrameArgs<type> name##_frame0
#define WT_BIL_FRAME(name) const ChainArgsT<double> name = wt_frame_args<MODE_DECOMP>(name##_frame0)
#include "wt_bilateral64_march.h"
#undef WT_BIL_NAME
#undef WT_BIL_PARAM
#undef WT_BIL_FRAME
