// The float32 bilateral march: its helpers and the two kernels compiled from wt_bilateral_march.h - the image
// kernel (wt_transform.hip) and the batched one (wt_bilateral32_batch.hip).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wt_internal.h"
#include "wt_device.h"
#include "wt_stencil.h"

// ---------------------------------------------------------------------------------------------
// K10  bilateral (range-weighted) dilated convolution - watroo/wavelets.py:74-105
//   out = (k_c I + sum_t k_t e_t I_t) / (k_c + sum_t k_t e_t),
//   e_t = exp(-((I - I_t)^2) / var / 2)                        (numexpr expression, :97)
// Full K x K tap set (not separable): K*K-1 exponentials per pixel.  Per tap the weight is ONE v_exp_f32:
//   k_t * exp(-d^2/(2 var)) = 2^( d^2 * (-log2(e)/(2 var)) + log2(k_t) )
// with the per-pixel factor -log2(e)/(2 var) formed once (one division per pixel instead of
// one per tap).  fp32 rounding differs from the reference's exp()/divide sequence by a few
// ulp of the weight - inside the stated bilateral tolerance.
// Work decomposition is the chain march of K1: a thread owns a group of columns and one polyphase row
// chain, and keeps the K x K (dilated) neighbourhood rows in a register window that advances one
// chain step per iteration - every input row is fetched once per chain (K coalesced
// loads at x + j*d, L2-served) instead of once per output row, which is what makes the large
// dilations of wow() (d up to 1024, where a tile has no spatial reuse) HBM-neutral.
// (Until round 5 a four-pixel-per-thread form of this kernel was kept beside the two-pixel one as its bitwise
//  cross-check; it lost every timing since round 3 and went in round 6 - the cross-check is now the generic
//  load path of the kernel below, option "bilateral_paired" = 0.)
// ---------------------------------------------------------------------------------------------
// K10b  TWO pixels per thread (any dilation): a K x K float2 window, 92 VGPRs, 5 waves per SIMD.
//
// Round 6: the row that enters the window is fetched with raw BUFFER loads (SGPR descriptor of the row +
// one 32-bit lane offset per operand, 2 K four-byte loads per row) instead of per-lane branches between one
// 8-byte and two 4-byte flat loads.  The branches cost nothing by themselves, but loads inside divergent
// regions make the number of loads in flight path-dependent, so the compiler's wait-count pass fell back to
// `s_waitcnt vmcnt(0)` at the join - in front of the tap loop: the "prefetched" row was waited for BEFORE the
// 24 taps it was meant to hide behind, and the VALU idled whenever the four waves of a SIMD sat in that wait
// together (0.78 issue-busy).  With straight-line loads the wait is counted exactly and lands where the row is
// first used, one whole step later.  For the same reason the variance source is a template parameter (the
// plane form loads through the same descriptors), the LDS ring slots follow the unroll phase (immediate
// offsets), and only the border rules the launch code admits (0, 1) are compiled in.
// ---------------------------------------------------------------------------------------------
typedef unsigned int wt_su2 __attribute__((ext_vector_type(2)));
typedef float wt_sf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wt_store2(float *row, int x, int P, float2 v)
{
    const wt_sf2 t = {v.x, v.y};
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(wt_su2, t), wt_row_rsrc(row, P), (unsigned)x * 4u, 0, 0);
}
#define WT_BIL_NAME(base) base##_kernel
#define WT_BIL_PARAM(type, name) type name
#define WT_BIL_FRAME(name)
#include "wt_bilateral_march.h"
#undef WT_BIL_NAME
#undef WT_BIL_PARAM
#undef WT_BIL_FRAME
// (templates: instantiated only where a batched launch names them - wt_bilateral32_batch.hip; in-kernel variance only)
#define WT_BIL_NAME(base) base##_batch_kernel
#define WT_BIL_PARAM(type, name) WtFrameArgs<type> name##_frame0
#define WT_BIL_FRAME(name) const ChainArgs name = wt_frame_args<MODE_DECOMP>(name##_frame0)
#include "wt_bilateral_march.h"
#undef WT_BIL_NAME
#undef WT_BIL_PARAM
#undef WT_BIL_FRAME
