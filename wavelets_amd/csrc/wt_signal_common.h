// The device text the two 1-D engines share: the signal unit (wt_signals_kernels.h: one signal per workgroup) and the
// axis unit (wt_along_kernels.h: [n][ti] tiles).  The loops differ on purpose and stay in those headers; what is ONE
// expression in both - the filter, the point of the thresholded sum, the key, pair and median of the exact |w_0|
// median - stands here once.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wt_internal.h"
#include "wt_device.h"
#include "wt_math64.h"
#include "wt_stencil.h"      // wt_sig: the float32 significance of the per-signal thresholded sum

// LDS of one workgroup: the two ping-pong buffers of a signal (signal unit) or of a tile (axis unit).  A CHOSEN
// budget, not a measured optimum: 64 KiB lets two workgroups share the 160 KiB of a CU, and it admits N <= 8192 in
// float32 and N <= 4096 in float64.  Longer signals keep the per-signal route (wt_signals_ok).
#define WT_SIGNALS_LDS_BYTES 65536
#define WT_SIGNALS_THREADS 256

// c_{s+1}(x) from the K samples v[j] = c_s(R(x + (j - hw) d)), R = the 'mirror' rule (wt_refl_b, border 2).
// float: what the per-scale stencil kernels compute on a 1 x N image under that border (wt_stencil.h): the x taps
// of wt_hrow_filter - a product, then an FMA chain in tap order - and then WtVert::emit's y taps.  The K rows of the
// y pass all reflect onto the one row, so they hold the same row sum h; their products with the taps round, which is
// why the y pass is kept: a plain 1-D filter gives other bits.
template <int K>
__device__ __forceinline__ float wt_signal_smooth(const float (&v)[K])
{
#pragma clang fp contract(off)
    float h = wt_tap_s<K, float>(0) * v[0];
#pragma unroll
    for (int j = 1; j < K; ++j) h = fmaf(wt_tap_s<K, float>(j), v[j], h);
    float o = wt_tap_s<K, float>(0) * h;
#pragma unroll
    for (int j = 1; j < K; ++j) o = fmaf(wt_tap_s<K, float>(j), h, o);
    return o;
}
// double: what wt64_decompose takes for a signal (smooth64 in wt_f64.h: wt64_rows_kernel / wt64_rows2_kernel of
// wt_kernels_f64.h, no column pass for a 1 x N image under the 'mirror' border) - the row filter alone.
template <int K>
__device__ __forceinline__ double wt_signal_smooth(const double (&v)[K])
{
#pragma clang fp contract(off)
    double acc = wt_tap_s<K, double>(0) * v[0];
#pragma unroll
    for (int j = 1; j < K; ++j) acc = fma(wt_tap_s<K, double>(j), v[j], acc);
    return acc;
}

// the point of the thresholded sum on a sample of detail plane k < n_den, thresholded and weighted.
// float: the point text of wt_denoise_sum_kernel (wt_kernels_apps.h) - wt_sig, the weight rounded to float as
// wt_denoise_sum rounds it, contraction off; tau <= 0: the significance is one
__device__ __forceinline__ float wt_signal_point(float c, double t, double, double wgtd, int soft)
{
#pragma clang fp contract(off)
    const float tauf = (float)t, wgt = (float)wgtd, nn = 1.f;
    const float sgn = t > 0.0 ? wt_sig(c, tauf * nn, t * (double)nn, soft) : 1.f;
    return c * (wgt * sgn);
}
// double: the expressions of wt64_denoise_sum_kernel (wt_kernels_f64.h) without a noise plane - wt_sig64_inv with
// the host's 1 / tau
__device__ __forceinline__ double wt_signal_point(double v, double tau, double inv_tau, double wgt, int soft)
{
#pragma clang fp contract(off)
    double sg = 1.0;
    if (tau > 0.0) sg = wt_sig64_inv(v, tau, inv_tau, soft);
    return v * (wgt * sg);
}

// generalized_anscombe (watroo/wavelets.py:14-21) with alpha = 1, g = 0, sigma = 0 - what denoise(..., anscombe=True)
// runs around the transform of a signal (watroo/utils.py:93-94, 99-100) - as ONE point, so that the 1-D engines
// apply it where a sample is loaded and where the sum is stored.  The expressions are the per-signal call's device
// kernels', step by step, with the constants their host entries derive for these arguments:
// float: wt_anscombe_kernel (wt_kernels_apps.h) after launch_anscombe (wt_apps.hip) - forward c1 = (float)(3 / 8),
// c2 = 0, c3 = 0; inverse c1 = 0, c2 = 0, c3 = (float)(3 / 8); contraction off, as there.
// double: wt64_anscombe_kernel (wt_kernels_f64.h) - with alpha = 1 and g = sigma = 0 every product of that kernel is
// exact and every term it may contract into an FMA is zero, so its value does not depend on contraction:
// forward 2 sqrt(max(v + 3 / 8, 0)), inverse (v / 2)^2 - 3 / 8, each operation rounded once.
// Forward: samples <= -3 / 8 and -inf give 0, NaN stays NaN, +inf stays +inf; the square root is the correctly rounded
// one of those kernels, so the bits are also numpy's 2 * np.sqrt(x + 0.375).
__device__ __forceinline__ float wt_anscombe_fwd(float x)
{
#pragma clang fp contract(off)
    const float alpha = 1.f, c1 = (float)(3.0 * 1.0 * 1.0 / 8.0), c2 = (float)(0.0 * 0.0), c3 = (float)(1.0 * 0.0);
    float t = alpha * x;
    t = t + c1;
    t = t + c2;
    t = t - c3;
    t = t <= 0.f ? 0.f : t;
    return (2.f * sqrtf(t)) / alpha;
}
__device__ __forceinline__ float wt_anscombe_inv(float x)
{
#pragma clang fp contract(off)
    const float alpha = 1.f, c1 = (float)(1.0 * 0.0), c2 = (float)(0.0 * 0.0), c3 = (float)(3.0 * 1.0 / 8.0);
    float t = alpha * x;
    t = t / 2.f;
    t = t * t;
    t = t + c1;
    t = t - c2;
    t = t - c3;
    return t / alpha;
}
__device__ __forceinline__ double wt_anscombe_fwd(double v)
{
#pragma clang fp contract(off)
    const double alpha = 1.0, g = 0.0, sigma = 0.0;
    double dum = alpha * v + 3.0 * alpha * alpha / 8.0 + sigma * sigma - alpha * g;
    if (dum <= 0.0) dum = 0.0;
    return 2.0 * sqrt(dum) / alpha;
}
__device__ __forceinline__ double wt_anscombe_inv(double v)
{
#pragma clang fp contract(off)
    const double alpha = 1.0, g = 0.0, sigma = 0.0;
    const double h = alpha * v / 2.0;
    return (h * h + alpha * g - sigma * sigma - 3.0 * alpha / 8.0) / alpha;
}
// a 16-byte group of samples, point by point
__device__ __forceinline__ float4 wt_anscombe_fwd(float4 v) { return make_float4(wt_anscombe_fwd(v.x), wt_anscombe_fwd(v.y), wt_anscombe_fwd(v.z), wt_anscombe_fwd(v.w)); }
__device__ __forceinline__ double2 wt_anscombe_fwd(double2 v) { return make_double2(wt_anscombe_fwd(v.x), wt_anscombe_fwd(v.y)); }

// The exact np.median(np.abs(w_0)): the magnitudes' bit patterns order like the values, so a bitonic network sorts
// them as unsigned keys (the tail of the power of two filled with all-ones keys).
template <typename T>
struct WtSignalKey { typedef typename std::conditional<sizeof(T) == 8, unsigned long long, uint32_t>::type U; };
// |x| as an ordered key
template <typename T>
__device__ __forceinline__ typename WtSignalKey<T>::U wt_signal_abs_key(T x)
{
    typedef typename WtSignalKey<T>::U U;
    U u;
    memcpy(&u, &x, sizeof(T));
    return u & ~((U)1 << (8 * sizeof(T) - 1));
}
// compare-exchange t of a stage of distance j works on the pair (lo, lo + j): lo.  (A macro: an inline function is
// simplified before it meets the caller's loop, and one scalar instruction of the median kernels comes out different.)
#define WT_SIGNAL_PAIR_LO(t, j) ((((t) & ~((j) - 1)) << 1) | ((t) & ((j) - 1)))
// the median of a signal of N samples from its sorted keys: key[at] is the key (N - 1) / 2, key[next] the one after
// it - that key for an odd N, and the mean of the two, in T, for an even N
template <typename T>
__device__ __forceinline__ T wt_signal_median(const typename WtSignalKey<T>::U *key, int at, int next, int N)
{
    typedef typename WtSignalKey<T>::U U;
    const U ulo = key[at], uhi = (N & 1) ? ulo : key[next];
    T lo, hi;
    memcpy(&lo, &ulo, sizeof(T));
    memcpy(&hi, &uhi, sizeof(T));
    return (N & 1) ? lo : (lo + hi) / (T)2;
}
