// The float64 pieces of wow (watroo/utils.py:174-217) that the per-frame kernels (wt_kernels_f64.h) and their batched
// forms (wt_batch64.hip: one frame per grid slice) share, as wt_reduce.h does in float32: one text for the update of
// a coefficient, the gamma blend of a pixel, a block's share of the {sum, sumsq, min, max} reduction and the plane
// sum, so that a frame of a batch performs the operations of the per-frame call in its order and gives its doubles.
#pragma once
#include <hip/hip_runtime.h>

#include "wt_math64.h"

typedef double wt_ntd2 __attribute__((ext_vector_type(2)));     // streaming 16-byte accesses

// wow per-scale update (watroo/utils.py:193-203): c <- c * significance; gamma += c;
// c <- c * factor / sqrt(clip(power, 1e-15)).  power / noise / gamma may be null.
// one coefficient of the update; `pw`: its local power (has_power) - shared by the pointwise kernel and the
// column pass that forms the power itself (wt64_wow_axis_kernel): identical bits
__device__ __forceinline__ double wt64_wow_point(double t, bool has_power, double pw, const double *noise, double *gamma, int64_t o,
                                                 double tau, int soft, double factor)
{
    if (tau > 0.0) {
        const double tt = noise ? tau * noise[o] : tau;
        t = t * wt_sig64(t, tt, soft);
    }
    if (gamma) gamma[o] = gamma[o] + t;
    double q = factor;
    if (has_power) {
        const double lp = pw <= 0.0 ? 1e-15 : pw;
        q = factor * wt_rsq64(lp);       // (as wt_wow_point<double> of wt_stencil.h: the fused update gives identical bits)
    }
    return t * q;
}

// gamma blend of one pixel (watroo/utils.py:212-217): (1 - h) recon + h clip((gamma - gmin) / range)^inv_gamma
__device__ __forceinline__ double wt64_gamma_point(double recon, double gamma, double gmin, double range, double inv_gamma, double h)
{
    double t = (gamma - gmin) / range;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    t = pow(t, inv_gamma);
    return (1.0 - h) * recon + h * t;
}

// {sum, sumsq, min, max} of the rows blockIdx.x, blockIdx.x + gridDim.x, ... of a plane -> o[4] (one 256-thread
// block): four 16-byte loads in flight per thread feeding independent accumulators (folded in a fixed order)
__device__ __forceinline__ void wt64_reduce_rows_block(const double *p, int nrows, int P, int W, double *o)
{
    constexpr int U = 4;
    double sa[U] = {0.0, 0.0, 0.0, 0.0}, sb[U] = {0.0, 0.0, 0.0, 0.0}, mn = INFINITY, mx = -INFINITY;
    const int X2 = (W + 1) / 2;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const double *row = p + (int64_t)r * P;
        for (int x2 = threadIdx.x; x2 < X2; x2 += 256 * U) {
            double2 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const double2 *>(row + 2 * min(x2 + 256 * u, X2 - 1));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int xx = x2 + 256 * u;
                const double e[2] = {v[u].x, v[u].y};
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (xx < X2 && 2 * xx + k < W) {
                        sa[u] += e[k];
                        sb[u] = fma(e[k], e[k], sb[u]);
                        mn = fmin(mn, e[k]);
                        mx = fmax(mx, e[k]);
                    }
            }
        }
    }
    double s = (sa[0] + sa[1]) + (sa[2] + sa[3]), s2 = (sb[0] + sb[1]) + (sb[2] + sb[3]);
    __shared__ double red[4][4];
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        s2 += __shfl_down(s2, off);
        mn = fmin(mn, __shfl_down(mn, off));
        mx = fmax(mx, __shfl_down(mx, off));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = s; red[wave][1] = s2; red[wave][2] = mn; red[wave][3] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { s += red[w][0]; s2 += red[w][1]; mn = fmin(mn, red[w][2]); mx = fmax(mx, red[w][3]); }
        o[0] = s; o[1] = s2; o[2] = mn; o[3] = mx;
    }
}

struct Sum64Args {
    const double *p[32];
    int n;
};
// np.sum(planes, axis=0) in plane order (watroo/utils.py:98) over n2 16-byte groups; a lane owns two samples
// As wt_plane_sum_kernel (round 5): one 16-byte group per thread - a large grid of short-lived waves keeps the
// most loads in flight for this n-reads-1-write stream - and streaming (nontemporal) accesses: planes read
// exactly once should not displace cache lines (8192^2, 12 planes: 1.33 -> 1.1x ms).
__device__ __forceinline__ void wt64_plane_sum_groups(const Sum64Args &a, double *dst, int64_t n2)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
        wt_ntd2 acc = __builtin_nontemporal_load(reinterpret_cast<const wt_ntd2 *>(a.p[0]) + i);
        for (int k = 1; k < a.n; ++k) {
            const wt_ntd2 v = __builtin_nontemporal_load(reinterpret_cast<const wt_ntd2 *>(a.p[k]) + i);
            acc = acc + v;
        }
        __builtin_nontemporal_store(acc, reinterpret_cast<wt_ntd2 *>(dst) + i);
    }
}
