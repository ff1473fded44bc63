// The {sum, sumsq, min, max} reduction shared by the per-frame kernels and their batched forms in wt_batch.hip
// (one frame per grid row), so that a frame of a batch folds its pixels in the order of the per-frame call and
// gives the same doubles: the streaming load, the fold of the partials (wt_reduce_final_kernel's body,
// wt_kernels_common.h) and - in wt_reduce_rows.h - the text of the first stage (wt_reduce_kernel).
#pragma once
#include <hip/hip_runtime.h>

typedef float wt_nt4 __attribute__((ext_vector_type(4)));
// streaming (non-temporal) 16-byte load: planes that are read exactly once should not displace
// L2 / Infinity-Cache lines (measured on MI355X, 7 reads + 1 write: 4.7 -> 6.1 TB/s)
__device__ __forceinline__ float4 wt_ldnt4(const float *p)
{
    const wt_nt4 v = __builtin_nontemporal_load(reinterpret_cast<const wt_nt4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// one 256-thread block: thread t folds partials t, t+256, ... in index order, then a fixed tree
__device__ __forceinline__ void wt_reduce_final_block(const double *partials, int nblocks, double *out)
{
    double s = 0.0, s2 = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        s += partials[b * 4 + 0];
        s2 += partials[b * 4 + 1];
        mn = fmin(mn, partials[b * 4 + 2]);
        mx = fmax(mx, partials[b * 4 + 3]);
    }
    __shared__ double red[256][4];
    red[threadIdx.x][0] = s; red[threadIdx.x][1] = s2; red[threadIdx.x][2] = mn; red[threadIdx.x][3] = mx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            red[threadIdx.x][0] += red[threadIdx.x + off][0];
            red[threadIdx.x][1] += red[threadIdx.x + off][1];
            red[threadIdx.x][2] = fmin(red[threadIdx.x][2], red[threadIdx.x + off][2]);
            red[threadIdx.x][3] = fmax(red[threadIdx.x][3], red[threadIdx.x + off][3]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = red[0][0]; out[1] = red[0][1]; out[2] = red[0][2]; out[3] = red[0][3];
    }
}
