// Seeded standard-normal fill of a plane (wt_fill_normal on a wt_plan, wt_batch_fill_normal on a wt_batch): the frame
// np.random.normal(size=...).astype(np.float32) draws on the host in compute_noise_weights (watroo/wavelets.py:225),
// made where it is consumed.  Included by wt_apps.hip and wt_batch.hip; wavelets_amd/rng.py mirrors it on the host.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// constants), key = (seed low word, seed high word).  One call serves four horizontally adjacent pixels of one row of
// one frame: counter = (x >> 2, y, trial, 0) with x, y the LOGICAL pixel coordinates (global row of a strip, never a
// pitch offset) and trial = first_trial + frame index.  The layout is a contract: a pixel's value depends on
// (seed, trial, y, x) alone - not on the pitch, the chunk, the batch size or the kind of plan.
// Uniforms: u = ((bits >> 8) + 0.5) * 2^-24, exact in float32 and strictly inside (0, 1).  Normals: Box-Muller,
// (r0, r1) -> pixels x, x + 1 and (r2, r3) -> pixels x + 2, x + 3 as (sqrt(-2 ln u1) cos(2 pi u2), ... sin(2 pi u2)),
// with the accurate logf / sqrtf / sincosf: the kernel runs once per trial next to a multi-pass transform, and the
// tails are what a noise calibration is about.
#pragma once
#include <cstdint>

#include "wt_host.h"

struct WtPhilox4 {
    uint32_t v[4];
};

__device__ __forceinline__ WtPhilox4 wt_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return WtPhilox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ void wt_box_muller(uint32_t b1, uint32_t b2, float *za, float *zb)
{
    const float u1 = ((float)(b1 >> 8) + 0.5f) * 0x1p-24f;
    const float u2 = ((float)(b2 >> 8) + 0.5f) * 0x1p-24f;
    const float rad = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    *za = rad * cs;
    *zb = rad * sn;
}

// grid: x = groups of four pixels of a row (256 per block), y = rows, z = frames (both strided: the grid's y / z
// limits); each thread owns one group: one 16-byte store where the group is whole (rows start 16-byte aligned: P is a
// multiple of 4), the tail of a row whose width is not a multiple of 4 element by element.  Nothing is written
// beyond column W - 1, beyond row `rows` - 1 or into frames >= nf.
static __global__ __launch_bounds__(256) void wt_fill_normal_kernel(float *d, int W, int P, int rows, int y0, int nf, int64_t fstride,
                                                                    uint32_t k0, uint32_t k1, uint32_t trial0)
{
#pragma clang fp contract(off)
    const int x4 = blockIdx.x * 256 + threadIdx.x;
    if (4 * (int64_t)x4 >= W) return;
    const int x = 4 * x4;
    for (int f = blockIdx.z; f < nf; f += gridDim.z) {
        float *fp = d + (int64_t)f * fstride;
        for (int r = blockIdx.y; r < rows; r += gridDim.y) {
            const WtPhilox4 b = wt_philox4x32_10((uint32_t)x4, (uint32_t)(y0 + r), trial0 + (uint32_t)f, 0u, k0, k1);
            float z[4];
            wt_box_muller(b.v[0], b.v[1], &z[0], &z[1]);
            wt_box_muller(b.v[2], b.v[3], &z[2], &z[3]);
            float *q = fp + (int64_t)r * P + x;
            if (x + 3 < W) {
                *reinterpret_cast<float4 *>(q) = make_float4(z[0], z[1], z[2], z[3]);
            } else {
                q[0] = z[0];
                if (x + 1 < W) q[1] = z[1];
                if (x + 2 < W) q[2] = z[2];
            }
        }
    }
}

// `d`: local row 0 of frame 0 of a plane of `nf` frames, `fstride` floats apart, `rows` rows of pitch g.P each, the
// first of them the image's row g.row0 (one frame: a wt_plan; a strip fills its own rows of the image's field)
static inline int wt_launch_fill_normal(wt_ctx *c, float *d, const Geo &g, int rows, int nf, int64_t fstride, uint64_t seed, uint32_t trial0)
{
    const int W4 = (g.W + 3) / 4;
    const dim3 grid((unsigned)((W4 + 255) / 256), (unsigned)std::min(rows, 65535), (unsigned)std::min(nf, 65535));
    ProfScope ps(c, "wt_fill_normal_kernel");
    hipLaunchKernelGGL(wt_fill_normal_kernel, grid, dim3(256), 0, c->stream, d, g.W, g.P, rows, g.row0, nf, fstride, (uint32_t)seed,
                       (uint32_t)(seed >> 32), trial0);
    WT_HIP(hipGetLastError());
    return 0;
}
