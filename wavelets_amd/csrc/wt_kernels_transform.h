// Kernels of the transform unit (wt_transform.hip): the float32 bilateral march (wt_bilateral32.h) and the column
// pass of the run-time-tap filter.  (The chain / lattice / row kernels are wt_stencil.h, the fused passes
// wt_fused.h.)  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wt_internal.h"
#include "wt_device.h"
#include "wt_stencil.h"
#include "wt_kernels_common.h"

#include "wt_bilateral32.h"   // K10 / K10b: the bilateral march (image and batched kernel from one text)

__global__ __launch_bounds__(256) void wt_custom_cols_kernel(const float *tmp, const float *in, float *out_c,
                                                             float *out_w, Geo g, int d, CustomTaps t)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= g.W) return;
    const int hw = t.n / 2;
    for (int y = blockIdx.y; y < g.nrows; y += gridDim.y) {
        float acc = 0.f;
        for (int i = 0; i < t.n; ++i) {
            const int yy = wt_refl_b(g.row0 + y + (i - hw) * d, g.H, d, g.border) - g.row0;
            const float v = tmp[(int64_t)yy * g.P + x];
            acc = i == 0 ? t.k[0] * v : fmaf(t.k[i], v, acc);
        }
        const int64_t o = (int64_t)y * g.P + x;
        if (out_w) out_w[o] = in[o] - acc;
        out_c[o] = acc;
    }
}

