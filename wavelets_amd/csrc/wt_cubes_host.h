// Host rules of the cube engines, one copy for both element types: the WT_CUBE_FUSED switch and the geometry of one
// fused scale (wt_cube_scale_kernel, wt_cubes_kernels.h).  Included by wt_cubes.hip (float32, wt_decompose_cube) and
// by the float64 unit (wt_cubes64.h, wt64_decompose_cube).
#pragma once
#include <algorithm>
#include <cstdlib>

#include "wt_cubes_kernels.h"

// WT_CUBE_FUSED=1 / 0 in the environment forces the fused kernel / the old sequence at every scale (tests, the bench);
// -1: the rule of the engine
static int cube_forced()
{
    const char *e = getenv("WT_CUBE_FUSED");     // read at every call: the tests switch it within one process
    return (e && *e) ? (atoi(e) != 0) : -1;
}

// geometry of one fused scale of a cube of `depth` slices held in a plane of geometry g, K taps, on a device of
// num_cus compute units; false: the grid does not fit (the old sequence serves the scale)
template <typename T>
static bool cube_geometry_t(const Geo &g, int num_cus, int K, int s, int depth, CubeArgsT<T> &a, dim3 &grid)
{
    constexpr int XB = 64 * WtVec<T>::PX;        // columns of a workgroup: 256 float, 128 double
    if (s > 24) return false;
    a.W = g.W; a.P = g.P;
    a.Z = depth; a.Y = g.H / depth;
    a.d = 1 << s;
    a.ycls = std::min(a.d, a.Y);
    a.zcls = std::min(a.d, a.Z);
    const int ny = (a.Y + a.d - 1) / a.d, nz = (a.Z + a.d - 1) / a.d;      // longest row class / z chain
    const int64_t gx = (a.W + XB - 1) / XB;
    const int64_t gy = (int64_t)a.ycls * ((ny + WT_CUBE_TY - 1) / WT_CUBE_TY);
    // chunks of the z chains: about two rounds of resident workgroups (4 per CU), chunks of at least 4 (K - 1) steps so
    // that the warm-up slices stay a fifth of the work
    const int64_t want = (int64_t)num_cus * 8;
    const int64_t have = gx * gy * a.zcls;
    int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(nz, (want + have - 1) / have));
    int S = (nz + chunks - 1) / chunks;
    S = std::min(nz, std::max(S, 4 * (K - 1)));
    chunks = (nz + S - 1) / S;
    a.S = S;
    const int64_t gz = (int64_t)a.zcls * chunks;
    if (gx > 0x7fffffff || gy > 65535 || gz > 65535) return false;
    a.nt = (int64_t)g.H * a.P * (int64_t)sizeof(T) >= ((int64_t)32 << 20);      // planes >> L2: streaming stores
    grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
    return true;
}
