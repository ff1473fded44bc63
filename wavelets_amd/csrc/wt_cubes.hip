// libwatroo_hip.so - the float32 cube engine: wt_decompose_cube, the a-trous transform of a (Z, Y, X) cube with one
// launch per scale (wt_cube_scale_kernel, wt_cubes_kernels.h) where wt_decompose3d (wt_apps.hip) takes Z + 2.  The
// planes are those of wt_decompose3d bit for bit, so the host chooses per scale between the fused kernel and the old
// sequence (wt_smooth3d + wt_binary(SUB)).  gfx950 only.
#include <algorithm>
#include <cstdlib>

#include "wt_host.h"
#include "wt_cubes_host.h"
#include "wt_rl_point.h"      // WT_OP_SUB
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

// The fused kernel marches polyphase chains along z: a chunk of S steps pays K - 1 warm-up slices, and a chain has
// only ceil(Z / d) steps.  Below WT_CUBE_MIN_STEPS steps per chain the scale goes to the old sequence.
// tools/bench_cubes.py times every scale both ways (profiles/r25_cubes.json, MI355X; table in DESIGN.md section 3.21):
// the fused kernel won at every (Z, d) measured, chains of ONE step included - 8x512x512 d = 8: 0.043 against
// 0.098 ms, 16x64x64 d = 16: 0.022 against 0.101 ms, 4x1024x1024 Triangle d = 4: 0.032 against 0.057 ms - so the
// constant is 1 and the old sequence serves only a scale whose grid does not fit (cube_geometry_t, wt_cubes_host.h,
// which also reads the WT_CUBE_FUSED switch).
#define WT_CUBE_MIN_STEPS 1

static int cube_scale_launch(wt_plan *p, const float *in, float *oc, float *ow, int s, int depth, bool *done)
{
    CubeArgs a{};
    dim3 grid;
    *done = false;
    if (!cube_geometry_t<float>(p->g, p->ctx->num_cus, family_taps(p->family), s, depth, a, grid)) return 0;
    const int forced = cube_forced();
    const int steps = (a.Z + a.d - 1) / a.d;
    if (forced == 0 || (forced < 0 && steps < WT_CUBE_MIN_STEPS)) return 0;
    a.in = in; a.out_c = oc; a.out_w = ow;
    const dim3 block(64, 4);
    const bool small = a.d < 4;
    ProfScope ps(p->ctx, "wt_cube_scale_kernel");
    if (p->family == WT_B3SPLINE) {
        if (small) hipLaunchKernelGGL((wt_cube_scale_kernel<float, 5, true>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_scale_kernel<float, 5, false>), grid, block, 0, p->ctx->stream, a);
    } else {
        if (small) hipLaunchKernelGGL((wt_cube_scale_kernel<float, 3, true>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_scale_kernel<float, 3, false>), grid, block, 0, p->ctx->stream, a);
    }
    WT_HIP(hipGetLastError());
    *done = true;
    return 0;
}

// atrous_standard on the cube (watroo/wavelets.py:432,442 over the 3-D branch of convolution(), :46-64): the plane
// contract of wt_decompose3d - planes[0..level-1] <- detail, planes[level] <- smooth, src intact, scratch 0/1 as
// ping-pong (and scratch 15 where a scale runs on the old sequence).
extern "C" int wt_decompose_cube(wt_plan *p, int src, int level, int depth)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_decompose_cube: null plan");
    if (p->nranks != 1) WT_FAIL("wt_decompose_cube: single-GPU plans only (%d ranks)", p->nranks);
    if (p->g.border != 0) WT_FAIL("wt_decompose_cube: the symmetric border only (plan border %d)", p->g.border);
    if (p->ntaps) WT_FAIL("wt_decompose_cube: built-in scaling functions only (the plan holds %d user-defined taps)", p->ntaps);
    if (depth < 1 || p->g.H % depth) WT_FAIL("wt_decompose_cube: plan height %d is not a multiple of depth %d", p->g.H, depth);
    if (level < 0 || level > p->max_level) WT_FAIL("wt_decompose_cube: level %d exceeds plan max_level %d", level, p->max_level);
    if (src >= 0 && src <= level) WT_FAIL("wt_decompose_cube: src plane %d is one of the output planes", src);
    if (level == 0) return wt_copy_plane(p, src, 0);
    int cur = src;
    for (int s = 0; s < level; ++s) {
        const int nxt = (s == level - 1) ? level : WT_PLANE_SCRATCH(s & 1);
        if (cur == nxt) WT_FAIL("wt_decompose_cube: scratch planes 0/1 are used internally");
        float *in = nullptr, *oc = nullptr, *ow = nullptr;
        WT_TRY(plane_base(p, cur, &in));
        WT_TRY(plane_base(p, nxt, &oc));
        WT_TRY(plane_base(p, s, &ow));
        bool done = false;
        WT_TRY(cube_scale_launch(p, in, oc, ow, s, depth, &done));
        if (!done) {
            WT_TRY(wt_smooth3d(p, cur, nxt, s, depth));
            WT_TRY(wt_binary(p, WT_OP_SUB, cur, nxt, s));        // w_s = c_s - c_{s+1}   (wavelets.py:442)
        }
        cur = nxt;
    }
    return 0;
}
