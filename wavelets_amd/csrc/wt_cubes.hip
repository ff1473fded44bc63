// libwatroo_hip.so - the float32 cube engine: wt_decompose_cube, the a-trous transform of a (Z, Y, X) cube with one
// launch per scale (wt_cube_scale_kernel, wt_cubes_kernels.h) where wt_decompose3d (wt_apps.hip) takes Z + 2.  The
// planes are those of wt_decompose3d bit for bit, so the host chooses per scale between the fused kernel and the old
// sequence (wt_smooth3d + wt_binary(SUB)).  wt_wow_cube_scale is the whitening step of wow on such a cube, one launch
// per scale (wt_cube_wow_kernel) where mul + wt_smooth3d + wt_wow_update take Z + 3.  gfx950 only.
#include <algorithm>
#include <cstdlib>

#include "wt_host.h"
#include "wt_cubes_host.h"
#include "wt_rl_point.h"      // WT_OP_SUB, WT_OP_MUL
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

template <bool PLAIN>
static void cube_wow_launch(wt_plan *p, const CubeWowArgsT<float> &a, dim3 grid)
{
    const dim3 block(64, 4);
    const bool small = a.c.d < 4;
    if (p->family == WT_B3SPLINE) {
        if (small) hipLaunchKernelGGL((wt_cube_wow_kernel<float, 5, true, PLAIN>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_wow_kernel<float, 5, false, PLAIN>), grid, block, 0, p->ctx->stream, a);
    } else {
        if (small) hipLaunchKernelGGL((wt_cube_wow_kernel<float, 3, true, PLAIN>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_wow_kernel<float, 3, false, PLAIN>), grid, block, 0, p->ctx->stream, a);
    }
}

// One scale of the whitening loop of wow on a cube (watroo/utils.py:193-203 over wavelets.py:46-64): plane <- the
// update of wt_wow_update with the local power conv_s(plane^2) of the 3-D filter, in one launch; the result is written
// to WT_PLANE_SCRATCH(3), whose pointer is then swapped with the plane's, as wt_wow_scale does.  The per-scale rule is
// that of wt_decompose_cube (WT_CUBE_MIN_STEPS, the WT_CUBE_FUSED switch); a scale it or the grid limit refuses runs
// wt_binary(MUL) -> scratch 6, wt_smooth3d -> scratch 7 (through scratch 15), wt_wow_update: the same bits.
extern "C" int wt_wow_cube_scale(wt_plan *p, int plane, int s, int depth, double tau, int soft, int noise_plane, float factor,
                                 int gamma_plane)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt_wow_cube_scale: null plan");
    if (p->nranks != 1) WT_FAIL("wt_wow_cube_scale: single-GPU plans only (%d ranks)", p->nranks);
    if (p->g.border != 0) WT_FAIL("wt_wow_cube_scale: the symmetric border only (plan border %d)", p->g.border);
    if (p->ntaps) WT_FAIL("wt_wow_cube_scale: built-in scaling functions only (the plan holds %d user-defined taps)", p->ntaps);
    if (depth < 1 || p->g.H % depth) WT_FAIL("wt_wow_cube_scale: plan height %d is not a multiple of depth %d", p->g.H, depth);
    if (plane < 0 || plane > p->max_level) WT_FAIL("wt_wow_cube_scale: plane %d is not a coefficient plane", plane);
    WT_TRY(check_scale(p, s, "wt_wow_cube_scale"));
    const int spare = WT_PLANE_SCRATCH(3), sq = WT_PLANE_SCRATCH(6), pw = WT_PLANE_SCRATCH(7), tmp = WT_PLANE_SCRATCH(15);
    for (int op : {noise_plane, gamma_plane}) {
        if (op == WT_PLANE_NONE) continue;
        if (op == plane || op == spare || op == sq || op == pw || op == tmp)
            WT_FAIL("wt_wow_cube_scale: operand plane %d aliases the plane or scratch 3 / 6 / 7 / 15, which are used internally", op);
    }
    if (noise_plane != WT_PLANE_NONE && noise_plane == gamma_plane) WT_FAIL("wt_wow_cube_scale: the noise map and the gamma plane alias");
    float *c = nullptr, *t = nullptr, *nz = nullptr, *gm = nullptr;
    WT_TRY(plane_base(p, plane, &c));
    if (noise_plane != WT_PLANE_NONE) WT_TRY(plane_base(p, noise_plane, &nz));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(plane_base(p, gamma_plane, &gm));
    CubeWowArgsT<float> a{};
    dim3 grid;
    const int forced = cube_forced();
    bool fused = forced != 0 && cube_geometry_t<float>(p->g, p->ctx->num_cus, family_taps(p->family), s, depth, a.c, grid);
    if (fused && forced < 0 && (a.c.Z + a.c.d - 1) / a.c.d < WT_CUBE_MIN_STEPS) fused = false;
    if (!fused) {
        WT_TRY(wt_binary(p, WT_OP_MUL, plane, plane, sq));
        WT_TRY(wt_smooth3d(p, sq, pw, s, depth));
        return wt_wow_update(p, plane, pw, tau, soft, noise_plane, factor, gamma_plane);
    }
    WT_TRY(plane_base(p, spare, &t));
    a.c.in = c; a.c.out_c = t; a.c.out_w = nullptr;
    a.noise = nz; a.gamma = gm; a.tau = tau; a.factor = factor; a.soft = soft;
    {
        ProfScope ps(p->ctx, "wt_cube_wow_kernel");
        if (!nz && !gm) cube_wow_launch<true>(p, a, grid);
        else cube_wow_launch<false>(p, a, grid);
        WT_HIP(hipGetLastError());
    }
    std::swap(p->coef[plane], p->scratch[3]);     // both are "first margin row" pointers (wt_wow_scale)
    return 0;
}
