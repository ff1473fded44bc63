// float64 cube engine, host side: wt64_decompose_cube, the a-trous transform of a (Z, Y, X) float64 cube with one
// launch per scale (wt_cube_scale_kernel<double, K, SMALL_D>, wt_cubes_kernels.h) where wt64_decompose(depth) runs
// smooth64's three generic launches through two private temporaries.  The planes are those of wt64_decompose bit for
// bit, so the host chooses per scale between the fused kernel and smooth64.  wt64_wow_cube_scale is the whitening step
// of wow on such a cube in one launch (wt_cube_wow_kernel<double, ...>).  Part of the float64 unit (wt_f64.hip,
// behind wt_f64.h: smooth64, plan64_base and fused64_family are static there).  gfx950 only.
#pragma once
#include "wt_cubes_host.h"

// The per-scale rule.  A workgroup of the fused kernel marches S + K - 1 slices one after the other (S chain steps of
// its chunk and K - 1 warm-up slices, about 1.7 us each when nothing else hides the latency), while smooth64's three
// launches cost about 4 us each and then 25 ps per voxel.  tools/bench_cubes.py --dtypes float64 times every scale
// both ways (profiles/r26_cubes64.json, MI355X; table in DESIGN.md section 3.22): ordered by voxels per serial step,
// Z Y X / (S + K - 1), the 80 scales measured separate - smooth64 is as fast or faster, within the spread, at every
// scale up to 52 429 (16x64x64 d = 1: 0.013 against 0.035 ms; 64x128x128 d = 1: 0.039 against 0.045 ms), the fused
// kernel at every scale from 65 536 on (8x256x256 d = 2: 0.020 against 0.024 ms; 64x512x512 d = 1: 0.114 against
// 0.416 ms).  The chain steps
// alone, the float32 engine's WT_CUBE_MIN_STEPS, do not separate them: 16x64x64 loses at 16 steps where 8x512x512
// wins at one.
#define WT_CUBE64_MIN_VOXELS_PER_STEP 65536

static int cube64_scale_launch(wt_plan64 *p, int K, const double *in, double *oc, double *ow, int s, int depth, bool *done)
{
    CubeArgsT<double> a{};
    dim3 grid;
    *done = false;
    if (!cube_geometry_t<double>(p->g, p->ctx->num_cus, K, s, depth, a, grid)) return 0;
    const int forced = cube_forced();
    const int64_t voxels = (int64_t)a.Z * a.Y * a.W;
    if (forced == 0 || (forced < 0 && voxels < (int64_t)WT_CUBE64_MIN_VOXELS_PER_STEP * (a.S + K - 1))) return 0;
    a.in = in; a.out_c = oc; a.out_w = ow;
    const dim3 block(64, 4);
    const bool small = a.d < 2;          // d < PX: the three-group form of wt_hrow_filter
    ProfScope ps(p->ctx, "wt_cube_scale_kernel64");
    if (K == 5) {
        if (small) hipLaunchKernelGGL((wt_cube_scale_kernel<double, 5, true>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_scale_kernel<double, 5, false>), grid, block, 0, p->ctx->stream, a);
    } else {
        if (small) hipLaunchKernelGGL((wt_cube_scale_kernel<double, 3, true>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_scale_kernel<double, 3, false>), grid, block, 0, p->ctx->stream, a);
    }
    WT_HIP(hipGetLastError());
    *done = true;
    return 0;
}

/* atrous_standard on a float64 cube (watroo/wavelets.py:432,442 over the 3-D branch of convolution(), :46-64): the
 * plane contract of wt64_decompose(depth) - planes[0..level-1] <- detail, planes[level] <- smooth, src intact,
 * scratch 0/1 as ping-pong; a scale on the fused kernel touches no private temporary. */
extern "C" int wt64_decompose_cube(wt_plan64 *p, int src, int level, int depth)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt64_decompose_cube: null plan");
    if (p->g.border != 0) WT_FAIL("wt64_decompose_cube: the symmetric border only (plan border %d)", p->g.border);
    const int fam = fused64_family(p);
    if (fam < 0) WT_FAIL("wt64_decompose_cube: built-in scaling functions only (the plan holds %d user-defined taps)", p->ntaps);
    if (depth < 1 || p->g.H % depth) WT_FAIL("wt64_decompose_cube: plan height %d is not a multiple of depth %d", p->g.H, depth);
    if (level < 0 || level > p->max_level) WT_FAIL("wt64_decompose_cube: level %d exceeds plan max_level %d", level, p->max_level);
    if (src >= 0 && src <= level) WT_FAIL("wt64_decompose_cube: src plane %d is one of the output planes", src);
    if (src == WT_PLANE_SCRATCH(0) || src == WT_PLANE_SCRATCH(1)) WT_FAIL("wt64_decompose_cube: scratch planes 0/1 are used internally");
    double *in = nullptr;
    WT_TRY(plan64_base(p, src, &in));
    if (level == 0) {
        double *o = nullptr;
        WT_TRY(plan64_base(p, 0, &o));
        WT_HIP(hipMemcpyAsync(o, in, (size_t)p->g.nrows * p->g.P * 8, hipMemcpyDeviceToDevice, p->ctx->stream));
        return 0;
    }
    const int K = fam == WT_B3SPLINE ? 5 : 3;
    int cur = src;
    for (int s = 0; s < level; ++s) {
        const int nxt = (s == level - 1) ? level : WT_PLANE_SCRATCH(s & 1);
        double *ci = nullptr, *co = nullptr, *w = nullptr;
        WT_TRY(plan64_base(p, cur, &ci));
        WT_TRY(plan64_base(p, nxt, &co));
        WT_TRY(plan64_base(p, s, &w));
        bool done = false;
        WT_TRY(cube64_scale_launch(p, K, ci, co, w, s, depth, &done));
        if (!done) WT_TRY(smooth64(p, ci, co, w, s, 0, depth));
        cur = nxt;
    }
    return 0;
}

template <bool PLAIN>
static void cube64_wow_launch(wt_plan64 *p, int K, const CubeWowArgsT<double> &a, dim3 grid)
{
    const dim3 block(64, 4);
    const bool small = a.c.d < 2;        // d < PX: the three-group form of wt_hrow_filter
    if (K == 5) {
        if (small) hipLaunchKernelGGL((wt_cube_wow_kernel<double, 5, true, PLAIN>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_wow_kernel<double, 5, false, PLAIN>), grid, block, 0, p->ctx->stream, a);
    } else {
        if (small) hipLaunchKernelGGL((wt_cube_wow_kernel<double, 3, true, PLAIN>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_cube_wow_kernel<double, 3, false, PLAIN>), grid, block, 0, p->ctx->stream, a);
    }
}

/* One scale of the whitening loop of wow on a float64 cube (watroo/utils.py:193-203 over wavelets.py:46-64): plane <-
 * the update of wt64_wow_update with the local power conv_s(plane^2) of the 3-D filter, in one launch into the first
 * private temporary, whose pointer is then swapped with the plane's, as wt64_wow_scale does.  The per-scale rule is
 * that of wt64_decompose_cube; a scale it or the grid limit refuses runs wt64_binary(mul) -> scratch 6,
 * wt64_smooth(depth) -> scratch 7, wt64_wow_update: the same bits. */
extern "C" int wt64_wow_cube_scale(wt_plan64 *p, int plane, int s, int depth, double tau, int soft, int noise_plane, double factor,
                                   int gamma_plane)
{
    WtGuard guard_(ctx_of(p));
    if (!p) WT_FAIL("wt64_wow_cube_scale: null plan");
    if (p->g.border != 0) WT_FAIL("wt64_wow_cube_scale: the symmetric border only (plan border %d)", p->g.border);
    const int fam = fused64_family(p);
    if (fam < 0) WT_FAIL("wt64_wow_cube_scale: built-in scaling functions only (the plan holds %d user-defined taps)", p->ntaps);
    if (depth < 1 || p->g.H % depth) WT_FAIL("wt64_wow_cube_scale: plan height %d is not a multiple of depth %d", p->g.H, depth);
    if (plane < 0 || plane > p->max_level) WT_FAIL("wt64_wow_cube_scale: plane %d is not a coefficient plane", plane);
    if (s < 0 || s > 24) WT_FAIL("wt64_wow_cube_scale: scale %d out of range", s);
    const int sq = WT_PLANE_SCRATCH(6), pw = WT_PLANE_SCRATCH(7);
    for (int op : {noise_plane, gamma_plane}) {
        if (op == WT_PLANE_NONE) continue;
        if (op == plane || op == sq || op == pw)
            WT_FAIL("wt64_wow_cube_scale: operand plane %d aliases the plane or scratch 6 / 7, which are used internally", op);
    }
    if (noise_plane != WT_PLANE_NONE && noise_plane == gamma_plane) WT_FAIL("wt64_wow_cube_scale: the noise map and the gamma plane alias");
    double *c = nullptr, *nz = nullptr, *gm = nullptr, *spare = nullptr;
    WT_TRY(plan64_base(p, plane, &c));
    if (noise_plane != WT_PLANE_NONE) WT_TRY(plan64_base(p, noise_plane, &nz));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(plan64_base(p, gamma_plane, &gm));
    const int K = fam == WT_B3SPLINE ? 5 : 3;
    CubeWowArgsT<double> a{};
    dim3 grid;
    const int forced = cube_forced();
    bool fused = forced != 0 && cube_geometry_t<double>(p->g, p->ctx->num_cus, K, s, depth, a.c, grid);
    if (fused && forced < 0 && (int64_t)a.c.Z * a.c.Y * a.c.W < (int64_t)WT_CUBE64_MIN_VOXELS_PER_STEP * (a.c.S + K - 1)) fused = false;
    if (!fused) {
        WT_TRY(wt64_binary(p, 2, plane, plane, sq));
        WT_TRY(wt64_smooth(p, sq, pw, s, 0, depth));
        return wt64_wow_update(p, plane, pw, tau, soft, noise_plane, factor, gamma_plane);
    }
    WT_TRY(plan64_tmp(p, 0, &spare));
    a.c.in = c; a.c.out_c = spare; a.c.out_w = nullptr;
    a.noise = nz; a.gamma = gm; a.tau = tau; a.factor = factor; a.soft = soft;
    {
        ProfScope ps(p->ctx, "wt_cube_wow_kernel");
        if (!nz && !gm) cube64_wow_launch<true>(p, K, a, grid);
        else cube64_wow_launch<false>(p, K, a, grid);
        WT_HIP(hipGetLastError());
    }
    std::swap(p->coef[plane], p->tmp[0]);
    return 0;
}
