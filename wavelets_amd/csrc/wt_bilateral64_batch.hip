// Translation unit of the batched float64 bilateral march (wt_batch64_decompose_bilateral): wt_bilateral64_march.h's
// batched kernel in the forms a batch runs - K = 5 / 3, the variance formed in the kernel.  A unit of its own, so
// that wt_stencil64.hip compiles exactly the code it had before batches existed.  gfx950 only.
// Compiled with -DWT_TU_NAME=bilateral64_batch (wt_math64.h: per-unit names of the polynomial and exp2 tables).
#include <hip/hip_runtime.h>

#include "wt_internal.h"
#include "wt_stencil_launch.h"
#include "wt_bilateral64.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

// One scale of the float64 bilateral transform for fr.n frames: the per-frame geometry of wt64_bilateral_launch
// (wt_stencil64.hip: one pixel per lane, 4 waves side by side on one chain item) with grid z = the frame.  A pixel's
// result does not depend on the chunking, so any geometry gives the image kernel's bits; the per-frame one is kept.
// a: in / out_c / out_w of frame 0, f1, f2.
int wt64_bilateral_batch_launch(const StencilCtx &sc, ChainArgsT<double> a, int s, const WtFrames &fr)
{
    if (fr.n < 1 || fr.n > 65535) WT_FAIL("batched float64 bilateral march: %d frames (1..65535 per launch)", fr.n);
    if (sc.g.border != 0) WT_FAIL("batched float64 bilateral march: the symmetric border of the whole frame only");
    if (s < 0 || s > 24) WT_FAIL("float64 bilateral scale %d out of range", s);
    if (!a.in || !a.out_c) WT_FAIL("batched float64 bilateral march: null plane");
    if (sc.g.row0 != 0 || sc.g.nrows != sc.g.H || fr.fstride < (int64_t)sc.g.H * sc.g.P)
        WT_FAIL("batched float64 bilateral march: whole frames at least H * P doubles apart");
    a.aux = nullptr;
    a.inline_var = 1;
    dim3 grid, block;
    WT_TRY(wt_march_geometry<double>(sc.g, s, a, grid, block, (sc.g.W + 63) / 64, 4));
    grid.z = (unsigned)fr.n;
    const WtFrameArgs<ChainArgsT<double>> fa{a, fr.fstride, nullptr};
    ProfScope ps(sc.ctx, "wt64_bilateral_batch_kernel", sc.stream);
    if (sc.family == WT_B3SPLINE) hipLaunchKernelGGL((wt64_bilateral_march_batch_kernel<5, true>), grid, block, 0, sc.stream, fa);
    else hipLaunchKernelGGL((wt64_bilateral_march_batch_kernel<3, true>), grid, block, 0, sc.stream, fa);
    WT_HIP(hipGetLastError());
    return 0;
}
