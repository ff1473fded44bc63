// Translation unit of the batched float32 bilateral march (wt_batch_decompose_bilateral): wt_bilateral_march.h's
// batched kernel in the forms a batch runs - K = 5 / 3, the variance formed in the kernel, paired and generic
// loads (option "bilateral_paired").  A unit of its own, so that wt_transform.hip compiles exactly the code it had
// before batches existed.  gfx950 only.  Compiled with -DWT_TU_NAME=bilateral32_batch.
#include <hip/hip_runtime.h>

#include "wt_internal.h"
#include "wt_bilateral32.h"
#include "wt_stencil_launch.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

// One scale of the bilateral transform for fr.n frames: the per-frame geometry of launch_bilateral (wt_transform.hip)
// with grid z = the frame.  A pixel's result does not depend on the chunking, so any geometry gives the image
// kernel's bits; the per-frame one is kept.  a: in / out_c / out_w of frame 0, f1, f2.
int wt32_bilateral_batch_launch(const StencilCtx &sc, ChainArgs a, int s, bool paired, const WtFrames &fr)
{
    if (fr.n < 1 || fr.n > 65535) WT_FAIL("batched bilateral march: %d frames (1..65535 per launch)", fr.n);
    if (sc.g.border != 0) WT_FAIL("batched bilateral march: the symmetric border of the whole frame only");
    if (s < 0 || s > 30) WT_FAIL("bilateral scale %d out of range", s);
    if (!a.in || !a.out_c) WT_FAIL("batched bilateral march: null plane");
    a.aux = nullptr;
    a.inline_var = 1;
    dim3 grid, block;
    // 4 waves side by side on one chain item (the LDS ring holds 256 threads)
    WT_TRY(wt_march_geometry<float>(sc.g, s, a, grid, block, ((sc.g.W + 1) / 2 + 63) / 64, 4));
    grid.z = (unsigned)fr.n;
    const WtFrameArgs<ChainArgs> fa{a, fr.fstride, nullptr};
    ProfScope ps(sc.ctx, "wt_bilateral2_batch_kernel", sc.stream);
#define WT_BIL2B(KK, PR) hipLaunchKernelGGL((wt_bilateral2_batch_kernel<KK, true, PR>), grid, block, 0, sc.stream, fa)
    if (sc.family == WT_B3SPLINE) { if (paired) WT_BIL2B(5, true); else WT_BIL2B(5, false); }
    else { if (paired) WT_BIL2B(3, true); else WT_BIL2B(3, false); }
#undef WT_BIL2B
    WT_HIP(hipGetLastError());
    return 0;
}
