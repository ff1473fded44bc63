// Translation unit of the batched float32 per-scale kernels (wt_batch): wt_stencil_march.h's batched chain,
// lattice and row kernels in the modes a batch runs - MODE_DECOMP (the single-scale passes of a schedule that
// have no fused kernel) and the wow update of wt_batch_wow_scale (MODE_WOW_PLAIN / MODE_WOW_GAMMA) and of
// wt_batch_wow_scale_map (MODE_WOW: the per-pixel noise map of the batch, with or without the gamma plane).  A unit of
// its own, so that wt_stencil32.hip compiles exactly the code it had before batches existed.  gfx950 only.
// Compiled with -DWT_TU_NAME=stencil32_batch.
#include <hip/hip_runtime.h>

#include "wt_internal.h"
#include "wt_stencil_launch.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

int wt32_stencil_batch_launch(const StencilCtx &sc, int mode, const ChainArgs &a, int s, const char *name, const WtFrames &fr)
{
    if (fr.n < 1 || fr.n > 65535) WT_FAIL("batched stencil: %d frames (1..65535 per launch)", fr.n);
    if (WT_IS_WOW(mode) && !fr.ftab) WT_FAIL("batched stencil: the wow modes need the per-frame {tau, factor} table");
    switch (mode) {
        case MODE_DECOMP: return wt_launch_stencil<float, MODE_DECOMP, true>(sc, a, s, name, fr);
        case MODE_WOW_PLAIN: return wt_launch_stencil<float, MODE_WOW_PLAIN, true>(sc, a, s, name, fr);
        case MODE_WOW_GAMMA: return wt_launch_stencil<float, MODE_WOW_GAMMA, true>(sc, a, s, name, fr);
        case MODE_WOW:
            if (!a.noise) WT_FAIL("batched stencil: MODE_WOW is the update with a noise map (plain / gamma otherwise)");
            return wt_launch_stencil<float, MODE_WOW, true>(sc, a, s, name, fr);
    }
    WT_FAIL("batched stencil: mode %d has no batched kernel (decomp, wow plain / gamma / map)", mode);
}
