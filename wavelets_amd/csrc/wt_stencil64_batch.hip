// Translation unit of the batched float64 per-scale kernels (wt_batch64): wt_stencil_march.h's batched chain,
// lattice and row kernels instantiated for double in the modes a float64 batch runs - MODE_DECOMP (the single-scale
// passes of a schedule that have no fused kernel: wow asks for 9 scales at 2048^2, 10 at 4096^2) and the wow update of
// wt_batch64_wow_scale (MODE_WOW_PLAIN / MODE_WOW_GAMMA) and of wt_batch64_wow_scale_map (MODE_WOW: the per-pixel
// noise map of the batch, with or without the gamma plane).  The twin of wt_stencil32_batch.hip, and a unit of its
// own, so that wt_stencil64.hip compiles exactly the code it had before.  gfx950 only.
// Compiled with -DWT_TU_NAME=stencil64_batch (wt_math64.h: per-unit names of the polynomial tables).
#include <hip/hip_runtime.h>

#include "wt_internal.h"
#include "wt_stencil_launch.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

int wt64_stencil_batch_launch(const StencilCtx &sc, int mode, const ChainArgsT<double> &a, int s, const char *name, const WtFrames &fr)
{
    if (s < 0 || s > 24) WT_FAIL("batched float64 stencil: scale %d out of range", s);
    if (fr.n < 1 || fr.n > 65535) WT_FAIL("batched float64 stencil: %d frames (1..65535 per launch)", fr.n);
    if (WT_IS_WOW(mode) && !fr.ftab) WT_FAIL("batched float64 stencil: the wow modes need the per-frame {tau, factor} table");
    switch (mode) {
        case MODE_DECOMP: return wt_launch_stencil<double, MODE_DECOMP, true>(sc, a, s, name, fr);
        case MODE_WOW_PLAIN: return wt_launch_stencil<double, MODE_WOW_PLAIN, true>(sc, a, s, name, fr);
        case MODE_WOW_GAMMA: return wt_launch_stencil<double, MODE_WOW_GAMMA, true>(sc, a, s, name, fr);
        case MODE_WOW:
            if (!a.noise) WT_FAIL("batched float64 stencil: MODE_WOW is the update with a noise map (plain / gamma otherwise)");
            return wt_launch_stencil<double, MODE_WOW, true>(sc, a, s, name, fr);
    }
    WT_FAIL("batched float64 stencil: mode %d has no batched kernel (decomp, wow plain / gamma / map)", mode);
}
