#!/usr/bin/env python3
"""Stacks of float32 frames through richardson_lucy with one PSF: richardson_lucy_stack (the float32 batch: per
iteration the PSF correlation of all frames in one launch, the operands resident in the batch, one support update per
scale for all frames) against the per-frame loop on the same frames, same process, same card.  One JSON line per
shape and PSF (16 x 512^2, 16 x 1024^2, 8 x 2048^2; 9 x 9 and 25 x 25 PSFs; the default three coefficients, 10
iterations):
  * host to host through the numpy API: richardson_lucy_stack vs a plain loop of richardson_lucy() (wall clock, each
    call ends in its download; the two alternate sample by sample; median / min / max, >= 20 samples after warm-up)
    and whether the two results are the same bits at that shape;
  * device time of ONE batched correlation (wt_batch_filter2d, HIP events) against the N per-frame ones
    (wt_filter2d_ex on pre-acquired plans, which drains the stream and copies the PSF on every call), alternating.
The environment variable WT_BATCH_F2D_SKEW=1 makes the batched kernel use the row-skewed tap loop (one LDS read per
four FMAs) instead of the per-image one (one per FMA): run the tool once with and once without it to compare the two
tilings (`--correlation-only` skips the host-to-host part).
`--fft`: the same two measurements for fft=True with PSFs the per-frame call hands to the engine's FFT (16 x 512^2 with
33 x 33, 16 x 1024^2 with 65 x 65, 8 x 2048^2 with 129 x 129): richardson_lucy_stack(fft=True) on the batched FFT
products against the loop of richardson_lucy(fft=True), and ONE batched product of the whole stack (wt_batch_fft_apply,
six launches) against N wt_fft_apply calls on pre-acquired plans (HIP events).
`--dtype float64` / `--dtype int16`: stacks the reference computes in float64, on the float64 batch (rl64_eligible;
RLBatchPlan64) against the per-frame loop on Plan64s - 16 x 1024^2 with a 15 x 15 PSF, 4 x 2048^2 with 15 x 15 and
4 x 4096^2 with 31 x 31:
  * ONE batched correlation (wt_batch64_filter2d: the 64 x 16 tile staged in LDS as doubles) against the N per-frame
    ones (wt64_filter2d: one sample per thread, every tap a global load), HIP events, alternating;
  * device-resident: the 10 iterations of the chunk loop on a batch of all N frames against the same calls on N
    pre-acquired Plan64s (HIP events around all of it; the thresholds are constants);
  * host to host through the numpy API, as above (integer frames cross PCIe as they are on both sides).
    python tools/bench_rl_stack.py [samples] [--correlation-only] [--fft] [--dtype float64|int16]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wavelets_amd as W                      # noqa: E402
from wavelets_amd import _lib as L            # noqa: E402
from wavelets_amd import batch as B           # noqa: E402
from wavelets_amd import utils as U           # noqa: E402

SHAPES = [(16, 512), (16, 1024), (8, 2048)]
PSFS = [(9, 9), (25, 25)]
FFT_PSFS = {512: (33, 33), 1024: (65, 65), 2048: (129, 129)}
ITERATIONS, COEFFICIENTS = 10, (5, 2, 1)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "samples": len(ms)}


def alternate(fa, fb, n, clock, warm=2):
    """n samples of fa and of fb, taken in turns"""
    for _ in range(warm):
        fa()
        fb()
    a, b = [], []
    for _ in range(n):
        a.append(clock(fa))
        b.append(clock(fb))
    return a, b


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def frames(N, side):
    rng = np.random.default_rng(0)
    ridge = 4 * np.exp(-((np.arange(side) - 0.45 * side) ** 2) / (2 * (0.05 * side) ** 2))[None, :]
    fr = rng.uniform(0.5, 1.5, (N, side, side)) + ridge
    return (fr * np.logspace(-1, 1, N)[:, None, None]).astype(np.float32)


def make_psf(kh, kw):
    psf = (np.outer(np.hanning(kh + 2)[1:-1], np.hanning(kw + 2)[1:-1]) + 0.05) \
        * (1 + 0.3 * np.linspace(-1, 1, kh)[:, None] + 0.2 * np.linspace(-1, 1, kw)[None, :])
    return (psf / psf.sum()).astype(np.float32)


SHAPES64 = [(16, 1024, (15, 15)), (4, 2048, (15, 15)), (4, 4096, (31, 31))]


def frames64(N, side, dtype):
    fr = frames(N, side).astype(np.float64)
    return np.rint(fr * 300).astype(np.int16) if dtype == "int16" else fr


def rl_iterations(p, nf, psf_of, level, taus):
    """the iterations of richardson_lucy_stack's chunk loop on a batch (nf frames) or, nf None, of utils.richardson_lucy
    on a Plan64; psf_of(slot): what the correlation of that slot takes (a slot number / the kernel)"""
    DATA, PSI, PHI, RES, CONV = (L.PLANE_SCRATCH(i) for i in (6, 7, 8, 9, 10))
    a = () if nf is None else (nf,)
    for it in range(ITERATIONS):
        p.filter2d(*a, PSI, PHI, psf_of(0))
        p.binary(*a, "sub", DATA, PHI, RES)
        if nf is None:
            p.decompose(RES, level)
        else:
            p.decompose(nf, RES, level, L.FLAG_FUSED)
        for s in range(level):
            if nf is None:
                p.mrs_update(s, L.PLANE_SCRATCH(16 + s), taus[s], True, L.PLANE_NONE, True, 1.0 / (it + 1))
            else:
                p.mrs_update(nf, s, L.PLANE_SCRATCH(16 + s), [taus[s]] * nf, True, True, 1.0 / (it + 1))
        p.plane_sum(*a, 0, level + 1, RES)
        p.binary(*a, "add_div", RES, PHI, RES)
        p.filter2d(*a, RES, CONV, psf_of(1))
        p.binary(*a, "mul", PSI, CONV, PSI)


def main64(dtype, samples, corr_only):
    ctx = L.default_context()
    level = len(COEFFICIENTS)
    taps = U._taps_f64(W.B3spline(2), 2)
    for N, side, (kh, kw) in SHAPES64:
        fr = frames64(N, side, dtype)
        psf = make_psf(kh, kw).astype(np.float64)
        flipped = np.ascontiguousarray(psf[::-1, ::-1])
        assert B.rl64_eligible(fr, psf, level), "not a float64 batch case"
        rec = {"dtype": dtype, "shape": [N, side, side], "psf": [kh, kw], "iterations": ITERATIONS,
               "denoise_coefficients": list(COEFFICIENTS)}
        DATA, PSI, PHI = (L.PLANE_SCRATCH(i) for i in (6, 7, 8))
        bp = L.RLBatchPlan64(ctx, N, side, side, L.B3SPLINE, level)
        bp.set_psf(0, flipped)
        bp.set_psf(1, psf)
        bp.upload(DATA, fr)
        bp.upload(PSI, fr)
        plans = []
        for f in range(N):
            p = L.Plan64(ctx, side, side, taps, level)
            p.upload(DATA, fr[f].astype(np.float64))
            p.upload(PSI, fr[f].astype(np.float64))
            plans.append(p)

        def device(fn):
            ctx.timer_start()
            fn()
            return ctx.timer_stop()

        def loop_correlation():
            for p in plans:
                p.filter2d(PSI, PHI, flipped)

        tb, tl = alternate(lambda: bp.filter2d(N, PSI, PHI, 0), loop_correlation, samples, device)
        same = all(np.array_equal(bp.download(PHI, N)[f].view(np.uint64), plans[f].download(PHI).view(np.uint64)) for f in range(N))
        b, lp = stats(tb), stats(tl)
        rec["device_correlation"] = {"batched": b, "loop_of_per_frame_calls": lp, "speedup": lp["median_ms"] / b["median_ms"],
                                     "speedup_range": [lp["min_ms"] / b["max_ms"], lp["max_ms"] / b["min_ms"]],
                                     "batched_tfma_per_s": N * side * side * kh * kw / 1e9 / b["median_ms"],
                                     "loop_tfma_per_s": N * side * side * kh * kw / 1e9 / lp["median_ms"], "bit_identical": bool(same)}
        if not corr_only and dtype == "float64":        # (after the upload an integer stack is the same device work)
            taus = [0.05, 0.02, 0.01]
            for m in range(level):
                bp.fill(N, L.PLANE_SCRATCH(16 + m), 1.0)
                for p in plans:
                    p.fill(L.PLANE_SCRATCH(16 + m), 1.0)

            def reset():                                  # (the estimate of every sample starts from the data)
                bp.upload(PSI, fr)
                for f, p in enumerate(plans):
                    p.upload(PSI, fr[f])

            def batched_iterations():
                rl_iterations(bp, N, lambda slot: slot, level, taus)

            def loop_iterations():
                for p in plans:
                    rl_iterations(p, None, lambda slot: (flipped, psf)[slot], level, taus)

            n_res = max(20, samples // 2)
            tb, tl = [], []
            for i in range(n_res + 1):
                reset()
                t = device(batched_iterations)
                u = device(loop_iterations)
                if i:                                     # (the first pair warms up)
                    tb.append(t)
                    tl.append(u)
            rb, rl = stats(tb), stats(tl)
            same = all(np.array_equal(bp.download(PSI, N)[f].view(np.uint64), plans[f].download(PSI).view(np.uint64)) for f in range(N))
            rec["device_resident"] = {"batched": rb, "loop_of_per_frame_calls": rl, "speedup": rl["median_ms"] / rb["median_ms"],
                                      "speedup_range": [rl["min_ms"] / rb["max_ms"], rl["max_ms"] / rb["min_ms"]], "bit_identical": bool(same)}
        bp.close()
        for p in plans:
            p.close()
        if not corr_only:
            kw_rl = dict(iterations=ITERATIONS, denoise_coefficients=COEFFICIENTS)
            got = W.richardson_lucy_stack(fr, psf, **kw_rl)
            exp = np.stack([W.richardson_lucy(f, psf, **kw_rl) for f in fr])
            ts, tl = alternate(lambda: W.richardson_lucy_stack(fr, psf, **kw_rl),
                               lambda: [W.richardson_lucy(f, psf, **kw_rl) for f in fr], samples, wall, warm=1)
            hs, hl = stats(ts), stats(tl)
            rec["host_to_host"] = {"richardson_lucy_stack": hs, "richardson_lucy_loop": hl, "speedup": hl["median_ms"] / hs["median_ms"],
                                   "speedup_range": [hl["min_ms"] / hs["max_ms"], hl["max_ms"] / hs["min_ms"]],
                                   "stack_median_below_loop_min": hs["median_ms"] < hl["min_ms"],
                                   "bit_identical": bool(got.dtype == exp.dtype == np.float64 and np.array_equal(got.view(np.uint64), exp.view(np.uint64)))}
        L.trim_batches()
        print(json.dumps(rec), flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--dtype" in sys.argv:
        dtype = sys.argv[sys.argv.index("--dtype") + 1]
        if dtype not in ("float64", "int16"):
            sys.exit("--dtype float64 | int16")
        args.remove(dtype)
    else:
        dtype = None
    samples = max(20, int(args[0])) if args else 20
    corr_only = "--correlation-only" in sys.argv
    fft = "--fft" in sys.argv
    if dtype:
        return main64(dtype, samples, corr_only)
    ctx = L.default_context()
    tiling = "row-skewed tap loop" if os.environ.get("WT_BATCH_F2D_SKEW") else "per-image tap loop"
    for N, side in SHAPES:
        fr = frames(N, side)
        for kh, kw in ([FFT_PSFS[side]] if fft else PSFS):
            psf = make_psf(kh, kw)
            level = len(COEFFICIENTS)
            if fft:
                assert B.rl_fft_eligible(fr, psf, level) and not B.rl_eligible(fr, psf, level, fft=True), "not a batched FFT case"
            else:
                assert B.rl_eligible(fr, psf, level), "not a batch case"
            rec = {"shape": [N, side, side], "psf": [kh, kw], "iterations": ITERATIONS, "denoise_coefficients": list(COEFFICIENTS),
                   "batched_tiling": tiling}
            if fft:
                rec["batched_tiling"] = "fft"
            # ---- one batched correlation against N per-frame ones (device events)
            S, D, K = L.PLANE_SCRATCH(7), L.PLANE_SCRATCH(8), L.PLANE_SCRATCH(10)
            bp = L.BatchPlan(ctx, N, side, side, L.B3SPLINE, level)
            bp.upload(S, fr)
            kimg = U._rl_fft_kernel_image(psf, side, side) if fft else None
            if fft:
                bp.upload(K, kimg[None])
                bp.fft_spectrum(K)
            else:
                bp.set_psf(0, psf)
            plans = []
            for f in range(N):
                p = L.Plan(ctx, side, side, L.B3SPLINE, level)
                p.upload(S, fr[f])
                if fft:
                    p.upload(K, kimg)
                    p.fft_spectrum(K)
                plans.append(p)

            def device(fn):
                ctx.timer_start()
                fn()
                return ctx.timer_stop()

            def batched():
                if fft:
                    bp.fft_apply(N, S, D, False)
                else:
                    bp.filter2d(N, S, D, 0)

            def loop():
                for p in plans:
                    if fft:
                        p.fft_apply(S, D, False)
                    else:
                        p.filter2d(S, D, psf)

            tb, tl = alternate(batched, loop, samples, device)
            same = all(np.array_equal(bp.download(D, N)[f].view(np.uint32), plans[f].download(D).view(np.uint32)) for f in range(N))
            b, lp = stats(tb), stats(tl)
            gfma = N * side * side * kh * kw / 1e9
            rec["device_correlation"] = {"batched": b, "loop_of_per_frame_calls": lp, "speedup": lp["median_ms"] / b["median_ms"],
                                         "speedup_range": [lp["min_ms"] / b["max_ms"], lp["max_ms"] / b["min_ms"]],
                                         "batched_tfma_per_s": gfma / b["median_ms"], "bit_identical": bool(same)}
            if fft:      # (no tap count to rate: the six kernels move 8-byte complex elements; pixels per second instead)
                del rec["device_correlation"]["batched_tfma_per_s"]
                rec["device_correlation"]["batched_gpix_per_s"] = N * side * side / 1e6 / b["median_ms"]
            bp.close()
            for p in plans:
                p.close()
            # ---- host to host
            if not corr_only:
                kw_rl = dict(iterations=ITERATIONS, denoise_coefficients=COEFFICIENTS, fft=fft)
                got = W.richardson_lucy_stack(fr, psf, **kw_rl)
                exp = np.stack([W.richardson_lucy(f, psf, **kw_rl) for f in fr])
                ts, tl = alternate(lambda: W.richardson_lucy_stack(fr, psf, **kw_rl),
                                   lambda: [W.richardson_lucy(f, psf, **kw_rl) for f in fr], samples, wall, warm=1)
                hs, hl = stats(ts), stats(tl)
                rec["host_to_host"] = {"richardson_lucy_stack": hs, "richardson_lucy_loop": hl, "speedup": hl["median_ms"] / hs["median_ms"],
                                       "stack_median_below_loop_min": hs["median_ms"] < hl["min_ms"],
                                       "bit_identical": bool(np.array_equal(got.view(np.uint32), exp.view(np.uint32)))}
            L.trim_batches()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
