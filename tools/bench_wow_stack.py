#!/usr/bin/env python3
"""Stacks of frames through wow: the batched engine (wow_stack: one launch per scale for all frames, one host round
trip per reduction / median for all frames) against the per-frame loop on the same frames.  One JSON line per shape
(64 x 512^2, 64 x 1024^2, 16 x 2048^2; B3, wow's default n_scales, denoise_coefficients=[5, 2]):
  * device-resident wow (transform + per-scale updates + sum): batched vs a loop over pre-acquired per-frame plans
    (HIP events around the whole stack; median / min / max of the samples);
  * host to host: wow_stack vs a plain loop of wow() (wall clock).
--bilateral: the same with bilateral=1 (the flagship flow wow(img, bilateral=1, denoise_coefficients=[5, 2])): the
batched bilateral march (wt_batch_decompose_bilateral) against per-frame wt_decompose_bilateral.
    python tools/bench_wow_stack.py [samples] [--bilateral]"""
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
from wavelets_amd.utils import _wow_device, _wow_n_scales, _wow_sigma_bilateral  # noqa: E402
from wavelets_amd.wavelets import Coefficients  # noqa: E402

SHAPES = [(64, 512), (64, 1024), (16, 2048)]
DC = [5, 2]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "samples": len(ms)}


def timed(ctx, fn, n, warm=3):
    for _ in range(warm):
        fn()
    ctx.sync()
    out = []
    for _ in range(n):
        ctx.timer_start()
        fn()
        out.append(ctx.timer_stop())
    return out


def wall(fn, n, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    argv = [a for a in sys.argv[1:] if a != "--bilateral"]
    bil = 1 if "--bilateral" in sys.argv[1:] else None
    samples = int(argv[0]) if argv else 15
    ctx = L.default_context()
    for N, side in SHAPES:
        level = _wow_n_scales((side, side), W.B3spline, None, 0, DC)
        fr = np.random.default_rng(0).standard_normal((N, side, side)).astype(np.float32)
        fr *= np.logspace(-1, 1, N).astype(np.float32)[:, None, None]
        bp = L.BatchPlan(ctx, N, side, side, L.B3SPLINE, level)
        bp.upload(L.PLANE_INPUT, fr)
        plans = []
        for f in range(N):
            p = L.Plan(ctx, side, side, L.B3SPLINE, level)
            p.upload(L.PLANE_INPUT, fr[f])
            plans.append(p)
        rec = {"shape": [N, side, side], "n_scales": level, "denoise_coefficients": DC, "bilateral": bil}
        sb = _wow_sigma_bilateral(bil, level)

        def batched():
            if bil is None:
                bp.decompose(N, L.PLANE_INPUT, level)
            else:
                bp.decompose_bilateral(N, L.PLANE_INPUT, level, sb, False)
            B._wow_batch_device(bp, N, [None] * N, W.B3spline, level, [], True, DC, True, False, 3.2, None, None, 0, bil)

        def loop():
            for p in plans:
                if bil is None:
                    p.decompose(L.PLANE_INPUT, level, L.FLAG_FUSED | L.FLAG_MEDIAN_HIST)
                else:
                    p.decompose_bilateral(L.PLANE_INPUT, level, sb, False, 0)     # (AtrousTransform._run)
                c = Coefficients(p, W.B3spline(2), sb)
                _wow_device(c, level, [], True, DC, True, False, 3.2, None, None, 0)
                c._plan = None                   # (the plan stays ours: not released to the pool)

        b = stats(timed(ctx, batched, samples))
        lp = stats(timed(ctx, loop, samples))
        rec["device_wow"] = {"batched": b, "loop": lp, "speedup": lp["median_ms"] / b["median_ms"],
                             "speedup_range": [lp["min_ms"] / b["max_ms"], lp["max_ms"] / b["min_ms"]]}
        bp.close()
        for p in plans:
            p.close()
        hb = stats(wall(lambda: W.wow_stack(fr, denoise_coefficients=DC, bilateral=bil), max(3, samples // 3)))
        hl = stats(wall(lambda: [W.wow(f, denoise_coefficients=DC, bilateral=bil) for f in fr], max(3, samples // 3)))
        rec["host_to_host"] = {"wow_stack": hb, "wow_loop": hl, "speedup": hl["median_ms"] / hb["median_ms"]}
        L.trim_batches()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
