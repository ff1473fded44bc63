#!/usr/bin/env python3
"""Stacks of small / mid-size frames: the batched engine (wt_batch, one launch per fused pass for all frames)
against the per-frame loop on the same frames.  One JSON line per shape (64 x 512^2, 64 x 1024^2, 16 x 2048^2,
B3, L = 6):
  * device-resident decompose_sum: batched vs a loop over pre-acquired per-frame plans (HIP events around the
    whole stack; median / min / max of the samples), Gpix/s and the fraction of 8 TB/s at 64 B/pixel;
  * device-resident denoise([5, 3]) (MAD median, thresholds, sum), both ways;
  * host to host: denoise_stack vs denoise_many(lanes=3) vs a plain loop of denoise().
    python tools/bench_batch.py [samples]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wavelets_amd as W                      # noqa: E402
from wavelets_amd import _lib as L            # noqa: E402
from wavelets_amd.wavelets import _noise_from_median  # noqa: E402

SHAPES = [(64, 512), (64, 1024), (16, 2048)]
LEVEL = 6
PEAK = 8e12                                   # B/s
BPP = 64                                      # bytes per pixel of decompose_sum L = 6 (2 fused passes)


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


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    ctx = L.default_context()
    sf = W.B3spline(2)
    for N, side in SHAPES:
        rng = np.random.default_rng(0)
        fr = rng.standard_normal((N, side, side)).astype(np.float32)
        npx = N * side * side
        bp = L.BatchPlan(ctx, N, side, side, L.B3SPLINE, LEVEL)
        bp.upload(L.PLANE_INPUT, fr)
        plans = []
        for f in range(N):
            p = L.Plan(ctx, side, side, L.B3SPLINE, LEVEL)
            p.upload(L.PLANE_INPUT, fr[f])
            plans.append(p)
        rec = {"shape": [N, side, side], "level": LEVEL}
        b = stats(timed(ctx, lambda: bp.decompose_sum(N, L.PLANE_INPUT, LEVEL), samples))
        lp = stats(timed(ctx, lambda: [p.decompose_sum(L.PLANE_INPUT, LEVEL) for p in plans], samples))
        for name, s in (("batched", b), ("loop", lp)):
            s["gpix_s"] = npx / (s["median_ms"] * 1e-3) / 1e9
            s["roofline"] = npx * BPP / (s["median_ms"] * 1e-3) / PEAK
        rec["decompose_sum"] = {"batched": b, "loop": lp, "speedup": lp["median_ms"] / b["median_ms"]}
        # device-resident denoise([5, 3]): passes, one median per frame, thresholds + sum, remaining passes
        sched = L.schedule(L.B3SPLINE, 2, True)

        def den_batched():
            bp.decompose(N, L.PLANE_INPUT, 2)
            med = bp.abs_median(N, 0)
            taus = [[float(5 * _noise_from_median(m, sf.sigma_e()) * sf.sigma_e()[0]),
                     float(3 * _noise_from_median(m, sf.sigma_e()) * sf.sigma_e()[1])] for m in med]
            bp.denoise_sum(N, 3, taus, [1, 1])

        def den_loop():
            for p in plans:
                p.decompose(L.PLANE_INPUT, 2, L.FLAG_FUSED | L.FLAG_MEDIAN_HIST)
                nz = _noise_from_median(p.abs_median(0), sf.sigma_e())
                p.denoise_sum(3, [float(5 * nz * sf.sigma_e()[0]), float(3 * nz * sf.sigma_e()[1])], [1, 1])

        assert len(sched) == 1
        db = stats(timed(ctx, den_batched, samples))
        dl = stats(timed(ctx, den_loop, samples))
        rec["denoise_53_device"] = {"batched": db, "loop": dl, "speedup": dl["median_ms"] / db["median_ms"]}
        # host to host
        def wall(fn, n=5):
            fn()
            t = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            return stats(t)
        rec["denoise_53_host"] = {"denoise_stack": wall(lambda: W.denoise_stack(fr, [5, 3])),
                                  "denoise_many_lanes3": wall(lambda: W.denoise_many(list(fr), [5, 3], lanes=3)),
                                  "loop": wall(lambda: [W.denoise(f, [5, 3]) for f in fr])}
        for p in plans:
            p.close()
        bp.close()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
