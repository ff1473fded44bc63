#!/usr/bin/env python3
"""Float64 and integer stacks of frames through wow: the float64 batch (wow_stack on a BatchPlan64: one launch per
scale for all frames, one host round trip per reduction / median for all frames) against the per-frame loop on the
same frames, same process, same card.  One JSON line per shape and case
(16 x 1024^2 int16, 8 x 2048^2 float64, 2 x 4096^2 float64; B3, wow's default n_scales; cases: default,
denoise_coefficients=[5, 2], bilateral=1):
  * device-resident wow (transform + per-scale updates + sum): batched vs a loop over pre-acquired per-frame plans
    (HIP events around the whole stack; median / min / max of the samples, >= 20 after warm-up);
  * host to host through the numpy API: wow_stack vs a plain loop of wow() (wall clock; integer frames cross PCIe
    as they are on both sides).  The few-large-frames rule of wow64_eligible (WOW64_FEW_FRAMES) is switched off for
    the run: the tool measures the batch at every shape, the rule is derived from its numbers.
    python tools/bench_wow64_stack.py [samples]"""
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
from wavelets_amd.wavelets import Coefficients, _taps_f64  # noqa: E402

SHAPES = [(16, 1024, np.int16), (8, 2048, np.float64), (2, 4096, np.float64)]
CASES = {"default": dict(), "dc52": dict(denoise_coefficients=[5, 2]), "bilateral1": dict(bilateral=1)}


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


def frames(N, side, dtype):
    fr = np.random.default_rng(0).standard_normal((N, side, side))
    fr *= np.logspace(-1, 1, N)[:, None, None]
    if np.dtype(dtype).kind in "iu":
        fr = np.clip(np.round(fr * 300 + 3000), 0, 30000)
    return fr.astype(dtype)


def main():
    samples = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
    ctx = L.default_context()
    B.WOW64_FEW_FRAMES = 0
    for N, side, dtype in SHAPES:
        fr = frames(N, side, dtype)
        for case, kw in CASES.items():
            dc = kw.get("denoise_coefficients", [])
            bil = kw.get("bilateral")
            level = _wow_n_scales((side, side), W.B3spline, None, 0, dc)
            assert B.wow64_eligible(fr, level, W.B3spline, bil, [None] * N), "not a float64 batch case"
            bp = L.BatchPlan64(ctx, N, side, side, L.B3SPLINE, level)
            bp.upload(L.PLANE_INPUT, fr)
            plans = []
            for f in range(N):
                p = L.Plan64(ctx, side, side, _taps_f64(W.B3spline, 2), level)
                p.upload(L.PLANE_INPUT, fr[f])
                plans.append(p)
            rec = {"shape": [N, side, side], "dtype": np.dtype(dtype).name, "case": case, "n_scales": level}
            sb = _wow_sigma_bilateral(bil, level)

            def batched():
                if bil is None:
                    bp.decompose(N, L.PLANE_INPUT, level)
                else:
                    bp.decompose_bilateral(N, L.PLANE_INPUT, level, sb, False)
                B._wow_batch_device(bp, N, [None] * N, W.B3spline, level, [], True, list(dc), True, False, 3.2, None, None, 0, bil)

            def loop():
                for p in plans:
                    if bil is None:
                        p.decompose(L.PLANE_INPUT, level, L.FLAG_MEDIAN_HIST)          # (AtrousTransform._call_f64)
                    else:
                        p.decompose_bilateral(L.PLANE_INPUT, level, sb, False)
                    c = Coefficients(p, W.B3spline(2), sb, _dtype=np.float64)
                    _wow_device(c, level, [], True, list(dc), True, False, 3.2, None, None, 0)
                    c._plan = None                   # (the plan stays ours: not released to the pool)

            b = stats(timed(ctx, batched, samples))
            lp = stats(timed(ctx, loop, samples))
            rec["device_wow"] = {"batched": b, "loop": lp, "speedup": lp["median_ms"] / b["median_ms"],
                                 "speedup_range": [lp["min_ms"] / b["max_ms"], lp["max_ms"] / b["min_ms"]]}
            bp.close()
            for p in plans:
                p.close()
            hb = stats(wall(lambda: W.wow_stack(fr, **kw), 5))
            hl = stats(wall(lambda: [W.wow(f, **kw) for f in fr], 5))
            rec["host_to_host"] = {"wow_stack": hb, "wow_loop": hl, "speedup": hl["median_ms"] / hb["median_ms"]}
            L.trim_batches()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
