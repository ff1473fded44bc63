#!/usr/bin/env python3
"""compute_noise_weights with host frames (seed=None: np.random.normal on the host, one upload per trial) against
the seeded device route (seed=int: frames made on the GPU, trials batched) - B3 and Triangle, plain and
bilateral=1, n_scales 4, 6, 8, 10 at the reference's side 11 * 2**n_scales, with trial counts small enough for the
host route; host wall-clock per call (each call ends in the device round trip of its last reduction).  Plus the
device time of the fill kernel alone (HIP events; 4 frames of 4096^2 per launch) in Gpix/s and GB/s written.

    python tools/bench_noise_weights.py [--scales 4,6,8,10] [--samples K]          one JSON line"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRIALS = {4: 16, 6: 8, 8: 4, 10: 2}


def wall(fn, samples):
    fn()                                              # warm-up: plans, code objects
    out = []
    for _ in range(samples):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="4,6,8,10")
    ap.add_argument("--samples", type=int, default=3)
    args = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    res = {"tool": "bench_noise_weights", "device": ctx.device_info(), "samples": args.samples, "cases": []}
    for n_scales in [int(v) for v in args.scales.split(",")]:
        trials = TRIALS.get(n_scales, 2)
        for fam in (W.B3spline, W.Triangle):
            for bil in (None, 1):
                sf = fam(2)
                np.random.seed(1)
                host = wall(lambda: sf.compute_noise_weights(n_scales, trials, bil), args.samples)
                dev = wall(lambda: sf.compute_noise_weights(n_scales, trials, bil, seed=1), args.samples)
                res["cases"].append({"family": fam.__name__, "bilateral": bil, "n_scales": n_scales, "trials": trials,
                                     "side": 11 * 2 ** n_scales, "host_s": host, "seeded_s": dev, "speedup": host / dev})
                L.trim_batches()
    n, side = 4, 4096
    bp = L.BatchPlan(ctx, n, side, side, L.B3SPLINE, 0)
    ms = []
    for i in range(3 + 15):
        ctx.timer_start()
        bp.fill_normal(n, L.PLANE_INPUT, 1, i)
        ms.append(ctx.timer_stop())
    bp.close()
    ms = sorted(ms[3:])
    med = ms[len(ms) // 2]
    res["fill_kernel"] = {"frames": n, "side": side, "median_ms": med, "min_ms": ms[0], "max_ms": ms[-1],
                          "gpix_per_s": n * side * side / med / 1e6, "gb_written_per_s": 4 * n * side * side / med / 1e6}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
