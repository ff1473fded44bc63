#!/usr/bin/env python3
"""(Z, Y, X) float32 cubes: the cube engine (wavelets_amd.cubes: transform_cube / denoise_cube, one launch per scale)
against the path before it, AtrousTransform(sf)(cube, L) and denoise(cube, [5, 3]) - Z + 2 launches per scale - both in
one process.

    B3spline 16x64x64 L3, 64x512x512 L3 and L4, 128x256x256 L4, 32x1024x1024 L3; Triangle 64x512x512 L4;
    short z chains, down to one step: B3spline 8x512x512 L4, 16x64x64 L5, Triangle 4x1024x1024 L3

  * host to host: transform_cube(cube, L).data against AtrousTransform(sf)(cube, L).data, and denoise_cube against
    denoise, sampled in ALTERNATION (engine, existing, engine, ...), wall clock around a drained stream, 20 samples
    per side (--samples): median / min / max / spread of either side and the ratio of the medians;
  * device, per scale: the cube already in HBM, Plan.decompose_cube at levels 1 .. L between two HIP events on the
    stream (Context.timer_start / timer_stop), the fused kernel forced at every scale (WT_CUBE_FUSED=1) and the old
    sequence forced at every scale (WT_CUBE_FUSED=0); the time of scale s is median(level s + 1) - median(level s).
    Next to it: the steps of a z chain at that scale, ceil(Z / d), the quantity of the host's per-scale rule
    (WT_CUBE_MIN_STEPS in csrc/wt_cubes.hip), and the whole transform under the rule.

    python tools/bench_cubes.py [--samples 20] [--cases 64x512x512xL4xB3spline,...] [--out profiles/NAME.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_signals import alternate, stats          # noqa: E402  (the sampling of the signal engine's tool)

CASES = ["16x64x64xL3xB3spline", "64x512x512xL3xB3spline", "64x512x512xL4xB3spline", "128x256x256xL4xB3spline",
         "32x1024x1024xL3xB3spline", "64x512x512xL4xTriangle",
         "8x512x512xL4xB3spline", "16x64x64xL5xB3spline", "4x1024x1024xL3xTriangle"]      # (short chains: down to one step)
WEIGHTS = [5, 3]


def device_ms(ctx, run, n):
    """stats of n runs of run() between two HIP events on the stream, after one warm-up run"""
    run()
    ctx.sync()
    t = []
    for _ in range(n):
        ctx.timer_start()
        run()
        t.append(ctx.timer_stop())
    return stats(t)


def forced(value):
    if value is None:
        os.environ.pop("WT_CUBE_FUSED", None)
    else:
        os.environ["WT_CUBE_FUSED"] = value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    rows = []
    for item in a.cases.split(","):
        z, y, x, lv, fam = item.split("x")
        shape, level, cls = (int(z), int(y), int(x)), int(lv[1:]), getattr(W, fam)
        cube = (np.random.default_rng(0).standard_normal(shape) * 3.0 + 10.0).astype(np.float32)
        assert W.cube_eligible(cube, level, cls)
        rec = {"shape": list(shape), "family": fam, "level": level, "weights": WEIGHTS}
        forced(None)
        new, old = alternate(ctx, lambda: W.transform_cube(cube, level, cls).data,
                             lambda: W.AtrousTransform(cls)(cube, level).data, a.samples)
        rec["transform_host"] = {"cube": new, "existing": old, "existing_over_cube": old["median_ms"] / new["median_ms"]}
        new, old = alternate(ctx, lambda: W.denoise_cube(cube, WEIGHTS, cls), lambda: W.denoise(cube, WEIGHTS, cls), a.samples)
        rec["denoise_host"] = {"cube": new, "existing": old, "existing_over_cube": old["median_ms"] / new["median_ms"]}
        print(json.dumps({k: rec[k] for k in ("shape", "family", "level", "transform_host", "denoise_host")}), flush=True)
        Z, Y, X = shape
        plan = L.Plan(ctx, Z * Y, X, L.B3SPLINE if fam == "B3spline" else L.TRIANGLE, level)
        plan.upload(L.PLANE_INPUT, cube.reshape(Z * Y, X))
        dev = {}
        for tag, env in (("fused", "1"), ("sequence", "0")):
            forced(env)
            upto = [device_ms(ctx, lambda l=l: plan.decompose_cube(L.PLANE_INPUT, l, Z), a.samples) for l in range(1, level + 1)]
            dev[tag] = {"levels_1_to_L": upto,
                        "scale_ms": [upto[s]["median_ms"] - (upto[s - 1]["median_ms"] if s else 0.0) for s in range(level)]}
        forced(None)
        dev["rule"] = device_ms(ctx, lambda: plan.decompose_cube(L.PLANE_INPUT, level, Z), a.samples)
        dev["existing"] = device_ms(ctx, lambda: plan.decompose3d(L.PLANE_INPUT, level, Z), a.samples)
        dev["chain_steps"] = [-(-Z // (1 << s)) for s in range(level)]
        dev["sequence_over_fused"] = [q / f for f, q in zip(dev["fused"]["scale_ms"], dev["sequence"]["scale_ms"])]
        plan.close()
        rec["device"] = dev
        print(json.dumps({"shape": rec["shape"], "family": fam, "level": level, "device": dev}), flush=True)
        rows.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_cubes.py", "samples": a.samples, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
