#!/usr/bin/env python3
"""(Z, Y, X) cubes: the cube engine (wavelets_amd.cubes: transform_cube / denoise_cube, one launch per scale)
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

  * --dtypes float64,int16: the float64 engine (wt64_decompose_cube against smooth64's three launches per scale, the
    rule WT_CUBE64_MIN_VOXELS_PER_STEP of csrc/wt_cubes64.h).  There the two forced device series are sampled in
    ALTERNATION too (fused, sequence, fused, ...), level by level, and next to them stand the serial steps of a
    workgroup, S + K - 1 (cube_geometry_t, csrc/wt_cubes_host.h), the voxels per serial step - the quantity of that
    rule - and the choice the rule made at every scale (read from the profile scope of the fused kernel).  The
    mid-size cubes of CASES_MID, where the two paths cross, are timed as well.  An integer cube is widened on the
    device into the same float64 planes, so its device rows are those of float64 and only its host-to-host rows are
    taken.

    python tools/bench_cubes.py [--samples 20] [--cases 64x512x512xL4xB3spline,...] [--dtypes float32]
                                [--out profiles/NAME.json]"""
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
# float64: between 0.13 and 2 M voxels, where the fused kernel and smooth64's three launches cross
CASES_MID = ["32x64x64xL5xTriangle", "64x64x64xL5xB3spline", "16x128x128xL4xB3spline", "32x128x128xL5xB3spline",
             "8x256x256xL3xB3spline", "64x128x128xL5xB3spline", "16x256x256xL4xB3spline", "16x256x256xL4xTriangle",
             "4x512x512xL3xB3spline", "32x256x256xL5xB3spline", "16x64x2048xL4xB3spline"]
WEIGHTS = [5, 3]
SCOPE64 = "wt_cube_scale_kernel64"


def serial_steps(shape, s, K, cus, xb=128, ty=8):
    """S + K - 1 of cube_geometry_t (csrc/wt_cubes_host.h) for scale s of a float64 cube on a device of `cus` CUs"""
    Z, Y, X = shape
    d = 1 << s
    ycls, zcls, ny, nz = min(d, Y), min(d, Z), -(-Y // d), -(-Z // d)
    have = -(-X // xb) * ycls * -(-ny // ty) * zcls
    chunks = max(1, min(nz, -(-cus * 8 // have)))
    return min(nz, max(-(-nz // chunks), 4 * (K - 1))) + K - 1


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


def device_alternate(ctx, run_a, run_b, n):
    """stats of n runs of run_a() and of run_b(), sampled a, b, a, b, ... between two HIP events, one warm-up each"""
    run_a()
    run_b()
    ctx.sync()
    ta, tb = [], []
    for _ in range(n):
        for run, t in ((run_a, ta), (run_b, tb)):
            ctx.timer_start()
            run()
            t.append(ctx.timer_stop())
    return stats(ta), stats(tb)


def forced(value):
    if value is None:
        os.environ.pop("WT_CUBE_FUSED", None)
    else:
        os.environ["WT_CUBE_FUSED"] = value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--cases", default=None)
    ap.add_argument("--dtypes", default="float32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    cus = ctx.device_info()["cus"]
    rows = []
    def cases_of(dt):
        return a.cases.split(",") if a.cases else CASES + (CASES_MID if dt != "float32" else [])

    for dt, item in ((dt, item) for dt in a.dtypes.split(",") for item in cases_of(dt)):
        z, y, x, lv, fam = item.split("x")
        shape, level, cls = (int(z), int(y), int(x)), int(lv[1:]), getattr(W, fam)
        f64 = dt != "float32"
        cube = np.random.default_rng(0).standard_normal(shape) * 3.0 + 10.0
        cube = np.rint(cube * 100).astype(dt) if np.dtype(dt).kind in "iu" else cube.astype(dt)
        assert W.cube64_eligible(cube, level, cls) if f64 else W.cube_eligible(cube, level, cls)
        rec = {"shape": list(shape), "family": fam, "level": level, "weights": WEIGHTS, "dtype": dt}
        forced(None)
        new, old = alternate(ctx, lambda: W.transform_cube(cube, level, cls).data,
                             lambda: W.AtrousTransform(cls)(cube, level).data, a.samples)
        rec["transform_host"] = {"cube": new, "existing": old, "existing_over_cube": old["median_ms"] / new["median_ms"]}
        new, old = alternate(ctx, lambda: W.denoise_cube(cube, WEIGHTS, cls), lambda: W.denoise(cube, WEIGHTS, cls), a.samples)
        rec["denoise_host"] = {"cube": new, "existing": old, "existing_over_cube": old["median_ms"] / new["median_ms"]}
        print(json.dumps({k: rec[k] for k in ("shape", "family", "level", "dtype", "transform_host", "denoise_host")}), flush=True)
        if f64 and dt != "float64":
            rows.append(rec)
            continue
        Z, Y, X = shape
        if f64:
            plan = L.Plan64(ctx, Z * Y, X, W.wavelets._taps_f64(cls(3), 3), level)
        else:
            plan = L.Plan(ctx, Z * Y, X, L.B3SPLINE if fam == "B3spline" else L.TRIANGLE, level)
        plan.upload(L.PLANE_INPUT, cube.reshape(Z * Y, X))
        dev = {}

        def run_forced(env, l):
            forced(env)
            plan.decompose_cube(L.PLANE_INPUT, l, Z)

        if f64:
            pairs = [device_alternate(ctx, lambda l=l: run_forced("1", l), lambda l=l: run_forced("0", l), a.samples)
                     for l in range(1, level + 1)]
            series = (("fused", [p[0] for p in pairs]), ("sequence", [p[1] for p in pairs]))
        else:
            series = tuple((tag, [device_ms(ctx, lambda l=l: run_forced(env, l), a.samples) for l in range(1, level + 1)])
                           for tag, env in (("fused", "1"), ("sequence", "0")))
        for tag, upto in series:
            dev[tag] = {"levels_1_to_L": upto,
                        "scale_ms": [upto[s]["median_ms"] - (upto[s - 1]["median_ms"] if s else 0.0) for s in range(level)]}
        forced(None)
        dev["rule"] = device_ms(ctx, lambda: plan.decompose_cube(L.PLANE_INPUT, level, Z), a.samples)
        dev["existing"] = device_ms(ctx, lambda: plan.decompose3d(L.PLANE_INPUT, level, Z), a.samples)
        dev["chain_steps"] = [-(-Z // (1 << s)) for s in range(level)]
        if f64:
            K = len(plan.family)
            dev["serial_steps"] = [serial_steps(shape, s, K, cus) for s in range(level)]
            dev["voxels_per_serial_step"] = [Z * Y * X / n for n in dev["serial_steps"]]
            ctx.profile(True)
            calls = []
            for l in range(1, level + 1):
                ctx.profile_reset()
                plan.decompose_cube(L.PLANE_INPUT, l, Z)
                calls.append(ctx.profile_entries().get(SCOPE64, (0, 0.0))[0])
            ctx.profile(False)
            dev["rule_fused"] = [bool(calls[s] - (calls[s - 1] if s else 0)) for s in range(level)]
        dev["sequence_over_fused"] = [q / f for f, q in zip(dev["fused"]["scale_ms"], dev["sequence"]["scale_ms"])]
        plan.close()
        rec["device"] = dev
        print(json.dumps({"shape": rec["shape"], "family": fam, "level": level, "dtype": dt, "device": dev}), flush=True)
        rows.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_cubes.py", "samples": a.samples, "compute_units": cus, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
