#!/usr/bin/env python3
"""wow on (Z, Y, X) cubes: wavelets_amd.cubes.wow_cube (the cube transform and wt_cube_wow_kernel, one launch per scale
each) against utils.wow (Z + 2 launches per scale for the transform, then a multiplication, Z + 2 launches of the 3-D
filter and the update for the whitening; float64: generic launches through cube-sized temporaries), both in one process.

    the cubes of tools/bench_cubes.py (CASES and CASES_MID), float32, float64 and int16; n_scales = the case's level,
    which wow caps by the cube's shortest side (ref utils.py:122-127): "level" in the output is the one that ran

  * host to host: wow_cube(cube, sf, n_scales=L) against wow(cube, sf, n_scales=L), sampled in ALTERNATION (cube,
    existing, cube, ...), wall clock around a drained stream, 20 samples per side (--samples): median / min / max /
    spread of either side and the ratio of the medians;
  * device (float32 and float64; an integer cube is widened into the same float64 planes): the cube already in HBM, the
    device-resident part of either call - Plan.decompose_cube + the per-scale loop of wow with wow_cube_scale, against
    Plan.decompose3d + the loop as wow runs it, then the plane sum - between two HIP events on the stream
    (Context.timer_start / timer_stop), sampled in alternation; the kernel scopes of one wow_cube call
    (Context.profile / profile_entries) are listed next to it;
  * device, per scale, at the case's own level (through Coefficients, which wow does not cap): Plan.wow_cube_scale on
    plane s between two HIP events, the fused kernel forced (WT_CUBE_FUSED=1) and the sequence it replaces forced
    (WT_CUBE_FUSED=0) in ALTERNATION, the plane restored from a copy before every sample.  Next to them the quantities
    of the per-scale rules (chain steps: WT_CUBE_MIN_STEPS, csrc/wt_cubes.hip; voxels per serial step:
    WT_CUBE64_MIN_VOXELS_PER_STEP, csrc/wt_cubes64.h) and the choice the rule made (read from the profile scope of the
    kernel).

    python tools/bench_wow_cube.py [--samples 20] [--cases 64x512x512xL4xB3spline,...] [--dtypes float32,float64,int16]
                                   [--out profiles/NAME.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_signals import alternate, stats                                         # noqa: E402
from tools.bench_cubes import CASES, CASES_MID, forced, serial_steps                     # noqa: E402

SCOPE = "wt_cube_wow_kernel"
TAU, FACTOR = 1.5, 0.75


def device_alternate(ctx, run_a, run_b, n):
    """stats of n runs of run_a() and of run_b() between two HIP events on the stream, sampled a, b, a, b, ..."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--cases", default=None)
    ap.add_argument("--dtypes", default="float32,float64,int16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    cus = ctx.device_info()["cus"]
    rows = []
    cases = a.cases.split(",") if a.cases else CASES + CASES_MID
    for dt, item in ((dt, item) for dt in a.dtypes.split(",") for item in cases):
        z, y, x, lv, fam = item.split("x")
        shape, asked, cls = (int(z), int(y), int(x)), int(lv[1:]), getattr(W, fam)
        f64 = dt != "float32"
        cube = np.random.default_rng(0).standard_normal(shape) * 3.0 + 10.0
        cube = np.rint(cube * 100).astype(dt) if np.dtype(dt).kind in "iu" else cube.astype(dt)
        assert W.wow_cube_eligible(cube, cls)
        forced(None)
        level = len(W.wow_cube(cube, cls, n_scales=asked)[1]) - 1
        rec = {"shape": list(shape), "family": fam, "level": level, "asked": asked, "dtype": dt}
        new, old = alternate(ctx, lambda: W.wow_cube(cube, cls, n_scales=asked), lambda: W.wow(cube, cls, n_scales=asked), a.samples)
        rec["host"] = {"cube": new, "existing": old, "existing_over_cube": old["median_ms"] / new["median_ms"]}
        print(json.dumps(rec), flush=True)
        if f64 and dt != "float64":
            rows.append(rec)
            continue
        Z, Y, X = shape
        from wavelets_amd.utils import _wow_device
        planes = W.transform_cube(cube, level, cls)       # (its plan keeps the cube in PLANE_INPUT)
        plan = planes._device()

        def resident(cube_kernel):
            if cube_kernel:
                plan.decompose_cube(L.PLANE_INPUT, level, Z)
            else:
                plan.decompose3d(L.PLANE_INPUT, level, Z)
            _wow_device(planes, level, [], True, [], True, False, 3.2, None, None, 0, cube_kernel=cube_kernel)

        new, old = device_alternate(ctx, lambda: resident(True), lambda: resident(False), a.samples)
        rec["device"] = {"cube": new, "existing": old, "existing_over_cube": old["median_ms"] / new["median_ms"]}
        ctx.profile(True)
        ctx.profile_reset()
        resident(True)
        ctx.sync()
        rec["device"]["cube_scopes"] = {k: [n, ms] for k, (n, ms) in ctx.profile_entries().items()}
        ctx.profile(False)
        ctx.profile_reset()
        del planes
        level = asked
        planes = W.transform_cube(cube, level, cls)
        plan = planes._device()
        K = len(cls.coefficients_1d)
        KEEP = L.PLANE_SCRATCH(8)
        per = {"fused": [], "sequence": [], "rule_fused": []}

        def run_forced(env, s):
            forced(env)
            plan.wow_cube_scale(s, s, Z, TAU, True, L.PLANE_NONE, FACTOR, L.PLANE_NONE)

        def restoring(run, s):
            def sample():
                ctx.timer_start()
                run()
                ms = ctx.timer_stop()
                plan.copy(KEEP, s)
                return ms
            return sample

        for s in range(level):
            plan.copy(s, KEEP)
            fused, seq = restoring(lambda: run_forced("1", s), s), restoring(lambda: run_forced("0", s), s)
            fused(), seq()
            ctx.sync()
            tf, ts = [], []
            for _ in range(a.samples):
                tf.append(fused())
                ts.append(seq())
            per["fused"].append(stats(tf))
            per["sequence"].append(stats(ts))
            forced(None)
            ctx.profile(True)
            ctx.profile_reset()
            plan.wow_cube_scale(s, s, Z, TAU, True, L.PLANE_NONE, FACTOR, L.PLANE_NONE)
            per["rule_fused"].append(bool(ctx.profile_entries().get(SCOPE, (0, 0.0))[0]))
            ctx.profile(False)
            ctx.profile_reset()
            plan.copy(KEEP, s)
        per["chain_steps"] = [-(-Z // (1 << s)) for s in range(level)]
        if f64:
            per["serial_steps"] = [serial_steps(shape, s, K, cus) for s in range(level)]
            per["voxels_per_serial_step"] = [Z * Y * X / n for n in per["serial_steps"]]
        per["sequence_over_fused"] = [q["median_ms"] / f["median_ms"] for f, q in zip(per["fused"], per["sequence"])]
        del planes
        rec["scales"] = per
        print(json.dumps({"shape": rec["shape"], "family": fam, "level": asked, "dtype": dt, "device": rec["device"], "scales": per}), flush=True)
        rows.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_wow_cube.py", "samples": a.samples, "compute_units": cus, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
