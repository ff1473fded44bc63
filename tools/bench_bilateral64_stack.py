#!/usr/bin/env python3
"""Float64 stacks with bilateral filtering: the batched float64 march (wt_batch64_decompose_bilateral) against the
per-frame float64 loop that transform_stack / denoise_stack ran for them before it existed.  B3, float64 N(1e4, 30)
frames, 64 x 512^2, 64 x 1024^2, 16 x 2048^2; HIP-event samples (median / min / max, spread = max / median - 1):
  * device-resident transform L = 6, bilateral = 1, and denoise([5, 3], bilateral = 1) (transform, MAD median,
    thresholds, sum) - batched: one BatchPlan64 over the stack; loop: one Plan64 per frame, the per-frame API's call
    sequence;
  * host to host: transform_stack(frames, 6, bilateral=1) and denoise_stack(frames, [5, 3], bilateral=1).

    python tools/bench_bilateral64_stack.py [--samples K] [--baseline-root DIR] [--out FILE]

--baseline-root DIR: a checkout of the commit to compare with (built): its numbers come from a child process that
imports the package from DIR (its transform_stack / denoise_stack; its per-frame loop device-resident), then this
tree's in this process - one RESULT JSON line with every shape, both sides, the ratios and the parent's spread
(--out FILE: also written there).  Without it: this tree only, both ways (--impl batched | loop | both)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

SHAPES = [(64, 512), (64, 1024), (16, 2048)]
LEVEL = 6
KEYS = ("transform_device", "denoise_53_device", "transform_stack_host", "denoise_stack_host")


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": med, "min_ms": ms[0], "max_ms": ms[-1], "spread": ms[-1] / med - 1.0, "samples": len(ms)}


def timed(ctx, fn, n, warm=2):
    for _ in range(warm):
        fn()
    ctx.sync()
    out = []
    for _ in range(n):
        ctx.timer_start()
        fn()
        out.append(ctx.timer_stop())
    return out


def run(impl, samples, shapes=SHAPES):
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    from wavelets_amd.wavelets import _noise_from_median
    ctx = L.default_context()
    se = W.B3spline(2).sigma_e(bilateral=1)
    taps = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
    sb = [1] * (LEVEL + 1)

    def taus_of(m):
        nz = _noise_from_median(m, se)
        return [float(5 * nz * se[0]), float(3 * nz * se[1])]

    res = []
    for N, side in shapes:
        fr = np.random.default_rng(0).standard_normal((N, side, side)) * 30.0 + 1e4
        rec = {"shape": [N, side, side], "impl": impl}
        if impl == "batched":
            bp = L.BatchPlan64(ctx, N, side, side, L.B3SPLINE, LEVEL)
            bp.upload(L.PLANE_INPUT, fr)

            def tr():
                bp.decompose_bilateral(N, L.PLANE_INPUT, LEVEL, sb)

            def den():
                bp.decompose_bilateral(N, L.PLANE_INPUT, 2, sb)
                bp.denoise_sum(N, 3, [taus_of(m) for m in bp.abs_median(N, 0)], [1, 1])
            closers = [bp]
        else:
            plans = []
            for f in range(N):
                p = L.Plan64(ctx, side, side, taps, LEVEL)
                p.upload(L.PLANE_INPUT, fr[f])
                plans.append(p)

            def tr():
                for p in plans:
                    p.decompose_bilateral(L.PLANE_INPUT, LEVEL, sb)

            def den():                     # utils.denoise(bilateral=1) on a float64 image: transform, then Coefficients._denoise_sum
                for p in plans:
                    p.decompose_bilateral(L.PLANE_INPUT, 2, sb)
                    p.denoise_sum(3, taus_of(p.abs_median(0)), [1, 1], True, write_back=False)
            closers = plans
        rec["transform_device"] = stats(timed(ctx, tr, samples))
        rec["denoise_53_device"] = stats(timed(ctx, den, samples))
        for c in closers:
            c.close()
        rec["transform_stack_host"] = stats(timed(ctx, lambda: W.transform_stack(fr, LEVEL, bilateral=1), samples, warm=1))
        rec["denoise_stack_host"] = stats(timed(ctx, lambda: W.denoise_stack(fr, [5, 3], bilateral=1), samples, warm=1))
        L.trim_batches()
        res.append(rec)
        print(json.dumps(rec), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--impl", choices=["batched", "loop", "both"], default="both")
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="N:side,N:side,... (default: the three stacks above)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    shapes = SHAPES if a.shapes is None else [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    sys.path.insert(0, os.path.abspath(a.root))
    if a.baseline_root is None:
        for impl in (["batched", "loop"] if a.impl == "both" else [a.impl]):
            run(impl, a.samples, shapes)
        return
    # the baseline commit in a child process of its own (its package, its library), then this tree
    cmd = [sys.executable, os.path.abspath(__file__), "--impl", "loop", "--samples", str(a.samples),
           "--root", os.path.abspath(a.baseline_root)]
    if a.shapes is not None:
        cmd += ["--shapes", a.shapes]
    child = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if child.returncode != 0:
        sys.stderr.write(child.stdout + child.stderr)
        sys.exit(child.returncode)
    base = [json.loads(ln) for ln in child.stdout.splitlines() if ln.startswith("{")]
    new = run("batched", a.samples, shapes)
    rows = []
    for b, n in zip(base, new):
        row = {"shape": n["shape"]}
        for k in KEYS:
            row[k] = {"parent": b[k], "new": n[k], "speedup": b[k]["median_ms"] / n[k]["median_ms"],
                      "new_over_parent_minus_1": n[k]["median_ms"] / b[k]["median_ms"] - 1.0,
                      "parent_spread": b[k]["spread"]}
        rows.append(row)
    line = json.dumps({"bench": "bilateral64_stack", "dtype": "float64", "family": "B3spline", "bilateral": 1, "level": LEVEL,
                       "samples": a.samples, "stacks": rows})
    print("RESULT " + line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
