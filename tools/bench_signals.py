#!/usr/bin/env python3
"""Stacks of 1-D signals: the signal engine (wt_signals: transform_signals / denoise_signals, one launch per chunk of
signals) against the per-signal loop - AtrousTransform(sf)(s, level) and denoise(s, weights) signal by signal, which is
what a user ran before the engine existed and what the parent commit runs.  B3spline, level 6:

    4096 x 4096 float32,  65536 x 512 float32,  256 x 8192 float32,  4096 x 4096 float64

  * host to host: transform_signals(stack, 6) against np.stack([AtrousTransform(B3spline)(s, 6).data for s in stack]),
    denoise_signals(stack, [5, 3]) against the loop of denoise(s, [5, 3]);
  * device-resident (input already in HBM, nothing crosses PCIe): SignalBatch.decompose over the stack against M times
    Plan.decompose / Plan64.decompose of a resident 1 x N plan under the 'mirror' border - the launches of the loop
    without its transfers.

Both sides are sampled in ALTERNATION (batch, loop, batch, loop, ...), wall clock around a drained stream, at least 20
samples per side (--samples); one JSON line per shape with median / min / max / spread of either side and the ratio of
the medians.  The loop of the large stacks takes seconds per sample: --loop-samples caps ITS samples below --samples
only when given (the default keeps both sides equal).

--sections names the measurements to take (transform_host, denoise_host, transform_device).

    python tools/bench_signals.py [--samples 20] [--loop-samples K] [--shapes 4096x4096xf32,...] [--sections ...] [--out profiles/NAME.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 4096, "f32"), (65536, 512, "f32"), (256, 8192, "f32"), (4096, 4096, "f64")]
LEVEL = 6
WEIGHTS = [5, 3]


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": med, "min_ms": ms[0], "max_ms": ms[-1], "spread": ms[-1] / med - 1.0, "samples": len(ms)}


def alternate(ctx, a, b, n, n_b=None):
    """n samples of a() and of b() in alternation (wall clock, the stream drained around every sample), after one
    warm-up call each; n_b < n: b is sampled in the first n_b rounds only"""
    n_b = n if n_b is None else n_b
    a()
    b()
    ctx.sync()
    ta, tb = [], []
    for i in range(n):
        for fn, acc, on in ((a, ta, True), (b, tb, i < n_b)):
            if not on:
                continue
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            acc.append((time.perf_counter() - t0) * 1e3)
    return stats(ta), stats(tb)


def pair(name, rec, batch, loop):
    rec[name] = {"batch": batch, "loop": loop, "loop_over_batch": loop["median_ms"] / batch["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--loop-samples", type=int, default=None)
    ap.add_argument("--shapes", default=",".join(f"{m}x{n}x{t}" for m, n, t in SHAPES))
    ap.add_argument("--sections", default="transform_host,denoise_host,transform_device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    taps = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
    rows = []
    for item in a.shapes.split(","):
        M, N, t = item.split("x")
        M, N, dtype = int(M), int(N), np.float32 if t == "f32" else np.float64
        sig = (np.random.default_rng(0).standard_normal((M, N)) * 3.0 + 10.0).astype(dtype)
        rec = {"shape": [M, N], "dtype": np.dtype(dtype).name, "family": "B3spline", "level": LEVEL, "weights": WEIGHTS}
        assert W.signals_eligible(sig, LEVEL)
        sections = a.sections.split(",")
        # host to host
        if "transform_host" in sections:
            pair("transform_host", rec, *alternate(
                ctx, lambda: W.transform_signals(sig, LEVEL),
                lambda: np.stack([W.AtrousTransform(W.B3spline)(s, LEVEL).data for s in sig]), a.samples, a.loop_samples))
            print(json.dumps({"shape": rec["shape"], "dtype": rec["dtype"], "transform_host": rec["transform_host"]}), flush=True)
        if "denoise_host" in sections:
            pair("denoise_host", rec, *alternate(
                ctx, lambda: W.denoise_signals(sig, WEIGHTS),
                lambda: np.stack([W.denoise(s, WEIGHTS) for s in sig]), a.samples, a.loop_samples))
            print(json.dumps({"shape": rec["shape"], "dtype": rec["dtype"], "denoise_host": rec["denoise_host"]}), flush=True)
        if "transform_device" not in sections:
            rows.append(rec)
            continue
        # device-resident
        L.trim_signals()
        sb = L.SignalBatch(ctx, M, N, L.B3SPLINE, LEVEL, dtype)
        sb.upload(sig)
        if dtype == np.float32:
            plan = L.Plan(ctx, 1, N, L.B3SPLINE, LEVEL)
        else:
            plan = L.Plan64(ctx, 1, N, taps, LEVEL)
        plan.upload(L.PLANE_INPUT, sig[:1])
        plan.set_border(2)

        def loop_device():
            for _ in range(M):
                plan.decompose(L.PLANE_INPUT, LEVEL, 0)
        pair("transform_device", rec, *alternate(ctx, lambda: sb.decompose(M, LEVEL), loop_device, a.samples, a.loop_samples))
        sb.close()
        plan.close()
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_signals.py", "samples": a.samples, "loop_samples": a.loop_samples, "sections": a.sections,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
