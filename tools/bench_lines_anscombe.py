#!/usr/bin/env python3
"""anscombe=True in the two 1-D engines (denoise_signals / denoise_along): the forward transform fused into the load
of the transform kernels and the inverse into the store of the sum.  B3spline, weights [5, 3], Poisson counts of mean 5:

    denoise_signals  4096 x 4096 float32,  4096 x 4096 float64,  65536 x 512 float32
    denoise_along    (64, 1024, 1024) float32 along axis 0

Per shape three comparisons, host to host, wall clock around a drained stream, the two sides of each sampled in
ALTERNATION, --samples per side (tools/bench_signals.alternate); median / min / max / spread of either side:

  * off:    anscombe=True against anscombe=False on the same tree - the cost of the fusion;
  * host:   anscombe=True against the route a user could write without the keyword - numpy's 2 * sqrt(max(x + 3/8, 0))
            over the whole array, the engine with anscombe=False, numpy's (y / 2)^2 - 3/8 over the result (NOT what
            denoise(..., anscombe=True) computes bit for bit: the per-signal call inverts on the device);
  * loop:   anscombe=True against the per-signal loop of denoise(signal, [5, 3], anscombe=True), timed on a SUBSET of
            the signals (--loop-signals, 256; for the axis engine the first 256 light curves, contiguous copies made
            outside the clock) in the first --loop-samples rounds and scaled to the stack, as tools/bench_wow_signals.py.

    python tools/bench_lines_anscombe.py [--samples 20] [--loop-samples 3] [--loop-signals 256] [--shapes ...] [--out profiles/NAME.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_signals import alternate                 # noqa: E402  (the sampling of the signal engine's tool)

SHAPES = ["4096x4096xf32", "4096x4096xf64", "65536x512xf32", "64x1024x1024xf32@0"]
WEIGHTS = [5, 3]


def host_forward(x):
    t = x + x.dtype.type(0.375)
    np.maximum(t, 0, out=t)
    np.sqrt(t, out=t)
    t *= x.dtype.type(2)
    return t


def host_inverse(y):
    y = y * y.dtype.type(0.5)
    y *= y
    y -= y.dtype.type(0.375)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--loop-samples", type=int, default=3)
    ap.add_argument("--loop-signals", type=int, default=256)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    rows = []
    for item in a.shapes.split(","):
        item, _, axis = item.partition("@")
        *dims, t = item.split("x")
        shape, dtype = tuple(int(d) for d in dims), np.float32 if t == "f32" else np.float64
        data = np.random.default_rng(0).poisson(5.0, shape).astype(dtype)
        if axis == "":
            assert W.signals_eligible(data, len(WEIGHTS))
            engine = lambda x, **kw: W.denoise_signals(x, WEIGHTS, **kw)
            sub, M = data[:a.loop_signals], shape[0]
        else:
            ax = int(axis)
            assert W.along_eligible(data, len(WEIGHTS), axis=ax)
            engine = lambda x, **kw: W.denoise_along(x, WEIGHTS, axis=ax, **kw)
            moved = np.moveaxis(data, ax, -1)
            M = moved.size // shape[ax]
            sub = np.ascontiguousarray(moved.reshape(-1, shape[ax])[:a.loop_signals])
        rec = {"shape": list(shape), "axis": None if axis == "" else int(axis), "dtype": np.dtype(dtype).name, "family": "B3spline",
               "weights": WEIGHTS, "signals": M}
        on, off = alternate(ctx, lambda: engine(data, anscombe=True), lambda: engine(data), a.samples)
        rec["off"] = {"anscombe": on, "plain": off, "anscombe_over_plain": on["median_ms"] / off["median_ms"]}
        on, host = alternate(ctx, lambda: engine(data, anscombe=True), lambda: host_inverse(engine(host_forward(data))), a.samples)
        rec["host"] = {"anscombe": on, "host_wrapped": host, "host_wrapped_over_anscombe": host["median_ms"] / on["median_ms"]}
        on, loop = alternate(ctx, lambda: engine(data, anscombe=True), lambda: [W.denoise(s, WEIGHTS, anscombe=True) for s in sub],
                             a.samples, a.loop_samples)
        scale = M / len(sub)
        rec["loop"] = {"anscombe": on, "loop_subset": loop, "loop_signals": len(sub), "loop_scaled_median_ms": loop["median_ms"] * scale,
                       "loop_over_anscombe": loop["median_ms"] * scale / on["median_ms"]}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_lines_anscombe.py", "samples": a.samples, "loop_samples": a.loop_samples, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
