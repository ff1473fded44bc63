#!/usr/bin/env python3
"""The 1-D transform along an axis that is not the last one: the axis engine (wt_along: transform_along / denoise_along,
no transpose) against the best route before it - transpose on the host, transform_signals / denoise_signals, transpose
back.  B3spline, level 4, denoise weights [5, 3]:

    float32 (64, 1024, 1024), (512, 256, 256), (32, 2048, 2048) along axis 0,  float32 (1024, 64, 1024) along axis 1,
    float64 (64, 1024, 1024) along axis 0

  * host to host: transform_along / denoise_along against the transposed route (both return arrays of the same layout);
  * device-resident (the first chunk already in HBM, nothing crosses PCIe): the three kernels of the axis engine timed
    by HIP events on the stream (Context.profile) - bytes per second from their stated traffic: decompose
    sizeof(T) * (level + 2), abs_median sizeof(T), denoise 2 * sizeof(T) per sample - and SignalBatch.decompose on the
    transposed chunk beside them.

Both host routes are sampled in ALTERNATION (engine, transposed, engine, ...), wall clock around a drained stream, 20
samples per side (--samples); one JSON line per shape with median / min / max / spread of either side and the ratio of
the medians.

    python tools/bench_along.py [--samples 20] [--shapes 64x1024x1024xf32@0,...] [--sections ...] [--out profiles/NAME.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_signals import alternate                 # noqa: E402  (the sampling of the signal engine's tool)

SHAPES = ["64x1024x1024xf32@0", "512x256x256xf32@0", "32x2048x2048xf32@0", "1024x64x1024xf32@1", "64x1024x1024xf64@0"]
LEVEL = 4
WEIGHTS = [5, 3]


def transposed_transform(W, a, axis):
    m = np.moveaxis(a, axis, -1)
    res = W.transform_signals(np.ascontiguousarray(m).reshape(-1, a.shape[axis]), LEVEL)
    r = np.moveaxis(res.reshape(m.shape[:-1] + res.shape[1:]), -2, 0)
    return np.ascontiguousarray(np.moveaxis(r, -1, 1 + axis))


def transposed_denoise(W, a, axis):
    m = np.moveaxis(a, axis, -1)
    res = W.denoise_signals(np.ascontiguousarray(m).reshape(-1, a.shape[axis]), WEIGHTS)
    return np.ascontiguousarray(np.moveaxis(res.reshape(m.shape), -1, axis))


def pair(name, rec, engine, other):
    rec[name] = {"along": engine, "transposed": other, "transposed_over_along": other["median_ms"] / engine["median_ms"]}


def kernel_rates(ctx, run, n, bytes_of):
    """{kernel: {calls, mean ms, GB/s}} of n runs of run() from the stream's HIP events"""
    run()
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(n):
        run()
    ctx.sync()
    out = {}
    for name, (calls, ms) in ctx.profile_entries().items():
        if calls and name in bytes_of:
            out[name] = {"calls": calls, "mean_ms": ms / calls, "GB_per_s": bytes_of[name] / (ms / calls) / 1e6}
    ctx.profile(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sections", default="transform_host,denoise_host,device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    from wavelets_amd import along as A
    ctx = L.default_context()
    sections = a.sections.split(",")
    rows = []
    for item in a.shapes.split(","):
        dims, axis = item.split("@")
        *shape, t = dims.split("x")
        shape, axis, dtype = tuple(int(v) for v in shape), int(axis), np.float32 if t == "f32" else np.float64
        arr = (np.random.default_rng(0).standard_normal(shape) * 3.0 + 10.0).astype(dtype)
        assert A.along_eligible(arr, LEVEL, axis=axis)
        rec = {"shape": list(shape), "axis": axis, "dtype": np.dtype(dtype).name, "family": "B3spline", "level": LEVEL, "weights": WEIGHTS}
        if "transform_host" in sections:
            pair("transform_host", rec, *alternate(ctx, lambda: W.transform_along(arr, LEVEL, axis=axis),
                                                   lambda: transposed_transform(W, arr, axis), a.samples))
            print(json.dumps({"shape": rec["shape"], "dtype": rec["dtype"], "transform_host": rec["transform_host"]}), flush=True)
        if "denoise_host" in sections:
            pair("denoise_host", rec, *alternate(ctx, lambda: W.denoise_along(arr, WEIGHTS, axis=axis),
                                                 lambda: transposed_denoise(W, arr, axis), a.samples))
            print(json.dumps({"shape": rec["shape"], "dtype": rec["dtype"], "denoise_host": rec["denoise_host"]}), flush=True)
        if "device" in sections:
            L.trim_along()
            L.trim_signals()
            O, N, I = A._view(shape, axis)
            isz, sfx = arr.dtype.itemsize, "<double>" if dtype == np.float64 else "<float>"
            o0, no, i0, ni = L.along_chunks(O, N, I, LEVEL, isz)[0]
            block = arr.reshape(O, N, I)[o0:o0 + no, :, i0:i0 + ni]
            samples = no * N * ni
            dev = {"chunk": [no, N, ni]}
            ab = L.AlongBatch(ctx, no * ni, N, L.B3SPLINE, LEVEL, dtype, planes=True)
            ab.upload(block)
            dev.update(kernel_rates(ctx, lambda: ab.decompose(LEVEL), a.samples,
                                    {"wt_along_decompose_kernel" + sfx: samples * isz * (LEVEL + 2)}))
            ab.close()
            ab = L.AlongBatch(ctx, no * ni, N, L.B3SPLINE, len(WEIGHTS), dtype, planes=False)
            ab.upload(block)
            taus = np.full((no * ni, len(WEIGHTS)), 1.0)
            dev.update(kernel_rates(ctx, lambda: (ab.abs_median(), ab.denoise(len(WEIGHTS), taus, [1.0, 1.0])), a.samples,
                                    {"wt_along_abs_median_kernel" + sfx: samples * isz, "wt_along_denoise_kernel" + sfx: 2 * samples * isz}))
            ab.close()
            sig = np.ascontiguousarray(np.moveaxis(block, 1, -1)).reshape(-1, N)
            sb = L.SignalBatch(ctx, len(sig), N, L.B3SPLINE, LEVEL, dtype)
            sb.upload(sig)
            dev.update(kernel_rates(ctx, lambda: sb.decompose(len(sig), LEVEL), a.samples,
                                    {"wt_signals_decompose_kernel" + sfx: samples * isz * (LEVEL + 2)}))
            sb.close()
            rec["device"] = dev
            print(json.dumps({"shape": rec["shape"], "dtype": rec["dtype"], "device": dev}), flush=True)
        rows.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_along.py", "samples": a.samples, "sections": a.sections, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
