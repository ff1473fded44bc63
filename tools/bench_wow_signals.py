#!/usr/bin/env python3
"""wow of stacks of 1-D signals: the signal engine's route (wow_signals: per chunk one transform launch, the medians
and the plane moments in one round trip each, one wow launch) against the route before it - a Python loop of
wow(signal, ...) calls, each an upload, a launch per scale, up to n_scales + 1 reductions with a host round trip each,
a plane sum and a download.  B3spline, n_scales as wow() resolves it for the length, three keyword cases:

    default  (whitening: the last plane's moments)
    den_pv   (denoise_coefficients=[5, 2], preserve_variance=True: the MAD medians and every plane's moments)
    plain    (whitening=False: no reduction, the bits of the loop)

    float32 and float64 (4096, 2048), (65536, 256), (256, 8192 | 4096)

Host to host, wall clock around a drained stream.  The loop is timed on a SUBSET of the signals (--loop-signals, 256)
and scaled to the stack - a whole loop over 65536 signals takes minutes; its time is linear in the signal count.  The
engine and the subset loop are sampled in ALTERNATION, --samples per side (the loop in the first --loop-samples
rounds only); one JSON line per shape and case with median / min / max / spread of either side and the ratio of the
scaled loop's median to the engine's.

    python tools/bench_wow_signals.py [--samples 10] [--loop-samples 3] [--loop-signals 256] [--shapes 4096x2048xf32,...]
                                      [--out profiles/NAME.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_signals import alternate                 # noqa: E402  (the sampling of the signal engine's tool)

SHAPES = ["4096x2048xf32", "65536x256xf32", "256x8192xf32", "4096x2048xf64", "65536x256xf64", "256x4096xf64"]
CASES = {"default": dict(),
         "den_pv": dict(denoise_coefficients=[5, 2], preserve_variance=True),
         "plain": dict(whitening=False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--loop-samples", type=int, default=3)
    ap.add_argument("--loop-signals", type=int, default=256)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    rows = []
    for item in a.shapes.split(","):
        m, n, t = item.split("x")
        M, N, dtype = int(m), int(n), np.float32 if t == "f32" else np.float64
        sig = (np.random.default_rng(0).standard_normal((M, N)) * 3.0 + 10.0).astype(dtype)
        assert W.wow_signals_eligible(sig, None)
        sub = sig[:min(M, a.loop_signals)]
        for case in a.cases.split(","):
            kw = CASES[case]
            engine, loop = alternate(ctx, lambda: W.wow_signals(sig, **kw),
                                     lambda: [W.wow(s, **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()})[0] for s in sub],
                                     a.samples, a.loop_samples)
            scale = M / len(sub)
            rec = {"shape": [M, N], "dtype": np.dtype(dtype).name, "family": "B3spline", "case": case, "keywords": kw,
                   "engine": engine, "loop_subset": loop, "loop_signals": len(sub),
                   "loop_scaled_median_ms": loop["median_ms"] * scale,
                   "loop_over_engine": loop["median_ms"] * scale / engine["median_ms"]}
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_wow_signals.py", "samples": a.samples, "loop_samples": a.loop_samples, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
