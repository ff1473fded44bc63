#!/usr/bin/env python3
"""Stacks whose noise is a per-pixel map: denoise_stack / wow_stack on the batch's noise plane (wt_batch_denoise_sum_map,
wt_batch_wow_scale_map, wt_batch_wow_update_map) against the per-frame loop those calls ran before the batch took maps -
denoise(f, ..., noise=map_i) / wow(f, ..., noise=map_i) per frame, in the same process.  B3, float32 N(10, 3) frames,
16 x 1024^2 and 4 x 4096^2, maps uniform in [0.5, 2); HIP-event samples (median / min / max, spread = max / median - 1):
  * device-resident (frames and maps uploaded before the clock starts): denoise([5, 3]) = transform + thresholds + sum,
    and wow(denoise_coefficients=[5, 2]) = transform + the per-scale updates + sum - batched: one BatchPlan over the
    stack; loop: one Plan per frame, the per-frame API's call sequence;
  * host to host, with a shared map and with per-frame maps: denoise_stack / wow_stack against the loop of
    denoise / wow calls.

    python tools/bench_noise_map_stack.py [--samples K] [--shapes N:side,...] [--out FILE]

One JSON line per stack and a final RESULT line with the ratios loop / batch (> 1: the batch is faster)."""
import argparse
import json
import os
import sys

import numpy as np

SHAPES = [(16, 1024), (4, 4096)]
DENOISE = [5, 3]
WOW_DENOISE = [5, 2]


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


def device_resident(ctx, fr, maps, samples):
    """{key: stats} of the device-resident steps, batched and looped (per-frame maps: the loop's plans hold one each)"""
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    from wavelets_amd import batch as B
    from wavelets_amd import utils as U
    from wavelets_amd import wavelets as WV
    N, H, Wd = fr.shape
    sf = W.B3spline(2)
    se = sf.sigma_e()
    Lw = U._wow_scale_limit(U._wow_n_scales((H, Wd), W.B3spline, None, 0, WOW_DENOISE), W.B3spline, 2, None, WOW_DENOISE)
    taus = [float(s * se[i]) for i, s in enumerate(DENOISE)]
    rec = {}
    bp = L.BatchPlan(ctx, N, H, Wd, L.B3SPLINE, Lw)
    bp.upload(L.PLANE_INPUT, fr)
    bp.fill(N, WV._NOISE_PLANE, 1.0)
    bp.upload(WV._NOISE_PLANE, maps)

    def den_b():
        bp.decompose(N, L.PLANE_INPUT, len(DENOISE))
        bp.denoise_sum(N, len(DENOISE) + 1, [taus] * N, [1] * len(DENOISE), True, noise_plane=WV._NOISE_PLANE)

    def wow_b():
        bp.decompose(N, L.PLANE_INPUT, Lw)
        B._wow_batch_device(bp, N, list(maps), W.B3spline, Lw, [], True, WOW_DENOISE, True, False, 3.2, None, None, 0)
    rec["denoise_device_batch"] = stats(timed(ctx, den_b, samples))
    rec["wow_device_batch"] = stats(timed(ctx, wow_b, samples))
    bp.close()
    plans, coefs = [], []
    for f in range(N):
        p = L.Plan(ctx, H, Wd, L.B3SPLINE, Lw)
        p.upload(L.PLANE_INPUT, fr[f])
        p.upload(WV._NOISE_PLANE, maps[f])
        c = WV.Coefficients(p, sf)
        c.noise = maps[f]
        c._noise_uploaded = maps[f]
        plans.append(p)
        coefs.append(c)

    def den_l():                      # utils.denoise with a map: transform, then wt_denoise_sum with the noise plane
        for p in plans:
            p.decompose(L.PLANE_INPUT, len(DENOISE))
            p.denoise_sum(len(DENOISE) + 1, taus, [1] * len(DENOISE), True, WV._NOISE_PLANE)

    def wow_l():                      # utils.wow with a map: transform, utils._wow_device
        for p, c in zip(plans, coefs):
            p.decompose(L.PLANE_INPUT, Lw)
            U._wow_device(c, Lw, [], True, WOW_DENOISE, True, False, 3.2, None, None, 0)
    rec["denoise_device_loop"] = stats(timed(ctx, den_l, samples))
    rec["wow_device_loop"] = stats(timed(ctx, wow_l, samples))
    for c in coefs:
        c._plan = None
    for p in plans:
        p.close()
    return rec


def host_to_host(ctx, fr, maps, samples):
    import wavelets_amd as W
    rec = {}
    for kind, arg, per in (("shared", maps[0], [maps[0]] * len(fr)), ("per_frame", list(maps), list(maps))):
        rec[f"denoise_host_{kind}_batch"] = stats(timed(ctx, lambda: W.denoise_stack(fr, DENOISE, noise=arg), samples, warm=1))
        rec[f"denoise_host_{kind}_loop"] = stats(timed(
            ctx, lambda: [W.denoise(f, DENOISE, noise=n) for f, n in zip(fr, per)], samples, warm=1))
        rec[f"wow_host_{kind}_batch"] = stats(timed(
            ctx, lambda: W.wow_stack(fr, noise=arg, denoise_coefficients=list(WOW_DENOISE)), samples, warm=1))
        rec[f"wow_host_{kind}_loop"] = stats(timed(
            ctx, lambda: [W.wow(f, noise=n, denoise_coefficients=list(WOW_DENOISE)) for f, n in zip(fr, per)], samples, warm=1))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--shapes", default=None, help="N:side,N:side,... (default: 16:1024,4:4096)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.samples < 20:
        ap.error("at least 20 samples per step")
    shapes = SHAPES if a.shapes is None else [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    rows = []
    for N, side in shapes:
        rng = np.random.default_rng(0)
        fr = (rng.standard_normal((N, side, side)) * 3 + 10).astype(np.float32)
        maps = rng.uniform(0.5, 2.0, (N, side, side)).astype(np.float32)
        rec = {"shape": [N, side, side]}
        rec.update(device_resident(ctx, fr, maps, a.samples))
        L.trim_batches()
        rec.update(host_to_host(ctx, fr, maps, a.samples))
        L.trim_batches()
        rec["loop_over_batch"] = {k[:-6]: rec[k[:-6] + "_loop"]["median_ms"] / rec[k]["median_ms"]
                                  for k in rec if k.endswith("_batch")}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    line = json.dumps({"bench": "noise_map_stack", "dtype": "float32", "family": "B3spline", "samples": a.samples,
                       "stacks": [{"shape": r["shape"], "loop_over_batch": r["loop_over_batch"],
                                   "max_spread": max(v["spread"] for v in r.values() if isinstance(v, dict) and "spread" in v)}
                                  for r in rows]})
    print("RESULT " + line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
