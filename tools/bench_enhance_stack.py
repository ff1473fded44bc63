#!/usr/bin/env python3
"""enhance_stack against the loop of utils.enhance (the only route before it), in one process.  Stacks: 1 x 3 x 512^2,
1 x 3 x 1024^2, 1 x 3 x 2048^2 (one colour image), 64 x 512^2 (gray), 16 x 3 x 1024^2; float32 plain, float32
bilateral=1, float64; three scales, every channel its own sigmas and weights, no noise given (the MAD estimate of
every frame).  15 HIP-event samples each, median with min - max:
  * device-resident: the frames already in HBM - batched: transform, medians in one round trip, one thresholded
    weighted sum (wt_batch_enhance_sum) over all frames; loop: per frame the transform, its median, wt_denoise_sum;
  * host to host: enhance_stack(frames, ...) against np.stack([enhance(f, ...) for f in frames]).
The condition of DESIGN.md section 3.11: the batched median is not above the loop's median at any stack.

    python tools/bench_enhance_stack.py [--samples K] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STACKS = [(1, 3, 512), (1, 3, 1024), (1, 3, 2048), (64, 1, 512), (16, 3, 1024)]
COLOUR = dict(weights=[[.5, 2, 1], [1, 1.5, .5], [2, 2, 1]], denoise=[[5, 3, 0], [3, 2, 1], [3, 0, 0]])
GRAY = dict(weights=[.5, 2, 1], denoise=[5, 3, 1])
LEVEL = 3
MODES = [("float32", np.float32, None), ("float32 bilateral=1", np.float32, 1), ("float64", np.float64, None)]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "samples": len(ms)}


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


def device_pair(ctx, fr, rows, bilateral, samples):
    """(batched, loop) device-resident samples: fr (n, H, W), rows[f] = (sigmas, weights) of frame f"""
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    from wavelets_amd.wavelets import _noise_from_median, _tau_row, _sigma_bilateral_list
    n, H, Wd = fr.shape
    f64 = fr.dtype == np.float64
    sf = W.B3spline(2)
    se = sf.sigma_e(bilateral=bilateral)
    sb = None if bilateral is None else _sigma_bilateral_list(bilateral, LEVEL)
    ent = [list(zip(range(LEVEL + 1), d, w)) for d, w in rows]
    bp = (L.BatchPlan64 if f64 else L.BatchPlan)(ctx, n, H, Wd, L.B3SPLINE, LEVEL)
    bp.upload(L.PLANE_INPUT, fr)

    def batched():
        if sb is None:
            bp.decompose(n, L.PLANE_INPUT, LEVEL, L.FLAG_FUSED)
        else:
            bp.decompose_bilateral(n, L.PLANE_INPUT, LEVEL, sb, False)
        nz = [_noise_from_median(m, se) for m in bp.abs_median(n, 0)]
        bp.enhance_sum(n, LEVEL + 1, [_tau_row(e, z, se, True) for e, z in zip(ent, nz)], [w for _, w in rows], True)
    tb = timed(ctx, batched, samples)
    bp.close()
    plans = []
    for f in range(n):
        p = L.Plan64(ctx, H, Wd, (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16), LEVEL) if f64 else L.Plan(ctx, H, Wd, L.B3SPLINE, LEVEL)
        p.upload(L.PLANE_INPUT, fr[f])
        plans.append(p)

    def loop():
        for p, e, (_, w) in zip(plans, ent, rows):
            if sb is None:
                p.decompose(L.PLANE_INPUT, LEVEL, L.FLAG_MEDIAN_HIST if f64 else L.FLAG_FUSED | L.FLAG_MEDIAN_HIST)
            else:
                p.decompose_bilateral(L.PLANE_INPUT, LEVEL, sb, False, 0)
            z = _noise_from_median(p.abs_median(0), se)
            p.denoise_sum(LEVEL + 1, _tau_row(e, z, se, True), w, True, L.PLANE_NONE, False)
    tl = timed(ctx, loop, samples)
    for p in plans:
        p.close()
    return tb, tl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wavelets_amd as W
    from wavelets_amd import _lib as L
    from wavelets_amd.utils import enhance
    ctx = L.default_context()
    rows_out, ok = [], True
    for mode, dt, bil in MODES:
        for N, C, side in STACKS:
            rng = np.random.default_rng(0)
            fr = (rng.standard_normal((N, C, side, side) if C == 3 else (N, side, side)) * 30.0 + 100.0).astype(dt)
            par = COLOUR if C == 3 else GRAY
            kw = dict(par, **({} if bil is None else {"bilateral": bil}))
            chan = list(zip(par["denoise"], par["weights"])) if C == 3 else [(par["denoise"], par["weights"])]
            tb, tl = device_pair(ctx, fr.reshape(N * C, side, side), [chan[f % C] for f in range(N * C)], bil, a.samples)
            hb = timed(ctx, lambda: W.enhance_stack(fr, **kw), a.samples, warm=1)
            hl = timed(ctx, lambda: np.stack([enhance(f, **kw) for f in fr]), a.samples, warm=1)
            L.trim_batches()
            rec = {"mode": mode, "stack": [N, C, side, side] if C == 3 else [N, side, side],
                   "device": {"batched": stats(tb), "loop": stats(tl)}, "host": {"batched": stats(hb), "loop": stats(hl)}}
            for k in ("device", "host"):
                rec[k]["speedup"] = rec[k]["loop"]["median_ms"] / rec[k]["batched"]["median_ms"]
                ok &= rec[k]["batched"]["median_ms"] <= rec[k]["loop"]["median_ms"]
            rows_out.append(rec)
            print(json.dumps(rec), flush=True)
    res = {"bench": "enhance_stack", "level": LEVEL, "samples": a.samples, "batched_not_above_loop": bool(ok), "rows": rows_out}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)
    print("RESULT " + json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
