#!/usr/bin/env python3
"""Frames that stay on the device against frames that cross PCIe twice: resident.transform_stack(frames, 2) and
resident.denoise_stack(frames, [5, 3]) from a DeviceArray into a DeviceArray, against batch.transform_stack /
batch.denoise_stack numpy to numpy (the path every caller had before, unchanged), in one process.  B3; stacks
16 x 1024^2 float32, 1 x 8192^2 float32, 16 x 1024^2 int16 (the float64 batch, widened on the way in).

Per stack and call, after a warm-up, `--samples` (>= 20) samples each of
  * resident, device side: HIP events on the context's stream around the call (loads, passes, medians, stores);
  * resident, wall clock around the call (it ends with the context's stream synchronised: stream=None);
  * host to host, wall clock around the numpy-to-numpy call
as median / min / max in ms, and the ratio of the two wall-clock medians (> 1: the resident call is faster).  The
results of the two routes are compared bit for bit once per case before anything is timed.

    python tools/bench_resident.py [--samples K] [--out profiles/rNN_resident.json] [--time-limit SECONDS]

One JSON line per case, the whole record into --out.  One process; --time-limit ends it (exit code 3, what was measured
so far is written)."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STACKS = [(16, 1024, "float32"), (1, 8192, "float32"), (16, 1024, "int16")]
LEVEL, WEIGHTS = 2, [5, 3]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "samples": len(ms)}


def frames(n, side, dtype):
    x = np.random.default_rng(n * side).standard_normal((n, side, side), dtype=np.float32) * 3 + 10
    return x if dtype == "float32" else np.rint(x * 100).astype(dtype)


class TimeLimit(Exception):
    pass


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--time-limit", type=int, default=540)
    args = ap.parse_args()
    if args.samples < 20:
        ap.error("--samples: at least 20")

    def alarm(*_):
        raise TimeLimit

    signal.signal(signal.SIGALRM, alarm)
    signal.alarm(args.time_limit)

    from wavelets_amd import _lib as L
    from wavelets_amd import batch as B
    from wavelets_amd import resident as R
    ctx = L.default_context()
    record = {"tool": "tools/bench_resident.py", "device": ctx.device_info(), "samples": args.samples, "level": LEVEL,
              "weights": WEIGHTS, "scaling_function": "B3spline", "cases": [], "complete": False}
    rc = 0
    try:
        for n, side, dtype in STACKS:
            host = frames(n, side, dtype)
            dev = R.DeviceArray.from_numpy(host)
            calls = {"transform_stack": (lambda o: R.transform_stack(dev, LEVEL, out=o), lambda: B.transform_stack(host, LEVEL)),
                     "denoise_stack": (lambda o: R.denoise_stack(dev, WEIGHTS, out=o), lambda: B.denoise_stack(host, WEIGHTS))}
            for name, (resident, host_call) in calls.items():
                want = host_call()
                out = R.DeviceArray.empty(want.shape, want.dtype)
                same = bool(np.array_equal(resident(out).numpy().view(np.uint8), want.view(np.uint8)))
                del want
                for _ in range(2):
                    resident(out)
                    host_call()
                ev, wall, h2h = [], [], []
                for _ in range(args.samples):
                    ctx.timer_start()
                    t0 = time.perf_counter()
                    resident(out)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ev.append(ctx.timer_stop())
                for _ in range(args.samples):
                    t0 = time.perf_counter()
                    host_call()
                    h2h.append((time.perf_counter() - t0) * 1e3)
                case = {"frames": n, "side": side, "dtype": dtype, "result_dtype": str(out.dtype), "call": name, "bits_equal": same,
                        "resident_device": stats(ev), "resident_wall": stats(wall), "host_to_host_wall": stats(h2h)}
                case["host_over_resident_wall"] = case["host_to_host_wall"]["median_ms"] / case["resident_wall"]["median_ms"]
                record["cases"].append(case)
                print(json.dumps(case), flush=True)
                out.free()
            dev.free()
        record["complete"] = True
    except TimeLimit:
        print(f"time limit of {args.time_limit} s reached", file=sys.stderr)
        rc = 3
    signal.alarm(0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
