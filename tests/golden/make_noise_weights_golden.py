#!/usr/bin/env python3
"""Writes tests/golden/g25_noise_weights.npz (CPU only): the reference side of the statistical test of
compute_noise_weights(seed=...) in tests/test_gpu_noise_rng.py.

Per case - family x (plain | bilateral=1) x n_scales in (3, 4) - the C oracle (oracle/cref.py) transforms T0 = 400
frames of np.random.default_rng noise of the side compute_noise_weights uses (len(sigma_e_1d) * 2**n_scales); the
per-plane np.std of every trial gives, per scale, the mean m and the per-trial standard deviation d (ddof=1) of the
estimate.  Keys: <family>_<plain|bil>_L<n_scales>_m / _d, plus T0.

    python tests/golden/make_noise_weights_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import cref  # noqa: E402

T0 = 400
N_TAB = 11                        # len(sigma_e_1d), both families (watroo/wavelets.py:239-241, 268-270)
CASES = [(fam, bil, L) for fam in ("b3spline", "triangle") for bil in (None, 1) for L in (3, 4)]


def main():
    cref.build()
    out = {"T0": np.int64(T0)}
    for i, (fam, bil, L) in enumerate(CASES):
        rng = np.random.default_rng(2500 + i)
        side = N_TAB * 2 ** L
        est = np.empty((T0, L))
        for t in range(T0):
            img = rng.standard_normal((side, side)).astype(np.float32)
            planes = cref.decompose(img, L, fam) if bil is None else cref.decompose_bilateral(img, L, fam, bil)
            est[t] = [np.std(planes[s].astype(np.float64)) for s in range(L)]
        key = f"{fam}_{'plain' if bil is None else 'bil'}_L{L}"
        out[key + "_m"] = est.mean(axis=0)
        out[key + "_d"] = est.std(axis=0, ddof=1)
        print(key, out[key + "_m"], out[key + "_d"])
    np.savez(os.path.join(ROOT, "tests", "golden", "g25_noise_weights.npz"), **out)


if __name__ == "__main__":
    main()
