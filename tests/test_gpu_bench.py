"""GPU tests of bench.py's plain line and of --dump-outputs (run with -m gpu on an MI355X): a run without --full
times the steps and says so, nothing more; the outputs it writes are what the path computes (C oracle), and two runs
with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_is_the_timed_steps_and_its_outputs_match_the_oracle(tmp_path):
    from conftest import plane_bound, recon_bound
    import __graft_entry__ as entry
    entry.build()
    from oracle import cref
    out = _bench("--steps", "7", "--warmup", "2", "--size", "1024", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 7 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "Mpix/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - 1024 * 1024 / out["ms_per_step"] / 1e3) < 0.02 * out["value"]      # (ms_per_step: 4 decimals)
    for key in ("roofline", "kernels", "configs", "cpu_baseline", "first_call", "sequence", "pcie_inclusive_mpix_s",
                "ms_per_step_samples", "n1_same_image", "odd_width", "float64"):
        assert key not in out, key
    # 1024^2 = 2^20 pixels: the arrays are written whole
    c = np.load(tmp_path / "coefficients.npy")
    r = np.load(tmp_path / "reconstruction.npy")
    assert c.dtype == np.float32 and c.shape == (7, 1024, 1024) and r.shape == (1024, 1024)
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    img = B.make_strip(1024, 1024, seed=0)                   # the bench's input (rank 0)
    amax = float(np.abs(img).max())
    ref = cref.decompose(img, 6, "b3spline")
    for s in range(7):
        assert float(np.abs(c[s] - ref[s]).max()) <= plane_bound(s, amax), s
    assert float(np.abs(r - cref.plane_sum(ref)).max()) <= recon_bound(amax)


def test_two_runs_dump_the_same_outputs(tmp_path):
    for d in ("a", "b"):
        _bench("--steps", "3", "--warmup", "1", "--size", "2048", "--dump-outputs", str(tmp_path / d))
    for name in ("coefficients", "reconstruction"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape[-1] == 1 << 20          # 2048^2 pixels: the fixed sample
        np.testing.assert_array_equal(a, b, err_msg=name)


def test_cfg3_dump_carries_the_denoised_planes_and_the_noise(tmp_path):
    out = _bench("--config", "cfg3", "--steps", "3", "--warmup", "1", "--size", "1024", "--dump-outputs", str(tmp_path))
    assert out["config"]["name"] == "cfg3" and out["steps"] == 3
    c = np.load(tmp_path / "coefficients.npy")
    r = np.load(tmp_path / "reconstruction.npy")
    noise = np.load(tmp_path / "noise.npy")
    assert c.shape == (9, 1024, 1024) and r.shape == (1024, 1024) and noise.shape == (1,) and noise[0] > 0
    # the reconstruction is the sum of the (thresholded) planes, in plane order
    acc = c[0].copy()
    for s in range(1, 9):
        acc += c[s]
    assert float(np.abs(acc - r).max()) <= 1e-5 * float(np.abs(r).max())
