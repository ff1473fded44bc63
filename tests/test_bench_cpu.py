"""CPU tests of bench.py's --dump-outputs writer (bench.dump_outputs) on a stand-in plan: which arrays, what
shapes, the fixed sample of a large image, and the size bound of the whole dump."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class FakePlan:
    """planes 0 .. n-1 and PLANE_OUT of an H x W image, filled with values that name plane and pixel"""

    def __init__(self, H, W, nplanes):
        from wavelets_amd._lib import PLANE_OUT
        self.shape = (H, W)
        pix = np.arange(H * W, dtype=np.float32).reshape(H, W)
        self.planes = {s: pix + np.float32(s) * 1e7 for s in range(nplanes)}
        self.planes[PLANE_OUT] = -pix

    def download(self, plane, out=None):
        if out is None:
            out = np.empty(self.shape, np.float32)
        out[...] = self.planes[plane]
        return out


def test_small_image_is_written_whole(tmp_path):
    B = _bench()
    plan = FakePlan(24, 40, 4)
    B.dump_outputs(str(tmp_path), plan, 4, {"noise": 0.25})
    c = np.load(tmp_path / "coefficients.npy")
    r = np.load(tmp_path / "reconstruction.npy")
    assert c.dtype == np.float32 and c.shape == (4, 24, 40)
    for s in range(4):
        np.testing.assert_array_equal(c[s], plan.planes[s])
    assert r.dtype == np.float32 and r.shape == (24, 40)
    np.testing.assert_array_equal(r, -np.arange(24 * 40, dtype=np.float32).reshape(24, 40))
    n = np.load(tmp_path / "noise.npy")
    assert n.dtype == np.float64 and n.tolist() == [0.25]
    assert sorted(os.listdir(tmp_path)) == ["coefficients.npy", "noise.npy", "reconstruction.npy"]


def test_large_image_is_sampled_at_the_same_fixed_positions(tmp_path):
    B = _bench()
    H, W = 1100, 1000                                   # 1.1 M pixels > DUMP_SAMPLE
    assert H * W > B.DUMP_SAMPLE
    plan = FakePlan(H, W, 3)
    B.dump_outputs(str(tmp_path / "a"), plan, 3)
    B.dump_outputs(str(tmp_path / "b"), plan, 3)
    c = np.load(tmp_path / "a" / "coefficients.npy")
    r = np.load(tmp_path / "a" / "reconstruction.npy")
    assert c.dtype == np.float32 and c.shape == (3, B.DUMP_SAMPLE) and r.shape == (B.DUMP_SAMPLE,)
    # the pixel positions: the same in every array (the planes' values encode them) and the same in every run
    idx = -r.astype(np.int64)
    assert np.all(np.diff(idx) >= 0) and idx[0] >= 0 and idx[-1] < H * W
    for s in range(3):
        np.testing.assert_array_equal(c[s], idx.astype(np.float32) + np.float32(s) * 1e7)
    np.testing.assert_array_equal(c, np.load(tmp_path / "b" / "coefficients.npy"))
    np.testing.assert_array_equal(r, np.load(tmp_path / "b" / "reconstruction.npy"))
    assert not os.path.exists(tmp_path / "a" / "noise.npy")


def test_the_largest_bench_dump_stays_within_64_mb():
    """cfg5 at 32768^2 (the most planes a bench run has: wow's own scale count, 13 scales + the smooth plane) plus the
    reconstruction, every one a DUMP_SAMPLE sample of float32, plus the noise scalar"""
    B = _bench()
    level = int(np.round(np.log2(32768) - np.log2(5)))
    total = (level + 2) * B.DUMP_SAMPLE * 4 + 8
    assert total <= 64 * 2 ** 20, total
