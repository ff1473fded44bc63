"""Host logic of the batched wow (wavelets_amd.batch.wow_stack): the eligibility predicate, the n_scales resolution
shared with utils.wow, per-frame noise lists, the fallback loop and chunking with wow's extra planes.  No GPU
needed: the device steps are replaced by stand-ins where a call gets that far."""
import warnings

import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B
from wavelets_amd import utils as U


def test_wow_stack_is_exported():
    assert W.wow_stack is B.wow_stack
    assert "wow_stack" in B.__all__ and "wow_eligible" in B.__all__


def test_wow_eligibility_predicate():
    f32 = np.zeros((3, 64, 80), np.float32)
    assert B.wow_eligible(f32, 4)
    assert B.wow_eligible(f32, 1) and B.wow_eligible(f32, 9) and B.wow_eligible(f32, 10)    # stencil passes
    assert B.wow_eligible(f32, 6, W.Triangle)
    assert not B.wow_eligible(f32, 0) and not B.wow_eligible(f32, 25)
    assert not B.wow_eligible(f32.astype(np.float64), 4)                    # float64: per frame
    assert not B.wow_eligible(f32.astype(np.int16), 4)                      # integers
    assert not B.wow_eligible(f32.astype(">f4"), 4)                         # byte-swapped
    assert not B.wow_eligible(f32, 4, bilateral=1)
    assert not B.wow_eligible(f32, 4, noise_per_frame=None)                 # a 2-D noise map
    assert not B.wow_eligible(f32, 4, noise_per_frame=[np.ones((64, 80))] * 3)
    assert not B.wow_eligible(f32, 4, noise_per_frame=[np.array(2.0)] * 3)  # 0-d array: wow()'s noise-map branch
    assert B.wow_eligible(f32, 4, noise_per_frame=[None, 0.0, np.float32(2)])
    assert not B.wow_eligible([f32[0], f32[1]], 4)                          # not stacked
    assert not B.wow_eligible(np.zeros((3, 64, 200000), np.float32), 4)     # rows too wide for the fused passes

    class Retapped(W.B3spline):
        coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9
    assert not B.wow_eligible(f32, 4, Retapped)

    class Custom(W.AbstractScalingFunction):
        coefficients_1d = np.array([0.2, 0.6, 0.2])

        def __init__(self, n_dim):
            super().__init__("custom", n_dim)
    assert not B.wow_eligible(f32, 4, Custom)


def test_batch_eligible_keeps_its_answers():
    f32 = np.zeros((3, 64, 80), np.float32)
    assert B.batch_eligible(f32, 6) and B.batch_eligible(f32, 8, W.Triangle)
    assert not B.batch_eligible(f32, 1) and not B.batch_eligible(f32, 9)
    assert not B.batch_eligible(f32, 6, bilateral=1)
    assert B.batch_eligible(f32, 6, noise_per_frame=[None, 0.5, np.float32(2)])


def test_n_scales_resolution_is_wows():
    # ref:122-127: log2(min side) - log2(taps), None -> that (h < 1) or len(denoise_coefficients) (h >= 1)
    assert U._wow_n_scales((2048, 2048), W.B3spline, None, 0, []) == 9
    assert U._wow_n_scales((4096, 4096), W.B3spline, None, 0, []) == 10
    assert U._wow_n_scales((512, 512), W.Triangle, None, 0, []) == 7
    assert U._wow_n_scales((300, 517), W.B3spline, None, 0, []) == 6
    assert U._wow_n_scales((512, 512), W.B3spline, None, 1, [5, 2]) == 2
    assert U._wow_n_scales((512, 512), W.B3spline, 12, 0, []) == 7
    assert U._wow_n_scales((512, 512), W.B3spline, 3, 0, []) == 3
    # ref:135-138: denoise_coefficients at least as long as the sigma_e table cap n_scales, with the warning
    n = len(W.B3spline(2).sigma_e())
    with pytest.warns(UserWarning, match="maximum for scaling"):
        assert U._wow_scale_limit(4, W.B3spline, 2, None, [1] * n) == n
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert U._wow_scale_limit(4, W.B3spline, 2, None, [5, 2]) == 4


def _fake_wow(calls):
    """a stand-in for utils.wow: records its arguments, returns (frame * 2, coefficients-like)"""
    class Coef:
        def __init__(self, f):
            self.data = np.stack([f, -f])

    def fake(data, scaling_function=W.B3spline, n_scales=None, *args, **kw):
        calls.append(dict(kw, n_scales=n_scales, scaling_function=scaling_function))
        return data * 2, Coef(data)
    return fake


def test_fallback_runs_the_per_frame_loop_with_each_frames_noise(monkeypatch):
    calls = []
    monkeypatch.setattr(B, "wow", _fake_wow(calls))
    fr = np.arange(3 * 8 * 8, dtype=np.float64).reshape(3, 8, 8)           # float64: not a batch case
    img = B.wow_stack(fr, noise=[1.0, None, 0], denoise_coefficients=[5, 2], h=0.5, gamma=2)
    assert img.dtype == np.float64 and np.array_equal(img, fr * 2)
    assert [c["noise"] for c in calls] == [1.0, None, 0]
    assert all(c["n_scales"] is None and c["denoise_coefficients"] == [5, 2] and c["h"] == 0.5 and c["gamma"] == 2
               for c in calls)
    calls.clear()
    out = np.empty((3, 8, 8))
    img, planes = B.wow_stack(fr, noise=0.5, bilateral=1, out=out, return_coefficients=True)
    assert img is out and np.array_equal(out, fr * 2)
    assert planes.shape == (3, 2, 8, 8) and np.array_equal(planes[:, 1], -fr)
    assert [c["noise"] for c in calls] == [0.5] * 3 and all(c["bilateral"] == 1 for c in calls)
    calls.clear()
    maps = np.ones((8, 8))                                                  # a noise map: per frame, the map each time
    B.wow_stack(fr.astype(np.float32), noise=maps)
    assert len(calls) == 3 and all(c["noise"] is maps for c in calls)


def test_batched_path_resolves_n_scales_once(monkeypatch):
    seen = []

    def elig(frames, n_scales, *a, **k):
        seen.append(n_scales)
        return False
    monkeypatch.setattr(B, "wow_eligible", elig)
    monkeypatch.setattr(B, "wow", _fake_wow([]))
    B.wow_stack(np.zeros((2, 2048, 16), np.float32))
    B.wow_stack(np.zeros((2, 64, 64), np.float32), n_scales=9)
    B.wow_stack(np.zeros((2, 64, 64), np.float32), h=1, denoise_coefficients=[5, 2, 1])
    assert seen == [2, 4, 3]
    n = len(W.B3spline(2).sigma_e())
    with pytest.warns(UserWarning, match="maximum for scaling"):
        B.wow_stack(np.zeros((2, 8, 8), np.float32), denoise_coefficients=[1] * n)
    assert seen[-1] == n


def test_argument_errors_before_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(L, "default_context", boom)
    monkeypatch.setattr(L, "acquire_batch", boom)
    with pytest.raises(ValueError, match="ndim|shape"):
        W.wow_stack(np.zeros((64, 64), np.float32))
    with pytest.raises(ValueError, match="one shape"):
        W.wow_stack([np.zeros((64, 64), np.float32), np.zeros((64, 65), np.float32)])
    with pytest.raises(ValueError, match="one entry per frame"):
        W.wow_stack(np.zeros((3, 64, 64), np.float32), noise=[1.0, 2.0])
    with pytest.raises(ValueError, match="empty"):
        W.wow_stack([])
    with pytest.raises(ValueError, match="out"):
        W.wow_stack(np.zeros((2, 64, 64), np.float32), out=np.zeros((2, 64, 64), np.float64))


def test_wow_lists_and_factor_are_the_reference_rules():
    rw, sdc = U._wow_lists([.5], [5, 2], 3)
    assert rw == [.5, 1, 1, 1] and sdc == [5, 2, 0, 1]                     # ref:160-170
    rw, sdc = U._wow_lists([], [5, 2, 1], 3)
    assert rw == [1, 1, 1, 1] and sdc == [5, 2, 1, 1]
    rw, sdc = U._wow_lists([], [5, 2, 1, 1], 3)
    assert sdc == [5, 2, 1, 1]                                              # (no trailing 1 added: ref:169)
    ft = np.float32
    assert U._wow_needs_moments(3, 3, False, True, 0) and not U._wow_needs_moments(2, 3, False, True, 0)
    assert U._wow_needs_moments(0, 3, True, True, 0) and not U._wow_needs_moments(3, 3, False, True, 1)
    assert U._wow_factor(1, 3, 2, None, 100.0, False, True, 0, ft) == ft(2)
    # last plane, whitened: w / std;  std = 0 -> 1e-15 (ref:187-188)
    m = (10.0, 200.0, 0.0, 0.0)                                             # mean 0.1, E[c^2] 2
    std = ft(np.sqrt(2.0 - 0.01))
    assert U._wow_factor(3, 3, 1, m, 100.0, False, True, 0, ft) == ft(1 / std)
    assert U._wow_factor(3, 3, 1, (0.0, 0.0, 0, 0), 100.0, False, True, 0, ft) == ft(1e15)
    assert U._wow_factor(0, 3, 1, m, 100.0, True, True, 0, ft) == ft(np.sqrt(2.0))   # preserve_variance: rms
    assert U._gamma_range(None, 4.0, (0, 0, -1.0, 9.0)) == (-1.0, 4.0)
    assert U._gamma_range(1.0, 2.0, None) == (1.0, 2.0)


def test_chunking_counts_wows_extra_planes():
    per = L.batch_frame_bytes(512, 512, 7)
    plane = 512 * 512 * 4
    assert L.batch_chunks(10, 512, 512, 7, budget=3 * per) == L.batch_chunks(10, 512, 512, 7, budget=3 * per, extra_planes=0)
    assert [n for _, n in L.batch_chunks(10, 512, 512, 7, budget=3 * per + 2 * plane)] == [3, 3, 3, 1]
    assert [n for _, n in L.batch_chunks(10, 512, 512, 7, budget=3 * per + 2 * plane, extra_planes=2)] == [2] * 5
    assert [n for _, n in L.batch_chunks(10, 512, 512, 7, budget=3 * (per + 2 * plane), extra_planes=2)] == [3, 3, 3, 1]
    assert L.batch_chunks(4, 512, 512, 7, budget=1, extra_planes=2) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    with pytest.raises(ValueError):
        L.batch_chunks(4, 512, 512, 7, extra_planes=-1)


def test_batch_plane_ids_of_wow_are_utils_ids():
    assert U._GAMMA_PLANE == L.PLANE_SCRATCH(4)
