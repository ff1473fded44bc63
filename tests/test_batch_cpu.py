"""Host logic of the batched engine (wavelets_amd.batch, _lib.batch_chunks): chunk planning, the eligibility /
fallback predicate, and argument errors raised before any device work.  No GPU needed."""
import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B


def test_chunk_planner_memory_budget_and_last_short_chunk():
    per = L.batch_frame_bytes(512, 512, 6)
    assert per == (6 + 5) * 512 * 512 * 4
    assert L.batch_chunks(10, 512, 512, 6, budget=3 * per) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert L.batch_chunks(64, 512, 512, 6, budget=64 * per) == [(0, 64)]
    # a budget below one frame still makes progress, one frame at a time
    assert L.batch_chunks(3, 512, 512, 6, budget=1) == [(0, 1), (1, 1), (2, 1)]
    # the pitch is the plan's: rows padded to 4 pixels
    assert L.batch_frame_bytes(300, 517, 5) == 10 * 300 * 520 * 4
    assert L.batch_chunks(0, 8, 8, 2) == []


def test_chunk_planner_grid_limit():
    big = 10 ** 15
    ch = L.batch_chunks(70000, 16, 16, 2, budget=big)
    assert [n for _, n in ch] == [L.BATCH_MAX_FRAMES, 70000 - L.BATCH_MAX_FRAMES]
    assert sum(n for _, n in ch) == 70000 and ch[1][0] == L.BATCH_MAX_FRAMES
    assert L.batch_chunks(5, 16, 16, 2, budget=big, max_frames=2) == [(0, 2), (2, 2), (4, 1)]


def test_eligibility_predicate():
    f32 = np.zeros((3, 64, 80), np.float32)
    assert B.batch_eligible(f32, 6)
    assert B.batch_eligible(f32, 2, W.Triangle) and B.batch_eligible(f32, 8, W.Triangle)
    assert not B.batch_eligible(f32.astype(np.float64), 6)                 # float64: per frame
    assert not B.batch_eligible(f32.astype(">f4"), 6)                       # byte-swapped
    assert not B.batch_eligible(f32, 1) and not B.batch_eligible(f32, 9)   # no all-fused schedule
    assert not B.batch_eligible(f32, 6, bilateral=1)
    assert not B.batch_eligible(f32, 6, noise_per_frame=None)              # ndarray noise map
    assert not B.batch_eligible(f32, 6, noise_per_frame=[np.ones((64, 80))] * 3)
    assert B.batch_eligible(f32, 6, noise_per_frame=[None, 0.5, np.float32(2)])
    assert not B.batch_eligible([f32[0], f32[1]], 6)                        # not stacked

    class Retapped(W.B3spline):
        coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9

    class Even(W.AbstractScalingFunction):
        coefficients_1d = np.array([0.5, 0.5])

        def __init__(self, n_dim):
            super().__init__("even", n_dim)

    assert not B.batch_eligible(f32, 6, Retapped)
    assert not B.batch_eligible(f32, 6, Even)
    assert not B.batch_eligible(np.zeros((3, 64, 200000), np.float32), 6)  # rows too wide for the fused passes


def test_noise_list():
    assert B._noise_list(None, 3) == [None] * 3
    assert B._noise_list(0.5, 2) == [0.5, 0.5]
    assert B._noise_list([1, None], 2) == [1, None]
    assert B._noise_list(np.ones((4, 4)), 2) is None
    assert B._noise_list(np.array([0.5, 2.0]), 2) == [0.5, 2.0]          # a 1-D array: one level per frame
    with pytest.raises(ValueError, match="one entry per frame"):
        B._noise_list([1, 2, 3], 2)


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(L, "default_context", boom)
    monkeypatch.setattr(L, "acquire_batch", boom)


def test_argument_errors_before_device_work(monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="ndim|shape"):
        W.transform_stack(np.zeros((64, 64), np.float32), 3)
    with pytest.raises(ValueError, match="ndim|shape"):
        W.denoise_stack(np.zeros((2, 2, 64, 64), np.float32), [5, 3])
    with pytest.raises(ValueError, match="one shape"):
        W.transform_stack([np.zeros((64, 64), np.float32), np.zeros((64, 65), np.float32)], 3)
    with pytest.raises(ValueError, match="2-D"):
        W.denoise_stack([np.zeros((64, 64), np.float32), np.zeros(64, np.float32)], [5, 3])
    with pytest.raises(ValueError, match="one entry per frame"):
        W.denoise_stack(np.zeros((3, 64, 64), np.float32), [5, 3], noise=[1.0, 2.0])
    with pytest.raises(ValueError, match="empty"):
        W.transform_stack([], 3)
    with pytest.raises(ValueError, match="out"):
        W.transform_stack(np.zeros((2, 64, 64), np.float32), 3, out=np.zeros((2, 3, 64, 64), np.float32))
    with pytest.raises(ValueError, match="out"):
        W.denoise_stack(np.zeros((2, 64, 64), np.float32), [5, 3], out=np.zeros((2, 64, 64), np.float64))


def test_interleave_split_is_the_per_frame_decision():
    from wavelets_amd.wavelets import _interleave_split
    sched = L.schedule(L.B3SPLINE, 5, True)           # (0, 3), (3, 2)
    entries, k, covered = _interleave_split(sched, 5, [4, 2, 1, 0, 0], (1,) * 5)
    assert (k, covered) == (1, 3) and len(entries) == 5
    assert _interleave_split(L.schedule(L.B3SPLINE, 2, True), 2, [5, 3], (1, 1))[1:] == (1, 2)   # whole schedule
    assert _interleave_split([], 2, [5, 3], (1, 1))[1:] == (0, 0)


def test_scalar_tau_rules():
    from wavelets_amd.wavelets import _scalar_tau
    assert _scalar_tau(5, 0, 0.9) is None
    assert _scalar_tau(5, 2.0, 0.5) == (5.0, L.PLANE_NONE)
    assert _scalar_tau(-5, 2.0, 0.5, soft=True) == (5.0, L.PLANE_NONE)
    assert _scalar_tau(-5, 2.0, 0.5, soft=False) is None
