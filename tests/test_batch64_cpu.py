"""Host logic of the float64 batch (wt_batch64: transform_stack / denoise_stack on the stacks the reference computes
in float64) and what tests/test_gpu_batch64.py rests on, checked without a device: the eligibility predicate
batch64_eligible (and the three older predicates, unchanged on the same inputs), argument errors raised before any
device work, chunking by 8-byte planes, and the input premise of the hard-threshold comparisons - no thresholded
coefficient of the float64 numpy oracle lies within 1e-10 (relative) of its threshold, so those comparisons leave no
sample out.  The GPU module imports its inputs from here."""
import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B
from oracle import atrous_numpy as O
from test_stack_edges_cpu import SHAPES, FAMILIES, AMPS, OFFSETS, DENOISE_WEIGHTS, noise_modes, per_frame_noise

TRUE_TYPES = [np.float64, ">f8", ">f4", np.int16, np.uint16, np.int32, np.uint32, np.int64]
FALSE_TYPES = [np.float32, np.uint8, np.int8, np.bool_]
ROUTE_TYPES = [np.float64, np.int16, np.uint16, np.int32, ">f4", ">f8"]      # the GPU module's batched-route check
PLANES_TOL = 1e-12              # tests/test_gpu_parity.py, float64 transform: times max|frame|
DENOISE64_TOL = 1e-12           # tests/test_gpu_round3.py, float64 denoise([5, 3, 2]): times max|frame|
HARD_MARGIN = 1e-10             # the premise: every thresholded |w| at least this far (relative) from its threshold
DTYPE_SHAPE = (33, 31)
ANSCOMBE_SHAPES = [(33, 31), (64, 9), (300, 517)]


def hostile_stack64(shape, n=9, seed=0):
    """n float64 frames of `shape`, neighbouring frames nine decades apart (as test_stack_edges_cpu.hostile_stack,
    in float64); the first k frames of the n-frame stack are the k-frame stack"""
    rng = np.random.default_rng([seed, 64, shape[0], shape[1]])
    fr = rng.standard_normal((n,) + tuple(shape))
    for i in range(n):
        fr[i] = fr[i] * AMPS[i % 2] + OFFSETS[i % 3] * AMPS[i % 2]
    return fr


def typed_stack(dtype, shape=DTYPE_SHAPE, n=3, seed=0):
    """n frames of `dtype` whose values use that type's range (int32 above 2**24, int64 up to 2**53: exact in float64
    only); the frames alternate between loud and quiet where the type allows it"""
    rng = np.random.default_rng([seed, 11, shape[0], shape[1]])
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return hostile_stack64(shape, n, seed).astype(dt)
    out = []
    for i in range(n):
        if dt == np.int16:
            f = rng.integers(-30000, 30001, shape) if i % 2 == 0 else rng.integers(-3, 4, shape)
        elif dt == np.uint16:
            f = rng.poisson(100 if i % 2 == 0 else 3, shape)
        elif dt == np.int32:
            f = rng.integers(2 ** 24, 2 ** 30, shape) * (1 if i % 2 == 0 else -1)
        elif dt == np.uint32:
            f = rng.integers(2 ** 24, 2 ** 32, shape, dtype=np.uint64)
        elif dt == np.int64:
            f = rng.integers(-2 ** 53, 2 ** 53, shape)
        else:
            raise ValueError(dt)
        out.append(f.astype(dt))
    return np.stack(out)


def hard_margin(frame64, weights, fam, noise):
    """min over the thresholded coefficients of | |w| - tau | / tau in the float64 oracle's denoise (hard threshold);
    inf when nothing is thresholded"""
    c = O.Coeffs(O.atrous_standard(np.array(frame64, np.float64), len(weights), fam.lower()), fam.lower())
    c.noise = noise
    worst = np.inf
    for s, sig in enumerate(weights):
        if sig == 0:
            continue
        if c.noise is None:
            c.noise = c.get_noise()                               # (lazy, as the reference: plane 0 is untouched here)
        if c.noise == 0:
            continue
        tau = sig * c.noise * c.sigma_e[s]
        worst = min(worst, float((np.abs(np.abs(c.data[s]) - abs(tau)) / abs(tau)).min()))
    return worst


def hard_cases():
    """(label, frames as float64, fam, weights, per-frame noise) of every hard-threshold comparison of the GPU module"""
    for shape in SHAPES:
        fr = hostile_stack64(shape)
        for fam in FAMILIES:
            for weights in DENOISE_WEIGHTS:
                for mode, noise in noise_modes(len(fr)):
                    yield f"{shape} {fam} {weights} {mode}", fr, fam, weights, per_frame_noise(noise, len(fr))
    for dt in ROUTE_TYPES + [np.uint32, np.int64]:
        fr = typed_stack(dt).astype(np.float64)
        for fam in FAMILIES:
            for weights in DENOISE_WEIGHTS:
                for noise in (None, 0.8):
                    yield f"{np.dtype(dt).str} {fam} {weights} {noise}", fr, fam, weights, [noise] * len(fr)


# ---------------------------------------------------------------- the predicate

def test_batch64_predicate_truth_table():
    shape = (3, 64, 80)
    for dt in TRUE_TYPES:
        fr = np.zeros(shape, dt)
        assert B.batch64_eligible(fr, 6), dt
        assert B.batch64_eligible(fr, 2, W.Triangle) and B.batch64_eligible(fr, 8, W.Triangle), dt
        assert B.batch64_eligible(fr, 5, noise_per_frame=[None, 0.5, np.float64(2)]), dt
    for dt in FALSE_TYPES:
        assert not B.batch64_eligible(np.zeros(shape, dt), 6), dt
    f64 = np.zeros(shape)
    assert not B.batch64_eligible(f64, 6, bilateral=1)

    class Retapped(W.B3spline):
        coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9

    class Even(W.AbstractScalingFunction):
        coefficients_1d = np.array([0.5, 0.5])

        def __init__(self, n_dim):
            super().__init__("even", n_dim)

    assert not B.batch64_eligible(f64, 6, Retapped) and not B.batch64_eligible(f64, 6, Even)
    # levels outside the float64 all-fused range (1: a single-scale pass without a fused kernel; from 9 on:
    # single-scale passes at D >= 256)
    for level in (0, 1, 9, 10, 25):
        assert not B.batch64_eligible(f64, level), level
    assert not B.batch64_eligible(f64, 6, noise_per_frame=[np.ones((64, 80))] * 3)      # 2-D noise maps
    assert not B.batch64_eligible(f64, 6, noise_per_frame=None)                         # one noise map for all
    assert not B.batch64_eligible([f64[0], f64[1]], 6)                                   # not stacked
    assert not B.batch64_eligible(np.zeros((1, 2, 100000)), 6)       # rows too wide for the fused passes at 8 bytes
    assert B.batch64_eligible(np.zeros((1, 2, 80000)), 6)
    assert not B.batch64_eligible(np.zeros((2, 1, 64)), 6)          # one-row frames: signals for the float64 engine
    assert B.batch64_eligible(np.zeros((2, 2, 3)), 6) and B.batch64_eligible(np.zeros((2, 513, 6)), 8)
    assert not B.batch64_eligible(np.zeros((3, 64, 80), ">i2"), 6)  # big-endian int16 is served in float32
    assert not B.batch64_eligible(np.zeros((3, 64, 80)), True)


def test_the_older_predicates_are_unchanged_on_the_same_inputs():
    for dt in TRUE_TYPES + FALSE_TYPES:
        fr = np.zeros((3, 64, 80), dt)
        f32 = np.dtype(dt) == np.float32
        assert B.batch_eligible(fr, 6) == f32, dt
        assert B.wow_eligible(fr, 6) == f32, dt
        assert B.bilateral_eligible(fr, 6, bilateral=1) == f32, dt
        assert not B.bilateral_eligible(fr, 6), dt
    assert "batch64_eligible" in B.__all__


def test_float64_all_fused_levels_follow_the_float64_schedule():
    """batch64_eligible's levels are the levels whose float64 schedule is fused passes only (wt_batch64_fused_ok):
    for both families 2..8 at a frame of several rows - the same range as the float32 BATCH_LEVELS today, but derived"""
    for code, fam in ((L.B3SPLINE, W.B3spline), (L.TRIANGLE, W.Triangle)):
        got = [lv for lv in range(0, 26) if L.batch64_fused_ok(code, 64, 80, lv)]
        assert got == list(range(2, 9)), (fam, got)
        assert got == [lv for lv in range(0, 26) if B.batch64_eligible(np.zeros((2, 64, 80)), lv, fam)]


# ---------------------------------------------------------------- chunking and argument errors

def test_chunking_counts_8_byte_planes():
    per4 = L.batch_frame_bytes(512, 512, 6)
    per8 = L.batch_frame_bytes(512, 512, 6, itemsize=8)
    assert per8 == 2 * per4 == (6 + 5) * 512 * 512 * 8
    budget = 16 * per4
    c4 = L.batch_chunks(64, 512, 512, 6, budget=budget)
    c8 = L.batch_chunks(64, 512, 512, 6, budget=budget, itemsize=8)
    assert [n for _, n in c4] == [16] * 4 and [n for _, n in c8] == [8] * 8
    assert L.batch_frame_bytes(300, 517, 5, itemsize=8) == 10 * 300 * 518 * 8        # the pitch of a wt_plan64
    assert L.batch_chunks(70000, 8, 8, 2, budget=10 ** 15, itemsize=8)[0] == (0, L.BATCH_MAX_FRAMES)
    with pytest.raises(ValueError, match="itemsize"):
        L.batch_chunks(4, 8, 8, 2, itemsize=2)


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    for name in ("default_context", "acquire_batch", "acquire_batch64", "BatchPlan64"):
        monkeypatch.setattr(L, name, boom)


def test_argument_errors_before_device_work(monkeypatch):
    _no_device(monkeypatch)
    f64 = np.zeros((3, 64, 64))
    i16 = np.zeros((3, 64, 64), np.int16)
    with pytest.raises(ValueError, match="one entry per frame"):
        W.denoise_stack(f64, [5, 3], noise=[1.0, 2.0])
    with pytest.raises(ValueError, match="one entry per frame"):
        W.denoise_stack(i16, [5, 3], noise=[1.0, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError, match="out"):
        W.transform_stack(f64, 3, out=np.zeros((3, 3, 64, 64)))
    with pytest.raises(ValueError, match="out"):
        W.denoise_stack(i16, [5, 3], out=np.zeros((2, 64, 64), np.float32))
    with pytest.raises(ValueError, match="ndim|shape"):
        W.transform_stack(np.zeros((64, 64)), 3)
    with pytest.raises(ValueError, match="one shape"):
        W.transform_stack([np.zeros((64, 64)), np.zeros((64, 65))], 3)


# ---------------------------------------------------------------- the premise of the GPU module's inputs

def test_typed_stacks_hold_what_they_claim():
    for dt in ROUTE_TYPES + [np.uint32, np.int64]:
        fr = typed_stack(dt)
        assert fr.dtype == np.dtype(dt) and fr.shape == (3,) + DTYPE_SHAPE
        assert B.batch64_eligible(fr, 5)
    assert np.abs(typed_stack(np.int32)).min() > 2 ** 24
    big = typed_stack(np.int64)
    assert np.abs(big).max() > 2 ** 52 and np.abs(big).max() <= 2 ** 53
    assert np.array_equal(big.astype(np.float64).astype(np.int64), big)           # exact in float64
    assert not np.array_equal(big.astype(np.float32).astype(np.int64), big)       # ... and not in float32
    for shape in SHAPES:
        fr = hostile_stack64(shape)
        amax = np.abs(fr).reshape(9, -1).max(axis=1)
        for i in range(1, 9, 2):
            assert amax[i] * 1e7 < min(amax[i - 1], amax[i + 1]), shape


@pytest.mark.parametrize("part", [0, 1, 2, 3])
def test_reference_keeps_every_hard_threshold_sample_clear_of_its_threshold(part):
    """For every input the GPU module compares under hard thresholds: no thresholded coefficient of the float64 oracle
    lies within HARD_MARGIN (relative) of its threshold - a condition on the inputs, evaluated on the reference alone.
    With it a hard-threshold comparison leaves no sample out."""
    worst = np.inf
    for k, (label, fr, fam, weights, noises) in enumerate(hard_cases()):
        if k % 4 != part:
            continue
        for i, (f, n_i) in enumerate(zip(fr, noises)):
            m = hard_margin(f, weights, fam, n_i)
            worst = min(worst, m)
            assert m > HARD_MARGIN, (label, i, m)
    print(f"worst relative margin to a hard threshold: {worst:.3e}")
