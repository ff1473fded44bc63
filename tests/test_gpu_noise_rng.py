"""The seeded normal fill on the MI355X (wt_fill_normal / wt_batch_fill_normal, csrc/wt_rng.h) and
compute_noise_weights(seed=...) on top of it.

Device against the host mirror (rng.normal_frames_host: the same bits and uniforms, Box-Muller in float64): the
error measure is max |device - mirror| / max(1, |mirror|).  Measured on MI355X over the shapes of DEVICE_SHAPES:
MEASURED_ERR below (1.28e-6, at (9, 258); 1.19e-6 at (88, 88), 1.07e-6 at (33, 31)); asserted 4 x that (the convention of tests/conftest.py).  A mix-up of counter words, key words
or pair order gives differences of order 1, so the asserted bound must itself stay below 1e-5 - a condition on the
bound, not a tolerance."""
import numpy as np
import pytest

from conftest import load_golden
from test_noise_rng_cpu import STAT_N, STAT_SHAPE, STAT_SEED, assert_normal_stats

pytestmark = pytest.mark.gpu

MEASURED_ERR = 1.2815e-06          # max |device - mirror| / max(1, |mirror|) over DEVICE_SHAPES, MI355X
DEVICE_BOUND = 4 * MEASURED_ERR
DEVICE_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (33, 31), (64, 9), (9, 258), (88, 88)]
SEED = (0xC0FFEE << 32) | 0x5EED1234       # both key words in use


@pytest.fixture(scope="module")
def W():
    import wavelets_amd
    return wavelets_amd


@pytest.fixture(scope="module")
def L():
    from wavelets_amd import _lib
    return _lib


@pytest.mark.parametrize("shape", DEVICE_SHAPES)
def test_device_matches_the_mirror(W, shape):
    from wavelets_amd import rng
    got = W.normal_frames(3, shape, SEED)
    ref = rng.normal_frames_host(3, shape, SEED)
    assert got.dtype == np.float32 and got.shape == (3,) + shape
    err = float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"normal_frames {shape}: max |device - mirror| / max(1, |z|) = {err:.4e}")
    assert DEVICE_BOUND < 1e-5
    assert err <= DEVICE_BOUND, f"{shape}: {err:.3e} > {DEVICE_BOUND:.3e}"


def test_nothing_else_is_written(L):
    """fill_normal(nf=2) on a batch of 4: the other frames of the plane and every other plane keep their bits"""
    H, Wd, level = 33, 31, 2
    sentinel = np.float32(-1234.5)
    bp = L.BatchPlan(L.default_context(), 4, H, Wd, L.B3SPLINE, level)
    try:
        planes = list(range(level + 1)) + [L.PLANE_INPUT, L.PLANE_OUT] + [L.PLANE_SCRATCH(i) for i in (0, 1, 3, 4)]
        for p in planes:
            bp.fill(4, p, sentinel)
        bp.fill_normal(2, L.PLANE_INPUT, SEED, 0)
        got = bp.download(L.PLANE_INPUT, 4)
        assert (got[2:] == sentinel).all()
        assert not (got[:2] == sentinel).any()
        for p in planes:
            if p != L.PLANE_INPUT:
                assert (bp.download(p, 4) == sentinel).all(), p
    finally:
        bp.close()


def test_layout_contract_on_the_device(W, L):
    shape = (33, 31)
    a = W.normal_frames(5, shape, SEED)
    assert np.array_equal(a, W.normal_frames(5, shape, SEED))
    assert np.array_equal(a[3], W.normal_frames(1, shape, SEED, first_trial=3)[0])
    assert not np.array_equal(a, W.normal_frames(5, shape, SEED + 1))
    # a wt_plan of the same shape (its own pitch and allocation): trial f is frame f
    plan = L.Plan(L.default_context(), shape[0], shape[1], L.TRIANGLE, 1)
    try:
        for f in (0, 4):
            plan.fill_normal(L.PLANE_INPUT, SEED, f)
            assert np.array_equal(plan.download(L.PLANE_INPUT), a[f]), f
    finally:
        plan.close()
    # a narrower frame is the left part of a wider one, a shorter one the top
    assert np.array_equal(W.normal_frames(1, (33, 29), SEED)[0], a[0][:, :29])
    assert np.array_equal(W.normal_frames(1, (20, 31), SEED)[0], a[0][:20])


def test_chunked_stack_equals_one_chunk(W, L, monkeypatch):
    shape, n = (40, 50), 7
    whole = W.normal_frames(n, shape, SEED, first_trial=2)
    monkeypatch.setattr(L, "BATCH_BYTES", 3 * L.batch_frame_bytes(shape[0], shape[1], 0) + 8)
    assert [nf for _, nf in L.batch_chunks(n, shape[0], shape[1], 0)] == [3, 3, 1]
    out = np.empty((n,) + shape, dtype=np.float32)
    assert W.normal_frames(n, shape, SEED, first_trial=2, out=out) is out
    assert np.array_equal(out, whole)


def test_statistics(W):
    assert_normal_stats(W.normal_frames(STAT_N, STAT_SHAPE, STAT_SEED))


CASES = [(fam, bil, lev) for fam in ("B3spline", "Triangle") for bil in (None, 1) for lev in (3, 4)]


@pytest.mark.parametrize("family,bilateral,level", CASES)
def test_noise_weights_equal_the_per_trial_loop(W, L, family, bilateral, level):
    """the batched route, to the last bit of the accumulated doubles, is the loop over public pieces"""
    sf = getattr(W, family)
    trials, seed = 8, SEED + level
    got = sf(2).compute_noise_weights(level, trials, bilateral, seed=seed)
    side = len(sf.sigma_e_1d) * 2 ** level
    frames = W.normal_frames(trials, (side, side), seed)
    std = np.zeros(level)
    for t in range(trials):
        plan = W.AtrousTransform(sf, bilateral)(frames[t], level)._device()
        for s in range(level):
            tot, tot2, _, _ = plan.reduce(s)
            std[s] += np.sqrt(max(tot2 / side ** 2 - (tot / side ** 2) ** 2, 0.0))
    assert np.array_equal(got, std / trials), (got, std / trials)
    # reproducible, and the seed matters
    assert np.array_equal(got, sf(2).compute_noise_weights(level, trials, bilateral, seed=seed))
    assert not np.array_equal(got, sf(2).compute_noise_weights(level, trials, bilateral, seed=seed + 1))


def test_noise_weights_chunked_equal_one_chunk(W, L, monkeypatch):
    sf, level, trials = W.B3spline, 3, 5
    whole = sf(2).compute_noise_weights(level, trials, seed=SEED)
    monkeypatch.setattr(L, "BATCH_BYTES", 2 * L.batch_frame_bytes(88, 88, level) + 8)
    assert np.array_equal(whole, sf(2).compute_noise_weights(level, trials, seed=SEED))


def test_noise_weights_of_user_defined_taps(W, L):
    """a scaling function the batch predicates refuse: a plan per trial, Plan.fill_normal making the frame"""
    class Binomial7(W.AbstractScalingFunction):
        coefficients_1d = np.array([1, 6, 15, 20, 15, 6, 1]) / 64
        sigma_e_1d = np.ones(3)                      # (its length sets the side: 3 * 2**n_scales)

        def __init__(self, *a, **k):
            super().__init__('binomial7', *a, **k)

    level, trials = 3, 4
    got = Binomial7(2).compute_noise_weights(level, trials, seed=SEED)
    frames = W.normal_frames(trials, (24, 24), SEED)
    std = np.zeros(level)
    for t in range(trials):
        planes = W.AtrousTransform(Binomial7)(frames[t], level).data
        std += [np.std(planes[s].astype(np.float64)) for s in range(level)]
    np.testing.assert_allclose(got, std / trials, rtol=1e-12)


@pytest.mark.parametrize("family,bilateral,level", CASES)
def test_noise_weights_against_the_oracle_fixture(W, family, bilateral, level):
    """64 seeded trials against the C oracle's 400 np.random trials of the same side (g25_noise_weights.npz,
    tests/golden/make_noise_weights_golden.py): |device - m| <= 5 d sqrt(1/64 + 1/400), m and d from the oracle"""
    g = load_golden("g25_noise_weights")
    key = f"{family.lower()}_{'plain' if bilateral is None else 'bil'}_L{level}"
    m, d, t0 = g[key + "_m"], g[key + "_d"], int(g["T0"])
    trials = 64
    got = getattr(W, family)(2).compute_noise_weights(level, trials, bilateral, seed=SEED)
    bound = 5 * d * np.sqrt(1 / trials + 1 / t0)
    print(key, "device", got, "oracle", m, "|diff| / bound", np.abs(got - m) / bound)
    assert (np.abs(got - m) <= bound).all(), (key, got, m, bound)
