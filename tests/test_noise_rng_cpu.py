"""The seeded normal noise without a GPU: the host mirror of the device generator (wavelets_amd/rng.py) against the
Random123 known-answer vectors, the counter layout as a contract, the statistics of the mirror on exactly the
(n, shape, seed) the GPU statistics test uses, and the host logic of compute_noise_weights(seed=...)."""
import numpy as np
import pytest

from wavelets_amd import _lib as L
from wavelets_amd import rng
from wavelets_amd import wavelets as WV

# the case of the statistics tests (here on the mirror, in test_gpu_noise_rng.py on the device): n = 2**20 samples
STAT_N, STAT_SHAPE, STAT_SEED = 16, (256, 256), 20261017
P_3SIGMA = 0.0026998              # P(|z| > 3) of a standard normal


def normal_stats(z):
    """[(name, |statistic|, bound)] of an (n, H, W) stack that claims to be standard normal white noise: every bound
    is 5 standard errors of the estimator under that null"""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    zc = z - z.mean()
    v = (zc * zc).mean()
    se = 1.0 / np.sqrt(n)
    return [("mean", abs(z.mean()), 5 * se),
            ("var - 1", abs(z.var() - 1.0), 5 * np.sqrt(2.0 / n)),
            ("lag-1 along x", abs((zc[:, :, 1:] * zc[:, :, :-1]).mean() / v), 5 * se),
            ("lag-1 along y", abs((zc[:, 1:] * zc[:, :-1]).mean() / v), 5 * se),
            ("lag-1 between frames", abs((zc[1:] * zc[:-1]).mean() / v), 5 * se),
            ("share beyond 3 sigma", abs((np.abs(z) > 3.0).mean() - P_3SIGMA), 5 * np.sqrt(P_3SIGMA * (1 - P_3SIGMA) / n))]


def assert_normal_stats(z):
    for name, got, bound in normal_stats(z):
        print(f"{name}: {got:.3e} (bound {bound:.3e})")
        assert got <= bound, f"{name}: {got:.3e} > {bound:.3e}"


KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,expected", KAT)
def test_philox_known_answers(ctr, key, expected):
    got = rng.philox4x32(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert " ".join(f"{int(v):08x}" for v in got) == expected


def test_philox_is_vectorised():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint32)
    key = np.array([k[1] for k in KAT], dtype=np.uint32)
    got = rng.philox4x32(ctr, key)
    for row, (_, _, expected) in zip(got, KAT):
        assert " ".join(f"{int(v):08x}" for v in row) == expected
    # one key for many counters
    many = rng.philox4x32(np.zeros((3, 2, 4), dtype=np.uint32), np.zeros(2, dtype=np.uint32))
    assert many.shape == (3, 2, 4) and (many == got[0]).all()


def test_mirror_follows_the_counter_layout():
    """pixel (y, x) of trial t is word (x & 3) of Philox(counter (x >> 2, y, t, 0), key (seed lo, seed hi)) through
    the bits -> uniform map and Box-Muller, pairs (r0, r1) -> x, x + 1 and (r2, r3) -> x + 2, x + 3"""
    seed = (0x12345678 << 32) | 0x9abcdef0
    z = rng.normal_frames_host(2, (3, 10), seed, first_trial=5)
    assert z.dtype == np.float32 and z.shape == (2, 3, 10)
    for f, y, x in [(0, 0, 0), (1, 2, 9), (0, 1, 6), (1, 0, 5)]:
        r = rng.philox4x32(np.array([x >> 2, y, 5 + f, 0], dtype=np.uint32), np.array([0x9abcdef0, 0x12345678], dtype=np.uint32))
        pair = r[2 * ((x & 3) // 2):][:2]
        u = [(np.float32(int(b) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24) for b in pair]
        rad, ang = np.sqrt(-2.0 * np.log(np.float64(u[0]))), 2.0 * np.pi * np.float64(u[1])
        want = np.float32(rad * (np.sin(ang) if x & 1 else np.cos(ang)))
        assert z[f, y, x] == want, (f, y, x)


def test_mirror_layout_contract():
    seed, s = 77, (9, 14)
    stack = rng.normal_frames_host(3, s, seed)
    assert np.array_equal(stack[2], rng.normal_frames_host(1, s, seed, first_trial=2)[0])
    assert np.array_equal(rng.normal_frames_host(1, (5, 7), seed)[0], rng.normal_frames_host(1, (5, 8), seed)[0][:, :7])
    assert np.array_equal(rng.normal_frames_host(1, (4, 8), seed)[0], rng.normal_frames_host(1, (5, 8), seed)[0][:4])
    assert not np.array_equal(stack, rng.normal_frames_host(3, s, seed + 1))
    assert not np.array_equal(stack, rng.normal_frames_host(3, s, seed + (1 << 32)))     # the high word is part of the key
    assert not np.array_equal(stack[0], stack[1])
    assert np.isfinite(stack).all()


@pytest.mark.parametrize("call", [rng.normal_frames_host, rng.normal_frames])
def test_argument_errors(call):
    """refused before any device work"""
    for bad in [dict(n=0), dict(n=-1), dict(shape=(4,)), dict(shape=(2, 3, 4)), dict(shape=5), dict(shape=(0, 4)),
                dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(first_trial=-1), dict(first_trial=(1 << 32) - 1)]:
        kw = dict(n=2, shape=(4, 4), seed=1, first_trial=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            call(**kw)


def test_mirror_statistics_of_the_gpu_case():
    """the seed of the GPU statistics test lies inside every one of its bounds on the mirror"""
    assert STAT_N * STAT_SHAPE[0] * STAT_SHAPE[1] == 1 << 20
    assert_normal_stats(rng.normal_frames_host(STAT_N, STAT_SHAPE, STAT_SEED))


# ---------------------------------------------------------------------------- compute_noise_weights: host logic
class _FakePlan:
    H, W = 4, 6

    def reduce(self, s):
        return (2.0 * (s + 1), 30.0 * (s + 1), 0.0, 0.0)


class _FakeCoefficients:
    def _device(self):
        return _FakePlan()


def _raiser(name):
    def f(*a, **k):
        raise AssertionError(f"rng.{name} reached")
    return f


def test_seed_none_is_the_host_path(monkeypatch):
    """seed=None: np.random.normal frames of the reference's side, one transform per trial, nothing of rng"""
    for name in ("philox4x32", "normal_frames_host", "normal_frames"):
        monkeypatch.setattr(rng, name, _raiser(name))
    drawn, seen = [], []

    def normal(*a, size=None, **k):
        drawn.append(size)
        return np.zeros(size)

    class Transform:
        def __init__(self, cls, bilateral=None):
            seen.append(("init", cls, bilateral))

        def __call__(self, data, level):
            seen.append(("call", data.dtype, data.shape, level))
            return _FakeCoefficients()

    monkeypatch.setattr(np.random, "normal", normal)
    monkeypatch.setattr(WV, "AtrousTransform", Transform)
    got = WV.B3spline(2).compute_noise_weights(2, n_trials=3, bilateral=1)
    assert drawn == [(44, 44)] * 3
    assert seen == [("init", WV.B3spline, 1)] + [("call", np.dtype(np.float32), (44, 44), 2)] * 3
    npix = 24.0
    want = [np.sqrt(30.0 * (s + 1) / npix - (2.0 * (s + 1) / npix) ** 2) for s in range(2)]
    np.testing.assert_array_equal(got, np.array(want) * 3 / 3)
    # ... and as the default
    drawn.clear()
    WV.Triangle(2).compute_noise_weights(1, 2)
    assert drawn == [(22, 22)] * 2


class _FakeBatch:
    def __init__(self, log, n):
        self.log, self.n = log, n

    def fill_normal(self, nf, plane, seed, first_trial=0):
        self.trials = list(range(first_trial, first_trial + nf))
        self.log.append(("fill_normal", nf, plane, seed, first_trial))

    def decompose(self, nf, src, level, flags):
        self.log.append(("decompose", nf, src, level, flags))

    def decompose_bilateral(self, nf, src, level, sb):
        self.log.append(("decompose_bilateral", nf, src, level, list(sb)))

    def reduce(self, nf, plane):
        # moments that tell trials and scales apart: std = sqrt(tot2 / npix) = (trial + 1) * (scale + 1)
        return [(0.0, float(self.npix) * ((t + 1) * (plane + 1)) ** 2, 0.0, 0.0) for t in self.trials[:nf]]


@pytest.mark.parametrize("bilateral", [None, 1])
def test_seeded_images_run_in_chunks_on_one_batch(monkeypatch, bilateral):
    """built-in family, image: one BatchPlan, per chunk fill_normal(first_trial = f0) -> transform -> reduce per
    scale, nothing uploaded or downloaded; trial t contributes in trial order"""
    log, made, released = [], [], []
    for name in ("normal_frames_host", "normal_frames"):
        monkeypatch.setattr(rng, name, _raiser(name))
    monkeypatch.setattr(np.random, "normal", _raiser("np.random.normal"))
    side, level, trials = 44, 2, 5
    frame = L.batch_frame_bytes(side, side, level)
    monkeypatch.setattr(L, "BATCH_BYTES", 2 * frame + 8)               # two frames per chunk: 2 + 2 + 1

    def acquire(ctx, n, H, W, family, max_level):
        made.append((n, H, W, family, max_level))
        b = _FakeBatch(log, n)
        b.npix = H * W
        return b

    monkeypatch.setattr(L, "acquire_batch", acquire)
    monkeypatch.setattr(L, "release_batch", released.append)
    monkeypatch.setattr(WV, "default_context", lambda: None)
    got = WV.B3spline(2).compute_noise_weights(level, trials, bilateral, seed=99)
    assert made == [(2, side, side, L.B3SPLINE, level)] and len(released) == 1
    step = ("decompose_bilateral", L.PLANE_INPUT, level, [1, 1, 1]) if bilateral else ("decompose", L.PLANE_INPUT, level, L.FLAG_FUSED)
    want = []
    for f0, nf in [(0, 2), (2, 2), (4, 1)]:
        want += [("fill_normal", nf, L.PLANE_INPUT, 99, f0), (step[0], nf) + step[1:]]
    assert log == want
    np.testing.assert_allclose(got, [np.mean([(t + 1) * (s + 1) for t in range(trials)]) for s in range(level)], rtol=1e-15)


def test_seeded_signals_and_cubes_take_the_mirror_over_the_flat_index(monkeypatch):
    """n_dim 1 / 3: frame t is the mirror's field over the flattened index, counter (i >> 2, 0, t, 0)"""
    monkeypatch.setattr(rng, "normal_frames", _raiser("normal_frames"))
    monkeypatch.setattr(np.random, "normal", _raiser("np.random.normal"))
    for nd, level in ((1, 2), (3, 1)):
        frames = []

        class Transform:
            def __init__(self, cls, bilateral=None):
                pass

            def __call__(self, data, lev):
                frames.append(np.array(data))
                return _FakeCoefficients()

        monkeypatch.setattr(WV, "AtrousTransform", Transform)
        WV.B3spline(nd).compute_noise_weights(level, 2, seed=5)
        side = 11 * 2 ** level
        assert [f.shape for f in frames] == [(side,) * nd] * 2
        for t, f in enumerate(frames):
            assert f.dtype == np.float32
            assert np.array_equal(f.ravel(), rng.normal_frames_host(1, (1, side ** nd), 5, first_trial=t)[0, 0])


def test_seed_is_validated():
    for bad in (-1, 1 << 64, 2.0, "7", True):
        with pytest.raises(ValueError):
            WV.B3spline(2).compute_noise_weights(2, 2, seed=bad)
