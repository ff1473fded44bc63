"""transform_signals / denoise_signals on the GPU: the batched signal engine (wt_signals: a workgroup per signal, the
scales in LDS) against the per-signal loop, bit for bit (np.testing.assert_array_equal), in float32 and float64, both
families - every length at which the kernel takes another path (one sample, fewer samples than a tap's reach, many
bounces of the 'mirror' border, lengths that are no multiple of the 16-byte group or of the workgroup, the LDS budget
and one past it), more workgroups than resident slots, several chunks, even and odd medians - and against the
reference's recorded planes of tests/golden/g11_1d.npz."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FAMS = ("B3spline", "Triangle")
DTYPES = (np.float32, np.float64)
LENGTHS = (1, 2, 3, 5, 17, 255, 256, 257, 1000, 1023)


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


def stack(M, N, dtype, seed=0):
    """M signals of N samples: seeded normal plus an offset, no NaN or inf"""
    rng = np.random.default_rng([seed, M, N])
    return (rng.standard_normal((M, N)) * 3.0 + 10.0).astype(dtype)


def loop_transform(W, sig, level, cls):
    return np.stack([W.AtrousTransform(cls)(s, level).data for s in sig])


def loop_denoise(W, sig, weights, cls, noises, soft):
    return np.stack([W.denoise(s, weights, cls, n, soft_threshold=soft) for s, n in zip(sig, noises)])


def bounce_level(N, hw):
    """the smallest level whose last scale reaches at least 2 N samples: hw * 2**(level - 1) >= 2 * N"""
    level = 1
    while hw * 2 ** (level - 1) < 2 * N:
        level += 1
    return level


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", FAMS)
def test_transform_equals_the_loop(W, fam, dtype):
    from wavelets_amd import signals as S
    cls = getattr(W, fam)
    hw = len(cls.coefficients_1d) // 2
    for N in LENGTHS:
        sig = stack(3, N, dtype, seed=N)
        for level in sorted({1, 3, bounce_level(N, hw)}):
            assert hw * 2 ** (level - 1) >= 2 * N or level in (1, 3)
            assert S.signals_eligible(sig, level, cls)
            got = W.transform_signals(sig, level, cls)
            assert got.dtype == dtype and got.shape == (3, level + 1, N)
            np.testing.assert_array_equal(got, loop_transform(W, sig, level, cls), err_msg=f"{fam} N={N} L={level}")
    sig5 = stack(3, 5, dtype, seed=55)
    np.testing.assert_array_equal(W.transform_signals(sig5, 6, cls), loop_transform(W, sig5, 6, cls))   # level 6 at N = 5


@pytest.mark.parametrize("dtype,N", [(np.float32, 8192), (np.float64, 4096)], ids=("f32", "f64"))
@pytest.mark.parametrize("fam", FAMS)
def test_transform_at_the_budget_and_one_past_it(W, fam, dtype, N):
    from wavelets_amd import signals as S
    cls = getattr(W, fam)
    sig = stack(2, N, dtype, seed=1)
    assert S.signals_eligible(sig, 8, cls)
    np.testing.assert_array_equal(W.transform_signals(sig, 8, cls), loop_transform(W, sig, 8, cls))
    past = stack(2, N + 1, dtype, seed=2)                         # the loop route: still equal
    assert not S.signals_eligible(past, 8, cls)
    np.testing.assert_array_equal(W.transform_signals(past, 8, cls), loop_transform(W, past, 8, cls))


def test_one_signal_many_signals_and_chunks(W, monkeypatch):
    from wavelets_amd import signals as S
    one = stack(1, 300, np.float32, seed=3)
    np.testing.assert_array_equal(W.transform_signals(one, 4), loop_transform(W, one, 4, W.B3spline))
    many = stack(600, 64, np.float32, seed=4)                      # more workgroups than resident slots
    got = W.transform_signals(many, 3)
    np.testing.assert_array_equal(got, loop_transform(W, many, 3, W.B3spline))
    # a stack split into chunks of 2 signals at M = 5: 2 + 2 + 1
    seen = []

    def two_per_chunk(M, N, level, itemsize):
        chunks = [(f0, min(2, M - f0)) for f0 in range(0, M, 2)]
        seen.append(chunks)
        return chunks
    monkeypatch.setattr(S, "_chunks", two_per_chunk)
    for dtype in DTYPES:
        five = stack(5, 257, dtype, seed=5)
        np.testing.assert_array_equal(W.transform_signals(five, 3, W.Triangle), loop_transform(W, five, 3, W.Triangle))
        noises = [None, 0.7, None, 2.0, None]
        np.testing.assert_array_equal(W.denoise_signals(five, [5, 3], W.Triangle, noise=noises),
                                      loop_denoise(W, five, [5, 3], W.Triangle, noises, True))
    assert len(seen) == 4 and all(c == [(0, 2), (2, 2), (4, 1)] for c in seen)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", FAMS)
def test_denoise_equals_the_loop(W, fam, dtype):
    from wavelets_amd import signals as S
    cls = getattr(W, fam)
    for N in (16, 17, 300):                                        # even and odd medians
        sig = stack(4, N, dtype, seed=100 + N)
        sig[2] = 7.25                                              # an all-constant signal: median 0
        M = len(sig)
        mixed = [None, 0.9, None, np.float32(1.5)]
        for weights in ([5, 3], [5, 3, 2, 1], [0, 3, 0]):
            for soft in (True, False):
                for noise, per in ((None, [None] * M), (1.25, [1.25] * M), (mixed, mixed)):
                    assert S.signals_eligible(sig, len(weights), cls, per)
                    got = W.denoise_signals(sig, weights, cls, noise=noise, soft_threshold=soft)
                    assert got.dtype == dtype and got.shape == (M, N)
                    np.testing.assert_array_equal(got, loop_denoise(W, sig, weights, cls, per, soft),
                                                  err_msg=f"{fam} N={N} {weights} soft={soft} noise={noise}")
        out = np.full((M, N), np.nan, dtype)
        assert W.denoise_signals(sig, [5, 3], cls, out=out) is out
        np.testing.assert_array_equal(out, loop_denoise(W, sig, [5, 3], cls, [None] * M, True))
        cube = np.full((M, 3, N), np.nan, dtype)
        assert W.transform_signals(sig, 2, cls, out=cube) is cube
        np.testing.assert_array_equal(cube, loop_transform(W, sig, 2, cls))


def test_against_the_reference_fixture(W):
    """the reference's own planes (tests/golden/g11_1d.npz), at the tolerance tests/test_gpu_parity.py::
    test_one_dimensional_signals uses for these fixtures: 1e-5 * max|signal|"""
    from wavelets_amd import _lib as L
    g = load_golden("g11_1d")
    for n in (300, 17, 5):
        a = g[f"sig_{n}"]
        tol = 1e-5 * np.abs(a).max()
        for fam in FAMS:
            for level in (1, 3, 5):
                got = W.transform_signals(a[None], level, getattr(W, fam))
                assert got.shape == (1, level + 1, n)
                np.testing.assert_allclose(got[0].astype(np.float64), g[f"coef_{fam.lower()}_{n}_L{level}"].astype(np.float64),
                                           rtol=0, atol=tol)
    a = g["sig_300"]
    np.testing.assert_array_equal(W.denoise_signals([a], [5, 3])[0], W.denoise(a, [5, 3]))
    # the level-4 noise of sig_300 through the medians the batch returns
    from wavelets_amd.wavelets import _noise_from_median
    sb = L.acquire_signals(L.default_context(), 1, 300, L.B3SPLINE, 4, np.float32)
    try:
        sb.upload(a[None])
        sb.decompose(1, 4)
        med = sb.abs_median(1)
    finally:
        L.release_signals(sb)
    np.testing.assert_allclose(_noise_from_median(med[0], W.B3spline(1).sigma_e()), g["noise_300"], rtol=1e-5)
