"""transform_along / denoise_along on the GPU: the axis engine (wt_along: a tile of neighbouring signals per workgroup,
samples a stride apart, the scales in LDS) against the signal engine on the host-transposed stack, bit for bit
(np.testing.assert_array_equal), in float32 and float64, both families - every length and inner extent at which the
kernels take another path (one sample, fewer samples than a tap's reach, many bounces of the 'mirror' border, inner
extents below, at and past a tile, the budget N = 512 and one past it), more tiles than resident workgroups, outer and
inner chunks, even and odd medians with a constant and a tied column - and against the reference's recorded planes of
tests/golden/g11_1d.npz."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FAMS = ("B3spline", "Triangle")
DTYPES = (np.float32, np.float64)
LENGTHS = (1, 2, 3, 5, 17, 255, 256, 257, 511, 512)
INNERS = (2, 3, 15, 16, 17, 65, 300)


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


def cube(shape, dtype, seed=0):
    """seeded normal plus an offset, no NaN or inf"""
    rng = np.random.default_rng([seed] + list(shape))
    return (rng.standard_normal(shape) * 3.0 + 10.0).astype(dtype)


def via_signals_transform(W, a, level, cls, axis):
    """the definition: transform_signals on the host-transposed stack, rearranged"""
    m = np.moveaxis(a, axis, -1)
    res = W.transform_signals(np.ascontiguousarray(m).reshape(-1, a.shape[axis]), level, cls)
    return np.stack([np.moveaxis(res[:, s].reshape(m.shape), -1, axis) for s in range(level + 1)])


def via_signals_denoise(W, a, weights, cls, axis, noise, soft):
    m = np.moveaxis(a, axis, -1)
    per = list(noise.reshape(-1)) if isinstance(noise, np.ndarray) else noise
    res = W.denoise_signals(np.ascontiguousarray(m).reshape(-1, a.shape[axis]), weights, cls, noise=per, soft_threshold=soft)
    return np.moveaxis(res.reshape(m.shape), -1, axis)


def bounce_level(N, hw):
    """the smallest level whose last scale reaches at least 2 N samples: hw * 2**(level - 1) >= 2 * N"""
    level = 1
    while hw * 2 ** (level - 1) < 2 * N:
        level += 1
    return level


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", FAMS)
def test_transform_equals_the_signal_engine(W, fam, dtype):
    from wavelets_amd import along as A
    cls = getattr(W, fam)
    hw = len(cls.coefficients_1d) // 2
    for N in LENGTHS:
        for I in INNERS:
            a = cube((3, N, I), dtype, seed=N)
            for level in sorted({1, 3, bounce_level(N, hw)}):
                assert A.along_eligible(a, level, cls, axis=1)
                got = W.transform_along(a, level, cls, axis=1)
                assert got.dtype == dtype and got.shape == (level + 1, 3, N, I)
                np.testing.assert_array_equal(got, via_signals_transform(W, a, level, cls, 1), err_msg=f"{fam} N={N} I={I} L={level}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", FAMS)
def test_transform_at_the_budget_and_one_past_it(W, fam, dtype):
    from wavelets_amd import along as A
    cls = getattr(W, fam)
    for I in (16, 17):
        a = cube((3, 512, I), dtype, seed=1)
        assert A.along_eligible(a, 8, cls, axis=1)
        np.testing.assert_array_equal(W.transform_along(a, 8, cls, axis=1), via_signals_transform(W, a, 8, cls, 1))
    past = cube((2, 513, 17), dtype, seed=2)                     # the transposed route: still equal
    assert not A.along_eligible(past, 4, cls, axis=1)
    np.testing.assert_array_equal(W.transform_along(past, 4, cls, axis=1), via_signals_transform(W, past, 4, cls, 1))
    np.testing.assert_array_equal(W.denoise_along(past, [5, 3], cls, axis=1), via_signals_denoise(W, past, [5, 3], cls, 1, None, True))


def test_dimensions_axes_views_and_many_tiles(W):
    for dtype in DTYPES:
        two = cube((40, 33), dtype, seed=3)
        np.testing.assert_array_equal(W.transform_along(two, 3), via_signals_transform(W, two, 3, W.B3spline, 0))
        four = cube((2, 19, 3, 7), dtype, seed=4)
        for axis in (1, -2):
            np.testing.assert_array_equal(W.transform_along(four, 3, W.Triangle, axis=axis),
                                          via_signals_transform(W, four, 3, W.Triangle, axis % 4))
            np.testing.assert_array_equal(W.denoise_along(four, [5, 3], axis=axis),
                                          via_signals_denoise(W, four, [5, 3], W.B3spline, axis % 4, None, True))
        view = cube((2, 21, 40), dtype, seed=5)[:, :, ::2]          # non-contiguous: copied once
        assert not view.flags.c_contiguous
        np.testing.assert_array_equal(W.transform_along(view, 2, axis=1), via_signals_transform(W, view, 2, W.B3spline, 1))
        last = cube((3, 4, 50), dtype, seed=6)                       # the last axis: the signal engine itself
        np.testing.assert_array_equal(W.transform_along(last, 3, axis=-1), via_signals_transform(W, last, 3, W.B3spline, 2))
    many = cube((8, 40000), np.float32, seed=7)                      # more tiles than resident workgroups
    np.testing.assert_array_equal(W.transform_along(many, 3), via_signals_transform(W, many, 3, W.B3spline, 0))
    np.testing.assert_array_equal(W.denoise_along(many, [5, 3]), via_signals_denoise(W, many, [5, 3], W.B3spline, 0, None, True))


def test_outer_and_inner_chunks(W, monkeypatch):
    from wavelets_amd import along as A
    from wavelets_amd import _lib as L
    for dtype in DTYPES:
        a = cube((5, 64, 300), dtype, seed=8)
        noise = np.abs(cube((5, 300), np.float64, seed=9)) / 10
        noise[1, 7] = 0
        whole_t = W.transform_along(a, 3, W.Triangle, axis=1)
        whole_d = [W.denoise_along(a, [5, 3], W.Triangle, axis=1, noise=n) for n in (None, noise)]
        np.testing.assert_array_equal(whole_t, via_signals_transform(W, a, 3, W.Triangle, 1))
        tile = L.along_tile(64, a.dtype.itemsize)
        for rule, want in ((lambda O, N, I, level, itemsize, planes: [(o0, min(2, O - o0), 0, I) for o0 in range(0, O, 2)], 3),
                           (lambda O, N, I, level, itemsize, planes: [(o, 1, i0, min(2 * tile, I - i0)) for o in range(O)
                                                                      for i0 in range(0, I, 2 * tile)], 5 * -(-300 // (2 * tile)))):
            seen = []

            def chunked(*args, _rule=rule):
                seen.append(_rule(*args))
                return seen[-1]
            monkeypatch.setattr(A, "_chunks", chunked)
            np.testing.assert_array_equal(W.transform_along(a, 3, W.Triangle, axis=1), whole_t)
            for n, whole in zip((None, noise), whole_d):
                np.testing.assert_array_equal(W.denoise_along(a, [5, 3], W.Triangle, axis=1, noise=n), whole)
            assert len(seen) == 3 and all(len(c) == want for c in seen)
            monkeypatch.undo()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_medians_equal_the_signal_engine(W, dtype):
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    for fam in (L.B3SPLINE, L.TRIANGLE):
        for N in (16, 17, 300, 512, 1, 2):                           # even and odd N
            I = 21
            a = cube((2, N, I), dtype, seed=20 + N)
            a[:, :, 3] = 7.25                                        # a constant column: median 0
            a[0, :, 5] = np.where(np.arange(N) % 2 == 0, 1.0, 3.0)  # tied magnitudes
            ab = L.acquire_along(ctx, 2 * I, N, fam, 2, dtype, planes=False)
            try:
                ab.upload(a)
                got = ab.abs_median()
            finally:
                L.release_along(ab)
            sig = np.ascontiguousarray(np.moveaxis(a, 1, -1)).reshape(-1, N)
            sb = L.acquire_signals(ctx, len(sig), N, fam, 2, dtype)
            try:
                sb.upload(sig)
                sb.decompose(len(sig), 2)
                want = sb.abs_median(len(sig))
            finally:
                L.release_signals(sb)
            assert got.shape == (2, I) and got.dtype == dtype
            np.testing.assert_array_equal(got, want.reshape(2, I), err_msg=f"family {fam} N={N}")
            assert got[0, 3] == 0 and got[1, 3] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", FAMS)
def test_denoise_equals_the_signal_engine(W, fam, dtype):
    from wavelets_amd import along as A
    cls = getattr(W, fam)
    for N, I in ((16, 21), (17, 3), (300, 33), (512, 17), (1, 5), (2, 2)):
        a = cube((2, N, I), dtype, seed=100 + N)
        a[:, :, 1] = 7.25                                            # a constant column: median 0, noise 0, significance one
        levels = np.abs(cube((2, I), np.float32, seed=N)) / 8
        levels[0, 0] = 0
        levels[1, I - 1] = 0
        for weights in ([5, 3], [3, 0, 1], [0, 0]):
            for soft in (True, False):
                for noise in (None, 1.25, levels):
                    assert A.along_eligible(a, len(weights), cls, 1, noise)
                    got = W.denoise_along(a, weights, cls, axis=1, noise=noise, soft_threshold=soft)
                    assert got.dtype == dtype and got.shape == a.shape
                    np.testing.assert_array_equal(got, via_signals_denoise(W, a, weights, cls, 1, noise, soft),
                                                  err_msg=f"{fam} N={N} I={I} {weights} soft={soft} noise={type(noise).__name__}")
        out = np.full(a.shape, np.nan, dtype)
        assert W.denoise_along(a, [5, 3], cls, axis=1, out=out) is out
        np.testing.assert_array_equal(out, via_signals_denoise(W, a, [5, 3], cls, 1, None, True))
        planes = np.full((3,) + a.shape, np.nan, dtype)
        assert W.transform_along(a, 2, cls, axis=1, out=planes) is planes
        np.testing.assert_array_equal(planes, via_signals_transform(W, a, 2, cls, 1))


def test_against_the_reference_fixture(W):
    """the reference's own planes (tests/golden/g11_1d.npz), the fixture's signal in every column of an (N, 5) array at
    axis 0, at the tolerance tests/test_gpu_signals.py uses for these fixtures: 1e-5 * max|signal|"""
    g = load_golden("g11_1d")
    for n in (300, 17, 5):
        sig = g[f"sig_{n}"]
        a = np.repeat(sig[:, None], 5, axis=1)
        tol = 1e-5 * np.abs(sig).max()
        for fam in FAMS:
            for level in (1, 3, 5):
                got = W.transform_along(a, level, getattr(W, fam))
                assert got.shape == (level + 1, n, 5)
                ref = g[f"coef_{fam.lower()}_{n}_L{level}"].astype(np.float64)
                for col in range(5):
                    np.testing.assert_allclose(got[:, :, col].astype(np.float64), ref, rtol=0, atol=tol)
    sig = g["sig_300"]
    a = np.repeat(sig[:, None], 5, axis=1)
    got = W.denoise_along(a, [5, 3])
    for col in range(5):
        np.testing.assert_array_equal(got[:, col], W.denoise(sig, [5, 3]))
