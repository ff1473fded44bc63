"""denoise_signals / denoise_along with anscombe=True on the GPU: the forward transform fused into the load of the
transform kernels and the inverse into the one store of the sum, against the per-signal loop of denoise(signal, ...,
anscombe=True) - bit for bit (np.testing.assert_array_equal), in float32 and float64, both families, Poisson counts with
zeros and a row below -3/8, every length at which the signal kernel takes another path up to its LDS budget, given and
estimated noise levels, soft and hard thresholds - and the axis engine against the signal engine on the transposed
stack.  While an engine call runs the per-signal call is replaced by an error: no quiet fall-back to the loop."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMS = ("B3spline", "Triangle")
DTYPES = (np.float32, np.float64)
BUDGET = {np.float32: 8192, np.float64: 4096}
NOISES = (None, 1.25, [None, 0, 2.5])
WEIGHTS = ([5, 3], [3, 0, 1])


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


@pytest.fixture
def no_loop(monkeypatch):
    """inside it the engines cannot reach the per-signal call or, from the axis engine, the signal engine"""
    from wavelets_amd import signals as S
    from wavelets_amd import along as A

    class Guard:
        def __enter__(self):
            def refuse(*a, **k):
                raise AssertionError("the engine fell back to the per-signal route")
            monkeypatch.setattr(S, "denoise", refuse)
            monkeypatch.setattr(A, "denoise_signals", refuse)

        def __exit__(self, *exc):
            monkeypatch.undo()
    return Guard()


def counts(shape, dtype, seed=0):
    """Poisson counts of mean 5 (zeros occur), cast to dtype"""
    return np.random.default_rng([seed] + list(shape)).poisson(5.0, shape).astype(dtype)


def stack(N, dtype, seed=0):
    """3 signals of Poisson counts with a zero, the middle one shifted below -3/8 throughout (the forward transform
    clamps it to 0)"""
    sig = counts((3, N), dtype, seed)
    sig[0, N // 2] = 0
    sig[1] -= sig[1].max() + 1
    assert (sig[1] < -0.375).all()
    return sig


def per(noise, M):
    return list(noise) if isinstance(noise, list) else [noise] * M


def loop(W, sig, weights, cls, noises, soft, anscombe=True):
    return np.stack([W.denoise(s, weights, cls, n, soft_threshold=soft, anscombe=anscombe) for s, n in zip(sig, noises)])


def transposed(W, a, weights, cls, axis, noise, soft, anscombe=True):
    """the definition of denoise_along: denoise_signals on the host-transposed stack, rearranged"""
    m = np.moveaxis(a, axis, -1)
    flat = list(noise.reshape(-1)) if isinstance(noise, np.ndarray) else noise
    res = W.denoise_signals(np.ascontiguousarray(m).reshape(-1, a.shape[axis]), weights, cls, noise=flat, soft_threshold=soft,
                            anscombe=anscombe)
    return np.moveaxis(res.reshape(m.shape), -1, axis)


# ---------------------------------------------------------------- signals

@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", FAMS)
def test_signals_equal_the_loop(W, no_loop, fam, dtype):
    from wavelets_amd import signals as S
    cls = getattr(W, fam)
    for N in (1, 2, 8, 255, 256, 257, 1000, BUDGET[dtype]):
        sig = stack(N, dtype, seed=N)
        for weights, soft, noise in [(w, s, n) for w in WEIGHTS for s in (True, False) for n in NOISES]:
            assert S.signals_eligible(sig, len(weights), cls, per(noise, 3))
            with no_loop:
                got = W.denoise_signals(sig, weights, cls, noise=noise, soft_threshold=soft, anscombe=True)
            assert got.dtype == dtype and got.shape == sig.shape
            np.testing.assert_array_equal(got, loop(W, sig, weights, cls, per(noise, 3), soft),
                                          err_msg=f"{fam} N={N} {weights} soft={soft} noise={noise}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_the_forward_transform_has_numpys_bits(W, dtype):
    """the fused forward transform is numpy's 2 * sqrt(max(x + 3/8, 0)) in the stack's element type, NaN kept, -inf
    to 0, +inf kept: the planes of decompose(anscombe=True) equal those of the plain decompose of numpy's transform"""
    from wavelets_amd import _lib as L
    sig = stack(257, dtype, seed=7)
    sig[0] = (np.random.default_rng(8).random(257) * 100).astype(dtype)     # not only whole counts: the square root rounds
    sig[2, :4] = [np.nan, np.inf, -np.inf, -0.375]
    with np.errstate(invalid="ignore"):
        t = sig + dtype(0.375)
        fwd = dtype(2) * np.sqrt(np.where(t <= 0, dtype(0), t))            # NaN stays NaN, -inf -> 0, +inf stays inf
    assert fwd.dtype == dtype and np.isnan(fwd[2, 0]) and fwd[2, 1] == np.inf and fwd[2, 2] == 0 and fwd[2, 3] == 0
    sb = L.acquire_signals(L.default_context(), 3, 257, L.B3SPLINE, 2, dtype)
    try:
        sb.upload(sig)
        sb.decompose(3, 2, anscombe=True)
        got = sb.download_planes(3).copy()
        sb.upload(fwd)
        sb.decompose(3, 2)
        want = sb.download_planes(3).copy()
    finally:
        L.release_signals(sb)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_non_finite_samples_stay_in_their_row(W, no_loop, dtype):
    sig = stack(300, dtype, seed=11)
    clean = sig.copy()
    sig[2, 40], sig[2, 120], sig[2, 200] = np.nan, np.inf, -np.inf
    for noise in (None, 1.25):
        with no_loop:
            got = W.denoise_signals(sig, [5, 3], noise=noise, anscombe=True)
            ref = W.denoise_signals(clean, [5, 3], noise=noise, anscombe=True)
        want = loop(W, sig, [5, 3], W.B3spline, [noise] * 3, True)
        np.testing.assert_array_equal(got, want)                       # (equal_nan is assert_array_equal's default)
        assert np.isnan(got[2]).any()
        np.testing.assert_array_equal(got[:2], ref[:2])                # the other rows: the bits of the clean stack
        assert np.isfinite(got[:2]).all()


# ---------------------------------------------------------------- along

ALONG = (((6, 40, 7), 1, np.float32), ((40, 33), 0, np.float64), ((2, 512, 17), 1, np.float32), ((2, 512, 17), 1, np.float64),
         ((5, 64, 2), 1, np.float32))


@pytest.mark.parametrize("shape,axis,dtype", ALONG, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_along_equals_the_signal_engine(W, no_loop, shape, axis, dtype):
    from wavelets_amd import along as A
    a = counts(shape, dtype, seed=21)
    a[(slice(None),) * axis + (slice(None), 0)] -= a.max() + 1        # inner position 0: below -3/8 along the whole axis
    rest = shape[:axis] + shape[axis + 1:]
    levels = np.abs(np.random.default_rng(5).standard_normal(rest)).astype(np.float32) + 0.25
    levels.reshape(-1)[1] = 0
    for fam in FAMS:
        cls = getattr(W, fam)
        for weights, soft in ((WEIGHTS[0], True), (WEIGHTS[1], False)):
            for noise in (None, 1.25, levels):
                assert A.along_eligible(a, len(weights), cls, axis, noise)
                with no_loop:
                    got = W.denoise_along(a, weights, cls, axis=axis, noise=noise, soft_threshold=soft, anscombe=True)
                assert got.dtype == dtype and got.shape == a.shape
                np.testing.assert_array_equal(got, transposed(W, a, weights, cls, axis, noise, soft),
                                              err_msg=f"{fam} {shape} {weights} soft={soft} noise={type(noise).__name__}")
    # ... and one column straight against the per-signal call
    col = (0,) * axis + (slice(None),) + (1,) * (len(shape) - axis - 1)
    got = W.denoise_along(a, [5, 3], axis=axis, anscombe=True)
    np.testing.assert_array_equal(got[col], W.denoise(np.ascontiguousarray(a[col]), [5, 3], anscombe=True))


# ---------------------------------------------------------------- chunks, out=, the keyword off, the raw flags

def test_chunks_give_the_bits_of_the_whole_run(W, no_loop, monkeypatch):
    from wavelets_amd import signals as S
    from wavelets_amd import along as A
    for dtype in DTYPES:
        five = np.concatenate([stack(257, dtype, seed=31), stack(257, dtype, seed=32)[:2]])
        noises = [None, 0.7, None, 2.0, None]
        cube = counts((3, 64, 40), dtype, seed=33)
        with no_loop:
            whole_s = W.denoise_signals(five, [5, 3], W.Triangle, noise=noises, anscombe=True)
            whole_a = W.denoise_along(cube, [5, 3], axis=1, anscombe=True)
        seen = []
        monkeypatch.setattr(S, "_chunks", lambda M, N, level, itemsize: seen.append("s") or [(f0, min(2, M - f0)) for f0 in range(0, M, 2)])
        monkeypatch.setattr(A, "_chunks", lambda O, N, I, level, itemsize, planes: seen.append("a") or [(o, 1, 0, I) for o in range(O)])
        got_s = W.denoise_signals(five, [5, 3], W.Triangle, noise=noises, anscombe=True)
        got_a = W.denoise_along(cube, [5, 3], axis=1, anscombe=True)
        monkeypatch.undo()
        assert seen == ["s", "a"]
        np.testing.assert_array_equal(got_s, whole_s)
        np.testing.assert_array_equal(got_a, whole_a)
        np.testing.assert_array_equal(whole_s, loop(W, five, [5, 3], W.Triangle, noises, True))


def test_out_is_returned_and_filled(W, no_loop):
    for dtype in DTYPES:
        sig = stack(100, dtype, seed=41)
        out = np.full(sig.shape, np.nan, dtype)
        with no_loop:
            assert W.denoise_signals(sig, [5, 3], out=out, anscombe=True) is out
        np.testing.assert_array_equal(out, loop(W, sig, [5, 3], W.B3spline, [None] * 3, True))
        a = counts((3, 20, 9), dtype, seed=42)
        out = np.full(a.shape, np.nan, dtype)
        with no_loop:
            assert W.denoise_along(a, [5, 3], axis=1, out=out, anscombe=True) is out
        np.testing.assert_array_equal(out, transposed(W, a, [5, 3], W.B3spline, 1, None, True))


def test_the_keyword_off_still_equals_the_loop_and_a_cached_stack_keeps_no_mode(W, no_loop):
    sig = stack(257, np.float32, seed=51) + np.float32(20)
    a = counts((3, 40, 9), np.float64, seed=52)
    with no_loop:
        on_s = W.denoise_signals(sig, [5, 3], anscombe=True)            # the cached stacks serve the next calls
        off_s = W.denoise_signals(sig, [5, 3], anscombe=False)
        on_a = W.denoise_along(a, [5, 3], axis=1, anscombe=True)
        off_a = W.denoise_along(a, [5, 3], axis=1)
    np.testing.assert_array_equal(off_s, loop(W, sig, [5, 3], W.B3spline, [None] * 3, True, anscombe=False))
    np.testing.assert_array_equal(off_a, transposed(W, a, [5, 3], W.B3spline, 1, None, True, anscombe=False))
    assert not np.array_equal(on_s, off_s) and not np.array_equal(on_a, off_a)


def test_raw_entries_refuse_unknown_flag_bits_on_a_live_stack(W):
    from wavelets_amd import _lib as L
    lib, ctx = L.load(), L.default_context()
    dp = ctypes.POINTER(ctypes.c_double)
    tau = (ctypes.c_double * 8)(*([1.0] * 8))
    sb = L.acquire_signals(ctx, 2, 16, L.B3SPLINE, 2, np.float32)
    ab = L.acquire_along(ctx, 6, 16, L.B3SPLINE, 2, np.float32, planes=False)
    try:
        sb.upload(np.ones((2, 16), np.float32))
        sb.decompose(2, 2)
        ab.upload(np.ones((2, 16, 3), np.float32))
        med = np.empty(6, np.float32)
        t = ctypes.cast(tau, dp)
        calls = (("wt_signals_decompose_ex", lambda f: lib.wt_signals_decompose_ex(sb._h, 2, 2, f)),
                 ("wt_signals_denoise_sum_ex", lambda f: lib.wt_signals_denoise_sum_ex(sb._h, 2, 1, t, t, 1, f)),
                 ("wt_along_abs_median_ex", lambda f: lib.wt_along_abs_median_ex(ab._h, ctypes.c_void_p(med.ctypes.data), f)),
                 ("wt_along_denoise_ex", lambda f: lib.wt_along_denoise_ex(ab._h, 2, 1, t, t, 1, f)))
        for flags in (2, 3, -2, 1 << 8):
            for name, call in calls:
                with pytest.raises(L.WatrooHipError, match=name + ": flags"):
                    L.check(call(flags))
        # flags = 0 is the old entry: the same planes
        want = sb.download_planes(2).copy()
        L.check(lib.wt_signals_decompose_ex(sb._h, 2, 2, 0))
        np.testing.assert_array_equal(sb.download_planes(2), want)
    finally:
        L.release_signals(sb)
        L.release_along(ab)
