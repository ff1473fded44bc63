"""richardson_lucy_stack(fft=True) with large PSFs on the MI355X (wt_batch_fft_spectrum / wt_batch_fft_apply behind it).

The primitive first: BatchPlan.fft_apply against Plan.fft_apply on a plan of each frame, bit for bit, and against
numpy's irfft2(rfft2(x) * rfft2(k)) in float64 within 4e-6 * max|x| per frame - the bound
test_fft_circular_products_vs_numpy (tests/test_gpu_round4.py) holds the per-image FFT to.  Then every case of
tests/test_rl_fft_stack_cpu.py with the per-frame entry point it would fall back to patched to raise: soft-threshold
cases meet the float64 numpy oracle per frame - atol = 2e-4 * max|ref_frame| and rtol = 2e-4, the project's bound for
richardson_lucy (tests/test_gpu_round2.py, test_richardson_lucy_fft_large_psf_vs_reference_golden), over all samples
- and every case equals the per-frame richardson_lucy(fft=True) bit for bit, through out= too; the hard-threshold
case rests on the bit check alone.  Frames lie nine decades apart, so a mixed-up frame is an error of order one."""
import numpy as np
import pytest

from test_rl_stack_cpu import make_frames, make_psf
from test_rl_fft_stack_cpu import CASES, CASE_IDS, case, case_inputs, case_reference, call_kw, is_soft

pytestmark = pytest.mark.gpu

ATOL_OF_MAX, RTOL = 2e-4, 2e-4
FFT_BOUND = 4e-6


def _mods():
    import wavelets_amd as W
    from wavelets_amd import batch as B, utils as U, _lib as L
    return W, B, U, L


def _same_bits(got, exp, what):
    assert got.dtype == exp.dtype == np.float32 and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    g, e = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(exp).view(np.uint32)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _no_fallback(monkeypatch, B):
    def refuse(*a, **k):
        raise AssertionError("richardson_lucy_stack fell back to the per-frame utils.richardson_lucy")
    monkeypatch.setattr(B, "richardson_lucy", refuse)


def _kernel_image(shape, seed):
    """a normalised 9 x 7 kernel (the whole frame if that is smaller) rolled to the origin"""
    rng = np.random.default_rng(seed)
    k = np.zeros(shape, np.float32)
    kh, kw = min(shape[0], 9), min(shape[1], 7)
    k[:kh, :kw] = rng.random((kh, kw))
    k /= k.sum()
    return np.roll(k, (-(kh // 2), -(kw // 2)), axis=(0, 1))


# ---------------------------------------------------------------------------------------------- the primitive
@pytest.mark.parametrize("shape", [(2, 8), (32, 64), (45, 48), (50, 60), (8192, 4), (4, 8192)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_fft_apply_equals_fft_apply_per_frame(shape):
    """nf = 3 in a batch of 4 frames; (2, 8): the smallest; (32, 64): radix 2, H != W; (45, 48): an odd height without
    a factor 2 next to 2^4 * 3, partial transpose tiles; (50, 60): 5 * 5 * 2 and 3 * 5 * 4; (8192, 4) and (4, 8192): the
    longest row - 64 KB of LDS - in each pass"""
    W, B, U, L = _mods()
    H, Wd = shape
    assert L.batch_fft_ok(H, Wd)
    ctx = L.default_context()
    nf = 3
    x = make_frames(nf, H, Wd, 17)
    k = _kernel_image(shape, H + Wd)
    f = np.fft.rfft2(k.astype(np.float64))
    X = np.fft.rfft2(x.astype(np.float64), axes=(1, 2))
    want = {False: np.fft.irfft2(X * f, s=shape, axes=(1, 2)), True: np.fft.irfft2(X * f.conj(), s=shape, axes=(1, 2))}
    S, D, K = L.PLANE_SCRATCH(7), L.PLANE_SCRATCH(8), L.PLANE_SCRATCH(10)
    bp = L.BatchPlan(ctx, 4, H, Wd, L.B3SPLINE, 2)
    plan = L.Plan(ctx, H, Wd, L.B3SPLINE, 2)
    try:
        bp.fill(4, D, np.nan)
        bp.upload(K, k[None])
        bp.fft_spectrum(K)
        bp.upload(S, x)
        plan.upload(K, k)
        plan.fft_spectrum(K)
        for conj in (False, True):
            bp.fft_apply(nf, S, D, conj)
            got = bp.download(D, 4)
            assert np.isnan(got[3]).all()                                   # the inactive frame is not written
            for i in range(nf):
                plan.upload(S, x[i])
                plan.fft_apply(S, D, conj)
                _same_bits(got[i], plan.download(D), f"{shape} conj={conj} frame {i}")
                err = float(np.abs(got[i].astype(np.float64) - want[conj][i]).max())
                bound = FFT_BOUND * float(np.abs(x[i]).max())
                print(f"{shape} conj={conj} frame {i}: {err:.3e} against numpy, bound {bound:.3e}")
                assert err <= bound, (shape, conj, i, err, bound)
        assert np.array_equal(bp.download(S, nf), x)                        # the source plane is left alone
    finally:
        plan.close()
        bp.close()


def test_batch_fft_argument_errors():
    """each on a valid small batch; none launches anything"""
    W, B, U, L = _mods()
    ctx = L.default_context()
    S, D = L.PLANE_SCRATCH(7), L.PLANE_SCRATCH(8)
    bp = L.BatchPlan(ctx, 2, 8, 12, L.B3SPLINE, 2)
    try:
        bp.upload(S, make_frames(2, 8, 12, 1))
        with pytest.raises(L.WatrooHipError, match="no kernel spectrum"):
            bp.fft_apply(2, S, D)                                           # apply before spectrum
        bp.fft_spectrum(S)
        bp.fft_apply(2, S, D)
        with pytest.raises(L.WatrooHipError, match="src and dst must differ"):
            bp.fft_apply(2, S, S)
        with pytest.raises(L.WatrooHipError, match="active frames"):
            bp.fft_apply(3, S, D)
        with pytest.raises(L.WatrooHipError, match="active frames"):
            bp.fft_apply(0, S, D)
        with pytest.raises(L.WatrooHipError, match="not a plane of a batch"):
            bp.fft_apply(2, S, L.PLANE_SCRATCH(11))
        with pytest.raises(L.WatrooHipError, match="not a plane of a batch"):
            bp.fft_spectrum(L.PLANE_SCRATCH(11))
    finally:
        bp.close()
    odd = L.BatchPlan(ctx, 2, 14, 12, L.B3SPLINE, 2)                        # 14 = 2 * 7
    try:
        odd.upload(S, make_frames(2, 14, 12, 1))
        with pytest.raises(L.WatrooHipError, match="prime factor above 5"):
            odd.fft_spectrum(S)
        with pytest.raises(L.WatrooHipError, match="no kernel spectrum"):
            odd.fft_apply(2, S, D)
    finally:
        odd.close()


# ---------------------------------------------------------------------------------------------- the stack function
@pytest.mark.parametrize("name", CASE_IDS)
def test_richardson_lucy_stack_fft(name, monkeypatch):
    W, B, U, L = _mods()
    c = case(name)
    kw = call_kw(c)
    frames, psf = case_inputs(name)
    n = len(frames)
    if c.get("min_taps"):
        monkeypatch.setattr(U, "_FFT_MIN_TAPS", c["min_taps"])
    assert psf.size >= U._FFT_MIN_TAPS
    chunks = []
    if c.get("chunk"):
        def forced(N, H, Wd, level, *a, **k):
            assert k.get("extra_planes") == B._rl_fft_extra_planes(level) == level + 8
            chunks.append([(f0, min(c["chunk"], N - f0)) for f0 in range(0, N, c["chunk"])])
            return chunks[-1]
        monkeypatch.setattr(L, "batch_chunks", forced)
    out = np.full(frames.shape, np.nan, np.float32)
    with monkeypatch.context() as m:
        _no_fallback(m, B)
        got = W.richardson_lucy_stack(frames, psf, **kw)
        res = W.richardson_lucy_stack(frames, psf, out=out, **kw)
    assert res is out
    if c.get("chunk"):
        assert chunks and chunks[0][-1][1] < c["chunk"] <= n        # the last chunk is shorter than the batch
    assert got.shape == frames.shape and got.dtype == np.float32
    if is_soft(c):
        ref = case_reference(name)
        for i in range(n):
            tol = ATOL_OF_MAX * np.abs(ref[i]).max() + RTOL * np.abs(ref[i])
            worst = float((np.abs(got[i].astype(np.float64) - ref[i]) / tol).max())
            print(f"{name} frame {i}: worst error {worst:.3e} of the tolerance")
            assert worst <= 1.0, f"{name} frame {i}: {worst:.3e} of atol 2e-4 max|ref| + rtol 2e-4 against the float64 oracle"
    for i in range(n):
        exp = U.richardson_lucy(frames[i].copy(), psf.copy(), **kw)
        _same_bits(got[i], exp, f"{name} frame {i}")
    _same_bits(out, got, f"{name} out=")


def test_stack_of_one_frame_and_a_list_of_frames(monkeypatch):
    W, B, U, L = _mods()
    frames, psf = case_inputs("radix2_32x64_psf23x23")
    with monkeypatch.context() as m:
        _no_fallback(m, B)
        one = W.richardson_lucy_stack(frames[1:2], psf, iterations=2, fft=True)
        lst = W.richardson_lucy_stack([f for f in frames], psf, iterations=2, fft=True)
    _same_bits(one[0], U.richardson_lucy(frames[1].copy(), psf, iterations=2, fft=True), "one frame")
    for i in range(len(frames)):
        _same_bits(lst[i], U.richardson_lucy(frames[i].copy(), psf, iterations=2, fft=True), f"list frame {i}")


def test_a_second_call_on_the_cached_batch_uses_its_own_psf(monkeypatch):
    """the batch of the first call comes back from the cache with the first PSF's spectrum in it"""
    W, B, U, L = _mods()
    frames, psf = case_inputs("radix2_32x64_psf23x23")
    other = np.ascontiguousarray(make_psf(24, 25)[::-1, ::-1])
    taken = []
    real = L.acquire_batch
    monkeypatch.setattr(L, "acquire_batch", lambda *a: taken.append(real(*a)) or taken[-1])
    with monkeypatch.context() as m:
        _no_fallback(m, B)
        first = W.richardson_lucy_stack(frames, psf, iterations=2, fft=True)
        second = W.richardson_lucy_stack(frames, other, iterations=2, fft=True)
    assert len(taken) == 2 and taken[0] is taken[1]
    for i in range(len(frames)):
        _same_bits(first[i], U.richardson_lucy(frames[i].copy(), psf, iterations=2, fft=True), f"first PSF, frame {i}")
        _same_bits(second[i], U.richardson_lucy(frames[i].copy(), other, iterations=2, fft=True), f"second PSF, frame {i}")
    assert not np.array_equal(first, second)
