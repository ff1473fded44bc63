"""The FFT products (wavelets_amd/csrc/wt_fft.h: Plan.fft_spectrum / fft_apply, Plan64's, BatchPlan's, and
utils._ExtendedFFT on top of them) on EVERY admitted length, on an MI355X (run with -m gpu).

The arithmetic of wt_fft_rows_mixed_kernel changes with the factor list of the side - digit weights, twiddle strides,
the shift / division split of the butterfly index, one stage sequence per n = 2^a 3^b 5^c - so the 166 admitted
lengths are 166 code paths, and the radix-2 kernel has its own 13.  Every product here is held against numpy's float64
fft2 / ifft2 of the same product, within the project's bounds for these products (test_gpu_round5.py,
test_mixed_radix_fft_circular_products_vs_numpy): 4e-6 * max|x| in float32, 1e-13 * max|x| in float64.  Each group
prints the worst fraction of its bound and appends it to the suite's log of measured errors (conftest.measured)."""
import time

import numpy as np
import pytest

from conftest import measured
from test_fft_rules_cpu import ADMITTED, EXT_CASES, EXT_NOT_OK, ext_case_inputs, factor_list, periodic_products

pytestmark = pytest.mark.gpu

B3_TAPS = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
BOUND = {np.float32: 4e-6, np.float64: 1e-13}             # times max|x|
OTHER_SIDES = (2, 3, 4, 5, 6)
SHIFT_LENGTHS = (2, 3, 5, 6, 30, 2 * 3 ** 7, 5 ** 5, 3 ** 8, 2 * 5 ** 5, 2 ** 5 * 3 ** 5, 8100, 8192)
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as entry
    entry.build()
    from wavelets_amd import _lib
    return _lib


def _name(dtype):
    return np.dtype(dtype).name


def _plan(L, dtype, H, W, level=0):
    if dtype == np.float32:
        return L.Plan(L.default_context(), H, W, L.B3SPLINE, level)
    return L.Plan64(L.default_context(), H, W, B3_TAPS, level)


def _kernel_image(shape, rng, dtype):
    """a normalised 9 x 7 random kernel, clipped to the frame, rolled to the origin"""
    k = np.zeros(shape, dtype)
    kh, kw = min(shape[0], 9), min(shape[1], 7)
    k[:kh, :kw] = rng.random((kh, kw))
    k /= k.sum()
    return np.roll(k, (-(kh // 2), -(kw // 2)), axis=(0, 1))


def _oracle(x, k):
    """numpy's float64 products of what was uploaded: (ifft2(fft2 x * fft2 k), ifft2(fft2 x * conj(fft2 k)))"""
    f = np.fft.fft2(k.astype(np.float64))
    X = np.fft.fft2(x.astype(np.float64))
    return np.fft.ifft2(X * f).real, np.fft.ifft2(X * f.conj()).real


def _device_products(L, p, x, k):
    """(conv, corr) of the plan: the spectrum of k, then both products of x"""
    S = L.PLANE_SCRATCH(6)
    p.upload(S, k)
    p.fft_spectrum(S)
    p.upload(L.PLANE_INPUT, x)
    out = []
    for conj in (False, True):
        p.fft_apply(L.PLANE_INPUT, L.PLANE_OUT, conj)
        out.append(p.download(L.PLANE_OUT).copy())
    return out


def _worst(got, want):
    """(max abs difference, its position)"""
    d = np.abs(np.asarray(got, np.float64) - want)
    pos = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[pos]), tuple(int(v) for v in pos)


def _record(what, fraction, extra=""):
    """print the worst fraction of the bound and append it to the log of measured errors (as a value against a
    bound of 1; the caller asserts afterwards, with the lengths and positions in its message)"""
    print(f"{what}: worst {fraction:.4f} of the bound{extra}")
    try:
        measured(f"{what}, fraction of the bound{extra}", fraction, 0.0, 1.0)
    except AssertionError:
        pass


def _shape(n, orientation, other):
    return (other, n) if orientation == "width" else (n, other)


# ------------------------------------------------------------------------------------------------- length sweep
@pytest.mark.parametrize("orientation", ["width", "height"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_fft_products_on_every_admitted_length_vs_numpy(L, dtype, orientation):
    """All 166 lengths n = 2^a 3^b 5^c in 2 .. 8192 as the width (the first forward and the last inverse pass: real
    input, real output) or as the height (the passes on the transposed spectra, the kernel-spectrum product fused into
    the load), the other side cycling through 2, 3, 4, 5, 6 - so every stage sequence of the mixed kernel and every
    log2 n of the radix-2 kernel runs, in both passes, float32 and float64 (above 4096: more than 64 KB of LDS a row).
    A failure names every length that missed, its factor list and where the worst sample lies."""
    assert len(ADMITTED) == 166
    rng = np.random.default_rng(20 + (dtype == np.float64) + 2 * (orientation == "height"))
    worst, failures, t0 = (-1.0, None), [], time.perf_counter()
    for i, n in enumerate(ADMITTED):
        shape = _shape(n, orientation, OTHER_SIDES[i % len(OTHER_SIDES)])
        assert L.fft_supported(*shape), shape
        x = rng.standard_normal(shape).astype(dtype)
        k = _kernel_image(shape, rng, dtype)
        want = _oracle(x, k)
        p = _plan(L, dtype, *shape)
        try:
            got = _device_products(L, p, x, k)
        finally:
            p.close()
        bound = BOUND[dtype] * float(np.abs(x).max())
        for what, g, w in zip(("conv", "corr"), got, want):
            d, pos = _worst(g, w)
            if d / bound > worst[0]:
                worst = (d / bound, (n, what))
            if not d <= bound:
                failures.append(f"n = {n} = {'*'.join(map(str, factor_list(n)))} as {orientation} ({shape[0]} x {shape[1]}), {what}: "
                                f"{d:.3e} > {bound:.3e} at {pos}")
    _record(f"fft length sweep {_name(dtype)} {orientation}, 166 lengths", worst[0],
            f" (at n = {worst[1][0]}, {worst[1][1]}); {time.perf_counter() - t0:.1f} s")
    assert not failures, f"{len(failures)} products beyond the bound:\n" + "\n".join(failures)


# ------------------------------------------------------------------------------------------------- exact shifts
@pytest.mark.parametrize("orientation", ["width", "height"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_unit_impulse_kernels_shift_the_image_exactly(L, dtype, orientation):
    """A unit impulse at the asymmetric offset (1, n - 2) along the long side (transposed for n as the height) as the
    kernel: the product is np.roll(x, offset), with conj=True the opposite roll - which pins the orientation of
    both passes.  A unit impulse at the LAST pixel as the image, against the random kernel: the product is that
    kernel rolled by (-1, -1), with conj=True the kernel read backwards from the last pixel - which pins the addressing
    of the last index without relying on a smooth answer.  The other side is 5: a roll by +1 there is not a roll
    by -1.  Lengths: the smallest, the pure powers 3^8 and 5^5, a single 2 in front of 3^7 and of 5^5, 2^5 3^5 (ten
    factors), 8100 (the longest mixed row) and 8192."""
    rng = np.random.default_rng(40 + (dtype == np.float64) + 2 * (orientation == "height"))
    worst, failures = (-1.0, None), []
    for n in SHIFT_LENGTHS:
        shape = _shape(n, orientation, 5)
        H, W = shape
        off = (1, n - 2) if orientation == "width" else (n - 2, 1)
        x = rng.standard_normal(shape).astype(dtype)
        delta = np.zeros(shape, dtype)
        delta[off] = 1
        k = _kernel_image(shape, rng, dtype)
        last = np.zeros(shape, dtype)
        last[H - 1, W - 1] = 1
        yy, xx = np.mgrid[0:H, 0:W]
        k64 = k.astype(np.float64)
        p = _plan(L, dtype, H, W)
        try:
            shifted = _device_products(L, p, x, delta)
            kernels = _device_products(L, p, last, k)
        finally:
            p.close()
        x64 = x.astype(np.float64)
        checks = (("impulse kernel, conv", shifted[0], np.roll(x64, off, axis=(0, 1)), float(np.abs(x).max())),
                  ("impulse kernel, corr", shifted[1], np.roll(x64, (-off[0], -off[1]), axis=(0, 1)), float(np.abs(x).max())),
                  ("impulse image, conv", kernels[0], np.roll(k64, (-1, -1), axis=(0, 1)), 1.0),
                  ("impulse image, corr", kernels[1], k64[(H - 1 - yy) % H, (W - 1 - xx) % W], 1.0))
        for what, g, w, amax in checks:
            bound = BOUND[dtype] * amax
            d, pos = _worst(g, w)
            if d / bound > worst[0]:
                worst = (d / bound, (n, what))
            if not d <= bound:
                failures.append(f"n = {n} = {'*'.join(map(str, factor_list(n)))} as {orientation}, {what}: {d:.3e} > {bound:.3e} at {pos}")
    _record(f"fft exact shifts {_name(dtype)} {orientation}", worst[0], f" (at n = {worst[1][0]}, {worst[1][1]})")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------- raised LDS
@pytest.mark.parametrize("shape", [(8192, 4), (4, 8192), (6561, 6), (6, 8100), (2, 6250)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float64_rows_above_64_kb_of_lds(L, shape):
    """Float64 rows longer than 4096 need more than 64 KB of LDS (8192: a 128 KB workgroup), which wt_fft_rows asks
    for by raising the kernel's dynamic LDS limit: the radix-2 kernel (8192) and the mixed kernel (3^8, 2^2 3^4 5^2,
    2 5^5) in the column passes (as the height) and in the row passes (as the width).  The sweep reaches these
    lengths too; this test keeps them visible by name."""
    H, W = shape
    assert max(H, W) * 16 > 64 * 1024
    rng = np.random.default_rng(H + W)
    x = rng.standard_normal(shape)
    k = _kernel_image(shape, rng, np.float64)
    want = _oracle(x, k)
    p = _plan(L, np.float64, H, W)
    try:
        got = _device_products(L, p, x, k)
    finally:
        p.close()
    bound = BOUND[np.float64] * float(np.abs(x).max())
    errs = [_worst(g, w) for g, w in zip(got, want)]
    _record(f"float64 fft above 64 KB of LDS, {H} x {W}", max(e[0] for e in errs) / bound)
    for what, (d, pos) in zip(("conv", "corr"), errs):
        assert d <= bound, f"{H} x {W} {what}: {d:.3e} > {bound:.3e} at {pos}"


# ------------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("shape", [(6561, 2), (2, 8000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_fft_apply_on_the_longest_mixed_rows_equals_the_plan_bitwise(L, shape):
    """BatchPlan.fft_apply on nf = 2 of 3 frames at the longest mixed-radix rows (3^8 in the column passes, 2^6 5^3
    in the row passes; the frame is a grid dimension of the same kernels): each frame has the bits of Plan.fft_apply
    on that frame, the inactive frame - NaN beforehand - is not written, and each frame meets numpy within the bound."""
    H, W = shape
    assert L.batch_fft_ok(H, W)
    ctx = L.default_context()
    rng = np.random.default_rng(H * 3 + W)
    nf = 2
    x = rng.standard_normal((3, H, W)).astype(np.float32) * np.array([1.0, 30.0, 1000.0], np.float32)[:, None, None]
    k = _kernel_image(shape, rng, np.float32)
    S, D, K = L.PLANE_SCRATCH(7), L.PLANE_SCRATCH(8), L.PLANE_SCRATCH(10)
    bp = L.BatchPlan(ctx, 3, H, W, L.B3SPLINE, 2)
    plan = L.Plan(ctx, H, W, L.B3SPLINE, 2)
    worst = 0.0
    try:
        bp.upload(K, k[None])
        bp.fft_spectrum(K)
        bp.upload(S, x)
        plan.upload(K, k)
        plan.fft_spectrum(K)
        for conj in (False, True):
            bp.fill(3, D, np.nan)
            bp.fft_apply(nf, S, D, conj)
            got = bp.download(D, 3).copy()
            assert np.isnan(got[2]).all(), f"{shape} conj={conj}: the inactive frame was written"
            for i in range(nf):
                plan.upload(S, x[i])
                plan.fft_apply(S, D, conj)
                one = plan.download(D)
                assert got[i].dtype == one.dtype == np.float32
                same = got[i].view(np.uint32) == np.ascontiguousarray(one).view(np.uint32)
                assert same.all(), (f"{shape} conj={conj} frame {i}: {int((~same).sum())} samples differ in bits from Plan.fft_apply, "
                                    f"first at {tuple(np.argwhere(~same)[0])}")
                bound = BOUND[np.float32] * float(np.abs(x[i]).max())
                d, pos = _worst(got[i], _oracle(x[i], k)[int(conj)])
                worst = max(worst, d / bound)
                assert d <= bound, f"{shape} conj={conj} frame {i}: {d:.3e} > {bound:.3e} at {pos}"
        assert np.array_equal(bp.download(S, 3), x)                         # the source plane is left alone
        _record(f"batch fft {H} x {W}, 2 of 3 frames", worst)
    finally:
        plan.close()
        bp.close()


# ------------------------------------------------------------------------------------------------- extended frame
#   H   W  kh  kw
#   7  22   3   3   prime odd height
#   7  22  13   1   hy = 7 = H (the halo a whole copy of the image), hx = 0
#  14  22   1   1   no halo at all, frame 15 x 24
#  49  26   9   7   general
#  97  14   5  29   hx = 14 = W, odd frame width 45
#  11  14  21  29   PSF larger than the image, both halos whole copies
#  77  98  25  23   general
@pytest.mark.parametrize("case", EXT_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_extended_frame_products_vs_numpy_periodic_products(L, dtype, case):
    """utils._ExtendedFFT (prepare, apply) on images with a side the FFT does not take, against the float64 numpy
    product of period (H, W) with the PSF wrapped into the image (test_fft_rules_cpu.periodic_products): the window
    copies, the frame's FFT product and the copy back, on the device.  Same bounds: the sums are as long, only
    inside a larger frame."""
    from wavelets_amd import utils as U
    H, W, kh, kw = case
    x, psf = ext_case_inputs(H, W, kh, kw, dtype)
    want = periodic_products(x, psf)
    p = _plan(L, dtype, H, W, 1)
    ext = None
    try:
        ext = U._ExtendedFFT(p, dtype == np.float64, psf)
        assert ext.ok and not L.fft_supported(H, W)
        assert (ext.e, ext.hy, ext.hx, ext.Mh, ext.Mw) == U._ext_geometry(H, W, kh, kw)
        ext.prepare(U.B3spline(2))
        p.upload(L.PLANE_INPUT, x)
        bound = BOUND[dtype] * float(np.abs(x).max())
        errs = []
        for conj in (False, True):
            p.fill(L.PLANE_OUT, np.nan)                     # every pixel of the window must be written
            ext.apply(L.PLANE_INPUT, L.PLANE_OUT, conj)
            errs.append(_worst(p.download(L.PLANE_OUT), want[int(conj)]))
        assert np.array_equal(p.download(L.PLANE_INPUT), x)                  # the source plane is left alone
        _record(f"extended frame {H} x {W}, PSF {kh} x {kw}, frame {ext.Mh} x {ext.Mw}, {_name(dtype)}", max(e[0] for e in errs) / bound)
        for what, (d, pos) in zip(("conv", "corr"), errs):
            assert d <= bound, f"{case} {_name(dtype)} {what}: {d:.3e} > {bound:.3e} at {pos}"
    finally:
        if ext is not None:
            ext.close()
        p.close()


def test_halo_beyond_the_image_is_refused_and_richardson_lucy_stays_direct(L, monkeypatch):
    """A PSF whose halo exceeds the image (26 x 5 on 13 x 34; 14 x 29 on 7 x 14: hy = H + 1) cannot be extended by
    window copies: _ExtendedFFT.ok is False, and richardson_lucy(fft=True) - even with every PSF pushed to the FFT
    form - never calls _ExtendedFFT.apply there and returns the bits of the direct periodic form."""
    import wavelets_amd as WA
    from wavelets_amd import utils as U
    for H, W, kh, kw in EXT_NOT_OK:
        p = _plan(L, np.float32, H, W, 1)
        try:
            assert not U._ExtendedFFT(p, False, np.ones((kh, kw), np.float32)).ok, (H, W, kh, kw)
        finally:
            p.close()
    H, W, kh, kw = EXT_NOT_OK[0]
    x, psf = ext_case_inputs(H, W, kh, kw, np.float32)
    data = np.abs(x) + np.float32(1)
    calls = []
    monkeypatch.setattr(U._ExtendedFFT, "apply", lambda self, *a: calls.append(a))
    monkeypatch.setattr(U, "_FFT_MIN_TAPS", 1)
    got = WA.richardson_lucy(data.copy(), psf, iterations=2, fft=True)
    assert calls == []
    monkeypatch.setattr(U, "_FFT_MIN_TAPS", 1 << 30)
    direct = WA.richardson_lucy(data.copy(), psf, iterations=2, fft=True)
    assert calls == []
    assert got.dtype == direct.dtype == np.float32 and np.isfinite(direct).all()
    assert np.array_equal(got.view(np.uint32), direct.view(np.uint32))
