"""CPU checks of the host rules behind the hand-written FFT (wavelets_amd/csrc/wt_fft.h) and the extended frame
(utils._ExtendedFFT), exhaustively instead of at hand-picked sizes: which lengths the FFT admits (wt_fft_supported,
wt_batch_fft_ok: 2 .. 8192 without a prime factor above 5 - 166 lengths, 30 of them above 4096, where a float64 row
needs more than 64 KB of LDS), what utils._next_smooth rounds to, the geometry and the window copies of the extended
frame, and a numpy model of the whole extended-frame product against the true product of period (H, W) at the
shapes tests/test_gpu_fft_lengths.py runs on the device.  `is_smooth` below is the only statement of the rule these
checks trust: trial division, nothing shared with the code under test."""
import numpy as np
import pytest

from wavelets_amd import _lib as L
from wavelets_amd import utils as U

MAX_N = 8192


def is_smooth(n):
    """no prime factor above 5 (1 counts: the empty product), by trial division"""
    if n < 1:
        return False
    for r in (2, 3, 5):
        while n % r == 0:
            n //= r
    return n == 1


def admitted(n):
    return 2 <= n <= MAX_N and is_smooth(n)


def factor_list(n):
    """the factors of an admitted length in the order wt_fft_factor lists them: 2s, then 3s, then 5s"""
    out = []
    for r in (2, 3, 5):
        while n % r == 0:
            out.append(r)
            n //= r
    assert n == 1
    return out


ADMITTED = [n for n in range(0, 8301) if admitted(n)]

# (H, W, kh, kw) of the extended-frame products: what each covers is in the table of the GPU test
EXT_CASES = [(7, 22, 3, 3), (7, 22, 13, 1), (14, 22, 1, 1), (49, 26, 9, 7), (97, 14, 5, 29), (11, 14, 21, 29), (77, 98, 25, 23)]
# halo taller than the image: _ExtendedFFT.ok is False
EXT_NOT_OK = [(13, 34, 26, 5), (7, 14, 14, 29)]


def periodic_products(x, psf):
    """(conv, corr) of period (H, W), float64: the PSF wrapped and summed into an H x W kernel image whose centre
    psf.shape // 2 lies at the origin (one row above it for an odd H, ref utils.py:246-250), then
    ifft2(fft2(x) * K) and the product with conj(K).  Wrapping makes it the true periodic product for a PSF of
    any size, larger than the image included."""
    H, W = x.shape
    kh, kw = psf.shape
    k = np.zeros((H, W), np.float64)
    rows = (np.arange(kh) - kh // 2 - H % 2) % H
    cols = (np.arange(kw) - kw // 2) % W
    np.add.at(k, (rows[:, None], cols[None, :]), psf.astype(np.float64))
    K = np.fft.fft2(k)
    X = np.fft.fft2(x.astype(np.float64))
    return np.fft.ifft2(X * K).real, np.fft.ifft2(X * K.conj()).real


def ext_case_inputs(H, W, kh, kw, dtype=np.float64):
    """image and PSF (sum 1) of one extended-frame case, the same on the CPU and on the device"""
    rng = np.random.default_rng(1000 * H + 100 * W + 10 * kh + kw)
    x = rng.standard_normal((H, W)).astype(dtype)
    psf = rng.uniform(0.1, 1.0, (kh, kw))
    psf = (psf / psf.sum()).astype(dtype)
    return x, psf


# ------------------------------------------------------------------------------------------------ admitted lengths
def test_fft_supported_is_the_five_smooth_rule_on_every_length_to_8300():
    for n in range(0, 8301):
        want = admitted(n)
        assert L.fft_supported(n, 4) == want, n
        assert L.fft_supported(4, n) == want, n


def test_batch_fft_ok_is_the_five_smooth_rule_on_every_length_to_8300():
    for n in range(0, 8301):
        want = admitted(n)
        assert L.batch_fft_ok(n, 4) == want, n
        assert L.batch_fft_ok(4, n) == want, n


def test_there_are_166_admitted_lengths_and_30_above_4096():
    """above 4096 a float64 row is more than 64 KB of LDS: wt_fft_rows raises the kernel's dynamic LDS limit"""
    got = [n for n in range(0, 8301) if L.fft_supported(n, 4)]
    assert got == ADMITTED
    assert len(got) == 166
    above = [n for n in got if n > 4096]
    assert len(above) == 30 and above[0] == 4320 and above[1] == 4374 and above[-2:] == [8100, 8192]
    assert all(n * 16 > 64 * 1024 for n in above) and all(n * 16 <= 64 * 1024 for n in got if n <= 4096)
    # float32: the longest mixed row is 8100 * 8 = 64 800 bytes and 8192 * 8 is 64 KB exactly - no float32 row
    # exceeds 64 KB, so the raised limit is a float64 matter in both kernels
    assert max(n * 8 for n in got if n != 8192) == 64800 and all(n * 8 <= 64 * 1024 for n in got)
    # WtFftFactors holds 16 factors: no admitted length has more than 13 (2^13)
    assert max(len(factor_list(n)) for n in got) == 13


def test_next_smooth_is_the_smallest_smooth_length_from_n_up():
    smooth_from = {}
    nxt = None
    for m in range(8192 + 1000, 1, -1):               # 8192 is smooth: every n <= 8192 has an answer <= 8192
        if is_smooth(m):
            nxt = m
        smooth_from[m] = nxt
    for n in range(0, 8193):
        assert U._next_smooth(n) == smooth_from[max(n, 2)], n


# ------------------------------------------------------------------------------------------------ extended frame
def _geometry_grid():
    """H, W in 2 .. 40 and kh, kw in 1 .. 41.  _ext_geometry and _ext_windows treat the two axes independently
    (rows from (H, kh), columns from (W, kw)), so the grid takes EVERY (H, kh) pair against a coarse set of (W, kw)
    - the extremes, odd and even, halo 0 / small / the image's own size / beyond it - and every (W, kw) pair against
    the same coarse set of (H, kh): each axis sees all 39 * 41 of its pairs, the full product of the two coarse sets
    is in both halves, and the whole is 64 000 geometries instead of 2.5 million."""
    coarse_n, coarse_k = (2, 3, 7, 14, 40), (1, 2, 13, 41)
    seen = set()
    for n in range(2, 41):
        for k in range(1, 42):
            for m in coarse_n:
                for j in coarse_k:
                    for case in ((n, m, k, j), (m, n, j, k)):
                        if case not in seen:
                            seen.add(case)
                            yield case


def test_ext_geometry_holds_the_extended_image_in_a_smooth_frame():
    count = 0
    for H, W, kh, kw in _geometry_grid():
        e, hy, hx, Mh, Mw = U._ext_geometry(H, W, kh, kw)
        assert e == H % 2, (H, W, kh, kw)
        assert (hy, hx) == (kh // 2 + e, kw // 2), (H, W, kh, kw)
        assert Mh >= H + 2 * hy and Mw >= W + 2 * hx, (H, W, kh, kw)
        assert is_smooth(Mh) and is_smooth(Mw), (H, W, kh, kw, Mh, Mw)
        # and no larger than need be: the next smooth length
        assert not any(is_smooth(m) for m in range(max(H + 2 * hy, 2), Mh)), (H, kh, Mh)
        assert not any(is_smooth(m) for m in range(max(W + 2 * hx, 2), Mw)), (W, kw, Mw)
        count += 1
    assert count > 60000


def test_ext_windows_tile_the_extended_image_exactly_once():
    """Every geometry of the grid that _ExtendedFFT admits (`ok`: hy <= H and hx <= W - a halo is at most one whole
    copy of the image; beyond that the class refuses, see test_ext_not_ok_shapes_have_a_halo_beyond_the_image): the
    rectangles lie inside the image and inside the extended region, none is empty, every element of the
    (H + 2 hy) x (W + 2 hx) region is written exactly once, and it receives pixel ((y - hy) mod H, (x - hx) mod W)."""
    tiled = refused = 0
    for H, W, kh, kw in _geometry_grid():
        e, hy, hx, Mh, Mw = U._ext_geometry(H, W, kh, kw)
        if hy > H or hx > W:
            refused += 1
            continue
        src = np.arange(H * W).reshape(H, W)
        dst = np.full((H + 2 * hy, W + 2 * hx), -1)
        hits = np.zeros_like(dst)
        wins = U._ext_windows(H, W, hy, hx)
        assert len(wins) == (3 if hy else 1) * (3 if hx else 1), (H, W, kh, kw)
        for sy, sx, dy, dx, nr, nc in wins:
            assert nr > 0 and nc > 0, (H, W, kh, kw)
            assert 0 <= sy and sy + nr <= H and 0 <= sx and sx + nc <= W, (H, W, kh, kw)
            assert 0 <= dy and dy + nr <= H + 2 * hy and 0 <= dx and dx + nc <= W + 2 * hx, (H, W, kh, kw)
            dst[dy:dy + nr, dx:dx + nc] = src[sy:sy + nr, sx:sx + nc]
            hits[dy:dy + nr, dx:dx + nc] += 1
        assert (hits == 1).all(), (H, W, kh, kw)
        yy, xx = np.mgrid[0:H + 2 * hy, 0:W + 2 * hx]
        assert np.array_equal(dst, src[(yy - hy) % H, (xx - hx) % W]), (H, W, kh, kw)
        tiled += 1
    assert tiled > 30000 and refused > 1000, (tiled, refused)


def test_ext_not_ok_shapes_have_a_halo_beyond_the_image():
    for H, W, kh, kw in EXT_NOT_OK:
        e, hy, hx, Mh, Mw = U._ext_geometry(H, W, kh, kw)
        assert hy > H and hx <= W, (H, W, kh, kw)
    for H, W, kh, kw in EXT_CASES:
        e, hy, hx, Mh, Mw = U._ext_geometry(H, W, kh, kw)
        assert hy <= H and hx <= W and L.fft_supported(Mh, Mw), (H, W, kh, kw)
        assert not L.fft_supported(H, W), (H, W)             # a side the FFT does not take: what the frame is for
    # what each case is there for
    geo = {c: U._ext_geometry(*c) for c in EXT_CASES}
    assert geo[(7, 22, 13, 1)][1:3] == (7, 0)
    assert geo[(14, 22, 1, 1)] == (0, 0, 0, 15, 24)
    assert geo[(97, 14, 5, 29)][2] == 14 and geo[(97, 14, 5, 29)][4] == 45
    assert geo[(11, 14, 21, 29)][1:3] == (11, 14)


@pytest.mark.parametrize("case", EXT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_numpy_model_of_the_extended_frame_equals_the_periodic_product(case):
    """The zero frame filled with the window copies, times the spectrum of _ext_kernel_frame, cut at (hy, hx): inside
    the window no term has wrapped around the frame, so it is the product of period (H, W) - to float64 rounding
    (1e-12 * max|x|; measured 3e-14 at worst)."""
    H, W, kh, kw = case
    x, psf = ext_case_inputs(H, W, kh, kw)
    want_conv, want_corr = periodic_products(x, psf)
    e, hy, hx, Mh, Mw = U._ext_geometry(H, W, kh, kw)
    F = np.fft.fft2(U._ext_kernel_frame(psf, H, Mh, Mw))
    frame = np.zeros((Mh, Mw))
    for sy, sx, dy, dx, nr, nc in U._ext_windows(H, W, hy, hx):
        frame[dy:dy + nr, dx:dx + nc] = x[sy:sy + nr, sx:sx + nc]
    X = np.fft.fft2(frame)
    conv = np.fft.ifft2(X * F).real[hy:hy + H, hx:hx + W]
    corr = np.fft.ifft2(X * F.conj()).real[hy:hy + H, hx:hx + W]
    bound = 1e-12 * float(np.abs(x).max())
    d_conv, d_corr = float(np.abs(conv - want_conv).max()), float(np.abs(corr - want_corr).max())
    print(f"extended frame model {case}: frame {Mh} x {Mw}, conv {d_conv:.2e} corr {d_corr:.2e}, bound {bound:.2e}")
    assert d_conv <= bound and d_corr <= bound, (case, d_conv, d_corr, bound)
