"""wow_signals / wow_along on the device (the signal engine's moments and wow kernels) against the per-signal loop
of utils.wow: bit-identical where no reduction takes part (whitening=False, preserve_variance=False), at the bounds of
the existing 1-D and float64 wow tests and against the float64 numpy oracle where the plane moments take part, the
moments themselves through the binding, the reference's own 1-D results (tests/golden/g14_wow_denoise_nd.npz), chunks,
more workgroups than are resident, wow_along on its axes, and ineligible stacks.

Bounds.  float32 against the loop and the fixture: atol = 3e-5 * max|ref|, the bound of tests/test_gpu_parity.py::
test_wow_and_denoise_nd_vs_golden for 1-D wow.  float64 against the loop: F64_WOW = 1e-10 * max|ref|, the bound of
tests/test_gpu_wow64_stack.py (its reference-fixture test) for float64 wow.  Against the oracle on float64 copies:
max|engine - oracle| <= max(2 * max|loop - oracle|, 4 * eps(T) * max|oracle|) - the engine and the loop differ only in
the fold order of the moments, so neither is systematically further from the oracle; 2 is the margin for that, the
floor covers a loop that happens to be exact.  Moments: |sum - ref| <= 2 * N * 2^-53 * sum|x|, the worst case of any
summation order in double."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

F32_WOW = 3e-5            # tests/test_gpu_parity.py, 1-D wow, times max|ref|
F64_WOW = 1e-10           # tests/test_gpu_wow64_stack.py, float64 wow, times max|ref|
FAMS = (("B3spline", "b3spline"), ("Triangle", "triangle"))
DTYPES = ("float32", "float64")
LENGTHS = (8, 9, 17, 255, 256, 257, 1000, "budget")
NOISES = (None, 1.25, [None, 0, 2.5])


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


def _mod():
    return __import__("importlib").import_module("wavelets_amd.wow_signals")


def _n(N, dtype):
    return (8192 if dtype == "float32" else 4096) if N == "budget" else N


def _stack(M, N, dtype, seed=0, constant=None):
    """seeded normal samples times 3 plus 10; row `constant` is flat (median 0, noise 0: significance one)"""
    a = np.random.default_rng(seed).standard_normal((M, N)) * 3 + 10
    if constant is not None:
        a[constant] = 10
    return a.astype(dtype)


def _loop(W, sig, noise, kw):
    per = list(noise) if isinstance(noise, (list, tuple)) else [noise] * len(sig)
    res = [W.wow(s, noise=n, **kw) for s, n in zip(sig, per)]
    return np.stack([r[0] for r in res]), np.stack([r[1].data for r in res])


def _engine(W, monkeypatch, sig, **kw):
    """wow_signals with the per-signal loop an error: the stack must run on the engine"""
    def boom(*a, **k):
        raise AssertionError("wow_signals ran the per-signal loop")
    with monkeypatch.context() as m:
        m.setattr(_mod(), "wow", boom)
        return W.wow_signals(sig, **kw)


# ---------------------------------------------------------------- bit-identity where no reduction is involved

@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("fam", [f for f, _ in FAMS])
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_reductions_the_engine_equals_the_loop_bit_for_bit(W, monkeypatch, dtype, fam, N):
    N = _n(N, dtype)
    cls = getattr(W, fam)
    sig = _stack(3, N, dtype, seed=N, constant=1)
    for dc in ([], [5, 2], [3, 0, 1]):
        for soft in (True, False):
            for noise in NOISES:
                kw = dict(scaling_function=cls, whitening=False, preserve_variance=False, denoise_coefficients=dc,
                          soft_threshold=soft)
                img, planes = _engine(W, monkeypatch, sig, noise=noise, return_coefficients=True, **kw)
                ref_img, ref_planes = _loop(W, sig, noise, kw)
                assert img.dtype == sig.dtype and planes.dtype == sig.dtype and planes.shape == ref_planes.shape
                np.testing.assert_array_equal(img, ref_img, err_msg=f"{dc} {soft} {noise}")
                np.testing.assert_array_equal(planes, ref_planes, err_msg=f"planes {dc} {soft} {noise}")
    assert dc == [3, 0, 1]
    out = np.empty_like(sig)
    got = _engine(W, monkeypatch, sig, out=out, noise=NOISES[-1], **kw)
    assert got is out
    np.testing.assert_array_equal(out, ref_img)
    # weights ride on the factors: still no reduction
    kw["weights"] = [0.5, 2]
    np.testing.assert_array_equal(_engine(W, monkeypatch, sig, noise=1.25, **kw), _loop(W, sig, 1.25, kw)[0])


# ---------------------------------------------------------------- whitening and preserve_variance

WHITE_CASES = {
    "default": dict(),
    "pv": dict(preserve_variance=True),
    "pv_nowhite": dict(preserve_variance=True, whitening=False),
    "w_dc": dict(weights=[0.5, 2], denoise_coefficients=[5, 2]),
    "pv_dc_hard": dict(preserve_variance=True, denoise_coefficients=[3, 0, 1], soft_threshold=False),
}


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("fam,ofam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_with_moments_the_engine_agrees_with_the_loop_and_the_oracle(W, monkeypatch, dtype, fam, ofam, N):
    from oracle import atrous_numpy as O
    N = _n(N, dtype)
    cls = getattr(W, fam)
    sig = _stack(3, N, dtype, seed=100 + N)
    eps = float(np.finfo(dtype).eps)
    bound = F32_WOW if dtype == "float32" else F64_WOW
    for name, case in WHITE_CASES.items():
        for noise in (None, [None, 0, 2.5]):
            kw = dict(case, scaling_function=cls)
            img, planes = _engine(W, monkeypatch, sig, noise=noise, return_coefficients=True, **kw)
            ref_img, ref_planes = _loop(W, sig, noise, kw)
            per = noise if isinstance(noise, list) else [noise] * 3
            okw = {k: (list(v) if isinstance(v, list) else v) for k, v in case.items()}
            orc = np.stack([O.wow(s.astype(np.float64), ofam, noise=n, **okw)[0] for s, n in zip(sig, per)])
            d_loop = float(np.abs(img.astype(np.float64) - ref_img).max())
            e_eng = float(np.abs(img - orc).max())
            e_loop = float(np.abs(ref_img - orc).max())
            top = float(np.abs(ref_img).max())
            print(f"{dtype} {fam} N={N} {name} noise={noise}: |engine-loop| {d_loop:.3e} (bound {bound * top:.3e}), "
                  f"|engine-oracle| {e_eng:.3e}, |loop-oracle| {e_loop:.3e}, floor {4 * eps * float(np.abs(orc).max()):.3e}")
            assert d_loop <= bound * top, (name, noise)
            assert float(np.abs(planes.astype(np.float64) - ref_planes).max()) <= bound * float(np.abs(ref_planes).max()), (name, noise)
            assert e_eng <= max(2 * e_loop, 4 * eps * float(np.abs(orc).max())), (name, noise)


# ---------------------------------------------------------------- the moments through the binding

@pytest.mark.parametrize("N", (1, 2, 255, 256, 257, "budget"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_moments_through_the_binding(W, dtype, N):
    from wavelets_amd import _lib as L
    N = _n(N, dtype)
    sig = _stack(4, N, dtype, seed=7 + N)
    level = 2
    sb = L.acquire_signals(L.default_context(), 4, N, L.B3SPLINE, level, np.dtype(dtype))
    try:
        sb.upload(sig)
        sb.decompose(4, level)
        planes = sb.download_planes(4).astype(np.float64)
        first = sb.moments(4)
        again = sb.moments(4)
    finally:
        L.release_signals(sb)
    assert first.shape == (4, level + 1, 2) and first.dtype == np.float64
    np.testing.assert_array_equal(first.view(np.uint64), again.view(np.uint64))
    u = 2.0 * N * 2.0 ** -53
    err_s = np.abs(first[..., 0] - planes.sum(axis=-1))
    err_q = np.abs(first[..., 1] - (planes * planes).sum(axis=-1))
    print(f"{dtype} N={N}: sum error {err_s.max():.3e}, sumsq error {err_q.max():.3e}")
    assert np.all(err_s <= u * np.abs(planes).sum(axis=-1))
    assert np.all(err_q <= u * (planes * planes).sum(axis=-1))


# ---------------------------------------------------------------- the reference's own results

ND_WOW_CASES = {                                   # tests/test_gpu_parity.py
    "default": dict(),
    "den": dict(denoise_coefficients=[5, 2], n_scales=3),
    "gamma": dict(denoise_coefficients=[4, 2], n_scales=2, h=0.5, gamma=2.5),
    "pv": dict(preserve_variance=True, weights=[0.5, 2]),
    "tri": dict(scaling_function="Triangle", denoise_coefficients=[3]),
}


def test_the_reference_fixture(W, monkeypatch):
    g = load_golden("g14_wow_denoise_nd")
    sig = np.ascontiguousarray(np.broadcast_to(g["sig"], (4, 300)))
    for name, case in ND_WOW_CASES.items():
        kw = {k: (list(v) if isinstance(v, list) else v) for k, v in case.items()}
        kw["scaling_function"] = W.Triangle if "scaling_function" in kw else W.B3spline
        if name == "gamma":
            assert not W.wow_signals_eligible(sig, kw["n_scales"], h=kw["h"])
            got = W.wow_signals(sig, **kw)
            one = W.wow(g["sig"].copy(), **kw)[0]
            for row in got:
                np.testing.assert_array_equal(row, one)
            continue
        assert W.wow_signals_eligible(sig, kw.get("n_scales"), kw["scaling_function"], noise_per_signal=[None] * 4)
        got = _engine(W, monkeypatch, sig, **kw)
        ref = g[f"wow_sig_{name}"]
        assert got.shape == (4, 300) and got.dtype == np.float32
        for row in got:
            np.testing.assert_allclose(row.astype(np.float64), ref.astype(np.float64), rtol=0, atol=F32_WOW * np.abs(ref).max())
            np.testing.assert_array_equal(row, got[0])


# ---------------------------------------------------------------- chunks and many workgroups

@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks_of_two_signals_give_the_bits_of_the_whole_stack(W, monkeypatch, dtype):
    sig = _stack(5, 300, dtype, seed=3)
    kw = dict(preserve_variance=True, denoise_coefficients=[5, 2], noise=[None, 1.0, None, 0, None], return_coefficients=True)
    whole = _engine(W, monkeypatch, sig, **kw)
    asked = []

    def by_two(M, N, level, itemsize):
        asked.append((M, N, level, itemsize))
        return [(f0, min(2, M - f0)) for f0 in range(0, M, 2)]
    monkeypatch.setattr(_mod(), "_chunks", by_two)
    parts = _engine(W, monkeypatch, sig, **kw)
    assert asked == [(5, 300, 6, np.dtype(dtype).itemsize)]
    np.testing.assert_array_equal(parts[0], whole[0])
    np.testing.assert_array_equal(parts[1], whole[1])


def test_more_workgroups_than_are_resident_and_a_single_signal(W, monkeypatch):
    sig = _stack(5000, 64, "float32", seed=5)
    rows = np.random.default_rng(6).choice(5000, 50, replace=False)
    kw = dict(whitening=False, denoise_coefficients=[5, 2])
    got = _engine(W, monkeypatch, sig, **kw)
    np.testing.assert_array_equal(got[rows], _loop(W, sig[rows], None, kw)[0])
    got = _engine(W, monkeypatch, sig, preserve_variance=True)
    ref = _loop(W, sig[rows], None, dict(preserve_variance=True))[0]
    np.testing.assert_allclose(got[rows].astype(np.float64), ref.astype(np.float64), rtol=0, atol=F32_WOW * np.abs(ref).max())
    for dtype in DTYPES:
        one = _stack(1, 257, dtype, seed=8)
        got = _engine(W, monkeypatch, one, whitening=False, denoise_coefficients=[5, 2])
        np.testing.assert_array_equal(got, _loop(W, one, None, dict(whitening=False, denoise_coefficients=[5, 2]))[0])
        assert _engine(W, monkeypatch, one).shape == (1, 257)


# ---------------------------------------------------------------- wow_along

def test_wow_along_equals_wow_signals_on_the_transposed_stack(W):
    rng = np.random.default_rng(11)
    cube = (rng.standard_normal((6, 40, 7)) * 3 + 10).astype(np.float32)
    flat = (rng.standard_normal((40, 33)) * 3 + 10)
    view = (rng.standard_normal((12, 40, 7)) * 3 + 10).astype(np.float32)[::2]
    assert not view.flags.c_contiguous
    kw = dict(preserve_variance=True, denoise_coefficients=[5, 2])
    for a, axis in ((cube, 1), (cube, -2), (flat, 0), (view, 1)):
        moved = np.moveaxis(a, axis, -1)
        sig = np.ascontiguousarray(moved).reshape(-1, a.shape[axis])
        want, wplanes = W.wow_signals(sig, return_coefficients=True, **kw)
        got, planes = W.wow_along(a, axis=axis, return_coefficients=True, **kw)
        assert got.shape == a.shape and got.dtype == a.dtype and got.flags.c_contiguous
        np.testing.assert_array_equal(got, np.moveaxis(want.reshape(moved.shape), -1, axis))
        assert planes.shape == (wplanes.shape[1],) + a.shape
        for s in range(planes.shape[0]):
            np.testing.assert_array_equal(planes[s], np.moveaxis(wplanes[:, s].reshape(moved.shape), -1, axis))
    # one noise level per signal, in the shape of the array without the axis
    noise = np.abs(rng.standard_normal((6, 7))) + 0.5
    got = W.wow_along(cube, axis=1, noise=noise, **kw)
    want = W.wow_signals(np.ascontiguousarray(np.moveaxis(cube, 1, -1)).reshape(42, 40), noise=list(noise.reshape(-1)), **kw)
    np.testing.assert_array_equal(got, np.moveaxis(want.reshape(6, 7, 40), -1, 1))
    # the last axis is wow_signals' own layout
    got = W.wow_along(cube, axis=2, **kw)
    np.testing.assert_array_equal(got, W.wow_signals(cube.reshape(-1, 7), **kw).reshape(cube.shape))
    out = np.empty_like(cube)
    assert W.wow_along(cube, axis=-1, out=out, **kw) is out
    np.testing.assert_array_equal(out, got)


# ---------------------------------------------------------------- ineligible stacks on the device

def test_ineligible_stacks_return_what_the_loop_returns(W):
    ints = np.round(_stack(3, 64, "float64", seed=9) * 100).astype(np.int16)
    long_ = _stack(2, 8193, "float32", seed=10)
    for sig in (ints, long_):
        assert not W.wow_signals_eligible(sig, None)
        kw = dict(denoise_coefficients=[5, 2])
        got, planes = W.wow_signals(sig, return_coefficients=True, **kw)
        ref, ref_planes = _loop(W, sig, None, kw)
        assert got.dtype == ref.dtype
        np.testing.assert_array_equal(got, ref)
        np.testing.assert_array_equal(planes, ref_planes)
