"""Batched wow over stacks of same-shape frames (wavelets_amd.wow_stack, wt_batch_wow_*) against the per-frame
utils.wow: bit-identical images and whitened planes, the golden fixture, frame isolation, chunking, fallbacks,
the batched MODE_DECOMP stencil passes of 9 and 10 scales and one wow launch per scale for any frame count."""
import numpy as np
import pytest

from conftest import measured_tol, load_golden

pytestmark = pytest.mark.gpu

WOW_TOL = 5.2e-6              # as tests/test_gpu_parity.py: wow() planes and image vs the reference

# the non-bilateral keyword cases of test_gpu_parity.WOW_CASES (g4_wow)
CASES = {
    "default": dict(),
    "triangle": dict(scaling_function="triangle"),
    "dc52": dict(denoise_coefficients=[5, 2]),
    "n3_w_dc": dict(n_scales=3, weights=[.5], denoise_coefficients=[5, 2]),
    "h05_g2": dict(h=.5, gamma=2, denoise_coefficients=[5, 2]),
    "h1": dict(h=1, denoise_coefficients=[5, 2]),
    "pv": dict(preserve_variance=True, denoise_coefficients=[5, 2]),
    "nowhite": dict(whitening=False, denoise_coefficients=[5, 2]),
    "hard": dict(denoise_coefficients=[5, 2], soft_threshold=False),
}


def _W():
    import wavelets_amd as W
    return W


def _bits(a):
    """the float32 bits, every NaN as the one quiet NaN (an all-zero frame's gamma blend is 0 / 0 in both paths)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), a).view(np.uint32)


def _kw(W, name, fam="B3spline"):
    kw = dict(CASES[name])
    kw["scaling_function"] = W.Triangle if kw.get("scaling_function") == "triangle" else getattr(W, fam)
    return kw


def _stack(n, H, W_, seed=0, zero=None):
    """n frames, amplitudes two decades apart (0.1 .. 10: per-frame tau / factor tables differ), frame `zero` all 0"""
    rng = np.random.default_rng(seed)
    fr = rng.standard_normal((n, H, W_)).astype(np.float32)
    fr *= np.logspace(-1, 1, n).astype(np.float32)[:, None, None]
    fr += np.float32(0.5) * fr[:, ::-1, :]                 # some structure across the frame
    if zero is not None:
        fr[zero] = 0
    return fr


def _per_frame(W, fr, noise, kw):
    per = list(noise) if isinstance(noise, (list, tuple)) else [noise] * len(fr)
    res = [W.wow(f, noise=n, **kw) for f, n in zip(fr, per)]
    return np.stack([r[0] for r in res]), np.stack([r[1].data for r in res])


def _noise_for(i, n):
    """None, a scalar, or a per-frame list that holds a 0 - in turn"""
    return (None, 0.7, [0.0] + [0.3 * (k + 1) for k in range(n - 1)])[i % 3]


def _check(W, fr, noise, kw, what):
    img, planes = W.wow_stack(fr, noise=noise, return_coefficients=True, **kw)
    exp_img, exp_planes = _per_frame(W, fr, noise, kw)
    assert img.shape == exp_img.shape and planes.shape == exp_planes.shape, what
    assert np.array_equal(_bits(img), _bits(exp_img)), f"{what}: image bits differ"
    assert np.array_equal(_bits(planes), _bits(exp_planes)), f"{what}: plane bits differ"
    return img, planes


SHAPES = [(512, 512), (300, 517), (64, 2048), (1000, 1000)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", ["B3spline", "Triangle"])
def test_wow_stack_is_bitwise_the_per_frame_wow(shape, fam):
    W = _W()
    H, Wd = shape
    for n in (1, 3, 17):
        fr = _stack(n, H, Wd, seed=n + H, zero=n // 2 if n == 17 else None)
        for i, name in enumerate(CASES):
            noise = _noise_for(i + n, n)
            _check(W, fr, noise, _kw(W, name, fam), f"{shape} {fam} n={n} {name} noise={noise!r}")
        # the image alone (no planes downloaded) is the same
        img = W.wow_stack(fr, **_kw(W, "h05_g2", fam))
        assert np.array_equal(_bits(img), _bits(_per_frame(W, fr, None, _kw(W, "h05_g2", fam))[0]))


@pytest.mark.parametrize("fam,name", [("B3spline", "default"), ("Triangle", "h05_g2"), ("B3spline", "dc52")])
def test_wow_stack_2048_at_the_default_nine_scales(fam, name):
    """2048^2: 9 scales by default - the lattice kernel runs the large scales of the update and the transform's
    single-scale pass without a fused kernel runs on the batched MODE_DECOMP stencil"""
    W = _W()
    fr = _stack(3, 2048, 2048, seed=5)
    img, planes = _check(W, fr, None, _kw(W, name, fam), f"2048^2 {fam} {name}")
    assert planes.shape == (3, 10, 2048, 2048)


def test_wow_stack_golden_fixture():
    W = _W()
    g = load_golden("g4_wow")
    a = g["img"]
    fr = np.stack([a, a * np.float32(0.25), a * np.float32(4)]).astype(np.float32)
    for name in CASES:
        kw = _kw(W, name)
        img, planes = W.wow_stack(fr, return_coefficients=True, **kw)
        ref_c, ref_r = g[f"coef_{name}"], g[f"recon_{name}"]
        assert planes[0].shape == ref_c.shape
        measured_tol(f"wow_stack planes {name}", planes[0], ref_c, atol=WOW_TOL * np.abs(ref_c).max(), rtol=WOW_TOL)
        measured_tol(f"wow_stack image {name}", img[0], ref_r, atol=WOW_TOL * max(1.0, np.abs(ref_r).max()), rtol=WOW_TOL)
        exp_img, exp_planes = _per_frame(W, fr, None, kw)
        assert np.array_equal(_bits(img), _bits(exp_img)) and np.array_equal(_bits(planes), _bits(exp_planes)), name


def test_wow_stack_frame_isolation():
    W = _W()
    fr = np.zeros((3, 300, 517), np.float32)
    rng = np.random.default_rng(3)
    fr[0] = rng.standard_normal((300, 517)).astype(np.float32) * 1e6
    fr[2] = rng.standard_normal((300, 517)).astype(np.float32) * 1e6
    for name in ("default", "h05_g2", "nowhite", "pv"):
        img, planes = W.wow_stack(fr, return_coefficients=True, **_kw(W, name))
        assert not np.any(_bits(planes[1])), name
        if CASES[name].get("h", 0) == 0:
            assert not np.any(_bits(img[1])), name            # (h > 0: the gamma blend of an all-zero frame is 0 / 0)
        exp_img, exp_planes = _per_frame(W, fr, None, _kw(W, name))
        assert np.array_equal(_bits(img), _bits(exp_img)) and np.array_equal(_bits(planes), _bits(exp_planes)), name


def test_wow_stack_small_chunks_give_the_same_bits(monkeypatch):
    W = _W()
    from wavelets_amd import _lib as L
    fr = _stack(7, 300, 517, seed=11)
    for name in ("dc52", "h05_g2"):
        kw = _kw(W, name)
        whole = W.wow_stack(fr, noise=[0.2, None, 0.0, 1.0, None, 3.0, None], return_coefficients=True, **kw)
        monkeypatch.setattr(L, "BATCH_BYTES", 3 * L.batch_frame_bytes(300, 517, 6))     # chunks of 2, 2, 2, 1 frames
        assert [n for _, n in L.batch_chunks(7, 300, 517, 6, extra_planes=2)] == [2, 2, 2, 1]
        parts = W.wow_stack(fr, noise=[0.2, None, 0.0, 1.0, None, 3.0, None], return_coefficients=True, **kw)
        monkeypatch.undo()
        assert np.array_equal(_bits(whole[0]), _bits(parts[0])) and np.array_equal(_bits(whole[1]), _bits(parts[1]))


def test_wow_stack_fallbacks_are_the_per_frame_loop():
    W = _W()
    fr = _stack(3, 128, 160, seed=13)
    f64 = fr.astype(np.float64)
    got = W.wow_stack(f64, denoise_coefficients=[5, 2])
    exp = _per_frame(W, f64, None, dict(denoise_coefficients=[5, 2]))[0]
    assert got.dtype == np.float64 and np.array_equal(got, exp)
    got, planes = W.wow_stack(fr, bilateral=1, return_coefficients=True)
    exp, exp_planes = _per_frame(W, fr, None, dict(bilateral=1))
    assert np.array_equal(_bits(got), _bits(exp)) and np.array_equal(_bits(planes), _bits(exp_planes))

    class Retapped(W.Triangle):                      # run-time taps (wow needs the class's sigma_e table)
        coefficients_1d = np.array([0.2, 0.6, 0.2])

    got, planes = W.wow_stack(fr, Retapped, n_scales=3, denoise_coefficients=[4], return_coefficients=True)
    exp, exp_planes = _per_frame(W, fr, None, dict(scaling_function=Retapped, n_scales=3, denoise_coefficients=[4]))
    assert np.array_equal(_bits(got), _bits(exp)) and np.array_equal(_bits(planes), _bits(exp_planes))


@pytest.mark.parametrize("level", [9, 10])
def test_batch_decompose_with_stencil_passes_is_the_transform(level):
    W = _W()
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    fr = _stack(2, 2048, 2048, seed=17)
    for fam, cls in ((L.B3SPLINE, W.B3spline), (L.TRIANGLE, W.Triangle)):
        bp = L.BatchPlan(ctx, 2, 2048, 2048, fam, level)
        try:
            bp.upload(L.PLANE_INPUT, fr)
            bp.decompose(2, L.PLANE_INPUT, level)
            got = np.stack([bp.download(s, 2) for s in range(level + 1)], axis=1)
        finally:
            bp.close()
        exp = np.stack([W.AtrousTransform(cls)(f, level).data for f in fr])
        assert np.array_equal(_bits(got), _bits(exp)), (fam, level)


def test_one_wow_launch_per_scale_for_any_frame_count():
    from wavelets_amd import _lib as L
    ctx = L.default_context()

    def wow_calls(n):
        fr = _stack(n, 512, 512, seed=n)
        bp = L.BatchPlan(ctx, n, 512, 512, L.B3SPLINE, 7)
        try:
            bp.upload(L.PLANE_INPUT, fr)
            bp.decompose(n, L.PLANE_INPUT, 7)
            ctx.sync()
            ctx.profile_reset()
            ctx.profile(True)
            for s in range(7):
                bp.wow_scale(n, s, s, [0.5] * n, True, [1.0] * n)
            bp.wow_update(n, 7, [0.0] * n, True, [2.0] * n)
            ctx.sync()
            ent = ctx.profile_entries()
            ctx.profile(False)
        finally:
            bp.close()
        return {k: v[0] for k, v in ent.items() if "wow" in k}

    two, many = wow_calls(2), wow_calls(16)
    assert two == many, (two, many)
    assert sum(two.values()) == 8                               # 7 scales + the last plane
