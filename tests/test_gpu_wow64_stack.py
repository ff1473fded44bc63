"""wow over float64 and integer frame stacks (wavelets_amd.wow_stack on the float64 batch, wt_batch64_wow_*) against
the per-frame utils.wow: bit-identical images and whitened planes, every kernel choice of the batched float64 stencil
against Plan64.wow_scale, the transform's stencil passes at 9 and 10 scales, noise maps, the bilateral march, routing,
one launch per scale for any frame count, chunking, frame isolation and the reference's own float64 output."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

# the nine keyword cases of tests/test_gpu_wow_stack.py
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
    """the float64 bits, every NaN as the one quiet NaN (an all-zero frame's gamma blend is 0 / 0 in both paths)"""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)


def _kw(W, name, fam="B3spline"):
    kw = dict(CASES[name])
    kw["scaling_function"] = W.Triangle if kw.get("scaling_function") == "triangle" else getattr(W, fam)
    return kw


def _stack(n, H, W_, seed=0, zero=None, dtype=np.float64):
    """n frames, amplitudes two decades apart (per-frame tau / factor tables differ) on a pedestal, frame `zero` all 0;
    integer types: counts of a few thousand"""
    rng = np.random.default_rng(seed)
    fr = rng.standard_normal((n, H, W_))
    fr *= np.logspace(-1, 1, n)[:, None, None]
    fr += 0.5 * fr[:, ::-1, :]                              # some structure across the frame
    if np.dtype(dtype).kind in "iu":
        fr = np.clip(np.round(fr * 300 + 3000), 0, 30000)
    if zero is not None:
        fr[zero] = 0
    return fr.astype(dtype)


def _per_frame(W, fr, noise, kw):
    per = list(noise) if isinstance(noise, (list, tuple)) else [noise] * len(fr)
    res = [W.wow(f, noise=n, **kw) for f, n in zip(fr, per)]
    return np.stack([r[0] for r in res]), np.stack([r[1].data for r in res])


def _noise_for(i, n):
    """None, a scalar, or a per-frame list that holds a 0 - in turn"""
    return (None, 0.7, [0.0] + [0.3 * (k + 1) for k in range(n - 1)])[i % 3]


def _batched(monkeypatch):
    """from here on the per-frame loop of wow_stack is an error: the stack must run on the batch"""
    from wavelets_amd import batch as B

    def boom(*a, **k):
        raise AssertionError("wow_stack ran the per-frame loop")
    monkeypatch.setattr(B, "wow", boom)


def _check(W, fr, noise, kw, what, monkeypatch):
    exp_img, exp_planes = _per_frame(W, fr, noise, kw)
    with monkeypatch.context() as m:
        _batched(m)
        img, planes = W.wow_stack(fr, noise=noise, return_coefficients=True, **kw)
    assert img.dtype == np.float64 and planes.dtype == np.float64, what
    assert exp_img.dtype == np.float64 and exp_planes.dtype == np.float64, what
    assert img.shape == exp_img.shape and planes.shape == exp_planes.shape, what
    assert np.array_equal(_bits(img), _bits(exp_img)), f"{what}: image bits differ"
    assert np.array_equal(_bits(planes), _bits(exp_planes)), f"{what}: plane bits differ"
    return img, planes


SHAPES = [(512, 512), (300, 517), (64, 2048)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", ["B3spline", "Triangle"])
def test_wow_stack_is_bitwise_the_per_frame_wow(shape, fam, monkeypatch):
    W = _W()
    H, Wd = shape
    for n in (1, 3, 9):
        fr = _stack(n, H, Wd, seed=n + H, zero=n // 2 if n == 9 else None)
        for i, name in enumerate(CASES):
            noise = _noise_for(i + n, n)
            _check(W, fr, noise, _kw(W, name, fam), f"{shape} {fam} n={n} {name} noise={noise!r}", monkeypatch)


@pytest.mark.parametrize("dtype,shape", [(np.int16, (300, 517)), (">f4", (512, 512)), (np.uint16, (64, 2048))],
                         ids=["int16", "big-endian-f4", "uint16"])
def test_wow_stack_of_integer_and_byteswapped_frames(dtype, shape, monkeypatch):
    W = _W()
    fr = _stack(3, *shape, seed=21, dtype=dtype)
    assert fr.dtype == np.dtype(dtype)
    for i, name in enumerate(("default", "dc52", "h05_g2", "pv")):
        _check(W, fr, _noise_for(i, 3), _kw(W, name), f"{dtype} {name}", monkeypatch)


@pytest.mark.parametrize("width", [517, 512, 200])
def test_batched_wow_scale_is_plan64_wow_scale_for_every_kernel_choice(width):
    """wt_launch_stencil's choices at H = 300: W = 517 (odd: no lattice) - the row kernel at 4 waves (s = 0, 1, 5) and at
    8 (s = 6), the chain at d = 128; W = 512 - the lattice with 4 columns at d = 64, 128; W = 200 - with 2 columns at
    d = 64 (wow_stack never gets there: it caps n_scales by the short side).  Plain, with the gamma plane, with the
    noise plane, with both."""
    W = _W()
    from wavelets_amd import _lib as L
    from wavelets_amd.wavelets import _taps_f64, _NOISE_PLANE
    from wavelets_amd.utils import _GAMMA_PLANE
    ctx = L.default_context()
    H, n = 300, 3
    rng = np.random.default_rng(width)
    coef = rng.standard_normal((n, H, width)) * np.array([0.1, 1.0, 30.0])[:, None, None]
    maps = np.abs(rng.standard_normal((n, H, width))) + 0.1
    maps[1, 5, 7] = 0.0
    gam0 = rng.standard_normal((n, H, width))
    taus, factors = [0.8, 0.0, 12.5], [1.0 / 3.0, 2.0, 0.7]
    for fam, cls in ((L.B3SPLINE, W.B3spline), (L.TRIANGLE, W.Triangle)):
        bp = L.BatchPlan64(ctx, n, H, width, fam, 7)
        plan = L.Plan64(ctx, H, width, _taps_f64(cls, 2), 7)
        try:
            for s in (0, 1, 5, 6, 7):
                for gamma, noise in ((False, False), (True, False), (False, True), (True, True)):
                    for soft in ((True, False) if s == 1 else (True,)):
                        bp.upload(s, coef)
                        if gamma:
                            bp.upload(_GAMMA_PLANE, gam0)
                        if noise:
                            bp.fill(n, _NOISE_PLANE, 1.0)
                            bp.upload(_NOISE_PLANE, maps)
                        bp.wow_scale(n, s, s, taus, soft, factors, _GAMMA_PLANE if gamma else L.PLANE_NONE,
                                     **(dict(noise_plane=_NOISE_PLANE) if noise else {}))
                        got = bp.download(s, n)
                        got_g = bp.download(_GAMMA_PLANE, n) if gamma else None
                        for f in range(n):
                            plan.upload(s, coef[f])
                            if gamma:
                                plan.upload(_GAMMA_PLANE, gam0[f])
                            if noise:
                                plan.upload(_NOISE_PLANE, maps[f])
                            plan.wow_scale(s, s, taus[f], soft, _NOISE_PLANE if noise else L.PLANE_NONE, factors[f],
                                           _GAMMA_PLANE if gamma else L.PLANE_NONE)
                            what = (width, fam, s, gamma, noise, soft, f)
                            assert np.array_equal(_bits(got[f]), _bits(plan.download(s))), what
                            if gamma:
                                assert np.array_equal(_bits(got_g[f]), _bits(plan.download(_GAMMA_PLANE))), what
        finally:
            bp.close()
            plan.close()


def test_batched_pointwise_steps_are_plan64s():
    """wow_update (with and without the noise and gamma planes), reduce, gamma_blend and plane_sum of a BatchPlan64
    against the Plan64 calls, frame by frame, on an odd width"""
    W = _W()
    from wavelets_amd import _lib as L
    from wavelets_amd.wavelets import _taps_f64, _NOISE_PLANE
    from wavelets_amd.utils import _GAMMA_PLANE
    ctx = L.default_context()
    n, H, Wd, level = 3, 300, 517, 4
    rng = np.random.default_rng(9)
    planes = rng.standard_normal((level + 1, n, H, Wd)) * np.array([1e-3, 1.0, 1e3])[None, :, None, None] + 7.0
    maps = np.abs(rng.standard_normal((n, H, Wd)))
    taus, factors = [0.8, 0.0, 900.0], [1.0 / 3.0, 2.0, 0.7]
    gmins, gmaxs = [-1.0, 0.25, 3.0], [9.5, 8.0, 2000.0]
    bp = L.BatchPlan64(ctx, n, H, Wd, L.B3SPLINE, level)
    plan = L.Plan64(ctx, H, Wd, _taps_f64(W.B3spline, 2), level)
    try:
        for s in range(level + 1):
            bp.upload(s, planes[s])
        bp.fill(n, _NOISE_PLANE, 1.0)
        bp.upload(_NOISE_PLANE, maps)
        bp.fill(n, _GAMMA_PLANE, 0.0)
        bp.wow_update(n, 0, taus, True, factors, _GAMMA_PLANE, noise_plane=_NOISE_PLANE)
        bp.wow_update(n, 1, taus, False, factors, _GAMMA_PLANE)
        bp.wow_update(n, 2, taus, True, factors)
        moments = bp.reduce(n, 3)
        bp.plane_sum(n, 0, level + 1, L.PLANE_OUT)
        total = bp.download(L.PLANE_OUT, n)
        bp.gamma_blend(n, L.PLANE_OUT, _GAMMA_PLANE, gmins, gmaxs, 1 / 2.2, 0.4)
        got = [bp.download(s, n) for s in range(3)] + [bp.download(_GAMMA_PLANE, n), total, bp.download(L.PLANE_OUT, n)]
        for f in range(n):
            for s in range(level + 1):
                plan.upload(s, planes[s, f])
            plan.upload(_NOISE_PLANE, maps[f])
            plan.fill(_GAMMA_PLANE, 0.0)
            plan.wow_update(0, L.PLANE_NONE, taus[f], True, _NOISE_PLANE, factors[f], _GAMMA_PLANE)
            plan.wow_update(1, L.PLANE_NONE, taus[f], False, L.PLANE_NONE, factors[f], _GAMMA_PLANE)
            plan.wow_update(2, L.PLANE_NONE, taus[f], True, L.PLANE_NONE, factors[f], L.PLANE_NONE)
            assert plan.reduce(3) == moments[f], f
            plan.plane_sum(0, level + 1, L.PLANE_OUT)
            exp_total = plan.download(L.PLANE_OUT).copy()
            plan.gamma_blend(L.PLANE_OUT, _GAMMA_PLANE, gmins[f], gmaxs[f], 1 / 2.2, 0.4)
            exp = [plan.download(s).copy() for s in range(3)] + [plan.download(_GAMMA_PLANE).copy(), exp_total, plan.download(L.PLANE_OUT)]
            for k, (g, e) in enumerate(zip(got, exp)):
                assert np.array_equal(_bits(g[f]), _bits(e)), (f, k)
    finally:
        bp.close()
        plan.close()


@pytest.mark.parametrize("level", [9, 10])
def test_batch64_decompose_with_stencil_passes_is_the_transform(level):
    W = _W()
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    fr = _stack(2, 640, 512, seed=17)
    for fam, cls in ((L.B3SPLINE, W.B3spline), (L.TRIANGLE, W.Triangle)):
        assert not L.batch64_fused_ok(fam, 640, 512, level) and L.batch64_wow_ok(fam, 640, 512, level)
        bp = L.BatchPlan64(ctx, 2, 640, 512, fam, level)
        try:
            bp.upload(L.PLANE_INPUT, fr)
            bp.decompose(2, L.PLANE_INPUT, level)
            got = np.stack([bp.download(s, 2) for s in range(level + 1)], axis=1)
        finally:
            bp.close()
        exp = np.stack([W.AtrousTransform(cls)(f.astype(np.float64), level).data for f in fr])
        assert exp.dtype == np.float64 and np.array_equal(_bits(got), _bits(exp)), (fam, level)


def test_wow_stack_2048_at_the_default_nine_scales(monkeypatch):
    """2 x 2048^2 float64: 9 scales by default - the transform's single-scale pass behind the fused ones and the
    lattice kernel in the updates of the large scales"""
    W = _W()
    fr = _stack(2, 2048, 2048, seed=5)
    exp = np.stack([W.wow(f)[0] for f in fr])
    _batched(monkeypatch)
    img = W.wow_stack(fr)
    assert np.array_equal(_bits(img), _bits(exp))


def test_wow_stack_with_noise_maps(monkeypatch):
    W = _W()
    H, Wd = 320, 260
    rng = np.random.default_rng(31)
    shared = np.abs(rng.standard_normal((H, Wd))).astype(np.float32) + np.float32(0.05)
    shared[3, 4] = 0
    own = np.abs(rng.standard_normal((H, Wd))) * 2.0
    for dtype in (np.float64, np.int16):
        fr = _stack(4, H, Wd, seed=33, dtype=dtype)
        for name in ("dc52", "h05_g2", "nowhite", "hard"):
            kw = _kw(W, name)
            exp = [W.wow(f, noise=shared, **kw) for f in fr]
            with monkeypatch.context() as m:
                _batched(m)
                img, planes = W.wow_stack(fr, noise=shared, return_coefficients=True, **kw)
            assert np.array_equal(_bits(img), _bits(np.stack([e[0] for e in exp]))), (dtype, name, "shared")
            assert np.array_equal(_bits(planes), _bits(np.stack([e[1].data for e in exp]))), (dtype, name, "shared")
            _check(W, fr, [own, 2.5, None, shared], kw, f"{dtype} {name} mixed maps", monkeypatch)


@pytest.mark.parametrize("bilateral", [1, [1, 2]], ids=["1", "list"])
def test_wow_stack_with_bilateral_filtering(bilateral, monkeypatch):
    W = _W()
    fr = _stack(3, 300, 517, seed=41) + 50.0
    for name, fam in (("default", "B3spline"), ("dc52", "Triangle"), ("h05_g2", "B3spline")):
        kw = dict(_kw(W, name, fam), bilateral=bilateral)
        _check(W, fr, _noise_for(1, 3) if name == "dc52" else None, kw, f"bilateral={bilateral} {name}", monkeypatch)
    _check(W, fr, None, dict(_kw(W, "dc52"), bilateral=bilateral, bilateral_scaling=True), "bilateral_scaling", monkeypatch)


def test_float64_stacks_no_longer_run_the_per_frame_loop(monkeypatch):
    W = _W()
    fr = _stack(3, 64, 80, seed=2)
    exp = _per_frame(W, fr, None, dict(denoise_coefficients=[5, 2]))[0]
    _batched(monkeypatch)
    out = np.empty((3, 64, 80))
    got = W.wow_stack(fr, denoise_coefficients=[5, 2], out=out)
    assert got is out and np.array_equal(_bits(got), _bits(exp))
    got = W.wow_stack([f for f in fr.astype(np.int32)], denoise_coefficients=[5, 2])      # a sequence of frames
    assert got.dtype == np.float64 and got.shape == (3, 64, 80)


def test_one_wow_launch_per_scale_for_any_frame_count():
    from wavelets_amd import _lib as L
    ctx = L.default_context()

    def wow_calls(n):
        fr = _stack(n, 512, 512, seed=n)
        bp = L.BatchPlan64(ctx, n, 512, 512, L.B3SPLINE, 7)
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


def test_wow_stack_small_chunks_give_the_same_bits(monkeypatch):
    W = _W()
    from wavelets_amd import _lib as L
    fr = _stack(7, 300, 517, seed=11)
    noise = [0.2, None, 0.0, 1.0, None, 3.0, None]
    _batched(monkeypatch)
    for name in ("dc52", "h05_g2"):
        kw = _kw(W, name)
        whole = W.wow_stack(fr, noise=noise, return_coefficients=True, **kw)
        with monkeypatch.context() as m:
            m.setattr(L, "BATCH_BYTES", 3 * L.batch_frame_bytes(300, 517, 6, itemsize=8))     # chunks of 2, 2, 2, 1 frames
            assert [n for _, n in L.batch_chunks(7, 300, 517, 6, extra_planes=2, itemsize=8)] == [2, 2, 2, 1]
            parts = W.wow_stack(fr, noise=noise, return_coefficients=True, **kw)
        assert np.array_equal(_bits(whole[0]), _bits(parts[0])) and np.array_equal(_bits(whole[1]), _bits(parts[1])), name


def test_wow_stack_frame_isolation(monkeypatch):
    W = _W()
    _batched(monkeypatch)
    fr = _stack(4, 300, 517, seed=3)
    other = fr.copy()
    other[2] = _stack(1, 300, 517, seed=99)[0] * 1e6
    for name in ("default", "h05_g2", "pv"):
        a = W.wow_stack(fr, return_coefficients=True, **_kw(W, name))
        b = W.wow_stack(other, return_coefficients=True, **_kw(W, name))
        for k in (0, 1, 3):                                     # changing frame 2 changes slot 2 only
            assert np.array_equal(_bits(a[0][k]), _bits(b[0][k])) and np.array_equal(_bits(a[1][k]), _bits(b[1][k])), (name, k)
        assert not np.array_equal(_bits(a[0][2]), _bits(b[0][2])), name


def test_wow_stack_against_the_references_float64_output(monkeypatch):
    """g20_float64 holds the reference's own wow of a float64 image.  The bound is the one the per-frame parity test
    applies to this fixture (tests/test_gpu_round2.py::test_float64_engine_vs_golden): 1e-10 of the maximum of the
    reference's planes / image (whitening divides by the local power); for the hard threshold at most 2 coefficients
    beyond it (ties within the rounding of tau)."""
    W = _W()
    g = load_golden("g20_float64")
    b = g["wow_img"]
    assert b.dtype == np.float64 and b.size >= 1024
    _batched(monkeypatch)
    fr = np.stack([b, b * 0.25, b * 4.0])
    cases = {"den": dict(denoise_coefficients=[5, 2], n_scales=3),                                   # B3spline
             "tri_hard": dict(scaling_function=W.Triangle, denoise_coefficients=[3, 1], soft_threshold=False, n_scales=4)}
    for name, kw in cases.items():
        img, planes = W.wow_stack(fr, return_coefficients=True, **kw)
        ref_r, ref_c = g[f"wow_{name}"], g[f"wow_{name}_coef"]
        assert planes[0].shape == ref_c.shape and img[0].shape == ref_r.shape
        err_c = np.abs(planes[0] - ref_c)
        print(f"wow_stack vs g20 {name}: planes {err_c.max() / np.abs(ref_c).max():.3e}, "
              f"image {np.abs(img[0] - ref_r).max() / np.abs(ref_r).max():.3e} (relative to the reference's maximum)")
        if name == "tri_hard":
            assert (err_c > 1e-10 * np.abs(ref_c).max()).sum() <= 2
        else:
            assert err_c.max() <= 1e-10 * float(np.abs(ref_c).max())
            assert np.abs(img[0] - ref_r).max() <= 1e-10 * float(np.abs(ref_r).max())
