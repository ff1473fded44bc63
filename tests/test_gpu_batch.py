"""Batched transform / denoise of stacks of same-shape frames (wavelets_amd.batch, wt_batch) against the
per-frame API: bit-identical results, exact per-frame medians, frame isolation, chunking, one launch per pass."""
import numpy as np
import pytest

from conftest import measured_tol, load_golden

pytestmark = pytest.mark.gpu


def _W():
    import wavelets_amd as W
    return W


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stack(n, H, W_, seed=0, scales=None):
    rng = np.random.default_rng(seed)
    fr = rng.standard_normal((n, H, W_)).astype(np.float32)
    if scales is not None:
        fr *= np.asarray(scales, np.float32)[:, None, None]
    return fr


SHAPES = [(512, 512), (300, 517), (64, 2048), (1000, 1000)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", ["B3spline", "Triangle"])
def test_transform_stack_is_bitwise_the_per_frame_transform(shape, fam):
    W = _W()
    cls = getattr(W, fam)
    H, Wd = shape
    for n in (1, 3, 17):
        fr = _stack(n, H, Wd, seed=n)
        levels = range(2, 9) if n == 3 else (2, 6, 8)
        for level in levels:
            got = W.transform_stack(fr, level, cls)
            exp = np.stack([W.AtrousTransform(cls)(f, level).data for f in fr])
            assert got.shape == (n, level + 1, H, Wd)
            assert np.array_equal(_bits(got), _bits(exp)), (shape, fam, n, level)


DENOISE_CASES = [
    dict(weights=[5, 3]),
    dict(weights=[5, 3, 2]),
    dict(weights=[4, 2, 1, 0, 0]),
    dict(weights=[5, 3], soft_threshold=False),
    dict(weights=[5, 3, 2], soft_threshold=False),
    dict(weights=[4, 2, 1, 0, 0], soft_threshold=False),
]


@pytest.mark.parametrize("case", DENOISE_CASES, ids=lambda c: f"{c['weights']}-{'soft' if c.get('soft_threshold', True) else 'hard'}")
@pytest.mark.parametrize("fam", ["B3spline", "Triangle"])
def test_denoise_stack_is_bitwise_the_per_frame_denoise(case, fam):
    W = _W()
    cls = getattr(W, fam)
    # noise levels two decades apart: the per-frame tau table really differs from frame to frame
    fr = _stack(5, 300, 517, seed=3, scales=[0.01, 1.0, 100.0, 3.0, 0.5])
    soft = case.get("soft_threshold", True)
    for noise in (None, 0.7, [0.1, None, 2.0, 0.0, 1.5]):
        got = W.denoise_stack(fr, case["weights"], cls, noise=noise, soft_threshold=soft)
        per = noise if isinstance(noise, list) else [noise] * len(fr)
        exp = np.stack([W.denoise(f, case["weights"], cls, n_i, soft_threshold=soft) for f, n_i in zip(fr, per)])
        assert np.array_equal(_bits(got), _bits(exp)), (case, fam, noise)


def test_denoise_stack_anscombe_and_sizes():
    W = _W()
    rng = np.random.default_rng(7)
    fr = rng.poisson(20.0, (4, 512, 512)).astype(np.float32)
    got = W.denoise_stack(fr, [5, 3], W.Triangle, anscombe=True)
    exp = np.stack([W.denoise(f, [5, 3], W.Triangle, anscombe=True) for f in fr])
    assert np.array_equal(_bits(got), _bits(exp))
    fr = _stack(3, 64, 2048, seed=8)
    got = W.denoise_stack(list(fr), [5, 3, 2])
    exp = np.stack([W.denoise(f, [5, 3, 2]) for f in fr])
    assert np.array_equal(_bits(got), _bits(exp))


def test_batch_medians_are_exact():
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    rng = np.random.default_rng(11)
    for H, Wd in ((33, 31), (32, 48), (300, 517)):          # odd and even pixel counts
        fr = rng.standard_normal((5, H, Wd)).astype(np.float32)
        fr[1] = np.round(fr[1] * 4) / 4                       # ties
        fr[2] = 0.0                                           # all zero: median 0, tau 0
        fr[3] = -np.abs(fr[3]) * 1e-30                        # denormals and signs
        fr[4] = rng.integers(0, 3, (H, Wd)).astype(np.float32)
        bp = L.BatchPlan(ctx, 5, H, Wd, L.B3SPLINE, 2)
        try:
            bp.upload(L.PLANE_INPUT, fr)
            med = bp.abs_median(5, L.PLANE_INPUT)
            for f in range(5):
                exp = np.float32(np.median(np.abs(fr[f])))
                assert np.array_equal(np.float32(med[f]).view(np.uint32), exp.view(np.uint32)), (H, Wd, f, med[f], exp)
            bad = fr.copy()
            bad[3, 5, 7] = np.nan
            bp.upload(L.PLANE_INPUT, bad)
            with pytest.raises(L.WatrooHipError, match="frame 3"):
                bp.abs_median(5, L.PLANE_INPUT)
        finally:
            bp.close()


def test_frames_do_not_leak_into_each_other():
    W = _W()
    fr = np.zeros((3, 256, 384), np.float32)
    fr[0, :8] = 1e6
    fr[0, -8:] = -1e6
    fr[2, :8] = 1e6
    fr[2, -8:] = 1e6
    got = W.transform_stack(fr, 6)
    assert not np.any(got[1])
    exp = np.stack([W.AtrousTransform(W.B3spline)(f, 6).data for f in fr])
    assert np.array_equal(_bits(got), _bits(exp))
    den = W.denoise_stack(fr, [5, 3], noise=1.0)
    assert not np.any(den[1])


def test_stacked_golden_denoise():
    W = _W()
    g = load_golden("g2_denoise")
    a = g["img"].astype(np.float32)
    fr = np.stack([a, a * 0.25, a * 4.0])
    tol = 5.2e-7 * np.abs(a).max()          # test_gpu_parity.DENOISE_TOL
    for fam, cls in (("b3spline", W.B3spline), ("triangle", W.Triangle)):
        got = W.denoise_stack(fr, [5, 3], cls)
        measured_tol(f"batched denoise {fam}", got[0], g[f"denoise_53_{fam}"], tol)
        for i, sc in enumerate((0.25, 4.0), start=1):
            measured_tol(f"batched denoise {fam} x{sc}", got[i] / np.float32(sc), g[f"denoise_53_{fam}"], tol)
        got = W.denoise_stack(fr[:1], [5, 3], cls, noise=0.9)
        measured_tol(f"batched denoise noise= {fam}", got[0], g[f"denoise_53_noise_{fam}"], tol)


def test_small_chunks_give_the_same_bits(monkeypatch):
    W = _W()
    from wavelets_amd import _lib as L
    fr = _stack(7, 200, 300, seed=5, scales=[1, 2, 3, 4, 5, 6, 7])
    one = W.denoise_stack(fr, [5, 3, 2])
    t_one = W.transform_stack(fr, 5)
    monkeypatch.setattr(L, "BATCH_BYTES", 3 * L.batch_frame_bytes(200, 300, 5))
    assert [n for _, n in L.batch_chunks(7, 200, 300, 5)] == [3, 3, 1]
    assert np.array_equal(_bits(W.transform_stack(fr, 5)), _bits(t_one))
    monkeypatch.setattr(L, "BATCH_BYTES", 3 * L.batch_frame_bytes(200, 300, 3))
    assert np.array_equal(_bits(W.denoise_stack(fr, [5, 3, 2])), _bits(one))


def test_one_launch_per_fused_pass_whatever_the_frame_count():
    from wavelets_amd import _lib as L
    ctx = L.default_context()

    def fused_calls(n):
        bp = L.BatchPlan(ctx, n, 512, 512, L.B3SPLINE, 6)
        try:
            bp.upload(L.PLANE_INPUT, _stack(n, 512, 512))
            bp.decompose_sum(n, L.PLANE_INPUT, 6)
            ctx.sync()
            ctx.profile_reset()
            ctx.profile(True)
            bp.decompose_sum(n, L.PLANE_INPUT, 6)
            ctx.sync()
            ent = ctx.profile_entries()
            ctx.profile(False)
        finally:
            bp.close()
        return {k: v[0] for k, v in ent.items() if k.startswith("wt_fused")}

    one, many = fused_calls(1), fused_calls(16)
    assert one and one == many, (one, many)


def test_batch_decompose_sum_is_the_per_frame_sum():
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    fr = _stack(4, 300, 517, seed=9)
    bp = L.BatchPlan(ctx, 4, 300, 517, L.TRIANGLE, 7)
    try:
        bp.upload(L.PLANE_INPUT, fr)
        bp.decompose_sum(4, L.PLANE_INPUT, 7)
        got = bp.download(L.PLANE_OUT, 4)
    finally:
        bp.close()
    for f in range(4):
        p = L.acquire_plan(ctx, 300, 517, L.TRIANGLE, 7)
        p.upload(L.PLANE_INPUT, fr[f])
        p.decompose_sum(L.PLANE_INPUT, 7)
        assert np.array_equal(_bits(got[f]), _bits(p.download(L.PLANE_OUT)))
        L.release_plan(p)


def test_fallback_inputs_give_the_per_frame_results():
    W = _W()
    fr = _stack(3, 96, 128, seed=12)
    f64 = fr.astype(np.float64)
    got = W.denoise_stack(f64, [5, 3])
    exp = np.stack([W.denoise(f, [5, 3]) for f in f64])
    assert got.dtype == np.float64 and np.array_equal(got, exp)
    got = W.denoise_stack(fr, [5, 3], bilateral=1)
    exp = np.stack([W.denoise(f, [5, 3], bilateral=1) for f in fr])
    assert np.array_equal(_bits(got), _bits(exp))

    class Custom(W.AbstractScalingFunction):
        coefficients_1d = np.array([0.2, 0.6, 0.2])

        def __init__(self, n_dim):
            super().__init__("custom", n_dim)

    got = W.transform_stack(fr, 3, Custom)
    exp = np.stack([W.AtrousTransform(Custom)(f, 3).data for f in fr])
    assert np.array_equal(got, exp)
    got = W.transform_stack(fr, 1)                       # L = 1: no all-fused schedule
    exp = np.stack([W.AtrousTransform(W.B3spline)(f, 1).data for f in fr])
    assert np.array_equal(_bits(got), _bits(exp))


def test_denoise_stack_zero_frame_and_pipelined_reference():
    W = _W()
    fr = _stack(4, 300, 517, seed=21, scales=[1.0, 0.0, 5.0, 0.2])       # frame 1 all zero: median 0, tau 0
    for weights in ([5, 3], [4, 2, 1, 0, 0]):
        got = W.denoise_stack(fr, weights)
        exp = np.stack([W.denoise(f, weights) for f in fr])
        assert np.array_equal(_bits(got), _bits(exp)) and not np.any(got[1])
    # scalar noise at 2048^2: the per-frame reference is the pipelined host call (wt_denoise_sum_host)
    big = _stack(2, 2048, 2048, seed=22, scales=[1.0, 3.0])
    for noise in (0.8, np.array([0.5, 2.0])):
        got = W.denoise_stack(big, [5, 3, 2], noise=noise)
        per = list(noise) if isinstance(noise, np.ndarray) else [noise] * 2
        exp = np.stack([W.denoise(f, [5, 3, 2], noise=n) for f, n in zip(big, per)])
        assert np.array_equal(_bits(got), _bits(exp))


@pytest.mark.parametrize("name", ["BatchPlan", "BatchPlan64"])
def test_upload_download_round_trip_of_both_batches(name):
    """3 frames of 5 x 7: the odd width pads the rows of both pitches (4 floats, 2 doubles), H >= 2 as the float64
    batch needs.  What goes up comes back bit for bit: into a fresh block, into a cube[:, s] view, and after an upload
    of one frame at f0 = 1; the float64 batch also widens int16 and '>f4' frames to frames.astype(np.float64)."""
    from wavelets_amd import _lib as L
    cls = getattr(L, name)
    rng = np.random.default_rng(31)
    fr = rng.standard_normal((3, 5, 7)).astype(cls.dtype)
    bp = cls(L.default_context(), 3, 5, 7, L.B3SPLINE, 2)
    try:
        assert bp.pitch == 8 and bp.frame_stride >= 5 * 8
        bp.upload(L.PLANE_INPUT, fr)
        got = bp.download(L.PLANE_INPUT, 3)
        assert got.dtype == cls.dtype and np.array_equal(got, fr)
        cube = np.full((3, 4, 5, 7), -1, cls.dtype)
        bp.download(L.PLANE_INPUT, 3, out=cube[:, 2])
        assert np.array_equal(cube[:, 2], fr) and np.all(cube[:, [0, 1, 3]] == -1)
        other = rng.standard_normal((1, 5, 7)).astype(cls.dtype)
        bp.upload(L.PLANE_INPUT, other, f0=1)
        want = fr.copy()
        want[1] = other[0]
        assert np.array_equal(bp.download(L.PLANE_INPUT, 3), want)
        assert np.array_equal(bp.download(L.PLANE_INPUT, 2, f0=1), want[1:])
        if cls is L.BatchPlan64:
            for dt in (np.int16, ">f4"):
                typed = (rng.standard_normal((3, 5, 7)) * 300).astype(dt)
                bp.upload(L.PLANE_INPUT, typed)
                assert np.array_equal(bp.download(L.PLANE_INPUT, 3), typed.astype(np.float64))
    finally:
        bp.close()


@pytest.mark.parametrize("engine", ["f32", "f64"])
def test_threshold_sums_and_wow_update_of_a_batch_are_the_per_frame_calls(engine):
    """Every instantiation of the shared kernel bodies of the two engines (wt_batch.hip, wt_batch64.hip) against the
    per-frame Plan / Plan64 calls, bit for bit, on 3 frames of 6 x 10: the threshold sum without a noise plane, with
    one (a map on frame 1 only) and with per-frame weights (enhance_sum), n_den 2 of count 3 with one tau of 0, soft and
    hard, write_back on and off; wow_update with and without a gamma plane, with and without the noise plane."""
    from wavelets_amd import _lib as L
    f64 = engine == "f64"
    real = np.float64 if f64 else np.float32
    ctx = L.default_context()
    n, H, Wd, S = 3, 6, 10, L.PLANE_SCRATCH
    rng = np.random.default_rng(5)
    planes = (rng.standard_normal((3, n, H, Wd)) * 2).astype(real)          # [plane][frame]
    noise = np.ones((n, H, Wd), real)
    noise[1] = rng.uniform(0.5, 2.0, (H, Wd)).astype(real)
    gamma0 = rng.uniform(0.0, 1.0, (n, H, Wd)).astype(real)
    has_map = [False, True, False]
    taus = [[1.5, 0.0], [0.0, 0.7], [0.9, 1.1]]
    wgts = [[0.8, 1.25], [1.0, 0.3], [2.0, 0.6]]                            # enhance_sum: per frame; denoise_sum: wgts[0]
    wtau, wfac = [1.2, 0.0, 0.6], [0.5, 1.5, 0.25]

    bp = (L.BatchPlan64 if f64 else L.BatchPlan)(ctx, n, H, Wd, L.B3SPLINE, 2)
    pl = L.Plan64(ctx, H, Wd, (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16), 2) if f64 else L.Plan(ctx, H, Wd, L.B3SPLINE, 2)

    def load_batch():
        for k in range(3):
            bp.upload(k, planes[k])
        bp.upload(S(5), noise)
        bp.upload(S(4), gamma0)

    def load_frame(f):
        for k in range(3):
            pl.upload(k, planes[k][f])
        pl.upload(S(5), noise[f])
        pl.upload(S(4), gamma0[f])

    def same(got, exp, what):
        assert np.array_equal(np.asarray(got), np.asarray(exp), equal_nan=True), what

    try:
        for soft in (True, False):
            for write_back in (True, False):
                for kind in ("plain", "map", "enhance"):
                    load_batch()
                    if kind == "enhance":
                        bp.enhance_sum(n, 3, taus, wgts, soft=soft, write_back=write_back)
                    else:
                        bp.denoise_sum(n, 3, taus, wgts[0], soft=soft, write_back=write_back,
                                       noise_plane=S(5) if kind == "map" else L.PLANE_NONE, has_map=has_map)
                    got = [np.array(bp.download(p, n)) for p in (L.PLANE_OUT, 0, 1, 2)]
                    for f in range(n):
                        load_frame(f)
                        pl.denoise_sum(3, taus[f], wgts[f] if kind == "enhance" else wgts[0], soft,
                                       noise_plane=S(5) if kind == "map" and has_map[f] else L.PLANE_NONE,
                                       write_back=write_back, dst=L.PLANE_OUT)
                        for g, p in zip(got, (L.PLANE_OUT, 0, 1, 2)):
                            same(g[f], pl.download(p), (engine, kind, soft, write_back, f, p))
            for gamma in (S(4), L.PLANE_NONE):
                for with_noise in (False, True):
                    load_batch()
                    bp.wow_update(n, 2, wtau, soft, wfac, gamma_plane=gamma, noise_plane=S(5) if with_noise else L.PLANE_NONE)
                    got = [np.array(bp.download(p, n)) for p in (2, S(4))]
                    for f in range(n):
                        load_frame(f)
                        pl.wow_update(2, L.PLANE_NONE, wtau[f], soft, S(5) if with_noise and has_map[f] else L.PLANE_NONE,
                                      wfac[f], gamma)
                        for g, p in zip(got, (2, S(4))):
                            same(g[f], pl.download(p), (engine, "wow", soft, gamma, with_noise, f, p))
    finally:
        bp.close()
        pl.close()
