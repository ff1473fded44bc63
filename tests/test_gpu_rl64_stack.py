"""richardson_lucy_stack over float64, integer and big-endian stacks on the MI355X (wt_batch64_filter2d / _binary /
_mrs_update behind it).  The three batched calls first equal their per-frame twins on a Plan64 of each frame, bit for
bit: the tiled correlation on every PSF shape and anchor the route produces, both borders, a PSF that reaches beyond
the frame; the five binary ops; the support update soft and hard, persistent or not.  Then every case of
tests/test_rl64_stack_cpu.py runs with the per-frame entry point it would fall back to patched to raise, and equals
the per-frame richardson_lucy bit for bit, through out= too.  The soft cases also meet the float64 numpy oracle: per
frame atol = 1e-9 * max|ref_frame|, rtol 0 - the bound tests/test_gpu_round4.py holds the per-frame float64 call to;
the hard-threshold case rests on the bit equality alone."""
import numpy as np
import pytest

from test_rl_stack_cpu import make_psf
from test_rl64_stack_cpu import CASES, CASE_IDS, case, case_inputs, case_reference, is_soft

pytestmark = pytest.mark.gpu

ATOL_OF_MAX = 1e-9


def _mods():
    import wavelets_amd as W
    from wavelets_amd import batch as B, utils as U, _lib as L
    return W, B, U, L


def _same_bits(got, exp, what):
    assert got.dtype == exp.dtype == np.float64 and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    g, e = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(exp).view(np.uint64)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _mixed(n, H, Wd, seed):
    """doubles of mixed sign and magnitude, another scale and another pattern per frame"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, H, Wd)) * 10.0 ** rng.integers(-3, 4, (n, H, Wd))
    return x * np.array([1e-3, 1.0, 1e4, 7.0])[:n, None, None]


def _psf64(kh, kw):
    """an asymmetric kh x kw kernel of doubles with digits beyond a float's, not normalised exactly: no tap is special"""
    wy = np.hanning(kh + 2)[1:-1] if kh > 1 else np.ones(1)
    wx = np.hanning(kw + 2)[1:-1] if kw > 1 else np.ones(1)
    k = (np.outer(wy, wx) + 0.05) * (1 + 0.3 * np.linspace(-1, 1, kh)[:, None] + 0.2 * np.linspace(-1, 1, kw)[None, :])
    return k / k.sum() * (1 + 1e-9 * np.arange(k.size).reshape(k.shape)) * 1.01


def _filter2d_case(L, bp, plan, frames, nf, psf, border_cases):
    S, D = L.PLANE_SCRATCH(6), L.PLANE_SCRATCH(8)
    for slot, (k, kw) in enumerate(border_cases):
        bp.set_psf(slot % 2, k)
        bp.filter2d(nf, S, D, slot % 2, **{a: b for a, b in kw.items() if a in ("anchor", "periodic")})
        got = bp.download(D, nf)
        for f in range(nf):
            plan.upload(S, frames[f])
            plan.filter2d(S, D, k, **kw)
            _same_bits(got[f], plan.download(D), f"psf {psf.shape} operand {k.shape} {kw} frame {f}")


@pytest.mark.parametrize("psf_shape", [(1, 1), (3, 3), (6, 4), (7, 5), (1, 9), (9, 1), (17, 33)])
def test_batch64_filter2d_equals_plan64_filter2d_per_frame(psf_shape):
    """3 x 37 x 70 frames: row tiles of 16, 16 and 5 rows, a full and a partial column tile.  Symmetric and periodic
    border with the centre anchor, and the operands and anchors richardson_lucy(fft=True) forms for an odd height
    (utils._rl_direct_operands: a zero row is added where the anchor leaves the PSF); nf = 3 of a batch of 4."""
    W, B, U, L = _mods()
    ctx = L.default_context()
    H, Wd = 37, 70
    frames = _mixed(3, H, Wd, 21)
    psf = _psf64(*psf_shape)
    flipped = np.ascontiguousarray(psf[::-1, ::-1])
    cases = [(flipped, {}), (psf, {}), (flipped, dict(periodic=True)), (psf, dict(periodic=True))]
    cases += list(U._rl_direct_operands(psf, H, True))
    bp = L.RLBatchPlan64(ctx, 4, H, Wd, L.B3SPLINE, 2)
    plan = L.Plan64(ctx, H, Wd, U._taps_f64(W.B3spline(2), 2), 2)
    try:
        bp.set_psf(0, psf)                                       # (richardson_lucy's planes come with the first PSF)
        bp.upload(L.PLANE_SCRATCH(6), frames)
        _filter2d_case(L, bp, plan, frames, 3, psf, cases)
    finally:
        plan.close()
        bp.close()


def test_batch64_filter2d_with_a_psf_that_reaches_beyond_the_frame_and_its_refusals():
    """a 21 x 5 PSF on 2 x 18 x 20 frames: the reach of 10 rows meets both borders of a frame at once (wt_refl bounces,
    the modulo wraps more than once); then the arguments the entry refuses"""
    W, B, U, L = _mods()
    ctx = L.default_context()
    H, Wd = 18, 20
    frames = _mixed(2, H, Wd, 22)
    psf = _psf64(21, 5)
    flipped = np.ascontiguousarray(psf[::-1, ::-1])
    wide = _psf64(3, 45)                                         # ... and further than the frame is wide
    S, D = L.PLANE_SCRATCH(6), L.PLANE_SCRATCH(8)
    bp = L.RLBatchPlan64(ctx, 2, H, Wd, L.B3SPLINE, 2)
    plan = L.Plan64(ctx, H, Wd, U._taps_f64(W.B3spline(2), 2), 2)
    try:
        with pytest.raises(L.WatrooHipError, match="not a plane of a batch"):
            bp.upload(S, frames)                                 # (no PSF yet: the plane list of every other stack function)
        bp.set_psf(0, psf)
        bp.upload(S, frames)
        _filter2d_case(L, bp, plan, frames, 2, psf, [(flipped, {}), (psf, {}), (psf, dict(periodic=True)),
                                                     (psf, dict(anchor=(0, 4))), (wide, {}), (wide, dict(periodic=True))])
        big = _psf64(64, 64)                                     # 4096 taps, an 80 KB tile: the raised dynamic-LDS attribute
        assert L.batch64_psf_ok(64, 64) and 127 * 79 * 8 > 64 * 1024
        _filter2d_case(L, bp, plan, frames, 2, big, [(big, {}), (big, dict(periodic=True, anchor=(31, 33)))])
        with pytest.raises(L.WatrooHipError, match="not applied in one launch"):
            bp.set_psf(0, np.ones((178, 1)))
    finally:
        plan.close()
        bp.close()
    bp = L.RLBatchPlan64(ctx, 2, H, Wd, L.B3SPLINE, 2)
    try:
        bp.set_psf(1, psf)
        with pytest.raises(L.WatrooHipError, match="slot 0 is not set"):
            bp.filter2d(2, S, D, 0)
        with pytest.raises(L.WatrooHipError, match="src and dst must differ"):
            bp.filter2d(2, S, S, 1)
        with pytest.raises(L.WatrooHipError, match="anchor"):
            bp.filter2d(2, S, D, 1, anchor=(21, 0))
        with pytest.raises(L.WatrooHipError, match="border"):
            L.check(L.load().wt_batch64_filter2d(bp._h, 2, S, D, 1, 0, 0, 1))
        with pytest.raises(L.WatrooHipError, match="active frames"):
            bp.filter2d(3, S, D, 1)
        with pytest.raises(L.WatrooHipError, match="must differ"):
            bp.mrs_update(2, 1, 1, [1.0, 1.0], True, True, 1.0)
        with pytest.raises(L.WatrooHipError, match="not a plane of a batch"):
            bp.binary(2, "sub", S, D, L.PLANE_SCRATCH(11))
        with pytest.raises(L.WatrooHipError, match="not a plane of a batch"):
            bp.fill(2, L.PLANE_SCRATCH(18), 0.0)                 # (support planes: one per scale of the batch, 16 and 17)
    finally:
        bp.close()


def test_batch64_binary_and_mrs_update_equal_the_plan64_calls():
    """wt_batch64_binary (every op) and wt_batch64_mrs_update (soft / hard, persistent or not, inv_pow 1 and 1/3, a
    frame with tau = 0) against wt64_binary / wt64_mrs_update on a Plan64 of each frame, bit for bit; an odd width, so
    the flat range crosses pitch padding"""
    W, B, U, L = _mods()
    ctx = L.default_context()
    rng = np.random.default_rng(3)
    n, H, Wd = 3, 21, 31
    a = _mixed(n, H, Wd, 23)
    b = rng.uniform(0.5, 1.5, (n, H, Wd))
    A, Bp, D, M = L.PLANE_SCRATCH(6), L.PLANE_SCRATCH(7), L.PLANE_SCRATCH(9), L.PLANE_SCRATCH(17)
    bp = L.RLBatchPlan64(ctx, 4, H, Wd, L.B3SPLINE, 3)
    plan = L.Plan64(ctx, H, Wd, U._taps_f64(W.B3spline(2), 2), 3)
    try:
        bp.set_psf(0, np.ones((1, 1)))                           # (richardson_lucy's planes come with the first PSF)
        bp.upload(A, a)
        bp.upload(Bp, b)
        for op in ("sub", "add", "mul", "div", "add_div"):
            bp.binary(n, op, A, Bp, D)
            got = bp.download(D, n)
            for f in range(n):
                plan.upload(A, a[f])
                plan.upload(Bp, b[f])
                plan.binary(op, A, Bp, D)
                _same_bits(got[f], plan.download(D), f"binary {op} frame {f}")
        taus = [2e-3, 0.0, 1.5e4]
        for soft in (True, False):
            for persistent in (True, False):
                support = b if soft else (b > 1).astype(np.float64)
                bp.upload(1, a)
                bp.upload(M, support)
                for inv_pow in (1.0, 1.0 / 3):
                    bp.mrs_update(n, 1, M, taus, soft, persistent, inv_pow)
                gc, gm = bp.download(1, n), bp.download(M, n)
                for f in range(n):
                    plan.upload(1, a[f])
                    plan.upload(M, support[f])
                    for inv_pow in (1.0, 1.0 / 3):
                        plan.mrs_update(1, M, taus[f], soft, L.PLANE_NONE, persistent, inv_pow)
                    _same_bits(gc[f], plan.download(1), f"mrs soft={soft} persistent={persistent} plane, frame {f}")
                    _same_bits(gm[f], plan.download(M), f"mrs soft={soft} persistent={persistent} support, frame {f}")
    finally:
        plan.close()
        bp.close()


def _no_fallback(monkeypatch, B):
    def refuse(*a, **k):
        raise AssertionError("richardson_lucy_stack fell back to the per-frame utils.richardson_lucy")
    monkeypatch.setattr(B, "richardson_lucy", refuse)


@pytest.mark.parametrize("name", CASE_IDS)
def test_richardson_lucy_stack_float64(name, monkeypatch):
    W, B, U, L = _mods()
    c = case(name)
    frames, psf = case_inputs(name)
    n = len(frames)
    chunks = []
    if c.get("chunk"):
        def forced(N, H, Wd, level, *a, **k):
            assert k.get("extra_planes") == B._rl_extra_planes(level) == level + 4 and k.get("itemsize") == 8
            chunks.append([(f0, min(c["chunk"], N - f0)) for f0 in range(0, N, c["chunk"])])
            return chunks[-1]
        monkeypatch.setattr(L, "batch_chunks", forced)
    out = np.full(frames.shape, np.nan, np.float64)
    with monkeypatch.context() as m:
        _no_fallback(m, B)
        got = W.richardson_lucy_stack(frames, psf, **c["kw"])
        res = W.richardson_lucy_stack(frames, psf, out=out, **c["kw"])
    assert res is out
    if c.get("chunk"):
        assert chunks and chunks[0][-1][1] < c["chunk"] <= n        # the last chunk is shorter than the batch
    assert got.shape == frames.shape and got.dtype == np.float64
    exp = [U.richardson_lucy(frames[i].copy(), psf.copy(), **c["kw"]) for i in range(n)]
    if is_soft(c):
        ref = case_reference(name)
        for i in range(n):
            tol = ATOL_OF_MAX * np.abs(ref[i]).max()
            worst, loop = float(np.abs(got[i] - ref[i]).max() / tol), float(np.abs(exp[i] - ref[i]).max() / tol)
            print(f"{name} frame {i}: worst error {worst:.3e} of the tolerance (the per-frame call: {loop:.3e})")
            assert worst <= 1.0, f"{name} frame {i}: {worst:.3e} of atol 1e-9 max|ref| against the float64 oracle"
    for i in range(n):
        _same_bits(got[i], exp[i], f"{name} frame {i}")
    _same_bits(out, got, f"{name} out=")
