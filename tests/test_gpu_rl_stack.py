"""richardson_lucy_stack on the MI355X (wt_batch_filter2d / _binary / _mrs_update behind it).  Every case of
tests/test_rl_stack_cpu.py runs with the per-frame entry point it would fall back to patched to raise.  Soft-threshold
cases meet the float64 numpy oracle first - per frame, atol = 2e-4 * max|ref_frame| and rtol = 2e-4, the project's
bound for richardson_lucy (tests/test_gpu_round2.py), over all samples: the frames lie nine decades apart, so the 1e4
frame cannot hide the 1e-3 one.  Every case then equals the per-frame richardson_lucy bit for bit, through out= too;
the hard-threshold cases rest on that check alone (the per-frame call is pinned to the reference by the g9 fixtures).

One more test compares wt_batch_filter2d with wt_filter2d_ex on a plan of each frame, bit for bit, both borders, at
4096 taps and on the PSFs whose LDS tile needs the raised dynamic-LDS attribute."""
import numpy as np
import pytest

from test_rl_stack_cpu import CASES, CASE_IDS, case, case_inputs, case_reference, is_soft, make_frames, make_psf

pytestmark = pytest.mark.gpu

ATOL_OF_MAX, RTOL = 2e-4, 2e-4


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


@pytest.mark.parametrize("name", CASE_IDS)
def test_richardson_lucy_stack(name, monkeypatch):
    W, B, U, L = _mods()
    c = case(name)
    frames, psf = case_inputs(name)
    n = len(frames)
    chunks = []
    if c.get("chunk"):
        def forced(N, H, Wd, level, *a, **k):
            assert k.get("extra_planes") == B._rl_extra_planes(level)
            chunks.append([(f0, min(c["chunk"], N - f0)) for f0 in range(0, N, c["chunk"])])
            return chunks[-1]
        monkeypatch.setattr(L, "batch_chunks", forced)
    out = np.full(frames.shape, np.nan, np.float32)
    with monkeypatch.context() as m:
        _no_fallback(m, B)
        got = W.richardson_lucy_stack(frames, psf, **c["kw"])
        res = W.richardson_lucy_stack(frames, psf, out=out, **c["kw"])
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
        exp = U.richardson_lucy(frames[i].copy(), psf.copy(), **c["kw"])
        _same_bits(got[i], exp, f"{name} frame {i}")
    _same_bits(out, got, f"{name} out=")


def test_stack_of_one_frame_and_a_list_of_frames(monkeypatch):
    W, B, U, L = _mods()
    frames, psf = case_inputs("ragged_37x50_psf7x5")
    with monkeypatch.context() as m:
        _no_fallback(m, B)
        one = W.richardson_lucy_stack(frames[1:2], psf, iterations=2)
        lst = W.richardson_lucy_stack([f for f in frames], psf, iterations=2)
    _same_bits(one[0], U.richardson_lucy(frames[1].copy(), psf, iterations=2), "one frame")
    for i in range(len(frames)):
        _same_bits(lst[i], U.richardson_lucy(frames[i].copy(), psf, iterations=2), f"list frame {i}")


@pytest.mark.parametrize("psf_shape", [(64, 64), (256, 16), (16, 256)])
def test_batch_filter2d_equals_filter2d_ex_per_frame(psf_shape):
    """wt_batch_filter2d against wt_filter2d_ex on a plan of each frame, both borders, off-centre anchors: 64 x 64 is
    the 4096 taps of a single launch (a 40 KB tile); 256 x 16 (85 KB) and 16 x 256 (39 KB) have 4096 taps too, the
    first beyond the 64 KB a kernel gets without the raised dynamic-LDS attribute"""
    W, B, U, L = _mods()
    ctx = L.default_context()
    frames = make_frames(2, 70, 70, 11)
    kh, kw = psf_shape
    assert kh * kw == 4096 and L.batch_psf_ok(kh, kw)
    psf = make_psf(kh, kw)
    S, D = L.PLANE_SCRATCH(6), L.PLANE_SCRATCH(8)
    bp = L.BatchPlan(ctx, 2, 70, 70, L.B3SPLINE, 2)
    plan = L.Plan(ctx, 70, 70, L.B3SPLINE, 2)
    try:
        bp.upload(S, frames)
        bp.set_psf(0, psf)
        bp.set_psf(1, psf[::-1, ::-1])
        for slot, k in ((0, psf), (1, np.ascontiguousarray(psf[::-1, ::-1]))):
            for periodic, anchor in ((False, None), (True, (kh // 2 - 1, kw - 1 - kw // 2)), (False, (0, kw - 1)), (True, (kh - 1, 0))):
                bp.filter2d(2, S, D, slot, anchor=anchor, periodic=periodic)
                got = bp.download(D, 2)
                for f in range(2):
                    plan.upload(S, frames[f])
                    plan.filter2d(S, D, k, anchor=anchor, periodic=periodic)
                    _same_bits(got[f], plan.download(D), f"psf {psf_shape} slot {slot} periodic {periodic} anchor {anchor} frame {f}")
        # arguments the single launch does not take
        with pytest.raises(L.WatrooHipError, match="not applied in one launch"):
            bp.set_psf(0, make_psf(65, 64))
        with pytest.raises(L.WatrooHipError, match="src and dst must differ"):
            bp.filter2d(2, S, S, 1)
        with pytest.raises(L.WatrooHipError, match="anchor"):
            bp.filter2d(2, S, D, 1, anchor=(kh, 0))
        with pytest.raises(L.WatrooHipError, match="border"):
            L.check(L.load().wt_batch_filter2d(bp._h, 2, S, D, 1, 0, 0, 1))
        with pytest.raises(L.WatrooHipError, match="active frames"):
            bp.filter2d(3, S, D, 1)
    finally:
        plan.close()
        bp.close()


def test_batch_binary_and_mrs_update_equal_the_per_frame_calls():
    """wt_batch_binary (every op) and wt_batch_mrs_update (soft / hard, persistent or not, a frame with tau = 0) against
    wt_binary / wt_mrs_update on a plan of each frame, bit for bit"""
    W, B, U, L = _mods()
    ctx = L.default_context()
    rng = np.random.default_rng(3)
    n, H, Wd = 3, 21, 30
    a = (rng.standard_normal((n, H, Wd)) * np.array([1e-3, 1, 1e4])[:, None, None]).astype(np.float32)
    b = rng.uniform(0.5, 1.5, (n, H, Wd)).astype(np.float32)
    A, Bp, D, M = L.PLANE_SCRATCH(6), L.PLANE_SCRATCH(7), L.PLANE_SCRATCH(9), L.PLANE_SCRATCH(17)
    bp = L.BatchPlan(ctx, 4, H, Wd, L.B3SPLINE, 3)
    plan = L.Plan(ctx, H, Wd, L.B3SPLINE, 3)
    try:
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
                bp.upload(1, a)
                bp.upload(M, b if soft else (b > 1).astype(np.float32))
                for it in range(2):
                    bp.mrs_update(n, 1, M, taus, soft, persistent, 1.0 / (it + 1))
                gc, gm = bp.download(1, n), bp.download(M, n)
                for f in range(n):
                    plan.upload(1, a[f])
                    plan.upload(M, b[f] if soft else (b[f] > 1).astype(np.float32))
                    for it in range(2):
                        plan.mrs_update(1, M, taus[f], soft, L.PLANE_NONE, persistent, 1.0 / (it + 1))
                    _same_bits(gc[f], plan.download(1), f"mrs soft={soft} persistent={persistent} plane, frame {f}")
                    _same_bits(gm[f], plan.download(M), f"mrs soft={soft} persistent={persistent} support, frame {f}")
        with pytest.raises(L.WatrooHipError, match="not a plane of a batch"):
            bp.binary(n, "sub", A, Bp, L.PLANE_SCRATCH(11))
        with pytest.raises(L.WatrooHipError, match="not a plane of a batch"):
            bp.fill(n, L.PLANE_SCRATCH(19), 0.0)             # (support planes: one per scale of the batch, 16 .. 18)
    finally:
        plan.close()
        bp.close()
