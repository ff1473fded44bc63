"""denoise_stack / wow_stack with per-pixel noise maps on the batched engines (the noise plane of wt_batch /
wt_batch64, wt_batch_denoise_sum_map, wt_batch64_denoise_sum_map, wt_batch_wow_update_map, wt_batch_wow_scale_map and
the batched MODE_WOW stencil): every result equals the per-frame call of this package - denoise(f, ..., noise=map_i),
wow(f, ..., noise=map_i) - bit for bit (the raw bits compared, NaNs included: a zero in a map under a zero coefficient
gives one).  For the whole module the per-frame fallback of batch.py is patched to raise: what succeeds ran the
batch.  The per-frame call itself is held against the numpy oracle on one small frame with a map, at
test_gpu_parity.DENOISE_TOL.  Inputs: tests/test_noise_map_stack_cpu.py."""
import numpy as np
import pytest

from test_noise_map_stack_cpu import (SHAPE_ODD, N_ODD, SHAPE_ROW, N_ROW, SHAPE_F64, N_F64, SHAPE_BLOCKS, N_BLOCKS,
                                      ORACLE_WEIGHTS, frames_of, noise_map, noise_arg, oracle_case)

pytestmark = pytest.mark.gpu

FAMILIES = ("B3spline", "Triangle")
WEIGHTS = {2: [5, 0], 5: [4, -2, 0, 1.5, 0]}           # levels 2 and 5: weights with a 0 and a negative value


@pytest.fixture
def no_fallback(monkeypatch):
    """the names the per-frame fallback of batch.py calls, patched to raise"""
    from wavelets_amd import batch as B

    def boom(*a, **k):
        raise AssertionError("the per-frame fallback ran")
    monkeypatch.setattr(B, "AtrousTransform", boom)
    monkeypatch.setattr(B, "denoise", boom)
    monkeypatch.setattr(B, "wow", boom)


def _W():
    import wavelets_amd as W
    return W


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    g, e = _bits(got), _bits(exp)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at index {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _per_frame_denoise(fr, weights, cls, per, **kw):
    from wavelets_amd.utils import denoise                      # (the per-frame function itself, not batch.denoise)
    return np.stack([denoise(f, list(weights), cls, n, **kw) for f, n in zip(fr, per)])


def _per_frame_wow(fr, cls, per, **kw):
    from wavelets_amd.utils import wow
    res = [wow(f, cls, noise=n, **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}) for f, n in zip(fr, per)]
    return np.stack([r[0] for r in res]), np.stack([r[1].data for r in res])


def test_the_per_frame_call_meets_the_oracle_with_a_map():
    from oracle import atrous_numpy as O
    from test_gpu_parity import DENOISE_TOL
    W = _W()
    frame, nmap = oracle_case()
    for fam in FAMILIES:
        for soft in (True, False):
            ref = O.denoise(frame.copy(), ORACLE_WEIGHTS, fam.lower(), noise=nmap, soft_threshold=soft)
            got = W.denoise(frame, list(ORACLE_WEIGHTS), getattr(W, fam), nmap, soft_threshold=soft)
            err = float(np.abs(got - ref).max())
            print(f"per-frame denoise with a map vs oracle, {fam} soft={soft}: {err:.3e}")
            assert err <= DENOISE_TOL * float(np.abs(frame).max()), (fam, soft, err)


DENOISE_STACKS = [("f32", SHAPE_ODD, N_ODD, np.float32), ("f32", SHAPE_ROW, N_ROW, np.float32),
                  ("f32", SHAPE_BLOCKS, N_BLOCKS, np.float32), ("f64", SHAPE_ODD, N_ODD, np.float64),
                  ("f64", SHAPE_F64, N_F64, np.float64), ("f64", SHAPE_BLOCKS, N_BLOCKS, np.float64)]


@pytest.mark.parametrize("kind", ["shared", "per_frame", "mixed"])
@pytest.mark.parametrize("engine,shape,n,dtype", DENOISE_STACKS, ids=[f"{e}-{n}x{s[0]}x{s[1]}" for e, s, n, _ in DENOISE_STACKS])
def test_denoise_stack_with_maps_is_the_per_frame_call(no_fallback, engine, shape, n, dtype, kind):
    W = _W()
    fr = frames_of(shape, n, dtype)
    arg, per = noise_arg(kind, shape, n)
    kept = [None if p is None or np.ndim(p) == 0 else p.copy() for p in per]
    for fam in FAMILIES:
        for level, weights in WEIGHTS.items():
            for soft in (True, False):
                got = W.denoise_stack(fr, list(weights), getattr(W, fam), noise=arg, soft_threshold=soft)
                assert got.dtype == dtype and got.shape == fr.shape
                exp = _per_frame_denoise(fr, weights, getattr(W, fam), per, soft_threshold=soft)
                _same_bits(got, exp, f"denoise_stack {engine} {shape} {kind} {fam} L{level} soft={soft}")
    for p, k in zip(per, kept):                                 # the caller's maps are not modified
        assert k is None or np.array_equal(p, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_anscombe_with_a_shared_map(no_fallback, dtype):
    W = _W()
    fr = frames_of(SHAPE_ODD, N_ODD, dtype, positive=True)
    m = noise_map(SHAPE_ODD)
    got = W.denoise_stack(fr, [5, 3], noise=m, anscombe=True)
    _same_bits(got, _per_frame_denoise(fr, [5, 3], W.B3spline, [m] * N_ODD, anscombe=True), f"anscombe {dtype}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bilateral_with_per_frame_maps(no_fallback, dtype):
    W = _W()
    fr = frames_of(SHAPE_BLOCKS, 3, dtype, positive=True)
    arg, per = noise_arg("per_frame", SHAPE_BLOCKS, 3)
    got = W.denoise_stack(fr, [5, 3, 1], noise=arg, bilateral=1.5)
    _same_bits(got, _per_frame_denoise(fr, [5, 3, 1], W.B3spline, per, bilateral=1.5), f"bilateral {dtype}")


@pytest.mark.parametrize("dtype", [np.int16, ">f4"])
def test_recast_stacks_with_a_shared_map_run_the_float64_batch(no_fallback, dtype):
    W = _W()
    fr = frames_of(SHAPE_ODD, N_ODD, np.float32).astype(dtype) if dtype == ">f4" else frames_of(SHAPE_ODD, N_ODD, dtype)
    m = noise_map(SHAPE_ODD)
    got = W.denoise_stack(fr, [5, 3], noise=m)
    assert got.dtype == np.float64
    _same_bits(got, _per_frame_denoise(fr, [5, 3], W.B3spline, [m] * N_ODD), f"recast {dtype}")


def test_three_chunks_with_per_frame_maps(no_fallback, monkeypatch):
    """a budget of two frames per chunk WITH the noise plane: five frames run as 2 + 2 + 1, every chunk takes its own
    maps from the list"""
    from wavelets_amd import _lib as L
    W = _W()
    H, Wd = SHAPE_BLOCKS
    for dtype, item, pitch in ((np.float32, 4, (Wd + 3) // 4 * 4), (np.float64, 8, (Wd + 1) // 2 * 2)):
        budget = 2 * (L.batch_frame_bytes(H, Wd, 2, itemsize=item) + H * pitch * item) + 8
        monkeypatch.setattr(L, "BATCH_BYTES", budget)
        assert [c for _, c in L.batch_chunks(N_BLOCKS, H, Wd, 2, extra_planes=1, itemsize=item)] == [2, 2, 1]
        fr = frames_of(SHAPE_BLOCKS, N_BLOCKS, dtype)
        for kind in ("per_frame", "shared"):
            arg, per = noise_arg(kind, SHAPE_BLOCKS, N_BLOCKS)
            got = W.denoise_stack(fr, [5, 3], noise=arg)
            _same_bits(got, _per_frame_denoise(fr, [5, 3], W.B3spline, per), f"three chunks {dtype} {kind}")


def test_out_is_filled_in_place(no_fallback):
    W = _W()
    fr = frames_of(SHAPE_ODD, N_ODD)
    m = noise_map(SHAPE_ODD)
    out = np.full(fr.shape, np.nan, np.float32)
    assert W.denoise_stack(fr, [5, 3], noise=m, out=out) is out
    _same_bits(out, _per_frame_denoise(fr, [5, 3], W.B3spline, [m] * N_ODD), "denoise_stack out=")
    fw = frames_of(SHAPE_BLOCKS, 3)
    mw = noise_map(SHAPE_BLOCKS)
    outw = np.full(fw.shape, np.nan, np.float32)
    assert W.wow_stack(fw, noise=mw, denoise_coefficients=[5, 2], out=outw) is outw
    _same_bits(outw, _per_frame_wow(fw, W.B3spline, [mw] * 3, denoise_coefficients=[5, 2])[0], "wow_stack out=")


def test_a_frames_result_does_not_depend_on_its_neighbours(no_fallback):
    W = _W()
    perm = [3, 0, 4, 2, 1]
    for dtype in (np.float32, np.float64):
        fr = frames_of(SHAPE_BLOCKS, N_BLOCKS, dtype)
        arg, per = noise_arg("mixed", SHAPE_BLOCKS, N_BLOCKS)
        a = W.denoise_stack(fr, [5, 3], noise=arg)
        b = W.denoise_stack(fr[perm], [5, 3], noise=[per[i] for i in perm])
        _same_bits(b, a[perm], f"permuted {dtype}")


WOW_CASES = {
    "defaults": {},
    "denoise": dict(denoise_coefficients=[5, 2]),
    "no_whitening": dict(whitening=False, denoise_coefficients=[5, 2]),
    "gamma": dict(h=0.5, denoise_coefficients=[5, 2]),
    "bilateral": dict(bilateral=1, denoise_coefficients=[5, 2]),
}


@pytest.mark.parametrize("kind", ["shared", "mixed"])
@pytest.mark.parametrize("case", sorted(WOW_CASES))
def test_wow_stack_with_maps_is_the_per_frame_call(no_fallback, case, kind):
    W = _W()
    fr = frames_of(SHAPE_BLOCKS, 3, positive=True)
    arg, per = noise_arg(kind, SHAPE_BLOCKS, 3)
    kw = WOW_CASES[case]
    img, planes = W.wow_stack(fr, noise=arg, return_coefficients=True, **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()})
    eimg, eplanes = _per_frame_wow(fr, W.B3spline, per, **kw)
    _same_bits(img, eimg, f"wow_stack {case} {kind} images")
    _same_bits(planes, eplanes, f"wow_stack {case} {kind} planes")             # return_coefficients: the planes too
    if case == "denoise":
        only = W.wow_stack(fr, noise=arg, denoise_coefficients=[5, 2], soft_threshold=False)
        _same_bits(only, _per_frame_wow(fr, W.B3spline, per, denoise_coefficients=[5, 2], soft_threshold=False)[0],
                   f"wow_stack hard {kind}")


def test_float64_wow_stack_with_a_map_is_the_loops_result():
    W = _W()
    fr = frames_of(SHAPE_BLOCKS, 2, np.float64, positive=True)
    m = noise_map(SHAPE_BLOCKS)
    got = W.wow_stack(fr, noise=m, denoise_coefficients=[5, 2])
    _same_bits(got, _per_frame_wow(fr, W.B3spline, [m, m], denoise_coefficients=[5, 2])[0], "float64 wow_stack")
