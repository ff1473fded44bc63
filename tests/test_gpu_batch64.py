"""The float64 batch (wt_batch64) behind transform_stack / denoise_stack: stacks the reference computes in float64 -
float64 frames and the integer / big-endian frames it recasts - run the batched route, every result meets the float64
numpy oracle per frame (bounds scaled by THAT frame's max|input|: 1e-12, the float64 engine's bounds of
tests/test_gpu_parity.py and tests/test_gpu_round3.py) and then equals np.stack of the per-frame API bit for bit.
Inputs and the reference-only premise of the hard-threshold comparisons: tests/test_batch64_cpu.py."""
import numpy as np
import pytest

from conftest import measured
from test_stack_edges_cpu import (SHAPES, FAMILIES, LEVELS, STACKS, DENOISE_WEIGHTS, noise_modes, per_frame_noise,
                                  REPS, big_stack, base_index)
from test_batch64_cpu import (ROUTE_TYPES, PLANES_TOL, DENOISE64_TOL, DTYPE_SHAPE, ANSCOMBE_SHAPES, hostile_stack64,
                              typed_stack)

pytestmark = pytest.mark.gpu

_shape_id = lambda s: f"{s[0]}x{s[1]}"


def _W():
    import wavelets_amd as W
    return W


def _O():
    from oracle import atrous_numpy as O
    return O


def _bits(a):
    """the float64 bits, every NaN as the one quiet NaN"""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)


def _same_bits(got, exp, what):
    assert got.dtype == np.float64 and exp.dtype == np.float64, (what, got.dtype, exp.dtype)
    g, e = _bits(got), _bits(exp)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at index {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _per_frame_transform(W, cls, fr, level):
    return np.stack([W.AtrousTransform(cls)(f, level).data for f in fr])


def _per_frame_denoise(W, cls, fr, weights, per, soft, anscombe=False):
    return np.stack([W.denoise(f, list(weights), cls, n_i, soft_threshold=soft, anscombe=anscombe) for f, n_i in zip(fr, per)])


def _check_transform(W, O, cls, fam, fr, level, got, what):
    assert got.shape == (len(fr), level + 1) + fr.shape[1:] and got.dtype == np.float64, what
    for i, f in enumerate(fr):
        f64 = f.astype(np.float64)
        measured(f"stack64 planes {what} frame {i}", got[i], O.atrous_standard(f64, level, fam.lower()),
                 PLANES_TOL * float(np.abs(f64).max()))
    _same_bits(got, _per_frame_transform(W, cls, fr, level), f"transform_stack vs per-frame {what}")


def _check_denoise(W, O, cls, fam, fr, weights, noise, soft, got, what, anscombe=False):
    per = per_frame_noise(noise, len(fr))
    assert got.shape == fr.shape and got.dtype == np.float64, what
    for i, (f, n_i) in enumerate(zip(fr, per)):
        f64 = f.astype(np.float64)
        ref = O.denoise(f64.copy(), list(weights), fam.lower(), n_i, soft_threshold=soft, anscombe=anscombe)
        measured(f"stack64 denoise {'soft' if soft else 'hard'} {what} frame {i}", got[i], ref,
                 DENOISE64_TOL * float(np.abs(f64).max()))
    _same_bits(got, _per_frame_denoise(W, cls, fr, weights, per, soft, anscombe), f"denoise_stack vs per-frame {what}")


@pytest.fixture
def no_fallback(monkeypatch):
    """the names the per-frame fallback of batch.py calls, patched to raise: what succeeds ran the batched route"""
    from wavelets_amd import batch as B

    def boom(*a, **k):
        raise AssertionError("the per-frame fallback ran")
    monkeypatch.setattr(B, "AtrousTransform", boom)
    monkeypatch.setattr(B, "denoise", boom)
    yield monkeypatch
    monkeypatch.undo()


@pytest.mark.parametrize("dtype", ROUTE_TYPES + [np.uint32, np.int64], ids=lambda d: np.dtype(d).str)
def test_float64_stacks_take_the_batched_route(dtype, no_fallback):
    """float64, int16, uint16, int32, uint32, int64, '>f4' and '>f8' stacks: transform_stack and denoise_stack succeed
    with the fallback disabled; the results meet the oracle and the per-frame API (int32 above 2**24, int64 up to
    2**53: exact only in float64)"""
    W, O = _W(), _O()
    fr = typed_stack(dtype)
    got_t = W.transform_stack(fr, 5)
    got_d = {(soft, noise): W.denoise_stack(fr, [5, 3], noise=noise, soft_threshold=soft)
             for soft in (True, False) for noise in (None, 0.8)}
    src = np.abs(fr).astype(fr.dtype)                           # (non-negative frames of the same element type)
    got_a = W.denoise_stack(src, [5, 3], anscombe=True)
    no_fallback.undo()
    for fam, cls in (("B3spline", W.B3spline),):
        _check_transform(W, O, cls, fam, fr, 5, got_t, f"{np.dtype(dtype).str} L5")
        for (soft, noise), got in got_d.items():
            _check_denoise(W, O, cls, fam, fr, [5, 3], noise, soft, got, f"{np.dtype(dtype).str} {noise}")
        _same_bits(got_a, np.stack([W.denoise(f, [5, 3], cls, anscombe=True) for f in src]),
                   f"anscombe denoise_stack vs per-frame {np.dtype(dtype).str}")


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_transform_stack64_against_the_oracle(shape, fam):
    W, O = _W(), _O()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    all9 = hostile_stack64(shape)
    for level in LEVELS:
        for n in STACKS:
            fr = all9[:n]
            assert B.batch64_eligible(fr, level, cls) == (shape[0] >= 2)      # one-row frames: the per-frame loop
            got = W.transform_stack(fr, level, cls)
            _check_transform(W, O, cls, fam, fr, level, got, f"{_shape_id(shape)} {fam} L{level} N{n}")


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_denoise_stack64_against_the_oracle(shape, fam):
    """noise None / scalar / one per frame, soft and hard thresholds, both weight lists ([4, 2, 1, 0, 0]: the threshold
    step between the fused passes); hard thresholds leave no sample out (tests/test_batch64_cpu.py: the premise)"""
    W, O = _W(), _O()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    all9 = hostile_stack64(shape)
    for weights in DENOISE_WEIGHTS:
        for mode, noise9 in noise_modes(len(all9)):
            for soft in (True, False):
                for n in STACKS:
                    fr = all9[:n]
                    noise = noise9[:n] if isinstance(noise9, list) else noise9
                    assert B.batch64_eligible(fr, len(weights), cls, None, per_frame_noise(noise, n)) == (shape[0] >= 2)
                    got = W.denoise_stack(fr, list(weights), cls, noise=noise, soft_threshold=soft)
                    _check_denoise(W, O, cls, fam, fr, weights, noise, soft, got,
                                   f"{_shape_id(shape)} {fam} {weights} {mode} N{n}")


@pytest.mark.parametrize("shape", ANSCOMBE_SHAPES, ids=_shape_id)
def test_denoise_stack64_anscombe(shape):
    W, O = _W(), _O()
    fr = np.abs(hostile_stack64(shape))
    for noise in (None, 0.8):
        got = W.denoise_stack(fr, [5, 3], noise=noise, anscombe=True)
        _check_denoise(W, O, W.B3spline, "B3spline", fr, [5, 3], noise, True, got, f"anscombe {_shape_id(shape)} {noise}",
                       anscombe=True)


def test_stack_in_chunks(monkeypatch):
    """a small budget splits the stack into >= 3 chunks (the last one shorter): same results"""
    W, O = _W(), _O()
    from wavelets_amd import _lib as L
    fr = hostile_stack64((64, 9))
    monkeypatch.setattr(L, "BATCH_BYTES", 3 * L.batch_frame_bytes(64, 9, 5, itemsize=8) + 1)
    assert len(L.batch_chunks(9, 64, 9, 5, itemsize=8)) == 3
    monkeypatch.setattr(L, "BATCH_BYTES", 4 * L.batch_frame_bytes(64, 9, 5, itemsize=8))
    chunks = L.batch_chunks(9, 64, 9, 5, itemsize=8)
    assert len(chunks) == 3 and chunks[-1][1] == 1
    _check_transform(W, O, W.B3spline, "B3spline", fr, 5, W.transform_stack(fr, 5), "chunks L5")
    per = [0.8 * (1 + i) for i in range(9)]
    per[4] = None
    for weights in DENOISE_WEIGHTS:
        got = W.denoise_stack(fr, list(weights), noise=per, soft_threshold=False)
        _check_denoise(W, O, W.B3spline, "B3spline", fr, weights, per, False, got, f"chunks {weights}")


def test_huge_stack_across_the_grid_limit():
    """65 540 frames of 8 x 8 (two chunks: the grid's z limit is 65 535 frames), every frame a representative times a
    power of two - exact in float64 - so that 64 oracle and per-frame calls vouch for every frame"""
    W, O = _W(), _O()
    n, shape, level = 65540, (8, 8), 2
    fr32, rep, scale = big_stack(n, shape)
    fr = fr32.astype(np.float64)
    got = W.transform_stack(fr, level)
    assert got.shape == (n, level + 1) + shape and got.dtype == np.float64
    base = got[[base_index(r) for r in range(REPS)]]
    _check_transform(W, O, W.B3spline, "B3spline", fr[[base_index(r) for r in range(REPS)]], level, base, "65540 x 8x8 base")
    _same_bits(got, base[rep] * scale.astype(np.float64)[:, None, None, None], "65540 frames vs their representatives")
    den = W.denoise_stack(fr, [5, 3], noise=0.5)
    bden = den[[base_index(r) for r in range(REPS)]]
    _same_bits(bden, _per_frame_denoise(W, W.B3spline, fr[[base_index(r) for r in range(REPS)]], [5, 3], [0.5] * REPS, True),
               "65540 denoise: representatives vs per-frame")


def test_zero_frame_between_loud_ones():
    """an all-zero frame (median 0: noise 0, no threshold) between loud frames stays zero"""
    W, O = _W(), _O()
    fr = hostile_stack64((33, 31), 3)
    fr[1] = 0.0
    for soft in (True, False):
        got = W.denoise_stack(fr, [5, 3], soft_threshold=soft)
        assert not got[1].any()
        _check_denoise(W, O, W.B3spline, "B3spline", fr, [5, 3], None, soft, got, f"zero frame soft={soft}")


def test_nan_frame_has_the_per_frame_outcome():
    """one frame holding a NaN, noise None: the batch gives what the per-frame float64 calls give (an error, or the
    same values)"""
    W = _W()
    fr = hostile_stack64((33, 31), 3)
    fr[1, 10, 7] = np.nan
    try:
        exp = np.stack([W.denoise(f, [5, 3]) for f in fr])
        exp_err = None
    except Exception as e:                          # noqa: BLE001 - the outcome is compared, whatever it is
        exp, exp_err = None, type(e)
    try:
        got = W.denoise_stack(fr, [5, 3])
        got_err = None
    except Exception as e:                          # noqa: BLE001
        got, got_err = None, type(e)
    assert got_err == exp_err, (got_err, exp_err)
    if exp is not None:
        _same_bits(got, exp, "NaN frame")


def test_out_arguments():
    """a C-contiguous float64 `out` receives the result; any other `out` the per-frame route accepts gets the same"""
    W = _W()
    fr = hostile_stack64((33, 31), 2)
    ref = W.transform_stack(fr, 3)
    out = np.empty((2, 4, 33, 31))
    assert W.transform_stack(fr, 3, out=out) is out
    _same_bits(out, ref, "out float64")
    out32 = np.empty((2, 4, 33, 31), np.float32)
    assert W.transform_stack(fr, 3, out=out32) is out32
    assert np.array_equal(out32, ref.astype(np.float32))
    big = np.empty((2, 4, 33, 62))[..., ::2]                  # a strided view
    assert W.transform_stack(fr, 3, out=big) is big
    _same_bits(np.ascontiguousarray(big), ref, "out strided")
    dref = W.denoise_stack(fr, [5, 3])
    dout = np.empty((2, 33, 31))
    assert W.denoise_stack(fr, [5, 3], out=dout) is dout
    _same_bits(dout, dref, "denoise out")


def test_batch64_median_is_wt64_abs_median():
    """the batched select gives the values wt64_abs_median gives, frames of an odd and an even pixel count, ties"""
    W = _W()
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    for shape in ((33, 31), (64, 9), (2, 3), (300, 517)):
        fr = hostile_stack64(shape)
        fr[2] = np.round(fr[2] / 1e5)                          # ties
        bp = L.BatchPlan64(ctx, len(fr), shape[0], shape[1], L.B3SPLINE, 2)
        try:
            bp.upload(L.PLANE_INPUT, fr)
            bp.decompose(len(fr), L.PLANE_INPUT, 2)
            med = bp.abs_median(len(fr), 0)
            w0 = np.array(bp.download(0, len(fr)))
        finally:
            bp.close()
        for i, f in enumerate(fr):
            p = L.Plan64(ctx, shape[0], shape[1], (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16), 2)
            try:
                p.upload(L.PLANE_INPUT, w0[i])
                m = p.abs_median(L.PLANE_INPUT)
            finally:
                p.close()
            assert med[i] == m == np.median(np.abs(w0[i])), (shape, i, med[i], m)
