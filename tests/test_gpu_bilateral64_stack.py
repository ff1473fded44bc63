"""The batched float64 bilateral transform (wt64_bilateral_march_batch_kernel behind transform_stack / denoise_stack
with bilateral= on the stacks the reference computes in float64): every result meets the float64 numpy oracle first -
per frame, under a bound scaled by THAT frame's max|input|, in stacks whose neighbouring frames are nine decades apart,
so that a read that lands in the next frame cannot hide - and the per-frame API second, bit for bit (NaNs compared as
bits).  For the whole module the per-frame fallback of batch.py is patched to raise: what succeeds ran the batched
march.  Inputs, bounds (1e-12 of max|frame| for the planes, the float64 engine's bilateral bound; for denoise 4 x the
per-frame API's own measured error: 3.9e-13, with anscombe=True 2.5e-10) and the reference-only premise of the
hard-threshold comparisons, which leave no sample out: tests/test_bilateral64_stack_cpu.py."""
import numpy as np
import pytest

from conftest import measured
from test_bilateral64_stack_cpu import (SHAPES, FAMILIES, STACKS, LEVEL, MODES, DEEP_SHAPE, DEEP_LEVELS, DENOISE_WEIGHTS,
                                        CHUNK_SHAPE, AMPS, BIL64_TRANSFORM_TOL, BIL64_DENOISE_TOL, BIL64_ANSCOMBE_TOL,
                                        bil64_stack, noise_modes, leak_stack, ref_transform, ref_denoise)
from test_batch64_cpu import ROUTE_TYPES, typed_stack
from test_stack_edges_cpu import per_frame_noise

pytestmark = pytest.mark.gpu

_shape_id = lambda s: f"{s[0]}x{s[1]}"


def _W():
    import wavelets_amd as W
    return W


@pytest.fixture(autouse=True)
def no_fallback(monkeypatch):
    """the names the per-frame fallback of batch.py calls, patched to raise for every test of this module"""
    from wavelets_amd import batch as B

    def boom(*a, **k):
        raise AssertionError("the per-frame fallback ran")
    monkeypatch.setattr(B, "AtrousTransform", boom)
    monkeypatch.setattr(B, "denoise", boom)


def _bits(a):
    """the float64 bits as they are (NaN payloads included)"""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(got, exp, what):
    assert got.dtype == np.float64 and exp.dtype == np.float64, (what, got.dtype, exp.dtype)
    g, e = _bits(got), _bits(exp)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at index {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _mode_args(mode):
    bil, scaling = MODES[mode]
    return (list(bil) if isinstance(bil, list) else bil), scaling


def _per_frame_transform(W, cls, fr, level, mode="one"):
    return np.stack([W.AtrousTransform(cls, *_mode_args(mode))(f, level).data for f in fr])


def _per_frame_denoise(W, cls, fr, weights, per, soft, anscombe=False):
    return np.stack([W.denoise(f, list(weights), cls, n_i, 1, soft, anscombe) for f, n_i in zip(fr, per)])


def _check_transform(W, cls, fam, fr, level, mode, got, what):
    assert got.shape == (len(fr), level + 1) + fr.shape[1:] and got.dtype == np.float64, what
    for i, f in enumerate(fr):
        f64 = f.astype(np.float64)
        measured(f"bilateral64 stack planes {what} frame {i}", got[i], ref_transform(f64, level, fam, *_mode_args(mode)),
                 BIL64_TRANSFORM_TOL * float(np.abs(f64).max()))
    _same_bits(got, _per_frame_transform(W, cls, fr, level, mode), f"transform_stack vs per-frame {what}")


def _check_denoise(W, cls, fam, fr, weights, noise, soft, got, what, anscombe=False):
    tol = BIL64_ANSCOMBE_TOL if anscombe else BIL64_DENOISE_TOL
    per = per_frame_noise(noise, len(fr))
    assert got.shape == fr.shape and got.dtype == np.float64, what
    for i, (f, n_i) in enumerate(zip(fr, per)):
        f64 = f.astype(np.float64)
        measured(f"bilateral64 stack denoise {'soft' if soft else 'hard'} {what} frame {i}", got[i],
                 ref_denoise(f64, weights, fam, n_i, soft, anscombe), tol * float(np.abs(f64).max()))
    _same_bits(got, _per_frame_denoise(W, cls, fr, weights, per, soft, anscombe), f"denoise_stack vs per-frame {what}")


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_transform_stack_bilateral64(shape, fam):
    W = _W()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    all9 = bil64_stack(shape)
    for mode in MODES:
        bil, scaling = _mode_args(mode)
        for n in STACKS:
            fr = all9[:n]
            assert B.bilateral64_eligible(fr, LEVEL, cls, bil)
            got = W.transform_stack(fr, LEVEL, cls, bilateral=bil, bilateral_scaling=scaling)
            _check_transform(W, cls, fam, fr, LEVEL, mode, got, f"{_shape_id(shape)} {fam} {mode} N{n}")


@pytest.mark.parametrize("fam", FAMILIES)
def test_levels_whose_dilation_exceeds_the_frame(fam):
    """levels 1, 4 and the family's sigma_e(bilateral=...) table (10 / 11 scales) on 40 x 24 frames"""
    W = _W()
    cls = getattr(W, fam)
    fr = bil64_stack(DEEP_SHAPE, 3)
    for level in DEEP_LEVELS[fam]:
        got = W.transform_stack(fr, level, cls, bilateral=1)
        _check_transform(W, cls, fam, fr, level, "one", got, f"{_shape_id(DEEP_SHAPE)} {fam} L{level}")
    got = W.denoise_stack(fr, [3] * DEEP_LEVELS[fam][-1], cls, bilateral=1)
    _same_bits(got, _per_frame_denoise(W, cls, fr, [3] * DEEP_LEVELS[fam][-1], [None] * 3, True), f"denoise_stack at the table's length {fam}")


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_denoise_stack_bilateral64(shape, fam):
    """noise None / scalar / one per frame, soft and hard thresholds, both weight lists; hard thresholds leave no
    sample out (tests/test_bilateral64_stack_cpu.py: the premise)"""
    W = _W()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    all9 = bil64_stack(shape)
    for weights in DENOISE_WEIGHTS:
        for mode, noise9 in noise_modes(len(all9)):
            for soft in (True, False):
                for n in (STACKS if (mode == "mad" and soft) else STACKS[-1:]):
                    fr = all9[:n]
                    noise = noise9[:n] if isinstance(noise9, list) else noise9
                    assert B.bilateral64_eligible(fr, len(weights), cls, 1, per_frame_noise(noise, n))
                    got = W.denoise_stack(fr, list(weights), cls, noise=noise, soft_threshold=soft, bilateral=1)
                    _check_denoise(W, cls, fam, fr, weights, noise, soft, got,
                                   f"{_shape_id(shape)} {fam} {weights} {mode} N{n}")


@pytest.mark.parametrize("dtype", ROUTE_TYPES, ids=lambda d: np.dtype(d).str)
def test_element_types_the_reference_recasts(dtype):
    """float64, int16, uint16, int32, '>f4' and '>f8' stacks (int32 above 2**24: exact only in float64)"""
    W = _W()
    from wavelets_amd import batch as B
    fr = typed_stack(dtype)
    name = np.dtype(dtype).str
    assert B.bilateral64_eligible(fr, 4, bilateral=1)
    _check_transform(W, W.B3spline, "B3spline", fr, 4, "one", W.transform_stack(fr, 4, bilateral=1), f"{name} L4")
    for soft in (True, False):
        for noise in (None, 0.8):
            got = W.denoise_stack(fr, [5, 3], noise=noise, soft_threshold=soft, bilateral=1)
            _check_denoise(W, W.B3spline, "B3spline", fr, [5, 3], noise, soft, got, f"{name} {noise}")
    src = np.abs(fr).astype(fr.dtype)                           # (non-negative frames of the same element type)
    got = W.denoise_stack(src, [5, 3], anscombe=True, bilateral=1)
    _check_denoise(W, W.B3spline, "B3spline", src, [5, 3], None, True, got, f"anscombe {name}", anscombe=True)


def test_stack_in_three_chunks(monkeypatch):
    """a budget of four frames per chunk: nine frames run as chunks of 4, 4 and 1; BatchPlan64.decompose_bilateral is
    called once per chunk and no per-frame entry point at all"""
    W = _W()
    from wavelets_amd import _lib as L
    H, Wd = CHUNK_SHAPE
    fr = bil64_stack(CHUNK_SHAPE)
    per = [0.8 * AMPS[i % 2] * (1 + i) for i in range(9)]
    per[4] = None
    one_t = W.transform_stack(fr, LEVEL, bilateral=1)
    calls = []
    real = L.BatchPlan64.decompose_bilateral

    def counted(self, nf, *a, **k):
        calls.append(nf)
        return real(self, nf, *a, **k)

    def boom(*a, **k):
        raise AssertionError("a per-frame entry point ran")
    with monkeypatch.context() as m:
        m.setattr(L.BatchPlan64, "decompose_bilateral", counted)
        m.setattr(L.Plan64, "decompose_bilateral", boom)
        m.setattr(L.Plan64, "bilateral_conv", boom)
        m.setattr(L, "BATCH_BYTES", 4 * L.batch_frame_bytes(H, Wd, LEVEL, itemsize=8) + 8)
        assert [c for _, c in L.batch_chunks(9, H, Wd, LEVEL, itemsize=8)] == [4, 4, 1]
        got_t = W.transform_stack(fr, LEVEL, bilateral=1)
        assert calls == [4, 4, 1]
        got_d = {}
        for weights in DENOISE_WEIGHTS:
            m.setattr(L, "BATCH_BYTES", 4 * L.batch_frame_bytes(H, Wd, len(weights), itemsize=8) + 8)
            del calls[:]
            got_d[tuple(weights)] = W.denoise_stack(fr, list(weights), noise=per, soft_threshold=False, bilateral=1)
            assert calls == [4, 4, 1]
    _same_bits(got_t, one_t, "transform_stack in three chunks vs one")
    _check_transform(W, W.B3spline, "B3spline", fr, LEVEL, "one", got_t, "chunks")
    for weights in DENOISE_WEIGHTS:
        _check_denoise(W, W.B3spline, "B3spline", fr, weights, per, False, got_d[tuple(weights)], f"chunks {weights}")


def test_no_frame_leaks_into_its_neighbours():
    """a constant frame (local variance exactly zero) and an all-NaN frame between finite frames: the finite frames
    come out finite and are what they are without the NaN frame; every frame has the per-frame bits"""
    W = _W()
    fr, bad = leak_stack()
    keep = [i for i in range(len(fr)) if i != bad]
    for fam in FAMILIES:
        cls = getattr(W, fam)
        got = W.transform_stack(fr, LEVEL, cls, bilateral=1)
        clean = W.transform_stack(fr[keep], LEVEL, cls, bilateral=1)
        den = W.denoise_stack(fr, [5, 3], cls, noise=0.7, bilateral=1)
        den_clean = W.denoise_stack(fr[keep], [5, 3], cls, noise=0.7, bilateral=1)
        for i in (0, 2, 4):
            assert np.isfinite(got[i]).all() and np.isfinite(den[i]).all(), (fam, i)
        assert np.isnan(got[bad]).all()
        _same_bits(got[keep], clean, f"transform_stack beside a NaN frame {fam}")
        _same_bits(den[keep], den_clean, f"denoise_stack beside a NaN frame {fam}")
        _same_bits(got, _per_frame_transform(W, cls, fr, LEVEL), f"transform_stack vs per-frame, NaN and constant frames {fam}")
        _same_bits(den, _per_frame_denoise(W, cls, fr, [5, 3], [0.7] * len(fr), True), f"denoise_stack vs per-frame, NaN and constant frames {fam}")
        for i in (0, 2, 4):
            measured(f"bilateral64 stack planes beside a NaN frame {fam} frame {i}", got[i], ref_transform(fr[i], LEVEL, fam),
                     BIL64_TRANSFORM_TOL * float(np.abs(fr[i]).max()))


def test_out_arguments():
    """a C-contiguous float64 `out` receives the result; a non-contiguous one gets the same values"""
    W = _W()
    fr = bil64_stack((33, 31), 2)
    ref = W.transform_stack(fr, LEVEL, bilateral=1)
    out = np.empty((2, LEVEL + 1, 33, 31))
    assert W.transform_stack(fr, LEVEL, out=out, bilateral=1) is out
    _same_bits(out, ref, "out float64")
    dref = W.denoise_stack(fr, [5, 3], bilateral=1)
    dout = np.empty((2, 33, 31))
    assert W.denoise_stack(fr, [5, 3], out=dout, bilateral=1) is dout
    _same_bits(dout, dref, "denoise out")
    _check_denoise(W, W.B3spline, "B3spline", fr, [5, 3], None, True, dout, "out")
    strided = np.empty((2, 33, 62))[..., ::2]
    assert not strided.flags.c_contiguous and W.denoise_stack(fr, [5, 3], out=strided, bilateral=1) is strided
    _same_bits(np.ascontiguousarray(strided), dref, "denoise out strided")
    big = np.empty((2, LEVEL + 1, 33, 62))[..., ::2]
    assert W.transform_stack(fr, LEVEL, out=big, bilateral=1) is big
    _same_bits(np.ascontiguousarray(big), ref, "out strided")


def test_the_option_sends_the_stack_to_the_loop(monkeypatch):
    """with "stencil64" off the per-frame call runs the generic three-kernel form: the stack takes the loop (here
    restored for the occasion) and still equals the per-frame results"""
    W = _W()
    from wavelets_amd import _lib as L
    from wavelets_amd import batch as B
    fr = bil64_stack((33, 31), 2)
    monkeypatch.setattr(B, "AtrousTransform", W.AtrousTransform)
    try:
        L.set_option("stencil64", 0)
        assert not B.bilateral64_eligible(fr, LEVEL, bilateral=1)
        got = W.transform_stack(fr, LEVEL, bilateral=1)
        _same_bits(got, _per_frame_transform(W, W.B3spline, fr, LEVEL), "stencil64 off")
    finally:
        L.set_option("stencil64", 1)
