"""The batched bilateral transform (wt_bilateral2_batch_kernel behind transform_stack / denoise_stack / wow_stack with
bilateral=): every result meets the numpy oracle in float64 first - per frame, under a bound scaled by THAT frame's
max|input| (max|reference| for wow), in stacks whose neighbouring frames are nine decades apart, so that a read that
lands in the next frame cannot hide - and the per-frame API second, bit for bit.  Inputs, bounds (test_gpu_parity's
BIL_TRANSFORM_TOL and WOW_BIL_TOL by value; BIL_DENOISE_TOL, measured on the per-frame API because DENOISE_TOL does
not hold for it) and their reference-only premises:
tests/test_bilateral_stack_cpu.py.  A stack whose reference is not finite (reference_is_finite, decided there from
the oracle alone) is held to the bitwise comparison only, non-finite positions included."""
import numpy as np
import pytest

from conftest import measured, measured_tol
from test_bilateral_stack_cpu import (SHAPES, FLAT_SHAPES, FAMILIES, STACKS, LEVEL, MODES, DENOISE_WEIGHTS, WOW_KW,
                                      BIL_TRANSFORM_TOL, WOW_BIL_TOL, BIL_DENOISE_TOL, bil_stack, flat_stack, noise_modes,
                                      ref_transform, ref_denoise, ref_wow, reference_is_finite)
from test_stack_edges_cpu import hard_allow, per_frame_noise, fresh

pytestmark = pytest.mark.gpu

_shape_id = lambda s: f"{s[0]}x{s[1]}"
KINDS = [("noise", s) for s in SHAPES] + [("flat", s) for s in FLAT_SHAPES]
_kind_id = lambda k: f"{k[0]}-{_shape_id(k[1])}"


def _W():
    import wavelets_amd as W
    return W


def _stack(kind, shape, n=None):
    if kind == "flat":
        return flat_stack(shape) if n is None else flat_stack(shape, n)
    return bil_stack(shape) if n is None else bil_stack(shape, n)


def _nanbits(a):
    """the float32 bits, every NaN as the one quiet NaN"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), a).view(np.uint32)


def _same_bits(got, exp, what):
    g, e = _nanbits(got), _nanbits(exp)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at index {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _mode_args(mode):
    bil, scaling = MODES[mode]
    return (list(bil) if isinstance(bil, list) else bil), scaling


@pytest.mark.parametrize("kind", KINDS, ids=_kind_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_transform_stack_bilateral(kind, fam):
    W = _W()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    name, shape = kind
    all_fr = _stack(name, shape)
    finite = reference_is_finite(name, shape, fam)
    for mode in MODES:
        refs = [ref_transform(f.astype(np.float64), fam, mode) for f in all_fr] if finite else None
        for n in [k for k in STACKS if k <= len(all_fr)]:
            fr = all_fr[:n]
            bil, scaling = _mode_args(mode)
            assert B.bilateral_eligible(fr, LEVEL, cls, bil)
            got = W.transform_stack(fr, LEVEL, cls, bilateral=bil, bilateral_scaling=scaling)
            assert got.shape == (n, LEVEL + 1) + shape and got.dtype == np.float32
            if finite:
                for i in range(n):
                    measured(f"bilateral stack planes {_kind_id(kind)} {fam} {mode} N{n} frame {i}", got[i], refs[i],
                             BIL_TRANSFORM_TOL * float(np.abs(fr[i]).max()))
            exp = np.stack([W.AtrousTransform(cls, _mode_args(mode)[0], scaling)(f, LEVEL).data for f in fr])
            _same_bits(got, exp, f"transform_stack vs per-frame {_kind_id(kind)} {fam} {mode} N{n}")


@pytest.mark.parametrize("kind", KINDS, ids=_kind_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_denoise_stack_bilateral(kind, fam):
    """soft threshold: every sample within BIL_DENOISE_TOL * max|frame| (DENOISE_TOL does not hold for the per-frame
    bilateral denoise on these inputs: measured 6.99e-7, bound 4 x that, test_bilateral_stack_cpu); hard threshold: all but hard_allow(shape) samples
    of a frame (none for frames under 1000 samples; the reference itself needs none, test_bilateral_stack_cpu)"""
    W = _W()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    name, shape = kind
    all_fr = _stack(name, shape)
    finite = reference_is_finite(name, shape, fam)
    for mode, noise_all in noise_modes(len(all_fr)):
        for soft in (True, False):
            refs = [ref_denoise(f.astype(np.float64), fam, n_i, soft)
                    for f, n_i in zip(all_fr, per_frame_noise(noise_all, len(all_fr)))] if finite else None
            for n in [k for k in STACKS if k <= len(all_fr)]:
                fr = all_fr[:n]
                noise = noise_all[:n] if isinstance(noise_all, list) else noise_all
                per = per_frame_noise(noise, n)
                assert B.bilateral_eligible(fr, len(DENOISE_WEIGHTS), cls, 1, per)
                got = W.denoise_stack(fr, list(DENOISE_WEIGHTS), cls, noise=noise, soft_threshold=soft, bilateral=1)
                assert got.shape == (n,) + shape and got.dtype == np.float32
                if finite:
                    for i in range(n):
                        tol = BIL_DENOISE_TOL * float(np.abs(fr[i]).max())
                        what = f"bilateral stack denoise {'soft' if soft else 'hard'} {_kind_id(kind)} {fam} {mode} N{n} frame {i}"
                        if soft:
                            measured(what, got[i], refs[i], tol)
                        else:
                            measured_tol(what, got[i], refs[i], atol=tol, allow=hard_allow(shape))
                exp = np.stack([W.denoise(f, list(DENOISE_WEIGHTS), cls, n_i, 1, soft_threshold=soft)
                                for f, n_i in zip(fr, per)])
                _same_bits(got, exp, f"denoise_stack vs per-frame {_kind_id(kind)} {fam} {mode} soft={soft} N{n}")


@pytest.mark.parametrize("kind", KINDS, ids=_kind_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_wow_stack_bilateral(kind, fam):
    """the flagship flow wow(bilateral=1, denoise_coefficients=[5, 2]), default scales; frames too small for one scale:
    wow_stack raises what wow() raises"""
    W = _W()
    cls = getattr(W, fam)
    name, shape = kind
    finite = reference_is_finite(name, shape, fam)
    fr = _stack(name, shape, 3)
    for mode, noise in noise_modes(3):
        per = per_frame_noise(noise, 3)
        what = f"{_kind_id(kind)} {fam} {mode}"
        try:
            res = [W.wow(f, cls, noise=n_i, **fresh(WOW_KW)) for f, n_i in zip(fr, per)]
        except Exception as e:              # noqa: BLE001 - whatever wow() raises is the contract here
            with pytest.raises(type(e)):
                W.wow_stack(fr, cls, noise=noise, return_coefficients=True, **fresh(WOW_KW))
            continue
        img, planes = W.wow_stack(fr, cls, noise=noise, return_coefficients=True, **fresh(WOW_KW))
        if finite:
            for i, (f, n_i) in enumerate(zip(fr, per)):
                ref = ref_wow(f.astype(np.float64), fam, n_i)
                assert not isinstance(ref, type), (what, ref)
                ref_img, ref_c = ref
                assert planes[i].shape == ref_c.shape and img[i].shape == ref_img.shape, what
                measured_tol(f"bilateral wow_stack planes {what} frame {i}", planes[i], ref_c,
                             atol=WOW_BIL_TOL * float(np.abs(ref_c).max()), rtol=WOW_BIL_TOL)
                measured_tol(f"bilateral wow_stack image {what} frame {i}", img[i], ref_img,
                             atol=WOW_BIL_TOL * float(np.abs(ref_img).max()), rtol=WOW_BIL_TOL)
        _same_bits(img, np.stack([r[0] for r in res]), f"wow_stack image vs per-frame {what}")
        _same_bits(planes, np.stack([r[1].data for r in res]), f"wow_stack planes vs per-frame {what}")
        _same_bits(W.wow_stack(fr, cls, noise=noise, **fresh(WOW_KW)), img, f"wow_stack without planes {what}")


@pytest.mark.parametrize("fam", FAMILIES)
def test_wow_stack_bilateral_keywords(fam):
    """bilateral as True and as a list with bilateral_scaling, hard threshold, the gamma blend, explicit n_scales"""
    W = _W()
    cls = getattr(W, fam)
    fr = bil_stack((96, 128), 3)
    for kw in (dict(bilateral=True), dict(bilateral=[2., .5], bilateral_scaling=True, denoise_coefficients=[5, 2]),
               dict(bilateral=1, denoise_coefficients=[5, 2], soft_threshold=False, n_scales=3),
               dict(bilateral=1, h=.5, gamma=2, preserve_variance=True), dict(bilateral=1, whitening=False, weights=[2, 1])):
        res = [W.wow(f, cls, **fresh(kw)) for f in fr]
        img, planes = W.wow_stack(fr, cls, return_coefficients=True, **fresh(kw))
        _same_bits(img, np.stack([r[0] for r in res]), f"wow_stack image vs per-frame {fam} {kw}")
        _same_bits(planes, np.stack([r[1].data for r in res]), f"wow_stack planes vs per-frame {fam} {kw}")


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_stack_that_spans_two_chunks(fam, monkeypatch):
    """a budget of four frames per chunk (through batch_chunks, as WATROO_HIP_BATCH_BYTES sets it): nine frames run as
    chunks of 4, 4 and 1 and give the bits of the one-chunk run"""
    W = _W()
    from wavelets_amd import _lib as L
    cls = getattr(W, fam)
    shape = (37, 50)
    fr = bil_stack(shape)
    one = (W.transform_stack(fr, LEVEL, cls, bilateral=1), W.denoise_stack(fr, [5, 3], cls, bilateral=1),
           W.wow_stack(fr, cls, **fresh(WOW_KW)))
    budget = 4 * L.batch_frame_bytes(shape[0], shape[1], LEVEL) + 8
    assert [c for _, c in L.batch_chunks(9, shape[0], shape[1], LEVEL, budget=budget)] == [4, 4, 1]
    monkeypatch.setattr(L, "BATCH_BYTES", budget)
    assert len(L.batch_chunks(9, shape[0], shape[1], LEVEL)) == 3
    two = (W.transform_stack(fr, LEVEL, cls, bilateral=1), W.denoise_stack(fr, [5, 3], cls, bilateral=1),
           W.wow_stack(fr, cls, **fresh(WOW_KW)))
    for a, b, what in zip(one, two, ("transform_stack", "denoise_stack", "wow_stack")):
        _same_bits(b, a, f"{what} in three chunks vs one {fam}")


@pytest.mark.parametrize("fam", FAMILIES)
def test_paired_and_generic_loads_give_identical_bits(fam):
    W = _W()
    from wavelets_amd import _lib as L
    cls = getattr(W, fam)
    try:
        for shape in [(33, 31), (17, 4), (37, 50), (64, 9), (1, 2)]:
            fr = bil_stack(shape)
            L.set_option("bilateral_paired", 1)
            paired = W.transform_stack(fr, LEVEL, cls, bilateral=1)
            L.set_option("bilateral_paired", 0)
            generic = W.transform_stack(fr, LEVEL, cls, bilateral=1)
            per = np.stack([W.AtrousTransform(cls, 1)(f, LEVEL).data for f in fr])
            _same_bits(generic, paired, f"bilateral_paired 0 vs 1 {_shape_id(shape)} {fam}")
            _same_bits(generic, per, f"bilateral_paired 0: stack vs per-frame {_shape_id(shape)} {fam}")
    finally:
        L.set_option("bilateral_paired", 1)


def test_the_batched_path_ran(monkeypatch):
    """with the per-frame entry points of the fallback loop patched to raise, the three stack calls with bilateral=1
    still return the per-frame results: they came out of the batched march"""
    W = _W()
    from wavelets_amd import batch as B
    fr = bil_stack((37, 50), 3)
    exp_t = np.stack([W.AtrousTransform(W.B3spline, 1)(f, LEVEL).data for f in fr])
    exp_d = np.stack([W.denoise(f, [5, 3], W.B3spline, None, 1) for f in fr])
    exp_w = np.stack([W.wow(f, **fresh(WOW_KW))[0] for f in fr])

    def boom(*a, **k):
        raise AssertionError("the per-frame loop ran")
    monkeypatch.setattr(B, "wow", boom)
    monkeypatch.setattr(B, "denoise", boom)
    monkeypatch.setattr(B, "AtrousTransform", boom)
    _same_bits(W.transform_stack(fr, LEVEL, bilateral=1), exp_t, "transform_stack(bilateral=1)")
    _same_bits(W.denoise_stack(fr, [5, 3], bilateral=1), exp_d, "denoise_stack(bilateral=1)")
    _same_bits(W.wow_stack(fr, **fresh(WOW_KW)), exp_w, "wow_stack(bilateral=1)")
