"""The batched engines (transform_stack / denoise_stack: wt_fused_batch_kernel; wow_stack: the batched stencil and
reduction kernels) where a wrong address lands in a neighbouring frame instead of faulting: frames smaller than the
filters' reach packed back to back, every row-pitch remainder, stacks of thousands of frames and across the grid
limit.  Every result meets the numpy oracle first - per frame, under a bound scaled by THAT frame's max|input|,
with neighbours nine decades louder - and the per-frame API second (bit for bit).  Inputs, shape list and the
reference-only premises of the bounds: tests/test_stack_edges_cpu.py.  Bounds: conftest's SMALL_PLANES / SMALL_RECON,
test_gpu_parity's DENOISE_TOL and the wow modules' WOW_TOL, none of them set on these kernels."""
import numpy as np
import pytest

from conftest import measured, measured_tol, SMALL_PLANES, SMALL_RECON
from test_stack_edges_cpu import (SHAPES, FAMILIES, LEVELS, STACKS, DENOISE_WEIGHTS, DENOISE_TOL, REPS, BIG_STACKS,
                                  WOW_TOL, H1_COEFFICIENTS, H1_SHAPES, WOW_CASE_SHAPES, hostile_stack, noise_modes,
                                  wow_noise_modes, h1_keywords, fresh, per_frame_noise, hard_allow, representatives,
                                  big_stack, base_index)
from test_gpu_wow_stack import CASES as WOW_CASES

pytestmark = pytest.mark.gpu

_shape_id = lambda s: f"{s[0]}x{s[1]}"


def _W():
    import wavelets_amd as W
    return W


def _O():
    from oracle import atrous_numpy as O
    return O


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _nanbits(a):
    """the float32 bits, every NaN as the one quiet NaN (tests/test_gpu_wow_stack.py: _bits)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), a).view(np.uint32)


def _same_bits(got, exp, what):
    g, e = _nanbits(got), _nanbits(exp)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at index {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


# ---------------------------------------------------------------- A: tiny and ragged frames against the oracle

@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_transform_stack_of_tiny_frames_against_the_oracle(shape, fam):
    W, O = _W(), _O()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    all9 = hostile_stack(shape)
    for level in LEVELS:
        refs = [O.atrous_standard(f, level, fam.lower()) for f in all9]
        for n in STACKS:
            fr = all9[:n]
            assert B.batch_eligible(fr, level, cls)                     # the batched kernels, not the per-frame loop
            got = W.transform_stack(fr, level, cls)
            assert got.shape == (n, level + 1) + shape and got.dtype == np.float32
            for i in range(n):
                amax = float(np.abs(fr[i]).max())
                what = f"{_shape_id(shape)} {fam} L{level} N{n} frame {i}"
                measured(f"stack planes {what}", got[i], refs[i], SMALL_PLANES * amax)
                measured(f"stack recon {what}", got[i].sum(axis=0), fr[i], SMALL_RECON * amax)
            exp = np.stack([W.AtrousTransform(cls)(f, level).data for f in fr])
            _same_bits(got, exp, f"transform_stack vs per-frame {_shape_id(shape)} {fam} L{level} N{n}")


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_denoise_stack_of_tiny_frames_against_the_oracle(shape, fam):
    """soft threshold: every sample within DENOISE_TOL * max|frame|; hard threshold: all but hard_allow(shape) samples
    of a frame (none for frames under 1000 samples; the reference itself flips none, test_stack_edges_cpu)"""
    W, O = _W(), _O()
    from wavelets_amd import batch as B
    cls = getattr(W, fam)
    all9 = hostile_stack(shape)
    for weights in DENOISE_WEIGHTS:
        for mode, noise9 in noise_modes(len(all9)):
            for soft in (True, False):
                refs = [O.denoise(f.copy(), list(weights), fam.lower(), n_i, soft_threshold=soft)
                        for f, n_i in zip(all9, per_frame_noise(noise9, len(all9)))]
                for n in STACKS:
                    fr = all9[:n]
                    noise = noise9[:n] if isinstance(noise9, list) else noise9
                    per = per_frame_noise(noise, n)
                    assert B.batch_eligible(fr, len(weights), cls, None, per)
                    got = W.denoise_stack(fr, list(weights), cls, noise=noise, soft_threshold=soft)
                    assert got.shape == (n,) + shape and got.dtype == np.float32
                    for i in range(n):
                        tol = DENOISE_TOL * float(np.abs(fr[i]).max())
                        what = (f"stack denoise {'soft' if soft else 'hard'} {_shape_id(shape)} {fam} {weights} {mode} "
                                f"N{n} frame {i}")
                        if soft:
                            measured(what, got[i], refs[i], tol)
                        else:
                            measured_tol(what, got[i], refs[i], atol=tol, allow=hard_allow(shape))
                    exp = np.stack([W.denoise(f, list(weights), cls, n_i, soft_threshold=soft) for f, n_i in zip(fr, per)])
                    _same_bits(got, exp, f"denoise_stack vs per-frame {_shape_id(shape)} {fam} {weights} {mode} N{n}")


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_batch_mad_noise_is_the_median_of_plane_0(shape, fam):
    """noise=None: the noise level the batch uses for frame f is np.median(|w0[f]|) / 0.6745 / sigma_e[0] exactly -
    frames of 1, 2, an odd and an even number of samples - and denoise_stack(noise=None) is denoise_stack with
    these levels passed in"""
    W = _W()
    from wavelets_amd import _lib as L
    from wavelets_amd.wavelets import _noise_from_median
    cls = getattr(W, fam)
    sigma_e = cls(2).sigma_e()
    fr = hostile_stack(shape)
    n = len(fr)
    bp = L.BatchPlan(L.default_context(), n, shape[0], shape[1], getattr(L, fam.upper()), 2)
    try:
        bp.upload(L.PLANE_INPUT, fr)
        bp.decompose(n, L.PLANE_INPUT, 2)
        med = bp.abs_median(n, 0)
        w0 = np.array(bp.download(0, n))
    finally:
        bp.close()
    _same_bits(w0, W.transform_stack(fr, 2, cls)[:, 0], "plane 0 of the batch")
    noises = []
    for f in range(n):
        exp = np.median(np.abs(w0[f]))
        assert exp.dtype == np.float32 and _bits(med[f]) == _bits(exp), (shape, fam, f, med[f], exp)
        noises.append(_noise_from_median(med[f], sigma_e))
        assert noises[f] == np.median(np.abs(w0[f])) / 0.6745 / sigma_e[0], (shape, fam, f)
    for soft in (True, False):
        _same_bits(W.denoise_stack(fr, [5, 3], cls, soft_threshold=soft),
                   W.denoise_stack(fr, [5, 3], cls, noise=noises, soft_threshold=soft),
                   f"denoise_stack MAD vs explicit noise {_shape_id(shape)} {fam} soft={soft}")


@pytest.mark.parametrize("shape", [(3, 130), (33, 31)], ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_zero_frame_between_loud_frames_stays_zero_at_level_8(shape, fam):
    W = _W()
    cls = getattr(W, fam)
    fr = hostile_stack(shape, 3)
    fr[2] = fr[0][::-1, ::-1] * np.float32(1.5)                  # both neighbours at 1e6
    fr[1] = 0
    assert np.abs(fr[0]).max() > 1e6 and np.abs(fr[2]).max() > 1e6
    got = W.transform_stack(fr, 8, cls)
    assert not np.any(_bits(got[1])), f"{int(np.count_nonzero(_bits(got[1])))} non-zero samples in the planes of frame 1"
    assert np.any(got[0]) and np.any(got[2])
    weights = [5, 3, 2, 1, 1, 0, 0, 0]
    for noise in (None, 0.7, [1e5, None, 3e5]):
        for soft in (True, False):
            den = W.denoise_stack(fr, weights, cls, noise=noise, soft_threshold=soft)
            assert not np.any(_bits(den[1])), (noise, soft)
            assert np.any(den[0]) and np.any(den[2])


# ---------------------------------------------------------------- B: wow_stack where its stencils bounce

def _wow_against_oracle(W, fr, fam, noise, kw, what):
    """wow_stack image and whitened planes of every frame vs oracle.wow of that frame, then bitwise vs wow()"""
    O = _O()
    cls = getattr(W, fam)

    def args():
        return fresh(kw)

    per = per_frame_noise(noise, len(fr))
    img, planes = W.wow_stack(fr, cls, noise=noise, return_coefficients=True, **args())
    for i, (f, n_i) in enumerate(zip(fr, per)):
        ref_img, ref_c = O.wow(f.copy(), fam.lower(), noise=n_i, **args())
        ref_c = ref_c.data
        assert planes[i].shape == ref_c.shape and img[i].shape == ref_img.shape, what
        measured_tol(f"wow_stack planes {what} frame {i}", planes[i], ref_c,
                     atol=WOW_TOL * float(np.abs(ref_c).max()), rtol=WOW_TOL)
        measured_tol(f"wow_stack image {what} frame {i}", img[i], ref_img,
                     atol=WOW_TOL * float(np.abs(ref_img).max()), rtol=WOW_TOL)
    res = [W.wow(f, cls, noise=n_i, **args()) for f, n_i in zip(fr, per)]
    _same_bits(img, np.stack([r[0] for r in res]), f"wow_stack image vs per-frame {what}")
    _same_bits(planes, np.stack([r[1].data for r in res]), f"wow_stack planes vs per-frame {what}")
    return planes


@pytest.mark.parametrize("shape", H1_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("ndc", sorted(H1_COEFFICIENTS))
def test_wow_stack_with_more_scales_than_the_frame_holds(shape, fam, ndc):
    """h = 1: n_scales = len(denoise_coefficients), not capped by the frame - dilations up to 256 on 4-pixel rows
    (gamma = 1: see test_stack_edges_cpu on the conditioning of the reference)"""
    W = _W()
    from wavelets_amd import batch as B
    fr = hostile_stack(shape, 3)
    kw = h1_keywords(ndc)
    for mode, noise in wow_noise_modes(3):
        assert B.wow_eligible(fr, ndc, getattr(W, fam), None, per_frame_noise(noise, 3))
        planes = _wow_against_oracle(W, fr, fam, noise, kw, f"h=1 dc{ndc} {_shape_id(shape)} {fam} {mode}")
        assert planes.shape == (3, ndc + 1) + shape


@pytest.mark.parametrize("shape", WOW_CASE_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("name", list(WOW_CASES))
def test_wow_stack_keyword_cases_against_the_oracle(shape, name):
    W = _W()
    kw = dict(WOW_CASES[name])
    fam = "Triangle" if kw.pop("scaling_function", None) == "triangle" else "B3spline"
    fr = hostile_stack(shape, 3)
    for mode, noise in wow_noise_modes(3):
        _wow_against_oracle(W, fr, fam, noise, kw, f"{name} {_shape_id(shape)} {mode}")


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (3, 130), (5, 5)], ids=_shape_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_wow_stack_without_scales_does_what_wow_does(shape, fam):
    """frames too small for one scale (utils._wow_n_scales <= 0 for B3): wow_stack raises what wow() raises for one
    such frame, or returns its bits"""
    W = _W()
    cls = getattr(W, fam)
    fr = hostile_stack(shape, 3)
    for kw in (dict(), dict(denoise_coefficients=[5, 2]), dict(h=.5, gamma=2)):
        try:
            res = [W.wow(f, cls, **dict(kw)) for f in fr]
        except Exception as e:              # noqa: BLE001 - whatever wow() raises is the contract here
            with pytest.raises(type(e)):
                W.wow_stack(fr, cls, return_coefficients=True, **dict(kw))
            continue
        img, planes = W.wow_stack(fr, cls, return_coefficients=True, **dict(kw))
        _same_bits(img, np.stack([r[0] for r in res]), f"degenerate wow_stack image {shape} {fam} {kw}")
        _same_bits(planes, np.stack([r[1].data for r in res]), f"degenerate wow_stack planes {shape} {fam} {kw}")


# ---------------------------------------------------------------- C: thousands of frames, and across the grid limit

def _all_frames_are_their_representative(got, rep, scale, what):
    """frame i of `got` == the result of representative rep[i] (the frame of scaling 1) times scale[i], bit for bit"""
    base = np.ascontiguousarray(got[base_index(0):base_index(0) + REPS])
    exp = base[rep] * scale.reshape((-1,) + (1,) * (got.ndim - 1))
    same = (_nanbits(got) == _nanbits(exp)).reshape(len(got), -1).all(axis=1)
    assert same.all(), f"{what}: {int((~same).sum())} of {len(got)} frames differ from their representative, " \
                       f"first frame {int(np.argmin(same))}"
    return base


@pytest.mark.parametrize("n,shape,level", BIG_STACKS, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("fam", FAMILIES)
def test_transform_stack_of_thousands_of_frames(n, shape, level, fam):
    """Frame i is representative i % 64 times 2 ** (i // 64 % 5 - 2).  A scaling by a power of two is exact in every
    step of the transform (products, sums and differences of values around 1: nothing comes near the denormal range,
    test_stack_edges_cpu.test_power_of_two_scaling_is_exact_in_the_reference), so every frame must be its
    representative's planes times that power bit for bit, and 64 oracle calls check all frames.  65 540 frames cross
    BATCH_MAX_FRAMES: two chunks, the second of five frames."""
    W, O = _W(), _O()
    from wavelets_amd import _lib as L
    cls = getattr(W, fam)
    fr, rep, scale = big_stack(n, shape)
    chunks = L.batch_chunks(n, shape[0], shape[1], level)
    assert [c for _, c in chunks] == ([L.BATCH_MAX_FRAMES, n - L.BATCH_MAX_FRAMES] if n > L.BATCH_MAX_FRAMES else [n])
    got = W.transform_stack(fr, level, cls)
    assert got.shape == (n, level + 1) + shape
    base = _all_frames_are_their_representative(got, rep, scale, f"transform_stack N={n} {fam}")
    for r, f in enumerate(representatives(shape)):
        amax = float(np.abs(f).max())
        measured(f"big stack planes N{n} {fam} representative {r}", base[r], O.atrous_standard(f, level, fam.lower()),
                 SMALL_PLANES * amax)
        measured(f"big stack recon N{n} {fam} representative {r}", base[r].sum(axis=0), f, SMALL_RECON * amax)
    # time budget: 1.8 s per case at 65 540 frames and 0.2 s at 4096 on the MI355X (host arithmetic included)


@pytest.mark.parametrize("fam", FAMILIES)
def test_denoise_and_wow_stack_of_thousands_of_frames(fam):
    """4096 frames of 16 x 16: the MAD medians, the moments and the gamma range of every frame come out of one
    reduction with the frame as a grid dimension.  Soft threshold only, where everything is exactly invariant: the
    thresholds scale with the frame (median, then products with constants), so the denoised frame is the
    representative's times the power of two; wow's whitened planes (without preserve_variance) and its gamma term are
    ratios in which the power cancels exactly, so they are the representative's own bits."""
    W, O = _W(), _O()
    cls = getattr(W, fam)
    n, shape, level = BIG_STACKS[0]
    fr, rep, scale = big_stack(n, shape)
    reps = representatives(shape)
    weights = [5, 3, 2, 1][:level]
    den = W.denoise_stack(fr, weights, cls, noise=None)
    base = _all_frames_are_their_representative(den, rep, scale, f"denoise_stack N={n} {fam}")
    for r, f in enumerate(reps):
        measured(f"big stack denoise N{n} {fam} representative {r}", base[r],
                 O.denoise(f.copy(), list(weights), fam.lower()), DENOISE_TOL * float(np.abs(f).max()))
    one = np.ones_like(scale)
    for kw in (dict(), dict(h=.5, gamma=2)):
        img, planes = W.wow_stack(fr, cls, return_coefficients=True, **kw)
        bimg = _all_frames_are_their_representative(img, rep, one, f"wow_stack image N={n} {fam} {kw}")
        bpl = _all_frames_are_their_representative(planes, rep, one, f"wow_stack planes N={n} {fam} {kw}")
        for r, f in enumerate(reps):
            ref_img, ref_c = O.wow(f.copy(), fam.lower(), **kw)
            measured_tol(f"big stack wow planes N{n} {fam} {kw} representative {r}", bpl[r], ref_c.data,
                         atol=WOW_TOL * float(np.abs(ref_c.data).max()), rtol=WOW_TOL)
            measured_tol(f"big stack wow image N{n} {fam} {kw} representative {r}", bimg[r], ref_img,
                         atol=WOW_TOL * float(np.abs(ref_img).max()), rtol=WOW_TOL)
    # time budget: 0.4 s per family on the MI355X; the whole module runs in about 15 s
