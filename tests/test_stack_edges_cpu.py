"""What tests/test_gpu_stack_edges.py rests on, checked without a device: the shape list and the edges it claims to
cover, the inputs (stacks whose neighbouring frames differ by nine decades), the oracle's own float32 error at those
shapes (the bounds of the GPU module are conftest's; the reference alone must use under half of them), the absence
of hard-threshold flips in the reference for the seeds used, and the exactness of a power-of-two scaling that lets
64 oracle calls vouch for 65 540 frames.  The GPU module imports its inputs from here."""
import numpy as np
import pytest

from conftest import SMALL_PLANES
from oracle import atrous_numpy as O

# (H, W) of the batched-engine edge tests.  (1, 2) and (513, 6) complete the list for two edges: a frame of exactly
# two samples (the even median of the smallest size) and a frame taller than the level-8 reach of both families
# (510 rows for B3, 255 for Triangle) while narrower than it.
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 130), (5, 5), (17, 4), (33, 31), (64, 9), (9, 258), (300, 517),
          (1, 2), (513, 6)]
FAMILIES = ["B3spline", "Triangle"]           # the package's classes; .lower() names the oracle's family
LEVELS = (2, 5, 8)
STACKS = (1, 2, 9)
AMPS = (1e6, 1e-3)                            # frame i: AMPS[i % 2] - every quiet frame lies between two loud ones
OFFSETS = (0.5, -0.75, 1.0)                   # frame i: + OFFSETS[i % 3] * its amplitude (no frame is zero-mean)
# Seed of every shape's stack: the smallest for which the REFERENCE-ONLY conditions of this module hold (the float32
# oracle within half of each bound of the float64 oracle, no hard-threshold flip between the two).  They are
# conditions on the inputs, evaluated without the engine: the dense 25-tap float32 sums of the oracle drift by more
# than half of SMALL_PLANES over eight scales for about one 1 x 1 B3 frame in five, and a seed is what keeps that
# noise of the reference out of a comparison that is about the engine.
SEED = 0
SEEDS = {(1, 1): 8, (7, 1): 1, (300, 517): 3, (1, 2): 7}
DENOISE_WEIGHTS = ([5, 3], [4, 2, 1, 0, 0])
DENOISE_TOL = 5.2e-7                          # tests/test_gpu_parity.py: DENOISE_TOL, times max|frame|

# section B (wow_stack).  h = 1 with gamma = 1: with the default gamma the image is x ** (1 / 3.2) of the normalised
# gamma term, whose slope near the frame's minimum amplifies the float32 rounding of the REFERENCE beyond WOW_TOL for
# these frames (float32 oracle against float64 oracle: up to 57 tolerances); test_wow_reference_is_well_conditioned
# holds the inputs used to under half a tolerance.  The default gamma is covered by the keyword cases h1 and h05_g2.
WOW_TOL = 5.2e-6                              # tests/test_gpu_parity.py, tests/test_gpu_wow_stack.py
WOW_SCALAR = 7e-4                             # the scalar noise of the wow cases: the quiet frames' order of magnitude
H1_COEFFICIENTS = {6: [5, 3, 2, 1, 0, 1], 9: [5, 3, 2, 1, 1, 0, 0.5, 0, 1]}
H1_SHAPES = [(33, 31), (17, 4), (64, 9), (300, 517)]
WOW_CASE_SHAPES = [(33, 31), (64, 9), (130, 67), (300, 517)]


def h1_keywords(ndc):
    return dict(h=1, gamma=1, denoise_coefficients=list(H1_COEFFICIENTS[ndc]))


def wow_noise_modes(n):
    return [(m, WOW_SCALAR if m == "scalar" else v) for m, v in noise_modes(n)]


def fresh(kw):
    """a copy of keyword arguments with fresh lists (wow() implementations extend the lists they are given)"""
    return {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}


# section C: N frames of a small shape, frame i = representative i % REPS times 2 ** (i // REPS % 5 - 2)
REPS = 64
BIG_STACKS = [(4096, (16, 16), 4), (65540, (8, 8), 2)]          # (N, shape, level)


def reach(level, fam):
    """rows / columns on either side that the smooth of `level` scales draws on"""
    return (2 if fam.lower() == "b3spline" else 1) * (2 ** level - 1)


def hostile_stack(shape, n=max(STACKS), seed=None):
    """n float32 frames of `shape`; the first k frames of the n-frame stack are the k-frame stack"""
    seed = SEEDS.get(tuple(shape), SEED) if seed is None else seed
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    fr = rng.standard_normal((n,) + tuple(shape))
    for i in range(n):
        fr[i] = fr[i] * AMPS[i % 2] + OFFSETS[i % 3] * AMPS[i % 2]
    return fr.astype(np.float32)


def noise_modes(n):
    """(name, `noise` of denoise_stack / wow_stack for n hostile frames): MAD, one scalar, one entry per frame (of
    the frame's own order of magnitude, with a None and a 0.0 among them when the stack is long enough)"""
    per = [0.8 * AMPS[i % 2] * (1 + 0.125 * i) for i in range(n)]
    if n > 3:
        per[3] = 0.0
    if n > 4:
        per[4] = None
    return [("mad", None), ("scalar", 0.7), ("list", per)]


def per_frame_noise(noise, n):
    return list(noise) if isinstance(noise, list) else [noise] * n


def hard_allow(shape):
    """samples of ONE frame that a hard-thresholded comparison may leave out: at most 0.1 % of the frame, none for
    frames of fewer than 1000 samples (a condition set before any measurement, not a measured figure)"""
    npix = shape[0] * shape[1]
    return npix // 1000 if npix >= 1000 else 0


def representatives(shape, seed=SEED):
    """REPS float32 frames of amplitude ~1 (|x| in ~1e-4 .. 6: with scalings by 2 ** -2 .. 2 ** 2 no product, sum or
    difference of the transform comes anywhere near the denormal range)"""
    rng = np.random.default_rng([seed, 7, shape[0], shape[1]])
    fr = rng.standard_normal((REPS,) + tuple(shape)) + np.linspace(-1.5, 1.5, REPS)[:, None, None]
    return fr.astype(np.float32)


def big_stack(n, shape):
    """(frames (n, H, W), representative index per frame, float32 power of two per frame)"""
    reps = representatives(shape)
    i = np.arange(n)
    rep, scale = i % REPS, np.exp2(i // REPS % 5 - 2).astype(np.float32)
    return reps[rep] * scale[:, None, None], rep, scale


def base_index(rep):
    """index of the frame of big_stack that IS representative `rep` (its scaling is 2 ** 0)"""
    return 2 * REPS + rep


def hard_masks(frame, weights, fam, noise, dtype):
    """the significance masks of oracle.denoise(frame.astype(dtype), weights, hard threshold), one per scale"""
    c = O.Coeffs(O.atrous_standard(frame.astype(dtype), len(weights), fam.lower()), fam.lower())
    c.noise = noise
    return [np.asarray(c.significance(sig, s, soft_threshold=False), bool) for s, sig in enumerate(weights)]


def test_shape_list_covers_the_edges_it_claims():
    hw = [h * w for h, w in SHAPES]
    assert len(set(SHAPES)) == len(SHAPES)
    # the eleven shapes the edge tests were specified with are all here
    assert set(SHAPES) >= {(1, 1), (1, 7), (7, 1), (2, 3), (3, 130), (5, 5), (17, 4), (33, 31), (64, 9), (9, 258),
                           (300, 517)}
    assert any(h == 1 for h, _ in SHAPES) and any(w == 1 for _, w in SHAPES) and 1 in hw and 2 in hw
    assert any(n % 2 and n > 1 for n in hw) and any(n % 2 == 0 and n > 2 for n in hw)
    assert any(1 < h < 5 for h, _ in SHAPES) and any(1 < w < 5 for _, w in SHAPES)
    assert {w % 4 for _, w in SHAPES} == {0, 1, 2, 3}
    assert {w % 4 for h, w in SHAPES if h > 1 and w > 1} == {0, 1, 2, 3}       # ... on frames of several rows
    for fam in FAMILIES:
        r = reach(8, fam)
        assert any(h < r < w for h, w in SHAPES), fam         # rows reflect (many times), columns do not leave the row
        assert any(w < r < h for h, w in SHAPES), fam         # and the reverse
        assert any(r > 8 * h for h, _ in SHAPES) and any(r > 8 * w for _, w in SHAPES)        # many bounces
    for fam in FAMILIES:                                      # the ordinary control: beyond the reach of level 5
        assert any(h > 2 * reach(5, fam) and w > 2 * reach(5, fam) for h, w in SHAPES)
    assert reach(8, "B3spline") == 510 and reach(8, "Triangle") == 255 and reach(2, "B3spline") == 6
    assert hard_allow((300, 517)) == 155 and hard_allow((33, 31)) == 1 and hard_allow((64, 9)) == 0
    assert all(hard_allow(s) <= 0.001 * s[0] * s[1] for s in SHAPES)


def test_hostile_stacks_are_hostile():
    for shape in SHAPES:
        fr = hostile_stack(shape)
        assert fr.dtype == np.float32 and fr.shape == (9,) + shape
        amax = np.abs(fr).reshape(9, -1).max(axis=1)
        for i in range(1, 9, 2):          # every quiet frame: both neighbours at least 1e7 times louder than it
            assert amax[i] * 1e7 < min(amax[i - 1], amax[i + 1]), shape
        assert len({f.tobytes() for f in fr}) == 9                             # all frames differ
        if shape[0] * shape[1] >= 30:                                          # no frame is zero-mean
            assert np.all(np.abs(fr.reshape(9, -1).mean(axis=1)) > 0.05 * np.take(AMPS, np.arange(9) % 2))
        for n in STACKS:
            assert np.array_equal(hostile_stack(shape, n), fr[:n])


@pytest.mark.parametrize("fam", FAMILIES)
def test_float32_reference_uses_under_half_of_the_plane_bound(fam):
    """oracle in float32 (what the GPU tests compare with) against the same oracle in float64, level 8, every shape
    and frame: below SMALL_PLANES / 2 times max|frame|"""
    worst = 0.0
    for shape in SHAPES:
        for f in hostile_stack(shape):
            d = np.abs(O.atrous_standard(f, 8, fam.lower()).astype(np.float64)
                       - O.atrous_standard(f.astype(np.float64), 8, fam.lower())).max()
            ratio = float(d) / (SMALL_PLANES * float(np.abs(f).max()))
            worst = max(worst, ratio)
            assert ratio < 0.5, (shape, fam, ratio)
    print(f"float32 oracle vs float64 oracle, {fam}: worst {worst:.3f} of SMALL_PLANES")


@pytest.mark.parametrize("fam", FAMILIES)
def test_reference_flips_no_hard_threshold_sample(fam):
    """For the seeds in use and every denoise case of the GPU module (both weight lists, the three noise modes, soft
    and hard threshold, all nine frames): the float32 reference lies within HALF of DENOISE_TOL of the float64
    reference at every sample - so no hard-threshold flip shows in the reference, and a sample beyond the bound on
    the GPU is the engine's - and the two agree on the significance of every sample.  (Frames of one or two samples
    are left out of the second statement only: their plane 0 is pure rounding, 0 in float64, and the MAD threshold
    with it; the first statement holds for them too.)"""
    for shape in SHAPES:
        fr = hostile_stack(shape)
        for weights in DENOISE_WEIGHTS:
            for name, noise in noise_modes(len(fr)):
                for i, (f, n_i) in enumerate(zip(fr, per_frame_noise(noise, len(fr)))):
                    for soft in (True, False):
                        d32 = O.denoise(f.copy(), weights, fam.lower(), n_i, soft_threshold=soft)
                        d64 = O.denoise(f.astype(np.float64), weights, fam.lower(), n_i, soft_threshold=soft)
                        ratio = float(np.abs(d32 - d64).max()) / (DENOISE_TOL * float(np.abs(f).max()))
                        assert ratio < 0.5, (shape, fam, weights, name, i, soft, ratio)
                    if shape[0] * shape[1] > 2:
                        m32 = hard_masks(f, weights, fam, n_i, np.float32)
                        m64 = hard_masks(f, weights, fam, n_i, np.float64)
                        flips = sum(int((a != b).sum()) for a, b in zip(m32, m64))
                        assert flips == 0, (shape, fam, weights, name, i, flips)


@pytest.mark.parametrize("n,shape,level", BIG_STACKS, ids=lambda v: str(v).replace(" ", ""))
def test_power_of_two_scaling_is_exact_in_the_reference(n, shape, level):
    """oracle(frame * 2 ** k) == oracle(frame) * 2 ** k bit for bit in float32 for the 64 representatives and k in
    -2 .. 2: every step of the transform is linear and no value is near the denormal range"""
    reps = representatives(shape)
    assert np.abs(reps).min() > 1e-6 and np.abs(reps).max() < 8
    fr, rep, scale = big_stack(n, shape)
    assert fr.dtype == np.float32 and fr.shape == (n,) + shape
    assert set(np.log2(scale).astype(int)) == {-2, -1, 0, 1, 2} and set(rep) == set(range(REPS))
    assert all(np.array_equal(fr[base_index(r)], reps[r]) for r in range(REPS))
    for fam in FAMILIES:
        for r in range(REPS):
            ref = O.atrous_standard(reps[r], level, fam.lower())
            nz = ref[ref != 0]
            assert nz.size == 0 or np.abs(nz).min() > 1e-30            # nothing that a scaling by 1/4 could denormalise
            for k in range(-2, 3):
                s = np.float32(2.0 ** k)
                got = O.atrous_standard(reps[r] * s, level, fam.lower())
                assert np.array_equal(got.view(np.uint32), (ref * s).view(np.uint32)), (shape, fam, r, k)


def _wow_reference_ratio(got, ref):
    ref = np.asarray(ref, np.float64)
    tol = WOW_TOL * np.abs(ref).max() + WOW_TOL * np.abs(ref)
    return float((np.abs(np.asarray(got, np.float64) - ref) / tol).max())


def test_wow_reference_is_well_conditioned():
    """every wow comparison of the GPU module (section B): the float32 oracle against the float64 oracle, planes and
    image of every frame, stays under half of the tolerance the engine is held to"""
    from test_gpu_wow_stack import CASES
    todo = [(shape, fam, h1_keywords(ndc)) for shape in H1_SHAPES for fam in FAMILIES for ndc in sorted(H1_COEFFICIENTS)]
    for shape in WOW_CASE_SHAPES:
        for kw in CASES.values():
            kw = dict(kw)
            fam = "Triangle" if kw.pop("scaling_function", None) == "triangle" else "B3spline"
            todo.append((shape, fam, kw))
    for shape, fam, kw in todo:
        fr = hostile_stack(shape, 3)
        for mode, noise in wow_noise_modes(3):
            for i, (f, n_i) in enumerate(zip(fr, per_frame_noise(noise, 3))):
                i32, c32 = O.wow(f.copy(), fam.lower(), noise=n_i, **fresh(kw))
                i64, c64 = O.wow(f.astype(np.float64), fam.lower(), noise=n_i, **fresh(kw))
                worst = max(_wow_reference_ratio(c32.data, c64.data), _wow_reference_ratio(i32, i64))
                assert worst < 0.5, (shape, fam, kw, mode, i, worst)
