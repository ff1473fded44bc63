"""The numpy oracle against the reference at the edge shapes of signals and cubes (tests/golden/g26_nd_edges.npz:
axes of length 1 and 2, n = 1..3 under the 1-D 'mirror' border, dozens of bounces on Y), and the bookkeeping of
tests/test_gpu_nd_edges.py: its parameter lists hold every shape and level, its hard-threshold inputs keep clear of
their thresholds.  CPU only.

Tolerances: those tests/test_oracle_golden.py uses for the same oracle functions - float64: 1e-12 * max|input| for
the standard transform, convolutions and denoise, 1e-11 for user-defined taps and the recursive algorithm, 1e-10
with bilateral weights; float32 (the two wide cubes): 1e-5 * max|input|; wow: 2e-5 * max|reference|.
"""
import numpy as np
import pytest

from oracle import atrous_numpy as O
from conftest import load_golden
import test_gpu_nd_edges as T

ISSUE_SIGNALS = (1, 2, 3, 4, 5, 9, 257)
ISSUE_CUBES = ((1, 1, 1), (2, 2, 2), (1, 5, 7), (7, 1, 5), (5, 4, 1), (2, 3, 4), (3, 2, 9),
               (6, 3, 130), (3, 5, 257), (33, 3, 5))
WIDE = ((6, 3, 130), (3, 5, 257))
SHAPES = tuple((n,) for n in ISSUE_SIGNALS) + ISSUE_CUBES


def close(a, b, atol):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    np.testing.assert_allclose(a.astype(np.float64), b.astype(np.float64), rtol=0, atol=atol)


def test_fixture_holds_every_shape():
    g = load_golden("g26_nd_edges")
    assert tuple(g["signals"]) == ISSUE_SIGNALS and tuple(map(tuple, g["cubes"])) == ISSUE_CUBES
    for shape in SHAPES:
        a = g[f"in_{T.tag_of(shape)}"]
        assert a.shape == shape and a.dtype == np.float32


@pytest.mark.parametrize("shape", SHAPES, ids=T.tag_of)
def test_oracle_vs_reference(shape):
    g = load_golden("g26_nd_edges")
    tag, nd = T.tag_of(shape), len(shape)
    wide = shape in WIDE
    a = g[f"in_{tag}"] if wide else g[f"in_{tag}"].astype(np.float64)
    amax = float(np.abs(a).max())
    plain, taps, weighted = ((1e-5 * amax,) * 3) if wide else (1e-12 * amax, 1e-11 * amax, 1e-10 * amax)
    levels = T.LEVELS[nd]
    standard, conv = (O.atrous_standard_1d, O.convolution_1d) if nd == 1 else (O.atrous_standard_3d, O.convolution_3d)
    for fam in T.FAMS:
        top = f"coef_{fam}_{tag}_L{levels[-1]}"
        if top in g:
            close(standard(a, levels[-1], fam), g[top], plain)
            close(O.atrous_standard_nd(a, levels[-1], fam), g[top], plain)
            for L in levels[:-1]:
                ref = np.concatenate([g[top][:L], g[f"smooth_{fam}_{tag}_L{L}"][None]])
                close(standard(a, L, fam), ref, plain)
            close(conv(a, fam, 0), g[f"smooth_{fam}_{tag}_L1"], plain)
        for s in (2, 5):
            if f"conv_{fam}_{tag}_s{s}" in g:
                close(conv(a, fam, s), g[f"conv_{fam}_{tag}_s{s}"], plain)
                close(O.convolution_nd(a, fam, s), g[f"conv_{fam}_{tag}_s{s}"], plain)
    assert f"conv_triangle_{tag}_s5" in g and f"coef_b3spline_{tag}_L{levels[-1]}" in g
    noise = O.Coeffs(O.atrous_standard_nd(a, 2, "b3spline"), "b3spline").get_noise()
    assert abs(noise - float(g[f"noise_{tag}"])) <= (1e-5 if wide else 1e-12) * float(g[f"noise_{tag}"])
    close(O.denoise(a.copy(), [4, 2], "b3spline"), g[f"den_{tag}"], plain)
    if f"raises_wow_{tag}" in g:
        with pytest.raises(getattr(__import__("builtins"), str(g[f"raises_wow_{tag}"]))):
            O.wow(a.copy(), denoise_coefficients=[4], n_scales=2)
    elif shape in T.WOW_SHAPES:
        r, c = O.wow(a.copy(), denoise_coefficients=[4], n_scales=2)
        close(r, g[f"wow_{tag}"], 2e-5 * float(np.abs(g[f"wow_{tag}"]).max()))
        close(c.data, g[f"wow_{tag}_coef"], 2e-5 * float(np.abs(g[f"wow_{tag}"]).max()))
    if wide:
        return
    close(O.sdev_loc_nd(a, "b3spline", 1, variance=True), g[f"var_{tag}_s1"], 2e-5)
    close(O.atrous_standard_nd(a, 3, "b3spline", 1), g[f"bil_{tag}_L3"], weighted)
    close(O.atrous_standard_bilateral_taps_nd(a, 3, O.TAPS["b3spline"], 1), g[f"bil_{tag}_L3"], weighted)
    close(O.atrous_recursive_nd(a, 3, "b3spline"), g[f"rec_{tag}_L3"], taps)
    close(O.atrous_recursive_taps_nd(a, 3, O.TAPS["b3spline"]), g[f"rec_{tag}_L3"], taps)
    close(O.atrous_recursive_nd(a, 3, "b3spline", 1), g[f"recbil_{tag}_L3"], weighted)
    skew5 = O.CustomFamily(g["skew5_taps"], {})
    close(O.atrous_standard_nd(a, 3, skew5), g[f"skew5_coef_{tag}_L3"], taps)
    close(O.atrous_standard_taps_nd(a, 3, g["skew5_taps"]), g[f"skew5_coef_{tag}_L3"], taps)
    close(O.atrous_recursive_taps_nd(a, 3, g["even4_taps"], 1), g[f"even4_recbil_{tag}_L3"], weighted)


def test_gpu_parameter_lists_hold_every_shape_and_level():
    """tests/test_gpu_nd_edges.py must keep every shape, level, family and dtype: dropping one fails here"""
    assert T.SIGNALS == ISSUE_SIGNALS and T.CUBES == ISSUE_CUBES and T.SHAPES == SHAPES
    assert T.LEVELS == {1: (1, 3, 7), 3: (1, 3, 5)} and T.CONV_SCALES == (0, 2, 5)
    assert T.FAMS == ("b3spline", "triangle") and T.DTYPES == ("float32", "float64")
    assert len(T.CASES) == len(set(T.CASES)) == 17 * 2 * 2
    assert set(T.CASES) == {(s, f, d) for s in SHAPES for f in T.FAMS for d in T.DTYPES}
    assert set(T.CUSTOM_CASES) == {(s, n, d) for s in SHAPES for n in ("skew5", "even4") for d in T.DTYPES}
    assert T.CUSTOM_MODES == ("plain", "bilateral", "recursive", "recursive_bilateral")
    assert T.WOW_SHAPES == ((5,), (9,), (257,), (2, 2, 2), (2, 3, 4), (3, 2, 9), (6, 3, 130), (3, 5, 257), (33, 3, 5))
    assert set(T.WOW_CASES) == {(s, d) for s in T.WOW_SHAPES for d in T.DTYPES}

    def cases_of(test):
        (mark,) = [m for m in test.pytestmark if m.name == "parametrize" and m.args[0] == "case"]
        return mark.args[1]
    for name in ("test_transform_planes_and_reconstruction", "test_convolution", "test_bilateral_transform",
                 "test_recursive_transform", "test_denoise_soft", "test_noise_estimate"):
        assert cases_of(getattr(T, name)) is T.CASES, name
    assert cases_of(T.test_user_defined_taps) is T.CUSTOM_CASES and cases_of(T.test_wow) is T.WOW_CASES
    # the reach of the top level exceeds two periods of Y in at least one cube case; a signal of one sample is there
    hw = {"b3spline": 2, "triangle": 1}
    assert any(len(s) == 3 and hw[f] * 2 ** (T.LEVELS[3][-1] - 1) > 2 * s[1] for s, f, _ in T.CASES)
    assert any(s == (1,) for s, _, _ in T.CASES)
    assert sorted(len(s) for s, _ in T.HARD_CASES) == [1, 3]


@pytest.mark.parametrize("shape,seed", T.HARD_CASES, ids=lambda v: T.tag_of(v) if isinstance(v, tuple) else str(v))
def test_hard_threshold_inputs_keep_clear_of_their_thresholds(shape, seed):
    """no coefficient of the float64 oracle within 1e-4 relative of its threshold: rounding of either engine (1e-6
    relative at worst) cannot flip a sample, so the GPU test allows none"""
    assert T.hard_threshold_margin(O, shape, seed) > T.HARD_MARGIN == 1e-4
