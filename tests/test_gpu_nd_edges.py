"""1-D signals and (Z, Y, X) cubes at their edge shapes, on the float32 and the float64 engine, through the
public API (run with -m gpu on an MI355X).

Signals go through the 'mirror' border of the reference's 1-D branch (period 2n - 2, a constant for n = 1:
border codes 2 and 3 of wt_refl_b); a cube lives on a plan as a (Z*Y) x X image whose y reflection has to stay
inside its own slice.  The shapes: axes of length 1 and 2, n = 1..3, Y = 1..5 under a reach of up to 32 samples
(dozens of bounces inside every slice), wide-and-shallow and narrow-and-deep cubes around the float4 group.

Reference: tests/golden/g26_nd_edges.npz (the unmodified reference, float64 arithmetic on the float32 input
samples; float32 on the two wide cubes) where it has the key, else the numpy oracle in the engine's dtype -
tests/test_nd_edges_cpu.py pins the oracle to the same fixture on every shape.

Tolerances.  float64 engine: 1e-13 * max|input| for planes and convolutions, 1e-12 * max|input| with bilateral
weights, denoise or wow (the bounds of test_dtype_policy and of the g20 tests).  float32 engine: SMALL_PLANES /
SMALL_RECON for planes and convolutions; for bilateral transforms, denoise and wow 4 x the worst error these
tests logged on MI355X through conftest.measured / measured_tol (profiles/nd_edges_parity_errors.log).
"""
import numpy as np
import pytest

from conftest import measured_tol, load_golden, measured, SMALL_PLANES, SMALL_RECON

pytestmark = pytest.mark.gpu

FAMS = ("b3spline", "triangle")
DTYPES = ("float32", "float64")
SIGNALS = (1, 2, 3, 4, 5, 9, 257)
CUBES = ((1, 1, 1), (2, 2, 2), (1, 5, 7), (7, 1, 5), (5, 4, 1), (2, 3, 4), (3, 2, 9),
         (6, 3, 130), (3, 5, 257), (33, 3, 5))
SHAPES = tuple((n,) for n in SIGNALS) + CUBES
LEVELS = {1: (1, 3, 7), 3: (1, 3, 5)}            # by dimensionality
CONV_SCALES = (0, 2, 5)
WIDE = ((6, 3, 130), (3, 5, 257))                # the fixture holds a float32 run of the reference for these two
CUSTOM = ("skew5", "even4")
CUSTOM_MODES = ("plain", "bilateral", "recursive", "recursive_bilateral")


def tag_of(shape):
    return "x".join(map(str, shape))


def _id(case):
    return "-".join([tag_of(case[0])] + [str(v) for v in case[1:]])


CASES = [(shape, fam, dtype) for shape in SHAPES for fam in FAMS for dtype in DTYPES]
CUSTOM_CASES = [(shape, name, dtype) for shape in SHAPES for name in CUSTOM for dtype in DTYPES]
WOW_SHAPES = tuple(s for s in SHAPES if (s[0] >= 5 if len(s) == 1 else min(s) >= 2))
WOW_CASES = [(shape, dtype) for shape in WOW_SHAPES for dtype in DTYPES]
# hard threshold, one input per dimensionality: seeds at which no float64 coefficient of the oracle lies within 1e-4
# relative of its threshold (asserted by tests/test_nd_edges_cpu.py), so no sample may flip on either engine
HARD_CASES = (((257,), 2), ((3, 5, 257), 1))
HARD_MARGIN = 1e-4

# float64 engine (the bounds test_dtype_policy and the g20 tests assert for the same calls), times max|input|
F64_PLANES = 1e-13
F64_WEIGHTED = 1e-12
# float32 engine: 4 x the worst error of each group in profiles/nd_edges_parity_errors.log, times max|input|
# (wow: times max|reference|; the log's third column is the absolute error, its fourth the bound asserted)
BIL32 = 6.6e-6       # bilateral transforms (measured 1.65e-6, log line 625: test_bilateral_transform[2-b3spline-float32], L1 - on two
                     # samples the variance conv(I^2) - conv(I)^2 cancels to its rounding; 7.5e-7 at worst on every other shape)
RECBIL32 = 5.7e-5    # recursive bilateral (measured 1.40e-5, log line 844: test_recursive_transform[2-triangle-float32], L3 - as above,
                     # on every two-sample sub-array of the padded signal)
DEN32 = 5.7e-7       # denoise, soft and hard threshold (measured 1.41e-7, log line 1385: test_denoise_soft[257-b3spline-float32])
WOW32 = 7.7e-7       # wow planes and image (measured 1.91e-7, log line 1441: test_wow[257-float32], "wow planes")


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


@pytest.fixture(scope="module")
def O():
    from oracle import atrous_numpy
    return atrous_numpy


_G = []


def fixture():
    if not _G:
        _G.append(load_golden("g26_nd_edges"))
    return _G[0]


def data(shape, dtype):
    return fixture()[f"in_{tag_of(shape)}"].astype(dtype)


def custom_taps(name):
    return fixture()[f"{name}_taps"]


_REF = {}


def reference(O, kind, shape, fam, dtype, *args):
    """The reference result of one call: from the fixture where it has the key, else from the oracle in `dtype`.
    Computed once per (call, shape, family, dtype) and shared; callers must not modify it.  A recorded exception
    of the reference comes back as its class name (a str)."""
    key = (kind, shape, fam, dtype) + args
    if key not in _REF:
        r = _reference(O, kind, shape, fam, dtype, *args)
        if isinstance(r, np.ndarray):
            r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _reference(O, kind, shape, fam, dtype, *args):
    g, tag, a = fixture(), tag_of(shape), data(shape, dtype)
    if shape in WIDE and dtype == "float64":          # (a float32 run is no reference for the float64 engine: the oracle)
        g = {}
    if kind == "planes":
        (L,) = args
        top = f"coef_{fam}_{tag}_L{LEVELS[len(shape)][-1]}"
        if top in g and L == LEVELS[len(shape)][-1]:
            return g[top]
        if top in g and f"smooth_{fam}_{tag}_L{L}" in g:      # (detail planes do not depend on the level count)
            return np.concatenate([g[top][:L], g[f"smooth_{fam}_{tag}_L{L}"][None]])
        return O.atrous_standard_nd(a, L, fam)
    if kind == "conv":
        (s,) = args
        k = f"smooth_{fam}_{tag}_L1" if s == 0 else f"conv_{fam}_{tag}_s{s}"
        return g[k] if k in g else O.convolution_nd(a, fam, s)
    if kind == "bilateral":
        L, scaling = args
        k = f"bil_{tag}_L{L}"
        if fam == "b3spline" and not scaling and k in g:
            return g[k]
        return O.atrous_standard_nd(a, L, fam, 1, scaling)
    if kind == "recursive":
        L, bil = args
        k = f"{'recbil' if bil else 'rec'}_{tag}_L{L}"
        if fam == "b3spline" and k in g:
            return g[k]
        return O.atrous_recursive_nd(a, L, fam, bil)
    if kind == "custom":                              # `fam` is the name of the user-defined scaling function
        mode, L = args
        k = {"plain": f"{fam}_coef_{tag}_L{L}", "recursive_bilateral": f"{fam}_recbil_{tag}_L{L}"}.get(mode)
        if k in g:
            return g[k]
        t = custom_taps(fam)
        if mode == "plain":
            return O.atrous_standard_taps_nd(a, L, t)
        if mode == "bilateral":
            return O.atrous_standard_bilateral_taps_nd(a, L, t, 1)
        return O.atrous_recursive_taps_nd(a, L, t, 1 if mode == "recursive_bilateral" else None)
    if kind == "denoise":
        k = f"den_{tag}"
        return g[k] if fam == "b3spline" and k in g else O.denoise(a.copy(), [4, 2], fam)
    if kind == "noise":
        k = f"noise_{tag}"
        if fam == "b3spline" and k in g:
            return float(g[k])
        return float(O.Coeffs(O.atrous_standard_nd(a, 2, fam), fam).get_noise())
    if kind == "wow":
        if f"raises_wow_{tag}" in fixture():           # (n_scales < 0 whatever the dtype: holds for both engines)
            return str(fixture()[f"raises_wow_{tag}"])
        if f"wow_{tag}" in g and f"wow_{tag}_coef" in g:
            return g[f"wow_{tag}"], g[f"wow_{tag}_coef"]
        r, c = O.wow(a.copy(), denoise_coefficients=[4], n_scales=2)
        return r, c.data
    raise KeyError(kind)


def hard_input(shape, seed, dtype):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32).astype(dtype)


def hard_threshold_margin(O, shape, seed):
    """min over the thresholded coefficients of | |w| / tau - 1 | for the float64 oracle's denoise(a, [4, 2])"""
    a = hard_input(shape, seed, np.float64)
    c = O.Coeffs(O.atrous_standard_nd(a, 2, "b3spline"), "b3spline")
    noise = c.get_noise()
    return min(float(np.abs(np.abs(c.data[s]) / (sig * noise * c.sigma_e[s]) - 1).min()) for s, sig in enumerate([4, 2]))


def cls_of(W, fam):
    return {"b3spline": W.B3spline, "triangle": W.Triangle}[fam]


_CUSTOM_CLS = {}


def custom_cls(W, name):
    """Skew5: five taps that are not symmetric (a reversed tap order shows; wt_custom_rows_kernel /
    wt_custom_axis_kernel).  Even4: the four-tap class of test_gpu_round4.py (tap-list operator, pad modes 5, 6)."""
    if name not in _CUSTOM_CLS:
        g = fixture()

        class Custom(W.AbstractScalingFunction):
            coefficients_1d = np.array(g[f"{name}_taps"])
            sigma_e_1d = np.array(g["custom_sigma_e_1d"])
            sigma_e_2d = np.array([0.9, 0.2, 0.09, 0.04, 0.02, 0.01])
            sigma_e_3d = np.array(g["custom_sigma_e_3d"])

            def __init__(self, *args, **kwargs):
                super().__init__(name, *args, **kwargs)
        _CUSTOM_CLS[name] = Custom
    return _CUSTOM_CLS[name]


def bounds(dtype, a, weighted32=None):
    """(bound on planes / convolutions, bound on np.sum(planes)) - or the weighted bound when one is named"""
    amax = float(np.abs(a).max())
    if dtype == "float64":
        return (F64_WEIGHTED if weighted32 is not None else F64_PLANES) * amax, F64_PLANES * amax
    return (weighted32 if weighted32 is not None else SMALL_PLANES) * amax, SMALL_RECON * amax


def check_planes(what, c, ref, a, dtype, bound):
    assert c.data.shape == ref.shape == (len(c),) + a.shape and c.data.dtype == np.dtype(dtype)
    measured(what, c.data, ref, bound)


# --------------------------------------------------------------------------- plain transform, convolution
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_transform_planes_and_reconstruction(W, O, case):
    shape, fam, dtype = case
    a = data(shape, dtype)
    plane_b, recon_b = bounds(dtype, a)
    for L in LEVELS[len(shape)]:
        c = W.AtrousTransform(cls_of(W, fam))(a, L)
        check_planes(f"planes {dtype} L{L}", c, reference(O, "planes", shape, fam, dtype, L), a, dtype, plane_b)
        measured(f"reconstruction {dtype} L{L}", np.sum(c, axis=0), a, recon_b)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_convolution(W, O, case):
    shape, fam, dtype = case
    a = data(shape, dtype)
    for s in CONV_SCALES:
        got = W.convolution(a, cls_of(W, fam)(len(shape)), s=s)
        assert got.shape == a.shape and got.dtype == np.dtype(dtype)
        measured(f"convolution {dtype} s{s}", got, reference(O, "conv", shape, fam, dtype, s), bounds(dtype, a)[0])


# --------------------------------------------------------------------------- bilateral, recursive
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bilateral_transform(W, O, case):
    """K^3 range-weighted kernel + wt_local_variance3d on a cube; on a signal the variance under 'mirror' and
    the filter under the symmetric pad"""
    shape, fam, dtype = case
    a = data(shape, dtype)
    b = bounds(dtype, a, BIL32)[0]
    for L, scaling in ((1, False), (3, False), (3, True)):
        c = W.AtrousTransform(cls_of(W, fam), bilateral=1, bilateral_scaling=scaling)(a, L)
        check_planes(f"bilateral {dtype} L{L} scaling={scaling}", c, reference(O, "bilateral", shape, fam, dtype, L, scaling),
                     a, dtype, b)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_recursive_transform(W, O, case):
    shape, fam, dtype = case
    a = data(shape, dtype)
    for L in (1, 3):
        c = W.AtrousTransform(cls_of(W, fam))(a, L, recursive=True)
        check_planes(f"recursive {dtype} L{L}", c, reference(O, "recursive", shape, fam, dtype, L, None), a, dtype,
                     bounds(dtype, a)[0])
        c = W.AtrousTransform(cls_of(W, fam), bilateral=1)(a, L, recursive=True)
        check_planes(f"recursive bilateral {dtype} L{L}", c, reference(O, "recursive", shape, fam, dtype, L, 1), a, dtype,
                     bounds(dtype, a, RECBIL32)[0])


# --------------------------------------------------------------------------- user-defined scaling functions
@pytest.mark.parametrize("case", CUSTOM_CASES, ids=_id)
def test_user_defined_taps(W, O, case):
    shape, name, dtype = case
    a = data(shape, dtype)
    cls = custom_cls(W, name)
    for mode in CUSTOM_MODES:
        bil = 1 if "bilateral" in mode else None
        c = W.AtrousTransform(cls, bilateral=bil)(a, 3, recursive=mode.startswith("recursive"))
        b = bounds(dtype, a, None if bil is None else (RECBIL32 if mode.startswith("recursive") else BIL32))[0]
        check_planes(f"{name} {mode} {dtype} L3", c, reference(O, "custom", shape, name, dtype, mode, 3), a, dtype, b)


# --------------------------------------------------------------------------- denoise, wow, noise estimate
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_denoise_soft(W, O, case):
    shape, fam, dtype = case
    a = data(shape, dtype)
    got = W.denoise(a.copy(), [4, 2], cls_of(W, fam))
    assert got.shape == a.shape and got.dtype == np.dtype(dtype)
    measured(f"denoise {dtype}", got, reference(O, "denoise", shape, fam, dtype), bounds(dtype, a, DEN32)[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,seed", HARD_CASES, ids=lambda v: tag_of(v) if isinstance(v, tuple) else str(v))
def test_denoise_hard_threshold_flips_no_sample(W, O, shape, seed, dtype):
    a = hard_input(shape, seed, dtype)
    got = W.denoise(a.copy(), [4, 2], W.B3spline, soft_threshold=False)
    ref = O.denoise(a.copy(), [4, 2], "b3spline", soft_threshold=False)
    measured_tol(f"denoise hard {dtype}", got, ref, bounds(dtype, a, DEN32)[0], allow=0)


@pytest.mark.parametrize("case", WOW_CASES, ids=_id)
def test_wow(W, O, case):
    """wow(a, denoise_coefficients=[4], n_scales=2): the reference cuts n_scales to round(log2(min(shape)) -
    log2(5)) - 0 for n = 5 and 9, and -1 for every cube here, where it raises IndexError: so must the engine"""
    shape, dtype = case
    a = data(shape, dtype)
    ref = reference(O, "wow", shape, "b3spline", dtype)
    if isinstance(ref, str):
        with pytest.raises(getattr(__import__("builtins"), ref)):
            W.wow(a.copy(), denoise_coefficients=[4], n_scales=2)
        return
    r, c = W.wow(a.copy(), denoise_coefficients=[4], n_scales=2)
    assert r.shape == a.shape and r.dtype == np.dtype(dtype) and c.data.shape == ref[1].shape
    scale = float(np.abs(ref[0]).max())
    b = (F64_WEIGHTED if dtype == "float64" else WOW32) * scale
    measured(f"wow planes {dtype}", c.data, ref[1], b)
    measured(f"wow {dtype}", r, ref[0], b)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_noise_estimate(W, O, case):
    """Coefficients.get_noise(): the exact median of a plane of 1 to 3855 samples, 1-D and 3-D sigma_e tables.
    The median is 1-Lipschitz in the sup norm, so the estimate inherits the bound of plane 0."""
    shape, fam, dtype = case
    a = data(shape, dtype)
    c = W.AtrousTransform(cls_of(W, fam))(a, 2)
    got = c.get_noise()
    assert got == np.median(np.abs(c.data[0])) / 0.6745 / c.sigma_e[0]
    sigma_e0 = float(O.sigma_e(fam, None, len(shape))[0])
    assert float(c.sigma_e[0]) == sigma_e0
    measured(f"noise {dtype}", got, reference(O, "noise", shape, fam, dtype), bounds(dtype, a)[0] / 0.6745 / sigma_e0)


# --------------------------------------------------------------------------- slice isolation
def _dyadic5(W):
    """asymmetric user-defined taps with dyadic values: on integer samples every product and sum is exact"""
    if "dyadic5" not in _CUSTOM_CLS:
        class Dyadic5(W.AbstractScalingFunction):
            coefficients_1d = np.array([1 / 16, 1 / 4, 1 / 2, 1 / 8, 1 / 16])

            def __init__(self, *args, **kwargs):
                super().__init__("dyadic5", *args, **kwargs)
        _CUSTOM_CLS["dyadic5"] = Dyadic5
    return _CUSTOM_CLS["dyadic5"]


def _z_filter(O, taps, values, s, flip):
    """1-D filter along axis 0 under the symmetric border (the reference correlates: ref wavelets.py:54-63)"""
    taps = np.asarray(taps, np.float64)[::-1] if flip else np.asarray(taps, np.float64)
    hw, Z = len(taps) // 2, values.shape[0]
    out = np.zeros(values.shape, np.float64)
    for j, k in enumerate(taps):
        out += k * values[O.reflect_index(np.arange(Z) + (j - hw) * 2 ** s, Z)]
    return out


ISOLATION = ("b3spline", "triangle", "dyadic5")


def _isolation_cls(W, name):
    return _dyadic5(W) if name == "dyadic5" else cls_of(W, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ISOLATION)
def test_one_slice_cube_equals_the_image_bit_for_bit(W, O, name, dtype):
    """Integer samples in [-8, 8] and dyadic taps: every partial sum of the separable filter is exact in float32,
    whatever its order, so the comparisons are bit for bit.  (a) A cube with Z = 1 is its only slice run as an
    image (all z taps reflect onto that slice and add up to 1).  (b) In a cube whose slices are zero but for z0,
    slice z holds the image's result times the z response of a delta at z0: nothing of slice z0 may reach the
    rows of another slice except through the z filter."""
    cls = _isolation_cls(W, name)
    rng = np.random.default_rng(26)
    for (Y, X) in ((3, 9), (2, 130), (5, 7)):
        img = rng.integers(-8, 9, (Y, X)).astype(dtype)
        for s in (0, 1, 2, 4):
            want = W.convolution(img, cls(2), s=s)
            np.testing.assert_array_equal(W.convolution(img[None], cls(3), s=s)[0], want)
            Z, z0 = 4, 1
            cube = np.zeros((Z, Y, X), dtype)
            cube[z0] = img
            delta = np.zeros(Z)
            delta[z0] = 1
            zresp = _z_filter(O, cls.coefficients_1d, delta, s, flip=False)
            got = W.convolution(cube, cls(3), s=s)
            np.testing.assert_array_equal(got, (zresp[:, None, None] * want[None].astype(np.float64)).astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ISOLATION)
@pytest.mark.parametrize("shape", [(6, 3, 130), (3, 2, 9)], ids=tag_of)
def test_constant_slices_pass_the_in_slice_stages_unchanged(W, O, shape, name, dtype):
    """Slices that are constant, with a different value each, at s = 4 (a reach of 32 on Y = 3 or 2): the in-slice
    stages must leave every slice at its value, so the result is the 1-D z filter of the per-slice constants.  A
    y reflection that leaves its slice (period Z*Y instead of Y) mixes the constants and fails here."""
    cls = _isolation_cls(W, name)
    consts = np.random.default_rng(27).standard_normal(shape[0]).astype(np.float32).astype(dtype)
    cube = np.ascontiguousarray(np.broadcast_to(consts[:, None, None], shape))
    got = W.convolution(cube, cls(3), s=4)
    want = _z_filter(O, cls.coefficients_1d, consts.astype(np.float64), 4, flip=False)
    measured(f"constant slices {name} {dtype}", got, np.broadcast_to(want[:, None, None], shape), bounds(dtype, consts)[0])
