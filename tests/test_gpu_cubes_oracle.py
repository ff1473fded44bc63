"""The float32 cube engine (wavelets_amd.cubes: transform_cube / denoise_cube over wt_decompose_cube and
wt_cube_scale_kernel) against the float64 numpy oracle - oracle.atrous_numpy.atrous_standard_3d and denoise in float64 on
the float32 samples - where the kernel can go wrong and tests/test_gpu_cubes.py only meets the library's own old
sequence (run with -m gpu on an MI355X).

  A  planes at the kernel's edges: a dilation beyond Y or Z, chunked z chains, full and ragged row groups and x blocks
  B  a cube whose planes reach the size at which the kernel stores with streaming stores
  C  values: NaN and inf samples, signed zeros, flat cubes, powers of two, denormals, slice isolation
  D  denoise_cube: soft and hard thresholds and the Anscombe pair
  E  a pooled plan handed from cube to cube to image, a plan closed while pooled, and the eligible inputs that are not
     contiguous float32

Every A - D test runs with the per-scale choice left to the host and forced each way (WT_CUBE_FUSED, the MODES of
tests/test_gpu_cubes.py).  Every engine call runs on a plan whose planes were just filled with NaN (poisoned_plan): a
pooled plan keeps the planes of its last owner, which would otherwise be the reference's own right answer.

Bounds.  Planes SMALL_PLANES, reconstruction SMALL_RECON (conftest), denoise DEN32 (tests/test_gpu_nd_edges.py), each
times max|input|: the bounds the project holds the same operations to through the old sequence.  ANSCOMBE32 is 4 x the
error of the utils.denoise route against the oracle, quoted at the constant from
profiles/cubes_oracle_parity_errors.log.  No bound comes from the cube engine's own output.  "Same bytes" is equality of
the uint32 views once every NaN is one canonical NaN: the signs of zeros count.

tests/test_cubes_oracle_cpu.py holds, without a device, what this file rests on: the hard-threshold margins of
HARD_SEEDS, the oracle's NaN masks, the corner-block rule of B and the chunk layouts claimed in A.
"""
import numpy as np
import pytest

from conftest import measured, measured_tol, SMALL_PLANES, SMALL_RECON
from test_gpu_nd_edges import DEN32, HARD_MARGIN
from test_gpu_cubes import FAMS, MODES, cls_of, cube

pytestmark = pytest.mark.gpu

WEIGHTS = [5, 3]
HW = {"b3spline": 2, "triangle": 1}

modes = pytest.mark.parametrize("mode", MODES, ids=lambda m: "rule" if m is None else "fused" + m)
fams = pytest.mark.parametrize("fam", FAMS)


def tag_of(shape):
    return "x".join(map(str, shape))


def _case_id(v):
    return tag_of(v) if isinstance(v, tuple) else f"L{v}"


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


def use_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("WT_CUBE_FUSED", raising=False)
    else:
        monkeypatch.setenv("WT_CUBE_FUSED", mode)


_CACHE = {}


def shared(key, make):
    """make() once per key; arrays are left read-only and shared among the tests"""
    if key not in _CACHE:
        r = make()
        if isinstance(r, np.ndarray):
            r.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def oracle_planes(O, a, level, fam):
    return O.atrous_standard_3d(np.asarray(a, np.float32).astype(np.float64), level, fam)


def old_planes(W, a, level, fam):
    """the planes of AtrousTransform (wt_decompose3d: the old sequence), a copy"""
    return np.array(W.AtrousTransform(cls_of(W, fam))(a, level).data, copy=True)


def poisoned_plan(W, shape, level, fam):
    """A pooled plan is handed out with the planes of its last owner (release_plan), and the references of this file
    run on the key of the engine call they are compared with: a sample the engine fails to store would keep the
    right answer.  So before every engine call the old sequence transforms an all-NaN cube of the same shape, level
    and family and lets its plan go: the plan the engine is handed next holds NaN in its input, scratch and output
    planes, and a sample that is not stored shows in every assertion."""
    nan = shared(("nan", tuple(shape)), lambda: np.full(shape, np.nan, np.float32))
    c = W.AtrousTransform(cls_of(W, fam))(nan, level)
    plan = c._plan
    del c
    return plan


def engine_transform(W, a, level, fam):
    """transform_cube on the poisoned plan (asserted: the hand-over is what makes the poison count)"""
    plan = poisoned_plan(W, np.shape(a), level, fam)
    c = W.transform_cube(a, level, cls_of(W, fam))
    assert c._plan is plan
    return c


def engine_denoise(W, a, fam, **kw):
    """denoise_cube(a, WEIGHTS) with the plan of its transform poisoned"""
    poisoned_plan(W, np.shape(a), len(WEIGHTS), fam)
    return W.denoise_cube(a, WEIGHTS, cls_of(W, fam), **kw)


def canonical(a):
    """the uint32 view of a float32 array with every NaN mapped to one NaN"""
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    b = np.array(a, copy=True, order="C")
    b[np.isnan(b)] = np.nan
    return b.view(np.uint32)


def assert_same_bytes(got, want, msg=""):
    g, w = canonical(got), canonical(want)
    assert g.shape == w.shape, msg
    bad = int((g != w).sum())
    assert bad == 0, f"{msg}: {bad} of {g.size} samples differ in their bytes"


def outcome(f):
    try:
        return f()
    except Exception as e:                                  # noqa: BLE001 (the class is what is compared)
        return e


def assert_same_outcome(got, want, msg):
    """two results with the same bytes, or two exceptions of the same class"""
    if isinstance(want, Exception) or isinstance(got, Exception):
        assert type(got) is type(want), f"{msg}: {got!r} against {want!r}"
    else:
        assert_same_bytes(got, want, msg)


# =========================================================================== A. planes at the kernel's edges
# (shape, level); B3spline has K = 5 taps, Triangle K = 3; a chunk of a z chain is at least 4 (K - 1) steps
# (tests/test_cubes_oracle_cpu.py derives the layouts named here from the arithmetic of cube_geometry).  SMALL_PLANES was
# set at levels up to 5; it holds at level 6 unchanged: the old sequence lies 1.09e-5 (B3spline) and 9.8e-6 (Triangle)
# from the oracle on the (6, 5, 9) cube, against a bound of 4.74e-5 (the "AtrousTransform planes L6" lines of
# profiles/cubes_oracle_parity_errors.log)
EDGE_CASES = (
    ((6, 5, 9), 6),       # d >= Y > 1 from s = 3: every row class holds ONE row, 7 of a workgroup's 8 rows are masked, and
                          # its 12 x-filtered rows reflect up to 64-fold inside the 5 rows of a slice; d >= Z too
    ((3, 17, 5), 5),      # d >= Z > 1 with d < Y (s = 2, 3, 4): chains of one step, all of whose taps are reflections
    ((2, 3, 261), 5),     # two slices across the 256-column seam: one float4 group and a 1-element tail in the 2nd block
    ((1, 1, 1), 3),       # one sample: every tap of every axis lands on it
    ((2, 2, 2), 4),       # the smallest cube with a neighbour on every axis
    ((16, 9, 12), 2),     # B3spline z chain at s = 0: exactly one chunk of 16 steps (Triangle: 8 + 8)
    ((17, 9, 12), 2),     # 16 + 1: a chunk of a single step that is nothing but warm-up and one output
    ((32, 9, 12), 2),     # 16 + 16
    ((33, 9, 12), 2),     # 16 + 16 + 1
    ((8, 9, 12), 2),      # Triangle (chunks of 8): exactly one chunk
    ((9, 9, 12), 2),      # Triangle: 8 + 1
    ((20, 8, 7), 1),      # a row group of exactly 8 rows
    ((20, 9, 7), 1),      # 8 + 1 rows: the second group masks seven of its rows
    ((20, 16, 7), 1),     # two full row groups
    ((5, 4, 256), 3),     # exactly one x block of 256 columns
    ((5, 4, 257), 3),     # one column into the second block
    ((5, 4, 260), 3),     # one float4 group into the second block
)


@modes
@fams
@pytest.mark.parametrize("shape,level", EDGE_CASES, ids=_case_id)
def test_planes_at_the_kernels_edges(W, O, monkeypatch, shape, level, fam, mode):
    a = cube(shape)
    amax = float(np.abs(a).max())
    ref = shared(("oracle", shape, level, fam), lambda: oracle_planes(O, a, level, fam))
    old = shared(("old", shape, level, fam), lambda: old_planes(W, a, level, fam))
    if mode is None:      # (once per case: the old sequence's own distance from the oracle, for the log)
        measured(f"AtrousTransform planes L{level}", old, ref, SMALL_PLANES * amax)
    use_mode(monkeypatch, mode)
    c = engine_transform(W, a, level, fam)
    assert c.data.shape == (level + 1,) + shape and c.data.dtype == np.float32
    measured(f"planes L{level}", c.data, ref, SMALL_PLANES * amax)
    measured(f"reconstruction L{level}", np.sum(c, axis=0), a, SMALL_RECON * amax)
    assert np.array_equal(c.data, old)


# =========================================================================== B. streaming stores
STREAM_SHAPE, STREAM_LEVEL, BLOCK, INNER = (32, 512, 512), 2, 48, 40


@modes
def test_streaming_stores(W, O, monkeypatch, mode):
    """(32, 512, 512) float32: a plane is exactly 32 MiB, the size from which the kernel stores with streaming stores;
    the z chain of 32 steps runs in two chunks.  Bit for bit against the old sequence, and against the oracle on two
    opposite corner blocks: the filter reaches 2 + 4 = 6 samples at level 2, so the planes of a[:, :48, :48] are those
    of the whole cube on [:, :40, :40] (tests/test_cubes_oracle_cpu.py), true borders and the whole z axis included."""
    fam = "b3spline"
    a = shared(("stream", "input"), lambda: cube(STREAM_SHAPE, 9))
    assert a[0].nbytes * STREAM_SHAPE[0] == 32 << 20
    amax = float(np.abs(a).max())

    def forced0():
        with pytest.MonkeyPatch.context() as m:
            m.setenv("WT_CUBE_FUSED", "0")
            return np.array(engine_transform(W, a, STREAM_LEVEL, fam).data, copy=True)
    old = shared(("stream", "fused0"), forced0)
    use_mode(monkeypatch, mode)
    got = engine_transform(W, a, STREAM_LEVEL, fam).data
    assert got.shape == (STREAM_LEVEL + 1,) + STREAM_SHAPE and got.dtype == np.float32
    assert np.array_equal(got, old)
    lo, hi = slice(None, BLOCK), slice(-BLOCK, None)
    for name, blk, inner in (("first", lo, slice(None, INNER)), ("last", hi, slice(-INNER, None))):
        ref = shared(("stream", name), lambda: oracle_planes(O, a[:, blk, blk], STREAM_LEVEL, fam)[:, :, inner, inner])
        measured(f"streaming planes, {name} corner", got[:, :, inner, inner], ref, SMALL_PLANES * amax)


# =========================================================================== C. values
VALUE_SHAPES = ((9, 11, 13), (5, 4, 261))
VALUE_LEVEL = 3
KINDS = ("nan_corner", "nan_face", "nan_centre", "nan_last", "pinf", "ninf", "all_nan")
NAN_ONLY = ("nan_corner", "nan_face", "nan_centre", "nan_last", "all_nan")
DENOISE_FORMS = ({}, {"soft_threshold": False}, {"noise": 2.5})

value_shapes = pytest.mark.parametrize("shape", VALUE_SHAPES, ids=tag_of)


def bad_sample(shape, kind):
    """(index, value) of the sample of value class `kind`; None for all_nan"""
    Z, Y, X = shape
    if kind == "all_nan":
        return None
    at = {"nan_corner": (0, 0, 0), "nan_face": (0, Y // 2, X // 2), "nan_last": (Z - 1, Y - 1, X - 1)}.get(
        kind, (Z // 2, Y // 2, X // 2))
    return at, {"pinf": np.inf, "ninf": -np.inf}.get(kind, np.nan)


def spoil(a, kind):
    r = a.copy()
    spot = bad_sample(a.shape, kind)
    if spot is None:
        r[...] = np.nan
    else:
        r[spot[0]] = spot[1]
    return r


@modes
@fams
@value_shapes
def test_non_finite_samples(W, O, monkeypatch, shape, fam, mode):
    """transform_cube gives AtrousTransform's bytes and, where the cube holds NaN only, the oracle's NaN mask on every
    plane; denoise_cube gives utils.denoise's bytes, or raises what it raises"""
    cls = cls_of(W, fam)
    clean = cube(shape, 1)
    use_mode(monkeypatch, mode)
    for kind in KINDS:
        a = spoil(clean, kind)
        old = shared(("old", kind, shape, fam), lambda: old_planes(W, a, VALUE_LEVEL, fam))
        got = engine_transform(W, a, VALUE_LEVEL, fam).data
        assert_same_bytes(got, old, f"transform {kind}")
        if kind in NAN_ONLY:
            mask = shared(("mask", kind, shape, fam), lambda: np.isnan(oracle_planes(O, a, VALUE_LEVEL, fam)))
            assert mask.any() and np.array_equal(np.isnan(got), mask), f"NaN mask {kind}"
        for i, kw in enumerate(DENOISE_FORMS):
            want = shared(("den", kind, shape, fam, i), lambda: outcome(lambda: W.denoise(a, WEIGHTS, cls, **kw)))
            assert_same_outcome(outcome(lambda: engine_denoise(W, a, fam, **kw)), want, f"denoise {kind} {kw}")


@modes
@fams
@value_shapes
def test_signed_zeros_and_flat_cubes(W, monkeypatch, shape, fam, mode):
    cls = cls_of(W, fam)
    use_mode(monkeypatch, mode)
    delta = np.zeros(shape, np.float32)
    delta[shape[0] // 2, 1, shape[2] - 2] = -3.0
    for name, a in (("minus zero", np.full(shape, -0.0, np.float32)), ("flat", np.full(shape, 7.25, np.float32)),
                    ("one sample", delta)):
        old = shared(("old", name, shape, fam), lambda: old_planes(W, a, VALUE_LEVEL, fam))
        got = engine_transform(W, a, VALUE_LEVEL, fam).data
        assert_same_bytes(got, old, name)
        if name == "flat":            # dyadic taps that sum to one: every smooth plane is 7.25 exactly
            assert np.all(got[:VALUE_LEVEL] == 0) and np.all(got[VALUE_LEVEL] == np.float32(7.25))
        if name == "minus zero":
            assert np.all(got == 0)
        for i, kw in enumerate(DENOISE_FORMS):
            want = shared(("den", name, shape, fam, i), lambda: outcome(lambda: W.denoise(a, WEIGHTS, cls, **kw)))
            assert_same_outcome(outcome(lambda: engine_denoise(W, a, fam, **kw)), want, f"denoise {name} {kw}")


@modes
@fams
@value_shapes
def test_scaling_by_a_power_of_two_scales_the_results_exactly(W, monkeypatch, shape, fam, mode):
    """the transform and the MAD-thresholded denoise hold only products, quotients and comparisons of scaled quantities:
    while everything stays normal, a * 2^k gives the bits of the result of a, times 2^k.  No reference takes part."""
    cls = cls_of(W, fam)
    a = cube(shape, 2)
    use_mode(monkeypatch, mode)
    t = np.array(engine_transform(W, a, VALUE_LEVEL, fam).data, copy=True)
    d = {soft: engine_denoise(W, a, fam, soft_threshold=soft) for soft in (True, False)}
    for k in (40, -40):
        s = np.float32(2.0) ** k
        assert np.isfinite(s) and s > 0 and np.all(np.isfinite(a * s)) and np.all(np.abs(a * s) > np.finfo(np.float32).tiny)
        assert np.array_equal(engine_transform(W, a * s, VALUE_LEVEL, fam).data, t * s), f"transform k={k}"
        for soft in (True, False):
            assert np.array_equal(engine_denoise(W, a * s, fam, soft_threshold=soft), d[soft] * s), f"denoise k={k} soft={soft}"


@modes
@fams
@value_shapes
def test_denormal_cubes_equal_the_old_sequence(W, monkeypatch, shape, fam, mode):
    """a cube scaled into the float32 denormals (* 2^-140): the planes and denoise_cube against AtrousTransform and
    utils.denoise, same bytes; no oracle is consulted in this range"""
    cls = cls_of(W, fam)
    a = cube(shape, 2) * np.float32(2.0 ** -140)
    assert np.all(a != 0) and np.abs(a).max() < np.finfo(np.float32).tiny
    old = shared(("old", "denormal", shape, fam), lambda: old_planes(W, a, VALUE_LEVEL, fam))
    use_mode(monkeypatch, mode)
    assert_same_bytes(engine_transform(W, a, VALUE_LEVEL, fam).data, old, "transform")
    for soft in (True, False):
        want = shared(("den", "denormal", shape, fam, soft), lambda: outcome(lambda: W.denoise(a, WEIGHTS, cls, soft_threshold=soft)))
        assert_same_outcome(outcome(lambda: engine_denoise(W, a, fam, soft_threshold=soft)), want, f"denoise soft={soft}")


# --------------------------------------------------------------------------- slice isolation
ISOLATION_LEVEL = 5                  # scales s = 0 .. 4: a reach of up to 32 samples on 2 to 5 rows and 4 to 6 slices
# Integer samples in [-8, 8] through taps k / 2^b (b = 4: B3spline, b = 2: Triangle): after L scales a smooth sample is a
# multiple of 2^(-3 b L) of magnitude <= 8 and a detail sample one of magnitude <= 16 - 3 b L + 5 bits, which fit the 24
# of float32 up to the level below.  Up to there every partial sum is exact in any order and the comparison is bit for
# bit; from there to ISOLATION_LEVEL the planes are held to SMALL_PLANES * 8.
EXACT_LEVEL = {"b3spline": 1, "triangle": 3}


def z_filter(O, fam, values, s):
    """the 1-D filter along axis 0 under the symmetric border, float64"""
    taps = O.TAPS[fam]
    hw, Z = len(taps) // 2, values.shape[0]
    out = np.zeros(values.shape, np.float64)
    for j, k in enumerate(taps):
        out += k * values[O.reflect_index(np.arange(Z) + (j - hw) * 2 ** s, Z)]
    return out


def planes_of_product(O, fam, zvalues, img, level):
    """the planes of the cube zvalues[:, None, None] * img[None]: the 3-D filter is separable, so the cube stays the
    product of the z filter of zvalues and the 2-D filter of img at every scale (float64)"""
    zv, im = np.asarray(zvalues, np.float64), np.asarray(img, np.float64)
    out = []
    for s in range(level):
        zn, imn = z_filter(O, fam, zv, s), O.convolution(im, fam, s)
        out.append(zv[:, None, None] * im[None] - zn[:, None, None] * imn[None])
        zv, im = zn, imn
    out.append(zv[:, None, None] * im[None])
    return np.stack(out)


@modes
@fams
def test_one_non_zero_slice_is_the_image_times_the_z_response(W, O, monkeypatch, fam, mode):
    """a cube whose slices are zero but for z0: slice z holds the image's transform times the z response of a delta at
    z0.  Nothing of slice z0 may reach the rows of another slice except through the z filter."""
    for b, f in ((4, "b3spline"), (2, "triangle")):
        assert 3 * b * EXACT_LEVEL[f] + 5 <= 24 < 3 * b * (EXACT_LEVEL[f] + 1) + 5
    cls = cls_of(W, fam)
    rng = np.random.default_rng(26)
    use_mode(monkeypatch, mode)
    for (Z, z0), (Y, X) in (((4, 1), (3, 9)), ((4, 1), (2, 130)), ((5, 4), (5, 7)), ((6, 0), (4, 261))):
        img = rng.integers(-8, 9, (Y, X)).astype(np.float32)
        a = np.zeros((Z, Y, X), np.float32)
        a[z0] = img
        delta = np.zeros(Z)
        delta[z0] = 1
        want = planes_of_product(O, fam, delta, img, EXACT_LEVEL[fam])
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)          # (exact in float32, as reasoned)
        got = engine_transform(W, a, EXACT_LEVEL[fam], fam).data
        np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=f"{(Z, Y, X)} z0={z0}")
        want = planes_of_product(O, fam, delta, img, ISOLATION_LEVEL)
        measured(f"one slice {tag_of((Z, Y, X))} L{ISOLATION_LEVEL}", engine_transform(W, a, ISOLATION_LEVEL, fam).data, want,
                 SMALL_PLANES * 8)


@modes
@fams
@pytest.mark.parametrize("shape", [(6, 3, 130), (3, 2, 9), (5, 5, 261)], ids=tag_of)
def test_constant_slices_reproduce_the_z_filter_of_their_constants(W, O, monkeypatch, shape, fam, mode):
    """Slices that are constant, with a different value each, up to s = 4: the in-slice stages must leave every slice at
    its value, so plane s is the 1-D z transform of the per-slice constants.  A y reflection that leaves its slice
    (period Z*Y instead of Y) mixes the constants and fails here.  Integer constants in [-4, 4]: the in-slice sums of
    a constant are exact, only the z filter adds bits (4 per scale for B3spline: 20 + 4 at level 5), so the planes
    are exact; random constants: within SMALL_PLANES."""
    cls = cls_of(W, fam)
    rng = np.random.default_rng(27)
    one = np.ones((1, 1), np.float64)
    use_mode(monkeypatch, mode)
    ints = rng.integers(-4, 5, shape[0]).astype(np.float32)
    want = planes_of_product(O, fam, ints, one, ISOLATION_LEVEL)[:, :, 0, 0]
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    got = engine_transform(W, np.ascontiguousarray(np.broadcast_to(ints[:, None, None], shape)), ISOLATION_LEVEL, fam).data
    np.testing.assert_array_equal(got, np.broadcast_to(want.astype(np.float32)[:, :, None, None], got.shape))
    consts = rng.standard_normal(shape[0]).astype(np.float32)
    want = planes_of_product(O, fam, consts, one, ISOLATION_LEVEL)[:, :, 0, 0]
    got = engine_transform(W, np.ascontiguousarray(np.broadcast_to(consts[:, None, None], shape)), ISOLATION_LEVEL, fam).data
    measured("constant slices", got, np.broadcast_to(want[:, :, None, None], got.shape), SMALL_PLANES * float(np.abs(consts).max()))


# =========================================================================== D. denoise_cube against the oracle
DENOISE_SHAPES = ((17, 19, 23), (6, 5, 9), (12, 10, 258))
# cube(shape, seed) of tests/test_gpu_cubes.py: the seed among 0 .. 11 whose float64 oracle coefficients keep farthest
# from the hard thresholds of denoise(a, [5, 3]) with the MAD noise estimate; tests/test_cubes_oracle_cpu.py re-derives
# them and asserts a margin above HARD_MARGIN, so no sample may flip
HARD_SEEDS = {((17, 19, 23), "b3spline"): 3, ((17, 19, 23), "triangle"): 11,
              ((6, 5, 9), "b3spline"): 11, ((6, 5, 9), "triangle"): 10,
              ((12, 10, 258), "b3spline"): 11, ((12, 10, 258), "triangle"): 2}
HARD_ALLOW = 0                       # the samples a hard-threshold test may leave out
# denoise(counts, [5, 3], anscombe=True) on Poisson(30) counts, times max|counts|: 4 x the worst error of the
# utils.denoise route against the oracle in profiles/cubes_oracle_parity_errors.log (measured 3.52e-7 on MI355X: log line
# 35, "test_denoise_cube_anscombe[17x19x23-b3spline-rule]  utils.denoise anscombe  1.8287e-05", max|counts| = 52; 1.8e-7
# to 3.3e-7 on the other five cases)
ANSCOMBE32 = 1.4e-6

denoise_shapes = pytest.mark.parametrize("shape", DENOISE_SHAPES, ids=tag_of)


def hard_margin(O, shape, fam, seed):
    """min over the thresholded coefficients of | |w| / tau - 1 | for the float64 oracle's denoise(a, WEIGHTS)"""
    c = O.Coeffs(oracle_planes(O, cube(shape, seed), len(WEIGHTS), fam), fam)
    noise = c.get_noise()
    return min(float(np.abs(np.abs(c.data[s]) / (sig * noise * c.sigma_e[s]) - 1).min()) for s, sig in enumerate(WEIGHTS))


def counts_of(shape):
    return np.random.default_rng(4).poisson(30.0, shape).astype(np.float32)


@modes
@fams
@denoise_shapes
def test_denoise_cube_soft_threshold(W, O, monkeypatch, shape, fam, mode):
    a = cube(shape, HARD_SEEDS[shape, fam])
    use_mode(monkeypatch, mode)
    for noise in (None, 2.5):
        ref = shared(("den", shape, fam, noise), lambda: O.denoise(a.astype(np.float64), WEIGHTS, fam, noise=noise))
        got = engine_denoise(W, a, fam, noise=noise)
        assert got.shape == shape and got.dtype == np.float32
        measured(f"denoise_cube soft noise={noise}", got, ref, DEN32 * float(np.abs(a).max()))


@modes
@fams
@denoise_shapes
def test_denoise_cube_hard_threshold_flips_no_sample(W, O, monkeypatch, shape, fam, mode):
    assert HARD_MARGIN == 1e-4 and HARD_ALLOW == 0
    a = cube(shape, HARD_SEEDS[shape, fam])
    ref = shared(("hard", shape, fam), lambda: O.denoise(a.astype(np.float64), WEIGHTS, fam, soft_threshold=False))
    use_mode(monkeypatch, mode)
    got = engine_denoise(W, a, fam, soft_threshold=False)
    assert got.shape == shape and got.dtype == np.float32
    measured_tol("denoise_cube hard", got, ref, DEN32 * float(np.abs(a).max()), allow=HARD_ALLOW)


@modes
@fams
@denoise_shapes
def test_denoise_cube_anscombe(W, O, monkeypatch, shape, fam, mode):
    counts = counts_of(shape)
    bound = ANSCOMBE32 * float(np.abs(counts).max())
    ref = shared(("ans", shape, fam), lambda: O.denoise(counts.astype(np.float64), WEIGHTS, fam, anscombe=True))
    loop = shared(("ans loop", shape, fam), lambda: W.denoise(counts, WEIGHTS, cls_of(W, fam), anscombe=True))
    if mode is None:      # (once per case: the route the bound is measured on)
        measured("utils.denoise anscombe", loop, ref, bound)
    use_mode(monkeypatch, mode)
    got = engine_denoise(W, counts, fam, anscombe=True)
    assert got.dtype == np.float32 and np.array_equal(got, loop)
    measured("denoise_cube anscombe", got, ref, bound)


# =========================================================================== E. plans and inputs
def test_a_pooled_plan_goes_from_cube_to_cube_to_image(W, O):
    """Pooled plans are keyed (Z*Y, X, family, level): a (4, 6, 70) cube, a (6, 4, 70) cube and a 24 x 70 image take
    the same plan in turn.  Each result against its oracle; the first cube again, bit for bit; and a Coefficients
    object kept from the first call still reads back its own planes."""
    fam, L = "b3spline", 2
    cls = cls_of(W, fam)
    a, b = cube((4, 6, 70), 11), cube((6, 4, 70), 12)
    img = cube((24, 70), 13)

    def check(what, data, x, ref):
        amax = float(np.abs(x).max())
        measured(f"hand-over {what}", data, ref, SMALL_PLANES * amax)
        measured(f"hand-over {what} reconstruction", np.sum(data, axis=0), x, SMALL_RECON * amax)
    kept = engine_transform(W, a, L, fam)                       # holds its plan: the later calls cannot take that one
    c = engine_transform(W, b, L, fam)
    second = np.array(c.data, copy=True)
    plan = c._plan
    del c                                                    # back to the pool
    c = W.AtrousTransform(cls)(img, L)
    assert c._plan is plan                                   # (the hand-over this test is about)
    image = np.array(c.data, copy=True)
    del c
    c = engine_transform(W, a, L, fam)
    assert c._plan is plan and kept._plan is not plan
    last = np.array(c.data, copy=True)
    first = kept.data                                        # read only now, after three other transforms
    check("first cube", first, a, oracle_planes(O, a, L, fam))
    check("second cube", second, b, oracle_planes(O, b, L, fam))
    check("image", image, img, O.atrous_standard(img.astype(np.float64), L, fam))
    check("first cube again", last, a, oracle_planes(O, a, L, fam))
    assert np.array_equal(first, last)
    assert np.array_equal(np.sum(kept, axis=0), np.sum(c, axis=0))


def test_a_plan_closed_in_the_pool_is_not_handed_out(W):
    """A Coefficients object caught in a reference cycle (the traceback of a failed test is one) is collected together
    with its plan: Coefficients.__del__ pools the plan and Plan.__del__ closes it, in either order.  The next call on
    that key used to be handed the closed plan ("wt_plan_set_border: null plan"); it must get a working one."""
    import gc
    fam, L = "triangle", 2
    a = cube((3, 4, 70), 14)
    old = old_planes(W, a, L, fam)
    c = W.transform_cube(a, L, cls_of(W, fam))
    plan = c._plan
    del c                                                    # pooled
    plan.close()                                             # (what the finalizer of a collected plan does)
    c = W.transform_cube(a, L, cls_of(W, fam))
    assert c._plan is not plan and np.array_equal(c.data, old)
    cycle = [c]
    cycle.append(cycle)
    del c, cycle
    gc.collect()                                             # both finalizers, in the collector's order
    assert np.array_equal(W.transform_cube(a, L, cls_of(W, fam)).data, old)


@pytest.mark.parametrize("kind", ("uint8", "float16", "fortran", "strided"))
def test_eligible_inputs_that_are_not_contiguous_float32(W, O, monkeypatch, kind):
    """uint8 and float16 cubes, a Fortran-ordered cube and the view a[:, :, ::2] run on the engine (AtrousTransform and
    denoise made an error inside wavelets_amd.cubes: no silent fallback) and give the bits of AtrousTransform and of
    utils.denoise"""
    from wavelets_amd import cubes as C
    from wavelets_amd.wavelets import _result_dtype
    shape, L = (5, 6, 37), 3
    x = {"uint8": lambda: np.random.default_rng(5).integers(0, 256, shape).astype(np.uint8),
         "float16": lambda: cube(shape, 6).astype(np.float16),
         "fortran": lambda: np.asfortranarray(cube(shape, 7)),
         "strided": lambda: cube(shape[:2] + (2 * shape[2],), 8)[:, :, ::2]}[kind]()
    assert x.shape == shape and (x.dtype != np.float32 or not x.flags.c_contiguous)
    values = np.asarray(x, np.float32)
    amax = float(np.abs(values).max())

    def boom(*args, **kwargs):
        raise AssertionError("wavelets_amd.cubes fell back to the host functions")
    for fam in FAMS:
        cls = cls_of(W, fam)
        assert W.cube_eligible(x, L, cls)
        old = W.AtrousTransform(cls)(x, L).data.copy()
        old_denoised = W.denoise(x, WEIGHTS, cls)
        with monkeypatch.context() as m:
            m.setattr(C, "AtrousTransform", boom)
            m.setattr(C, "denoise", boom)
            got = engine_transform(W, x, L, fam).data
            denoised = engine_denoise(W, x, fam)
        assert got.dtype == _result_dtype(x) == old.dtype and got.shape == (L + 1,) + shape
        assert np.array_equal(got, old)
        measured(f"{kind} planes", got, oracle_planes(O, values, L, fam), SMALL_PLANES * amax)
        assert denoised.dtype == _result_dtype(x) == old_denoised.dtype and np.array_equal(denoised, old_denoised)
        measured(f"{kind} denoise", denoised, O.denoise(values.astype(np.float64), WEIGHTS, fam), DEN32 * amax)
