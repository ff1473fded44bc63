"""wow on (Z, Y, X) cubes through the cube engines (wavelets_amd.cubes.wow_cube over wt_wow_cube_scale /
wt64_wow_cube_scale and wt_cube_wow_kernel<T, K, SMALL_D, PLAIN>) against the float64 numpy oracle,
oracle.atrous_numpy.wow in float64 on the float32 samples (on the float64 samples for the float64 engine), where
tests/test_gpu_wow_cube.py only meets utils.wow on the same GPU (run with -m gpu on an MI355X).

  A  Edge shapes, through Coefficients (the level may exceed wow's own cap for arrays): the march of wt_cube_wow_kernel
     over the squares at a dilation beyond Y or Z (row classes and z chains of one step, 64-fold reflections), chunked
     z chains with a chunk of one step, full and ragged groups of 8 rows, the 256-column workgroup seam with a float4
     group and a one-element tail (float32) and the 128-column seam with a double2 group and an odd tail (float64);
     both tap counts K = 5 and K = 3, SMALL_D (d < 4) and the large-dilation row loads, the PLAIN instantiation.
  B  The twelve options of wow on arrays: the non-PLAIN instantiation (noise map and / or gamma accumulator read and
     written per voxel), hard and soft significance, preserve_variance and weights in the factor; (33, 20, 130) float64
     runs the z chain in 3 chunks at s = 0 and in 2 at s = 1; integer and big-endian inputs on either engine.
  C  Planes of exactly 32 MiB, the size from which cube_geometry_t sets a.nt: wt_storev of the result plane and, with
     h > 0, of the gamma plane with streaming stores, PLAIN and not.
  D  Values: NaN and inf samples, flat cubes and signed zeros (the power <= 0 ? 1e-15 : power clip of wt_wow_point),
     inputs scaled by powers of two up to where the float32 squares of MODE_SMOOTH_SQ underflow and overflow, and one
     non-zero slice in a zero cube.
  E  One pooled plan handed from wow_cube on a cube to wow_cube on a cube of another depth to wow on an image: the
     std::swap(p->coef[plane], p->scratch[3]) that wt_wow_cube_scale leaves behind on the plan.

Every A - D case runs with the per-scale choice left to the host and forced each way (WT_CUBE_FUSED: MODES), and every
engine call of A - D runs on a plan whose planes were just filled with NaN (poisoned: the idea of
tests/test_gpu_cubes_oracle.py::poisoned_plan), asserted to be the plan the engine got.  The oracle's result is
computed once per case (shared).  "Same bytes" is equality of the integer views once every NaN is one canonical NaN:
the signs of zeros count.

Bounds.  No bound comes from wow_cube's own output.
  float32 detail planes: WOW32 = 7.7e-7 times max|reference image|, the bound tests/test_gpu_nd_edges.py::test_wow
  holds wow to, unchanged.  float64 detail planes: F64_WEIGHTED = 1e-12 times the detail planes' own max|reference|.
  Which planes: the plane_ulps premise, decided by the reference alone.  Every scale adds half an ulp of max|input| in
  each of its three filter stages, so w_s = c_s - c_{s+1} is off by up to plane_ulps(s) = 3 s + 1.5 ulp; whitening
  divides it by its local rms, so the whitened plane is off by plane_ulps(s) ulp / rms(w_s) of its size.  Plane s
  meets the oracle where that, times max|reference plane s|, stays within the bound, with the oracle's rms(w_s); the
  other planes - on the pedestal of these cubes (50 + 3 N(0, 1)) the scales from 2 on in float32, and the scales
  whose planes are flat to rounding on cubes of a few samples - are held to the old route's bytes.  The deep float32 cases run in float64 too (DEEP_CASES), where the premise admits more scales.
  The last plane and the image.  wow divides the last plane by its np.std (ref utils.py:186).  STD_PREMISE is the
  premise the reference alone decides: r = variance / mean square of the oracle's last plane of at least 1e-6 in
  float32 (a spread of 1e-3 of the pedestal, 1.7e4 ulp) and 1e-7 in float64.  Below it (levels 4 - 6 on cubes of a few
  samples, flat cubes) the two are held to the old route's bytes only, and so are the float32 detail planes, whose
  bound is the image's.  float32: LAST32 and IMAGE32 times the array's own max|reference|, 4 x the worst figure of the
  old route (utils.wow under WT_CUBE_FUSED=0) in profiles/wow_cube_oracle_parity_errors.log, quoted at the constants.
  float64: the engine takes the std from the plane's {sum, sum of squares}, off by 3 u / r relative (u = 2^-53;
  wavelets_amd/utils.py at _STD_CANCELS): F64_WEIGHTED + 3 u / r with the oracle's r, a law and no measurement.
  inf samples in float64.  wt_rsq64(inf) is NaN where the reference's c / sqrt(inf) is 0: the float64 engine's NaN mask
  holds the oracle's and stays inside the reach of the sample (test_non_finite_samples).
The log holds, per case and class, the worst "utils.wow" line over the two families and the forms of the call, as
conftest.measured writes them from this file (test id, what, error, bound); "not held" lines carry what the premises
leave out, with no bound: the figures of DESIGN.md section 3.23.

tests/test_wow_cube_oracle_cpu.py holds, without a device, what this file rests on: the chunk layouts of A, the
hard-threshold margin of B, the NaN reach of D, the block rule of C and the normal range of the scalings of D.
"""
import numpy as np
import pytest

from conftest import measured, measured_tol
from test_gpu_nd_edges import F64_WEIGHTED, HARD_MARGIN, WOW32
from test_gpu_cubes_oracle import (EDGE_CASES, FAMS, HW, KINDS, MODES, VALUE_SHAPES, assert_same_bytes, bad_sample,
                                   canonical, cls_of, poisoned_plan, shared, spoil, tag_of, use_mode)
from test_gpu_wow_cube import OPTION_SHAPES, OPTIONS, cube, options

pytestmark = pytest.mark.gpu

modes = pytest.mark.parametrize("mode", MODES, ids=lambda m: "rule" if m is None else "fused" + m)
fams = pytest.mark.parametrize("fam", FAMS)
dtypes = pytest.mark.parametrize("dtype", ("float32", "float64"))

SCOPE = "wt_cube_wow_kernel"
DENOISE = dict(denoise_coefficients=[5, 2], noise=2.5)

# --------------------------------------------------------------------------- bounds (see the header)
# the last plane and the image, float32, times the array's own max|reference|: 4 x the worst figure of the old route
# among the cases STD_PREMISE admits (profiles/wow_cube_oracle_parity_errors.log, quoted below)
# (log line 42: test_edge_shapes_through_coefficients[5x4x256-3-float32-b3spline-rule]  utils.wow denoise float32 last
#  plane L3 r=7.7e-06  5.6511e-04, over max|reference| = 364.1: 1.552e-06)
LAST32 = 6.2e-6
# (log line 43: the same case, utils.wow denoise float32 image L3 r=7.7e-06  6.4819e-04, over 368.5: 1.759e-06)
IMAGE32 = 7.1e-6
DETAIL64 = F64_WEIGHTED               # times the detail planes' own max|reference|
LAST64 = F64_WEIGHTED                 # plus 3 u / r (against_oracle)
IMAGE64 = F64_WEIGHTED
assert WOW32 == 7.7e-7 and F64_WEIGHTED == 1e-12
STD_PREMISE = {"float32": 1e-6, "float64": 1e-7}


def plane_ulps(s):
    """the rounding of w_s = c_s - c_{s+1} in ulp of max|input|, at worst: every scale adds half an ulp in each of its
    three filter stages (taps that sum to one pass the error of their input on, no larger), so c_s carries 1.5 s ulp,
    c_{s+1} 1.5 (s + 1), and the difference of two neighbours is exact"""
    return 3 * s + 1.5


U64 = 2.0 ** -53
BOUNDS = {"float32": (LAST32, IMAGE32), "float64": (LAST64, IMAGE64)}


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


def fresh(kw):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}


def engine_of(dtype):
    """the element type of the engine that serves an input of `dtype` (ref wavelets.py:297,319-320)"""
    return "float32" if np.dtype(dtype) in (np.dtype("float32"), np.dtype("uint8"), np.dtype("float16")) else "float64"


def absmax(a):
    a = np.asarray(a)
    return float(np.abs(a).max()) if a.size else 0.0


def spread(plane):
    """r = variance / mean square of a plane, float64 (0 for a plane of zeros)"""
    p = np.asarray(plane, np.float64)
    ms = float(np.mean(p * p))
    return float(np.var(p)) / ms if ms > 0 else 0.0


# --------------------------------------------------------------------------- the three routes
def oracle_wow(O, a, fam, level=None, noise=None, **kw):
    """(image, planes, info) of oracle.atrous_numpy.wow in float64 on the samples of `a`, through Coeffs of `level` (wow
    takes the noise of a Coeffs object from the object, ref utils.py:148-151).  info: the rms of every detail plane
    before the update and the ulp of max|input| in the engine's element type, for plane_ulps."""
    x = np.asarray(a).astype(np.float64)
    if isinstance(noise, np.ndarray):
        noise = noise.astype(np.float64)
    if level is None:     # (wow's own rule, then the same two steps: ref utils.py:121-151)
        level = O.wow_n_scales(x.shape, fam, kw.get("n_scales"), kw.get("h", 0), kw.get("denoise_coefficients", []), None)
    c = O.Coeffs(O.atrous_standard_nd(x, level, fam), fam)
    c.noise = noise
    ulp = float(np.spacing(np.asarray(absmax(x), engine_of(np.asarray(a).dtype))))
    info = {"rms": [float(np.sqrt(np.mean(w * w))) for w in c.data[:level]], "ulp": ulp}
    kw = {k: v for k, v in fresh(kw).items() if k != "n_scales"}
    r, c = O.wow(c, **kw)
    out = (np.array(r, copy=True), np.array(c.data, copy=True))
    for v in out:
        v.setflags(write=False)
    return out + (info,)


def old_wow(W, a, fam, level=None, noise=None, **kw):
    """(image, planes) of utils.wow - on the array, or on AtrousTransform's Coefficients of `level` - with the old
    sequences forced: the route wow_cube replaces, and the one the bounds are measured on"""
    with pytest.MonkeyPatch.context() as m:
        m.setenv("WT_CUBE_FUSED", "0")
        if level is None:
            r, c = W.wow(a, cls_of(W, fam), noise=noise, **fresh(kw))
        else:
            c = W.AtrousTransform(cls_of(W, fam))(a, level)
            c.noise = noise
            r, c = W.wow(c, **fresh(kw))
        out = (np.array(r, copy=True), np.array(c.data, copy=True))
    for v in out:
        v.setflags(write=False)
    return out


def poisoned(W, shape, level, fam, engine):
    """poisoned_plan of tests/test_gpu_cubes_oracle.py for either engine: the old route transforms an all-NaN cube of the
    same shape, level and family and lets its plan go, so the plan the engine is handed next holds NaN in its input and
    coefficient planes and in the scratch planes the old transform went through"""
    if engine == "float32":
        return poisoned_plan(W, shape, level, fam)
    nan = shared(("nan64", tuple(shape)), lambda: np.full(shape, np.nan, np.float64))
    c = W.AtrousTransform(cls_of(W, fam))(nan, level)
    plan = c._plan
    del c
    return plan


def engine_wow(W, a, fam, level, noise=None, **kw):
    """transform_cube(a, level), then wow_cube on its Coefficients, on the poisoned plan (asserted).  wow ignores its
    noise keyword for a Coefficients object (ref utils.py:148-151), so the noise is given on the object as well."""
    plan = poisoned(W, np.shape(a), level, fam, engine_of(np.asarray(a).dtype))
    c = W.transform_cube(a, level, cls_of(W, fam))
    assert c._plan is plan
    c.noise = noise
    image, out = W.wow_cube(c, noise=noise, **fresh(kw))
    assert out is c and c._plan is plan
    return image, c.data


def engine_wow_array(W, O, a, fam, noise=None, **kw):
    """wow_cube on the array itself, on the poisoned plan of the level wow's own rule gives (asserted)"""
    level = O.wow_n_scales(np.shape(a), fam, kw.get("n_scales"), kw.get("h", 0), kw.get("denoise_coefficients", []), None)
    plan = poisoned(W, np.shape(a), level, fam, engine_of(np.asarray(a).dtype))
    image, c = W.wow_cube(a, cls_of(W, fam), noise=noise, **fresh(kw))
    assert c._plan is plan and len(c) == level + 1
    return image, c.data


def wide(a):
    """the integer view of a float32 / float64 array with every NaN mapped to one NaN"""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return canonical(a)
    assert a.dtype == np.float64, a.dtype
    b = np.array(a, copy=True, order="C")
    b[np.isnan(b)] = np.nan
    return b.view(np.uint64)


def assert_same(got, want, msg=""):
    """assert_same_bytes of tests/test_gpu_cubes_oracle.py, for float64 arrays too; the dtypes must agree"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{msg}: {got.dtype} against {want.dtype}"
    if got.dtype == np.float32:
        return assert_same_bytes(got, want, msg)
    g, w = wide(got), wide(want)
    assert g.shape == w.shape, msg
    bad = int((g != w).sum())
    assert bad == 0, f"{msg}: {bad} of {g.size} samples differ in their bytes"


def assert_same_result(got, want, msg):
    assert_same(got[0], want[0], msg + " image")
    assert_same(got[1], want[1], msg + " planes")


def detail_terms(ref, dtype):
    """(the detail planes that meet the oracle, their absolute bound): the header's plane_ulps premise"""
    ri, rd, info = ref
    L = len(rd) - 1
    if dtype == "float64":
        bound = DETAIL64 * absmax(rd[:L])
    else:
        bound = WOW32 * (absmax(ri) if spread(rd[L]) >= STD_PREMISE[dtype] else absmax(rd[:L]))
    held = [s for s in range(L)
            if info["rms"][s] > 0 and plane_ulps(s) * info["ulp"] / info["rms"][s] * absmax(rd[s]) <= bound]
    return held, bound


def against_oracle(what, got, ref, dtype, detail=True, log_rest=False):
    """The detail planes plane_ulps admits, together, against the oracle's; the last plane and the image under
    STD_PREMISE (the header).  log_rest (the old route, once per case): what the premises leave out goes to the log with
    no bound, so that the figures of DESIGN.md section 3.23 can be read from it."""
    (image, data), (ri, rd, _) = got, ref
    L = len(rd) - 1
    assert data.shape == rd.shape and image.shape == ri.shape
    assert data.dtype == np.dtype(dtype) and image.dtype == np.dtype(dtype)
    held, bound = detail_terms(ref, dtype)
    rest = [s for s in range(L) if s not in held]
    if detail and held:
        measured(f"{what} detail planes {held} of L{L}", data[held], rd[held], bound)
    if log_rest and rest:
        measured(f"{what} detail planes {rest} of L{L}, not held", data[rest], rd[rest], np.inf)
    r = spread(rd[L])             # (of the oracle's last plane; whitened or not, r is scale-free)
    if r >= STD_PREMISE[dtype]:
        last, img = BOUNDS[dtype]
        one_pass = 3 * U64 / r if dtype == "float64" else 0.0
        measured(f"{what} last plane L{L} r={r:.1e}", data[L], rd[L], (last + one_pass) * absmax(rd[L]))
        measured(f"{what} image L{L} r={r:.1e}", image, ri, (img + one_pass) * absmax(ri))
    elif log_rest:
        measured(f"{what} last plane L{L} r={r:.1e}, not held", data[L], rd[L], np.inf)


def kernel_calls(W, run):
    """launches of wt_cube_wow_kernel recorded while run() runs"""
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    ctx.profile(True)
    try:
        ctx.profile_reset()
        out = run()
        return out, ctx.profile_entries().get(SCOPE, (0, 0.0))[0]
    finally:
        ctx.profile(False)
        ctx.profile_reset()


# =========================================================================== A. edge shapes, through Coefficients
# the float32 shapes are EDGE_CASES of tests/test_gpu_cubes_oracle.py (its comments name what each one reaches); the
# float64 ones are their counterparts at the 128-column seam of the double2 groups: exactly one x block, one column and
# one double2 group into the second, a double2 group and a one-element tail, and two slices with a 3-column second block
EDGE_CASES64 = (((5, 4, 128), 3), ((5, 4, 129), 3), ((5, 4, 130), 3), ((2, 3, 131), 5))
# the float32 cases whose deep scales fall to plane_ulps in float32 run in float64 too
DEEP_CASES = (((6, 5, 9), 6), ((3, 17, 5), 5), ((2, 3, 261), 5), ((2, 2, 2), 4))
A_CASES = (tuple((s, l, "float32") for s, l in EDGE_CASES)
           + tuple((s, l, "float64") for s, l in EDGE_CASES64 + DEEP_CASES))
A_FORMS = (("denoise", DENOISE), ("defaults", {}))


@modes
@fams
@pytest.mark.parametrize("shape,level,dtype", A_CASES, ids=lambda v: tag_of(v) if isinstance(v, tuple) else str(v))
def test_edge_shapes_through_coefficients(W, O, monkeypatch, shape, level, dtype, fam, mode):
    a = cube(shape, dtype)
    for name, kw in A_FORMS:
        ref = shared(("A", shape, level, dtype, fam, name), lambda: oracle_wow(O, a, fam, level, **kw))
        old = shared(("A old", shape, level, dtype, fam, name), lambda: old_wow(W, a, fam, level, **kw))
        if mode is None:      # (once per case: the old route's own distance from the oracle, for the log)
            against_oracle(f"utils.wow {name} {dtype}", old, ref, dtype, log_rest=True)
        with monkeypatch.context() as m:
            use_mode(m, mode)
            got = engine_wow(W, a, fam, level, **kw)
        assert got[0].shape == shape and got[1].shape == (level + 1,) + shape
        against_oracle(f"wow_cube {name} {dtype}", got, ref, dtype)
        assert_same_result(got, old, name)


@pytest.mark.parametrize("shape,level,dtype", (((5, 4, 257), 3, "float32"), ((5, 4, 129), 3, "float64")),
                         ids=lambda v: tag_of(v) if isinstance(v, tuple) else str(v))
def test_section_a_runs_the_wow_kernel(W, monkeypatch, shape, level, dtype):
    """with the fused kernels forced every detail scale of an A case is one launch of wt_cube_wow_kernel: without it a
    silent fallback would make the comparison with the old route trivially true"""
    monkeypatch.setenv("WT_CUBE_FUSED", "1")
    _, calls = kernel_calls(W, lambda: engine_wow(W, cube(shape, dtype), "b3spline", level, **DENOISE))
    assert calls == level


# =========================================================================== B. options on arrays
B_SEED = 3                # cube(shape, dtype, 3), the input of tests/test_gpu_wow_cube.py::test_options_on_arrays
# the hard option: the first seed of cube(shape, dtype, seed) at which no float64 oracle coefficient of either element
# type lies within HARD_MARGIN of its threshold 5 | 2 x 2.5 x sigma_e[s].  Seed 3 leaves 3.7e-5 on (17, 19, 23); of the
# seeds 0 .. 63, 62 keeps farthest (9.6e-4).  On (33, 20, 130), 85800 samples with the second threshold at 1.7 standard
# deviations of its plane, no seed of 0 .. 63 holds (7.4e-5 at best, seed 20): the seeds were tried in order from 64 on, and 485 is the
# first that holds (1.7e-4).  tests/test_wow_cube_oracle_cpu.py asserts the margins.
HARD_SEEDS = {(17, 19, 23): 62, (33, 20, 130): 485}


def b_input(shape, dtype):
    return cube(shape, dtype, B_SEED)


def hard_margin(O, shape, dtype, seed):
    """min over the thresholded coefficients of | |w| / tau - 1 | for the float64 oracle's wow(a, **OPTIONS["hard"])"""
    kw = OPTIONS["hard"]
    planes = O.atrous_standard_3d(cube(shape, dtype, seed).astype(np.float64), len(kw["denoise_coefficients"]), "b3spline")
    se = O.sigma_e("b3spline", None, 3)
    return min(float(np.abs(np.abs(planes[s]) / (sig * kw["noise"] * se[s]) - 1).min())
               for s, sig in enumerate(kw["denoise_coefficients"]))


@modes
@dtypes
@pytest.mark.parametrize("name", sorted(set(OPTIONS) - {"estimated_noise", "hard"}))
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=tag_of)
def test_options_on_arrays(W, O, monkeypatch, shape, name, dtype, mode):
    a = b_input(shape, dtype)
    kw = options(name, shape, dtype)
    ref = shared(("B", shape, name, dtype), lambda: oracle_wow(O, a, "b3spline", **kw))
    old = shared(("B old", shape, name, dtype), lambda: old_wow(W, a, "b3spline", **kw))
    if mode is None:
        against_oracle(f"utils.wow {name} {dtype}", old, ref, dtype)
    use_mode(monkeypatch, mode)
    got = engine_wow_array(W, O, a, "b3spline", **kw)
    against_oracle(f"wow_cube {name} {dtype}", got, ref, dtype)
    assert_same_result(got, old, name)


@modes
@dtypes
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=tag_of)
def test_hard_threshold_flips_no_sample(W, O, monkeypatch, shape, dtype, mode):
    """soft_threshold=False with the noise given: tests/test_wow_cube_oracle_cpu.py asserts that no float64 coefficient
    of the oracle lies within HARD_MARGIN of its threshold, so no sample may flip and none is allowed to"""
    assert HARD_MARGIN == 1e-4
    a = cube(shape, dtype, HARD_SEEDS[shape])
    kw = options("hard", shape, dtype)
    ref = shared(("B", shape, "hard", dtype), lambda: oracle_wow(O, a, "b3spline", **kw))
    old = shared(("B old", shape, "hard", dtype), lambda: old_wow(W, a, "b3spline", **kw))
    use_mode(monkeypatch, mode)
    got = engine_wow_array(W, O, a, "b3spline", **kw)
    held, bound = detail_terms(ref, dtype)
    assert held == [0, 1]                   # (both thresholded planes)
    measured_tol(f"wow_cube hard {dtype} detail planes", got[1][held], ref[1][held], bound, allow=0)
    against_oracle(f"wow_cube hard {dtype}", got, ref, dtype, detail=False)
    assert_same_result(got, old, "hard")


@modes
@dtypes
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=tag_of)
def test_estimated_noise(W, O, monkeypatch, shape, dtype, mode):
    """denoise_coefficients=[5, 2] without a noise: wow takes the MAD estimate from plane 0 as the device holds it
    (float32 on the float32 engine).  The median is 1-Lipschitz in the sup norm, so the estimate lies within the bound
    of plane 0 over 0.6745 sigma_e[0] of the oracle's (tests/test_gpu_nd_edges.py::test_noise_estimate), and every
    threshold sigma * noise * sigma_e[s] moves by that relative amount - up to 1e-6 relative in float32, more than the
    bound on a whitened coefficient allows for a coefficient near its threshold.  So: (1) the call as it stands gives
    the old route's bytes and an estimate within that bound of the oracle's; (2) the values are compared with the
    oracle on a second call that is GIVEN the oracle's own estimate as its noise - a premise the reference alone
    sets."""
    from conftest import SMALL_PLANES
    from test_gpu_nd_edges import F64_PLANES
    a = b_input(shape, dtype)
    kw = options("estimated_noise", shape, dtype)
    level = O.wow_n_scales(shape, "b3spline", None, 0, kw["denoise_coefficients"], None)
    planes = shared(("B planes", shape, dtype), lambda: O.atrous_standard_3d(a.astype(np.float64), level, "b3spline"))
    noise = float(O.Coeffs(planes, "b3spline").get_noise())
    ref = shared(("B", shape, "estimated", dtype), lambda: oracle_wow(O, a, "b3spline", **kw))
    old = shared(("B old", shape, "estimated", dtype), lambda: old_wow(W, a, "b3spline", **kw))
    use_mode(monkeypatch, mode)
    plan = poisoned(W, shape, level, "b3spline", dtype)
    image, c = W.wow_cube(a, **fresh(kw))
    assert c._plan is plan
    assert_same_result((image, c.data), old, "estimated noise")
    plane_bound = (SMALL_PLANES if dtype == "float32" else F64_PLANES) * absmax(a)
    measured(f"wow_cube MAD estimate {dtype}", c.noise, noise, plane_bound / 0.6745 / float(O.sigma_e("b3spline", None, 3)[0]))
    got = engine_wow_array(W, O, a, "b3spline", noise=noise, **kw)
    against_oracle(f"wow_cube given the oracle's estimate {dtype}", got, ref, dtype)


@modes
@pytest.mark.parametrize("dt", ("int16", "uint8", ">f4"))
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=tag_of)
def test_integer_and_big_endian_inputs(W, O, monkeypatch, shape, dt, mode):
    """the inputs of tests/test_gpu_wow_cube.py::test_integer_and_big_endian_inputs; the oracle gets the values as
    float64 and the noise is given (the MAD estimate is the matter of test_estimated_noise)"""
    a = np.random.default_rng(1).integers(0, 200, shape).astype(dt) if np.dtype(dt).kind in "iu" else cube(shape, dt, 1)
    engine = engine_of(dt)
    ref = shared(("B", shape, dt), lambda: oracle_wow(O, a, "triangle", **DENOISE))
    old = shared(("B old", shape, dt), lambda: old_wow(W, a, "triangle", **DENOISE))
    if mode is None:
        against_oracle(f"utils.wow {dt}", old, ref, engine)
    use_mode(monkeypatch, mode)
    got = engine_wow_array(W, O, a, "triangle", **DENOISE)
    against_oracle(f"wow_cube {dt}", got, ref, engine)
    assert_same_result(got, old, dt)


# =========================================================================== C. streaming stores
STREAM_SHAPES = {"float32": (32, 512, 512), "float64": (16, 512, 512)}
STREAM_LEVEL, BLOCK = 2, 48
# a detail plane w_s of the transform reaches HW (2^(s+1) - 1) samples and the power of scale s HW 2^s more: at level 2
# the last detail plane reaches 6 + 4 = 10 samples (B3spline), so the updated detail planes of a[:, :48, :48] are those
# of the whole cube on [:, :38, :38] (tests/test_wow_cube_oracle_cpu.py: exact there, and not one sample further)
INNER = BLOCK - HW["b3spline"] * (2 ** STREAM_LEVEL - 1) - HW["b3spline"] * 2 ** (STREAM_LEVEL - 1)
STREAM_FORMS = ("plain", "map_gamma")


def stream_input(dtype):
    return shared(("stream", dtype), lambda: cube(STREAM_SHAPES[dtype], dtype, 9))


def stream_noise(dtype):
    return shared(("stream map", dtype),
                  lambda: (np.random.default_rng(9).random(STREAM_SHAPES[dtype]) + 0.5).astype(dtype) * 2)


def stream_form(form, dtype, block=None):
    """(noise, keywords) of a form of C; block: the noise map cut to a[:, block, block].  With the gamma bounds given,
    nothing global enters the detail planes."""
    if form == "plain":
        return 2.5, dict(denoise_coefficients=[5, 2])
    noise = stream_noise(dtype)
    return (noise if block is None else np.ascontiguousarray(noise[:, block, block]),
            dict(denoise_coefficients=[5, 2], h=0.5, gamma_min=30.0, gamma_max=70.0))


@modes
@dtypes
@pytest.mark.parametrize("form", STREAM_FORMS)
def test_streaming_stores(W, O, monkeypatch, form, dtype, mode):
    """Planes of exactly 32 MiB: the result plane and, in map_gamma, the gamma plane are stored with streaming stores.
    The whole result has the bytes of the run with the old sequences forced; the detail planes meet the oracle on two
    opposite corner blocks (the last plane and the image depend on np.std of the whole smooth plane)."""
    fam = "b3spline"
    a = stream_input(dtype)
    assert INNER == 38 and a[0].nbytes * a.shape[0] == 32 << 20
    noise, kw = stream_form(form, dtype)

    def forced0():
        with pytest.MonkeyPatch.context() as m:
            m.setenv("WT_CUBE_FUSED", "0")
            image, data = engine_wow(W, a, fam, STREAM_LEVEL, noise, **kw)
            return np.array(image, copy=True), np.array(data, copy=True)
    old = shared(("stream fused0", form, dtype), forced0)
    use_mode(monkeypatch, mode)
    got, calls = kernel_calls(W, lambda: engine_wow(W, a, fam, STREAM_LEVEL, noise, **kw))
    if mode == "1":
        assert calls == STREAM_LEVEL
    assert got[0].shape == a.shape and got[1].shape == (STREAM_LEVEL + 1,) + a.shape
    assert got[0].dtype == got[1].dtype == np.dtype(dtype)
    assert_same_result(got, old, form)
    for name, blk, inner in (("first", slice(None, BLOCK), slice(None, INNER)),
                             ("last", slice(-BLOCK, None), slice(-INNER, None))):
        def block():          # (planes, the scales held, bound: detail_terms on the block's own wow, image included)
            bn, bkw = stream_form(form, dtype, blk)
            ref = oracle_wow(O, a[:, blk, blk], fam, STREAM_LEVEL, bn, **bkw)
            return (ref[1][:, :, inner, inner],) + detail_terms(ref, dtype)
        ref, held, bound = shared(("stream", form, dtype, name), block)
        assert held in ([0, 1], [0])          # ([0]: float32 with h = 0.5, which halves the image and so the bound)
        measured(f"wow_cube streaming {form} {dtype} detail planes, {name} corner", got[1][held][:, :, inner, inner],
                 ref[held], bound)


# =========================================================================== D. values
VALUE_LEVEL = 3
value_shapes = pytest.mark.parametrize("shape", VALUE_SHAPES, ids=tag_of)


def dilate(cur, hw, d):
    """the samples of an axis that a tap at distance j d, |j| <= hw, brings a marked sample to, under np.pad's symmetric
    border (no index arithmetic shared with the oracle)"""
    n = cur.shape[0]
    padded = np.pad(cur, hw * d, mode="symmetric")
    out = np.zeros(n, bool)
    for j in range(2 * hw + 1):
        out |= padded[j * d:j * d + n]
    return out


def wow_reach_masks(shape, at, hw, level):
    """NaN masks of the `level` updated detail planes of wow for a NaN sample at `at`: w_s is NaN where c_{s+1} is (the
    transform's reach, a product of its three axes), and the update divides by the root of conv_s(w_s^2), which is NaN
    hw 2^s further on every axis"""
    planes = []
    axes = [np.zeros(n, bool) for n in shape]
    for cur, i in zip(axes, at):
        cur[i] = True
    for s in range(level):
        axes = [dilate(cur, hw, 2 ** s) for cur in axes]                    # c_{s+1}, so w_s
        z, y, x = (dilate(cur, hw, 2 ** s) for cur in axes)                 # the local power of w_s
        planes.append(z[:, None, None] & y[None, :, None] & x[None, None, :])
    return np.stack(planes)


@modes
@fams
@dtypes
@value_shapes
def test_non_finite_samples(W, O, monkeypatch, shape, dtype, fam, mode):
    """a NaN, +inf or -inf sample at the positions of KINDS: neither route raises, wow_cube gives utils.wow's bytes
    (the last plane and the image are NaN throughout: np.std of a plane that holds one), and the NaN mask of every
    detail plane is the oracle's - the transform's reach plus HW 2^s for the power (tests/test_wow_cube_oracle_cpu.py);
    in float64 with an inf sample it holds the oracle's and stays inside that reach (the header)"""
    clean = cube(shape, dtype, 1)
    use_mode(monkeypatch, mode)
    for kind in KINDS:
        a = spoil(clean, kind)
        old = shared(("D old", kind, shape, dtype, fam), lambda: old_wow(W, a, fam, VALUE_LEVEL))
        mask = shared(("D mask", kind, shape, dtype, fam),
                      lambda: np.isnan(oracle_wow(O, a, fam, VALUE_LEVEL)[1][:VALUE_LEVEL]))
        got = engine_wow(W, a, fam, VALUE_LEVEL)
        assert_same_result(got, old, kind)
        nan = np.isnan(got[1][:VALUE_LEVEL])
        if dtype == "float64" and kind in ("pinf", "ninf"):      # (wt_rsq64(inf) is NaN, c / sqrt(inf) is 0: the header)
            reach = wow_reach_masks(shape, bad_sample(shape, kind)[0], HW[fam], VALUE_LEVEL)
            assert mask.any() and not (mask & ~nan).any() and not (nan & ~reach).any(), f"NaN mask {kind}"
        else:
            assert mask.any() and np.array_equal(nan, mask), f"NaN mask {kind}"


@modes
@fams
@dtypes
@value_shapes
def test_flat_cubes_and_signed_zeros(W, monkeypatch, shape, dtype, fam, mode):
    """A flat cube at 50, at 0 and at -0.0: every detail plane is zero, its power is zero and wt_wow_point clips it to
    1e-15 (power <= 0), so the updated detail planes are zeros - with the signs the old route leaves - and nothing is
    NaN.  The last plane and the image are held to the old route's bytes only: on a flat cube the oracle divides by
    1e-15 (the image of a flat 50 is 5e16), and a device std that is a rounding error away from zero changes the result
    by orders of magnitude - an exact std of zero is a premise only the reference satisfies, so the oracle is no
    reference for that plane."""
    use_mode(monkeypatch, mode)
    for name, value in (("flat 50", 50.0), ("flat 0", 0.0), ("flat -0", -0.0)):
        a = np.full(shape, value, dtype)
        old = shared(("D old", name, shape, dtype, fam), lambda: old_wow(W, a, fam, VALUE_LEVEL))
        got = engine_wow(W, a, fam, VALUE_LEVEL)
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any(), name
        assert np.all(got[1][:VALUE_LEVEL] == 0), name
        assert_same_result(got, old, name)


SCALINGS = (20, -20, 40, -40)


@modes
@fams
@dtypes
@value_shapes
def test_scaling_by_a_power_of_two(W, O, monkeypatch, shape, dtype, fam, mode):
    """a * 2^k, k = +-20 and +-40, no denoising: the whitened planes are scale-free, and the float32 squares stay
    normal (tests/test_wow_cube_oracle_cpu.py asserts it on the oracle's planes).  Against the oracle of the scaled
    input under the bounds of every other case, and the bytes of utils.wow."""
    base = cube(shape, dtype, 2)
    use_mode(monkeypatch, mode)
    for k in SCALINGS:
        a = base * np.dtype(dtype).type(2.0 ** k)
        assert np.all(np.isfinite(a)) and a.dtype == np.dtype(dtype)
        ref = shared(("D scaled", k, shape, dtype, fam), lambda: oracle_wow(O, a, fam, VALUE_LEVEL))
        old = shared(("D scaled old", k, shape, dtype, fam), lambda: old_wow(W, a, fam, VALUE_LEVEL))
        if mode is None:
            against_oracle(f"utils.wow 2^{k} {dtype}", old, ref, dtype)
        got = engine_wow(W, a, fam, VALUE_LEVEL)
        against_oracle(f"wow_cube 2^{k} {dtype}", got, ref, dtype)
        assert_same_result(got, old, f"2^{k}")


@modes
@fams
@value_shapes
def test_float32_squares_that_underflow_and_overflow(W, monkeypatch, shape, fam, mode):
    """a * 2^-70 and a * 2^62 in float32: the squares of the detail coefficients (MODE_SMOOTH_SQ rounds v * v once in
    float32, as wt_binary(MUL) stores it) are denormals of a few bits (or zero) or exceed its maximum, so the local power
    has lost its bits, is 0 (clipped to 1e-15) or is inf.  The float64 oracle squares in float64, where neither happens, and returns the
    scale-free planes: it describes another arithmetic there and is not the reference.  The old route is: same bytes,
    and neither route raises."""
    base = cube(shape, "float32", 2)
    use_mode(monkeypatch, mode)
    for k in (-70, 62):
        a = base * np.float32(2.0 ** k)
        assert np.all(np.isfinite(a)) and np.all(a != 0)
        old = shared(("D range old", k, shape, fam), lambda: old_wow(W, a, fam, VALUE_LEVEL))
        assert_same_result(engine_wow(W, a, fam, VALUE_LEVEL), old, f"2^{k}")


ISOLATION_SHAPES = ((16, 5, 9), (16, 3, 261))
ISOLATION_LEVEL, Z0 = 2, 2


@modes
@fams
@dtypes
@pytest.mark.parametrize("shape", ISOLATION_SHAPES, ids=tag_of)
def test_one_non_zero_slice_on_a_pedestal(W, O, monkeypatch, shape, dtype, fam, mode):
    """a zero cube with one slice of the pedestal cube (50 + noise) at z0 = 2, level 2.  With whitening off the planes
    and the image are zero, exactly, in every slice further from z0 than the z reach of the transform, HW (2^2 - 1);
    with it on, the detail plane of scale s is zero further than HW (2^(s+1) - 1) + HW 2^s: the power of a zero
    neighbourhood is zero and is clipped, not divided by.  (The symmetric border never brings a sample nearer: -k
    reflects to k - 1.)  Both against the oracle, and the bytes of utils.wow."""
    a = np.zeros(shape, dtype)
    a[Z0] = cube(shape[1:], dtype, 4)
    hw = HW[fam]
    use_mode(monkeypatch, mode)
    for whitening in (False, True):
        kw = dict(whitening=whitening)
        ref = shared(("D slice", shape, dtype, fam, whitening), lambda: oracle_wow(O, a, fam, ISOLATION_LEVEL, **kw))
        old = shared(("D slice old", shape, dtype, fam, whitening), lambda: old_wow(W, a, fam, ISOLATION_LEVEL, **kw))
        got = engine_wow(W, a, fam, ISOLATION_LEVEL, **kw)
        against_oracle(f"wow_cube one slice whitening={whitening} {dtype}", got, ref, dtype)
        assert_same_result(got, old, f"whitening={whitening}")
        for s in range(ISOLATION_LEVEL):
            far = Z0 + hw * (2 ** (s + 1) - 1) + (hw * 2 ** s if whitening else 0) + 1
            assert far < shape[0] and not np.any(got[1][s, far:]), f"whitening={whitening} plane {s}"
            assert np.array_equal(ref[1][s, far:], np.zeros_like(ref[1][s, far:]))
        if not whitening:
            far = Z0 + hw * (2 ** ISOLATION_LEVEL - 1) + 1
            assert not np.any(got[1][ISOLATION_LEVEL, far:]) and not np.any(got[0][far:])


# =========================================================================== E. one pooled plan
def test_a_pooled_plan_goes_from_cube_to_cube_to_image(W, O):
    """Pooled plans are keyed (Z*Y, X, family, level): wow_cube on a (4, 6, 70) cube, wow_cube on a (6, 4, 70) cube and
    wow on a 24 x 70 image take the same plan in turn (asserted), each after wt_wow_cube_scale has swapped the pointers
    of the plan's coefficient planes with scratch 3.  Each result against its oracle."""
    fam, L = "b3spline", 2
    monkeypatch = pytest.MonkeyPatch()
    monkeypatch.setenv("WT_CUBE_FUSED", "1")
    try:
        a, b = cube((4, 6, 70), "float32", 11), cube((6, 4, 70), "float32", 12)
        img = cube((24, 70), "float32", 13)
        assert O.wow_n_scales(img.shape, fam, None, 0, [], None) == L

        def run(x):
            c = W.transform_cube(x, L, cls_of(W, fam))
            image, c = W.wow_cube(c)
            return (np.array(image, copy=True), np.array(c.data, copy=True)), c._plan
        (first, plan), calls = kernel_calls(W, lambda: run(a))
        assert calls == L
        second, plan2 = run(b)
        assert plan2 is plan
        image, c = W.wow(img)
        assert c._plan is plan
        third = (np.array(image, copy=True), np.array(c.data, copy=True))
        del c
        again, plan3 = run(a)
        assert plan3 is plan
    finally:
        monkeypatch.undo()
    against_oracle("hand-over first cube", first, oracle_wow(O, a, fam, L), "float32")
    against_oracle("hand-over second cube", second, oracle_wow(O, b, fam, L), "float32")
    against_oracle("hand-over image", third, oracle_wow(O, img, fam), "float32")
    assert_same_result(again, first, "first cube again")
