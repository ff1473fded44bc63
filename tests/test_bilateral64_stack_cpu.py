"""Host logic of the batched float64 bilateral transform (wavelets_amd.batch: bilateral64_eligible, the routes of
transform_stack / denoise_stack, argument errors, the two new entry points) and what
tests/test_gpu_bilateral64_stack.py rests on, checked without a device: its inputs (float64 stacks whose neighbouring
frames are nine decades apart, the element types the reference recasts) and the premise of its hard-threshold
comparisons - no thresholded coefficient of the float64 numpy oracle lies within 1e-10 (relative) of its threshold,
so those comparisons leave no sample out.  The GPU module imports its inputs and bounds from here."""
import ctypes
import os
import re
import warnings
from functools import lru_cache

import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B
from oracle import atrous_numpy as O
from test_batch64_cpu import TRUE_TYPES, FALSE_TYPES, ROUTE_TYPES, HARD_MARGIN, DTYPE_SHAPE, typed_stack
from test_stack_edges_cpu import per_frame_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the float64 engine's bilateral bound (wt_bilateral64.h's header, tests/test_gpu_round2.py): times max|frame|
BIL64_TRANSFORM_TOL = 1e-12
# The worst error of the PER-FRAME denoise(bilateral=1) in float64 against the float64 oracle over every denoise case
# of the GPU module (all shapes, both families, the three noise modes, both weight lists, the element types, the
# chunked stack), in units of max|frame|, measured on the MI355X with the per-frame API, whose kernels this module's
# subject does not touch: 9.64e-14 soft and 9.66e-14 hard (both on the 2 x 1 B3spline frames).  With anscombe=True
# 6.33e-11 (the quiet '>f4' frame: max|frame| 4e-3 under the transform's 3/8 pedestal, whose inverse subtracts it
# again).  The batched results - the same bits - are held to 4 x those figures (the project's rule).
BIL64_DENOISE_MEASURED = 9.66e-14
BIL64_ANSCOMBE_MEASURED = 6.33e-11
BIL64_DENOISE_TOL = 4 * BIL64_DENOISE_MEASURED
BIL64_ANSCOMBE_TOL = 4 * BIL64_ANSCOMBE_MEASURED

FAMILIES = ["B3spline", "Triangle"]
# (H, W): the minimum height and the pitch padding of odd widths; one column short of, at and one past a wave (64
# lanes); one short of and one past a workgroup (256 columns: two workgroups across); two ordinary frames
SHAPES = [(2, 1), (2, 2), (3, 3), (5, 63), (4, 64), (7, 65), (6, 255), (6, 257), (33, 31), (96, 128)]
STACKS = (1, 2, 9)
AMPS = (1e6, 1e-3)                    # frame i: N(0, 1) * AMPS[i % 2] - every quiet frame lies between two loud ones
LEVEL = 3
# (bilateral, bilateral_scaling) of the transform cases
MODES = {"one": (1, False), "true": (True, False), "list_scaling": ([2., .5], True)}
# levels on DEEP_SHAPE frames: the dilation exceeds the frame many times over (reflections bounce repeatedly); the
# last one is the family's sigma_e(bilateral=...) table
DEEP_SHAPE = (40, 24)
DEEP_LEVELS = {"B3spline": (1, 4, 10), "Triangle": (1, 4, 11)}
DENOISE_WEIGHTS = ([5, 3], [4, 2, 1, 0, 0])
CHUNK_SHAPE = (7, 65)
# Seed of a shape's stack where seed 0 does not meet the premise of the hard-threshold comparisons (below)
SEEDS = {}


def bil64_stack(shape, n=max(STACKS)):
    """n float64 frames of `shape`, zero-mean (the variance conv(I^2) - conv(I)^2 of a frame on a pedestal cancels, and
    the order of the additions alone is then worth more than the bound: __graft_entry__.smoke's note); the first k
    frames of the n-frame stack are the k-frame stack"""
    rng = np.random.default_rng([SEEDS.get(tuple(shape), 0), 64, 11, shape[0], shape[1]])
    fr = rng.standard_normal((n,) + tuple(shape))
    for i in range(n):
        fr[i] *= AMPS[i % 2]
    return fr


def noise_modes(n):
    """(name, `noise` of denoise_stack): MAD, one scalar, one entry per frame of the frame's own order of magnitude
    (with a None among them when the stack is long enough)"""
    per = [0.8 * AMPS[i % 2] * (1 + 0.125 * i) for i in range(n)]
    if n > 4:
        per[4] = None
    return [("mad", None), ("scalar", 0.7), ("list", per)]


def leak_stack(shape=(33, 31)):
    """(stack, index of the NaN frame): loud, constant (local variance exactly zero), quiet, NaN, loud"""
    fr = bil64_stack(shape, 5)
    fr[1] = 2e6
    fr[3] = np.nan
    return fr, 3


def _quiet(fn, *a, **k):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _key(frame):
    a = np.ascontiguousarray(frame, np.float64)
    return a.shape, a.tobytes()


@lru_cache(maxsize=None)
def _ref_planes(key, level, fam, bil, scaling):
    shape, raw = key
    f = np.frombuffer(raw, np.float64).reshape(shape).copy()
    out = _quiet(O.atrous_standard, f, level, fam.lower(), list(bil) if isinstance(bil, tuple) else bil, scaling)
    out.setflags(write=False)
    return out


def ref_transform(frame, level, fam, bilateral=1, scaling=False):
    """the float64 oracle's planes of one frame (computed once per input, read-only)"""
    return _ref_planes(_key(frame), level, fam, tuple(bilateral) if isinstance(bilateral, list) else bilateral, scaling)


def ref_denoise(frame, weights, fam, noise, soft, anscombe=False):
    """oracle.denoise(frame, weights, fam, noise, bilateral=1, soft, anscombe) in float64 - its statements, on the
    shared planes"""
    if anscombe:
        return _quiet(O.denoise, np.array(frame, np.float64), list(weights), fam.lower(), noise, 1, soft, True)
    c = O.Coeffs(ref_transform(frame, len(weights), fam).copy(), fam.lower(), 1)
    c.noise = noise
    _quiet(c.denoise, list(weights), soft_threshold=soft)
    return np.sum(c.data, axis=0)


def hard_margin(frame, weights, fam, noise):
    """min over the thresholded coefficients of | |w| - tau | / tau in the float64 oracle's denoise(bilateral=1, hard
    threshold); inf when nothing is thresholded"""
    c = O.Coeffs(ref_transform(frame, len(weights), fam), fam.lower(), 1)
    c.noise = noise
    worst = np.inf
    for s, sig in enumerate(weights):
        if sig == 0:
            continue
        if c.noise is None:
            c.noise = c.get_noise()                               # (lazy, as the reference: plane 0 is untouched here)
        if c.noise == 0:
            continue
        tau = sig * c.noise * c.sigma_e[s]
        worst = min(worst, float((np.abs(np.abs(c.data[s]) - abs(tau)) / abs(tau)).min()))
    return worst


def hard_cases():
    """(label, frames as float64, fam, weights, per-frame noise) of every hard-threshold comparison of the GPU module"""
    for shape in SHAPES:
        fr = bil64_stack(shape)
        for fam in FAMILIES:
            for weights in DENOISE_WEIGHTS:
                for mode, noise in noise_modes(len(fr)):
                    yield f"{shape} {fam} {weights} {mode}", fr, fam, weights, per_frame_noise(noise, len(fr))
    for dt in ROUTE_TYPES:
        fr = typed_stack(dt).astype(np.float64)
        for noise in (None, 0.8):
            yield f"{np.dtype(dt).str} {noise}", fr, "B3spline", [5, 3], [noise] * len(fr)
    fr = bil64_stack(CHUNK_SHAPE)
    per = [0.8 * AMPS[i % 2] * (1 + i) for i in range(9)]
    per[4] = None
    for weights in DENOISE_WEIGHTS:
        yield f"chunks {weights}", fr, "B3spline", weights, per


# ---------------------------------------------------------------- the predicate

class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


class Custom(W.AbstractScalingFunction):
    coefficients_1d = np.array([0.2, 0.6, 0.2])

    def __init__(self, n_dim):
        super().__init__("custom", n_dim)


GOOD_BILATERAL = (1, True, 0.5, np.float32(2), np.int64(1), [2., .5], [], [1, True, np.float64(3)])
BAD_BILATERAL = ("1", (1, 2), np.ones(3), [1, "a"], [[1]], 1j, [None])


def test_bilateral64_eligible_truth_table():
    assert "bilateral64_eligible" in B.__all__ and W.batch.bilateral64_eligible is B.bilateral64_eligible
    shape = (3, 64, 80)
    f64 = np.zeros(shape)
    assert not B.bilateral64_eligible(f64, 4)                                # no bilateral filtering: not its case
    assert not B.bilateral64_eligible(f64, 4, W.B3spline, None)
    for dt in TRUE_TYPES:                       # float64, '>f8', '>f4', int16, uint16, int32, uint32, int64
        fr = np.zeros(shape, dt)
        assert B.bilateral64_eligible(fr, 4, bilateral=1), dt
        assert B.bilateral64_eligible(fr, 1, W.Triangle, True) and B.bilateral64_eligible(fr, 6, W.Triangle, [2., .5]), dt
        assert B.bilateral64_eligible(fr, 5, bilateral=1, noise_per_frame=[None, 0.5, np.float64(2)]), dt
    for dt in FALSE_TYPES + [np.uint64, np.float16, ">i2"]:       # float32, uint8, int8, bool: not float64 for the reference
        assert not B.bilateral64_eligible(np.zeros(shape, dt), 4, bilateral=1), dt
    assert not B.bilateral64_eligible([f64[0], f64[1]], 4, bilateral=1)                       # not stacked
    assert not B.bilateral64_eligible([f64[0], f64[1].astype(np.float32)], 4, bilateral=1)     # mixed element types
    assert not B.bilateral64_eligible(f64[0], 4, bilateral=1) and not B.bilateral64_eligible(f64[None], 4, bilateral=1)
    # `bilateral`: bilateral_eligible's table, form by form
    f32 = np.zeros(shape, np.float32)
    for bil in GOOD_BILATERAL:
        assert B.bilateral_eligible(f32, 4, W.B3spline, bil), bil
        assert B.bilateral64_eligible(f64, 4, W.B3spline, bil), bil
        assert B.bilateral64_eligible(f64, 1, W.Triangle, bil), bil
    for bil in BAD_BILATERAL:
        assert not B.bilateral_eligible(f32, 4, W.B3spline, bil), bil
        assert not B.bilateral64_eligible(f64, 4, W.B3spline, bil), bil
    # 1 <= level <= the family's sigma_e(bilateral=...) table and the march's 25 scales
    assert not B.bilateral64_eligible(f64, 0, bilateral=1) and not B.bilateral64_eligible(f64, -1, bilateral=1)
    assert not B.bilateral64_eligible(f64, True, bilateral=1) and not B.bilateral64_eligible(f64, 2.0, bilateral=1)
    assert B.bilateral64_eligible(f64, np.int64(2), bilateral=1)
    for fam, cls in (("B3spline", W.B3spline), ("Triangle", W.Triangle)):
        n_tab = len(cls(2).sigma_e(bilateral=1))
        assert n_tab == DEEP_LEVELS[fam][-1] <= B.BILATERAL_MAX_LEVEL == 25
        assert B.bilateral64_eligible(f64, n_tab, cls, 1) and not B.bilateral64_eligible(f64, n_tab + 1, cls, 1)
    # frames the float64 march does not take per frame: one row; rows the batch does not accept
    assert not B.bilateral64_eligible(np.zeros((2, 1, 64)), 4, bilateral=1)
    assert B.bilateral64_eligible(np.zeros((2, 2, 1)), 4, bilateral=1) and B.bilateral64_eligible(np.zeros((1, 2, 80000)), 4, bilateral=1)
    assert not B.bilateral64_eligible(np.zeros((1, 2, 100000)), 4, bilateral=1)
    # the noise levels follow bilateral_eligible
    for noise, want in ((None, False), ([np.ones((64, 80))] * 3, False), ([np.array(2.0)] * 3, False),
                        ([None, 0.0, np.float32(2)], True), ([None, None, None], True), ((), True)):
        assert B.bilateral_eligible(f32, 4, bilateral=1, noise_per_frame=noise) == want, noise
        assert B.bilateral64_eligible(f64, 4, bilateral=1, noise_per_frame=noise) == want, noise
    assert not B.bilateral64_eligible(f64, 4, Retapped, 1) and not B.bilateral64_eligible(f64, 4, Custom, 1)


def test_the_library_states_when_a_frame_takes_the_march():
    """wt_batch64_bilateral_ok: built-in family, H >= 2, rows wt_batch64_create accepts, 1 <= level <= 25 and the
    "stencil64" option - with it off the per-frame call runs the generic three-kernel form, so the stack goes to the loop"""
    for code in (L.B3SPLINE, L.TRIANGLE):
        assert L.batch64_bilateral_ok(code, 2, 1, 1) and L.batch64_bilateral_ok(code, 64, 80, 25)
        assert not L.batch64_bilateral_ok(code, 64, 80, 0) and not L.batch64_bilateral_ok(code, 64, 80, 26)
        assert not L.batch64_bilateral_ok(code, 1, 80, 3) and not L.batch64_bilateral_ok(code, 64, 0, 3)
        assert not L.batch64_bilateral_ok(code, 2, 100000, 3)
    assert not L.batch64_bilateral_ok(7, 64, 80, 3)
    f64 = np.zeros((3, 64, 80))
    try:
        L.set_option("stencil64", 0)
        assert not L.batch64_bilateral_ok(L.B3SPLINE, 64, 80, 3)
        assert not B.bilateral64_eligible(f64, 3, bilateral=1)
    finally:
        L.set_option("stencil64", 1)
    assert L.batch64_bilateral_ok(L.B3SPLINE, 64, 80, 3) and B.bilateral64_eligible(f64, 3, bilateral=1)


def test_the_older_predicates_keep_their_answers():
    for dt in TRUE_TYPES + FALSE_TYPES:
        fr = np.zeros((3, 64, 80), dt)
        f32 = np.dtype(dt) == np.float32
        f64 = dt in TRUE_TYPES
        for bil in (1, True, [2., .5]):
            assert not B.batch_eligible(fr, 6, bilateral=bil) and not B.wow_eligible(fr, 4, bilateral=bil), dt
            assert not B.batch64_eligible(fr, 6, bilateral=bil), dt
            assert B.bilateral_eligible(fr, 6, bilateral=bil) == f32, dt
            assert B.enhance_eligible(fr, 3, bilateral=bil) == ("bilateral" if f32 else None), dt
        assert B.batch_eligible(fr, 6) == f32 and B.wow_eligible(fr, 6) == f32, dt
        assert B.batch64_eligible(fr, 6) == f64 and not B.bilateral_eligible(fr, 6), dt
        assert B.enhance_eligible(fr, 3) == ("batch" if f32 else "batch64" if f64 else None), dt
    f64 = np.zeros((3, 64, 80))
    assert not B.batch64_eligible(f64, 6, bilateral=1) and B.enhance_eligible(f64, 3, bilateral=1) is None
    for bil in GOOD_BILATERAL:
        assert not B.bilateral_eligible(f64, 4, W.B3spline, bil), bil
    for noise in (None, [np.ones((64, 80))] * 3, [np.array(2.0)] * 3):
        assert not B.bilateral_eligible(np.zeros((3, 64, 80), np.float32), 4, bilateral=1, noise_per_frame=noise)


# ---------------------------------------------------------------- the entry points

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "watroo_hip.h")).read(), flags=re.S)


def test_the_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    want = {"wt_batch64_decompose_bilateral": ["batch", "nf", "src", "level", "sigma_b", "bilateral_scaling", "flags"],
            "wt_batch64_bilateral_ok": ["family", "H", "W", "level", "ok"]}
    for name, params in want.items():
        assert hasattr(lib, name), name
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", _header())
        assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == params, name
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), name
    assert L.SIGNATURES["wt_batch64_decompose_bilateral"][1][4] == ctypes.POINTER(ctypes.c_double)
    assert L.SIGNATURES["wt_batch64_bilateral_ok"][1][4] == ctypes.POINTER(ctypes.c_int)
    # every entry point cites its reference call site
    raw = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    for name in want:
        comment = raw[:raw.index("int " + name)].rsplit("/*", 1)[1]
        assert "watroo/wavelets.py:" in comment, name
    assert callable(L.BatchPlan64.decompose_bilateral) and callable(L.batch64_bilateral_ok)
    assert L.load().wt_abi_version() == 8                                         # additive: the version stays


def test_the_new_unit_is_built_and_probed():
    import __graft_entry__ as G
    units = {obj: (src, flags) for obj, src, flags in G._units()}
    assert units["bilateral64_batch.o"] == ("wt_bilateral64_batch.hip", ["-DWT_TU_NAME=bilateral64_batch"])
    probe = open(os.path.join(ROOT, "wavelets_amd", "csrc", "wt_unit_probe.h")).read()
    assert "X(bilateral64_batch)" in probe


# ---------------------------------------------------------------- argument errors, routes

def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    for name in ("default_context", "acquire_batch", "acquire_batch64", "BatchPlan64"):
        monkeypatch.setattr(L, name, boom)


def test_argument_errors_before_device_work(monkeypatch):
    _no_device(monkeypatch)
    f64 = np.zeros((3, 64, 64))
    i16 = np.zeros((3, 64, 64), np.int16)
    assert B.bilateral64_eligible(f64, 3, bilateral=1) and B.bilateral64_eligible(i16, 2, bilateral=1)
    with pytest.raises(ValueError, match="one entry per frame"):
        W.denoise_stack(f64, [5, 3], noise=[1.0, 2.0], bilateral=1)
    with pytest.raises(ValueError, match="one entry per frame"):
        W.denoise_stack(i16, [5, 3], noise=[1.0, 2.0, 3.0, 4.0], bilateral=True)
    with pytest.raises(ValueError, match="out"):
        W.transform_stack(f64, 3, out=np.zeros((3, 3, 64, 64)), bilateral=1, bilateral_scaling=True)
    with pytest.raises(ValueError, match="out"):
        W.denoise_stack(i16, [5, 3], out=np.zeros((2, 64, 64), np.float32), bilateral=[2., .5])
    with pytest.raises(ValueError, match="ndim|shape"):
        W.transform_stack(np.zeros((64, 64)), 3, bilateral=1)
    with pytest.raises(ValueError, match="one shape"):
        W.transform_stack([np.zeros((64, 64)), np.zeros((64, 65))], 3, bilateral=1)


class _Recorder:
    """a BatchPlan64 without a device: records the calls of the stack routes"""

    def __init__(self, n, H, W_):
        self.n, self.H, self.W, self.calls = n, H, W_, []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name,) + tuple(x for x in a if not isinstance(x, np.ndarray)))
            if name == "abs_median":
                return [np.float64(1.0)] * a[0]
        return call


def test_the_routes_call_the_batched_march_once_per_chunk(monkeypatch):
    """transform_stack and denoise_stack on a float64 stack with bilateral=: a BatchPlan64 of batch_chunks(itemsize=8)
    frames, per chunk one upload, ONE decompose_bilateral with the transform's sigma list, and the downloads; the
    per-frame loop is not entered.  enhance_stack and wow_stack keep their routes (the per-frame loop)."""
    recs = []

    def acquire(ctx, n, H, W_, fam, level):
        recs.append(_Recorder(n, H, W_))
        return recs[-1]

    def boom(*a, **k):
        raise AssertionError("the per-frame loop ran")
    monkeypatch.setattr(L, "default_context", lambda: None)
    monkeypatch.setattr(L, "acquire_batch64", acquire)
    monkeypatch.setattr(L, "release_batch64", lambda bp: None)
    monkeypatch.setattr(L, "acquire_batch", boom)
    monkeypatch.setattr(B, "AtrousTransform", boom)
    monkeypatch.setattr(B, "denoise", boom)
    monkeypatch.setattr(L, "BATCH_BYTES", 4 * L.batch_frame_bytes(7, 65, 3, itemsize=8) + 8)
    fr = bil64_stack(CHUNK_SHAPE)
    out = np.empty((9, 4, 7, 65))
    assert W.transform_stack(fr, 3, out=out, bilateral=[2., .5], bilateral_scaling=True) is out
    calls = recs[-1].calls
    assert recs[-1].n == 4 and [c for c in calls if c[0] == "decompose_bilateral"] == \
        [("decompose_bilateral", nf, L.PLANE_INPUT, 3, [2., .5, 1, 1], True) for nf in (4, 4, 1)]
    assert [c[0] for c in calls].count("upload") == 3 and [c[0] for c in calls].count("download") == 3 * 4
    assert not any(c[0] == "decompose" for c in calls)
    monkeypatch.setattr(L, "BATCH_BYTES", 4 * L.batch_frame_bytes(7, 65, 2, itemsize=8) + 8)
    den = np.empty((9, 7, 65))
    assert W.denoise_stack(fr.astype(">f8"), [5, 3], bilateral=1, anscombe=True, out=den) is den
    names = [c[0] for c in recs[-1].calls]
    assert names == ["upload", "anscombe", "decompose_bilateral", "abs_median", "denoise_sum", "anscombe", "download"] * 3
    assert [c for c in recs[-1].calls if c[0] == "decompose_bilateral"] == \
        [("decompose_bilateral", nf, L.PLANE_INPUT, 2, [1, 1, 1], False) for nf in (4, 4, 1)]


# ---------------------------------------------------------------- premises of the GPU module (oracle only)

def test_inputs_are_what_the_gpu_module_claims():
    assert min(h for h, _ in SHAPES) == 2 and {(2, 1), (2, 2), (3, 3)} <= set(SHAPES)
    assert {63, 64, 65, 255, 257} <= {w for _, w in SHAPES} and sum(w % 2 for _, w in SHAPES) >= 5
    for shape in SHAPES + [DEEP_SHAPE, CHUNK_SHAPE]:
        fr = bil64_stack(shape)
        assert fr.dtype == np.float64 and fr.shape == (9,) + shape
        amax = np.abs(fr).reshape(9, -1).max(axis=1)
        if shape[0] * shape[1] >= 4:
            for i in range(1, 9, 2):          # every quiet frame: both neighbours at least 1e7 times louder than it
                assert amax[i] * 1e7 < min(amax[i - 1], amax[i + 1]), shape
        for n in STACKS:
            assert np.array_equal(bil64_stack(shape, n), fr[:n])
        assert B.bilateral64_eligible(fr, LEVEL, bilateral=1)
    for fam in FAMILIES:                      # the deepest dilation exceeds the frame many times over
        assert 2 ** (DEEP_LEVELS[fam][-1] - 1) >= 10 * max(DEEP_SHAPE)
    fr, bad = leak_stack()
    assert np.isnan(fr[bad]).all() and np.ptp(fr[1]) == 0 and all(np.isfinite(fr[i]).all() for i in (0, 1, 2, 4))
    for dt in ROUTE_TYPES:
        ts = typed_stack(dt)
        assert ts.dtype == np.dtype(dt) and ts.shape == (3,) + DTYPE_SHAPE and B.bilateral64_eligible(ts, 2, bilateral=1)


@pytest.mark.parametrize("part", [0, 1, 2, 3])
def test_reference_keeps_every_hard_threshold_sample_clear_of_its_threshold(part):
    """For every input the GPU module compares under hard thresholds: no thresholded coefficient of the float64 oracle
    (bilateral=1) lies within HARD_MARGIN (relative) of its threshold - a condition on the inputs, evaluated on the
    reference alone.  With it a hard-threshold comparison leaves no sample out."""
    worst = np.inf
    for k, (label, fr, fam, weights, noises) in enumerate(hard_cases()):
        if k % 4 != part:
            continue
        for i, (f, n_i) in enumerate(zip(fr, noises)):
            m = hard_margin(f, weights, fam, n_i)
            worst = min(worst, m)
            assert m > HARD_MARGIN, (label, i, m)
    print(f"worst relative margin to a hard threshold: {worst:.3e}")
