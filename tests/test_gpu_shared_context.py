"""Two plans on ONE context, their calls interleaved in host order on one thread.

The lanes of sequence.map_frames are shared by concurrent callers: several plans live on one lane context and their C
calls interleave between lock releases (the context's lock serialises calls, not call sequences).  The context carries
state a sequence relies on across calls - the select's bins, state and window base word (d_hist), the reduction partials
and the sample keys of the windowed median (d_partials), the pinned host scratch, the riding-histogram marker, the side
stream with its pending flag.  Every case here

  1. runs sequence B alone and sequence A alone, each on its own plan, and records every result (the bitwise reference;
     every median of it is also held against numpy on the downloaded plane, by the rule of tests/test_gpu_parity.py's
     test_exact_median: equality with np.median(np.abs(plane)), i.e. the lower / upper median of the magnitudes taken
     in float64 and averaged in the plane's type);
  2. uploads again and runs the calls of A between the calls of B;
  3. asserts that no call raised and that every result has the recorded bits.

B is a sequence that leaves work on the side stream (a bilateral transform, then the MAD median of w_0, the wow update of
a scale, the early plane sum, or wow's whole per-scale order, utils._wow_scales); A is a main-stream user of the context
scratch (a transform whose first pass rides the median's histogram and the median that takes it, a median without
marker, wt_reduce).  Both in float32 (Plan) and float64 (Plan64).  The host arranges no timing: what varies between
repetitions is only how far the GPU has come when the next call is queued, hence the repetitions.

Images are a seeded normal field on a ramp, without NaN: "rank ... not found (NaN input?)" must never come from them.
Shapes: plain bins with an even and with an odd pixel count (the upper median is or is not looked for), 2^20 pixels -
the first size of the windowed histogram, riding and sampled - and the size just below it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

B3 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
SHAPES = [(256, 300), (67, 131), (64, 66), (1023, 1024), (1024, 1024)]
LEVELS = [1, 2, 4]
A_LEVEL = 2                   # scales of plan A's transform: one fused pass, the one that rides the histogram
TAU = 0.5                     # threshold of the single wow updates (the whole-order sequence derives its own from the MAD)
B_KINDS = ["median", "wow_scale", "wow_update", "sum", "wow"]
A_KINDS = ["prehist", "median", "reduce"]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as entry
    entry.build()
    from wavelets_amd import _lib
    if _lib.device_count() == 0:
        pytest.skip("no GPU")
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def _reps(shape):
    return 20 if shape[0] * shape[1] < (1 << 19) else 3


def _img(shape, seed, f64):
    H, W = shape
    a = np.random.default_rng(seed).standard_normal(shape) * (1 + seed % 5) + 3.0 * np.arange(W)[None, :] / W + seed % 7
    return a if f64 else a.astype(np.float32)


def _plan(L, ctx, shape, level, f64):
    H, W = shape
    return L.Plan64(ctx, H, W, B3, level) if f64 else L.Plan(ctx, H, W, L.B3SPLINE, level)


def _np_median(plane):
    """np.median(np.abs(plane)) from the lower and upper median of the float64 magnitudes"""
    a = np.abs(plane.astype(np.float64)).ravel()
    n = a.size
    part = np.partition(a, [(n - 1) // 2, n // 2])
    t = plane.dtype.type
    lo, hi = t(part[(n - 1) // 2]), t(part[n // 2])
    return lo if n & 1 else t((lo + hi) / t(2))


def _bits(x):
    if isinstance(x, np.ndarray):
        return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)
    return np.asarray(x)


def _same(x, y):
    return np.array_equal(_bits(x), _bits(y))


def _hist_flags(L):
    return L.FLAG_FUSED | L.FLAG_MEDIAN_HIST


# --------------------------------------------------------------------------- sequence B: leaves work on the side stream
def _run_b(L, kind, p, src, level, gap):
    """One B sequence on plan p; gap() runs between the transform and the next call and between every later pair of
    calls.  Returns {name: result}: the scalars the calls returned and the planes they wrote."""
    import wavelets_amd as W
    from wavelets_amd import utils, wavelets
    NONE, OUT = L.PLANE_NONE, L.PLANE_OUT
    f64 = isinstance(p, L.Plan64)
    ft = np.float64 if f64 else np.float32
    out, planes = {}, [0]
    p.upload(L.PLANE_INPUT, src)
    p.decompose_bilateral(L.PLANE_INPUT, level, wavelets._sigma_bilateral_list(1, level))
    gap()
    if kind == "median":
        out["median"] = p.abs_median(0)
    elif kind == "wow_scale":
        p.wow_scale(0, 0, TAU, True, NONE, 1.0, NONE)
    elif kind == "wow_update":
        p.wow_update(0, NONE, TAU, True, NONE, 1.0, NONE)
    elif kind == "sum":
        # the early plane sum wants its planes updated on the side stream since the transform (wt_plane_sum_early)
        count = max(1, level // 2)
        for s in range(count):
            p.wow_scale(s, s, TAU, True, NONE, 1.0, NONE)
            gap()
        early = p.plane_sum_early(count, OUT)
        gap()
        if early:
            p.plane_sum_resume(count, level + 1 - count, OUT)
        else:
            p.plane_sum(0, level + 1, OUT)
        planes = list(range(count)) + [OUT]
    elif kind == "wow":
        # utils._wow_scales + the sum of utils._wow_device for wow(img, bilateral=1, denoise_coefficients=[5, 2])
        sigma_e = W.B3spline(2).sigma_e(bilateral=1)
        nplanes, npix = level + 1, float(p.H) * float(p.W)
        weights, sdc = utils._wow_lists([], [5, 2], level)
        tail = utils._SUM_TAIL_PLANES_F64 if f64 else utils._SUM_TAIL_PLANES
        early, early_at = 0, (nplanes - tail if nplanes >= 2 * tail else 0)
        noise = None
        for s, (_, w, d) in enumerate(zip(range(nplanes), weights, sdc)):
            if s and s == early_at and p.plane_sum_early(s, OUT):
                early = s
                gap()
            if s == level:
                out["moments"] = moments = p.reduce(s)
                gap()
                factor = utils._wow_factor(s, level, w, moments, npix, False, True, 0, ft)
                p.wow_update(s, NONE, 0.0, True, NONE, factor, NONE)
            else:
                tau = 0.0
                if d:
                    if noise is None:
                        out["median"] = p.abs_median(0)
                        gap()
                        noise = wavelets._noise_from_median(out["median"], sigma_e)
                    tau = wavelets._scalar_tau(d, noise, sigma_e[s], True)[0]
                p.wow_scale(s, s, tau, True, NONE, ft(1), NONE)
            gap()
        if early:
            p.plane_sum_resume(early, nplanes - early, OUT)
        else:
            p.plane_sum(0, nplanes, OUT)
        planes = list(range(nplanes)) + [OUT]
    gap()
    for q in planes:
        out[f"plane {q}"] = p.download(q).copy()
    return out


# --------------------------------------------------------------------------- sequence A: main-stream users of the scratch
class _A:
    """The calls of plan A that go between B's: gap() issues the next ones and records what they return."""

    def __init__(self, L, kind, p):
        self.L, self.kind, self.p, self.got, self.riding = L, kind, p, [], False

    def gap(self):
        L, p = self.L, self.p
        if self.kind == "prehist":
            if self.riding:
                self.got.append(p.abs_median(0))
            p.decompose(L.PLANE_INPUT, A_LEVEL, _hist_flags(L))        # the first pass rides the histogram of |w_0|
            self.riding = True
        elif self.kind == "median":
            self.got.append(p.abs_median(L.PLANE_INPUT))               # no marker: the select's own passes
        else:
            self.got.append(p.reduce(L.PLANE_INPUT))

    def finish(self):
        if self.riding:
            self.got.append(self.p.abs_median(0))
            self.riding = False
        return self.got


def _a_reference(L, p, src):
    """A alone: every value its calls return, each median held against numpy, the moments against the float64 sums"""
    p.upload(L.PLANE_INPUT, src)
    p.decompose(L.PLANE_INPUT, A_LEVEL, _hist_flags(L))
    ref = {"prehist": p.abs_median(0)}
    assert ref["prehist"] == _np_median(p.download(0)), "plan A alone: riding median != numpy"
    ref["median"] = p.abs_median(L.PLANE_INPUT)
    assert ref["median"] == _np_median(src), "plan A alone: median != numpy"
    ref["reduce"] = p.reduce(L.PLANE_INPUT)
    s, s2, lo, hi = ref["reduce"]
    wide = src.astype(np.float64)
    assert lo == float(src.min()) and hi == float(src.max())
    assert abs(s - wide.sum()) <= 1e-6 * src.size * float(np.abs(wide).max())
    assert abs(s2 - (wide * wide).sum()) <= 1e-6 * src.size * float((wide * wide).max())
    return ref


@pytest.mark.parametrize("a64", [False, True], ids=["A32", "A64"])
@pytest.mark.parametrize("b64", [False, True], ids=["B32", "B64"])
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_side_stream_sequence_with_another_plans_calls_between_its_own(L, ctx, shape, level, b64, a64):
    """B: bilateral transform over `level` scales (with 1 nothing stays queued behind scale 0, with 4 three scales do),
    then each continuation of B_KINDS; A: each of A_KINDS in every gap of B.  Every value and plane of both equals the
    un-interleaved run bit for bit, no call raises."""
    _interleave(L, ctx, shape, level, b64, a64, B_KINDS)


def test_wow_order_with_the_early_plane_sum_and_another_plans_calls_between(L, ctx):
    """8 planes: the size from which utils._wow_scales queues the sum of the leading planes early (float32)"""
    _interleave(L, ctx, (256, 300), 7, False, False, ["wow"])
    _interleave(L, ctx, (256, 300), 7, False, True, ["wow"])


def _interleave(L, ctx, shape, level, b64, a64, b_kinds):
    src_b, src_a = _img(shape, 11 + level, b64), _img(shape, 23, a64)
    pb, pa = _plan(L, ctx, shape, level, b64), _plan(L, ctx, shape, A_LEVEL, a64)
    bad = []
    try:
        ref_a = _a_reference(L, pa, src_a)
        for bk in b_kinds:
            ref_b = _run_b(L, bk, pb, src_b, level, lambda: None)
            if "median" in ref_b:
                w0 = ref_b["plane 0"]
                if bk == "wow":              # plane 0 is whitened by then: the median's plane is the transform's
                    pb.decompose_bilateral(L.PLANE_INPUT, level, [1.0] * (level + 1))
                    w0 = pb.download(0)
                assert ref_b["median"] == _np_median(w0), f"B {bk} alone: median != numpy"
            for ak in A_KINDS:
                for rep in range(_reps(shape)):
                    tag = f"B={bk} A={ak} rep {rep}"
                    a = _A(L, ak, pa)
                    try:
                        pa.upload(L.PLANE_INPUT, src_a)
                        got_b = _run_b(L, bk, pb, src_b, level, a.gap)
                        got_a = a.finish()
                    except L.WatrooHipError as e:
                        bad.append(f"{tag}: raised {e}")
                        continue
                    bad += [f"{tag}: B's {k} differs ({got_b[k]!r} != {v!r})" if np.ndim(v) == 0 or isinstance(v, tuple)
                            else f"{tag}: B's {k} differs in {int((_bits(got_b[k]) != _bits(v)).sum())} pixels"
                            for k, v in ref_b.items() if not _same(got_b[k], v)]
                    bad += [f"{tag}: A's call {i} returned {g!r} != {ref_a[ak]!r}" for i, g in enumerate(got_a)
                            if not _same(g, ref_a[ak])]
                    assert got_a, "no call of A was issued"
    finally:
        pb.close()
        pa.close()
    assert not bad, f"{len(bad)} interleaved results differ or raised:\n" + "\n".join(bad[:40])


# --------------------------------------------------------------------------- the riding-histogram marker, no side stream
@pytest.mark.parametrize("b64", [False, True], ids=["B32", "B64"])
@pytest.mark.parametrize("a64", [False, True], ids=["A32", "A64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_riding_histogram_marker_with_two_plans_on_the_context(L, ctx, shape, a64, b64):
    """The marker names ONE plan and the bins hold ONE plane's histogram: a second plan's riding transform, or its
    median of another plane, between a plan's transform and its median must cost that plan the shortcut, not the value;
    a plan closed with its marker standing must not hand it to a new plan (which may get the same address)."""
    IN = L.PLANE_INPUT
    src_a, src_b, other = _img(shape, 5, a64), _img(shape, 6, b64), _img(shape, 8, a64)
    pa, pb = _plan(L, ctx, shape, A_LEVEL, a64), _plan(L, ctx, shape, A_LEVEL, b64)
    bad = []
    try:
        ref = {}
        for name, p, src in (("A", pa, src_a), ("B", pb, src_b)):
            r = _a_reference(L, p, src)
            ref[name], ref[name + " input"] = r["prehist"], r["median"]
        flags = _hist_flags(L)

        def check(tag, **got):
            bad.extend(f"{tag}: {k} {v!r} != {ref[k.replace('_', ' ')]!r}" for k, v in got.items() if not _same(v, ref[k.replace("_", " ")]))
        for rep in range(5):
            try:
                pa.decompose(IN, A_LEVEL, flags)
                pb.decompose(IN, A_LEVEL, flags)
                a, b = pa.abs_median(0), pb.abs_median(0)
                check(f"A.t B.t A.m B.m rep {rep}", A=a, B=b)
                pa.decompose(IN, A_LEVEL, flags)
                pb.decompose(IN, A_LEVEL, flags)
                b, a = pb.abs_median(0), pa.abs_median(0)
                check(f"A.t B.t B.m A.m rep {rep}", A=a, B=b)
                pa.decompose(IN, A_LEVEL, flags)
                b, a = pb.abs_median(IN), pa.abs_median(0)
                check(f"A.t B.m(input) A.m rep {rep}", A=a, B_input=b)
                pb.decompose(IN, A_LEVEL, flags)
                a, b = pa.abs_median(1), pb.abs_median(0)
                check(f"B.t A.m(1) B.m rep {rep}", B=b)
            except L.WatrooHipError as e:
                bad.append(f"rep {rep}: raised {e}")
        for rep in range(3):
            pa.decompose(IN, A_LEVEL, flags)
            pa.close()
            pa = _plan(L, ctx, shape, A_LEVEL, a64)
            pa.upload(0, other)
            got = pa.abs_median(0)
            if got != _np_median(other):
                bad.append(f"closed plan's marker, rep {rep}: {got!r} != {_np_median(other)!r}")
            pa.upload(IN, src_a)
    finally:
        pa.close()
        pb.close()
    assert not bad, f"{len(bad)} results differ or raised:\n" + "\n".join(bad[:40])
