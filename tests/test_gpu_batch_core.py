"""The refusals of the batch engines' shared host core (wt_batch_core.h), byte for byte.

A fixed list of calls on a float32 and a float64 batch of 3 frames of 5 x 8 with max_level 2, every one an argument
error that the library refuses by return code BEFORE any launch: the frame count and frame range checks, the plane
lookup, the aliasing rules of the transform, of the threshold sums, of wow, of the gamma blend and of the plane sum.
tests/test_gpu_batch_core.json holds (engine, method, arguments) -> (exception class, message) as the commit BEFORE
the core was factored out answered them:

    python tests/test_gpu_batch_core.py --record          (on that commit's library; rewrites the table)

As a test the module replays the list and requires the recorded class and message for every call; a call missing from
the table, or one the library accepts, fails.  Several calls hold two errors at once (a bad level AND a bad source
plane, no frames AND no noise plane): they pin the ORDER of the checks, which differs between the engines in places.

The Richardson-Lucy entry points (wt_batch_rl.h) need a batch with a PSF before their later checks can speak, and the
float64 batch owns richardson_lucy's planes only from its first set_psf on.  So a method may carry a label after "@":
"@ok" marks a call the library must ACCEPT (a set_psf, a plane_ptr: an allocation and a copy, no launch) and whose
acceptance is recorded like a refusal; any other label ("@psf") only tells apart the same call before and after it.
These entries were recorded on the commit before the Richardson-Lucy half was folded into one header; the older
entries of the table came out of that recording unchanged."""
import ctypes as _c
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

TABLE = os.path.splitext(os.path.abspath(__file__))[0] + ".json"
N, H, W, ML = 3, 5, 8, 2
IN, OUT, NONE = -1, -2, -1000
S = lambda i: -3 - i            # WT_PLANE_SCRATCH(i)


# arguments that are not plain numbers: (kind, payload) pairs the replay turns into ctypes objects
def D(*v): return ["double[]", list(v)]         # noqa: E704
def R(*v): return ["real[]", list(v)]           # noqa: E704  (the engine's element type)
BUF = ["real buffer", 4 * H * W]                # host frames
VBUF = ["void buffer", 4 * H * W * 8]
PTR, I64 = ["void** out", 0], ["int64* out", 0]
NUL = ["null", 0]
T4, F4, T16 = D(1, 1, 1, 1), R(1, 1, 1, 1), D(*([1.0] * 16))


def calls(engine):
    """[(method, [arguments after the handle])] for "f32" (BatchPlan) or "f64" (BatchPlan64)"""
    f64 = engine == "f64"
    c = []
    add = lambda m, *a: c.append((m, list(a)))
    # ---- the active-frame check: nf of 0 and of n + 1 on every entry point that takes nf
    for nf in (0, N + 1):
        add("decompose", nf, IN, 2, 1)
        add("decompose_bilateral", nf, IN, 2, D(1, 1, 1), 0, 0)
        add("decompose_sum", nf, IN, 2, OUT, 1)
        add("decompose_pass", nf, IN, S(0), 0, 2, 1)
        add("decompose_pass_sum", nf, IN, S(0), 0, 2, 1, OUT, 1, 0)
        add("abs_median", nf, 0, F4)
        add("denoise_sum", nf, 2, OUT, 1, T16, T4, 1, 0)
        add("denoise_sum_map", nf, 2, OUT, 1, T16, T4, 1, 0, S(5), *([NUL] if f64 else []))
        add("denoise_sum_map", nf, 2, OUT, 1, T16, T4, 1, 0, NONE, *([NUL] if f64 else []))     # (two errors: the order)
        add("enhance_sum", nf, 2, OUT, 1, T16, T16, 1, 0)
        add("anscombe", nf, IN, OUT, 1.0, 0.0, 0.0, 0)
        add("fill", nf, OUT, 1.0)
        add("replicate", nf, OUT)
        add("wow_update", nf, 0, T4, 1, F4, NONE)
        add("wow_update_map", nf, 0, T4, 1, F4, NONE, S(5))
        add("wow_scale", nf, 0, 0, T4, 1, F4, NONE)
        add("wow_scale_map", nf, 0, 0, T4, 1, F4, NONE, S(5))
        add("reduce", nf, 0, T16)
        add("gamma_blend", nf, OUT, S(4), F4, F4, 1.0, 0.5)
        add("plane_sum", nf, 0, 2, OUT)
        if not f64:
            add("fill_normal", nf, OUT, 1, 0)
            add("filter2d", nf, IN, OUT, 0, 0, 0, 0)
            add("binary", nf, 0, IN, OUT, S(3))
            add("mrs_update", nf, 0, S(16), T4, 1, 0, 1.0)
            add("fft_apply", nf, IN, OUT, 0)
    # ---- the plane lookup: ids that are no plane of a batch
    for p in [S(2), ML + 1, NONE, S(11), S(15), S(18)] + ([S(6), S(16)] if f64 else []):
        add("plane_ptr", p, PTR, I64)
    for m, a in (("fill", (N, S(2), 1.0)), ("replicate", (N, S(2))), ("reduce", (N, S(2), T16)), ("abs_median", (N, S(2), F4)),
                 ("decompose", (N, S(2), 0, 1)), ("decompose_pass", (N, S(2), S(0), 0, 2, 1)),
                 ("decompose_bilateral", (N, S(2), 1, D(1, 1, 1), 0, 0)), ("denoise_sum", (N, 2, S(2), 1, T16, T4, 1, 0)),
                 ("wow_update", (N, S(2), T4, 1, F4, NONE)), ("gamma_blend", (N, S(2), S(4), F4, F4, 1.0, 0.5)),
                 ("plane_sum", (N, 0, 2, S(2))), ("upload", (S(2), 0, 1, BUF, 0)), ("download", (S(2), 0, 1, BUF, 0))):
        add(m, *a)
    # ---- host <-> plane copies: frame ranges outside the batch, a host stride below a frame's pixels
    for m in ("upload", "download"):
        for f0, nf in ((2, 2), (-1, 1), (0, 0), (0, N + 1), (N, 1)):
            add(m, IN, f0, nf, BUF, 0)
        add(m, IN, 0, 2, BUF, H * W - 1)
    if f64:
        for f0, nf in ((2, 2), (-1, 1), (0, 0)):
            add("upload_elems", IN, f0, nf, VBUF, 10)
    # ---- decompose / decompose_sum: flags, level 0, sources among the outputs or the internal planes, levels
    add("decompose", N, IN, 2, 0)
    add("decompose", N, 0, 0, 1)
    for src in (0, 1, 2, S(0), S(1)):
        add("decompose", N, src, 2, 1)
        add("decompose_sum", N, src, 2, OUT, 1)
        add("decompose", N, src, ML + 1, 1)             # (two errors: the order)
        add("decompose_sum", N, src, ML + 1, OUT, 1)
    for level in (ML + 1, -1):
        add("decompose", N, IN, level, 1)
        add("decompose_sum", N, IN, level, OUT, 1)
    add("decompose_sum", N, IN, 0, OUT, 1)
    add("decompose_sum", N, IN, 2, OUT, 0)
    for dst in (0, 1, 2, IN, S(0), S(1)):
        add("decompose_sum", N, IN, 2, dst, 1)
    add("decompose_sum", N, IN, ML + 1, 1, 1)           # (two errors: the order)
    # ---- single passes: scales outside the batch, aliasing planes, no such kernel, `first`, the sum plane
    add("decompose_pass", N, IN, S(0), 0, 2, 0)
    add("decompose_pass_sum", N, IN, S(0), 0, 2, 0, OUT, 1, 0)
    for s0, ns in ((0, 0), (0, 5), (-1, 2), (1, 3), (0, 4), (1, 1), (1, 2), (0, 1), (2, 1)):
        add("decompose_pass", N, IN, S(0), s0, ns, 1)
        add("decompose_pass_sum", N, IN, S(0), s0, ns, 1, OUT, int(s0 == 0), 0)
    for cur, nxt in ((IN, IN), (1, S(0)), (0, S(0)), (IN, 0), (IN, 1)):
        add("decompose_pass", N, cur, nxt, 0, 2, 1)
        add("decompose_pass_sum", N, cur, nxt, 0, 2, 1, OUT, 1, 0)
    add("decompose_pass_sum", N, IN, S(0), 0, 2, 1, OUT, 0, 0)
    add("decompose_pass_sum", N, IN, S(0), 0, 2, 1, OUT, 0, 1)
    for sum_plane in (IN, S(0), 0, 1):
        add("decompose_pass_sum", N, IN, S(0), 0, 2, 1, sum_plane, 1, 0)
    # ---- decompose_bilateral: levels, sources among the outputs or the internal planes
    for src, level in ((IN, ML + 1), (IN, -1), (1, 2), (0, 0), (2, 2), (S(0), 2), (S(1), 1), (1, ML + 1)):
        add("decompose_bilateral", N, src, level, D(1, 1, 1), 0, 0)
    # ---- the threshold sums
    # (count, dst, n_den); n_den = 0 is an error for enhance_sum only - denoise_sum would launch
    bad_sums = ((0, OUT, 0), (ML + 2, OUT, 1), (17, OUT, 1), (2, OUT, 3), (2, OUT, -1), (2, 1, 1), (1, 0, 1), (2, 0, 3))
    for count, dst, n_den in bad_sums:
        add("denoise_sum", N, count, dst, n_den, T16, T4, 1, 0)
        for noise in (S(5), NONE):
            add("denoise_sum_map", N, count, dst, n_den, T16, T4, 1, 0, noise, *([NUL] if f64 else []))
    for count, dst, n_den in bad_sums + ((2, OUT, 0),):
        add("enhance_sum", N, count, dst, n_den, T16, T16, 1, 0)
    for noise in (OUT, 0, 1, NONE):
        add("denoise_sum_map", N, 2, OUT, 1, T16, T4, 1, 0, noise, *([NUL] if f64 else []))
    # ---- wow
    add("wow_update", N, 0, T4, 1, F4, 0)
    add("wow_update_map", N, 0, T4, 1, F4, 0, S(5))
    add("wow_update_map", N, 0, T4, 1, F4, S(4), NONE)
    add("wow_update_map", N, 0, T4, 1, F4, S(4), 0)
    add("wow_update_map", N, 0, T4, 1, F4, S(4), S(4))
    for plane, s, gamma in ((IN, 0, NONE), (ML + 1, 0, NONE), (0, 25, NONE), (0, -1, NONE), (IN, 25, NONE), (0, 0, 0), (0, 0, S(3))):
        add("wow_scale", N, plane, s, T4, 1, F4, gamma)
        add("wow_scale_map", N, plane, s, T4, 1, F4, gamma, S(5))
    add("wow_scale_map", N, 0, 0, T4, 1, F4, S(4), NONE)
    for noise in (0, S(3), S(4)):
        add("wow_scale_map", N, 0, 0, T4, 1, F4, S(4), noise)
    add("gamma_blend", N, OUT, OUT, F4, F4, 1.0, 0.5)
    add("gamma_blend", N, S(4), S(4), F4, F4, 1.0, 0.5)
    # ---- plane_sum
    for first, count, dst in ((0, 0, OUT), (0, 33, OUT), (0, 17, OUT), (-1, 2, OUT), (1, 3, OUT), (ML + 1, 1, OUT), (0, 2, 1),
                              (0, 3, 0), (1, 2, 2)):
        add("plane_sum", N, first, count, dst)
    # ---- richardson_lucy: the calls run in this order on ONE batch, which has no PSF up to the first "set_psf@ok"
    K9, BAD = R(*([1.0] * 9)), S(2)
    if f64:
        for nf in (0, N + 1):                           # (float32: in the active-frame list above)
            add("filter2d", nf, IN, OUT, 0, 0, 0, 0)
            add("binary", nf, 0, IN, OUT, S(3))
            add("mrs_update", nf, 0, S(16), T4, 1, 0, 1.0)
        # the planes of richardson_lucy are no planes of a float64 batch that has no PSF yet
        add("binary", N, 0, S(6), S(7), S(8))
        add("mrs_update", N, 0, S(16), T4, 1, 0, 1.0)
    add("filter2d", 0, IN, IN, 2, 9, 9, 7)              # (every error at once: the order)
    for slot in (0, 1, -1, 2):
        add("filter2d", N, IN, OUT, slot, 0, 0, 0)
    add("filter2d", N, IN, IN, 0, 9, 9, 7)              # (slot not set AND the rest)
    for slot in (-1, 2):
        add("set_psf", slot, K9, 3, 3)
        add("set_psf", slot, NUL, 3, 3)                 # (two errors: the order)
        add("set_psf", slot, K9, 1, 513)
    add("set_psf", 0, NUL, 3, 3)
    for kh, kw in ((1, 513), (65, 64), (0, 3), (3, 0)) + (((8, 512),) if f64 else ()):   # (8 x 512: the LDS tile, as doubles)
        add("set_psf", 0, K9, kh, kw)
    add("set_psf@ok", 0, K9, 3, 3)
    if f64:
        for p in (S(6), S(10), S(16), S(17)):
            add("plane_ptr@ok", p, PTR, I64)
        for p in (S(2), S(11), S(15), S(18), ML + 1):
            add("plane_ptr@psf", p, PTR, I64)
    add("filter2d@psf", N, IN, OUT, 1, 0, 0, 0)         # (the other slot is still not set)
    for ay, ax in ((3, 0), (0, 3), (-1, 0), (0, -1)):
        add("filter2d@psf", N, IN, OUT, 0, ay, ax, 0)
    add("filter2d@psf", N, IN, IN, 0, 3, 0, 7)          # (anchor, src == dst AND border: the order)
    add("filter2d@psf", N, IN, IN, 0, 1, 1, 7)          # (src == dst AND border)
    add("filter2d@psf", N, IN, IN, 0, 1, 1, 0)
    for border in (1, 2, 7, -1):
        add("filter2d@psf", N, IN, OUT, 0, 1, 1, border)
    add("filter2d@psf", N, BAD, OUT, 0, 1, 1, 7)        # (border AND a bad plane)
    for src, dst in ((BAD, OUT), (IN, BAD), (S(18), OUT), (IN, ML + 1), (BAD, S(11))):
        add("filter2d@psf", N, src, dst, 0, 1, 1, 0)
        add("filter2d@psf", N, src, dst, 0, 1, 1, 3)
    for op in (-1, 5, 99):
        add("binary", N, op, IN, OUT, S(3))
        add("binary", N, op, BAD, OUT, S(3))            # (two errors: the order)
    for a, b2, dst in ((BAD, OUT, S(3)), (IN, BAD, S(3)), (IN, OUT, BAD), (BAD, S(11), S(18)), (S(6), S(7), S(18))):
        add("binary@psf", N, 4, a, b2, dst)
    add("mrs_update@psf", N, 0, S(16), NUL, 1, 0, 1.0)
    add("mrs_update@psf", N, 0, 0, NUL, 1, 0, 1.0)      # (null tau AND plane == mrs_plane)
    add("mrs_update@psf", N, BAD, BAD, T4, 1, 0, 1.0)   # (plane == mrs_plane AND a bad plane)
    for plane, mrs in ((0, 0), (S(16), S(16)), (BAD, S(16)), (0, BAD), (0, S(18)), (ML + 1, S(17)), (BAD, S(18))):
        add("mrs_update@psf", N, plane, mrs, T4, 1, 0, 1.0)
    return c


def accepted_on_purpose(method):
    return method.endswith("@ok")


def key(engine, method, args):
    return json.dumps([engine, method, args])


def _convert(a, real, keep):
    if not isinstance(a, list):
        return a
    kind, v = a
    if kind == "null":
        return None
    if kind == "void** out":
        obj = _c.c_void_p()
    elif kind == "int64* out":
        obj = _c.c_int64()
    elif kind == "void buffer":
        obj = (_c.c_char * v)()
        keep.append(obj)
        return _c.c_void_p(_c.addressof(obj))
    elif kind == "real buffer":
        obj = (real * v)()
    else:
        obj = ((_c.c_double if kind == "double[]" else real) * len(v))(*v)
    keep.append(obj)
    return _c.byref(obj) if kind.endswith("out") else obj


def answers():
    """{key: [exception class name or None, message]} of every listed call on this library"""
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    out = {}
    for engine, cls in (("f32", L.BatchPlan), ("f64", L.BatchPlan64)):
        bp = cls(ctx, N, H, W, L.B3SPLINE, ML)
        try:
            for method, args in calls(engine):
                keep = []
                try:
                    bp._call(method.split("@")[0], *[_convert(a, bp._real, keep) for a in args])
                    out[key(engine, method, args)] = [None, ""]
                except L.WatrooHipError as e:
                    out[key(engine, method, args)] = [type(e).__name__, str(e)]
        finally:
            ctx.sync()
            bp.close()
    return out


def test_the_core_refuses_what_the_two_engines_refused_in_their_words():
    table = json.load(open(TABLE))
    listed = [key(e, m, a) for e in ("f32", "f64") for m, a in calls(e)]
    assert table and len(set(listed)) == len(listed) > 400
    missing = [k for k in listed if k not in table]
    assert not missing, f"{len(missing)} listed calls are not in the recorded table, first: {missing[0]}"
    got = answers()
    on_purpose = {key(e, m, a) for e in ("f32", "f64") for m, a in calls(e) if accepted_on_purpose(m)}
    accepted = [k for k in listed if got[k][0] is None and k not in on_purpose]
    assert not accepted, f"{len(accepted)} calls were not refused, first: {accepted[0]}"
    wrong = [(k, got[k], table[k]) for k in listed if got[k] != table[k]]
    assert not wrong, f"{len(wrong)} refusals changed, first: {wrong[0][0]}: {wrong[0][1]} != recorded {wrong[0][2]}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_batch_core.py --record [--out FILE]")
    got = answers()
    accepted = [k for k, v in got.items() if v[0] is None and not accepted_on_purpose(json.loads(k)[1])]
    if accepted:
        sys.exit("not refused, so not an argument error - take it off the list:\n" + "\n".join(accepted))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else TABLE
    json.dump(got, open(path, "w"), indent=0, sort_keys=True)
    print(f"{len(got)} refusals recorded in {path}")
