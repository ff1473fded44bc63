"""enhance_stack on the MI355X (wt_batch_enhance_sum / wt_batch64_enhance_sum behind it): every batched result meets
the float64 numpy oracle first - per frame, every 2-D plane (a gray frame, a channel of a colour frame) under a bound
scaled by THAT plane's max|input|, in stacks whose neighbouring planes are nine decades apart and carry different
threshold and weight rows, so that a row or a pixel read from the wrong frame is an error of order one - and the
per-frame utils.enhance second, bit for bit.  While the batched call runs, the per-frame entry point it would fall
back to raises.  Inputs, cases, oracles and their reference-only premises (every hard-threshold comparison is over
all samples): tests/test_enhance_stack_cpu.py.

Bounds: 4 x the worst error of the per-frame utils.enhance - which this change does not touch; the batched result
is required to be the same bits - against the float64 oracle on these same inputs, measured on MI355X in units of
max|plane| (test_per_frame_enhance_against_the_oracle prints them per case):
    float32 plain      measured 2.95e-7  (gray 2 x 96 x 128, 10 scales)       -> F32_TOL     = 1.18e-6
    float32 bilateral  measured 3.06e-7  (colour 2 x 3 x 33 x 31, bilateral=1) -> F32_BIL_TOL = 1.224e-6
    float64            measured 8.46e-16 (colour 2 x 3 x 33 x 31)              -> F64_TOL     = 3.384e-15
The batched results of the same run: the same figures, case by case (they are the same bits)."""
import copy

import numpy as np
import pytest

from test_enhance_stack_cpu import (CASES, CASE_IDS, case_reference, case_kwargs, case_class, plane_errors)

pytestmark = pytest.mark.gpu

MEASURED_F32, MEASURED_F32_BIL, MEASURED_F64 = 2.95e-7, 3.06e-7, 8.46e-16
F32_TOL, F32_BIL_TOL, F64_TOL = 4 * MEASURED_F32, 4 * MEASURED_F32_BIL, 4 * MEASURED_F64
TOL = {"f32": F32_TOL, "f32_bilateral": F32_BIL_TOL, "f64": F64_TOL}


def _mods():
    import wavelets_amd as W
    from wavelets_amd import batch as B, utils as U, _lib as L
    return W, B, U, L


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    g, e = _bits(got), _bits(exp)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} samples differ in bits, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _no_fallback(monkeypatch, B):
    def refuse(*a, **k):
        raise AssertionError("enhance_stack fell back to the per-frame utils.enhance")
    monkeypatch.setattr(B, "enhance", refuse)


def _per_frame(U, frames, per, kw):
    return [U.enhance(frames[i], **copy.deepcopy(kw)) if per is None else U.enhance(frames[i], per[i], **copy.deepcopy(kw))
            for i in range(len(frames))]


def _check(c, got, frames, per, ref, U, kw):
    """oracle first (every plane under its own scale), then the per-frame call bit for bit"""
    tol = TOL[case_class(c)]
    assert got.shape == frames.shape and got.dtype == (np.float32 if c["dtype"] == np.float32 else np.float64)
    worst = max(plane_errors(got[i], ref[i], frames[i]) for i in range(c["n"]))
    print(f"{c['name']}: batched vs float64 oracle {worst:.3e} of max|plane| (bound {tol:.3e})")
    assert worst <= tol, f"{c['name']}: {worst:.3e} of max|plane| against the float64 oracle > {tol:.3e}"
    exp = _per_frame(U, frames, per, kw)
    for i in range(c["n"]):
        _same_bits(got[i], exp[i], f"{c['name']} frame {i}")


@pytest.mark.parametrize("name", CASE_IDS)
def test_enhance_stack(name, monkeypatch):
    W, B, U, L = _mods()
    c = CASES[CASE_IDS.index(name)]
    frames, noise, per, ref = case_reference(name)
    kw = case_kwargs(c, W)
    if c["chunk_frames"]:       # a budget of chunk_frames batch frames per chunk, as WATROO_HIP_BATCH_BYTES sets it
        H, Wd = c["shape"]
        level = max(len(w) for _, _, w in U._enhance_lists(3 if c["colour"] else 2, *(copy.deepcopy(kw[k]) for k in ("weights", "denoise"))))
        monkeypatch.setattr(L, "BATCH_BYTES", c["chunk_frames"] * L.batch_frame_bytes(H, Wd, level, itemsize=4 if c["dtype"] == np.float32 else 8) + 8)
    with monkeypatch.context() as m:
        _no_fallback(m, B)
        args = () if noise is None else (noise,)
        got = W.enhance_stack(frames, *args, **copy.deepcopy(kw))
    _check(c, got, frames, per, ref, U, kw)


def test_chunked_cases_run_in_three_chunks(monkeypatch):
    """the chunked cases really are three chunks: three launches of the thresholded sum per group"""
    W, B, U, L = _mods()
    for name, groups in (("gray-n7-33x31-L2-chunks", 1), ("colour-n3-17x4-L3-chunks", 1), ("colour-n2-17x4-three-levels-f64-chunks", 3)):
        c = CASES[CASE_IDS.index(name)]
        frames, noise, per, ref = case_reference(name)
        kw = case_kwargs(c, W)
        H, Wd = c["shape"]
        level = max(len(w) for _, _, w in U._enhance_lists(3 if c["colour"] else 2, *(copy.deepcopy(kw[k]) for k in ("weights", "denoise"))))
        calls = []
        cls = L.BatchPlan if c["dtype"] == np.float32 else L.BatchPlan64
        orig = cls.enhance_sum
        with monkeypatch.context() as m:
            m.setattr(L, "BATCH_BYTES", c["chunk_frames"] * L.batch_frame_bytes(H, Wd, level, itemsize=4 if c["dtype"] == np.float32 else 8) + 8)
            m.setattr(cls, "enhance_sum", lambda self, nf, *a, **k: (calls.append(nf), orig(self, nf, *a, **k))[1])
            W.enhance_stack(frames, **copy.deepcopy(kw))
        if name == "colour-n2-17x4-three-levels-f64-chunks":
            assert calls == [1] * 6, calls                 # three groups of one channel, two images, one frame per chunk
        else:
            assert len(calls) == 3 * groups and sum(calls) == c["n"] * (3 if c["colour"] else 1), calls


def test_sequence_of_frames_and_out(monkeypatch):
    """a list of frames, and `out`: float32 and float64 results land in the caller's array"""
    W, B, U, L = _mods()
    for name in ("colour-n2-17x4-L3-perchannel", "colour-n2-33x31-L3-f64", "gray-n2-5x7-L2-int16-perframe"):
        c = CASES[CASE_IDS.index(name)]
        frames, noise, per, ref = case_reference(name)
        kw = case_kwargs(c, W)
        out = np.full(frames.shape, 7, np.float32 if c["dtype"] == np.float32 else np.float64)
        with monkeypatch.context() as m:
            _no_fallback(m, B)
            args = () if noise is None else (noise,)
            got = W.enhance_stack([f for f in frames], *args, out=out, **copy.deepcopy(kw))
        assert got is out
        _check(c, got, frames, per, ref, U, kw)


def _outcome(fn):
    try:
        return fn(), None
    except Exception as e:                          # noqa: BLE001 - the outcome is compared, whatever it is
        return None, type(e)


def test_nan_frame_raises():
    """noise=None: the MAD estimate of a float32 frame that holds NaN is an error naming NaN (wt_batch_abs_median) - also
    when every sigma is 0, because enhance calls get_noise() eagerly (ref:74) and so does the batch.  Measured on MI355X:
    the per-frame float32 utils.enhance does NOT raise for such a frame (its median comes from the histogram of the
    first fused pass, which orders NaN keys above infinity), so here the stack is the stricter of the two, as
    denoise_stack has been since it exists.  On the float64 route the batch gives the per-frame outcome, an error or
    the same values (as test_gpu_batch64.test_nan_frame_has_the_per_frame_outcome holds denoise_stack to).  With the
    noise given there is no estimate: the NaN goes through, the same bits as per frame."""
    W, B, U, L = _mods()
    frames = np.array(case_reference("gray-n2-33x31-L1")[0])
    frames[1, 5, 7] = np.nan
    for kw in (dict(weights=[2.], denoise=[3]), dict(weights=[2., 1.], denoise=None)):
        with pytest.raises(L.WatrooHipError, match="NaN"):
            W.enhance_stack(frames, **kw)
    f64 = frames.astype(np.float64)
    kw = dict(weights=[2., 1.], denoise=[3, 0])
    exp, exp_err = _outcome(lambda: np.stack([U.enhance(f, **kw) for f in f64]))
    got, got_err = _outcome(lambda: W.enhance_stack(f64, **kw))
    assert got_err == exp_err, (got_err, exp_err)
    if exp is not None:
        assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(got[~np.isnan(got)], exp[~np.isnan(exp)])
    got = W.enhance_stack(frames, 1e5, weights=[2.], denoise=[3])
    exp = np.stack([U.enhance(f, 1e5, weights=[2.], denoise=[3]) for f in frames])
    assert np.isnan(got[1]).any() and np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.array_equal(got[~np.isnan(got)], exp[~np.isnan(exp)])


@pytest.mark.parametrize("name", CASE_IDS)
def test_per_frame_enhance_against_the_oracle(name):
    """where the bounds come from: the per-frame utils.enhance against the float64 oracle on the cases' inputs (the
    figures in this file's header are the worst of these per class), under the bound of the batched result"""
    W, B, U, L = _mods()
    c = CASES[CASE_IDS.index(name)]
    frames, noise, per, ref = case_reference(name)
    exp = _per_frame(U, frames, per, case_kwargs(c, W))
    worst = max(plane_errors(exp[i], ref[i], frames[i]) for i in range(c["n"]))
    print(f"MEASURE {case_class(c)} {name} {worst:.4e}")
    assert worst <= TOL[case_class(c)]
