"""Host logic of the signal engine (wt_signals: transform_signals / denoise_signals), checked without a device: the
clauses of signals_eligible one by one, the routing of ineligible inputs to the per-signal loop with their arguments
passed through, argument errors raised before any device work, the header, the exports and the Python binding of the
new entries, wt_signals_ok at the edges of its LDS budget, and the public methods of the three older batch classes."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import signals as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["wt_signals_ok", "wt_signals_create", "wt_signals_destroy", "wt_signals_info", "wt_signals_upload",
           "wt_signals_decompose", "wt_signals_abs_median", "wt_signals_denoise_sum", "wt_signals_download_planes",
           "wt_signals_download_sum"]


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


class SixTaps(W.B3spline):
    coefficients_1d = np.ones(6) / 6


def f32(M=3, N=64):
    return np.zeros((M, N), np.float32)


def ineligible_inputs():
    """(label, signals, level, scaling function, noise) of inputs the per-signal loop serves"""
    return [("level 0", f32(), 0, W.B3spline, None),
            ("level 25", f32(), 25, W.B3spline, None),
            ("8193 float32 samples", f32(2, 8193), 3, W.B3spline, None),
            ("4097 float64 samples", np.zeros((2, 4097)), 3, W.B3spline, None),
            ("custom taps", f32(), 3, Retapped, None),
            ("generic taps", f32(), 3, SixTaps, None),
            ("a noise array", f32(), 3, W.B3spline, [np.ones(64), None, 1.0]),
            ("int16", np.zeros((3, 64), np.int16), 3, W.B3spline, None),
            (">f4", np.zeros((3, 64), ">f4"), 3, W.B3spline, None)]


# ---------------------------------------------------------------- the predicate, clause by clause

def test_eligible_types_and_ndim():
    assert S.signals_eligible(f32(), 3) and S.signals_eligible(np.zeros((3, 64)), 3)
    assert S.signals_eligible(f32(), 3, W.Triangle)
    for dt in (np.int16, ">f4", ">f8", np.float16, np.uint8, np.int32, np.complex64):
        assert not S.signals_eligible(np.zeros((3, 64), dt), 3), dt
    assert not S.signals_eligible(np.zeros(64, np.float32), 3)
    assert not S.signals_eligible(np.zeros((3, 1, 64), np.float32), 3)
    assert not S.signals_eligible([np.zeros(64, np.float32)] * 3, 3)            # (a list is stacked first)
    assert not S.signals_eligible(np.zeros((0, 64), np.float32), 3)
    assert not S.signals_eligible(np.zeros((3, 0), np.float32), 3)
    assert S.signals_eligible(np.zeros((1, 1), np.float32), 1)


def test_eligible_levels():
    assert not S.signals_eligible(f32(), 0) and not S.signals_eligible(f32(), 25)
    assert S.signals_eligible(f32(), 1) and S.signals_eligible(f32(), 24) and S.signals_eligible(f32(), np.int64(5))
    assert not S.signals_eligible(f32(), 3.0) and not S.signals_eligible(f32(), True) and not S.signals_eligible(f32(), -1)


def test_eligible_lds_budget():
    assert S.signals_eligible(f32(2, 8192), 3) and not S.signals_eligible(f32(2, 8193), 3)
    assert S.signals_eligible(np.zeros((2, 4096)), 3) and not S.signals_eligible(np.zeros((2, 4097)), 3)


def test_eligible_scaling_functions_and_noise():
    assert not S.signals_eligible(f32(), 3, Retapped) and not S.signals_eligible(f32(), 3, SixTaps)
    assert S.signals_eligible(f32(), 3, noise_per_signal=[None, 0.5, np.float32(2)])
    assert S.signals_eligible(f32(), 3, noise_per_signal=[1, True, np.int64(3)])
    assert not S.signals_eligible(f32(), 3, noise_per_signal=[None, np.ones(64), 1.0])
    assert not S.signals_eligible(f32(), 3, noise_per_signal=[np.array(1.0), None, None])     # a 0-d array is an array
    assert not S.signals_eligible(f32(), 3, noise_per_signal=[None, "1", None])
    assert not S.signals_eligible(f32(), 3, noise_per_signal=[None, 1j, None])
    assert not S.signals_eligible(f32(), 3, noise_per_signal=None)
    for label, sig, level, sf, noise in ineligible_inputs():
        per = [None] * len(sig) if noise is None else noise
        assert not S.signals_eligible(sig, level, sf, per), label


# ---------------------------------------------------------------- routing

class Reached(Exception):
    pass


@pytest.fixture
def recorder(monkeypatch):
    """default_context raises (no device work may start), the per-signal calls record their arguments"""
    calls = []

    def no_device(*a, **k):
        raise Reached("device")

    def one_transform(signal, level, scaling_function):
        calls.append(("transform", signal, level, scaling_function))
        return np.zeros((max(level, 0) + 1, len(signal)), W.wavelets._result_dtype(signal))

    def one_denoise(signal, weights, scaling_function, noise, soft_threshold=True):
        calls.append(("denoise", signal, weights, scaling_function, noise, soft_threshold))
        return np.zeros(len(signal), W.wavelets._result_dtype(signal))
    monkeypatch.setattr(L, "default_context", no_device)
    monkeypatch.setattr(S, "_transform_one", one_transform)
    monkeypatch.setattr(S, "denoise", one_denoise)
    return calls


def test_ineligible_inputs_run_the_loop_with_their_arguments(recorder):
    for label, sig, level, sf, noise in ineligible_inputs():
        del recorder[:]
        M, N = sig.shape
        if noise is None:
            res = W.transform_signals(sig, level, sf)
            assert res.shape == (M, level + 1, N), label
            assert [c[0] for c in recorder] == ["transform"] * M, label
            for i, c in enumerate(recorder):
                assert c[1].base is sig and np.shares_memory(c[1], sig[i]) and c[2] == level and c[3] is sf, label
        if level == 0:
            continue
        del recorder[:]
        weights = [5, 3, 1][:level] if level <= 3 else [1] * level
        res = W.denoise_signals(sig, weights, sf, noise=noise, soft_threshold=False)
        assert res.shape == (M, N), label
        assert [c[0] for c in recorder] == ["denoise"] * M, label
        for i, c in enumerate(recorder):
            assert np.shares_memory(c[1], sig[i]) and c[2] is weights and c[3] is sf and c[5] is False, label
            assert c[4] is (None if noise is None else noise[i]), label
    # a noise array (a per-sample map of denoise()) goes whole to every signal; 16 planes and more: the loop
    del recorder[:]
    amap = np.ones(64)
    W.denoise_signals(f32(), [5, 3], noise=amap)
    assert len(recorder) == 3 and all(c[4] is amap for c in recorder)
    del recorder[:]
    W.denoise_signals(f32(), [1] * 16)
    assert len(recorder) == 3
    # sequences of mixed element types: the loop, signal by signal
    del recorder[:]
    mixed = [np.zeros(8, np.float32), np.zeros(8, np.float64)]
    assert W.transform_signals(mixed, 2).shape == (2, 3, 8) and len(recorder) == 2


def test_eligible_inputs_make_no_per_signal_call_and_reach_for_the_device(recorder):
    for sig in (f32(), np.zeros((3, 64)), [np.zeros(64, np.float32)] * 3, f32(2, 8192), np.zeros((2, 4096))):
        with pytest.raises(Reached):
            W.transform_signals(sig, 3)
        with pytest.raises(Reached):
            W.denoise_signals(sig, [5, 3], noise=[None, 1.0, 2][:len(sig)])
    assert recorder == []


# ---------------------------------------------------------------- argument errors, before device work

def test_argument_errors(recorder):
    with pytest.raises(ValueError, match="one length"):
        W.transform_signals([np.zeros(8, np.float32), np.zeros(9, np.float32)], 2)
    with pytest.raises(ValueError, match="one length"):
        W.denoise_signals([np.zeros(8), np.zeros(9)], [5, 3])
    with pytest.raises(ValueError, match="1-D"):
        W.transform_signals([np.zeros((2, 8), np.float32)], 2)
    with pytest.raises(ValueError, match="non-empty"):
        W.transform_signals(np.zeros((2, 3, 8), np.float32), 2)
    with pytest.raises(ValueError, match="empty"):
        W.transform_signals([], 2)
    with pytest.raises(ValueError, match="one entry per signal"):
        W.denoise_signals(f32(), [5, 3], noise=[None, 1.0])
    for sig in (f32(), np.zeros((3, 64), np.int16)):                  # the device route and the loop route
        res = W.wavelets._result_dtype(sig)
        other = np.float64 if res == np.float32 else np.float32
        for bad in (np.zeros((3, 4, 63), res), np.zeros((3, 3, 64), res), np.zeros((3, 4, 64), other),
                    np.zeros((3, 4, 128), res)[:, :, ::2], [[0.0]]):
            with pytest.raises(ValueError, match="out:"):
                W.transform_signals(sig, 3, out=bad)
        for bad in (np.zeros((3, 63), res), np.zeros((4, 64), res), np.zeros((3, 64), other), np.zeros((64, 3), res).T):
            with pytest.raises(ValueError, match="out:"):
                W.denoise_signals(sig, [5, 3], out=bad)
        ro = np.zeros((3, 64), res)
        ro.flags.writeable = False
        with pytest.raises(ValueError, match="out:"):
            W.denoise_signals(sig, [5, 3], out=ro)
    assert recorder == []


# ---------------------------------------------------------------- header, exports, binding

def test_header_declares_and_library_exports_the_entries():
    txt = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert "typedef struct wt_signals wt_signals;" in code
    assert "signals" in L.unit_names()
    for name in ("transform_signals", "denoise_signals", "signals_eligible"):
        assert getattr(W, name) is getattr(S, name)


def test_signals_ok_answers_without_a_device_and_agrees_with_the_predicate():
    ok = L.load().wt_signals_ok
    for N, item, want in ((8192, 4, 1), (8193, 4, 0), (4096, 8, 1), (4097, 8, 0)):
        for fam, cls in ((L.B3SPLINE, W.B3spline), (L.TRIANGLE, W.Triangle)):
            assert ok(fam, N, 6, item) == want, (N, item)
            sig = np.zeros((2, N), np.float32 if item == 4 else np.float64)
            assert S.signals_eligible(sig, 6, cls) is bool(want), (N, item)
    assert ok(L.B3SPLINE, 64, 0, 4) == 0 and ok(L.B3SPLINE, 64, 25, 4) == 0 and ok(L.B3SPLINE, 64, 24, 4) == 1
    assert ok(L.B3SPLINE, 0, 3, 4) == 0 and ok(L.B3SPLINE, 64, 3, 2) == 0 and ok(7, 64, 3, 4) == 0
    assert ok(L.B3SPLINE, 1 << 40, 3, 4) == 0
    assert L.signals_ok(L.B3SPLINE, 8192, 6, 4) and not L.signals_ok((0.25, 0.5, 0.25), 64, 3, 4)


def test_signal_chunks():
    per = L.signal_bytes(4096, 6)
    assert per == (6 + 3) * 4096 * 4 and L.signal_bytes(4097, 6, 8) == 9 * 4098 * 8 and L.signal_bytes(5, 1) == 4 * 8 * 4
    assert L.signal_chunks(10, 4096, 6, budget=4 * per) == [(0, 4), (4, 4), (8, 2)]
    assert L.signal_chunks(3, 4096, 6, budget=1) == [(0, 1), (1, 1), (2, 1)]
    assert L.signal_chunks(5, 64, 3) == [(0, 5)] and L.signal_chunks(0, 64, 3) == []
    assert S._chunks(10, 4096, 6, 4) == L.signal_chunks(10, 4096, 6)
    with pytest.raises(ValueError):
        L.signal_chunks(-1, 64, 3)


# ---------------------------------------------------------------- the older batch classes keep their methods

def _public(cls):
    return sorted(n for n in dir(cls) if not n.startswith("_"))


def test_batch_classes_keep_their_public_methods():
    base = ["abs_median", "anscombe", "close", "decompose", "decompose_bilateral", "decompose_pass", "decompose_pass_sum",
            "decompose_sum", "denoise_sum", "download", "dtype", "enhance_sum", "fill", "gamma_blend", "plane_ptr",
            "plane_sum", "reduce", "replicate", "upload", "wow_scale", "wow_update"]
    rl = ["binary", "filter2d", "mrs_update", "set_psf"]
    assert _public(L.BatchPlan) == sorted(base + rl + ["fft_apply", "fft_spectrum", "fill_normal"])
    assert _public(L.BatchPlan64) == sorted(base)
    assert _public(L.RLBatchPlan64) == sorted(base + rl)
    assert not any("signal" in n for c in (L.BatchPlan, L.BatchPlan64, L.RLBatchPlan64) for n in dir(c))
    assert not issubclass(L.SignalBatch, L._BatchBase)
