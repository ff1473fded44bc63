"""Host logic of wow_signals / wow_along (wow of stacks of 1-D signals on the signal engine), checked without a device:
the exports and the two C entries, the clauses of wow_signals_eligible one by one, the routing of ineligible inputs to
the per-signal loop with the call's arguments, what wow_along hands to wow_signals, argument errors raised before any
device work, and the caller's lists left as they were."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import __graft_entry__ as entry
import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import utils as U

WS = __import__("importlib").import_module("wavelets_amd.wow_signals")      # (the package attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["wt_signals_moments", "wt_signals_wow_sum"]


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


def f32(M=3, N=64):
    return np.zeros((M, N), np.float32)


# ---------------------------------------------------------------- exports, header, binding

def test_exports_header_and_binding():
    for name in ("wow_signals", "wow_along", "wow_signals_eligible"):
        assert getattr(W, name) is getattr(WS, name)
    txt = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert callable(L.SignalBatch.moments) and callable(L.SignalBatch.wow_sum)


def test_raw_entries_refuse_a_null_stack():
    lib = L.load()
    buf = (ctypes.c_double * 4)()
    assert lib.wt_signals_moments(None, 1, buf) != 0
    assert lib.wt_signals_wow_sum(None, 1, 1, buf, buf, 1, 1, 0) != 0
    with pytest.raises(L.WatrooHipError, match="null signal stack"):
        L.check(lib.wt_signals_wow_sum(None, 1, 1, buf, buf, 1, 1, 0))


def test_the_wow_route_has_its_own_chunk_rule():
    plain = L.signal_bytes(256, 5)
    assert L.signal_bytes(256, 5, 4, wow=True) == plain + 8 * (4 * 5 + 3)
    assert L.signal_bytes(256, 5, 4, wow=False) == plain
    assert L.signal_chunks(10, 256, 5, budget=4 * plain) == [(0, 4), (4, 4), (8, 2)]                 # (unchanged)
    assert L.signal_chunks(10, 256, 5, budget=4 * plain, wow=True) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert WS._chunks(10, 256, 5, 4) == L.signal_chunks(10, 256, 5, wow=True)


# ---------------------------------------------------------------- the predicate, clause by clause

def test_eligible_element_types():
    assert WS.wow_signals_eligible(f32(), None) and WS.wow_signals_eligible(np.zeros((3, 64)), None)
    assert WS.wow_signals_eligible(f32(), None, W.Triangle) and WS.wow_signals_eligible(f32(), 2)
    for dt in (np.int16, ">f4", np.float16, np.complex64):
        assert not WS.wow_signals_eligible(np.zeros((3, 64), dt), None), dt
    assert not WS.wow_signals_eligible([np.zeros(64, np.float32)] * 3, None)
    assert not WS.wow_signals_eligible(np.zeros(64, np.float32), None)


@pytest.mark.parametrize("cls", [W.B3spline, W.Triangle])
@pytest.mark.parametrize("N", [5, 7, 8, 9, 300, 8192])
def test_scales_are_resolved_as_wow_resolves_them(cls, N, monkeypatch):
    """the engine is asked for the L that wow() would transform one signal over: signals_eligible sees that L"""
    seen = []
    real = WS._signals_family

    def spy(signals, level, *a, **k):
        seen.append(level)
        return real(signals, level, *a, **k)
    monkeypatch.setattr(WS, "_signals_family", spy)
    for n_scales in (None, 1, 3, 40):
        del seen[:]
        L0 = U._wow_scale_limit(U._wow_n_scales((N,), cls, n_scales, 0, []), cls, 1, None, [])
        got = WS.wow_signals_eligible(f32(2, N), n_scales, cls)
        assert got is (L0 >= 1), (N, n_scales, L0)
        assert seen == ([L0] if L0 >= 1 else []), (N, n_scales)
    want = int(np.round(np.log2(N) - np.log2(len(cls.coefficients_1d))))
    assert U._wow_n_scales((N,), cls, None, 0, []) == want


def test_no_scales_is_not_eligible():
    assert not WS.wow_signals_eligible(f32(2, 7), None) and WS.wow_signals_eligible(f32(2, 8), None)         # B3spline: 8 samples
    assert not WS.wow_signals_eligible(f32(2, 4), None, W.Triangle) and WS.wow_signals_eligible(f32(2, 5), None, W.Triangle)
    assert not WS.wow_signals_eligible(f32(), 0) and not WS.wow_signals_eligible(f32(), -1)
    assert not WS.wow_signals_eligible(f32(), 2.0) and not WS.wow_signals_eligible(f32(), "2")


def test_bilateral_gamma_noise_budget_and_taps():
    assert not WS.wow_signals_eligible(f32(), None, bilateral=1)
    assert not WS.wow_signals_eligible(f32(), None, h=0.5) and not WS.wow_signals_eligible(f32(), None, h=1)
    assert WS.wow_signals_eligible(f32(), None, h=0.0)
    assert WS.wow_signals_eligible(f32(), None, noise_per_signal=[None, 0.5, np.float32(2)])
    assert not WS.wow_signals_eligible(f32(), None, noise_per_signal=[None, np.ones(64), 1.0])
    assert WS.wow_signals_eligible(f32(2, 8192), None) and not WS.wow_signals_eligible(f32(2, 8193), None)
    assert WS.wow_signals_eligible(np.zeros((2, 4096)), None) and not WS.wow_signals_eligible(np.zeros((2, 4097)), None)
    assert not WS.wow_signals_eligible(f32(), None, Retapped)
    # as many denoise coefficients as the sigma_e table is long: wow() takes the whole table (ref utils.py:136-138)
    table = len(W.B3spline(1).sigma_e())
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # (the predicate does not warn)
        assert WS.wow_signals_eligible(f32(), None, denoise_coefficients=[1] * table)


# ---------------------------------------------------------------- routing

class Reached(Exception):
    pass


@pytest.fixture
def recorder(monkeypatch):
    """default_context raises (no device work may start), the per-signal wow records its arguments"""
    calls = []

    class Planes:
        def __init__(self, n):
            self.data = np.zeros((2, n), np.float32)

    def no_device(*a, **k):
        raise Reached("device")

    def one_wow(signal, **kw):
        calls.append((signal, kw))
        return np.zeros(len(signal), W.wavelets._result_dtype(signal)), Planes(len(signal))
    monkeypatch.setattr(L, "default_context", no_device)
    monkeypatch.setattr(WS, "wow", one_wow)
    return calls


def ineligible_calls():
    """(label, signals, keywords, noise) of calls the per-signal loop serves"""
    return [("int16", np.zeros((3, 64), np.int16), {}, None),
            (">f4", np.zeros((3, 64), ">f4"), {}, [None, 1.0, 2.0]),
            ("8193 float32 samples", f32(2, 8193), {}, None),
            ("4097 float64 samples", np.zeros((2, 4097)), {}, None),
            ("7 samples", f32(3, 7), {}, None),
            ("no scales", f32(), dict(n_scales=0), None),
            ("bilateral", f32(), dict(bilateral=1, bilateral_scaling=True), None),
            ("gamma", f32(), dict(h=0.5, gamma=2.0, gamma_min=0.1, gamma_max=3.0), None),
            ("custom taps", f32(), dict(scaling_function=Retapped), None),
            ("a noise array among the entries", f32(), {}, [np.ones(64), None, 1.0])]


def test_ineligible_inputs_run_the_loop_with_the_calls_arguments(recorder):
    defaults = dict(scaling_function=W.B3spline, n_scales=None, whitening=True, bilateral=None, bilateral_scaling=False,
                    soft_threshold=True, preserve_variance=False, gamma=3.2, gamma_min=None, gamma_max=None, h=0)
    for label, sig, kw, noise in ineligible_calls():
        del recorder[:]
        M, N = sig.shape
        res = W.wow_signals(sig, weights=[0.5, 2], denoise_coefficients=[5, 2], noise=noise, **kw)
        assert res.shape == (M, N) and res.dtype == W.wavelets._result_dtype(sig), label
        assert len(recorder) == M, label
        for i, (s, got) in enumerate(recorder):
            assert np.shares_memory(s, sig[i]) and s.shape == (N,), label
            assert got.pop("noise") is (None if noise is None else noise[i]), label
            assert got.pop("weights") == [0.5, 2] and got.pop("denoise_coefficients") == [5, 2], label
            assert got == {**defaults, **kw}, label
    # a per-sample noise array goes whole to every signal; the other keywords travel too
    del recorder[:]
    amap = np.ones(64)
    res, planes = W.wow_signals(f32(), noise=amap, whitening=False, soft_threshold=False, preserve_variance=True,
                                return_coefficients=True)
    assert len(recorder) == 3 and all(kw["noise"] is amap for _, kw in recorder)
    assert all(kw["whitening"] is False and kw["soft_threshold"] is False and kw["preserve_variance"] is True for _, kw in recorder)
    assert res.shape == (3, 64) and planes.shape == (3, 2, 64)
    # sequences of mixed element types: the loop, signal by signal
    del recorder[:]
    assert W.wow_signals([np.zeros(16, np.float32), np.zeros(16)]).shape == (2, 16) and len(recorder) == 2


def test_eligible_inputs_make_no_per_signal_call_and_reach_for_the_device(recorder):
    for sig in (f32(), np.zeros((3, 64)), [np.zeros(64, np.float32)] * 3, f32(2, 8192), np.zeros((2, 4096)), f32(1, 8)):
        with pytest.raises(Reached):
            W.wow_signals(sig)
        with pytest.raises(Reached):
            W.wow_signals(sig, W.Triangle, 2, [0.5, 2], False, [5, 2], [None, 1.0, 0][:len(sig)], soft_threshold=False,
                          preserve_variance=True, return_coefficients=True)
    assert recorder == []


def test_wow_along_hands_over_the_transposed_stack_and_the_flattened_noise(monkeypatch):
    calls = []

    def fake(signals, *args, **kw):
        calls.append((signals, args, kw))
        res = np.arange(signals.size, dtype=signals.dtype).reshape(signals.shape)
        return (res, np.stack([res, -res], axis=1)) if kw.get("return_coefficients") else res
    monkeypatch.setattr(WS, "wow_signals", fake)
    a = np.arange(6 * 40 * 7, dtype=np.float32).reshape(6, 40, 7)
    noise = np.arange(42, dtype=np.float64).reshape(6, 7) + 1
    res = W.wow_along(a, W.Triangle, 1, 3, [0.5], False, [5, 2], noise, None, False, False, True, 2.0, 0.1, 0.9, 0)
    sig, args, kw = calls[0]
    np.testing.assert_array_equal(sig, np.moveaxis(a, 1, -1).reshape(42, 40))
    assert sig.flags.c_contiguous
    assert args[:5] == (W.Triangle, 3, [0.5], False, [5, 2]) and args[6:] == (None, False, False, True, 2.0, 0.1, 0.9, 0)
    assert isinstance(args[5], list) and args[5] == list(noise.reshape(-1))
    assert kw == dict(return_coefficients=False)
    np.testing.assert_array_equal(res, np.moveaxis(np.arange(42 * 40, dtype=np.float32).reshape(6, 7, 40), -1, 1))
    assert res.flags.c_contiguous
    # the planes come back as (planes,) + a.shape; a negative axis; a scalar noise stays a scalar
    res, planes = W.wow_along(a, axis=-2, noise=1.5, return_coefficients=True)
    assert calls[1][1][5] == 1.5 and planes.shape == (2, 6, 40, 7)
    np.testing.assert_array_equal(planes[0], res)
    np.testing.assert_array_equal(planes[1], -res)
    # the last axis: the array itself, no copy
    b = np.zeros((5, 33), np.float32)
    W.wow_along(b, axis=1)
    assert calls[2][0] is b
    W.wow_along(a, axis=-1)
    assert calls[3][0].shape == (240, 7) and np.shares_memory(calls[3][0], a)
    out = np.empty_like(a)
    assert W.wow_along(a, axis=0, out=out) is out


# ---------------------------------------------------------------- argument handling

def test_argument_errors_come_before_device_work(recorder):
    with pytest.raises(ValueError, match="one length"):
        W.wow_signals([np.zeros(8, np.float32), np.zeros(9, np.float32)])
    with pytest.raises(ValueError, match="1-D"):
        W.wow_signals([np.zeros((2, 8), np.float32)])
    with pytest.raises(ValueError, match="non-empty"):
        W.wow_signals(np.zeros((2, 3, 8), np.float32))
    with pytest.raises(ValueError, match="one entry per signal"):
        W.wow_signals(f32(), noise=[None, 1.0])
    for sig in (f32(), np.zeros((3, 64), np.int16)):                  # the device route and the loop route
        res = W.wavelets._result_dtype(sig)
        other = np.float64 if res == np.float32 else np.float32
        for bad in (np.zeros((3, 63), res), np.zeros((4, 64), res), np.zeros((3, 64), other), np.zeros((64, 3), res).T, [[0.0]]):
            with pytest.raises(ValueError, match="out:"):
                W.wow_signals(sig, out=bad)
        ro = np.zeros((3, 64), res)
        ro.flags.writeable = False
        with pytest.raises(ValueError, match="out:"):
            W.wow_signals(sig, out=ro)
    a = np.zeros((4, 16, 5), np.float32)
    with pytest.raises(ValueError, match="noise:"):
        W.wow_along(a, axis=1, noise=np.ones((4, 16)))
    with pytest.raises(ValueError, match="out:"):
        W.wow_along(a, axis=1, out=np.zeros((4, 5, 16), np.float32))
    with pytest.raises(ValueError, match="axis"):
        W.wow_along(a, axis=3)
    with pytest.raises(ValueError, match="two dimensions"):
        W.wow_along(np.zeros(16, np.float32))
    assert recorder == []


def test_the_callers_lists_are_left_as_they_were(recorder):
    weights, dc = [0.5, 2], [5]
    for sig in (f32(), np.zeros((3, 64), np.int16)):                  # the device route (up to the device) and the loop
        try:
            W.wow_signals(sig, weights=weights, denoise_coefficients=dc)
        except Reached:
            pass
        assert weights == [0.5, 2] and dc == [5]
    # ... and the lists the loop hands to wow() are copies: what wow() does to them stays there
    for _, kw in recorder:
        assert kw["weights"] is not weights and kw["denoise_coefficients"] is not dc
    try:
        W.wow_along(np.zeros((3, 64, 2), np.float32), axis=1, weights=weights, denoise_coefficients=dc)
    except Reached:
        pass
    assert weights == [0.5, 2] and dc == [5] and W.wow_signals.__defaults__[2] == [] and W.wow_signals.__defaults__[4] == []
