"""Host logic of anscombe= in the two 1-D engines (denoise_signals / denoise_along), checked without a device: the
keyword and its place in the signatures, the four ..._ex entries in the header, the built library and the binding with
their refusals of a null handle and of unknown flag bits, the routing of ineligible inputs to the per-signal loop or the
transposed route with anscombe=True handed on (and NOT handed on when it is off: the calls as they always were), and
argument errors raised before any device work."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import along as A
from wavelets_amd import signals as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"wt_signals_decompose_ex": 4, "wt_signals_denoise_sum_ex": 7, "wt_along_abs_median_ex": 3, "wt_along_denoise_ex": 7}


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


# ---------------------------------------------------------------- the keyword

def test_the_keyword_is_last_and_off_by_default():
    for fn, names in ((W.denoise_signals, ["signals", "weights", "scaling_function", "noise", "soft_threshold", "out", "anscombe"]),
                      (W.denoise_along, ["a", "weights", "scaling_function", "axis", "noise", "soft_threshold", "out", "anscombe"])):
        par = inspect.signature(fn).parameters
        assert list(par) == names
        assert par["anscombe"].default is False
    for cls, methods in ((L.SignalBatch, ("decompose", "denoise_sum")), (L.AlongBatch, ("abs_median", "denoise"))):
        for m in methods:
            par = inspect.signature(getattr(cls, m)).parameters
            assert list(par)[-1] == "anscombe" and par["anscombe"].default is False, (cls.__name__, m)


# ---------------------------------------------------------------- header, exports, binding, refusals

def test_header_declares_and_library_exports_the_entries():
    txt = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m and len(m.group(1).split(",")) == nargs and m.group(1).split(",")[-1].strip() == "int flags", name
        assert hasattr(lib, name), name
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and args[-1] is ctypes.c_int, name
        assert L.SIGNATURES[name[:-3]][1] == args[:-1], name              # the old entry's arguments, then the flags
        # the comment right above the declaration names the reference lines
        head = txt[:txt.index("int " + name + "(")]
        assert "watroo/" in head[head.rindex("/*"):], name
    assert L.LINES_ANSCOMBE == 1
    assert L.load().wt_abi_version() == 8


def test_raw_entries_refuse_a_null_handle_and_unknown_flag_bits():
    lib = L.load()
    dp = ctypes.POINTER(ctypes.c_double)()
    buf = (ctypes.c_double * 8)()
    calls = {"wt_signals_decompose_ex": lambda f: lib.wt_signals_decompose_ex(None, 1, 1, f),
             "wt_signals_denoise_sum_ex": lambda f: lib.wt_signals_denoise_sum_ex(None, 1, 0, dp, dp, 1, f),
             "wt_along_abs_median_ex": lambda f: lib.wt_along_abs_median_ex(None, ctypes.cast(buf, ctypes.c_void_p), f),
             "wt_along_denoise_ex": lambda f: lib.wt_along_denoise_ex(None, 1, 0, dp, dp, 1, f)}
    for name, call in calls.items():
        for flags in (0, 1, 2):
            assert call(flags) != 0, (name, flags)
            with pytest.raises(L.WatrooHipError, match=name + ": null"):
                L.check(call(flags))
    # a live handle would need a device; the flag rule itself is host logic and is the first check behind the handle:
    # the source of both units refuses any bit but bit 0 through the one shared rule
    host = open(os.path.join(ROOT, "wavelets_amd", "csrc", "wt_lines_host.h")).read()
    assert "flags & ~WT_LINES_ANSCOMBE" in host and "#define WT_LINES_ANSCOMBE 1" in host
    for unit, n in (("wt_signals.hip", 2), ("wt_along.hip", 2)):
        assert open(os.path.join(ROOT, "wavelets_amd", "csrc", unit)).read().count("lines_flags(flags, who)") == n


class FakeLib:
    """records the entries a binding method calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(handle, *args):
            self.calls.append((name, args))
            return 0
        return entry


def test_binding_methods_pick_the_entry_by_the_keyword(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(L, "load", lambda: fake)
    sb = object.__new__(L.SignalBatch)
    sb._h, sb.level, sb.dtype = 1, 0, np.dtype(np.float32)
    sb.decompose(3, 2)
    sb.decompose(3, 2, anscombe=True)
    sb.denoise_sum(1, [[1.0, 2.0]], [[1.0, 1.0]], True)
    sb.denoise_sum(1, [[1.0, 2.0]], [[1.0, 1.0]], False, anscombe=True)
    ab = object.__new__(L.AlongBatch)
    ab._h, ab.level, ab.dtype, ab.chunk = 1, 0, np.dtype(np.float64), (1, 2)
    ab.abs_median()
    ab.abs_median(anscombe=True)
    ab.denoise(2, np.zeros((2, 2)), [1.0, 1.0])
    ab.denoise(2, np.zeros((2, 2)), [1.0, 1.0], False, anscombe=True)
    names = [c[0] for c in fake.calls]
    assert names == ["wt_signals_decompose", "wt_signals_decompose_ex", "wt_signals_denoise_sum", "wt_signals_denoise_sum_ex",
                     "wt_along_abs_median", "wt_along_abs_median_ex", "wt_along_denoise", "wt_along_denoise_ex"]
    assert fake.calls[0][1] == (3, 2) and fake.calls[1][1] == (3, 2, 1)
    for old, new in ((2, 3), (4, 5), (6, 7)):
        assert len(fake.calls[new][1]) == len(fake.calls[old][1]) + 1 and fake.calls[new][1][-1] == 1
    sb._h = ab._h = None


# ---------------------------------------------------------------- routing

class Reached(Exception):
    pass


@pytest.fixture
def recorder(monkeypatch):
    """default_context raises (no device work may start); denoise (under denoise_signals) and denoise_signals (under
    denoise_along) record their arguments, keywords included"""
    calls = []

    def no_device(*a, **k):
        raise Reached("device")

    def one_denoise(signal, weights, scaling_function, noise, **kw):
        calls.append(("denoise", signal, weights, scaling_function, noise, kw))
        return np.zeros(len(signal), W.wavelets._result_dtype(signal))

    def signals_denoise(sig, weights, scaling_function, noise, soft_threshold, **kw):
        calls.append(("denoise_signals", sig, weights, scaling_function, noise, soft_threshold, kw))
        return np.zeros(sig.shape, W.wavelets._result_dtype(sig))
    monkeypatch.setattr(L, "default_context", no_device)
    monkeypatch.setattr(S, "denoise", one_denoise)
    monkeypatch.setattr(A, "denoise_signals", signals_denoise)
    return calls


def test_ineligible_signals_reach_the_loop_with_anscombe(recorder):
    for label, sig, sf in (("int16", np.ones((3, 64), np.int16), W.B3spline),
                           ("8193 samples", np.ones((2, 8193), np.float32), W.B3spline),
                           ("custom taps", np.ones((3, 64), np.float32), Retapped)):
        weights = [5, 3]
        del recorder[:]
        res = W.denoise_signals(sig, weights, sf, noise=[0.5] * len(sig), soft_threshold=False, anscombe=True)
        assert res.shape == sig.shape, label
        assert [c[0] for c in recorder] == ["denoise"] * len(sig), label
        for i, c in enumerate(recorder):
            assert np.shares_memory(c[1], sig[i]) and c[2] is weights and c[3] is sf and c[4] == 0.5, label
            assert c[5] == {"soft_threshold": False, "anscombe": True}, label
        del recorder[:]
        W.denoise_signals(sig, weights, sf)
        assert all(c[5] == {"soft_threshold": True} for c in recorder) and len(recorder) == len(sig), label


def test_ineligible_arrays_reach_the_signal_engine_transposed_with_anscombe(recorder):
    rng = np.random.default_rng(3)
    for label, a, sf, axis in (("513 samples", rng.random((513, 3)).astype(np.float32), W.B3spline, 0),
                               ("513 float64 samples", rng.random((2, 513, 3)), W.B3spline, 1),
                               ("int16", rng.integers(0, 100, (8, 3, 2)).astype(np.int16), W.B3spline, 0),
                               ("custom taps", rng.random((8, 6)).astype(np.float32), Retapped, 0),
                               ("the last axis", rng.random((3, 4, 16)).astype(np.float32), W.B3spline, -1)):
        moved = np.moveaxis(a, axis, -1)
        M, N = moved.size // a.shape[axis], a.shape[axis]
        weights = [5, 3]
        del recorder[:]
        res = W.denoise_along(a, weights, sf, axis=axis, noise=1.5, soft_threshold=False, anscombe=True)
        assert res.shape == a.shape and len(recorder) == 1 and recorder[0][0] == "denoise_signals", label
        _, sig, wg, f, noise, soft, kw = recorder[0]
        assert wg is weights and f is sf and noise == 1.5 and soft is False and kw == {"anscombe": True}, label
        np.testing.assert_array_equal(sig, moved.reshape(M, N))
        del recorder[:]
        W.denoise_along(a, weights, sf, axis=axis)
        assert len(recorder) == 1 and recorder[0][6] == {}, label


def test_eligible_inputs_reach_for_the_device(recorder):
    with pytest.raises(Reached):
        W.denoise_signals(np.ones((3, 64), np.float32), [5, 3], anscombe=True)
    with pytest.raises(Reached):
        W.denoise_signals(np.ones((2, 4096)), [5, 3], noise=[None, 1.0], anscombe=True)
    with pytest.raises(Reached):
        W.denoise_along(np.ones((16, 4, 6), np.float32), [5, 3], anscombe=True)
    with pytest.raises(Reached):
        W.denoise_along(np.ones((2, 512, 9)), [5, 3], axis=1, noise=np.ones((2, 9)), anscombe=True)
    assert recorder == []


def test_out_errors_come_before_any_device_work(recorder):
    for sig in (np.ones((3, 64), np.float32), np.ones((3, 64), np.int16)):         # the device route and the loop route
        res = W.wavelets._result_dtype(sig)
        other = np.float64 if res == np.float32 else np.float32
        ro = np.zeros((3, 64), res)
        ro.flags.writeable = False
        for bad in (np.zeros((3, 63), res), np.zeros((3, 64), other), np.zeros((64, 3), res).T, ro, [[0.0]]):
            with pytest.raises(ValueError, match="out:"):
                W.denoise_signals(sig, [5, 3], out=bad, anscombe=True)
    for a in (np.ones((16, 4, 6), np.float32), np.ones((16, 4, 6), np.int16)):      # the device route and the transposed route
        res = W.wavelets._result_dtype(a)
        other = np.float64 if res == np.float32 else np.float32
        for bad in (np.zeros((16, 4, 5), res), np.zeros((16, 4, 6), other), np.zeros((6, 4, 16), res).T):
            with pytest.raises(ValueError, match="out:"):
                W.denoise_along(a, [5, 3], out=bad, anscombe=True)
        with pytest.raises(ValueError, match="noise:"):
            W.denoise_along(a, [5, 3], noise=np.ones((6, 4)), anscombe=True)
    assert recorder == []
