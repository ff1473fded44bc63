"""Host logic of the axis engine (wt_along: transform_along / denoise_along), checked without a device: the clauses of
along_eligible one by one, wt_along_ok at the edges of its LDS budget, the tile and chunk rules, the vectorised
threshold table against the per-signal rule row by row, the routing (the last axis to the signal engine, ineligible
inputs to the transposed route with their arguments passed through, eligible inputs to the device), argument errors
raised before any device work, and the header, the exports and the Python binding of the ten new entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import along as A
from wavelets_amd.wavelets import _tau_row, _noise_from_median, _interleave_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["wt_along_ok", "wt_along_create", "wt_along_destroy", "wt_along_info", "wt_along_upload", "wt_along_decompose",
           "wt_along_abs_median", "wt_along_denoise", "wt_along_download_planes", "wt_along_download_sum"]


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


class SixTaps(W.B3spline):
    coefficients_1d = np.ones(6) / 6


def f32(shape=(16, 4, 6)):
    return np.zeros(shape, np.float32)


# ---------------------------------------------------------------- the predicate, clause by clause

def test_eligible_types_ndim_and_axis():
    assert A.along_eligible(f32(), 3) and A.along_eligible(np.zeros((16, 4, 6)), 3) and A.along_eligible(f32(), 3, W.Triangle)
    for dt in (np.int16, ">f4", np.float16, ">f8", np.uint8, np.complex64):
        assert not A.along_eligible(np.zeros((16, 4, 6), dt), 3), dt
    assert not A.along_eligible(np.zeros(64, np.float32), 3)                       # ndim 1
    assert not A.along_eligible([[0.0, 1.0], [2.0, 3.0]], 3)
    assert A.along_eligible(f32((16, 2)), 3) and A.along_eligible(f32(), 3, axis=1) and A.along_eligible(f32(), 3, axis=-2)
    # I == 1 is not the engine's: the last axis, or trailing dimensions of one element
    assert not A.along_eligible(f32(), 3, axis=2) and not A.along_eligible(f32(), 3, axis=-1)
    assert not A.along_eligible(f32((4, 16, 1)), 3, axis=1)
    assert not A.along_eligible(f32(), 3, axis=3) and not A.along_eligible(f32(), 3, axis=-4) and not A.along_eligible(f32(), 3, axis=1.0)
    assert not A.along_eligible(f32((0, 16, 4)), 3, axis=1) and not A.along_eligible(f32((0, 4)), 3)
    assert A.along_eligible(f32((4, 16, 6))[:, :, ::2], 3, axis=1)                 # (copied once before anything else)


def test_eligible_levels_and_scaling_functions():
    assert not A.along_eligible(f32(), 0) and not A.along_eligible(f32(), 25)
    assert A.along_eligible(f32(), 1) and A.along_eligible(f32(), 24) and A.along_eligible(f32(), np.int64(5))
    assert not A.along_eligible(f32(), 3.0) and not A.along_eligible(f32(), True) and not A.along_eligible(f32(), -1)
    assert not A.along_eligible(f32(), 3, Retapped) and not A.along_eligible(f32(), 3, SixTaps)


def test_eligible_lds_budget():
    for dt in (np.float32, np.float64):
        assert A.along_eligible(np.zeros((512, 4), dt), 3) and not A.along_eligible(np.zeros((513, 4), dt), 3)
        assert A.along_eligible(np.zeros((2, 512, 4), dt), 3, axis=1) and not A.along_eligible(np.zeros((2, 513, 4), dt), 3, axis=1)


def test_eligible_noise():
    a = f32()
    assert A.along_eligible(a, 3, noise=None) and A.along_eligible(a, 3, noise=0.5) and A.along_eligible(a, 3, noise=np.float32(2))
    assert A.along_eligible(a, 3, noise=True) and A.along_eligible(a, 3, noise=np.int64(3))
    assert A.along_eligible(a, 3, noise=np.ones((4, 6))) and A.along_eligible(a, 3, noise=np.ones((4, 6), np.int32))
    assert A.along_eligible(a, 3, axis=1, noise=np.ones((16, 6), np.float32))
    assert not A.along_eligible(a, 3, noise=np.ones((6, 4))) and not A.along_eligible(a, 3, noise=np.ones(24))
    assert not A.along_eligible(a, 3, noise=np.ones((16, 4, 6)))
    assert not A.along_eligible(a, 3, noise=np.ones((4, 6), np.complex64)) and not A.along_eligible(a, 3, noise=1j)
    assert not A.along_eligible(a, 3, noise="1") and not A.along_eligible(a, 3, noise=[1.0] * 24)
    assert not A.along_eligible(a, 3, noise=np.full((4, 6), "1"))


def test_along_ok_answers_without_a_device_and_agrees_with_the_predicate():
    ok = L.load().wt_along_ok
    for N, item, want in ((512, 4, 1), (513, 4, 0), (512, 8, 1), (513, 8, 0), (1, 4, 1), (1, 8, 1)):
        for fam, cls in ((L.B3SPLINE, W.B3spline), (L.TRIANGLE, W.Triangle)):
            assert ok(fam, N, 4, 6, item) == want, (N, item)
            a = np.zeros((N, 4), np.float32 if item == 4 else np.float64)
            assert A.along_eligible(a, 6, cls) is bool(want), (N, item)
    assert ok(L.B3SPLINE, 64, 4, 0, 4) == 0 and ok(L.B3SPLINE, 64, 4, 25, 4) == 0 and ok(L.B3SPLINE, 64, 4, 24, 4) == 1
    assert ok(L.B3SPLINE, 0, 4, 3, 4) == 0 and ok(L.B3SPLINE, 64, 0, 3, 4) == 0 and ok(L.B3SPLINE, 64, 1, 3, 4) == 0
    assert ok(L.B3SPLINE, 64, 4, 3, 2) == 0 and ok(7, 64, 4, 3, 4) == 0 and ok(L.B3SPLINE, 1 << 40, 4, 3, 4) == 0
    assert ok(L.B3SPLINE, 64, 2, 3, 4) == 1
    assert L.along_ok(L.B3SPLINE, 512, 4, 6, 4) and not L.along_ok((0.25, 0.5, 0.25), 64, 4, 3, 4)


def test_along_tile():
    assert L.along_tile(512, 4) == 16 and L.along_tile(512, 8) == 8 and L.along_tile(32, 4) == 256
    assert L.along_tile(1, 4) == 256 and L.along_tile(33, 4) == 128 and L.along_tile(513, 4) == 8 and L.along_tile(0, 4) == 0
    for N in (1, 2, 31, 32, 33, 100, 256, 257, 511, 512):
        for item in (4, 8):
            ti = L.along_tile(N, item)
            assert 2 * N * ti * item <= 65536 and (ti == 256 or 2 * N * 2 * ti * item > 65536) and ti & (ti - 1) == 0
            assert ti * item >= 64                                   # N <= 512: runs of at least 64 bytes


def test_along_chunks():
    per = L.along_bytes(64, 3, 4)
    assert per == 5 * 64 * 4 + 4 and L.along_bytes(64, 3, 8, planes=False) == 2 * 64 * 8 + 8 + 2 * 3 * 8
    # whole outer slices: 10 outer indices of 100 signals, room for 250 signals -> 2 slices per chunk
    assert L.along_chunks(5, 64, 100, 3, budget=250 * per) == [(0, 2, 0, 100), (2, 2, 0, 100), (4, 1, 0, 100)]
    assert L.along_chunks(5, 64, 100, 3) == [(0, 5, 0, 100)]
    # not one outer slice fits: the inner axis in multiples of the tile (N = 128 float32: 64)
    assert L.along_tile(128, 4) == 64
    per = L.along_bytes(128, 3, 4)
    assert L.along_chunks(2, 128, 300, 3, budget=150 * per) == [(0, 1, 0, 128), (0, 1, 128, 128), (0, 1, 256, 44),
                                                                  (1, 1, 0, 128), (1, 1, 128, 128), (1, 1, 256, 44)]
    assert L.along_chunks(1, 128, 130, 3, budget=1) == [(0, 1, 0, 64), (0, 1, 64, 64), (0, 1, 128, 2)]    # at least one tile
    assert L.along_chunks(0, 64, 100, 3) == [] and L.along_chunks(3, 64, 0, 3) == []
    assert L.along_chunks(2, 128, 300, 3, budget=150 * L.along_bytes(128, 3, 4, False), planes=False)[0] == (0, 1, 0, 128)
    assert A._chunks(5, 64, 100, 3, 4, True) == L.along_chunks(5, 64, 100, 3)
    for bad in ((-1, 64, 4), (1, -64, 4), (1, 64, -4)):
        with pytest.raises(ValueError):
            L.along_chunks(*bad, 3)


# ---------------------------------------------------------------- the threshold table

def test_tau_table_equals_the_per_signal_rule_row_by_row():
    rng = np.random.default_rng(7)
    for cls in (W.B3spline, W.Triangle):
        sigma_e = cls(1).sigma_e()
        for weights in ([5, 3], [3, 0, 1], [0, 0], [2.5, 0.0, 1, 4], [-2, 3]):
            level = len(weights)
            entries, _, _ = _interleave_split([], level, list(weights), (1,) * level)
            for soft in (True, False):
                for dt in (np.float32, np.float64):
                    med = np.abs(rng.standard_normal(300)).astype(dt)
                    med[[0, 17, 299]] = 0
                    noises = A._noise_table(med, sigma_e)
                    want = [_noise_from_median(m, sigma_e) for m in med]
                    assert noises.dtype == np.asarray(want[0]).dtype
                    np.testing.assert_array_equal(noises, np.asarray(want))
                    tab = A._tau_table(entries, noises, sigma_e, soft)
                    assert tab.shape == (300, level) and tab.dtype == np.float64
                    np.testing.assert_array_equal(tab, np.asarray([_tau_row(entries, n, sigma_e, soft) for n in want]))
                # given noise levels, 0 and a negative one among them, in several element types
                for given in (np.array([0.0, 1.5, -0.75, 2.0, 0.0, 1e-3]), np.array([0, 1.5, -0.75, 2], np.float32),
                              np.array([0, 3, -2, 1], np.int32), np.full(5, 1.25), np.full(4, np.float32(0.7), np.float32),
                              np.full(3, 2), np.array([True, False])):
                    tab = A._tau_table(entries, given, sigma_e, soft)
                    np.testing.assert_array_equal(tab, np.asarray([_tau_row(entries, n, sigma_e, soft) for n in given]).reshape(len(given), level))


# ---------------------------------------------------------------- routing

class Reached(Exception):
    pass


@pytest.fixture
def recorder(monkeypatch):
    """default_context raises (no device work may start), the signal engine's entries record their arguments"""
    calls = []

    def no_device(*a, **k):
        raise Reached("device")

    def signals_transform(sig, level, scaling_function=W.B3spline, out=None):
        calls.append(("transform", sig, level, scaling_function))
        return np.arange(sig.shape[0] * (level + 1) * sig.shape[1], dtype=W.wavelets._result_dtype(sig)).reshape(
            sig.shape[0], level + 1, sig.shape[1])

    def signals_denoise(sig, weights, scaling_function=W.B3spline, noise=None, soft_threshold=True, out=None):
        calls.append(("denoise", sig, weights, scaling_function, noise, soft_threshold))
        return np.arange(sig.size, dtype=W.wavelets._result_dtype(sig)).reshape(sig.shape)
    monkeypatch.setattr(L, "default_context", no_device)
    monkeypatch.setattr(A, "transform_signals", signals_transform)
    monkeypatch.setattr(A, "denoise_signals", signals_denoise)
    return calls


def ineligible_inputs():
    rng = np.random.default_rng(3)
    return [("513 samples", rng.standard_normal((513, 3)).astype(np.float32), 3, W.B3spline, 0),
            ("513 float64 samples", rng.standard_normal((2, 513, 3)), 3, W.B3spline, 1),
            ("int16", rng.integers(0, 100, (8, 3, 2)).astype(np.int16), 2, W.B3spline, 0),
            (">f4", rng.standard_normal((8, 6)).astype(">f4"), 2, W.Triangle, 0),
            ("custom taps", rng.standard_normal((8, 6)).astype(np.float32), 2, Retapped, 0),
            ("level 25", rng.standard_normal((8, 6)).astype(np.float32), 25, W.B3spline, 0)]


def test_ineligible_inputs_reach_the_signal_engine_transposed_with_their_arguments(recorder):
    for label, a, level, sf, axis in ineligible_inputs():
        del recorder[:]
        moved = np.moveaxis(a, axis, -1)
        M, N = moved.size // a.shape[axis], a.shape[axis]
        res = W.transform_along(a, level, sf, axis=axis)
        assert len(recorder) == 1 and recorder[0][0] == "transform", label
        _, sig, lv, f = recorder[0]
        assert sig.shape == (M, N) and sig.dtype == a.dtype and lv == level and f is sf, label
        np.testing.assert_array_equal(sig, moved.reshape(M, N))
        assert res.shape == (level + 1,) + a.shape and res.flags.c_contiguous, label
        fake = np.arange(M * (level + 1) * N, dtype=res.dtype).reshape(M, level + 1, N)
        for s in (0, level):
            np.testing.assert_array_equal(res[s], np.moveaxis(fake[:, s].reshape(moved.shape), -1, axis), err_msg=label)
        if level > 15:
            continue
        del recorder[:]
        weights = [5, 3, 1][:level]
        noise = np.arange(M, dtype=np.float64).reshape(moved.shape[:-1])
        res = W.denoise_along(a, weights, sf, axis=axis, noise=noise, soft_threshold=False)
        assert len(recorder) == 1 and recorder[0][0] == "denoise", label
        _, sig, wg, f, per, soft = recorder[0]
        assert wg is weights and f is sf and soft is False and list(per) == list(range(M)), label
        np.testing.assert_array_equal(sig, moved.reshape(M, N))
        np.testing.assert_array_equal(res, np.moveaxis(np.arange(M * N, dtype=res.dtype).reshape(moved.shape), -1, axis))
    # 16 planes and more, complex and string noise: the transposed route, the noise handed through
    a = np.zeros((8, 6), np.float32)
    for kw in (dict(weights=[1] * 16), dict(weights=[5, 3], noise=1j), dict(weights=[5, 3], noise="1")):
        del recorder[:]
        W.denoise_along(a, kw["weights"], noise=kw.get("noise"))
        assert len(recorder) == 1 and recorder[0][4] is kw.get("noise") or recorder[0][4] == kw.get("noise")


def test_the_last_axis_goes_to_the_signal_engine(recorder):
    a = np.random.default_rng(5).standard_normal((3, 4, 16)).astype(np.float32)
    for axis in (2, -1):
        del recorder[:]
        res = W.transform_along(a, 2, axis=axis)
        assert len(recorder) == 1 and recorder[0][1].shape == (12, 16) and res.shape == (3, 3, 4, 16)
        np.testing.assert_array_equal(recorder[0][1], a.reshape(12, 16))
        del recorder[:]
        assert W.denoise_along(a, [5, 3], axis=axis, noise=0.5).shape == a.shape
        assert len(recorder) == 1 and recorder[0][0] == "denoise" and recorder[0][4] == 0.5
    del recorder[:]
    W.transform_along(np.zeros((4, 16, 1), np.float32), 2, axis=1)                # I == 1 behind a dimension of one
    assert len(recorder) == 1 and recorder[0][1].shape == (4, 16)


def test_eligible_inputs_reach_for_the_device_and_make_no_signal_call(recorder):
    for a, axis in ((f32(), 0), (np.zeros((16, 4, 6)), 1), (f32((512, 40)), 0), (np.zeros((2, 512, 9)), -2),
                    (f32((4, 16, 6))[:, :, ::2], 1)):
        with pytest.raises(Reached):
            W.transform_along(a, 3, axis=axis)
        for noise in (None, 1.0, np.ones(np.delete(a.shape, axis))):
            with pytest.raises(Reached):
                W.denoise_along(a, [5, 3], axis=axis, noise=noise)
    assert recorder == []


# ---------------------------------------------------------------- argument errors, before device work

def test_argument_errors(recorder):
    for axis in (3, -4, 1.5, None):
        with pytest.raises(ValueError, match="axis"):
            W.transform_along(f32(), 2, axis=axis)
        with pytest.raises(ValueError, match="axis"):
            W.denoise_along(f32(), [5, 3], axis=axis)
    with pytest.raises(ValueError, match="two dimensions"):
        W.transform_along(np.zeros(16, np.float32), 2)
    with pytest.raises(ValueError, match="two dimensions"):
        W.denoise_along([[1.0, 2.0]], [5, 3])
    for a in (f32(), np.zeros((16, 4, 6), np.int16)):                 # the device route and the transposed route
        with pytest.raises(ValueError, match="noise:"):
            W.denoise_along(a, [5, 3], noise=np.ones((6, 4)))
        with pytest.raises(ValueError, match="noise:"):
            W.denoise_along(a, [5, 3], axis=1, noise=np.ones((4, 6)))
        res = W.wavelets._result_dtype(a)
        other = np.float64 if res == np.float32 else np.float32
        for bad in (np.zeros((3, 16, 4, 6), res), np.zeros((4, 16, 4, 5), res), np.zeros((4, 16, 4, 6), other),
                    np.zeros((4, 16, 4, 12), res)[..., ::2], [[0.0]]):
            with pytest.raises(ValueError, match="out:"):
                W.transform_along(a, 3, out=bad)
        ro = np.zeros((16, 4, 6), res)
        ro.flags.writeable = False
        for bad in (np.zeros((16, 4, 5), res), np.zeros((16, 4, 6), other), np.zeros((6, 4, 16), res).T, ro):
            with pytest.raises(ValueError, match="out:"):
                W.denoise_along(a, [5, 3], out=bad)
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
    assert "typedef struct wt_along wt_along;" in code
    assert "along" in L.unit_names()
    assert L.load().wt_abi_version() == 8
    for name in ("transform_along", "denoise_along", "along_eligible"):
        assert getattr(W, name) is getattr(A, name)
    assert not issubclass(L.AlongBatch, L._BatchBase)
