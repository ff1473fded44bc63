"""Host logic of wavelets_amd.resident (transform_stack / denoise_stack from a device array to a device array): the
exported names, the seven additive entries of the C ABI, the parsing of __cuda_array_interface__, the truth table of
resident.eligible, and what is checked before any device work - `out`, `stream`, the choice between the device route
and the staged one.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B
from wavelets_amd import resident as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("wt_device_alloc", "wt_device_free", "wt_device_copy", "wt_batch_load_device", "wt_batch_store_device",
           "wt_batch64_load_device", "wt_batch64_store_device")
ADDR = 0x7f0000001000            # an address nothing here ever dereferences


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Fake:
    """an object that speaks the protocol and owns nothing"""

    def __init__(self, shape, dtype=np.float32, strides=None, ptr=ADDR, version=3, **more):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=np.dtype(dtype).str, data=(ptr, False),
                                             version=version, strides=strides, **more)


class Retapped(W.B3spline):
    """a built-in family with other taps: the generic route of the host functions"""
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


# ---------------------------------------------------------------------------------------------------------- names, ABI
def test_names_are_exported():
    assert W.resident is R and W.DeviceArray is R.DeviceArray
    for name in ("DeviceArray", "view", "eligible", "transform_stack", "denoise_stack"):
        assert name in R.__all__ and callable(getattr(R, name))


def test_header_library_and_binding_hold_the_seven_entries():
    txt = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"(/\*(?:(?!\*/).)*\*/)\s*\n\s*int " + name + r"\(", txt, flags=re.S)
        assert m, f"{name}: no declaration with a comment above it"
        assert "Replaces" in m.group(1), f"{name}: the comment names what the entry replaces"
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert L.load().wt_abi_version() == 8
    assert "resident" in L.unit_names() and any(src == "wt_resident.hip" for _, src, _ in entry._units())


def test_raw_entries_refuse_a_null_handle_and_name_themselves():
    lib = L.load()
    p = ctypes.c_void_p()
    st = (ctypes.c_int64 * 3)(4, 4, 4)
    calls = {"wt_device_alloc": (None, 16, ctypes.byref(p)),
             "wt_device_free": (None, ADDR),
             "wt_device_copy": (None, ADDR, ADDR, 16, L.COPY_DEVICE_TO_DEVICE),
             "wt_batch_load_device": (None, L.PLANE_INPUT, 0, 1, ADDR, 9, st, None, 0),
             "wt_batch_store_device": (None, L.PLANE_OUT, 0, 1, ADDR, st, None, 0),
             "wt_batch64_load_device": (None, L.PLANE_INPUT, 0, 1, ADDR, 10, st, None, 0),
             "wt_batch64_store_device": (None, L.PLANE_OUT, 0, 1, ADDR, st, None, 0)}
    assert sorted(calls) == sorted(ENTRIES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        assert lib.wt_last_error().decode().startswith(name + ":"), (name, lib.wt_last_error())


def test_stream_arg():
    assert L.stream_arg(None) == (None, L.STREAM_NONE)
    assert L.stream_arg(1) == (None, L.STREAM_LEGACY) and L.stream_arg(2) == (None, L.STREAM_PER_THREAD)
    h, kind = L.stream_arg(0x5500)
    assert h.value == 0x5500 and kind == L.STREAM_HANDLE
    assert L.stream_arg(0) == (None, L.STREAM_LEGACY)                  # the null hipStream_t: the legacy default stream
    for bad in (True, False, -1, 1.0, "1"):
        with pytest.raises(ValueError, match="stream"):
            L.stream_arg(bad)


# ---------------------------------------------------------------------------------------------------- the interface
def test_interface_versions_and_strides():
    for version in (2, 3):
        d = R._describe(Fake((2, 5, 7), version=version))
        assert (d.ptr, d.shape, d.dtype, d.strides, d.stream) == (ADDR, (2, 5, 7), np.dtype(np.float32), (140, 28, 4), None)
    d = R._describe(Fake((2, 5, 7), np.int16, strides=(200, 20, 2), stream=2))
    assert d.strides == (200, 20, 2) and d.stream == 2 and not d.c_contiguous
    for version in (None, 0, 1, 4):
        with pytest.raises(ValueError, match="version"):
            R._describe(Fake((2, 5, 7), version=version))


def test_interface_refusals():
    for obj in (np.zeros((2, 3, 4), np.float32), [[1.0]], None, 3):
        with pytest.raises(TypeError, match="__cuda_array_interface__"):
            R.eligible(obj, 2)
    with pytest.raises(ValueError, match="null device pointer"):
        R.eligible(Fake((2, 5, 7), ptr=0), 2)
    assert R._describe(Fake((0, 5, 7), ptr=0)).size == 0              # (an empty array may have no block)
    for shape in ((5, 7), (1, 2, 5, 7), (7,)):
        with pytest.raises(ValueError, match=r"\(N, H, W\)"):
            R.eligible(Fake(shape), 2)
    for dt in (np.complex64, np.complex128):
        with pytest.raises(ValueError, match="complex"):
            R.eligible(Fake((2, 5, 7), dt), 2)
    with pytest.raises(TypeError):
        R.view(1.5, (2, 5, 7), np.float32)


def test_view_and_device_array_descriptions():
    v = R.view(ADDR, (2, 5, 7), np.float64, (560, 56, 8))
    assert R._describe(v) is v and v.extent() == (0, 560 + 4 * 56 + 6 * 8 + 8)
    assert R.view(ADDR, (3, 4, 5), np.uint8).strides == (20, 5, 1)
    neg = R.view(ADDR, (2, 5, 7), np.float32, (140, -28, 4))
    assert neg.extent() == (-4 * 28, 140 + 6 * 4 + 4)
    d = R.DeviceArray(ADDR, (2, 3, 4), np.float32, None)              # (described, never allocated nor freed)
    cai = d.__cuda_array_interface__
    assert cai == {"shape": (2, 3, 4), "typestr": "<f4", "data": (ADDR, False), "version": 3, "strides": None}
    assert d.strides == (48, 16, 4) and d.nbytes == 96 and d.ndim == 3
    d.ptr = 0                                                         # (so that __del__ has nothing to release)


# ------------------------------------------------------------------------------------------------------- eligible
def test_eligible_accepted_types_agree_with_the_batch_predicates():
    shape = (3, 40, 50)
    for dt in (np.float32, np.float64, np.uint8, np.int16, np.uint16, np.int32):
        assert R.eligible(Fake(shape, dt), 2), dt
        assert R.eligible(R.view(ADDR, shape, dt), 3, W.Triangle), dt
        host = np.zeros(shape, np.float32 if dt is np.uint8 else dt)  # (uint8 is served in float32, widened on the way in)
        for level in (1, 2, 5, 8, 9):
            want = B.batch_eligible(host, level) or B.batch64_eligible(host, level)
            assert R.eligible(Fake(shape, dt), level) == want, (dt, level)
    assert R._route(R._frames(Fake(shape, np.float32)), 2, W.B3spline, ()) is False
    assert R._route(R._frames(Fake(shape, np.uint8)), 2, W.B3spline, ()) is False
    for dt in (np.float64, np.int16, np.uint16, np.int32):
        assert R._route(R._frames(Fake(shape, dt)), 2, W.B3spline, ()) is True


def test_eligible_refuses_what_is_staged():
    shape = (3, 40, 50)
    for dt in (np.float16, ">f4", ">f8", np.int64, np.uint32, np.int8, np.bool_):
        assert not R.eligible(Fake(shape, dt), 2), dt
    assert not R.eligible(Fake(shape, strides=(8000, -200, 4)), 2)                  # a negative stride
    assert not R.eligible(Fake(shape, strides=(8000, 200, 0)), 2)                   # a zero stride
    assert not R.eligible(Fake(shape, strides=(8002, 200, 4)), 2)                   # no multiple of the itemsize
    assert not R.eligible(Fake(shape, np.float64, strides=(16000, 400, 12)), 2)
    assert R.eligible(Fake(shape, strides=(16000, 400, 8)), 2)                      # pitched, inner stride 2
    assert not R.eligible(Fake(shape), 2, Retapped)                                 # custom taps
    assert not R.eligible(Fake(shape), 0) and not R.eligible(Fake(shape), 99)       # levels outside the engine
    assert not R.eligible(Fake(shape, np.float64), 0) and not R.eligible(Fake(shape, np.float64), 99)
    assert not R.eligible(Fake(shape), True) and not R.eligible(Fake(shape, np.float64), 2.0)
    assert not R.eligible(Fake((0, 40, 50), ptr=0), 2)                              # an empty stack
    assert R.eligible(Fake(shape), 2, noise_per_frame=[None, 1.0, 2])
    assert not R.eligible(Fake(shape), 2, noise_per_frame=[None, np.ones((40, 50)), 2])   # a noise map


# --------------------------------------------------------------------------------- what comes before any device work
class Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """default_context raises (no device work may start); the staged route's download records the stack it was given"""
    staged = []

    def reach(*a, **k):
        raise Reached

    def download(d):
        staged.append(d)
        raise Reached("staged")

    monkeypatch.setattr(L, "default_context", reach)
    monkeypatch.setattr(R, "_download", download)
    return staged


def test_bad_out_is_refused_before_any_device_work(no_device):
    fr = Fake((3, 40, 50))
    cases = [(lambda o: R.transform_stack(fr, 2, out=o), (3, 3, 40, 50)), (lambda o: R.denoise_stack(fr, [5, 3], out=o), (3, 40, 50))]
    for call, shape in cases:
        st = R._c_strides(shape, 4)
        bad = [Fake(shape[:-1] + (shape[-1] + 1,)), Fake(shape[1:]), Fake(shape, np.float64), Fake(shape, ">f4"),
               Fake(shape, strides=st[:-2] + (-st[-2], 4)), Fake(shape, strides=st[:-1] + (6,)), Fake(shape, ptr=0),
               np.zeros(shape, np.float32), object()]
        for o in bad:
            with pytest.raises(ValueError, match=r"^out: "):
                call(o)
        with pytest.raises(Reached):                                   # a good one goes on to the device
            call(Fake(shape, strides=st[:-2] + (2 * st[-2], 4)))
    with pytest.raises(ValueError, match=r"^out: "):                   # the element type of the result, not of the frames
        R.denoise_stack(Fake((3, 40, 50), np.int16), [5, 3], out=Fake((3, 40, 50), np.int16))
    with pytest.raises(ValueError, match=r"^out: "):
        R.denoise_stack(Fake((3, 40, 50), np.uint8), [5, 3], out=Fake((3, 40, 50), np.float64))
    assert not no_device


def test_bad_stream_is_refused_before_any_device_work(no_device):
    fr = Fake((3, 40, 50))
    for bad in (True, -1, 2.0):
        with pytest.raises(ValueError, match="stream"):
            R.transform_stack(fr, 2, stream=bad)
        with pytest.raises(ValueError, match="stream"):
            R.denoise_stack(fr, [5, 3], stream=bad)
    with pytest.raises(ValueError, match="stream"):                    # ... the interface's own entry as well
        R.denoise_stack(Fake((3, 40, 50), stream=-3), [5, 3])
    for good in (None, 0, 1, 2, 0x5500):
        with pytest.raises(Reached):
            R.transform_stack(fr, 2, stream=good)
    assert not no_device


def test_eligible_calls_reach_for_the_device_and_the_others_are_staged(no_device):
    for dt in (np.float32, np.float64, np.uint8, np.int16, np.uint16, np.int32):
        fr = Fake((3, 40, 50), dt)
        for call in (lambda: R.transform_stack(fr, 2), lambda: R.denoise_stack(fr, [5, 3]),
                     lambda: R.denoise_stack(fr, [5, 3], W.Triangle, [None, 1.0, 2], False, True)):
            with pytest.raises(Reached) as e:
                call()
            assert not e.value.args and not no_device, dt
    staged = [lambda: R.transform_stack(Fake((3, 40, 50)), 2, Retapped),
              lambda: R.transform_stack(Fake((3, 40, 50), np.float16), 2),
              lambda: R.transform_stack(Fake((3, 40, 50), ">f4"), 2),
              lambda: R.transform_stack(Fake((3, 40, 50)), 12),
              lambda: R.transform_stack(Fake((3, 40, 50), strides=(8000, -200, 4)), 2),
              lambda: R.denoise_stack(Fake((3, 40, 50)), [5, 3], noise=np.ones((40, 50))),
              lambda: R.denoise_stack(Fake((3, 40, 50), np.int64), [5, 3])]
    for i, call in enumerate(staged):
        with pytest.raises(Reached, match="staged"):
            call()
        assert len(no_device) == i + 1 and no_device[-1].shape == (3, 40, 50)


def test_host_functions_keep_their_routing_of_device_arrays(no_device):
    """the host functions are not widened: a device array is no ndarray to them"""
    assert not B.batch_eligible(Fake((3, 40, 50)), 2) and not B.batch64_eligible(Fake((3, 40, 50), np.float64), 2)
