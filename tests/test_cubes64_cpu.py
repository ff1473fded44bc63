"""Host logic of the float64 cube engine (wt_cubes64: transform_cube / denoise_cube on float64 and integer cubes),
checked without a device: the truth table of cube64_eligible beside cube_eligible, the header, the export and the Python
binding of wt64_decompose_cube, its refusal of a null plan, and the package's exports."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import cubes as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F64_TYPES = (np.float64, np.int16, np.uint16, np.int32, np.int64, ">f4", ">f8")
# (a big-endian int16 is not among the types the reference recasts, ref wavelets.py:297: native 'int16' only - it stays
# a float32-class cube, as for AtrousTransform)
F32_TYPES = (np.float32, np.uint8, np.float16, ">i2")


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


class Seventeen(W.B3spline):
    coefficients_1d = np.ones(17) / 17


def f64(shape=(4, 5, 6)):
    return np.zeros(shape, np.float64)


def test_eligible_element_types():
    assert C.cube64_eligible(f64(), 2) and C.cube64_eligible(f64(), 2, W.Triangle)
    for dt in F64_TYPES:
        assert C.cube64_eligible(np.zeros((4, 5, 6), dt), 2), dt
    for dt in F32_TYPES:
        assert not C.cube64_eligible(np.zeros((4, 5, 6), dt), 2) and C.cube_eligible(np.zeros((4, 5, 6), dt), 2), dt
    # the predicate follows the reference's own rule (wavelets._is_f64), whatever the element type, and the two engines
    # never claim the same cube
    for dt in F64_TYPES + F32_TYPES + (np.uint32, np.uint64, np.int8, "<f8", ">i4", bool):
        for shape in ((4, 5, 6), (5, 6), (7,)):
            a = np.zeros(shape, dt)
            assert C.cube64_eligible(a, 2) is (W.wavelets._is_f64(a) and a.ndim == 3), (dt, shape)
            assert not (C.cube64_eligible(a, 2) and C.cube_eligible(a, 2)), (dt, shape)
            assert (C.cube64_eligible(a, 2) or C.cube_eligible(a, 2)) is (a.ndim == 3), (dt, shape)


def test_eligible_shapes():
    assert C.cube64_eligible(f64((1, 1, 1)), 2) and C.cube64_eligible(f64((1, 4, 9)), 2)
    assert not C.cube64_eligible(f64((5, 6)), 2) and not C.cube64_eligible(f64((2, 3, 4, 5)), 2)
    assert not C.cube64_eligible(np.zeros(7, np.float64), 2)
    for shape in ((0, 5, 6), (4, 0, 6), (4, 5, 0)):
        assert not C.cube64_eligible(f64(shape), 2), shape
    assert not C.cube64_eligible([[[0.0, 1.0]]], 2)                      # not an ndarray
    assert C.cube64_eligible(f64((4, 5, 12))[:, :, ::2], 2)              # (copied once before the upload)
    assert C.cube64_eligible(np.zeros((4, 5, 12), np.int16)[:, :, ::2], 2)


def test_eligible_modes_levels_and_scaling_functions():
    assert not C.cube64_eligible(f64(), 2, bilateral=1) and not C.cube64_eligible(f64(), 2, recursive=True)
    assert C.cube64_eligible(f64(), 2, bilateral=None, recursive=False)
    assert C.cube64_eligible(f64(), 0) and C.cube64_eligible(f64(), np.int64(3))
    assert not C.cube64_eligible(f64(), -1) and not C.cube64_eligible(f64(), 2.0) and not C.cube64_eligible(f64(), True)
    assert not C.cube64_eligible(f64(), 2, Seventeen) and not C.cube64_eligible(f64(), 2, Retapped)


def test_header_declares_library_exports_and_python_binds_the_entry():
    txt = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+wt64_decompose_cube\s*\(\s*wt_plan64\s*\*\s*plan\s*,\s*int\s+src\s*,\s*int\s+level\s*,\s*int\s+depth\s*\)\s*;", code)
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "wt64_decompose_cube")
    assert L.SIGNATURES["wt64_decompose_cube"] == L.SIGNATURES["wt64_decompose"]
    assert callable(L.Plan64.decompose_cube)
    assert L.load().wt_abi_version() == 8


def test_null_plan_is_refused_without_a_device():
    lib = L.load()
    assert lib.wt64_decompose_cube(None, L.PLANE_INPUT, 2, 4) == 1
    assert lib.wt_last_error().decode().startswith("wt64_decompose_cube: null plan")


def test_package_exports():
    for name in ("transform_cube", "denoise_cube", "cube_eligible", "cube64_eligible"):
        assert name in C.__all__ and getattr(W, name) is getattr(C, name)
    assert W.cubes is C
