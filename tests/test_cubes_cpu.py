"""Host logic of the cube engine (wt_cubes: transform_cube / denoise_cube), checked without a device: the truth table
of cube_eligible, the header, the exports and the Python binding of wt_decompose_cube, its refusal of a null plan, and
the package's exports."""
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


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


class Seventeen(W.B3spline):
    coefficients_1d = np.ones(17) / 17


def f32(shape=(4, 5, 6)):
    return np.zeros(shape, np.float32)


def test_eligible_element_types():
    assert C.cube_eligible(f32(), 2) and C.cube_eligible(f32(), 2, W.Triangle)
    assert C.cube_eligible(np.zeros((4, 5, 6), np.uint8).astype(np.float32), 2)
    assert not C.cube_eligible(np.zeros((4, 5, 6), np.float64), 2)
    assert not C.cube_eligible(np.zeros((4, 5, 6), np.int16), 2)
    # the predicate follows the reference's own rule (wavelets._is_f64), whatever the element type
    for dt in (np.uint8, np.int32, np.float16, ">f4", ">f8", np.int64):
        a = np.zeros((4, 5, 6), dt)
        assert C.cube_eligible(a, 2) is (not W.wavelets._is_f64(a)), dt


def test_eligible_shapes():
    assert C.cube_eligible(f32((1, 1, 1)), 2) and C.cube_eligible(f32((1, 4, 9)), 2)
    assert not C.cube_eligible(f32((5, 6)), 2) and not C.cube_eligible(f32((2, 3, 4, 5)), 2)
    assert not C.cube_eligible(np.zeros(7, np.float32), 2)
    for shape in ((0, 5, 6), (4, 0, 6), (4, 5, 0)):
        assert not C.cube_eligible(f32(shape), 2), shape
    assert not C.cube_eligible([[[0.0, 1.0]]], 2)                      # not an ndarray
    assert C.cube_eligible(f32((4, 5, 12))[:, :, ::2], 2)              # (copied once before the upload)


def test_eligible_modes_levels_and_scaling_functions():
    assert not C.cube_eligible(f32(), 2, bilateral=1) and not C.cube_eligible(f32(), 2, recursive=True)
    assert C.cube_eligible(f32(), 2, bilateral=None, recursive=False)
    assert C.cube_eligible(f32(), 0) and C.cube_eligible(f32(), np.int64(3))
    assert not C.cube_eligible(f32(), -1) and not C.cube_eligible(f32(), 2.0) and not C.cube_eligible(f32(), True)
    assert not C.cube_eligible(f32(), 2, Seventeen) and not C.cube_eligible(f32(), 2, Retapped)


def test_header_declares_library_exports_and_python_binds_the_entry():
    txt = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+wt_decompose_cube\s*\(\s*wt_plan\s*\*\s*plan\s*,\s*int\s+src\s*,\s*int\s+level\s*,\s*int\s+depth\s*\)\s*;", code)
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "wt_decompose_cube")
    assert L.SIGNATURES["wt_decompose_cube"] == L.SIGNATURES["wt_decompose3d"]
    assert callable(L.Plan.decompose_cube)
    assert "cubes" in L.unit_names()
    assert "cubes" in [obj[:-2] for obj, _, _ in entry._units()]
    assert L.load().wt_abi_version() == 8


def test_null_plan_is_refused_without_a_device():
    lib = L.load()
    assert lib.wt_decompose_cube(None, L.PLANE_INPUT, 2, 4) == 1
    assert lib.wt_last_error().decode().startswith("wt_decompose_cube: null plan")


def test_package_exports():
    for name in ("transform_cube", "denoise_cube", "cube_eligible"):
        assert name in C.__all__ and getattr(W, name) is getattr(C, name)
    assert W.cubes is C
