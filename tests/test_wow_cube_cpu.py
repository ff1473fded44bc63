"""Host logic of wow on cubes (wavelets_amd.cubes.wow_cube), checked without a device: the truth table of
wow_cube_eligible, the package's exports, the two C entries in the header, the library and the Python binding, their
refusal of a null plan, and the keyword of utils._wow_scales, which defaults to off."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import cubes as C
from wavelets_amd import utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


class Seventeen(W.B3spline):
    coefficients_1d = np.ones(17) / 17


def zeros(dt, shape=(4, 5, 6)):
    return np.zeros(shape, dt)


def test_eligible_element_types_either_engine():
    for dt in (np.float32, np.float64, np.int16, np.uint16, np.int32, np.uint8, np.float16, ">f4", ">f8", ">i2", np.int64):
        a = zeros(dt)
        assert C.wow_cube_eligible(a) and C.wow_cube_eligible(a, W.Triangle), dt
        # exactly one engine takes it, at every scale count
        assert C.cube_eligible(a, 3) is not C.cube64_eligible(a, 3), dt


def test_eligible_shapes():
    assert C.wow_cube_eligible(zeros(np.float32, (1, 1, 1))) and C.wow_cube_eligible(zeros(np.float64, (1, 4, 9)))
    for shape in ((5, 6), (7,), (2, 3, 4, 5), (0, 5, 6), (4, 0, 6), (4, 5, 0)):
        assert not C.wow_cube_eligible(zeros(np.float32, shape)), shape
    assert not C.wow_cube_eligible([[[0.0, 1.0]]])                         # not an ndarray
    assert C.wow_cube_eligible(zeros(np.float32, (4, 5, 12))[:, :, ::2])   # (copied once before the upload)


def test_eligible_bilateral_and_scaling_functions():
    a = zeros(np.float32)
    assert C.wow_cube_eligible(a, W.B3spline, None) and C.wow_cube_eligible(a, bilateral=None)
    assert not C.wow_cube_eligible(a, bilateral=1) and not C.wow_cube_eligible(a, W.Triangle, bilateral=[1, 2])
    assert not C.wow_cube_eligible(a, Seventeen) and not C.wow_cube_eligible(a, Retapped)
    assert not C.wow_cube_eligible(zeros(np.float64), Seventeen) and not C.wow_cube_eligible(zeros(np.int16), Retapped)
    assert list(inspect.signature(C.wow_cube_eligible).parameters) == ["data", "scaling_function", "bilateral"]


def test_package_exports_and_signature():
    for name in ("wow_cube", "wow_cube_eligible"):
        assert name in C.__all__ and getattr(W, name) is getattr(C, name)
    p = inspect.signature(C.wow_cube).parameters
    assert list(p) == ["data", "scaling_function", "n_scales", "weights", "whitening", "denoise_coefficients", "noise",
                       "soft_threshold", "preserve_variance", "gamma", "gamma_min", "gamma_max", "h"]
    q = inspect.signature(U.wow).parameters               # wow's defaults, without its bilateral options
    assert all(p[k].default == q[k].default or p[k].default is q[k].default for k in p if k != "data")


def test_header_declares_library_exports_and_python_binds_the_entries():
    txt = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    args = (r"\s*\*\s*plan\s*,\s*int\s+plane\s*,\s*int\s+s\s*,\s*int\s+depth\s*,\s*double\s+tau\s*,\s*int\s+soft\s*,"
            r"\s*int\s+noise_plane\s*,\s*%s\s+factor\s*,\s*int\s+gamma_plane\s*\)\s*;")
    assert re.search(r"\bint\s+wt_wow_cube_scale\s*\(\s*wt_plan" + args % "float", code)
    assert re.search(r"\bint\s+wt64_wow_cube_scale\s*\(\s*wt_plan64" + args % "double", code)
    # ... each with the reference call site it replaces
    for name in ("wt_wow_cube_scale", "wt64_wow_cube_scale"):
        comment = txt[:txt.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "utils.py:193-203" in comment and "wavelets.py:46-64" in comment, name
    lib = ctypes.CDLL(L.LIB_PATH)
    c = ctypes
    assert hasattr(lib, "wt_wow_cube_scale") and hasattr(lib, "wt64_wow_cube_scale")
    head = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_double, c.c_int, c.c_int]
    assert L.SIGNATURES["wt_wow_cube_scale"] == (c.c_int, head + [c.c_float, c.c_int])
    assert L.SIGNATURES["wt64_wow_cube_scale"] == (c.c_int, head + [c.c_double, c.c_int])
    assert callable(L.Plan.wow_cube_scale) and callable(L.Plan64.wow_cube_scale)
    assert list(inspect.signature(L.Plan.wow_cube_scale).parameters) == list(inspect.signature(L.Plan64.wow_cube_scale).parameters) \
        == ["self", "plane", "s", "depth", "tau", "soft", "noise_plane", "factor", "gamma_plane"]
    assert L.load().wt_abi_version() == 8                  # additive entries


def test_null_plans_are_refused_without_a_device():
    lib = L.load()
    assert lib.wt_wow_cube_scale(None, 0, 0, 4, 1.0, 1, L.PLANE_NONE, 1.0, L.PLANE_NONE) == 1
    assert lib.wt_last_error().decode().startswith("wt_wow_cube_scale: null plan")
    assert lib.wt64_wow_cube_scale(None, 0, 0, 4, 1.0, 1, L.PLANE_NONE, 1.0, L.PLANE_NONE) == 1
    assert lib.wt_last_error().decode().startswith("wt64_wow_cube_scale: null plan")


class FakePlan:
    """records the calls of the per-scale loop"""

    custom = False

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + args)
            return (0.0, 1.0, 0.0, 1.0) if name == "reduce" else None
        return call


class FakeCoefficients:
    _ndim, _shape, scaling_function = 3, (4, 5, 6), W.B3spline(3)

    def _tau(self, d, s, soft):
        return None


def test_the_keyword_of_wow_scales_defaults_to_off():
    p = inspect.signature(U._wow_scales).parameters["cube_kernel"]
    assert p.default is False and inspect.signature(U._wow_device).parameters["cube_kernel"].default is False

    def names(**kw):
        plan = FakePlan()
        U._wow_scales(plan, FakeCoefficients(), 2, 3, [1, 1, 1], [0, 0, 1], 120.0, False, True, 0, True, L.PLANE_NONE, **kw)
        return [c[0] for c in plan.calls]

    old = ["binary", "smooth3d", "wow_update"]
    assert names() == names(cube_kernel=False) == old * 2 + ["reduce", "wow_update"]
    assert names(cube_kernel=True) == ["wow_cube_scale"] * 2 + ["reduce", "wow_update"]   # the last plane: wow_update
    plan = FakePlan()
    U._wow_scales(plan, FakeCoefficients(), 2, 3, [1, 1, 1], [0, 0, 1], 120.0, False, True, 0, True, L.PLANE_NONE, cube_kernel=True)
    assert plan.calls[1][:4] == ("wow_cube_scale", 1, 1, 4)                 # plane, scale, depth = Z
    # modes without a local power need no kernel of their own
    plan = FakePlan()
    U._wow_scales(plan, FakeCoefficients(), 2, 3, [1, 1, 1], [0, 0, 1], 120.0, False, False, 0, True, L.PLANE_NONE, cube_kernel=True)
    assert [c[0] for c in plan.calls] == ["wow_update"] * 3
