"""(Z, Y, X) cubes - solar image sequences, spectral cubes - through the float32 cube engine (wt_cubes): ONE launch
per scale computes the x, y and z filters of the 3-D branch of convolution() (ref wavelets.py:46-64) and the detail
subtraction (ref wavelets.py:442), where AtrousTransform launches the 2-D filter once per slice, a z filter and a
subtraction.

    transform_cube(cube, level).data  == AtrousTransform(sf)(cube, level).data
    denoise_cube(cube, weights, ...)  == denoise(cube, weights, sf, ...)

bit for bit: the kernel keeps the arithmetic of the kernels it replaces (x, then y, then z; every K-tap sum in
ascending tap order), and a scale whose z chains are too short for the fused march still runs
on them.  Cubes the engine does not cover - float64 and integer cubes, bilateral or recursive transforms, user-defined
scaling functions - return what AtrousTransform / denoise return; cube_eligible says which.  AtrousTransform, denoise
and wow keep their own routing."""
import numpy as np

from ._lib import PLANE_INPUT, PLANE_OUT, acquire_plan, default_context
from .wavelets import (AtrousTransform, B3spline, Coefficients, _family_of, _is_f64, _needs_generic, _result_dtype,
                       generalized_anscombe)
from .utils import denoise

__all__ = ['transform_cube', 'denoise_cube', 'cube_eligible']


def _cube_family(cube, level, scaling_function, bilateral=None, recursive=False):
    """the family (an int) the cube engine computes this cube with, or None (cube_eligible)"""
    if not isinstance(cube, np.ndarray) or cube.ndim != 3 or min(cube.shape) < 1:
        return None
    if _is_f64(cube) or bilateral is not None or recursive:
        return None
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level < 0:
        return None
    if _needs_generic(scaling_function):
        return None
    try:
        fam = _family_of(scaling_function(3))
    except (ValueError, NotImplementedError, TypeError):
        return None
    return fam if isinstance(fam, int) else None      # (a tuple: user-defined taps, the plan's generic kernels)


def cube_eligible(cube, level, scaling_function=B3spline, bilateral=None, recursive=False):
    """True when the cube engine computes this transform (host logic): a 3-D ndarray with every side >= 1 that the
    reference would not compute in float64 (ref wavelets.py:297,319-320); a built-in scaling function with its own
    taps; no bilateral filtering, the standard algorithm, an int level >= 0.  Everything else runs AtrousTransform."""
    return _cube_family(cube, level, scaling_function, bilateral, recursive) is not None


def transform_cube(cube, level, scaling_function=B3spline):
    """``Coefficients`` of the standard transform of a (Z, Y, X) cube, AtrousTransform(scaling_function)(cube, level)
    bit for bit (ref wavelets.py:307-328 over :46-64), one launch per scale."""
    fam = _cube_family(cube, level, scaling_function)
    if fam is None:
        return AtrousTransform(scaling_function)(cube, level)
    level = int(level)
    data = np.ascontiguousarray(cube, dtype=np.float32)
    Z, Y, X = data.shape
    sf = scaling_function(3)
    plan = acquire_plan(default_context(), Z * Y, X, fam, level)
    plan.upload(PLANE_INPUT, data.reshape(Z * Y, X))
    plan.decompose_cube(PLANE_INPUT, level, Z)
    return Coefficients(plan, sf, None, _shape=(Z, Y, X), _dtype=_result_dtype(cube))


def denoise_cube(cube, weights, scaling_function=B3spline, noise=None, soft_threshold=True, anscombe=False):
    """utils.denoise(cube, weights, scaling_function, noise, soft_threshold=..., anscombe=...) bit for bit (ref
    utils.py:83-102 on a 3-D array): its call sequence on transform_cube's coefficients."""
    if not cube_eligible(cube, len(weights), scaling_function):
        return denoise(cube, weights, scaling_function, noise, soft_threshold=soft_threshold, anscombe=anscombe)
    arr = np.asarray(cube, np.float32)
    if anscombe:
        arr = generalized_anscombe(arr)
    coefficients = transform_cube(arr, len(weights), scaling_function)
    coefficients.noise = noise
    plan = coefficients._denoise_sum(weights, soft_threshold=soft_threshold, write_back=False)
    if anscombe:
        plan.anscombe(PLANE_OUT, PLANE_OUT, inverse=True)
    return coefficients._from_plane(plan.download(PLANE_OUT)).astype(_result_dtype(cube), copy=False)
