"""(Z, Y, X) cubes - solar image sequences, spectral cubes - through the cube engines (wt_cubes, float32; wt_cubes64,
float64): ONE launch per scale computes the x, y and z filters of the 3-D branch of convolution() (ref wavelets.py:46-64)
and the detail subtraction (ref wavelets.py:442), where AtrousTransform launches the 2-D filter once per slice, a z
filter and a subtraction (float32) or three one-sample-per-thread filters through two temporaries (float64).

    transform_cube(cube, level).data  == AtrousTransform(sf)(cube, level).data
    denoise_cube(cube, weights, ...)  == denoise(cube, weights, sf, ...)
    wow_cube(cube, ...)               == wow(cube, ...)                 (image and coefficients.data)

bit for bit: the kernel keeps the arithmetic of the kernels it replaces (x, then y, then z; every K-tap sum in
ascending tap order, DESIGN.md sections 3.21 and 3.22), and a scale the fused march does not serve still runs on them.
float64 cubes and the cubes the reference recasts to float64 (ref wavelets.py:297,319-320: int16 / uint16 / int32 /
big-endian FITS data) run in float64, integers and big-endian floats crossing PCIe as they are.  Cubes the engines do
not cover - bilateral or recursive transforms, user-defined scaling functions - return what AtrousTransform / denoise
return; cube_eligible and cube64_eligible say which.  wow_cube whitens each detail scale in one more launch
(wt_cube_wow_kernel: the same march over the squares, the pointwise update of wow as its epilogue, section 3.23) where wow
runs a multiplication, Z + 2 launches of the 3-D filter and the update; wow_cube_eligible says which cubes.
AtrousTransform, denoise and wow keep their own routing."""
import numpy as np

from ._lib import PLANE_INPUT, PLANE_OUT, acquire_plan, acquire_plan64, default_context, device_widens
from .wavelets import (AtrousTransform, B3spline, Coefficients, _family_of, _is_f64, _needs_generic, _result_dtype,
                       _taps_f64, generalized_anscombe)
from .utils import _wow_device, _wow_n_scales, _wow_scale_limit, denoise, wow

__all__ = ['transform_cube', 'denoise_cube', 'wow_cube', 'cube_eligible', 'cube64_eligible', 'wow_cube_eligible']


def _builtin_family(scaling_function):
    """the family (an int) of a built-in scaling function with its own taps, the ones the cube kernels hold, or None"""
    if _needs_generic(scaling_function):
        return None
    try:
        fam = _family_of(scaling_function(3))
    except (ValueError, NotImplementedError, TypeError):
        return None
    return fam if isinstance(fam, int) else None      # (a tuple: user-defined taps, the plan's generic kernels)


def _cube_family(cube, level, scaling_function, bilateral=None, recursive=False, f64=False):
    """the family (an int) the float32 (f64: the float64) cube engine computes this cube with, or None (cube_eligible,
    cube64_eligible)"""
    if not isinstance(cube, np.ndarray) or cube.ndim != 3 or min(cube.shape) < 1:
        return None
    if _is_f64(cube) != f64 or bilateral is not None or recursive:
        return None
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level < 0:
        return None
    return _builtin_family(scaling_function)


def cube_eligible(cube, level, scaling_function=B3spline, bilateral=None, recursive=False):
    """True when the float32 cube engine computes this transform (host logic): a 3-D ndarray with every side >= 1 that
    the reference would not compute in float64 (ref wavelets.py:297,319-320); a built-in scaling function with its own
    taps; no bilateral filtering, the standard algorithm, an int level >= 0.  Everything else runs the float64 engine
    (cube64_eligible) or AtrousTransform."""
    return _cube_family(cube, level, scaling_function, bilateral, recursive) is not None


def cube64_eligible(cube, level, scaling_function=B3spline, bilateral=None, recursive=False):
    """True when the float64 cube engine computes this transform (host logic): the rule of cube_eligible for the cubes
    the reference DOES compute in float64 (ref wavelets.py:297,319-320) - float64, and the integer and big-endian types
    it recasts.  Never true together with cube_eligible."""
    return _cube_family(cube, level, scaling_function, bilateral, recursive, f64=True) is not None


def _cube64_coefficients(cube, level, scaling_function, anscombe=False):
    """transform_cube on the float64 engine: ``Coefficients`` on a Plan64 (anscombe: of the Anscombe transform of the
    cube, taken on the plan's input plane - the pointwise kernel generalized_anscombe runs, ref utils.py:93-94).  Element
    types Plan64.upload widens on the device - integers, big-endian floats - go up as they are, as (Z*Y, X) rows."""
    a = np.asarray(cube)
    a = np.ascontiguousarray(a) if device_widens(a.dtype) else np.ascontiguousarray(a, dtype=np.float64)
    Z, Y, X = a.shape
    sf = scaling_function(3)
    plan = acquire_plan64(default_context(), Z * Y, X, _taps_f64(sf, 3), level)
    plan.upload(PLANE_INPUT, a.reshape(Z * Y, X))
    if anscombe:
        plan.anscombe(PLANE_INPUT, PLANE_INPUT)
    plan.decompose_cube(PLANE_INPUT, level, Z)
    return Coefficients(plan, sf, None, _shape=(Z, Y, X), _dtype=np.float64)


def transform_cube(cube, level, scaling_function=B3spline):
    """``Coefficients`` of the standard transform of a (Z, Y, X) cube, AtrousTransform(scaling_function)(cube, level)
    bit for bit (ref wavelets.py:307-328 over :46-64), one launch per scale."""
    if cube64_eligible(cube, level, scaling_function):
        return _cube64_coefficients(cube, int(level), scaling_function)
    fam = _cube_family(cube, level, scaling_function)
    if fam is None:
        return AtrousTransform(scaling_function)(cube, level)
    return _cube32_coefficients(cube, int(level), scaling_function, fam)


def _cube32_coefficients(cube, level, scaling_function, fam):
    """transform_cube on the float32 engine: ``Coefficients`` on a Plan of family `fam` (_cube_family)"""
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
    f64 = cube64_eligible(cube, len(weights), scaling_function)
    if not f64 and not cube_eligible(cube, len(weights), scaling_function):
        return denoise(cube, weights, scaling_function, noise, soft_threshold=soft_threshold, anscombe=anscombe)
    if f64:
        coefficients = _cube64_coefficients(cube, len(weights), scaling_function, anscombe)
    else:
        arr = np.asarray(cube, np.float32)
        if anscombe:
            arr = generalized_anscombe(arr)
        coefficients = transform_cube(arr, len(weights), scaling_function)
    coefficients.noise = noise
    plan = coefficients._denoise_sum(weights, soft_threshold=soft_threshold, write_back=False)
    if anscombe:
        plan.anscombe(PLANE_OUT, PLANE_OUT, inverse=True)
    return coefficients._from_plane(plan.download(PLANE_OUT)).astype(_result_dtype(cube), copy=False)


def _wow_cube_family(data, scaling_function, bilateral=None):
    """the family (an int) wow_cube runs this cube with on either engine, or None (wow_cube_eligible): _cube_family
    without the element-type test and at any scale count"""
    if not isinstance(data, np.ndarray) or data.ndim != 3 or min(data.shape) < 1 or bilateral is not None:
        return None
    return _builtin_family(scaling_function)


def wow_cube_eligible(data, scaling_function=B3spline, bilateral=None):
    """True when wow_cube runs this cube on a cube engine (host logic): the rule of cube_eligible / cube64_eligible,
    either engine, at any scale count - a 3-D ndarray with every side >= 1, a built-in scaling function with its own
    taps, no bilateral filtering.  Everything else returns wow's result."""
    return _wow_cube_family(data, scaling_function, bilateral) is not None


def wow_cube(data, scaling_function=B3spline, n_scales=None, weights=[], whitening=True, denoise_coefficients=[],
             noise=None, soft_threshold=True, preserve_variance=False, gamma=3.2, gamma_min=None, gamma_max=None, h=0):
    """utils.wow(data, scaling_function, n_scales, weights, ...) on a (Z, Y, X) cube, bit for bit - the image and
    coefficients.data, in wow's dtypes (ref utils.py:105-219 on a 3-D array): the transform through transform_cube's
    route and the whitening of every detail scale in one launch (Plan.wow_cube_scale).  ``data`` is a 3-D ndarray or
    a 3-D ``Coefficients`` (transform_cube's, AtrousTransform's), which is mutated and returned as wow does."""
    kwargs = dict(n_scales=n_scales, weights=weights, whitening=whitening, denoise_coefficients=denoise_coefficients,
                  noise=noise, soft_threshold=soft_threshold, preserve_variance=preserve_variance, gamma=gamma,
                  gamma_min=gamma_min, gamma_max=gamma_max, h=h)
    fam = None
    if type(data) is Coefficients:                                        # ref utils.py:128-131
        scaling_function = data.scaling_function.__class__
        if data._ndim != 3 or data.bilateral is not None or _builtin_family(scaling_function) is None:
            return wow(data, scaling_function, **kwargs)
        n_scales = len(data) - 1
    else:
        fam = _wow_cube_family(data, scaling_function) if type(data) is np.ndarray else None
        if fam is None:
            return wow(data, scaling_function, **kwargs)
        n_scales = _wow_n_scales(data.shape, scaling_function, n_scales, h, denoise_coefficients)     # ref utils.py:122-127
    n_scales = _wow_scale_limit(n_scales, scaling_function, 3, None, denoise_coefficients)            # ref utils.py:135-138
    if fam is None:
        coefficients = data
    else:                                                                 # ref utils.py:148-151
        if type(n_scales) is not int or n_scales < 0:                     # (not a level: AtrousTransform's own refusal)
            coefficients = transform_cube(data, n_scales, scaling_function)
        elif _is_f64(data):
            coefficients = _cube64_coefficients(data, n_scales, scaling_function)
        else:
            coefficients = _cube32_coefficients(data, n_scales, scaling_function, fam)
        coefficients.noise = noise
    plan = _wow_device(coefficients, n_scales, weights, whitening, denoise_coefficients, soft_threshold,
                       preserve_variance, gamma, gamma_min, gamma_max, h, cube_kernel=True)
    recon = coefficients._from_plane(plan.download(PLANE_OUT)).astype(coefficients._dtype, copy=False)
    coefficients._refresh_host(range(len(coefficients)))
    return recon, coefficients
