"""The 1-D transform along ANY axis of an array - the light curve of every pixel of a (T, H, W) movie, the spectrum of
every pixel of a (lambda, Y, X) raster or of a (Y, lambda, X) detector read-out - through the axis engine (wt_along):
the array is viewed as (O, N, I), a workgroup takes a tile of neighbouring signals whose samples lie I elements apart,
filters them in LDS and writes every plane in the layout of the input.  No transpose, on the host or on the device.

With sig = np.moveaxis(a, axis, -1).reshape(M, N) and moved = np.moveaxis(a, axis, -1).shape:

    transform_along(a, level, sf, axis)[s] == np.moveaxis(transform_signals(sig, level, sf)[:, s].reshape(moved), -1, axis)
    denoise_along(a, weights, sf, axis)    == np.moveaxis(denoise_signals(sig, weights, sf, noise).reshape(moved), -1, axis)

bit for bit - and transform_signals equals the per-signal loop bit for bit (ref wavelets.py:65-69 under :408-444).
The thresholds are the per-signal path's own (wavelets._interleave_split, _tau_row, _noise_from_median), evaluated for
all signals of a chunk at once (_tau_table).

Non-finite samples follow signals.py: a signal holding NaN or inf gets what the per-signal call gives it (a NaN median
makes NaN thresholds in _noise_table / _tau_table, which the kernel takes as significance one), nothing is raised, and
its neighbours in the tile keep their bits.

The last axis is the signal engine's own layout and goes there.  Inputs the axis engine does not cover (along_eligible:
more than 512 samples along the axis, other element types, custom scaling functions ...) are transposed on the host,
go through transform_signals / denoise_signals and return what those return."""
import numpy as np

from . import _lib
from .wavelets import B3spline, _result_dtype
from .signals import transform_signals, denoise_signals, _engine_family, _target, _hand_over, _result, _thresholds
from .batch import _real_scalar

__all__ = ['transform_along', 'denoise_along', 'along_eligible']


def _axis_of(a, axis):
    """the axis as a non-negative int, or None"""
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not -a.ndim <= axis < a.ndim:
        return None
    return int(axis) % a.ndim


def _view(shape, axis):
    """(O, N, I) of an array of `shape` along `axis`: the products of the dimensions before and after it"""
    return int(np.prod(shape[:axis], dtype=np.int64)), shape[axis], int(np.prod(shape[axis + 1:], dtype=np.int64))


def _real_array(noise):
    return isinstance(noise, np.ndarray) and noise.dtype.kind in "biuf"


def _along_family(a, level, scaling_function, axis, noise=None):
    """the family the axis engine computes this array with, or None (along_eligible)"""
    if not isinstance(a, np.ndarray) or a.ndim < 2:
        return None
    axis = _axis_of(a, axis)
    if axis is None:
        return None
    O, N, I = _view(a.shape, axis)
    if O < 1 or N < 1 or I < 2:
        return None
    fam = _engine_family(a.dtype, level, scaling_function)
    if fam is None:
        return None
    if isinstance(noise, np.ndarray):
        if not _real_array(noise) or noise.shape != a.shape[:axis] + a.shape[axis + 1:]:
            return None
    elif noise is not None and not _real_scalar(noise):
        return None
    return fam if _lib.along_ok(fam, N, I, int(level), a.dtype.itemsize) else None


def along_eligible(a, level, scaling_function=B3spline, axis=0, noise=None):
    """True when the axis engine computes this array (host logic): an ndarray of at least two dimensions of native
    float32 or native float64 with at least one signal; an axis that is not in effect the last one (I >= 2: the last
    axis is the signal engine's); a built-in scaling function with its own taps; an int level, 1 <= level <= 24;
    `noise` None, a real scalar or a real ndarray of the shape of `a` without `axis`; and an axis within the LDS budget
    of the kernel (_lib.along_ok: at most 512 samples).  Everything else runs the transposed route."""
    return _along_family(a, level, scaling_function, axis, noise) is not None


# ---------------------------------------------------------------- thresholds of all signals at once

def _like_scalar(x, probe, other):
    """`x` (an array) combined with the scalar `other` as numpy combines ONE element of x with it: both sides in the
    element type numpy promotes the scalar pair to (`probe`: that pair's result)"""
    dt = np.asarray(probe).dtype
    return x.astype(dt, copy=False), dt.type(other)


def _noise_table(medians, sigma_e):
    """wavelets._noise_from_median of every median of an array of the stack's element type, element by element what
    the scalar expression median / 0.6745 / sigma_e[0] gives (numpy's promotion of a scalar of that type included)"""
    med = np.asarray(medians)
    one = med.dtype.type(1)
    x, c = _like_scalar(med, one / 0.6745, 0.6745)
    x = x / c
    x, c = _like_scalar(x, one / 0.6745 / sigma_e[0], sigma_e[0])
    return x / c


def _tau_table(entries, noises, sigma_e, soft):
    """(signals, entries) float64: row i is wavelets._tau_row(entries, noises[i], sigma_e, soft) - Coefficients._tau
    for a scalar noise level (ref wavelets.py:129-143), 0.0 = significance one - without a Python loop over the
    signals.  `noises`: an array of one noise level per signal, of any real element type."""
    noises = np.asarray(noises)
    tab = np.zeros((noises.shape[0], len(entries)), np.float64)
    one = noises.dtype.type(1)
    for k, (scl, sig, _) in enumerate(entries):
        if sig == 0:
            continue
        x, c = _like_scalar(noises, sig * one, sig)                      # float(sigma * noise * sigma_e[scale])
        x = x * c
        x, c = _like_scalar(x, sig * one * sigma_e[scl], sigma_e[scl])
        t = (x * c).astype(np.float64)
        t = np.where(t < 0, -t if soft else 0.0, t)                    # a negative threshold: |tau| (soft), one (hard)
        t[noises == 0] = 0.0                                           # ref:133-135
        tab[:, k] = t
    return tab


# ---------------------------------------------------------------- the transposed route

def _moved(a, axis):
    """the (M, N) stack of the signals along `axis` (a host transpose) and the shape it came from"""
    m = np.moveaxis(a, axis, -1)
    return np.ascontiguousarray(m).reshape(-1, a.shape[axis]), m.shape


def _back(res, moved_shape, axis, lead):
    """`lead` leading axes of per-signal results + (M, [.], N) -> the signals back along `axis`"""
    if lead:      # (M, level + 1, N) -> (level + 1, ...)
        r = np.moveaxis(res.reshape(moved_shape[:-1] + res.shape[1:]), -2, 0)
        return np.moveaxis(r, -1, 1 + axis)
    return np.moveaxis(res.reshape(moved_shape), -1, axis)


def _chunks(O, N, I, level, itemsize, planes):
    """the chunk rule of an array over device memory (_lib.along_chunks)"""
    return _lib.along_chunks(O, N, I, level, itemsize=itemsize, planes=planes)


def _checked(a, axis):
    if not isinstance(a, np.ndarray) or a.ndim < 2:
        raise ValueError("a: an ndarray of at least two dimensions expected")
    ax = _axis_of(a, axis)
    if ax is None:
        raise ValueError(f"axis: an int within [-{a.ndim}, {a.ndim}) expected (got {axis!r})")
    return np.ascontiguousarray(a), ax


def transform_along(a, level, scaling_function=B3spline, axis=0, out=None):
    """(level + 1,) + a.shape, float32 or - for the arrays the reference computes in float64 - float64: the standard
    transform of every 1-D signal along `axis` (AtrousTransform(scaling_function)(signal, level).data, ref
    wavelets.py:307-328 over :65-69), plane s of all signals at [s].  One launch per chunk."""
    a, axis = _checked(a, axis)
    O, N, I = _view(a.shape, axis)
    fam = None if I == 1 else _along_family(a, level, scaling_function, axis)
    if fam is None:
        # the signal engine's layout (the last axis), or the route a user would write: transpose, transform_signals
        # (which routes further by itself and raises what it raises), rearrange
        if isinstance(level, (int, np.integer)) and level >= 0:
            out = _target(out, (level + 1,) + a.shape, _result_dtype(a))
        sig, moved = _moved(a, axis)
        res = _back(transform_signals(sig, level, scaling_function), moved, axis, 1)
        return _hand_over(res, out) if out is not None else np.ascontiguousarray(res)
    level = int(level)
    res, ctx = _result(_target(out, (level + 1,) + a.shape, a.dtype), (level + 1,) + a.shape, a.dtype)
    a3, r4 = a.reshape(O, N, I), res.reshape(level + 1, O, N, I)
    chunks = _chunks(O, N, I, level, a.dtype.itemsize, True)
    ab = _lib.acquire_along(ctx, max(no * ni for _, no, _, ni in chunks), N, fam, level, a.dtype, planes=True)
    try:
        for o0, no, i0, ni in chunks:
            ab.upload(a3[o0:o0 + no, :, i0:i0 + ni])
            ab.decompose(level)
            ab.download_planes(r4[:, o0:o0 + no, :, i0:i0 + ni])
    finally:
        _lib.release_along(ab)
    return res


def denoise_along(a, weights, scaling_function=B3spline, axis=0, noise=None, soft_threshold=True, out=None, anscombe=False):
    """a.shape: utils.denoise of every 1-D signal along `axis` (ref utils.py:83-102 on a 1-D array), float32 or float64
    as transform_along.  `noise`: None (each signal's own MAD estimate, ref wavelets.py:126-132), one real scalar, or
    an ndarray of the shape of `a` without `axis`: one level per signal.  The transform, the thresholds and the sum are
    one launch per chunk (no plane reaches device memory); only when a MAD estimate is needed a launch before it
    brings the medians of all signals of the chunk in one round trip.
    `anscombe`: denoise_signals(..., anscombe=True) on the transposed stack, bit for bit - hence denoise(signal, ...,
    anscombe=True) of every signal (ref utils.py:93-94, 99-100): the forward transform where the kernels load the chunk,
    the inverse where the sum is stored, in the same launches.  Noise levels refer to the transformed data."""
    a, axis = _checked(a, axis)
    ans = {"anscombe": True} if anscombe else {}               # (without it: the calls as they always were)
    O, N, I = _view(a.shape, axis)
    rest = a.shape[:axis] + a.shape[axis + 1:]
    if isinstance(noise, np.ndarray) and noise.shape != rest:
        raise ValueError(f"noise: an array of shape {rest} expected, one level per signal (got {noise.shape})")
    level = len(weights)
    fam = None if I == 1 else _along_family(a, level, scaling_function, axis, noise)
    if fam is None or level + 1 > _lib.MAX_SUM_PLANES:
        out = _target(out, a.shape, _result_dtype(a))
        sig, moved = _moved(a, axis)
        per = list(noise.reshape(-1)) if isinstance(noise, np.ndarray) else noise
        res = _back(denoise_signals(sig, weights, scaling_function, per, soft_threshold, **ans), moved, axis, 0)
        return _hand_over(res, out) if out is not None else np.ascontiguousarray(res)
    res = _target(out, a.shape, a.dtype)
    sigma_e, entries, need_noise = _thresholds(weights, scaling_function)       # (as denoise_signals)
    wgts = [w for _, _, w in entries]
    res, ctx = _result(res, a.shape, a.dtype)
    a3, r3 = a.reshape(O, N, I), res.reshape(O, N, I)
    levels = noise.reshape(O, I) if isinstance(noise, np.ndarray) else None
    chunks = _chunks(O, N, I, level, a.dtype.itemsize, False)
    ab = _lib.acquire_along(ctx, max(no * ni for _, no, _, ni in chunks), N, fam, level, a.dtype, planes=False)
    try:
        for o0, no, i0, ni in chunks:
            ab.upload(a3[o0:o0 + no, :, i0:i0 + ni])
            if not need_noise:
                taus = np.zeros((no * ni, len(entries)))               # no threshold is non-zero: no median, no table
            else:
                if levels is not None:
                    noises = levels[o0:o0 + no, i0:i0 + ni].reshape(-1)
                elif noise is not None:
                    noises = np.full(no * ni, noise, dtype=np.asarray(noise).dtype)
                else:
                    noises = _noise_table(ab.abs_median(**ans).reshape(-1), sigma_e)  # ref wavelets.py:131-132 (lazy)
                taus = _tau_table(entries, noises, sigma_e, soft_threshold)
            ab.denoise(level, taus, wgts, soft_threshold, **ans)
            ab.download_sum(r3[o0:o0 + no, :, i0:i0 + ni])
    finally:
        _lib.release_along(ab)
    return res
