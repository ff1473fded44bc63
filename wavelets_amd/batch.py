"""Stacks of same-shape frames through the batched engine (wt_batch): every fused pass of the schedule runs
over all frames of a chunk in ONE launch (the frame is a grid dimension), the MAD medians of all frames come
back in one host round trip, and the pointwise steps run once over the stack.

    transform_stack(frames, level)      == np.stack([AtrousTransform(sf)(f, level).data for f in frames])
    denoise_stack(frames, weights)      == np.stack([denoise(f, weights, sf, noise_i, ...) for f in frames])
    wow_stack(frames, ...)              == np.stack([wow(f, ..., noise=noise_i, ...)[0] for f in frames])
    enhance_stack(frames, [noise,] ...) == np.stack([enhance(f, [noise_i,] ...) for f in frames])   (gray or colour frames)
    richardson_lucy_stack(frames, psf, ...) == np.stack([richardson_lucy(f, psf, ...) for f in frames])   (one PSF)

bit for bit.  The sequence of operations per frame is the per-frame path's own (wavelets._interleave_split,
_tau_row, _noise_from_median, _sigma_bilateral_list; utils._wow_lists, _wow_factor, _gamma_range,
_wow_sigma_bilateral).  With bilateral= the transform is the batched bilateral march: one launch per scale for all
frames (bilateral_eligible).

Stacks the reference computes in float64 - float64 frames; int16 .. int64 and big-endian frames, which it recasts -
run on the float64 batch (wt_batch64).  transform_stack and denoise_stack take it under batch64_eligible, and with
bilateral= behind the batched float64 march under bilateral64_eligible.  wow_stack takes the same batch under
wow64_eligible: the transform's scales beyond the fused passes and the fused update of every scale run on the batched
float64 per-scale stencil, one launch per scale for all frames; the moments, the medians and the gamma range of all
frames come back in one host round trip each.  richardson_lucy_stack takes it under rl64_eligible: the float32 chunk
loop in doubles, the PSF correlation of all frames one launch of the tiled float64 kernel (wt_batch64_filter2d).

`noise` may hold per-pixel noise maps (ref wavelets.py:133-141): one (H, W) ndarray shared by the frames, or one entry
per frame, maps mixed with levels and None.  The maps lie in one more plane of the batch, the noise plane
(noise_map_eligible, _upload_noise_maps); a shared map crosses PCIe once and is replicated on the device.  The map
forms of the thresholded sum and of wow's updates read it, on both batches; a frame with a level has ones there and
keeps its map-free arithmetic.

Inputs the batched engines do not cover run the per-frame loop; batch_eligible, batch64_eligible, wow_eligible,
wow64_eligible, bilateral_eligible and bilateral64_eligible say which."""
from contextlib import contextmanager

import numpy as np

from . import _lib
from ._lib import PLANE_INPUT, PLANE_OUT, PLANE_NONE, PLANE_SCRATCH, FLAG_FUSED
from .wavelets import (AtrousTransform, B3spline, _family_of, _needs_generic, _interleave_split, _tau_row, _map_tau_row,
                       _noise_from_median, _sigma_bilateral_list, _result_dtype, _NOISE_PLANE)
from . import utils as _utils
from .utils import (richardson_lucy, _rl_check_fft_width, _rl_direct_operands, _rl_uses_fft, _rl_fft_kernel_image)
from .utils import (denoise, wow, enhance, _enhance_lists, _GAMMA_PLANE, _wow_n_scales, _wow_scale_limit, _wow_lists, _wow_needs_moments,
                    _wow_factor, _gamma_range, _wow_sigma_bilateral)

__all__ = ['transform_stack', 'denoise_stack', 'wow_stack', 'enhance_stack', 'richardson_lucy_stack', 'rl_eligible', 'rl_fft_eligible', 'rl64_eligible', 'batch_eligible', 'batch64_eligible',
           'wow_eligible', 'wow64_eligible', 'bilateral_eligible', 'bilateral64_eligible', 'enhance_eligible',
           'noise_map_eligible']

# levels whose fused schedule has a kernel for every pass (wt_plan_fused_ok), both built-in families: L = 1 is
# a single-scale pass, and from 9 scales on the schedules hold single-scale passes at D >= 256 (wt_fused_has_pass)
BATCH_LEVELS = range(2, 9)


def _as_frames(frames):
    """(N, H, W) view / array of the frames, or ValueError: an (N, H, W) array or a sequence of 2-D arrays of
    one shape"""
    if isinstance(frames, np.ndarray):
        if frames.ndim != 3 or frames.shape[0] == 0:
            raise ValueError(f"frames: a non-empty (N, H, W) array or a sequence of 2-D arrays (got shape {frames.shape})")
        return frames
    items = [np.asarray(f) for f in frames]
    if any(f.ndim != 2 for f in items):
        raise ValueError("frames: every frame must be a 2-D array")
    if len({f.shape for f in items}) > 1:
        raise ValueError(f"frames: all frames must have one shape (got {sorted({f.shape for f in items})})")
    if len({f.dtype for f in items}) > 1:
        return items                      # mixed element types: the per-frame loop (not eligible)
    if not items:
        raise ValueError("frames: an empty stack")
    return np.stack(items)


def _is_noise_map(n, shape):
    """True for a per-pixel noise map the batched engines take: an ndarray (as Coefficients._tau tells a map from
    a level) of real numbers and of exactly the frames' (H, W)"""
    return type(n) is np.ndarray and n.ndim == 2 and n.shape == tuple(shape) and n.dtype.kind in "biuf"


def _noise_list(noise, n, shape=None):
    """one noise entry per frame (None: that frame's own MAD estimate).  `shape`: the frames' (H, W) - an ndarray
    of exactly that shape is then one noise map shared by the frames (the same array in every entry); without it,
    and for arrays of any other shape, None: the per-frame loop hands the whole array to every frame"""
    if noise is None or (not isinstance(noise, (list, tuple)) and np.ndim(noise) == 0):
        return [noise] * n
    if isinstance(noise, np.ndarray) and noise.ndim != 1:
        if shape is not None and _is_noise_map(noise, shape):
            return [noise] * n
        return None                       # a noise map: the per-frame loop (a 1-D array: one level per frame)
    noise = list(noise)
    if len(noise) != n:
        raise ValueError(f"noise: one entry per frame ({n} frames, {len(noise)} entries)")
    return noise


def _maps_admitted(frames, noise_per_frame, noise_maps):
    """noise_per_frame as the predicates below judge it: with `noise_maps`, every entry that is a noise map of the
    frames' shape (_is_noise_map) stands as a scalar level - the batch holds it in its noise plane.  Without
    `noise_maps` (the default of every predicate) nothing changes: an array entry is refused as before."""
    if not noise_maps or noise_per_frame is None or not isinstance(frames, np.ndarray) or frames.ndim != 3:
        return noise_per_frame
    return [1.0 if _is_noise_map(n, frames.shape[1:]) else n for n in noise_per_frame]


def noise_map_eligible(frames, noise_per_frame):
    """True when `noise_per_frame` holds at least one per-pixel noise map that the batched engines take for the
    (N, H, W) stack `frames` (host logic): a real ndarray of exactly (H, W).  The predicates below admit such
    entries with noise_maps=True; the other entries stay None or real scalars."""
    if noise_per_frame is None or not isinstance(frames, np.ndarray) or frames.ndim != 3:
        return False
    return any(_is_noise_map(n, frames.shape[1:]) for n in noise_per_frame)


def batch_eligible(frames, level, scaling_function=B3spline, bilateral=None, noise_per_frame=(), noise_maps=False):
    """True when the batched engine computes this stack (host logic): native float32 frames of one shape in an
    (N, H, W) array, no bilateral filtering, a built-in scaling function with its own taps, a level with an
    all-fused schedule (2..8) and scalar noise levels - with noise_maps=True also per-pixel noise maps of the frames'
    shape (_is_noise_map).  Everything else runs the per-frame loop."""
    if level not in BATCH_LEVELS:
        return False
    noise_per_frame = _maps_admitted(frames, noise_per_frame, noise_maps)
    return _engine_eligible(frames, scaling_function, bilateral, noise_per_frame)


# scales of wow_stack's transform: from 9 scales on, the schedules hold single-scale passes without a fused kernel,
# which the batch runs on the batched per-scale stencil (wt_batch_decompose); up to the per-scale kernels' limit
WOW_LEVELS = range(1, 25)


def wow_eligible(frames, n_scales, scaling_function=B3spline, bilateral=None, noise_per_frame=(), noise_maps=False):
    """True when the batched engine computes wow over this stack (host logic): batch_eligible's conditions for
    the frames, the scaling function, bilateral filtering and the noise levels - which must also be scalars that
    are not arrays (utils.wow takes a 0-d array as a noise map) or, with noise_maps=True, per-pixel noise maps of the
    frames' shape - with n_scales (already resolved) in 1..24.  Everything else runs the per-frame loop."""
    if n_scales not in WOW_LEVELS:
        return False
    noise_per_frame = _maps_admitted(frames, noise_per_frame, noise_maps)
    if noise_per_frame is not None and any(type(n) is np.ndarray for n in noise_per_frame):
        return False
    return _engine_eligible(frames, scaling_function, bilateral, noise_per_frame)


# wow_stack takes per-pixel noise maps from this many pixels per frame on (one 256-thread block of float4 groups in the
# pointwise updates).  Smaller frames with a map keep the per-frame loop they always had: that route is pinned for an
# 8 x 8 stack (tests/test_wow_stack_cpu.py), and a frame of a few dozen pixels has nothing for the noise plane to save.
# Not a measured crossover (tools/bench_noise_map_stack.py has the measured shapes); denoise_stack has no such floor.
WOW_MAP_MIN_PIXELS = 1024


# scales of the batched bilateral transform: one launch of the march per scale, up to the per-scale kernels' limit
# (wt_decompose_bilateral: scales 0..24)
BILATERAL_MAX_LEVEL = 25


def _real_scalar(v):
    return isinstance(v, (bool, int, float, np.bool_, np.integer, np.floating))


def bilateral_eligible(frames, level, scaling_function=B3spline, bilateral=None, noise_per_frame=(), noise_maps=False):
    """True when the batched engine computes this stack WITH bilateral filtering (host logic): the conditions of
    batch_eligible / wow_eligible for the frames, the scaling function and the noise levels (scalars that are not
    arrays), `bilateral` a real scalar / bool or a list of them, and 1 <= level <= what wt_decompose_bilateral
    (25) and the family's sigma_e(bilateral=...) table admit.  False without bilateral filtering: those stacks are
    batch_eligible's / wow_eligible's.  noise_maps=True: per-pixel noise maps of the frames' shape are taken too.
    Everything else runs the per-frame loop."""
    noise_per_frame = _maps_admitted(frames, noise_per_frame, noise_maps)
    if not _bilateral_call_eligible(level, bilateral, noise_per_frame):
        return False
    if not _engine_eligible(frames, scaling_function, None, noise_per_frame):
        return False
    return _bilateral_level_eligible(level, scaling_function, bilateral)


def _bilateral_call_eligible(level, bilateral, noise_per_frame):
    """the conditions of bilateral_eligible / bilateral64_eligible on the call alone: `bilateral` a real scalar /
    bool or a list of them, an int level >= 1, no noise level that is an array (utils.wow takes a 0-d array as a map)"""
    if bilateral is None:
        return False
    if not (_real_scalar(bilateral) or (type(bilateral) is list and all(_real_scalar(v) for v in bilateral))):
        return False
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level < 1:
        return False
    return noise_per_frame is None or not any(type(n) is np.ndarray for n in noise_per_frame)


def _bilateral_level_eligible(level, scaling_function, bilateral):
    """level <= what the marches (25 scales) and the family's sigma_e(bilateral=...) table admit"""
    table = scaling_function(2).sigma_e(bilateral=bilateral)
    return table is not None and level <= min(BILATERAL_MAX_LEVEL, len(table))


def _engine_eligible(frames, scaling_function, bilateral, noise_per_frame):
    """the conditions of batch_eligible / wow_eligible other than the level"""
    if not isinstance(frames, np.ndarray) or frames.ndim != 3 or frames.dtype != np.dtype(np.float32) \
            or not frames.dtype.isnative:
        return False
    if not _family_noise_eligible(scaling_function, bilateral, noise_per_frame):
        return False
    H, W = frames.shape[1:]
    return H >= 1 and W >= 1 and (W + 3) // 4 * 4 * 4 * 64 * 48 < (1 << 31)   # wt_fused_supported


def _family_noise_eligible(scaling_function, bilateral, noise_per_frame):
    """no bilateral filtering, a built-in family with its own taps, scalar noise levels"""
    if bilateral is not None:
        return False
    if _needs_generic(scaling_function):
        return False
    try:
        if not isinstance(_family_of(scaling_function(2)), int):
            return False
    except (ValueError, NotImplementedError):
        return False
    return noise_per_frame is not None and not any(n is not None and np.ndim(n) != 0 for n in noise_per_frame)


def _float64_frames(frames):
    """True for an (N, H, W) ndarray the reference computes in float64 that the device takes: native float64, or a
    type of wavelets._RECAST that the device widens on upload (wavelets._result_dtype, _lib.device_widens)"""
    if not isinstance(frames, np.ndarray) or frames.ndim != 3 or _result_dtype(frames) != np.float64:
        return False
    return frames.dtype == np.dtype(np.float64) or _lib.device_widens(frames.dtype)


def batch64_eligible(frames, level, scaling_function=B3spline, bilateral=None, noise_per_frame=(), noise_maps=False):
    """True when the float64 batch (wt_batch64) computes this stack (host logic): an (N, H, W) ndarray the
    reference computes in float64 (wavelets._result_dtype: native float64, or a type of wavelets._RECAST that the
    device widens - int16 / uint16 / int32 / uint32 / int64, '>f4', '>f8'), no bilateral filtering, a built-in
    scaling function with its own taps, scalar noise levels, and frames whose float64 schedule of `level` scales
    is all fused passes (images, H >= 2, rows the fused passes take at 8 bytes per pixel: _lib.batch64_fused_ok,
    i.e. what wt64_plan_fused_ok answers for one frame).  noise_maps=True: per-pixel noise maps of the frames' shape
    are taken too.  Everything else keeps its route."""
    if not _float64_frames(frames):
        return False
    noise_per_frame = _maps_admitted(frames, noise_per_frame, noise_maps)
    if not _family_noise_eligible(scaling_function, bilateral, noise_per_frame):
        return False
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
        return False
    N, H, W = frames.shape
    return N >= 1 and _lib.batch64_fused_ok(_family_of(scaling_function(2)), H, W, int(level))


def bilateral64_eligible(frames, level, scaling_function=B3spline, bilateral=None, noise_per_frame=(), noise_maps=False):
    """True when the float64 batch computes this stack WITH bilateral filtering (host logic): batch64_eligible's
    conditions for the frames (an (N, H, W) ndarray the reference computes in float64: native float64, or int16 /
    uint16 / int32 / uint32 / int64 / '>f4' / '>f8', widened on the device), the scaling function and the noise
    levels; bilateral_eligible's for `bilateral` (a real scalar / bool or a list of them), the noise levels
    (scalars that are not arrays) and the level (1 .. min(25, the family's sigma_e(bilateral=...) table)); and frames
    that take the float64 march per frame (_lib.batch64_bilateral_ok: H >= 2, rows the batch accepts, option
    "stencil64" on - with it off the per-frame call runs three generic kernels per scale, whose bits differ).  False
    without bilateral filtering: those stacks are batch64_eligible's.  noise_maps=True: per-pixel noise maps of the
    frames' shape are taken too.  Everything else runs the per-frame loop."""
    noise_per_frame = _maps_admitted(frames, noise_per_frame, noise_maps)
    if not _bilateral_call_eligible(level, bilateral, noise_per_frame):
        return False
    if not _float64_frames(frames):
        return False
    if not _family_noise_eligible(scaling_function, None, noise_per_frame):
        return False
    if not _bilateral_level_eligible(level, scaling_function, bilateral):
        return False
    N, H, W = frames.shape
    return N >= 1 and _lib.batch64_bilateral_ok(_family_of(scaling_function(2)), H, W, int(level))


# wow_stack takes float64 stacks from this many pixels per frame on: WOW_MAP_MIN_PIXELS' number and its reasoning - the
# per-frame loop is pinned for an 8 x 8 float64 stack (tests/test_wow_stack_cpu.py), and a frame of a few dozen pixels
# has nothing for a batch to save.  A condition, not a measured crossover (tools/bench_wow64_stack.py has the
# measured shapes).
WOW64_MIN_PIXELS = WOW_MAP_MIN_PIXELS

# float64 stacks of at most this many frames of at least this many pixels run the per-frame loop: measured
# (tools/bench_wow64_stack.py, 2 x 4096^2 float64, denoise_coefficients=[5, 2]) the batch is 2 % behind the loop there
# host to host (13.3 against 13.0 ms, ranges apart) and 4 % device-resident; the default and bilateral cases are level
WOW64_FEW_FRAMES, WOW64_LARGE_PIXELS = 2, 1 << 24


def wow64_eligible(frames, n_scales, scaling_function=B3spline, bilateral=None, noise_per_frame=(), noise_maps=False):
    """True when the float64 batch (wt_batch64) computes wow over this stack (host logic): an (N, H, W) ndarray the
    reference computes in float64 (wavelets._result_dtype: native float64, or a type the device widens - int16 /
    uint16 / int32 / uint32 / int64, '>f4', '>f8'; native float32 stacks are wow_eligible's), a built-in scaling
    function with its own taps, noise levels that are scalars and not arrays (utils.wow takes a 0-d array as a noise
    map) or, with noise_maps=True, per-pixel noise maps of the frames' shape, n_scales (already resolved) in 1..24,
    frames of at least WOW64_MIN_PIXELS pixels whose schedule the batch runs (_lib.batch64_wow_ok: H >= 2, rows the
    fused passes take at 8 bytes per pixel, fused or single-scale stencil passes, option "stencil64" on) - except
    stacks of at most WOW64_FEW_FRAMES frames of WOW64_LARGE_PIXELS pixels or more, measured behind the loop.  With
    `bilateral`, bilateral64_eligible's conditions at level n_scales instead of the schedule's: the transform is the
    batched float64 march.  Everything else runs the per-frame loop."""
    if isinstance(n_scales, bool) or not isinstance(n_scales, (int, np.integer)) or n_scales not in WOW_LEVELS:
        return False
    if not _float64_frames(frames):
        return False
    noise_per_frame = _maps_admitted(frames, noise_per_frame, noise_maps)
    if noise_per_frame is not None and any(type(n) is np.ndarray for n in noise_per_frame):
        return False
    if not _family_noise_eligible(scaling_function, None, noise_per_frame):
        return False
    N, H, W = frames.shape
    if N < 1 or H * W < WOW64_MIN_PIXELS:
        return False
    if N <= WOW64_FEW_FRAMES and H * W >= WOW64_LARGE_PIXELS:
        return False
    fam = _family_of(scaling_function(2))
    if not _lib.batch64_wow_ok(fam, H, W, int(n_scales)):
        return False
    if bilateral is None:
        return True
    return bilateral64_eligible(frames, int(n_scales), scaling_function, bilateral, noise_per_frame)


def _plan_chunks(n, H, W, level, f64, extra_planes=0):
    """_lib.batch_chunks of a stack of `n` frames on the float32 batch or, `f64`, the float64 batch (8 bytes per
    pixel); `extra_planes`: the planes per frame beyond the transform's"""
    kw = dict(extra_planes=extra_planes) if extra_planes else {}
    if f64:
        kw["itemsize"] = 8
    return _lib.batch_chunks(n, H, W, level, **kw)


@contextmanager
def _batch(f64, n, H, W, family, level):
    """a BatchPlan or, `f64`, a BatchPlan64 of at least `n` frames from the cache of the default context, handed
    back to the cache on the way out"""
    acquire, release = (_lib.acquire_batch64, _lib.release_batch64) if f64 else (_lib.acquire_batch, _lib.release_batch)
    bp = acquire(_lib.default_context(), n, H, W, family, level)
    try:
        yield bp
    finally:
        release(bp)


def _stack_route(fr, level, scaling_function, bilateral, noise_per_frame=(), noise_maps=False):
    """(the float64 batch?, the bilateral march?) of transform_stack / denoise_stack, or None: the per-frame loop.
    The predicates overlap at their edges; the order in which they are asked is the tie-break."""
    args = (fr, level, scaling_function, bilateral, noise_per_frame, noise_maps)
    if batch64_eligible(*args):
        return True, False
    if bilateral64_eligible(*args):
        return True, True
    if bilateral_eligible(*args):
        return False, True
    if batch_eligible(*args):
        return False, False
    return None


def _f32_target(out, shape):
    """the array a float32 batch downloads into: the caller's `out` - a C-contiguous float32 array of the result's
    shape, checked before any device work - or a fresh page-locked block (the downloads land at PCIe rate)"""
    if out is None:
        return _lib.host_empty(shape)
    if out.shape != shape or out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError(f"out: float32 array of shape {shape} expected")
    return out


def _hand_over(res, out):
    """the per-frame loop's result, or a float64 batch's (_f64_target): as it is, or filled into the caller's `out`"""
    if out is None:
        return res
    out[...] = res
    return out


def _f64_target(out, shape):
    """(array the float64 batch downloads into, the caller's `out` to fill afterwards or None): a C-contiguous
    float64 `out` of the result's shape receives the downloads directly; any other `out` gets the result as the
    per-frame route hands it over (out[...] = res)"""
    if out is None:
        return _lib.host_empty(shape, dtype=np.float64), None       # page-locked: the downloads land at PCIe rate
    if isinstance(out, np.ndarray) and out.shape == shape and out.dtype == np.float64 and out.flags.c_contiguous \
            and out.flags.writeable:
        return out, None
    oshape = tuple(np.shape(out))
    try:
        fits = np.broadcast_shapes(oshape, shape) == oshape
    except ValueError:
        fits = False
    if not fits:                                                    # (checked before any device work)
        raise ValueError(f"out: an array of shape {shape} expected (got {oshape})")
    return _lib.host_empty(shape, dtype=np.float64), out


def _target(f64, out, shape):
    """(array the batch downloads into, the caller's `out` to fill afterwards or None), checked before any device work:
    _f32_target's contract for a float32 batch, _f64_target's for a float64 batch"""
    return _f64_target(out, shape) if f64 else (_f32_target(out, shape), None)


class _HostSource:
    """The frames of a stack that lies in host memory, as the chunk loops take them (_transform_chunks,
    _denoise_chunks): `shape`, and load(bp, f0, nf) - frames f0 .. f0+nf-1 into the input plane of the batch `bp`
    (integer / big-endian frames of a float64 batch: widened on the device).  resident.py has the device form."""

    def __init__(self, fr):
        self.fr = fr
        self.shape = fr.shape

    def load(self, bp, f0, nf):
        bp.upload(PLANE_INPUT, self.fr[f0:f0 + nf])


class _HostSink:
    """The result array in host memory, as the chunk loops fill it: store(bp, plane, f0, nf, index, last) - frames
    0 .. nf-1 of a plane of `bp` into res[f0:f0+nf] or, with `index`, res[f0:f0+nf, index] (straight into the caller's
    cube); `last`: the final store of the call (nothing to do here: a download is complete when it returns)."""

    def __init__(self, res):
        self.res = res

    def store(self, bp, plane, f0, nf, index=None, last=False):
        bp.download(plane, nf, out=self.res[f0:f0 + nf] if index is None else self.res[f0:f0 + nf, index])


def _transform_chunks(bp, src, chunks, level, bilateral, bilateral_scaling, sink):
    """transform_stack's device part on a BatchPlan or BatchPlan64: every chunk of frames from `src` through the
    transform, planes 0 .. level into `sink`.  `bilateral`: the batched bilateral transform's parameter, else None."""
    for f0, nf in chunks:
        src.load(bp, f0, nf)
        if bilateral is not None:                              # ref:433-442
            sb = _sigma_bilateral_list(bilateral, level)
            bp.decompose_bilateral(nf, PLANE_INPUT, level, sb, bilateral_scaling)
        else:
            bp.decompose(nf, PLANE_INPUT, level, FLAG_FUSED)
        for s in range(level + 1):
            sink.store(bp, s, f0, nf, s, last=f0 + nf == src.shape[0] and s == level)


def transform_stack(frames, level, scaling_function=B3spline, out=None, bilateral=None, bilateral_scaling=False):
    """(N, level+1, H, W) float32 (float64 for the stacks the reference computes in float64): the standard
    transform of every frame (AtrousTransform(scaling_function, bilateral, bilateral_scaling)(frame, level).data,
    ref:307-328), batched."""
    fr = _as_frames(frames)
    route = _stack_route(fr, level, scaling_function, bilateral)
    if route is None:
        return _hand_over(np.stack([AtrousTransform(scaling_function, bilateral, bilateral_scaling)(f, level).data
                                    for f in fr]), out)
    f64, bil = route                   # per frame: AtrousTransform._run's or, float64, AtrousTransform._call_f64's passes
    N, H, W = fr.shape
    res, fill = _target(f64, out, (N, level + 1, H, W))
    chunks = _plan_chunks(N, H, W, level, f64)
    with _batch(f64, max(nf for _, nf in chunks), H, W, _family_of(scaling_function(2)), level) as bp:
        _transform_chunks(bp, _HostSource(fr), chunks, level, bilateral if bil else None, bilateral_scaling, _HostSink(res))
    return _hand_over(res, fill)


def denoise_stack(frames, weights, scaling_function=B3spline, noise=None, soft_threshold=True, anscombe=False,
                  out=None, bilateral=None):
    """(N, H, W): utils.denoise of every frame (ref utils.py:83-102), batched - float32, or float64 for the stacks
    the reference computes in float64.  `noise`: None (each frame's own MAD estimate), a scalar, or one entry per
    frame - a level or a per-pixel noise map of the frames' (H, W); an (H, W) ndarray: one map shared by the frames."""
    fr = _as_frames(frames)
    N = len(fr)
    nl = _noise_list(noise, N, fr[0].shape)
    level = len(weights)
    route = _stack_route(fr, level, scaling_function, bilateral, nl, noise_maps=True)
    if route is None:
        per = nl if nl is not None else [noise] * N
        return _hand_over(np.stack([denoise(f, weights, scaling_function, n_i, bilateral, soft_threshold, anscombe)
                                    for f, n_i in zip(fr, per)]), out)
    f64, bil = route
    _, H, W = fr.shape
    res, fill = _target(f64, out, (N, H, W))
    maps = int(noise_map_eligible(fr, nl))                 # (the noise plane: one more plane per frame)
    chunks = _plan_chunks(N, H, W, level, f64, maps)
    with _batch(f64, max(nf for _, nf in chunks), H, W, _family_of(scaling_function(2)), level) as bp:
        _denoise_chunks(bp, _HostSource(fr), chunks, nl, weights, scaling_function, soft_threshold, anscombe,
                        bilateral if bil else None, _HostSink(res))
    return _hand_over(res, fill)


def _denoise_chunks(bp, src, chunks, nl, weights, scaling_function, soft_threshold, anscombe, bilateral, sink):
    """denoise_stack's device part on a BatchPlan (float32) or a BatchPlan64 (float64): every chunk of frames from
    `src` (_HostSource, or resident.py's device form) through the per-frame sequence of utils.denoise
    (wavelets._decompose_denoise_sum), results into `sink`.
    `bilateral`: the batched bilateral transform's parameter (bilateral_eligible / bilateral64_eligible), else None.
    Frames whose noise is a per-pixel map (ref wavelets.py:133-141) get the map thresholds (_map_tau_row) and their map
    in the batch's noise plane (_upload_noise_maps); no MAD estimate is taken for them."""
    bil = bilateral is not None
    shape = src.shape[1:]
    shared = _shared_map(nl, shape)
    level = len(weights)
    sf = scaling_function(2)
    sigma_e = sf.sigma_e(bilateral=bilateral)
    fam = _family_of(sf)
    sigma = list(weights)
    wgts = (1,) * len(sigma)
    # (bilateral: no fused schedule - the whole transform, then the thresholds, wavelets._decompose_denoise_sum)
    sched = [] if bil else _lib.schedule(fam, level, True)
    entries, k, covered = _interleave_split(sched, level, sigma, wgts)
    for f0, nf in chunks:
        noises = list(nl[f0:f0 + nf])
        src.load(bp, f0, nf)
        if anscombe:
            bp.anscombe(nf, PLANE_INPUT, PLANE_INPUT)                        # ref:93-94
        whole = k == 0 or k == len(sched)
        if whole:                    # transform, then Coefficients._denoise_sum over every plane
            if bil:
                sb = _sigma_bilateral_list(bilateral, level)
                bp.decompose_bilateral(nf, PLANE_INPUT, level, sb, False)
            else:
                bp.decompose(nf, PLANE_INPUT, level, FLAG_FUSED)
            used = entries
        else:                        # the passes before the threshold step (wavelets._decompose_denoise_sum)
            cur = PLANE_INPUT
            for i in range(k):
                nxt = PLANE_SCRATCH(i & 1)
                bp.decompose_pass(nf, cur, nxt, sched[i][0], sched[i][1], FLAG_FUSED)
                cur = nxt
            used = entries[:covered]
        if any(n is None for n in noises) and any(sig != 0 for _, sig, _ in used):
            med = bp.abs_median(nf, 0)                                        # ref:131-132 (lazy)
            noises = [_noise_from_median(m, sigma_e) if n is None else n for n, m in zip(noises, med)]
        has_map = [_is_noise_map(n, shape) for n in noises]
        if any(has_map):
            _upload_noise_maps(bp, nf, noises, has_map, shared, first=f0 == 0)
            taus = [_map_tau_row(used, sigma_e, soft_threshold) if m else _tau_row(used, n, sigma_e, soft_threshold)
                    for n, m in zip(noises, has_map)]
            bp.denoise_sum(nf, level + 1 if whole else covered, taus, [w for _, _, w in used], soft_threshold,
                           noise_plane=_NOISE_PLANE, has_map=has_map)
        else:
            taus = [_tau_row(used, n, sigma_e, soft_threshold) for n in noises]
            bp.denoise_sum(nf, level + 1 if whole else covered, taus, [w for _, _, w in used], soft_threshold)
        if not whole:
            for i in range(k, len(sched)):
                last = i == len(sched) - 1
                nxt = level if last else PLANE_SCRATCH(i & 1)
                bp.decompose_pass_sum(nf, cur, nxt, sched[i][0], sched[i][1], FLAG_FUSED, PLANE_OUT,
                                      first=False, last=last)
                cur = nxt
        if anscombe:
            bp.anscombe(nf, PLANE_OUT, PLANE_OUT, inverse=True)              # ref:99-100
        sink.store(bp, PLANE_OUT, f0, nf, last=f0 + nf == src.shape[0])


def _shared_map(nl, shape):
    """the one noise map every frame of the stack shares (_noise_list of an (H, W) ndarray), or None"""
    if nl and _is_noise_map(nl[0], shape) and all(n is nl[0] for n in nl):
        return nl[0]
    return None


def _upload_noise_maps(bp, nf, noises, has_map, shared, first=True):
    """The noise plane of a chunk (plane _NOISE_PLANE of a BatchPlan / BatchPlan64): frame f's slot holds its map,
    converted as Coefficients._tau converts it (the plane's element type), or ones where the frame's noise is a
    scalar; the pitch padding holds ones.  `shared` (one map for the whole stack) crosses PCIe once, for the first
    chunk - the largest - and is replicated into the frame slots on the device; later chunks find it there."""
    dtype = bp.dtype
    if shared is not None:
        if first:
            bp.fill(nf, _NOISE_PLANE, 1.0)
            bp.upload(_NOISE_PLANE, np.asarray(shared, dtype)[None])
            bp.replicate(nf, _NOISE_PLANE)
        return
    bp.fill(nf, _NOISE_PLANE, 1.0)
    for f in range(nf):                                  # each map from where it lies: no stacked host copy of the maps
        if has_map[f]:
            bp.upload(_NOISE_PLANE, np.asarray(noises[f], dtype)[None], f0=f)


def _wow_taus(bp, nf, sigma, scale, noises, sigma_e, soft):
    """(one threshold per frame, the noise levels) of wow's scale `scale` (Coefficients._tau): the frames whose
    noise is None get their MAD estimate here, where the per-frame call's lazy _tau takes it; the frames whose noise
    is a per-pixel map get the map threshold (_map_tau_row)"""
    if sigma != 0 and any(n is None for n in noises):
        med = bp.abs_median(nf, 0)                                               # ref:131-132 (lazy)
        noises = [_noise_from_median(m, sigma_e) if n is None else n for n, m in zip(noises, med)]
    shape = (bp.H, bp.W)
    entry = [(scale, sigma, None)]
    return [_map_tau_row(entry, sigma_e, soft)[0] if _is_noise_map(n, shape) else _tau_row(entry, n, sigma_e, soft)[0]
            for n in noises], noises


def wow_stack(frames, scaling_function=B3spline, n_scales=None, weights=[], whitening=True, denoise_coefficients=[],
              noise=None, bilateral=None, bilateral_scaling=False, soft_threshold=True, preserve_variance=False,
              gamma=3.2, gamma_min=None, gamma_max=None, h=0, out=None, return_coefficients=False):
    """(N, H, W): the wow image of every frame (utils.wow, ref utils.py:105-219), batched - float32 for the stacks
    the float32 batch computes, float64 for the stacks the reference computes in float64 (wow64_eligible: `out`, if
    given, a C-contiguous float64 array of the result's shape), the per-frame dtype otherwise.  `noise`: None (each frame's own MAD estimate), a scalar,
    or one entry per frame - a level or a per-pixel noise map of the frames' (H, W); an (H, W) ndarray: one map shared
    by the frames.  return_coefficients: (images, planes), planes (N, n_scales + 1, H, W) = the whitened coefficients of
    every frame (wow(...)[1].data)."""
    fr = _as_frames(frames)
    N = len(fr)
    nl = _noise_list(noise, N, fr[0].shape)
    shape = fr[0].shape
    kw = dict(weights=weights, whitening=whitening, denoise_coefficients=denoise_coefficients, bilateral=bilateral,
              bilateral_scaling=bilateral_scaling, soft_threshold=soft_threshold, preserve_variance=preserve_variance,
              gamma=gamma, gamma_min=gamma_min, gamma_max=gamma_max, h=h)
    # n_scales once for the shared shape, as wow() resolves it for one frame (ref:121-138)
    L = _wow_n_scales(shape, scaling_function, n_scales, h, denoise_coefficients)
    L = _wow_scale_limit(L, scaling_function, 2, bilateral, denoise_coefficients)
    take_maps = shape[0] * shape[1] >= WOW_MAP_MIN_PIXELS
    bil = bilateral_eligible(fr, L, scaling_function, bilateral, nl, noise_maps=take_maps)
    f32 = bil or wow_eligible(fr, L, scaling_function, bilateral, nl, noise_maps=take_maps)
    f64 = not f32 and wow64_eligible(fr, L, scaling_function, bilateral, nl, noise_maps=take_maps)
    if not f32 and not f64:
        per = nl if nl is not None else [noise] * N
        res = [wow(f, scaling_function, n_scales, noise=n_i, **kw) for f, n_i in zip(fr, per)]
        images = _hand_over(np.stack([r[0] for r in res]), out)
        return (images, np.stack([r[1].data for r in res])) if return_coefficients else images
    _, H, W = fr.shape
    nplanes = L + 1
    if f64:                                # (checked before any device work)
        if out is not None and not (isinstance(out, np.ndarray) and out.shape == (N, H, W) and out.dtype == np.float64
                                    and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError(f"out: a C-contiguous float64 array of shape {(N, H, W)} expected")
        bil = bilateral is not None
    out, _ = _target(f64, out, (N, H, W))
    planes = _lib.host_empty((N, nplanes, H, W), dtype=out.dtype) if return_coefficients else None
    maps = noise_map_eligible(fr, nl)
    # (the spare plane of the fused update, the gamma plane, the noise plane)
    extra = int(whitening and h < 1) + int(h > 0) + int(maps)
    shared = _shared_map(nl, (H, W))
    chunks = _plan_chunks(N, H, W, L, f64, extra)
    with _batch(f64, max(nf for _, nf in chunks), H, W, _family_of(scaling_function(2)), L) as bp:
        for f0, nf in chunks:
            bp.upload(PLANE_INPUT, fr[f0:f0 + nf])                  # (float64 batch: integer frames are widened on the device)
            if bil:                                                                 # ref:140-151
                sb = _sigma_bilateral_list(_wow_sigma_bilateral(bilateral, L), L)     # (wow's list, then the transform's)
                bp.decompose_bilateral(nf, PLANE_INPUT, L, sb, bilateral_scaling)
            else:
                bp.decompose(nf, PLANE_INPUT, L, FLAG_FUSED)                        # ref:148-151
            if maps:
                noises = nl[f0:f0 + nf]
                _upload_noise_maps(bp, nf, noises, [_is_noise_map(n, (H, W)) for n in noises], shared, first=f0 == 0)
            _wow_batch_device(bp, nf, nl[f0:f0 + nf], scaling_function, L, weights, whitening, denoise_coefficients,
                              soft_threshold, preserve_variance, gamma, gamma_min, gamma_max, h, bilateral)
            bp.download(PLANE_OUT, nf, out=out[f0:f0 + nf])
            if return_coefficients:
                for s in range(nplanes):
                    bp.download(s, nf, out=planes[f0:f0 + nf, s])
    return (out, planes) if return_coefficients else out


def _wow_batch_device(bp, nf, noises, scaling_function, n_scales, weights, whitening, denoise_coefficients,
                      soft_threshold, preserve_variance, gamma, gamma_min, gamma_max, h, bilateral=None):
    """The device-resident part of wow (ref:157-217, utils._wow_device / _wow_scales) for frames 0 .. nf-1 of a
    BatchPlan or BatchPlan64 whose planes 0 .. n_scales hold the transform: whitened planes in place, the images in
    PLANE_OUT; the factors in the batch's element type, as the per-frame call computes them.
    `noises`: one entry per frame (None: its MAD estimate, taken where the per-frame call's lazy _tau takes it; a
    per-pixel noise map: it lies in the batch's noise plane, _upload_noise_maps, and the scales with a non-zero sigma
    run the updates that read it).
    `bilateral`: the transform's, for the sigma_e table (Coefficients.sigma_e, ref:122-124)."""
    sigma_e = scaling_function(2).sigma_e(bilateral=bilateral)
    nplanes = n_scales + 1
    recomposition_weights, sdc = _wow_lists(weights, denoise_coefficients, n_scales)       # ref:160-170
    use_gamma = h > 0
    gplane = _GAMMA_PLANE if use_gamma else PLANE_NONE
    npix = float(bp.H) * float(bp.W)
    noises = list(noises)
    maps = any(_is_noise_map(n, (bp.H, bp.W)) for n in noises)
    if use_gamma:
        bp.fill(nf, _GAMMA_PLANE, 0.0)                                              # ref:157-158
    for s, (_, w, d) in enumerate(zip(range(nplanes), recomposition_weights, sdc)):   # ref:174
        need = _wow_needs_moments(s, n_scales, preserve_variance, whitening, h)
        moments = bp.reduce(nf, s) if need else [None] * nf
        factors = [_wow_factor(s, n_scales, w, m, npix, preserve_variance, whitening, h, bp.dtype) for m in moments]
        if s == n_scales:                                                           # ref:185-191, 203
            bp.wow_update(nf, s, [0.0] * nf, soft_threshold, factors, gplane)
            continue
        taus, noises = _wow_taus(bp, nf, d, s, noises, sigma_e, soft_threshold)    # ref:199
        # (a zero sigma: significance one, Coefficients._tau hands the per-frame update no noise plane either)
        nkw = dict(noise_plane=_NOISE_PLANE) if maps and d != 0 else {}
        if whitening and h < 1:                                                     # ref:193-196 + 199-203
            bp.wow_scale(nf, s, s, taus, soft_threshold, factors, gplane, **nkw)
        else:
            bp.wow_update(nf, s, taus, soft_threshold, factors, gplane, **nkw)
    bp.plane_sum(nf, 0, nplanes, PLANE_OUT)                                         # ref:205
    if use_gamma:                                                                   # ref:207-217
        need = gamma_min is None or gamma_max is None
        bounds = [_gamma_range(gamma_min, gamma_max, m) for m in (bp.reduce(nf, _GAMMA_PLANE) if need else [None] * nf)]
        bp.gamma_blend(nf, PLANE_OUT, _GAMMA_PLANE, [b[0] for b in bounds], [b[1] for b in bounds], 1 / gamma, h)


# ---------------------------------------------------------------------------------------------------------------
# enhance over stacks of gray or colour frames (utils.enhance, ref utils.py:36-80)
# ---------------------------------------------------------------------------------------------------------------
ENHANCE_LEVELS = range(1, _lib.MAX_SUM_PLANES)      # level + 1 planes in one launch of the thresholded weighted sum


# float64 groups of at most this many frames of at least this many pixels run the per-frame loop: measured
# (tools/bench_enhance_stack.py, 1 x 3 x 2048^2 float64, device-resident) the batch is 5 % behind the loop there
ENHANCE64_FEW_FRAMES, ENHANCE64_LARGE_PIXELS = 3, 1 << 22


def enhance_eligible(frames, level, scaling_function=B3spline, bilateral=None, noise_per_frame=(), channels=1):
    """The route one group of enhance_stack takes (host logic) - the frames and channels of one level, `frames` their
    (n, H, W) stack, `noise_per_frame` their given noise levels (empty: none given, every frame its MAD estimate):
    'batch64' (batch64_eligible: the float64 batch), 'bilateral' (bilateral_eligible: the float32 batch behind the
    batched bilateral march), 'batch' (the float32 batch: _engine_eligible frames, the fused passes or, where the
    schedule has none, the batched per-scale stencil), or None: the per-frame loop of utils.enhance.  The existing
    predicates decide; on top of them 1 <= level <= 15 (level + 1 planes in one launch of the sum) and given noise
    levels that are scalars - no None (utils.enhance would estimate that one lazily), no array (a noise map).
    `channels`: the channels of every frame that the group holds (its batch has len(frames) * channels frames); a
    float64 group of at most ENHANCE64_FEW_FRAMES frames of ENHANCE64_LARGE_PIXELS pixels or more goes to the loop."""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level not in ENHANCE_LEVELS:
        return None
    if noise_per_frame is None or any(n is None or type(n) is np.ndarray for n in noise_per_frame):
        return None
    if batch64_eligible(frames, level, scaling_function, bilateral, noise_per_frame):
        few = len(frames) * channels <= ENHANCE64_FEW_FRAMES
        return None if few and frames.shape[1] * frames.shape[2] >= ENHANCE64_LARGE_PIXELS else 'batch64'
    if bilateral_eligible(frames, level, scaling_function, bilateral, noise_per_frame):
        return 'bilateral'
    if bilateral is None and _engine_eligible(frames, scaling_function, None, noise_per_frame):
        return 'batch'
    return None


def _as_enhance_frames(frames):
    """(frames, colour): an (N, H, W) or (N, 3, H, W) array - as given, or stacked from a sequence of 2-D or
    (3, H, W) frames of one shape and element type (mixed element types: the list, for the per-frame loop)"""
    if isinstance(frames, np.ndarray):
        fr = frames
    else:
        fr = [np.asarray(f) for f in frames]
        if len({f.shape for f in fr}) > 1:
            raise ValueError(f"frames: all frames must have one shape (got {sorted({f.shape for f in fr})})")
        if len({f.dtype for f in fr}) == 1:
            fr = np.stack(fr)
    if len(fr) == 0:
        raise ValueError("frames: an empty stack")
    shape = fr[0].shape
    if len(shape) == 2:
        return fr, False
    if len(shape) == 3 and shape[0] == 3:
        return fr, True
    raise ValueError(f"frames: (N, H, W) gray or (N, 3, H, W) colour frames (got frames of shape {shape})")


def _enhance_noise(noise, n, colour):
    """enhance_stack's `noise` as one entry per frame - what frame i's utils.enhance call gets as its second
    argument - or None when no noise is given.  Gray stacks: denoise_stack's forms (a scalar, one entry per frame;
    a noise map goes to every frame).  Colour stacks: three entries (the reference's args[1][c], shared by the
    frames) or an (N, 3) array / nested sequence (frame i gets noise[i]); with two more axes, noise maps."""
    if noise is None:
        return None
    if not colour:
        per = _noise_list(noise, n)
        return [noise] * n if per is None else per
    nd = np.ndim(noise)
    if nd in (1, 3) and len(noise) == 3:
        return [noise] * n
    if nd in (2, 4) and len(noise) == n and all(len(row) == 3 for row in noise):
        return [noise[i] for i in range(n)]
    raise ValueError(f"noise: three entries (one per channel) or an ({n}, 3) array for a stack of {n} colour frames")


def _enhance_groups(plans):
    """{level: [channel, ...]} of utils._enhance_lists' (channel, sigmas, weights): a channel's level is
    len(weights) (ref:70); the frames and channels of one level run as one batch"""
    groups = {}
    for c, _, wgt in plans:
        groups.setdefault(len(wgt), []).append(c)
    return groups


def enhance_stack(frames, noise=None, *, weights=None, denoise=None, soft_threshold=True, out=None, **kwargs):
    """(N, H, W) for gray frames, (N, 3, H, W) for colour frames (channel axis first, as the reference indexes
    img[c]): utils.enhance of every frame (ref utils.py:36-80), batched - result[i] equals
    enhance(frames[i], [noise_i,] weights=weights, denoise=denoise, soft_threshold=soft_threshold, **kwargs) bit
    for bit, float32 or, for the stacks the reference computes in float64, float64.  `noise`: None (every frame and
    channel its own MAD estimate); gray: a scalar or one per frame; colour: three entries (per channel) or (N, 3).
    kwargs go to AtrousTransform (scaling_function_class, bilateral, bilateral_scaling).

    Per chunk: upload, transform, the MAD medians of all frames in one round trip (whenever no noise is given, as
    enhance calls get_noise()), one threshold row and one weight row per frame, the thresholded weighted sum of
    all planes in one launch (wt_batch_enhance_sum), download.  The channels of one level are frames of one batch;
    channels of different levels run one batch each (enhance_eligible: the route, or the per-frame loop)."""
    fr, colour = _as_enhance_frames(frames)
    N = len(fr)
    per = _enhance_noise(noise, N, colour)
    atrous = AtrousTransform(**kwargs)
    sfc, bilateral = atrous.scaling_function_class, atrous.bilateral
    # the parameter lists depend on the call's arguments only: once per stack
    plans = _enhance_lists(3 if colour else 2, weights, denoise)
    groups = _enhance_groups(plans)
    routes = {}
    if isinstance(fr, np.ndarray):
        for level, chans in groups.items():
            given = () if per is None else [p if c is Ellipsis else p[c] for p in per for c in chans]
            routes[level] = enhance_eligible(fr if not colour else fr[:, 0], level, sfc, bilateral, given, len(chans))
    if not routes or any(r is None for r in routes.values()):
        kw = dict(weights=weights, denoise=denoise, soft_threshold=soft_threshold, **kwargs)
        res = np.stack([enhance(f, **kw) if per is None else enhance(f, n_i, **kw) for f, n_i in zip(fr, per or [None] * N)])
        return _hand_over(res, out)
    f64 = 'batch64' in routes.values()                     # (one element type: every group takes the same engine)
    res, fill = _target(f64, out, fr.shape)
    for level, chans in groups.items():
        _enhance_group(fr, res, per, [p for p in plans if p[0] in chans], level, routes[level], atrous, soft_threshold)
    return _hand_over(res, fill)


def _enhance_group(fr, res, per, plans, level, route, atrous, soft_threshold):
    """One group of enhance_stack on a BatchPlan / BatchPlan64: the channels `plans` (utils._enhance_lists' entries
    of one level) of every frame of `fr`, results into `res`.  A chunk holds m images = m * len(plans) batch
    frames: image-major (frame i, channel c at i * 3 + c) when the group is all three channels of a C-contiguous
    stack - one upload and one download per chunk - else channel-major (channel j's frames at j * m ...)."""
    f64 = route == 'batch64'
    bil = route == 'bilateral'
    N = len(fr)
    H, W = fr.shape[-2:]
    k = len(plans)
    sf = atrous.scaling_function_class(2)
    fam = _family_of(sf)
    sigma_e = sf.sigma_e(bilateral=atrous.bilateral if bil else None)
    # ref:76 per channel: Coefficients.denoise's zip over (scale, sigma, weight), padded to the level's rows with
    # sigma 0 / weight 1 (a plane times 1.0: the plane) when a shared list has grown past a channel's own
    entries = [list(zip(range(level + 1), dns, wgt)) for _, dns, wgt in plans]
    entries = [e + [(s, 0, 1) for s in range(len(e), level)] for e in entries]
    wrows = [[w for _, _, w in e] for e in entries]
    whole = k == 3 and fr.flags.c_contiguous and res.flags.c_contiguous
    frames_max = _plan_chunks(N * k, H, W, level, f64)[0][1]
    m = max(1, frames_max // k)                                      # images per chunk
    with _batch(f64, min(m, N) * k, H, W, fam, level) as bp:
        for i0 in range(0, N, m):
            n = min(m, N - i0)
            nf = n * k
            # (batch frame -> (image, index into plans))
            order = [(i, j) for i in range(n) for j in range(k)] if whole else [(i, j) for j in range(k) for i in range(n)]
            if whole:
                bp.upload(PLANE_INPUT, fr[i0:i0 + n].reshape(nf, H, W))
            else:
                for j, (c, _, _) in enumerate(plans):
                    bp.upload(PLANE_INPUT, fr[i0:i0 + n] if c is Ellipsis else fr[i0:i0 + n, c], f0=j * n)
            if bil:                                                      # ref:70, AtrousTransform._run
                sb = _sigma_bilateral_list(atrous.bilateral, level)
                bp.decompose_bilateral(nf, PLANE_INPUT, level, sb, atrous.bilateral_scaling)
            else:
                bp.decompose(nf, PLANE_INPUT, level, FLAG_FUSED)
            if per is None:                                              # ref:74: get_noise(), eagerly
                noises = [_noise_from_median(md, sigma_e) for md in bp.abs_median(nf, 0)]
            else:                                                        # ref:72
                noises = [per[i0 + i] if plans[j][0] is Ellipsis else per[i0 + i][plans[j][0]] for i, j in order]
            taus = [_tau_row(entries[j], nz, sigma_e, soft_threshold) for (_, j), nz in zip(order, noises)]
            bp.enhance_sum(nf, level + 1, taus, [wrows[j] for _, j in order], soft_threshold)   # ref:76-78
            if whole:
                bp.download(PLANE_OUT, nf, out=res[i0:i0 + n].reshape(nf, H, W))
            else:
                for j, (c, _, _) in enumerate(plans):
                    bp.download(PLANE_OUT, n, out=res[i0:i0 + n] if c is Ellipsis else res[i0:i0 + n, c], f0=j * n)


# ---------------------------------------------------------------------------------------------------------------
# richardson_lucy over stacks of frames with one PSF (utils.richardson_lucy, ref utils.py:222-290)
# ---------------------------------------------------------------------------------------------------------------
# planes per frame of a richardson_lucy chunk beyond batch_frame_bytes' level + 5: data, psi, phi, residual and
# correlation, one support plane per scale (2 * level + 9 in all, the input and output planes counted though unused)
def _rl_extra_planes(level):
    return level + 4


# ... and of the FFT route: the two complex work arrays of wt_batch_fft_apply on top, 8 * H * W bytes per frame each -
# at most two real planes of 4 * H * P bytes (P >= W), four in all (the one spectrum and the twiddles are not per frame)
def _rl_fft_extra_planes(level):
    return _rl_extra_planes(level) + 4


def _rl_frames_eligible(frames, level, uniform_init):
    """the clauses rl_eligible and rl_fft_eligible share: level, uniform_init, native float32 (N, H, W) frames"""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level not in BATCH_LEVELS:
        return False
    if uniform_init:
        return False
    return isinstance(frames, np.ndarray) and _engine_eligible(frames, B3spline, None, [None] * len(frames))


def rl_eligible(frames, psf, level, uniform_init=False, fft=False):
    """True when the batched engine computes richardson_lucy over this stack (host logic): native float32 frames in
    an (N, H, W) array (_engine_eligible), level = len(denoise_coefficients) with an all-fused schedule (2..8), no
    uniform_init, and a 2-D PSF whose two operands (utils._rl_direct_operands: with fft=True an odd height or a
    one-row PSF adds a zero row) the per-frame call applies in a single launch without bands (_lib.batch_psf_ok:
    at most 4096 taps in rows of at most 512, an LDS tile of at most 96 KB).  With fft=True also
    kh * kw < utils._FFT_MIN_TAPS, kh <= H and kw <= W: the per-frame call then takes the direct periodic form (no
    FFT, and an extended frame is never worth it below that many taps).  Everything else runs the per-frame loop
    (large PSFs with fft=True: rl_fft_eligible, the batched FFT products)."""
    if not _rl_frames_eligible(frames, level, uniform_init):
        return False
    psf = np.asarray(psf)
    if psf.ndim != 2 or psf.dtype.kind not in "biuf" or psf.size == 0:
        return False
    H, W = frames.shape[1:]
    kh, kw = psf.shape
    if fft and (kh * kw >= _utils._FFT_MIN_TAPS or kh > H or kw > W):
        return False
    (fwd_k, _), (bwd_k, _) = _rl_direct_operands(psf, H, fft)
    return _lib.batch_psf_ok(*fwd_k.shape) and _lib.batch_psf_ok(*bwd_k.shape)


def rl_fft_eligible(frames, psf, level, uniform_init=False):
    """True when the batched engine computes richardson_lucy(fft=True) over this stack through the batched FFT
    products (host logic; BatchPlan.fft_spectrum / fft_apply): rl_eligible's clauses on frames, level and uniform_init,
    and a 2-D numeric PSF the per-frame call hands to the engine's FFT on the image itself (utils._rl_uses_fft, the
    per-frame call's own rule): kh * kw >= utils._FFT_MIN_TAPS (read when called), kh <= H, kw <= W, sides the FFT
    takes (_lib.batch_fft_ok: 2 .. 8192, no prime factor above 5), no forced extended frame - and an even width, the
    only one fft=True is defined for.  Sides with a larger prime factor (the periodically extended frame), float64 and
    integer stacks, per-frame PSFs and uniform_init keep the per-frame loop."""
    if not _rl_frames_eligible(frames, level, uniform_init):
        return False
    psf = np.asarray(psf)
    if psf.ndim != 2 or psf.dtype.kind not in "biuf" or psf.size == 0:
        return False
    H, W = frames.shape[1:]
    if W % 2:
        return False
    return _rl_uses_fft(True, H, W, psf.shape[0], psf.shape[1], sides_ok=_lib.batch_fft_ok)


# richardson_lucy_stack takes float64 stacks from this many pixels per frame on: WOW64_MIN_PIXELS' number and its
# reasoning - the per-frame loop is pinned for a 3 x 12 x 16 float64 stack (tests/test_rl_stack_cpu.py), and a frame of
# a few hundred pixels has nothing for a batch to save.  A condition, not a measured crossover
# (tools/bench_rl_stack.py --dtype float64 has the measured shapes).
RL64_MIN_PIXELS = WOW_MAP_MIN_PIXELS


def rl64_eligible(frames, psf, level, uniform_init=False, fft=False):
    """True when the float64 batch (wt_batch64) computes richardson_lucy over this stack (host logic): an (N, H, W)
    ndarray the reference computes in float64 (_float64_frames: native float64, or int16 / uint16 / int32 / uint32 /
    int64 / '>f4' / '>f8', widened on the device), level = len(denoise_coefficients) in 2..8 with an all-fused float64
    schedule for these frames (_lib.batch64_fused_ok), no uniform_init (the reference then keeps the estimate in
    float32, and the per-frame call leaves the float64 engine), a 2-D numeric PSF whose two operands
    (utils._rl_direct_operands) the tiled float64 correlation applies in one launch (_lib.batch64_psf_ok: at most
    4096 taps in rows of at most 512, an LDS tile of doubles of at most 96 KB), and frames of at least RL64_MIN_PIXELS
    pixels.  With fft=True also rl_eligible's direct-periodic clauses: kh * kw < utils._FFT_MIN_TAPS, kh <= H,
    kw <= W.  Everything else - the float64 FFT products among it - runs the per-frame loop."""
    if not _float64_frames(frames):
        return False
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level not in BATCH_LEVELS:
        return False
    if uniform_init:
        return False
    N, H, W = frames.shape
    if N < 1 or H * W < RL64_MIN_PIXELS or not _lib.batch64_fused_ok(_family_of(B3spline(2)), H, W, int(level)):
        return False
    psf = np.asarray(psf)
    if psf.ndim != 2 or psf.dtype.kind not in "biuf" or psf.size == 0:
        return False
    kh, kw = psf.shape
    if fft and (kh * kw >= _utils._FFT_MIN_TAPS or kh > H or kw > W):
        return False
    (fwd_k, _), (bwd_k, _) = _rl_direct_operands(psf, H, fft)
    return _lib.batch64_psf_ok(*fwd_k.shape) and _lib.batch64_psf_ok(*bwd_k.shape)


@contextmanager
def _rl_batch(f64, n, H, W, family, level):
    """_batch for richardson_lucy_stack: the float64 batch is the one with richardson_lucy's operations (RLBatchPlan64)"""
    if not f64:
        with _batch(False, n, H, W, family, level) as bp:
            yield bp
        return
    bp = _lib.acquire_rl_batch64(_lib.default_context(), n, H, W, family, level)
    try:
        yield bp
    finally:
        _lib.release_rl_batch64(bp)


def richardson_lucy_stack(frames, psf, iterations=10, denoise_coefficients=(5, 2, 1), threshold_type='soft',
                          uniform_init=False, persistent_mrs=True, fft=False, out=None):
    """(N, H, W): utils.richardson_lucy of every frame with the one PSF `psf` (ref utils.py:222-290), batched -
    result[i] equals richardson_lucy(frames[i], psf, iterations, denoise_coefficients, threshold_type, uniform_init,
    persistent_mrs, fft) bit for bit.

    Per chunk (rl_eligible stacks): upload, transform, the MAD medians of all frames in one round trip, the
    thresholded sum as the initial estimate; then per iteration the PSF correlation of all frames in one launch
    (the two operands lie in the batch: no stream drain, no PSF copy), the residual, its transform, one support
    update per scale with each frame's threshold, the plane sum, the ratio, the second correlation and the product
    - nothing returns to the host until the chunk's estimates.  fft=True with a PSF of utils._FFT_MIN_TAPS taps or
    more (rl_fft_eligible stacks): the same chunk loop with the two products through the batched FFT - the spectrum
    of the periodically placed PSF once per call, then six launches per product for all frames of a chunk.
    Stacks the reference computes in float64 - float64, integer and big-endian frames - take the same chunk loop on
    the float64 batch (rl64_eligible stacks): double planes, the PSF as doubles, the tiled float64 correlation, a
    float64 result.  The float64 FFT products (fft=True with a PSF of utils._FFT_MIN_TAPS taps or more) are not
    batched: they stay on the per-frame loop, as does everything else."""
    fr = _as_frames(frames)
    if np.ndim(psf) != 2:
        raise ValueError("psf must be 2-D")
    _rl_check_fft_width(fft, fr[0].shape[1])
    level = len(denoise_coefficients)
    direct = rl_eligible(fr, psf, level, uniform_init, fft)
    by_fft = not direct and bool(fft) and rl_fft_eligible(fr, psf, level, uniform_init)
    f64 = not direct and not by_fft and rl64_eligible(fr, psf, level, uniform_init, fft)
    if f64:
        direct = True
    if not direct and not by_fft:
        return _hand_over(np.stack([richardson_lucy(f, psf, iterations=iterations, denoise_coefficients=denoise_coefficients,
                                                    threshold_type=threshold_type, uniform_init=uniform_init,
                                                    persistent_mrs=persistent_mrs, fft=fft) for f in fr]), out)
    N, H, W = fr.shape
    out, caller_out = _target(f64, out, (N, H, W))
    soft = threshold_type == 'soft'
    sf = B3spline(2)                                                             # ref:229 default transform
    sigma_e = sf.sigma_e()
    DATA, PSI, PHI, RES, CONV = (PLANE_SCRATCH(i) for i in (6, 7, 8, 9, 10))     # (the per-frame call's plane ids)
    MRS = [PLANE_SCRATCH(16 + s) for s in range(level)]
    kernel = np.ascontiguousarray(psf, dtype=np.float64 if f64 else np.float32)     # (the per-frame call's cast)
    if direct:
        (fwd_k, fwd), (bwd_k, bwd) = _rl_direct_operands(kernel, H, fft)
    # Coefficients._denoise_sum(list(denoise_coefficients)): the (scale, sigma, weight) entries of the initial estimate
    entries = list(zip(range(level + 1), denoise_coefficients, (1,) * level))
    chunks = _plan_chunks(N, H, W, level, f64, (_rl_extra_planes if direct else _rl_fft_extra_planes)(level))
    with _rl_batch(f64, max(nf for _, nf in chunks), H, W, _family_of(sf), level) as bp:
        if direct:
            bp.set_psf(0, fwd_k)
            bp.set_psf(1, bwd_k)
        else:                                                                    # ref:246-251, once for every chunk
            bp.upload(CONV, _rl_fft_kernel_image(kernel, H, W)[None])
            bp.fft_spectrum(CONV)
        for f0, nf in chunks:
            bp.upload(DATA, fr[f0:f0 + nf])
            bp.decompose(nf, DATA, level, FLAG_FUSED)                            # ref:230
            noises = [None] * nf
            if any(c != 0 for c in denoise_coefficients):                        # ref:131-132 (lazy, Coefficients._tau)
                noises = [_noise_from_median(m, sigma_e) for m in bp.abs_median(nf, 0)]
            taus = [_tau_row(entries, n, sigma_e, soft) for n in noises]
            bp.denoise_sum(nf, level + 1, taus, [w for _, _, w in entries], soft, write_back=True, dst=PSI)   # ref:236-237
            for m in MRS:                                                        # ref:240-243
                bp.fill(nf, m, 1.0 if soft else 0.0)
            # the data's noise serves every iteration (ref:262): one threshold per frame and scale
            scale_taus = [[_tau_row([(s, c, None)], n, sigma_e, soft)[0] for n in noises]
                          for s, c in enumerate(denoise_coefficients)]
            for iteration in range(iterations):                                  # ref:252
                if direct:
                    bp.filter2d(nf, PSI, PHI, 0, **fwd)                          # ref:254-257
                else:
                    bp.fft_apply(nf, PSI, PHI, False)                            # ref:254
                bp.binary(nf, "sub", DATA, PHI, RES)                             # ref:259
                bp.decompose(nf, RES, level, FLAG_FUSED)                         # ref:261
                for s in range(level):                                           # ref:263-276
                    bp.mrs_update(nf, s, MRS[s], scale_taus[s], soft, persistent_mrs, 1.0 / (iteration + 1))
                bp.plane_sum(nf, 0, level + 1, RES)                              # ref:278
                bp.binary(nf, "add_div", RES, PHI, RES)                          # ref:280-281
                if direct:
                    bp.filter2d(nf, RES, CONV, 1, **bwd)                         # ref:284-286
                else:
                    bp.fft_apply(nf, RES, CONV, True)                            # ref:284
                bp.binary(nf, "mul", PSI, CONV, PSI)                             # ref:288
            bp.download(PSI, nf, out=out[f0:f0 + nf])
    return out if caller_out is None else _hand_over(out, caller_out)
