"""Stacks of same-shape frames through the batched engine (wt_batch): every fused pass of the schedule runs
over all frames of a chunk in ONE launch (the frame is a grid dimension), the MAD medians of all frames come
back in one host round trip, and the pointwise steps run once over the stack.

    transform_stack(frames, level)      == np.stack([AtrousTransform(sf)(f, level).data for f in frames])
    denoise_stack(frames, weights)      == np.stack([denoise(f, weights, sf, noise_i, ...) for f in frames])

bit for bit.  The sequence of operations per frame is the per-frame path's own (wavelets._interleave_split,
_scalar_tau, _noise_from_median).  Inputs the batched engine does not cover run the per-frame loop
(batch_eligible says which)."""
import numpy as np

from . import _lib
from ._lib import PLANE_INPUT, PLANE_OUT, PLANE_SCRATCH, FLAG_FUSED
from .wavelets import (AtrousTransform, B3spline, _family_of, _needs_generic, _interleave_split, _scalar_tau,
                       _noise_from_median)
from .utils import denoise

__all__ = ['transform_stack', 'denoise_stack', 'batch_eligible']

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


def _noise_list(noise, n):
    """one noise entry per frame (None: that frame's own MAD estimate)"""
    if noise is None or np.ndim(noise) == 0:
        return [noise] * n
    if isinstance(noise, np.ndarray) and noise.ndim != 1:
        return None                       # a noise map: the per-frame loop (a 1-D array: one level per frame)
    noise = list(noise)
    if len(noise) != n:
        raise ValueError(f"noise: one entry per frame ({n} frames, {len(noise)} entries)")
    return noise


def batch_eligible(frames, level, scaling_function=B3spline, bilateral=None, noise_per_frame=()):
    """True when the batched engine computes this stack (host logic): native float32 frames of one shape in an
    (N, H, W) array, no bilateral filtering, a built-in scaling function with its own taps, a level with an
    all-fused schedule (2..8) and scalar noise levels.  Everything else runs the per-frame loop."""
    if not isinstance(frames, np.ndarray) or frames.ndim != 3 or frames.dtype != np.dtype(np.float32) \
            or not frames.dtype.isnative:
        return False
    if bilateral is not None or level not in BATCH_LEVELS:
        return False
    if _needs_generic(scaling_function):
        return False
    try:
        if not isinstance(_family_of(scaling_function(2)), int):
            return False
    except (ValueError, NotImplementedError):
        return False
    if noise_per_frame is None or any(n is not None and np.ndim(n) != 0 for n in noise_per_frame):
        return False
    H, W = frames.shape[1:]
    return H >= 1 and W >= 1 and (W + 3) // 4 * 4 * 4 * 64 * 48 < (1 << 31)   # wt_fused_supported


def _chunks(frames, level):
    N, H, W = frames.shape
    return _lib.batch_chunks(N, H, W, level)


def transform_stack(frames, level, scaling_function=B3spline, out=None):
    """(N, level+1, H, W) float32: the standard transform of every frame (AtrousTransform(scaling_function)
    (frame, level).data, ref:307-328), batched."""
    fr = _as_frames(frames)
    if not batch_eligible(fr, level, scaling_function):
        res = np.stack([AtrousTransform(scaling_function)(f, level).data for f in fr])
        if out is not None:
            out[...] = res
            return out
        return res
    N, H, W = fr.shape
    if out is None:
        out = _lib.host_empty((N, level + 1, H, W))          # page-locked: the downloads land at PCIe rate
    elif out.shape != (N, level + 1, H, W) or out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError(f"out: float32 array of shape {(N, level + 1, H, W)} expected")
    if N == 0:
        return out
    ctx = _lib.default_context()
    fam = _family_of(scaling_function(2))
    chunks = _chunks(fr, level)
    bp = _lib.acquire_batch(ctx, max(nf for _, nf in chunks), H, W, fam, level)
    try:
        for f0, nf in chunks:
            bp.upload(PLANE_INPUT, fr[f0:f0 + nf])
            bp.decompose(nf, PLANE_INPUT, level, FLAG_FUSED)
            for s in range(level + 1):
                bp.download(s, nf, out=out[f0:f0 + nf, s])         # straight into the caller's cube
    finally:
        _lib.release_batch(bp)
    return out


def _taus_of(entries, noise, sigma_e, soft):
    """one frame's threshold row over `entries` (Coefficients._tau, scalar noise): 0.0 = significance one"""
    row = []
    for scl, sig, _ in entries:
        t = None if sig == 0 else _scalar_tau(sig, noise, sigma_e[scl], soft)
        row.append(0.0 if t is None else t[0])
    return row


def denoise_stack(frames, weights, scaling_function=B3spline, noise=None, soft_threshold=True, anscombe=False,
                  out=None, bilateral=None):
    """(N, H, W): utils.denoise of every frame (ref utils.py:83-102), batched.  `noise`: None (each frame's
    own MAD estimate), a scalar, or one entry per frame."""
    fr = _as_frames(frames)
    N = len(fr)
    nl = _noise_list(noise, N)
    level = len(weights)
    if not batch_eligible(fr, level, scaling_function, bilateral, nl):
        per = nl if nl is not None else [noise] * N
        res = np.stack([denoise(f, weights, scaling_function, n_i, bilateral, soft_threshold, anscombe)
                        for f, n_i in zip(fr, per)])
        if out is not None:
            out[...] = res
            return out
        return res
    _, H, W = fr.shape
    if out is None:
        out = _lib.host_empty((N, H, W))                     # page-locked (as denoise(): _download_to)
    elif out.shape != (N, H, W) or out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError(f"out: float32 array of shape {(N, H, W)} expected")
    if N == 0:
        return out
    ctx = _lib.default_context()
    sf = scaling_function(2)
    sigma_e = sf.sigma_e()
    fam = _family_of(sf)
    sigma = list(weights)
    wgts = (1,) * len(sigma)
    sched = _lib.schedule(fam, level, True)
    entries, k, covered = _interleave_split(sched, level, sigma, wgts)
    chunks = _chunks(fr, level)
    bp = _lib.acquire_batch(ctx, max(nf for _, nf in chunks), H, W, fam, level)
    try:
        for f0, nf in chunks:
            noises = list(nl[f0:f0 + nf])
            bp.upload(PLANE_INPUT, fr[f0:f0 + nf])
            if anscombe:
                bp.anscombe(nf, PLANE_INPUT, PLANE_INPUT)                        # ref:93-94
            whole = k == 0 or k == len(sched)
            if whole:                    # transform, then Coefficients._denoise_sum over every plane
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
            taus = [_taus_of(used, n, sigma_e, soft_threshold) for n in noises]
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
            bp.download(PLANE_OUT, nf, out=out[f0:f0 + nf])
    finally:
        _lib.release_batch(bp)
    return out
