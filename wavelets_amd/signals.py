"""Stacks of 1-D signals of one length - the spectra of a spectrograph frame, the light curves of a survey, detector
rows - through the signal engine (wt_signals): ONE launch transforms every signal of a chunk, a workgroup per signal
with the scales of its signal in LDS, the MAD medians of all signals come back in one host round trip, and the
thresholded sum runs once over the stack.

    transform_signals(signals, level)  == np.stack([AtrousTransform(sf)(s, level).data for s in signals])
    denoise_signals(signals, weights)  == np.stack([denoise(s, weights, sf, noise_i, ...) for s in signals])

bit for bit.  The reference transforms a signal in the 1-D branch of convolution() (ref wavelets.py:65-69, scipy's
'mirror' border); the per-signal call runs it as a 1 x N image, a launch per scale and an upload and a download per
call.  The thresholds are the per-signal path's own (wavelets._interleave_split, _tau_row, _noise_from_median).

Non-finite samples are data, as in the per-signal call, and nothing is raised for them: NaN spreads through the
filter's reach, an inf becomes NaN in w_0, and the MAD median is the middle key of the sorted magnitudes with NaN above
infinity - finite while fewer than half of |w_0| are NaN (np.median would say NaN), else NaN, which gives NaN
thresholds and leaves that signal unthresholded.  Other signals of the stack are not touched ("Non-finite
samples in the 1-D engines").

Inputs the engine does not cover run the per-signal loop and return what the loop returns; signals_eligible says
which."""
import numpy as np

from . import _lib
from .wavelets import (AtrousTransform, B3spline, _family_of, _needs_generic, _interleave_split, _tau_row,
                       _noise_from_median, _result_dtype)
from .utils import denoise
from .batch import _real_scalar

__all__ = ['transform_signals', 'denoise_signals', 'signals_eligible']


def _as_signals(signals):
    """(M, N) view / array of the signals, or ValueError: an (M, N) array or a sequence of 1-D arrays of one length
    (a sequence of mixed element types stays a list: the per-signal loop)"""
    if isinstance(signals, np.ndarray):
        if signals.ndim != 2 or signals.shape[0] == 0:
            raise ValueError(f"signals: a non-empty (M, N) array or a sequence of 1-D arrays (got shape {signals.shape})")
        return signals
    items = [np.asarray(s) for s in signals]
    if any(s.ndim != 1 for s in items):
        raise ValueError("signals: every signal must be a 1-D array")
    if len({s.shape for s in items}) > 1:
        raise ValueError(f"signals: all signals must have one length (got {sorted({s.shape[0] for s in items})})")
    if not items:
        raise ValueError("signals: an empty stack")
    if len({s.dtype for s in items}) > 1:
        return items                      # mixed element types: the per-signal loop (not eligible)
    return np.stack(items)


def _noise_list(noise, n):
    """one noise entry per signal (None: that signal's own MAD estimate): None or a scalar for all of them, or a list /
    tuple of one entry per signal; an ndarray is handed whole to every signal (a per-sample noise map of denoise())"""
    if isinstance(noise, (list, tuple)):
        if len(noise) != n:
            raise ValueError(f"noise: one entry per signal ({n} signals, {len(noise)} entries)")
        return list(noise)
    return [noise] * n


def _engine_family(dtype, level, scaling_function):
    """the family (an int) the 1-D engines run this element type, level and scaling function with, or None: native
    float32 or native float64; an int level (not a bool), 1 <= level <= 24; a built-in scaling function with its own taps"""
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)) or not dtype.isnative:
        return None
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 1 <= level <= _lib.SIGNAL_MAX_LEVEL:
        return None
    if _needs_generic(scaling_function):
        return None
    try:
        fam = _family_of(scaling_function(1), 1)
    except (ValueError, NotImplementedError):
        return None
    return fam if isinstance(fam, int) else None


def _signals_family(signals, level, scaling_function, noise_per_signal=()):
    """the family the signal engine computes this stack with, or None (signals_eligible)"""
    if not isinstance(signals, np.ndarray) or signals.ndim != 2 or signals.shape[0] < 1 or signals.shape[1] < 1:
        return None
    fam = _engine_family(signals.dtype, level, scaling_function)
    if fam is None or noise_per_signal is None or any(n is not None and not _real_scalar(n) for n in noise_per_signal):
        return None
    return fam if _lib.signals_ok(fam, signals.shape[1], int(level), signals.dtype.itemsize) else None


def signals_eligible(signals, level, scaling_function=B3spline, noise_per_signal=()):
    """True when the signal engine computes this stack (host logic): an (M, N) ndarray, M >= 1 and N >= 1, of native
    float32 or native float64; a built-in scaling function with its own taps; an int level, 1 <= level <= 24; signals
    within the LDS budget of the kernel (_lib.signals_ok: at most 8192 float32 or 4096 float64 samples); noise
    entries that are None or real scalars.  Everything else runs the per-signal loop."""
    return _signals_family(signals, level, scaling_function, noise_per_signal) is not None


def _transform_one(signal, level, scaling_function):
    """the per-signal call of transform_signals"""
    return AtrousTransform(scaling_function)(signal, level).data


def _loop_dtype(sig):
    """element type of the per-signal loop's result: what every per-signal call hands back, stacked"""
    if isinstance(sig, np.ndarray):
        return _result_dtype(sig)
    return np.result_type(*[_result_dtype(s) for s in sig])


def _target(out, shape, dtype):
    """the caller's `out`, checked before any device work: a writable C-contiguous ndarray of the result's shape and
    element type, or ValueError; None stays None"""
    if out is None:
        return None
    if not isinstance(out, np.ndarray) or out.shape != tuple(shape) or out.dtype != np.dtype(dtype) \
            or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError(f"out: a writable C-contiguous {np.dtype(dtype)} array of shape {tuple(shape)} expected")
    return out


def _hand_over(res, out):
    if out is None:
        return res
    out[...] = res
    return out


def _result(res, shape, dtype):
    """(the checked `out`, or without one a page-locked block for the result: the downloads land at PCIe rate; the context)"""
    ctx = _lib.default_context()
    return (_lib.host_empty(shape, ctx, dtype) if res is None else res), ctx


def _thresholds(weights, scaling_function):
    """(sigma_e, entries, whether any threshold needs a noise level) of Coefficients._denoise_sum(weights): sigma = weights,
    every weight 1, no fused schedule for a signal"""
    entries, _, _ = _interleave_split([], len(weights), list(weights), (1,) * len(weights))
    return scaling_function(1).sigma_e(), entries, any(s != 0 for _, s, _ in entries)


def _chunks(M, N, level, itemsize):
    """the chunk rule of a stack over device memory (_lib.signal_chunks)"""
    return _lib.signal_chunks(M, N, level, itemsize=itemsize)


def transform_signals(signals, level, scaling_function=B3spline, out=None):
    """(M, level + 1, N), float32 or - for the stacks the reference computes in float64 - float64: the standard
    transform of every signal (AtrousTransform(scaling_function)(signal, level).data, ref wavelets.py:307-328 over
    :65-69), one launch per chunk of signals."""
    sig = _as_signals(signals)
    M, N = len(sig), len(sig[0])
    fam = _signals_family(sig, level, scaling_function)
    if fam is None:
        # (the loop raises what the per-signal call raises; `out` is checked first where the result's shape is known)
        if isinstance(level, (int, np.integer)) and level >= 0:
            out = _target(out, (M, level + 1, N), _loop_dtype(sig))
        return _hand_over(np.stack([_transform_one(s, level, scaling_function) for s in sig]), out)
    level = int(level)
    res, ctx = _result(_target(out, (M, level + 1, N), sig.dtype), (M, level + 1, N), sig.dtype)
    chunks = _chunks(M, N, level, sig.dtype.itemsize)
    sb = _lib.acquire_signals(ctx, max(nf for _, nf in chunks), N, fam, level, sig.dtype)
    try:
        for f0, nf in chunks:
            sb.upload(sig[f0:f0 + nf])
            sb.decompose(nf, level)
            sb.download_planes(nf, out=res[f0:f0 + nf])
    finally:
        _lib.release_signals(sb)
    return res


def denoise_signals(signals, weights, scaling_function=B3spline, noise=None, soft_threshold=True, out=None, anscombe=False):
    """(M, N): utils.denoise of every signal (ref utils.py:83-102 on a 1-D array), float32 or float64 as
    transform_signals.  `noise`: None (each signal's own MAD estimate, ref wavelets.py:126-132), one scalar, or a list
    of one entry per signal, each None or a scalar; signals with a scalar skip the median.
    `anscombe`: denoise(signal, ..., anscombe=True) of every signal, bit for bit - photon counts (ref utils.py:93-94,
    99-100).  The forward transform is applied as the transform kernel loads a signal and the inverse on the sum before
    its one store: the same launches and the same device traffic as without it.  Noise levels, given or estimated, refer
    to the transformed data (ref utils.py:95-97)."""
    sig = _as_signals(signals)
    M, N = len(sig), len(sig[0])
    nl = _noise_list(noise, M)
    level = len(weights)
    # (the thresholded sum folds level + 1 planes in one launch, as the per-signal call's does)
    fam = _signals_family(sig, level, scaling_function, nl)
    if fam is None or level + 1 > _lib.MAX_SUM_PLANES:
        out = _target(out, (M, N), _loop_dtype(sig))
        more = {"anscombe": True} if anscombe else {}          # (without it: the call as it always was)
        return _hand_over(np.stack([denoise(s, weights, scaling_function, n_i, soft_threshold=soft_threshold, **more)
                                    for s, n_i in zip(sig, nl)]), out)
    res = _target(out, (M, N), sig.dtype)
    sigma_e, entries, need_noise = _thresholds(weights, scaling_function)
    res, ctx = _result(res, (M, N), sig.dtype)
    chunks = _chunks(M, N, level, sig.dtype.itemsize)
    ans = {"anscombe": True} if anscombe else {}               # (without it: the calls as they always were)
    sb = _lib.acquire_signals(ctx, max(nf for _, nf in chunks), N, fam, level, sig.dtype)
    try:
        for f0, nf in chunks:
            noises = nl[f0:f0 + nf]
            sb.upload(sig[f0:f0 + nf])
            sb.decompose(nf, level, **ans)
            if need_noise and any(n is None for n in noises):
                med = sb.abs_median(nf)                                       # ref wavelets.py:131-132 (lazy)
                noises = [_noise_from_median(m, sigma_e) if n is None else n for n, m in zip(noises, med)]
            taus = [_tau_row(entries, n, sigma_e, soft_threshold) for n in noises]
            sb.denoise_sum(nf, taus, [[w for _, _, w in entries]] * nf, soft_threshold, **ans)
            sb.download_sum(nf, out=res[f0:f0 + nf])
    finally:
        _lib.release_signals(sb)
    return res
