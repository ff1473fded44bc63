"""Wavelets Optimized Whitening of stacks of 1-D signals of one length - spectra, light curves, the time axis of a
(T, H, W) movie - on the signal engine (wt_signals): per chunk of signals ONE launch transforms them (a workgroup per
signal, the scales in LDS), the MAD medians and the plane moments of all signals come back in one host round trip each,
and ONE launch runs the per-scale loop of wow and the plane sum of every signal.

    wow_signals(signals, ...)[i]     == wow(signals[i], ..., noise=noise_i, ...)[0]
    wow_along(a, axis=k, ...)        == the same along axis k of an array

The reference whitens a signal in the 1-D branch of its transform (ref utils.py:105-219 over wavelets.py:65-69); the
per-signal call runs it as a 1 x N image: an upload, a launch per scale, up to n_scales + 1 reductions with a host
round trip each, a plane sum and a download per signal.  Without whitening and preserve_variance no reduction takes
part and the stack's results equal the per-signal loop bit for bit; with them the moments are folded in another order
(wt_signals_moments_kernel) and the results agree to rounding.  The rules are the per-signal path's own: utils.
_wow_n_scales, _wow_scale_limit, _wow_lists, _wow_needs_moments and _wow_factor, wavelets._tau_row and
_noise_from_median.

Non-finite samples follow signals.py: nothing is raised for them, the median is the per-signal call's, and without
moments a signal holding NaN or inf gets the per-signal call's bits.  With moments its sums are NaN or inf, so are its
factors, and the row is NaN where the loop's is; the other signals of the stack are not touched.

A signal on a pedestal (or a flat one), whose last plane has a variance below 1e-3 of its mean square, gets that
plane's standard deviation from its samples in float64 instead of from sumsq / N - mean^2, whose cancellation error
would exceed what the two routes may differ by (utils._STD_CANCELS; the per-signal call does the same): the planes of
each such signal come down once more, one small download per signal.

Inputs the engine does not cover run the per-signal loop and return what the loop returns; wow_signals_eligible says
which."""
import warnings

import numpy as np

from . import _lib
from .wavelets import B3spline, _tau_row, _noise_from_median, _result_dtype
from .utils import (wow, _wow_n_scales, _wow_scale_limit, _wow_lists, _wow_needs_moments, _wow_factor, _std_cancels,
                    _plane_std)
from .signals import _as_signals, _noise_list, _signals_family, _loop_dtype, _target, _hand_over, _result
from .along import _checked, _moved, _back

__all__ = ['wow_signals', 'wow_along', 'wow_signals_eligible']


def _resolved_scales(n_samples, scaling_function, n_scales, h, bilateral, denoise_coefficients, quiet):
    """n_scales as wow() resolves it for one signal of `n_samples` samples (ref utils.py:122-127, 135-138), or None
    where wow() itself would raise; `quiet`: without the reference's warning (a predicate does not warn)"""
    try:
        with warnings.catch_warnings():
            if quiet:
                warnings.simplefilter("ignore")
            L = _wow_n_scales((n_samples,), scaling_function, n_scales, h, denoise_coefficients)
            return _wow_scale_limit(L, scaling_function, 1, bilateral, denoise_coefficients)
    except (TypeError, ValueError, AttributeError, OverflowError):
        return None


def _wow_family(signals, L, scaling_function, bilateral, h, noise_per_signal):
    """the family the signal engine runs wow of this stack over the resolved `L` scales with, or None"""
    if bilateral is not None or isinstance(h, np.ndarray) or h != 0 or L is None:
        return None
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < 1:
        return None
    return _signals_family(signals, L, scaling_function, noise_per_signal)


def wow_signals_eligible(signals, n_scales, scaling_function=B3spline, bilateral=None, h=0, noise_per_signal=(),
                         denoise_coefficients=()):
    """True when the signal engine computes wow of this stack (host logic): signals_eligible(signals, L,
    scaling_function, noise_per_signal) at the L that wow() resolves `n_scales` to for the shared length (None: the most
    scales the length allows; capped by the length and by the scaling function's sigma_e table, which
    `denoise_coefficients` as long as that table selects whole) - native float32 or float64, a built-in family with its
    own taps, at most 8192 float32 or 4096 float64 samples, noise entries None or real scalars; L >= 1 (a B3spline
    signal shorter than 8 samples, a Triangle signal shorter than 5 resolve to L <= 0); no bilateral filtering and
    h == 0.  Everything else runs the per-signal loop."""
    if not isinstance(signals, np.ndarray) or signals.ndim != 2 or signals.shape[1] < 1 or bilateral is not None:
        return False
    L = _resolved_scales(signals.shape[1], scaling_function, n_scales, h, bilateral, list(denoise_coefficients), True)
    return _wow_family(signals, L, scaling_function, bilateral, h, noise_per_signal) is not None


def _wow_one(signal, noise, args):
    """the per-signal call of wow_signals: (image, Coefficients)"""
    return wow(signal, noise=noise, **args)


def _chunks(M, N, level, itemsize):
    """the chunk rule of a stack over device memory (_lib.signal_chunks with the wow route's tables)"""
    return _lib.signal_chunks(M, N, level, itemsize=itemsize, wow=True)


def _factor_rows(moments, base, needs, L, w, npix, preserve_variance, whitening, ft, stds=None):
    """(signals, L + 1) rows of utils._wow_factor: `base` where a scale needs no moments, else from the signal's
    {sum, sumsq} of that plane (`moments`: nested lists of Python floats, as Plan.reduce hands them over); `stds`: per
    signal None or the standard deviation of its last plane taken from the samples (_cancelled_stds)"""
    if not needs:
        return [base] * len(moments)
    rows = []
    for i, mom in enumerate(moments):
        row = list(base)
        for s in needs:
            std = stds[i] if stds is not None and s == L else None
            row[s] = _wow_factor(s, L, w[s], (mom[s][0], mom[s][1], None, None), npix, preserve_variance, whitening, 0, ft, std)
        rows.append(row)
    return rows


def _cancelled_stds(sb, nf, moments, needs, L, npix):
    """per signal None, or - where sumsq / N - mean^2 of the last plane has cancelled away (utils._std_cancels: a
    pedestal, a flat signal) - np.std of that plane from its samples, as the per-signal call takes it.  Only those
    signals come down, before wow_sum updates them: the L + 1 planes of each (the engine downloads whole signals),
    where the per-signal call downloads the one plane"""
    if L not in needs:
        return None
    bad = [i for i, mom in enumerate(moments) if _std_cancels(mom[L], npix)]
    if not bad:
        return None
    host = _lib.host_empty((1, L + 1, int(npix)), sb.ctx, sb.dtype)
    stds = [None] * nf
    for i in bad:
        stds[i] = _plane_std(sb.download_planes(1, out=host, f0=i)[0, L])
    return stds


def _tau_rows(entries, noises, sigma_e, soft):
    """wavelets._tau_row of every signal; signals of one noise level (of one type) share their row"""
    rows, seen = [], {}
    for n in noises:
        key = (type(n), n)
        if key not in seen:
            seen[key] = _tau_row(entries, n, sigma_e, soft)
        rows.append(seen[key])
    return rows


def wow_signals(signals, scaling_function=B3spline, n_scales=None, weights=[], whitening=True,
                denoise_coefficients=[], noise=None, bilateral=None, bilateral_scaling=False,
                soft_threshold=True, preserve_variance=False, gamma=3.2, gamma_min=None, gamma_max=None,
                h=0, out=None, return_coefficients=False):
    """(M, N): utils.wow of every signal (ref utils.py:105-219 on a 1-D array) - row i is wow(signals[i], ...,
    noise=noise_i, ...)[0] - float32 or, for the stacks the reference computes in float64, float64.  `signals` and
    `noise` as denoise_signals takes them: an (M, N) array or a sequence of 1-D arrays of one length; None (each
    signal's own MAD estimate, ref wavelets.py:126-132), one scalar, or a list of one entry per signal (an ndarray goes
    whole to every signal of the loop).  n_scales is resolved once for the shared length, as wow() resolves it for one
    signal.  return_coefficients: also (M, n_scales + 1, N), the whitened planes wow(...)[1].data of every signal.
    The caller's `weights` and `denoise_coefficients` are not changed."""
    sig = _as_signals(signals)
    M, N = len(sig), len(sig[0])
    nl = _noise_list(noise, M)
    weights, denoise_coefficients = list(weights), list(denoise_coefficients)
    L = None
    if bilateral is None and isinstance(sig, np.ndarray):
        L = _resolved_scales(N, scaling_function, n_scales, h, None, denoise_coefficients, False)
    fam = None if L is None else _wow_family(sig, L, scaling_function, bilateral, h, nl)
    if fam is None:
        out = _target(out, (M, N), _loop_dtype(sig))
        args = dict(scaling_function=scaling_function, n_scales=n_scales, weights=weights, whitening=whitening,
                    denoise_coefficients=denoise_coefficients, bilateral=bilateral, bilateral_scaling=bilateral_scaling,
                    soft_threshold=soft_threshold, preserve_variance=preserve_variance, gamma=gamma, gamma_min=gamma_min,
                    gamma_max=gamma_max, h=h)
        done = [_wow_one(s, n_i, args) for s, n_i in zip(sig, nl)]
        res = _hand_over(np.stack([r for r, _ in done]), out)
        return (res, np.stack([c.data for _, c in done])) if return_coefficients else res
    L = int(L)
    res = _target(out, (M, N), sig.dtype)
    ft = np.float64 if sig.dtype == np.float64 else np.float32                       # the data's compute type
    sf = scaling_function(1)
    sigma_e = sf.sigma_e()
    w, sdc = _wow_lists(weights, denoise_coefficients, L)                              # ref:160-170
    entries = [(s, sdc[s], 1) for s in range(L)]                                       # ref:199 per detail scale
    need_noise = any(d != 0 for _, d, _ in entries)
    whitening, soft = bool(whitening), bool(soft_threshold)
    needs = [s for s in range(L + 1) if _wow_needs_moments(s, L, preserve_variance, whitening, 0)]
    base = [None if s in needs else _wow_factor(s, L, w[s], None, float(N), preserve_variance, whitening, 0, ft)
            for s in range(L + 1)]
    res, ctx = _result(res, (M, N), sig.dtype)
    planes = _lib.host_empty((M, L + 1, N), ctx, sig.dtype) if return_coefficients else None
    chunks = _chunks(M, N, L, sig.dtype.itemsize)
    sb = _lib.acquire_signals(ctx, max(nf for _, nf in chunks), N, fam, L, sig.dtype)
    try:
        for f0, nf in chunks:
            noises = nl[f0:f0 + nf]
            sb.upload(sig[f0:f0 + nf])
            sb.decompose(nf, L)
            if need_noise and any(n is None for n in noises):
                med = sb.abs_median(nf)                                               # ref wavelets.py:131-132 (lazy)
                noises = [_noise_from_median(m, sigma_e) if n is None else n for n, m in zip(noises, med)]
            taus = _tau_rows(entries, noises, sigma_e, soft) if need_noise else [[0.0] * L] * nf
            # (the moments of the planes before any update: the reference takes `power` before the significance, ref:177-184)
            moments = sb.moments(nf).tolist() if needs else [None] * nf
            stds = _cancelled_stds(sb, nf, moments, needs, L, float(N)) if needs else None
            factors = _factor_rows(moments, base, needs, L, w, float(N), preserve_variance, whitening, ft, stds)
            sb.wow_sum(nf, taus, factors, whitening, soft, return_coefficients)
            sb.download_sum(nf, out=res[f0:f0 + nf])
            if return_coefficients:
                sb.download_planes(nf, out=planes[f0:f0 + nf])
    finally:
        _lib.release_signals(sb)
    return (res, planes) if return_coefficients else res


def wow_along(a, scaling_function=B3spline, axis=0, n_scales=None, weights=[], whitening=True,
              denoise_coefficients=[], noise=None, bilateral=None, bilateral_scaling=False,
              soft_threshold=True, preserve_variance=False, gamma=3.2, gamma_min=None, gamma_max=None,
              h=0, out=None, return_coefficients=False):
    """a.shape: utils.wow of every 1-D signal along `axis` (ref utils.py:105-219 on a 1-D array) - the light curve of
    every pixel of a (T, H, W) movie at axis=0.  `noise`: None, one real scalar, or an ndarray of the shape of `a`
    without `axis`: one level per signal, as in denoise_along.  return_coefficients: also (n_scales + 1,) + a.shape,
    plane s of all signals at [s].
    The array is transposed on the host, goes through wow_signals and is rearranged; the last axis is wow_signals' own
    layout and goes there as it is.  A tiled kernel that whitens along a strided axis without the transposes, as
    denoise_along's does, is out of scope here."""
    a, axis = _checked(a, axis)
    rest = a.shape[:axis] + a.shape[axis + 1:]
    if isinstance(noise, np.ndarray) and noise.shape != rest:
        raise ValueError(f"noise: an array of shape {rest} expected, one level per signal (got {noise.shape})")
    out = _target(out, a.shape, _result_dtype(a))
    if axis == a.ndim - 1:
        sig, moved = (a if a.ndim == 2 else a.reshape(-1, a.shape[-1])), a.shape
    else:
        sig, moved = _moved(a, axis)
    per = list(noise.reshape(-1)) if isinstance(noise, np.ndarray) else noise
    got = wow_signals(sig, scaling_function, n_scales, weights, whitening, denoise_coefficients, per, bilateral,
                      bilateral_scaling, soft_threshold, preserve_variance, gamma, gamma_min, gamma_max, h,
                      return_coefficients=return_coefficients)
    res, planes = got if return_coefficients else (got, None)
    res = _back(res, moved, axis, 0)
    res = _hand_over(res, out) if out is not None else np.ascontiguousarray(res)
    return (res, np.ascontiguousarray(_back(planes, moved, axis, 1))) if return_coefficients else res
