"""Seeded standard-normal frames: the device fill (wt_fill_normal / wt_batch_fill_normal, csrc/wt_rng.h) and its
host mirror.

Layout (a contract, DESIGN.md "Seeded normal noise"): Philox4x32-10 keyed by the 64-bit seed (low word, high word);
one call serves four horizontally adjacent pixels, counter = (x >> 2, y, trial, 0) with x, y the pixel's coordinates
in its frame and trial = first_trial + frame index.  The four words give two Box-Muller pairs: (r0, r1) -> pixels
x, x + 1 and (r2, r3) -> pixels x + 2, x + 3.  A pixel depends on (seed, trial, y, x) alone.

    normal_frames(n, (H, W), seed)          (n, H, W) float32, filled on the GPU
    normal_frames_host(n, (H, W), seed)     the same field on the host: Box-Muller in float64, rounded to float32 -
                                            the oracle of the device fill, and the frames of the signals and cubes
                                            of compute_noise_weights(seed=...)
"""
import numpy as np

from . import _lib
from ._lib import PLANE_INPUT

__all__ = ['philox4x32', 'normal_frames_host', 'normal_frames']

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # Random123's Philox4x32 multipliers
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)          # ... and Weyl key increments
_LOW, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """Philox4x32 (10 rounds) of `counter` (..., 4) under `key` (..., 2), uint32 words: (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32)
    if c.shape[-1:] != (4,) or k.shape[-1:] != (2,):
        raise ValueError("philox4x32: counter (..., 4) and key (..., 2) uint32 words")
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(rounds):
        p0 = _M0 * c0.astype(np.uint64)
        p1 = _M1 * c2.astype(np.uint64)
        c0, c1, c2, c3 = ((p1 >> _32).astype(np.uint32) ^ c1 ^ k0, (p1 & _LOW).astype(np.uint32),
                          (p0 >> _32).astype(np.uint32) ^ c3 ^ k1, (p0 & _LOW).astype(np.uint32))
        with np.errstate(over="ignore"):  # (uint32: wraps)
            k0 = k0 + _W0
            k1 = k1 + _W1
    return np.stack([c0, c1, c2, c3], axis=-1)


def _uniform(bits):
    """the device's bits -> uniform map, operation by operation in float32: ((bits >> 8) + 0.5f) * 2^-24"""
    return ((bits >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def _check(n, shape, seed, first_trial):
    if np.ndim(shape) != 1 or len(shape) != 2 or min(shape) < 1:
        raise ValueError(f"shape: a 2-D (H, W) frame shape expected (got {shape!r})")
    shape = tuple(int(v) for v in shape)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"n: at least one frame expected (got {n!r})")
    seed = _lib._seed64(seed)
    _lib._trial32(first_trial)
    _lib._trial32(first_trial + int(n) - 1)
    return int(n), shape, seed, int(first_trial)


def normal_frames_host(n, shape, seed, first_trial=0):
    """(n, H, W) float32 standard-normal frames of (seed, first_trial .. first_trial + n - 1) on the host: the
    device's generator, counter layout and bits -> uniform map, Box-Muller in float64 rounded to float32."""
    n, (H, W), seed, first_trial = _check(n, shape, seed, first_trial)
    W4 = (W + 3) // 4
    ctr = np.zeros((n, H, W4, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(W4, dtype=np.uint32)
    ctr[..., 1] = np.arange(H, dtype=np.uint32)[:, None]
    ctr[..., 2] = (first_trial + np.arange(n, dtype=np.uint64)).astype(np.uint32)[:, None, None]
    bits = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))
    u = _uniform(bits).astype(np.float64).reshape(n, H, W4, 2, 2)          # [pair][u1, u2]
    rad = np.sqrt(-2.0 * np.log(u[..., 0]))
    ang = 2.0 * np.pi * u[..., 1]
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1)          # (n, H, W4, pair, [z_a, z_b])
    return np.ascontiguousarray(z.reshape(n, H, 4 * W4)[:, :, :W].astype(np.float32))


def normal_frames(n, shape, seed, first_trial=0, out=None):
    """(n, H, W) float32 standard-normal frames of (seed, first_trial .. first_trial + n - 1), filled on the GPU
    (BatchPlan.fill_normal, chunks of _lib.batch_chunks) and downloaded straight into `out` - a C-contiguous
    float32 (n, H, W) array - or into a page-locked block.  Frame f is Plan.fill_normal(seed, first_trial + f)."""
    n, (H, W), seed, first_trial = _check(n, shape, seed, first_trial)
    if out is None:
        out = _lib.host_empty((n, H, W))
    elif not isinstance(out, np.ndarray) or out.shape != (n, H, W) or out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError(f"out: float32 array of shape {(n, H, W)} expected")
    chunks = _lib.batch_chunks(n, H, W, 0)
    bp = _lib.acquire_batch(_lib.default_context(), max(nf for _, nf in chunks), H, W, _lib.B3SPLINE, 0)
    try:
        for f0, nf in chunks:
            bp.fill_normal(nf, PLANE_INPUT, seed, first_trial + f0)
            bp.download(PLANE_INPUT, nf, out=out[f0:f0 + nf])
    finally:
        _lib.release_batch(bp)
    return out
