"""wavelets_amd.resident on the GPU: transform_stack / denoise_stack from a device array to a device array have the
bits and the element type of batch.transform_stack / batch.denoise_stack on the downloaded input - at the shapes where
the two copy kernels can go wrong (one element, widths that are no multiple of the 16-byte group, pitched rows, an
inner stride of two, every second frame), with every widened element type, through more than one chunk, into views of
larger blocks, on every stream form, through the staged route and through a PyTorch tensor; and they meet the float64
numpy oracle under the bounds batch.* is held to.

No call may lean on an earlier right answer.  The batch of a call is a cached one (batch._batch) and keeps the planes
of its last owner; a result from DeviceArray.empty is unfilled memory that a block freed a moment earlier may have left
the right answer in.  So the expected values are computed first, then poison_batch runs the host functions on an
all-NaN stack on the very batch the resident call is handed next (NaN in the input plane, the coefficient, scratch and
output planes), and the resident call stores into an `out=` filled with NaN (r_transform, r_denoise): a load or a
store that moves nothing, or not everything, shows as NaN.  The kernels on their own: tests/test_gpu_resident_copies.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B
from wavelets_amd import resident as R
from wavelets_amd.wavelets import _result_dtype

from conftest import measured, SMALL_PLANES
from test_batch64_cpu import PLANES_TOL, DENOISE64_TOL           # what tests/test_gpu_batch64.py holds batch.* to
from test_stack_edges_cpu import DENOISE_TOL                      # tests/test_gpu_batch.py:131 (test_gpu_parity.DENOISE_TOL)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def stack(shape, dtype=np.float32, seed=0):
    x = np.random.default_rng(seed).standard_normal(shape) * 20 + 100
    return x.astype(dtype)


def sub_view(dev, host_block, host_view):
    """resident.view of the part of the DeviceArray `dev` (a copy of host_block) that host_view is of host_block"""
    off = host_view.__array_interface__["data"][0] - host_block.__array_interface__["data"][0]
    return R.view(dev.ptr + off, host_view.shape, host_view.dtype, host_view.strides)


def plane_type(dtype):
    """the element type of the batch that serves a stack of `dtype` (resident._route): uint8 and float32 the float32
    batch, everything else the float64 batch"""
    return np.dtype(np.float32 if np.dtype(dtype) in (np.dtype(np.uint8), np.dtype(np.float32)) else np.float64)


def poison_batch(host_frames, level, scaling_function=W.B3spline, weights=None, **kw):
    """NaN into every plane of the batch the next resident call on a stack like host_frames gets: the cache is emptied,
    then batch.transform_stack and batch.denoise_stack run on an all-NaN stack of that shape through the host route, in
    the element type of the planes (integers hold no NaN: plane_type), at that level and with that scaling function.
    They make the one batch of that key, leave NaN in its input plane and in every plane they write, and hand it back
    to the cache.  The noise level is given (1.0): the MAD estimate of a NaN frame is an error.  Both results must be
    all NaN - what shows that the planes are."""
    nan = np.full(host_frames.shape, np.nan, plane_type(host_frames.dtype))
    L.trim_batches()
    weights = [1] * level if weights is None else list(weights)
    kw = {k: v for k, v in kw.items() if k in ("soft_threshold", "anscombe")}
    assert np.isnan(B.denoise_stack(nan, weights, scaling_function, noise=1.0, **kw)).all()
    assert np.isnan(B.transform_stack(nan, level, scaling_function)).all()


def nan_out(shape, dtype):
    return R.DeviceArray.from_numpy(np.full(shape, np.nan, dtype))


def r_transform(dev, want, level, *args, **kw):
    """the host copy of R.transform_stack stored into an `out=` of want's shape and element type filled with NaN"""
    o = nan_out(want.shape, want.dtype)
    assert R.transform_stack(dev, level, *args, out=o, **kw) is o
    return o.numpy()


def r_denoise(dev, want, weights, *args, **kw):
    """the host copy of R.denoise_stack stored into an `out=` of want's shape and element type filled with NaN"""
    o = nan_out(want.shape, want.dtype)
    assert R.denoise_stack(dev, list(weights), *args, out=o, **kw) is o
    return o.numpy()


def check_both(dev_frames, host_frames, level=2, weights=(5, 3), fresh=False, **kw):
    """`fresh`: the calls go without out= (the DeviceArray.empty branch of resident._run)"""
    before = host_frames.copy()
    want_t = B.transform_stack(host_frames, level)
    want_d = B.denoise_stack(host_frames, list(weights), **kw)
    assert want_t.dtype == _result_dtype(host_frames) == want_d.dtype
    poison_batch(host_frames, level)
    if fresh:
        t = R.transform_stack(dev_frames, level)
        assert isinstance(t, R.DeviceArray) and t.dtype == want_t.dtype and same(t.numpy(), want_t)
    else:
        assert same(r_transform(dev_frames, want_t, level), want_t)
    poison_batch(host_frames, len(weights), weights=weights, **kw)
    if fresh:
        d = R.denoise_stack(dev_frames, list(weights), **kw)
        assert isinstance(d, R.DeviceArray) and d.dtype == want_d.dtype and same(d.numpy(), want_d)
    else:
        assert same(r_denoise(dev_frames, want_d, weights, **kw), want_d)
    assert same(host_frames, before)
    return before


# ------------------------------------------------------------------------------------------------ the copy kernels
@pytest.mark.parametrize("shape, dtype", [((3, 5, 7), np.float32), ((2, 1, 1), np.float32), ((2, 16, 64), np.float32),
                                          ((2, 9, 33), np.float64), ((2, 16, 64), np.float64), ((2, 2, 1), np.float64)])
def test_contiguous_stacks(shape, dtype):
    a = stack(shape, dtype)
    dev = R.DeviceArray.from_numpy(a)
    assert R.eligible(dev, 2)
    check_both(dev, a, fresh=shape == (2, 16, 64))                 # (one call without out= per element type)
    assert same(dev.numpy(), a)                                    # the input is left untouched


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8, np.int16])
def test_strided_views(dtype):
    if np.dtype(dtype).kind == "f":
        block = stack((4, 64, 160), dtype, 1)
    else:
        info = np.iinfo(dtype)
        block = np.random.default_rng(1).integers(info.min, info.max, (4, 64, 160), dtype=dtype, endpoint=True)
    dev = R.DeviceArray.from_numpy(block)
    for hv in (block[:1, :, :130],                                 # row-pitched: (1, 64, 130) of a (1, 64, 160) block
               block[:, :9, 3:36],                                  # rows that start off the 16-byte grid
               block[:2, :7, ::2],                                  # an inner stride of two elements
               block[::2, :12, :64],                                # every second frame (the vector path, pitched)
               block[1::2, 5:7, 7:8]):                              # one element per row
        v = sub_view(dev, block, hv)
        assert R.eligible(v, 2)
        check_both(v, hv)
    assert same(dev.numpy(), block)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint16, np.int32])
def test_widened_types(dtype):
    info = np.iinfo(dtype)
    a = np.random.default_rng(2).integers(info.min, info.max, (3, 5, 7), dtype=dtype, endpoint=True)
    a[0, 0, :2] = info.min, info.max
    dev = R.DeviceArray.from_numpy(a)
    assert R.eligible(dev, 2)
    check_both(dev, a)
    wide = np.random.default_rng(3).integers(max(info.min, -30000), min(info.max, 30000), (2, 16, 64), dtype=dtype)
    check_both(R.DeviceArray.from_numpy(wide), wide)               # ... and on the vector path
    assert same(dev.numpy(), a)


def test_chunks(monkeypatch):
    a = stack((5, 12, 20))
    dev = R.DeviceArray.from_numpy(a)
    noise = [None, 1.0, 2, None, 0.5]
    want_t, want_d = B.transform_stack(a, 3), B.denoise_stack(a, [4, 2, 1], noise=noise)
    a64 = a.astype(np.float64)
    want_d64 = B.denoise_stack(a64, [4, 2, 1])
    seen = []

    def chunks_of_two(n, H, W, level, f64, extra_planes=0):
        return [(f0, min(2, n - f0)) for f0 in range(0, n, 2)]

    def seen_chunks_of_two(n, *args, **kw):
        seen.append(n)
        return chunks_of_two(n, *args, **kw)

    monkeypatch.setattr(B, "_plan_chunks", chunks_of_two)          # (the poisoning host calls: the same batch of two)
    monkeypatch.setattr(R, "_plan_chunks", seen_chunks_of_two)
    poison_batch(a, 3)
    assert same(r_transform(dev, want_t, 3), want_t)
    poison_batch(a, 3)
    assert same(r_denoise(dev, want_d, [4, 2, 1], noise=noise), want_d)
    poison_batch(a64, 3)
    assert same(r_denoise(R.DeviceArray.from_numpy(a64), want_d64, [4, 2, 1]), want_d64)
    assert seen == [5, 5, 5]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_real_chunking(monkeypatch, dtype):
    """the chunks planned for real (_lib.batch_chunks, not a stand-in): a budget of two frames' planes gives 5 frames the
    chunks 2, 2, 1 - a last chunk shorter than the batch, whose second frame still holds the chunk before.  The budget
    is read from the environment at import, hence the patch of _lib.BATCH_BYTES.  Chunking changes no bit: the
    expected values are also those of the unchunked host call."""
    f64 = np.dtype(dtype) == np.float64
    a = stack((5, 12, 20), dtype, 10)
    dev = R.DeviceArray.from_numpy(a)
    noise = [None, 1.0, 2, None, 0.5]
    monkeypatch.setattr(L, "BATCH_BYTES", 2 * L.batch_frame_bytes(12, 20, 3, a.itemsize))
    assert B._plan_chunks(5, 12, 20, 3, f64) == [(0, 2), (2, 2), (4, 1)] == R._plan_chunks(5, 12, 20, 3, f64)
    want_t, want_d = B.transform_stack(a, 3), B.denoise_stack(a, [4, 2, 1], noise=noise)
    monkeypatch.undo()
    assert same(B.transform_stack(a, 3), want_t) and same(B.denoise_stack(a, [4, 2, 1], noise=noise), want_d)
    monkeypatch.setattr(L, "BATCH_BYTES", 2 * L.batch_frame_bytes(12, 20, 3, a.itemsize))
    poison_batch(a, 3)
    assert same(r_transform(dev, want_t, 3), want_t)
    poison_batch(a, 3)
    assert same(r_denoise(dev, want_d, [4, 2, 1], noise=noise), want_d)
    assert same(dev.numpy(), a)


def outcome(call):
    """(shape, element type, None) of what a call returns, or (None, None, the type of what it raises)"""
    try:
        res = call()
    except Exception as e:
        return None, None, type(e)
    return tuple(res.shape), np.dtype(res.dtype), None


@pytest.mark.parametrize("shape", [(0, 4, 5), (2, 0, 5), (2, 4, 0)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_empty_stacks(shape, dtype):
    """a stack without elements: what batch.* does on the host copy - the same shape and element type, or the same
    exception type - and a result is a DeviceArray without a device block"""
    host = np.empty(shape, dtype)
    dev = R.DeviceArray.from_numpy(host)
    assert dev.ptr == 0 and dev.size == 0
    for r_call, b_call in ((lambda: R.transform_stack(dev, 2), lambda: B.transform_stack(host, 2)),
                           (lambda: R.denoise_stack(dev, [5, 3]), lambda: B.denoise_stack(host, [5, 3]))):
        want = outcome(b_call)
        kept = []
        assert outcome(lambda: kept.append(r_call()) or kept[0]) == want
        if want[2] is None:
            assert isinstance(kept[0], R.DeviceArray) and kept[0].ptr == 0 and kept[0].size == 0 and kept[0].nbytes == 0
            assert kept[0].numpy().shape == want[0]


# ---------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strided_views_against_the_oracle(dtype):
    """resident.* against oracle.atrous_numpy in float64, per frame and scaled by that frame's max|input|, under the
    bounds batch.* is held to: float32 - conftest.SMALL_PLANES (tests/test_gpu_stack_edges.py) and DENOISE_TOL
    (tests/test_gpu_batch.py, test_stack_edges_cpu); float64 - PLANES_TOL and DENOISE64_TOL (tests/test_gpu_batch64.py,
    test_batch64_cpu)"""
    from oracle import atrous_numpy as O
    f64 = np.dtype(dtype) == np.float64
    planes_tol, denoise_tol = (PLANES_TOL, DENOISE64_TOL) if f64 else (SMALL_PLANES, DENOISE_TOL)
    block = stack((3, 24, 50), dtype, 12)
    hv = block[::2, 2:21, 3:40]                                    # every second frame, pitched, off the 16-byte grid
    dev = R.DeviceArray.from_numpy(block)
    v = sub_view(dev, block, hv)
    assert R.eligible(v, 3)
    refs_t = [O.atrous_standard(f.astype(np.float64), 3, "b3spline") for f in hv]
    refs_d = [O.denoise(f.astype(np.float64), [5, 3, 2], "b3spline") for f in hv]
    rdt = np.dtype(dtype)
    poison_batch(hv, 3)
    got_t = r_transform(v, np.empty((2, 4) + hv.shape[1:], rdt), 3)
    poison_batch(hv, 3)
    got_d = r_denoise(v, np.empty(hv.shape, rdt), [5, 3, 2])
    for i, f in enumerate(hv):
        amax = float(np.abs(f).max())
        measured(f"resident planes {rdt.name} frame {i}", got_t[i], refs_t[i], planes_tol * amax)
        measured(f"resident denoise {rdt.name} frame {i}", got_d[i], refs_d[i], denoise_tol * amax)
    assert same(dev.numpy(), block)


# ------------------------------------------------------------------------------------------------------------- out
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_out_views_of_larger_blocks(dtype):
    a = stack((3, 9, 13), dtype, 4)
    dev = R.DeviceArray.from_numpy(a)
    want = B.denoise_stack(a, [5, 3])
    big = np.random.default_rng(5).standard_normal((3, 4, 11, 18)).astype(want.dtype)
    for hv in (lambda b: b[:, 2, 1:-1, 2:-3], lambda b: b[:, 1, :9, 5:]):
        dbig = R.DeviceArray.from_numpy(big)
        o = sub_view(dbig, big, hv(big))
        poison_batch(a, 2)
        assert R.denoise_stack(dev, [5, 3], out=o) is o
        expect = big.copy()
        hv(expect)[...] = want
        assert same(dbig.numpy(), expect)                          # the view filled, every other byte as it was
    # transform_stack: the planes into a cropped view big[:, :, 1:-1, 2:-3] of a larger cube
    want = B.transform_stack(a, 3)
    dbig = R.DeviceArray.from_numpy(big)
    o = sub_view(dbig, big, big[:, :, 1:-1, 2:-3])
    poison_batch(a, 3)
    assert R.transform_stack(dev, 3, out=o) is o
    expect = big.copy()
    expect[:, :, 1:-1, 2:-3] = want
    assert same(dbig.numpy(), expect)
    with pytest.raises(ValueError, match="^out: "):
        R.transform_stack(dev, 3, out=R.DeviceArray.empty((3, 4, 9, 14), want.dtype))
    assert same(dev.numpy(), a)


# ---------------------------------------------------------------------------------------------------------- denoise
def test_denoise_forms():
    a = np.abs(stack((3, 24, 40), np.float32, 6))
    dev = R.DeviceArray.from_numpy(a)
    a64 = a.astype(np.float64)
    dev64 = R.DeviceArray.from_numpy(a64)
    for kw in (dict(), dict(noise=1.5), dict(noise=[None, 1.0, 2]), dict(soft_threshold=False),
               dict(noise=[None, 1.0, 2], soft_threshold=False), dict(anscombe=True),
               dict(anscombe=True, noise=[1.0, None, 0.5]), dict(scaling_function=W.Triangle)):
        for host, d in ((a, dev), (a64, dev64)):
            want = B.denoise_stack(host, [5, 3, 1], **kw)
            poison_batch(host, 3, **kw)
            assert same(r_denoise(d, want, [5, 3, 1], **kw), want), (kw, host.dtype)
    want = B.transform_stack(a, 4, W.Triangle)
    poison_batch(a, 4, W.Triangle)
    assert same(r_transform(dev, want, 4, W.Triangle), want)


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


def test_staged_route():
    a = stack((2, 12, 17))
    dev = R.DeviceArray.from_numpy(a)
    assert not R.eligible(dev, 2, Retapped)
    want = B.transform_stack(a, 2, Retapped)
    assert same(r_transform(dev, want, 2, Retapped), want)
    res = R.transform_stack(dev, 2, Retapped)                      # (without out=: a fresh DeviceArray from the host result)
    assert isinstance(res, R.DeviceArray) and same(res.numpy(), want)
    want = B.denoise_stack(a, [5, 3], Retapped)
    assert same(r_denoise(dev, want, [5, 3], Retapped), want)
    block = stack((2, 12, 40), np.float32, 7)
    dblock = R.DeviceArray.from_numpy(block)
    hv = block[:, ::-1, 3:20]                                      # a negative stride: staged
    v = sub_view(dblock, block, hv)
    assert not R.eligible(v, 2)
    big = np.full((2, 12, 30), np.nan, np.float32)
    dbig = R.DeviceArray.from_numpy(big)
    o = sub_view(dbig, big, big[:, :, 5:22])
    assert R.denoise_stack(v, [5, 3], out=o) is o
    big[:, :, 5:22] = B.denoise_stack(hv, [5, 3])
    assert same(dbig.numpy(), big)
    half = a.astype(np.float16)
    want = B.denoise_stack(half, [5, 3])
    assert same(r_denoise(R.DeviceArray.from_numpy(half), want, [5, 3]), want)


# ------------------------------------------------------------------------------------------------- interface, streams
def test_device_array_hand_off():
    a = stack((2, 6, 10), np.float64, 8)
    d = R.DeviceArray.from_numpy(a)
    assert same(d.numpy(), a) and same(d.numpy(out=np.empty_like(a)), a)
    cai = d.__cuda_array_interface__
    assert cai["version"] == 3 and cai["strides"] is None and cai["data"] == (d.ptr, False)
    alias = R.view(cai["data"][0], cai["shape"], cai["typestr"])
    want = B.denoise_stack(a, [5, 3])
    res = nan_out(a.shape, np.float64)
    poison_batch(a, 2)
    assert R.denoise_stack(alias, [5, 3], out=res) is res and same(res.numpy(), want)
    poison_batch(a, 2)
    R.denoise_stack(d, [5, 3], out=alias)                          # in place: the view aliases d
    assert same(d.numpy(), want)
    d.free()
    d.free()
    assert d.ptr == 0


class Hip:
    """the few calls of the HIP runtime the stream tests make themselves, through ctypes on the runtime library the
    process has mapped (the one libwatroo_hip.so is linked against)"""

    D2H, D2D = 2, 3                                                # hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice

    def __init__(self):
        L.load()
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln.rsplit("/", 1)[-1]})
        assert len(paths) == 1, paths
        self.lib = ctypes.CDLL(paths[0])
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        for name, args in (("hipStreamCreate", [ctypes.POINTER(vp)]), ("hipStreamDestroy", [vp]),
                           ("hipStreamSynchronize", [vp]), ("hipMemcpyAsync", [vp, vp, sz, ctypes.c_int, vp])):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = ctypes.c_int, args

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        assert rc == 0, f"{name}: hipError_t {rc}"

    def stream_create(self):
        h = ctypes.c_void_p()
        self.call("hipStreamCreate", ctypes.byref(h))
        assert h.value
        return h.value

    def copy_async(self, dst, src, nbytes, kind, stream):
        self.call("hipMemcpyAsync", dst, src, nbytes, kind, stream)


def test_streams_give_the_same_bits():
    a = stack((3, 20, 36), np.float32, 9)
    dev = R.DeviceArray.from_numpy(a)
    want_t, want_d = B.transform_stack(a, 3), B.denoise_stack(a, [5, 3])
    hip = Hip()
    h = hip.stream_create()
    try:
        for stream in (None, 1, 2, h):
            poison_batch(a, 3)
            assert same(r_transform(dev, want_t, 3, stream=stream), want_t), stream
            if stream is not None:
                L.default_context().sync()
            poison_batch(a, 2)
            assert same(r_denoise(dev, want_d, [5, 3], stream=stream), want_d), stream
        hip.call("hipStreamSynchronize", h)
    finally:
        L.default_context().sync()
        hip.call("hipStreamDestroy", h)


def test_stream_handle_orders_both_ends():
    """A hipStream_t made here, work queued on it, and no host synchronisation between that work and the call.
    Load side: the source array holds NaN; the stream copies twenty times 256 MiB between two scratch blocks (a few
    milliseconds) and then the true frames into the source; denoise_stack(stream=h) is called at once - its first load
    must wait for the stream (resident_order before the load).  Store side: the same producer, then
    transform_stack(out=o, stream=h), which returns without a host synchronisation, then a copy of o to the host queued
    on the stream: it must wait for the last store (resident_order after the store).  A pass is deterministic; with a
    wait removed the NaN underneath is only very likely to show."""
    hip = Hip()
    ctx = L.default_context()
    block = stack((3, 20, 40), np.float32, 13)
    hv = block[:, :, :36]
    want_d, want_t = B.denoise_stack(hv, [5, 3]), B.transform_stack(hv, 2)
    nan_block = np.full(block.shape, np.nan, np.float32)
    staging = R.DeviceArray.from_numpy(block)
    source = R.DeviceArray.from_numpy(nan_block)
    view = sub_view(source, block, hv)
    big = 256 << 20
    s1, s2 = R.DeviceArray.empty((big,), np.uint8), R.DeviceArray.empty((big,), np.uint8)
    host = L.host_empty(want_t.shape, ctx, np.float32)             # page-locked: the copy to it is asynchronous
    h = hip.stream_create()

    def produce():
        for i in range(20):
            hip.copy_async(s2.ptr if i % 2 == 0 else s1.ptr, s1.ptr if i % 2 == 0 else s2.ptr, big, Hip.D2D, h)
        hip.copy_async(source.ptr, staging.ptr, block.nbytes, Hip.D2D, h)

    try:
        poison_batch(hv, 2)
        o = nan_out(want_d.shape, np.float32)
        ctx.sync()
        produce()
        assert R.denoise_stack(view, [5, 3], out=o, stream=h) is o
        hip.call("hipStreamSynchronize", h)
        ctx.sync()
        assert same(o.numpy(), want_d), "the first load did not wait for the caller's stream"

        L.device_copy(ctx, source.ptr, nan_block.ctypes.data, nan_block.nbytes, L.COPY_HOST_TO_DEVICE)
        poison_batch(hv, 2)
        o = nan_out(want_t.shape, np.float32)
        host[...] = 0
        ctx.sync()
        produce()
        assert R.transform_stack(view, 2, out=o, stream=h) is o
        hip.copy_async(host.ctypes.data, o.ptr, o.nbytes, Hip.D2H, h)
        hip.call("hipStreamSynchronize", h)
        assert same(np.array(host), want_t), "the caller's stream did not wait for the last store"
        ctx.sync()
        assert same(o.numpy(), want_t) and same(staging.numpy(), block)
    finally:
        try:
            ctx.sync()
            hip.call("hipStreamSynchronize", h)
        finally:
            hip.call("hipStreamDestroy", h)
            for d in (s1, s2, source, staging):
                d.free()


TORCH_CHILD = r"""
import sys
try:
    import torch                                   # (first: INTEGRATION.md, "import torch first")
    if not torch.cuda.is_available():
        print("SKIP torch sees no device"); sys.exit(0)
    import numpy as np
    import wavelets_amd as W
    from wavelets_amd import resident as R, batch as B
except (ImportError, OSError) as e:
    print("SKIP the two ROCm stacks do not load together:", repr(e)[:200]); sys.exit(0)
g = torch.Generator(device="cuda").manual_seed(0)
t = torch.randn((3, 48, 80), device="cuda", generator=g) * 20 + 100
print("HAS_CAI", hasattr(t, "__cuda_array_interface__"))
host = t.cpu().numpy()
src = t if hasattr(t, "__cuda_array_interface__") else R.view(t.data_ptr(), tuple(t.shape), np.float32)
res = R.denoise_stack(src, [5, 3], stream=torch.cuda.current_stream().cuda_stream)
back = torch.as_tensor(res, device="cuda")
assert back.data_ptr() == res.ptr, "torch copied the result"
want = B.denoise_stack(host, [5, 3])
got = back.cpu().numpy()
assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), "bits differ"
assert np.array_equal(t.cpu().numpy(), host), "the input changed"
print("OK")
"""


def test_torch_tensor_in_and_out():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    print(r.stdout, r.stderr[-2000:])
    skip = [ln for ln in r.stdout.splitlines() if ln.startswith("SKIP")]
    if r.returncode == 0 and skip:
        pytest.skip(skip[0])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr[-2000:]
