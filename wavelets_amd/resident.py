"""Stacks of frames that stay on the device: transform_stack and denoise_stack from a device array to a device array.

    resident.transform_stack(frames, level)    has the bits of  batch.transform_stack(host copy of frames, level)
    resident.denoise_stack(frames, weights)    has the bits of  batch.denoise_stack(host copy of frames, weights)

and their element type (wavelets._result_dtype), without the two PCIe crossings and the host copy of the numpy-to-numpy
calls.  `frames` and `out` are a DeviceArray (a block of device memory this library owns), a view(ptr, shape, dtype,
strides) of someone else's device memory, or any object with a __cuda_array_interface__ dict of version 2 or 3 (a
GPU tensor of PyTorch-ROCm, a CuPy-ROCm array); a DeviceArray carries that attribute itself, so whatever speaks the
protocol takes a result without a copy.  Nothing here imports such a library.

The device part is batch.py's: the same chunks (_plan_chunks), the same cached batch (_batch), the same chunk loops
(_transform_chunks, _denoise_chunks).  Only the two ends differ: a chunk is loaded from and stored to device memory by
one kernel each (wt_batch_load_device / wt_batch_store_device and the wt_batch64 pair: any pitch, any inner stride,
uint8 / int16 / uint16 / int32 widened on the way in).  eligible says which stacks take that route.  Everything else
the host functions accept - custom taps, other element types, byte-swapped data, noise maps, levels outside the
engine, negative or unaligned strides - is staged: downloaded, run through the host function, uploaded into the result.

Streams.  The library works on its context's stream.  `stream` names the stream the caller produced `frames` on and
will read the result on, in the protocol's convention: 1 - the legacy default stream, 2 - the per-thread default
stream, any other positive int - a hipStream_t (0, the null handle, is the legacy default stream); None - the `stream`
entry of frames' interface if it has one.  With a
stream the context's stream waits for it before the first load and it waits for the context's stream after the last
store, and the call returns without a host synchronisation (except where the algorithm needs one: the MAD medians).
Without one the input is taken as ready - the protocol's rule - and the context's stream is synchronised before the
call returns.  The staged route is a host round trip and orders nothing: synchronise the producing stream first."""
import numpy as np

from . import _lib
from . import batch as _batch_mod
from ._lib import PLANE_INPUT
from .batch import (_plan_chunks, _batch, _transform_chunks, _denoise_chunks, _noise_list, batch_eligible,
                    batch64_eligible)
from .wavelets import B3spline, _family_of, _result_dtype

__all__ = ['DeviceArray', 'view', 'eligible', 'transform_stack', 'denoise_stack']

# the element types a chunk is loaded from (wt_batch_load_device: uint8 and float32 into float planes;
# wt_batch64_load_device: the others into double planes)
_TYPES = tuple(np.dtype(t) for t in (np.float32, np.float64, np.uint8, np.int16, np.uint16, np.int32))


def _c_strides(shape, itemsize):
    st, acc = [], itemsize
    for n in reversed(shape):
        st.append(acc)
        acc *= max(int(n), 1)
    return tuple(reversed(st))


class _Desc:
    """A device array as this module sees it: address, shape, element type, strides in bytes, the stream its
    interface names (or None), and the object that keeps the memory alive"""

    __slots__ = ("ptr", "shape", "dtype", "strides", "stream", "owner")

    def __init__(self, ptr, shape, dtype, strides=None, stream=None, owner=None):
        self.ptr = int(ptr or 0)
        self.shape = tuple(int(n) for n in shape)
        self.dtype = np.dtype(dtype)
        if any(n < 0 for n in self.shape):
            raise ValueError(f"a device array of shape {self.shape}")
        if self.dtype.kind == "c":
            raise ValueError(f"complex element type {self.dtype}: real frames expected")
        if self.dtype.kind not in "biuf":
            raise ValueError(f"element type {self.dtype}: real numbers expected")
        self.strides = _c_strides(self.shape, self.dtype.itemsize) if strides is None else tuple(int(s) for s in strides)
        if len(self.strides) != len(self.shape):
            raise ValueError(f"{len(self.strides)} strides for {len(self.shape)} axes")
        if not self.ptr and self.size:
            raise ValueError("a null device pointer for an array that is not empty")
        self.stream = stream
        self.owner = owner

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def extent(self):
        """(lo, hi): the bytes [ptr + lo, ptr + hi) the elements lie in"""
        if not self.size:
            return 0, 0
        lo = sum(min(0, (n - 1) * s) for n, s in zip(self.shape, self.strides))
        hi = sum(max(0, (n - 1) * s) for n, s in zip(self.shape, self.strides)) + self.dtype.itemsize
        return lo, hi

    @property
    def c_contiguous(self):
        return self.strides == _c_strides(self.shape, self.dtype.itemsize)


class DeviceArray:
    """A C-contiguous block of device memory owned by this library: `shape`, `dtype`, `strides` (bytes), `nbytes`,
    `ptr`.  DeviceArray.empty(shape, dtype) allocates, DeviceArray.from_numpy(a) uploads, .numpy() downloads, .free()
    releases (idempotent; __del__ does the same).  __cuda_array_interface__ (version 3) hands the block to anything
    that speaks the protocol without a copy; the block lives as long as this object."""

    def __init__(self, ptr, shape, dtype, ctx):
        self.ptr, self.shape, self.dtype, self.ctx = ptr, tuple(shape), np.dtype(dtype), ctx

    @classmethod
    def empty(cls, shape, dtype, ctx=None):
        shape = tuple(int(n) for n in (shape if np.ndim(shape) else (shape,)))
        dtype = np.dtype(dtype)
        if any(n < 0 for n in shape) or dtype.kind not in "biuf":
            raise ValueError(f"DeviceArray: shape {shape} of {dtype}")
        ctx = ctx if ctx is not None else _lib.default_context()
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        return cls(_lib.device_alloc(ctx, nbytes), shape, dtype, ctx)

    @classmethod
    def from_numpy(cls, a, ctx=None):
        a = np.ascontiguousarray(a)
        d = cls.empty(a.shape, a.dtype, ctx)
        if a.size:
            _lib.device_copy(d.ctx, d.ptr, a.ctypes.data, a.nbytes, _lib.COPY_HOST_TO_DEVICE)
        return d

    @property
    def strides(self):
        return _c_strides(self.shape, self.dtype.itemsize)

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def ndim(self):
        return len(self.shape)

    def numpy(self, out=None):
        """the block as an ndarray; `out`: a C-contiguous writable ndarray of this shape and element type"""
        if out is None:
            out = np.empty(self.shape, self.dtype)
        elif not (isinstance(out, np.ndarray) and out.shape == self.shape and out.dtype == self.dtype
                  and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError(f"out: a C-contiguous {self.dtype} ndarray of shape {self.shape} expected")
        if self.size:
            if not self.ptr:
                raise ValueError("DeviceArray: the block has been freed")
            _lib.device_copy(self.ctx, out.ctypes.data, self.ptr, self.nbytes, _lib.COPY_DEVICE_TO_HOST)
        return out

    def free(self):
        ptr, self.ptr = self.ptr, 0
        if ptr and self.ctx is not None and self.ctx._h:          # (a closed context took its device's blocks along)
            _lib.device_free(self.ctx, ptr)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def __cuda_array_interface__(self):
        if self.size and not self.ptr:
            raise ValueError("DeviceArray: the block has been freed")
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 3, "strides": None}

    def __repr__(self):
        return f"DeviceArray(shape={self.shape}, dtype={self.dtype}, ptr={self.ptr:#x})"


class DeviceView(_Desc):
    """view()'s result: a borrowed description of device memory; whoever made it keeps the memory alive"""


def view(ptr, shape, dtype, strides=None):
    """A borrowed, non-owning description of someone else's device memory: `ptr` the address of element [0, ...],
    `strides` in bytes (None: C-contiguous).  Always available, whatever protocol the owner speaks:
    view(t.data_ptr(), t.shape, np.float32) of a tensor, view(d.ptr + s * d.strides[1], ...) of a plane of a cube."""
    if isinstance(ptr, bool) or not isinstance(ptr, (int, np.integer)):
        raise TypeError(f"view: the device address as an int expected (got {type(ptr).__name__})")
    return DeviceView(ptr, shape, dtype, strides)


def _describe(obj):
    """the _Desc of a DeviceArray, a view or an object with a __cuda_array_interface__ (version 2 or 3); TypeError
    for anything else, ValueError for an interface this module cannot read"""
    if isinstance(obj, _Desc):
        return obj
    if isinstance(obj, DeviceArray):
        return _Desc(obj.ptr, obj.shape, obj.dtype, None, None, obj)
    cai = getattr(obj, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise TypeError(f"a DeviceArray, a resident.view or an object with a __cuda_array_interface__ expected "
                        f"(got {type(obj).__name__})")
    if cai.get("version") not in (2, 3):
        raise ValueError(f"__cuda_array_interface__ version {cai.get('version')!r}: 2 or 3 expected")
    if cai.get("mask") is not None:
        raise ValueError("__cuda_array_interface__ with a mask")
    try:
        dtype = np.dtype(cai["typestr"])
        ptr = cai["data"][0]
        shape = tuple(cai["shape"])
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f"__cuda_array_interface__: {e!r}") from None
    return _Desc(ptr, shape, dtype, cai.get("strides"), cai.get("stream"), obj)


def _frames(frames):
    d = _describe(frames)
    if len(d.shape) != 3:
        raise ValueError(f"frames: an (N, H, W) device array expected (got shape {d.shape})")
    return d


def _route(d, level, scaling_function, noise_per_frame):
    """True: the float64 batch, False: the float32 batch, None: staged.  batch._stack_route's plain routes, asked of a
    zero-stride ndarray of the stack's shape and of the element type the host function would hand the batch (uint8
    frames are served in float32: the float32 batch, which widens them exactly on the way in)"""
    if len(d.shape) != 3 or min(d.shape) < 1:
        return None
    if d.dtype not in _TYPES or not d.dtype.isnative:
        return None
    if any(s <= 0 or s % d.dtype.itemsize for s in d.strides):
        return None
    probe = np.broadcast_to(np.zeros((), np.float32 if d.dtype == np.uint8 else d.dtype), d.shape)
    if batch64_eligible(probe, level, scaling_function, None, noise_per_frame):
        return True
    if batch_eligible(probe, level, scaling_function, None, noise_per_frame):
        return False
    return None


def eligible(frames, level, scaling_function=B3spline, noise_per_frame=()):
    """True when the stack runs device to device (host logic): a 3-D stack with N, H, W >= 1 of native float32,
    float64, uint8, int16, uint16 or int32, every stride a positive multiple of the element size, and a call the host
    functions would run on a batch without bilateral filtering (batch.batch_eligible / batch.batch64_eligible: a
    built-in scaling function with its own taps, a level the fused passes cover, scalar noise levels).  Everything
    else is staged through the host function."""
    return _route(_frames(frames), level, scaling_function, noise_per_frame) is not None


def _stream_of(stream, d):
    """the stream of a call (None: nothing to order), checked - host logic"""
    if stream is None:
        stream = d.stream
    _lib.stream_arg(stream)
    return None if stream is None else int(stream)


def _out_desc(out, shape, dtype):
    """the caller's `out`, checked before any device work"""
    try:
        o = _describe(out)
    except (TypeError, ValueError) as e:
        raise ValueError(f"out: {e}") from None
    if o.shape != tuple(shape) or o.dtype != dtype or not o.dtype.isnative:
        raise ValueError(f"out: a {np.dtype(dtype)} device array of shape {tuple(shape)} expected (got {o.dtype} {o.shape})")
    if any(s <= 0 or s % o.dtype.itemsize for s in o.strides):
        raise ValueError(f"out: strides {o.strides}: positive multiples of the {o.dtype.itemsize} bytes of an element expected")
    return o


class _DeviceSource:
    """batch._HostSource's device form: frames f0 .. f0+nf-1 of the caller's array into the input plane, one kernel;
    the first load makes the context's stream wait for the caller's"""

    def __init__(self, d, stream):
        self.d, self.stream, self.shape = d, stream, d.shape

    def load(self, bp, f0, nf):
        d = self.d
        _lib.batch_load_device(bp, PLANE_INPUT, nf, d.ptr + f0 * d.strides[0], d.dtype, d.strides,
                               stream=self.stream if f0 == 0 else None)


class _DeviceSink:
    """batch._HostSink's device form: a plane of the batch into out[f0:f0+nf] or out[f0:f0+nf, index], one kernel;
    the last store makes the caller's stream wait for the context's"""

    def __init__(self, o, stream):
        self.o, self.stream = o, stream

    def store(self, bp, plane, f0, nf, index=None, last=False):
        o = self.o
        ptr = o.ptr + f0 * o.strides[0]
        strides = o.strides
        if index is not None:
            ptr += index * o.strides[1]
            strides = (o.strides[0],) + o.strides[2:]
        _lib.batch_store_device(bp, plane, nf, ptr, strides, stream=self.stream if last else None)


def _download(d):
    """the device array as an ndarray of its shape and element type (any strides): its byte extent crosses once"""
    if not d.size:
        return np.empty(d.shape, d.dtype)
    lo, hi = d.extent()
    raw = np.empty(hi - lo, np.uint8)
    ctx = _lib.default_context()
    _lib.device_copy(ctx, raw.ctypes.data, d.ptr + lo, hi - lo, _lib.COPY_DEVICE_TO_HOST)
    return np.ndarray(d.shape, d.dtype, raw, -lo, d.strides)


def _upload_into(o, res):
    """out[...] = res for a checked `out`: one copy where it is contiguous; else its byte extent is read, filled and
    written back (the bytes between its elements keep their values)"""
    if not o.size:
        return
    ctx = _lib.default_context()
    if o.c_contiguous:
        a = np.ascontiguousarray(res, dtype=o.dtype)
        _lib.device_copy(ctx, o.ptr, a.ctypes.data, a.nbytes, _lib.COPY_HOST_TO_DEVICE)
        return
    lo, hi = o.extent()
    raw = np.empty(hi - lo, np.uint8)
    _lib.device_copy(ctx, raw.ctypes.data, o.ptr + lo, hi - lo, _lib.COPY_DEVICE_TO_HOST)
    np.ndarray(o.shape, o.dtype, raw, -lo, o.strides)[...] = res
    _lib.device_copy(ctx, o.ptr + lo, raw.ctypes.data, hi - lo, _lib.COPY_HOST_TO_DEVICE)


def _staged(d, out, o, host_call):
    """the route of everything the device route does not cover: download, the host function, upload"""
    res = host_call(_download(d))
    if out is None:
        return DeviceArray.from_numpy(res)
    _upload_into(o, res)
    return out


def _run(d, out, o, shape, rdt, f64, level, scaling_function, stream, chunks, body):
    """the device route: the result array, the cached batch, `body(bp, source, sink)`, the end of the stream contract"""
    ctx = _lib.default_context()
    res = out
    if out is None:
        res = DeviceArray.empty(shape, rdt, ctx)
        o = _describe(res)
    N, H, W = d.shape
    with _batch(f64, max(nf for _, nf in chunks), H, W, _family_of(scaling_function(2)), level) as bp:
        body(bp, _DeviceSource(d, stream), _DeviceSink(o, stream))
    if stream is None:
        ctx.sync()                       # (no stream to hand the result over on: it is complete on return)
    return res


def transform_stack(frames, level, scaling_function=B3spline, out=None, stream=None):
    """(N, level+1, H, W) device array: batch.transform_stack(host copy of frames, level, scaling_function), bit for
    bit and in its element type, from and to device memory.  `out`: a device array of that shape and type with
    positive strides that are multiples of the element size (cube[:, s] of a larger block, a cropped view), returned
    as given; else a fresh DeviceArray.  `stream`: see the module's text.  `frames` is left untouched."""
    d = _frames(frames)
    stream = _stream_of(stream, d)
    N, H, W = d.shape
    rdt = _result_dtype(np.zeros((), d.dtype))
    o = None if out is None else _out_desc(out, (N, level + 1, H, W), rdt)
    f64 = _route(d, level, scaling_function, ())
    if f64 is None:
        return _staged(d, out, o, lambda host: _batch_mod.transform_stack(host, level, scaling_function))
    level = int(level)                   # (an eligible level is a whole number)
    chunks = _plan_chunks(N, H, W, level, f64)
    return _run(d, out, o, (N, level + 1, H, W), rdt, f64, level, scaling_function, stream, chunks,
                lambda bp, src, sink: _transform_chunks(bp, src, chunks, level, None, False, sink))


def denoise_stack(frames, weights, scaling_function=B3spline, noise=None, soft_threshold=True, anscombe=False,
                  out=None, stream=None):
    """(N, H, W) device array: batch.denoise_stack(host copy of frames, weights, scaling_function, noise,
    soft_threshold, anscombe), bit for bit and in its element type, from and to device memory.  `noise` (host
    values): None, a real scalar, or one entry per frame, each None or a real scalar; noise maps are staged.
    `out`, `stream`: as transform_stack's.  `frames` is left untouched."""
    d = _frames(frames)
    stream = _stream_of(stream, d)
    N, H, W = d.shape
    rdt = _result_dtype(np.zeros((), d.dtype))
    o = None if out is None else _out_desc(out, (N, H, W), rdt)
    level = len(weights)
    nl = _noise_list(noise, N, (H, W)) if N else None
    f64 = _route(d, level, scaling_function, nl)
    if f64 is None:
        return _staged(d, out, o, lambda host: _batch_mod.denoise_stack(host, weights, scaling_function, noise,
                                                                        soft_threshold, anscombe))
    chunks = _plan_chunks(N, H, W, level, f64)
    return _run(d, out, o, (N, H, W), rdt, f64, level, scaling_function, stream, chunks,
                lambda bp, src, sink: _denoise_chunks(bp, src, chunks, nl, weights, scaling_function, soft_threshold,
                                                      anscombe, None, sink))
