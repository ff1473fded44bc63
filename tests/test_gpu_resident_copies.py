"""The two copy kernels of wavelets_amd.resident on their own: wt_resident_copy_kernel<E, T, STORE, VEC>
(wavelets_amd/csrc/wt_resident_kernels.h) through _lib.batch_load_device / _lib.batch_store_device on a BatchPlan and a
BatchPlan64 made here, against the copy written in numpy:

    a load    plane[f0:f0+nf, :H, :W] = view.astype(T)      and every other frame of the plane keeps what it held
    a store   view[...] = plane[f0:f0+nf]                    and every other byte of the array's block keeps what it held

Every comparison is on bits.  Before a load every frame of the plane holds a sentinel (poison), before a store every byte
of the array's block does: a lane that moves nothing, or the wrong row, leaves the sentinel where the data belongs.  The
cases are the paths of the kernel and of its launcher (resident_launch, resident_copy in wt_resident.hip): the four-row
unrolled loop and its remainder, a second x block, the partial last 16-byte group at every remainder, every term of the
VEC condition, every element type off the vector path, a first frame other than 0, the plane's padding columns, frame
strides beyond 2^31 bytes, and the refusals."""
import numpy as np
import pytest

from wavelets_amd import _lib as L
from wavelets_amd import resident as R

pytestmark = pytest.mark.gpu

PLANE = L.PLANE_INPUT
NAN = float("nan")
FINITE = -2.5e38                 # the sentinel of the cases whose data holds NaNs: a float32 value no case's data holds
FLOAT_PLANE = (np.uint8, np.float32)                                          # resident_loads(dtype, float)
DOUBLE_PLANE = (np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64)  # resident_loads(dtype, double)

_batches = {}


def batch(f64, n, H, W):
    """a BatchPlan (float planes) or, `f64`, a BatchPlan64 (double planes) of n frames of H x W; closed with the module"""
    key = (bool(f64), n, H, W)
    if key not in _batches:
        _batches[key] = (L.BatchPlan64 if f64 else L.BatchPlan)(L.default_context(), n, H, W, L.B3SPLINE, 0)
    return _batches[key]


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    while _batches:
        _batches.popitem()[1].close()


both_batches = pytest.mark.parametrize("f64", [False, True], ids=["float-planes", "double-planes"])


def real(f64):
    return np.dtype(np.float64 if f64 else np.float32)


def loadable(f64):
    return DOUBLE_PLANE if f64 else FLOAT_PLANE


def values(shape, dtype, seed=0):
    """distinct-looking values of an element type, exact in it (integers: the whole range)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        return (rng.standard_normal(shape) * 20 + 100).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)


def specials(dtype):
    """the values a conversion or a copy can get wrong: the ends of the range; for float types -0.0, both infinities,
    the smallest and the largest denormal, and quiet and signalling NaNs with a payload and either sign"""
    dtype = np.dtype(dtype)
    if dtype.kind != "f":
        info = np.iinfo(dtype)
        return np.array([info.min, info.max, 0, 1], dtype)
    fi = np.finfo(dtype)
    u = np.uint32 if dtype.itemsize == 4 else np.uint64
    nans = (0x7FC12345, 0xFFC00001, 0x7F812345, 0xFFBFFFFF) if dtype.itemsize == 4 else \
        (0x7FF8123456789ABC, 0xFFF8000000000001, 0x7FF0123456789ABC, 0xFFF7FFFFFFFFFFFF)
    denormal = np.array([1, (1 << (fi.nmant)) - 1], u).view(dtype)
    return np.concatenate([np.array([fi.min, fi.max, -0.0, 0.0, np.inf, -np.inf, fi.tiny], dtype), denormal, -denormal,
                           np.array(nans, u).view(dtype)])


def special_block(shape, dtype, seed=0):
    """values() with every third element, in memory order, one of specials(): every view of the block holds them all"""
    block = values(shape, dtype, seed)
    flat = block.reshape(-1)
    flat[::3] = np.resize(specials(dtype), flat[::3].size)
    return block


def bits(a, nan_equal=False):
    """the bytes of an array in C order; `nan_equal`: every NaN first becomes the one quiet NaN"""
    a = np.array(a, order="C", copy=True)
    if nan_equal and a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a.reshape(-1).view(np.uint8)


def assert_bits(got, want, what, nan_equal=False):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = bits(got, nan_equal), bits(want, nan_equal)
    if not np.array_equal(g, w):
        item = got.dtype.itemsize
        bad = np.unique(np.flatnonzero(g != w) // item)
        at = np.unravel_index(bad[0], got.shape)
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at {tuple(int(i) for i in at)}: "
                             f"{got[at]!r} != {want[at]!r}")


def offset_of(host_block, host_view):
    return host_view.__array_interface__["data"][0] - host_block.__array_interface__["data"][0]


def device_view(dev, host_block, host_view):
    """resident.view of the part of the device block `dev` (a copy of host_block) that host_view is of host_block"""
    return R.view(dev.ptr + offset_of(host_block, host_view), host_view.shape, host_view.dtype, host_view.strides)


def same_view(other_block, host_block, host_view):
    """the view of other_block (same bytes layout as host_block) that host_view is of host_block"""
    raw = other_block.reshape(-1).view(np.uint8)
    return np.ndarray(host_view.shape, host_view.dtype, raw, offset_of(host_block, host_view), host_view.strides)


def poison(bp, plane=PLANE, sentinel=NAN):
    """the sentinel into all bp.n frames of the plane, padding columns included"""
    bp.fill(bp.n, plane, sentinel)


def check_load(bp, host_block, host_view, f0=0, sentinel=NAN, what="load"):
    """upload the block, load the view at f0: frames [f0, f0+nf) of the plane are host_view.astype(T), every other
    frame still holds the sentinel.  Returns the downloaded plane."""
    nf = host_view.shape[0]
    dev = R.DeviceArray.from_numpy(host_block)
    try:
        poison(bp, PLANE, sentinel)
        v = device_view(dev, host_block, host_view)
        L.batch_load_device(bp, PLANE, nf, v.ptr, v.dtype, v.strides, f0=f0)
        got = np.array(bp.download(PLANE, bp.n))
        assert_bits(dev.numpy(), host_block, f"{what}: the array after the load")
    finally:
        dev.free()
    want = np.full((bp.n, bp.H, bp.W), sentinel, bp.dtype)
    with np.errstate(invalid="ignore"):                            # (numpy reports the signalling NaNs it widens)
        want[f0:f0 + nf] = host_view.astype(bp.dtype)
    # same-type copies keep every bit (NaN payloads: the sentinel is then FINITE); a widening float32 -> float64 is
    # numpy's astype with NaNs taken as equal; with the NaN sentinel the data holds no NaN and every NaN is the sentinel
    exact = host_view.dtype == np.dtype(bp.dtype) and sentinel == sentinel
    assert_bits(got, want, what, nan_equal=not exact)
    return got


def check_store(bp, frames, host_block, host_view, f0=0, what="store"):
    """upload `frames` (bp.n of them) into a plane, a device copy of the sentinel-filled block in place, store nf
    frames at f0 into the view: the whole block equals the host block with host_view[...] = frames[f0:f0+nf], byte for
    byte - the view filled and nothing else touched"""
    nf = host_view.shape[0]
    assert frames.shape == (bp.n, bp.H, bp.W) and frames.dtype == bp.dtype and host_view.dtype == bp.dtype
    bp.upload(L.PLANE_OUT, frames)
    dev = R.DeviceArray.from_numpy(host_block)
    try:
        v = device_view(dev, host_block, host_view)
        L.batch_store_device(bp, L.PLANE_OUT, nf, v.ptr, v.strides, f0=f0)
        got = dev.numpy()
    finally:
        dev.free()
    assert_bits(np.array(bp.download(L.PLANE_OUT, bp.n)), frames, f"{what}: the plane after the store")
    want = host_block.copy()
    same_view(want, host_block, host_view)[...] = frames[f0:f0 + nf]
    assert_bits(got, want, what)


def check_both_ways(bp, host_block, host_view, f0=0, sentinel=NAN, what=""):
    """check_load, and for an array of the plane's own type check_store into the same arrangement (the block then
    filled with a byte pattern that is no value of the frames)"""
    got = check_load(bp, host_block, host_view, f0, sentinel, f"load {what}")
    if host_view.dtype == np.dtype(bp.dtype):
        frames = values((bp.n, bp.H, bp.W), bp.dtype, 11)
        sblock = np.frombuffer(bytes([0xA5]) * host_block.nbytes, host_block.dtype).reshape(host_block.shape).copy()
        check_store(bp, frames, sblock, same_view(sblock, host_block, host_view), f0, f"store {what}")
    return got


# ------------------------------------------------------------------------------------- the unrolled loop of the rows
@both_batches
def test_unrolled_rows_and_remainder(f64):
    """64 frames of 300 x 5 (rows of 20 or 40 bytes: no VEC) and of 300 x 8 (contiguous, 16-byte aligned: VEC).
    resident_launch: gx = 1 and nf = 64, so want = ceil(8 * num_cus / 64) = ceil(num_cus / 8) and gy = min(300, want):
    gy <= 64 for any device of up to 512 compute units, so 4 * gy <= 256 < 300 and every workgroup runs the unrolled
    body at least once.  On the 256 compute units of an MI355X gy = 32: a workgroup with blockIdx.y = y0 < 32 runs the
    unrolled body twice (rows y0 + 32 u and y0 + 128 + 32 u, u = 0..3: y0 + 128 + 96 < 300, y0 + 256 + 96 >= 300), then
    the remainder loop for row y0 + 256 and, for y0 < 12, row y0 + 288 - remainders of one and of two rows."""
    t = real(f64)
    for W in (5, 8):
        bp = batch(f64, 64, 300, W)
        block = values((64, 300, W), t, W)
        check_both_ways(bp, block, block, what=f"64 x 300 x {W}")


# ---------------------------------------------------------------------------------------------- a second x block
@both_batches
def test_second_x_block_element_path(f64):
    """2 x 3 x 261 at an inner stride of two elements: no VEC, gx = ceil(261 / 256) = 2, the boundary inside the row"""
    block = values((2, 3, 522), real(f64), 1)
    check_both_ways(batch(f64, 2, 3, 261), block, block[:, :, ::2], what="2 x 3 x 261, stride 2")


@both_batches
def test_second_x_block_vec_path(f64):
    """float planes: 1030 floats = 257 full groups and one of two elements, 258 lanes; double planes: 517 doubles = 258
    full groups and one element, 259 lanes: gx = 2, the boundary inside the row, a partial last group in block 1.
    Rows pitched to a multiple of 16 bytes (1032 floats, 518 doubles).  The 1030 floats also go into double planes
    (515 groups of two: gx = 3)."""
    W, pitch = (517, 518) if f64 else (1030, 1032)
    block = values((2, 3, pitch), real(f64), 2)
    assert block.strides[1] % 16 == 0
    check_both_ways(batch(f64, 2, 3, W), block, block[:, :, :W], what=f"2 x 3 x {W} pitched")
    if f64:
        block = values((2, 3, 1032), np.float32, 3)
        check_load(batch(True, 2, 3, 1030), block, block[:, :, :1030], what="float32 2 x 3 x 1030 into doubles")


# ------------------------------------------------------------------------------------- the partial last group (VEC)
@both_batches
def test_partial_last_group_at_every_remainder(f64):
    """rows of 16 elements of every loadable type (16-byte aligned whatever the type: VEC), widths with every remainder
    of the plane's group (4 floats: 4k, 4k+1, 4k+2, 4k+3; 2 doubles: 2k, 2k+1), W = 3 (float planes: one partial group
    and no full one) and W = 1"""
    for W in (1, 3, 8, 9, 10, 11):
        bp = batch(f64, 2, 3, W)
        for dtype in loadable(f64):
            block = values((2, 3, 16), dtype, W)
            assert block.strides[1] % 16 == 0 and block.strides[0] % 16 == 0
            check_both_ways(bp, block, block[:, :, :W], what=f"{np.dtype(dtype).name} W={W}")


# ------------------------------------------------------------------------------ every term of the VEC condition
@both_batches
def test_vec_refused_by_each_term(f64):
    """The same 2 x 3 x 10 values from an aligned arrangement (VEC) and from four that each break one term of
    resident_copy's condition: the planes must come out identical.
    The plane side cannot break it: a plane comes from hipMalloc (256-byte aligned), its pitch is a multiple of 4
    floats or 2 doubles (16 bytes), and its frame stride is H * pitch, so frame_stride * sizeof(T) is a multiple of 16
    for every shape - there is no batch, float64 or float32, on which an odd f0 moves `base` off the 16-byte grid.  The
    odd f0 is run all the same (a batch of 3 frames): it stays on the VEC path."""
    t = real(f64)
    item = t.itemsize
    vals = values((2, 3, 10), t, 4)
    odd_pitch = 13 if not f64 else 11                # 52 or 88 bytes a row; 4 rows a frame: 208 or 352 bytes, 16 | both
    flat = np.zeros(2 * 3 * 12 + 64, t)
    odd_frame = np.lib.stride_tricks.as_strided(flat, (2, 3, 10), ((3 * 12 + 1) * item, 12 * item, item))
    arrangements = {
        "aligned": (np.zeros((2, 3, 12), t), lambda b: b[:, :, :10]),
        "base off the grid by one element": (np.zeros((2, 3, 16), t), lambda b: b[:, :, 1:11]),
        "row pitch": (np.zeros((2, 4, odd_pitch), t), lambda b: b[:, :3, :10]),
        "frame stride": (flat, lambda b: odd_frame),
    }
    bp = batch(f64, 2, 3, 10)
    planes = {}
    for name, (block, view_of) in arrangements.items():
        hv = view_of(block)
        a, r, c = hv.strides
        aligned = c == item and (hv.__array_interface__["data"][0] - block.__array_interface__["data"][0]) % 16 == 0 \
            and r % 16 == 0 and a % 16 == 0
        assert aligned == (name == "aligned"), name
        hv[...] = vals
        planes[name] = check_both_ways(bp, block, hv, what=name)
        assert_bits(planes[name], planes["aligned"], f"{name} against the aligned arrangement")
    bp3 = batch(f64, 3, 3, 10)
    assert (bp3.frame_stride * item) % 16 == 0
    block, view_of = arrangements["aligned"]
    got = check_both_ways(bp3, block[:1], view_of(block)[:1], f0=1, what="f0 = 1")
    assert_bits(got[1], planes["aligned"][0], "f0 = 1 against the aligned arrangement")


# --------------------------------------------------------------------------- every element type, the element path
@both_batches
def test_every_element_type_off_the_vector_path(f64):
    """rows of 23 elements (23, 46, 92 and 184 bytes: never a multiple of 16, so no view of the block takes VEC): a
    pitched view off the grid, an inner stride of two, every second frame, one element per row.  A third of the elements
    are specials(): same-type copies keep their bits, float32 into doubles is numpy's astype (NaNs taken as equal)."""
    for dtype in loadable(f64):
        block = special_block((4, 6, 23), dtype, 5)
        assert block.strides[1] % 16
        sentinel = FINITE if np.dtype(dtype).kind == "f" else NAN
        for name, hv in (("pitched", block[:2, :5, 1:20]), ("inner stride two", block[:2, :5, ::2]),
                         ("every second frame", block[::2, :5, :19]), ("one element per row", block[1::2, 2:4, 7:8])):
            bp = batch(f64, hv.shape[0], hv.shape[1], hv.shape[2])
            check_both_ways(bp, block, hv, sentinel=sentinel, what=f"{np.dtype(dtype).name} {name}")


def test_special_values_on_the_vector_path():
    """the same-type copies and the float32 widening once more with specials(), through 16-byte groups"""
    for f64, dtype in ((False, np.float32), (True, np.float64), (True, np.float32)):
        block = special_block((2, 3, 16), dtype, 6)
        check_both_ways(batch(f64, 2, 3, 11), block, block[:, :, :11], sentinel=FINITE, what=f"{np.dtype(dtype).name} VEC")


# ------------------------------------------------------------------------------------------------------- f0 > 0
@both_batches
def test_first_frame_three_of_six(f64):
    """2 frames at f0 = 3 of a batch of 6, from and to frames 3 and 4 of a block of 6 (the view starts at
    ptr + 3 * stride): frames 0..2 and 5 of the plane keep the sentinel, the rest of the block its bytes.  Once on the
    VEC path, once off it."""
    bp = batch(f64, 6, 3, 10)
    block = values((6, 3, 12), real(f64), 7)
    check_both_ways(bp, block, block[3:5, :, :10], f0=3, what="f0 = 3 VEC")
    check_both_ways(bp, block, block[3:5, :, 1:11], f0=3, what="f0 = 3 element path")


# ---------------------------------------------------------------------------------------------- padding columns
@both_batches
def test_padding_columns_keep_their_values(f64):
    """W = 5: a pitch of 8 floats or 6 doubles.  The raw plane (plane_ptr, n * frame_stride elements) is written with
    values of its own, padding columns included; after a load the columns [W, pitch) hold them still.  VEC (a full
    group and a partial one) and the element path."""
    ctx = L.default_context()
    t = real(f64)
    bp = batch(f64, 2, 3, 5)
    assert bp.pitch == (6 if f64 else 8) and bp.frame_stride == 3 * bp.pitch
    for name, block, view_of in (("VEC", values((2, 3, 8), t, 8), lambda b: b[:, :, :5]),
                                 ("element path", values((2, 3, 5), t, 9), lambda b: b)):
        hv = view_of(block)
        before = values((bp.n * bp.frame_stride,), t, 10) + 1000
        ptr, fs = bp.plane_ptr(PLANE)
        assert fs == bp.frame_stride
        L.device_copy(ctx, ptr, before.ctypes.data, before.nbytes, L.COPY_HOST_TO_DEVICE)
        dev = R.DeviceArray.from_numpy(block)
        try:
            v = device_view(dev, block, hv)
            L.batch_load_device(bp, PLANE, 2, v.ptr, v.dtype, v.strides)
            after = np.empty_like(before)
            L.device_copy(ctx, after.ctypes.data, ptr, after.nbytes, L.COPY_DEVICE_TO_HOST)
        finally:
            dev.free()
        want = before.copy().reshape(bp.n, bp.H, bp.pitch)
        want[:, :, :5] = hv
        assert_bits(after.reshape(want.shape), want, f"raw plane after a load, {name}")


# ------------------------------------------------------------------------------------- offsets beyond 2^31 bytes
def test_frame_stride_beyond_two_gib():
    """2 frames of 3 x 5 float32, 2**31 + 16 bytes apart, in a block of about 2 GiB that is never uploaded: the two
    frames are written with one device_copy each.  Rows of 20 bytes (the element path) and rows pitched to 32 bytes
    (VEC); a load from the array into float and double planes, a store into it."""
    ctx = L.default_context()
    stride = 2 ** 31 + 16
    free, _ = ctx.device_memory()
    if free < 8 << 30:
        pytest.fail(f"{free / 2 ** 30:.1f} GiB of device memory free: the case of frame strides beyond 2**31 bytes needs "
                    f"8 GiB and was NOT run")
    span = 3 * 32                                             # bytes of a frame at the wider of the two row pitches
    ptr = L.device_alloc(ctx, stride + span)
    try:
        for name, pitch in (("element path", 5), ("VEC", 8)):
            frames_in = values((2, 3, pitch), np.float32, 12 + pitch)
            hv = frames_in[:, :, :5]
            strides = (stride, pitch * 4, 4)
            for f in range(2):
                L.device_copy(ctx, ptr + f * stride, frames_in[f].ctypes.data, frames_in[f].nbytes, L.COPY_HOST_TO_DEVICE)
            for f64 in (False, True):
                bp = batch(f64, 2, 3, 5)
                poison(bp)
                L.batch_load_device(bp, PLANE, 2, ptr, np.float32, strides)
                want = hv.astype(bp.dtype)
                assert_bits(np.array(bp.download(PLANE, 2)), want, f"load across 2**31 bytes, {name}, f64={f64}")
            bp = batch(False, 2, 3, 5)
            frames = values((2, 3, 5), np.float32, 13)
            bp.upload(L.PLANE_OUT, frames)
            marked = np.frombuffer(bytes([0xA5]) * frames_in.nbytes, np.float32).reshape(frames_in.shape).copy()
            for f in range(2):
                L.device_copy(ctx, ptr + f * stride, marked[f].ctypes.data, marked[f].nbytes, L.COPY_HOST_TO_DEVICE)
            L.batch_store_device(bp, L.PLANE_OUT, 2, ptr, strides)
            got = np.empty_like(marked)
            for f in range(2):
                L.device_copy(ctx, got[f].ctypes.data, ptr + f * stride, got[f].nbytes, L.COPY_DEVICE_TO_HOST)
            marked[:, :, :5] = frames
            assert_bits(got, marked, f"store across 2**31 bytes, {name}")
    finally:
        L.device_free(ctx, ptr)


# ----------------------------------------------------------------------------------------------------- refusals
@both_batches
def test_refusals_leave_planes_and_array_untouched(f64):
    """host logic, before any launch: each raises WatrooHipError naming the entry; afterwards the plane still holds the
    sentinel in every frame and the array's block its bytes"""
    t = real(f64)
    item = t.itemsize
    entry = "wt_batch64_" if f64 else "wt_batch_"
    bp = batch(f64, 3, 3, 10)
    block = values((3, 3, 10), t, 14)
    dev = R.DeviceArray.from_numpy(block)
    frames = values((3, 3, 10), t, 15)
    try:
        poison(bp)
        bp.upload(L.PLANE_OUT, frames)
        good = block.strides
        code = L._ELEM_CODES[t.str[1:]]

        def load(nf=2, dtype=t, strides=good, f0=0):
            L.batch_load_device(bp, PLANE, nf, dev.ptr, dtype, strides, f0=f0)

        def store(nf=2, strides=good, f0=0):
            L.batch_store_device(bp, L.PLANE_OUT, nf, dev.ptr, strides, f0=f0)

        def load_null_handle():
            bp._call("load_device", PLANE, 0, 2, L._vp(dev.ptr), code, (L._i64 * 3)(*good), None, L.STREAM_HANDLE)

        def store_null_handle():
            bp._call("store_device", L.PLANE_OUT, 0, 2, L._vp(dev.ptr), (L._i64 * 3)(*good), None, L.STREAM_HANDLE)

        refused = []
        if not f64:
            refused.append(("int16 into a float plane", lambda: load(dtype=np.int16, strides=(60, 20, 2))))
        for axis in range(3):
            for name, s in (("a stride of 0", 0), ("a negative stride", -good[axis]), ("a stride off the item size", good[axis] + 1)):
                st = tuple(s if i == axis else g for i, g in enumerate(good))
                refused.append((f"load, {name}, axis {axis}", lambda st=st: load(strides=st)))
                refused.append((f"store, {name}, axis {axis}", lambda st=st: store(strides=st)))
        refused += [("load, f0 + nf > n", lambda: load(nf=2, f0=2)), ("store, f0 + nf > n", lambda: store(nf=2, f0=2)),
                    ("load, nf = 0", lambda: load(nf=0)), ("store, nf = 0", lambda: store(nf=0)),
                    ("load, a negative f0", lambda: load(f0=-1)), ("store, a negative f0", lambda: store(f0=-1)),
                    ("load, a null stream handle", load_null_handle), ("store, a null stream handle", store_null_handle)]
        for name, call in refused:
            which = entry + ("store_device" if name.startswith("store") else "load_device")
            with pytest.raises(L.WatrooHipError, match=which):
                call()
        assert_bits(np.array(bp.download(PLANE, 3)), np.full((3, 3, 10), NAN, t), "the plane after the refusals", nan_equal=True)
        assert_bits(np.array(bp.download(L.PLANE_OUT, 3)), frames, "the stored plane after the refusals")
        assert_bits(dev.numpy(), block, "the array after the refusals")
        load()                                                                 # ... and the same calls, unbroken, go through
        assert_bits(np.array(bp.download(PLANE, 3))[:2], block[:2], "a good load after the refusals")
    finally:
        dev.free()
