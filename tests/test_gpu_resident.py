"""wavelets_amd.resident on the GPU: transform_stack / denoise_stack from a device array to a device array have the
bits and the element type of batch.transform_stack / batch.denoise_stack on the downloaded input - at the shapes where
the two copy kernels can go wrong (one element, widths that are no multiple of the 16-byte group, pitched rows, an
inner stride of two, every second frame), with every widened element type, through more than one chunk, into views of
larger blocks, on every stream form, through the staged route and through a PyTorch tensor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import batch as B
from wavelets_amd import resident as R
from wavelets_amd.wavelets import _result_dtype

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


def check_both(dev_frames, host_frames, level=2, weights=(5, 3), **kw):
    before = host_frames.copy()
    t = R.transform_stack(dev_frames, level)
    want = B.transform_stack(host_frames, level)
    assert t.dtype == _result_dtype(host_frames) == want.dtype and same(t.numpy(), want)
    d = R.denoise_stack(dev_frames, list(weights), **kw)
    want = B.denoise_stack(host_frames, list(weights), **kw)
    assert d.dtype == want.dtype and same(d.numpy(), want)
    return before


# ------------------------------------------------------------------------------------------------ the copy kernels
@pytest.mark.parametrize("shape, dtype", [((3, 5, 7), np.float32), ((2, 1, 1), np.float32), ((2, 16, 64), np.float32),
                                          ((2, 9, 33), np.float64), ((2, 16, 64), np.float64), ((2, 2, 1), np.float64)])
def test_contiguous_stacks(shape, dtype):
    a = stack(shape, dtype)
    dev = R.DeviceArray.from_numpy(a)
    assert R.eligible(dev, 2)
    check_both(dev, a)
    assert same(dev.numpy(), a)                                    # the input is left untouched


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strided_views(dtype):
    block = stack((4, 64, 160), dtype, 1)
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
    want_t, want_d = B.transform_stack(a, 3), B.denoise_stack(a, [4, 2, 1], noise=[None, 1.0, 2, None, 0.5])
    seen = []

    def chunks_of_two(n, H, W, level, f64, extra_planes=0):
        seen.append(n)
        return [(f0, min(2, n - f0)) for f0 in range(0, n, 2)]

    monkeypatch.setattr(R, "_plan_chunks", chunks_of_two)
    assert same(R.transform_stack(dev, 3).numpy(), want_t)
    assert same(R.denoise_stack(dev, [4, 2, 1], noise=[None, 1.0, 2, None, 0.5]).numpy(), want_d)
    a64 = a.astype(np.float64)
    assert same(R.denoise_stack(R.DeviceArray.from_numpy(a64), [4, 2, 1]).numpy(), B.denoise_stack(a64, [4, 2, 1]))
    assert seen == [5, 5, 5]


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
        assert R.denoise_stack(dev, [5, 3], out=o) is o
        expect = big.copy()
        hv(expect)[...] = want
        assert same(dbig.numpy(), expect)                          # the view filled, every other byte as it was
    # transform_stack: the planes into a cropped view big[:, :, 1:-1, 2:-3] of a larger cube
    want = B.transform_stack(a, 3)
    dbig = R.DeviceArray.from_numpy(big)
    o = sub_view(dbig, big, big[:, :, 1:-1, 2:-3])
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
        assert same(R.denoise_stack(dev, [5, 3, 1], **kw).numpy(), B.denoise_stack(a, [5, 3, 1], **kw)), kw
        assert same(R.denoise_stack(dev64, [5, 3, 1], **kw).numpy(), B.denoise_stack(a64, [5, 3, 1], **kw)), kw
    assert same(R.transform_stack(dev, 4, W.Triangle).numpy(), B.transform_stack(a, 4, W.Triangle))


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


def test_staged_route():
    a = stack((2, 12, 17))
    dev = R.DeviceArray.from_numpy(a)
    assert not R.eligible(dev, 2, Retapped)
    assert same(R.transform_stack(dev, 2, Retapped).numpy(), B.transform_stack(a, 2, Retapped))
    assert same(R.denoise_stack(dev, [5, 3], Retapped).numpy(), B.denoise_stack(a, [5, 3], Retapped))
    block = stack((2, 12, 40), np.float32, 7)
    dblock = R.DeviceArray.from_numpy(block)
    hv = block[:, ::-1, 3:20]                                      # a negative stride: staged
    v = sub_view(dblock, block, hv)
    assert not R.eligible(v, 2)
    big = np.zeros((2, 12, 30), np.float32)
    dbig = R.DeviceArray.from_numpy(big)
    o = sub_view(dbig, big, big[:, :, 5:22])
    assert R.denoise_stack(v, [5, 3], out=o) is o
    big[:, :, 5:22] = B.denoise_stack(hv, [5, 3])
    assert same(dbig.numpy(), big)
    half = a.astype(np.float16)
    assert same(R.denoise_stack(R.DeviceArray.from_numpy(half), [5, 3]).numpy(), B.denoise_stack(half, [5, 3]))


# ------------------------------------------------------------------------------------------------- interface, streams
def test_device_array_hand_off():
    a = stack((2, 6, 10), np.float64, 8)
    d = R.DeviceArray.from_numpy(a)
    assert same(d.numpy(), a) and same(d.numpy(out=np.empty_like(a)), a)
    cai = d.__cuda_array_interface__
    assert cai["version"] == 3 and cai["strides"] is None and cai["data"] == (d.ptr, False)
    alias = R.view(cai["data"][0], cai["shape"], cai["typestr"])
    res = R.DeviceArray.empty(a.shape, np.float64)
    assert R.denoise_stack(alias, [5, 3], out=res) is res and same(res.numpy(), B.denoise_stack(a, [5, 3]))
    R.denoise_stack(d, [5, 3], out=alias)                          # in place: the view aliases d
    assert same(d.numpy(), B.denoise_stack(a, [5, 3]))
    d.free()
    d.free()
    assert d.ptr == 0


def test_streams_give_the_same_bits():
    a = stack((3, 20, 36), np.float32, 9)
    dev = R.DeviceArray.from_numpy(a)
    want_t, want_d = B.transform_stack(a, 3), B.denoise_stack(a, [5, 3])
    for stream in (None, 1, 2):
        assert same(R.transform_stack(dev, 3, stream=stream).numpy(), want_t), stream
        assert same(R.denoise_stack(dev, [5, 3], stream=stream).numpy(), want_d), stream


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
