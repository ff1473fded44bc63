"""Host logic of wow over float64 and integer frame stacks (wavelets_amd.batch.wow_stack on the float64 batch): the
eligibility predicate wow64_eligible, the older predicates' unchanged answers, the new entry points of the library
(exported, declared, bound), the new translation unit and the argument checks that come before device work.  No GPU
needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B
from wavelets_amd import wavelets as WV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (3, 64, 80)
F64_TYPES = [np.float64, np.int16, np.uint16, np.int32, ">f4"]


def test_wow64_eligible_is_exported():
    assert "wow64_eligible" in B.__all__ and callable(B.wow64_eligible)
    assert B.WOW64_MIN_PIXELS == B.WOW_MAP_MIN_PIXELS == 1024


def test_wow64_eligibility_predicate():
    for dt in F64_TYPES:
        fr = np.zeros(SHAPE, dt)
        for level in (1, 4, 9, 10):
            assert B.wow64_eligible(fr, level), (dt, level)
        assert B.wow64_eligible(fr, 6, W.Triangle), dt
        assert B.wow64_eligible(fr, 4, noise_per_frame=[None, 0.0, np.float64(2)]), dt
    f64 = np.zeros(SHAPE)
    assert not B.wow64_eligible(f64.astype(np.float32), 4)                   # that route is wow_eligible's
    u8 = np.zeros(SHAPE, np.uint8)
    if WV._result_dtype(u8) == np.float32:
        assert not B.wow64_eligible(u8, 4)
    assert not B.wow64_eligible(np.zeros((3, 8, 8)), 1)                      # below the pixel floor
    assert not B.wow64_eligible(np.zeros((3, 1, 2048)), 4)                   # one-row frames: signals for the float64 engine
    assert not B.wow64_eligible(np.zeros((3, 31, 33)), 2) and B.wow64_eligible(np.zeros((3, 32, 32)), 2)
    assert not B.wow64_eligible(f64, 0) and not B.wow64_eligible(f64, 25)
    assert not B.wow64_eligible(f64, True) and not B.wow64_eligible(f64, 4.0)
    assert not B.wow64_eligible([f64[0], f64[1]], 4)                         # not stacked
    assert not B.wow64_eligible(np.zeros((1, 2, 100000)), 4)                 # rows too wide for the fused passes at 8 bytes

    class Retapped(W.B3spline):
        coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9
    assert not B.wow64_eligible(f64, 4, Retapped)

    class Custom(W.AbstractScalingFunction):
        coefficients_1d = np.array([0.2, 0.6, 0.2])

        def __init__(self, n_dim):
            super().__init__("custom", n_dim)
    assert not B.wow64_eligible(f64, 4, Custom)
    assert not B.wow64_eligible(f64, 4, noise_per_frame=[np.array(2.0)] * 3)  # 0-d array: wow()'s noise-map branch
    maps = [np.ones((64, 80))] * 3
    assert not B.wow64_eligible(f64, 4, noise_per_frame=maps)                 # maps: only with noise_maps=True
    assert B.wow64_eligible(f64, 4, noise_per_frame=maps, noise_maps=True)
    assert B.wow64_eligible(f64, 4, noise_per_frame=[maps[0], 2.0, None], noise_maps=True)
    assert not B.wow64_eligible(f64, 4, noise_per_frame=[np.ones((64, 81))] * 3, noise_maps=True)   # another shape
    assert not B.wow64_eligible(f64, 4, noise_per_frame=None)                 # one array of another shape for all


def test_few_large_float64_frames_stay_on_the_loop():
    """the measured rule (tools/bench_wow64_stack.py: 2 x 4096^2 float64 is behind the loop batched)"""
    assert (B.WOW64_FEW_FRAMES, B.WOW64_LARGE_PIXELS) == (2, 1 << 24)
    big = np.lib.stride_tricks.as_strided(np.zeros(1), (3, 4096, 4096), (0, 0, 0))      # (no 400 MB of zeros)
    assert not B.wow64_eligible(big[:1], 10) and not B.wow64_eligible(big[:2], 10, bilateral=1)
    assert B.wow64_eligible(big, 10)
    assert B.wow64_eligible(big[:2, :2048, :2048], 9) and B.wow64_eligible(big[:1, :4096, :4095], 9)


def test_wow64_eligible_with_bilateral_follows_bilateral64_eligible():
    f64 = np.zeros(SHAPE)
    assert B.wow64_eligible(f64, 4, bilateral=1) and B.wow64_eligible(f64, 3, bilateral=[1, 2])
    assert B.wow64_eligible(np.zeros(SHAPE, np.int16), 4, W.Triangle, bilateral=True)
    assert not B.wow64_eligible(f64, 4, bilateral="1") and not B.wow64_eligible(f64, 4, bilateral=np.ones(3))
    n = len(W.B3spline(2).sigma_e(bilateral=1))
    assert B.wow64_eligible(f64, min(n, 24), bilateral=1)
    if n < 24:
        assert not B.wow64_eligible(f64, n + 1, bilateral=1)                  # beyond the sigma_e(bilateral=) table
    assert not B.wow64_eligible(f64.astype(np.float32), 4, bilateral=1)


def test_the_schedule_condition_is_the_librarys():
    for code in (L.B3SPLINE, L.TRIANGLE):
        got = [lv for lv in range(0, 27) if L.batch64_wow_ok(code, 64, 80, lv)]
        assert got == list(range(1, 25)), (code, got)
        # wt_batch64_fused_ok keeps its meaning and its answers
        assert [lv for lv in range(0, 27) if L.batch64_fused_ok(code, 64, 80, lv)] == list(range(2, 9))
    assert not L.batch64_wow_ok(L.B3SPLINE, 1, 2048, 4) and not L.batch64_wow_ok(7, 64, 80, 4)
    assert not L.batch64_wow_ok(L.B3SPLINE, 2, 100000, 4) and L.batch64_wow_ok(L.B3SPLINE, 2, 80000, 4)


def test_the_older_predicates_keep_their_answers():
    for dt in F64_TYPES + [np.float32, np.uint8]:
        fr = np.zeros(SHAPE, dt)
        f32 = np.dtype(dt) == np.float32
        f64 = any(np.dtype(dt) == np.dtype(t) for t in F64_TYPES)
        for level in (1, 4, 9, 10):
            assert B.wow_eligible(fr, level) == f32, (dt, level)
            assert B.batch_eligible(fr, level) == (f32 and level == 4), (dt, level)
            assert B.batch64_eligible(fr, level) == (f64 and level == 4), (dt, level)
        assert B.bilateral_eligible(fr, 4, bilateral=1) == f32 and B.bilateral64_eligible(fr, 4, bilateral=1) == f64, dt
    f64 = np.zeros(SHAPE)
    assert not B.wow_eligible(f64, 4, noise_per_frame=[np.ones((64, 80))] * 3, noise_maps=True)
    assert not B.batch64_eligible(f64, 9) and not B.batch64_eligible(f64, 1)


def _header():
    raw = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    return raw, re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


def test_the_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    raw, header = _header()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    want = {"wt_batch64_wow_ok": ["family", "H", "W", "level", "ok"],
            "wt_batch64_wow_update": ["batch", "nf", "plane", "tau", "soft", "factor", "gamma_plane"],
            "wt_batch64_wow_scale": ["batch", "nf", "plane", "s", "tau", "soft", "factor", "gamma_plane"],
            "wt_batch64_wow_update_map": ["batch", "nf", "plane", "tau", "soft", "factor", "gamma_plane", "noise_plane"],
            "wt_batch64_wow_scale_map": ["batch", "nf", "plane", "s", "tau", "soft", "factor", "gamma_plane", "noise_plane"],
            "wt_batch64_reduce": ["batch", "nf", "plane", "out"],
            "wt_batch64_gamma_blend": ["batch", "nf", "recon", "gamma_plane", "gmin", "gmax", "inv_gamma", "h"],
            "wt_batch64_plane_sum": ["batch", "nf", "first", "count", "dst"]}
    for name, params in want.items():
        assert hasattr(lib, name), name
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == params, name
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        comment = raw[:raw.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "watroo/" in comment, name                                     # cites its reference call site
        # the float64 twin of the float32 entry: the same parameters, double where that has float
        twin = name.replace("wt_batch64_", "wt_batch_")
        if twin in L.SIGNATURES:
            m32 = re.search(r"int\s+" + twin + r"\s*\(([^)]*)\)", header)
            assert [a.split()[-1].lstrip("*") for a in m32.group(1).split(",")] == params, name
            assert "float" not in m.group(1) and m.group(1).replace("wt_batch64", "wt_batch").split() == \
                m32.group(1).replace("float", "double").split(), name
    # the factors travel as doubles (a float table would round what utils._wow_factor computed in float64)
    assert L.SIGNATURES["wt_batch64_wow_scale"][1][6] == dp and L.SIGNATURES["wt_batch64_wow_update"][1][5] == dp
    assert L.SIGNATURES["wt_batch64_gamma_blend"][1][4:] == [dp, dp, ctypes.c_double, ctypes.c_double]
    assert L.SIGNATURES["wt_batch64_wow_ok"][1][4] == ip
    for meth in ("wow_scale", "wow_update", "reduce", "gamma_blend", "plane_sum"):
        assert callable(getattr(L.BatchPlan64, meth)), meth
    assert callable(L.batch64_wow_ok)
    # the entries they stand beside keep their signatures
    for name, nargs in (("wt_batch64_decompose", 5), ("wt_batch64_fused_ok", 5), ("wt_batch_wow_scale", 8), ("wt_batch_reduce", 4)):
        assert len(L.SIGNATURES[name][1]) == nargs, name
    assert L.load().wt_abi_version() == 8                                     # additive: the version stays


def test_batchplan64_takes_batchplans_wow_arguments():
    import inspect
    for meth in ("wow_scale", "wow_update", "reduce", "gamma_blend", "plane_sum"):
        assert list(inspect.signature(getattr(L.BatchPlan64, meth)).parameters) == \
            list(inspect.signature(getattr(L.BatchPlan, meth)).parameters), meth
    with pytest.raises(ValueError, match="one value per active frame"):
        L.BatchPlan64._per_frame([1.0], 2, ctypes.c_double, "wow_scale taus")


def test_the_new_unit_is_built_and_probed():
    import __graft_entry__ as G
    units = {obj: (src, flags) for obj, src, flags in G._units()}
    assert units["stencil64_batch.o"] == ("wt_stencil64_batch.hip", ["-DWT_TU_NAME=stencil64_batch"])
    assert units["stencil64.o"] == ("wt_stencil64.hip", ["-DWT_TU_NAME=stencil64"])
    probe = open(os.path.join(ROOT, "wavelets_amd", "csrc", "wt_unit_probe.h")).read()
    assert "X(stencil64_batch)" in probe
    assert "stencil64_batch" in L.unit_names()
    launch = open(os.path.join(ROOT, "wavelets_amd", "csrc", "wt_stencil_launch.h")).read()
    assert re.search(r"int wt64_stencil_batch_launch\(const StencilCtx &\w+, int mode, const ChainArgsT<double> &\w+, int s, "
                     r"const char \*name, const WtFrames &\w+\);", launch)
    # wt_stencil64.hip itself instantiates no batched kernel
    assert "_batch" not in open(os.path.join(ROOT, "wavelets_amd", "csrc", "wt_stencil64.hip")).read()


def test_chunking_counts_wows_extra_planes_at_8_bytes():
    per = L.batch_frame_bytes(300, 517, 6, itemsize=8)
    plane = 300 * 518 * 8
    assert per == 11 * plane
    assert [n for _, n in L.batch_chunks(7, 300, 517, 6, budget=2 * (per + 3 * plane), extra_planes=3, itemsize=8)] == [2, 2, 2, 1]
    assert [n for _, n in L.batch_chunks(7, 300, 517, 6, budget=2 * (per + 3 * plane) - 1, extra_planes=3, itemsize=8)] == [1] * 7


# ---------------------------------------------------------------- routing and argument errors, without a device

def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    for name in ("default_context", "acquire_batch", "acquire_batch64"):
        monkeypatch.setattr(L, name, boom)


def test_argument_errors_before_device_work(monkeypatch):
    _no_device(monkeypatch)
    f64 = np.zeros((2, 64, 64))
    assert B.wow64_eligible(f64, 4)
    with pytest.raises(ValueError, match="out"):
        W.wow_stack(f64, out=np.zeros((2, 64, 64), np.float32))               # wrong dtype
    with pytest.raises(ValueError, match="out"):
        W.wow_stack(f64, out=np.zeros((2, 64, 65)))                            # wrong shape
    with pytest.raises(ValueError, match="out"):
        W.wow_stack(f64, out=np.zeros((2, 64, 128))[:, :, ::2])                # not C-contiguous
    with pytest.raises(ValueError, match="out"):
        W.wow_stack(f64.astype(np.int16), out=np.zeros((2, 64, 64), np.int16), bilateral=1)
    with pytest.raises(ValueError, match="one entry per frame"):
        W.wow_stack(np.zeros((3, 64, 64)), noise=[1.0, 2.0])
    with pytest.raises(ValueError, match="one shape"):
        W.wow_stack([np.zeros((64, 64)), np.zeros((64, 65))])


class _Recorder:
    """a stand-in for a BatchPlan64: records the calls wow_stack makes"""
    dtype = np.float64

    def __init__(self, n, H, W_, level):
        self.n, self.H, self.W, self.max_level, self.calls = n, H, W_, level, []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            if name == "reduce":
                return [(0.0, float(self.H * self.W), -1.0, 1.0)] * a[0]
            if name == "abs_median":
                return [np.float64(0.5)] * a[0]
            if name == "download":
                k["out"][...] = 7.0
        return call


def test_float64_stacks_take_the_float64_batch(monkeypatch):
    recs, chunk_calls = [], []
    real_chunks = L.batch_chunks
    monkeypatch.setattr(L, "default_context", lambda *a: object())
    monkeypatch.setattr(L, "acquire_batch", lambda *a: (_ for _ in ()).throw(AssertionError("float32 batch")))
    monkeypatch.setattr(L, "acquire_batch64", lambda ctx, n, H, W_, fam, lv: recs.append(_Recorder(n, H, W_, lv)) or recs[-1])
    monkeypatch.setattr(L, "release_batch64", lambda b: None)
    monkeypatch.setattr(L, "batch_chunks", lambda *a, **k: chunk_calls.append((a, k)) or real_chunks(*a, **k))
    monkeypatch.setattr(B, "wow", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the per-frame loop")))
    fr = np.ones((3, 64, 80), np.int16)
    out = np.empty((3, 64, 80))
    img, planes = W.wow_stack(fr, denoise_coefficients=[5, 2], h=0.5, noise=[1.0, None, 0], out=out, return_coefficients=True)
    assert img is out and img.dtype == np.float64 and planes.dtype == np.float64 and planes.shape == (3, 5, 64, 80)
    assert chunk_calls[0] == ((3, 64, 80, 4), {"extra_planes": 2, "itemsize": 8})       # spare + gamma planes, 8 bytes
    names = [c[0] for c in recs[0].calls]
    assert names[0] == "upload" and recs[0].calls[0][1][1].dtype == np.int16            # integer frames go up as they are
    assert names[1] == "decompose" and names.count("wow_scale") == 4 and names.count("wow_update") == 1
    assert names.count("abs_median") == 1 and names.count("plane_sum") == 1 and names.count("gamma_blend") == 1
    # the factors are computed in the batch's element type
    scales = [c for c in recs[0].calls if c[0] in ("wow_scale", "wow_update")]
    assert all(type(f) is np.float64 for c in scales for f in c[1][-2])
    # bilateral: the batched float64 march; a shared noise map: one more plane, the map forms of the updates
    chunk_calls.clear()
    m = np.ones((64, 80), np.float32)
    W.wow_stack(fr.astype(">f4"), bilateral=1, noise=m, denoise_coefficients=[5])
    assert chunk_calls[0][1] == {"extra_planes": 2, "itemsize": 8}
    names = [c[0] for c in recs[-1].calls]
    assert "decompose_bilateral" in names and "decompose" not in names and names.count("replicate") == 1
    ups = [c for c in recs[-1].calls if c[0] == "wow_scale"]
    assert ups[0][2] == {"noise_plane": WV._NOISE_PLANE} and all(c[2] == {} for c in ups[1:])
    assert [c[1][1].dtype for c in recs[-1].calls if c[0] == "upload"][1] == np.float64   # the map in the batch's type


def test_small_and_float32_stacks_keep_their_routes(monkeypatch):
    _no_device(monkeypatch)
    seen = []
    monkeypatch.setattr(B, "wow", lambda f, *a, **k: seen.append(f.dtype) or (f * 2, type("C", (), {"data": f[None]})()))
    img = B.wow_stack(np.ones((2, 8, 8)))                                     # below the floor: the loop, as before
    assert len(seen) == 2 and img.dtype == np.float64
    img = B.wow_stack(np.ones((2, 1, 2048)))                                  # one-row frames: the loop
    assert len(seen) == 4
    B.wow_stack(np.ones((2, 64, 64)), scaling_function=type("R", (W.B3spline,), {"coefficients_1d": np.array([1, 2, 3, 2, 1]) / 9}),
                n_scales=2)
    assert len(seen) == 6
