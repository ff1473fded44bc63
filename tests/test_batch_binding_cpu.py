"""The Python layer above the batched engines makes the calls it always made (no GPU):

* binding traces - every public method of _lib.BatchPlan and _lib.BatchPlan64, called once on an object built without a
  device, with a stand-in for the library that records (symbol, arguments);
* route traces - transform_stack, denoise_stack, wow_stack, enhance_stack and richardson_lucy_stack on recorders that
  stand in for the batches: the batch_chunks and acquire arguments, every call on the batch, where the downloads land.

The expected traces (test_batch_binding_cpu.json, next to this file) were recorded by binding_traces() and
route_traces() of this module on the commit before BatchPlan and BatchPlan64 got their common base and the stack
functions their common drivers; they are data, not derived from the code under test."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

import wavelets_amd as W
from wavelets_amd import _lib as L
from wavelets_amd import batch as B

with open(os.path.splitext(os.path.abspath(__file__))[0] + ".json") as _f:
    EXPECTED = json.load(_f)

NF, H, Wd = 3, 5, 7


# ---------------------------------------------------------------- plain data of what a call was given
def _plain(v):
    """ctypes arrays -> [element type name, values]; pointers -> their type name; numpy scalars -> [type name, value];
    ndarrays -> their element type, shape and strides; sequences -> lists; numbers as they are"""
    if isinstance(v, ctypes.Array):
        return [v._type_.__name__, list(v)]
    if isinstance(v, (ctypes._Pointer, ctypes.c_void_p)) or type(v).__name__ == "CArgObject":
        return type(v).__name__
    if isinstance(v, np.ndarray):
        return ["ndarray", v.dtype.str, list(v.shape), list(v.strides)]
    if isinstance(v, np.generic):
        return [type(v).__name__, v.item()]
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def _json(v):
    return json.loads(json.dumps(v))


# ---------------------------------------------------------------- binding traces
class _Library:
    """stands in for the loaded library: every attribute records (symbol, arguments) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        def entry(*args):
            self.calls.append([symbol, [_plain(a) for a in args]])
            return 0
        return entry


class _Ctx:
    _h = ctypes.c_void_p(1)


def _frames(dtype):
    return (np.arange(NF * H * Wd).reshape(NF, H, Wd) % 11 - 3).astype(dtype)


def _binding_calls(cls):
    """(method, arguments, keywords) of one call of every public method, in a fixed order"""
    item = np.dtype(cls.dtype)
    cube = np.zeros((NF, 4, H, Wd), item)
    calls = [("upload", (L.PLANE_INPUT, _frames(dt)), {}) for dt in (np.float32, np.float64, np.int16, ">f4")]
    calls += [
        ("upload", (2, _frames(np.float64)[1:2]), {"f0": 1}),
        ("download", (L.PLANE_OUT, NF), {"out": np.zeros((NF, H, Wd), item)}),
        ("download", (1, NF), {"out": cube[:, 1]}),
        ("download", (1, 2), {"out": cube[1:, 2], "f0": 1}),
        ("plane_ptr", (2,), {}),
        ("decompose", (NF, L.PLANE_INPUT, 3), {}),
        ("decompose", (2, 1, 2, 0), {}),
        ("decompose_bilateral", (NF, L.PLANE_INPUT, 2, [2.0, 0.5, 1]), {}),
        ("decompose_bilateral", (NF, L.PLANE_INPUT, 3, [2.0, 0.5, 1], True, 1), {}),
        ("decompose_sum", (NF, L.PLANE_INPUT, 3), {}),
        ("decompose_sum", (NF, L.PLANE_INPUT, 3, 2, 0), {}),
        ("decompose_pass", (NF, L.PLANE_INPUT, 1, 0, 2), {}),
        ("decompose_pass_sum", (NF, 1, 2, 2, 1, L.FLAG_FUSED, L.PLANE_OUT), {"first": False, "last": True}),
        ("abs_median", (NF, 0), {}),
        ("denoise_sum", (NF, 3, [[1.0, 0.5], [2, 0], [0.25, 3.0]], [1, 0.5]), {}),
        ("denoise_sum", (NF, 3, [[1.0, 0.5], [2, 0], [0.25, 3.0]], [1, 0.5], False, True, 4), {}),
        ("denoise_sum", (NF, 3, [[1.0, 0.5], [2, 0], [0.25, 3.0]], [1, 0.5], True), {"noise_plane": 5}),
        ("denoise_sum", (NF, 3, [[1.0, 0.5], [2, 0], [0.25, 3.0]], [1, 0.5], True),
         {"noise_plane": 5, "has_map": [True, False, 1]}),
        ("denoise_sum", (NF, 3, [[1.0, 0.5], [2, 0], [0.25, 3.0]], [1, 0.5]), {"has_map": [True, False, True]}),
        ("enhance_sum", (NF, 3, [[1.0, 0.5], [2, 0], [0.25, 3.0]], [[1, 0.5], [1, 1], [0, 2]]), {}),
        ("enhance_sum", (NF, 3, [[1.0, 0.5], [2, 0], [0.25, 3.0]], [[1, 0.5], [1, 1], [0, 2]], False, True, 4), {}),
        ("anscombe", (NF, L.PLANE_INPUT, L.PLANE_INPUT), {}),
        ("anscombe", (NF, L.PLANE_OUT, L.PLANE_OUT, 2.0, 0.5, 0.25), {"inverse": True}),
        ("fill", (NF, 3, 1.0), {}),
        ("replicate", (NF, 3), {}),
        ("wow_update", (NF, 1, [0.0, 1.5, 2], True, [0.1, np.float32(0.2), 3]), {}),
        ("wow_update", (NF, 1, [0.0, 1.5, 2], False, [0.1, np.float64(0.2), 3], 4), {"noise_plane": 5}),
        ("wow_scale", (NF, 1, 1, [0.0, 1.5, 2], True, [0.1, np.float32(0.2), 3]), {}),
        ("wow_scale", (NF, 1, 1, [0.0, 1.5, 2], False, [0.1, np.float64(0.2), 3], 4), {"noise_plane": 5}),
        ("reduce", (NF, 2), {}),
        ("gamma_blend", (NF, L.PLANE_OUT, 4, [0.1, 0.2, 0.3], [1.1, 1.2, 1.3], 1 / 3.2, 0.5), {}),
        ("plane_sum", (NF, 0, 4), {}),
        ("plane_sum", (NF, 0, 4, 2), {}),
    ]
    if cls is L.BatchPlan:
        calls += [
            ("fill_normal", (NF, 1, 12345), {}),
            ("fill_normal", (NF, 1, 2 ** 63 + 1, 7), {}),
            ("filter2d", (NF, 1, 2, 0), {}),
            ("set_psf", (0, np.ones((3, 5))), {}),
            ("set_psf", (1, np.ones((4, 2), np.float32)), {}),
            ("filter2d", (NF, 1, 2, 0), {}),
            ("filter2d", (NF, 1, 2, 1, (0, 1), True), {}),
            ("binary", (NF, "add_div", 1, 2, 3), {}),
            ("binary", (NF, "sub", 1, 2, 3), {}),
            ("mrs_update", (NF, 1, 6, [0.0, 1.5, 2], True, False, 0.5), {}),
            ("fft_spectrum", (3,), {}),
            ("fft_apply", (NF, 1, 2), {}),
            ("fft_apply", (NF, 1, 2, True), {}),
        ]
    return calls


def _public_methods(cls):
    return sorted(n for n in dir(cls) if not n.startswith("_") and inspect.isfunction(getattr(cls, n)))


def binding_traces(monkeypatch):
    """{class name: [[method, library calls, result]]}: the constructor, every public method, close"""
    traces = {}
    for cls in (L.BatchPlan, L.BatchPlan64):
        lib = _Library()
        monkeypatch.setattr(L, "load", lambda lib=lib: lib)
        rows = []
        made = object.__new__(cls)                      # the constructor's own calls (the info it reads back is zeros)
        cls.__init__(made, _Ctx(), NF, H, Wd, L.B3SPLINE, 4)
        rows.append(["__init__", lib.calls[:], [made.n, made.H, made.W, made.pitch, made.frame_stride]])
        made._h = ctypes.c_void_p()                     # nothing left to destroy
        bp = object.__new__(cls)
        bp._h, bp.ctx = ctypes.c_void_p(2), _Ctx()
        bp.n, bp.H, bp.W, bp.max_level, bp.family = NF, H, Wd, 4, L.B3SPLINE
        bp.pitch = L._batch_pitch(Wd, np.dtype(cls.dtype).itemsize)
        bp.frame_stride = H * bp.pitch
        called = set()
        try:
            for name, args, kw in _binding_calls(cls) + [("close", (), {})]:
                del lib.calls[:]
                res = getattr(bp, name)(*args, **kw)
                rows.append([name, lib.calls[:], None if name == "download" else _plain(res)])
                called.add(name)
            assert not bp._h                            # closed: __del__ finds nothing to destroy
        finally:
            bp._h = ctypes.c_void_p()
        assert called == set(_public_methods(cls)), called ^ set(_public_methods(cls))
        traces[cls.__name__] = rows
    return _json(traces)


def test_every_binding_call_is_the_recorded_one(monkeypatch):
    got = binding_traces(monkeypatch)
    for name in ("BatchPlan", "BatchPlan64"):
        want = EXPECTED["binding"][name]
        assert [r[0] for r in got[name]] == [r[0] for r in want]
        for g, w in zip(got[name], want):
            assert g == w, (name, g[0])


def signatures():
    """the methods both classes have, the ones only BatchPlan has, and the signature of each common one"""
    both = sorted(set(_public_methods(L.BatchPlan)) & set(_public_methods(L.BatchPlan64)))
    return {"common_methods": both, "float32_only": sorted(set(_public_methods(L.BatchPlan)) - set(both)),
            "signatures": {m: str(inspect.signature(getattr(L.BatchPlan, m))) for m in both + ["__init__", "_per_frame"]}}


def test_the_two_classes_keep_their_own_methods_and_common_signatures():
    got = signatures()
    assert got == {k: EXPECTED[k] for k in got}
    assert set(_public_methods(L.BatchPlan64)) == set(got["common_methods"])      # nothing of the float32 batch's own
    assert not issubclass(L.BatchPlan64, L.BatchPlan) and not hasattr(L.BatchPlan64, "filter2d")
    for meth, sig in got["signatures"].items():
        assert str(inspect.signature(getattr(L.BatchPlan64, meth))) == sig, meth
    assert L.BatchPlan.dtype is np.float32 and L.BatchPlan64.dtype is np.float64
    with pytest.raises(ValueError, match="one value per active frame"):
        L.BatchPlan64._per_frame([1.0], 2, ctypes.c_double, "wow_scale taus")


# ---------------------------------------------------------------- route traces
FH, FW = 64, 80            # wow_stack's floor of 1024 pixels per frame for float64 stacks and noise maps, with room to spare


class _Batch:
    """a BatchPlan / BatchPlan64 without a device: records the calls of the stack routes; a download writes the
    number of the call into its target, so the result shows where every download landed"""

    def __init__(self, n, Hh, Ww, dtype, level):
        self.n, self.H, self.W, self.dtype, self.max_level, self.calls = n, Hh, Ww, dtype, level, []

    def __getattr__(self, name):
        def call(*a, **k):
            args = [_plain(x) + [float(np.sum(x, dtype=np.float64))] if isinstance(x, np.ndarray) else _plain(x) for x in a]
            self.calls.append([name, args, _plain(k)])
            if name == "abs_median":
                return [self.dtype(0.5 + f) for f in range(a[0])]
            if name == "reduce":
                return [(1.0 + f, 2.0 * self.H * self.W, -1.0, 1.0 + f) for f in range(a[0])]
            if name == "download":
                k["out"][...] = len(self.calls)
        return call


def _stack(dtype, colour=False):
    shape = (3, 3, FH, FW) if colour else (3, FH, FW)
    return (np.arange(int(np.prod(shape))).reshape(shape) % 23 - 4).astype(dtype)


def _map(seed):
    return (np.arange(FH * FW).reshape(FH, FW) % (5 + seed) + 0.5) / 3


def _effective(a, k):
    """(n, H, W, level, extra_planes, itemsize) of a batch_chunks call, defaults filled in"""
    assert len(a) == 4 and set(k) <= {"extra_planes", "itemsize"}, (a, k)
    return list(a) + [k.get("extra_planes", 0), k.get("itemsize", 4)]


def route_cases():
    """[(label, function, arguments, keywords, BATCH_BYTES or None)]"""
    cases = []
    for dt in ("<f4", "<f8", "<i2", ">f4"):
        for bil in (None, 1):
            cases.append((f"transform-{dt}-bil{bil}", "transform_stack", (_stack(dt), 3), dict(bilateral=bil), None))
    cases.append(("transform-<f8-bil-list-scaling", "transform_stack", (_stack("<f8"), 3, W.Triangle),
                  dict(bilateral=[2., .5], bilateral_scaling=True), None))
    cases.append(("transform-<f4-three-chunks", "transform_stack", (_stack("<f4"), 3), {}, 1))
    cases.append(("transform-<i2-three-chunks", "transform_stack", (_stack("<i2"), 3), {}, 1))
    m0, m1 = _map(0), _map(1)
    noises = {"scalar": 0.7, "per-frame": [1.0, None, 0.5], "shared-map": m0, "mixed": [m0, 2.5, None], "maps": [m0, m1, m0]}
    for dt in ("<f4", "<f8"):
        for label, noise in noises.items():
            for ans in (False, True):
                for budget in (None, 1):
                    cases.append((f"denoise-{dt}-{label}-ans{int(ans)}-chunks{3 if budget else 1}", "denoise_stack",
                                  (_stack(dt), [5, 3]), dict(noise=noise, anscombe=ans), budget))
        cases.append((f"denoise-{dt}-bilateral-hard", "denoise_stack", (_stack(dt), [5, 0, 3]),
                      dict(bilateral=1, soft_threshold=False), None))
        cases.append((f"denoise-{dt}-split-schedule", "denoise_stack", (_stack(dt), [4, 2, 1, 0, 0]), dict(noise=None), None))
    wows = {"default": {}, "h": dict(h=0.5), "no-whitening": dict(whitening=False, denoise_coefficients=[5, 2]),
            "map": dict(noise=m0, denoise_coefficients=[5, 2]),
            "mixed-maps": dict(noise=[m0, 1.5, None], denoise_coefficients=[5, 0, 2], h=1),
            "bilateral": dict(bilateral=1, denoise_coefficients=[5]), "coefficients": dict(return_coefficients=True, h=0.25)}
    for dt in ("<f4", "<f8", "<i2"):
        for label, kw in wows.items():
            cases.append((f"wow-{dt}-{label}", "wow_stack", (_stack(dt),), kw, None))
        cases.append((f"wow-{dt}-three-chunks", "wow_stack", (_stack(dt),), dict(h=0.5, noise=[1.0, None, 0]), 1))
    for dt in ("<f4", "<f8"):
        cases.append((f"enhance-{dt}-gray", "enhance_stack", (_stack(dt),), dict(weights=[1, 2], denoise=[3, 1]), None))
        cases.append((f"enhance-{dt}-gray-noise", "enhance_stack", (_stack(dt), [0.5, 1, 2]), dict(weights=[1, 2]), None))
        cases.append((f"enhance-{dt}-colour", "enhance_stack", (_stack(dt, True),),
                      dict(weights=[[1, 2], [1, 2], [1, 2]], denoise=[[3, 1], [3, 1], [3, 1]]), None))
        cases.append((f"enhance-{dt}-colour-levels", "enhance_stack", (_stack(dt, True), [0.5, 1, 2]),
                      dict(weights=[[1, 2], [1, 2, 3], [2, 1]]), None))
        cases.append((f"enhance-{dt}-colour-chunks", "enhance_stack", (_stack(dt, True),),
                      dict(weights=[[1, 2], [2, 1], [1, 1]]), 1))
    psf_small = np.outer([1., 2, 3, 2, 1], [1., 2, 4, 2, 1])
    psf_large = np.outer(np.hanning(25)[1:-1], np.hanning(25)[1:-1])
    cases.append(("rl-direct", "richardson_lucy_stack", (_stack("<f4"), psf_small), dict(iterations=2), None))
    cases.append(("rl-direct-hard-chunks", "richardson_lucy_stack", (_stack("<f4"), psf_small),
                  dict(iterations=1, threshold_type="hard", persistent_mrs=False, denoise_coefficients=(3, 0)), 1))
    cases.append(("rl-fft", "richardson_lucy_stack", (_stack("<f4"), psf_large), dict(iterations=2, fft=True), None))
    cases.append(("rl-fft-small-psf", "richardson_lucy_stack", (_stack("<f4"), psf_small), dict(iterations=1, fft=True), None))
    return cases


def _landing(res):
    """the value every frame (and plane) of a result holds: the number of the download that wrote it"""
    res = np.asarray(res)
    assert res.shape[-2:] == (FH, FW)
    flat = res.reshape(-1, FH * FW)
    assert np.all(flat == flat[:, :1])                  # (every download fills whole frames)
    return [res.dtype.str, list(res.shape), flat[:, 0].tolist()]


def route_trace(monkeypatch, case):
    label, func, args, kw, budget = case
    batches, chunk_calls, acquired, released = [], [], [], []
    real_chunks = L.batch_chunks

    def boom(*a, **k):
        raise AssertionError(f"{label}: the per-frame loop ran")

    def acquire(dtype, which):
        def fn(ctx, n, Hh, Ww, fam, level):
            assert ctx == "ctx"
            acquired.append([which, n, Hh, Ww, fam, level])
            batches.append(_Batch(n, Hh, Ww, dtype, level))
            return batches[-1]
        return fn

    with monkeypatch.context() as m:
        m.setattr(L, "default_context", lambda: "ctx")
        m.setattr(L, "batch_chunks", lambda *a, **k: chunk_calls.append(_effective(a, k)) or real_chunks(*a, **k))
        m.setattr(L, "acquire_batch", acquire(np.float32, "acquire_batch"))
        m.setattr(L, "acquire_batch64", acquire(np.float64, "acquire_batch64"))
        m.setattr(L, "release_batch", lambda bp: released.append(["release_batch", batches.index(bp)]))
        m.setattr(L, "release_batch64", lambda bp: released.append(["release_batch64", batches.index(bp)]))
        for name in ("AtrousTransform", "denoise", "wow", "enhance", "richardson_lucy"):
            if not (name == "AtrousTransform" and func == "enhance_stack"):     # (enhance_stack reads its options there)
                m.setattr(B, name, boom)
        if budget is not None:
            m.setattr(L, "BATCH_BYTES", budget)
        res = getattr(B, func)(*args, **kw)
    assert batches, label
    results = [_landing(r) for r in (res if isinstance(res, tuple) else (res,))]
    return _json({"chunks": chunk_calls, "acquired": acquired, "released": released,
                  "calls": [b.calls for b in batches], "results": results})


CASES = route_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_route_makes_the_recorded_calls(monkeypatch, case):
    got = route_trace(monkeypatch, case)
    want = EXPECTED["routes"][case[0]]
    for key in ("chunks", "acquired", "released", "results"):
        assert got[key] == want[key], key
    assert len(got["calls"]) == len(want["calls"])
    for g_batch, w_batch in zip(got["calls"], want["calls"]):
        assert [c[0] for c in g_batch] == [c[0] for c in w_batch]
        for i, (g, w) in enumerate(zip(g_batch, w_batch)):
            assert g == w, (i, g[0])


def test_the_recorded_routes_are_the_issue_s_cases():
    assert sorted(EXPECTED["routes"]) == sorted(c[0] for c in CASES) and len(set(c[0] for c in CASES)) == len(CASES)
    for dt in ("<f4", "<f8"):
        for label in ("scalar", "per-frame", "shared-map", "mixed"):
            for ans in (0, 1):
                one, three = (EXPECTED["routes"][f"denoise-{dt}-{label}-ans{ans}-chunks{n}"] for n in (1, 3))
                assert [c[0] for c in one["calls"][0]].count("download") == 1
                assert [c[0] for c in three["calls"][0]].count("download") == 3
    kinds = {k.split("-")[0] for k in EXPECTED["routes"]}
    assert kinds == {"transform", "denoise", "wow", "enhance", "rl"}
    assert EXPECTED["routes"]["wow-<f8-default"]["acquired"][0][0] == "acquire_batch64"
    assert EXPECTED["routes"]["rl-fft"]["calls"][0][1][0] == "fft_spectrum"
