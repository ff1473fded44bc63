"""richardson_lucy_stack over float64, integer and big-endian stacks without a GPU: the routing predicate rl64_eligible
clause by clause, the PSF limits of the tiled float64 correlation (8-byte samples in the LDS tile), the chunk
arithmetic at 8 bytes per pixel, the loud failure of an eligible stack without a device, the binding (RLBatchPlan64,
a subclass: BatchPlan64 keeps its method set) and the five new entries of the C ABI - and the cases of
tests/test_gpu_rl64_stack.py with their float64 numpy oracle (oracle.atrous_numpy.richardson_lucy per frame), settled
here: finite and positive.

Frames are those of tests/test_rl_stack_cpu.py in float64 - positive, neighbouring frames decades apart - or their
int16 / '>f4' casts (scaled to counts first), so a row or a tap read from the wrong frame is an error of order one."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from test_rl_stack_cpu import make_psf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


def _mods():
    import wavelets_amd as W
    from wavelets_amd import batch as B, utils as U, _lib as L
    return W, B, U, L


def make_frames64(n, H, W, seed, dtype="<f8"):
    """positive frames, frame i scaled by 10 ** (i % 3) (integer frames: by 30 * that, counts up to a few thousand)"""
    rng = np.random.default_rng(seed)
    ridge = 4 * np.exp(-((np.arange(W) - 0.45 * W) ** 2) / (2 * (0.08 * W + 1) ** 2))[None, :]
    dt = np.dtype(dtype)
    unit = 30.0 if dt.kind in "iu" else 1e-2
    frames = np.stack([(rng.uniform(0.5, 1.5, (H, W)) + ridge) * unit * 10.0 ** (i % 3) for i in range(n)])
    return np.rint(frames).astype(dt) if dt.kind in "iu" else frames.astype(dt)


# name, dtype, frames (n, H, W), PSF (kh, kw), keywords of the call, frames per chunk (0: one chunk)
CASES = [
    dict(name="float64_default", dtype="<f8", shape=(4, 40, 48), psf=(7, 5), kw=dict(iterations=3)),
    dict(name="int16", dtype="<i2", shape=(4, 40, 48), psf=(7, 5), kw=dict(iterations=3)),
    dict(name="big_endian_f4", dtype=">f4", shape=(4, 40, 48), psf=(7, 5), kw=dict(iterations=3)),
    dict(name="hard_fresh_support_level_2", dtype="<f8", shape=(4, 40, 48), psf=(7, 5),
         kw=dict(iterations=3, threshold_type="hard", persistent_mrs=False, denoise_coefficients=(4, 2))),
    dict(name="fft_odd_height", dtype="<f8", shape=(3, 37, 50), psf=(5, 5), kw=dict(iterations=3, fft=True)),
    dict(name="eight_scales", dtype="<f8", shape=(2, 64, 80), psf=(3, 3),
         kw=dict(iterations=3, denoise_coefficients=(5, 4, 3, 2, 1, 1, 1, 1))),
    dict(name="chunks_of_2", dtype="<f8", shape=(5, 40, 48), psf=(6, 4), kw=dict(iterations=3), chunk=2),
]
CASE_IDS = [c["name"] for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


def is_soft(c):
    return c["kw"].get("threshold_type", "soft") == "soft"


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(frames, psf) of a case, from a generator seeded by the case's position; read-only"""
    c = case(name)
    frames = make_frames64(*c["shape"], seed=300 + CASE_IDS.index(name), dtype=c["dtype"])
    psf = make_psf(*c["psf"])
    frames.setflags(write=False)
    psf.setflags(write=False)
    return frames, psf


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the float64 numpy oracle of every frame of a soft-threshold case, computed once; read-only"""
    from oracle import atrous_numpy as O
    c = case(name)
    frames, psf = case_inputs(name)
    ref = np.stack([np.asarray(O.richardson_lucy(f.astype(np.float64), psf.astype(np.float64), **c["kw"]), np.float64)
                    for f in frames])
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", [n for n in CASE_IDS if is_soft(case(n))])
def test_oracle_of_the_gpu_cases_is_settled(name):
    frames, psf = case_inputs(name)
    assert (frames > 0).all() and abs(float(psf.sum(dtype=np.float64)) - 1) < 1e-6
    ref = case_reference(name)
    assert ref.shape == frames.shape and ref.dtype == np.float64 and np.isfinite(ref).all()
    assert (ref > 0).all()
    # the frames are decades apart and so are their estimates: a mixed-up frame is an error of order one
    for i in range(len(frames)):
        ratio = float(ref[i].mean() / frames[i].astype(np.float64).mean())
        assert 0.5 < ratio < 2.0, (i, ratio)


def test_every_gpu_case_is_rl64_eligible_and_not_the_float32_routes():
    W, B, U, L = _mods()
    for c in CASES:
        frames, psf = case_inputs(c["name"])
        level = len(c["kw"].get("denoise_coefficients", (5, 2, 1)))
        fft = c["kw"].get("fft", False)
        assert B.rl64_eligible(frames, psf, level, False, fft), c["name"]
        assert not B.rl_eligible(frames, psf, level, False, fft) and not B.rl_fft_eligible(frames, psf, level), c["name"]


# ---------------------------------------------------------------- the predicate, clause by clause
def test_rl64_eligible_frames_clause():
    W, B, U, L = _mods()
    assert "rl64_eligible" in B.__all__ and W.batch.rl64_eligible is B.rl64_eligible
    psf = make_psf(3, 3)
    for dt in ("<f8", "<i2", "<u2", "<i4", "<u4", "<i8", ">f4", ">f8"):
        assert B.rl64_eligible(make_frames64(2, 32, 32, 1, dt), psf, 3), dt
    f64 = make_frames64(2, 32, 32, 1)
    assert not B.rl64_eligible(f64.astype(np.float32), psf, 3)                   # rl_eligible's
    assert B.rl_eligible(f64.astype(np.float32), psf, 3) and not B.rl_eligible(f64, psf, 3)
    assert not B.rl64_eligible([f for f in f64], psf, 3)                          # a list of frames
    assert not B.rl64_eligible(f64[0], psf, 3)                                    # one image
    assert not B.rl64_eligible(f64, psf, 3, uniform_init=True)
    assert not B.rl64_eligible(f64, psf, 3, True)


def test_rl64_eligible_level_clause():
    W, B, U, L = _mods()
    f64, psf = make_frames64(2, 32, 32, 1), make_psf(3, 3)
    assert [lv for lv in range(0, 11) if B.rl64_eligible(f64, psf, lv)] == list(B.BATCH_LEVELS) == list(range(2, 9))
    assert not B.rl64_eligible(f64, psf, 1) and not B.rl64_eligible(f64, psf, 9)
    assert not B.rl64_eligible(f64, psf, True) and not B.rl64_eligible(f64, psf, 3.0)
    assert B.rl64_eligible(f64, psf, np.int64(3))


def test_rl64_eligible_pixel_floor():
    W, B, U, L = _mods()
    psf = make_psf(3, 3)
    assert B.RL64_MIN_PIXELS == B.WOW_MAP_MIN_PIXELS == 1024
    assert not B.rl64_eligible(make_frames64(2, 31, 33, 1), psf, 3)              # 1023 pixels
    assert B.rl64_eligible(make_frames64(2, 32, 32, 1), psf, 3)                  # 1024
    assert not B.rl64_eligible(make_frames64(3, 12, 16, 1), psf, 3)              # (the loop pinned by test_rl_stack_cpu.py)


def test_rl64_eligible_psf_and_fft_clauses(monkeypatch):
    W, B, U, L = _mods()
    f64 = make_frames64(2, 40, 48, 1)
    assert not B.rl64_eligible(f64, np.ones(9), 3) and not B.rl64_eligible(f64, np.ones((3, 3, 1)), 3)
    assert not B.rl64_eligible(f64, np.ones((0, 3)), 3) and not B.rl64_eligible(f64, np.ones((3, 3), complex), 3)
    assert B.rl64_eligible(f64, np.ones((3, 3), np.int32), 3)
    assert U._FFT_MIN_TAPS == 512
    assert B.rl64_eligible(f64, make_psf(22, 23), 3, fft=True)                    # 506 taps: the direct periodic form
    assert not B.rl64_eligible(f64, make_psf(23, 23), 3, fft=True)                # 529: the per-frame call leaves it
    assert B.rl64_eligible(f64, make_psf(23, 23), 3, fft=False)
    monkeypatch.setattr(U, "_FFT_MIN_TAPS", 100)                                  # (read when called)
    assert not B.rl64_eligible(f64, make_psf(22, 23), 3, fft=True) and B.rl64_eligible(f64, make_psf(9, 11), 3, fft=True)
    monkeypatch.undo()
    short = make_frames64(2, 18, 64, 1)
    assert not B.rl64_eligible(short, make_psf(21, 5), 3, fft=True)               # kh > H
    assert not B.rl64_eligible(short.transpose(0, 2, 1).copy(), make_psf(5, 21), 3, fft=True)     # kw > W
    assert B.rl64_eligible(short, make_psf(21, 5), 3)                             # a tall PSF on a short frame: symmetric border


def _rule64(kh, kw):
    return kh >= 1 and kw >= 1 and kw <= 512 and kh * kw <= 4096 and (64 + kw - 1) * (16 + kh - 1) * 8 <= 96 * 1024


def test_psf_limits_at_eight_bytes_per_sample():
    W, B, U, L = _mods()
    f64 = make_frames64(2, 96, 96, 1)
    assert 127 * 79 * 8 <= 96 * 1024 and B.rl64_eligible(f64, make_psf(64, 64), 3)
    assert L.batch_psf_ok(369, 1) and not L.batch64_psf_ok(369, 1)               # 64 x 384 samples: 96 KB of floats
    assert B.rl_eligible(f64.astype(np.float32), make_psf(369, 1), 3) and not B.rl64_eligible(f64, make_psf(369, 1), 3)
    assert not B.rl64_eligible(f64, make_psf(65, 65), 3)                          # 4225 taps
    shapes = [(1, 1), (64, 64), (65, 64), (64, 65), (65, 65), (1, 512), (1, 513), (8, 512), (4, 512), (5, 512),
              (176, 1), (177, 1), (178, 1), (369, 1), (177, 2), (176, 2), (128, 32), (100, 40), (90, 45), (0, 3), (3, 0), (-1, 3)]
    for kh, kw in shapes:
        assert L.batch64_psf_ok(kh, kw) == _rule64(kh, kw), (kh, kw)
    assert L.batch64_psf_ok(177, 1) and not L.batch64_psf_ok(178, 1)             # 64 * 192 * 8 = 96 KB exactly
    # with fft=True an odd height adds a zero row to the operands (utils._rl_direct_operands): the operand is what counts
    odd = make_frames64(2, 181, 64, 1)
    (fk, _), (bk, _) = U._rl_direct_operands(make_psf(177, 1), 181, True)
    assert B.rl64_eligible(odd, make_psf(177, 1), 3, fft=True) == (L.batch64_psf_ok(*fk.shape) and L.batch64_psf_ok(*bk.shape))


def test_chunks_count_the_planes_of_the_float64_route(monkeypatch):
    W, B, U, L = _mods()
    for level in (2, 3, 8):
        H, Wd = 40, 47
        pitch = 48                                                                # doubles, even
        frame = (2 * level + 9) * H * pitch * 8
        assert L.batch_frame_bytes(H, Wd, level, 8) + B._rl_extra_planes(level) * H * pitch * 8 == frame
        monkeypatch.setattr(L, "BATCH_BYTES", 3 * frame + frame // 2)
        assert B._plan_chunks(7, H, Wd, level, True, B._rl_extra_planes(level)) == [(0, 3), (3, 3), (6, 1)]
        monkeypatch.setattr(L, "BATCH_BYTES", 3 * frame - 1)
        assert B._plan_chunks(7, H, Wd, level, True, B._rl_extra_planes(level)) == [(0, 2), (2, 2), (4, 2), (6, 1)]


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, data, psf, **kw):
        self.calls.append((data, psf, kw))
        return np.zeros(np.shape(data))


def test_eligible_float64_stack_without_a_gpu_fails_loudly_instead_of_looping(monkeypatch):
    W, B, U, L = _mods()
    if L.device_count() > 0:
        pytest.skip("a GPU is visible")
    rec = _Recorder()
    monkeypatch.setattr(B, "richardson_lucy", rec)
    for dt in ("<f8", "<i2"):
        with pytest.raises(L.WatrooHipError, match="no CPU fallback"):
            W.richardson_lucy_stack(make_frames64(2, 32, 32, 3, dt), make_psf(3, 3))
    assert not rec.calls


def test_ineligible_float64_stacks_keep_the_per_frame_loop(monkeypatch):
    W, B, U, L = _mods()
    rec = _Recorder()
    monkeypatch.setattr(B, "richardson_lucy", rec)
    monkeypatch.setattr(L, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    small = make_frames64(3, 12, 16, 3)
    got = B.richardson_lucy_stack(small, make_psf(3, 3), iterations=2)
    assert len(rec.calls) == 3 and got.shape == small.shape
    big = make_frames64(2, 40, 48, 3)
    B.richardson_lucy_stack(big, make_psf(23, 23), iterations=1, fft=True)       # the float64 FFT products: per frame
    assert len(rec.calls) == 5 and rec.calls[-1][2]["fft"] is True


def test_out_is_checked_before_any_device_work(monkeypatch):
    W, B, U, L = _mods()
    monkeypatch.setattr(L, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    monkeypatch.setattr(B, "richardson_lucy", lambda *a, **k: (_ for _ in ()).throw(AssertionError("per-frame call")))
    f64 = make_frames64(2, 32, 32, 3)
    with pytest.raises(ValueError, match="out: an array of shape"):
        B.richardson_lucy_stack(f64, make_psf(3, 3), out=np.zeros((3, 32, 32)))
    with pytest.raises(ValueError, match="out: float32 array of shape"):          # (a float32 stack: the text it had)
        B.richardson_lucy_stack(f64.astype(np.float32), make_psf(3, 3), out=np.zeros((2, 32, 32), np.float64))


# ---------------------------------------------------------------- binding and C ABI
def _public(cls):
    return {n for n in dir(cls) if not n.startswith("_") and inspect.isfunction(getattr(cls, n))}


def test_rl_batch_plan64_is_a_subclass_with_the_four_calls_of_batch_plan():
    W, B, U, L = _mods()
    assert issubclass(L.RLBatchPlan64, L.BatchPlan64) and not issubclass(L.RLBatchPlan64, L.BatchPlan)
    extra = _public(L.RLBatchPlan64) - _public(L.BatchPlan64)
    assert extra == {"set_psf", "filter2d", "binary", "mrs_update"}
    for m in extra:
        assert not hasattr(L.BatchPlan64, m)
        assert str(inspect.signature(getattr(L.RLBatchPlan64, m))) == str(inspect.signature(getattr(L.BatchPlan, m))), m
    assert L.RLBatchPlan64._prefix == "wt_batch64_" and L.RLBatchPlan64.dtype is np.float64
    assert L.release_rl_batch64 is L.release_batch


class _Fake:
    """an object of a batch class without a device, for the cache"""

    def __init__(self, cls, ctx, n, shape):
        self.__class__ = cls
        self._h, self.ctx, self.n = 1, ctx, n
        (self.H, self.W, self.family, self.max_level) = shape

    def close(self):
        self._h = None


def test_the_cache_keeps_the_two_float64_classes_apart(monkeypatch):
    W, B, U, L = _mods()
    monkeypatch.setattr(L, "_batch_cache", L._StackCache())
    made = []
    for cls in (L.BatchPlan64, L.RLBatchPlan64):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, _c=cls: made.append(_c))
        monkeypatch.setattr(cls, "__del__", lambda self: None, raising=False)
    ctx = object()
    shape = (32, 32, L.B3SPLINE, 3)
    plain, rl = _Fake(L.BatchPlan64, ctx, 4, shape), _Fake(L.RLBatchPlan64, ctx, 4, shape)
    L.release_batch64(plain)
    assert type(L.acquire_rl_batch64(ctx, 2, *shape)) is L.RLBatchPlan64 and made == [L.RLBatchPlan64]     # a new one
    assert L.acquire_batch64(ctx, 2, *shape) is plain
    L.release_rl_batch64(rl)
    assert type(L.acquire_batch64(ctx, 2, *shape)) is L.BatchPlan64 and made == [L.RLBatchPlan64, L.BatchPlan64]
    assert L.acquire_rl_batch64(ctx, 2, *shape) is rl


NEW_SYMBOLS = ("wt_batch64_psf_ok", "wt_batch64_set_psf", "wt_batch64_filter2d", "wt_batch64_binary", "wt_batch64_mrs_update")


def test_header_declares_and_library_exports_the_new_entries():
    W, B, U, L = _mods()
    header = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for sym in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % sym, header, re.M), sym
        assert sym in L.SIGNATURES and sym in exported, sym
    assert re.search(r"wt_batch64_set_psf\(wt_batch64 \*batch, int slot, const double \*kernel, int kh, int kw\)", header)
    assert re.search(r"wt_batch64_mrs_update\([^)]*double inv_pow\)", header)
