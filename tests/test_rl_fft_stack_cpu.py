"""richardson_lucy_stack(fft=True) with a large PSF, without a GPU: the routing predicate rl_fft_eligible clause by
clause (and rl_eligible unchanged beside it), wt_batch_fft_ok against wt_fft_supported, the planes the chunk budget
counts for the two complex work arrays, the calls each route issues on a recorded batch - and the cases of
tests/test_gpu_rl_fft_stack.py with their float64 numpy oracle (oracle.atrous_numpy.richardson_lucy per frame),
settled here: finite and positive.

Frames and PSFs are test_rl_stack_cpu's: positive frames nine decades apart, asymmetric normalised PSFs."""
import functools

import numpy as np
import pytest

import __graft_entry__ as entry
from test_rl_stack_cpu import make_frames, make_psf


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


def _mods():
    import wavelets_amd as W
    from wavelets_amd import batch as B, utils as U, _lib as L
    return W, B, U, L


# name, frames (n, H, W), PSF (kh, kw), keywords of the call (fft=True is added), frames per chunk (0: one chunk),
# utils._FFT_MIN_TAPS for the call (None: the default)
CASES = [
    dict(name="radix2_32x64_psf23x23", shape=(3, 32, 64), psf=(23, 23), kw=dict(iterations=3)),
    dict(name="odd_height_45x48_psf23x23", shape=(3, 45, 48), psf=(23, 23), kw=dict(iterations=3)),
    dict(name="hard_fresh_50x60_psf25x21", shape=(2, 50, 60), psf=(25, 21),
         kw=dict(iterations=3, threshold_type="hard", persistent_mrs=False)),
    dict(name="chunks_of_2_40x64_psf23x23", shape=(5, 40, 64), psf=(23, 23), kw=dict(iterations=3), chunk=2),
    dict(name="psf_fills_the_frame_32x64", shape=(2, 32, 64), psf=(32, 64), kw=dict(iterations=3)),
    dict(name="min_taps_30_36x50_psf7x5", shape=(3, 36, 50), psf=(7, 5),
         kw=dict(iterations=3, denoise_coefficients=(4, 2)), min_taps=30),
]
CASE_IDS = [c["name"] for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


def is_soft(c):
    return c["kw"].get("threshold_type", "soft") == "soft"


def call_kw(c):
    return dict(c["kw"], fft=True)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(frames, psf) of a case, from a generator seeded by the case's position; read-only"""
    c = case(name)
    frames = make_frames(*c["shape"], seed=300 + CASE_IDS.index(name))
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
    ref = np.stack([np.asarray(O.richardson_lucy(f.copy(), psf.copy(), **call_kw(c)), np.float64) for f in frames])
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", [n for n in CASE_IDS if is_soft(case(n))])
def test_oracle_of_the_gpu_cases_is_settled(name):
    frames, psf = case_inputs(name)
    assert (frames > 0).all() and abs(float(psf.sum(dtype=np.float64)) - 1) < 1e-6
    ref = case_reference(name)
    assert ref.shape == frames.shape and np.isfinite(ref).all()
    assert (ref > 0).all()
    for i in range(len(frames)):
        ratio = float(ref[i].mean() / frames[i].astype(np.float64).mean())
        assert 0.5 < ratio < 2.0, (i, ratio)


def test_every_gpu_case_takes_the_fft_route_and_not_the_direct_one(monkeypatch):
    W, B, U, L = _mods()
    for c in CASES:
        frames, psf = case_inputs(c["name"])
        level = len(c["kw"].get("denoise_coefficients", (5, 2, 1)))
        with monkeypatch.context() as m:
            if c.get("min_taps"):
                m.setattr(U, "_FFT_MIN_TAPS", c["min_taps"])
            assert not B.rl_eligible(frames, psf, level, fft=True), c["name"]
            assert B.rl_fft_eligible(frames, psf, level), c["name"]
        assert frames.shape[2] % 2 == 0
    assert sum(not is_soft(c) for c in CASES) == 1


# ---------------------------------------------------------------------------------------------- rl_fft_eligible
def test_rl_fft_eligible_clause_by_clause(monkeypatch):
    W, B, U, L = _mods()
    fr = np.ones((3, 40, 48), np.float32)
    psf = make_psf(23, 23)                                                   # 529 taps
    assert B.rl_fft_eligible(fr, psf, 3) is True
    assert B.rl_fft_eligible(fr, psf, 2) and B.rl_fft_eligible(fr, psf, 8)
    assert B.rl_fft_eligible(fr, psf.astype(np.float64), 3) and B.rl_fft_eligible(fr, (psf * 1000).astype(np.int32), 3)
    # the clauses shared with rl_eligible, each alone
    assert not B.rl_fft_eligible(fr.astype(np.float64), psf, 3)              # float64 frames
    assert not B.rl_fft_eligible(fr.astype(np.int16), psf, 3)                # integer frames
    assert not B.rl_fft_eligible(fr.astype(">f4"), psf, 3)                   # big-endian
    assert not B.rl_fft_eligible(list(fr), psf, 3)                           # not an (N, H, W) array
    assert not B.rl_fft_eligible(fr, psf, 1) and not B.rl_fft_eligible(fr, psf, 9)
    assert not B.rl_fft_eligible(fr, psf, True)
    assert not B.rl_fft_eligible(fr, psf, 3, uniform_init=True)
    # the PSF
    assert not B.rl_fft_eligible(fr, np.ones(600, np.float32), 3)            # not 2-D
    assert not B.rl_fft_eligible(fr, np.stack([psf, psf]), 3)                # per-frame PSFs
    assert not B.rl_fft_eligible(fr, psf.astype(np.complex64), 3)            # not numeric
    assert not B.rl_fft_eligible(fr, np.zeros((0, 5), np.float32), 3)
    assert not B.rl_fft_eligible(fr, make_psf(22, 23), 3)                    # 506 taps: the direct periodic products
    assert B.rl_fft_eligible(fr, make_psf(16, 32), 3)                        # 512 taps
    assert not B.rl_fft_eligible(fr, make_psf(41, 23), 3)                    # kh > H
    assert B.rl_fft_eligible(fr, make_psf(40, 23), 3)
    assert not B.rl_fft_eligible(fr, make_psf(23, 49), 3)                    # kw > W
    assert B.rl_fft_eligible(fr, make_psf(23, 48), 3)
    # the frame shape
    assert not B.rl_fft_eligible(np.ones((3, 40, 45), np.float32), psf, 3)   # odd width (45 = 3 * 3 * 5 is a length the FFT takes)
    assert L.batch_fft_ok(40, 45)
    assert not B.rl_fft_eligible(np.ones((3, 56, 48), np.float32), psf, 3)   # 56 = 8 * 7
    assert not B.rl_fft_eligible(np.ones((3, 40, 44), np.float32), psf, 3)   # 44 = 4 * 11
    assert B.rl_fft_eligible(np.ones((3, 45, 48), np.float32), psf, 3)       # odd heights are fine
    # it asks _lib.batch_fft_ok
    asked = []
    with monkeypatch.context() as m:
        m.setattr(L, "batch_fft_ok", lambda H, W_: asked.append((H, W_)) or False)
        assert not B.rl_fft_eligible(fr, psf, 3)
    assert asked == [(40, 48)]
    # a forced extended frame
    with monkeypatch.context() as m:
        m.setattr(U, "_FFT_FORCE_EXTENDED", True)
        assert not B.rl_fft_eligible(fr, psf, 3)
    assert B.rl_fft_eligible(fr, psf, 3)


def test_fft_threshold_is_read_when_called(monkeypatch):
    W, B, U, L = _mods()
    fr = np.ones((3, 40, 48), np.float32)
    assert not B.rl_fft_eligible(fr, make_psf(7, 5), 3)
    monkeypatch.setattr(U, "_FFT_MIN_TAPS", 30)
    assert B.rl_fft_eligible(fr, make_psf(7, 5), 3)                          # 35 taps
    assert B.rl_fft_eligible(fr, make_psf(5, 6), 3)                          # 30 taps
    assert not B.rl_fft_eligible(fr, make_psf(5, 5), 3)                      # 25 taps


def test_rl_eligible_answers_as_before(monkeypatch):
    """what tests/test_rl_stack_cpu.py pins for the same arguments: rl_eligible still means the direct batch"""
    W, B, U, L = _mods()
    fr = np.ones((3, 40, 48), np.float32)
    assert B.rl_eligible(fr, make_psf(23, 23), 3)
    assert not B.rl_eligible(fr, make_psf(23, 23), 3, fft=True)
    assert B.rl_eligible(fr, make_psf(22, 23), 3, fft=True)
    assert not B.rl_eligible(fr, make_psf(41, 3), 3, fft=True) and not B.rl_eligible(fr, make_psf(3, 49), 3, fft=True)
    assert not B.rl_eligible(fr, make_psf(23, 23), 3, uniform_init=True)
    assert not B.rl_eligible(fr.astype(np.float64), make_psf(7, 5), 3)
    monkeypatch.setattr(U, "_FFT_MIN_TAPS", 30)
    assert not B.rl_eligible(fr, make_psf(7, 5), 3, fft=True) and B.rl_eligible(fr, make_psf(5, 5), 3, fft=True)


def test_one_rule_for_the_per_frame_call_and_the_stack():
    """utils.richardson_lucy and batch.rl_fft_eligible take the FFT decision from utils._rl_uses_fft, and the kernel
    image from utils._rl_fft_kernel_image (one copy of each)"""
    W, B, U, L = _mods()
    import inspect
    assert "_rl_uses_fft(" in inspect.getsource(U.richardson_lucy) and "_rl_uses_fft(" in inspect.getsource(B.rl_fft_eligible)
    assert "_rl_fft_kernel_image(" in inspect.getsource(U.richardson_lucy)
    assert "_rl_fft_kernel_image(" in inspect.getsource(B.richardson_lucy_stack)
    assert U._rl_uses_fft(True, 40, 48, 23, 23) and not U._rl_uses_fft(False, 40, 48, 23, 23)
    assert not U._rl_uses_fft(True, 56, 48, 23, 23) and not U._rl_uses_fft(True, 40, 48, 22, 23)
    # the kernel image: ref utils.py:246-250 - the PSF centre at the origin, one row above it for an odd height
    psf = make_psf(5, 3)
    for H in (8, 9):
        k = U._rl_fft_kernel_image(psf, H, 6)
        assert k.shape == (H, 6) and k.dtype == psf.dtype and np.isclose(k.sum(dtype=np.float64), psf.sum(dtype=np.float64))
        pad = np.zeros((H, 6), np.float32)
        pad[H // 2 - 2:H // 2 + 3, 2:5] = psf
        assert np.array_equal(k, np.roll(pad, (H // 2, 3), axis=(0, 1)))
        assert k[-(H % 2), 0] == psf[2, 1]


def test_batch_fft_ok_is_fft_supported():
    W, B, U, L = _mods()
    sides = (1, 2, 3, 4, 5, 7, 30, 45, 48, 56, 60, 121, 125, 4096, 6561, 8000, 8192, 8193, 9000, 16384)
    for a in sides:
        for b in (2, 64, 45, 56, 8192, 16384):
            assert L.batch_fft_ok(a, b) == L.fft_supported(a, b), (a, b)
            assert L.batch_fft_ok(b, a) == L.fft_supported(b, a), (b, a)
    assert L.batch_fft_ok(2, 2) and L.batch_fft_ok(45, 8192) and L.batch_fft_ok(8192, 8192)
    assert not L.batch_fft_ok(56, 64) and not L.batch_fft_ok(64, 16384) and not L.batch_fft_ok(1, 64)
    with pytest.raises(L.WatrooHipError, match="null pointer"):
        L.check(L.load().wt_batch_fft_ok(8, 8, None))


@pytest.mark.parametrize("Wd", [48, 50, 45, 2])
def test_chunks_count_the_two_complex_work_arrays(Wd):
    """the FFT route's extra planes times H * P * 4 hold the direct route's planes and two complex arrays of
    8 * H * W bytes each; W = 48 has P = W, W = 50 and 45 have P > W"""
    W, B, U, L = _mods()
    H = 40
    P = L._batch_pitch(Wd, 4)
    assert (P > Wd) == (Wd in (50, 45, 2))
    for level in (2, 3, 8):
        extra = B._rl_fft_extra_planes(level)
        assert extra == B._rl_extra_planes(level) + 4
        assert (extra - B._rl_extra_planes(level)) * H * P * 4 >= 2 * 8 * H * Wd
        frame = (level + 5 + extra) * H * P * 4
        assert L.batch_chunks(7, H, Wd, level, budget=3 * frame + 8, extra_planes=extra) == [(0, 3), (3, 3), (6, 1)]
        assert L.batch_chunks(7, H, Wd, level, budget=3 * frame - 8, extra_planes=extra)[0] == (0, 2)


# ---------------------------------------------------------------------------------------------- routing
class _Recorder:
    """a BatchPlan without a device: records the calls of the stack route"""

    def __init__(self, n, H, W_):
        self.n, self.H, self.W, self.calls = n, H, W_, []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            if name == "abs_median":
                return [np.float32(1.0)] * a[0]
        return call

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def recorders(monkeypatch):
    W, B, U, L = _mods()
    recs, chunk_calls, loop = [], [], []
    real_chunks = L.batch_chunks

    def chunks(*a, **k):
        chunk_calls.append((a, k))
        return real_chunks(*a, **k)

    def per_frame(data, psf, **kw):
        loop.append(kw)
        return np.zeros(np.shape(data), np.float32)
    monkeypatch.setattr(L, "default_context", lambda: None)
    monkeypatch.setattr(L, "batch_chunks", chunks)
    monkeypatch.setattr(L, "acquire_batch", lambda ctx, n, H, W_, fam, lv: recs.append(_Recorder(n, H, W_)) or recs[-1])
    monkeypatch.setattr(L, "release_batch", lambda bp: None)
    monkeypatch.setattr(B, "richardson_lucy", per_frame)
    return recs, chunk_calls, loop


def test_an_eligible_stack_issues_one_spectrum_and_two_products_per_iteration_and_chunk(recorders, monkeypatch):
    W, B, U, L = _mods()
    recs, chunk_calls, loop = recorders
    n, H, Wd, level, iterations = 5, 40, 48, 3, 4
    frames = make_frames(n, H, Wd, 5)
    psf = make_psf(23, 23)
    frame = L.batch_frame_bytes(H, Wd, level) + B._rl_fft_extra_planes(level) * H * Wd * 4
    monkeypatch.setattr(L, "BATCH_BYTES", 2 * frame + 8)                     # chunks of 2, 2 and 1
    out = np.empty((n, H, Wd), np.float32)
    assert B.richardson_lucy_stack(frames, psf, iterations=iterations, fft=True, out=out) is out
    assert not loop
    (a, k), = chunk_calls
    assert a == (n, H, Wd, level) and k == {"extra_planes": B._rl_fft_extra_planes(level)}
    rec, = recs
    assert rec.n == 2
    names = rec.names()
    assert names.count("fft_spectrum") == 1 and names.count("fft_apply") == 3 * 2 * iterations
    assert "filter2d" not in names and "set_psf" not in names
    DATA, PSI, PHI, RES, CONV = (L.PLANE_SCRATCH(i) for i in (6, 7, 8, 9, 10))
    # the spectrum: the rolled padded PSF into frame 0 of CONV, before the first chunk's frames
    ups = [c for c in rec.calls if c[0] == "upload"]
    assert ups[0][1][0] == CONV and ups[0][1][1].shape == (1, H, Wd) and ups[0][1][1].dtype == np.float32
    assert np.array_equal(ups[0][1][1][0], U._rl_fft_kernel_image(psf, H, Wd))
    assert names.index("fft_spectrum") == 1 and rec.calls[1][1] == (CONV,)
    assert [c[1][1].shape[0] for c in ups[1:]] == [2, 2, 1] and all(c[1][0] == DATA for c in ups[1:])
    applies = [c[1] for c in rec.calls if c[0] == "fft_apply"]
    for i, nf in enumerate((2, 2, 1)):
        chunk = applies[i * 2 * iterations:(i + 1) * 2 * iterations]
        assert chunk == [(nf, PSI, PHI, False), (nf, RES, CONV, True)] * iterations
    assert [c[1][:2] for c in rec.calls if c[0] == "download"] == [(PSI, 2), (PSI, 2), (PSI, 1)]


def test_a_small_psf_keeps_the_direct_route(recorders):
    W, B, U, L = _mods()
    recs, chunk_calls, loop = recorders
    B.richardson_lucy_stack(make_frames(3, 40, 48, 5), make_psf(7, 5), iterations=2, fft=True)
    assert not loop and chunk_calls[0][1] == {"extra_planes": B._rl_extra_planes(3)}
    names = recs[0].names()
    assert names.count("filter2d") == 4 and names.count("set_psf") == 2
    assert "fft_apply" not in names and "fft_spectrum" not in names


@pytest.mark.parametrize("why", ["56_rows", "fft_false_banded", "float64", "uniform_init", "forced_extended"])
def test_an_ineligible_stack_goes_to_the_per_frame_function(why, recorders, monkeypatch):
    W, B, U, L = _mods()
    recs, chunk_calls, loop = recorders
    frames, psf, kw = make_frames(3, 40, 48, 5), make_psf(23, 23), dict(iterations=2, fft=True)
    if why == "56_rows":
        frames = make_frames(3, 56, 48, 5)
    elif why == "fft_false_banded":
        psf, kw = make_psf(65, 65), dict(iterations=2, fft=False)
    elif why == "float64":
        frames = frames.astype(np.float64)
    elif why == "uniform_init":
        kw["uniform_init"] = True
    else:
        monkeypatch.setattr(U, "_FFT_FORCE_EXTENDED", True)
    got = B.richardson_lucy_stack(frames, psf, **kw)
    assert got.shape == frames.shape and len(loop) == 3 and not recs and not chunk_calls
    assert all(k["fft"] == kw["fft"] and k["iterations"] == 2 for k in loop)


def test_exports_and_bindings():
    W, B, U, L = _mods()
    assert "rl_fft_eligible" in B.__all__
    for name in ("wt_batch_fft_ok", "wt_batch_fft_spectrum", "wt_batch_fft_apply"):
        assert name in L.SIGNATURES and hasattr(L.load(), name)
    assert callable(L.BatchPlan.fft_spectrum) and callable(L.BatchPlan.fft_apply)
