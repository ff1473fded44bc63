"""richardson_lucy_stack without a GPU: the routing predicate rl_eligible clause by clause, the per-frame loop of the
stacks the batch does not take (caller's keywords, out=), the loud failure of an eligible stack without a device, the
argument errors raised before any device work - and the cases of tests/test_gpu_rl_stack.py with their float64 numpy
oracle (oracle.atrous_numpy.richardson_lucy per frame), settled here: finite, and positive where the data are.

Frames are positive - uniform(0.5, 1.5) plus a Gaussian ridge - and neighbouring frames are scaled by 1e-3, 1 and
1e4, so a row or a tap read from the wrong frame is an error of order one.  PSFs are asymmetric, normalised and have
no zero tap, so the flipped and the unflipped operand differ."""
import functools

import numpy as np
import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


def _mods():
    import wavelets_amd as W
    from wavelets_amd import batch as B, utils as U, _lib as L
    return W, B, U, L


SCALES = (1e-3, 1.0, 1e4)


def make_frames(n, H, W, seed):
    rng = np.random.default_rng(seed)
    ridge = 4 * np.exp(-((np.arange(W) - 0.45 * W) ** 2) / (2 * (0.08 * W + 1) ** 2))[None, :]
    frames = [(rng.uniform(0.5, 1.5, (H, W)) + ridge) * SCALES[i % 3] for i in range(n)]
    return np.stack(frames).astype(np.float32)


def make_psf(kh, kw):
    """asymmetric, normalised, no zero tap"""
    wy = np.hanning(kh + 2)[1:-1] if kh > 1 else np.ones(1)
    wx = np.hanning(kw + 2)[1:-1] if kw > 1 else np.ones(1)
    tilt = 1 + 0.3 * np.linspace(-1, 1, kh)[:, None] + 0.2 * np.linspace(-1, 1, kw)[None, :]
    psf = (np.outer(wy, wx) + 0.05) * tilt
    psf = (psf / psf.sum()).astype(np.float32)
    assert (psf > 0).all() and not np.array_equal(psf, psf[::-1, ::-1])
    return psf


# name, frames (n, H, W), PSF (kh, kw), keywords of the call, frames per chunk (0: one chunk)
CASES = [
    dict(name="ragged_37x50_psf7x5", shape=(3, 37, 50), psf=(7, 5), kw=dict(iterations=3)),
    dict(name="one_tile_16x64_psf3x3", shape=(5, 16, 64), psf=(3, 3), kw=dict(iterations=3)),
    dict(name="tiles_96x130_psf1x9", shape=(2, 96, 130), psf=(1, 9), kw=dict(iterations=3)),
    dict(name="tiles_96x130_psf9x1", shape=(2, 96, 130), psf=(9, 1), kw=dict(iterations=3)),
    dict(name="even_20x24_psf6x4", shape=(3, 20, 24), psf=(6, 4), kw=dict(iterations=3)),
    dict(name="reach_12x16_psf15x15", shape=(3, 12, 16), psf=(15, 15), kw=dict(iterations=3)),
    dict(name="chunks_of_2", shape=(5, 37, 50), psf=(7, 5), kw=dict(iterations=3), chunk=2),
    dict(name="fft_odd_height", shape=(3, 37, 50), psf=(7, 5), kw=dict(iterations=3, fft=True)),
    dict(name="fft_even_height", shape=(3, 36, 50), psf=(7, 5), kw=dict(iterations=3, fft=True)),
    dict(name="fft_odd_height_one_row_psf", shape=(3, 37, 50), psf=(1, 9), kw=dict(iterations=3, fft=True)),
    dict(name="hard_persistent", shape=(3, 37, 50), psf=(7, 5),
         kw=dict(iterations=3, threshold_type="hard", persistent_mrs=True)),
    dict(name="hard_fresh_support", shape=(3, 37, 50), psf=(7, 5),
         kw=dict(iterations=3, threshold_type="hard", persistent_mrs=False)),
    dict(name="soft_fresh_support", shape=(3, 37, 50), psf=(7, 5), kw=dict(iterations=3, persistent_mrs=False)),
    dict(name="iterations_0", shape=(3, 37, 50), psf=(7, 5), kw=dict(iterations=0)),
    dict(name="default_iterations", shape=(3, 20, 24), psf=(3, 3), kw=dict()),
    dict(name="two_scales", shape=(3, 37, 50), psf=(7, 5), kw=dict(iterations=3, denoise_coefficients=(4, 2))),
    dict(name="eight_scales", shape=(3, 37, 50), psf=(7, 5),
         kw=dict(iterations=3, denoise_coefficients=(5, 4, 3, 2, 1, 1, 1, 1))),
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
    frames = make_frames(*c["shape"], seed=100 + CASE_IDS.index(name))
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
    ref = np.stack([np.asarray(O.richardson_lucy(f.copy(), psf.copy(), **c["kw"]), np.float64) for f in frames])
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", [n for n in CASE_IDS if is_soft(case(n))])
def test_oracle_of_the_gpu_cases_is_settled(name):
    frames, psf = case_inputs(name)
    assert (frames > 0).all() and abs(float(psf.sum(dtype=np.float64)) - 1) < 1e-6
    ref = case_reference(name)
    assert ref.shape == frames.shape and np.isfinite(ref).all()
    assert (ref > 0).all()
    # the frames are nine decades apart and so are their estimates: a mixed-up frame is an error of order one
    for i in range(len(frames)):
        ratio = float(ref[i].mean() / frames[i].astype(np.float64).mean())
        assert 0.5 < ratio < 2.0, (i, ratio)


def test_every_gpu_case_is_eligible_and_the_hard_ones_have_no_oracle_claim():
    W, B, U, L = _mods()
    for c in CASES:
        frames, psf = case_inputs(c["name"])
        level = len(c["kw"].get("denoise_coefficients", (5, 2, 1)))
        assert B.rl_eligible(frames, psf, level, fft=c["kw"].get("fft", False)), c["name"]
    assert sum(not is_soft(c) for c in CASES) == 2


# ---------------------------------------------------------------------------------------------- rl_eligible
def test_rl_eligible_clause_by_clause():
    W, B, U, L = _mods()
    fr = np.ones((3, 40, 48), np.float32)
    psf = make_psf(7, 5)
    assert B.rl_eligible(fr, psf, 3)
    assert B.rl_eligible(fr, psf, 2) and B.rl_eligible(fr, psf, 8)
    assert B.rl_eligible(fr, psf, 3, fft=True)
    # each clause alone
    assert not B.rl_eligible(fr.astype(np.float64), psf, 3)                 # float64 frames: the per-frame float64 engine
    assert not B.rl_eligible(fr.astype(">f4"), psf, 3)                      # big-endian
    assert not B.rl_eligible(list(fr), psf, 3)                              # not an (N, H, W) array
    assert not B.rl_eligible(fr, psf, 1) and not B.rl_eligible(fr, psf, 9)  # levels without an all-fused schedule
    assert not B.rl_eligible(fr, psf, True)
    assert not B.rl_eligible(fr, psf, 3, uniform_init=True)
    assert not B.rl_eligible(fr, make_psf(65, 65), 3)                       # beyond 4096 taps: bands
    assert B.rl_eligible(fr, make_psf(64, 64), 3)                           # 4096 taps: one launch
    assert not B.rl_eligible(fr, make_psf(1, 600), 3)                       # rows beyond 512 taps: bands
    assert not B.rl_eligible(fr, make_psf(370, 1), 3)                       # 64 x 385 x 4 bytes: beyond the 96 KB tile
    assert B.rl_eligible(fr, make_psf(369, 1), 3)
    assert not B.rl_eligible(fr, np.ones(5, np.float32), 3)                 # not 2-D
    assert B.rl_eligible(fr, make_psf(23, 23), 3)
    assert not B.rl_eligible(fr, make_psf(23, 23), 3, fft=True)             # 529 taps: the per-frame call takes an FFT
    assert B.rl_eligible(fr, make_psf(22, 23), 3, fft=True)                 # 506 taps: direct periodic products
    assert not B.rl_eligible(fr, make_psf(41, 3), 3, fft=True)              # kh > H
    assert not B.rl_eligible(fr, make_psf(3, 49), 3, fft=True)              # kw > W
    assert B.rl_eligible(fr, make_psf(41, 3), 3)


def test_rl_eligible_counts_the_zero_row_of_the_periodic_operand():
    """fft=True on an odd height anchors the operands one row off; a one-row PSF then grows by a zero row
    (utils._periodic_operand), and it is the grown operand the per-frame call applies"""
    W, B, U, L = _mods()
    assert B.rl_eligible(np.ones((2, 37, 50), np.float32), make_psf(1, 9), 3, fft=True)
    (fk, _), (bk, _) = U._rl_direct_operands(make_psf(1, 9), 37, True)
    assert fk.shape == (2, 9) and bk.shape == (2, 9)
    assert not fk[0].any() and not bk[1].any()


def test_fft_threshold_is_read_when_called(monkeypatch):
    W, B, U, L = _mods()
    fr = np.ones((2, 40, 48), np.float32)
    monkeypatch.setattr(U, "_FFT_MIN_TAPS", 30)
    assert not B.rl_eligible(fr, make_psf(7, 5), 3, fft=True)
    assert B.rl_eligible(fr, make_psf(5, 5), 3, fft=True)


def test_batch_psf_ok_is_the_single_launch_rule():
    W, B, U, L = _mods()
    def rule(kh, kw):
        return kh >= 1 and kw >= 1 and kw <= 512 and kh * kw <= 4096 and (64 + kw - 1) * (16 + kh - 1) * 4 <= 96 * 1024
    for kh, kw in ((1, 1), (64, 64), (65, 64), (64, 65), (8, 512), (8, 513), (4096, 1), (1, 4096), (256, 16), (16, 256),
                   (369, 1), (370, 1), (0, 3), (3, 0)):
        assert L.batch_psf_ok(kh, kw) == rule(kh, kw), (kh, kw)


def test_chunks_count_the_planes_of_an_rl_frame():
    W, B, U, L = _mods()
    for level in (2, 3, 8):
        planes = level + 5 + B._rl_extra_planes(level)
        assert planes == 2 * level + 9
        H, Wd = 64, 100
        budget = 3 * planes * H * 100 * 4 + 8
        assert L.batch_chunks(7, H, Wd, level, budget=budget, extra_planes=B._rl_extra_planes(level)) == [(0, 3), (3, 3), (6, 1)]


# ---------------------------------------------------------------------------------------------- the per-frame loop
class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, data, psf, **kw):
        self.calls.append((data, psf, kw))
        return np.full(np.shape(data), float(len(self.calls)), np.float32)


@pytest.mark.parametrize("why", ["float64", "uniform_init", "level_1", "banded_psf", "list_of_mixed_types"])
def test_ineligible_stacks_loop_over_the_frames_with_the_callers_keywords(why, monkeypatch):
    W, B, U, L = _mods()
    rec = _Recorder()
    monkeypatch.setattr(B, "richardson_lucy", rec)
    monkeypatch.setattr(L, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    frames = make_frames(3, 12, 16, 7)
    psf = make_psf(3, 3)
    kw = dict(iterations=4, denoise_coefficients=(3, 1), threshold_type="hard", uniform_init=False, persistent_mrs=False,
              fft=False)
    if why == "float64":
        frames = frames.astype(np.float64)
    elif why == "uniform_init":
        kw["uniform_init"] = True
    elif why == "level_1":
        kw["denoise_coefficients"] = (3,)
    elif why == "banded_psf":
        psf = make_psf(65, 65)
    else:
        frames = [frames[0], frames[1].astype(np.float64), frames[2]]
    got = B.richardson_lucy_stack(frames, psf, **kw)
    assert len(rec.calls) == 3
    for i, (d, p, k) in enumerate(rec.calls):
        assert np.array_equal(d, frames[i]) and p is psf and k == kw
    assert got.shape == (3, 12, 16) and [float(got[i, 0, 0]) for i in range(3)] == [1.0, 2.0, 3.0]
    out = np.zeros((3, 12, 16), np.float64)
    assert B.richardson_lucy_stack(frames, psf, out=out, **kw) is out
    assert [float(out[i, 0, 0]) for i in range(3)] == [4.0, 5.0, 6.0]


def test_eligible_stack_without_a_gpu_fails_loudly_instead_of_looping(monkeypatch):
    W, B, U, L = _mods()
    if L.device_count() > 0:
        pytest.skip("a GPU is visible")
    rec = _Recorder()
    monkeypatch.setattr(B, "richardson_lucy", rec)
    with pytest.raises(L.WatrooHipError, match="no CPU fallback"):
        W.richardson_lucy_stack(make_frames(2, 12, 16, 3), make_psf(3, 3))
    assert not rec.calls


def test_argument_errors_come_before_any_device_work(monkeypatch):
    W, B, U, L = _mods()
    monkeypatch.setattr(L, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    monkeypatch.setattr(B, "richardson_lucy", lambda *a, **k: (_ for _ in ()).throw(AssertionError("per-frame call")))
    frames = make_frames(2, 12, 16, 3)
    for bad in (np.ones(5, np.float32), np.ones((2, 3, 3), np.float32), 1.0):
        with pytest.raises(ValueError, match="psf must be 2-D"):
            B.richardson_lucy_stack(frames, bad)
    with pytest.raises(ValueError, match="even image width"):
        B.richardson_lucy_stack(make_frames(2, 12, 15, 3), make_psf(3, 3), fft=True)
    with pytest.raises(ValueError, match="even image width"):                      # ineligible stacks too
        B.richardson_lucy_stack(make_frames(2, 12, 15, 3).astype(np.float64), make_psf(3, 3), fft=True)
    with pytest.raises(ValueError, match="out: float32 array of shape"):
        B.richardson_lucy_stack(frames, make_psf(3, 3), out=np.zeros((2, 12, 16), np.float64))
    with pytest.raises(ValueError):
        B.richardson_lucy_stack(np.ones((0, 4, 4), np.float32), make_psf(3, 3))


def test_the_operand_rule_is_the_per_frame_calls_own():
    """utils.richardson_lucy takes its direct operands from utils._rl_direct_operands, which the stack function calls
    too (one copy of the rule): symmetric border - the flipped PSF, then the PSF, anchor at the centre; periodic -
    anchors k - 1 - k // 2 and k // 2, one row off on odd heights"""
    W, B, U, L = _mods()
    import inspect
    assert "_rl_direct_operands(" in inspect.getsource(U.richardson_lucy)
    assert "_rl_check_fft_width(" in inspect.getsource(U.richardson_lucy)
    psf = make_psf(6, 4)
    (fk, fkw), (bk, bkw) = U._rl_direct_operands(psf, 20, False)
    assert np.array_equal(fk, psf[::-1, ::-1]) and fk.flags.c_contiguous and bk is psf and fkw == {} and bkw == {}
    (fk, fkw), (bk, bkw) = U._rl_direct_operands(psf, 20, True)
    assert fkw == dict(anchor=(2, 1), periodic=True) and bkw == dict(anchor=(3, 2), periodic=True)
    (fk, fkw), (bk, bkw) = U._rl_direct_operands(psf, 21, True)
    assert fkw == dict(anchor=(1, 1), periodic=True) and bkw == dict(anchor=(4, 2), periodic=True)


def test_exports():
    W, B, U, L = _mods()
    assert W.richardson_lucy_stack is B.richardson_lucy_stack
    assert "richardson_lucy_stack" in B.__all__ and "rl_eligible" in B.__all__
