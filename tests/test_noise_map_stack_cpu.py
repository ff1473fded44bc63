"""Host logic of the stacks whose noise is a per-pixel map (denoise_stack / wow_stack behind the batch's noise plane;
no GPU: recorders stand in for the batch plans):

* the map threshold rule (watroo/wavelets.py:129-143 with an ndarray noise) - wavelets._map_tau against a transcription
  written out here, and Coefficients._tau calling it;
* which `noise` arguments _noise_list and the eligibility predicates take as maps, and that every call form the
  predicates had before answers as before;
* the noise plane in the chunk budget and the calls that fill it (a shared map: one upload, replicated on the device);
* the inputs of tests/test_gpu_noise_map_stack.py, and the numpy oracle's result for one small frame with a map, which
  the GPU module holds the per-frame call against."""
import ctypes
import os
import re

import numpy as np
import pytest

import wavelets_amd as W
from oracle import atrous_numpy as O
from wavelets_amd import _lib as L
from wavelets_amd import batch as B
from wavelets_amd import wavelets as WV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- inputs shared with the GPU module
# the smallest shapes that exercise the index arithmetic: W % 4 != 0 (pitch padding of the noise plane), H = 1
# (float32 only), H = 2 (the smallest the float64 batch takes), and more than one 256-thread block per frame with the
# frame boundary inside a block (33 x 132 floats / 4 = 1089 float4 groups per frame)
SHAPE_ODD, N_ODD = (5, 7), 3
SHAPE_ROW, N_ROW = (1, 9), 2
SHAPE_F64, N_F64 = (2, 6), 3
SHAPE_BLOCKS, N_BLOCKS = (33, 130), 5
MIXED = ("map", 2.5, None, "map", 0)          # the mixed list of the 5-frame stack


def frames_of(shape, n, dtype=np.float32, seed=0, positive=False):
    rng = np.random.default_rng(1000 * seed + shape[0] * shape[1] + n)
    fr = rng.standard_normal((n,) + shape) * 3 + (40 if positive else 1)
    if np.dtype(dtype).kind in "iu":
        return np.round(fr * 50).astype(dtype)
    return fr.astype(dtype)


def noise_map(shape, seed=0):
    """positive random values, a few exact zeros and one large value (1e6); float64, as a calibration would give it"""
    rng = np.random.default_rng(77 + seed)
    m = rng.uniform(0.2, 3.0, shape)
    flat = m.reshape(-1)
    flat[:: max(2, flat.size // 3)] = 0.0
    flat[flat.size // 2] = 1e6
    return m


def noise_arg(kind, shape, n):
    """the `noise` argument of a stacked call and the per-frame list it stands for"""
    if kind == "shared":
        m = noise_map(shape)
        return m, [m] * n
    if kind == "per_frame":
        per = [noise_map(shape, i + 1) for i in range(n)]
        return per, per
    assert kind == "mixed"
    per = [noise_map(shape, i + 1) if v == "map" else v for i, v in zip(range(n), MIXED)]
    return per, per


# the oracle case: one small frame, a strictly positive map (the reference divides by sigma * map * sigma_e)
ORACLE_SHAPE, ORACLE_WEIGHTS = (12, 10), [4, 2]


def oracle_case():
    rng = np.random.default_rng(5)
    frame = (rng.standard_normal(ORACLE_SHAPE) * 2 + 10).astype(np.float32)
    nmap = rng.uniform(0.5, 2.0, ORACLE_SHAPE).astype(np.float32)
    return frame, nmap


def test_the_oracle_denoises_one_frame_with_a_map():
    frame, nmap = oracle_case()
    for fam in ("b3spline", "triangle"):
        for soft in (True, False):
            ref = O.denoise(frame.copy(), ORACLE_WEIGHTS, fam, noise=nmap, soft_threshold=soft)
            assert ref.shape == ORACLE_SHAPE and np.isfinite(ref).all()
            # the map matters: a constant level of the map's mean gives another image
            flat = O.denoise(frame.copy(), ORACLE_WEIGHTS, fam, noise=float(nmap.mean()), soft_threshold=soft)
            assert np.abs(ref - flat).max() > 1e-3
            # ... and the transcription of ref:137-141 on the oracle's own planes gives the oracle's image
            planes = O.atrous_standard(frame, 2, fam)
            sigma_e = O.SIGMA_E_2D[fam]
            acc = planes[2].astype(np.float64)
            for s, sig in enumerate(ORACLE_WEIGHTS):
                t = sig * nmap * sigma_e[s]
                from scipy.special import erf
                sg = erf(np.abs(planes[s] / t)) if soft else (np.abs(planes[s]) > t)
                acc = acc + planes[s] * sg
            assert np.abs(acc - ref).max() <= 1e-5 * np.abs(frame).max()


# ---------------------------------------------------------------- the threshold rule
SIGMAS = [0, 5, 3, -2, 1.5, np.float32(2)]


def reference_map_tau(sigma, sigma_e_scale, soft):
    """watroo/wavelets.py:129-143 with an ndarray noise, as the factor t the kernels apply to the map - erf(|w| / (t *
    map)) (soft) or |w| > t * map (hard) - with None standing for a significance of one everywhere"""
    if sigma == 0:                                               # :142-143
        return None
    t = float(sigma * sigma_e_scale)
    if t < 0 and not soft:                                       # |w| > t * map holds everywhere for t < 0 (map >= 0)
        return None
    return abs(t)                                                # erf(|w / (t * map)|) = erf(|w| / (|t| * map))


class _PlanStub:
    shape = (4, 6)

    def __init__(self):
        self.uploads = []

    def upload(self, plane, host):
        self.uploads.append((plane, np.array(host)))


def _coefficients_with_map(family, nmap):
    c = WV.Coefficients(np.zeros((3, 4, 6), np.float32), family(2))
    c._plan = _PlanStub()
    c.noise = nmap
    return c


@pytest.mark.parametrize("soft", [True, False])
@pytest.mark.parametrize("family", [W.B3spline, W.Triangle])
def test_map_tau_is_the_map_branch_of_coefficients_tau(family, soft):
    sigma_e = family(2).sigma_e()
    nmap = np.full((4, 6), 2.0)
    seen = set()
    for scale in range(4):
        for sigma in SIGMAS:
            want = reference_map_tau(sigma, sigma_e[scale], soft)
            got = WV._map_tau(sigma, sigma_e[scale], soft)
            c = _coefficients_with_map(family, nmap)
            via = c._tau(sigma, scale, soft)
            if want is None:
                assert got is None and via is None
                seen.add("one")
                continue
            assert got == (want, WV._NOISE_PLANE) and type(got[0]) is float and via == got
            seen.add("neg" if sigma < 0 else "pos")
            # the map went up as float32, on the noise plane
            (plane, host), = c._plan.uploads
            assert plane == WV._NOISE_PLANE and host.dtype == np.float32 and np.array_equal(host, nmap)
    assert seen == ({"one", "pos", "neg"} if soft else {"one", "pos"})
    assert WV._map_tau_row([(0, 5, 1), (1, 0, 1), (2, -2, 1)], sigma_e, soft) == \
        [5 * sigma_e[0], 0.0, 2 * sigma_e[2] if soft else 0.0]


def test_coefficients_tau_calls_the_one_rule(monkeypatch):
    c = _coefficients_with_map(W.B3spline, np.ones((4, 6)))
    monkeypatch.setattr(WV, "_map_tau", lambda sigma, se, soft=True: ("patched", sigma, se, soft))
    assert c._tau(3, 1, False) == ("patched", 3, W.B3spline(2).sigma_e()[1], False)
    c.noise = 0.5                                                 # a scalar level: not the map rule
    assert c._tau(3, 1, True) == WV._scalar_tau(3, 0.5, W.B3spline(2).sigma_e()[1], True)


# ---------------------------------------------------------------- _noise_list and the predicates
F32 = np.zeros((3, 64, 80), np.float32)
F64 = np.zeros((3, 64, 80))
I16 = np.zeros((3, 64, 80), np.int16)
MAP = np.ones((64, 80))


def test_noise_list_takes_frame_shaped_maps_only():
    shared = B._noise_list(MAP, 3, (64, 80))
    assert len(shared) == 3 and all(n is MAP for n in shared)
    per = [MAP.copy(), MAP.copy(), MAP.copy()]
    assert all(a is b for a, b in zip(B._noise_list(per, 3, (64, 80)), per))
    mixed = [MAP, 2.5, None]
    got = B._noise_list(mixed, 3, (64, 80))
    assert got[0] is MAP and got[1:] == [2.5, None]
    # not taken: the old answer
    assert B._noise_list(np.ones((1, 80)), 3, (64, 80)) is None
    assert B._noise_list(np.ones((3, 64, 80)), 3, (64, 80)) is None
    assert B._noise_list(MAP, 3, (64, 81)) is None
    z = np.array(2.0)
    assert all(n is z for n in B._noise_list(z, 3, (64, 80)))      # a 0-d array: repeated, as before
    # the call form without a shape is the old function
    assert B._noise_list(MAP, 3) is None and B._noise_list(None, 2) == [None, None]
    assert B._noise_list(0.5, 2) == [0.5, 0.5] and B._noise_list(np.array([0.5, 2.0]), 2) == [0.5, 2.0]
    with pytest.raises(ValueError, match="one entry per frame"):
        B._noise_list([MAP, MAP], 3, (64, 80))


def test_is_noise_map():
    assert B._is_noise_map(MAP, (64, 80)) and B._is_noise_map(MAP.astype(np.float32), (64, 80))
    assert B._is_noise_map(np.ones((64, 80), np.int32), (64, 80))
    assert not B._is_noise_map(np.ones((1, 80)), (64, 80)) and not B._is_noise_map(np.array(2.0), (64, 80))
    assert not B._is_noise_map(np.ones((3, 64, 80)), (64, 80))
    assert not B._is_noise_map(MAP.astype(complex), (64, 80)) and not B._is_noise_map(MAP.astype(object), (64, 80))
    assert not B._is_noise_map(MAP.tolist(), (64, 80)) and not B._is_noise_map(2.0, (64, 80))


TAKEN = ([MAP] * 3, [MAP.copy(), MAP.copy(), MAP.copy()], [MAP, 2.5, None], [None, MAP.astype(np.float32), 0])
NOT_TAKEN = ([np.ones((1, 80))] * 3, [np.ones((3, 64, 80))] * 3, [np.array(2.0)] * 3, [MAP.astype(complex)] * 3,
             [MAP.astype(object), 1.0, 1.0], [MAP[:, :79], 1.0, 1.0])


def test_the_predicates_take_maps_on_request():
    for per in TAKEN:
        assert B.noise_map_eligible(F32, per) and B.noise_map_eligible(F64, per)
        assert B.batch_eligible(F32, 6, noise_per_frame=per, noise_maps=True)
        assert B.wow_eligible(F32, 4, noise_per_frame=per, noise_maps=True)
        assert B.bilateral_eligible(F32, 4, bilateral=1, noise_per_frame=per, noise_maps=True)
        for fr in (F64, I16, F64.astype(">f8"), F32.astype(">f4")):
            assert B.batch64_eligible(fr, 5, noise_per_frame=per, noise_maps=True)
            assert B.bilateral64_eligible(fr, 3, bilateral=1, noise_per_frame=per, noise_maps=True)
        # ... and only there: the other conditions hold as they did
        assert not B.batch_eligible(F32, 9, noise_per_frame=per, noise_maps=True)
        assert not B.batch_eligible(F64, 6, noise_per_frame=per, noise_maps=True)
        assert not B.wow_eligible(F64, 4, noise_per_frame=per, noise_maps=True)          # float64 wow: the loop
        assert not B.wow_eligible(I16, 4, noise_per_frame=per, noise_maps=True)
        assert not B.batch64_eligible(F32, 5, noise_per_frame=per, noise_maps=True)
        assert not B.batch_eligible(F32, 6, bilateral=1, noise_per_frame=per, noise_maps=True)
    for per in NOT_TAKEN:
        assert not B.noise_map_eligible(F32, per) and not B.noise_map_eligible(F64, per)
        zero_d = per[0].ndim == 0              # (batch_eligible / batch64_eligible take a 0-d array as a level, as before)
        for name, args, kw in (("batch_eligible", (F32, 6), {}), ("wow_eligible", (F32, 4), {}),
                               ("bilateral_eligible", (F32, 4), {"bilateral": 1}), ("batch64_eligible", (F64, 5), {}),
                               ("bilateral64_eligible", (F64, 3), {"bilateral": 1})):
            old = getattr(B, name)(*args, noise_per_frame=per, **kw)
            assert getattr(B, name)(*args, noise_per_frame=per, noise_maps=True, **kw) is old, (name, per[0].shape)
            assert old is (zero_d and name in ("batch_eligible", "batch64_eligible")), (name, per[0].shape)
    assert not B.noise_map_eligible(F32, None) and not B.noise_map_eligible(F32, [None, 0.5, 2])
    assert not B.noise_map_eligible([F32[0], F32[1]], [MAP, MAP]) and not B.noise_map_eligible(F32, ())


class Retapped(W.B3spline):
    coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9


# (predicate, positional arguments, keywords, answer) of the call forms the predicates had before noise_maps= existed:
# the cases of tests/test_batch_cpu.py, test_wow_stack_cpu.py, test_bilateral_stack_cpu.py, test_batch64_cpu.py and
# test_bilateral64_stack_cpu.py, answers as those files state them
PINNED = [
    ("batch_eligible", (F32, 6), {}, True),
    ("batch_eligible", (F32, 2, W.Triangle), {}, True),
    ("batch_eligible", (F32, 8, W.Triangle), {}, True),
    ("batch_eligible", (F64, 6), {}, False),
    ("batch_eligible", (F32.astype(">f4"), 6), {}, False),
    ("batch_eligible", (F32, 1), {}, False),
    ("batch_eligible", (F32, 9), {}, False),
    ("batch_eligible", (F32, 6), {"bilateral": 1}, False),
    ("batch_eligible", (F32, 6), {"noise_per_frame": None}, False),
    ("batch_eligible", (F32, 6), {"noise_per_frame": [MAP] * 3}, False),
    ("batch_eligible", (F32, 6), {"noise_per_frame": [None, 0.5, np.float32(2)]}, True),
    ("batch_eligible", ([F32[0], F32[1]], 6), {}, False),
    ("batch_eligible", (F32, 6, Retapped), {}, False),
    ("wow_eligible", (F32, 4), {}, True),
    ("wow_eligible", (F32, 1), {}, True),
    ("wow_eligible", (F32, 10), {}, True),
    ("wow_eligible", (F32, 25), {}, False),
    ("wow_eligible", (F32, 4), {"noise_per_frame": None}, False),
    ("wow_eligible", (F32, 4), {"noise_per_frame": [MAP] * 3}, False),
    ("wow_eligible", (F32, 4), {"noise_per_frame": [np.array(2.0)] * 3}, False),
    ("wow_eligible", (F32, 4), {"noise_per_frame": [None, 0.0, np.float32(2)]}, True),
    ("bilateral_eligible", (F32, 4), {}, False),
    ("bilateral_eligible", (F32, 4, W.B3spline, 1), {}, True),
    ("bilateral_eligible", (F32, 4), {"bilateral": 1, "noise_per_frame": None}, False),
    ("bilateral_eligible", (F32, 4), {"bilateral": 1, "noise_per_frame": [MAP] * 3}, False),
    ("bilateral_eligible", (F32, 4), {"bilateral": 1, "noise_per_frame": [np.array(2.0)] * 3}, False),
    ("bilateral_eligible", (F32, 4), {"bilateral": 1, "noise_per_frame": [None, 0.0, np.float32(2)]}, True),
    ("batch64_eligible", (F64, 6), {}, True),
    ("batch64_eligible", (I16, 5), {"noise_per_frame": [None, 0.5, np.float64(2)]}, True),
    ("batch64_eligible", (F64, 6), {"noise_per_frame": [MAP] * 3}, False),
    ("batch64_eligible", (F32, 6), {}, False),
    ("bilateral64_eligible", (F64, 4), {"bilateral": 1}, True),
    ("bilateral64_eligible", (F64, 4), {"bilateral": 1, "noise_per_frame": [MAP] * 3}, False),
    ("bilateral64_eligible", (F64, 5), {"bilateral": 1, "noise_per_frame": [None, 0.5, np.float64(2)]}, True),
    ("bilateral64_eligible", (F64, 4), {}, False),
]


@pytest.mark.parametrize("name,args,kw,want", PINNED, ids=[f"{i}-{c[0]}" for i, c in enumerate(PINNED)])
def test_every_earlier_call_form_answers_as_before(name, args, kw, want):
    assert getattr(B, name)(*args, **kw) is want
    assert getattr(B, name)(*args, noise_maps=False, **kw) is want
    assert B.enhance_eligible(F32, 3, noise_per_frame=[MAP] * 3) is None      # enhance_stack: maps stay on the loop


# ---------------------------------------------------------------- routes: the noise plane in the budget, its uploads
class _Recorder:
    """a BatchPlan / BatchPlan64 without a device: records the calls of the stack routes"""

    def __init__(self, n, H, W_, dtype):
        self.n, self.H, self.W, self.dtype, self.calls = n, H, W_, dtype, []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            if name == "abs_median":
                return [self.dtype(1.0)] * a[0]
            if name == "reduce":
                return [(1.0, 2.0, 0.0, 1.0)] * a[0]
        return call

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def recorders(monkeypatch):
    recs, chunk_calls = [], []
    real_chunks = L.batch_chunks

    def chunks(*a, **k):
        chunk_calls.append((a, k))
        return real_chunks(*a, **k)

    def boom(*a, **k):
        raise AssertionError("the per-frame loop ran")
    monkeypatch.setattr(L, "default_context", lambda: None)
    monkeypatch.setattr(L, "batch_chunks", chunks)
    monkeypatch.setattr(L, "acquire_batch", lambda ctx, n, H, W_, fam, lv: recs.append(_Recorder(n, H, W_, np.float32)) or recs[-1])
    monkeypatch.setattr(L, "acquire_batch64", lambda ctx, n, H, W_, fam, lv: recs.append(_Recorder(n, H, W_, np.float64)) or recs[-1])
    monkeypatch.setattr(L, "release_batch", lambda bp: None)
    monkeypatch.setattr(L, "release_batch64", lambda bp: None)
    monkeypatch.setattr(B, "AtrousTransform", boom)
    monkeypatch.setattr(B, "denoise", boom)
    monkeypatch.setattr(B, "wow", boom)
    return recs, chunk_calls


def test_denoise_stack_budgets_and_fills_the_noise_plane(recorders, monkeypatch):
    recs, chunk_calls = recorders
    H, Wd, level = 5, 7, 2
    fr = frames_of((H, Wd), 5)
    # room for two frames WITH the noise plane (three without it)
    monkeypatch.setattr(L, "BATCH_BYTES", 2 * (L.batch_frame_bytes(H, Wd, level) + H * 8 * 4) + 8)
    shared = noise_map((H, Wd))
    kept = shared.copy()
    out = np.empty((5, H, Wd), np.float32)
    assert W.denoise_stack(fr, [5, 3], noise=shared, out=out) is out
    (a, k), = chunk_calls
    assert a == (5, H, Wd, level) and k == {"extra_planes": 1}
    calls = recs[-1].calls
    assert recs[-1].n == 2 and recs[-1].names().count("denoise_sum") == 3
    # the shared map: filled, uploaded and replicated once (the first chunk is the largest), ONE map over PCIe
    ups = [c for c in calls if c[0] == "upload" and c[1][0] == WV._NOISE_PLANE]
    assert len(ups) == 1 and ups[0][1][1].shape == (1, H, Wd) and ups[0][1][1].dtype == np.float32
    assert np.array_equal(ups[0][1][1][0], shared.astype(np.float32))
    assert [c[1] for c in calls if c[0] == "fill"] == [(2, WV._NOISE_PLANE, 1.0)]
    assert [c[1] for c in calls if c[0] == "replicate"] == [(2, WV._NOISE_PLANE)]
    assert recs[-1].names().index("fill") < recs[-1].names().index("replicate") < recs[-1].names().index("denoise_sum")
    assert "abs_median" not in recs[-1].names()                                # no MAD estimate for a frame with a map
    sigma_e = W.B3spline(2).sigma_e()
    for c in calls:
        if c[0] == "denoise_sum":
            nf = c[1][0]
            assert c[2] == {"noise_plane": WV._NOISE_PLANE, "has_map": [True] * nf}
            assert c[1][2] == [[5 * sigma_e[0], 3 * sigma_e[1]]] * nf
    assert np.array_equal(shared, kept)

    # a mixed list: per chunk the plane is filled with ones and the runs of maps go up at their frame offsets; the
    # scalar and None frames get their usual rows, the median is taken for the None frame's chunk only
    chunk_calls.clear()
    per, _ = noise_arg("mixed", (H, Wd), 5)
    W.denoise_stack(fr, [5, 3], noise=per, soft_threshold=False)
    assert chunk_calls[0][1] == {"extra_planes": 1}
    calls = recs[-1].calls
    ups = [(c[1][1].shape[0], c[2].get("f0", 0)) for c in calls if c[0] == "upload" and c[1][0] == WV._NOISE_PLANE]
    assert ups == [(1, 0), (1, 1)]                        # chunks [0, 1], [2, 3], [4]: maps at frames 0 and 3
    assert [c[1] for c in calls if c[0] == "fill"] == [(2, WV._NOISE_PLANE, 1.0)] * 2
    assert recs[-1].names().count("abs_median") == 1 and "replicate" not in recs[-1].names()
    sums = [c for c in calls if c[0] == "denoise_sum"]
    assert [c[2].get("has_map") for c in sums] == [[True, False], [False, True], None]
    assert sums[2][2] == {}                               # the last chunk holds no map: the call without a noise plane
    assert sums[0][1][2][1] == WV._tau_row([(0, 5, 1), (1, 3, 1)], 2.5, sigma_e, False)

    # float64 stacks: the float64 batch, float64 maps
    chunk_calls.clear()
    f64 = frames_of((4, 6), 3, np.float64)
    m32 = noise_map((4, 6)).astype(np.float32)
    W.denoise_stack(f64, [5, 3], noise=m32, bilateral=1.5)
    assert chunk_calls[0][1] == {"extra_planes": 1, "itemsize": 8}
    up, = [c for c in recs[-1].calls if c[0] == "upload" and c[1][0] == WV._NOISE_PLANE]
    assert up[1][1].dtype == np.float64 and np.array_equal(up[1][1][0], m32.astype(np.float64))
    assert "decompose_bilateral" in recs[-1].names()

    # without a map nothing changes: no extra plane, no noise-plane call, the old denoise_sum call
    chunk_calls.clear()
    W.denoise_stack(fr, [5, 3], noise=[1.0, None, 2.0, 0, 3])
    assert chunk_calls[0] == ((5, H, Wd, level), {})
    assert not {"fill", "replicate"} & set(recs[-1].names())
    assert all(c[2] == {} and len(c[1]) == 5 for c in recs[-1].calls if c[0] == "denoise_sum")


def test_wow_stack_budgets_the_noise_plane_and_picks_the_map_updates(recorders):
    recs, chunk_calls = recorders
    fr = frames_of(SHAPE_BLOCKS, 3)
    shared = noise_map(SHAPE_BLOCKS)
    W.wow_stack(fr, noise=shared, denoise_coefficients=[5, 2], h=0.5)
    assert chunk_calls[0][1] == {"extra_planes": 3}       # the spare plane, the gamma plane, the noise plane
    calls = recs[-1].calls
    scales = [c for c in calls if c[0] == "wow_scale"]
    sigma_e = W.B3spline(2).sigma_e()
    # scales 0 and 1 have a sigma: the updates that read the map, with the map thresholds; scale 2 (sigma 0) has none
    assert [c[2] for c in scales] == [{"noise_plane": WV._NOISE_PLANE}] * 2 + [{}]
    assert [c[1][3] for c in scales] == [[5 * sigma_e[0]] * 3, [2 * sigma_e[1]] * 3, [0.0] * 3]
    assert [c[0] for c in calls if c[0] in ("fill", "replicate")].count("replicate") == 1
    assert "abs_median" not in recs[-1].names()
    chunk_calls.clear()
    W.wow_stack(fr, noise=shared, whitening=False, denoise_coefficients=[5])
    assert chunk_calls[0][1] == {"extra_planes": 1}
    ups = [c for c in recs[-1].calls if c[0] == "wow_update"]
    assert ups[0][2] == {"noise_plane": WV._NOISE_PLANE} and all(c[2] == {} for c in ups[1:])
    chunk_calls.clear()
    W.wow_stack(fr, noise=[1.0, 2.0, 3.0])
    assert chunk_calls[0][1] == {"extra_planes": 1} and all(c[2] == {} for c in recs[-1].calls if c[0] == "wow_scale")


def test_float64_wow_with_a_map_stays_on_the_loop(monkeypatch):
    seen = []
    monkeypatch.setattr(B, "wow", lambda f, *a, **k: seen.append(k["noise"]) or (f * 2, type("C", (), {"data": f[None]})()))
    m = noise_map((16, 16))
    img = B.wow_stack(np.ones((2, 16, 16)), noise=m)
    assert len(seen) == 2 and all(n is m for n in seen) and np.array_equal(img, np.full((2, 16, 16), 2.0))


def test_wow_stack_keeps_small_frames_with_a_map_on_the_loop(monkeypatch):
    """below WOW_MAP_MIN_PIXELS per frame wow_stack hands maps to the per-frame loop, as it always did; at the floor
    and above the batch takes them (test_wow_stack_budgets_the_noise_plane_and_picks_the_map_updates)"""
    seen = []
    monkeypatch.setattr(B, "wow", lambda f, *a, **k: seen.append(k["noise"]) or (f * 2, type("C", (), {"data": f[None]})()))
    assert B.WOW_MAP_MIN_PIXELS == 1024 and SHAPE_BLOCKS[0] * SHAPE_BLOCKS[1] >= B.WOW_MAP_MIN_PIXELS
    m = np.ones((31, 33), np.float32)                      # 1023 pixels
    B.wow_stack(np.ones((2, 31, 33), np.float32), noise=m)
    assert len(seen) == 2 and all(n is m for n in seen)
    B.wow_stack(np.ones((2, 31, 33), np.float32), noise=[m, 2.0])
    assert len(seen) == 4 and seen[2] is m and seen[3] == 2.0


# ---------------------------------------------------------------- the entry points
def test_the_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    raw = open(os.path.join(ROOT, "include", "watroo_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    want = {"wt_batch_denoise_sum_map": 10, "wt_batch_replicate": 3, "wt_batch_wow_update_map": 8,
            "wt_batch_wow_scale_map": 9, "wt_batch64_denoise_sum_map": 11, "wt_batch64_fill": 4, "wt_batch64_replicate": 3}
    for name, nargs in want.items():
        assert hasattr(lib, name), name
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert L.SIGNATURES[name][0] is ctypes.c_int and len(L.SIGNATURES[name][1]) == nargs, name
        comment = raw[:raw.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "watroo/" in comment, name                                     # cites its reference call site
    # the entries they extend keep their signatures
    for name, nargs in (("wt_batch_denoise_sum", 9), ("wt_batch_wow_update", 7), ("wt_batch_wow_scale", 8),
                        ("wt_batch64_denoise_sum", 9), ("wt_batch_upload", 6)):
        assert len(L.SIGNATURES[name][1]) == nargs, name
    assert L.load().wt_abi_version() == 8                                     # additive: the version stays


def test_inputs_are_what_the_gpu_module_claims():
    for shape in (SHAPE_ODD, SHAPE_ROW, SHAPE_F64, SHAPE_BLOCKS):
        m = noise_map(shape)
        assert m.shape == shape and (m >= 0).all() and np.isfinite(m).all()
        assert (m == 0).sum() >= 2 and (m == 1e6).sum() == 1
    assert SHAPE_ODD[1] % 4 and SHAPE_ROW[0] == 1 and SHAPE_F64[0] == 2
    f4 = SHAPE_BLOCKS[0] * ((SHAPE_BLOCKS[1] + 3) // 4 * 4) // 4
    assert f4 > 256 and f4 % 256                                             # several blocks, a frame boundary inside one
    per, lst = noise_arg("mixed", SHAPE_BLOCKS, N_BLOCKS)
    assert [type(n) is np.ndarray for n in lst] == [True, False, False, True, False] and lst[1] == 2.5 and lst[4] == 0
    assert frames_of(SHAPE_ODD, 3, positive=True).min() > 0 and frames_of(SHAPE_ODD, 3, np.int16).dtype == np.int16
