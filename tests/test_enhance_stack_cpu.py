"""enhance_stack without a GPU: the list plumbing shared with utils.enhance against a transcription of the
reference (watroo/utils.py:10-33, 55-68), grouping by level, the routes (enhance_eligible), the noise forms and
refusals, `out` refused before any device work, the fallback loop's arguments, the two new ABI symbols - and the
inputs, cases and oracles of tests/test_gpu_enhance_stack.py with their reference-only premises: at every
hard-threshold sample the float32 and the float64 numpy oracle take the same decision, with |w| at least
HARD_MARGIN (relative) away from the threshold, so that no comparison of the GPU tests has to leave a sample out."""
import copy
import functools

import numpy as np
import pytest

import __graft_entry__ as entry
from oracle import atrous_numpy as O


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


def _mods():
    import wavelets_amd as W
    from wavelets_amd import batch as B, utils as U, _lib as L
    return W, B, U, L


# --------------------------------------------------------------------------------------------- the reference's lists
def ref_prepare_params(param, ndims):
    """watroo/utils.py:10-33, line by line"""
    if ndims == 2:
        if param is None:
            lst = []
        elif type(param) is not list:
            lst = [param]
        else:
            lst = copy.copy(param)
    else:
        if type(param) is not list:
            if param is None:
                lst = [[], ] * ndims
            else:
                lst = [[param], ] * ndims
        else:
            if len(param) != ndims:
                raise ValueError("Invalid number of parameters")
            else:
                lst = []
                for p in param:
                    lst.append(ref_prepare_params(p, 2))
                if None in lst:
                    lst[lst.index(None)] = []
    return lst


def ref_lists(ndim, weights, denoise):
    """watroo/utils.py:47-50, 55-56, 60-68: [(channel, sigmas, weights)], each channel's lists as the reference's
    loop body sees them at ref:70-76 (a copy, taken before the next channel can pad a shared list)"""
    channels = [0, 1, 2] if ndim == 3 else [Ellipsis]
    weights = ref_prepare_params(weights, ndim)
    denoise = ref_prepare_params(denoise, ndim)
    seen = []
    for c in channels:
        dns = denoise if c is Ellipsis else denoise[c]
        wgt = weights if c is Ellipsis else weights[c]
        if len(wgt) < len(dns):
            wgt.extend([1] * (len(dns) - len(wgt)))
        elif len(dns) < len(wgt):
            dns.extend([0] * (len(wgt) - len(dns)))
        seen.append((c, list(dns), list(wgt)))
    return seen


# parameter forms in which no later channel lengthens a shared WEIGHT list: the helper hands out the lists as they
# stand after the loop (what utils.enhance has always run on), the reference reads each channel's as it goes, and
# the two agree on every level and on every sigma up to it
PARAM_FORMS = [
    (2, None, None), (2, 2., None), (2, None, 3), (2, [.5, 2], [5]), (2, [1], [5, 3, 2]), (2, [1, 2], [0, 3]),
    (3, None, None), (3, 2., 3), (3, 2., None), (3, None, [5, 3, 1]),
    (3, [[.5, 2], [1], [2, 2, 1]], None), (3, [[.5, 2], None, [2, 2, 1]], [None, [3], [1, 1, 1, 1]]),
    (3, [1, 2, 3], [[5], [5, 3], [5, 3, 2]]), (3, [[.5, 2, 1], [1, -1.5, 0], [2, 2, 1]], [[5, 3, 0], [0, 5, 2], [3, 0, 0]]),
    (3, 2., [[3, 2], [3], None]),                       # the shared-list quirk: channel 0's padding reaches 1 and 2
]


@pytest.mark.parametrize("ndim,weights,denoise", PARAM_FORMS)
def test_enhance_lists_match_the_reference(ndim, weights, denoise):
    _, _, U, _ = _mods()
    w0, d0 = copy.deepcopy(weights), copy.deepcopy(denoise)
    got = U._enhance_lists(ndim, weights, denoise)
    # (the sigmas up to the level: Coefficients.denoise zips them with the weights, ref wavelets.py:148, so zeros that
    #  a later channel appends to a shared sigma list never reach a plane)
    cut = lambda plans: [(c, list(d)[:len(w)], list(w)) for c, d, w in plans]
    assert cut(got) == cut(ref_lists(ndim, w0, d0))
    assert [len(w) for _, _, w in got] == [len(w) for _, _, w in ref_lists(ndim, w0, d0)]      # the levels
    assert (weights, denoise) == (w0, d0)                # the caller's lists are not touched


def test_enhance_lists_shared_list_quirk():
    _, _, U, _ = _mods()
    got = U._enhance_lists(3, 2., [[3, 2], [3], None])
    assert got == [(0, [3, 2], [2., 1]), (1, [3, 0], [2., 1]), (2, [0, 0], [2., 1])]
    assert got[0][2] is got[1][2] is got[2][2]           # ONE weight list ([[param], ] * ndims, ref:23)
    assert ref_lists(3, 2., [[3, 2], [3], None]) == got


def test_enhance_lists_are_read_after_the_loop():
    """the one form in which utils.enhance (unchanged here) departs from the reference: a scalar weight shared by the
    channels and sigma lists that get LONGER from channel to channel - the shared weight list is read once every
    channel has padded it, so channel 0 runs at the last channel's level (the reference: at its own)"""
    _, _, U, _ = _mods()
    got = U._enhance_lists(3, 2., [[3], [3, 2], None])
    assert [len(w) for _, _, w in got] == [2, 2, 2]
    assert [len(w) for _, _, w in ref_lists(3, 2., [[3], [3, 2], None])] == [1, 2, 2]


def test_enhance_lists_wrong_length():
    _, _, U, _ = _mods()
    for bad in ([1, 2], [[1], [2]], [1, 2, 3, 4]):
        with pytest.raises(ValueError, match="Invalid number of parameters"):
            U._enhance_lists(3, bad, None)
        with pytest.raises(ValueError, match="Invalid number of parameters"):
            ref_lists(3, None, bad)
    assert U._enhance_lists(2, [1, 2], None) == [(Ellipsis, [0, 0], [1, 2])]


# ------------------------------------------------------------------------------------------------ grouping / routes
def test_groups_by_level():
    _, B, U, _ = _mods()
    assert B._enhance_groups(U._enhance_lists(2, [1, 2], [3])) == {2: [Ellipsis]}
    assert B._enhance_groups(U._enhance_lists(3, 2., [[3, 2], [3], None])) == {2: [0, 1, 2]}
    assert B._enhance_groups(U._enhance_lists(3, [[.5, 2], [-1], [2, 0, 1]], [[5], [3], None])) == {2: [0], 1: [1], 3: [2]}
    assert B._enhance_groups(U._enhance_lists(3, [[1], [1, 1], [1]], None)) == {1: [0], 2: [1, 2]}    # (the shared sigma list, padded by channel 1)
    assert B._enhance_groups(U._enhance_lists(3, None, None)) == {0: [0, 1, 2]}


def test_enhance_eligible_routes():
    W, B, _, _ = _mods()
    f32 = np.zeros((2, 8, 8), np.float32)
    f64 = f32.astype(np.float64)
    E = B.enhance_eligible
    assert E(f32, 1) == E(f32, 2) == E(f32, 8) == 'batch'
    assert E(f32, 9) == E(f32, 10) == E(f32, 15) == 'batch'         # the non-fused levels: wt_batch_decompose
    assert E(f32, 0) is None and E(f32, 16) is None and E(f32, True) is None and E(f32, 2.0) is None
    assert E(f32, 3, W.Triangle) == 'batch' and E(f64, 3, W.Triangle) == 'batch64'
    assert E(f32, 3, bilateral=1) == 'bilateral' and E(f32, 3, bilateral=[1., 2.]) == 'bilateral'
    assert E(f32, 11, bilateral=1) is None                          # the family's bilateral sigma_e table ends at 10
    for dt in (np.float64, np.int16, np.uint16, np.int32, '>f4', '>f8'):
        assert E(f32.astype(dt), 3) == 'batch64', dt
    assert E(f64, 3, bilateral=1) is None                           # float64 with bilateral=: the loop
    assert E(f64, 1) is None                                        # float64, one scale: no fused pass (wt_batch64_fused_ok)
    # the measured regime where the float64 batch is behind the loop: at most three frames of 2048^2 or more
    big = np.lib.stride_tricks.as_strided(np.zeros(1), (1, 2048, 2048), (0, 0, 0))
    big4 = np.lib.stride_tricks.as_strided(np.zeros(1), (4, 2048, 2048), (0, 0, 0))
    assert E(big, 3) is None and E(big, 3, channels=3) is None and E(big4, 3) == 'batch64'
    assert E(big, 3, channels=2) is None and E(np.broadcast_to(big, (2, 2048, 2048)), 3, channels=2) == 'batch64'
    assert E(big[:, :2047], 3, channels=3) == 'batch64' and E(big.astype(np.float32), 3, channels=3) == 'batch'
    assert E(np.zeros((2, 1, 8)), 3) is None                        # one-row float64 frames: no fused passes
    assert E(f32.astype(np.uint8), 3) is None and E(f32.astype(np.float16), 3) is None
    assert E([f32[0], f32[1]], 3) is None and E(f32[0], 3) is None
    # noise: scalars only; None (the lazy estimate) and arrays (noise maps) go to the loop
    assert E(f32, 3, noise_per_frame=[1., np.float32(2)]) == 'batch'
    assert E(f32, 3, noise_per_frame=[1., None]) is None
    assert E(f32, 3, noise_per_frame=[np.ones((8, 8), np.float32)] * 2) is None
    assert E(f32, 3, noise_per_frame=[np.array(1.), 1.]) is None
    assert E(f32, 3, noise_per_frame=None) is None

    class Odd(W.B3spline):                                          # re-tapped family: the generic operator
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.coefficients_1d = np.array([.25, .25, .25, .25])
    assert E(f32, 3, Odd) is None


def test_noise_forms_and_refusals():
    _, B, _, _ = _mods()
    N = B._enhance_noise
    assert N(None, 4, False) is None and N(None, 4, True) is None
    assert N(2., 3, False) == [2., 2., 2.] and N([1, 2, 3], 3, False) == [1, 2, 3]
    with pytest.raises(ValueError, match="one entry per frame"):
        N([1, 2], 3, False)
    m = np.ones((8, 8), np.float32)
    assert all(p is m for p in N(m, 3, False))                      # a noise map: to every frame (the loop)
    per = N([1., 2., 3.], 5, True)                                  # colour: per channel, shared by the frames
    assert len(per) == 5 and all(p == [1., 2., 3.] for p in per)
    a = np.arange(6.).reshape(2, 3)
    per = N(a, 2, True)                                             # (N, 3): frame i gets noise[i]
    assert len(per) == 2 and np.array_equal(per[0], a[0]) and np.array_equal(per[1], a[1])
    per = N(np.arange(9.).reshape(3, 3), 3, True)                   # N == 3: still (N, 3), not per channel
    assert np.array_equal(per[1], [3., 4., 5.])
    for bad in (2., [1., 2.], np.ones((2, 2)), np.ones((3, 3))):
        with pytest.raises(ValueError, match="noise"):
            N(bad, 2, True)


def test_frames_forms_and_refusals():
    _, B, _, _ = _mods()
    F = B._as_enhance_frames
    g, c = np.zeros((2, 4, 5), np.float32), np.zeros((2, 3, 4, 5), np.float32)
    assert F(g)[1] is False and F(c)[1] is True and F(g)[0] is g
    fr, col = F([c[0], c[1]])
    assert col and fr.shape == (2, 3, 4, 5)
    fr, col = F([g[0], g[1].astype(np.float64)])                    # mixed element types: the list (the loop)
    assert not col and isinstance(fr, list)
    for bad in (np.zeros((4, 5)), np.zeros((2, 4, 4, 5)), np.zeros((0, 4, 5)), [], [g[0], np.zeros((3, 3))]):
        with pytest.raises(ValueError, match="frames"):
            F(bad)


def test_out_is_refused_before_any_device_work(monkeypatch):
    W, B, _, L = _mods()

    def no_device(*a, **k):
        raise AssertionError("device work before the `out` check")
    monkeypatch.setattr(L, "default_context", no_device)
    monkeypatch.setattr(L, "acquire_batch", no_device)
    monkeypatch.setattr(L, "acquire_batch64", no_device)
    g = np.zeros((2, 8, 8), np.float32)
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros((2, 8, 8), np.float64), np.zeros((2, 8, 16), np.float32)[:, :, ::2]):
        with pytest.raises(ValueError, match="out"):
            W.enhance_stack(g, weights=[1, 2], out=bad)
    with pytest.raises(ValueError, match="out"):
        W.enhance_stack(np.zeros((2, 3, 8, 8)), weights=[[1, 2]] * 3, out=np.zeros((2, 3, 8, 9)))
    with pytest.raises(TypeError):
        W.enhance_stack(g, weights=[1, 2], no_such_option=1)


def test_fallback_loop_passes_the_per_frame_arguments(monkeypatch):
    W, B, _, _ = _mods()
    calls = []

    def recorder(*args, **kw):
        calls.append((args, kw))
        return np.zeros(np.shape(args[0]), np.float32)
    monkeypatch.setattr(B, "enhance", recorder)
    g = np.arange(2 * 4 * 5, dtype=np.float32).reshape(2, 4, 5)
    kw = dict(weights=None, denoise=None, soft_threshold=False)     # level 0: the loop
    res = W.enhance_stack(g, **kw)
    assert res.shape == g.shape and len(calls) == 2
    for i, (args, k) in enumerate(calls):
        assert len(args) == 1 and args[0] is not None and np.array_equal(args[0], g[i]) and k == kw
    calls.clear()
    nmap = np.ones((4, 5), np.float32)                              # a noise map: the loop, the map to every frame
    W.enhance_stack(g, nmap, weights=[1, 2], bilateral=1, scaling_function_class=W.Triangle)
    assert [len(a) for a, _ in calls] == [2, 2] and all(a[1] is nmap for a, _ in calls)
    assert calls[0][1] == dict(weights=[1, 2], denoise=None, soft_threshold=True, bilateral=1, scaling_function_class=W.Triangle)
    calls.clear()
    c = np.zeros((2, 3, 4, 5), np.uint8)                            # uint8 frames: the loop; (N, 3) noise by frame
    noise = np.arange(6.).reshape(2, 3)
    out = np.empty((2, 3, 4, 5), np.float32)
    assert W.enhance_stack(c, noise, weights=2., out=out) is out
    assert [len(a) for a, _ in calls] == [2, 2]
    assert np.array_equal(calls[0][0][1], noise[0]) and np.array_equal(calls[1][0][1], noise[1])
    calls.clear()
    W.enhance_stack(g, [1., None], weights=[1, 2])                   # a None entry: that frame's lazy estimate, the loop
    assert [a[1] for a, _ in calls] == [1., None]


def test_new_abi_symbols_exist():
    import ctypes
    _, _, _, L = _mods()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("wt_batch_enhance_sum", "wt_batch64_enhance_sum"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert hasattr(L.BatchPlan, "enhance_sum") and hasattr(L.BatchPlan64, "enhance_sum")
    assert L.MAX_SUM_PLANES == 16


def test_public_names():
    W, B, _, _ = _mods()
    assert W.enhance_stack is B.enhance_stack and {"enhance_stack", "enhance_eligible"} <= set(B.__all__)


# ------------------------------------------------------------------------ the GPU tests' inputs, cases and oracles
SCALES = (1e6, 1e-3)              # neighbouring frames (and channels) nine decades apart
HARD_MARGIN = 1e-5                # |w| / tau stays this far from 1 at every hard-threshold sample (relative)

# rows that differ between neighbouring channels: a negative weight, a zero weight, sigma 0 where the neighbour has 5
COLOUR_W3 = [[.5, 2, 1], [1, -1.5, 0], [2, 2, 1]]
COLOUR_D3 = [[5, 3, 0], [0, 5, 2], [3, 0, 0]]
GRAY_W = [-1.5, 0, 2, .5, 1, 2, 1, -1, .5, 1]
GRAY_D = [5, 0, 3, 2, 0, 1, 0, 1, 0, 1]


def _gray(level):
    return dict(weights=GRAY_W[:level], denoise=GRAY_D[:level])


def case(name, n, shape, colour=False, dtype=np.float32, noise=None, soft=True, seed=0, family="b3spline", bilateral=None,
         bilateral_scaling=False, chunk_frames=None, **params):
    return dict(name=name, n=n, shape=shape, colour=colour, dtype=np.dtype(dtype), noise=noise, soft=soft, seed=seed,
                family=family, bilateral=bilateral, bilateral_scaling=bilateral_scaling, chunk_frames=chunk_frames,
                params=params)


_C3 = dict(weights=COLOUR_W3, denoise=COLOUR_D3)
CASES = [
    # stack sizes 1, 2, 9, gray and colour; every shape; levels 1, 2, 5, 8, 10; every noise form
    case("gray-n1-1x1-L1", 1, (1, 1), **_gray(1)),
    case("gray-n2-1x2-L2-scalar", 2, (1, 2), noise="scalar", **_gray(2)),
    case("gray-n9-3x5-L5-perframe", 9, (3, 5), noise="frame", **_gray(5)),
    case("gray-n2-33x31-L1", 2, (33, 31), **_gray(1)),
    case("gray-n2-96x128-L8-hard-scalar", 2, (96, 128), noise="scalar", soft=False, seed=3, **_gray(8)),
    case("gray-n2-96x128-L10", 2, (96, 128), **_gray(10)),
    case("colour-n1-5x7-L3", 1, (5, 7), colour=True, **_C3),
    case("colour-n2-17x4-L3-perchannel", 2, (17, 4), colour=True, noise="channel", **_C3),
    case("colour-n9-64x64-L3-n3", 9, (64, 64), colour=True, noise="frame", **_C3),
    case("colour-n2-33x31-L3-hard", 2, (33, 31), colour=True, soft=False, **_C3),
    case("colour-n2-33x31-three-levels", 2, (33, 31), colour=True, weights=[[.5, 2], [-1], [2, 0, 1]], denoise=[[5], [3], None]),
    case("colour-n2-33x31-three-levels-hard-n3", 2, (33, 31), colour=True, noise="frame", soft=False, seed=1,
         weights=[[.5, 2], [-1], [2, 0, 1]], denoise=[[5], [3], [0, 2]]),
    case("colour-n2-5x7-quirk-triangle", 2, (5, 7), colour=True, family="triangle", weights=2., denoise=[[3, 2], [3], None]),
    case("gray-n2-64x64-L5-triangle-hard", 2, (64, 64), family="triangle", soft=False, **_gray(5)),
    case("gray-n7-33x31-L2-chunks", 7, (33, 31), chunk_frames=3, **_gray(2)),
    case("colour-n3-17x4-L3-chunks", 3, (17, 4), colour=True, chunk_frames=3, **_C3),
    case("colour-n2-33x31-L3-bilateral", 2, (33, 31), colour=True, bilateral=1, **_C3),
    case("gray-n2-17x4-L2-bilateral-list-scaling", 2, (17, 4), noise="scalar", bilateral=[1., 2.], bilateral_scaling=True, **_gray(2)),
    case("gray-n9-5x7-L5-bilateral-hard", 9, (5, 7), noise="frame", soft=False, bilateral=1, **_gray(5)),
    case("colour-n2-33x31-L3-f64", 2, (33, 31), colour=True, dtype=np.float64, **_C3),
    case("gray-n2-5x7-L2-int16-perframe", 2, (5, 7), dtype=np.int16, noise="frame", **_gray(2)),
    case("gray-n9-3x5-L5-uint16", 9, (3, 5), dtype=np.uint16, **_gray(5)),
    case("colour-n1-64x64-L8-bef4-hard", 1, (64, 64), colour=True, dtype='>f4', soft=False,
         weights=[GRAY_W[:8], GRAY_W[1:9], GRAY_W[2:10]], denoise=[GRAY_D[:8], GRAY_D[1:9], GRAY_D[2:10]]),
    case("colour-n2-17x4-three-levels-f64-chunks", 2, (17, 4), colour=True, dtype=np.float64, chunk_frames=1,
         weights=[[.5, 2], [-1, 1, 0, 2], [2, 0, 1]], denoise=[[5], [3], None]),
]
CASE_IDS = [c["name"] for c in CASES]


def case_frames(c):
    """the stack of a case: N(0, 1) planes, neighbouring planes (frames, and the channels of a frame) nine decades
    apart; integer types: amplitudes 3000 / 30 around a pedestal"""
    n, (H, W) = c["n"], c["shape"]
    k = 3 if c["colour"] else 1
    rng = np.random.default_rng(1000 + c["seed"])
    z = rng.standard_normal((n * k, H, W))
    dt = c["dtype"]
    if dt.kind in "iu":
        amp = np.array([3000. if i % 2 == 0 else 30. for i in range(n * k)])[:, None, None]
        a = np.rint(z * amp + (20000 if dt.kind == "u" else 0)).clip(np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)
    else:
        amp = np.array([SCALES[i % 2] for i in range(n * k)])[:, None, None]
        a = (z * amp).astype(dt)
    return a.reshape((n, 3, H, W) if c["colour"] else (n, H, W))


def case_noise(c, frames):
    """(the `noise` argument of enhance_stack, [frame i's second argument of utils.enhance]) - levels near each
    plane's own sigma, so that the thresholds bite"""
    form, n = c["noise"], c["n"]
    if form is None:
        return None, None
    sd = np.asarray(frames, np.float64).std(axis=(-2, -1)) + 1e-30          # (n,) or (n, 3)
    if form == "scalar":
        v = float(sd.reshape(n, -1)[0, 0]) * 0.9
        return v, [v] * n
    if form == "channel":                                                    # colour: shared by the frames
        v = [float(x) * 1.1 for x in sd[0]]
        return v, [v] * n
    arr = sd * 0.8                                                           # "frame": (n,) gray, (n, 3) colour
    if not c["colour"]:
        arr = [float(x) for x in arr]
    return arr, [arr[i] for i in range(n)]


def oracle_enhance(img, noise, c, dtype=np.float64):
    """utils.enhance of ONE frame in numpy at `dtype`: oracle.atrous_numpy.enhance, or - with bilateral=, which that
    function does not take - composed from atrous_standard(..., bilateral) and the oracle's Coeffs.denoise over
    ref_lists' lists"""
    img = np.asarray(img).astype(dtype)
    p = c["params"]
    if c["bilateral"] is None:
        return O.enhance(img, noise, copy.deepcopy(p["weights"]), copy.deepcopy(p["denoise"]), c["soft"], c["family"])
    out = np.empty_like(img)
    for ch, dns, wgt in ref_lists(img.ndim, copy.deepcopy(p["weights"]), copy.deepcopy(p["denoise"])):
        bil = copy.deepcopy(c["bilateral"])
        co = O.Coeffs(O.atrous_standard(img[ch], len(wgt), c["family"], bil, c["bilateral_scaling"]), c["family"], bil)
        co.noise = (noise if ch is Ellipsis else noise[ch]) if noise is not None else co.get_noise()
        co.denoise(dns, weights=wgt, soft_threshold=c["soft"])
        out[ch] = co.data.sum(axis=0)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(frames, noise argument, per-frame noise, [float64 oracle result per frame]) of a case, computed once"""
    c = CASES[CASE_IDS.index(name)]
    frames = case_frames(c)
    noise, per = case_noise(c, frames)
    ref = [oracle_enhance(frames[i], None if per is None else per[i], c) for i in range(c["n"])]
    for r in ref:
        r.setflags(write=False)
    frames.setflags(write=False)
    return frames, noise, per, ref


def case_kwargs(c, W):
    """the keyword arguments of enhance_stack / utils.enhance for a case"""
    kw = dict(weights=copy.deepcopy(c["params"]["weights"]), denoise=copy.deepcopy(c["params"]["denoise"]),
              soft_threshold=c["soft"])
    if c["family"] == "triangle":
        kw["scaling_function_class"] = W.Triangle
    if c["bilateral"] is not None:
        kw["bilateral"] = copy.deepcopy(c["bilateral"])
        if c["bilateral_scaling"]:
            kw["bilateral_scaling"] = True
    return kw


def case_class(c):
    """which measured bound a case is held to"""
    if c["dtype"] != np.float32:
        return "f64"
    return "f32_bilateral" if c["bilateral"] is not None else "f32"


def _hard_ratios(img, noise, c, dtype):
    """|w| / tau of every sample that meets a hard threshold, per (channel, scale), in numpy at `dtype`"""
    img = np.asarray(img).astype(dtype)
    p = c["params"]
    out = []
    for ch, dns, wgt in ref_lists(img.ndim, copy.deepcopy(p["weights"]), copy.deepcopy(p["denoise"])):
        bil = copy.deepcopy(c["bilateral"])
        co = O.Coeffs(O.atrous_standard(img[ch], len(wgt), c["family"], bil, c["bilateral_scaling"]), c["family"], bil)
        nz = (noise if ch is Ellipsis else noise[ch]) if noise is not None else co.get_noise()
        for scl, (_, sig) in enumerate(zip(co.data, dns)):
            if sig != 0 and nz != 0:
                out.append(np.abs(co.data[scl]) / (sig * nz * co.sigma_e[scl]))
    return out


HARD_CASES = [c["name"] for c in CASES if not c["soft"]]


@pytest.mark.parametrize("name", HARD_CASES)
def test_premise_hard_decisions_are_the_same_in_float32_and_float64(name):
    """every hard-threshold comparison of the GPU tests is over ALL samples: the float32 and the float64 oracle
    decide alike everywhere, and no |w| is within HARD_MARGIN (relative) of its threshold"""
    c = CASES[CASE_IDS.index(name)]
    frames, _, per, _ = case_reference(name)
    low = np.float32 if c["dtype"] == np.float32 else np.float64
    closest = np.inf
    for i in range(c["n"]):
        nz = None if per is None else per[i]
        r64 = _hard_ratios(frames[i], nz, c, np.float64)
        rlo = _hard_ratios(frames[i], nz, c, low)
        assert len(r64) == len(rlo) and len(r64) > 0
        for a, b in zip(r64, rlo):
            assert np.array_equal(a > 1, b > 1), f"{name}: frame {i}: float32 and float64 decide differently"
            closest = min(closest, float(np.abs(a - 1).min()), float(np.abs(b - 1).min()))
    print(f"{name}: closest |w| / tau to 1: {closest:.3e}")
    assert closest > HARD_MARGIN


def test_premise_every_batched_case_has_a_route():
    """host logic: every case of the GPU file runs on a batch (its fallback is patched to raise there)"""
    W, B, U, L = _mods()
    for c in CASES:
        frames = case_frames(c)
        sfc = W.Triangle if c["family"] == "triangle" else W.B3spline
        plans = U._enhance_lists(3 if c["colour"] else 2, copy.deepcopy(c["params"]["weights"]), copy.deepcopy(c["params"]["denoise"]))
        want = {"f64": "batch64", "f32": "batch", "f32_bilateral": "bilateral"}[case_class(c)]
        for level in B._enhance_groups(plans):
            rep = frames[:, 0] if c["colour"] else frames
            assert B.enhance_eligible(rep, level, sfc, copy.deepcopy(c["bilateral"])) == want, (c["name"], level)


# how much of the GPU file's bounds (4 x the per-frame API's measured error, test_gpu_enhance_stack.py) the float32
# numpy oracle alone uses against the float64 one, in units of max|plane|: printed, and recorded here from this run
#   f32 plain 1.9e-07 .. worst case, f32 bilateral 1.6e-07 (see the test's output for every case)
@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["dtype"] == np.float32])
def test_premise_float32_oracle_share_of_the_bounds(name):
    c = CASES[CASE_IDS.index(name)]
    frames, _, per, ref = case_reference(name)
    worst = 0.0
    for i in range(c["n"]):
        lo = oracle_enhance(frames[i], None if per is None else per[i], c, np.float32)
        worst = max(worst, plane_errors(lo, ref[i], frames[i]))
    print(f"{name}: float32 oracle vs float64 oracle: {worst:.3e} of max|plane|")
    assert np.isfinite(worst)


def plane_errors(got, ref, frame):
    """worst |got - ref| / max|plane| over the 2-D planes of one frame (a gray frame, or the channels of a colour
    frame): every plane under its own scale"""
    got, ref, frame = (np.asarray(a, np.float64) for a in (got, ref, frame))
    if frame.ndim == 2:
        got, ref, frame = got[None], ref[None], frame[None]
    worst = 0.0
    for g, r, f in zip(got, ref, frame):
        amax = float(np.abs(f).max())
        d = float(np.abs(g - r).max())
        worst = max(worst, d / amax if amax > 0 else (0.0 if d == 0 else np.inf))
    return worst
