"""What tests/test_gpu_lines_values.py relies on, checked without a device: numpy's median of its tie / padding rows is
the (lo + hi) / 2 rule in the stack's type; the float64 oracle's NaN mask is what the filter's reach predicts under the
'mirror' border (so the GPU test's mask reference is not circular); no hard-thresholded coefficient of its finite
inputs lies within HARD_MARGIN of its threshold; and the drivers on stub batches: a NaN median reaches the thresholds
of its own signal only, as the per-signal rule (wavelets._tau_row) gives them, and a batch goes back to its cache
whether the call returns or raises."""
import numpy as np
import pytest

from oracle import atrous_numpy as O
import test_gpu_lines_values as T

FAMS = T.FAMS
HW = {"b3spline": 2, "triangle": 1}


# ---------------------------------------------------------------- class 3: numpy's median is the (lo + hi) / 2 rule

@pytest.mark.parametrize("dtype", T.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam,ofam", FAMS)
def test_numpy_median_is_the_mean_of_the_two_middle_values_in_the_stacks_type(fam, ofam, dtype):
    budget = 8192 if dtype == np.float32 else 4096
    for seed, lengths in ((3, T.MEDIAN_LENGTHS + (budget,)), (4, T.MEDIAN_LENGTHS + (512,)), (5, T.MEDIAN_LENGTHS + (512,))):
        for N in lengths:
            rows = T.median_rows(N, dtype, seed=seed)
            assert rows.dtype == dtype and rows.shape == (6, N) and np.all(np.isfinite(rows))
            assert np.signbit(rows[3]).any() and not rows[3].any() and len(np.unique(rows[5])) == 1
            w0 = np.stack([O.atrous_standard_1d(r, 1, ofam)[0] for r in rows])
            assert w0.dtype == dtype
            v = np.sort(np.abs(w0), axis=-1)
            lo, hi = v[:, (N - 1) // 2], v[:, N // 2]
            with np.errstate(over="raise"):
                want = lo if N % 2 else (lo + hi) / dtype(2)
            got = np.median(np.abs(w0), axis=-1)
            assert got.dtype == dtype
            np.testing.assert_array_equal(got, want, err_msg=f"{fam} N={N}")
            np.testing.assert_array_equal(T.rank_median(w0), want)
            for r, least in ((1, 255), (2, 16)):          # ties straddle the median rank of the quantised and the +-x row
                if N >= least:
                    assert v[r, (N - 1) // 2] in (v[r, (N - 1) // 2 - 1], v[r, (N - 1) // 2 + 1]), (fam, N, r)


# ---------------------------------------------------------------- class 1: the oracle's NaN mask is the filter's reach

def reach_mask(bad, level, hw):
    """(level + 1, N) bool: where the planes of a signal hold NaN when its samples `bad` do.  c_{s+1}(x) takes c_s at
    the mirror images of x + j 2^s, |j| <= hw, with non-zero taps: it is NaN where any of them is; w_s = c_s - c_{s+1}
    is NaN where either is, and c_s is among the samples c_{s+1} takes."""
    N = len(bad)
    out = np.zeros((level + 1, N), bool)
    cur = bad.copy()
    for s in range(level):
        nxt = np.zeros(N, bool)
        for x in range(N):
            for j in range(-hw, hw + 1):
                i = x + j * 2 ** s
                if N > 1:
                    i %= 2 * N - 2
                    i = i if i < N else 2 * N - 2 - i
                else:
                    i = 0
                nxt[x] |= cur[i]
        out[s] = nxt
        cur = nxt
    out[level] = cur
    return out


@pytest.mark.parametrize("fam,ofam", FAMS)
def test_the_oracles_nan_mask_is_the_reach_of_the_filter(fam, ofam):
    for N in T.LENGTHS:
        base = T.clean_stack(1, N, np.float64, seed=N)[0]
        for kind in T.NAN_ONLY:
            row = T.spoil(base, kind)
            for level in (1, 3):
                with np.errstate(invalid="ignore"):
                    mask = np.isnan(O.atrous_standard_1d(row, level, ofam))
                np.testing.assert_array_equal(mask, reach_mask(np.isnan(row), level, HW[ofam]), err_msg=f"{fam} N={N} {kind} L={level}")
                assert mask.any() and (kind != "nan_mid" or N < 256 or not mask.all())


# ---------------------------------------------------------------- classes 1 and 4: hard thresholds keep clear

def margin(rows, ofam, noises):
    """min over the signals `rows` (any float type; the oracle works on their float64 copies) and the finite
    thresholded coefficients of | |w| / tau - 1 | for denoise(row, WEIGHTS): tau = sigma * noise * sigma_e[s], noise
    the entry of `noises` or - None - the rank rule's MAD estimate; a NaN or zero noise level thresholds nothing"""
    best = np.inf
    for row, noise in zip(rows, noises):
        with np.errstate(invalid="ignore"):
            c = O.Coeffs(O.atrous_standard_1d(row.astype(np.float64), len(T.WEIGHTS), ofam), ofam)
            if noise is None:
                noise = T.rank_median(c.data[0]) / 0.6745 / c.sigma_e[0]
            if not np.isfinite(noise) or noise == 0:
                continue
            for s, sig in enumerate(T.WEIGHTS):
                r = np.abs(np.abs(c.data[s]) / (sig * noise * c.sigma_e[s]) - 1)
                r = r[np.isfinite(r)]
                if r.size:
                    best = min(best, float(r.min()))
    return best


@pytest.mark.parametrize("dtype", T.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam,ofam", FAMS)
def test_hard_thresholded_signals_keep_clear_of_their_thresholds(fam, ofam, dtype):
    """the stacks of the signal engine's class 1 and class 4 tests: no float64 oracle coefficient within HARD_MARGIN
    (relative) of its threshold, so no rounding of either route can flip a sample.  Of the cubes of the axis engine's
    class 1 / 2 test the touched columns are held to it, for the three noise forms: they are what is compared with the
    per-signal call; the untouched columns are compared between two runs of the engine."""
    for N in T.LENGTHS:
        clean = T.clean_stack(8, N, dtype, seed=T.SEEDS[N])
        for stack in (clean,) + tuple(T.mixed_stack(clean, mix) for mix in T.MIXES):
            for noise in (None, 1.25):
                assert margin(stack, ofam, [noise] * 8) > T.HARD_MARGIN == 1e-4, (N, noise)
    for N in T.LENGTHS:
        I, cols = T.bad_columns(N, dtype)
        a = T.mixed_cube(T.clean_cube(N, I, dtype), cols)
        levels = T.cube_levels(N, I)
        touched = [a[o, :, i] for o, i, _ in cols]
        for noises in ([None] * 10, [1.25] * 10, [levels[o, i] for o, i, _ in cols]):
            assert margin(touched, ofam, noises) > T.HARD_MARGIN, (N, noises[0])
    for N in (17, 300):
        assert margin(T.clean_stack(4, N, dtype, seed=40 + N), ofam, [None] * 4) > T.HARD_MARGIN
        assert margin(T.clean_stack(38, N, dtype, seed=41 + N), ofam, [None] * 38) > T.HARD_MARGIN


# ---------------------------------------------------------------- the drivers on stub batches

class FakeSignals:
    """a SignalBatch without a device: records what the driver hands it; signal 1's median is NaN"""
    made = []

    def __init__(self, ctx, n, n_samples, family, max_level, dtype):
        self._h, self.ctx, self.n, self.key, self.dtype = 1, ctx, n, (n_samples, family, max_level, dtype), dtype
        self.n_samples, self.level, self.taus, self.fail = n_samples, 0, None, None
        FakeSignals.made.append(self)

    def _key(self):
        return self.key

    def close(self):
        self._h = None

    def upload(self, signals, f0=0):
        pass

    def decompose(self, nf, level):
        self.level = level

    def abs_median(self, nf):
        if self.fail:
            raise self.fail
        med = np.full(nf, 2.0, self.dtype)
        med[1] = np.nan
        return med

    def denoise_sum(self, nf, taus, wgts, soft=True):
        self.taus = np.array(taus, np.float64)

    def moments(self, nf):
        return np.ones((nf, self.level + 1, 2))

    def wow_sum(self, nf, taus, factors, whitening, soft=True, write_planes=False):
        self.taus = np.array(taus, np.float64)

    def download_sum(self, nf, out=None, f0=0):
        out[...] = 0
        return out

    def download_planes(self, nf, out=None, f0=0):
        out[...] = 0
        return out


class FakeAlong(FakeSignals):
    def __init__(self, ctx, n, n_samples, family, max_level, dtype, planes):
        FakeSignals.__init__(self, ctx, n, n_samples, family, max_level, dtype)
        self.key += (planes,)

    def upload(self, block):
        self.chunk = (block.shape[0], block.shape[2])

    def abs_median(self):
        return FakeSignals.abs_median(self, self.chunk[0] * self.chunk[1]).reshape(self.chunk)

    def denoise(self, level, taus, wgts, soft=True):
        self.taus = np.array(taus, np.float64)

    def download_sum(self, out):
        out[...] = 0
        return out


@pytest.fixture
def stubbed(monkeypatch):
    """_lib with stub batches behind acquire_signals / acquire_along and fresh caches: (the module, the two caches)"""
    from wavelets_amd import _lib as L
    import wavelets_amd                                          # noqa: F401 (the drivers import the names below)
    ctx = object()
    caches = L._StackCache(), L._StackCache()
    monkeypatch.setattr(L, "_signal_cache", caches[0])
    monkeypatch.setattr(L, "_along_cache", caches[1])
    monkeypatch.setattr(L, "SignalBatch", FakeSignals)
    monkeypatch.setattr(L, "AlongBatch", FakeAlong)
    monkeypatch.setattr(L, "default_context", lambda: ctx)
    monkeypatch.setattr(L, "host_empty", lambda shape, ctx, dtype=np.float32: np.empty(shape, dtype))
    monkeypatch.setattr(L, "signals_ok", lambda *a: True)
    monkeypatch.setattr(L, "along_ok", lambda *a: True)
    FakeSignals.made.clear()
    return L, caches, ctx


@pytest.mark.parametrize("dtype", T.DTYPES, ids=("f32", "f64"))
def test_a_nan_median_reaches_the_thresholds_of_its_own_signal_only(stubbed, dtype):
    """the rule of the per-signal call: a NaN median is a NaN noise level and a row of NaN thresholds
    (wavelets._tau_row), which the kernels take as significance one; the other signals' rows are those of their own
    medians; the batch goes back to its cache"""
    import wavelets_amd as W
    from wavelets_amd.wavelets import _tau_row, _noise_from_median
    from wavelets_amd.signals import _thresholds
    L, caches, ctx = stubbed
    sig = T.clean_stack(3, 32, dtype, seed=1)
    sigma_e, entries, _ = _thresholds(T.WEIGHTS, W.B3spline)
    for soft in (True, False):
        rows = np.array([_tau_row(entries, _noise_from_median(dtype(m), sigma_e), sigma_e, soft) for m in (2.0, np.nan, 2.0)])
        assert np.isnan(rows[1]).all() and np.isfinite(rows[[0, 2]]).all() and (rows[[0, 2]] > 0).all()
        W.denoise_signals(sig, T.WEIGHTS, soft_threshold=soft)
        (sb,) = caches[0].lists[id(ctx)]                             # back in its cache
        assert type(sb) is FakeSignals
        np.testing.assert_array_equal(sb.taus, rows)
        # a scalar for signal 1 skips its median
        W.denoise_signals(sig, T.WEIGHTS, noise=[None, 1.5, None], soft_threshold=soft)
        np.testing.assert_array_equal(sb.taus[1], _tau_row(entries, 1.5, sigma_e, soft))
        np.testing.assert_array_equal(sb.taus[[0, 2]], rows[[0, 2]])
        a = np.ascontiguousarray(sig.T.reshape(32, 1, 3).transpose(1, 0, 2))                   # (1, 32, 3): signal i = column i
        W.denoise_along(a, T.WEIGHTS, axis=1, soft_threshold=soft)
        (ab,) = caches[1].lists[id(ctx)]
        assert type(ab) is FakeAlong
        np.testing.assert_array_equal(ab.taus, rows)
        W.wow_signals(sig, denoise_coefficients=[5, 2], n_scales=2, soft_threshold=soft)
        wrows = np.array([_tau_row([(0, 5, 1), (1, 2, 1)], _noise_from_median(dtype(m), sigma_e), sigma_e, soft) for m in (2.0, np.nan, 2.0)])
        assert caches[0].lists[id(ctx)] == [sb]
        np.testing.assert_array_equal(sb.taus, wrows)


def test_a_failing_median_leaves_the_batch_in_its_cache(stubbed):
    import wavelets_amd as W
    L, caches, ctx = stubbed
    sig = T.clean_stack(3, 32, np.float32, seed=2)
    W.denoise_signals(sig, T.WEIGHTS)
    sb = FakeSignals.made[-1]
    sb.fail = L.WatrooHipError("wt_signals_abs_median: device lost")
    for call in (lambda: W.denoise_signals(sig, T.WEIGHTS), lambda: W.wow_signals(sig, denoise_coefficients=[5, 2], n_scales=2)):
        with pytest.raises(L.WatrooHipError, match="device lost"):
            call()
        assert caches[0].lists[id(ctx)] == [sb] and sb._h
    a = np.ascontiguousarray(sig.T.reshape(32, 1, 3).transpose(1, 0, 2))
    W.denoise_along(a, T.WEIGHTS, axis=1)
    ab = FakeSignals.made[-1]
    ab.fail = L.WatrooHipError("wt_along_abs_median: device lost")
    with pytest.raises(L.WatrooHipError, match="device lost"):
        W.denoise_along(a, T.WEIGHTS, axis=1)
    assert caches[1].lists[id(ctx)] == [ab] and ab._h


def test_a_one_sample_axis_takes_its_pitch_from_the_slices():
    """numpy keeps any stride for an axis of length one (a transposed copy made contiguous keeps the old one): the
    pitch of an (O, 1, I) block is then the slices' distance, not that stride"""
    from types import SimpleNamespace
    from wavelets_amd import _lib as L
    me = SimpleNamespace(dtype=np.dtype(np.float32), n_samples=1)
    a = np.ascontiguousarray(np.zeros((2, 6, 1), np.float32).transpose(0, 2, 1))
    assert a.flags.c_contiguous and a.shape == (2, 1, 6)
    assert L.AlongBatch._rows(me, a) == 6
    assert L.AlongBatch._rows(me, a[:1]) == 6 and L.AlongBatch._rows(me, np.zeros((3, 1, 7), np.float32)[:, :, :4]) == 7
    me.n_samples = 5
    assert L.AlongBatch._rows(me, np.zeros((2, 5, 9), np.float32)[:, :, 2:6]) == 9
    with pytest.raises(ValueError):
        L.AlongBatch._rows(me, np.zeros((2, 5, 9), np.float32)[:, :, ::2])


def test_the_cancelled_standard_deviation_comes_from_the_samples(stubbed):
    """utils._std_cancels says where the error of sumsq / N - mean^2 can exceed what float64 wow allows between its
    routes; there _wow_factor takes the standard deviation it is handed, and wow_signals hands every such signal
    np.std of its downloaded last plane.  At the gate the two values agree far inside that bound, whichever way the
    sums are folded, so routes on different sides of it agree too."""
    import math
    from wavelets_amd import utils as U
    WS = T.TW._mod()                                             # (the module: the package exports the function)
    N = 4096
    x = 1e4 + 0.01 * np.random.default_rng(0).standard_normal(N)
    exact = (float(x.sum()), float((x * x).sum()))
    assert U._std_cancels(exact, float(N)) and U._std_cancels((N * 7.25, N * 7.25 ** 2), float(N))
    y = 10 + 3 * np.random.default_rng(1).standard_normal(N)
    assert not U._std_cancels((float(y.sum()), float((y * y).sum())), float(N))
    assert not U._std_cancels((np.nan, np.nan), float(N)) and not U._std_cancels((np.inf, np.inf), float(N))
    assert not U._std_cancels((0.0, 0.0), float(N))
    one_pass = np.sqrt(max(exact[1] / N - (exact[0] / N) ** 2, 0.0))
    assert abs(one_pass / np.std(x) - 1) > 1e-7                     # (what the one-pass formula loses here)
    assert U._plane_std(x.astype(np.float64)[None]) == np.std(x)
    for ft in (np.float32, np.float64):
        got = U._wow_factor(3, 3, 2.0, exact + (None, None), float(N), False, True, 0, ft, std=np.std(x))
        assert type(got) is ft and got == ft(2.0 / ft(np.std(x)))
        assert U._wow_factor(3, 3, 2.0, exact + (None, None), float(N), False, True, 0, ft) == ft(2.0 / ft(one_pass))

    # around the gate: a variance of 0.5 .. 2 times _STD_CANCELS of the mean square; three fold orders of the sums
    # (exact, pairwise, sequential) give one-pass values within 1e-11 of np.std, a tenth of F64_WOW = 1e-10
    assert U._STD_CANCELS == 1e-3
    for ped in (22.0, 31.0, 32.0, 45.0):
        z = ped + np.random.default_rng(int(ped)).standard_normal(N)
        r = z.var() / (z * z).mean()
        assert 0.4e-3 < r < 2.2e-3 and U._std_cancels((math.fsum(z), math.fsum(z * z)), float(N)) == (r < 1e-3)
        for tot, tot2 in ((math.fsum(z), math.fsum(z * z)), (float(z.sum()), float((z * z).sum())),
                          (float(np.cumsum(z)[-1]), float(np.cumsum(z * z)[-1]))):
            assert abs(math.sqrt(tot2 / N - (tot / N) ** 2) / np.std(z) - 1) <= 0.1 * T.TW.F64_WOW

    class Planes:
        dtype, ctx = np.dtype(np.float64), None          # (the stubbed host_empty allocates the target)
        asked = []

        def download_planes(self, nf, out=None, f0=0):
            self.asked.append((nf, f0))
            out[:] = 0
            out[0, 2] = (x, y)[f0]
            return out
    mom = [[[0.0, 1.0]] * 2 + [list(exact)], [[0.0, 1.0]] * 2 + [[float(y.sum()), float((y * y).sum())]]]
    assert WS._cancelled_stds(Planes(), 2, mom, [2], 2, float(N)) == [np.std(x), None]
    assert Planes.asked == [(1, 0)]                                                        # that signal alone comes down
    assert WS._cancelled_stds(None, 2, mom, [0, 1], 2, float(N)) is None                   # the last plane needs no moments
    assert WS._cancelled_stds(None, 1, mom[1:], [2], 2, float(N)) is None                  # nothing cancelled: no download
    rows = WS._factor_rows(mom, [None] * 3, [2], 2, [1, 1, 2.0], float(N), False, True, np.float64, [np.std(x), None])
    assert rows[0][2] == 2.0 / np.std(x) and rows[1][2] == U._wow_factor(2, 2, 2.0, mom[1][2] + [None, None], float(N), False, True, 0, np.float64)
