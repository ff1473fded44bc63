"""The 1-D engines (transform_signals, denoise_signals, transform_along, denoise_along, wow_signals, wow_along) on the
values the shape tests leave out: NaN and inf samples, abnormal signals next to normal ones, ties and padding in the
exact median, inputs scaled by powers of two into the far normal range and into the denormals, wow on a pedestal.

THE CONTRACT FOR NON-FINITE SAMPLES, read from the per-signal call (wt_abs_median in wt_apps.hip over wt_hist_kernel /
wt_select_step_kernel / wt_min_greater_kernel of wt_kernels_apps.h; wt64_abs_median in wt_f64.h over wt_select64.h; a
signal is transformed with flags 0, so no riding histogram and - below 2^20 samples - no window takes part):

  * every level of the radix select bins EVERY magnitude key, the keys of NaN (exponent all ones, above infinity)
    included.  "rank ... not found (NaN input?)" is raised when a level counts fewer keys than the rank, which a key
    that is always counted cannot cause: the per-signal call does NOT raise on a NaN or an inf;
  * its median is the key of rank (N - 1) / 2 in the order of the bit patterns - numpy's sort order of |w_0|, NaN last -
    and for an even N the mean of that key and the next one (the next greater key of wt_min_greater_kernel, or the
    same key when the count of keys <= it reaches the next rank).  So a signal of which fewer than half the |w_0| are
    NaN gets a finite median (np.median would give NaN), and one whose rank falls among the NaN keys a NaN median;
  * a NaN median gives a NaN noise level and NaN thresholds (wavelets._scalar_tau: NaN == 0 and NaN < 0 are False),
    and every kernel takes `tau > 0` False as significance one: such a signal comes back unthresholded, NaN where its
    planes hold NaN.

The engines sort the same keys (wt_signal_abs_key, all-ones padding above every key) and read the same ranks, so they
must return the loop's rows bit for bit, NaN positions included, and raise nothing: an exception of either route fails
the test that meets it.  test_the_loop_takes_nan_keys_as_ordinary_keys holds the reading itself against the device.

Bounds: exact equality everywhere but in the wow tests with moments, which use the bounds of
tests/test_gpu_wow_signals.py (F32_WOW, F64_WOW, its oracle rule and its moments bound) unchanged.  The oracle's NaN
masks are checked against the filter's reach, and the hard-threshold margins of the finite inputs against HARD_MARGIN,
without a device in tests/test_lines_values_cpu.py."""
import numpy as np
import pytest

import test_gpu_wow_signals as TW

pytestmark = pytest.mark.gpu

FAMS = (("B3spline", "b3spline"), ("Triangle", "triangle"))
DTYPES = (np.float32, np.float64)
LENGTHS = (5, 16, 17, 256, 300)
WEIGHTS = [5, 3]
HARD_MARGIN = 1e-4            # tests/test_gpu_nd_edges.py
# the seed of the class 1 stack of every length: chosen so that no float64 oracle coefficient of its rows lies within
# HARD_MARGIN of a threshold (tests/test_lines_values_cpu.py asserts it; seed 256 at N = 256 comes to 9.7e-5)
SEEDS = {5: 5, 16: 16, 17: 17, 256: 2256, 300: 300}

KINDS = ("nan_first", "nan_last", "nan_mid", "pinf", "ninf", "all_nan", "most_nan")
NAN_ONLY = ("nan_first", "nan_last", "nan_mid", "all_nan", "most_nan")
# two mixed stacks of 8 rows: row -> kind; the other rows stay clean
MIXES = ({1: "nan_first", 3: "nan_last", 4: "nan_mid", 6: "pinf"}, {0: "ninf", 2: "all_nan", 7: "most_nan"})


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


def clean_stack(M, N, dtype, seed=0):
    """M signals of N samples: seeded normal times 3 plus 10"""
    rng = np.random.default_rng([seed, M, N])
    return (rng.standard_normal((M, N)) * 3.0 + 10.0).astype(dtype)


def spoil(row, kind):
    """a copy of the 1-D `row` with the samples of value class `kind`"""
    r = row.copy()
    N = len(r)
    if kind == "nan_first":
        r[0] = np.nan                                  # (on the mirror border)
    elif kind == "nan_last":
        r[N - 1] = np.nan
    elif kind == "nan_mid":
        r[N // 2] = np.nan
    elif kind == "pinf":
        r[N // 2] = np.inf
    elif kind == "ninf":
        r[min(3, N - 1)] = -np.inf
    elif kind == "all_nan":
        r[:] = np.nan
    elif kind == "most_nan":
        r[:N // 2 + 1] = np.nan                        # more than half: the median rank lies among the NaN keys
    else:
        raise KeyError(kind)
    return r


def mixed_stack(clean, mix):
    a = clean.copy()
    for i, kind in mix.items():
        a[i] = spoil(clean[i], kind)
    return a


def rank_median(w0):
    """the median of the contract along the last axis, in the type of w0: sorted magnitudes, NaN last"""
    v = np.sort(np.abs(w0), axis=-1)
    N = v.shape[-1]
    lo = v[..., (N - 1) // 2]
    return lo if N % 2 else (lo + v[..., N // 2]) / w0.dtype.type(2)


def follows_the_loop(engine, per_row, clean_result, n, touched, label, rows=lambda r, i: r[i]):
    """the two assertions of a public call on a mixed stack of n signals.  engine(): the call; per_row(i): the
    per-signal call of touched signal i; clean_result: the engine's result on the clean stack; rows(result, i): signal
    i of a result.  Under the contract neither call raises: an exception of either fails the test."""
    got = engine()
    for i in range(n):
        if i in touched:
            np.testing.assert_array_equal(rows(got, i), per_row(i), err_msg=f"{label}: touched signal {i}")
        else:
            np.testing.assert_array_equal(rows(got, i), rows(clean_result, i), err_msg=f"{label}: untouched signal {i}")
    return got


def no_loop(monkeypatch, module, *names):
    """the per-signal calls of a driver module made an error: the stack must run on the engine"""
    def boom(*a, **k):
        raise AssertionError(f"{module.__name__} ran the per-signal loop")
    for name in names:
        monkeypatch.setattr(module, name, boom)


# ---------------------------------------------------------------- the reading itself

@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_the_loop_takes_nan_keys_as_ordinary_keys(W, dtype):
    """the per-signal call raises on no value class, and its noise level is the rank rule's (module docstring)"""
    from wavelets_amd.wavelets import _noise_from_median
    for fam, _ in FAMS:
        cls = getattr(W, fam)
        for N in (5, 16, 17):
            base = clean_stack(1, N, dtype, seed=N)[0]
            for kind in KINDS:
                row = spoil(base, kind)
                c = W.AtrousTransform(cls)(row, 1)
                w0 = np.array(c.data[0])
                noise = c.get_noise()
                want = _noise_from_median(rank_median(w0), cls(1).sigma_e())
                np.testing.assert_array_equal(noise, want, err_msg=f"{fam} N={N} {kind}")
                if kind in ("all_nan", "most_nan"):
                    assert np.isnan(noise)
                elif N >= 16 and kind.startswith("nan"):
                    assert np.isfinite(noise)                      # np.median gives NaN here: the loop does not


# ---------------------------------------------------------------- class 1: non-finite rows in the signal engine

@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam,ofam", FAMS)
def test_signals_with_non_finite_rows(W, monkeypatch, fam, ofam, dtype):
    from wavelets_amd import signals as S
    from oracle import atrous_numpy as O
    cls = getattr(W, fam)
    transform = S._transform_one
    for N in LENGTHS:
        clean = clean_stack(8, N, dtype, seed=SEEDS[N])
        level = 3
        clean_t = W.transform_signals(clean, level, cls)
        clean_d = {(noise, soft): W.denoise_signals(clean, WEIGHTS, cls, noise=noise, soft_threshold=soft)
                   for noise in (None, 1.25) for soft in (True, False)}
        for mix in MIXES:
            a = mixed_stack(clean, mix)
            assert S.signals_eligible(a, level, cls)
            with monkeypatch.context() as m:
                no_loop(m, S, "_transform_one")
                got = follows_the_loop(lambda: W.transform_signals(a, level, cls), lambda i: transform(a[i], level, cls),
                                       clean_t, 8, mix, f"transform {fam} N={N}")
            for i, kind in mix.items():
                if kind in NAN_ONLY:
                    mask = np.isnan(O.atrous_standard_1d(a[i].astype(np.float64), level, ofam))
                    np.testing.assert_array_equal(np.isnan(got[i]), mask, err_msg=f"NaN mask {fam} N={N} {kind}")
            for (noise, soft), ref in clean_d.items():
                per = [noise] * 8
                with monkeypatch.context() as m:
                    no_loop(m, S, "denoise")
                    follows_the_loop(lambda: W.denoise_signals(a, WEIGHTS, cls, noise=noise, soft_threshold=soft),
                                     lambda i: W.denoise(a[i], WEIGHTS, cls, per[i], soft_threshold=soft),
                                     ref, 8, mix, f"denoise {fam} N={N} noise={noise} soft={soft}")
            # a scalar for the bad rows only: their median is skipped, the clean rows keep their own estimate
            per = [1.25 if i in mix else None for i in range(8)]
            for soft in (True, False):
                with monkeypatch.context() as m:
                    no_loop(m, S, "denoise")
                    follows_the_loop(lambda: W.denoise_signals(a, WEIGHTS, cls, noise=per, soft_threshold=soft),
                                     lambda i: W.denoise(a[i], WEIGHTS, cls, per[i], soft_threshold=soft),
                                     clean_d[(None, soft)], 8, mix, f"denoise {fam} N={N} scalar for the bad rows soft={soft}")


def test_signals_with_a_nan_row_at_the_budget(W, monkeypatch):
    from wavelets_amd import signals as S
    for dtype, N in ((np.float32, 8192), (np.float64, 4096)):
        clean = clean_stack(3, N, dtype, seed=1)
        mix = {1: "most_nan"}
        a = mixed_stack(clean, mix)
        ref = W.denoise_signals(clean, WEIGHTS)
        with monkeypatch.context() as m:
            no_loop(m, S, "denoise")
            follows_the_loop(lambda: W.denoise_signals(a, WEIGHTS), lambda i: W.denoise(a[i], WEIGHTS), ref, 3, mix, f"budget {N}")


# ---------------------------------------------------------------- classes 1 and 2: bad columns in the axis engine

def bad_columns(N, dtype):
    """(I, [(outer index, inner index, kind)]): an inner extent just past one tile, a bad column at inner indices 0,
    tile - 1, tile, I - 1 and in the middle of both outer slices, the kinds rotated so that all seven occur"""
    from wavelets_amd import _lib as L
    tile = L.along_tile(N, np.dtype(dtype).itemsize)
    I = tile + 3
    at = (0, tile - 1, tile, I - 1, tile // 2)
    assert len(set(at)) == 5
    return I, [(o, i, KINDS[(j + 2 * o) % 7]) for o in range(2) for j, i in enumerate(at)]


# the seed of the class 1 / 2 cube of every length: chosen so that no float64 oracle coefficient of its TOUCHED columns
# lies within HARD_MARGIN of a threshold, for the three noise forms (tests/test_lines_values_cpu.py asserts it); the
# untouched columns are compared between two runs of the engine, which decide on the same bits
CUBE_SEEDS = {5: 7, 16: 8, 17: 8, 256: 173, 300: 18}


def clean_cube(N, I, dtype):
    """(2, N, I): seeded normal times 3 plus 10, the signals along axis 1"""
    rng = np.random.default_rng([CUBE_SEEDS[N], N])
    return (rng.standard_normal((2, N, I)) * 3.0 + 10.0).astype(dtype)


def cube_levels(N, I):
    """(2, I) noise levels, one per signal of the cube, one of them zero"""
    levels = np.abs(np.random.default_rng([8, N]).standard_normal((2, I))) / 8 + 0.1
    levels[0, 1] = 0
    return levels


def mixed_cube(clean, cols):
    a = clean.copy()
    for o, i, kind in cols:
        a[o, :, i] = spoil(clean[o, :, i], kind)
    return a


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam,ofam", FAMS)
def test_along_with_non_finite_columns(W, monkeypatch, fam, ofam, dtype):
    from wavelets_amd import along as A
    from wavelets_amd import signals as S
    from wavelets_amd import _lib as L
    from oracle import atrous_numpy as O
    cls = getattr(W, fam)
    no_loop(monkeypatch, A, "transform_signals", "denoise_signals")          # the axis engine, not the transposed route
    level = 3
    for N in LENGTHS:
        I, cols = bad_columns(N, dtype)
        assert {k for _, _, k in cols} == set(KINDS)
        clean = clean_cube(N, I, dtype)
        a = mixed_cube(clean, cols)
        touched = {o * I + i: kind for o, i, kind in cols}
        sig = np.ascontiguousarray(np.moveaxis(a, 1, -1)).reshape(-1, N)
        assert A.along_eligible(a, level, cls, axis=1)

        def column(res, s):                        # signal s = o * I + i of an (..., 2, N, I) result
            return res[..., s // I, :, s % I]
        follows_the_loop(lambda: W.transform_along(a, level, cls, axis=1), lambda s: S._transform_one(sig[s], level, cls),
                         W.transform_along(clean, level, cls, axis=1), 2 * I, touched, f"transform_along {fam} N={N}", column)
        got = W.transform_along(a, level, cls, axis=1)
        for s, kind in touched.items():
            if kind in NAN_ONLY:
                mask = np.isnan(O.atrous_standard_1d(sig[s].astype(np.float64), level, ofam))
                np.testing.assert_array_equal(np.isnan(column(got, s)), mask, err_msg=f"NaN mask {fam} N={N} {kind}")
        levels = cube_levels(N, I)
        for noise in (None, 1.25, levels):
            for soft in (True, False):
                per = list(levels.reshape(-1)) if isinstance(noise, np.ndarray) else [noise] * (2 * I)
                ref = W.denoise_along(clean, WEIGHTS, cls, axis=1, noise=noise, soft_threshold=soft)
                follows_the_loop(lambda: W.denoise_along(a, WEIGHTS, cls, axis=1, noise=noise, soft_threshold=soft),
                                 lambda s: W.denoise(sig[s], WEIGHTS, cls, per[s], soft_threshold=soft),
                                 ref, 2 * I, touched, f"denoise_along {fam} N={N} noise={type(noise).__name__} soft={soft}", column)
        # the medians through the binding: the neighbours of a bad column keep their bits, a bad column gets the rank rule's
        meds = []
        for block in (clean, a):
            ab = L.acquire_along(L.default_context(), 2 * I, N, getattr(L, fam.upper()), 2, dtype, planes=False)
            try:
                ab.upload(block)
                meds.append(ab.abs_median().reshape(-1))
            finally:
                L.release_along(ab)
        w0 = np.ascontiguousarray(np.moveaxis(got[0], 1, -1)).reshape(-1, N)
        for s in range(2 * I):
            if s in touched:
                np.testing.assert_array_equal(meds[1][s], rank_median(w0[s]), err_msg=f"median {fam} N={N} {touched[s]}")
            else:
                np.testing.assert_array_equal(meds[1][s], meds[0][s], err_msg=f"median of untouched column {s} {fam} N={N}")


# ---------------------------------------------------------------- class 3: the exact median against numpy

MEDIAN_KINDS = ("random", "quantised", "alternating", "zeros", "outlier", "flat")
MEDIAN_LENGTHS = (1, 2, 5, 16, 17, 255, 256, 257, 300)


def median_rows(N, dtype, seed=0):
    """one row per kind of MEDIAN_KINDS: (6, N)"""
    rng = np.random.default_rng([seed, N])
    x = rng.standard_normal((6, N)) * 3.0 + 10.0
    x[1] = np.round(x[1])                                          # integers: runs of ties straddle the median rank
    x[2] = np.where(np.arange(N) % 2 == 0, 2.5, -2.5)              # |w_0| of few distinct values
    x[3] = np.where(np.arange(N) % 3 == 0, -0.0, 0.0)
    x[4, N // 3] = 1e30 if np.dtype(dtype) == np.float32 else 1e300
    x[5] = 7.25
    return x.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", [f for f, _ in FAMS])
def test_signal_medians_equal_numpy(W, fam, dtype):
    from wavelets_amd import _lib as L
    budget = 8192 if dtype == np.float32 else 4096
    for N in MEDIAN_LENGTHS + (budget,):
        sig = median_rows(N, dtype, seed=3)
        sb = L.acquire_signals(L.default_context(), 6, N, getattr(L, fam.upper()), 1, dtype)
        try:
            sb.upload(sig)
            sb.decompose(6, 1)
            w0 = sb.download_planes(6)[:, 0]
            med = sb.abs_median(6)
        finally:
            L.release_signals(sb)
        assert w0.dtype == dtype and med.dtype == dtype
        np.testing.assert_array_equal(med, np.median(np.abs(w0), axis=-1), err_msg=f"{fam} N={N} {MEDIAN_KINDS}")
        assert med[5] == 0 and med[3] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", [f for f, _ in FAMS])
def test_along_medians_equal_numpy(W, fam, dtype):
    from wavelets_amd import _lib as L
    cls = getattr(W, fam)
    for N in MEDIAN_LENGTHS + (512,):
        a = np.ascontiguousarray(np.stack([median_rows(N, dtype, seed=4 + o) for o in range(2)]).transpose(0, 2, 1))   # (2, N, 6)
        w0 = W.transform_along(a, 1, cls, axis=1)[0]
        ab = L.acquire_along(L.default_context(), 12, N, getattr(L, fam.upper()), 1, dtype, planes=False)
        try:
            ab.upload(a)
            med = ab.abs_median()
        finally:
            L.release_along(ab)
        assert med.shape == (2, 6) and med.dtype == dtype and w0.dtype == dtype
        np.testing.assert_array_equal(med, np.median(np.abs(w0), axis=1), err_msg=f"{fam} N={N} {MEDIAN_KINDS}")


# ---------------------------------------------------------------- class 4: scaling by powers of two

@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", [f for f, _ in FAMS])
def test_scaling_by_a_power_of_two_scales_the_results_exactly(W, monkeypatch, fam, dtype):
    """the transform and the MAD-thresholded denoise hold only products, quotients and comparisons of scaled quantities:
    while everything stays normal, a * 2^k gives the bits of the result of a, times 2^k.  No reference takes part."""
    from wavelets_amd import along as A
    from wavelets_amd import signals as S
    cls = getattr(W, fam)
    no_loop(monkeypatch, S, "_transform_one", "denoise")
    no_loop(monkeypatch, A, "transform_signals", "denoise_signals")
    k = 40 if dtype == np.float32 else 400
    for N in (17, 300):
        sig = clean_stack(4, N, dtype, seed=40 + N)
        cube = np.ascontiguousarray(clean_stack(38, N, dtype, seed=41 + N).reshape(2, 19, N).transpose(0, 2, 1))   # (2, N, 19)
        t_sig, t_cube = W.transform_signals(sig, 3, cls), W.transform_along(cube, 3, cls, axis=1)
        d_sig = {soft: W.denoise_signals(sig, WEIGHTS, cls, soft_threshold=soft) for soft in (True, False)}
        d_cube = {soft: W.denoise_along(cube, WEIGHTS, cls, axis=1, soft_threshold=soft) for soft in (True, False)}
        for kk in (k, -k):
            s = dtype(2.0) ** kk
            assert np.isfinite(s) and s > 0 and np.all(np.isfinite(sig * s))
            np.testing.assert_array_equal(W.transform_signals(sig * s, 3, cls), t_sig * s, err_msg=f"{fam} N={N} k={kk}")
            np.testing.assert_array_equal(W.transform_along(cube * s, 3, cls, axis=1), t_cube * s, err_msg=f"{fam} N={N} k={kk}")
            for soft in (True, False):
                np.testing.assert_array_equal(W.denoise_signals(sig * s, WEIGHTS, cls, soft_threshold=soft), d_sig[soft] * s,
                                              err_msg=f"denoise_signals {fam} N={N} k={kk} soft={soft}")
                np.testing.assert_array_equal(W.denoise_along(cube * s, WEIGHTS, cls, axis=1, soft_threshold=soft), d_cube[soft] * s,
                                              err_msg=f"denoise_along {fam} N={N} k={kk} soft={soft}")


@pytest.mark.parametrize("fam", [f for f, _ in FAMS])
def test_denormal_float32_stacks_equal_the_loop(W, monkeypatch, fam):
    """a stack scaled into the float32 denormals (* 2^-140): the engines (their per-signal fallbacks made an error)
    against the per-signal calls, bit for bit; no oracle is consulted in this range"""
    from wavelets_amd import along as A
    from wavelets_amd import signals as S
    cls = getattr(W, fam)
    no_loop(monkeypatch, S, "_transform_one", "denoise")
    no_loop(monkeypatch, A, "transform_signals", "denoise_signals")
    for N in (17, 300):
        sig = clean_stack(4, N, np.float32, seed=50 + N) * np.float32(2.0 ** -140)
        assert np.all(sig != 0) and np.abs(sig).max() < np.finfo(np.float32).tiny
        np.testing.assert_array_equal(W.transform_signals(sig, 3, cls), np.stack([W.AtrousTransform(cls)(s, 3).data for s in sig]))
        cube = np.ascontiguousarray(sig.T.reshape(N, 2, 2).transpose(1, 0, 2))           # (2, N, 2): signal o * 2 + i is sig[...]
        cols = np.ascontiguousarray(np.moveaxis(cube, 1, -1)).reshape(-1, N)
        assert S.signals_eligible(sig, 3, cls) and A.along_eligible(cube, 3, cls, axis=1)
        t = W.transform_along(cube, 3, cls, axis=1)
        for j, col in enumerate(cols):
            np.testing.assert_array_equal(t[:, j // 2, :, j % 2], W.AtrousTransform(cls)(col, 3).data)
        for soft in (True, False):
            np.testing.assert_array_equal(W.denoise_signals(sig, WEIGHTS, cls, soft_threshold=soft),
                                          np.stack([W.denoise(s, WEIGHTS, cls, soft_threshold=soft) for s in sig]))
            d = W.denoise_along(cube, WEIGHTS, cls, axis=1, soft_threshold=soft)
            for j, col in enumerate(cols):
                np.testing.assert_array_equal(d[j // 2, :, j % 2], W.denoise(col, WEIGHTS, cls, soft_threshold=soft))


# ---------------------------------------------------------------- class 5: wow on a pedestal

def pedestal(M, N, dtype, seed=0, level=1e4):
    return (level + np.random.default_rng([seed, N]).standard_normal((M, N))).astype(dtype)


# (pedestal, N): 1e4 at both lengths, and at N = 300 the pedestals below it down to where the one-pass variance of the
# last plane is safe again - the rule that takes the standard deviation from the samples (utils._STD_CANCELS) must hold
# the bounds on both of its sides and at the change between them, not at one pedestal
PEDESTALS = ((1e4, 300), (1e4, "budget"), (3e3, 300), (1e3, 300), (3e2, 300), (1e2, 300), (30.0, 300), (10.0, 300), (3.0, 300),
             (1.0, 300), (0.3, 300))
# the oracle rule is asserted from this pedestal up, where both routes take the standard deviation from the same
# samples and so lie equally far from the oracle.  Below it (variance above _STD_CANCELS of the mean square) each
# route keeps its own one-pass value, a few ulps from the oracle either way: "twice the loop's error" is then a coin
# toss between two errors of 1e-15 of max|ref|, so there the errors are printed and the routes held to each other
ORACLE_RULE_FROM = 3.0


@pytest.mark.parametrize("level,N", PEDESTALS)
@pytest.mark.parametrize("fam,ofam", FAMS)
@pytest.mark.parametrize("dtype", TW.DTYPES)
def test_wow_on_a_pedestal(W, monkeypatch, dtype, fam, ofam, level, N):
    """unit noise on a pedestal: the variance of the smooth last plane is 1e-2 (pedestal 0.3) down to 1e-12 (pedestal
    1e4) of its mean square, and with whitening that plane is divided by its standard deviation.  The engine against
    the loop at F32_WOW / F64_WOW and against the float64 oracle with the rule of tests/test_gpu_wow_signals.py.  The
    two routes hold bit-identical planes and fold {sum, sumsq} in different orders: sumsq / N - mean^2 of those sums
    alone keeps neither bound at the higher pedestals."""
    from oracle import atrous_numpy as O
    N = TW._n(N, dtype)
    cls = getattr(W, fam)
    sig = pedestal(2, N, dtype, seed=9, level=level)
    eps = float(np.finfo(dtype).eps)
    bound = TW.F32_WOW if dtype == "float32" else TW.F64_WOW
    for name, case in TW.WHITE_CASES.items():
        kw = dict(case, scaling_function=cls)
        img = TW._engine(W, monkeypatch, sig, **kw)
        ref_img = TW._loop(W, sig, None, kw)[0]
        okw = {k: (list(v) if isinstance(v, list) else v) for k, v in case.items()}
        orc = np.stack([O.wow(s.astype(np.float64), ofam, **okw)[0] for s in sig])
        d_loop = float(np.abs(img.astype(np.float64) - ref_img).max())
        e_eng, e_loop = float(np.abs(img - orc).max()), float(np.abs(ref_img - orc).max())
        top, floor = float(np.abs(ref_img).max()), 4 * eps * float(np.abs(orc).max())
        print(f"{dtype} {fam} pedestal {level:g} N={N} {name}: |engine-loop| {d_loop:.3e} (bound {bound * top:.3e}), |engine-oracle| {e_eng:.3e}, "
              f"|loop-oracle| {e_loop:.3e}, floor {floor:.3e}")
        assert d_loop <= bound * top, name
        if level >= ORACLE_RULE_FROM:
            assert e_eng <= max(2 * e_loop, floor), name


@pytest.mark.parametrize("N", (300, "budget"))
@pytest.mark.parametrize("dtype", TW.DTYPES)
def test_moments_on_a_pedestal(W, dtype, N):
    from wavelets_amd import _lib as L
    N = TW._n(N, dtype)
    sig = pedestal(2, N, dtype, seed=10)
    sb = L.acquire_signals(L.default_context(), 2, N, L.B3SPLINE, 2, np.dtype(dtype))
    try:
        sb.upload(sig)
        sb.decompose(2, 2)
        planes = sb.download_planes(2).astype(np.float64)
        mom = sb.moments(2)
    finally:
        L.release_signals(sb)
    u = 2.0 * N * 2.0 ** -53
    err_s = np.abs(mom[..., 0] - planes.sum(axis=-1))
    err_q = np.abs(mom[..., 1] - (planes * planes).sum(axis=-1))
    print(f"{dtype} N={N}: sum error {err_s.max():.3e}, sumsq error {err_q.max():.3e}")
    assert np.all(err_s <= u * np.abs(planes).sum(axis=-1))
    assert np.all(err_q <= u * (planes * planes).sum(axis=-1))


# ---------------------------------------------------------------- class 6: wow with bad rows

def along_engine(W, monkeypatch, a, **kw):
    """wow_along with the per-signal loop an error (it goes through wow_signals)"""
    def boom(*a, **k):
        raise AssertionError("wow_along ran the per-signal loop")
    with monkeypatch.context() as m:
        m.setattr(TW._mod(), "wow", boom)
        return W.wow_along(a, **kw)


def wow_outcome(f):
    try:
        return f()
    except Exception as e:                                  # noqa: BLE001 (the class is what is compared)
        return e


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("fam", [f for f, _ in FAMS])
def test_wow_with_non_finite_rows(W, monkeypatch, fam, dtype):
    cls = getattr(W, fam)
    bound = TW.F32_WOW if dtype == np.float32 else TW.F64_WOW
    plain = dict(scaling_function=cls, whitening=False, preserve_variance=False, denoise_coefficients=[5, 2])
    white = dict(scaling_function=cls, preserve_variance=True, denoise_coefficients=[5, 2])
    for N in (16, 17, 300):
        clean = clean_stack(8, N, dtype, seed=60 + N)
        clean_plain = TW._engine(W, monkeypatch, clean, **plain)
        clean_white = TW._engine(W, monkeypatch, clean, **white)
        for mix in MIXES:
            a = mixed_stack(clean, mix)
            for soft in (True, False):
                kw = dict(plain, soft_threshold=soft)
                ref = clean_plain if soft else TW._engine(W, monkeypatch, clean, **kw)
                loop = {i: wow_outcome(lambda i=i: W.wow(a[i], **kw)[0]) for i in mix}
                got = wow_outcome(lambda: TW._engine(W, monkeypatch, a, **kw))
                failed = [i for i in mix if isinstance(loop[i], Exception)]
                if failed:
                    assert type(got) is type(loop[failed[0]]), (got, loop[failed[0]])
                    continue
                assert not isinstance(got, Exception), got
                for i in range(8):
                    np.testing.assert_array_equal(got[i], loop[i] if i in mix else ref[i], err_msg=f"{fam} N={N} row {i} {mix.get(i)}")
                # wow_along of the same signals as the columns of an (N, 8) array
                along = wow_outcome(lambda: along_engine(W, monkeypatch, np.ascontiguousarray(a.T), axis=0, **kw))
                assert not isinstance(along, Exception), along
                np.testing.assert_array_equal(along, got.T)
            loop = {i: wow_outcome(lambda i=i: W.wow(a[i], **white)[0]) for i in mix}
            got = wow_outcome(lambda: TW._engine(W, monkeypatch, a, **white))
            failed = [i for i in mix if isinstance(loop[i], Exception)]
            if failed:
                assert type(got) is type(loop[failed[0]]), (got, loop[failed[0]])
                continue
            assert not isinstance(got, Exception), got
            for i in range(8):
                if i not in mix:
                    np.testing.assert_array_equal(got[i], clean_white[i], err_msg=f"moments: {fam} N={N} untouched row {i}")
                    continue
                nan = np.isnan(loop[i])
                np.testing.assert_array_equal(np.isnan(got[i]), nan, err_msg=f"moments: NaN mask {fam} N={N} {mix[i]}")
                keep = ~nan & np.isfinite(loop[i])
                np.testing.assert_array_equal(got[i][~nan & ~keep], loop[i][~nan & ~keep])          # (infinities: equal)
                if keep.any():
                    err = float(np.abs(got[i][keep].astype(np.float64) - loop[i][keep]).max())
                    assert err <= bound * float(np.abs(loop[i][keep]).max()), (fam, N, mix[i], err)
            along = along_engine(W, monkeypatch, np.ascontiguousarray(a.T), axis=0, **white)
            np.testing.assert_array_equal(along, got.T)
