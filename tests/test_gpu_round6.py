"""Round-6 GPU tests: fast addressing of the fused passes at any width (float64 side), sequences of frames through the
double-buffered batch entry points, replicas."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as entry
    entry.build()
    from wavelets_amd import _lib
    if _lib.device_count() == 0:
        pytest.skip("no GPU")
    return _lib


@pytest.mark.parametrize("H,W,fam,level", [(130, 261, "b3spline", 6), (301, 1001, "b3spline", 6), (700, 1101, "b3spline", 6),
                                           (90, 129, "triangle", 4), (600, 533, "triangle", 8), (64, 51, "b3spline", 2)])
def test_float64_fused_fast_addressing_at_odd_widths_is_bitwise_the_generic_one(L, H, W, fam, level):
    """wt_fused_kernel<double>: a lane owns two pixels, so an odd width leaves one pair that straddles the right border
    ((g0, g0) after the swizzle) and reversed pairs beyond it; the fast addressing must write the bits of the generic
    (gather) addressing - planes, carried sum, and the plain decomposition."""
    import wavelets_amd as WA
    cls = {"b3spline": WA.B3spline, "triangle": WA.Triangle}[fam]
    a = np.random.default_rng(H * 7 + W).standard_normal((H, W)) * 3 + 1e3
    plan = L.Plan64(L.default_context(), H, W, tuple(float(t) for t in cls.coefficients_1d), level)
    plan.upload(L.PLANE_INPUT, a)
    got = {}
    try:
        for mode in (1, 0):
            L.set_option("fused_fast", mode)
            assert plan.decompose_sum(L.PLANE_INPUT, level, L.PLANE_OUT)
            out = [plan.download(s).copy() for s in range(level + 1)] + [plan.download(L.PLANE_OUT).copy()]
            plan.decompose(L.PLANE_INPUT, level)
            got[mode] = out + [plan.download(s).copy() for s in range(level + 1)]
    finally:
        L.set_option("fused_fast", 1)
    for i, (x, y) in enumerate(zip(got[1], got[0])):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64), err_msg=f"output {i}")
    plan.close()


# --------------------------------------------------------------------------- sequences of frames / channels
GOLD = os.path.join(ROOT, "tests", "golden")


def _rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_denoise_many_is_bitwise_the_per_call_api_and_keeps_the_order(L):
    """16 frames (each different) through sequence.denoise_many on 3 lanes == denoise() frame by frame, bit for bit,
    in input order; a generator as input; per-frame noise values; float64 and integer frames too."""
    import wavelets_amd as W
    frames = [_rnd((300, 517), 100 + i) * (1 + i) + i for i in range(16)]
    ref = [W.denoise(f, [5, 3]) for f in frames]
    got = W.denoise_many((f for f in frames), [5, 3])
    assert len(got) == 16
    for i in range(16):
        np.testing.assert_array_equal(got[i].view(np.uint32), ref[i].view(np.uint32), err_msg=f"frame {i}")
    noise = [0.5 + 0.1 * i for i in range(16)]
    ref = [W.denoise(f, [4, 2, 1], W.Triangle, n, soft_threshold=False) for f, n in zip(frames, noise)]
    got = W.denoise_many(frames, [4, 2, 1], W.Triangle, noise, soft_threshold=False, lanes=4)
    for i in range(16):
        np.testing.assert_array_equal(got[i].view(np.uint32), ref[i].view(np.uint32), err_msg=f"frame {i} (given noise)")
    f64 = [f.astype(np.float64) * 10 + 1e3 for f in frames[:5]] + [(f * 50).astype(np.int16) for f in frames[5:8]]
    ref = [W.denoise(f, [5, 3]) for f in f64]
    got = W.denoise_many(f64, [5, 3], lanes=2)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype == np.float64
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=f"float64 frame {i}")
    # a preallocated target, one lane (the plain loop), and an exception inside a lane
    out = np.empty((16, 300, 517), np.float32)
    assert W.denoise_many(frames, [5, 3], out=out, lanes=1) is out
    np.testing.assert_array_equal(out[7].view(np.uint32), W.denoise(frames[7], [5, 3]).view(np.uint32))
    with pytest.raises(ValueError, match="Unsupported number of dimensions"):
        W.denoise_many(frames[:3] + [np.ones((2, 2, 2, 2), np.float32)] + frames[3:], [5, 3])


def test_sequences_vs_reference_golden_g2_and_wow(L):
    """the reference-generated denoise fixtures (g2) through denoise_many, wow through wow_many (g4's first case),
    transform_many == AtrousTransform per frame (device-resident Coefficients from three lanes)."""
    import wavelets_amd as W
    g2 = np.load(os.path.join(GOLD, "g2_denoise.npz"))
    img = g2["img"]
    frames = [img, img[::-1].copy(), img[:, ::-1].copy(), img.T.copy()]
    got = W.denoise_many(frames, [5, 3])
    for a, f in zip(got, frames):
        np.testing.assert_array_equal(a, W.denoise(f, [5, 3]))
    assert float(np.abs(got[0] - g2["denoise_53_b3spline"]).max()) <= 4e-5 * float(np.abs(img).max())
    w_ref = [W.wow(f, denoise_coefficients=[5, 2])[0] for f in frames]
    w_got = W.wow_many(frames, denoise_coefficients=[5, 2])
    for a, b in zip(w_got, w_ref):
        np.testing.assert_array_equal(a[0], b)
    cs = W.transform_many(frames, 4, W.Triangle)
    for c, f in zip(cs, frames):
        np.testing.assert_array_equal(c.data, W.AtrousTransform(W.Triangle)(f, 4).data)


def test_enhance_channels_through_the_lanes_vs_golden_g10(L):
    """enhance() on a (3, H, W) image runs its three channels on three lanes (ref utils.py:60-78 is a loop): the
    reference-generated g10 fixtures hold, and each channel equals the 2-D call on that channel bit for bit."""
    from wavelets_amd.utils import enhance
    g = np.load(os.path.join(GOLD, "g10_enhance.npz"))
    rgb = g["rgb"]
    tol = 4e-5 * float(np.abs(g["img"]).max())
    assert float(np.abs(enhance(rgb.copy(), weights=[[.5, 2], [1], [2, 2, 1]], denoise=[[3], [4, 2], None]) - g["enh_rgb"]).max()) <= tol
    got = enhance(rgb, weights=[[1.5, 1.2, 1.0]] * 3, denoise=[[3, 2]] * 3)
    for c in range(3):
        np.testing.assert_array_equal(got[c], enhance(rgb[c], weights=[1.5, 1.2, 1.0], denoise=[3, 2]), err_msg=f"channel {c}")
    # a colour image large enough for the lanes (>= 1 Mpixel per channel): three lanes, downloads straight into `out`
    big = _rnd((3, 1100, 1024), 9) * 3 + 7
    got = enhance(big, weights=[[1.5, 1.2, 1.0]] * 3, denoise=[[3, 2]] * 3)
    for c in range(3):
        np.testing.assert_array_equal(got[c], enhance(big[c], weights=[1.5, 1.2, 1.0], denoise=[3, 2]), err_msg=f"big channel {c}")
    mine = np.full((3, 1100, 1024), np.nan, np.float32)
    assert enhance(big, weights=[[1.5, 1.2, 1.0]] * 3, denoise=[[3, 2]] * 3, out=mine) is mine
    np.testing.assert_array_equal(mine, got)
    # per-channel lists (ref:19-33) and a given noise per channel
    got = enhance(rgb, [0.3, 0.2, 0.1], weights=[[1, 2], [1.5], [2, 1, 1]], denoise=[[3], [2, 1], []])
    for c, (w, d) in enumerate(zip([[1, 2], [1.5], [2, 1, 1]], [[3], [2, 1], []])):
        np.testing.assert_array_equal(got[c], enhance(rgb[c], [0.3, 0.2, 0.1][c], weights=list(w), denoise=list(d)), err_msg=f"channel {c}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bilateral_transform_propagates_nan_like_the_reference(L, dtype):
    """A NaN sample reaches every coefficient whose dilated neighbourhood (or local variance) holds it, exactly where the
    numpy oracle's does (the float64 march clamps the exponent argument - weights never fall below k_t 2^-64 -, but a
    NaN neighbour still enters through value x weight and a NaN centre through k_c I); everything else stays finite
    and within the bilateral tolerance."""
    from oracle import atrous_numpy as O
    import wavelets_amd as W
    a = (np.random.default_rng(3).standard_normal((96, 130)) * 2 + 10).astype(dtype)
    a[40, 77] = np.nan
    got = W.AtrousTransform(W.B3spline, bilateral=1)(a, 3).data
    ref = O.atrous_standard(a, 3, "b3spline", bilateral=1)
    assert got.dtype == dtype
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    tol = (1e-11 if dtype == np.float64 else 2e-5) * float(np.nanmax(np.abs(a)))
    assert float(np.abs(got[ok] - ref[ok]).max()) <= tol


def test_failed_allreduce_surfaces_and_leaves_the_context_usable(tmp_path):
    """The all-reduced scalars of a strip (wt_reduce's moments, the MAD median's histograms - Coefficients.get_noise and
    wow's np.std / min / max on N GPUs) over the stand-in RCCL (tests/stubs/rccl_stub.c) with the n-th ncclAllReduce
    failing: the call raises RCCL's error naming the entry point, nothing hangs, and the SAME calls succeed right
    afterwards on the same context and plan (no marker, scratch buffer or side-stream state is left behind)."""
    import subprocess
    import textwrap
    so = tmp_path / "librccl_stub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-o", str(so), os.path.join(ROOT, "tests", "stubs", "rccl_stub.c")])
    script = textwrap.dedent(f'''
        import ctypes, os, sys
        import numpy as np
        sys.path.insert(0, {ROOT!r})
        from wavelets_amd import _lib as L
        ctx = L.Context(0)
        assert L.comm_version() == 29999
        stub = ctypes.CDLL(os.environ["WATROO_HIP_RCCL_LIB"])
        ctx.comm_init(0, 2, L.Context.unique_id())
        plan = L.Plan(ctx, 256, 320, L.B3SPLINE, 2, row0=0, nrows=128, halo_rows=16, rank=0, nranks=2)
        a = np.random.default_rng(0).standard_normal((128, 320), dtype=np.float32)
        plan.upload(L.PLANE_INPUT, a)
        def failing(call, what):
            os.environ["RCCL_STUB_FAIL_ALLREDUCE"] = str(stub.rccl_stub_allreduces() + 1)
            try:
                call()
            except L.WatrooHipError as e:
                assert "RCCL error 3" in str(e) and "AllReduce" in str(e) and ("wt_" in str(e) or "select_pass" in str(e)), str(e)
            else:
                raise SystemExit(what + ": the failing all-reduce did not raise")
            finally:
                os.environ["RCCL_STUB_FAIL_ALLREDUCE"] = "0"
        failing(lambda: plan.reduce(L.PLANE_INPUT), "wt_reduce")
        s, s2, lo, hi = plan.reduce(L.PLANE_INPUT)              # the stub moves nothing: this rank's own moments
        assert abs(s - float(a.astype(np.float64).sum())) < 1e-6 * a.size and lo == float(a.min()) and hi == float(a.max())
        failing(lambda: plan.abs_median(L.PLANE_INPUT), "wt_abs_median")
        # (the stub adds nobody's bins: a strip's median over the GLOBAL count cannot succeed with it - what must work
        #  afterwards is everything that shares the context's select state and histogram words)
        whole = L.Plan(ctx, 128, 320, L.B3SPLINE, 2)
        whole.upload(L.PLANE_INPUT, a)
        assert whole.abs_median(L.PLANE_INPUT) == float(np.median(np.abs(a)))
        # a transform whose first pass rode the histogram, a median whose all-reduce fails, then the same on the
        # unsharded plan: the riding-histogram marker of the failed call must not leak into it
        plan.decompose(L.PLANE_INPUT, 2, L.FLAG_FUSED | L.FLAG_MEDIAN_HIST | L.FLAG_NO_EXCHANGE)
        failing(lambda: plan.abs_median(0), "wt_abs_median")
        whole.decompose(L.PLANE_INPUT, 2, L.FLAG_FUSED | L.FLAG_MEDIAN_HIST)
        assert whole.abs_median(0) == float(np.median(np.abs(whole.download(0))))
        s, s2, lo, hi = plan.reduce(L.PLANE_INPUT)
        assert lo == float(a.min()) and hi == float(a.max())
        whole.close()
        plan.close()
        print("OK", stub.rccl_stub_allreduces())
    ''')
    env = dict(os.environ, WATROO_HIP_RCCL_LIB=str(so), RCCL_STUB_NRANKS="2")
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_float64_wow_bilateral_vs_oracle_at_a_megapixel(L):
    """BASELINE configs[4] in the reference's default dtype at 1024 x 1536 (8 scales: dilations up to 128, every
    kernel of the float64 cfg5 flow - bilateral march, fused wow updates on row AND lattice kernels, windowed exact
    median, early plane sum - at a size the numpy oracle still finishes in seconds): image and whitened planes at
    1e-11 of their maximum.  (Round 5 checked this path against the oracle at 256 x 320 only; the full 8192^2 size is
    property-checked in test_gpu_round5.py.)"""
    import wavelets_amd as WA
    from oracle import atrous_numpy as O
    rng = np.random.default_rng(11)
    img = rng.standard_normal((1024, 1536)) + 3 * np.sin(np.arange(1536) / 50.0)[None, :] + 10.0
    rec, co = WA.wow(img.copy(), bilateral=1, denoise_coefficients=[5, 2])
    rref, cref = O.wow(img.copy(), "b3spline", bilateral=1, denoise_coefficients=[5, 2])
    assert rec.dtype == np.float64 and co.data.shape == cref.data.shape == (9, 1024, 1536)
    assert float(np.abs(rec - rref).max()) <= 1e-11 * float(np.abs(rref).max())
    for s in range(9):
        assert float(np.abs(co.data[s] - cref.data[s]).max()) <= 1e-11 * float(np.abs(cref.data).max()), f"plane {s}"
    assert abs(co.noise - cref.noise) <= 1e-12 * abs(cref.noise)


def test_denoise_many_downloads_straight_into_a_preallocated_cube(L):
    """`out=` as an (N, H, W) array of the result dtype: every frame's download lands in its rows (no intermediate
    block, no host copy) - also through the pipelined host call (noise given, image above its size threshold) - and a
    cube of another dtype still gets the values by assignment."""
    import wavelets_amd as W
    frames = [_rnd((2304, 2048), 40 + i) for i in range(4)]
    ref = [W.denoise(f, [5, 3]) for f in frames]
    out = np.full((4, 2304, 2048), np.nan, np.float32)
    assert W.denoise_many(frames, [5, 3], out=out) is out
    for i in range(4):
        np.testing.assert_array_equal(out[i].view(np.uint32), ref[i].view(np.uint32))
    refn = [W.denoise(f, [5, 3], noise=1.0) for f in frames]            # 4.7 Mpixel: the pipelined host call
    out[...] = np.nan
    W.denoise_many(frames, [5, 3], noise=1.0, out=out, lanes=2)
    for i in range(4):
        np.testing.assert_array_equal(out[i].view(np.uint32), refn[i].view(np.uint32))
    out64 = np.zeros((4, 2304, 2048), np.float64)
    W.denoise_many(frames, [5, 3], out=out64)
    np.testing.assert_array_equal(out64[2], ref[2].astype(np.float64))
    view = np.zeros((4, 2304, 4096), np.float32)[:, :, ::2]            # rows not contiguous: falls back to assignment
    W.denoise_many(frames, [5, 3], out=view)
    np.testing.assert_array_equal(view[1], ref[1])


def test_sequences_over_a_device_list(L):
    """devices=[0] / "all" (one GPU here): the lanes of every listed GPU take frames from one queue; same bits, same order."""
    import wavelets_amd as W
    frames = [_rnd((200, 333), 70 + i) for i in range(9)]
    ref = [W.denoise(f, [5, 3]) for f in frames]
    for devs in ([0], "all"):
        got = W.denoise_many(frames, [5, 3], lanes=2, devices=devs)
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_lanes_shared_by_concurrent_callers(L):
    """Three host threads call denoise_many / wow_many / transform_many at the same time: they share the lanes' contexts
    (calls on one context are serialised by its lock, plans are taken from the pool one caller at a time) - every result
    still equals the per-call API bit for bit."""
    import threading
    import wavelets_amd as W
    rng = np.random.default_rng(0)
    frames = [rng.standard_normal((256, 300)).astype(np.float32) * (1 + i % 5) + i for i in range(60)]
    ref_d = [W.denoise(f, [5, 3]) for f in frames]
    ref_w = [W.wow(f, denoise_coefficients=[5, 2], bilateral=1)[0] for f in frames[:20]]
    ref_t = [W.AtrousTransform(W.Triangle)(f, 4).data.copy() for f in frames[:20]]
    bad = []

    def t1():
        for rep in range(2):
            got = W.denoise_many(frames, [5, 3], lanes=4)
            if any(not np.array_equal(a, b) for a, b in zip(got, ref_d)):
                bad.append(("denoise", rep))

    def t2():
        for rep in range(2):
            got = W.wow_many(frames[:20], lanes=3, denoise_coefficients=[5, 2], bilateral=1)
            if any(not np.array_equal(a[0], b) for a, b in zip(got, ref_w)):
                bad.append(("wow", rep))

    def t3():
        for rep in range(2):
            cs = W.transform_many(frames[:20], 4, W.Triangle, lanes=2)
            if any(not np.array_equal(c.data, r) for c, r in zip(cs, ref_t)):
                bad.append(("transform", rep))
    raised = []             # a bare Thread that raises prints a traceback and dies: the test would not see it

    def guarded(f):
        def run():
            try:
                f()
            except BaseException as e:             # noqa: BLE001 - reported on the test's thread
                raised.append((f.__name__, repr(e)))
        return run
    ts = [threading.Thread(target=guarded(f)) for f in (t1, t2, t3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not raised, f"worker threads raised: {raised}"
    assert not bad, bad
