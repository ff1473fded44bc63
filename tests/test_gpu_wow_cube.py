"""wow on (Z, Y, X) cubes through the cube engines (wavelets_amd.cubes.wow_cube, wt_wow_cube_scale /
wt64_wow_cube_scale, wt_cube_wow_kernel) on the GPU.  Every comparison is np.array_equal on the image and on
coefficients.data against the existing route, utils.wow, on the same input: the edge shapes of test_gpu_cubes.py /
test_gpu_cubes64.py with the per-scale choice left to the host and forced each way (WT_CUBE_FUSED), the options of wow
(the noise-map / gamma instantiation included), the profile scopes of the two kernels, the plane contract on a plan
whose scratch planes hold NaN, the fallbacks, and the reference's own 3-D wow results (g14_wow_denoise_nd)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FAMS = ("b3spline", "triangle")
MODES = (None, "1", "0")          # the host's per-scale rule, the fused kernels wherever their grid fits, the old sequences
# (shape, level, dtype), driven through Coefficients (wow on an array caps the scale count at these sizes): one slice;
# one row; one column; d = 4 > Z (multi-bounce on every axis); nothing a multiple of anything; float32: the 256-column
# workgroup seam and the float4 tail; float64: the 128-column seam with an even and an odd tail, d = 8 with chains of
# 4 - 5 steps
SMALL = (((1, 4, 9), 2), ((5, 1, 6), 2), ((8, 9, 1), 2), ((3, 5, 7), 3), ((17, 19, 23), 3))
EDGES = tuple((s, l, dt) for s, l in SMALL for dt in ("float32", "float64")) + \
    (((12, 10, 258), 2, "float32"), ((33, 20, 130), 4, "float64"), ((12, 10, 129), 2, "float64"))
OPTION_SHAPES = ((17, 19, 23), (33, 20, 130))
OPTIONS = {
    "defaults": dict(),
    "denoise": dict(denoise_coefficients=[5, 2], noise=2.5),
    "estimated_noise": dict(denoise_coefficients=[5, 2]),
    "hard": dict(denoise_coefficients=[5, 2], noise=2.5, soft_threshold=False),
    "variance": dict(preserve_variance=True),
    "weights": dict(weights=[0.5, 2]),
    "gamma": dict(denoise_coefficients=[4, 2], noise=2.5, h=0.5, gamma=2.5),
    "gamma_bounds": dict(denoise_coefficients=[4, 2], noise=2.5, h=0.5, gamma_min=-1.0, gamma_max=6.0),
    "noise_map": dict(denoise_coefficients=[5, 2], noise="map"),
    "noise_map_gamma": dict(denoise_coefficients=[5, 2], noise="map", h=0.5),
    "no_whitening": dict(whitening=False, denoise_coefficients=[5, 2], noise=2.5),
    "h_one": dict(h=1, denoise_coefficients=[5, 2], noise=2.5),
}


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


def cls_of(W, fam):
    return {"b3spline": W.B3spline, "triangle": W.Triangle}[fam]


def cube(shape, dtype="float32", seed=0):
    """cube() of test_gpu_cubes.py / test_gpu_cubes64.py"""
    return (np.random.default_rng(seed).standard_normal(shape) * 3 + 50).astype(dtype)      # (pedestal 50)


def set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("WT_CUBE_FUSED", raising=False)
    else:
        monkeypatch.setenv("WT_CUBE_FUSED", mode)


def options(name, shape, dtype):
    kw = {k: (list(v) if isinstance(v, list) else v) for k, v in OPTIONS[name].items()}
    if isinstance(kw.get("noise"), str):
        kw["noise"] = (np.random.default_rng(9).random(shape) + 0.5).astype(dtype) * 2
    return kw


def frozen(image, c):
    out = (np.array(image, copy=True), np.array(c.data, copy=True))
    for a in out:
        a.setflags(write=False)
    return out


def same(got, want):
    (gi, gc), (wi, wc) = got, want
    return gi.dtype == wi.dtype and gc.data.dtype == wc.dtype and np.array_equal(gi, wi) and np.array_equal(gc.data, wc)


_REF = {}


def reference(W, key, make):
    """wow's (image, coefficients.data) for `key`, computed once on the existing route and left unchanged"""
    if key not in _REF:
        _REF[key] = frozen(*make())
    return _REF[key]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "rule" if m is None else "fused" + m)
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape,level,dtype", EDGES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_edge_shapes_through_coefficients(W, monkeypatch, shape, level, dtype, fam, mode):
    sf = cls_of(W, fam)
    a = cube(shape, dtype)
    want = reference(W, (shape, level, dtype, fam), lambda: W.wow(W.AtrousTransform(sf)(a, level)))
    set_mode(monkeypatch, mode)
    c = W.transform_cube(a, level, sf)
    image, out = W.wow_cube(c)
    assert out is c and image.shape == shape and c.data.shape == (level + 1,) + shape
    assert same((image, out), want)


@pytest.mark.parametrize("mode", (None, "1"), ids=("rule", "fused1"))
@pytest.mark.parametrize("dtype", ("float32", "float64"))
@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_options_on_arrays(W, monkeypatch, shape, name, dtype, mode):
    a = cube(shape, dtype, 3)
    keep = a.copy()
    want = reference(W, (shape, name, dtype), lambda: W.wow(a, **options(name, shape, dtype)))
    set_mode(monkeypatch, mode)
    assert W.wow_cube_eligible(a)
    assert same(W.wow_cube(a, **options(name, shape, dtype)), want)
    assert np.array_equal(a, keep)                         # the input array is not modified


@pytest.mark.parametrize("mode", (None, "1"), ids=("rule", "fused1"))
@pytest.mark.parametrize("dt", ("int16", ">f4", "uint8"))
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_and_big_endian_inputs(W, monkeypatch, shape, dt, mode):
    a = np.random.default_rng(1).integers(0, 200, shape).astype(dt) if np.dtype(dt).kind in "iu" else cube(shape, dt, 1)
    kw = dict(denoise_coefficients=[5, 2], scaling_function=W.Triangle)
    want = reference(W, (shape, dt), lambda: W.wow(a, **kw))
    set_mode(monkeypatch, mode)
    got = W.wow_cube(a, **kw)
    assert got[0].dtype == (np.float32 if dt == "uint8" else np.float64)       # (result dtype as wow: ref wavelets.py:297)
    assert same(got, want)


def test_the_kernels_ran(W, monkeypatch):
    """Three scales of (17, 19, 23) record exactly 3 launches of wt_cube_wow_kernel and 3 of wt_cube_scale_kernel with
    the fused kernels forced, and none of either with the old sequences forced: a silent fallback cannot pass the bit
    tests.  (Through Coefficients: wow_cube(array, n_scales=3) is capped at 2 scales at this size, ref utils.py:122-127,
    and then records 2 and 2.)"""
    from wavelets_amd import _lib as L
    ctx = L.default_context()
    a = cube((17, 19, 23), "float32", 2)

    def calls(mode, run):
        set_mode(monkeypatch, mode)
        ctx.profile_reset()
        run()
        e = ctx.profile_entries()
        return e.get("wt_cube_wow_kernel", (0, 0.0))[0], e.get("wt_cube_scale_kernel", (0, 0.0))[0]

    ctx.profile(True)
    try:
        assert calls("1", lambda: W.wow_cube(W.transform_cube(a, 3))) == (3, 3)
        assert calls("0", lambda: W.wow_cube(W.transform_cube(a, 3))) == (0, 0)
        assert calls("1", lambda: W.wow_cube(a, n_scales=3)) == (2, 2)
        assert calls("1", lambda: W.wow_cube(a, n_scales=3, denoise_coefficients=[5, 2], h=0.5)) == (2, 2)
        assert calls("1", lambda: W.wow_cube(a, whitening=False)) == (0, 2)         # no local power: wow_update alone
        assert calls("1", lambda: W.wow(a, n_scales=3)) == (0, 0)                   # wow keeps its routing
    finally:
        ctx.profile(False)
        ctx.profile_reset()


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_plane_contract_on_poisoned_scratch_planes(W, monkeypatch, dtype):
    """One scale on a raw plan: every scratch plane (the spare of the pointer swap among them) holds NaN before each
    call; the fused kernel and the sequence it replaces leave the same plane, the gamma plane included, a second call
    on the reused plan repeats the bits, and the operands that alias internal planes are refused."""
    from wavelets_amd import _lib as L
    Z, Y, X = 9, 11, 261
    f64 = dtype == "float64"
    w = (np.random.default_rng(7).standard_normal((Z * Y, X)) * 3).astype(dtype)
    nmap = (np.random.default_rng(8).random((Z * Y, X)) + 0.5).astype(dtype)
    ctx = L.default_context()
    plan = L.Plan64(ctx, Z * Y, X, (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16), 2) if f64 else L.Plan(ctx, Z * Y, X, L.B3SPLINE, 2)
    NOISE, GAMMA = L.PLANE_SCRATCH(5), L.PLANE_SCRATCH(4)
    nan = np.full((Z * Y, X), np.nan, dtype)

    def run(mode, noise_plane, gamma_plane):
        set_mode(monkeypatch, mode)
        for i in (0, 1, 2, 3, 6, 7):
            plan.upload(L.PLANE_SCRATCH(i), nan)
        plan.upload(1, w)
        plan.upload(NOISE, nmap)
        plan.fill(GAMMA, 0.25)
        plan.wow_cube_scale(1, 1, Z, 1.5, True, noise_plane, 0.75, gamma_plane)
        return plan.download(1).copy(), plan.download(GAMMA).copy()

    try:
        for noise_plane, gamma_plane in ((L.PLANE_NONE, L.PLANE_NONE), (NOISE, L.PLANE_NONE), (L.PLANE_NONE, GAMMA), (NOISE, GAMMA)):
            fused, again, old = (run(m, noise_plane, gamma_plane) for m in ("1", "1", "0"))
            for got in (fused, again):
                assert np.isfinite(got[0]).all()
                assert np.array_equal(got[0], old[0]) and np.array_equal(got[1], old[1])
            assert bool((old[1] != 0.25).any()) == (gamma_plane != L.PLANE_NONE)
        assert np.array_equal(plan.download(NOISE), nmap)
        with pytest.raises(L.WatrooHipError, match="not a multiple of depth"):
            plan.wow_cube_scale(1, 1, 7, 1.5, True, L.PLANE_NONE, 1.0, L.PLANE_NONE)
        with pytest.raises(L.WatrooHipError, match="not a coefficient plane"):
            plan.wow_cube_scale(3, 1, Z, 1.5, True, L.PLANE_NONE, 1.0, L.PLANE_NONE)
        with pytest.raises(L.WatrooHipError, match="aliases"):
            plan.wow_cube_scale(1, 1, Z, 1.5, True, 1, 1.0, L.PLANE_NONE)
        with pytest.raises(L.WatrooHipError, match="aliases"):
            plan.wow_cube_scale(1, 1, Z, 1.5, True, L.PLANE_NONE, 1.0, L.PLANE_SCRATCH(6))
        plan.set_border(1)
        with pytest.raises(L.WatrooHipError, match="symmetric border"):
            plan.wow_cube_scale(1, 1, Z, 1.5, True, L.PLANE_NONE, 1.0, L.PLANE_NONE)
        plan.set_border(0)
    finally:
        plan.close()


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_a_second_call_on_the_reused_plan_gives_the_same_bits(W, monkeypatch, dtype):
    monkeypatch.setenv("WT_CUBE_FUSED", "1")
    a = cube((17, 19, 23), dtype, 5)
    kw = dict(denoise_coefficients=[5, 2], h=0.5)
    first = frozen(*W.wow_cube(a, **kw))          # (the Coefficients object is dropped: its plan goes back to the pool)
    assert same(W.wow_cube(a, **kw), first)
    assert same(W.wow_cube(a, **kw), frozen(*W.wow(a, **kw)))


def test_fallbacks_return_wows_result(W):
    class Seventeen(W.B3spline):
        coefficients_1d = np.hanning(19)[1:-1] / np.hanning(19)[1:-1].sum()

    class Retapped(W.B3spline):
        coefficients_1d = np.array([1, 2, 3, 2, 1]) / 9

    a = cube((17, 19, 23), "float32", 6)
    big = cube((36, 36, 36), "float32", 6)
    for sf in (Seventeen, Retapped):
        assert not W.wow_cube_eligible(a, sf)
    assert not W.wow_cube_eligible(a, bilateral=1)
    kw = dict(whitening=False, denoise_coefficients=[5], noise=2.5)
    assert same(W.wow_cube(big, Seventeen, **kw), frozen(*W.wow(big, Seventeen, **kw)))
    assert same(W.wow_cube(a, Retapped), frozen(*W.wow(a, Retapped)))
    c, c2 = (W.AtrousTransform(Retapped)(a, 2) for _ in range(2))
    assert same(W.wow_cube(c), frozen(*W.wow(c2)))
    img = cube((24, 31), "float32", 6)                     # an image: not a cube, wow serves it
    assert not W.wow_cube_eligible(img) and same(W.wow_cube(img), frozen(*W.wow(img)))
    cb, cb2 = (W.AtrousTransform(W.B3spline, bilateral=1)(a, 1) for _ in range(2))     # bilateral coefficients: wow's route
    assert same(W.wow_cube(cb), frozen(*W.wow(cb2)))
    with pytest.raises(ValueError, match="Unknown input type"):
        W.wow_cube([1, 2, 3])


def test_golden_3d_wow_cases(W, monkeypatch):
    """The reference's own wow results on a (20, 24, 28) cube, at the bound of tests/test_gpu_parity.py::
    test_wow_and_denoise_nd_vs_golden for wow (3e-5 * max|ref|), and equal to wow bit for bit"""
    g = load_golden("g14_wow_denoise_nd")
    a = g["cube"]
    cases = {"default": dict(), "den": dict(denoise_coefficients=[5, 2], n_scales=3),
             "gamma": dict(denoise_coefficients=[4, 2], n_scales=2, h=0.5, gamma=2.5),
             "pv": dict(preserve_variance=True, weights=[0.5, 2]), "tri": dict(scaling_function=W.Triangle, denoise_coefficients=[3])}
    for mode in (None, "1"):
        set_mode(monkeypatch, mode)
        for name, case in cases.items():
            kw = {k: (list(v) if isinstance(v, list) else v) for k, v in case.items()}
            r, c = W.wow_cube(a.copy(), **kw)
            ref = g[f"wow_cube_{name}"]
            tol = 3e-5 * np.abs(ref).max()
            assert r.shape == a.shape and r.dtype == np.float32
            np.testing.assert_allclose(np.asarray(r, np.float64), ref, rtol=0, atol=tol)
            if f"wow_cube_{name}_coef" in g:
                np.testing.assert_allclose(np.asarray(c.data, np.float64), g[f"wow_cube_{name}_coef"], rtol=0, atol=tol)
            assert same((r, c), frozen(*W.wow(a.copy(), **kw)))
