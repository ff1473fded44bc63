"""The float32 cube engine (wavelets_amd.cubes, wt_decompose_cube) on the GPU: bit identity with AtrousTransform at the
shapes where the fused kernel can go wrong, with the per-scale choice left to the host and forced each way
(WT_CUBE_FUSED), the numpy oracle's golden cubes, denoise_cube against utils.denoise, the Coefficients object, the
fallbacks, and the plane contract on a reused plan."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FAMS = ("b3spline", "triangle")
# (shape, level): one slice (every z tap reflects onto it); one row; one column; d = 4 > Z (multi-bounce on every
# axis); nothing a multiple of anything; across the 256-column workgroup and the float4 tail; d = 8 with chains of
# 4 - 5 steps; level 0
CASES = (((1, 4, 9), 2), ((5, 1, 6), 2), ((8, 9, 1), 2), ((3, 5, 7), 3), ((17, 19, 23), 3), ((12, 10, 258), 2),
         ((33, 20, 130), 4), ((17, 19, 23), 0))
MODES = (None, "1", "0")          # the host's per-scale rule, the fused kernel at every scale, the old sequence


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


def cls_of(W, fam):
    return {"b3spline": W.B3spline, "triangle": W.Triangle}[fam]


def cube(shape, seed=0):
    return (np.random.default_rng(seed).standard_normal(shape) * 3 + 50).astype(np.float32)      # (pedestal 50)


_REF = {}


def reference(W, shape, level, fam):
    """AtrousTransform's planes of cube(shape), computed once and left unchanged"""
    key = (shape, level, fam)
    if key not in _REF:
        ref = W.AtrousTransform(cls_of(W, fam))(cube(shape), level).data.copy()
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "rule" if m is None else "fused" + m)
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape,level", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"L{v}")
def test_bit_identity_with_atrous_transform(W, monkeypatch, shape, level, fam, mode):
    ref = reference(W, shape, level, fam)
    if mode is None:
        monkeypatch.delenv("WT_CUBE_FUSED", raising=False)
    else:
        monkeypatch.setenv("WT_CUBE_FUSED", mode)
    c = W.transform_cube(cube(shape), level, cls_of(W, fam))
    assert c.data.shape == (level + 1,) + shape and c.data.dtype == np.float32
    assert np.array_equal(c.data, ref)


def test_golden_cubes_against_the_numpy_oracle(W):
    g = load_golden("g12_3d")
    for tag in ("12x10x14", "5x33x20"):
        a = np.asarray(g[f"cube_{tag}"], np.float32)
        tol = 1e-5 * np.abs(a).max()
        for fam in FAMS:
            for L in (1, 3):
                assert W.cube_eligible(a, L, cls_of(W, fam))
                c = W.transform_cube(a, L, cls_of(W, fam))
                assert c.data.shape == (L + 1,) + a.shape
                np.testing.assert_allclose(np.asarray(c.data, np.float64), g[f"coef_{fam}_{tag}_L{L}"], rtol=0, atol=tol)
                np.testing.assert_allclose(np.asarray(np.sum(c, axis=0), np.float64), a, rtol=0, atol=2 * tol)


@pytest.mark.parametrize("shape", ((17, 19, 23), (12, 10, 258)), ids=lambda s: "x".join(map(str, s)))
def test_denoise_cube_equals_denoise(W, shape):
    a = cube(shape, 3)
    for kw in ({}, {"noise": 2.5}, {"soft_threshold": False}):
        got = W.denoise_cube(a, [5, 3], **kw)
        assert got.dtype == np.float32 and np.array_equal(got, W.denoise(a, [5, 3], **kw)), kw
    counts = np.random.default_rng(4).poisson(30.0, shape).astype(np.float32)
    assert np.array_equal(W.denoise_cube(counts, [5, 3], anscombe=True), W.denoise(counts, [5, 3], anscombe=True))
    assert np.array_equal(W.denoise_cube(a, [4, 2], W.Triangle), W.denoise(a, [4, 2], W.Triangle))


def test_result_is_a_working_coefficients_object(W):
    a = cube((17, 19, 23), 5)
    new, old = W.transform_cube(a, 3), W.AtrousTransform(W.B3spline)(a, 3)
    assert type(new) is type(old) and len(new) == len(old) == 4 and new.shape == old.shape
    assert new.get_noise() == old.get_noise()
    for c in (new, old):
        c.data[1] *= 2                   # the host mirror is the caller's: the next device operation takes it back
        c.denoise([3, 3])
    assert np.array_equal(new.data, old.data)
    assert np.array_equal(np.sum(new, axis=0), np.sum(old, axis=0))


def test_fallbacks_return_the_host_functions_results(W):
    class Seventeen(W.B3spline):
        coefficients_1d = np.hanning(19)[1:-1] / np.hanning(19)[1:-1].sum()

    a = cube((6, 7, 9), 6)
    a64 = a.astype(np.float64)
    assert not W.cube_eligible(a64, 2) and not W.cube_eligible(a, 2, Seventeen)
    c = W.transform_cube(a64, 2)
    assert c.data.dtype == np.float64 and np.array_equal(c.data, W.AtrousTransform(W.B3spline)(a64, 2).data)
    c = W.transform_cube(a, 2, Seventeen)
    assert np.array_equal(c.data, W.AtrousTransform(Seventeen)(a, 2).data)
    got = W.denoise_cube(a64, [5, 3])
    assert got.dtype == np.float64 and np.array_equal(got, W.denoise(a64, [5, 3]))
    assert np.array_equal(W.denoise_cube(a, [5, 3], Seventeen), W.denoise(a, [5, 3], Seventeen))
    # bilateral cubes are not the engine's: the predicate says so and the host function serves them
    assert not W.cube_eligible(a, 2, bilateral=1)
    assert W.AtrousTransform(W.B3spline, bilateral=1)(a, 2).data.shape == (3,) + a.shape


def test_src_survives_and_a_reused_plan_repeats_its_bits(W, monkeypatch):
    from wavelets_amd import _lib as L
    monkeypatch.setenv("WT_CUBE_FUSED", "1")
    Z, Y, X = 9, 11, 261
    a = cube((Z, Y, X), 7).reshape(Z * Y, X)
    plan = L.Plan(L.default_context(), Z * Y, X, L.B3SPLINE, 3)
    try:
        plan.upload(L.PLANE_INPUT, a)
        plan.decompose_cube(L.PLANE_INPUT, 3, Z)
        first = [plan.download(s).copy() for s in range(4)]
        assert np.array_equal(plan.download(L.PLANE_INPUT), a)
        plan.decompose_cube(L.PLANE_INPUT, 3, Z)
        assert all(np.array_equal(plan.download(s), first[s]) for s in range(4))
        plan.decompose3d(L.PLANE_INPUT, 3, Z)
        assert all(np.array_equal(plan.download(s), first[s]) for s in range(4))
        assert np.array_equal(plan.download(L.PLANE_INPUT), a)
        with pytest.raises(L.WatrooHipError, match="not a multiple of depth"):
            plan.decompose_cube(L.PLANE_INPUT, 3, 7)
        with pytest.raises(L.WatrooHipError, match="exceeds plan max_level"):
            plan.decompose_cube(L.PLANE_INPUT, 4, Z)
        plan.set_border(1)
        with pytest.raises(L.WatrooHipError, match="symmetric border"):
            plan.decompose_cube(L.PLANE_INPUT, 3, Z)
        plan.set_border(0)
    finally:
        plan.close()
