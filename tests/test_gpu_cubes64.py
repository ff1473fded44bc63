"""The float64 cube engine (wavelets_amd.cubes on float64 and integer cubes, wt64_decompose_cube) on the GPU: bit
identity with AtrousTransform at the shapes where the fused kernel can go wrong, with the per-scale choice left to the
host and forced each way (WT_CUBE_FUSED); the element types the reference recasts to float64, uploaded as they are; the
profile scope of the new kernel; the float64 numpy oracle; denoise_cube against utils.denoise; the Coefficients object;
and the plane contract on a raw Plan64 with poisoned planes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMS = ("b3spline", "triangle")
# (shape, level): one slice; one row; one column (the straddling double2 group is the only group); d = 4 > Z
# (multi-bounce on every axis); nothing a multiple of anything, odd W; across the 128-column workgroup seam with an even
# W and with an odd tail; d = 8 with chains of 4 - 5 steps; level 0; 65537 row groups (an 8 MB plane): the grid of the
# fused kernel does not fit and the default rule itself falls back; RULE_SHAPE: the default rule takes the fused kernel
# at every scale (the small cubes go to smooth64 under it: their fused bits are those of WT_CUBE_FUSED=1)
RULE_SHAPE = (4, 512, 512)
CASES = (((1, 4, 9), 2), ((5, 1, 6), 2), ((8, 9, 1), 2), ((3, 5, 7), 3), ((17, 19, 23), 3), ((12, 10, 130), 2),
         ((12, 10, 129), 2), ((33, 20, 66), 4), ((17, 19, 23), 0), ((1, 524296, 2), 1), (RULE_SHAPE, 3))
MODES = (None, "1", "0")          # the host's per-scale rule, the fused kernel wherever its grid fits, smooth64
F64_PLANES = 1e-13                # the project's float64 plane bound (tests/test_gpu_nd_edges.py), times max|input|
SCOPE = "wt_cube_scale_kernel64"
RULE_AND_FUSED = (None, "1")      # (cubes this small go to smooth64 under the rule: the fused kernel's bits need the switch)
B3 = "b3spline"


@pytest.fixture(scope="module")
def W():
    import __graft_entry__ as entry
    entry.build()
    import wavelets_amd
    return wavelets_amd


def cls_of(W, fam):
    return {"b3spline": W.B3spline, "triangle": W.Triangle}[fam]


def cube(shape, seed=0):
    """cube() of test_gpu_cubes.py, in float64"""
    return (np.random.default_rng(seed).standard_normal(shape) * 3 + 50).astype(np.float64)      # (pedestal 50)


def typed(shape, dt, seed=1):
    """a cube of element type dt: counts for the integer types, the float64 cube cast for the big-endian floats"""
    if np.dtype(dt).kind in "iu":
        return np.random.default_rng(seed).integers(0, 4000, shape).astype(dt)
    return cube(shape, seed).astype(dt)


_REF = {}


def reference(W, shape, level, fam):
    """AtrousTransform's planes of cube(shape), computed once and left unchanged"""
    key = (shape, level, fam)
    if key not in _REF:
        ref = W.AtrousTransform(cls_of(W, fam))(cube(shape), level).data.copy()
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("WT_CUBE_FUSED", raising=False)
    else:
        monkeypatch.setenv("WT_CUBE_FUSED", mode)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "rule" if m is None else "fused" + m)
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape,level", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"L{v}")
def test_bit_identity_with_atrous_transform(W, monkeypatch, shape, level, fam, mode):
    ref = reference(W, shape, level, fam)
    set_mode(monkeypatch, mode)
    assert W.cube64_eligible(cube(shape), level, cls_of(W, fam))
    c = W.transform_cube(cube(shape), level, cls_of(W, fam))
    assert c.data.shape == (level + 1,) + shape and c.data.dtype == np.float64
    assert np.array_equal(c.data, ref)


@pytest.mark.parametrize("shape", ((17, 19, 23), (12, 10, 129)), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ("int16", "uint16", "int32", ">i2", ">f4", ">f8"))
def test_element_types(W, monkeypatch, shape, dt):
    x = typed(shape, dt)
    ref = W.AtrousTransform(W.B3spline)(x, 3)
    # every type the reference recasts to float64 (ref wavelets.py:297) runs on the float64 engine; a big-endian int16
    # is not among them (native 'int16' only) and stays a float32 cube, for AtrousTransform as for transform_cube
    want = np.float32 if dt == ">i2" else np.float64
    assert W.cube64_eligible(x, 3) is (dt != ">i2")
    for mode in RULE_AND_FUSED:
        set_mode(monkeypatch, mode)
        c = W.transform_cube(x, 3)
        assert c.data.dtype == ref.data.dtype == want, mode
        assert np.array_equal(c.data, ref.data), mode


def test_non_contiguous_int16_view(W, monkeypatch):
    x = typed((17, 19, 46), "int16")[:, :, ::2]
    assert not x.flags.c_contiguous and W.cube64_eligible(x, 3)
    ref = W.AtrousTransform(W.B3spline)(x, 3).data
    for mode in RULE_AND_FUSED:
        set_mode(monkeypatch, mode)
        c = W.transform_cube(x, 3)
        assert c.data.dtype == np.float64 and np.array_equal(c.data, ref), mode


def test_the_fused_kernel_ran(W, monkeypatch):
    """The measured per-scale rule (WT_CUBE64_MIN_VOXELS_PER_STEP) sends cubes of a few thousand
    voxels to smooth64, where three launches are faster than the march: at (17, 19, 23) the kernel's scope is counted
    with the fused kernel forced, and the default rule is counted at RULE_SHAPE, the smallest cube of the table's kind
    (one million voxels, an 8 MB plane) where it takes the fused kernel at all three scales."""
    from wavelets_amd import _lib as L
    ctx = L.default_context()

    def calls(a, mode):
        set_mode(monkeypatch, mode)
        ctx.profile_reset()
        W.transform_cube(a, 3).data
        return ctx.profile_entries().get(SCOPE, (0, 0.0))[0]

    small, big = cube((17, 19, 23), 2), cube(RULE_SHAPE, 2)
    ctx.profile(True)
    try:
        assert calls(big, None) == 3
        assert calls(big, "0") == 0
        assert calls(small, "1") == 3
        assert calls(small, "0") == 0
        assert calls(small, None) == 0
    finally:
        ctx.profile(False)
        ctx.profile_reset()


@pytest.mark.parametrize("shape", ((17, 19, 23), (12, 10, 129)), ids=lambda s: "x".join(map(str, s)))
def test_planes_against_the_float64_oracle(W, monkeypatch, shape):
    from oracle import atrous_numpy as O
    monkeypatch.setenv("WT_CUBE_FUSED", "1")
    a = cube(shape, 8)
    bound = F64_PLANES * np.abs(a).max()
    for fam in FAMS:
        c = W.transform_cube(a, 3, cls_of(W, fam))
        ref = O.atrous_standard_3d(a.copy(), 3, fam)
        err = np.abs(c.data - ref).max()
        tele = np.abs(np.sum(c.data, axis=0) - a).max()
        print(f"{shape} {fam}: planes {err:.3e} telescoping {tele:.3e} bound {bound:.3e}")
        assert c.data.dtype == np.float64 and err <= bound and tele <= bound


@pytest.mark.parametrize("shape", ((17, 19, 23), (12, 10, 129)), ids=lambda s: "x".join(map(str, s)))
def test_denoise_cube_equals_denoise(W, monkeypatch, shape):
    counts = np.random.default_rng(4).poisson(30.0, shape).astype(np.int32)
    sets = [(a, B3, [5, 3], kw) for a in (cube(shape, 3), typed(shape, "int16", 3))
            for kw in ({}, {"noise": 2.5}, {"soft_threshold": False})]
    sets += [(a, "triangle", [4, 2], {}) for a in (cube(shape, 3), typed(shape, "int16", 3))]
    sets += [(counts, B3, [5, 3], {"anscombe": True})]
    for a, fam, weights, kw in sets:
        want = W.denoise(a, weights, cls_of(W, fam), **kw)
        for mode in RULE_AND_FUSED:
            set_mode(monkeypatch, mode)
            got = W.denoise_cube(a, weights, cls_of(W, fam), **kw)
            assert got.dtype == np.float64 and np.array_equal(got, want), (a.dtype, fam, kw, mode)


def test_result_is_a_working_coefficients_object(W, monkeypatch):
    monkeypatch.setenv("WT_CUBE_FUSED", "1")
    a = cube((17, 19, 23), 5)
    new, old = W.transform_cube(a, 3), W.AtrousTransform(W.B3spline)(a, 3)
    assert type(new) is type(old) and len(new) == len(old) == 4 and new.shape == old.shape
    assert new.get_noise() == old.get_noise()
    for c in (new, old):
        c.data[1] *= 2                   # the host mirror is the caller's: the next device operation takes it back
        c.denoise([3, 3])
    assert new.data.dtype == np.float64 and np.array_equal(new.data, old.data)
    assert np.array_equal(np.sum(new, axis=0), np.sum(old, axis=0))


def test_plane_contract_on_a_raw_plan64(W, monkeypatch):
    from wavelets_amd import _lib as L
    monkeypatch.setenv("WT_CUBE_FUSED", "1")
    Z, Y, X = 9, 11, 261
    a = cube((Z, Y, X), 7).reshape(Z * Y, X)
    b3 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
    plan = L.Plan64(L.default_context(), Z * Y, X, b3, 3)
    try:
        plan.upload(L.PLANE_INPUT, a)
        for pl in (0, 1, 2, 3, L.PLANE_SCRATCH(0), L.PLANE_SCRATCH(1)):
            plan.fill(pl, float("nan"))
        plan.decompose_cube(L.PLANE_INPUT, 3, Z)
        first = [plan.download(s).copy() for s in range(4)]
        assert not any(np.isnan(p).any() for p in first)
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
        with pytest.raises(L.WatrooHipError, match="one of the output planes"):
            plan.decompose_cube(2, 3, Z)
        with pytest.raises(L.WatrooHipError, match="scratch planes 0/1 are used internally"):
            plan.decompose_cube(L.PLANE_SCRATCH(1), 3, Z)
        plan.set_border(1)
        with pytest.raises(L.WatrooHipError, match="symmetric border"):
            plan.decompose_cube(L.PLANE_INPUT, 3, Z)
        plan.set_border(0)
    finally:
        plan.close()
    # user-defined taps: a float64 plan holds at most 15 (17 are refused when the plan is made), and the cube entry
    # refuses every plan whose taps are not a built-in family's
    with pytest.raises(L.WatrooHipError, match="17 taps unsupported"):
        L.Plan64(L.default_context(), Z * Y, X, tuple(np.ones(17) / 17), 3)
    for taps in (tuple(np.ones(15) / 15), (1 / 9, 2 / 9, 3 / 9, 2 / 9, 1 / 9)):
        user = L.Plan64(L.default_context(), Z * Y, X, taps, 3)
        try:
            user.upload(L.PLANE_INPUT, a)
            with pytest.raises(L.WatrooHipError, match="built-in scaling functions only"):
                user.decompose_cube(L.PLANE_INPUT, 3, Z)
        finally:
            user.close()
