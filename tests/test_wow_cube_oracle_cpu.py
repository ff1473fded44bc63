"""What tests/test_gpu_wow_cube_oracle.py rests on, checked without a device: the chunk, row-group and x-block layouts
its edge shapes are claimed to hit, from the arithmetic of cube_geometry_t (wt_cubes_host.h) for either element type;
the margin of its hard-threshold inputs; the oracle's NaN masks against the reach of the transform plus the power; the
corner-block rule of its streaming cubes, noise map and gamma accumulator included; and the normal range of the float32
squares under its scalings."""
import numpy as np
import pytest

from oracle import atrous_numpy as O
import test_gpu_wow_cube_oracle as T
from test_gpu_cubes_oracle import EDGE_CASES, FAMS, HW, NAN_ONLY, KINDS, VALUE_SHAPES, bad_sample, spoil, tag_of
from test_gpu_wow_cube import OPTION_SHAPES, OPTIONS, cube

K = {"b3spline": 5, "triangle": 3}
TY = 8                                # WT_CUBE_TY (wt_cubes_kernels.h)
XBLOCK = {"float32": 256, "float64": 128}      # columns of a workgroup: 64 lanes x a float4 / double2 group


# --------------------------------------------------------------------------- layouts of wt_cube_wow_kernel
def layout(shape, s, taps, cus, dtype):
    """cube_geometry_t of wt_cubes_host.h in Python: scale s of a (Z, Y, X) cube of `dtype` on a device of `cus` compute
    units.  This records the assumption the edge cases are chosen under; it is not a search of the library."""
    Z, Y, X = shape
    d = 1 << s
    ycls, zcls = min(d, Y), min(d, Z)
    ny, nz = -(-Y // d), -(-Z // d)
    gx = -(-X // XBLOCK[dtype])
    have = gx * ycls * -(-ny // TY) * zcls
    chunks = max(1, min(nz, -(-(cus * 8) // have)))
    S = min(nz, max(-(-nz // chunks), 4 * (taps - 1)))
    return {"d": d, "ycls": ycls, "zcls": zcls, "rows": [min(TY, ny - r) for r in range(0, ny, TY)],
            "steps": [min(S, nz - t) for t in range(0, nz, S)], "xblocks": gx, "tail": X - (gx - 1) * XBLOCK[dtype],
            "nt": Z * Y * X * np.dtype(dtype).itemsize >= 32 << 20}


def test_the_layouts_the_edge_cases_name():
    cases = {(s, "float32"): l for s, l in EDGE_CASES}
    cases.update({(s, "float64"): l for s, l in T.EDGE_CASES64 + T.DEEP_CASES})
    assert set(T.DEEP_CASES) <= set(EDGE_CASES)
    assert set((s, l, dt) for (s, dt), l in cases.items()) == set(T.A_CASES)
    for cus in range(3, 513):
        def lay(shape, dtype, s=0, fam="b3spline"):
            assert s < cases[shape, dtype]
            return layout(shape, s, K[fam], cus, dtype)
        # float32: chunks of the z chains at s = 0 (S = 4 (K - 1)), row groups, the 256-column seam
        assert [lay((Z, 9, 12), "float32")["steps"] for Z in (16, 17, 32, 33)] == [[16], [16, 1], [16, 16], [16, 16, 1]]
        assert [lay((Z, 9, 12), "float32", 0, "triangle")["steps"] for Z in (8, 9, 16, 17)] == [[8], [8, 1], [8, 8], [8, 8, 1]]
        assert [lay((20, Y, 7), "float32")["rows"] for Y in (8, 9, 16)] == [[8], [8, 1], [8, 8]]
        assert [(v["xblocks"], v["tail"]) for v in (lay((5, 4, X), "float32") for X in (256, 257, 260))] == [(1, 256), (2, 1), (2, 4)]
        v = lay((2, 3, 261), "float32")
        assert (v["xblocks"], v["tail"]) == (2, 5)
        # d >= Y > 1 from s = 3 with up to 64-fold reach on 5 rows; d >= Z > 1 with d < Y
        for s in range(3, 6):
            v = lay((6, 5, 9), "float32", s)
            assert v["ycls"] == 5 and v["rows"] == [1] and v["steps"] == [1] and v["d"] >= 6
        for s in (2, 3, 4):
            v = lay((3, 17, 5), "float32", s)
            assert v["zcls"] == 3 and v["steps"] == [1] and v["d"] < 17
        # float64: the 128-column seam - one block; one column; a double2 group; a group and a one-element tail
        assert [(v["xblocks"], v["tail"]) for v in (lay((5, 4, X), "float64") for X in (128, 129, 130))] == [(1, 128), (2, 1), (2, 2)]
        v = lay((2, 3, 131), "float64")
        assert (v["xblocks"], v["tail"]) == (2, 3) and [lay((2, 3, 131), "float64", s)["zcls"] for s in range(5)] == [1, 2, 2, 2, 2]
        # B: (33, 20, 130) float64 - 3 chunks at s = 0 and 2 at s = 1 (wow's own rule gives it 2 scales)
        assert layout((33, 20, 130), 0, 5, cus, "float64")["steps"] == [16, 16, 1]
        assert layout((33, 20, 130), 1, 5, cus, "float64")["steps"] == [16, 1]
        # C: streaming stores on, and on no other shape of the file
        for dtype, shape in T.STREAM_SHAPES.items():
            assert all(layout(shape, s, 5, cus, dtype)["nt"] for s in range(T.STREAM_LEVEL))
        if cus > 16:
            assert layout(T.STREAM_SHAPES["float32"], 0, 5, cus, "float32")["steps"] == [16, 16]
        assert layout(T.STREAM_SHAPES["float64"], 0, 5, cus, "float64")["steps"] == [16]
        assert not any(layout(s, 0, 5, cus, dt)["nt"] for s, _, dt in T.A_CASES)
    for dtype, (Z, Y, X) in T.STREAM_SHAPES.items():
        assert Z * Y * X * np.dtype(dtype).itemsize == 32 << 20     # (the pitch is at least X: a.nt of cube_geometry_t is set)
    for shape in OPTION_SHAPES:                                     # the level of B's arrays under wow's own rule
        assert O.wow_n_scales(shape, "b3spline", None, 0, [5, 2], None) == 2
        assert O.wow_n_scales(shape, "triangle", None, 0, [5, 2], None) >= 2


# --------------------------------------------------------------------------- hard-threshold margins
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=tag_of)
def test_hard_threshold_inputs_keep_clear_of_their_thresholds(shape):
    """no coefficient of the float64 oracle within 1e-4 relative of its threshold, on the float32 samples and on the
    float64 samples: the rounding of either engine (1e-6 relative at worst) cannot flip a sample, and the noise is given,
    so the GPU test allows none.  The seeds tried are listed at HARD_SEEDS; the first ones are re-tried here."""
    assert T.HARD_MARGIN == 1e-4 and OPTIONS["hard"] == dict(denoise_coefficients=[5, 2], noise=2.5, soft_threshold=False)
    seed = T.HARD_SEEDS[shape]
    for dtype in ("float32", "float64"):
        assert T.hard_margin(O, shape, dtype, seed) > T.HARD_MARGIN
    assert T.hard_margin(O, shape, "float32", T.B_SEED) < T.HARD_MARGIN          # (why the seed of the other options is not used)
    if shape == (33, 20, 130):
        assert max(T.hard_margin(O, shape, "float32", s) for s in range(8)) < T.HARD_MARGIN


# --------------------------------------------------------------------------- NaN masks
wow_reach_masks = T.wow_reach_masks            # (np.pad dilations: no index arithmetic shared with the oracle)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape", VALUE_SHAPES, ids=tag_of)
def test_oracle_nan_masks_are_the_reach_of_transform_and_power(shape, fam):
    clean = cube(shape, "float32", 1)
    L = T.VALUE_LEVEL
    for kind in KINDS:
        image, planes, _ = T.oracle_wow(O, spoil(clean, kind), fam, L)
        mask = np.isnan(planes[:L])
        assert np.isnan(planes[L]).all() and np.isnan(image).all()           # np.std of a plane that holds a NaN
        spot = bad_sample(shape, kind)
        if spot is None:
            assert mask.all()
        elif kind in NAN_ONLY:
            assert np.array_equal(mask, wow_reach_masks(shape, spot[0], HW[fam], L)), kind
        else:         # an inf sample: w_s is inf - inf at the sample's reach and -+inf around it; NaN within the same cube
            assert mask.any() and not (mask & ~wow_reach_masks(shape, spot[0], HW[fam], L)).any(), kind


# --------------------------------------------------------------------------- the corner-block rule
@pytest.mark.parametrize("form", T.STREAM_FORMS)
def test_corner_block_detail_planes_are_the_whole_cubes(form):
    """the wow-updated detail planes of a[:, :48, :48] are those of the whole cube where the cut is out of reach: 6
    samples for the transform at level 2 plus 4 for the power of scale 1, so on [:, :38, :38] - and not on [:, :39, :39]"""
    fam, L, B = "b3spline", T.STREAM_LEVEL, T.BLOCK
    reach = HW[fam] * (2 ** L - 1) + HW[fam] * 2 ** (L - 1)
    assert (B, L, reach) == (48, 2, 10) and T.INNER == B - reach == 38
    shape = (8, 96, 96)
    a = cube(shape, "float64", 9)
    nmap = (np.random.default_rng(9).random(shape) + 0.5) * 2

    def run(blk):
        noise, kw = T.stream_form(form, "float64")
        assert (form == "plain") == (not isinstance(noise, np.ndarray))
        if form != "plain":
            assert kw["gamma_min"] is not None and kw["gamma_max"] is not None and 0 < kw["h"] < 1
            noise = nmap[:, blk, blk]
        return T.oracle_wow(O, a[:, blk, blk], fam, L, noise, **kw)[1][:L]
    whole = run(slice(None))
    first, last = run(slice(None, B)), run(slice(-B, None))
    I = T.INNER
    assert np.array_equal(first[:, :, :I, :I], whole[:, :, :I, :I])
    assert np.array_equal(last[:, :, -I:, -I:], whole[:, :, -I:, -I:])
    assert not np.array_equal(first[:, :, :I + 1, :I + 1], whole[:, :, :I + 1, :I + 1])      # (the rule is sharp)
    assert not np.array_equal(last[:, :, -I - 1:, -I - 1:], whole[:, :, -I - 1:, -I - 1:])


# --------------------------------------------------------------------------- the normal range of the scalings
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape", VALUE_SHAPES, ids=tag_of)
def test_float32_squares_stay_normal_under_the_scalings(shape, fam):
    """for k = +-20, +-40 every detail coefficient of the oracle, its square and the local power of the squares are
    normal float32 numbers (so is the input); for k = -70 every square is a denormal of a few bits or zero and for k = 62 the
    largest ones exceed the float32 maximum - the range in which the oracle is not the reference"""
    f = np.finfo(np.float32)
    base = cube(shape, "float32", 2)
    planes = O.atrous_standard_3d(base.astype(np.float64), T.VALUE_LEVEL, fam)[:T.VALUE_LEVEL]
    assert np.all(planes != 0)
    lo, hi = float(np.abs(planes).min()), float(np.abs(planes).max())
    assert set(T.SCALINGS) == {20, -20, 40, -40}
    for k in T.SCALINGS:
        s = 2.0 ** k
        assert f.tiny < (lo * s) ** 2 and (hi * s) ** 2 < f.max and f.tiny < float(np.abs(base).min()) * s
        assert float(np.abs(base).max()) * s < f.max
    assert (hi * 2.0 ** -70) ** 2 < f.tiny / 32 and (hi * 2.0 ** 62) ** 2 > f.max
    assert np.all(np.isfinite(base * np.float32(2.0 ** 62))) and np.all(base * np.float32(2.0 ** -70) != 0)
