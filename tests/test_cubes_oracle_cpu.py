"""What tests/test_gpu_cubes_oracle.py rests on, checked without a device: the seeds of its hard-threshold inputs keep
clear of their thresholds; the float64 oracle's NaN masks are the cube of the filter's reach; the planes of a corner
block are those of the whole cube away from the cut; and the chunk, row-group and x-block layouts its edge cases name
follow from the arithmetic of cube_geometry (wt_cubes.hip) for any number of compute units."""
import numpy as np
import pytest

from oracle import atrous_numpy as O
import test_gpu_cubes_oracle as T
from test_gpu_cubes import FAMS, cube

K = {"b3spline": 5, "triangle": 3}


# --------------------------------------------------------------------------- hard-threshold margins
# the best margin among the seeds 0 .. 11 of cube(shape, seed): (seed, margin to two digits)
BEST = {((17, 19, 23), "b3spline"): (3, 1.2e-2), ((17, 19, 23), "triangle"): (11, 5.8e-3),
        ((6, 5, 9), "b3spline"): (11, 3.0e-2), ((6, 5, 9), "triangle"): (10, 3.6e-2),
        ((12, 10, 258), "b3spline"): (11, 3.6e-4), ((12, 10, 258), "triangle"): (2, 7.9e-4)}


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape", T.DENOISE_SHAPES, ids=T.tag_of)
def test_hard_threshold_seeds_keep_clear_of_their_thresholds(shape, fam):
    """no coefficient of the float64 oracle within 1e-4 relative of its threshold: the rounding of the engine (1e-6
    relative at worst, in the coefficient and in the MAD estimate alike) cannot flip a sample, so the GPU test allows none"""
    assert T.HARD_MARGIN == 1e-4 and T.HARD_ALLOW == 0 and T.WEIGHTS == [5, 3]
    assert set(T.HARD_SEEDS) == {(s, f) for s in T.DENOISE_SHAPES for f in FAMS} == set(BEST)
    margins = [T.hard_margin(O, shape, fam, seed) for seed in range(12)]
    seed, best = BEST[shape, fam]
    assert int(np.argmax(margins)) == seed == T.HARD_SEEDS[shape, fam]
    assert abs(margins[seed] - best) <= 0.05 * best
    assert margins[seed] > T.HARD_MARGIN


# --------------------------------------------------------------------------- NaN masks
def reach_1d(n, at, hw, level):
    """the samples of an axis of n that a NaN at index `at` reaches in the smooth planes c_1 .. c_level: boolean dilation
    by the taps at distance j * 2^s under np.pad's symmetric border (no index arithmetic shared with the oracle)"""
    cur = np.zeros(n, bool)
    cur[at] = True
    out = []
    for s in range(level):
        d = 2 ** s
        padded = np.pad(cur, hw * d, mode="symmetric")
        nxt = np.zeros(n, bool)
        for j in range(2 * hw + 1):
            nxt |= padded[j * d:j * d + n]
        out.append(nxt)
        cur = nxt
    return out


def reach_masks(shape, at, hw, level):
    """NaN masks of the level + 1 planes: w_s = c_s - c_{s+1} is NaN where c_{s+1} is (its set holds that of c_s: the
    centre tap is not zero), and the separable filter keeps the set a product of its three axes"""
    axes = [reach_1d(n, i, hw, level) for n, i in zip(shape, at)]
    planes = [axes[0][s][:, None, None] & axes[1][s][None, :, None] & axes[2][s][None, None, :] for s in range(level)]
    return np.stack(planes + [planes[-1]])


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape", T.VALUE_SHAPES, ids=T.tag_of)
def test_oracle_nan_masks_are_the_cube_of_the_reach(shape, fam):
    clean = cube(shape, 1)
    for kind in T.NAN_ONLY:
        mask = np.isnan(T.oracle_planes(O, T.spoil(clean, kind), T.VALUE_LEVEL, fam))
        spot = T.bad_sample(shape, kind)
        if spot is None:
            assert mask.all()
            continue
        assert np.isnan(spot[1])
        assert np.array_equal(mask, reach_masks(shape, spot[0], T.HW[fam], T.VALUE_LEVEL)), kind
    for kind in set(T.KINDS) - set(T.NAN_ONLY):
        assert np.isinf(T.bad_sample(shape, kind)[1])
    sites = {T.bad_sample(shape, k)[0] for k in T.KINDS if k != "all_nan"}
    Z, Y, X = shape
    assert sites == {(0, 0, 0), (0, Y // 2, X // 2), (Z // 2, Y // 2, X // 2), (Z - 1, Y - 1, X - 1)}


def test_nan_counts_of_a_corner_sample():
    mask = reach_masks((9, 11, 13), (0, 0, 0), 2, 2)
    assert [int(m.sum()) for m in mask] == [27, 343, 343]
    a = T.spoil(cube((9, 11, 13), 1), "nan_corner")
    assert np.array_equal(np.isnan(T.oracle_planes(O, a, 2, "b3spline")), mask)


# --------------------------------------------------------------------------- the corner-block rule
@pytest.mark.parametrize("fam", FAMS)
def test_corner_block_planes_are_the_whole_cubes_planes(fam):
    """the planes of a[:, :48, :48] are those of the whole cube where the cut is out of reach (2 + 4 samples at level 2
    for B3spline), true borders and the whole z axis included: the same float64 operations on the same samples"""
    a = cube((8, 96, 96), 9)
    B, I, L = T.BLOCK, T.INNER, T.STREAM_LEVEL
    assert (B, I, L) == (48, 40, 2) and T.STREAM_SHAPE == (32, 512, 512)
    reach = T.HW[fam] * (2 ** L - 1)
    assert I <= B - reach
    whole = T.oracle_planes(O, a, L, fam)
    first = T.oracle_planes(O, a[:, :B, :B], L, fam)
    last = T.oracle_planes(O, a[:, -B:, -B:], L, fam)
    for keep in (I, B - reach):
        assert np.array_equal(first[:, :, :keep, :keep], whole[:, :, :keep, :keep])
        assert np.array_equal(last[:, :, -keep:, -keep:], whole[:, :, -keep:, -keep:])
    # (the rule is sharp: one sample nearer to the cut the block differs)
    assert not np.array_equal(first[L, :, :B - reach + 1, :B - reach + 1], whole[L, :, :B - reach + 1, :B - reach + 1])


# --------------------------------------------------------------------------- layouts of the fused kernel
TY, XBLOCK = 8, 256                   # WT_CUBE_TY, columns of a workgroup (wt_cubes_kernels.h)


def layout(shape, s, taps, cus):
    """cube_geometry of wt_cubes.hip in Python: the geometry of scale s of a (Z, Y, X) cube on a device of `cus` compute
    units.  This records the assumption the edge cases are chosen under; it is not a search of the library."""
    Z, Y, X = shape
    d = 1 << s
    ycls, zcls = min(d, Y), min(d, Z)
    ny, nz = -(-Y // d), -(-Z // d)                      # longest row class / z chain
    gx = -(-X // XBLOCK)
    groups = -(-ny // TY)
    have = gx * ycls * groups * zcls
    chunks = max(1, min(nz, -(-(cus * 8) // have)))
    S = min(nz, max(-(-nz // chunks), 4 * (taps - 1)))
    return {"d": d, "ycls": ycls, "zcls": zcls, "rows": [min(TY, ny - r) for r in range(0, ny, TY)],
            "steps": [min(S, nz - t) for t in range(0, nz, S)], "xblocks": gx, "tail": X - (gx - 1) * XBLOCK}


def test_the_layouts_the_edge_cases_name():
    cases = dict(T.EDGE_CASES)
    for cus in range(1, 513):
        def steps(shape, fam, s=0):
            assert shape in cases and s < cases[shape]
            return layout(shape, s, K[fam], cus)["steps"]
        # chunks of the z chains at s = 0: S = 4 (K - 1)
        assert [steps((Z, 9, 12), "b3spline") for Z in (16, 17, 32, 33)] == [[16], [16, 1], [16, 16], [16, 16, 1]]
        assert [steps((Z, 9, 12), "triangle") for Z in (8, 9, 16, 17)] == [[8], [8, 1], [8, 8], [8, 8, 1]]
        # row groups, x blocks
        assert [layout((20, Y, 7), 0, 5, cus)["rows"] for Y in (8, 9, 16)] == [[8], [8, 1], [8, 8]]
        assert [(lay["xblocks"], lay["tail"]) for lay in (layout((5, 4, X), 0, 5, cus) for X in (256, 257, 260, 261))] == \
            [(1, 256), (2, 1), (2, 4), (2, 5)]
        # d >= Y > 1: one row per class from s = 3 on, up to 64-fold reach (2 * 32) on 5 rows; d >= Z > 1 with d < Y
        for s in range(3, cases[(6, 5, 9)]):
            lay = layout((6, 5, 9), s, 5, cus)
            assert lay["ycls"] == 5 and lay["rows"] == [1] and lay["d"] >= 5
        assert 2 * layout((6, 5, 9), 5, 5, cus)["d"] == 64 and cases[(6, 5, 9)] == 6
        for s in (2, 3, 4):
            lay = layout((3, 17, 5), s, 5, cus)
            assert lay["zcls"] == 3 and lay["steps"] == [1] and lay["d"] < 17
        assert cases[(3, 17, 5)] == 5
        # the streaming cube: two chunks of 16 at s = 0 once the device has more workgroups to fill than the grid has
        lay = layout(T.STREAM_SHAPE, 0, 5, cus)
        assert lay["steps"] == ([16, 16] if cus > 16 else [32]) and layout(T.STREAM_SHAPE, 1, 5, cus)["steps"] == [16]
    Z, Y, X = T.STREAM_SHAPE
    assert Z * Y * X * 4 == 32 << 20          # (the pitch is at least X: streaming stores are on, a.nt of cube_geometry)
