"""CPU only: the C oracle's single-level Lucas-Kanade solve against the exact-integer NumPy model of tests/lk_ref.py, bit for bit, on binary scenes that
drive the window sums to the largest values 8-bit images allow -- where an accumulator narrower than the oracle's int64 (the HIP kernels keep int32
partials, 16-bit halves and 24-bit multiply-adds, tests/test_gpu_lk_extremes.py) would first go wrong -- and an assertion that the scenes really get
there."""
import numpy as np
import pytest

import lk_ref as R
from lk_support import bits as _bits
from oracle import klt_oracle as KO  # noqa: E402

WINDOWS = (3, 8, 15, 16, 21, 51, 63, 64, 65, 107)


@pytest.mark.parametrize("scene", sorted(R.SCENES))
@pytest.mark.parametrize("win", WINDOWS)
def test_oracle_equals_the_integer_model_bit_for_bit(win, scene):
    """Position, status and err of EVERY track -- grid tracks at integer, half, quarter and random sub-pixel positions, and the ring on both sides of the
    start-position rule -- for one Newton step, the coarse criteria and the fine criteria."""
    I, J = R.SCENES[scene]()
    for offset in R.OFFSETS:
        pts = R.tracks(win, offset)
        assert len(pts) <= 250
        for max_count, eps in R.CRITERIA:
            p, s, e, _ = R.model(scene, win, offset, max_count, eps)
            op, os_, oe = KO.pyr_lk(I, J, pts, win=win, max_level=0, max_count=max_count, eps=eps)
            ctx = (scene, win, offset, max_count, eps)
            assert np.array_equal(os_, s), (ctx, np.flatnonzero(os_ != s))
            bad = np.flatnonzero((_bits(op) != _bits(p)).any(1))
            assert not len(bad), (ctx, bad, op[bad], p[bad])
            bad = np.flatnonzero(_bits(oe) != _bits(e))
            assert not len(bad), (ctx, bad, oe[bad], e[bad])


@pytest.mark.parametrize("win", WINDOWS)
def test_track_sets_straddle_the_start_position_rule(win):
    """A condition on the inputs: the ring holds tracks the rule rejects (status 0, position and err untouched) and border tracks it keeps."""
    for offset in R.OFFSETS:
        pts = R.tracks(win, offset)
        p, s, e, _ = R.model("bars16", win, offset, 1, 0.0)
        half = np.float32((win - 1) * 0.5)
        origin = np.floor(pts - half)
        out = ((origin < -win) | (origin >= np.float32([R.W, R.H]))).any(1)
        assert out[-48:].sum() >= 4 and (~out[-48:]).sum() >= 8 and not out[:-48].any(), (win, offset)
        assert not s[out].any() and np.array_equal(p[out], pts[out]) and not e[out].any()
        near = ~out & ((origin < 0) | (origin + win + 1 >= np.float32([R.W, R.H]))).any(1)  # windows that hang over the frame: REFLECT_101 pixels, zero gradients
        assert (s & near).sum() >= (1 if win == 3 else 4), (win, offset)  # (a 3 x 3 window hangs over only within 2 px of the edge)


@pytest.mark.parametrize("scene, big, small", [("bars8", "A11", "b1"), ("bars16", "A11", "b1"), ("bars16_neg", "A11", "b1"), ("bars_t8", "A22", "b2"), ("bars_t16", "A22", "b2")])
@pytest.mark.parametrize("win", (15, 51, 63))
def test_bar_scenes_reach_the_operand_limits(win, scene, big, small):
    """A condition on the inputs, computed by the model alone, with the integer-position tracks: the largest Ix.Ix sum (Iy.Iy for the transposed bars) is
    at least 0.85 of win^2 4080^2, the largest |diff.Ix| (|diff.Iy|) sum at least 0.45 of win^2 8160 4080.  About a half is the most a binary pair can
    give the second: |diff| = 255 with the gradient's sign holds on only half of the edge pixels.  (The checkerboards load all five sums at once but
    cannot come as high: rows next to a cell's upper or lower edge have |Ix| = 10 * 255, not 16 * 255.)"""
    peaks = R.model(scene, win, "int", 1, 0.0)[3]
    n = win * win
    assert peaks[big] >= 0.85 * n * R.GX_MAX ** 2, (peaks[big] / (n * R.GX_MAX ** 2))
    assert peaks[small] >= 0.45 * n * R.DIFF_MAX * R.GX_MAX, (peaks[small] / (n * R.DIFF_MAX * R.GX_MAX))
    assert peaks[big] > 2 ** 31 and (win == 15 or peaks[small] > 2 ** 31)  # sums no int32 holds
    if scene == "bars16_neg":  # ... and here the large sum is the negative one
        assert -peaks["b1_min"] == peaks["b1"], peaks


# Largest Ix.Ix, Iy.Iy window sums as shares of win^2 4080^2 and largest |diff.Ix|, |diff.Iy| sums as shares of win^2 8160 4080, as the model computes them
# on the integer-position tracks with one Newton step.  The checkerboards cannot come near the bars: next to a cell's upper or lower edge the vertical
# smoothing leaves |Ix| = 10 * 255 of 16 * 255 ((10 / 16)^2 = 0.39 of the product, every row of the 2-px board), larger cells are flat inside, and
# with J = 255 - I the diff.Ix terms of the two sides of an edge cancel.  What they do reach is pinned here, so that a weakened scene fails.
CHECKER_REACH = {
    ("checker2", 15): (0.486, 0.5032, 0.3331, 0.0528),
    ("checker2", 51): (0.3797, 0.38, 0.2696, 0.0138),
    ("checker2", 63): (0.3833, 0.3741, 0.2663, 0.0088),
    ("checker2_inv", 15): (0.486, 0.5032, 0.0542, 0.055),
    ("checker2_inv", 51): (0.3797, 0.38, 0.0131, 0.0123),
    ("checker2_inv", 63): (0.3833, 0.3741, 0.0102, 0.0101),
    ("checker3", 15): (0.3967, 0.4041, 0.2383, 0.0481),
    ("checker3", 51): (0.3341, 0.3283, 0.2023, 0.0109),
    ("checker3", 63): (0.3275, 0.3237, 0.198, 0.0067),
    ("checker3_inv", 15): (0.3967, 0.4041, 0.0298, 0.0399),
    ("checker3_inv", 51): (0.3341, 0.3283, 0.0115, 0.01),
    ("checker3_inv", 63): (0.3275, 0.3237, 0.0054, 0.0075),
    ("checker4", 15): (0.3394, 0.3571, 0.2147, 0.0375),
    ("checker4", 51): (0.283, 0.2728, 0.1606, 0.0067),
    ("checker4", 63): (0.2686, 0.2606, 0.153, 0.0051),
    ("checker4_inv", 15): (0.3394, 0.3571, 0.0633, 0.065),
    ("checker4_inv", 51): (0.283, 0.2728, 0.0168, 0.0148),
    ("checker4_inv", 63): (0.2686, 0.2606, 0.0119, 0.0108),
    ("checker6", 15): (0.275, 0.245, 0.1267, 0.0178),
    ("checker6", 51): (0.2362, 0.2205, 0.1334, 0.0041),
    ("checker6", 63): (0.2257, 0.2122, 0.1234, 0.0029),
    ("checker6_inv", 15): (0.275, 0.245, 0.0571, 0.0621),
    ("checker6_inv", 51): (0.2362, 0.2205, 0.0162, 0.0179),
    ("checker6_inv", 63): (0.2257, 0.2122, 0.0128, 0.0135),
}


@pytest.mark.parametrize("scene, win", sorted(CHECKER_REACH))
def test_checkerboards_keep_their_reach(scene, win):
    """A condition on the inputs, computed by the model alone: every checkerboard at windows 15, 51 and 63 loads all four sums to at least 0.95 of the
    recorded share (the scenes are seeded, so the figures repeat exactly; the margin only allows for the 4-digit rounding of the table)."""
    peaks = R.model(scene, win, "int", 1, 0.0)[3]
    n = win * win
    got = (peaks["A11"] / (n * R.GX_MAX ** 2), peaks["A22"] / (n * R.GX_MAX ** 2), peaks["b1"] / (n * R.DIFF_MAX * R.GX_MAX), peaks["b2"] / (n * R.DIFF_MAX * R.GX_MAX))
    for name, g, want in zip(("Ix.Ix", "Iy.Iy", "diff.Ix", "diff.Iy"), got, CHECKER_REACH[(scene, win)]):
        assert g >= 0.95 * want, (name, g, want)
    assert peaks["Ix"] == R.GX_MAX and peaks["Iy"] == R.GX_MAX and peaks["diff"] == R.DIFF_MAX  # single samples at the largest gradient and difference
    if win > 15 and not scene.endswith("_inv"):
        assert peaks["A11"] > 2 ** 31 and peaks["A22"] > 2 ** 31 and peaks["b1"] > 2 ** 31  # sums no int32 holds
