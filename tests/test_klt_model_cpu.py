"""CPU only: oracle/klt_oracle.c held to the exact NumPy models of tests/image_ref.py and tests/lk_ref.py -- the image stages, the pyramidal
Lucas-Kanade descent with its forward-backward gate, KLTregional and KLTmain stage by stage -- bit for bit, and the models (with the oracle) held to
truth that no implementation supplied: a plane, on which bilinear interpolation is exact, and a frame pair built so that KLTregional must find no motion.
Every comparison is exact equality except the two bounds derived at the truth tests."""
import numpy as np
import pytest

import image_ref as IM
import klt_model_scenes as S
import lk_ref as R
from oracle import klt_oracle as KO

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# a. image stages: oracle == model
# ---------------------------------------------------------------------------------------------------------------------
PYR_SHAPES = ((21, 30), (33, 1), (1, 9), (2, 2), (5, 7), (64, 63))


@pytest.mark.parametrize("shape", PYR_SHAPES)
def test_pyr_down_equals_the_model(shape):
    """Down to one row, one column and 2 x 2, where every tap but the centre is a reflected one; chained until a single pixel is left."""
    img = np.random.default_rng(shape[0] * 100 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    while True:
        got, want = KO.pyr_down(img), IM.pyr_down(img)
        assert got.shape == want.shape == ((img.shape[0] + 1) // 2, (img.shape[1] + 1) // 2)
        assert np.array_equal(got, want), (shape, img.shape)
        if want.size == 1:
            break
        img = want


def test_pyramid_level_counts_equal_the_model():
    """Every size from 1 to 70 squared with itself and with a fixed 200, windows on both sides of the sizes, 0 to 5 levels asked for; and the pyramids
    the model builds have those counts and shapes."""
    for w in range(1, 71):
        for h in (w, 200):
            for win in (3, 8, 15, 21, 51):
                for max_level in range(6):
                    assert IM.pyramid_levels(w, h, win, max_level) == KO.pyramid_levels(w, h, win, max_level), (w, h, win, max_level)
    for case, levels in enumerate(S.LK_LEVELS):
        f0 = S.lk_scene(case)[0]
        W, H, win, max_level = S.LK_CASES[case][:4]
        pyr = IM.pyramid(f0, win, max_level)
        assert len(pyr) == levels == KO.pyramid_levels(W, H, win, max_level), case
        for a, b in zip(pyr, pyr[1:]):
            assert b.shape == ((a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2)


def test_remap_equals_the_model_on_seeded_maps():
    """60 maps of a 70 x 90 image: rotation, zoom, footprints that leave the frame, and translations on the 1/64 grid where the 1/32 quantisation ties."""
    img, cases = S.remap_cases()
    ties = outside = 0
    for k, (T, roi) in enumerate(cases):
        want = IM.remap_affine(img, T, roi)
        assert np.array_equal(KO.remap_affine(img, T, roi), want), (k, T, roi)
        ties += k % 3 == 0 and bool(((T[4:] * 64) % 2 == 1).any())
        outside += not S.footprint_inside(T, roi, img.shape)
    assert ties >= 10 and outside >= 10  # conditions on the inputs: both kinds are really there


def test_crop_shift_bounding_rect_resize_and_gray_equal_the_model():
    rng = np.random.default_rng(32)
    img = rng.integers(0, 256, (70, 90), dtype=np.uint8)
    for roi in ((5, 80, 3, 60), (1, 90, 1, 70), (17, 18, 9, 33)):
        for dx, dy in ((0, 0), (7, -2), (-30, 40), (200, 0), (-3, -5)):
            assert np.array_equal(KO.crop_shift(img, roi, dx, dy), IM.crop_shift(img, roi, dx, dy)), (roi, dx, dy)
    for n in (1, 3, 200):
        p = rng.uniform(-30, 330, (n, 2)).astype(F32)
        q = np.floor(p) + F32(0.0)  # integer coordinates: floor(max) + 1, not ceil(max)
        for pts in (p, q, p * F32(0.3) + F32(100.0)):
            for border in ((0, 0), (50, 50), (7, 300)):
                assert IM.bounding_rect(pts, (240, 320), border) == KO.bounding_rect(pts, (240, 320), border), (n, border)
    assert IM.bounding_rect(np.zeros((0, 2), F32), (240, 320), (50, 50)) == KO.bounding_rect(np.zeros((0, 2), F32), (240, 320), (50, 50))
    for shape in ((70, 90), (37, 53), (8, 5)):
        im = rng.integers(0, 256, shape, dtype=np.uint8)
        for f in (0.5, 0.25, 0.3, 1.7):
            assert np.array_equal(KO.resize_nearest(im, f), IM.resize_nearest(im, f)), (shape, f)
        assert np.array_equal(KO.resize_nearest(im, 0.3, 1.7), IM.resize_nearest(im, 0.3, 1.7))
        assert np.array_equal(KO.resize_quarter(im), IM.resize_nearest(im, 0.25))
    g = np.arange(256, dtype=np.uint8)
    zero = np.zeros(256, np.uint8)
    for bgr in ((g, zero, zero), (zero, g, zero), (zero, zero, g), (g, g, g), (g, g[::-1], zero), (g, zero, g[::-1])):
        px = np.stack(bgr, 1)[None]
        assert np.array_equal(KO.bgr2gray(px), IM.bgr2gray(px))
    px = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    assert np.array_equal(KO.bgr2gray(px), IM.bgr2gray(px))


# ---------------------------------------------------------------------------------------------------------------------
# b. pyramidal LK with the forward-backward gate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(S.LK_CASES)))
def test_lk_fb_equals_the_model(case):
    """Position (NaN included), status, err and the forward-backward error of all tracks, without a gate and at thresholds 1.0 and 0.3.  First, on the
    model alone: both branches of the status are populated."""
    f0, f1, pts = S.lk_scene(case)
    kw = S.lk_params(case)
    assert len(pts) == 210 + S.LK_CASES[case][7]
    for fbt in S.FBTS:
        p2, v, err, fbe = S.lk_model(case, fbt)
        assert v.sum() >= 20 and (~v).sum() >= 20, (case, fbt, int(v.sum()), int((~v).sum()))
    for fbt in S.FBTS:
        p2, v, err, fbe = S.lk_model(case, fbt)
        op, ov, oerr, ofbe = KO.lk_fb(f0, f1, pts, fbt=fbt, return_fbe=True, **kw)
        assert np.array_equal(ov, v), (case, fbt, np.flatnonzero(ov != v))
        assert np.array_equal(op, p2, equal_nan=True), (case, fbt)
        assert np.array_equal(oerr, err), (case, fbt)
        assert np.array_equal(ofbe, fbe, equal_nan=True), (case, fbt)


def test_forward_backward_gate_is_strict():
    """Identical frames and tracks at whole pixels (so that taking half a window off and adding it back is exact on every level): every surviving track
    comes back to exactly where it started, fbe = 0, and `fbe < fbt` at fbt = 0 keeps none of them (`<=` would keep them all).  The scenes above cannot
    tell the two comparisons apart: no fbe of theirs equals its threshold."""
    f0, _, pts = S.lk_scene(0)
    pts = np.rint(pts)
    kw = S.lk_params(0)
    p2, v, err, fbe = R.lk_fb(f0, f0, pts, 0.0, **kw)
    alive = R.lk_fb(f0, f0, pts, None, **kw)[1]
    assert alive.sum() >= 20 and not fbe[alive].any() and not v.any()
    op, ov, oerr, ofbe = KO.lk_fb(f0, f0, pts, fbt=0.0, return_fbe=True, **kw)
    assert np.array_equal(ov, v) and np.array_equal(op, p2, equal_nan=True) and np.array_equal(oerr, err) and np.array_equal(ofbe, fbe, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# c. KLTregional
# ---------------------------------------------------------------------------------------------------------------------
def test_regional_rois_lie_inside_the_frame_at_every_alignment():
    """A condition on the inputs, on the model alone: no clamp of boundingRect acts, and the ROI's left edge takes every residue modulo 4."""
    rois = [S.regional_model(shift, "translate coarse")[2] for shift in range(4)]
    for x0, x1, y0, y1 in rois:
        assert 1 < x0 < x1 < S.RW and 1 < y0 < y1 < S.RH
    assert sorted(r[0] % 4 for r in rois) == [0, 1, 2, 3]


@pytest.mark.parametrize("cfg", sorted(S.REGIONAL_CONFIGS))
@pytest.mark.parametrize("shift", range(4))
def test_klt_regional_equals_the_model(shift, cfg):
    f0, f1, T_af, T_tr = S.regional_scene()
    lk, fbt, translate = S.REGIONAL_CONFIGS[cfg]
    p, v, roi, warped = S.regional_model(shift, cfg)
    op, ov, oroi, owarped = KO.klt_regional(f0, f1, S.regional_points(shift), T_tr if translate else T_af, lk, fbt=fbt, translate=translate)
    assert oroi == roi
    assert np.array_equal(owarped, warped)
    assert np.array_equal(ov, v), np.flatnonzero(ov != v)
    assert np.array_equal(op, p, equal_nan=True)
    assert v.sum() >= 20  # the scene tracks


# ---------------------------------------------------------------------------------------------------------------------
# d. truth
# ---------------------------------------------------------------------------------------------------------------------
def test_remap_of_a_plane_is_the_plane_and_a_transposed_map_is_not():
    """Image rint(a x + b y + c), map 0.3 rad at zoom 0.9, footprint inside the frame.  Bilinear interpolation is exact on a plane, so
    |remap - (a mx + b my + c)| <= 1 + (|a| + |b|) / 64 + (|a| + |b|) 2^-12: 0.5 for the rounding of the input image, 0.5 for the rounding of the output,
    1/64 px of coordinate quantisation per axis (rint to 1/32 px) and the float32 rounding of the coordinates themselves (three roundings at
    magnitudes below 256, each below 2^-16 relative: under 2^-12 px in all).  The truth is the float64 bilinear sample of the UNROUNDED plane
    at the float64 map.  The same map with T[1] and T[2] exchanged must break the bound: that is what the test is for."""
    plane, img, T = S.ramp()
    assert S.footprint_inside(T, S.RAMP_ROI, img.shape) and S.footprint_inside(S.swapped(T), S.RAMP_ROI, img.shape)
    truth = IM.remap_truth(plane, T, S.RAMP_ROI)  # = a mx + b my + c
    for name, remap in (("oracle", KO.remap_affine), ("model", IM.remap_affine)):
        e = np.abs(remap(img, T, S.RAMP_ROI).astype(np.float64) - truth).max()
        print(f"{name}: max |remap - plane| = {e:.4f}, bound {S.RAMP_BOUND:.4f}")
        assert e <= S.RAMP_BOUND, (name, e)
        e = np.abs(remap(img, S.swapped(T), S.RAMP_ROI).astype(np.float64) - truth).max()
        print(f"{name}, T[1] and T[2] exchanged: {e:.2f}")
        assert e > S.RAMP_BOUND, (name, e)


@pytest.mark.parametrize("cfg", sorted(S.PAIR_CONFIGS))
def test_klt_regional_returns_the_map_of_a_pair_built_from_it(cfg):
    """im0's ROI is the model's own warp of im under T (4 degrees, zoom 0.95), so the warped frame equals the template, the first Newton step is zero on
    every level, every track is valid and p is p0 through T: |p - p0 T| <= 8 * 2^-15 px.  Every coordinate stays below 512, where a float32 rounding
    is at most 2^-16.  Each of x and y is rounded twice on the way into and out of the ROI (the origin subtracted, then added back): 2^-15 each, which
    the map-back carries through |T0| + |T2| <= 1.4 (likewise T1, T3), 1.4 * 2^-15; the map-back adds four roundings of its own (two products, two
    sums), 2 * 2^-15.  That is 3.4 * 2^-15 at the most, under the 8 * 2^-15 asserted.  With T[1] and T[2] exchanged the warp no longer matches and the
    call must lose tracks or leave the bound."""
    im0, im, p0, T, truth, roi = S.pair_scene()
    lk, fbt = S.PAIR_CONFIGS[cfg]
    assert S.footprint_inside(T, roi, im.shape) and np.abs(T[:4]).reshape(2, 2).sum(0).max() <= 1.4 and np.abs(truth).max() < 512 and p0.max() < 512
    for name, fn in (("oracle", lambda T_: KO.klt_regional(im0, im, p0, T_, lk, fbt=fbt, translate=False)), ("model", lambda T_: R.klt_regional(im0, im, p0, T_, lk, fbt, False))):
        p, v, r, _ = fn(T)
        assert r == roi
        e = np.abs(p.astype(np.float64) - truth).max()
        print(f"{name} {cfg}: {int(v.sum())} of {len(v)} valid, max |p - p0 T| = {e:.3g}, bound {S.PAIR_BOUND:.3g}")
        assert v.all() and e <= S.PAIR_BOUND, (name, int(v.sum()), e)
        p, v, _, _ = fn(S.swapped(T))
        with np.errstate(invalid="ignore"):
            e = np.abs(p.astype(np.float64) - truth)[v].max() if v.any() else np.inf
        print(f"{name} {cfg}, T[1] and T[2] exchanged: {int(v.sum())} valid, {e:.3g}")
        assert not v.all() or e > S.PAIR_BOUND, name


# ---------------------------------------------------------------------------------------------------------------------
# e. KLTmain, stage by stage
# ---------------------------------------------------------------------------------------------------------------------
def test_klt_main_stages_equal_the_model():
    """Every stage of the model fed from the oracle's own upstream output; RANSAC's choice of inliers is taken from the oracle (ransac_ref.py covers
    its refit).  On the oracle's outputs first: the scene runs the whole pipeline, and tracks live and die."""
    f0, f1, p0 = S.main_scene()
    p, v, small, St = KO.klt_main(f1, f0, None, p0, stages=True)
    assert St["flags"] == 0 and v.sum() >= 20 and (~v).sum() >= 4
    assert np.array_equal(small, IM.resize_nearest(f1, 0.25))
    St = dict(St, v=v)
    assert np.array_equal(St["p_fine"], St["p_all"], equal_nan=True)
    for name, ok in S.main_stage_checks(f0, f1, p0, St):
        assert ok, name
