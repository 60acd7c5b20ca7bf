"""The oracle's RANSAC affine (oracle/klt_oracle.c ko_ransac_affine) against plain float64 references, on the CPU.

The HIP kernels are bit-exact with this oracle (tests/test_gpu_ransac.py), so an error they share can only show here: the refit against
np.linalg.lstsq, the adaptive iteration count against cv::RANSACUpdateNumIters written in NumPy."""
import math

import numpy as np
import pytest

from oracle import klt_oracle as KO
from ransac_ref import affine_scene, check_refit, refit_scenes, threshold_scene

DBL_MIN = 2.2250738585072014e-308


@pytest.mark.parametrize("scene", refit_scenes(), ids=lambda s: s[0])
def test_oracle_refit_matches_float64_least_squares(scene):
    """Before the split mean sums the two scenes with the 1000-px box at 1e6 failed here (80 % inliers: the int64 sum of x 2^32 overflowed): the
    refit was off by 1.18 px (m = 3072) and 1.13 px (m = 20000) against bounds of 4e-8 px.  Every other scene gave the same M before and after.
    Measured now: <= 2.5e-10 px on the frames up to 8K and at offsets 1e5 / 1e6 (bounds 1e-8 - 5e-8 px), <= 2.7e-6 px on the 1-4 px clusters
    (bounds 9e-6 - 1.2e-4 px: there the 2^-21 rounding of each moment term is a relative 1e-6 of the moments)."""
    name, src, dst = scene
    M, inl, _ = KO.ransac_affine(src, dst)
    check_refit(name, src, dst, M, inl)


def test_oracle_keeps_the_hypothesis_when_the_inliers_are_nearly_collinear():
    """det <= 1e-9 tr^2 of the centred moments: the refit is skipped and the 3-point model that won stays (maps its three samples exactly)."""
    rng = np.random.default_rng(9)
    x = rng.uniform(0, 1000, 60)
    src = np.c_[x, 500 + rng.uniform(-1e-3, 1e-3, 60)]  # a 1000 px line, 2e-3 px thick: det / tr^2 ~ 1e-13
    dst = src + [2.0, -1.0]
    src, dst = src.astype(np.float32), dst.astype(np.float32)
    M, inl, _ = KO.ransac_affine(src, dst)
    check_refit("nearly collinear", src, dst, M, inl)


def test_refit_out_of_range_fails_loudly():
    """Coordinates of 2^31 and beyond, or inliers spread wider than sqrt(2^42 / count), have no representable refit: an error, never a wrong M."""
    rng = np.random.default_rng(4)
    src, dst = affine_scene(rng, 200, 1.0, (3e9, 3e9 + 1e4, 0, 1e4), noise=0.0, A=np.array([[1.0, 0, 0], [0, 1.0, 0]]))
    with pytest.raises(ValueError, match="representable"):
        KO.ransac_affine(src, dst)
    src, dst = affine_scene(rng, 4000, 1.0, (0, 1e6, 0, 1e6), noise=0.0, A=np.array([[1.0, 0, 0], [0, 1.0, 0]]))
    with pytest.raises(ValueError, match="representable"):
        KO.ransac_affine(src, dst)
    src, dst = affine_scene(rng, 4000, 1.0, (0, 2e4, 0, 2e4), noise=0.1)  # 20 000 px box, 4000 inliers: sqrt(2^42 / 4000) = 33 000 px -> fits
    check_refit("20 000 px box", src, dst, *KO.ransac_affine(src, dst)[:2])


def _cv_update_iters(ep, max_iters, conf=0.99):
    """cv::RANSACUpdateNumIters(conf, ep, 3, max_iters) in NumPy: std::pow / std::log, cvRound (round half to even)."""
    num = math.log(max(1.0 - conf, DBL_MIN))
    denom = 1.0 - np.power(1.0 - ep, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        ld = np.log(np.maximum(denom, DBL_MIN))
        r = num / ld
        out = np.where((ld >= 0) | (-num >= max_iters * (-ld)), max_iters, np.rint(np.where(np.isfinite(r), r, 0.0)))
    out = np.where(denom < DBL_MIN, 0, out).astype(np.int64)
    # np.power / np.log may use their own vector code: where the result is within reach of a rounding boundary recompute with the C library's
    # pow and log, which std::pow / std::log call
    near = np.nonzero((np.abs(r - np.floor(r) - 0.5) < 1e-6) | (np.abs(-num - max_iters * (-ld)) < 1e-9 * abs(num)))[0]
    for i in near:
        d = 1.0 - math.pow(1.0 - float(ep[i]), 3)
        if d < DBL_MIN:
            out[i] = 0
            continue
        lg = math.log(d)
        out[i] = max_iters if lg >= 0 or -num >= max_iters * (-lg) else int(np.rint(num / lg))
    return out


def test_adaptive_iteration_count_matches_cv_for_every_reachable_outlier_ratio():
    """Every ep = (m - c) / m with 3 <= c <= m <= 5000 (the selection rule only updates on a count c > 2), from the 2000-hypothesis start: the
    oracle's det_log-based count (the device's, bit for bit) equals cv::RANSACUpdateNumIters.  No disagreement was found, so none is listed."""
    ms = np.arange(3, 5001)
    m = np.repeat(ms, ms - 2)
    c = np.concatenate([np.arange(3, k + 1) for k in ms])
    ep = np.unique((m - c).astype(np.float64) / m)
    got = KO.ransac_update_iters(ep, 2000)
    exp = _cv_update_iters(ep, 2000)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(float(ep[i]), int(got[i]), int(exp[i])) for i in bad[:10]]
    assert got.max() == 2000 and got.min() == 0 and np.unique(got).size > 500


def test_adaptive_iteration_count_along_a_growing_best_count():
    """The count carried from one update to the next, as the rule does when every new hypothesis beats the last (c = 3, 4, ... m) for m up to 400."""
    L = KO.lib()
    for m in range(3, 401):
        k = kc = 2000
        for c in range(3, m + 1):
            ep = (m - c) / m
            k = L.ko_ransac_update_iters(0.99, ep, k)
            kc = int(_cv_update_iters(np.array([ep]), kc)[0])
            assert k == kc, (m, c, k, kc)


def test_threshold_is_float32_of_the_float64_squared_residual():
    """The inlier test is float32(ex^2 + ey^2) <= 9, with the sum taken in float64 (cv2's rule) -- checked against plain NumPy on a scene where every
    hypothesis from the exact pairs is exact; see ransac_ref.threshold_scene."""
    src, dst, exp = threshold_scene()
    M, inl, _ = KO.ransac_affine(src, dst)
    assert M is not None and np.array_equal(inl, exp)
