"""The small scenes that tests/test_klt_model_cpu.py (oracle against the NumPy model) and tests/test_gpu_klt_model.py (kernels against the NumPy model)
share, and the model's results on them: computed once per process, frozen, never written to.  Everything here comes from velocity_amd.synth, seeded
generators and the models of tests/image_ref.py / tests/lk_ref.py; nothing calls the oracle or the library."""
import functools
import math

import numpy as np

import image_ref as IM
import lk_ref as R
from _helpers import frozen
from velocity_amd import synth

F32 = np.float32
LK_COARSE = dict(win=15, max_level=4, max_count=10, eps=0.1)  # utils/KLT.py:106
LK_FINE = dict(win=51, max_level=0, max_count=30, eps=0.001)  # utils/KLT.py:107


def rot_T(theta, scale, tx, ty):
    """3 x 2 row-vector affine [x y 1] T of a rotation by theta (radians) and a zoom, float32 (6,)."""
    c, s = scale * math.cos(theta), scale * math.sin(theta)
    return np.array([c, s, -s, c, tx, ty], F32)


def swapped(T):
    """T with its off-diagonal pair exchanged: the slip the truth tests exist to catch."""
    T = np.asarray(T, F32).reshape(6).copy()
    T[1], T[2] = T[2], T[1]
    return T


# ---------------------------------------------------------------------------------------------------------------------
# pyramidal LK with the forward-backward gate
# ---------------------------------------------------------------------------------------------------------------------
# (W, H, win, max_level, max_count, eps, texture seed, off-frame points).  Levels kept: 3, 2, 2, 2 (truncated from 5), 1 (image smaller than the
# window), 4 (even window).  The off-frame points give the two large-window scenes dead tracks when no gate is on: a 51-px window reaches every point
# within 20 px of the frame.
# The last case is a checkerboard of 2-px cells against itself moved one pixel: level 1 of it has period 2, where the Scharr differences vanish, so
# every track fails the min-eigenvalue test up there and passes it on level 0 -- the case that tells whether an upper level may write the status.
CHECKER = -1
LK_CASES = ((96, 80, 15, 4, 10, 0.1, 11, 0), (160, 112, 51, 1, 30, 0.001, 12, 24), (101, 77, 21, 3, 30, 0.01, 13, 0), (40, 52, 15, 4, 10, 0.1, 14, 0),
            (12, 20, 51, 2, 10, 0.03, 3, 24), (97, 81, 8, 3, 10, 0.03, 16, 0), (64, 48, 15, 2, 10, 0.03, CHECKER, 0))
LK_LEVELS = (3, 2, 2, 2, 1, 4, 2)
FBTS = (None, 1.0, 0.3)


def lk_params(case):
    W, H, win, max_level, max_count, eps = LK_CASES[case][:6]
    return dict(win=win, max_level=max_level, max_count=max_count, eps=eps)


@functools.lru_cache(maxsize=None)
def lk_scene(case):
    """(f0, f1, pts): a synth pair under zoom 1.004, 0.3 degrees and (2.3, -1.4) px (or the checkerboard pair); 150 uniform points in [-20, W + 20] x [-20, H + 20], 60 grid
    points inside the frame, and the case's off-frame points (further out than a window plus its half)."""
    W, H, win, _, _, _, seed, extra = LK_CASES[case]
    m = synth.AffineMotion(W, H, s=1.004, theta_deg=0.3, tx=2.3, ty=-1.4)
    if seed == CHECKER:
        y, x = np.mgrid[0:H, 0:W]
        f0 = (255 * ((x // 2 + y // 2) % 2)).astype(np.uint8)
        f1 = np.roll(f0, 1, axis=1)
    else:
        f0 = synth.render_frame(W, H, m, 0, seed=seed).numpy()
        f1 = synth.render_frame(W, H, m, 1, seed=seed).numpy()
    rng = np.random.default_rng(1000 * W + H)
    uni = rng.uniform([-20, -20], [W + 20, H + 20], (150, 2))
    gx, gy = np.meshgrid(np.linspace(2, W - 3, 10), np.linspace(2, H - 3, 6))
    far = 1.5 * win + 2 + rng.uniform(0, 10, extra)
    along = rng.uniform(0, 1, extra)
    side = np.arange(extra) % 4
    off = np.where((side < 2)[:, None], np.stack([np.where(side == 0, -far, W + far), along * H], 1), np.stack([along * W, np.where(side == 2, -far, H + far)], 1))
    return frozen(f0, f1, np.concatenate([uni, np.stack([gx.ravel(), gy.ravel()], 1), off.reshape(-1, 2)]).astype(F32))


@functools.lru_cache(maxsize=None)
def lk_model(case, fbt):
    """(p2, v, err, fbe) of the model on lk_scene(case)."""
    f0, f1, pts = lk_scene(case)
    return frozen(*R.lk_fb(f0, f1, pts, fbt, **lk_params(case)))


# ---------------------------------------------------------------------------------------------------------------------
# the affine remap
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def remap_cases():
    """(image 70 x 90, [(T, roi)] * 60): random ROIs; rotations within 0.6 rad at zooms 0.6 to 1.5 with translations that push part of the footprint out
    of the frame; every third map a pure translation on the 1/64 grid, where rint(m * 32) meets its ties."""
    rng = np.random.default_rng(31)
    h, w = 70, 90
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cases = []
    for k in range(60):
        x0, y0 = int(rng.integers(0, 40)), int(rng.integers(0, 30))
        roi = (x0, int(rng.integers(x0 + 1, w + 1)), y0, int(rng.integers(y0 + 1, h + 1)))
        if k % 3 == 0:
            T = np.array([1, 0, 0, 1, rng.integers(-20 * 64, 20 * 64) / 64.0, rng.integers(-20 * 64, 20 * 64) / 64.0], F32)
        else:
            T = rot_T(rng.uniform(-0.6, 0.6), rng.uniform(0.6, 1.5), rng.uniform(-40, 40), rng.uniform(-40, 40))
        cases.append((T, roi))
    return frozen(img)[0], tuple(cases)


# the plane: bilinear interpolation is exact on it, so the remap of its rounded image can be held to the analytic value
RAMP_A, RAMP_B, RAMP_C = 0.5, 0.25, 10.0
RAMP_ROI = (20, 120, 10, 90)  # near the origin, so that the transposed map, which turns the other way about it, stays inside the frame too
RAMP_BOUND = 1 + (abs(RAMP_A) + abs(RAMP_B)) / 64 + (abs(RAMP_A) + abs(RAMP_B)) * 2.0 ** -12


@functools.lru_cache(maxsize=None)
def ramp():
    """(plane float64, image uint8 = rint(plane), T): a 240 x 200 plane a x + b y + c and a map of 0.3 rad at zoom 0.9 that takes the centre of RAMP_ROI
    to the centre of the frame."""
    W, H = 240, 200
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    plane = RAMP_A * x + RAMP_B * y + RAMP_C
    T = rot_T(0.3, 0.9, 0.0, 0.0)
    cx, cy = (RAMP_ROI[0] + RAMP_ROI[1] - 1) / 2, (RAMP_ROI[2] + RAMP_ROI[3] - 1) / 2
    T[4] = (W - 1) / 2 - (cx * T[0] + cy * T[2])
    T[5] = (H - 1) / 2 - (cx * T[1] + cy * T[3])
    return frozen(plane, np.rint(plane).astype(np.uint8), T)


def footprint_inside(T, roi, shape):
    """Whether every bilinear tap of the ROI's map lies inside the frame (float64 map of the float32 T, a pixel of margin for the quantisation)."""
    T = np.asarray(T, F32).reshape(6).astype(np.float64)
    x0, x1, y0, y1 = roi
    cx, cy = np.array([x0, x1 - 1, x0, x1 - 1], float), np.array([y0, y0, y1 - 1, y1 - 1], float)
    mx, my = cx * T[0] + cy * T[2] + T[4], cx * T[1] + cy * T[3] + T[5]
    return bool(mx.min() >= 1 and mx.max() <= shape[1] - 3 and my.min() >= 1 and my.max() <= shape[0] - 3)


# ---------------------------------------------------------------------------------------------------------------------
# KLTregional
# ---------------------------------------------------------------------------------------------------------------------
RW, RH = 320, 240
REGIONAL_CONFIGS = {"translate coarse": (LK_COARSE, 1.0, True), "affine fine": (LK_FINE, 0.3, False),
                    "affine 21": (dict(win=21, max_level=2, max_count=30, eps=0.01), 0.5, False)}


@functools.lru_cache(maxsize=None)
def regional_scene():
    """(f0, f1, T_affine, T_translate): 320 x 240 frames under 2 degrees, zoom 1.03 and (3.6, -2.7) px.  T_affine is the true motion, T_translate its
    translation at the frame centre, with a negative component so that truncation towards zero, floor and rounding all differ."""
    m = synth.AffineMotion(RW, RH, s=1.03, theta_deg=2.0, tx=3.6, ty=-2.7)
    f0 = synth.render_frame(RW, RH, m, 0, seed=21).numpy()
    f1 = synth.render_frame(RW, RH, m, 1, seed=21).numpy()
    T_af = np.ascontiguousarray(m.matrix(1).T, F32).reshape(6)
    return frozen(f0, f1, T_af, np.array([1, 0, 0, 1, 3.6, -2.7], F32))


@functools.lru_cache(maxsize=None)
def regional_points(shift):
    """80 jittered grid points in the box [62, 250] x [60, 175] moved `shift` px in x: the ROI (border 50) lies strictly inside the frame and its left
    edge moves with the shift, so four shifts give every x0 % 4."""
    g = synth.grid_tracks(80, RW, RH, seed=5, frac=1.0)
    p = np.stack([62 + g[:, 0] * (188 / RW) + shift, 60 + g[:, 1] * (115 / RH)], 1).astype(F32)
    return frozen(p)[0]


@functools.lru_cache(maxsize=None)
def regional_model(shift, cfg):
    """(p, v, roi, warped) of the model."""
    f0, f1, T_af, T_tr = regional_scene()
    lk, fbt, translate = REGIONAL_CONFIGS[cfg]
    p, v, roi, warped = R.klt_regional(f0, f1, regional_points(shift), T_tr if translate else T_af, lk, fbt, translate)
    return frozen(p, v) + (roi,) + frozen(warped)


# the self-consistent pair: im0's ROI IS the model's warp of im, so KLTregional must find no motion at all and return p0 mapped through T
PAIR_BOUND = 8 * 2.0 ** -15
PAIR_CONFIGS = {"fine": (LK_FINE, 0.3), "coarse": (LK_COARSE, 1.0)}


@functools.lru_cache(maxsize=None)
def pair_scene():
    """(im0, im, p0, T, truth): im a smooth texture, im0 noise with im0[roi] = image_ref.remap_affine(im, T, roi) for a map of 4 degrees at zoom 0.95
    about the frame centre; truth = p0 through the float32 T in float64."""
    rng = np.random.default_rng(77)
    ident = synth.AffineMotion(RW, RH, s=1.0, theta_deg=0.0, tx=0.0, ty=0.0)
    im = synth.render_frame(RW, RH, ident, 0, seed=33).numpy()
    p0 = regional_points(1)
    T = rot_T(math.radians(4.0), 0.95, 0.0, 0.0)
    cx, cy = (RW - 1) / 2, (RH - 1) / 2
    T[4] = cx - (cx * T[0] + cy * T[2])
    T[5] = cy - (cx * T[1] + cy * T[3])
    roi = IM.bounding_rect(p0, im.shape, (50, 50))
    x0, x1, y0, y1 = roi
    im0 = rng.integers(0, 256, im.shape, dtype=np.uint8)
    im0[y0:y1, x0:x1] = IM.remap_affine(im, T, roi)
    T64 = T.astype(np.float64)
    p64 = p0.astype(np.float64)
    truth = np.stack([p64[:, 0] * T64[0] + p64[:, 1] * T64[2] + T64[4], p64[:, 0] * T64[1] + p64[:, 1] * T64[3] + T64[5]], 1)
    return frozen(im0, im, p0, T, truth) + (roi,)


# ---------------------------------------------------------------------------------------------------------------------
# KLTmain
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_scene():
    """(f0, f1, p0): 320 x 240 frames under 0.8 degrees, zoom 1.012 and (5.3, -2.6) px, 120 grid tracks and 16 points near and beyond two corners."""
    m = synth.AffineMotion(RW, RH, s=1.012, theta_deg=0.8, tx=5.3, ty=-2.6)
    f0 = synth.render_frame(RW, RH, m, 0, seed=51).numpy()
    f1 = synth.render_frame(RW, RH, m, 1, seed=51).numpy()
    rng = np.random.default_rng(52)
    p0 = np.concatenate([synth.grid_tracks(120, RW, RH), rng.uniform(-10, 14, (8, 2)), rng.uniform([RW - 14, RH - 14], [RW + 10, RH + 10], (8, 2))]).astype(F32)
    return frozen(f0, f1, p0)


def main_stage_checks(f0, f1, p0, S):
    """Every modelled stage of KLTmain (utils/KLT.py:99-134) against the stage outputs S of an implementation (the keys of oracle.klt_oracle.klt_main's
    stage dict / velocity_amd.KLT.klt_stages), each stage of the model fed from S's own upstream output.  RANSAC's selection is not modelled: v_small
    and T23 are taken from S.  Returns a list of (name, passed)."""
    eq = functools.partial(np.array_equal, equal_nan=True)
    out = []
    q = F32(0.25)
    s0, s1 = IM.resize_nearest(f0, 0.25), IM.resize_nearest(f1, 0.25)
    ps, vs, _, _ = R.lk_fb(s0, s1, p0 * q, None, **LK_COARSE)
    v_small = np.asarray(S["v_small"]).astype(bool)
    out.append(("p_small", eq(ps / q, S["p_small"])))
    out.append(("v_small within the LK status", not (v_small & ~vs).any()))
    tr = IM.mean_translation(p0, S["p_small"], v_small)
    out.append(("T_trans", np.array_equal(tr, np.asarray(S["T_trans"]))))
    T_tr = np.array([1, 0, 0, 1, tr[0], tr[1]], F32)
    pc, vc, roi, _ = R.klt_regional(f0, f1, p0, T_tr, LK_COARSE, 1.0, True)
    out.append(("roi", tuple(int(x) for x in S["roi"]) == roi))
    out.append(("p_coarse", eq(pc, S["p_coarse"])))
    out.append(("v_coarse", np.array_equal(vc, np.asarray(S["v_coarse"]).astype(bool))))
    T_af = np.ascontiguousarray(np.asarray(S["T23"], np.float64).reshape(2, 3).T, F32).reshape(6)
    pf, vf, _, warped = R.klt_regional(f0, f1, p0, T_af, LK_FINE, 0.3, False)
    out.append(("warped", np.array_equal(warped, S["warped"])))
    out.append(("p_fine", eq(pf, S["p_fine"])))
    out.append(("v", np.array_equal(vf, np.asarray(S["v"]).astype(bool))))
    return out
