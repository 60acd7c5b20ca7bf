"""The small scenes that tests/test_subpix_model_cpu.py (oracle against the NumPy model) and tests/test_gpu_subpix_model.py (kernels against the NumPy
model) share, and the model's results on them: computed once per process, frozen, never written to.  Everything here comes from seeded generators and
the model of tests/subpix_ref.py (the frame-0 scenes add the camera and plate of tests/scenes.py and the detector's model, tests/gftt_ref.py); nothing
calls the oracle or the library's kernels."""
import functools

import numpy as np

import subpix_ref as SR
from _helpers import frozen

F32 = np.float32
WINS = tuple(range(1, SR.MAXWIN + 1))
# (max_iter, eps): the reference's call; one step; the cap alone; both clamps from below (= (1, 0.0)); both clamps' other side, a loose eps under the cap
# 1000 -> 100; the cap of 100 alone
STOPS = ((100, 0.001), (1, 0.001), (2, 0.0), (0, -1.0), (1000, 0.5), (100, 0.0))
COUNTS = (1, 63, 64, 65, 96)  # prefixes of the point list around the 64-thread block


def noise_texture(w, h, seed):
    """Box-filtered (5 x 5) uniform noise stretched to the full 8-bit range."""
    n = np.random.default_rng(seed).integers(0, 256, (h + 4, w + 4)).astype(np.float64)
    s = sum(n[j:j + h, i:i + w] for j in range(5) for i in range(5)) / 25.0
    return np.rint((s - s.min()) / (s.max() - s.min()) * 255.0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# texture: every exit of the loop, at every window
# ---------------------------------------------------------------------------------------------------------------------
TW, TH = 48, 40
FLAT = (38, 48, 0, 20)  # x0, x1, y0, y1 of the flat band

# start points found on the half-pixel grid of the image for the (exit, reverted) combinations that the regular points below do not reach at some window:
# `iter` kept and reverted at windows 1, 2, 5 and 7, `left` kept and reverted at windows 1, 2 and 3
SOUGHT = ((31.0, 0.0), (32.5, 5.5), (30.0, 7.0), (34.0, 8.5), (7.0, 0.0), (0.0, 6.0), (0.0, 17.0), (47.0, 17.5), (4.5, 33.0), (0.0, 34.0), (47.5, 28.5),
          (0.5, 35.0))

# the (exit, reverted) combinations that must occur at (100, 0.001), per window.  `det` with a revert occurs nowhere on the half-pixel grid of this
# image at any window: det vanishes on a flat patch, and a point that stands on one has not moved.  Windows 4 and 6 meet neither `iter` nor `left`
# there, window 3 no `iter`, windows 5 to 7 no `left`.
_ALL7 = tuple((e, r) for e in SR.EXITS for r in (False, True) if (e, r) != ("det", True))
_BASE = (("eps", False), ("eps", True), ("det", False))
CENSUS = {1: _ALL7, 2: _ALL7, 3: _BASE + (("left", False), ("left", True)), 4: _BASE, 5: _BASE + (("iter", False), ("iter", True)), 6: _BASE,
          7: _BASE + (("iter", False), ("iter", True))}


@functools.lru_cache(maxsize=None)
def texture():
    """(image 40 x 48, points [96, 2]): box-filtered noise with a flat band of value 120, ten columns wide, down the upper half of the right edge (at
    the edge, where the replicated border continues it, so that even the 17 x 17 patch of window 7 can lie wholly on it; the lower half of that edge
    stays textured).  Points: the four image corners; integer and fractional coordinates on each edge; points within 8 px (win + 1 for win = 7) of
    each edge; points on and beside the flat band; the sought points above; the rest uniform sub-pixel positions."""
    img = noise_texture(TW, TH, 7)
    x0, x1, y0, y1 = FLAT
    img[y0:y1, x0:x1] = 120
    pts = [(0, 0), (TW - 1, 0), (0, TH - 1), (TW - 1, TH - 1)]
    pts += [(0, 12), (0, 25.5), (TW - 1, 30), (TW - 0.25, 25.5), (13, 0), (20.25, 0), (9, TH - 1), (26.5, TH - 0.5)]
    pts += [(1.5, 8.25), (3.25, 31.5), (7.75, 20), (8, 14.5), (TW - 2.5, 27.25), (TW - 4.75, 35.5), (TW - 8.25, 30.25), (TW - 9, 24),
            (11.5, 1.25), (22.75, 3.5), (30.25, 7.75), (17, 8), (12.25, TH - 2.5), (25.5, TH - 4.25), (33.75, TH - 8.5), (19, TH - 9)]
    pts += [(43, 5), (44.5, 8.25), (TW - 1, 9), (46.25, 0.5), (40, 10), (38.5, 12.75), (42.25, 19.5), (36.75, 6.5)]
    pts += list(SOUGHT)
    rng = np.random.default_rng(70)
    pts += [tuple(p) for p in rng.uniform([0, 0], [TW - 9, TH], (96 - len(pts), 2))]
    pts = np.array(pts, F32)
    assert pts.shape == (96, 2) and (pts >= 0).all() and (pts[:, 0] < TW).all() and (pts[:, 1] < TH).all()
    return frozen(img, pts)


@functools.lru_cache(maxsize=None)
def texture_model(win, stop):
    """(points, exit, reverted, iterations) of the model on the texture at STOPS[stop]."""
    img, pts = texture()
    return frozen(*SR.corner_subpix(img, pts, win, *STOPS[stop], trace=True))


# ---------------------------------------------------------------------------------------------------------------------
# tiny: patches larger than the image
# ---------------------------------------------------------------------------------------------------------------------
TINY = {"8x6": (8, 6, 7), "3x3": (3, 3, 1)}  # (w, h, win): with the 17 x 17 patch of window 7 every tap of the 8 x 6 image is a clamped one


@functools.lru_cache(maxsize=None)
def tiny(name):
    """(image, points): raw noise; the four corners, the centre and sub-pixel positions up to the last quarter pixel inside the image."""
    w, h, _ = TINY[name]
    img = np.random.default_rng(10 * w + h).integers(0, 256, (h, w), dtype=np.uint8)
    fx, fy = (w - 1) / 7.0, (h - 1) / 5.0
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), ((w - 1) / 2, (h - 1) / 2), (w - 0.25, h - 0.25)]
    pts += [(0.25 + fx * (k % 7), 0.5 + fy * (k % 5)) for k in range(1, 11)]
    return frozen(img, np.array(pts, F32))


@functools.lru_cache(maxsize=None)
def tiny_model(name, stop):
    img, pts = tiny(name)
    return frozen(*SR.corner_subpix(img, pts, TINY[name][2], *STOPS[stop], trace=True))


# ---------------------------------------------------------------------------------------------------------------------
# step: one exact step onto the image's edge, of exactly the window's half-size
# ---------------------------------------------------------------------------------------------------------------------
STEP_WIN = 2
STEP_START, STEP_END = (6, 3), (8, 5)
STEP_ROWS = ((133, 122, 136, 116, 127), (133, 116, 150, 128, 128), (136, 105, 127, 127, 127), (139, 128, 128, 128, 128), (127, 127, 127, 127, 127),
             (128, 128, 128, 128, 128), (137, 139, 130, 131, 138))


@functools.lru_cache(maxsize=None)
def step():
    """(image 10 x 8, points [[6, 3]]), for window 2: rows 0 .. 6 of columns 3 .. 7 are STEP_ROWS, an integer solution of the 25 linear equations
    g . (p - (2, 2)) = 0, one for the central-difference gradient g at each offset p of the 5 x 5 window around (6, 3) -- the gradients of a corner at
    (8, 5); columns 8 and 9 are the replicated column 7, whose x-differences vanish.  The start is at whole pixels, where the patch is the image itself,
    and every term is a small integer times a mask value, so the exact solution of the 2 x 2 system is the step (2, 2) and what the float64 sums lose
    rounds away in the float32 coordinate.  The first step therefore lands on x = 8.0 = w exactly, having moved exactly win = 2 both ways: `left` ends
    the loop and `> win` keeps the point.  Nothing else in the suite puts a coordinate ON either threshold; a comparison off by its equality gives
    another result here: `> w` goes on iterating from the edge, where rows 7 .. 9 (noise, like columns 0 .. 2) enter the window, and a revert at
    `>= win` returns the start."""
    img = np.random.default_rng(86).integers(0, 256, (10, 8), dtype=np.uint8)
    img[:7, 3:] = np.array(STEP_ROWS, np.uint8)
    return frozen(img, np.array([STEP_START], F32))


# ---------------------------------------------------------------------------------------------------------------------
# junction: truth by symmetry
# ---------------------------------------------------------------------------------------------------------------------
JUNCTION_TRUTH = (23.5, 19.5)
JUNCTION_WINS = (2, 3, 4, 5, 6, 7)
JUNCTION_STOP = (100, 0.0)  # eps = 0: the stop rule is not what is measured
# max |corner_subpix_f64 - truth| over the 16 starts, per window 2 .. 7, as printed by test_subpix_model_cpu.py::test_junction_truth on the float64
# form of the model (subpix_ref.corner_subpix_f64: the same iteration, no float32 rounding), x86-64, NumPy float64:
JUNCTION_F64_ERR = {"axis": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0), "sheared": (0.0, 0.0, 3.553e-15, 3.553e-15, 3.553e-15, 3.553e-15)}
# the bound on the float32 model and on the device: 4 x the worst float64-form error, plus one float32 ulp of 23.5 (2^-19) for the final rounding of a
# coordinate
JUNCTION_BOUND = 4 * max(max(v) for v in JUNCTION_F64_ERR.values()) + 2.0 ** -19


@functools.lru_cache(maxsize=None)
def junction(kind):
    """48 x 40 image of an X-junction whose corner is (23.5, 19.5), drawn by a sign test in doubled integer coordinates X = 2 x - 47, Y = 2 y - 39
    (both odd, never 0): `axis` has the edges x = cx and y = cy (bright where X Y > 0), `sheared` the edges x = cx and y - cy = (x - cx) / 2
    (bright where X (2 Y - X) > 0; 2 Y - X is odd).  Both sign products are unchanged by (X, Y) -> (-X, -Y), so the uint8 image is exactly
    point-symmetric about the corner; the sheared one is not symmetric under x <-> y."""
    y, x = np.mgrid[0:40, 0:48]
    X, Y = 2 * x - 47, 2 * y - 39
    s = X * Y if kind == "axis" else X * (2 * Y - X)
    assert kind in ("axis", "sheared") and (s != 0).all()
    img = np.where(s > 0, 200, 50).astype(np.uint8)
    assert np.array_equal(img, img[::-1, ::-1])
    return frozen(img)[0]


def junction_starts(win):
    """A 4 x 4 grid of offsets up to win - 1 from the corner, none of them zero, at unequal fractions so that no start is the mirror of another."""
    d = np.array([-1.0, -0.35, 0.4, 1.0]) * (win - 1)
    gx, gy = np.meshgrid(JUNCTION_TRUTH[0] + d, JUNCTION_TRUTH[1] + d[::-1] * 0.9)
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(F32)


def junction_error(p):
    return float(np.abs(np.asarray(p, np.float64) - np.array(JUNCTION_TRUTH)).max())


@functools.lru_cache(maxsize=None)
def junction_model(kind, win, mutate=None):
    return frozen(SR.corner_subpix(junction(kind), junction_starts(win), win, *JUNCTION_STOP, mutate=mutate))[0]


# ---------------------------------------------------------------------------------------------------------------------
# frame 0: the batch kernel behind vh_frame0_init* and the replenishment birth
# ---------------------------------------------------------------------------------------------------------------------
F0_BORDER, F0_CORNERS = (60, 40), 90  # the border clips the plate ROI at the frame on every side; 90 corners span two 64-thread blocks
F0_SIZES = ((96, 64), (80, 56))


@functools.lru_cache(maxsize=None)
def frame0_scene(k):
    """(frame, q, K, roi): F0_SIZES[k] of box-filtered noise, the plate a few pixels wide near the middle, and the ROI (x0, x1, y0, y1) that
    image_ref.bounding_rect gives for it with F0_BORDER -- clipped to [1, w) x [1, h)."""
    import image_ref as IM
    from scenes import camera, plate_quad

    w, h = F0_SIZES[k]
    K = camera(w, h, 150.0)
    q = plate_quad(K, 0.02 - 0.05 * k, 0.01, 3.6)
    roi = IM.bounding_rect(q, (h, w), F0_BORDER)
    assert roi == (1, w, 1, h)
    return frozen(noise_texture(w, h, 40 + k), q, K) + (roi,)


@functools.lru_cache(maxsize=None)
def frame0_model(k, win, use_harris=True, min_distance=0.0):
    """The corners of frame0_scene(k): gftt_ref.good_features on the ROI, moved to the frame, then the model on the FULL frame at (100, 0.001)."""
    import gftt_ref as G

    frame, q, K, (x0, x1, y0, y1) = frame0_scene(k)
    c = G.good_features(frame[y0:y1, x0:x1], F0_CORNERS, 0.01, min_distance, block=5, use_harris=use_harris) + F32([x0, y0])
    return frozen(c, SR.corner_subpix(frame, c, win, 100, 0.001))
