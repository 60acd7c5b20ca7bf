"""Exact-integer NumPy model of Lucas-Kanade tracking as the reference uses it: one pyramid level (lk_level), the
pyramidal descent of cv2.calcOpticalFlowPyrLK (pyr_lk), the forward-backward gate of cv2calcOpticalFlowPyrLK (lk_fb, utils/KLT.py:37-51) and
KLTregional (klt_regional, utils/KLT.py:55-95) on top of the image stages of tests/image_ref.py; and the worst-case-contrast scenes and track sets
that the single-level tests share (tests/test_lk_ref_cpu.py, tests/test_gpu_lk_extremes.py).  tests/test_klt_model_cpu.py holds the oracle to the whole
call, tests/test_gpu_klt_model.py the kernels.

The oracle (oracle/klt_oracle.c) keeps every window sum in int64 and the HIP kernels (velocity_amd/csrc/vh_lk.hip) reproduce it bit for bit with int32
per-lane partials, 16-bit halves and 24-bit multiply-adds, each on the argument that 8-bit images cannot produce larger operands.  This module restates
the level independently of both -- all tracks at once, whole windows as arrays -- and reports the largest window sums it met, so a test can assert how
close to those operand limits its scenes really come.

The descent.  A level's positions are the full-resolution ones times float32(1 / 2^level), a power of two, so the scaling is exact.  The top level
starts at the scaled point, every lower one at twice the level above's result (exact again).  Status and err belong to level 0 alone: an upper level
that cannot start (window origin further out than a window) or that fails the min-eigenvalue test hands its guess down unchanged and says nothing.
The backward pass of lk_fb starts from the forward result; the error sqrt(dx dx + dy dy) and its comparison with the threshold are float32, and a NaN
compares false.  klt_regional subtracts and adds the ROI origin and maps back through T in float32, (ax T0 + ay T2) + T4, one rounding per operation.

Number formats.  Pixels, gradients, bilinear samples and the products of two samples are int32 arrays, and none of them can wrap: the weights are
non-negative and add up to 2^14, so a weighted sample is at most 4080 * 2^14 + 2^13 < 2^27, and a product of two samples is at most
8160 * 4080 < 2^25.  Every window sum is accumulated in int64: at most 2^14 pixels (win <= 128) of less than 2^25 each stay below 2^39.
Every floating-point step is an np.float32 array operation, one rounding per operation as in C without contraction, in the oracle's order; only the
eps^2 test is float64.  int64 -> float32 conversions round to nearest even, as the C cast does."""
import functools

import numpy as np

import image_ref as IM
from _helpers import frozen

F32 = np.float32
W_BITS = 14
FLT_SCALE = F32(2.0 ** -20)
FLT_EPSILON = F32(1.1920929e-07)
MIN_EIG_THR = F32(1e-4)
GX_MAX = 255 * 16  # largest |Scharr| of an 8-bit image: (3 + 10 + 3) * 255
DIFF_MAX = 255 * 32  # largest |J - I| of the x32 bilinear samples
W, H = 192, 160  # every scene below


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def scharr(img):
    """(Ix, Iy) int32 of a uint8 image: smoothing [3 10 3], difference [-1 0 1], no normalisation, REFLECT_101 support."""
    p = IM.pad101(img.astype(np.int32), 1)  # by index, so a dimension of 1 works too
    sm = 3 * (p[:-2, :] + p[2:, :]) + 10 * p[1:-1, :]  # vertical smoothing, all columns
    dv = p[2:, :] - p[:-2, :]  # vertical difference, all columns
    return sm[:, 2:] - sm[:, :-2], 3 * (dv[:, 2:] + dv[:, :-2]) + 10 * dv[:, 1:-1]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _weights(a, b):
    """14-bit bilinear weights of the float32 fractions (a along x, b along y), each (m, 1, 1) int32; the fourth is the remainder."""
    one, sc = F32(1.0), F32(1 << W_BITS)
    w00 = np.rint((one - a) * (one - b) * sc).astype(np.int32)  # rint: round half to even, like cvRound
    w01 = np.rint(a * (one - b) * sc).astype(np.int32)
    w10 = np.rint((one - a) * b * sc).astype(np.int32)
    w11 = (1 << W_BITS) - w00 - w01 - w10
    return [w[:, None, None] for w in (w00, w01, w10, w11)]


def _origin(x, y, win, w, h):
    """Window origin of the float32 corner (x, y): (inside, ix, iy, frac x, frac y).  `inside` is the oracle's rule -win <= origin < size; an
    origin that is not a number or beyond int32 counts as outside (the C cast of such a float gives INT_MIN on x86)."""
    fx, fy = np.floor(x), np.floor(y)
    with np.errstate(invalid="ignore"):
        inside = (fx >= -win) & (fx < w) & (fy >= -win) & (fy < h)
    ix = np.where(inside, fx, 0).astype(np.int64)
    iy = np.where(inside, fy, 0).astype(np.int64)
    return inside, ix, iy, (x - ix.astype(F32)).astype(F32), (y - iy.astype(F32)).astype(F32)


def _sample(planes, ix, iy, a, b, win, shifts):
    """Bilinear samples of the win x win windows at origins (ix, iy) in every padded plane: list of (m, win, win) int32."""
    k = np.arange(win + 1)
    rows = (iy[:, None] + win + k)[:, :, None]  # (the planes carry a border of `win`)
    cols = (ix[:, None] + win + k)[:, None, :]
    w00, w01, w10, w11 = _weights(a, b)
    out = []
    for p, sh in zip(planes, shifts):
        g = p[rows, cols]
        out.append(_descale(g[:, :-1, :-1] * w00 + g[:, :-1, 1:] * w01 + g[:, 1:, :-1] * w10 + g[:, 1:, 1:] * w11, sh))
    return out


def _wsum(x):
    """Exact window sums of (m, win, win) int32 terms."""
    return x.sum((1, 2), dtype=np.int64)


def _f32_of(s):
    return s.astype(F32) * FLT_SCALE


def _criteria(max_count, eps):
    """OpenCV's clamp of the termination criteria -> (max_count, eps^2)."""
    return min(max(int(max_count), 0), 100), min(max(float(eps), 0.0), 10.0) ** 2


def _new_peaks():
    return dict(A11=0, A12=0, A22=0, b1=0, b2=0, Ix=0, Iy=0, diff=0, b1_min=0, b2_min=0)


def lk_level(prev, nxt, pts, guess, level, top_level, win, max_count, eps2, status, err, peaks=None):
    """One level of calcOpticalFlowPyrLK for every track: prev / nxt are that level's images, pts (n, 2) float32 the FULL-resolution points, guess
    (n, 2) float32 the level above's result (ignored on the top level), max_count and eps2 already clamped (_criteria).  Returns this level's
    positions (n, 2) float32.  status (n,) bool and err (n,) float32 are updated in place, and only when level == 0; a track that cannot start or
    fails the min-eigenvalue test on an upper level keeps its starting guess.  peaks: a _new_peaks() dict to update (see lk_level0), or None."""
    assert prev.shape == nxt.shape and prev.dtype == np.uint8 and nxt.dtype == np.uint8 and 3 <= win <= 128
    h, w = prev.shape
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    base = level == 0
    peaks = _new_peaks() if peaks is None else peaks

    gx, gy = scharr(prev)
    pI = IM.pad101(prev.astype(np.int32), win)
    pJ = IM.pad101(nxt.astype(np.int32), win)
    pGx, pGy = np.pad(gx, win), np.pad(gy, win)  # gradients: zero outside the image

    half = F32((win - 1) * F32(0.5))
    lpts = pts * F32(1.0 / (1 << level))
    nxt_pt = lpts.copy() if level == top_level else np.ascontiguousarray(guess, F32).reshape(-1, 2) * F32(2.0)

    def peak(name, s):
        if s.size:
            peaks[name] = max(peaks[name], int(np.abs(s).max()))

    def drop(idx):
        if base:
            status[idx] = False

    # template: the window of prev at the track, its gradients, the structure tensor
    ok, ipx, ipy, a, b = _origin(lpts[:, 0] - half, lpts[:, 1] - half, win, w, h)
    drop(~ok)
    if base:
        err[~ok] = F32(0.0)
    live = np.flatnonzero(ok)
    Iw, Ix, Iy = _sample((pI, pGx, pGy), ipx[live], ipy[live], a[live], b[live], win, (W_BITS - 5, W_BITS, W_BITS))
    s11, s12, s22 = _wsum(Ix * Ix), _wsum(Ix * Iy), _wsum(Iy * Iy)
    peak("A11", s11), peak("A12", s12), peak("A22", s22), peak("Ix", Ix), peak("Iy", Iy)
    A11, A12, A22 = _f32_of(s11), _f32_of(s12), _f32_of(s22)
    D = A11 * A22 - A12 * A12
    min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4.0) * A12 * A12)) / F32(2 * win * win)
    good = ~((min_eig < MIN_EIG_THR) | (D < FLT_EPSILON))
    drop(live[~good])
    live, Iw, Ix, Iy, A11, A12, A22 = live[good], Iw[good], Ix[good], Iy[good], A11[good], A12[good], A22[good]
    D = F32(1.0) / D[good]

    # Newton iterations on the tracks still running; `cur` indexes into `live`
    m = len(live)
    nx, ny = nxt_pt[live, 0] - half, nxt_pt[live, 1] - half
    pdx, pdy = np.zeros(m, F32), np.zeros(m, F32)
    cur = np.arange(m)
    for j in range(max_count):
        ok, inx, iny, a, b = _origin(nx[cur], ny[cur], win, w, h)
        drop(live[cur[~ok]])
        cur, inx, iny, a, b = cur[ok], inx[ok], iny[ok], a[ok], b[ok]
        if not len(cur):
            break
        diff = _sample((pJ,), inx, iny, a, b, win, (W_BITS - 5,))[0] - Iw[cur]
        sb1, sb2 = _wsum(diff * Ix[cur]), _wsum(diff * Iy[cur])
        peak("b1", sb1), peak("b2", sb2), peak("diff", diff)
        peaks["b1_min"], peaks["b2_min"] = min(peaks["b1_min"], int(sb1.min())), min(peaks["b2_min"], int(sb2.min()))
        b1, b2 = _f32_of(sb1), _f32_of(sb2)
        with np.errstate(over="ignore", invalid="ignore"):
            dx = (A12[cur] * b2 - A22[cur] * b1) * D[cur]
            dy = (A12[cur] * b1 - A11[cur] * b2) * D[cur]
            nx[cur] = nx[cur] + dx
            ny[cur] = ny[cur] + dy
            t = live[cur]
            nxt_pt[t, 0], nxt_pt[t, 1] = nx[cur] + half, ny[cur] + half
            small = dx.astype(np.float64) * dx.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64) <= eps2
            osc = ~small & (j > 0) & (np.abs(dx + pdx[cur]) < F32(0.01)) & (np.abs(dy + pdy[cur]) < F32(0.01))
            nxt_pt[t[osc], 0] -= dx[osc] * F32(0.5)
            nxt_pt[t[osc], 1] -= dy[osc] * F32(0.5)
        pdx[cur], pdy[cur] = dx, dy
        cur = cur[~(small | osc)]

    if not base:
        return nxt_pt

    # err of the tracks still alive: mean |diff| of the final window, in intensity units
    fin = np.flatnonzero(status[live])
    ok, inx, iny, a, b = _origin(nxt_pt[live[fin], 0] - half, nxt_pt[live[fin], 1] - half, win, w, h)
    status[live[fin[~ok]]] = False
    fin, inx, iny, a, b = fin[ok], inx[ok], iny[ok], a[ok], b[ok]
    if len(fin):
        diff = _sample((pJ,), inx, iny, a, b, win, (W_BITS - 5,))[0] - Iw[fin]
        err[live[fin]] = _wsum(np.abs(diff)).astype(F32) * (F32(1.0) / F32(32 * win * win))
    return nxt_pt


def lk_level0(prev, nxt, pts, win, max_count, eps):
    """(next (n, 2) float32, status (n,) bool, err (n,) float32, peaks) of calcOpticalFlowPyrLK(prev, nxt, pts, winSize=(win, win), maxLevel=0,
    criteria=(COUNT | EPS, max_count, eps)): the one-level call of lk_level.  peaks: the largest |A11|, |A12|, |A22|, |b1|, |b2| integer window sums
    over every track and iteration, the largest single |Ix|, |Iy| and |diff| sample, and the most negative b1 and b2 sums (b1_min, b2_min), as
    Python ints."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    max_count, eps2 = _criteria(max_count, eps)
    status, err, peaks = np.ones(len(pts), bool), np.zeros(len(pts), F32), _new_peaks()
    nxt_pt = lk_level(prev, nxt, pts, None, 0, 0, win, max_count, eps2, status, err, peaks)
    return nxt_pt, status, err, peaks


def pyr_lk(prev, nxt, pts, win, max_level, max_count, eps):
    """(next (n, 2) float32, status (n,) bool, err (n,) float32) of calcOpticalFlowPyrLK(prev, nxt, pts, winSize=(win, win), maxLevel=max_level,
    criteria=(COUNT | EPS, max_count, eps)): the pyramids of image_ref.pyramid, lk_level from the top level down."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    max_count, eps2 = _criteria(max_count, eps)
    pI, pJ = IM.pyramid(prev, win, max_level), IM.pyramid(nxt, win, max_level)
    top = len(pI) - 1
    status, err = np.ones(len(pts), bool), np.zeros(len(pts), F32)
    guess = np.zeros_like(pts)
    for level in range(top, -1, -1):
        guess = lk_level(pI[level], pJ[level], pts, guess, level, top, win, max_count, eps2, status, err)
    return guess, status, err


def lk_fb(im1, im2, p1, fbt=None, win=15, max_level=4, max_count=10, eps=0.1):
    """cv2calcOpticalFlowPyrLK (utils/KLT.py:37-51) -> (p2, v, err, fbe): forward pyr_lk; with a threshold (fbt neither None nor negative) a backward
    pyr_lk from p2, fbe = |p1 - p1'| in float32 and v = v & v2 & (fbe < fbt), where a NaN compares false.  Without one fbe is zero."""
    p1 = np.ascontiguousarray(p1, F32).reshape(-1, 2)
    p2, v, err = pyr_lk(im1, im2, p1, win, max_level, max_count, eps)
    fbe = np.zeros(len(p1), F32)
    if fbt is not None and F32(fbt) >= 0:
        p1b, v2, _ = pyr_lk(im2, im1, p2, win, max_level, max_count, eps)
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy = p1[:, 0] - p1b[:, 0], p1[:, 1] - p1b[:, 1]
            fbe = np.sqrt(dx * dx + dy * dy)
            v = v & v2 & (fbe < F32(fbt))
    return p2, v, err, fbe


def klt_regional(im0, im, p0, T, lk, fbt=1.0, translate=False):
    """KLTregional (utils/KLT.py:55-95) -> (p (n, 2) float32, v (n,) bool, roi (x0, x1, y0, y1), warped): the ROI is boundingRect(p0, border 50);
    `im` is cropped at the integer shift int(T[4]), int(T[5]) (truncated towards zero; translate) or remapped through the float32 T (3 x 2) over it;
    lk_fb tracks p0 - origin from im0's ROI into that; the origin is added back and the result shifted or mapped through T.  lk: dict(win,
    max_level, max_count, eps).  At least one point."""
    p0 = np.ascontiguousarray(p0, F32).reshape(-1, 2)
    T = np.asarray(T, F32).reshape(6)
    roi = IM.bounding_rect(p0, im0.shape, (50, 50))
    x0, x1, y0, y1 = roi
    org = np.array([x0, y0], F32)
    dx, dy = int(T[4]), int(T[5])
    warped = IM.crop_shift(im, roi, dx, dy) if translate else IM.remap_affine(im, T, roi)
    pa, v, _, _ = lk_fb(np.ascontiguousarray(im0[y0:y1, x0:x1]), warped, p0 - org, fbt, **lk)
    with np.errstate(over="ignore", invalid="ignore"):
        a = pa + org
        if translate:
            p = a + np.array([dx, dy], F32)
        else:
            p = np.stack([(a[:, 0] * T[0] + a[:, 1] * T[2]) + T[4], (a[:, 0] * T[1] + a[:, 1] * T[3]) + T[5]], 1)
    return p.astype(F32), v, roi, warped


# ---------------------------------------------------------------------------------------------------------------------
# scenes: 192 x 160 binary frame pairs at the largest gradients and differences 8-bit images can hold
# ---------------------------------------------------------------------------------------------------------------------
def sign_pair(I, axis=1, negate=False):
    """J = 255 where the Scharr gradient of I along `axis` (1: x, 0: y) is positive, 0 where it is negative, I elsewhere: |J - I| = 255 with the
    gradient's sign on as many edge pixels as a binary pair allows (about half of them: the others already hold the value the rule asks for).
    negate: 0 where it is positive, 255 where it is negative -- the same magnitudes with diff.gradient <= 0 everywhere."""
    g = scharr(I)[0 if axis == 1 else 1]
    return np.where(g > 0, 0 if negate else 255, np.where(g < 0, 255 if negate else 0, I)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def bars(k, negate=False):
    """Vertical bars 0, 0, 255, 255 (|Ix| = 4080 at every pixel of a uniform column run), shifted by 2 px every k rows so that Iy is not zero."""
    y, x = np.mgrid[0:H, 0:W]
    I = (255 * (((x + 2 * ((y // k) % 2)) // 2) % 2)).astype(np.uint8)
    return frozen(I, sign_pair(I, 1, negate))


@functools.lru_cache(maxsize=None)
def bars_t(k):
    """bars(k) with x and y exchanged: loads Iy, A22 and b2."""
    y, x = np.mgrid[0:H, 0:W]
    I = (255 * (((y + 2 * ((x // k) % 2)) // 2) % 2)).astype(np.uint8)
    return frozen(I, sign_pair(I, 0))


@functools.lru_cache(maxsize=None)
def checker(cell, inverse=False):
    """Checkerboard of cell x cell squares, a quarter of the cells inverted at random (fixed seed): both gradients and the mixed sum are loaded.
    J by the sign rule, or 255 - I (inverse)."""
    rng = np.random.default_rng(7000 + cell)
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = y // cell, x // cell
    flip = rng.random((H // cell + 1, W // cell + 1)) < 0.25
    I = (255 * ((cx + cy + flip[cy, cx]) % 2)).astype(np.uint8)
    return frozen(I, (255 - I).astype(np.uint8) if inverse else sign_pair(I, 1))


SCENES = {f"bars{k}": functools.partial(bars, k) for k in (8, 16)}
SCENES["bars16_neg"] = functools.partial(bars, 16, True)  # the first Newton step's diff.Ix sum at its most NEGATIVE (the sign rule alone only gives positive ones)
SCENES.update({f"bars_t{k}": functools.partial(bars_t, k) for k in (8, 16)})
SCENES.update({f"checker{c}": functools.partial(checker, c) for c in (2, 3, 4, 6)})
SCENES.update({f"checker{c}_inv": functools.partial(checker, c, True) for c in (2, 3, 4, 6)})

OFFSETS = ("int", "half", "quarter", "rand")


@functools.lru_cache(maxsize=None)
def tracks(win, offset):
    """A grid of tracks whose windows lie inside the frame (pitch 10 px, wider where that would give more than 200), displaced by `offset` ('int': none,
    'half': (+0.5, +0.5), 'quarter': (+0.25, +0.75), 'rand': a seeded fraction per track), and a ring of 48 tracks within `win` of each border and
    beyond it, on both sides of the start-position rule (status 0 once the window origin is further out than `win`)."""
    lo = (win - 1) // 2 + 1
    pitch = 10
    while len(range(lo, W - 1 - lo, pitch)) * len(range(lo, H - 1 - lo, pitch)) > 200:
        pitch += 1
    gx, gy = np.meshgrid(np.arange(lo, W - 1 - lo, pitch), np.arange(lo, H - 1 - lo, pitch))
    grid = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64)
    rng = np.random.default_rng(100 * win + OFFSETS.index(offset))
    grid += {"int": (0.0, 0.0), "half": (0.5, 0.5), "quarter": (0.25, 0.75), "rand": rng.random(grid.shape)}[offset]
    d = rng.uniform(-win - 2.0, win, 48)  # distance from the border, inwards
    along = rng.random(48)
    side = np.arange(48) % 4
    ring = np.where((side < 2)[:, None], np.stack([np.where(side == 0, d, W - 1 - d), along * H], 1), np.stack([along * W, np.where(side == 2, d, H - 1 - d)], 1))
    return frozen(np.concatenate([grid, ring]).astype(F32))[0]


CRITERIA = ((1, 0.0), (10, 0.03), (30, 0.001))  # (max_count, eps): one Newton step, the coarse stage's kind, the fine stage's kind



@functools.lru_cache(maxsize=None)
def model(scene, win, offset, max_count, eps):
    """lk_level0 of a named scene and track set: computed once, shared by every test, never written to."""
    I, J = SCENES[scene]()
    p, s, e, peaks = lk_level0(I, J, tracks(win, offset), win, max_count, eps)
    return frozen(p, s, e) + (peaks,)
