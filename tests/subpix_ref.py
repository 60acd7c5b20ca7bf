"""Exact NumPy model of cv2.cornerSubPix(img, pts, (win, win), (-1, -1), (EPS + MAX_ITER, max_iter, eps)) on a uint8 image, written from OpenCV's
definition as SURVEY.md (section 8f, vidExample.py:113-115) and velocity_amd/csrc/vh_init.hip describe it.  Shared by tests/test_subpix_model_cpu.py,
which holds oracle/klt_oracle.c to it bit for bit, and tests/test_gpu_subpix_model.py, which holds the HIP kernels to it directly.  Nothing here calls
into oracle/ or the library.

Number formats.  Coordinates are float32.  The patch is getRectSubPix(8u -> 32f) of (2 win + 3)^2 pixels: its origin is the float32 c - (pw - 1) * 0.5f
(the product is exact), floor gives the integer part, the fractions a, b and the four weights (1-a)(1-b), a(1-b), (1-a)b, ab are float32; a pixel
converts to float32 exactly and the four taps are added left to right, one float32 rounding per product and per sum (NumPy float32 array arithmetic
rounds every operation and never contracts); tap indices are clamped to the image (replicated border).  The central differences are float32, then
widened to float64.  gxx = (tgx tgx) m, gxy = (tgx tgy) m, gyy = (tgy tgy) m with the float32 mask m widened, all float64; the five sums a, b, c,
bb1 += gxx px + gxy py, bb2 += gxy px + gyy py are float64 and accumulated ONE TERM AT A TIME in row-major order: np.cumsum(...)[-1] adds
sequentially, np.sum adds pairwise and gives other last bits.  det = a c - b b, the break at |det| <= DBL_EPSILON^2, sc = 1 / det,
nx = float32((cx + (c sc) bb1) - (b sc) bb2), ny = float32((cy - (b sc) bb1) + (a sc) bb2) in float64 with one final rounding; err is the sum of the
squares, in float64, of the float32 differences nx - cx, ny - cy.  The comparisons against the image size, eps^2 (float64) and win are exact.

The mask.  OpenCV's window is exp(-y^2) exp(-x^2) with y = float32(i - win) / float32(win), the argument a = float32(-y y) and libm's expf.  np.exp
on a float32 argument is NOT expf: it differs in the last bit at 30 of the 63 arguments that windows 1 .. 7 use.  np.float32(math.exp(float(a))) is
the float64 exponential rounded once to float32, which is what a correctly rounded expf returns unless the float64 result lies within 2^-29 relative of
a float32 rounding boundary; at these 63 arguments it does not, and the expf of the oracle and of the library's host code agrees with it at all 63
(tests/test_subpix_model_cpu.py and tests/test_gpu_subpix_model.py would fail at that window otherwise).  The products vy * vx are float32.

Stop rule.  max_iter is clamped to 1 .. 100 and eps < 0 to 0.  The loop is do { step } while (++iter < max_iter && err > eps^2), left early when det
vanishes (before the point moves) or when the new point lies outside [0, w) x [0, h) (after it has moved).  Finally the point returns to its start if
it has moved more than win in x or in y (float32 difference).

corner_subpix_f64 is the same iteration with every float32 rounding removed: what the exact model approximates, used only to derive the bound of the
truth test, as image_ref.remap_truth is for the remap."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
MAXWIN = 7
DBL_EPSILON = 2.220446049250313e-16
EXITS = ("eps", "iter", "left", "det")
# one deliberate defect each: what tests/test_subpix_model_cpu.py proves the scenes can see
MUTANTS = ("mask_neighbour", "mask_shifted", "mask_npexp", "pairwise_sum", "reflect101", "iter_le", "eps_unsquared", "revert_ge", "inside_gt",
           "bb_swapped")


def mask_offset(win):
    """Where window `win` starts in the table of all seven masks: those of half-sizes 1 .. win - 1 come first."""
    return sum((2 * k + 1) ** 2 for k in range(1, win))


def mask(win, npexp=False):
    """The (2 win + 1)^2 float32 Gaussian window (see the module docstring for why math.exp and not np.exp)."""
    y = np.arange(-win, win + 1).astype(F32) / F32(win)
    a = -(y * y)
    assert a.dtype == F32
    e = np.exp(a) if npexp else np.array([F32(math.exp(float(t))) for t in a], F32)
    return np.outer(e, e)


def mask_table():
    """All seven masks back to back: 679 floats."""
    return np.concatenate([mask(k).ravel() for k in range(1, MAXWIN + 1)])


def _mask_for(win, mutate, real):
    ww = 2 * win + 1
    if real is F64:
        y = np.arange(-win, win + 1, dtype=F64) / win
        e = np.exp(-(y * y))
        return np.outer(e, e).ravel()
    if mutate == "mask_neighbour":  # the table read at the neighbouring window's offset (window 1 has no lower neighbour: the upper one)
        off = mask_offset(win - 1 if win > 1 else 2)
        return mask_table()[off:off + ww * ww].astype(F64)
    if mutate == "mask_shifted":  # transposed (which alone changes nothing: the mask is symmetric) and read one entry late
        return np.roll(mask(win).T.ravel(), -1).astype(F64)
    return mask(win, npexp=mutate == "mask_npexp").ravel().astype(F64)


def _border(i, n, reflect):
    if not reflect:
        return np.clip(i, 0, n - 1)
    if n == 1:
        return np.zeros_like(i)
    i = np.mod(i, 2 * (n - 1))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def rect_subpix(img, c, pw, real=F32, reflect=False):
    """getRectSubPix(8u -> 32f) of a pw x pw patch around each centre of c [k, 2] -> [k, pw, pw] in `real`."""
    h, w = img.shape
    o = c - real(pw - 1) * real(0.5)
    ip = np.floor(o)
    fr = o - ip
    ip = ip.astype(np.int64)
    a, b = fr[:, 0, None, None], fr[:, 1, None, None]
    one = real(1.0)
    a11, a12, a21, a22 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    xs = _border(ip[:, 0, None] + np.arange(pw + 1), w, reflect)[:, None, :]
    ys = _border(ip[:, 1, None] + np.arange(pw + 1), h, reflect)[:, :, None]
    t = img[ys, xs].astype(real)  # [k, pw + 1, pw + 1]
    v = t[:, :-1, :-1] * a11
    v = v + t[:, :-1, 1:] * a12
    v = v + t[:, 1:, :-1] * a21
    v = v + t[:, 1:, 1:] * a22
    assert v.dtype == real
    return v


def _iterate(img, pts, win, max_iter, eps, mutate, real):
    assert mutate is None or mutate in MUTANTS, mutate
    assert 1 <= int(win) <= MAXWIN
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    win = int(win)
    ww, pw = 2 * win + 1, 2 * win + 3
    max_iter = min(max(int(max_iter), 1), 100)
    eps = max(float(eps), 0.0)
    eps2 = eps if mutate == "eps_unsquared" else eps * eps
    start = np.asarray(pts, F32).reshape(-1, 2).astype(real)
    n = len(start)
    m = _mask_for(win, mutate, real)
    off = np.arange(-win, win + 1, dtype=F64)
    px, py = np.tile(off, ww), np.repeat(off, ww)
    total = (lambda t: t.sum(1)) if mutate == "pairwise_sum" else (lambda t: np.cumsum(t, axis=1)[:, -1])
    cur = start.copy()
    iters = np.zeros(n, np.int64)
    exits = np.full(n, "", dtype="U4")
    live = np.arange(n)
    while len(live):
        c0 = cur[live]
        patch = rect_subpix(img, c0, pw, real, reflect=mutate == "reflect101")
        tgx = (patch[:, 1:-1, 2:] - patch[:, 1:-1, :-2]).astype(F64).reshape(len(live), -1)
        tgy = (patch[:, 2:, 1:-1] - patch[:, :-2, 1:-1]).astype(F64).reshape(len(live), -1)
        gxx, gxy, gyy = (tgx * tgx) * m, (tgx * tgy) * m, (tgy * tgy) * m
        t1, t2 = gxx * px + gxy * py, gxy * px + gyy * py
        if mutate == "bb_swapped":
            t1, t2 = t2, t1
        a, b, c, bb1, bb2 = total(gxx), total(gxy), total(gyy), total(t1), total(t2)
        det = a * c - b * b
        dead = np.abs(det) <= DBL_EPSILON * DBL_EPSILON
        sc = 1.0 / np.where(dead, 1.0, det)
        nx = ((c0[:, 0].astype(F64) + (c * sc) * bb1) - (b * sc) * bb2).astype(real)
        ny = ((c0[:, 1].astype(F64) - (b * sc) * bb1) + (a * sc) * bb2).astype(real)
        ex, ey = (nx - c0[:, 0]).astype(F64), (ny - c0[:, 1]).astype(F64)
        err = ex * ex + ey * ey
        if mutate == "inside_gt":
            left = (nx < 0) | (nx > w) | (ny < 0) | (ny > h)
        else:
            left = (nx < 0) | (nx >= w) | (ny < 0) | (ny >= h)
        left &= ~dead
        moved = ~dead
        cur[live[moved], 0], cur[live[moved], 1] = nx[moved], ny[moved]
        it = iters[live] + (~dead & ~left)
        iters[live] = it
        capped = (it > max_iter) if mutate == "iter_le" else (it >= max_iter)
        small = ~(err > eps2)
        kind = np.where(dead, "det", np.where(left, "left", np.where(capped, "iter", np.where(small, "eps", ""))))
        exits[live] = kind
        live = live[kind == ""]
    d = np.abs(cur - start)
    reverted = ((d >= real(win)) if mutate == "revert_ge" else (d > real(win))).any(1)
    cur[reverted] = start[reverted]
    return cur, exits, reverted, iters


def corner_subpix(img, pts, win, max_iter, eps, trace=False, mutate=None):
    """-> float32 [n, 2]; with trace=True also (exit [n] of EXITS, reverted [n] bool, iterations [n]): the exit that ended each corner's loop (`iter`
    where the cap and eps are reached together, as C evaluates ++iter < max_iter first), whether the result went back to the start, and the number of
    completed ++iter.  mutate names one deliberate defect of MUTANTS."""
    out, exits, reverted, iters = _iterate(img, pts, win, max_iter, eps, mutate, F32)
    assert out.dtype == F32
    return (out, exits, reverted, iters) if trace else out


def corner_subpix_f64(img, pts, win, max_iter, eps):
    """The same iteration with no float32 rounding anywhere (coordinates, patch, differences and the mask in float64) -> float64 [n, 2]."""
    return _iterate(img, pts, win, max_iter, eps, None, F64)[0]
