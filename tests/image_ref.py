"""Exact NumPy models of the image stages around the Lucas-Kanade solve: pyrDown and the pyramid's level truncation, the affine remap and the shifted
crop of KLTregional, boundingRect, the nearest-neighbour resize, BGR -> gray and KLTmain's mean translation (utils/KLT.py:55-134,
utils/images.py:9-19).  Shared by tests/test_klt_model_cpu.py, which holds oracle/klt_oracle.c to these models bit for bit, and
tests/test_gpu_klt_model.py, which holds the HIP kernels to them directly.  Nothing here calls into oracle/ or the library.

Number formats.  Pixels are uint8 and every integer stage works on int64 arrays, so nothing can wrap: pyrDown's sum is at most 256 * 255 < 2^16; the
remap's four weights are products of 5-bit fractions times 32 and add up to 2^15, so its sum is at most 255 * 2^15 + 2^14 < 2^23; the gray sum is at most
255 * 32768 + 2^14 < 2^23.  Map coordinates are np.float32 array operations, one rounding per operation as in C without contraction, in the oracle's
order (x * T0 + y * T2) + T4; the fixed-point coordinate rint(m * 32) is formed in float32 (rint: round half to even, like cvRound / lrintf) and must
stay below 2^31 in magnitude -- asserted, a map that far out has no defined C conversion.  boundingRect takes the floor of float32 minima and maxima.
The resize's sizes and source indices are float64, as OpenCV's.  mean_translation sums rint(d * 2^32) of float32 differences d as Python integers:
d * 2^32 is exact in float64, so the rint changes nothing for |d| >= 2^-9 and rounds the tiny ones half to even like llrint; the one conversion of the sum
to float64 and the one division round to nearest, as the C casts do.  remap_truth alone is float64 throughout: it is the un-quantised bilinear sample,
the truth that the fixed-point remap approximates, and only the plane test uses it."""
import numpy as np

F32 = np.float32
KERNEL = np.array([1, 4, 6, 4, 1], np.int64)


def reflect101(i, n):
    """BORDER_REFLECT_101 index of any integer array i into [0, n): gfedcb|abcdefgh|gfedcba, periodic, so any distance beyond the border works;
    a dimension of 1 maps everything to 0."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def pad101(img, border):
    """img with `border` REFLECT_101 pixels on every side, by index."""
    h, w = img.shape
    return img[reflect101(np.arange(-border, h + border), h)][:, reflect101(np.arange(-border, w + border), w)]


def pyr_down(img):
    """cv2.pyrDown of a uint8 image: 5 x 5 [1 4 6 4 1]^2 at the even pixels, REFLECT_101, (sum + 128) >> 8; ((h + 1) // 2, (w + 1) // 2) uint8."""
    h, w = img.shape
    a = np.asarray(img).astype(np.int64)
    dh, dw = (h + 1) // 2, (w + 1) // 2
    taps = np.arange(5) - 2
    cols = reflect101(2 * np.arange(dw)[:, None] + taps, w)  # (dw, 5)
    rows = reflect101(2 * np.arange(dh)[:, None] + taps, h)  # (dh, 5)
    hs = (a[:, cols] * KERNEL).sum(2)  # (h, dw)
    s = (hs[rows, :] * KERNEL[None, :, None]).sum(1)  # (dh, dw)
    return ((s + 128) >> 8).astype(np.uint8)


def pyramid_levels(w, h, win, max_level):
    """Levels calcOpticalFlowPyrLK keeps: level 0 always, a further one only while it is larger than the window in both dimensions."""
    n = 1
    while n <= max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            break
        n += 1
    return n


def pyramid(img, win, max_level):
    """[level 0, level 1, ...] with OpenCV's truncation: stop when the NEXT level would be <= win in either dimension."""
    h, w = img.shape
    levels = [np.ascontiguousarray(img)]
    for _ in range(pyramid_levels(w, h, win, max_level) - 1):
        levels.append(pyr_down(levels[-1]))
    return levels


def _t6(T):
    return np.asarray(T, F32).reshape(6)


def remap_affine(im, T, roi):
    """cv2.remap(im, mapx, mapy, INTER_LINEAR) over the ROI (x0, x1, y0, y1) with the float32 maps [x y 1] T, T 3 x 2 (KLT.py:70-73): coordinates
    quantised to 1/32 px, weights (32 - ax)(32 - ay) 32 ..., constant-0 border tap by tap, (sum + 2^14) >> 15."""
    T = _t6(T)
    h, w = im.shape
    x0, x1, y0, y1 = (int(v) for v in roi)
    x = np.arange(x0, x1).astype(F32)[None, :]
    y = np.arange(y0, y1).astype(F32)[:, None]
    mx = (x * T[0] + y * T[2]) + T[4]
    my = (x * T[1] + y * T[3]) + T[5]
    qx, qy = np.rint(mx * F32(32.0)), np.rint(my * F32(32.0))
    assert (np.abs(qx) < 2.0 ** 31).all() and (np.abs(qy) < 2.0 ** 31).all()
    qx, qy = qx.astype(np.int64), qy.astype(np.int64)
    sx, sy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    a = np.asarray(im).astype(np.int64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside, a[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)

    s = (tap(sy, sx) * ((32 - ax) * (32 - ay) * 32) + tap(sy, sx + 1) * (ax * (32 - ay) * 32)
         + tap(sy + 1, sx) * ((32 - ax) * ay * 32) + tap(sy + 1, sx + 1) * (ax * ay * 32))
    return ((s + (1 << 14)) >> 15).astype(np.uint8)


def remap_truth(im, T, roi):
    """float64 bilinear sample of im at the float64 map of the float32 T, zero outside the frame: what remap_affine approximates."""
    T = _t6(T).astype(np.float64)
    h, w = im.shape
    x0, x1, y0, y1 = (int(v) for v in roi)
    x = np.arange(x0, x1, dtype=np.float64)[None, :]
    y = np.arange(y0, y1, dtype=np.float64)[:, None]
    mx, my = x * T[0] + y * T[2] + T[4], x * T[1] + y * T[3] + T[5]
    fx, fy = np.floor(mx), np.floor(my)
    ax, ay = mx - fx, my - fy
    sx, sy = fx.astype(np.int64), fy.astype(np.int64)
    a = np.asarray(im).astype(np.float64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside, a[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0.0)

    return (tap(sy, sx) * (1 - ax) * (1 - ay) + tap(sy, sx + 1) * ax * (1 - ay) + tap(sy + 1, sx) * (1 - ax) * ay + tap(sy + 1, sx + 1) * ax * ay)


def crop_shift(im, roi, dx, dy):
    """im[y0 + dy:y1 + dy, x0 + dx:x1 + dx] with zeros where that leaves the frame (KLT.py:65-68, SURVEY App. B intent)."""
    h, w = im.shape
    x0, x1, y0, y1 = (int(v) for v in roi)
    sx = np.arange(x0, x1)[None, :] + int(dx)
    sy = np.arange(y0, y1)[:, None] + int(dy)
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    return np.where(inside, np.asarray(im)[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], 0).astype(np.uint8)


def bounding_rect(p, shape, border=(0, 0)):
    """boundingRect(p, imshape, border) of utils/images.py:9-19 -> (x0, x1, y0, y1): cv2.boundingRect of float points is the floor of the minima and
    floor of the maxima + 1; the border is added; the lower clamp is 1 (as the reference has it), the upper clamp the frame's width / height.
    No points: the empty ROI (1, 1, 1, 1)."""
    p = np.asarray(p, F32).reshape(-1, 2)
    if not len(p):
        return (1, 1, 1, 1)
    imh, imw = int(shape[0]), int(shape[1])
    bx, by = int(border[0]), int(border[1])
    x0, y0 = int(np.floor(p[:, 0].min())), int(np.floor(p[:, 1].min()))
    x1, y1 = int(np.floor(p[:, 0].max())) + 1 + bx, int(np.floor(p[:, 1].max())) + 1 + by
    return (max(x0 - bx, 1), min(x1, imw), max(y0 - by, 1), min(y1, imh))


def resize_nearest(img, fx, fy=None):
    """cv2.resize(img, (0, 0), fx=fx, fy=fy, interpolation=INTER_NEAREST): size rint(w fx) x rint(h fy), source min(floor(x (1 / fx)), w - 1)."""
    fy = fx if fy is None else fy
    h, w = img.shape[:2]
    dw, dh = int(np.rint(w * float(fx))), int(np.rint(h * float(fy)))
    sx = np.minimum(np.floor(np.arange(dw, dtype=np.float64) * (1.0 / float(fx))).astype(np.int64), w - 1)
    sy = np.minimum(np.floor(np.arange(dh, dtype=np.float64) * (1.0 / float(fy))).astype(np.int64), h - 1)
    return np.ascontiguousarray(np.asarray(img)[np.ix_(sy, sx)])


def bgr2gray(bgr):
    """cv2.cvtColor(bgr, COLOR_BGR2GRAY) of 8-bit pixels: (3735 B + 19235 G + 9798 R + 2^14) >> 15."""
    a = np.asarray(bgr).astype(np.int64)
    return ((a[..., 0] * 3735 + a[..., 1] * 19235 + a[..., 2] * 9798 + (1 << 14)) >> 15).astype(np.uint8)


def mean_translation(p0, p, v):
    """Mean of p - p0 over the valid tracks (KLT.py:121-123) -> (2,) float64: float32 differences, each rint(d 2^32) summed exactly, one conversion
    of the sum to float64 and one division by the count.  No valid track: zeros."""
    p0, p = np.asarray(p0, F32).reshape(-1, 2), np.asarray(p, F32).reshape(-1, 2)
    v = np.asarray(v).astype(bool)
    d = (p - p0)[v]  # float32
    c = len(d)
    if not c:
        return np.zeros(2)
    q = np.rint(d.astype(np.float64) * 2.0 ** 32)
    assert (np.abs(q) < 2.0 ** 62).all()
    sums = [sum(int(t) for t in q[:, k]) for k in (0, 1)]
    return np.array([float(s) * 2.0 ** -32 / float(c) for s in sums])
