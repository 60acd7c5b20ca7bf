"""NumPy restatement of goodFeaturesToTrack as vh_good_features2 / vh_frame0_init_batch2 compute it (include/velocity_hip.h), shared by
tests/test_gftt_cpu.py and tests/test_gpu_gftt.py.

Response: integer Sobel pair (aperture 3) and block x block box sums (anchor block / 2), REFLECT_101 at the image border, scaled by
s2 = float32(scale^2), scale = 1 / (4 block 255); Harris or OpenCV's calcMinEigenVal on that tensor, every step rounded to float32 (NumPy float32
arithmetic rounds each operation and never contracts).  Threshold: quality x the maximum over the pixels the mask keeps.  Candidates: the interior
3x3 maxima of the thresholded response that the mask keeps, ordered by the 64-bit key (response bits << 32 | pixel index) descending.  Spacing:
greedy in that order (spread_greedy); spread_grid is OpenCV's cell grid, which the CPU tests hold equal to it."""
import numpy as np


def sobel(img):
    """(dx, dy) int32 of a uint8 image, REFLECT_101 border."""
    a = np.pad(np.ascontiguousarray(img).astype(np.int32), 1, mode="reflect")
    dx = (a[:-2, 2:] - a[:-2, :-2]) + 2 * (a[1:-1, 2:] - a[1:-1, :-2]) + (a[2:, 2:] - a[2:, :-2])
    dy = (a[2:, :-2] - a[:-2, :-2]) + 2 * (a[2:, 1:-1] - a[:-2, 1:-1]) + (a[2:, 2:] - a[:-2, 2:])
    return dx, dy


def structure_sums(img, block):
    """Integer box sums (sxx, sxy, syy) over [x - block/2, x - block/2 + block), REFLECT_101 relative to the image."""
    dx, dy = sobel(img)
    h, w = dx.shape
    r0 = block // 2
    out = []
    for prod in (dx * dx, dx * dy, dy * dy):
        p = np.pad(prod.astype(np.int64), ((r0, block - 1 - r0), (r0, block - 1 - r0)), mode="reflect")
        s = np.zeros((h, w), np.int64)
        for j in range(block):
            for i in range(block):
                s += p[j:j + h, i:i + w]
        out.append(s)
    return out


def _s2(block):
    scale = 1.0 / (4.0 * block * 255.0)
    return np.float32(scale * scale)


def harris_response(img, block=3, k=0.04):
    sxx, sxy, syy = structure_sums(img, block)
    s2, kf = _s2(block), np.float32(k)
    a, b, c = sxx.astype(np.float32) * s2, sxy.astype(np.float32) * s2, syy.astype(np.float32) * s2
    tr = a + c
    return (a * c - b * b) - (kf * tr) * tr


def min_eig_response(img, block=3):
    sxx, sxy, syy = structure_sums(img, block)
    s2, half = _s2(block), np.float32(0.5)
    a, b, c = (sxx.astype(np.float32) * s2) * half, sxy.astype(np.float32) * s2, (syy.astype(np.float32) * s2) * half
    d = a - c
    return (a + c) - np.sqrt(d * d + b * b)


def response(img, block=3, use_harris=True, k=0.04):
    return harris_response(img, block, k) if use_harris else min_eig_response(img, block)


def candidate_keys(resp, quality, mask=None):
    """The candidates' 64-bit keys, descending (the order of the corners before any spacing)."""
    resp = np.asarray(resp, np.float32)
    h, w = resp.shape
    keep = np.ones((h, w), bool) if mask is None else (np.asarray(mask) != 0)
    if not keep.any():
        return np.zeros(0, np.uint64)
    thr = np.float32(float(resp[keep].max()) * quality)
    t = np.where(resp > thr, resp, np.float32(-np.inf))
    v = resp[1:-1, 1:-1]
    m = v.copy()
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            m = np.maximum(m, t[1 + j:h - 1 + j, 1 + i:w - 1 + i])
    hit = (v > thr) & (v == m) & (v != 0) & keep[1:-1, 1:-1]
    ys, xs = np.nonzero(hit)
    ys, xs = ys + 1, xs + 1
    keys = (resp[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64)
    return np.sort(keys)[::-1]


def keys_xy(keys, w):
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.stack([idx % w, idx // w], 1)


def spread_greedy(xy, min_distance, max_corners):
    """Indices into xy (in order) kept by the greedy rule: a point is kept iff no point kept before it lies at squared distance < min_distance^2."""
    md2 = float(min_distance) * float(min_distance)
    kept = []
    ax = np.empty(max(max_corners, 1), np.int64)
    ay = np.empty(max(max_corners, 1), np.int64)
    for i, (x, y) in enumerate(np.asarray(xy, np.int64)):
        n = len(kept)
        if n and bool((((ax[:n] - x) ** 2 + (ay[:n] - y) ** 2) < md2).any()):
            continue
        ax[n], ay[n] = x, y
        kept.append(i)
        if len(kept) == max_corners:
            break
    return np.asarray(kept, np.int64)


def spread_grid(xy, w, h, min_distance, max_corners):
    """OpenCV's spacing: cells of cvRound(min_distance) pixels, a point checked against the points kept in the 3 x 3 cells around its own."""
    cell = int(np.round(min_distance))  # cvRound: half to even
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    grid = [[] for _ in range(gw * gh)]
    md2 = float(min_distance) * float(min_distance)
    kept = []
    for i, (x, y) in enumerate(np.asarray(xy, np.int64)):
        cx, cy = int(x) // cell, int(y) // cell
        good = True
        for yy in range(max(cy - 1, 0), min(cy + 1, gh - 1) + 1):
            for xx in range(max(cx - 1, 0), min(cx + 1, gw - 1) + 1):
                for (mx, my) in grid[yy * gw + xx]:
                    dx, dy = np.float32(x) - mx, np.float32(y) - my
                    if float(dx * dx + dy * dy) < md2:
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid[cy * gw + cx].append((np.float32(x), np.float32(y)))
            kept.append(i)
            if len(kept) == max_corners:
                break
    return np.asarray(kept, np.int64)


def good_features(img, max_corners, quality, min_distance=0.0, mask=None, block=3, use_harris=True, k=0.04):
    """-> float32 [n, 2] (x, y) in image coordinates, in the device's order."""
    img = np.ascontiguousarray(img)
    h, w = img.shape
    keys = candidate_keys(response(img, block, use_harris, k), quality, mask)
    xy = keys_xy(keys, w)
    if min_distance >= 1:
        xy = xy[spread_greedy(xy, min_distance, max_corners)]
    else:
        xy = xy[:max_corners]
    return xy.astype(np.float32).reshape(-1, 2)
