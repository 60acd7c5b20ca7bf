"""NumPy model of vh_match_affine (include/velocity_hip.h): the stand-in for estimateAffine2D_SURF(im1, im2, p1, scale=1), utils/KLT.py:10-33, shared by
tests/test_match_cpu.py and tests/test_gpu_match.py.  The kernels of velocity_amd/csrc/vh_match.hip are held to this file bit for bit.

1. Levels: `levels` images per frame at s_l = 2^(-l/4); level l > 0 is level 0 resampled bilinearly (klt_oracle.remap_affine, the checker of
   vh_remap_affine) with T = [[1/s, 0], [0, 1/s], [0.5/s - 0.5, 0.5/s - 0.5]] (float32) over (0, rint(W s), 0, rint(H s)).
2. Keypoints: per level tests/gftt_ref.good_features (Shi-Tomasi, block 5, quality 0.01, minDistance 0) under a mask that keeps the pixels at least
   BORDER = 16 px from every edge; for the query image also inside boundingRect(p1, shape, border) with every bound multiplied by float32(s_l) in float32
   and truncated.  Level-0 position of a keypoint: (x + 0.5) * float32(1 / s_l) - 0.5, float32, multiply and subtract rounded separately.
3. Descriptor: 256 bits, bit k = box5(y + ay_k, x + ax_k) < box5(y + by_k, x + bx_k) on the 5x5 integer box sum of the level image (zero outside it;
   no pixel outside is ever read), offsets from velocity_amd/csrc/vh_match_pairs.hpp, packed most significant bit first (np.packbits).
4. Matching: nearest and second nearest train descriptor by (Hamming distance, train index) ascending; train order level-major, detector order within
   a level.  Good iff ratio_den * d1 < ratio_num * d2 (5 d1 < 4 d2).  Fewer than two train descriptors: nothing is good.
5. Model: klt_oracle.ransac_affine (the checker of vh_ransac_affine) on the good pairs in query order; fewer than min_good good pairs (or fewer than
   three), or no RANSAC model: status 0."""
import os
import re

import numpy as np

import gftt_ref as G
from oracle import klt_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS_HEADER = os.path.join(ROOT, "velocity_amd", "csrc", "vh_match_pairs.hpp")
BORDER = 16  # the descriptor reaches 13 + 2 px
DEFAULTS = dict(levels=5, query_per_level=500, train_per_level=1000, block=5, border_x=50, border_y=50, ratio_num=4, ratio_den=5, min_good=10, quality=0.01)


def pair_table():
    """The 256 x 4 offsets (ax, ay, bx, by) the kernel compiles, parsed from its header."""
    txt = open(PAIRS_HEADER).read()
    rows = re.findall(r"\{\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*\}", txt)
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def level_scale(l):
    return 2.0 ** (-l / 4.0)


def level_dims(w, h, l):
    s = level_scale(l)
    return (w, h) if l == 0 else (int(np.rint(w * s)), int(np.rint(h * s)))


def level_image(im, l):
    if l == 0:
        return np.ascontiguousarray(im)
    h, w = im.shape
    s = level_scale(l)
    wl, hl = level_dims(w, h, l)
    T = np.array([[1 / s, 0], [0, 1 / s], [0.5 / s - 0.5, 0.5 / s - 0.5]]).astype(np.float32)
    return KO.remap_affine(im, T, (0, wl, 0, hl))


def level_mask(wl, hl, l, box=None):
    m = np.zeros((hl, wl), np.uint8)
    x0, x1, y0, y1 = BORDER, wl - BORDER, BORDER, hl - BORDER
    if box is not None:
        sf = np.float32(level_scale(l))
        bx0, bx1, by0, by1 = (int(np.float32(v) * sf) for v in box)
        x0, x1, y0, y1 = max(x0, bx0), min(x1, bx1), max(y0, by0), min(y1, by1)
    if x1 > x0 and y1 > y0:
        m[y0:y1, x0:x1] = 1
    return m


def box5(img):
    a = np.pad(np.asarray(img, np.int32), 2)
    h, w = img.shape
    s = np.zeros((h, w), np.int32)
    for j in range(5):
        for i in range(5):
            s += a[j:j + h, i:i + w]
    return s


def describe(img, xy, pairs=None):
    """uint8 [n, 32] descriptors of the integer keypoints xy (x, y) of one level image."""
    pairs = pair_table() if pairs is None else pairs
    if len(xy) == 0:
        return np.zeros((0, 32), np.uint8)
    sm = box5(img)
    x, y = xy[:, 0].astype(np.int64)[:, None], xy[:, 1].astype(np.int64)[:, None]
    bits = sm[y + pairs[None, :, 1], x + pairs[None, :, 0]] < sm[y + pairs[None, :, 3], x + pairs[None, :, 2]]
    return np.packbits(bits, axis=1)


def features(im, per_level, P, box=None):
    """-> dict(kp: per-level float32 [n_l, 2] keypoints in level coordinates, pos float32 [n, 2] level-0 positions, desc uint8 [n, 32])."""
    h, w = im.shape
    kps, pos, desc = [], [], []
    for l in range(P["levels"]):
        g = level_image(im, l)
        hl, wl = g.shape
        if wl < 3 or hl < 3:
            xy = np.zeros((0, 2), np.float32)
        else:
            xy = G.good_features(g, per_level, P["quality"], 0.0, mask=level_mask(wl, hl, l, box), block=P["block"], use_harris=False)
        inv = np.float32(1.0 / level_scale(l))
        kps.append(xy)
        pos.append((xy + np.float32(0.5)) * inv - np.float32(0.5))
        desc.append(describe(g, xy))
    return dict(kp=kps, pos=np.concatenate(pos).astype(np.float32).reshape(-1, 2), desc=np.concatenate(desc).reshape(-1, 32))


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def match2nn(dq, dt):
    """-> int32 [nq, 4] = (nearest index, its distance, second index, its distance), -1 where there is none."""
    nq, nt = len(dq), len(dt)
    nn = np.full((nq, 4), -1, np.int32)
    if nq == 0 or nt == 0:
        return nn
    for a in range(0, nq, 256):
        d = _POP[dq[a:a + 256, None, :] ^ dt[None, :, :]].sum(-1)
        o = np.argsort(d, axis=1, kind="stable")[:, :2]
        r = np.arange(len(o))
        nn[a:a + 256, 0], nn[a:a + 256, 1] = o[:, 0], d[r, o[:, 0]]
        if nt > 1:
            nn[a:a + 256, 2], nn[a:a + 256, 3] = o[:, 1], d[r, o[:, 1]]
    return nn


def match_affine(im1, im2, p1, **params):
    """-> dict(M float64 [2,3] or None, status, inl uint8 [good], info int32 [4] = (status, good, inliers, query keypoints), pairs float32 [good, 4],
    good bool [nq], nn, q, t (features of the query / train image), box)."""
    P = dict(DEFAULTS, **params)
    im1, im2 = np.ascontiguousarray(im1), np.ascontiguousarray(im2)
    p1 = np.asarray(p1, np.float32).reshape(-1, 2)
    box = KO.bounding_rect(p1, im1.shape, (P["border_x"], P["border_y"]))
    q = features(im1, P["query_per_level"], P, box)
    t = features(im2, P["train_per_level"], P)
    nn = match2nn(q["desc"], t["desc"])
    good = (nn[:, 2] >= 0) & (P["ratio_den"] * nn[:, 1] < P["ratio_num"] * nn[:, 3])
    src, dst = q["pos"][good], t["pos"][nn[good, 0]] if len(t["pos"]) else np.zeros((0, 2), np.float32)
    pairs = np.concatenate([src, dst], 1).astype(np.float32).reshape(-1, 4)
    ng = int(good.sum())
    M, inl = None, np.zeros(ng, np.uint8)
    if ng >= max(P["min_good"], 3):
        M, inl_b, _ = KO.ransac_affine(src, dst)
        inl = inl_b.astype(np.uint8)
        if M is None:
            inl[:] = 0
    status = int(M is not None)
    info = np.array([status, ng, int(inl.sum()), len(q["pos"])], np.int32)
    return dict(M=M, status=status, inl=inl, info=info, pairs=pairs, good=good, nn=nn, q=q, t=t, box=box)


def estimate_affine_surf(im1, im2, p1, scale=1.0, **params):
    """The shim's estimateAffine2D_SURF on the model: scale != 1 resizes both images (nearest), scales p1 and divides the pairs by scale before RANSAC."""
    if scale == 1.0:
        r = match_affine(im1, im2, p1, **params)
        return r["M"], r["inl"].reshape(-1, 1)
    P = dict(DEFAULTS, **params)
    r = match_affine(KO.resize_nearest(im1, scale), KO.resize_nearest(im2, scale), np.asarray(p1, np.float32) * np.float32(scale), **params)
    pairs = r["pairs"] / np.float32(scale)
    if len(pairs) < max(P["min_good"], 3):
        return None, np.zeros((len(pairs), 1), np.uint8)
    M, inl, _ = KO.ransac_affine(pairs[:, :2], pairs[:, 2:])
    inl = inl.astype(np.uint8) if M is not None else np.zeros(len(pairs), np.uint8)
    return M, inl.reshape(-1, 1)


def recover(im0, im, p0, **params):
    """The recovery branch of KLTmain (utils/KLT.py:130-133) on the checker: -> (p_all, v, M) or None when no model is found."""
    r = match_affine(im0, im, p0, **params)
    if r["M"] is None:
        return None
    p, v, _, _ = KO.klt_regional(im0, im, p0, r["M"].T, KO.LK_FINE, fbt=0.3)
    return p, v, r["M"]
